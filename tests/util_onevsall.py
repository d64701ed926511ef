"""Case table, seeded problems, float64 expectations and tolerances of the 1vsAll tests (tests/test_host_onevsall.py,
tests/test_gpu_onevsall.py).  Host code only: nothing here touches the device.

The step is three matrix-core products (mkb_amd/csrc/all_plan.h: the forward S = Q . E^T, dQ = dS . E and dE += dS^T . Q) around
one softmax kernel.  ``CASES`` holds the smallest shapes at which each product takes each kernel family, the forward's lane
fallback, every N % 4, and a row longer than the softmax kernel's LDS staging (4096 columns).  ``families`` names what each case
claims; test_host_onevsall.py asks the planner itself (a host program built on gemm_plan.h) whether the claim holds.

Expectations: the same formulas in float64 by torch on the CPU -- q from the two fixed operands (oracle.scoring's expressions with
the candidate factored out), S = q E^T, logsumexp, autograd for dS and both table gradients.  ``err_ref`` of a quantity is the
largest difference between that computation in float32 and in float64 at the case's own tables, but never below one unit in the
last place of float32 at the quantity's largest magnitude (2^-24 max|x|: a reference that happens to round luckily must not turn
the bound into zero).  The device is held to 8 x err_ref, as in tests/util_rank_routes.py; MEASURED_RATIO lists the cases and
quantities whose honest ratio was measured above 8 on the MI355X (profiles/r23_onevsall_errors.txt), held to twice that ratio and
never to more than a quarter of one typical term of the sum behind the quantity.
"""
from __future__ import annotations

import functools
import zlib

import numpy as np
import torch

MODES = ("head-batch", "tail-batch")
R = 3  # relations: every batch repeats them
STAGE_COLS = 4096  # kAllStageCols of score_all.hip

# (name, model, hidden, B, N, families of (forward, dQ, dE)).  "lane": the forward's lane-owns-dims kernel.
CASES = [
    # lane fallback and ragged batch: B % 4 != 0, entity_dim % 4 != 0 (37; ComplEx 74)
    ("ragged-distmult", "DistMult", 37, 37, 129, ("lane", "f32tile64", "f32tile64")),
    ("ragged-complex", "ComplEx", 37, 37, 129, ("lane", "f32tile64", "f32tile64")),
    # the 64-row fp32 tiles with N % 4 = 1, 2, 3 at entity_dim 16 and 64
    ("t64-n129-d16", "DistMult", 16, 32, 129, ("f32tile64", "f32tile64", "f32tile64")),
    ("t64-n129-d64", "ComplEx", 32, 32, 129, ("f32tile64", "f32tile64", "f32tile64")),
    ("t64-n130-d16", "ComplEx", 8, 32, 130, ("f32tile64", "f32tile64", "f32tile64")),
    ("t64-n130-d64", "DistMult", 64, 32, 130, ("f32tile64", "f32tile64", "f32tile64")),
    ("t64-n131-d16", "DistMult", 16, 32, 131, ("f32tile64", "f32tile64", "f32tile64")),
    ("t64-n131-d64", "ComplEx", 32, 32, 131, ("f32tile64", "f32tile64", "f32tile64")),
    # all three products on the 128-row bf16x3 tiles (dE: M = N = 1537, K split in two, reduced and added once)
    ("bf16x3-distmult", "DistMult", 768, 512, 1537, ("bf16x3", "bf16x3", "bf16x3")),
    ("bf16x3-complex", "ComplEx", 384, 512, 1537, ("bf16x3", "bf16x3", "bf16x3")),
    # a row longer than the softmax kernel's LDS staging
    ("long-distmult", "DistMult", 16, 8, 5000, ("lane", "f32tile64", "bf16x3")),
    ("long-complex", "ComplEx", 8, 8, 5000, ("lane", "f32tile64", "bf16x3")),
]
CASE_IDS = [c[0] for c in CASES]
QUANTITIES = ("loss", "pos", "dS", "g_ent", "g_rel")


def entity_dim(model, hidden):
    return 2 * hidden if model == "ComplEx" else hidden


class Problem:
    """Seeded tables (uniform in [-1, 1], the distribution of tests/util_rank_routes.py for the two models), a batch with repeated
    heads, tails and relations, a row whose target is entity N - 1 (the one the forward's padding repeats) and one whose target is
    entity 0 on each side, and per-row weights in [0.5, 1.5]."""

    def __init__(self, case):
        name, model, hidden, B, N, _ = case
        self.case, self.model, self.hidden, self.B, self.N = case, model, hidden, B, N
        rs = np.random.RandomState(zlib.crc32(("onevsall-" + name).encode()) & 0x7FFFFFFF)
        de = entity_dim(model, hidden)
        self.ent = rs.uniform(-1, 1, size=(N, de)).astype(np.float32)
        self.rel = rs.uniform(-1, 1, size=(R, de)).astype(np.float32)
        s = np.stack([rs.randint(N, size=B), rs.randint(R, size=B), rs.randint(N, size=B)], 1).astype(np.int64)
        s[0, 2], s[1, 2] = N - 1, 0            # tail-batch targets
        s[2, 0], s[3, 0] = N - 1, 0            # head-batch targets
        s[5, 0], s[5, 2], s[5, 1] = s[4, 0], s[4, 2], s[4, 1]  # a repeated head, tail and relation
        s[7, 0], s[7, 2] = s[6, 0], s[6, 2]
        self.sample = s
        self.weight = rs.uniform(0.5, 1.5, size=B).astype(np.float32)

    def target(self, mode):
        return self.sample[:, 0 if mode == "head-batch" else 2]


@functools.lru_cache(maxsize=None)
def problem(case) -> Problem:
    return Problem(case)


def query(model, ent, rel, sample, mode):
    """q [B, De] with score(candidate x) = <q, x>: oracle.scoring.score's ComplEx / DistMult expressions, candidate factored out."""
    head = mode == "head-batch"
    e, r = ent[sample[:, 2 if head else 0]], rel[sample[:, 1]]
    if model == "DistMult":
        return e * r
    re_e, im_e = torch.chunk(e, 2, dim=1)
    re_r, im_r = torch.chunk(r, 2, dim=1)
    if head:  # the candidate is the head: coefficients of (re_h, im_h)
        return torch.cat([re_r * re_e + im_r * im_e, re_r * im_e - im_r * re_e], 1)
    return torch.cat([re_e * re_r - im_e * im_r, re_e * im_r + im_e * re_r], 1)


def n3(model, ent, rel, sample, weight, W, lam):
    """regularizers.N3(lam) on the batch's positive triples (include/mkb_hip.h, "embedding regularisers")."""
    def f(x):
        if model == "ComplEx":
            re, im = torch.chunk(x, 2, dim=1)
            return ((re * re + im * im) ** 1.5).sum(1)
        return (x.abs() ** 3).sum(1)
    rows = f(ent[sample[:, 0]]) + f(ent[sample[:, 2]]) + f(rel[sample[:, 1]])
    return lam * (weight * rows).sum() / W


def compute(model, ent, rel, sample, mode, weight, weight_sum=None, T=1.0, pad=0, reg=0.0):
    """The step in the dtype of ``ent``: -> dict of numpy arrays (QUANTITIES and "S").  ``pad`` > 0 repeats the last entity's
    column that many times INSIDE the softmax: what a kernel that lets the forward's pad columns in would compute."""
    ent = ent.clone().requires_grad_(True)
    rel = rel.clone().requires_grad_(True)
    sample = torch.as_tensor(sample)
    target = sample[:, 0 if mode == "head-batch" else 2]
    w = torch.ones(len(sample), dtype=ent.dtype) if weight is None else torch.as_tensor(weight).to(ent.dtype)
    W = w.sum() if weight_sum is None else torch.as_tensor(weight_sum, dtype=ent.dtype)
    S = query(model, ent, rel, sample, mode) @ ent.t()
    S.retain_grad()
    Z = S if pad == 0 else torch.cat([S] + [S[:, -1:]] * pad, 1)
    pos = S[torch.arange(len(sample)), target]
    loss = (w * (torch.logsumexp(Z / T, 1) - pos / T)).sum() / W
    total = loss + (n3(model, ent, rel, sample, w, W, reg) if reg else 0.0)
    total.backward()
    return {"loss": loss.detach().numpy(), "pos": pos.detach().numpy(), "dS": S.grad.numpy(), "g_ent": ent.grad.numpy(),
            "g_rel": rel.grad.numpy(), "S": S.detach().numpy(), "total": total.detach().numpy()}


@functools.lru_cache(maxsize=None)
def expected(case, mode, weighted=True, reg=0.0):
    """-> (float64 result, err_ref per quantity)."""
    pb = problem(case)
    w = pb.weight if weighted else None
    out = []
    for dtype in (torch.float64, torch.float32):
        out.append(compute(pb.model, torch.from_numpy(pb.ent).to(dtype), torch.from_numpy(pb.rel).to(dtype), pb.sample, mode, w, reg=reg))
    f64, f32 = out
    err = {}
    for k in QUANTITIES:
        ulp = 2.0 ** -24 * float(np.abs(f64[k]).max())
        err[k] = max(float(np.abs(f32[k].astype(np.float64) - f64[k]).max()), ulp)
    return f64, err


def typical_term(case, mode, quantity):
    """One typical term of the sum behind a quantity: a dropped or doubled dimension, column or batch row moves the quantity by
    about this much.  loss: one row's share; pos: rms(score) / sqrt(De); dS: the rms seed (each IS one term); g_ent: rms over
    the rows of |dS| |q| (one batch row's share of an entity row); g_rel: the same for |dQ| |e| with dQ one column's share."""
    pb = problem(case)
    f64, _ = expected(case, mode)
    de = entity_dim(pb.model, pb.hidden)
    rms = lambda a: float(np.sqrt((np.asarray(a, dtype=np.float64) ** 2).mean()))
    if quantity == "loss":
        return float(f64["loss"]) / pb.B
    if quantity == "pos":
        return rms(f64["S"]) / np.sqrt(de)
    if quantity == "dS":
        return rms(f64["dS"])
    # one (row, column) pair's contribution to a gradient element: seed x operand, operands uniform in [-1, 1] (rms 0.58) or products of two
    return rms(f64["dS"]) * 0.33


ERR_FACTOR = 8.0
# (case name, quantity) -> the largest device error / err_ref over both sides, measured on the MI355X, where it exceeds 8 with no
# defect behind it (profiles/r23_onevsall_errors.txt has every case, side and quantity).
MEASURED_RATIO: dict = {}


def tolerance(case, mode, quantity, steps=1) -> float:
    _, err = expected(case, mode)
    factor = max(ERR_FACTOR, 2.0 * MEASURED_RATIO.get((case[0], quantity), 0.0))
    return steps * min(factor * err[quantity], max(ERR_FACTOR * err[quantity], 0.25 * typical_term(case, mode, quantity)))


def pad_trap(case, mode):
    """|loss with the pad columns inside the softmax - loss| and the same for the gradient row of entity N - 1, in float64."""
    pb = problem(case)
    pad = (-pb.N) % 4
    good, _ = expected(case, mode)
    bad = compute(pb.model, torch.from_numpy(pb.ent).double(), torch.from_numpy(pb.rel).double(), pb.sample, mode, pb.weight, pad=pad)
    return abs(float(bad["loss"]) - float(good["loss"])), float(np.abs(bad["g_ent"][-1] - good["g_ent"][-1]).max())
