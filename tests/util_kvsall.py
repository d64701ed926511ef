"""Label sets, float64 expectations and tolerances of the KvsAll tests (tests/test_host_kvsall.py, tests/test_gpu_kvsall.py).
Host code only: nothing here touches the device.

The step is the 1vsAll step's three products (tests/util_onevsall.py: its case table, seeded tables and weights are reused) around
one other loss kernel, all_bce_kernel of mkb_amd/csrc/score_all.hip:

    y_ij  = (1 - eps) [j in A_i] + eps / N
    row_i = c sum_{j < N} (softplus(s_ij) - y_ij s_ij)        c = 1 / N ("mean") or 1 ("sum")
    loss  = sum_i w_i row_i / W          dS_ij = (w_i c / W) (sigmoid(s_ij) - y_ij)

What is new is the label set A_i, which the kernel reads as the range [q N, (q + 1) N) of a sorted key array, q = e R + r the row's
query.  ``labels(case, mode)`` builds one batch per case and side whose first eight rows are designed (``KINDS``): a query absent
from the keys, one label that is not the row's target, three label counts around the kernel's 256-lane loop (255 / 256 / 257; 63 /
64 / 65 where N is too small), a query whose neighbours q - 1 and q + 1 own the keys right next to its range, every entity
labelled -- twice, two rows with one query -- by the query that owns the last key of the array.  The rest of the batch draws
queries with 1 .. 6 labels from the case's seed.  ``label_kinds`` finds the kinds again from (sample, keys) alone; the host test
asserts that every case has all of them.

Expectations: the formulas above in float64 by torch on the CPU, S = q E^T with util_onevsall.query, a dense multi-hot matrix from
the keys, autograd for dS and both table gradients.  err_ref and the tolerance follow util_onevsall: the float32 evaluation's own
error, at least one float32 ulp of the quantity's largest magnitude; the device is held to 8 x err_ref.  MEASURED_RATIO is for
ratios measured above 8 on the MI355X with no defect behind them (profiles/r24_kvsall_errors.txt).
"""
from __future__ import annotations

import functools
import zlib

import numpy as np
import torch

import util_onevsall as U

R = U.R
KINDS = ("none", "one", "k0", "k1", "k2", "edge", "all", "same")  # the designed rows, in batch order
SETTINGS = ((0.0, "mean"), (0.1, "mean"), (0.0, "sum"), (0.1, "sum"))  # (label smoothing, reduction)


def lane_counts(N):
    """The three label counts around the 256-lane loop edge, or around one wave where the row is too short for them."""
    return (255, 256, 257) if N >= 300 else (63, 64, 65)


class Labels:
    """sample [B, 3]; keys: ascending int64 keys of ``mode``'s ordering; triples: the (h, r, t) they stand for; rows: KINDS -> row."""

    def __init__(self, case, mode):
        name, _, _, B, N, _ = case
        assert B >= len(KINDS) and N >= 100
        head = mode == "head-batch"
        rs = np.random.RandomState(zlib.crc32(f"kvsall-{name}-{mode}".encode()) & 0x7FFFFFFF)
        k0, k1, k2 = lane_counts(N)

        def subset(k, forced=()):
            rest = np.setdiff1d(np.arange(1, N - 1), np.asarray(forced, dtype=np.int64))
            return np.sort(np.concatenate([np.asarray(forced, dtype=np.int64), rs.choice(rest, k - len(forced), replace=False)]))

        sets = {}  # query -> label columns
        rows = []  # (query entity, relation, target)
        design = {
            "none": (0, 0, None, N // 2),
            "one": (0, 1, np.array([N // 3]), N // 3 + 1),       # owns the first key; its target is not a label
            "k0": (2, 0, subset(k0, (0, N - 1)), 0),
            "k1": (2, 1, subset(k1), None),
            "k2": (2, 2, subset(k2, (N - 1,)), N - 1),
            "edge": (4, 1, np.array([1, N - 2]), 1),
            "all": (N - 1, R - 1, np.arange(N), N - 1),           # owns the last key
            "same": (N - 1, R - 1, np.arange(N), 0),
        }
        for kind in KINDS:
            e, r, cols, target = design[kind]
            if cols is not None:
                sets[e * R + r] = cols
                if target is None:
                    target = int(cols[len(cols) // 2])
            rows.append((e, r, target))
        sets[4 * R + 0] = np.array([3, N - 1])  # q - 1 of "edge": its last key is the one right below the range of q
        sets[4 * R + 2] = np.array([0, 5])      # q + 1: its first key is the one right above
        for _ in range(B - len(KINDS)):
            e, r = int(rs.randint(6, N - 1)), int(rs.randint(R))
            cols = sets.setdefault(e * R + r, np.sort(rs.choice(N, rs.randint(1, 7), replace=False)))
            rows.append((e, r, int(cols[rs.randint(len(cols))]) if rs.randint(2) else int(rs.randint(N))))
        self.rows = {kind: i for i, kind in enumerate(KINDS)}
        e, r, target = (np.array(x, dtype=np.int64) for x in zip(*rows))
        self.sample = np.stack([target, r, e] if head else [e, r, target], 1)
        self.keys = np.sort(np.concatenate([q * N + cols.astype(np.int64) for q, cols in sets.items()]))
        qs, cols = self.keys // N, self.keys % N
        self.triples = [(int(c), int(q % R), int(q // R)) if head else (int(q // R), int(q % R), int(c)) for q, c in zip(qs, cols)]


@functools.lru_cache(maxsize=None)
def labels(case, mode) -> Labels:
    return Labels(case, mode)


def queries(sample, mode):
    sample = np.asarray(sample)
    return sample[:, 2 if mode == "head-batch" else 0] * R + sample[:, 1]


def label_ranges(sample, mode, keys, N):
    q = queries(sample, mode)
    return np.searchsorted(keys, q * N), np.searchsorted(keys, (q + 1) * N)


def multi_hot(sample, mode, keys, N):
    """Y [B, N] float64 of 0 / 1 from the key list."""
    lo, hi = label_ranges(sample, mode, keys, N)
    q = queries(sample, mode)
    Y = np.zeros((len(q), N))
    for i, (a, b) in enumerate(zip(lo, hi)):
        Y[i, keys[a:b] - q[i] * N] = 1.0
    return Y


def label_kinds(sample, mode, keys, N):
    """The kinds of label set found in a batch, from (sample, keys) alone -> set of names."""
    sample = np.asarray(sample)
    Y = multi_hot(sample, mode, keys, N)
    q = queries(sample, mode)
    lo, hi = label_ranges(sample, mode, keys, N)
    target = sample[:, 0 if mode == "head-batch" else 2]
    n = Y.sum(1).astype(int)
    found = {f"count-{k}" for k in set(n.tolist())}
    if (n == N).any():
        found.add("every-entity")
    if Y[:, 0].any():
        found.add("column-0")
    if Y[:, N - 1].any():
        found.add("column-last")
    if len(set(q.tolist())) < len(q):
        found.add("shared-query")
    present = set(keys.tolist())
    for i in range(len(q)):
        if n[i] and q[i] * N - 1 in present and (q[i] + 1) * N in present and not Y[i, 0] and not Y[i, N - 1]:
            found.add("adjacent-neighbours")  # a bound off by one would let column 0 or N - 1 in
        if n[i] and Y[i, target[i]] == 0:
            found.add("target-not-a-label")
        if n[i] and lo[i] == 0:
            found.add("owns-first-key")
        if n[i] and hi[i] == len(keys):
            found.add("owns-last-key")
        if n[i] == 0 and lo[i] == 0:
            found.add("absent-below-every-key")
    return found


def required_kinds(N):
    return {"count-0", "count-1", "every-entity", "column-0", "column-last", "shared-query", "adjacent-neighbours",
            "target-not-a-label", "owns-first-key", "owns-last-key"} | {f"count-{k}" for k in lane_counts(N)}


def softplus(x):
    return torch.clamp(x, min=0) + torch.log1p(torch.exp(-x.abs()))


def compute(model, ent, rel, sample, mode, keys, weight, weight_sum=None, eps=0.0, reduction="mean", pad=0, reg=0.0, S=None):
    """The step in the dtype of ``ent`` -> dict of numpy arrays (U.QUANTITIES, "S", "total").  ``S``: a given score block instead of
    q E^T (then in ITS dtype, and no table gradients).  ``pad`` > 0: the last column enters the row sums that many more times with
    the label eps / N -- what a kernel that lets the forward's pad columns in would compute."""
    sample = torch.as_tensor(np.asarray(sample))
    target = sample[:, 0 if mode == "head-batch" else 2]
    if S is None:
        ent = ent.clone().requires_grad_(True)
        rel = rel.clone().requires_grad_(True)
        S = U.query(model, ent, rel, sample, mode) @ ent.t()
        S.retain_grad()
    else:
        ent = rel = None
        S = S.clone().requires_grad_(True)
    dtype, N = S.dtype, S.shape[1]
    w = torch.ones(len(sample), dtype=dtype) if weight is None else torch.as_tensor(weight).to(dtype)
    W = w.sum() if weight_sum is None else torch.as_tensor(weight_sum, dtype=dtype)
    y = (1.0 - eps) * torch.from_numpy(multi_hot(sample.numpy(), mode, keys, N)).to(dtype) + eps / N
    c = 1.0 / N if reduction == "mean" else 1.0
    rows = (softplus(S) - y * S).sum(1)
    if pad:
        rows = rows + pad * (softplus(S[:, -1]) - (eps / N) * S[:, -1])
    pos = S[torch.arange(len(sample)), target]
    loss = (w * c * rows).sum() / W
    total = loss + (U.n3(model, ent, rel, sample, w, W, reg) if reg else 0.0)
    total.backward()
    out = {"loss": loss.detach().numpy(), "pos": pos.detach().numpy(), "dS": S.grad.numpy(), "S": S.detach().numpy(),
           "total": total.detach().numpy()}
    if ent is not None:
        out.update(g_ent=ent.grad.numpy(), g_rel=rel.grad.numpy())
    return out


def err_ref(f64, f32):
    err = {}
    for k in U.QUANTITIES:
        if k in f64:
            ulp = 2.0 ** -24 * float(np.abs(f64[k]).max())
            err[k] = max(float(np.abs(f32[k].astype(np.float64) - f64[k]).max()), ulp)
    return err


@functools.lru_cache(maxsize=None)
def expected(case, mode, eps=0.0, reduction="mean", weighted=True, reg=0.0):
    """-> (float64 result, err_ref per quantity) of the case's tables on the batch and keys of ``labels(case, mode)``."""
    pb, L = U.problem(case), labels(case, mode)
    w = pb.weight if weighted else None
    f64, f32 = (compute(pb.model, torch.from_numpy(pb.ent).to(dt), torch.from_numpy(pb.rel).to(dt), L.sample, mode, L.keys, w, eps=eps,
                        reduction=reduction, reg=reg) for dt in (torch.float64, torch.float32))
    return f64, err_ref(f64, f32)


def block_expected(S32, sample, mode, keys, weight, weight_sum, eps, reduction):
    """The loss kernel alone on a given float32 block: the float64 formulas on those very values -> (float64 result, err_ref)."""
    S32 = torch.as_tensor(S32)
    f64, f32 = (compute(None, None, None, sample, mode, keys, weight, weight_sum, eps, reduction, S=S32.to(dt))
                for dt in (torch.float64, torch.float32))
    return f64, err_ref(f64, f32)


def typical_term(f64, B, de, quantity):
    """One typical term of the sum behind a quantity, as util_onevsall.typical_term."""
    rms = lambda a: float(np.sqrt((np.asarray(a, dtype=np.float64) ** 2).mean()))
    if quantity == "loss":
        return abs(float(f64["loss"])) / B
    if quantity == "pos":
        return rms(f64["S"]) / np.sqrt(de)
    if quantity == "dS":
        return rms(f64["dS"])
    return rms(f64["dS"]) * 0.33


ERR_FACTOR = U.ERR_FACTOR
# (case name, quantity) -> the largest device error / err_ref over both sides and every setting, measured on the MI355X, where it
# exceeds 8 with no defect behind it (profiles/r24_kvsall_errors.txt has every case, side and quantity).
MEASURED_RATIO: dict = {}


def bound(name, quantity, err, term, steps=1) -> float:
    """8 x err_ref; a measured ratio widens it to twice that ratio, never past a quarter of one typical term."""
    factor = max(ERR_FACTOR, 2.0 * MEASURED_RATIO.get((name, quantity), 0.0))
    return steps * min(factor * err, max(ERR_FACTOR * err, 0.25 * term))


def tolerance(case, mode, quantity, eps=0.0, reduction="mean", weighted=True, reg=0.0) -> float:
    f64, err = expected(case, mode, eps, reduction, weighted, reg)
    pb = U.problem(case)
    return bound(case[0], quantity, err[quantity], typical_term(f64, pb.B, U.entity_dim(pb.model, pb.hidden), quantity))


def pad_trap(case, mode, eps=0.0, reduction="mean"):
    """|loss with the forward's pad columns inside the row sums - loss| in float64."""
    pb, L = U.problem(case), labels(case, mode)
    good, _ = expected(case, mode, eps, reduction)
    bad = compute(pb.model, torch.from_numpy(pb.ent).double(), torch.from_numpy(pb.rel).double(), L.sample, mode, L.keys, pb.weight, eps=eps,
                  reduction=reduction, pad=(-pb.N) % 4)
    return abs(float(bad["loss"]) - float(good["loss"]))


def own_target_labels(case, mode):
    """A batch of distinct queries in which every row's single label is its own target -> (sample, keys, triples)."""
    pb = U.problem(case)
    head = mode == "head-batch"
    s = pb.sample.copy()
    s[:, 2 if head else 0] = np.arange(pb.B)  # (B <= N in every case)
    keys = np.sort(queries(s, mode) * pb.N + s[:, 0 if head else 2])
    return s, keys, [tuple(int(v) for v in row) for row in s]
