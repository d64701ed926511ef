"""Designed batches, float64 expectations and tolerances of the filtered 1vsAll tests (tests/test_host_onevsall_filtered.py,
tests/test_gpu_onevsall_filtered.py).  Host code only: nothing here touches the device.

The step is the 1vsAll step's three products (tests/util_onevsall.py: its case table, seeded tables, weights and ``query`` are
reused) around a third loss kernel, all_softmax_filtered_kernel of mkb_amd/csrc/score_all.hip.  With A_i the keys of row i's query
in the mode's sorted key array (the range [q N, (q + 1) N): tests/util_kvsall.py's ``queries`` / ``label_ranges`` / ``multi_hot``
are reused) and t_i the row's target:

    F_i = A_i \\ {t_i} (filtered)     C_i = [0, N) \\ F_i (kept)     n_i = |C_i|
    y_ij  = (1 - eps) [j = t_i] + eps / n_i
    row_i = log sum_{C_i} exp(s_ij / T) - (1 - eps) s_it / T - (eps / n_i) sum_{C_i} s_ij / T
    loss  = sum_i w_i row_i / W          dS_ij = (w_i / (W T)) (p_ij - y_ij) on C_i, exactly 0 on F_i

``rows(name, B, N, mode)`` builds one batch whose first eight rows are designed (``KINDS``): the only key is the target (the query
that owns the first key of the array), no key at all, one filtered column with a target that is no key, filtered counts around the
kernel's 256-lane loop (255 / 256 / 257; 63 / 64 / 65 where N is too small) -- the first of them with columns 0 and N - 1 filtered,
the second with a target that IS a key --, and twice the query that owns the last key of the array and every entity: targets N - 1
and 0, so each of the two rows filters the other's target and keeps n_i = 1 column.  The rest of the batch draws queries with
1 .. 6 keys from the seed.  ``kinds`` finds all of that again from (sample, keys, target) alone; the host test asserts it.

Expectations: the formulas above in float64 by torch on the CPU, S = q E^T with util_onevsall.query or a given block, autograd for
dS and both table gradients.  err_ref is the float32 evaluation's own error, at least one float32 ulp of the quantity's largest
magnitude (2^-24 max|x|); the device is held to 8 x err_ref.  MEASURED_RATIO is for ratios measured above 8 on the MI355X with no
defect behind them (profiles/r25_onevsall_filtered_errors.txt has every ratio), held to twice the ratio and never to more than a
quarter of one typical term of the sum behind the quantity.
"""
from __future__ import annotations

import functools
import zlib

import numpy as np
import torch

import util_kvsall as K
import util_onevsall as U

R = U.R
KINDS = ("only", "none", "one", "k0", "k1", "k2", "all", "same")  # the designed rows, in batch order
SETTINGS = ((0.0, 1.0), (0.1, 1.0), (0.1, 0.5))  # (label smoothing, temperature)
STEP_CASES = ("ragged-complex", "t64-n130-d64", "bf16x3-distmult", "long-complex")
lane_counts = K.lane_counts


class Rows:
    """sample [B, 3]; keys: ascending int64 keys of ``mode``'s ordering; triples: the (h, r, t) they stand for; rows: KINDS -> row."""

    def __init__(self, name, B, N, mode):
        assert B >= len(KINDS) and N >= 100
        head = mode == "head-batch"
        rs = np.random.RandomState(zlib.crc32(f"onevsall-filtered-{name}-{mode}".encode()) & 0x7FFFFFFF)
        k0, k1, k2 = lane_counts(N)

        def subset(k, forced=(), avoid=()):
            forced = np.asarray(forced, dtype=np.int64)
            rest = np.setdiff1d(np.arange(1, N - 1), np.concatenate([forced, np.asarray(avoid, dtype=np.int64)]))
            return np.sort(np.concatenate([forced, rs.choice(rest, k - len(forced), replace=False)]))

        t1 = N // 2 + 3
        design = {  # kind -> (query entity, relation, key columns, target)
            "only": (0, 0, np.array([N // 3]), N // 3),                  # owns the first key
            "none": (0, 1, None, N // 2),
            "one": (0, 2, np.array([5]), 7),
            "k0": (2, 0, subset(k0, (0, N - 1), avoid=(N // 2,)), N // 2),  # the target is no key: all k0 are filtered
            "k1": (2, 1, subset(k1 + 1, (t1,)), t1),                     # the target is a key: k1 are filtered
            "k2": (2, 2, subset(k2, avoid=(N // 2,)), N // 2),
            "all": (N - 1, R - 1, np.arange(N), N - 1),                  # owns the last key
            "same": (N - 1, R - 1, np.arange(N), 0),
        }
        sets, rows = {}, []
        for kind in KINDS:
            e, r, cols, target = design[kind]
            if cols is not None:
                sets[e * R + r] = cols
            rows.append((e, r, target))
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
def rows(name, B, N, mode) -> Rows:
    return Rows(name, B, N, mode)


def case_rows(case, mode) -> Rows:
    return rows(case[0], case[3], case[4], mode)


def open_slot(sample, mode):
    return np.asarray(sample)[:, 0 if mode == "head-batch" else 2]


def filtered_mask(sample, mode, keys, N, target=None):
    """F [B, N] bool: the row's keys without its target."""
    target = open_slot(sample, mode) if target is None else np.asarray(target)
    F = K.multi_hot(np.asarray(sample), mode, keys, N) > 0
    F[np.arange(len(target)), target] = False
    return F


def kinds(sample, mode, keys, N, target=None):
    """The kinds of row found in a batch, from (sample, keys, target) alone -> set of names."""
    sample = np.asarray(sample)
    target = open_slot(sample, mode) if target is None else np.asarray(target)
    A = K.multi_hot(sample, mode, keys, N) > 0
    F = filtered_mask(sample, mode, keys, N, target)
    q = K.queries(sample, mode)
    lo, hi = K.label_ranges(sample, mode, keys, N)
    nA, nF = A.sum(1), F.sum(1)
    is_key = A[np.arange(len(q)), target]
    found = {f"filtered-{k}" for k in set(nF.tolist())}
    for i in range(len(q)):
        if nA[i] == 0:
            found.add("no-keys")
        if nA[i] == 1 and is_key[i]:
            found.add("target-is-the-only-key")
        if nA[i] and not is_key[i]:
            found.add("target-not-a-key")
        if F[i, 0]:
            found.add("column-0-filtered")
        if F[i, N - 1]:
            found.add("column-last-filtered")
        if nF[i] == N - 1:
            found.add("all-but-the-target")
        if nA[i] and lo[i] == 0:
            found.add("owns-first-key")
        if nA[i] and hi[i] == len(keys):
            found.add("owns-last-key")
        for k in range(i):
            if q[k] == q[i] and target[k] != target[i] and F[i, target[k]] and F[k, target[i]]:
                found.add("shared-query-filters-each-others-target")
    return found


def required_kinds(N):
    return {"no-keys", "target-is-the-only-key", "target-not-a-key", "filtered-1", "column-0-filtered", "column-last-filtered",
            "all-but-the-target", "owns-first-key", "owns-last-key", "shared-query-filters-each-others-target"} | {
                f"filtered-{k}" for k in lane_counts(N)}


def compute(model, ent, rel, sample, mode, keys, weight, weight_sum=None, eps=0.0, T=1.0, reg=0.0, S=None, target=None):
    """The step in the dtype of ``ent`` -> dict of numpy arrays (U.QUANTITIES, "S", "rows", "n", "total").  ``S``: a given score
    block instead of q E^T (then in ITS dtype, and no table gradients).  ``target``: the open slot of ``sample`` when None."""
    sample_np = np.asarray(sample)
    sample = torch.as_tensor(sample_np)
    target_np = open_slot(sample_np, mode) if target is None else np.asarray(target)
    target = torch.as_tensor(target_np)
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
    kept = torch.from_numpy(~filtered_mask(sample_np, mode, keys, N, target_np))
    n = kept.sum(1)
    Z = S / T
    lse = torch.logsumexp(torch.where(kept, Z, torch.full_like(Z, -float("inf"))), 1)
    lin = torch.where(kept, Z, torch.zeros_like(Z)).sum(1)
    pos = S[torch.arange(len(sample)), target]
    rows_ = lse - (1.0 - eps) * pos / T - (eps / n.to(dtype)) * lin
    loss = (w * rows_).sum() / W
    total = loss + (U.n3(model, ent, rel, sample, w, W, reg) if reg else 0.0)
    total.backward()
    out = {"loss": loss.detach().numpy(), "pos": pos.detach().numpy(), "dS": S.grad.numpy(), "S": S.detach().numpy(),
           "rows": rows_.detach().numpy(), "n": n.numpy(), "total": total.detach().numpy()}
    if ent is not None:
        out.update(g_ent=ent.grad.numpy(), g_rel=rel.grad.numpy())
    return out


err_ref = K.err_ref
typical_term = K.typical_term


@functools.lru_cache(maxsize=None)
def expected(case, mode, eps=0.0, T=1.0, weighted=True):
    """-> (float64 result, err_ref per quantity) of the case's tables on the batch and keys of ``case_rows(case, mode)``."""
    pb, L = U.problem(case), case_rows(case, mode)
    w = pb.weight if weighted else None
    f64, f32 = (compute(pb.model, torch.from_numpy(pb.ent).to(dt), torch.from_numpy(pb.rel).to(dt), L.sample, mode, L.keys, w, eps=eps, T=T)
                for dt in (torch.float64, torch.float32))
    return f64, err_ref(f64, f32)


def block_expected(S32, sample, mode, keys, weight, weight_sum, eps, T, target=None):
    """The loss kernel alone on a given float32 block: the float64 formulas on those very values -> (float64 result, err_ref)."""
    S32 = torch.as_tensor(S32)
    f64, f32 = (compute(None, None, None, sample, mode, keys, weight, weight_sum, eps, T, S=S32.to(dt), target=target)
                for dt in (torch.float64, torch.float32))
    return f64, err_ref(f64, f32)


ERR_FACTOR = U.ERR_FACTOR
# (name, quantity) -> the largest device error / err_ref over both sides and every setting, measured on the MI355X, where it
# exceeds 8 with no defect behind it (profiles/r25_onevsall_filtered_errors.txt has every name, side, setting and quantity).
MEASURED_RATIO: dict = {}


def bound(name, quantity, err, term) -> float:
    """8 x err_ref; a measured ratio widens it to twice that ratio, never past a quarter of one typical term."""
    factor = max(ERR_FACTOR, 2.0 * MEASURED_RATIO.get((name, quantity), 0.0))
    return min(factor * err, max(ERR_FACTOR * err, 0.25 * term))
