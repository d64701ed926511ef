"""Numpy restatements of the relation side's contract (include/mkb_hip.h, "relation prediction"), written from the contract and not
from the kernels: the filter, the filtered rank and the filtered top k of an ``(h, ?, t)`` query on a given score block."""
import numpy as np


def filter_mask(sample, keys, n_entity, n_relation):
    """bool [B, R]: ``(h_i, r', t_i)`` is one of the tail-batch keys ``(h * R + r) * N + t``."""
    sample = np.asarray(sample, dtype=np.int64).reshape(-1, 3)
    k = (sample[:, 0:1] * n_relation + np.arange(n_relation, dtype=np.int64)) * n_entity + sample[:, 2:3]
    return np.isin(k, np.asarray(keys, dtype=np.int64))


def ranks_before(a, ia, b, ib):
    """NaN first, then higher, then lower id (elementwise)."""
    an, bn = np.isnan(a), np.isnan(b)
    with np.errstate(invalid="ignore"):
        plain = (a > b) | ((a == b) & (ia < ib))
    return np.where(an | bn, an & (~bn | (ia < ib)), plain)


def rel_ranks(block, sample, mask):
    """int64 [B]: 1 + the relations r' != r whose v[r'] ranks before v[r]; v[r'] = s[r] + (-1) where r' != r is filtered."""
    block = np.asarray(block, dtype=np.float32)
    sample = np.asarray(sample, dtype=np.int64).reshape(-1, 3)
    R = block.shape[1]
    ids = np.arange(R, dtype=np.int64)
    out = np.empty(len(sample), dtype=np.int64)
    for i, r in enumerate(sample[:, 1]):
        s = block[i]
        with np.errstate(invalid="ignore", over="ignore"):
            biased = np.float32(s[r] + np.float32(-1.0))
        v = np.where(mask[i] & (ids != r), biased, s)
        out[i] = 1 + int((ranks_before(v, ids, np.full(R, s[r], np.float32), np.full(R, r)) & (ids != r)).sum())
    return out


def rel_topk(block, sample, mask, k, keep_target):
    """-> (ids int64 [B, k], scores float32 [B, k]): the unfiltered relations (and the target with keep_target) in a composite
    sort -- NaN first, higher score, lower id -- padded with -1 / -inf."""
    block = np.asarray(block, dtype=np.float32)
    sample = np.asarray(sample, dtype=np.int64).reshape(-1, 3)
    B, R = block.shape
    ids = np.full((B, k), -1, dtype=np.int64)
    scores = np.full((B, k), -np.inf, dtype=np.float32)
    for i in range(B):
        cand = ~mask[i]
        if keep_target:
            cand = cand.copy()
            cand[sample[i, 1]] = True
        c = np.flatnonzero(cand)
        s = block[i, c]
        nan = np.isnan(s)
        order = np.lexsort((c, -np.where(nan, np.float32(0), s) + np.float32(0), ~nan))[:k]  # last key first
        ids[i, : len(order)] = c[order]
        scores[i, : len(order)] = s[order]
    return ids, scores
