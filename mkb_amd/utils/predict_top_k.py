"""``predict_top_k``: batched, filtered link prediction on the device -- for each ``(h, r, ?)`` (tail-batch) or ``(?, r, t)``
(head-batch) query, the k best entities and their scores, known facts left out (``mkb_topk`` in mkb_amd/csrc/rank.hip).  The scores
are those of the all-entity block ``Evaluation.ranks(..., with_scores=True)`` hands out, the order that of the filtered rank (NaN
first, then higher score, then lower entity id); no ``[B, n_entity]`` block is ever returned or kept.  ``candidates`` limits the
predictions to a subset of the entities (``mkb_topk_masked``)."""
import operator

import torch

from .. import _hip
from .true_keys import true_keys

__all__ = ["predict_top_k", "candidate_bits"]

_MODES = ("head-batch", "tail-batch")


def candidate_bits(candidates, n_entity, device):
    """-> the candidate bitmask of ``mkb_topk_masked``: int32 words [ceil(n_entity / 32)] on ``device``, bit e % 32 of word e / 32
    set when entity e is a candidate.  ``candidates``: entity ids (any int sequence / tensor; duplicates allowed) or a bool mask
    of length ``n_entity``."""
    if isinstance(candidates, (list, tuple)) and len(candidates) == 0:
        c = torch.empty(0, dtype=torch.int64, device=device)
    else:
        c = torch.as_tensor(candidates, device=device)
    if c.dtype == torch.bool:
        if c.dim() != 1 or c.shape[0] != n_entity:
            raise ValueError(f"a bool candidate mask must have shape ({n_entity},), got {tuple(c.shape)}")
        mask = c
    else:
        if c.is_floating_point() or c.is_complex():
            raise ValueError("candidates must be entity ids (integers) or a bool mask over the entities")
        ids = c.reshape(-1).to(torch.int64)
        if ids.numel() and bool(((ids < 0) | (ids >= n_entity)).any()):
            raise ValueError(f"candidate entity ids must lie in [0, {n_entity})")
        mask = torch.zeros(n_entity, dtype=torch.bool, device=device)
        mask[ids] = True
    words = (n_entity + 31) // 32
    padded = torch.zeros(words * 32, dtype=torch.int64, device=device)
    padded[:n_entity] = mask.to(torch.int64)
    bits = (padded.view(words, 32) << torch.arange(32, device=device)).sum(dim=1)  # < 2^32
    return torch.where(bits >= 1 << 31, bits - (1 << 32), bits).to(torch.int32).contiguous()


def predict_top_k(model, sample, mode, k, true_triples=None, keep_target=False, chunk=1024, candidates=None):
    """-> ``(ids LongTensor [B, k], scores FloatTensor [B, k])`` on the model's device, best first.

    ``sample`` [B, 3] (h, r, t) ids; the column ``mode`` replaces (h for head-batch, t for tail-batch) is ignored unless
    ``keep_target=True``.  ``true_triples`` (any ``[n, 3]`` collection): every candidate whose corrupted triple is one of them is
    left out -- with ``keep_target=True`` except the query's own target, which gives the candidate set of the filtered rank.
    When fewer than k candidates are left, the trailing slots hold id -1 and score -inf.  ``chunk`` queries per launch.
    ``candidates``: entity ids, or a bool mask over the ``n_entity`` entities -- only those are predicted (an entity outside them
    is left out like a filtered one, the target with ``keep_target=True`` included); ``None``: every entity."""
    if mode not in _MODES:
        raise ValueError(f"mode must be 'head-batch' or 'tail-batch', got {mode!r}")
    try:
        k_ok = not isinstance(k, bool) and 1 <= operator.index(k) <= _hip.TOPK_MAX_K
    except TypeError:
        k_ok = False
    if not k_ok:
        raise ValueError(f"k must be an int in [1, {_hip.TOPK_MAX_K}], got {k!r}")
    k = operator.index(k)
    if chunk < 1:
        raise ValueError(f"chunk must be positive, got {chunk!r}")
    dev = model.entity_embedding.device
    bits = None if candidates is None else candidate_bits(candidates, model.n_entity, dev)
    _hip.require_device(model.entity_embedding)
    model.sync_parameters()
    s_all = torch.as_tensor(sample, dtype=torch.int64).reshape(-1, 3).to(dev)
    n = s_all.shape[0]
    ids = torch.empty((n, k), dtype=torch.int64, device=dev)
    scores = torch.empty((n, k), dtype=torch.float32, device=dev)
    if n == 0:
        return ids, scores
    # the columns the kernels read as table rows must be in range (the target column only with keep_target)
    cols = [1, 2] if mode == "head-batch" else [0, 1]
    if keep_target:
        cols = [0, 1, 2]
    limits = torch.tensor([model.n_entity, model.n_relation, model.n_entity], device=dev)
    bad = (s_all[:, cols] < 0) | (s_all[:, cols] >= limits[cols])
    if bool(bad.any()):
        raise ValueError("sample holds an entity or relation id outside the model's tables")
    if true_triples is not None and len(true_triples) > 0:
        keys = true_keys(true_triples, dev, model.n_entity, model.n_relation)[mode]
    else:
        keys = torch.empty(0, dtype=torch.int64, device=dev)
    flags = _hip.TOPK_KEEP_TARGET if keep_target else 0
    return _launch(model, s_all, mode, k, keys, flags, bits, chunk, ids, scores)


def _launch(model, s_all, mode, k, keys, flags, bits, chunk, ids, scores):
    """mkb_topk (bits None) / mkb_topk_masked over the rows of s_all in chunks; no validation, no synchronisation."""
    dev = model.entity_embedding.device
    lib, tb, ws = _hip.lib(), model._tables(), _hip.Workspace(dev)
    name, mask = ("mkb_topk", ()) if bits is None else ("mkb_topk_masked", (_hip.ptr(bits),))  # (the mask follows the keys)
    fn = getattr(lib, name)
    with _hip.on_device(dev):
        for lo in range(0, s_all.shape[0], chunk):
            s = s_all[lo: lo + chunk].contiguous()
            need = lib.mkb_topk_workspace_bytes(tb, s.shape[0], k)
            _hip.check(fn(tb, _hip.ptr(s), s.shape[0], _hip.mode_id(mode), _hip.ptr(keys), keys.numel(), *mask, k, flags,
                          _hip.ptr(ids[lo: lo + chunk]), _hip.ptr(scores[lo: lo + chunk]), ws.ptr(need), need, _hip.stream_ptr()),
                       name)
    return ids, scores


def topk_block(S, k, ids=None, scores=None):
    """-> ``(ids, scores)`` [B, k]: the k best columns of each row of the fp32 device block ``S`` [B, N] (row stride
    ``S.stride(0)``), NaN first, then higher value, then lower column; -1 / -inf past N (``mkb_topk_block``)."""
    _hip.require_device(S)
    if S.dtype != torch.float32 or S.dim() != 2 or S.stride(1) != 1:
        raise ValueError("S must be a 2-D float32 device tensor with unit column stride")
    B, N = S.shape
    if ids is None:
        ids = torch.empty((B, k), dtype=torch.int64, device=S.device)
    if scores is None:
        scores = torch.empty((B, k), dtype=torch.float32, device=S.device)
    if B:
        with _hip.on_device(S.device):
            _hip.check(_hip.lib().mkb_topk_block(_hip.ptr(S), B, N, max(S.stride(0), N), k, _hip.ptr(ids), _hip.ptr(scores),
                                                 _hip.stream_ptr()), "mkb_topk_block")
    return ids, scores


def topk_nearest(Q, X, cand, k, ids=None, dists=None, block=None):
    """-> ``(ids, dists)`` [B, k]: for each row of the fp32 device block ``Q`` [B, D] the k candidates of ``cand`` (int64 row ids
    of the fp32 device table ``X`` [n, D]) with the smallest squared L2 distance, nearest first; equal distances go to the lower
    position in ``cand``, NaN first; -1 / +inf past the candidates (``mkb_topk_nearest``).  ``ids`` hold the ``cand`` values.
    ``block``: a [B, len(cand)] fp32 device tensor that receives the whole distance block (``mkb_topk_nearest_dists``)."""
    _hip.require_device(Q, X, cand)
    for name, t in (("Q", Q), ("X", X)):
        if t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1:
            raise ValueError(f"{name} must be a 2-D float32 device tensor with unit column stride")
    if Q.shape[1] != X.shape[1]:
        raise ValueError(f"Q and X must have the same number of columns, got {Q.shape[1]} and {X.shape[1]}")
    cand = _hip.contiguous(cand.reshape(-1), torch.int64)
    (B, D), n = Q.shape, cand.numel()
    if ids is None:
        ids = torch.empty((B, k), dtype=torch.int64, device=Q.device)
    if dists is None:
        dists = torch.empty((B, k), dtype=torch.float32, device=Q.device)
    if B:
        lib = _hip.lib()
        need = lib.mkb_topk_nearest_workspace_bytes(B, n, k)
        ws = _hip.aligned_bytes(need, Q.device) if need > 0 else None
        args = (_hip.ptr(Q), Q.stride(0) if B > 1 else D, _hip.ptr(X), X.stride(0) if X.shape[0] > 1 else D, _hip.ptr(cand), n, B, D, k,
                _hip.ptr(ids), _hip.ptr(dists))
        with _hip.on_device(Q.device):
            if block is None:
                _hip.check(lib.mkb_topk_nearest(*args, _hip.ptr(ws), need, _hip.stream_ptr()), "mkb_topk_nearest")
            else:
                _hip.check(lib.mkb_topk_nearest_dists(*args, _hip.ptr(block), _hip.ptr(ws), need, _hip.stream_ptr()),
                           "mkb_topk_nearest_dists")
    return ids, dists
