"""``predict_top_k``: batched, filtered link prediction on the device -- for each ``(h, r, ?)`` (tail-batch) or ``(?, r, t)``
(head-batch) query, the k best entities and their scores, known facts left out (``mkb_topk`` in mkb_amd/csrc/rank.hip).  The scores
are those of the all-entity block ``Evaluation.ranks(..., with_scores=True)`` hands out, the order that of the filtered rank (NaN
first, then higher score, then lower entity id); no ``[B, n_entity]`` block is ever returned or kept."""
import ctypes
import operator

import torch

from .. import _hip
from .true_keys import true_keys

__all__ = ["predict_top_k"]

_MODES = ("head-batch", "tail-batch")


def predict_top_k(model, sample, mode, k, true_triples=None, keep_target=False, chunk=1024):
    """-> ``(ids LongTensor [B, k], scores FloatTensor [B, k])`` on the model's device, best first.

    ``sample`` [B, 3] (h, r, t) ids; the column ``mode`` replaces (h for head-batch, t for tail-batch) is ignored unless
    ``keep_target=True``.  ``true_triples`` (any ``[n, 3]`` collection): every candidate whose corrupted triple is one of them is
    left out -- with ``keep_target=True`` except the query's own target, which gives the candidate set of the filtered rank.
    When fewer than k candidates are left, the trailing slots hold id -1 and score -inf.  ``chunk`` queries per launch."""
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
    _hip.require_device(model.entity_embedding)
    dev = model.entity_embedding.device
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
    lib, tb = _hip.lib(), model._tables()
    ws = None
    with _hip.on_device(dev):
        for lo in range(0, n, chunk):
            s = s_all[lo: lo + chunk].contiguous()
            need = lib.mkb_topk_workspace_bytes(tb, s.shape[0], k)
            if ws is None or ws.numel() < need + 256:
                ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
            off = (-ws.data_ptr()) % 256
            _hip.check(lib.mkb_topk(tb, _hip.ptr(s), s.shape[0], _hip.mode_id(mode), _hip.ptr(keys), keys.numel(), k, flags,
                                    _hip.ptr(ids[lo: lo + chunk]), _hip.ptr(scores[lo: lo + chunk]),
                                    ctypes.c_void_p(ws.data_ptr() + off), need, _hip.stream_ptr()),
                       "mkb_topk")
    return ids, scores
