"""The relation side of link prediction, ``(h, ?, t)``, on the device (mkb_amd/csrc/score_relation.hip): ``relation_scores`` -- the
score of every pair of ``sample`` with every relation (or a list of them), bit for bit what ``model(triples)`` gives each
``(h, r, t)`` -- and ``predict_top_k_relations`` -- for each pair the k best relations and their scores, known facts left out, in
the order of the filtered rank (NaN first, then higher score, then lower relation id).  ``predict_top_k`` keeps answering the two
entity sides only."""
import operator

import torch

from .. import _hip
from .true_keys import true_keys

__all__ = ["relation_scores", "predict_top_k_relations"]


def _pairs(model, sample, relation_column=False):
    """``sample`` as int64 [B, 3] on the model's device, its entity columns (and the relation column when it is read) in range."""
    dev = model.entity_embedding.device
    s = torch.as_tensor(sample, dtype=torch.int64).reshape(-1, 3).to(dev).contiguous()
    if s.shape[0]:
        cols = [0, 1, 2] if relation_column else [0, 2]
        limits = torch.tensor([model.n_entity, model.n_relation, model.n_entity], device=dev)
        if bool(((s[:, cols] < 0) | (s[:, cols] >= limits[cols])).any()):
            raise ValueError("sample holds an entity or relation id outside the model's tables")
    return s


def general_relation_scores(model, s, rel):
    """The same block through the general forward of ``[b, len(rel), 3]`` triples: one workgroup per triple.  The route of shapes
    ``mkb_rel_scores`` does not support, and what the tests compare it with."""
    n_rel = rel.numel()
    block = torch.stack([s[:, 0:1].expand(-1, n_rel), rel.view(1, -1).expand(s.shape[0], -1), s[:, 2:3].expand(-1, n_rel)], dim=-1)
    return model(block.contiguous()).reshape(s.shape[0], n_rel).float().contiguous()


def rel_scores_launch(model, s, rel, out):
    """``mkb_rel_scores`` of the rows of ``s`` (int64 [b, 3], device, contiguous) into ``out`` [b, n_rel] (row stride
    ``out.stride(0)``); ``rel``: int64 device ids or None for every relation.  No validation, no synchronisation.  -> False when
    the library does not support the shape (nothing was launched)."""
    n_rel = model.n_relation if rel is None else rel.numel()
    with _hip.on_device(s.device):
        rc = _hip.lib().mkb_rel_scores(model._tables(), _hip.ptr(s), s.shape[0], _hip.ptr(rel), n_rel, _hip.ptr(out),
                                       max(out.stride(0), n_rel), _hip.stream_ptr())
    if rc == _hip.ERR_UNSUPPORTED:
        return False
    _hip.check(rc, "mkb_rel_scores")
    return True


def relation_scores(model, sample, relations=None):
    """-> FloatTensor ``[B, n_rel]`` on the model's device: entry ``[i, j]`` is the score of ``(h_i, relations[j], t_i)``
    (``relations=None``: relation ``j``, all ``n_relation`` of them), with the bits ``model`` gives that triple.  ``sample`` [B, 3]
    (h, r, t) ids, the relation column is ignored; ``relations``: relation ids in any order, duplicates allowed."""
    dev = model.entity_embedding.device
    _hip.require_device(model.entity_embedding)
    model.sync_parameters()
    s = _pairs(model, sample)
    rel = None
    if relations is not None:
        rel = _hip.contiguous(torch.as_tensor(relations, device=dev).reshape(-1), torch.int64)
        if rel.numel() == 0:
            raise ValueError("relations must hold at least one relation id")
        if bool(((rel < 0) | (rel >= model.n_relation)).any()):
            raise ValueError(f"relation ids must lie in [0, {model.n_relation})")
    out = torch.empty((s.shape[0], model.n_relation if rel is None else rel.numel()), dtype=torch.float32, device=dev)
    if s.shape[0] and not rel_scores_launch(model, s, rel, out):
        with torch.no_grad():
            out = general_relation_scores(model, s, torch.arange(model.n_relation, device=dev) if rel is None else rel)
    return out


def predict_top_k_relations(model, sample, k, true_triples=None, keep_target=False, chunk=4096):
    """-> ``(ids LongTensor [B, k], scores FloatTensor [B, k])`` on the model's device, best first: the k best relations of every
    ``(h, ?, t)`` of ``sample`` [B, 3]; the relation column is ignored unless ``keep_target=True``.  ``true_triples`` (any
    ``[n, 3]`` collection): every relation whose triple ``(h, r', t)`` is one of them is left out -- with ``keep_target=True``
    except the query's own relation, which gives the candidate set of ``Evaluation.relation_ranks``.  When fewer than k relations
    are left (``k > n_relation`` is allowed), the trailing slots hold id -1 and score -inf.  ``chunk`` queries per launch."""
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
    _hip.require_device(model.entity_embedding)
    model.sync_parameters()
    s_all = _pairs(model, sample, relation_column=keep_target)
    n = s_all.shape[0]
    ids = torch.empty((n, k), dtype=torch.int64, device=dev)
    scores = torch.empty((n, k), dtype=torch.float32, device=dev)
    if n == 0:
        return ids, scores
    if true_triples is not None and len(true_triples) > 0:
        keys = true_keys(true_triples, dev, model.n_entity, model.n_relation)["tail-batch"]
    else:
        keys = torch.empty(0, dtype=torch.int64, device=dev)
    flags = _hip.TOPK_KEEP_TARGET if keep_target else 0
    lib, tb, ws = _hip.lib(), model._tables(), _hip.Workspace(dev)
    with _hip.on_device(dev):
        for lo in range(0, n, chunk):
            s = s_all[lo: lo + chunk]
            need = lib.mkb_rel_topk_workspace_bytes(tb, s.shape[0], k)
            _hip.check(lib.mkb_rel_topk(tb, _hip.ptr(s), s.shape[0], _hip.ptr(keys), keys.numel(), k, flags, _hip.ptr(ids[lo: lo + chunk]),
                                        _hip.ptr(scores[lo: lo + chunk]), ws.ptr(need), need, _hip.stream_ptr()), "mkb_rel_topk")
    return ids, scores
