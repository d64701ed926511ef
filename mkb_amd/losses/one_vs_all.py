"""``OneVsAll`` -- the softmax cross entropy over ALL entities (1vsAll; no reference counterpart: the reference trains against
sampled negatives only).

``loss(scores, target, weight=None, sample=None, mode=None, n_relation=None)`` with ``scores`` [B, N] (one column per entity,
higher = more plausible: what ``model.score_all(sample, mode)`` returns), ``target`` [B] int64 (the true column of each row) and
an optional per-row ``weight`` [B] (absent: all ones):

    row_i = log sum_j exp(scores_ij / T) - scores_i,target_i / T          loss = sum_i w_i row_i / sum_i w_i

differentiable in ``scores``.  Forward and the gradient seeds come from ONE kernel sequence (``mkb_all_softmax``), as for the
sampled losses; backward scales the saved seeds by the upstream gradient.  That is plain 1vsAll, the defaults.  Two options go
through another kernel (``mkb_all_softmax_filtered``):

``filter_known=True`` takes a row's OTHER known answers out of its softmax: every ``t`` with ``(h_i, r_i, t)`` in ``true_triples``
(tail-batch; every ``h`` with ``(h, r_i, t_i)`` for head-batch) except the row's own target -- the columns the filtered evaluation
leaves out of the rank.  They are read on the device from the sorted key arrays of the filtered ranking (``utils.true_keys``); no
[B, N] mask is built.  A filtered column takes no part in the row and its gradient is exactly 0.  It needs ``sample`` [B, 3] int64
and ``mode`` (the row's query) and ``true_triples``; ``n_relation``: as for ``KvsAll``.

``label_smoothing=eps`` spreads eps over the n_i columns that stay in row i:

    y_ij  = (1 - eps) [j = target_i] + eps / n_i
    row_i = log sum_{j kept} exp(scores_ij / T) - sum_{j kept} y_ij scores_ij / T

(without filtering n_i = N: ``F.cross_entropy(scores / T, target, label_smoothing=eps)``).  Smoothing alone needs no sample.

The class is also the marker ``compose.Pipeline.learn`` reads: with this loss every batch goes through ``fused.OneVsAllStep`` (no
negatives are drawn; the dataset's alternating head-batch / tail-batch gives both sides; with ``filter_known=True`` and
``true_triples=None`` the known answers are the training triples of the dataset being iterated); with TransE, RotatE or pRotatE
through ``fused.DistanceAllStep``, whose explicit form is ``loss(fused.distance_score_all(model, sample, mode), target, weight)``.
"""
import torch

from .. import _hip
from . import _rows
from .kvs_all import REDUCTIONS, checked_settings, relation_count
from .ns_losses import _checked
from ..utils.true_keys import true_keys

__all__ = ["OneVsAll"]


def launch(S, n_cols, target, target_stride, weight, weight_sum, temperature):
    """One ``mkb_all_softmax`` call on a contiguous float32 device block ``S`` [B, ld] of which the first ``n_cols`` columns count;
    ``target``: int64 device tensor read at ``i * target_stride``.  ``S`` is OVERWRITTEN with the gradient seeds.
    -> (loss [1], pos [B])."""
    B, ld = S.shape
    loss, pos, scratch = _rows.block_outputs(S)
    with _hip.on_device(S.device):
        _hip.check(_hip.lib().mkb_all_softmax(_hip.ptr(S), B, n_cols, ld, _hip.ptr(target), target_stride, _hip.ptr(weight),
                                              _hip.ptr(weight_sum), temperature, _hip.ptr(loss), _hip.ptr(pos), _hip.ptr(scratch),
                                              _hip.stream_ptr()), "mkb_all_softmax")
    return loss, pos


def launch_filtered(S, n_cols, target, target_stride, sample, mode_id, n_relation, keys, weight, weight_sum, temperature, label_smoothing):
    """One ``mkb_all_softmax_filtered`` call on the block of ``launch``; ``sample`` [B, 3] and ``mode_id`` name each row's query,
    ``keys``: the sorted int64 device keys of ``mode_id``'s side, or None (nothing is filtered).  -> (loss [1], pos [B])."""
    B, ld = S.shape
    loss, pos, scratch = _rows.block_outputs(S)
    with _hip.on_device(S.device):
        _hip.check(_hip.lib().mkb_all_softmax_filtered(_hip.ptr(S), B, n_cols, ld, _hip.ptr(target), target_stride, _hip.ptr(sample), mode_id,
                                                       n_relation, _hip.ptr(keys), 0 if keys is None else keys.numel(), _hip.ptr(weight),
                                                       _hip.ptr(weight_sum), temperature, label_smoothing, _hip.ptr(loss), _hip.ptr(pos),
                                                       _hip.ptr(scratch), _hip.stream_ptr()), "mkb_all_softmax_filtered")
    return loss, pos


class OneVsAll:
    kind = None  # (not one of mkb_ns_loss's kinds: fused.PooledLossStep refuses it)

    def __init__(self, temperature=1.0, label_smoothing=0.0, filter_known=False, true_triples=None):
        self.temperature = _checked("temperature", temperature, positive=True)
        self.label_smoothing = checked_settings(label_smoothing, REDUCTIONS[0])[0]
        self.filter_known, self.true_triples = bool(filter_known), true_triples
        self._n_relation = None

    def __call__(self, scores, target, weight=None, sample=None, mode=None, n_relation=None):
        _hip.require_device(scores, target, weight, sample)
        if self.filter_known:
            if sample is None or mode is None:
                raise ValueError("OneVsAll(filter_known=True) needs sample and mode: they name the query whose known answers are filtered")
            if self.true_triples is None:
                raise ValueError("OneVsAll needs true_triples to filter a score block (only compose.Pipeline fills them in from its dataset)")
        _rows.check_scores(scores)
        if target.shape != (scores.size(0),) or target.dtype != torch.int64:
            raise ValueError("target must be an int64 tensor [B]")
        _rows.check_weight(weight, scores.size(0))
        if self.filter_known:
            mode_id = _hip.side_id(mode, "1vsAll filtering")
            if sample.shape != (scores.size(0), 3) or sample.dtype != torch.int64:
                raise ValueError("sample must be an int64 tensor [B, 3]")
        s, w = _rows.f32(scores), _rows.f32(weight)
        if s.shape[0] == 0:
            return _rows.empty_batch(w, s)
        target, T = _hip.contiguous(target, torch.int64), float(self.temperature)
        if not self.filter_known and self.label_smoothing == 0.0:
            return _rows.SeedsInPlaceFn.apply(s, lambda S: launch(S, S.shape[1], target, 1, w, None, T))
        if self.filter_known:
            n_relation = relation_count(self) if n_relation is None else int(n_relation)
            keys = true_keys(self.true_triples, s.device, s.size(1), n_relation)["head-batch" if mode_id == _hip.MODE_HEAD else "tail-batch"]
            sample = _hip.contiguous(sample, torch.int64)
        else:  # no keys: no query owns any, so any sample [B, 3] of ids inside the tables does
            sample, mode_id, n_relation, keys = torch.zeros((s.shape[0], 3), dtype=torch.int64, device=s.device), _hip.MODE_TAIL, 1, None
        return _rows.SeedsInPlaceFn.apply(s, lambda S: launch_filtered(S, S.shape[1], target, 1, sample, mode_id, n_relation, keys, w, None, T,
                                                                       self.label_smoothing))

    def __repr__(self):
        extra = "" if not (self.label_smoothing or self.filter_known) else f", label_smoothing={self.label_smoothing}, filter_known={self.filter_known}"
        return f"OneVsAll(temperature={self.temperature}{extra})"
