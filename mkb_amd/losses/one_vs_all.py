"""``OneVsAll`` -- the softmax cross entropy over ALL entities (1vsAll; no reference counterpart: the reference trains against
sampled negatives only).

``loss(scores, target, weight=None)`` with ``scores`` [B, N] (one column per entity, higher = more plausible: what
``model.score_all(sample, mode)`` returns), ``target`` [B] int64 (the true column of each row) and an optional per-row ``weight``
[B] (absent: all ones):

    row_i = log sum_j exp(scores_ij / T) - scores_i,target_i / T          loss = sum_i w_i row_i / sum_i w_i

differentiable in ``scores``.  No filtering of a row's other known answers: plain 1vsAll.  Forward and the gradient seeds come from
ONE kernel sequence (``mkb_all_softmax``), as for the sampled losses; backward scales the saved seeds by the upstream gradient.

The class is also the marker ``compose.Pipeline.learn`` reads: with this loss every batch goes through ``fused.OneVsAllStep`` (no
negatives are drawn; the dataset's alternating head-batch / tail-batch gives both sides).  ComplEx and DistMult only -- for the
distance models use the sampled ``CrossEntropy``.
"""
import torch

from .. import _hip
from . import _rows
from .ns_losses import _checked

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


class OneVsAll:
    kind = None  # (not one of mkb_ns_loss's kinds: fused.PooledLossStep refuses it)

    def __init__(self, temperature=1.0):
        self.temperature = _checked("temperature", temperature, positive=True)

    def __call__(self, scores, target, weight=None):
        _hip.require_device(scores, target, weight)
        _rows.check_scores(scores)
        if target.shape != (scores.size(0),) or target.dtype != torch.int64:
            raise ValueError("target must be an int64 tensor [B]")
        _rows.check_weight(weight, scores.size(0))
        s, w = _rows.f32(scores), _rows.f32(weight)
        if s.shape[0] == 0:
            return _rows.empty_batch(w, s)
        target, T = _hip.contiguous(target, torch.int64), float(self.temperature)
        return _rows.SeedsInPlaceFn.apply(s, lambda S: launch(S, S.shape[1], target, 1, w, None, T))

    def __repr__(self):
        return f"OneVsAll(temperature={self.temperature})"
