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
from .ns_losses import _checked

__all__ = ["OneVsAll"]


def launch(S, n_cols, target, target_stride, weight, weight_sum, temperature):
    """One ``mkb_all_softmax`` call on a contiguous float32 device block ``S`` [B, ld] of which the first ``n_cols`` columns count;
    ``target``: int64 device tensor read at ``i * target_stride``.  ``S`` is OVERWRITTEN with the gradient seeds.
    -> (loss [1], pos [B])."""
    B, ld = S.shape
    dev = S.device
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    pos = torch.empty(B, dtype=torch.float32, device=dev)
    scratch = torch.empty(B + 1, dtype=torch.float32, device=dev)
    with _hip.on_device(dev):
        _hip.check(_hip.lib().mkb_all_softmax(_hip.ptr(S), B, n_cols, ld, _hip.ptr(target), target_stride, _hip.ptr(weight),
                                              _hip.ptr(weight_sum), temperature, _hip.ptr(loss), _hip.ptr(pos), _hip.ptr(scratch),
                                              _hip.stream_ptr()), "mkb_all_softmax")
    return loss, pos


class _OneVsAllFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores, target, weight, temperature):
        seeds = scores.detach().clone(memory_format=torch.contiguous_format)  # the kernel works in place
        loss, _ = launch(seeds, seeds.shape[1], target, 1, weight, None, temperature)
        ctx.save_for_backward(seeds)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (seeds,) = ctx.saved_tensors
        return g * seeds, None, None, None


class OneVsAll:
    kind = None  # (not one of mkb_ns_loss's kinds: fused.PooledLossStep refuses it)

    def __init__(self, temperature=1.0):
        self.temperature = _checked("temperature", temperature, positive=True)

    def __call__(self, scores, target, weight=None):
        _hip.require_device(scores, target, weight)
        if scores.dim() != 2 or scores.size(1) < 1:
            raise ValueError("scores must be [B, N] with N >= 1")
        if target.shape != (scores.size(0),) or target.dtype != torch.int64:
            raise ValueError("target must be an int64 tensor [B]")
        if weight is not None and weight.shape != (scores.size(0),):
            raise ValueError("weight must be [B]")
        s = _hip.contiguous(scores, torch.float32)
        w = None if weight is None else _hip.contiguous(weight, torch.float32)
        if s.shape[0] == 0:  # as the sampled losses answer an empty batch: empty sums over W = 0 -> nan, no launch
            wsum = s.sum() if w is None else w.sum()
            return (s.sum() + wsum) / wsum
        return _OneVsAllFn.apply(s, _hip.contiguous(target, torch.int64), w, float(self.temperature))

    def __repr__(self):
        return f"OneVsAll(temperature={self.temperature})"
