"""``Adversarial`` -- self-adversarial negative-sampling loss (reference mkb/losses/adversarial.py:8-30).

``Adversarial(alpha)(positive_score, negative_score, weight)`` returns the scalar loss, differentiable w.r.t.
both score tensors.  Forward and the gradient seed come from ONE kernel sequence (``mkb_adversarial``): the
softmax weights are detached in the reference, so d loss / d scores is available in closed form as soon as the
row statistics are known; backward just scales the saved seeds by the upstream gradient.
"""
import torch

from .. import _hip
from . import _rows

__all__ = ["Adversarial"]


def launch(pos, neg, weight, alpha):
    """One ``mkb_adversarial`` call on contiguous float32 device tensors -> (loss [1], dpos [B], dneg [B, K])."""
    B, K = neg.shape
    loss, dpos, dneg, scratch = _rows.pair_outputs(neg)
    with _hip.on_device(neg.device):
        _hip.check(_hip.lib().mkb_adversarial(_hip.ptr(pos), _hip.ptr(neg), _hip.ptr(weight), None, B, K, alpha,
                                              None, _hip.ptr(loss), _hip.ptr(dpos), _hip.ptr(dneg), _hip.ptr(scratch),
                                              _hip.stream_ptr()), "mkb_adversarial")
    return loss, dpos, dneg


class Adversarial:
    def __init__(self, alpha=0.5):
        self.alpha = alpha

    def __call__(self, positive_score, negative_score, weight):
        _hip.require_device(positive_score, negative_score, weight)
        if positive_score.dim() != 2 or positive_score.size(1) != 1:
            raise ValueError("positive_score must be [B, 1]")  # the reference's squeeze(dim=1) contract
        pos, neg, w = _rows.f32(positive_score), _rows.f32(negative_score), _hip.contiguous(weight, torch.float32)
        if pos.shape[0] == 0:
            return _rows.empty_batch(w, pos, neg)
        alpha = float(self.alpha)
        return _rows.PairSeedsFn.apply(pos, neg, lambda p, n: launch(p, n, w, alpha))
