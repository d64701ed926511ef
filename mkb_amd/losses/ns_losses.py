"""``MarginRanking``, ``PairwiseLogistic`` and ``CrossEntropy`` -- the negative-sampling losses next to ``Adversarial``
(no reference counterpart: the reference trains with ``Adversarial`` only).

Each is called as ``loss(positive_score, negative_score, weight=None)`` with ``positive_score`` [B, 1], ``negative_score``
[B, K] (higher = more plausible) and an optional per-row ``weight`` [B] (absent: all ones); the scalar returned is
``sum_i w_i row_i / sum_i w_i`` and is differentiable in both score tensors.  With ``a_ij = margin + neg_ij - pos_i``:

  * ``MarginRanking(margin=1.0, alpha=0.0)``:      ``row_i = sum_j p_ij max(0, a_ij)``        (the loss TransE was published with)
  * ``PairwiseLogistic(margin=0.0, alpha=0.0)``:   ``row_i = sum_j p_ij softplus(a_ij)``      (BPR-style)
  * ``CrossEntropy(temperature=1.0)``:             ``row_i = -log softmax([pos_i, neg_i] / T)[0]``  (sampled softmax)

``p_ij = softmax_j(alpha * neg_ij)`` is the detached self-adversarial weight of ``Adversarial``; ``alpha = 0`` is the plain
mean over the negatives.  (The pointwise logistic loss is ``Adversarial(alpha=0)``.)

Forward and the gradient seeds come from ONE kernel sequence (``mkb_ns_loss``), as for ``Adversarial``; backward scales the
saved seeds by the upstream gradient.
"""
import math

import torch

from .. import _hip
from . import _rows

__all__ = ["MarginRanking", "PairwiseLogistic", "CrossEntropy"]


def launch(kind, pos, neg, weight, cnt, param, alpha, weight_sum=None):
    """One ``mkb_ns_loss`` call on contiguous float32 device tensors -> (loss [1], dpos [B], dneg [B, K]); ``cnt`` (uint16
    [B, K] multiplicities) and ``weight`` / ``weight_sum`` may be None."""
    B, K = neg.shape
    loss, dpos, dneg, scratch = _rows.pair_outputs(neg)
    with _hip.on_device(neg.device):
        _hip.check(_hip.lib().mkb_ns_loss(kind, _hip.ptr(pos), _hip.ptr(neg), _hip.ptr(weight), _hip.ptr(cnt), B, K, param, alpha,
                                          _hip.ptr(weight_sum), _hip.ptr(loss), _hip.ptr(dpos), _hip.ptr(dneg), _hip.ptr(scratch),
                                          _hip.stream_ptr()), "mkb_ns_loss")
    return loss, dpos, dneg


class _NsLoss:
    """What the three classes share: argument checks, the empty batch, the kernel call.  ``kind`` / ``param`` / ``alpha`` are the
    arguments of ``mkb_ns_loss`` (``fused.PooledLossStep`` reads them too)."""

    kind = None

    @property
    def param(self):
        raise NotImplementedError

    def __call__(self, positive_score, negative_score, weight=None):
        _hip.require_device(positive_score, negative_score, weight)
        if positive_score.dim() != 2 or positive_score.size(1) != 1:
            raise ValueError("positive_score must be [B, 1]")
        if negative_score.dim() != 2 or negative_score.size(0) != positive_score.size(0) or negative_score.size(1) < 1:
            raise ValueError("negative_score must be [B, K] with K >= 1")
        _rows.check_weight(weight, positive_score.size(0))
        pos, neg, w = _rows.f32(positive_score), _rows.f32(negative_score), _rows.f32(weight)
        if pos.shape[0] == 0:
            return _rows.empty_batch(w, pos, neg)
        kind, param, alpha = self.kind, float(self.param), float(self.alpha)
        return _rows.PairSeedsFn.apply(pos, neg, lambda p, n: launch(kind, p, n, w, None, param, alpha))


def _checked(name, value, positive=False, nonnegative=False):
    value = float(value)
    if not math.isfinite(value) or (positive and value <= 0) or (nonnegative and value < 0):
        raise ValueError(f"{name} must be finite" + (" and > 0" if positive else " and >= 0" if nonnegative else "") + f", not {value}")
    return value


class _Pairwise(_NsLoss):
    def __init__(self, margin, alpha):
        self.margin, self.alpha = _checked("margin", margin), _checked("alpha", alpha, nonnegative=True)

    @property
    def param(self):
        return self.margin

    def __repr__(self):
        return f"{type(self).__name__}(margin={self.margin}, alpha={self.alpha})"


class MarginRanking(_Pairwise):
    kind = _hip.LOSS_MARGIN

    def __init__(self, margin=1.0, alpha=0.0):
        super().__init__(margin, alpha)


class PairwiseLogistic(_Pairwise):
    kind = _hip.LOSS_PAIR_LOGISTIC

    def __init__(self, margin=0.0, alpha=0.0):
        super().__init__(margin, alpha)


class CrossEntropy(_NsLoss):
    kind = _hip.LOSS_SOFTMAX
    alpha = 0.0

    def __init__(self, temperature=1.0):
        self.temperature = _checked("temperature", temperature, positive=True)

    @property
    def param(self):
        return self.temperature

    def __repr__(self):
        return f"CrossEntropy(temperature={self.temperature})"
