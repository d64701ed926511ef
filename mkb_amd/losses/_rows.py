"""What the row losses share around their kernel call: the argument checks and conversions, the empty-batch answer, the output
allocations of the all-entity losses and the two autograd functions -- every loss of the package computes its gradient seeds in
the forward launch, and backward only scales them by the upstream gradient."""
import torch

from .. import _hip


def f32(t):
    """``t`` as a contiguous float32 tensor; None stays None."""
    return None if t is None else _hip.contiguous(t, torch.float32)


def check_weight(weight, B):
    if weight is not None and weight.shape != (B,):
        raise ValueError("weight must be [B]")


def check_scores(scores):
    """The [B, N] score block of the all-entity losses."""
    if scores.dim() != 2 or scores.size(1) < 1:
        raise ValueError("scores must be [B, N] with N >= 1")


def empty_batch(w, *scores):
    """What every loss answers for B = 0 without a launch: empty sums over W = 0 -> nan, attached to the graph of ``scores`` (the
    reference's Adversarial divides two empty sums by W = 0, losses/adversarial.py:28-30)."""
    wsum = scores[0].sum() if w is None else w.sum()
    return (sum(s.sum() for s in scores) + wsum) / wsum


def block_outputs(S):
    """-> (loss [1], pos [B], scratch [B + 1]) of one all-entity loss call on the block ``S`` [B, ld]."""
    B, dev = S.shape[0], S.device
    return (torch.empty(1, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.float32, device=dev),
            torch.empty(B + 1, dtype=torch.float32, device=dev))


def pair_outputs(neg):
    """-> (loss [1], dpos [B], dneg [B, K], scratch [B + 1]) of one sampled-loss call on the negatives' block [B, K]."""
    (B, K), dev = neg.shape, neg.device
    return (torch.empty(1, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.float32, device=dev),
            torch.empty((B, K), dtype=torch.float32, device=dev), torch.empty(B + 1, dtype=torch.float32, device=dev))


class SeedsInPlaceFn(torch.autograd.Function):
    """``launch(S) -> (loss [1], ...)`` overwrites the score block with the seeds (the all-entity losses)."""

    @staticmethod
    def forward(ctx, scores, launch):
        seeds = scores.detach().clone(memory_format=torch.contiguous_format)  # the kernel works in place
        loss = launch(seeds)[0]
        ctx.save_for_backward(seeds)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (seeds,) = ctx.saved_tensors
        return g * seeds, None


class PairSeedsFn(torch.autograd.Function):
    """``launch(pos, neg) -> (loss [1], dpos [B], dneg [B, K])`` (the sampled losses)."""

    @staticmethod
    def forward(ctx, pos, neg, launch):
        loss, dpos, dneg = launch(pos, neg)
        ctx.save_for_backward(dpos, dneg)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        dpos, dneg = ctx.saved_tensors
        return (g * dpos).view(-1, 1), g * dneg, None
