"""The float64 reference of the negative-sampling loss family (include/mkb_hip.h, mkb_ns_loss): a torch restatement of the
definitions, with autograd for the gradients.  CPU only; the kernel is never compared with itself.

    pairwise kinds, a_ij = param + neg_ij - pos_i:  row_i = sum_j p_ij f(a_ij), p_ij = c_ij exp(alpha neg_ij) / sum_l c_il exp(alpha
    neg_il) DETACHED, f = relu (margin) / softplus (pairwise logistic)
    softmax, T = param:  row_i = log(exp(pos_i / T) + sum_j c_ij exp(neg_ij / T)) - pos_i / T
    loss = sum_i w_i row_i / W, W = sum_i w_i or the caller's weight_sum

A position with c_ij = 0 takes no part and its neg value is not used (it may be NaN); a row with no position contributes 0.
"""
import numpy as np
import torch

MARGIN, PAIR_LOGISTIC, SOFTMAX = 0, 1, 2
KINDS = {"margin": MARGIN, "pairwise": PAIR_LOGISTIC, "softmax": SOFTMAX}


def rows(kind, pos, neg, cnt, param, alpha):
    """row_i [B] (float64 torch, differentiable in pos [B] and neg [B, K]); cnt [B, K] float64 or None."""
    B, K = neg.shape
    c = torch.ones_like(neg) if cnt is None else cnt
    used = c > 0
    v = torch.where(used, neg, torch.zeros_like(neg))  # an unused position's value never enters an expression
    neg_inf = torch.full_like(neg, -np.inf)
    if kind == SOFTMAX:
        logits = torch.cat([pos.view(B, 1) / param, torch.where(used, v / param + torch.log(c.clamp(min=1)), neg_inf)], 1)
        return torch.logsumexp(logits, 1) - pos / param
    lw = torch.where(used, alpha * v.detach() + torch.log(c.clamp(min=1)), neg_inf)
    any_used = used.any(1, keepdim=True)
    p = torch.where(any_used, torch.softmax(torch.where(any_used, lw, torch.zeros_like(lw)), 1), torch.zeros_like(lw))
    p = torch.where(used, p, torch.zeros_like(p))
    a = param + v - pos.view(B, 1)
    f = torch.relu(a) if kind == MARGIN else torch.nn.functional.softplus(a)
    return (p * f).sum(1)


def reference(kind, pos, neg, weight=None, cnt=None, param=1.0, alpha=0.0, weight_sum=None):
    """-> (loss, dpos [B], dneg [B, K]) as float64 numpy; inputs: anything np.asarray takes."""
    pos64 = torch.tensor(np.asarray(pos, dtype=np.float64).reshape(-1), requires_grad=True)
    neg64 = torch.tensor(np.asarray(neg, dtype=np.float64), requires_grad=True)
    w = torch.ones_like(pos64) if weight is None else torch.tensor(np.asarray(weight, dtype=np.float64))
    c = None if cnt is None else torch.tensor(np.asarray(cnt, dtype=np.float64))
    W = w.sum() if weight_sum is None else float(weight_sum)
    if c is not None:  # NaN at an unused position must not reach autograd's products: mask the INPUT, keep the leaf's shape
        neg_in = torch.where(c > 0, neg64, torch.zeros_like(neg64))
    else:
        neg_in = neg64
    loss = (w * rows(kind, pos64, neg_in, c, float(param), float(alpha))).sum() / W
    loss.backward()
    return float(loss.detach()), pos64.grad.numpy(), neg64.grad.numpy()


def expand_row(neg_row, cnt_row):
    """One row written out with repeated columns: what the multiplicities stand for."""
    return np.repeat(np.asarray(neg_row), np.asarray(cnt_row, dtype=np.int64))
