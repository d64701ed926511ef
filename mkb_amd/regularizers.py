"""Embedding regularisers on the device: ``Lp`` (p = 2, 3) with the shorthands ``N3`` and ``L2`` (``mkb_reg_rows``,
mkb_amd/csrc/reg_rows.hip).  No reference counterpart: with the reference a user writes the penalty in torch on gathered rows.

    reg = sum_i (w_i / W) [entity_weight (f(E[h_i]) + f(E[t_i])) + relation_weight f(R[r_i])]

over the POSITIVE triples of a batch, ``f(x) = sum_k |x_k|^p`` -- for a table whose rows the model reads as ``[re | im]`` halves
(ComplEx: both tables; RotatE: the entity table) ``f(x) = sum_k (re_k^2 + im_k^2)^(p / 2)``, the N3 of Lacroix et al. for
complex models.  pRotatE's modulus is not regularised.

    regulariser = regularizers.N3(1e-3)
    error = loss(positive_score, negative_score, weight) + regulariser(model, sample, weight)
    error.backward()

The torch expression gives the same numbers, but autograd's backward of its gather is a dense zero-filled table added into
``.grad`` behind the optimizer's back, after which a row-lazy ``mkb_amd.optim.Adam`` falls back to the dense kernel for good.
This one writes only the gradient rows of the batch's heads, tails and relations and reports them to the row-lazy protocol
exactly as ``model(...)`` does (``before_forward`` in front, ``_gradshare.direct`` / ``rows_written`` in backward).  The fused
steps take it as ``regularizer=`` (``fused.FusedTrainStep`` / ``PooledLossStep``), ``compose.Pipeline`` as its ``regularizer``
attribute.
"""
import math

import torch

from . import _gradshare, _hip, _links, fused
from .models import base as _base

__all__ = ["L2", "Lp", "N3"]


def _workspace(model, B):
    """Scratch of ``mkb_reg_rows`` (the sorted occurrence list and the per-row value slots), cached like the pooled kernels'
    (and guarded like it under MKB_WS_GUARD=1: ``fused.check_workspace_guards``)."""
    dev = model.entity_embedding.device
    key = (dev, _hip.stream_ptr(dev).value, "reg_rows", model.name, model.entity_dim, model.n_entity, model.n_relation, B)
    return fused.cached_workspace(key, dev, lambda: _hip.lib().mkb_reg_rows_workspace_bytes(model._tables(), B))


def _entity_rows(sample):
    return sample[:, 0::2].reshape(-1)


class _RegFn(torch.autograd.Function):
    """Forward launches the value only; backward launches the gradient with ``scale`` = the upstream gradient."""

    @staticmethod
    def forward(ctx, ent, rel, reg, model, sample, weight, weight_sum):
        value = torch.empty(1, dtype=torch.float32, device=ent.device)
        reg._call(model, model._tables(ent, rel), None, sample, weight, weight_sum, None, value)
        ctx.reg, ctx.model = reg, model
        ctx.save_for_backward(ent, rel, sample, weight, weight_sum)
        return value.reshape(())

    @staticmethod
    def backward(ctx, dvalue):
        ent, rel, sample, weight, weight_sum = ctx.saved_tensors
        reg, model = ctx.reg, ctx.model

        def buffer(param, table, lam, ids):  # -> (buffer or None, whether autograd gets it back)
            if lam == 0.0:
                return None, False  # (the call neither reads nor writes that table)
            g = _gradshare.direct(param, table, ids)  # a row-lazy optimizer's table: the rows go straight into .grad
            return _gradshare.take(param, table) if g is None else (g, False)

        g_ent, fresh_e = buffer(model.entity_embedding, ent, reg.entity_weight, lambda: _entity_rows(sample))
        g_rel, fresh_r = buffer(model.relation_embedding, rel, reg.relation_weight, lambda: sample[:, 1])
        gr = _hip.Grads(None if g_ent is None else g_ent.data_ptr(), None if g_rel is None else g_rel.data_ptr(), None)
        scale = _hip.contiguous(dvalue, torch.float32).reshape(1)
        reg._call(model, model._tables(ent, rel), gr, sample, weight, weight_sum, scale, None)
        return (g_ent if fresh_e else None), (g_rel if fresh_r else None), None, None, None, None, None


class Lp:
    """``reg = Lp(p, entity_weight, relation_weight)(model, sample, weight=None, weight_sum=None)``: a 0-dim device tensor,
    differentiable with respect to both tables.  ``sample`` [B, 3] int64; ``weight`` [B] (``None``: ones) and ``weight_sum``
    (a device scalar replacing the sum of weights when the rows are a data-parallel shard) as for the losses."""

    def __init__(self, p=3, entity_weight=0.0, relation_weight=0.0):
        if isinstance(p, bool) or p not in (2, 3):
            raise ValueError(f"p must be 2 or 3, not {p!r}")
        for name, v in (("entity_weight", entity_weight), ("relation_weight", relation_weight)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
                raise ValueError(f"{name} must be a finite number >= 0, not {v!r}")
        self.p, self.entity_weight, self.relation_weight = int(p), float(entity_weight), float(relation_weight)

    def __repr__(self):
        return f"{type(self).__name__}(p={self.p}, entity_weight={self.entity_weight}, relation_weight={self.relation_weight})"

    # ------------------------------------------------------------------ the library call
    def _call(self, model, tables, grads, sample, weight, weight_sum, scale, value):
        B = sample.shape[0]
        ws = _workspace(model, B)
        with _hip.on_device(sample.device):
            _hip.check(_hip.lib().mkb_reg_rows(tables, grads, _hip.ptr(sample), _hip.ptr(weight), B, self.p, self.entity_weight,
                                               self.relation_weight, _hip.ptr(weight_sum), _hip.ptr(scale), _hip.ptr(value),
                                               _hip.ptr(ws), ws.numel(), _hip.stream_ptr()), "mkb_reg_rows")

    def _arguments(self, model, sample, weight, weight_sum):
        _hip.require_device(model.entity_embedding, sample, weight, weight_sum)
        if sample.dim() != 2 or sample.shape[1] != 3:
            raise ValueError("sample must be [B, 3]")
        sample = _hip.contiguous(sample, torch.int64)
        if weight is not None:
            weight = _hip.contiguous(weight, torch.float32).reshape(-1)
            if weight.numel() != sample.shape[0]:
                raise ValueError("weight must hold one entry per row of sample")
        if weight_sum is not None:
            weight_sum = _hip.contiguous(weight_sum, torch.float32).reshape(-1)[:1]
        return sample, weight, weight_sum

    def launch(self, model, sample, weight=None, weight_sum=None, grads=None):
        """Value AND gradient in one launch sequence, no autograd (the fused steps): the gradient is added to ``grads`` (a
        ``_hip.Grads``; default: the model's dense ``.grad`` tensors) and the value returned as a 0-dim device tensor.  The
        caller keeps the row-lazy protocol: the batch's heads and tails are current and marked (``begin_step_on``)."""
        sample, weight, weight_sum = self._arguments(model, sample, weight, weight_sum)
        if sample.shape[0] == 0:
            return torch.zeros((), dtype=torch.float32, device=sample.device)
        value = torch.empty(1, dtype=torch.float32, device=sample.device)
        self._call(model, model._tables(), fused.grad_buffers(model) if grads is None else grads, sample, weight, weight_sum, None, value)
        return value.reshape(())

    def __call__(self, model, sample, weight=None, weight_sum=None):
        sample, weight, weight_sum = self._arguments(model, sample, weight, weight_sum)
        if sample.shape[0] == 0:  # an empty batch: no launch; differentiable, backward adds nothing
            return model.entity_embedding.sum() * 0.0
        if _base.VALIDATE_IDS:
            model._launch_id_check(sample, None)
        if _links.owner(model.entity_embedding) is not None or _links.owner(model.relation_embedding) is not None:
            model._make_current(sample, _entity_rows(sample))  # optim.Adam.before_forward: the rows read become current
        return _RegFn.apply(model.entity_embedding, model.relation_embedding, self, model, sample, weight, weight_sum)


class N3(Lp):
    """``Lp(3, weight, weight)``: the nuclear 3-norm penalty ComplEx / DistMult are trained with next to a softmax loss."""

    def __init__(self, weight):
        super().__init__(3, weight, weight)


class L2(Lp):
    """``Lp(2, weight, weight)``: the squared L2 norm of the batch's rows."""

    def __init__(self, weight):
        super().__init__(2, weight, weight)
