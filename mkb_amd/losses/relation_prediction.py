"""``RelationPrediction`` -- relation prediction as an auxiliary training term (Chen et al., AKBC 2021; no reference counterpart).
Next to the entity losses every batch also minimises ``-log P(r | h, t)`` over ALL relations:

    S_ij  = score(h_i, j, t_i)  for j < n_relation   (the default-mode score of the model, any of the five)
    row_i = logsumexp_j (S_ij / T) - S_{i, r_i} / T
    term  = weight * sum_i w_i row_i / W             (w: the batch's weights or ones; W: their sum, or the caller's weight_sum)

    term = losses.RelationPrediction(0.25)
    error = loss(positive_score, negative_score, weight) + term(model, sample, weight)
    error.backward()

It has the two entry points of the regularisers (``mkb_amd.regularizers.Lp``), and every step takes it the way it takes one:

``term(model, sample, weight=None, weight_sum=None)`` -- a 0-dim device tensor, differentiable in both tables and pRotatE's
modulus.  Forward scores the block (``mkb_rel_scores``) and runs the softmax on it (``mkb_all_softmax``); backward hands
``weight`` times its seeds to ``mkb_rel_score_bwd``, which writes the gradient rows of the batch's heads and tails and every row of
the relation table -- no dense zero-filled entity table goes through autograd, and a table stepped by a row-lazy optimizer takes
its rows straight into ``.grad`` (``_gradshare.direct``), reported exactly as ``model(...)`` reports them.

``term.launch(model, sample, weight, weight_sum, grads=None)`` -- value AND gradient in the one ``mkb_rel_step`` call, no autograd:
what ``fused.FusedTrainStep`` / ``PooledLossStep`` / ``OneVsAllStep`` / ``KvsAllStep`` / ``DistanceAllStep`` run behind their own
calls when they are given ``relation_prediction=term``; ``compose.Pipeline`` takes it as its ``relation_prediction`` attribute.
Both give the same bits.

Not covered: the sharded steps (``mkb_amd.parallel``, ``mkb_amd.table_rows``), filtering a pair's OTHER known relations out of
the softmax, and label smoothing on it.
"""
import torch

from .. import _gradshare, _hip, _links
from ..models import base as _base
from . import one_vs_all
from .ns_losses import _checked

__all__ = ["RelationPrediction"]


def _workspace(model, B):
    """Scratch of ``mkb_rel_step`` / ``mkb_rel_score_bwd``, cached like the pooled kernels' (``fused.cached_workspace``)."""
    from .. import fused

    dev = model.entity_embedding.device
    key = (dev, _hip.stream_ptr(dev).value, "rel_step", model.name, model.entity_dim, model.n_entity, model.n_relation, B)
    return fused.cached_workspace(key, dev, lambda: _hip.lib().mkb_rel_step_workspace_bytes(model._tables(), B))


def relation_table_written(model):
    """The term writes EVERY relation row: a relation table an optimizer steps by rows is handled as ``fused._AllEntityStep``
    handles its tables -- what is pending is applied, which rows were written is "unknown".  In front of anything that writes a
    gradient row."""
    p = model.relation_embedding
    lazy = _links.owner(p)
    if lazy is not None:
        lazy.before_forward(p, None)
        _links.record(p).wrote = True


def _entity_rows(sample):
    return sample[:, 0::2].reshape(-1)


def score_bwd(model, tables, grads, sample, dscore):
    """One ``mkb_rel_score_bwd`` call: ``dscore`` [B, ld] contiguous float32 -> added to ``grads``."""
    B = sample.shape[0]
    ws = _workspace(model, B)
    with _hip.on_device(sample.device):
        _hip.check(_hip.lib().mkb_rel_score_bwd(tables, grads, _hip.ptr(sample), B, _hip.ptr(dscore), dscore.shape[1], _hip.ptr(ws),
                                                ws.numel(), _hip.stream_ptr()), "mkb_rel_score_bwd")


def _grad_targets(model, ent, rel, modulus, sample):
    """Where a backward of the block adds: ``(Grads, what autograd gets back for ent, rel, modulus)``.  The entity table of a
    row-lazy optimizer takes the batch's rows straight into ``.grad``; the relation table is written in full, so it goes through
    autograd as a dense buffer like any dense gradient."""
    g_ent = _gradshare.direct(model.entity_embedding, ent, lambda: _entity_rows(sample))
    fresh_e = False
    if g_ent is None:
        g_ent, fresh_e = _gradshare.take(model.entity_embedding, ent)
    g_rel, _ = _gradshare.take(model.relation_embedding, rel)
    g_mod = torch.zeros_like(modulus) if model.name == "pRotatE" else None
    gr = _hip.Grads(g_ent.data_ptr(), g_rel.data_ptr(), None if g_mod is None else g_mod.data_ptr())
    return gr, (g_ent if fresh_e else None), g_rel, g_mod


class RelationScoresFn(torch.autograd.Function):
    """The block [B, n_relation] of ``model.score_relations``: forward ``mkb_rel_scores``, backward ``mkb_rel_score_bwd``."""

    @staticmethod
    def forward(ctx, ent, rel, modulus, model, sample):
        B = sample.shape[0]
        S = torch.empty((B, model.n_relation), dtype=torch.float32, device=ent.device)
        with _hip.on_device(ent.device):
            _hip.check(_hip.lib().mkb_rel_scores(model._tables(ent, rel, modulus), _hip.ptr(sample), B, None, model.n_relation,
                                                 _hip.ptr(S), model.n_relation, _hip.stream_ptr()), "mkb_rel_scores")
        ctx.model = model
        ctx.save_for_backward(ent, rel, modulus, sample)
        return S

    @staticmethod
    def backward(ctx, dscore):
        ent, rel, modulus, sample = ctx.saved_tensors
        model = ctx.model
        gr, out_e, out_r, g_mod = _grad_targets(model, ent, rel, modulus, sample)
        score_bwd(model, model._tables(ent, rel, modulus), gr, sample, _hip.contiguous(dscore, torch.float32))
        return out_e, out_r, g_mod, None, None


class _TermFn(torch.autograd.Function):
    """Forward: the block and the softmax on it (value and seeds); backward: upstream * weight * seeds -> ``mkb_rel_score_bwd``."""

    @staticmethod
    def forward(ctx, ent, rel, modulus, term, model, sample, weight, weight_sum):
        value, _, seeds = term.block_seeds(model, sample, weight, weight_sum, model._tables(ent, rel, modulus))
        ctx.term, ctx.model = term, model
        ctx.save_for_backward(ent, rel, modulus, sample, seeds)
        return value

    @staticmethod
    def backward(ctx, dvalue):
        ent, rel, modulus, sample, seeds = ctx.saved_tensors
        model = ctx.model
        gr, out_e, out_r, g_mod = _grad_targets(model, ent, rel, modulus, sample)
        dscore = (_hip.contiguous(dvalue, torch.float32) * ctx.term._scale(seeds.device)) * seeds
        score_bwd(model, model._tables(ent, rel, modulus), gr, sample, dscore)
        return out_e, out_r, g_mod, None, None, None, None, None


class RelationPrediction:
    kind = None  # (not one of mkb_ns_loss's kinds: it is a term next to a loss, not a loss of scores)

    def __init__(self, weight=1.0, temperature=1.0):
        self.weight = _checked("weight", weight, positive=True)
        self.temperature = _checked("temperature", temperature, positive=True)

    def __repr__(self):
        return f"RelationPrediction(weight={self.weight}, temperature={self.temperature})"

    def _scale(self, device):
        return torch.tensor(self.weight, dtype=torch.float32, device=device)

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

    # ------------------------------------------------------------------ the explicit sequence's forward half
    def block_seeds(self, model, sample, weight=None, weight_sum=None, tables=None):
        """-> (value 0-dim, pos [B], seeds [B, n_relation]) on checked arguments: ``mkb_rel_scores``, then ``mkb_all_softmax`` in
        place.  ``weight * seeds`` is d term / d block; value and pos have the bits ``launch`` gives."""
        B, R = sample.shape[0], model.n_relation
        S = torch.empty((B, R), dtype=torch.float32, device=sample.device)
        with _hip.on_device(sample.device):
            _hip.check(_hip.lib().mkb_rel_scores(model._tables() if tables is None else tables, _hip.ptr(sample), B, None, R, _hip.ptr(S), R,
                                                 _hip.stream_ptr()), "mkb_rel_scores")
        loss, pos = one_vs_all.launch(S, R, sample[:, 1], 3, weight, weight_sum, float(self.temperature))
        return (loss * self._scale(sample.device)).reshape(()), pos, S

    # ------------------------------------------------------------------ the two entry points
    def launch(self, model, sample, weight=None, weight_sum=None, grads=None):
        """Value AND gradient in one ``mkb_rel_step`` call, no autograd (the fused steps): the gradient is added to ``grads`` (a
        ``_hip.Grads``; default: the model's dense ``.grad`` tensors) and the value returned as a 0-dim device tensor;
        ``positive_score`` [B] keeps the block's target column, the bits of ``model(sample)``.  The caller keeps the row-lazy
        protocol of the entity table: the batch's heads and tails are current and marked (``begin_step_on``)."""
        from .. import fused

        sample, weight, weight_sum = self._arguments(model, sample, weight, weight_sum)
        B, dev = sample.shape[0], sample.device
        if B == 0:
            return torch.zeros((), dtype=torch.float32, device=dev)
        relation_table_written(model)
        gr = fused.grad_buffers(model) if grads is None else grads
        value, pos = torch.empty(1, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.float32, device=dev)
        ws = _workspace(model, B)
        with _hip.on_device(dev):
            _hip.check(_hip.lib().mkb_rel_step(model._tables(), gr, _hip.ptr(sample), _hip.ptr(weight), B, float(self.temperature),
                                               float(self.weight), _hip.ptr(weight_sum), _hip.ptr(value), _hip.ptr(pos), _hip.ptr(ws),
                                               ws.numel(), _hip.stream_ptr()), "mkb_rel_step")
        self.positive_score = pos
        return value.reshape(())

    def __call__(self, model, sample, weight=None, weight_sum=None):
        sample, weight, weight_sum = self._arguments(model, sample, weight, weight_sum)
        if sample.shape[0] == 0:  # an empty batch: no launch; differentiable, backward adds nothing
            return model.entity_embedding.sum() * 0.0
        if _base.VALIDATE_IDS:
            model._launch_id_check(sample, None)
        if _links.owner(model.entity_embedding) is not None or _links.owner(model.relation_embedding) is not None:
            model._make_current(sample, _entity_rows(sample), None)  # the batch's heads and tails; every relation row is read
        return _TermFn.apply(model.entity_embedding, model.relation_embedding, _base._modulus_slot(model), self, model, sample, weight,
                             weight_sum)
