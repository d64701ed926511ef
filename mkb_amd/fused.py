"""Pooled (shared-candidate-pool) scoring path and the fused training step.

``pooled_forward``   -- what ``model(sample, negative_sample, mode)`` runs when ``negative_sample`` came from
                        ``mkb_amd.sampling.NegativeSampling`` on the device: ``mkb_pool_score_fwd`` scores every
                        row against the shared pool once, the ``[B, size]`` view is a gather; backward scatters
                        ``d loss / d score`` back onto pool positions and calls ``mkb_pool_score_bwd``.
``FusedTrainStep``   -- one call = lines 211-236 of the reference's compose/pipeline.py (positive forward,
                        negative forward, Adversarial, backward into dense ``.grad``) through ``mkb_pool_step``,
                        bypassing autograd.  Used by ``compose.Pipeline`` when model / sampler / loss are ours.
``PooledLossStep``   -- the same step for ``losses.MarginRanking`` / ``PairwiseLogistic`` / ``CrossEntropy``: the separate
                        pooled entry points around ``mkb_ns_loss``, bypassing autograd.
``OneVsAllStep``     -- the 1vsAll step of ComplEx / DistMult (``losses.OneVsAll``): every entity scored for each row, the softmax
                        over the whole row and the dense backward in one call (``mkb_all_step``); no negatives are drawn.
``KvsAllStep``       -- the KvsAll ("1-N") step of the same two models (``losses.KvsAll``): the same products around the multi-label
                        binary cross entropy with label smoothing (``mkb_all_kvs_step``).
``score_all``        -- the ``[B, n_entity]`` block behind ``model.score_all``, differentiable (``mkb_all_score_fwd`` / ``_bwd``).
``DistanceAllStep``  -- the 1vsAll and KvsAll steps of TransE / RotatE / pRotatE, whose all-entity block is no product: the same loss
                        kernels between the evaluation's forward block and a backward that recomputes the pair terms
                        (``mkb_dist_all_step`` / ``_filtered_step`` / ``_kvs_step``).
``distance_score_all`` -- their differentiable ``[B, n_entity]`` block (``mkb_dist_all_score_fwd`` / ``_bwd``).
"""
import collections

import torch

from . import _gradshare, _hip, _links
from .losses import kvs_all, ns_losses, one_vs_all
from .losses.relation_prediction import relation_table_written
from .sampling.negative_sampling import PoolInfo
from .utils.true_keys import true_keys

__all__ = ["FusedTrainStep", "PooledLossStep", "OneVsAllStep", "KvsAllStep", "DistanceAllStep", "pooled_forward", "pooled_supported", "score_all",
           "distance_score_all"]

_workspaces = {}


def _workspace(model, B, K, slot=0):
    """Device scratch for the pooled kernels, cached per (device, STREAM, table shape, B, K, slot); ``slot`` separates the
    micro-batches of one step, whose forward scratch must survive until their backward half runs.  Per stream: launches on one
    stream use the scratch one after the other, two models of one shape stepped on two streams (the in-process ranks of
    tests/test_gpu_rows_loopback.py; a user training two models side by side) must not share it -- until round 6 they did."""
    dev = model.entity_embedding.device
    key = (dev, _hip.stream_ptr(dev).value, model.name, model.entity_dim, model.n_entity, model.n_relation, B, K, slot)  # (the size depends on the last six)
    return cached_workspace(key, dev, lambda: _hip.lib().mkb_pool_step_workspace_bytes(model._tables(), B, K))


def cached_workspace(key, dev, size):
    """The cache behind ``_workspace``, for any library call whose scratch depends on ``key`` alone (``key[:2]``: device and
    stream; ``size() -> bytes``, asked once per key): the pooled kernels' and the regulariser's (``mkb_amd.regularizers``)."""
    ws = _workspaces.get(key)
    if ws is None:
        n = size()
        guard = _GUARD_BYTES if _guard_on() else 0
        buf = _hip.aligned_bytes(n + guard, dev)
        ws = buf[:n]
        if guard:  # (debug: a pattern behind the workspace that no kernel may touch; check_workspace_guards() looks at it)
            _guards[key] = buf[n:].fill_(_GUARD_VALUE)
        _workspaces[key] = ws
    return ws


_GUARD_BYTES, _GUARD_VALUE = 1 << 16, 0xA5
_guards = {}


def _guard_on():
    import os

    return os.environ.get("MKB_WS_GUARD", "0") == "1"


def check_workspace_guards():
    """MKB_WS_GUARD=1 (tests): every cached workspace is followed by 64 KB of a byte pattern; raise if a kernel wrote there
    (the library takes the workspace as a bare pointer: nothing else would notice an overrun that stays inside the allocator's
    block).  Synchronises."""
    for key, g in _guards.items():
        if not bool((g == _GUARD_VALUE).all().item()):
            bad = int((g != _GUARD_VALUE).nonzero()[0].item())
            raise RuntimeError(f"pooled-kernel workspace overrun: byte {bad} behind the workspace of {key[2:]} was overwritten")


def pooled_supported(model, B, K):
    """True if the pooled kernels cover this table shape / batch (else the general kernels are used)."""
    return bool(_hip.lib().mkb_pool_supported(model._tables(), B, K))


class _PoolScoreFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ent, rel, modulus, model, sample, info, mode):
        B, K = sample.shape[0], info.size
        S = torch.empty((B, 2 * K), dtype=torch.float32, device=ent.device)
        ws = _workspace(model, B, K)
        with _hip.on_device(ent.device):
            _hip.check(_hip.lib().mkb_pool_score_fwd(model._tables(ent, rel, modulus), _hip.ptr(sample), _hip.ptr(info.pool),
                                                     _hip.ptr(info.cnt), B, K, mode, _hip.ptr(S), _hip.ptr(ws),
                                                     _hip.stream_ptr()), "mkb_pool_score_fwd")
        ctx.model, ctx.info, ctx.mode = model, info, mode
        ctx.save_for_backward(ent, rel, modulus, sample)
        return S.gather(1, info.pos.long())

    @staticmethod
    def backward(ctx, dneg):
        ent, rel, modulus, sample = ctx.saved_tensors
        model, info = ctx.model, ctx.info
        B, K = sample.shape[0], info.size
        G = torch.zeros((B, 2 * K), dtype=torch.float32, device=ent.device)
        G.scatter_add_(1, info.pos.long(), _hip.contiguous(dneg, torch.float32))
        # (a row-lazy optimizer's table takes its rows straight into .grad: _gradshare.direct)
        g_ent = _gradshare.direct(model.entity_embedding, ent, lambda: info.rows(sample))
        fresh_e = False
        if g_ent is None:
            g_ent, fresh_e = _gradshare.take(model.entity_embedding, ent)  # (shared with the positive scores' backward of this pass)
        g_rel, fresh_r = _gradshare.take(model.relation_embedding, rel)
        g_mod = torch.zeros_like(modulus) if model.name == "pRotatE" else None
        gr = _hip.Grads(g_ent.data_ptr(), g_rel.data_ptr(), None if g_mod is None else g_mod.data_ptr())
        ws = _workspace(model, B, K)
        with _hip.on_device(ent.device):
            _hip.check(_hip.lib().mkb_pool_score_bwd(model._tables(ent, rel, modulus), gr, _hip.ptr(sample),
                                                     _hip.ptr(info.pool), _hip.ptr(info.cnt), B, K, ctx.mode, _hip.ptr(G),
                                                     _hip.ptr(ws), _hip.stream_ptr()), "mkb_pool_score_bwd")
        return (g_ent if fresh_e else None), (g_rel if fresh_r else None), g_mod, None, None, None, None


def pooled_forward(model, sample, info, mode_id):
    modulus = getattr(model, "modulus", None)
    if modulus is None:
        modulus = model.gamma
    return _PoolScoreFn.apply(model.entity_embedding, model.relation_embedding, modulus, model, sample, info, mode_id)


PoolInfo.enabled = True


def grad_buffers(model):
    """``_hip.Grads`` of ``model``'s dense ``.grad`` tensors (allocated when missing: first step, ``zero_grad(set_to_none=True)``)."""
    params = [model.entity_embedding, model.relation_embedding] + ([model.modulus] if model.name == "pRotatE" else [])
    for p in params:
        if p.grad is None:
            p.grad = torch.zeros_like(p)
    return _hip.Grads(*[p.grad.data_ptr() for p in params])  # (g_modulus stays NULL without a trained modulus)


def sampled_step(step, sample, weight, sampler, mode, **kwargs):
    """``step.sampled(...)``: ``step(sample, weight, sampler.generate(sample, mode), mode, **kwargs)`` with the sampler folded
    into the optimizer's catch-up launch when the entity table of ``step.model`` steps row-lazily (``mkb_amd.optim.Adam(lazy_rows=
    True)``): no sampler launch, identical negatives.  An optimizer whose rows are always current (``rows_always_current``:
    ``mkb_amd.optim.Adagrad``) has no catch-up to fold the sampler into; its own step launch has drawn the pool already, and the
    plain ``generate`` only filters.  The negatives of the call stay available as ``step.negative_sample``."""
    ent = step.model.entity_embedding
    lazy = _links.owner(ent)
    sample = _hip.contiguous(sample, torch.int64)
    # (a sampler without generate_with_catch_up -- sampling.PoolNegativeSampling -- launches on its own; step(...) below catches the
    # row-lazy optimizer up on the rows the batch reads)
    if (lazy is not None and not getattr(lazy, "rows_always_current", False) and sampler.size <= 512 and sample.is_cuda
            and hasattr(sampler, "generate_with_catch_up")):
        neg = sampler.generate_with_catch_up(sample, mode, lazy, ent)
    else:
        neg = sampler.generate(sample=sample, mode=mode)
    step.negative_sample = neg
    return step(sample, weight, neg, mode, **kwargs)


class _PooledStep:
    """What the steps over a shared candidate pool share (``FusedTrainStep``, ``PooledLossStep``): the sampler entry point, the
    opening of a call and the outputs kept for inspection.  A subclass says whether ``weight`` may be None and whether its library
    calls honour ``rows_clear``, makes those calls in ``_launch`` and returns the loss [1]."""

    def sampled(self, sample, weight, sampler, mode, weight_sum=None):
        return sampled_step(self, sample, weight, sampler, mode, weight_sum=weight_sum)

    def __call__(self, sample, weight, negative_sample, mode, weight_sum=None):
        """``weight_sum``: optional device scalar = sum of weights of the WHOLE batch when these rows are one
        data-parallel shard of it (see mkb_amd.parallel); the returned loss is then this shard's share."""
        m = self.model
        info = getattr(negative_sample, "_mkb_pool", None)
        if info is None:
            raise ValueError("negative_sample does not come from mkb_amd.sampling.NegativeSampling.generate")
        mode_id = _hip.mode_id(mode)
        sample = _hip.contiguous(sample, torch.int64)
        weight = None if weight is None and self.weight_optional else _hip.contiguous(weight, torch.float32)
        _hip.require_device(m.entity_embedding, sample, weight)
        B, K = sample.shape[0], info.size
        dev = sample.device
        pos = torch.empty((B, 1), dtype=torch.float32, device=dev)
        S = torch.empty((B, 2 * K), dtype=torch.float32, device=dev)
        ws = _workspace(m, B, K)
        gr = grad_buffers(m)
        if self.relation_prediction is not None:
            relation_table_written(m)  # (the term writes every relation row; in front of anything that writes a gradient row)
        ent = m.entity_embedding
        lazy = _links.owner(ent)
        # row-lazy Adam: the rows read become current, and are marked as written, before anything writes a gradient row
        if lazy is not None and lazy.begin_step_on(ent, info.rows(sample)) and self.may_clear_rows:
            gr.rows_clear = 1
        loss = self._launch(m._tables(), gr, sample, weight, info, B, K, mode_id, weight_sum, pos, S, ws, dev)
        self.positive_score, self._S, self._info = pos, S, info
        return _with_regularizer(self, loss.reshape(()), sample, weight, weight_sum, gr)

    @property
    def negative_score(self):
        return self._S.gather(1, self._info.pos.long())


class FusedTrainStep(_PooledStep):
    """``loss = step(sample, weight, negative_sample, mode)``: fills ``param.grad`` (dense, accumulated) and returns
    the loss as a 0-dim device tensor.  ``positive_score`` [B,1] and ``negative_score`` [B,size] of the last call
    stay available for inspection.

    ``regularizer``: a ``mkb_amd.regularizers.Lp`` (``N3``, ``L2``) whose term on the batch's positive triples joins the step:
    one more library call (``mkb_reg_rows``, value and gradient in one launch sequence) behind ``mkb_pool_step`` -- which may
    STORE the batch's gradient rows (``rows_clear``), so the regulariser adds onto them afterwards.  Its rows are the batch's heads
    and tails, which the row-lazy protocol has already made current and marked.  The loss returned is loss + regulariser;
    ``regularization`` keeps the term alone.

    ``relation_prediction``: a ``losses.RelationPrediction`` whose term on the batch joins the step the same way: one more library
    call (``mkb_rel_step``) behind the step's own calls and behind the regulariser's, adding onto the rows they wrote.  Its entity
    rows are the batch's heads and tails; it writes every relation row (a relation table stepped by rows is flushed first and
    stepped densely).  The loss returned is loss + regulariser + term; ``relation_prediction_loss`` keeps the term alone."""

    def __init__(self, model, alpha, regularizer=None, relation_prediction=None):
        self.model, self.alpha, self.regularizer, self.regularization = model, float(alpha), regularizer, None
        self.relation_prediction, self.relation_prediction_loss = relation_prediction, None

    weight_optional = False  # (mkb_pool_step requires weights)
    may_clear_rows = True  # (mkb_pool_step honours rows_clear: it STORES rows the row-lazy optimizer has just consumed and cleared)

    def _launch(self, tb, gr, sample, weight, info, B, K, mode_id, weight_sum, pos, S, ws, dev):
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        with _hip.on_device(dev):
            _hip.check(_hip.lib().mkb_pool_step(tb, gr, _hip.ptr(sample), _hip.ptr(weight), _hip.ptr(info.pool),
                                                _hip.ptr(info.cnt), B, K, mode_id, self.alpha, _hip.ptr(weight_sum),
                                                _hip.ptr(pos), _hip.ptr(S),
                                                _hip.ptr(loss), _hip.ptr(ws), _hip.stream_ptr()), "mkb_pool_step")
        return loss


def _with_regularizer(step, loss, sample, weight, weight_sum, gr):
    """loss + the step's regulariser term + its relation-prediction term, in that order; their gradients are added to the
    buffers ``gr`` the step has just written."""
    if step.regularizer is not None:
        step.regularization = step.regularizer.launch(step.model, sample, weight, weight_sum, grads=gr)
        loss = loss + step.regularization
    if step.relation_prediction is not None:
        step.relation_prediction_loss = step.relation_prediction.launch(step.model, sample, weight, weight_sum, grads=gr)
        loss = loss + step.relation_prediction_loss
    return loss


class PooledLossStep(_PooledStep):
    """``FusedTrainStep`` for a loss of the ``mkb_ns_loss`` family (``losses.MarginRanking``, ``PairwiseLogistic``, ``CrossEntropy``):
    ``loss = step(sample, weight, negative_sample, mode)`` fills ``param.grad`` (dense, accumulated) and returns the loss as a
    0-dim device tensor; ``positive_score`` [B,1] and ``negative_score`` [B,size] of the last call stay available.

    Five library calls, no autograd: positive scores (``mkb_score_fwd``), pool scores (``mkb_pool_score_fwd``), ``mkb_ns_loss``
    over the ``[B, 2 size]`` pool block with the sampler's multiplicities, then ``mkb_pool_score_bwd`` on its seeds and the
    positive pair's ``mkb_score_bwd``.  Against the explicit autograd sequence this drops the gather of the ``[B, size]`` view,
    the scatter of its gradient back onto pool positions and the dense zero-filled buffers autograd adds into ``.grad``.
    ``regularizer``: as for ``FusedTrainStep`` (a sixth call, ``mkb_reg_rows``, behind the two backward calls);
    ``relation_prediction``: as for ``FusedTrainStep`` (``mkb_rel_step``, behind that)."""

    def __init__(self, model, loss, regularizer=None, relation_prediction=None):
        if getattr(loss, "kind", None) not in (_hip.LOSS_MARGIN, _hip.LOSS_PAIR_LOGISTIC, _hip.LOSS_SOFTMAX):
            raise TypeError("PooledLossStep takes losses.MarginRanking, losses.PairwiseLogistic or losses.CrossEntropy")
        self.model, self.loss, self.regularizer, self.regularization = model, loss, regularizer, None
        self.relation_prediction, self.relation_prediction_loss = relation_prediction, None

    weight_optional = True
    # rows_clear stays 0 whatever the optimizer answers: the promise is only honoured by mkb_pool_step / _bwd, and the two backward
    # calls of _launch both add to the rows of the batch's heads and tails -- they must accumulate.
    may_clear_rows = False

    def _launch(self, tb, gr, sample, weight, info, B, K, mode_id, weight_sum, pos, S, ws, dev):
        m = self.model
        lib, st = _hip.lib(), _hip.stream_ptr(dev)
        with _hip.on_device(dev):
            _hip.check(lib.mkb_score_fwd(tb, _hip.ptr(sample), None, B, 1, _hip.MODE_DEFAULT, _hip.ptr(pos), st), "mkb_score_fwd")
            _hip.check(lib.mkb_pool_score_fwd(tb, _hip.ptr(sample), _hip.ptr(info.pool), _hip.ptr(info.cnt), B, K, mode_id,
                                              _hip.ptr(S), _hip.ptr(ws), st), "mkb_pool_score_fwd")
        loss, dpos, dS = ns_losses.launch(self.loss.kind, pos, S, weight, info.cnt, float(self.loss.param), float(self.loss.alpha),
                                          weight_sum)
        # pRotatE's modulus: one scalar takes every pair's term, and the negatives' total and the positives' total nearly cancel.
        # Each backward call sums its own from zero and the two totals are added once, as autograd does for the explicit
        # sequence; the positives' small terms added one by one onto the negatives' large total lose its low bits.
        parts = [gr, gr]
        if gr.g_modulus:
            mod_parts = torch.zeros((2,) + tuple(m.modulus.shape), dtype=torch.float32, device=dev)
            parts = [_hip.Grads(gr.g_ent, gr.g_rel, mod_parts[k].data_ptr()) for k in range(2)]
        with _hip.on_device(dev):
            _hip.check(lib.mkb_pool_score_bwd(tb, parts[0], _hip.ptr(sample), _hip.ptr(info.pool), _hip.ptr(info.cnt), B, K, mode_id,
                                              _hip.ptr(dS), _hip.ptr(ws), st), "mkb_pool_score_bwd")
            _hip.check(lib.mkb_score_bwd(tb, parts[1], _hip.ptr(sample), None, B, 1, _hip.MODE_DEFAULT, _hip.ptr(dpos), None, st),
                       "mkb_score_bwd")
        if gr.g_modulus:
            m.modulus.grad += mod_parts[0] + mod_parts[1]
        return loss


# ------------------------------------------------------------------------------------- all-entity losses: the two call families
ONE_VS_ALL_MODELS = ("ComplEx", "DistMult")  # the models whose all-entity block is ONE matrix product
DISTANCE_MODELS = ("TransE", "RotatE", "pRotatE")  # the models whose all-entity block is a sum of distances

# One record per family of library calls (csrc/all_host.h has their one protocol): ``prefix + "score_fwd" / "score_bwd" / "step" /
# "filtered_step" / "kvs_step"`` are its calls, ``workspace_symbol`` sizes the scratch they share, ``tag`` keeps the families' cached
# workspaces apart, ``modulus_grad``: its backward fills pRotatE's modulus gradient, ``refusal``: what a step says of another model.
_AllFamily = collections.namedtuple("_AllFamily", "prefix workspace_symbol tag models modulus_grad refusal")
_DOT = _AllFamily("mkb_all_", "mkb_all_step_workspace_bytes", "all", ONE_VS_ALL_MODELS, False,
                  "{step} covers ComplEx and DistMult, whose all-entity block is one matrix product, not {model}: train it with the "
                  "sampled softmax, losses.CrossEntropy, or over all entities with fused.DistanceAllStep")
_DIST = _AllFamily("mkb_dist_all_", "mkb_dist_all_workspace_bytes", "dist_all", DISTANCE_MODELS, True,
                   "{step} covers TransE, RotatE, pRotatE, whose all-entity block is a sum of distances, not {model}: its block is one "
                   "matrix product, use fused.OneVsAllStep / fused.KvsAllStep")


def _family_workspace(fam, model, B):
    """Device scratch of the calls of ``fam`` that take tables, cached like ``_workspace``."""
    dev = model.entity_embedding.device
    key = (dev, _hip.stream_ptr(dev).value, fam.tag, model.name, model.entity_dim, model.n_entity, model.n_relation, B)
    return cached_workspace(key, dev, lambda: getattr(_hip.lib(), fam.workspace_symbol)(model._tables(), B))


def _all_workspace(model, B):
    return _family_workspace(_DOT, model, B)


def _dist_workspace(model, B):
    return _family_workspace(_DIST, model, B)


def _side_keys(triples, model, device, mode_id):
    """The sorted key array of the side ``mode_id`` scores (``utils.true_keys``, built once per triple set)."""
    return true_keys(triples, device, model.n_entity, model.n_relation)["head-batch" if mode_id == _hip.MODE_HEAD else "tail-batch"]


class _ScoreAllFn(torch.autograd.Function):
    """scores [B, n_entity] of every entity in the open slot of ``sample``, for either family (``modulus``: None for the models
    that have none); backward = dense d loss / d tables and pRotatE's d loss / d modulus."""

    @staticmethod
    def forward(ctx, ent, rel, modulus, fam, model, sample, mode):
        B = sample.shape[0]
        scores = torch.empty((B, model.n_entity), dtype=torch.float32, device=ent.device)
        ws = _family_workspace(fam, model, B)
        name = fam.prefix + "score_fwd"
        with _hip.on_device(ent.device):
            _hip.check(getattr(_hip.lib(), name)(model._tables(ent, rel, modulus), _hip.ptr(sample), B, mode, _hip.ptr(scores), _hip.ptr(ws),
                                                 ws.numel(), _hip.stream_ptr()), name)
        ctx.fam, ctx.model, ctx.mode = fam, model, mode
        ctx.save_for_backward(ent, rel, modulus, sample)
        return scores

    @staticmethod
    def backward(ctx, dscore):
        ent, rel, modulus, sample = ctx.saved_tensors
        fam, model, B = ctx.fam, ctx.model, sample.shape[0]
        dscore = _hip.contiguous(dscore, torch.float32)
        g_ent, g_rel = torch.zeros_like(ent), torch.zeros_like(rel)  # every entity row is written: dense, through autograd
        g_mod = torch.zeros_like(modulus) if fam.modulus_grad and model.name == "pRotatE" else None
        ws = _family_workspace(fam, model, B)
        name = fam.prefix + "score_bwd"
        with _hip.on_device(ent.device):
            gr = _hip.Grads(g_ent.data_ptr(), g_rel.data_ptr(), None if g_mod is None else g_mod.data_ptr())
            _hip.check(getattr(_hip.lib(), name)(model._tables(ent, rel, modulus), gr, _hip.ptr(sample), B, ctx.mode, _hip.ptr(dscore),
                                                 dscore.shape[1], _hip.ptr(ws), ws.numel(), _hip.stream_ptr()), name)
        return g_ent, g_rel, g_mod, None, None, None, None


def score_all(model, sample, mode):
    """What ``model.score_all(sample, mode)`` runs (models/base.py checks the arguments and makes row-lazy tables current)."""
    return _ScoreAllFn.apply(model.entity_embedding, model.relation_embedding, None, _DOT, model, sample,
                             _hip.side_id(mode, "1vsAll scores"))


# what a step's one library call is: ``kind`` its suffix ("step" / "filtered_step" / "kvs_step"), the settings that call takes (None:
# not one of its arguments) and whether it reads the key array of ``true_triples``
_AllLoss = collections.namedtuple("_AllLoss", "kind temperature smoothing reduction needs_keys")


class _AllEntityStep:
    """What the steps over the whole entity row share (``OneVsAllStep``, ``KvsAllStep``, ``DistanceAllStep``): the argument checks, the optimizer
    protocol of a step that writes EVERY entity row, the id check, the outputs, the workspace, the one library call and the
    regulariser hook.  A subclass names its ``family`` and describes its loss (``_loss_description() -> _AllLoss``)."""

    family = _DOT  # whose calls the subclass makes

    def __init__(self, model, regularizer=None, relation_prediction=None):
        if model.name not in self.family.models:
            raise NotImplementedError(self.family.refusal.format(step=type(self).__name__, model=model.name))
        self.model, self.regularizer, self.regularization = model, regularizer, None
        self.relation_prediction, self.relation_prediction_loss = relation_prediction, None

    def sampled(self, sample, weight, sampler, mode, weight_sum=None):
        """The other steps' entry point (``compose.Pipeline`` calls it): nothing is drawn from ``sampler``."""
        return self(sample, weight, mode, weight_sum=weight_sum)

    def __call__(self, sample, weight, mode, weight_sum=None):
        m = self.model
        mode_id = _hip.side_id(mode, "1vsAll scores")
        if sample.dim() != 2 or sample.shape[1] != 3 or sample.shape[0] < 1:
            raise ValueError("sample must be [B, 3] with B >= 1")
        if weight is not None and weight.shape != (sample.shape[0],):
            raise ValueError("weight must be [B]")
        sample = _hip.contiguous(sample, torch.int64)
        weight = None if weight is None else _hip.contiguous(weight, torch.float32)
        _hip.require_device(m.entity_embedding, sample, weight)
        B, dev = sample.shape[0], sample.device
        for p in (m.entity_embedding, m.relation_embedding):
            lazy = _links.owner(p)
            if lazy is not None:  # every row is read and written: what is pending is applied, which rows were written is "unknown"
                lazy.before_forward(p, None)
                _links.record(p).wrote = True
        m._launch_id_check(sample, None)
        pos = torch.empty((B, 1), dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        ws = _family_workspace(self.family, m, B)
        gr = grad_buffers(m)
        with _hip.on_device(dev):
            self._launch(m._tables(), gr, sample, weight, B, mode_id, weight_sum, loss, pos, ws)
        self.positive_score = pos
        return _with_regularizer(self, loss.reshape(()), sample, weight, weight_sum, gr)

    def _launch(self, tb, gr, sample, weight, B, mode_id, weight_sum, loss, pos, ws):
        L = self._loss_description()
        keys = _side_keys(self.true_triples, self.model, sample.device, mode_id) if L.needs_keys else None
        labels = (_hip.ptr(keys), 0 if keys is None else keys.numel())
        settings = {"step": (L.temperature,),
                    "filtered_step": labels + (L.temperature, L.smoothing),
                    "kvs_step": labels + (L.smoothing, int(L.reduction == "sum"))}[L.kind]
        name = self.family.prefix + L.kind
        _hip.check(getattr(_hip.lib(), name)(tb, gr, _hip.ptr(sample), _hip.ptr(weight), B, mode_id, *settings, _hip.ptr(weight_sum),
                                             _hip.ptr(loss), _hip.ptr(pos), _hip.ptr(ws), ws.numel(), _hip.stream_ptr()), name)


class OneVsAllStep(_AllEntityStep):
    """``loss = step(sample, weight, mode)``: the 1vsAll softmax step of ComplEx / DistMult.  Every entity is scored for each
    ``(h, r, ?)`` (``'tail-batch'``; ``(?, r, t)`` for ``'head-batch'``) and the cross entropy is taken over the whole row, at
    ``temperature``; fills ``param.grad`` (dense, accumulated) and returns the loss as a 0-dim device tensor.  ``positive_score``
    [B, 1] of the last call stays available.  One library call (``mkb_all_step``), no autograd, no negatives.  ``weight``: [B] or
    None (all ones); ``weight_sum``, ``regularizer`` and ``relation_prediction``: as for ``FusedTrainStep``.

    ``true_triples`` (not None) filters: a row's OTHER known answers in them -- the columns the filtered evaluation leaves out of
    the rank -- are taken out of its softmax and get a gradient of exactly 0; they are read from the sorted key arrays of the
    filtered ranking (``utils.true_keys``, built once), no [B, n_entity] mask exists.  ``label_smoothing`` spreads that much of the
    label over the columns that stay (``losses.OneVsAll`` has the formulas).  With either, the one call is
    ``mkb_all_filtered_step``: the same products around another loss kernel.

    Optimizers: the step writes EVERY entity row.  A row-lazily stepped table (``optim.Adam(lazy_rows=True)``) is flushed first and
    its step then takes the route "touched rows unknown -> dense"; ``optim.Adagrad`` uses its all-rows form."""

    def __init__(self, model, temperature=1.0, regularizer=None, label_smoothing=0.0, true_triples=None, relation_prediction=None):
        super().__init__(model, regularizer, relation_prediction)
        self.temperature = ns_losses._checked("temperature", temperature, positive=True)
        self.label_smoothing = kvs_all.checked_settings(label_smoothing, kvs_all.REDUCTIONS[0])[0]
        self.true_triples = true_triples

    def _loss_description(self):
        filtered = self.true_triples is not None or self.label_smoothing != 0.0
        return _AllLoss("filtered_step" if filtered else "step", self.temperature, self.label_smoothing, None, self.true_triples is not None)


class KvsAllStep(_AllEntityStep):
    """``loss = step(sample, weight, mode)``: the KvsAll ("1-N") step of ComplEx / DistMult.  Every entity is scored for each
    ``(h, r, ?)`` (``'tail-batch'``; ``(?, r, t)`` for ``'head-batch'``) and the binary cross entropy is taken over the whole row
    against the multi-hot labels of ALL the query's known answers in ``true_triples``, smoothed by ``label_smoothing``
    (``losses.KvsAll`` has the formula); fills ``param.grad`` (dense, accumulated) and returns the loss as a 0-dim device tensor.
    ``positive_score`` [B, 1] of the last call stays available.  One library call (``mkb_all_kvs_step``): the labels are read from
    the sorted key arrays of the filtered ranking (``utils.true_keys``, built once), no [B, n_entity] label matrix exists.
    Arguments of the call, optimizers, ``regularizer`` and ``relation_prediction``: as for ``OneVsAllStep``."""

    def __init__(self, model, true_triples, label_smoothing=0.0, reduction="mean", regularizer=None, relation_prediction=None):
        super().__init__(model, regularizer, relation_prediction)
        self.label_smoothing, self.reduction = kvs_all.checked_settings(label_smoothing, reduction)
        if true_triples is None:
            raise ValueError("KvsAllStep needs true_triples: the known triples its labels come from")
        self.true_triples = true_triples

    def _loss_description(self):
        return _AllLoss("kvs_step", None, self.label_smoothing, self.reduction, True)


class DistanceAllStep(_AllEntityStep):
    """``loss = step(sample, weight, mode)``: the all-entity step of TransE / RotatE / pRotatE.  ``loss`` is a ``losses.OneVsAll``
    (the softmax over the whole row at its temperature; with ``filter_known`` or ``label_smoothing`` the filtered form) or a
    ``losses.KvsAll`` (the multi-label binary cross entropy) -- the markers hold every setting, the formulas are theirs.  Every
    entity is scored for each ``(h, r, ?)`` (``'tail-batch'``; ``(?, r, t)`` for ``'head-batch'``); fills ``param.grad`` (dense,
    accumulated; pRotatE: the modulus too) and returns the loss as a 0-dim device tensor.  ``positive_score`` [B, 1] of the last
    call stays available.  One library call (``mkb_dist_all_step`` / ``mkb_dist_all_filtered_step`` / ``mkb_dist_all_kvs_step``), no
    autograd, no negatives.  The score is no product here, so the backward recomputes the pair terms in two passes (DESIGN.md has
    them); arguments of the call, optimizers, ``regularizer`` and ``relation_prediction``: as for ``OneVsAllStep``.

    ``true_triples``: the known triples of a ``KvsAll`` marker, or of a ``OneVsAll(filter_known=True)``, that holds none."""

    family = _DIST

    def __init__(self, model, loss, regularizer=None, true_triples=None, relation_prediction=None):
        if not isinstance(loss, (one_vs_all.OneVsAll, kvs_all.KvsAll)):
            raise TypeError("DistanceAllStep takes losses.OneVsAll or losses.KvsAll")
        super().__init__(model, regularizer, relation_prediction)
        self.loss = loss
        self.true_triples = loss.true_triples if loss.true_triples is not None else true_triples
        self.kvs = isinstance(loss, kvs_all.KvsAll)
        if self.true_triples is None and (self.kvs or loss.filter_known):
            raise ValueError("DistanceAllStep needs true_triples: the known triples the loss labels or filters by")
        self.filtered = not self.kvs and (loss.filter_known or loss.label_smoothing != 0.0)

    def _loss_description(self):
        L = self.loss
        if self.kvs:
            return _AllLoss("kvs_step", None, L.label_smoothing, L.reduction, True)
        return _AllLoss("filtered_step" if self.filtered else "step", L.temperature, L.label_smoothing, None, L.filter_known)


def distance_score_all(model, sample, mode):
    """float32 ``[B, n_entity]``: what ``model.score_all(sample, mode)`` is for ComplEx / DistMult, for TransE / RotatE / pRotatE --
    ``out[i, e]`` is the score of ``sample[i]`` with its tail (``'tail-batch'``; its head for ``'head-batch'``) replaced by entity
    ``e``, the bits ``Evaluation.ranks(..., with_scores=True)`` hands out, differentiable with respect to both tables and pRotatE's
    modulus: ``losses.OneVsAll()(fused.distance_score_all(m, sample, mode), target, weight)`` trains the explicit way."""
    from .models import base

    if model.name not in DISTANCE_MODELS:
        raise NotImplementedError(f"distance_score_all covers {', '.join(DISTANCE_MODELS)}, not {model.name}: use model.score_all")
    mode_id = _hip.side_id(mode, "all-entity scores")
    _hip.require_device(model.entity_embedding, sample)
    if sample.dim() != 2 or sample.shape[1] != 3 or sample.shape[0] < 1:
        raise ValueError("sample must be [B, 3] with B >= 1")
    sample = _hip.contiguous(sample, torch.int64)
    if base.VALIDATE_IDS:
        model._launch_id_check(sample, None)
    if _links.owner(model.entity_embedding) is not None or _links.owner(model.relation_embedding) is not None:
        model._make_current(sample, None)  # every entity row is read
    return _ScoreAllFn.apply(model.entity_embedding, model.relation_embedding, getattr(model, "modulus", None), _DIST, model, sample,
                             mode_id)
