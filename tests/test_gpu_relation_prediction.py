"""-m gpu: the relation-prediction term on the device (mkb_rel_step / mkb_rel_score_bwd, mkb_amd/csrc/rel_step.hip;
losses.RelationPrediction, model.score_relations) against the float64 replica of tests/util_relation_prediction.py, whose module
docstring has the tolerance scheme: through ``term.launch`` at every shape of the case table, as the differentiable block, through
autograd, inside each of the five steps and under the two row-wise optimizers.  Every test prints its ratios before it asserts."""
import numpy as np
import pytest
import torch

import util_relation_prediction as up
from util_gpu import make_model

pytestmark = pytest.mark.gpu

VARIANTS = {"weighted": dict(weighted=True), "unweighted": dict(weighted=False), "weight_sum": dict(weighted=True, weight_sum=61.5)}


def _bytes(d):
    return {k: None if v is None else np.asarray(v).tobytes() for k, v in d.items()}


@pytest.mark.parametrize("case", up.CASES, ids=up.CASE_IDS)
def test_launch_against_float64(case):
    """``term.launch`` (one mkb_rel_step) at T = 0.5, lambda = 0.25, weighted, unweighted and with the caller's weight sum: loss, pos
    and the three gradients against float64; pos is ``model(sample)`` bit for bit; two runs give the same bytes; R = 1 gives a value
    of exactly 0."""
    pb = up.problem(case)
    sample = torch.as_tensor(pb.sample).cuda()
    for what, kw in VARIANTS.items():
        f64, yard = up.expected(pb, (case, what), **kw)
        got = up.device_launch(pb, **kw)
        up.check(pb, got, f64, yard, "launch " + what)
        if pb.R == 1:
            assert float(got["loss"]) == 0.0
    again = up.device_launch(pb, **VARIANTS["weight_sum"])
    assert _bytes(again) == _bytes(got)
    with torch.no_grad():
        direct = up.device_model(pb)(sample).reshape(-1)
    assert np.array_equal(got["pos"].view(np.uint32), direct.cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("case", up.CASES, ids=up.CASE_IDS)
def test_block_and_seeds(case):
    """``model.score_relations`` is ``utils.relation_scores`` bit for bit; the block and lambda x the softmax's seeds against
    float64; the explicit sequence's value and pos have the bits of ``launch``."""
    from mkb_amd import utils

    pb = up.problem(case)
    f64, yard = up.expected(pb, (case, "weighted"), **VARIANTS["weighted"])
    got = up.device_block(pb)
    up.check(pb, got, f64, yard, "block")
    m = up.device_model(pb)
    block = utils.relation_scores(m, torch.as_tensor(pb.sample).cuda())
    assert np.array_equal(got["S"].view(np.uint32), block.cpu().numpy().view(np.uint32))
    launched = up.device_launch(pb)
    assert _bytes({k: got[k] for k in ("loss", "pos")}) == _bytes({k: launched[k] for k in ("loss", "pos")})


@pytest.mark.parametrize("case", up.CASES, ids=up.CASE_IDS)
def test_score_relations_backward(case):
    """``score_relations(sample).backward(dblock)`` with a random seed block against the replica's backward of the block."""
    pb = up.problem(case)
    dblock = up.seed_block(pb)
    f64, yard = up.expected(pb, (case, "dblock"), dblock=dblock)
    m = up.device_model(pb)
    S = m.score_relations(torch.as_tensor(pb.sample).cuda())
    assert S.shape == (pb.B, pb.R) and S.requires_grad
    S.backward(torch.as_tensor(dblock).cuda())
    torch.cuda.synchronize()
    up.check(pb, dict(up.grads_of(m, pb), S=S.detach().cpu().numpy()), f64, yard, "score_relations backward")


@pytest.mark.parametrize("case", up.CASES, ids=up.CASE_IDS)
def test_autograd_is_launch_bit_for_bit(case):
    """``term(model, sample, weight).backward()`` against ``launch`` on zeroed buffers: value and every gradient, bit for bit."""
    pb = up.problem(case)
    for weighted in (False, True):
        launched = up.device_launch(pb, weighted=weighted)
        m = up.device_model(pb)
        w = torch.tensor(pb.weight).cuda() if weighted else None
        value = up.term_of()(m, torch.as_tensor(pb.sample).cuda(), w)
        assert value.dim() == 0 and value.requires_grad
        value.backward()
        torch.cuda.synchronize()
        got = dict(up.grads_of(m, pb), loss=value.detach().cpu().numpy())
        for q, v in got.items():
            if v is not None:
                assert np.array_equal(np.asarray(v).reshape(-1), np.asarray(launched[q]).reshape(-1)), (q, weighted)


@pytest.mark.parametrize("case", up.CASES, ids=up.CASE_IDS)
def test_prefilled_buffers_and_rows_outside_the_batch(case):
    """Gradient buffers that held random values end within tolerance of prefill + gradient; entity rows that are neither a head nor
    a tail of the batch keep their bytes; with R = 1 every buffer is bit-unchanged."""
    pb = up.problem(case)
    pre = up.prefill(pb)
    f64, yard = up.expected(pb, (case, "prefill"), pre=pre, **VARIANTS["weighted"])
    got = up.device_launch(pb, pre=pre)
    up.check(pb, got, f64, yard, "prefilled")
    outside = np.setdiff1d(np.arange(up.N), np.concatenate([pb.sample[:, 0], pb.sample[:, 2]]))
    assert got["g_ent"][outside].tobytes() == pre[0][outside].tobytes()
    if len(outside) < up.N:
        inside = np.setdiff1d(np.arange(up.N), outside)
        assert pb.R == 1 or got["g_ent"][inside].tobytes() != pre[0][inside].tobytes()
    if pb.R == 1:
        assert got["g_ent"].tobytes() == pre[0].tobytes() and got["g_rel"].tobytes() == pre[1].tobytes()
        assert got["g_mod"] is None or got["g_mod"].tobytes() == pre[2].tobytes()


def test_entity_rows_beyond_the_slot_kernels_limit_are_refused():
    from mkb_amd import _hip

    ent, rel = np.zeros((3, 2800), dtype=np.float32), np.zeros((2, 2800), dtype=np.float32)
    m = make_model("TransE", ent, rel, 2800, 6.0)
    with pytest.raises(_hip.HipLibraryError, match="status -5"):
        up.term_of().launch(m, torch.tensor([[0, 1, 2]]).cuda())


# ---------------------------------------------------------------------------------------------------- the five steps
N_ENT, N_REL, HIDDEN, BATCH, SIZE = 4200, 5, 20, 37, 16  # (4096 rows and more step row-lazily)


def _problem(name, seed=11):
    from mkb_amd import sampling

    g = torch.Generator().manual_seed(seed)
    de, dr = up.dims(name, HIDDEN)
    ent = (torch.rand(N_ENT, de, generator=g) * 2 - 1) * 0.4
    rel = (torch.rand(N_REL, dr, generator=g) * 2 - 1) * 0.4
    rs = np.random.RandomState(seed)
    train = np.unique(np.stack([rs.randint(N_ENT, size=900), rs.randint(N_REL, size=900), rs.randint(N_ENT, size=900)], 1), axis=0)
    rs.shuffle(train)
    ents, rels = {i: i for i in range(N_ENT)}, {i: i for i in range(N_REL)}
    w = (torch.rand(BATCH, generator=g) + 0.5).cuda()
    triples = [tuple(int(x) for x in t) for t in train]

    def sampler():
        return sampling.NegativeSampling(size=SIZE, train_triples=triples, entities=ents, relations=rels, seed=3)

    def model():
        return make_model(name, ent, rel, HIDDEN, 6.0, torch.tensor([[0.1]]))

    return model, sampler, torch.as_tensor(train).cuda(), w, triples


STEPS = [("fused", "RotatE"), ("fused", "pRotatE"), ("pooled", "ComplEx"), ("onevsall", "DistMult"), ("kvsall", "ComplEx"),
         ("distance", "TransE"), ("distance", "pRotatE")]


def _step_of(kind, m, term, triples):
    from mkb_amd import fused, losses

    if kind == "fused":
        return fused.FusedTrainStep(m, 0.5, relation_prediction=term)
    if kind == "pooled":
        return fused.PooledLossStep(m, losses.CrossEntropy(), relation_prediction=term)
    if kind == "onevsall":
        return fused.OneVsAllStep(m, 0.5, relation_prediction=term)
    if kind == "kvsall":
        return fused.KvsAllStep(m, triples, 0.1, relation_prediction=term)
    return fused.DistanceAllStep(m, losses.OneVsAll(0.5), relation_prediction=term)


@pytest.mark.parametrize("kind,name", STEPS, ids=[f"{k}-{n}" for k, n in STEPS])
def test_steps_add_the_term(kind, name):
    """One step with ``relation_prediction=`` against the same step without it plus ``term.launch`` on fresh buffers.  The term's
    value is that launch's bit for bit (the same call), so what is left between the two sides is the step's own run-to-run
    difference -- the pooled steps add gradient rows with float atomics: the project's bound for two such runs, grad_close's
    min(1e-5, 2e-4 max|g|); the all-entity steps have none -- plus one rounding of the sum, 2^-24 of its largest entry.  The loss:
    1e-5 absolute and relative, the bound of the step comparisons in tests/test_gpu_regularizers.py."""
    from mkb_amd import _hip

    model, sampler, train, w, triples = _problem(name)
    sample = train[:BATCH].contiguous()
    term = up.term_of()
    out = []
    for t in (None, term):
        m = model()
        step = _step_of(kind, m, t, triples)
        if kind in ("fused", "pooled"):
            loss = step(sample, w, sampler().generate(sample, "head-batch"), "head-batch")
        else:
            loss = step(sample, w, "head-batch")
        torch.cuda.synchronize()
        mod = m.modulus.grad.cpu().numpy().copy() if name == "pRotatE" else None
        out.append((float(loss), m.entity_embedding.grad.cpu().numpy().copy(), m.relation_embedding.grad.cpu().numpy().copy(), mod, step))
    m = model()
    bufs = [torch.zeros_like(p) for p in (m.entity_embedding, m.relation_embedding)] + ([torch.zeros_like(m.modulus)] if name == "pRotatE" else [])
    value = term.launch(m, sample, w, grads=_hip.Grads(*[b.data_ptr() for b in bufs]))
    torch.cuda.synchronize()
    assert out[0][4].relation_prediction_loss is None and out[0][4].relation_prediction is None
    assert float(out[1][4].relation_prediction_loss) == float(value) and float(value) > 1e-3
    want = out[0][0] + float(value)
    assert abs(out[1][0] - want) <= 1e-5 + 1e-5 * abs(want)
    for k, buf in enumerate(bufs):
        t = buf.cpu().numpy().astype(np.float64)
        total = out[0][1 + k].astype(np.float64) + t
        atol = min(1e-5, 2e-4 * float(np.abs(total).max())) + 2.0 ** -24 * float(np.abs(total).max())
        print(f"{kind}-{name} buffer {k}: max |d| {np.abs(out[1][1 + k] - total).max():.3g} of {atol:.3g}")
        assert np.abs(t).max() > 0
        np.testing.assert_allclose(out[1][1 + k], total, rtol=0, atol=atol)


def test_fused_step_under_a_deferring_row_lazy_optimizer():
    """Five FusedTrainStep steps under ``optim.Adam(lazy_rows=True, defer_step=True)``, where ``mkb_pool_step`` STORES gradient rows
    from the third step on: the step with the term against the step without it followed by ``term.launch`` into .grad.  The same
    calls in the same order on the same buffers; the tables after the flush to atol 2e-6, the bound of tests/test_gpu_defer.py's
    comparison of two fused runs (float atomics in the step's kernels).  The entity table is still stepped row-lazily."""
    from mkb_amd import _links, fused, optim

    term = up.term_of()

    def run(joined):
        model, sampler, train, w, _ = _problem("ComplEx", seed=17)
        m, ns = model(), sampler()
        opt = optim.Adam([m.entity_embedding, m.relation_embedding], lr=1e-3, lazy_rows=True, defer_step=True)
        step = fused.FusedTrainStep(m, 0.5, relation_prediction=term if joined else None)
        values = []
        for it in range(5):
            s = train[it * BATCH:(it + 1) * BATCH].contiguous()
            loss = step.sampled(s, w, ns, "head-batch" if it % 2 else "tail-batch")
            if not joined:
                loss = loss + term.launch(m, s, w)
            values.append(float(loss))
            opt.step()
            opt.zero_grad()
        assert "last" in opt.state[m.entity_embedding] and _links.owner(m.entity_embedding) is opt
        opt.flush()
        torch.cuda.synchronize()
        return m.entity_embedding.detach().cpu().numpy(), m.relation_embedding.detach().cpu().numpy(), values

    a, b = run(True), run(False)
    np.testing.assert_allclose(a[2], b[2], rtol=1e-5, atol=1e-5)
    for x, y in zip(a[:2], b[:2]):
        print("deferred: max |d| %.3g" % np.abs(x - y).max())
        np.testing.assert_allclose(x, y, rtol=0, atol=2e-6)


# ---------------------------------------------------------------------------------------------------- optimizers
TRAIN_STEPS = 3
# Both optimizers divide a gradient by (a root of its squares + eps): at their default eps (1e-8, 1e-10) an element whose gradient
# all but cancels (|g| of the order of its own rounding error) steps by a full lr in a direction that rounding decides, in float32
# torch and on the device alike but not alike in both, and err_ref would measure that one element.  The gradients here are ~1e-3.
OPT_EPS = 1e-4


def _torch_training(name, ent, rel, batches, w, opt_name, lr, dtype):
    """TRAIN_STEPS steps of the term alone on dense torch tables in ``dtype`` (CPU) -> the two tables as float64 numpy."""
    e = torch.tensor(ent, dtype=dtype, requires_grad=True)
    r = torch.tensor(rel, dtype=dtype, requires_grad=True)
    mod = torch.tensor([[0.1]], dtype=dtype)
    opt = (torch.optim.Adam if opt_name == "adam" else torch.optim.Adagrad)([e, r], lr=lr, eps=OPT_EPS)
    kd = up.phase_div(6.0, HIDDEN)
    for s in batches:
        opt.zero_grad()
        S, _ = up.score_block(name, e, r, mod, s, 6.0, kd)
        row = torch.logsumexp(S / up.T, 1) - S[torch.arange(len(s)), s[:, 1]] / up.T
        (up.LAMBDA * (w.to(dtype) * row).sum() / w.to(dtype).sum()).backward()
        opt.step()
    return e.detach().double().numpy(), r.detach().double().numpy()


@pytest.mark.parametrize("opt_name", ["adam", "adagrad"])
@pytest.mark.parametrize("name", ["ComplEx", "RotatE"])
def test_training_steps_under_the_row_wise_optimizers(name, opt_name):
    """Three training steps of ``term(model, sample, weight).backward()`` under ``optim.Adam(lazy_rows=True)`` and ``optim.Adagrad``
    against the same steps of dense torch in float64.  err_ref of a table: the same steps of dense torch in float32 against float64,
    never below 4 float32 ulps of the table's largest entry; the device is held to steps x ERR_FACTOR x err_ref.  (The two smooth
    models: a step moves TransE's and pRotatE's tables across kinks that the case table's seeds were chosen to avoid.)  The entity
    table is still stepped by rows afterwards: no dense zero-filled table went through autograd."""
    from mkb_amd import _links, optim

    model, _, train, w, _ = _problem(name, seed=19)
    m = model()
    ent0, rel0 = m.entity_embedding.detach().cpu().numpy().copy(), m.relation_embedding.detach().cpu().numpy().copy()
    lr = 1e-2 if opt_name == "adam" else 0.1
    params = [m.entity_embedding, m.relation_embedding]
    opt = optim.Adam(params, lr=lr, eps=OPT_EPS, lazy_rows=True) if opt_name == "adam" else optim.Adagrad(params, lr=lr, eps=OPT_EPS)
    term = up.term_of()
    batches = [train[it * BATCH:(it + 1) * BATCH].contiguous() for it in range(TRAIN_STEPS)]
    for s in batches:
        opt.zero_grad()
        term(m, s, w).backward()
        opt.step()
    ent = m.entity_embedding
    assert "last" in opt.state[ent] and _links.owner(ent) is opt, "the optimizer fell back to the dense kernel"
    assert not _links.autograd_wrote(ent)
    opt.flush()
    torch.cuda.synchronize()
    got = (ent.detach().cpu().numpy(), m.relation_embedding.detach().cpu().numpy())
    cpu = [b.cpu() for b in batches]
    f64 = _torch_training(name, ent0, rel0, cpu, w.cpu(), opt_name, lr, torch.float64)
    f32 = _torch_training(name, ent0, rel0, cpu, w.cpu(), opt_name, lr, torch.float32)
    assert np.abs(f64[0] - ent0).max() > 0.5 * lr  # the steps moved the table
    for what, g, a, b in zip(("entity", "relation"), got, f64, f32):
        err_ref = max(float(np.abs(b - a).max()), up.FLOOR_ULPS * 2.0 ** -24 * float(np.abs(a).max()))
        err = float(np.abs(g - a).max())
        print(f"{name} {opt_name} {what} table after {TRAIN_STEPS} steps: error {err:.3g}, err_ref {err_ref:.3g}, ratio {err / err_ref:.2f}")
        assert err <= TRAIN_STEPS * up.ERR_FACTOR * err_ref
