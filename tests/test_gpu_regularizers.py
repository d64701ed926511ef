"""-m gpu: the embedding regularisers on the device (mkb_reg_rows, mkb_amd/csrc/reg_rows.hip; mkb_amd.regularizers) against the
float64 reference of tests/util_regularizers.py: through the C ABI at the shapes where the kernel can go wrong, through autograd
next to ``model(...)`` (with torch.optim.Adam and under the row-lazy optimizer, which must stay row-lazy), inside the two fused
steps, and as compose.Pipeline's ``regularizer``."""
import math

import numpy as np
import pytest
import torch

import util_regularizers as ur
from util_gpu import grad_close, make_model

pytestmark = pytest.mark.gpu

MODELS = ["TransE", "RotatE", "ComplEx", "DistMult", "pRotatE"]


def value_bound(D, B, run):
    """Relative bound on the value: every term is non-negative, so the relative error of each sum is at most (the roundings on
    the longest path from an input to the result) x 2^-24, to first order.  The path, as reg_rows.hip sums:
      6   one entry's term (paired, p = 3: re^2, im^2, their sum, the square root counted twice, m^2 * m)
      ceil(D / 256) + 2   a lane's serial chain over its entries of the row (the 16-byte form: a quarter of it, plus two levels
                          inside a group of four)
      9   block_sum_256: six butterfly levels, then four wave totals left to right
      ceil(run / 256) + 9 + 1   the run's weights: lane chain, the same tree, the division by W
      ceil(B / 256) + 9   W, reduced from the weights by the same tree
      2   lambda * c * s
      ceil(3 B / 256) + 9   the final pass over the 3 B slots
    capped at the project's 1e-4 parity bound."""
    c = lambda a, b: -(-a // b)  # noqa: E731
    ops = 6 + (c(D, 256) + 2) + 9 + (c(run, 256) + 10) + (c(B, 256) + 9) + 2 + (c(3 * B, 256) + 9)
    return min(1e-4, ops * 2.0 ** -24)


def _tables(name, N, R, hidden, seed):
    g = torch.Generator().manual_seed(seed)
    de, dr = ur.DIMS[name]
    ent = (torch.rand(N, de * hidden, generator=g) * 2 - 1) * 0.8
    rel = (torch.rand(R, dr * hidden, generator=g) * 2 - 1) * 0.8
    return ent, rel


def _sample(N, R, B, g):
    return torch.stack([torch.randint(N, (B,), generator=g), torch.randint(R, (B,), generator=g), torch.randint(N, (B,), generator=g)], 1)


# (what, N, R, hidden per model or one for all, B, weight, weight_sum, scale)
def _cases(name):
    wide = 2000 // ur.DIMS[name][0]  # entity_dim = 2000: the long-row loop (two strides of the 16-byte form)
    return [
        ("hidden 1", 7, 2, 1, 5, False, None, None),
        ("hidden 3, h == t", 11, 3, 3, 9, True, None, None),
        ("hidden 5, weight_sum and scale", 9, 2, 5, 33, True, 7.25, -1.75),
        ("hidden 66", 50, 4, 66, 70, True, None, 0.5),
        ("hidden 8, weight_sum only", 20, 3, 8, 17, False, 40.0, None),
        ("entity_dim 2000", 40, 5, wide, 64, True, None, None),
        ("B = 1", 5, 2, 12, 1, True, None, 2.0),
        ("runs of hundreds", 7, 1, 8, 1500, True, None, None),
        ("every triple the same", 6, 2, 4, 40, True, None, None),
    ]


def _call(name, ent, rel, hidden, sample, p, le, lr, weight, weight_sum, scale, g_ent, g_rel, want_value=True):
    """mkb_reg_rows through the C ABI on device copies -> (value or None); g_ent / g_rel (device, or None: value only) are added to."""
    from mkb_amd import _hip

    m = make_model(name, ent, rel, hidden, 6.0)
    lib, tb, B = _hip.lib(), m._tables(), sample.shape[0]
    s = sample.cuda().contiguous()
    w = None if weight is None else weight.cuda()
    ws_t = None if weight_sum is None else torch.tensor([weight_sum], dtype=torch.float32, device="cuda")
    sc = None if scale is None else torch.tensor([scale], dtype=torch.float32, device="cuda")
    value = torch.full((1,), float("nan"), device="cuda") if want_value else None
    need = lib.mkb_reg_rows_workspace_bytes(tb, B)
    assert need > 0
    ws = _hip.aligned_bytes(need + 4096, "cuda")
    ws[need:].fill_(0xA5)
    gr = None if g_ent is None and g_rel is None else _hip.Grads(None if g_ent is None else g_ent.data_ptr(),
                                                                  None if g_rel is None else g_rel.data_ptr(), None)
    _hip.check(lib.mkb_reg_rows(tb, gr, _hip.ptr(s), _hip.ptr(w), B, p, le, lr, _hip.ptr(ws_t), _hip.ptr(sc), _hip.ptr(value),
                                _hip.ptr(ws), need, _hip.stream_ptr()), "mkb_reg_rows")
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xA5).all()), "the call wrote past its workspace"
    return None if value is None else float(value)


@pytest.mark.parametrize("p", [2, 3])
@pytest.mark.parametrize("name", MODELS)
def test_kernel_against_float64(name, p):
    """Value and both gradients at every shape of ``_cases``: on zeroed buffers against the reference (grad_close; the value to
    ``value_bound``), and on buffers pre-filled with non-zero values, which the call must add to -- there the one extra rounding
    of ``prefill + gradient`` (2^-24 of the sum) joins grad_close's bound.  Rows of exact zeros in both tables: gradient exactly
    0, nothing NaN."""
    le, lr = 0.3, 0.7
    cases = _cases(name)
    if (name, p) == ("ComplEx", 3):  # past the rows up to which every workgroup reduces the weight sum itself: one launch in front
        cases.append(("B = 8193", 50, 4, 6, 8193, True, None, None))
    for k, (what, N, R, hidden, B, weighted, weight_sum, scale) in enumerate(cases):
        g = torch.Generator().manual_seed(100 * k + p)
        ent, rel = _tables(name, N, R, hidden, 7 * k + 1)
        ent[1] = 0.0
        if R > 1:
            rel[R - 1] = 0.0
        sample = _sample(N, R, B, g)
        if what.startswith("every triple"):
            sample[:] = torch.tensor([3, 0, 3])
        elif B == 1:
            sample[0] = torch.tensor([2, 0, 3])
        elif B >= 5:
            sample[0, 0] = 1                     # the zero rows are used
            sample[0, 1] = 0                     # ... and a relation row that is not zero
            sample[1, 1] = R - 1
            sample[2, 2] = sample[2, 0]          # h == t
            sample[4, 0] = sample[3, 0]          # a shared head
        weight = torch.rand(B, generator=g) + 0.1 if weighted else None
        ref, r_ent, r_rel = ur.reference(name, ent.numpy(), rel.numpy(), sample.numpy(), p, le, lr,
                                         None if weight is None else weight.numpy(), weight_sum)
        mult = 1.0 if scale is None else scale
        g_ent, g_rel = torch.zeros_like(ent).cuda(), torch.zeros_like(rel).cuda()
        got = _call(name, ent, rel, hidden, sample, p, le, lr, weight, weight_sum, scale, g_ent, g_rel)
        run = int(np.unique(np.concatenate([sample[:, 0].numpy(), sample[:, 2].numpy()]), return_counts=True)[1].max())
        bound = value_bound(ent.shape[1], B, max(run, B))
        print("reg_rows", name, p, what, "value", got, ref, "fraction of bound %.3f" % (abs(got - ref) / (bound * abs(ref))))
        assert abs(got - ref) <= bound * abs(ref), (what, got, ref)
        e, r = g_ent.cpu().numpy(), g_rel.cpu().numpy()
        assert not np.isnan(e).any() and not np.isnan(r).any(), what
        grad_close(e, mult * r_ent)
        grad_close(r, mult * r_rel)
        assert np.abs(r_ent).max() > 0 and np.abs(r_rel).max() > 0, what
        if not what.startswith("every triple") and B >= 5:
            assert not e[1].any() and (R == 1 or not r[R - 1].any()), what  # rows of exact zeros: exactly 0
        # value only, gradient only
        assert _call(name, ent, rel, hidden, sample, p, le, lr, weight, weight_sum, scale, None, None) == got, what
        # pre-filled buffers
        fill_e, fill_r = torch.rand(ent.shape, generator=g) - 0.5, torch.rand(rel.shape, generator=g) - 0.5
        p_ent, p_rel = fill_e.clone().cuda(), fill_r.clone().cuda()
        assert _call(name, ent, rel, hidden, sample, p, le, lr, weight, weight_sum, scale, p_ent, p_rel, want_value=False) is None
        for got_g, fill, want in ((p_ent, fill_e, mult * r_ent), (p_rel, fill_r, mult * r_rel)):
            total = fill.double().numpy() + want
            atol = min(1e-5, 2e-4 * float(np.abs(want).max())) + 2.0 ** -24 * float(np.abs(total).max())
            np.testing.assert_allclose(got_g.cpu().numpy(), total, rtol=0, atol=atol, err_msg=what)


@pytest.mark.parametrize("p", [2, 3])
@pytest.mark.parametrize("name", ["TransE", "RotatE", "ComplEx"])
def test_a_zero_weight_leaves_that_table_untouched_bit_for_bit(name, p):
    g = torch.Generator().manual_seed(5)
    N, R, hidden, B = 30, 4, 12, 50
    ent, rel = _tables(name, N, R, hidden, 3)
    sample = _sample(N, R, B, g)
    for le, lr in ((0.4, 0.0), (0.0, 0.4)):
        fill_e, fill_r = torch.rand(ent.shape, generator=g) - 0.5, torch.rand(rel.shape, generator=g) - 0.5
        g_ent, g_rel = fill_e.clone().cuda(), fill_r.clone().cuda()
        got = _call(name, ent, rel, hidden, sample, p, le, lr, None, None, None, g_ent, g_rel)
        ref, r_ent, r_rel = ur.reference(name, ent.numpy(), rel.numpy(), sample.numpy(), p, le, lr)
        assert abs(got - ref) <= value_bound(ent.shape[1], B, B) * abs(ref)
        untouched, fill, moved = (g_rel, fill_r, g_ent) if lr == 0.0 else (g_ent, fill_e, g_rel)
        assert torch.equal(untouched.cpu(), fill)
        assert not torch.equal(moved.cpu(), fill_e if lr == 0.0 else fill_r)
        # ... and its buffer may be missing altogether
        alone = (fill_e if lr == 0.0 else fill_r).clone().cuda()
        _call(name, ent, rel, hidden, sample, p, le, lr, None, None, None, alone if lr == 0.0 else None, None if lr == 0.0 else alone)
        assert torch.equal(alone, moved)


@pytest.mark.parametrize("name,p", [("TransE", 2), ("RotatE", 3), ("ComplEx", 3)])
def test_two_runs_give_the_same_bits(name, p):
    for N, R, hidden, B in ((7, 1, 8, 1500), (300, 6, 33, 257)):
        g = torch.Generator().manual_seed(B)
        ent, rel = _tables(name, N, R, hidden, 9)
        sample, weight = _sample(N, R, B, g), torch.rand(B, generator=g) + 0.1
        out = []
        for _ in range(2):
            g_ent, g_rel = torch.full(ent.shape, 0.25).cuda(), torch.full(rel.shape, -0.5).cuda()
            v = _call(name, ent, rel, hidden, sample, p, 0.3, 0.7, weight, None, None, g_ent, g_rel)
            out.append((np.float32(v).tobytes(), g_ent.cpu(), g_rel.cpu()))
        assert out[0][0] == out[1][0] and torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][2], out[1][2])


def test_ids_outside_the_tables_are_clamped_and_reported():
    from mkb_amd import regularizers

    ent, rel = _tables("DistMult", 10, 3, 8, 1)
    sample = torch.tensor([[0, 0, 1], [12, 1, 2], [3, 5, -4]])
    clamped = torch.tensor([[0, 0, 1], [9, 1, 2], [3, 2, 0]])
    g_ent, g_rel = torch.zeros_like(ent).cuda(), torch.zeros_like(rel).cuda()
    got = _call("DistMult", ent, rel, 8, sample, 3, 0.5, 0.5, None, None, None, g_ent, g_rel)
    ref, r_ent, r_rel = ur.reference("DistMult", ent.numpy(), rel.numpy(), clamped.numpy(), 3, 0.5, 0.5)
    assert abs(got - ref) <= value_bound(8, 3, 3) * abs(ref)
    grad_close(g_ent.cpu().numpy(), r_ent)
    grad_close(g_rel.cpu().numpy(), r_rel)
    m = make_model("DistMult", ent, rel, 8, 6.0)
    regularizers.N3(0.5)(m, sample.cuda())
    with pytest.raises(IndexError):
        m.check_ids()


# ---------------------------------------------------------------------------------------------------- autograd
N_ENT, N_REL, HIDDEN, BATCH, SIZE = 4200, 5, 20, 37, 16  # (4096 rows and more step row-lazily)


def _problem(name, seed=11):
    from mkb_amd import sampling

    g = torch.Generator().manual_seed(seed)
    ent, rel = _tables(name, N_ENT, N_REL, HIDDEN, seed)
    ent, rel = ent * 0.5, rel * 0.5
    rs = np.random.RandomState(seed)
    train = np.unique(np.stack([rs.randint(N_ENT, size=900), rs.randint(N_REL, size=900), rs.randint(N_ENT, size=900)], 1), axis=0)
    rs.shuffle(train)
    ents, rels = {i: i for i in range(N_ENT)}, {i: i for i in range(N_REL)}
    w = (torch.rand(BATCH, generator=g) + 0.5).cuda()

    def sampler():
        return sampling.NegativeSampling(size=SIZE, train_triples=[tuple(int(x) for x in t) for t in train], entities=ents,
                                         relations=rels, seed=3)

    def model():
        return make_model(name, ent, rel, HIDDEN, 6.0, torch.tensor([[0.1]]))

    return model, sampler, torch.as_tensor(train).cuda(), w


@pytest.mark.parametrize("name,p", [("ComplEx", 3), ("RotatE", 3), ("TransE", 2)])
def test_autograd_next_to_the_model_calls(name, p):
    """``(loss + 2 reg).backward()`` next to the two ``model(...)`` calls, torch.optim.Adam: .grad = that of the loss alone (a twin
    model) + 2 x the reference's gradient; the value is the reference's.  An empty batch gives 0 and a backward that adds nothing."""
    from mkb_amd import losses, regularizers

    model, sampler, train, w = _problem(name)
    sample = train[:BATCH].contiguous()
    crit, reg = losses.Adversarial(alpha=0.5), regularizers.Lp(p, 0.05, 0.02)
    grads, value = [], None
    ent0, rel0 = (t.detach().cpu().numpy().copy() for t in (model().entity_embedding, model().relation_embedding))
    for with_reg in (False, True):
        m, ns = model(), sampler()
        opt = torch.optim.Adam([m.entity_embedding, m.relation_embedding], lr=1e-3)
        opt.zero_grad()
        negatives = ns.generate(sample, "tail-batch")
        err = crit(m(sample), m(sample, negatives, "tail-batch"), w)
        if with_reg:
            value = reg(m, sample, w)
            assert value.dim() == 0 and value.requires_grad
            err = err + 2.0 * value
        err.backward()
        grads.append((m.entity_embedding.grad.cpu().numpy().copy(), m.relation_embedding.grad.cpu().numpy().copy()))
        opt.step()
    ref, r_ent, r_rel = ur.reference(name, ent0, rel0, sample.cpu().numpy(), p, 0.05, 0.02, w.cpu().numpy())
    assert abs(float(value.detach()) - ref) <= value_bound(m.entity_dim, BATCH, BATCH) * abs(ref)
    grad_close(grads[1][0] - grads[0][0], 2.0 * r_ent)
    grad_close(grads[1][1] - grads[0][1], 2.0 * r_rel)
    empty = reg(m, sample[:0])
    assert empty.dim() == 0 and float(empty.detach()) == 0.0
    empty.backward()


def _five_steps(name, reg, lazy):
    """Five explicit autograd steps (loss + regulariser) with mkb_amd.optim.Adam, row-lazy or dense -> the two tables."""
    from mkb_amd import _links, losses, optim

    model, sampler, train, w = _problem(name, seed=13)
    m, ns = model(), sampler()
    params = [m.entity_embedding, m.relation_embedding]
    opt = optim.Adam(params, lr=1e-2, lazy_rows=lazy)
    crit = losses.CrossEntropy()
    for it in range(5):
        s = train[it * BATCH:(it + 1) * BATCH].contiguous()
        mode = "head-batch" if it % 2 else "tail-batch"
        opt.zero_grad()
        err = crit(m(s), m(s, ns.generate(s, mode), mode), w) + reg(m, s, w)
        err.backward()
        opt.step()
    if lazy:
        ent = m.entity_embedding
        assert "last" in opt.state[ent] and _links.owner(ent) is opt, "the optimizer fell back to the dense kernel"
        assert not _links.autograd_wrote(ent)
        opt.flush()
    torch.cuda.synchronize()
    return m.entity_embedding.detach().cpu().numpy(), m.relation_embedding.detach().cpu().numpy()


@pytest.mark.parametrize("name", ["ComplEx", "DistMult"])
def test_autograd_route_keeps_the_row_lazy_optimizer(name):
    """Five steps of the explicit sequence with the regulariser under ``mkb_amd.optim.Adam(lazy_rows=True)`` against the same
    steps with the dense ``mkb_amd.optim.Adam``, flushed: the bound of tests/test_gpu_defer.py's README-loop comparison of the
    row-lazy route with a dense optimizer (atol 3e-4, mean below 2e-6; the score kernels add gradient rows with float atomics).
    The optimizer is still on its row-lazy route at the end.  The torch expression in the regulariser's place makes it fall back:
    the last assertion shows that the check can fail."""
    from mkb_amd import _links, losses, optim, regularizers

    reg = regularizers.N3(0.05)
    (ea, ra), (eb, rb) = _five_steps(name, reg, True), _five_steps(name, reg, False)
    print("row-lazy vs dense with N3: max |d ent| %.3g, max |d rel| %.3g" % (np.abs(ea - eb).max(), np.abs(ra - rb).max()))
    for x, y in ((ea, eb), (ra, rb)):
        np.testing.assert_allclose(x, y, rtol=0, atol=3e-4)
        assert float(np.abs(x - y).mean()) < 2e-6
    # the regulariser moved the tables at all
    e0, _ = _five_steps(name, regularizers.N3(0.0), False)
    assert float(np.abs(e0 - eb).max()) > 1e-5
    # what a user can do without it
    model, sampler, train, w = _problem(name, seed=13)
    m, ns = model(), sampler()
    opt = optim.Adam([m.entity_embedding, m.relation_embedding], lr=1e-2, lazy_rows=True)
    s = train[:BATCH].contiguous()
    err = losses.CrossEntropy()(m(s), m(s, ns.generate(s, "tail-batch"), "tail-batch"), w) + 0.05 * (m.entity_embedding[s[:, 0]].abs() ** 3).sum()
    err.backward()
    opt.step()
    assert _links.owner(m.entity_embedding) is None


# ---------------------------------------------------------------------------------------------------- fused steps
def _separate(m, reg, sample, w):
    """mkb_reg_rows on fresh buffers through the C ABI -> (value, g_ent, g_rel)."""
    g_ent, g_rel = torch.zeros_like(m.entity_embedding), torch.zeros_like(m.relation_embedding)
    v = _call(m.name, m.entity_embedding.detach().cpu(), m.relation_embedding.detach().cpu(), m.hidden_dim, sample.cpu(), reg.p,
              reg.entity_weight, reg.relation_weight, w.cpu(), None, None, g_ent, g_rel)
    return v, g_ent, g_rel


def _step_of(kind, m, reg):
    from mkb_amd import fused, losses

    if kind == "fused":
        return fused.FusedTrainStep(m, 0.5, regularizer=reg)
    return fused.PooledLossStep(m, losses.CrossEntropy(), regularizer=reg)


@pytest.mark.parametrize("kind", ["fused", "pooled"])
@pytest.mark.parametrize("name", ["RotatE", "ComplEx", "TransE"])
def test_fused_steps_add_the_regulariser(name, kind):
    """One step with a regulariser against the same step without it plus a separate mkb_reg_rows call on fresh buffers: the loss
    (1e-5 absolute and relative, the bound of the pooled-step comparison in tests/test_gpu_ns_losses.py) and .grad of both tables
    (grad_close; the step's own kernels add with float atomics)."""
    from mkb_amd import regularizers

    model, sampler, train, w = _problem(name)
    sample = train[:BATCH].contiguous()
    reg = regularizers.N3(0.05) if name != "TransE" else regularizers.Lp(2, 0.03, 0.0)
    out = []
    for r in (None, reg):
        m = model()
        step = _step_of(kind, m, r)
        loss = step(sample, w, sampler().generate(sample, "head-batch"), "head-batch")
        out.append((float(loss), m.entity_embedding.grad.cpu().numpy().copy(), m.relation_embedding.grad.cpu().numpy().copy(), step))
    value, g_ent, g_rel = _separate(m, reg, sample, w)
    assert out[0][3].regularization is None and float(out[1][3].regularization) == value  # (the same call: the same bits)
    want = out[0][0] + value
    assert abs(out[1][0] - want) <= 1e-5 + 1e-5 * abs(want)
    assert value > 1e-4
    grad_close(out[1][1], out[0][1].astype(np.float64) + g_ent.cpu().numpy())
    grad_close(out[1][2], out[0][2].astype(np.float64) + g_rel.cpu().numpy())
    assert np.abs(g_ent.cpu().numpy()).max() > 0


@pytest.mark.parametrize("kind", ["fused", "pooled"])
def test_fused_steps_under_a_deferring_row_lazy_optimizer(kind, monkeypatch):
    """Five steps with ``mkb_amd.optim.Adam(lazy_rows=True, defer_step=True)``: the step with a regulariser against the step
    without it followed by a separate mkb_reg_rows call whose fresh buffers are added to .grad before ``optimizer.step()``.  From
    the third step on ``mkb_pool_step`` is promised clear rows (``rows_clear = 1``) and STORES gradient rows: the regulariser,
    launched behind it, must survive.  Tables after the flush to atol 2e-6, the bound of tests/test_gpu_defer.py's comparison of
    two fused runs (float atomics in the step's kernels); losses as above.  ComplEx: product gradients, no exact cancellations
    (see tests/test_gpu_ns_losses.py on TransE's sign sums under Adam)."""
    from mkb_amd import _links, optim, regularizers

    reg = regularizers.N3(0.05)
    promised = []
    inner = optim.Adam.begin_step_on

    def spy(self, p, ids):
        promised.append(inner(self, p, ids))
        return promised[-1]

    monkeypatch.setattr(optim.Adam, "begin_step_on", spy)

    def run(joined):
        model, sampler, train, w = _problem("ComplEx", seed=17)
        m, ns = model(), sampler()
        opt = optim.Adam([m.entity_embedding, m.relation_embedding], lr=1e-3, lazy_rows=True, defer_step=True)
        step = _step_of(kind, m, reg if joined else None)
        losses_ = []
        for it in range(5):
            s = train[it * BATCH:(it + 1) * BATCH].contiguous()
            loss = step.sampled(s, w, ns, "head-batch" if it % 2 else "tail-batch")
            if not joined:
                value, g_ent, g_rel = _separate(m, reg, s, w)
                m.entity_embedding.grad.add_(g_ent)
                m.relation_embedding.grad.add_(g_rel)
                loss = loss + value
            losses_.append(float(loss))
            opt.step()
            opt.zero_grad()
        assert "last" in opt.state[m.entity_embedding] and _links.owner(m.entity_embedding) is opt
        opt.flush()
        torch.cuda.synchronize()
        return m.entity_embedding.detach().cpu().numpy(), m.relation_embedding.detach().cpu().numpy(), losses_

    a = run(True)
    if kind == "fused":
        # (the first step is applied at once, the second is the first to be deferred: clear rows are promised from the third on)
        assert promised[:2] == [False, False] and promised[2:5] == [True, True, True], promised
    b = run(False)
    np.testing.assert_allclose(a[2], b[2], rtol=1e-5, atol=1e-5)
    for x, y in zip(a[:2], b[:2]):
        print("deferred, %s: max |d| %.3g" % (kind, np.abs(x - y).max()))
        np.testing.assert_allclose(x, y, rtol=0, atol=2e-6)


@pytest.mark.parametrize("name,loss_name,reg_name", [("ComplEx", "CrossEntropy", "N3"), ("RotatE", "Adversarial", "L2")])
def test_pipeline_regulariser_on_the_fused_and_the_explicit_route(name, loss_name, reg_name):
    """Pipeline.learn with ``regularizer`` set, two epochs on CountriesS1: the fused route (PooledLossStep for the softmax loss,
    FusedTrainStep for Adversarial) against the explicit sequence (``fuse = False``), same sampler seed and torch.optim.Adam: the
    tables to the bound of the row-lazy comparison above (atol 3e-4, mean below 2e-6).  Without the regulariser the tables differ."""
    from mkb_amd import compose, datasets, fused, losses, models, regularizers, sampling

    def run(fuse, weight):
        ds = datasets.CountriesS1(batch_size=64, shuffle=False, seed=42, num_workers=0)
        ds.valid, ds.test = [], []
        torch.manual_seed(5)
        m = getattr(models, name)(hidden_dim=20, entities=ds.entities, relations=ds.relations, gamma=6.0).cuda()
        ns = sampling.NegativeSampling(size=16, train_triples=ds.train, entities=ds.entities, relations=ds.relations, seed=42)
        opt = torch.optim.Adam([m.entity_embedding, m.relation_embedding], lr=1e-3)
        pipe = compose.Pipeline(epochs=2, eval_every=100, device="cuda")
        pipe.fuse = fuse
        pipe.regularizer = getattr(regularizers, reg_name)(weight)
        loss = getattr(losses, loss_name)()
        step = pipe._fused_step_for(m, ds, ns, opt, loss)
        assert (step is not None) == fuse and (not fuse or step.regularizer is pipe.regularizer)
        assert not fuse or type(step) is (fused.FusedTrainStep if loss_name == "Adversarial" else fused.PooledLossStep)
        pipe.learn(model=m, dataset=ds, sampling=ns, optimizer=opt, loss=loss)
        return m.entity_embedding.detach().cpu().numpy(), m.relation_embedding.detach().cpu().numpy(), pipe.metric_loss.get()

    a, b, c = run(True, 0.05), run(False, 0.05), run(True, 0.0)
    assert math.isfinite(a[2]) and abs(a[2] - b[2]) <= 1e-4 * max(1.0, abs(b[2]))
    for x, y in zip(a[:2], b[:2]):
        print("pipeline fused vs explicit: max |d| %.3g mean %.3g" % (np.abs(x - y).max(), np.abs(x - y).mean()))
        np.testing.assert_allclose(x, y, rtol=0, atol=3e-4)
        assert float(np.abs(x - y).mean()) < 2e-6
    assert float(np.abs(a[0] - c[0]).max()) > 1e-4
