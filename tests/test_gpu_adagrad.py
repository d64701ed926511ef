"""``mkb_amd.optim.Adagrad`` / ``mkb_adagrad_step`` (mkb_amd/csrc/adagrad.hip) on the device: the row-sparse step is dense Adagrad
bit for bit, visits only the rows it is told about, stays within twice torch's own distance from a float64 restatement, carries
the dense tensors and the sampler's draw in its launch, and speaks the row-lazy protocol of the fused steps, the explicit
sequence, checkpoints and ``compose.Pipeline``."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, R_DENSE, N_IDS, STEPS = 5000, 37, 300, 12  # 5,000 rows: over the 4,096-row rule, so the table steps row-sparsely
LR, LR_DECAY, EPS = 0.1, 1e-3, 1e-10
SHAPES = [(64, 0.0), (64, 0.1), (33, 0.0), (33, 0.1), (2000, 0.0), (2000, 0.1)]  # D: float4 rows, unaligned scalar rows, 500 float4 per row


def _clr(step):
    return LR / (1 + (step - 1) * LR_DECAY)


@functools.lru_cache(maxsize=None)
def _stream(D, seed=11):
    """The hand-made gradients of STEPS steps (host tensors, made once per D): 300 row ids with duplicates, one value row per
    distinct id, a dense [37, D] gradient and a [1, 1] one."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return [(torch.randint(N, (N_IDS,), generator=g), torch.randn(N_IDS, D, generator=g), torch.randn(R_DENSE, D, generator=g),
             torch.randn(1, 1, generator=g)) for _ in range(STEPS)]


def _dense_grad(ids, vals):
    """[N, D] on the device: one deterministic value row per distinct id."""
    G = torch.zeros(N, vals.shape[1], device="cuda")
    uniq = torch.unique(ids.cuda())
    G[uniq] = vals[: uniq.numel()].cuda()
    return G


def _offset(t, off):
    """A copy of ``t`` whose storage starts ``off`` floats past an allocation: off = 1 makes every pointer 4-byte aligned only."""
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device="cuda")
    view = buf[off:].view(t.shape)
    view.copy_(t)
    return view


def _initial(D, init, off=0, seed=5):
    """(table, dense [37, D], dense [1, 1]) as (p, sum) pairs on the device, |p| up to ~4.8."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    out = []
    for shape in ((N, D), (R_DENSE, D), (1, 1)):
        p = torch.randn(shape, generator=g)
        out.append((_offset(p, off), _offset(torch.full(shape, init), off)))
    return out


def _abi_step(table, last, ids, step, dense=(), sampler=None, n_ids=None):
    """One ``mkb_adagrad_step``.  table: (p, g, sum) or None; ids: int64 device tensor, or None for the all-rows form; dense: (p, g, sum)s."""
    from mkb_amd import _hip

    arr = (_hip.AdagradDense * len(dense))(*[_hip.AdagradDense(p.data_ptr(), g.data_ptr(), s.data_ptr(), p.numel()) for p, g, s in dense]) \
        if dense else None
    if table is None:
        args = (None, None, None, None, 0, 0, None, 0)
    else:
        p, g, s = table
        args = (_hip.ptr(p), _hip.ptr(g), _hip.ptr(s), _hip.ptr(last), p.shape[0], p.shape[1], _hip.ptr(ids),
                (0 if ids is None else ids.numel()) if n_ids is None else n_ids)
    _hip.check(_hip.lib().mkb_adagrad_step(*args, step, _clr(step), EPS, arr, len(dense), sampler, _hip.stream_ptr()), "mkb_adagrad_step")


def _run_abi(D, init, form, off=0):
    """STEPS steps of the stream through the C ABI.  form: "listed" (the ids as drawn, plus one negative and one past the table),
    "sorted" (de-duplicated and sorted), "all" (the all-rows form).  -> [(p, sum)] x 3, last."""
    (p, s), (rp, rs), (mp, ms) = _initial(D, init, off)
    last = torch.zeros(N, dtype=torch.int32, device="cuda")
    for it, (ids, vals, relg, modg) in enumerate(_stream(D)):
        g, rg, mg = _offset(_dense_grad(ids, vals), off), _offset(relg, off), _offset(modg, off)
        if form == "listed":
            lst = torch.cat([ids[:150], torch.tensor([-7]), ids[150:], torch.tensor([N + 3])]).cuda()
        elif form == "sorted":
            lst = torch.unique(ids.cuda())
        else:
            lst = None
        _abi_step((p, g, s), last, lst, it + 1, dense=[(rp, rg, rs), (mp, mg, ms)])
        assert not g.any() and not rg.any() and not mg.any(), (form, it)
    return [(p, s), (rp, rs), (mp, ms)], last


@pytest.mark.parametrize("D,init", SHAPES)
def test_row_sparse_equals_dense_bit_for_bit(D, init):
    """The same gradients through the listed form, the all-rows form and a de-duplicated, sorted list: tables, accumulators and
    the dense tensors are the same bits (D = 33 with every pointer off the 16-byte grid as well)."""
    off = 1 if D == 33 else 0
    listed, _ = _run_abi(D, init, "listed", off)
    for form in ("all", "sorted"):
        other, _ = _run_abi(D, init, form, off)
        for (a, sa), (b, sb) in zip(listed, other):
            assert torch.equal(a, b) and torch.equal(sa, sb), (form, a.shape)


@pytest.mark.parametrize("D,off", [(64, 0), (33, 0), (2000, 0), (64, 1)])
def test_only_listed_rows_are_visited(D, off):
    (p, s), _, _ = _initial(D, 0.1, off)
    ids, vals = _stream(D)[0][:2]
    g = _offset(_dense_grad(ids, vals), off)
    free = int((torch.bincount(ids, minlength=N) == 0).nonzero()[0])  # a row nobody lists
    g[free] = 7.0
    last = torch.randint(0, 3, (N,), dtype=torch.int32, device="cuda")  # stamps of earlier steps
    p0, s0, last0, step = p.clone(), s.clone(), last.clone(), 3
    lst = torch.cat([ids, torch.tensor([-1, N])]).cuda()
    _abi_step((p, g, s), last, lst, step)
    assert bool((g[free] == 7.0).all()), "a row that was not listed had its gradient cleared"
    assert torch.equal(p[free], p0[free]) and torch.equal(s[free], s0[free]) and int(last[free]) == int(last0[free])
    g[free] = 0.0
    assert not g.any(), "a listed gradient row was left behind"
    uniq = torch.unique(ids.cuda())
    assert torch.equal((last == step).nonzero().flatten(), uniq), "the stamps of this step are not exactly the distinct valid ids"
    untouched = torch.ones(N, dtype=torch.bool, device="cuda")
    untouched[uniq] = False
    assert torch.equal(p[untouched], p0[untouched]) and torch.equal(s[untouched], s0[untouched]) and torch.equal(last[untouched], last0[untouched])
    assert not torch.equal(p[uniq], p0[uniq])


def _parameters(D, init):
    return [torch.nn.Parameter(p.clone()) for p, _ in _initial(D, init)]


def _optimizer_steps(opt, params, D, steps, on_grads=None):
    """The stream's gradients through the protocol, as tests/test_gpu_defer.py::_synthetic_steps does it: rows made current, THEN
    their gradient, the mark, the step."""
    from mkb_amd import _links

    ent, rel, mod = params
    for it in steps:
        ids, vals, relg, modg = _stream(D)[it]
        ids = ids.cuda()
        opt.catch_up(ent, ids)
        uniq = torch.unique(ids)
        ent.grad[uniq] += vals[: uniq.numel()].cuda()
        rel.grad, mod.grad = relg.cuda(), modg.cuda()
        _links.mark_touched(ent, ids)
        if on_grads is not None:
            on_grads(it)
        opt.step()
        opt.zero_grad()


def _rule64(p64, s64, g, clr):
    """The element rule restated in float64, in place."""
    g = g.double()
    s64 += g * g
    p64 -= clr * g / (s64.sqrt() + EPS)


def _dev(x, p64):
    return float((x.detach().double() - p64).abs().max())


def _assert_within_twice_torch(name, got, yard, p64):
    """The kernel's largest deviation from float64 against torch.optim.Adagrad's own (float32, on the device): both follow the
    rule with one rounding per operation and differ at most in where a multiply-add is contracted, so a factor of 2."""
    k, y = _dev(got, p64), _dev(yard, p64)
    print(f"{name}: kernel {k:.3e}  torch {y:.3e}")
    assert k <= 2 * y, f"{name}: kernel deviates {k:.3e} from float64, torch.optim.Adagrad {y:.3e}"


@pytest.mark.parametrize("D,init", SHAPES)
def test_against_float64_within_twice_torch(D, init):
    from mkb_amd import optim

    params = _parameters(D, init)
    opt = optim.Adagrad(params, lr=LR, lr_decay=LR_DECAY, initial_accumulator_value=init, eps=EPS)
    assert params[0].grad is not None and not params[0].grad.any()
    _optimizer_steps(opt, params, D, range(STEPS))
    assert all(not p.grad.any() for p in params)
    # the optimizer drives the very launches of the C ABI test
    abi, last = _run_abi(D, init, "listed")
    for q, (a, sa) in zip(params, abi):
        assert torch.equal(q.detach(), a) and torch.equal(opt.state[q]["sum"], sa)
    assert torch.equal(opt.state[params[0]]["last"], last)
    # torch's own step and the float64 rule on the same gradients
    yard = _parameters(D, init)
    ref = torch.optim.Adagrad(yard, lr=LR, lr_decay=LR_DECAY, initial_accumulator_value=init, eps=EPS, foreach=True)
    p64 = [q.detach().double().clone() for q in yard]
    s64 = [torch.full_like(q, init) for q in p64]
    for it, (ids, vals, relg, modg) in enumerate(_stream(D)):
        grads = [_dense_grad(ids, vals), relg.cuda(), modg.cuda()]
        for q, g, a, b in zip(yard, grads, p64, s64):
            q.grad = g
            _rule64(a, b, g, _clr(it + 1))
        ref.step()
    for name, q, y, a in zip(("table", "dense [37, D]", "dense [1, 1]"), params, yard, p64):
        _assert_within_twice_torch(f"D={D} init={init} {name}", q, y, a)
    # The documented claim: the kernel applies the operations of torch's FOREACH step (addcmul_, sqrt, add_, mul, addcdiv_), each
    # rounded once and none contracted, so it gives that step's bits.  (torch's single-tensor path forms p + (-clr) * (g / std)
    # and rounds differently; the claim is about the foreach path, torch's default on a device.)
    for name, q, y in zip(("table", "dense [37, D]", "dense [1, 1]"), params, yard):
        assert torch.equal(q.detach(), y.detach()), f"D={D} init={init} {name}: {int((q != y).sum())} elements differ from torch's foreach step"
        assert torch.equal(opt.state[q]["sum"], ref.state[y]["sum"]), f"D={D} init={init} {name}: accumulators differ"


def test_dense_only_form_and_an_empty_id_list():
    _, (rp, rs), (mp, ms) = _initial(33, 0.1, off=1)  # n = 37 * 33 = 1221 (no multiple of 4) and 1, unaligned
    _, _, relg, modg = _stream(33)[0]
    rg, mg = _offset(relg, 1), _offset(modg, 1)
    want = []
    for p, s, g in ((rp, rs, rg), (mp, ms, mg)):
        p64, s64 = p.double().clone(), s.double().clone()
        _rule64(p64, s64, g, _clr(1))
        want.append((p64, s64))
    _abi_step(None, None, None, 1, dense=[(rp, rg, rs), (mp, mg, ms)])
    assert not rg.any() and not mg.any()
    for (p, s), (p64, s64) in zip(((rp, rs), (mp, ms)), want):
        np.testing.assert_allclose(p.double().cpu().numpy(), p64.cpu().numpy(), rtol=0, atol=1e-6)
        np.testing.assert_allclose(s.double().cpu().numpy(), s64.cpu().numpy(), rtol=1e-6, atol=0)
    # a listed call with no ids: the dense tensor steps, the table is not touched (a null id list would be the all-rows form)
    (p, s), (rp, rs), _ = _initial(64, 0.0)
    g = torch.ones_like(p)
    last = torch.zeros(N, dtype=torch.int32, device="cuda")
    rg = _stream(64)[0][2].cuda()
    p0, s0, rp0 = p.clone(), s.clone(), rp.clone()
    _abi_step((p, g, s), last, torch.zeros(1, dtype=torch.int64, device="cuda"), 1, dense=[(rp, rg, rs)], n_ids=0)
    assert torch.equal(p, p0) and torch.equal(s, s0) and bool((g == 1).all()) and not last.any()
    assert not rg.any() and not torch.equal(rp, rp0)


def _triples(n=3000, n_rel=11, seed=1):
    rs = np.random.RandomState(seed)
    return np.stack([rs.randint(N, size=n), rs.randint(n_rel, size=n), rs.randint(N, size=n)], 1)


def test_the_samplers_draw_rides_the_launch(monkeypatch):
    """The negatives of 6 batches and the generator state behind them are the same whether the optimizer's launch draws the
    sampler's next pool or the sampler draws it itself -- and the launch did carry the sampler."""
    from mkb_amd import _hip, optim, sampling

    train = _triples()
    t = torch.as_tensor(train).cuda()
    ents, rels = {i: i for i in range(N)}, {i: i for i in range(11)}
    carried, inner = [], _hip.lib().mkb_adagrad_step
    monkeypatch.setattr(_hip.lib(), "mkb_adagrad_step", lambda *a: (carried.append(a[13] is not None), inner(*a))[1])
    out = []
    for ride in (False, True):
        ns = sampling.NegativeSampling(size=16, train_triples=train, entities=ents, relations=rels, seed=1)
        params = _parameters(64, 0.0)
        opt = optim.Adagrad(params, lr=LR, draw_ahead=ns if ride else None)
        negs, state = [], []
        del carried[:]

        def generate(it):
            negs.append(ns.generate(t[it * 32: (it + 1) * 32].contiguous(), "tail-batch" if it % 2 else "head-batch").clone())

        _optimizer_steps(opt, params, 64, range(6), on_grads=generate)
        ns.check()
        key, pos = ns.get_state()
        assert sum(carried) == (6 if ride else 0), carried  # (the sampler's device state exists from its first generate on)
        # ... and the launch TOOK the draw (sampler_draw_ahead answered true): a pool drawn ahead is pending behind the last step.
        # The library says so when asked to switch generators, which it refuses while one is pending (and otherwise does: this
        # sampler is not used again).  A pending flag without a pool really drawn would have given other negatives above.
        rc = _hip.lib().mkb_sampler_set_rng(ns._handle, 1, 0, 0)
        pending = rc == _hip.ERR_INVALID and b"drawn ahead" in _hip.lib().mkb_last_error()
        assert pending == ride and (ride or rc == 0), (ride, rc, _hip.lib().mkb_last_error())
        out.append((negs, np.asarray(key).copy(), pos, [q.detach().clone() for q in params]))
    for a, b in zip(out[0][0], out[1][0]):
        assert torch.equal(a, b)
    assert np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]
    for a, b in zip(out[0][3], out[1][3]):
        assert torch.equal(a, b)


def _model(name, hidden=32, n_rel=11, seed=3):
    from mkb_amd import models

    torch.manual_seed(seed)
    return getattr(models, name)(hidden_dim=hidden, entities={i: i for i in range(N)}, relations={i: i for i in range(n_rel)},
                                 gamma=6.0).cuda()


def _trained(m):
    return [m.entity_embedding, m.relation_embedding] + ([m.modulus] if m.name == "pRotatE" else [])


def _copy_of(m, name):
    fresh = _model(name)
    with torch.no_grad():
        for a, b in zip(_trained(fresh), _trained(m)):
            a.copy_(b)
    return fresh


@pytest.mark.parametrize("reg", [False, True])
@pytest.mark.parametrize("kind", ["adversarial", "softmax"])
@pytest.mark.parametrize("name", ["TransE", "ComplEx", "pRotatE"])
def test_through_the_fused_steps(name, kind, reg):
    """5 steps of ``step.sampled(...)``: the gradient the optimizer is about to consume is the one the same step class produces on
    a fresh model with no optimizer (a ``rows_clear`` promised wrongly, or a row left uncleared, shows here), every gradient is zero
    after the step, and the tables follow the float64 rule on those gradients as closely as torch.optim.Adagrad does."""
    from mkb_amd import fused, losses, optim, regularizers, sampling
    from util_gpu import grad_close

    B, K = 64, 16
    train = _triples()
    t = torch.as_tensor(train).cuda()
    m = _model(name)
    assert fused.pooled_supported(m, B, K)
    ns = sampling.NegativeSampling(size=K, train_triples=train, entities=m.entities, relations=m.relations, seed=1)

    def make_step(model):
        regulariser = regularizers.N3(1e-3) if reg else None
        if kind == "adversarial":
            return fused.FusedTrainStep(model, 1.0, regularizer=regulariser)
        return fused.PooledLossStep(model, losses.CrossEntropy(), regularizer=regulariser)

    params = _trained(m)
    opt = optim.Adagrad(params, lr=LR, lr_decay=LR_DECAY, draw_ahead=ns)
    answers, inner = [], opt.begin_step_on
    opt.begin_step_on = lambda p, ids: (answers.append(inner(p, ids)), answers[-1])[1]
    step = make_step(m)
    yard = [torch.nn.Parameter(q.detach().clone()) for q in params]
    ref = torch.optim.Adagrad(yard, lr=LR, lr_decay=LR_DECAY)
    p64 = [q.detach().double().clone() for q in params]
    s64 = [torch.zeros_like(q) for q in p64]
    weight = torch.rand(B, generator=torch.Generator().manual_seed(2)).cuda() + 0.5
    for it in range(5):
        sample, mode = t[it * B: (it + 1) * B].contiguous(), "tail-batch" if it % 2 else "head-batch"
        loss = step.sampled(sample, weight, ns, mode)
        assert bool(torch.isfinite(loss))
        fresh = _copy_of(m, name)
        make_step(fresh)(sample, weight, step.negative_sample, mode)
        # The two tables.  pRotatE's [1, 1] modulus is not compared here: its gradient is ONE scalar that sums B (2K + 1) terms whose
        # positive and negative totals cancel, accumulated with float atomics by both runs, and differs from run to run of the SAME
        # step by about grad_close's absolute 1e-5 (tests/test_gpu_ns_losses.py::test_pooled_step_equals_the_explicit_autograd_
        # sequence documents 0.38 - 1.06 of that bound).  What the optimizer does with it is covered: it is zero after every step
        # and follows the float64 rule below.
        for what, q, f in zip(("entities", "relations"), params, _trained(fresh)):
            got, want = q.grad.cpu().numpy(), f.grad.cpu().numpy()
            print(f"{name} {kind} reg={reg} step {it} {what}: fraction of grad_close's bound "
                  f"{np.abs(got - want).max() / min(1e-5, 2e-4 * max(float(np.abs(want).max()), 1e-30)):.4f}")
            grad_close(got, want)
        grads = [q.grad.clone() for q in params]
        opt.step()
        opt.zero_grad()
        assert all(not q.grad.any() for q in params), it
        for q, g, a, b in zip(yard, grads, p64, s64):
            q.grad = g
            _rule64(a, b, g, _clr(it + 1))
        ref.step()
    ns.check()
    assert len(answers) == 5
    if kind == "adversarial":
        assert all(answers[1:]), answers  # every row of .grad is known to be zero: mkb_pool_step may store its rows
    for label, q, y, a in zip(("entities", "relations", "modulus"), params, yard, p64):
        _assert_within_twice_torch(f"{name} {kind} reg={reg} {label}", q, y, a)


@pytest.mark.parametrize("kind,reg", [("adversarial", False), ("adversarial", True), ("softmax", True)])
def test_a_big_relation_table_whose_rows_no_step_reports_is_still_stepped_and_cleared(kind, reg):
    """A relation table of 4,096 rows or more is attached like the entity table, but the fused steps report entity rows only: they
    write ``rel.grad`` and mark nothing.  Such a table must not be taken for one nobody wrote to: every step it takes the all-rows
    form, trains, and has its gradient cleared -- the bits of torch's step on the same gradients."""
    from mkb_amd import _links, fused, losses, optim, regularizers, sampling

    B, K, n_rel = 64, 16, 4100
    train = _triples(n_rel=n_rel)
    t = torch.as_tensor(train).cuda()
    m = _model("TransE", n_rel=n_rel)
    ent, rel = m.entity_embedding, m.relation_embedding
    assert fused.pooled_supported(m, B, K)
    ns = sampling.NegativeSampling(size=K, train_triples=train, entities=m.entities, relations=m.relations, seed=1)
    opt = optim.Adagrad([ent, rel], lr=LR, lr_decay=LR_DECAY, draw_ahead=ns)
    assert _links.owner(ent) is opt and _links.owner(rel) is opt
    regulariser = regularizers.N3(1e-3) if reg else None
    step = fused.FusedTrainStep(m, 1.0, regularizer=regulariser) if kind == "adversarial" else \
        fused.PooledLossStep(m, losses.CrossEntropy(), regularizer=regulariser)
    yard = [torch.nn.Parameter(q.detach().clone()) for q in (ent, rel)]
    ref = torch.optim.Adagrad(yard, lr=LR, lr_decay=LR_DECAY, foreach=True)
    weight = torch.ones(B, device="cuda")
    for it in range(3):
        sample, mode = t[it * B: (it + 1) * B].contiguous(), "tail-batch" if it % 2 else "head-batch"
        before = rel.detach().clone()
        step.sampled(sample, weight, ns, mode)
        grads = [ent.grad.clone(), rel.grad.clone()]
        written = grads[1].abs().sum(1) > 0
        assert torch.equal(written.nonzero().flatten(), torch.unique(sample[:, 1])), "the step wrote other relation rows than the batch's"
        opt.step()
        opt.zero_grad()
        assert not ent.grad.any() and not rel.grad.any(), f"step {it}: a gradient survived the optimizer step"
        assert opt.state[rel]["n"] == it + 1 and opt.state[ent]["n"] == it + 1
        changed = (rel.detach() != before).any(1)
        assert torch.equal(changed, written), f"step {it}: the relation rows that moved are not the rows that had a gradient"
        for q, g in zip(yard, grads):
            q.grad = g
        ref.step()
        for what, q, y in zip(("entities", "relations"), (ent, rel), yard):
            assert torch.equal(q.detach(), y.detach()), f"step {it} {what}: {int((q != y).sum())} elements differ from torch's step"
    ns.check()


def test_the_explicit_sequence_stays_row_sparse_and_falls_back_for_one_step():
    from mkb_amd import losses, optim, sampling

    B, K = 64, 16
    train = _triples()
    t = torch.as_tensor(train).cuda()
    m = _model("TransE")
    ent, rel = m.entity_embedding, m.relation_embedding
    ns = sampling.NegativeSampling(size=K, train_triples=train, entities=m.entities, relations=m.relations, seed=1)
    opt = optim.Adagrad([ent, rel], lr=LR, lr_decay=LR_DECAY)
    loss_fn = losses.Adversarial(alpha=1.0)
    weight = torch.ones(B, device="cuda")
    last = opt.state[ent]["last"]
    for it in range(5):
        sample, mode = t[it * B: (it + 1) * B].contiguous(), "tail-batch" if it % 2 else "head-batch"
        positive = m(sample)
        neg = ns.generate(sample, mode)
        loss = loss_fn(positive, m(sample, neg, mode), weight)
        dense_step = it == 3
        if dense_step:  # a plain torch penalty on the whole table: autograd writes into .grad, which rows is unknown
            loss = loss + m.entity_embedding.pow(2).sum() * 1e-6
        loss.backward()
        read = torch.unique(neg._mkb_pool.rows(sample))
        if dense_step:
            before, before_sum, g = ent.detach().clone(), opt.state[ent]["sum"].clone(), ent.grad.clone()
            assert int((g.abs().sum(1) > 0).sum()) > read.numel()
        opt.step()
        opt.zero_grad()
        assert opt.state[ent]["n"] == it + 1
        assert not ent.grad.any() and not rel.grad.any()
        stamped = (last == it + 1).nonzero().flatten()
        if not dense_step:
            assert torch.equal(stamped, read), (it, stamped.numel(), read.numel())  # only the rows the batch read were visited
            continue
        assert stamped.numel() == N  # the all-rows form, this once
        p64, s64 = before.double(), before_sum.double()
        yard = torch.nn.Parameter(before.clone())
        ref = torch.optim.Adagrad([yard], lr=_clr(it + 1), eps=EPS)  # (its first step: the rate as given)
        ref.state[yard]["sum"].copy_(before_sum)
        yard.grad = g
        ref.step()
        _rule64(p64, s64, g, _clr(it + 1))
        _assert_within_twice_torch("all-rows step", ent, yard, p64)
    ns.check()


@pytest.mark.parametrize("D,init", [(64, 0.1), (33, 0.0)])
def test_checkpoint_round_trip_continues_bit_for_bit(D, init):
    from mkb_amd import optim

    kwargs = dict(lr=LR, lr_decay=LR_DECAY, initial_accumulator_value=init, eps=EPS)
    whole = _parameters(D, init)
    opt = optim.Adagrad(whole, **kwargs)
    _optimizer_steps(opt, whole, D, range(12))
    first = _parameters(D, init)
    opt1 = optim.Adagrad(first, **kwargs)
    _optimizer_steps(opt1, first, D, range(6))
    sd = opt1.state_dict()
    second = [torch.nn.Parameter(q.detach().clone()) for q in first]
    opt2 = optim.Adagrad(second, lr=7.0)  # (every hyper-parameter comes from the checkpoint)
    opt2.load_state_dict(sd)
    assert int(opt2.state[second[0]]["last"].max()) < 7 and opt2.state[second[0]]["n"] == 6
    _optimizer_steps(opt2, second, D, range(6, 12))
    for a, b in zip(whole, second):
        assert torch.equal(a.detach(), b.detach()) and torch.equal(opt.state[a]["sum"], opt2.state[b]["sum"])


def test_pipeline_learns_with_adagrad_on_the_fused_step(monkeypatch):
    from mkb_amd import compose, datasets, fused, losses, optim, sampling

    train = [tuple(int(v) for v in row) for row in _triples(n=128)]  # 2 head batches and 2 tail batches of 64
    ents, rels = {i: i for i in range(N)}, {i: i for i in range(11)}
    ds = datasets.Dataset(train=train, batch_size=64, entities=ents, relations=rels, shuffle=False, num_workers=0, seed=42)
    m = _model("TransE")
    ns = sampling.NegativeSampling(size=16, train_triples=train, entities=ents, relations=rels, seed=42)
    opt = optim.Adagrad([m.entity_embedding, m.relation_embedding], lr=LR)
    seen, inner = [], fused.FusedTrainStep.__call__

    def spy(self, *args, **kwargs):
        assert opt.draw_ahead is ns  # the pipeline lent the sampler for the length of learn()
        out = inner(self, *args, **kwargs)
        seen.append(out.detach())
        return out

    monkeypatch.setattr(fused.FusedTrainStep, "__call__", spy)
    before = m.entity_embedding.detach().clone()
    compose.Pipeline(epochs=1, eval_every=100, device="cuda").learn(model=m, dataset=ds, sampling=ns, optimizer=opt,
                                                                      loss=losses.Adversarial(alpha=1.0))
    assert len(seen) == 4, "the pipeline did not take the fused step for every batch"
    assert opt.draw_ahead is None, "the sampler was not given back"
    assert opt.step_count == 4 and opt.state[m.entity_embedding]["n"] == 4
    assert bool(torch.isfinite(torch.stack(seen)).all())
    assert not m.entity_embedding.grad.any() and not m.relation_embedding.grad.any()
    assert not torch.equal(before, m.entity_embedding.detach())


def test_sharded_tables_are_refused_loudly():
    from mkb_amd import optim

    ent = torch.nn.Parameter(torch.zeros(N, 8, device="cuda"))
    opt = optim.Adagrad([ent])
    with pytest.raises(NotImplementedError, match="single-device"):
        opt.catch_up_sharded(ent, torch.zeros(4, dtype=torch.int64, device="cuda"), 2, 0, None)
