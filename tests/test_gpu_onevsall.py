"""-m gpu: the 1vsAll softmax step of ComplEx / DistMult (mkb_amd/csrc/score_all.hip; fused.OneVsAllStep, losses.OneVsAll,
model.score_all) over the case table of tests/util_onevsall.py -- every kernel family of the three products, the forward's lane
fallback, every N % 4, a row longer than the softmax kernel's LDS staging -- on both sides.

  forward    model.score_all has the bits of Evaluation.ranks(..., with_scores=True);
  tolerance  loss, positive_score, dS, g_ent and g_rel against float64 within 8 x err_ref (util_onevsall.tolerance; the ratios
             measured on the MI355X are in profiles/r23_onevsall_errors.txt);
  pad trap   for N % 4 != 0 the loss and the gradient row of entity N - 1 agree with float64.  A kernel that lets the forward's pad
             columns into the softmax counts the last entity 2 to 4 times.  At N = 129 .. 131 that moves the loss by 3e-3 .. 3e-2
             (860 to 9,300 times its tolerance) and that gradient row by 2e-3 .. 2e-2 (6,800 to 51,000 times).  At N = 1537,
             entity_dim 768 the rows are peaked and the loss averages 512 of them: it moves by 3e-5 .. 2e-4, only 2 to 20 times its
             tolerance, and the gradient row carries the check there (3e-5 .. 1e-4: 186 to 1,177 times).  The sizes are asserted
             below from a float64 model of the defect, so the claim stays true if the cases change;
  exact      pad columns of dS exactly 0, rows of dS sum to 0 to rounding, two runs the same bits, prefilled gradient buffers end
             as prefill + result, weight of ones = no weight, twice the weight sum halves everything exactly;
  autograd   losses.OneVsAll()(model.score_all(...), target).backward() against the step, with and without the N3 term;
  optimizers optim.Adam(), optim.Adam(lazy_rows=True) behind a pooled step, optim.Adagrad against torch.optim on the step's gradients;
  pipeline   compose.Pipeline.learn with losses.OneVsAll: two epochs, both sides, no negatives drawn, losses against a float64 replica.
"""
import numpy as np
import pytest
import torch

import util_onevsall as U

pytestmark = pytest.mark.gpu


def _model(pb):
    from util_gpu import make_model

    return make_model(pb.model, pb.ent, pb.rel, pb.hidden, 6.0)


def _dev(a, dtype=None):
    t = torch.as_tensor(a)
    return (t if dtype is None else t.to(dtype)).cuda()


def _step(pb, mode, weight="own", weight_sum=None, prefill=None, reg=None, m=None):
    """One OneVsAllStep on a fresh model -> (loss, pos, g_ent, g_rel) as numpy.  prefill: (g_ent, g_rel) device tensors put into .grad."""
    from mkb_amd import fused

    m = _model(pb) if m is None else m
    if prefill is not None:
        m.entity_embedding.grad, m.relation_embedding.grad = prefill[0].clone(), prefill[1].clone()
    w = _dev(pb.weight) if weight == "own" else weight
    step = fused.OneVsAllStep(m, regularizer=reg)
    loss = step(_dev(pb.sample), w, mode, weight_sum=weight_sum)
    torch.cuda.synchronize()
    return (loss.cpu().numpy(), step.positive_score.cpu().numpy()[:, 0], m.entity_embedding.grad.cpu().numpy(),
            m.relation_embedding.grad.cpu().numpy())


def _seeds(pb, m, mode, padded):
    """dS of the row-softmax kernel on the model's own score block; padded: the forward's layout (ld = Npad, the pad columns holding
    the last entity's score again) -> the whole [B, ld] block."""
    from mkb_amd.losses import one_vs_all

    S = m.score_all(_dev(pb.sample), mode).detach()
    pad = (-pb.N) % 4 if padded else 0
    if pad:
        S = torch.cat([S] + [S[:, -1:]] * pad, 1)
    S = S.contiguous().clone()
    one_vs_all.launch(S, pb.N, _dev(pb.target(mode)), 1, _dev(pb.weight), None, 1.0)
    torch.cuda.synchronize()
    return S.cpu().numpy()


def _report(case, mode, got, f64, what):
    """Print error / err_ref and error / tolerance of one quantity, then hold it to the tolerance."""
    _, err = U.expected(case, mode)
    e = float(np.abs(np.asarray(got, dtype=np.float64) - f64[what]).max())
    tol = U.tolerance(case, mode, what)
    print(f"onevsall-error {case[0]} {mode} {what}: error {e:.3e} err_ref {err[what]:.3e} ratio {e / err[what]:.2f} tolerance {tol:.3e} "
          f"term {U.typical_term(case, mode, what):.3e}")
    return e, tol


@pytest.mark.parametrize("case", U.CASES, ids=U.CASE_IDS)
def test_forward_has_the_bits_of_the_evaluation(case):
    from mkb_amd import evaluation

    pb = U.problem(case)
    m = _model(pb).eval()
    ev = evaluation.Evaluation(true_triples=[tuple(t) for t in pb.sample.tolist()], entities={i: i for i in range(pb.N)},
                               relations={i: i for i in range(U.R)}, batch_size=64, device="cuda", num_workers=0)
    for mode in U.MODES:
        _, want = ev.ranks(m, pb.sample, mode, chunk=pb.B, with_scores=True)
        got = m.score_all(_dev(pb.sample), mode)
        assert got.shape == (pb.B, pb.N) and got.requires_grad
        assert torch.equal(got.detach().view(torch.int32), want.view(torch.int32)), (case[0], mode)
        f64, _ = U.expected(case, mode)
        assert np.abs(got.detach().cpu().numpy() - f64["S"]).max() <= 1e-3 * max(1.0, np.abs(f64["S"]).max())  # (the right block at all)


@pytest.mark.parametrize("case", U.CASES, ids=U.CASE_IDS)
def test_step_against_float64_and_the_pad_trap(case):
    pb = U.problem(case)
    failures = []
    for mode in U.MODES:
        f64, _ = U.expected(case, mode)
        loss, pos, g_ent, g_rel = _step(pb, mode)
        dS = _seeds(pb, _model(pb), mode, padded=True)
        assert not dS[:, pb.N:].any(), "pad columns of dS must be exactly 0"
        for what, got in (("loss", loss), ("pos", pos), ("dS", dS[:, :pb.N]), ("g_ent", g_ent), ("g_rel", g_rel)):
            e, tol = _report(case, mode, got, f64, what)
            if not e <= tol:
                failures.append((mode, what, e, tol))
        if pb.N % 4:
            d_loss, d_row = U.pad_trap(case, mode)
            tol_loss, tol_row = U.tolerance(case, mode, "loss"), U.tolerance(case, mode, "g_ent")
            print(f"onevsall-padtrap {case[0]} {mode}: a softmax over the pad columns moves the loss by {d_loss:.3e} ({d_loss / tol_loss:.0f} x "
                  f"tolerance) and the gradient row of entity N - 1 by {d_row:.3e} ({d_row / tol_row:.0f} x tolerance)")
            assert d_row > 100 * tol_row and (pb.N > 1000 or d_loss > 100 * tol_loss), "the case would not show the defect"
            assert abs(float(loss) - float(f64["loss"])) <= tol_loss
            assert np.abs(g_ent[-1] - f64["g_ent"][-1]).max() <= tol_row
    assert not failures, failures


@pytest.mark.parametrize("B", [8192, 8193])
def test_softmax_kernel_on_each_side_of_the_weight_sum_limit(B):
    """mkb_all_softmax on a [B, 130] block of given scores, one batch on each side of the limit up to which every workgroup reduces
    the weight sum itself: weights given, no weight sum, the leading dimension padded as the forward pads it.  Loss, positive scores
    and dS against the float64 formula on those very values within 8 x the float32 formula's own error (at least one float32 ulp of
    the largest magnitude); pad columns of dS exactly 0; two runs give the same loss bits."""
    from mkb_amd.losses import one_vs_all

    N, rs = 130, np.random.RandomState(B)
    S32 = rs.normal(0, 2, size=(B, N)).astype(np.float32)
    target, weight = rs.randint(N, size=B), rs.uniform(0.1, 1.1, size=B).astype(np.float32)
    out = []
    for dtype in (torch.float64, torch.float32):
        S = torch.from_numpy(S32).to(dtype).requires_grad_(True)
        w = torch.from_numpy(weight).to(dtype)
        pos = S[torch.arange(B), torch.from_numpy(target)]
        loss = (w * (torch.logsumexp(S, 1) - pos)).sum() / w.sum()
        loss.backward()
        out.append({"loss": loss.detach().numpy(), "pos": pos.detach().numpy(), "dS": S.grad.numpy()})
    f64, f32 = out
    runs = []
    for _ in range(2):
        block = torch.cat([_dev(S32)] + [_dev(S32[:, -1:])] * ((-N) % 4), 1).contiguous()  # (the pad columns repeat the last entity's score)
        loss, pos = one_vs_all.launch(block, N, _dev(target), 1, _dev(weight), None, 1.0)
        torch.cuda.synchronize()
        runs.append({"loss": loss.cpu().numpy()[0], "pos": pos.cpu().numpy(), "dS": block.cpu().numpy()})
    got = runs[0]
    assert got["dS"].shape[1] == 132 and not got["dS"][:, N:].any(), "pad columns of dS must be exactly 0"
    assert np.float32(got["loss"]).tobytes() == np.float32(runs[1]["loss"]).tobytes()
    failures = []
    for what, g in (("loss", got["loss"]), ("pos", got["pos"]), ("dS", got["dS"][:, :N])):
        err = max(float(np.abs(f32[what].astype(np.float64) - f64[what]).max()), 2.0 ** -24 * float(np.abs(f64[what]).max()))
        e = float(np.abs(np.asarray(g, dtype=np.float64) - f64[what]).max())
        print(f"onevsall-limit B={B} {what}: error {e:.3e} err_ref {err:.3e} ratio {e / err:.2f}")
        if not e <= U.ERR_FACTOR * err:
            failures.append((what, e, U.ERR_FACTOR * err))
    assert not failures, failures


@pytest.mark.parametrize("case", U.CASES, ids=U.CASE_IDS)
def test_checks_that_need_no_tolerance(case):
    pb = U.problem(case)
    mode = U.MODES[U.CASES.index(case) % 2]  # (the sides alternate over the table; the tolerance test runs both on every case)
    dS = _seeds(pb, _model(pb), mode, padded=True)
    assert not dS[:, pb.N:].any()
    row_sums = np.abs(dS.astype(np.float64).sum(1))
    assert (row_sums <= 2.0 ** -22 * np.abs(dS).astype(np.float64).sum(1) + 1e-30).all(), row_sums.max()  # a few ulp per term
    assert np.array_equal(dS, _seeds(pb, _model(pb), mode, padded=True))
    # two runs: the same bits
    first, second = _step(pb, mode), _step(pb, mode)
    for a, b in zip(first, second):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    # prefilled buffers end as prefill + (the result from zero buffers), bit for bit: every gradient element takes the finished
    # result in ONE rounded fp32 addition (a split-K product is reduced first; a query entity's row gets its row of dE and the
    # chain's term together).  The expectation is that same single addition, made on the host.
    g = torch.Generator().manual_seed(7)
    pre = [(torch.rand(shape, generator=g) - 0.5).float().cuda() for shape in (pb.ent.shape, pb.rel.shape)]
    filled = _step(pb, mode, prefill=pre)
    for k in (2, 3):
        want = pre[k - 2].cpu().numpy() + first[k]  # (fp32 + fp32, rounded once: what `+=` on the device does)
        assert np.array_equal(filled[k].view(np.int32), want.view(np.int32)), ("g_ent", "g_rel")[k - 2]
    assert np.array_equal(filled[0].view(np.int32), first[0].view(np.int32))
    # weight of ones = no weight
    ones, none = _step(pb, mode, weight=torch.ones(pb.B, device="cuda")), _step(pb, mode, weight=None)
    for a, b in zip(ones, none):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    # twice the weight sum halves loss and gradients exactly (positive_score stays)
    W = torch.as_tensor(pb.weight).sum().reshape(1).cuda()
    one, two = _step(pb, mode, weight_sum=W), _step(pb, mode, weight_sum=2 * W)
    assert np.array_equal(one[1], two[1])
    for k in (0, 2, 3):
        assert np.array_equal((0.5 * one[k]).view(np.int32), two[k].view(np.int32)), k


@pytest.mark.parametrize("case", U.CASES, ids=U.CASE_IDS)
def test_autograd_route_equals_the_step(case):
    from mkb_amd import losses

    pb = U.problem(case)
    for mode in U.MODES:
        f64, _ = U.expected(case, mode)
        m = _model(pb)
        scores = m.score_all(_dev(pb.sample), mode)
        loss = losses.OneVsAll()(scores, _dev(pb.target(mode)), _dev(pb.weight))
        loss.backward()
        torch.cuda.synchronize()
        step = _step(pb, mode)
        for what, got, ref in (("loss", loss.detach().cpu().numpy(), step[0]), ("g_ent", m.entity_embedding.grad.cpu().numpy(), step[2]),
                               ("g_rel", m.relation_embedding.grad.cpu().numpy(), step[3])):
            e, tol = _report(case, mode, got, f64, what)
            assert e <= tol, (mode, what, e, tol)
            assert np.abs(got.astype(np.float64) - ref).max() <= 2 * tol, (mode, what)  # (each within tol of float64)


@pytest.mark.parametrize("name", ["ragged-complex", "t64-n130-d64", "bf16x3-distmult"])
def test_n3_joins_both_routes(name):
    from mkb_amd import losses, regularizers

    case = U.CASES[U.CASE_IDS.index(name)]
    pb, lam = U.problem(case), 1e-2
    for mode in U.MODES:
        f64, err = U.expected(case, mode, True, lam)
        tol = {k: max(U.tolerance(case, mode, k), U.ERR_FACTOR * err[k]) for k in ("loss", "g_ent", "g_rel")}
        got_step = _step(pb, mode, reg=regularizers.N3(lam))
        m = _model(pb)
        sample, w = _dev(pb.sample), _dev(pb.weight)
        total = losses.OneVsAll()(m.score_all(sample, mode), _dev(pb.target(mode)), w) + regularizers.N3(lam)(m, sample, w)
        total.backward()
        torch.cuda.synchronize()
        got_auto = (total.detach().cpu().numpy(), None, m.entity_embedding.grad.cpu().numpy(), m.relation_embedding.grad.cpu().numpy())
        for label, got in (("step", got_step), ("autograd", got_auto)):
            for k, what, ref in ((0, "loss", f64["total"]), (2, "g_ent", f64["g_ent"]), (3, "g_rel", f64["g_rel"])):
                e = float(np.abs(got[k].astype(np.float64) - ref).max())
                print(f"onevsall-n3 {name} {mode} {label} {what}: error {e:.3e} tolerance {tol[what]:.3e}")
                assert e <= tol[what], (label, mode, what, e, tol[what])


# ---------------------------------------------------------------------------------------------------------------- optimizers
OPT_N, OPT_HIDDEN, OPT_B, OPT_K = 4100, 64, 64, 16  # (4,096 rows or more: the table a row-lazy optimizer attaches to)


def _opt_problem():
    rs = np.random.RandomState(11)
    ent = rs.uniform(-1, 1, size=(OPT_N, OPT_HIDDEN)).astype(np.float32)
    rel = rs.uniform(-1, 1, size=(U.R, OPT_HIDDEN)).astype(np.float32)
    triples = np.stack([rs.randint(OPT_N, size=4 * OPT_B), rs.randint(U.R, size=4 * OPT_B), rs.randint(OPT_N, size=4 * OPT_B)], 1).astype(np.int64)
    return ent, rel, triples


def _three_steps(make_opt, make_ref, pooled_first=False):
    """[one pooled step,] three 1vsAll steps under ``make_opt(params)``; a twin under ``make_ref(params)`` is fed the steps' own
    gradients.  -> (tables, twin's tables, the optimizer)."""
    from mkb_amd import fused, losses, sampling
    from util_gpu import make_model

    ent, rel, triples = _opt_problem()
    m = make_model("DistMult", ent, rel, OPT_HIDDEN, 6.0)
    params = [m.entity_embedding, m.relation_embedding]
    opt = make_opt(params)
    twin = [torch.nn.Parameter(p.detach().clone()) for p in params]
    ref = make_ref(twin)
    t = torch.as_tensor(triples).cuda()
    weight = torch.rand(OPT_B, generator=torch.Generator().manual_seed(3)).cuda() + 0.5
    steps = []
    if pooled_first:
        train = [tuple(int(v) for v in row) for row in triples]
        ns = sampling.NegativeSampling(size=OPT_K, train_triples=train, entities=m.entities, relations=m.relations, seed=1)
        assert fused.pooled_supported(m, OPT_B, OPT_K)
        pooled = fused.PooledLossStep(m, losses.CrossEntropy())
        steps.append(lambda s: pooled.sampled(s, weight, ns, "tail-batch"))
    one = fused.OneVsAllStep(m)
    steps += [lambda s, mode=mode: one(s, weight, mode) for mode in ("tail-batch", "head-batch", "tail-batch")]
    for it, run in enumerate(steps):
        loss = run(t[it * OPT_B: (it + 1) * OPT_B].contiguous())
        assert bool(torch.isfinite(loss))
        for q, p in zip(twin, params):
            q.grad = p.grad.detach().clone()
        opt.step()
        opt.zero_grad()
        ref.step()
        assert all(not p.grad.any() for p in params), it
    if hasattr(opt, "flush"):
        opt.flush()
    torch.cuda.synchronize()
    return params, twin, opt


def test_dense_adam_follows_torch_adam():
    from mkb_amd import optim

    params, twin, _ = _three_steps(lambda ps: optim.Adam(ps, lr=1e-2), lambda ps: torch.optim.Adam(ps, lr=1e-2))
    for p, q in zip(params, twin):  # the equality of the dense route's own test (tests/test_gpu_general.py): a few ulp of the update
        np.testing.assert_allclose(p.detach().cpu().numpy(), q.detach().cpu().numpy(), rtol=0, atol=2e-6)


def test_row_lazy_adam_flushes_and_goes_dense():
    from mkb_amd import _links, optim

    params, twin, opt = _three_steps(lambda ps: optim.Adam(ps, lr=1e-2, lazy_rows=True), lambda ps: torch.optim.Adam(ps, lr=1e-2),
                                     pooled_first=True)
    assert _links.owner(params[0]) is None, "the table should be on the route 'touched rows unknown -> dense'"
    assert opt.state[params[0]]["n"] == 4
    for p, q in zip(params, twin):
        np.testing.assert_allclose(p.detach().cpu().numpy(), q.detach().cpu().numpy(), rtol=0, atol=2e-6)


def test_adagrad_takes_its_all_rows_form_bit_for_bit():
    from mkb_amd import optim

    params, twin, opt = _three_steps(lambda ps: optim.Adagrad(ps, lr=0.1), lambda ps: torch.optim.Adagrad(ps, lr=0.1, foreach=True))
    assert opt.state[params[0]]["n"] == 3
    for p, q in zip(params, twin):  # the equality of tests/test_gpu_adagrad.py: torch's foreach step, bit for bit
        assert torch.equal(p.detach(), q.detach()), f"{int((p != q).sum())} elements differ from torch's foreach step"


# ---------------------------------------------------------------------------------------------------------------- pipeline
def test_pipeline_routes_onevsall_and_draws_no_negatives(monkeypatch):
    from mkb_amd import compose, datasets, fused, losses
    from util_gpu import make_model

    N, hidden, B = 131, 16, 32
    rs = np.random.RandomState(5)
    ent = rs.uniform(-1, 1, size=(N, 2 * hidden)).astype(np.float32)
    rel = rs.uniform(-1, 1, size=(U.R, 2 * hidden)).astype(np.float32)
    train = [(int(h), int(r), int(t)) for h, r, t in zip(rs.randint(N, size=4 * B), rs.randint(U.R, size=4 * B), rs.randint(N, size=4 * B))]
    ents, rels = {i: i for i in range(N)}, {i: i for i in range(U.R)}
    ds = datasets.Dataset(train=train, batch_size=B, entities=ents, relations=rels, shuffle=False, num_workers=0, seed=42)
    m = make_model("ComplEx", ent, rel, hidden, 6.0)

    class NoSampler:
        size = 16

        def generate(self, *args, **kwargs):
            raise AssertionError("the 1vsAll route draws no negatives")

    seen, inner = [], fused.OneVsAllStep.__call__

    def spy(self, sample, weight, mode, weight_sum=None):
        out = inner(self, sample, weight, mode, weight_sum=weight_sum)
        seen.append((sample.cpu().numpy(), weight.cpu().numpy(), mode, float(out)))
        return out

    monkeypatch.setattr(fused.OneVsAllStep, "__call__", spy)
    lr = 0.1
    opt = torch.optim.Adagrad([m.entity_embedding, m.relation_embedding], lr=lr)
    compose.Pipeline(epochs=2, eval_every=100, device="cuda").learn(model=m, dataset=ds, sampling=NoSampler(), optimizer=opt,
                                                                      loss=losses.OneVsAll())
    n_steps = len(seen)
    assert n_steps == 2 * len(ds) and n_steps >= 8
    assert {s[2] for s in seen} == {"head-batch", "tail-batch"}
    # the float64 replica of the same steps: the step's formulas (util_onevsall.compute) and torch's Adagrad rule in float64.  Per step
    # the bound is the tolerance of the other tests -- 8 x the fp32 evaluation's own error at the replica's tables, at least one ulp
    # of the loss -- times the number of steps taken so far: the tables the device holds have drifted by that many steps' errors.
    e64, r64 = torch.from_numpy(ent).double(), torch.from_numpy(rel).double()
    acc = [torch.zeros_like(e64), torch.zeros_like(r64)]
    for k, (sample, weight, mode, got) in enumerate(seen):
        f64 = U.compute("ComplEx", e64, r64, sample, mode, weight)
        f32 = U.compute("ComplEx", e64.float(), r64.float(), sample, mode, weight)
        err_ref = max(abs(float(f32["loss"]) - float(f64["loss"])), 2.0 ** -24 * abs(float(f64["loss"])))
        tol = (k + 1) * U.ERR_FACTOR * err_ref
        e = abs(got - float(f64["loss"]))
        print(f"onevsall-pipeline step {k} {mode}: loss {got:.6f} float64 {float(f64['loss']):.6f} error {e:.3e} tolerance {tol:.3e}")
        assert e <= tol, (k, e, tol)
        for p, a, g in ((e64, acc[0], f64["g_ent"]), (r64, acc[1], f64["g_rel"])):
            g = torch.from_numpy(g)
            a += g * g
            p -= lr * g / (a.sqrt() + 1e-10)
    assert float(seen[-1][3]) < float(seen[0][3])  # it learns
