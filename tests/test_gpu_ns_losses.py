"""-m gpu tests of the negative-sampling loss family: mkb_ns_loss against the float64 reference of tests/util_ns_losses.py at its
launch edges, its multiplicities, its run-to-run bits; fused.PooledLossStep against the explicit autograd sequence, under the
row-lazy optimizer, and as compose.Pipeline's route.

Bounds (the project's own): loss |got - ref| <= 1e-5 + 1e-5 |ref| (the atol=1e-5 of tests/test_gpu_general.py); gradients
util_gpu.grad_close.  Every figure is printed as a fraction of its bound before it is asserted (pytest -s shows them).

Shapes (B, K) of the kernel tests sit just past: the 4 rows of a workgroup, the 64-column group, the 256-lane weight tree and its
four-stride (1024-row) loop, the 1024-column LDS staging limit -- the edges mkb_adversarial has too.  The edges the new kernel
itself introduces: exactly AT the staging limit (1023 / 1024 / 1025 columns: the last staged row fills the LDS block to its last
word) and the 8192-row limit up to which every workgroup reduces the weight sum itself (8192 / 8193 rows)."""
import numpy as np
import pytest
import torch

import util_ns_losses as un
from util_gpu import grad_close, make_model, random_problem

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (4, 63), (5, 64), (5, 65), (257, 1), (257, 300), (1030, 65), (3, 1100),
          (3, 1023), (5, 1024), (3, 1025),  # the LDS staging limit itself
          (8192, 3), (8193, 3)]             # the limit of the in-kernel weight sum
KINDS = [("margin", 6.0, 0.0), ("margin", 1.0, 0.5), ("pairwise", 0.0, 0.0), ("pairwise", 2.0, 1.0), ("softmax", 1.0, 0.0),
         ("softmax", 0.5, 0.0)]
PAD = 97  # floats behind every output buffer that the kernel must leave alone


def draw(B, K, seed, kind, param):
    """Scores N(0, 4^2) clamped to +-20, weights uniform in [0.1, 1.1); margin: every neg whose a_ij lies within 1e-3 of the
    kink is moved by 4e-3 (nothing is left out of the comparison)."""
    g = torch.Generator().manual_seed(seed)
    pos = (torch.randn(B, generator=g) * 4).clamp(-20, 20)
    neg = (torch.randn(B, K, generator=g) * 4).clamp(-20, 20)
    w = torch.rand(B, generator=g) + 0.1
    if kind == "margin":
        a = param + neg.double() - pos.double().view(B, 1)
        neg = torch.where(a.abs() < 1e-3, neg + 4e-3, neg)
        assert float((param + neg.double() - pos.double().view(B, 1)).abs().min()) > 1e-3
    return pos, neg, w


def run_kernel(kind, pos, neg, w, cnt, param, alpha, weight_sum):
    """mkb_ns_loss on over-long, NaN-filled outputs -> (loss, dpos, dneg) numpy; asserts that nothing past the outputs was written."""
    from mkb_amd import _hip

    B, K = neg.shape
    dev = "cuda"
    posd, negd = pos.to(dev).float().contiguous(), neg.to(dev).float().contiguous()
    wd = None if w is None else w.to(dev).float().contiguous()
    cd = None if cnt is None else torch.as_tensor(np.asarray(cnt).astype(np.int32)).to(dev).to(torch.uint16).contiguous()
    wsd = None if weight_sum is None else torch.tensor([weight_sum], dtype=torch.float32, device=dev)
    nan = float("nan")
    loss = torch.full((1 + PAD,), nan, device=dev)
    dpos = torch.full((B + PAD,), nan, device=dev)
    dneg = torch.full((B * K + PAD,), nan, device=dev)
    scratch = torch.full((B + 1 + PAD,), nan, device=dev)
    _hip.check(_hip.lib().mkb_ns_loss(un.KINDS[kind], _hip.ptr(posd), _hip.ptr(negd), _hip.ptr(wd), _hip.ptr(cd), B, K, param, alpha,
                                      _hip.ptr(wsd), _hip.ptr(loss), _hip.ptr(dpos), _hip.ptr(dneg), _hip.ptr(scratch),
                                      _hip.stream_ptr()), "mkb_ns_loss")
    torch.cuda.synchronize()
    for name, buf, n in (("loss", loss, 1), ("dpos", dpos, B), ("dneg", dneg, B * K), ("scratch", scratch, B + 1)):
        assert bool(torch.isnan(buf[n:]).all()), f"{name}: written past its {n} floats"
    return float(loss[0]), dpos[:B].cpu().numpy(), dneg[: B * K].view(B, K).cpu().numpy()


def fractions(got, ref):
    """(loss, dpos, dneg) pairs -> the largest error as a fraction of each bound."""
    def grad_fraction(a, b):
        atol = min(1e-5, 2e-4 * max(float(np.abs(b).max()), 1e-30))
        return float(np.abs(a - b).max()) / atol

    return (abs(got[0] - ref[0]) / (1e-5 + 1e-5 * abs(ref[0])), grad_fraction(got[1], ref[1]), grad_fraction(got[2], ref[2]))


def check(got, ref, what):
    fr = fractions(got, ref)
    print("ns_loss fraction of bound", what, "loss %.4f dpos %.4f dneg %.4f" % fr)
    assert np.isfinite(got[0]) and np.isfinite(got[1]).all() and np.isfinite(got[2]).all(), what
    assert abs(got[0] - ref[0]) <= 1e-5 + 1e-5 * abs(ref[0]), (what, got[0], ref[0])
    grad_close(got[1], ref[1])
    grad_close(got[2], ref[2])
    return fr


@pytest.mark.parametrize("kind,param,alpha", KINDS)
@pytest.mark.parametrize("B,K", SHAPES)
def test_kernel_against_float64(B, K, kind, param, alpha):
    pos, neg, w = draw(B, K, 1000 + 7 * B + K, kind, param)
    for with_w in (True, False):
        for weight_sum in (None, 1.37 * float(w.sum()) if with_w else 1.37 * B):
            ref = un.reference(un.KINDS[kind], pos, neg, w if with_w else None, None, param, alpha, weight_sum)
            got = run_kernel(kind, pos, neg, w if with_w else None, None, param, alpha, weight_sum)
            check(got, ref, (kind, param, alpha, B, K, with_w, weight_sum is not None))


@pytest.mark.parametrize("kind,param,alpha", KINDS)
@pytest.mark.parametrize("B,K", [(2, 1), (5, 65), (6, 64), (9, 130), (3, 1100)])
def test_multiplicities_are_repeated_columns_and_unused_positions_take_no_part(B, K, kind, param, alpha):
    pos, neg, w = draw(B, K, 2000 + 7 * B + K, kind, param)
    rs = np.random.RandomState(B * 1000 + K)
    cnt = rs.randint(0, 4, size=(B, K))
    cnt[B // 2] = 0  # one row uses no position
    if B > 2:
        cnt[0, :] = 0
        cnt[0, K - 1] = 3  # and one row a single position, its last
    neg = torch.where(torch.as_tensor(cnt) > 0, neg, torch.full_like(neg, float("nan")))
    W = float(w.double().sum())
    # the reference: every row written out with repeated columns
    loss_ref, dpos_ref, dneg_ref = 0.0, np.zeros(B), np.zeros((B, K))
    for i in range(B):
        cols = np.repeat(np.arange(K), cnt[i])
        li, dp, dn = un.reference(un.KINDS[kind], pos[i:i + 1], un.expand_row(neg[i].numpy(), cnt[i])[None, :], w[i:i + 1], None,
                                  param, alpha, W)
        loss_ref += li
        dpos_ref[i] = dp[0]
        np.add.at(dneg_ref[i], cols, dn[0])
    got = run_kernel(kind, pos, neg, w, cnt, param, alpha, None)
    check(got, (loss_ref, dpos_ref, dneg_ref), (kind, param, alpha, B, K, "cnt"))
    assert not got[2][cnt == 0].any(), "dneg must be exactly 0 where the multiplicity is 0"
    assert got[1][B // 2] == 0.0 and not got[2][B // 2].any()
    # and the reference's own multiplicity form agrees with the written-out rows
    direct = un.reference(un.KINDS[kind], pos, neg, w, cnt, param, alpha, None)
    assert direct[0] == pytest.approx(loss_ref, abs=1e-12)
    np.testing.assert_allclose(direct[2], dneg_ref, atol=1e-12)


@pytest.mark.parametrize("kind,param,alpha", [KINDS[1], KINDS[3], KINDS[5]])
def test_two_runs_give_the_same_bits(kind, param, alpha):
    for B, K in ((1030, 65), (3, 1100), (8193, 3)):
        pos, neg, w = draw(B, K, 3000 + B, kind, param)
        cnt = np.random.RandomState(B).randint(0, 4, size=(B, K))
        a = run_kernel(kind, pos, neg, w, cnt, param, alpha, None)
        b = run_kernel(kind, pos, neg, w, cnt, param, alpha, None)
        assert np.float32(a[0]).tobytes() == np.float32(b[0]).tobytes()
        assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


@pytest.mark.parametrize("B,K", SHAPES[-2:])
def test_adversarial_on_each_side_of_the_weight_sum_limit(B, K):
    """losses.Adversarial shares the limit up to which every workgroup reduces the weight sum itself: one batch on each side of it,
    weights given, against the float64 formula (reference mkb/losses/adversarial.py) with ``check``'s bounds; two runs give the
    same loss bits."""
    from mkb_amd import losses

    alpha = 0.5
    pos, neg, w = draw(B, K, 4000 + B, "adversarial", alpha)
    p64, n64, w64 = pos.double().requires_grad_(True), neg.double().requires_grad_(True), w.double()
    logsig = torch.nn.functional.logsigmoid
    ns = (torch.softmax(alpha * n64, 1).detach() * logsig(-n64)).sum(1)
    ref = (-(w64 * logsig(p64)).sum() / w64.sum() - (w64 * ns).sum() / w64.sum()) / 2
    ref.backward()
    runs = []
    for _ in range(2):
        pd, nd = pos.cuda().view(B, 1).requires_grad_(True), neg.cuda().requires_grad_(True)
        loss = losses.Adversarial(alpha)(pd, nd, w.cuda())
        loss.backward()
        runs.append((float(loss), pd.grad.cpu().numpy()[:, 0], nd.grad.cpu().numpy()))
    check(runs[0], (float(ref), p64.grad.numpy(), n64.grad.numpy()), ("adversarial", alpha, B, K))
    assert np.float32(runs[0][0]).tobytes() == np.float32(runs[1][0]).tobytes()


def _loss_object(kind, param, alpha):
    from mkb_amd import losses

    if kind == "margin":
        return losses.MarginRanking(margin=param, alpha=alpha)
    if kind == "pairwise":
        return losses.PairwiseLogistic(margin=param, alpha=alpha)
    return losses.CrossEntropy(temperature=param)


@pytest.mark.parametrize("kind,param,alpha", KINDS)
def test_classes_are_differentiable_in_both_scores(kind, param, alpha):
    """The autograd.Function around the kernel: loss and both gradients (scaled by an upstream factor) against float64; weight
    absent = all ones; an empty batch answers as Adversarial does (nan, no launch)."""
    from mkb_amd import losses

    B, K = 37, 70
    pos, neg, w = draw(B, K, 4000, kind, param)
    loss = _loss_object(kind, param, alpha)
    for weight in (w, None):
        p = pos.view(B, 1).cuda().requires_grad_()
        n = neg.cuda().requires_grad_()
        out = loss(p, n, None if weight is None else weight.cuda())
        assert out.dim() == 0
        (3.0 * out).backward()
        ref = un.reference(un.KINDS[kind], pos, neg, weight, None, param, alpha)
        check((float(out.detach()), p.grad.view(-1).cpu().numpy() / 3.0, n.grad.cpu().numpy() / 3.0), ref, (kind, "class", weight is not None))
    empty = loss(torch.zeros(0, 1, device="cuda"), torch.zeros(0, K, device="cuda"), torch.zeros(0, device="cuda"))
    want = losses.Adversarial(0.5)(torch.zeros(0, 1, device="cuda"), torch.zeros(0, K, device="cuda"), torch.zeros(0, device="cuda"))
    assert empty.shape == want.shape and bool(torch.isnan(empty)) == bool(torch.isnan(want))


# ---------------------------------------------------------------------------------------------------- the pooled step
N_ENT, N_REL, HIDDEN, BATCH, SIZE = 203, 5, 20, 37, 16


def _problem(name, n_entity=N_ENT, seed=11):
    from mkb_amd import sampling

    ent, rel, _, _, w, modulus = random_problem(name, n_entity, N_REL, HIDDEN, BATCH, SIZE, seed)
    rs = np.random.RandomState(seed)
    train = np.unique(np.stack([rs.randint(n_entity, size=600), rs.randint(N_REL, size=600), rs.randint(n_entity, size=600)], 1), axis=0)
    rs.shuffle(train)
    ents, rels = {i: i for i in range(n_entity)}, {i: i for i in range(N_REL)}

    def sampler():
        return sampling.NegativeSampling(size=SIZE, train_triples=[tuple(int(x) for x in t) for t in train], entities=ents,
                                         relations=rels, seed=3)

    def model():
        return make_model(name, ent, rel, HIDDEN, 6.0, modulus)

    return model, sampler, torch.as_tensor(train).cuda(), w.cuda()


def _grads(m):
    out = [m.entity_embedding.grad, m.relation_embedding.grad]
    if m.name == "pRotatE":
        out.append(m.modulus.grad)
    return [g.detach().cpu().numpy().copy() for g in out]


@pytest.mark.parametrize("kind,param,alpha", [KINDS[0], KINDS[1], KINDS[3], KINDS[4]])
@pytest.mark.parametrize("mode", ["head-batch", "tail-batch"])
@pytest.mark.parametrize("name", ["TransE", "RotatE", "ComplEx", "DistMult", "pRotatE"])
def test_pooled_step_equals_the_explicit_autograd_sequence(name, mode, kind, param, alpha):
    """One PooledLossStep call against the explicit autograd sequence with the same loss object: loss, scores, and .grad of both
    tables and of pRotatE's modulus (grad_close).  Both sides are float32 with float atomics in the backward kernels.

    The softmax runs at T = 1, not at the kernel tests' second temperature 0.5 (which is checked against float64 there).
    grad_close's bound on pRotatE's modulus is an absolute 1e-5 on a scalar that sums B (2K + 1) terms whose negative and
    positive totals cancel (the seeds of a row sum to zero): each total is ~ (1 / T) * sum_d |sin| ~ 26 at T = 0.5, where one
    float32 ulp is 1.9e-6, so the bound is 5 ulps of the running totals of BOTH routes; at T = 1 it is 10.  Measured at
    T = 0.5, tail-batch, in three runs: 1.06 of the bound (with the positives added onto the negatives' total; PooledLossStep
    now sums each backward call's from zero, as autograd does), then 0.38 and 0.76: noise of the order of the bound."""
    from mkb_amd.fused import PooledLossStep

    model, sampler, train, w = _problem(name)
    sample = train[:BATCH].contiguous()
    negatives = sampler().generate(sample, mode)
    # the explicit sequence (compose.Pipeline's, with the same loss object)
    me = model()
    pos = me(sample)
    neg = me(sample=sample, negative_sample=negatives, mode=mode)
    if kind == "margin":  # step the margin until no a_ij of the explicit route lies within 1e-3 of the kink
        a = neg.detach().double() - pos.detach().double()
        for _ in range(1000):
            if float((param + a).abs().min()) > 1e-3:
                break
            param += 0.01
        assert float((param + a).abs().min()) > 1e-3
    loss = _loss_object(kind, param, alpha)
    want = loss(pos, neg, w)
    want.backward()
    # the pooled step
    mp = model()
    step = PooledLossStep(mp, loss)
    got = step(sample, w, negatives, mode)
    torch.cuda.synchronize()
    print("pooled step", name, mode, kind, "loss", float(got), float(want.detach()))
    want_value = float(want.detach())
    assert abs(float(got) - want_value) <= 1e-5 + 1e-5 * abs(want_value)
    np.testing.assert_allclose(step.positive_score.cpu().numpy(), pos.detach().cpu().numpy(), rtol=0, atol=1e-5)
    np.testing.assert_allclose(step.negative_score.cpu().numpy(), neg.detach().cpu().numpy(), rtol=0, atol=1e-5)
    pairs = list(zip(("entity", "relation", "modulus"), _grads(mp), _grads(me)))
    for what, g, r in pairs:
        atol = min(1e-5, 2e-4 * float(np.abs(r).max()))
        print("pooled step fraction of bound", name, mode, kind, what, "%.4f" % (float(np.abs(g - r).max()) / atol))
    for what, g, r in pairs:
        assert np.abs(r).max() > 0, what
        grad_close(g, r)


def _six_steps(name, loss, lazy):
    """Six PooledLossStep steps on a 4096-row entity table (the smallest that steps row-lazily) -> the two tables."""
    from mkb_amd import _links, optim
    from mkb_amd.fused import PooledLossStep

    model, sampler, train, w = _problem(name, n_entity=4096, seed=13)
    m, ns = model(), sampler()
    params = [m.entity_embedding, m.relation_embedding]
    opt = optim.Adam(params, lr=1e-3, lazy_rows=True) if lazy else torch.optim.Adam(params, lr=1e-3)
    assert (_links.owner(m.entity_embedding) is opt) == lazy
    step = PooledLossStep(m, loss)
    for it in range(6):
        s = train[it * BATCH:(it + 1) * BATCH].contiguous()
        step.sampled(s, w, ns, "head-batch" if it % 2 else "tail-batch")
        opt.step()
        opt.zero_grad()
    if lazy:
        opt.flush()
    torch.cuda.synchronize()
    return m.entity_embedding.detach().cpu().numpy(), m.relation_embedding.detach().cpu().numpy()


@pytest.mark.parametrize("kind,param,alpha", [KINDS[1], KINDS[3], KINDS[5]])
def test_pooled_step_under_the_row_lazy_optimizer_equals_dense_adam(kind, param, alpha):
    """Six steps with mkb_amd.optim.Adam(lazy_rows=True) against the same steps with dense torch.optim.Adam: equal to atol 2e-6,
    the bound tests/test_gpu_general.py uses for this comparison.

    The model is DistMult.  With these losses the seeds of a row sum to zero (dpos_i = -sum_j dneg_ij), and TransE's L1 gradient
    is +-seed per element: wherever every pair of a row agrees in sign, the exact gradient element is 0 and the order of the
    float atomics decides between 0 and +-1e-9 -- which Adam's m / sqrt(v) turns into a step of +-lr, so two runs of the SAME
    code differ there (measured with this set-up, margin (1, 0.5): dense Adam against dense Adam 1.2e-4 in 20 elements of
    81920; row-lazy against dense 6e-4 in ~50; RotatE, ComplEx, DistMult and pRotatE: at most 1.2e-7 in both comparisons).
    A product gradient (seed * r * t) has no such exact cancellations, and the comparison is about the protocol, not the
    model.  Observed for DistMult: 3e-8 on both tables."""
    loss = _loss_object(kind, param, alpha)
    (ea, ra), (eb, rb) = _six_steps("DistMult", loss, True), _six_steps("DistMult", loss, False)
    print("row-lazy vs dense: max |d ent| %.3g, max |d rel| %.3g" % (np.abs(ea - eb).max(), np.abs(ra - rb).max()))
    np.testing.assert_allclose(ea, eb, rtol=0, atol=2e-6)
    np.testing.assert_allclose(ra, rb, rtol=0, atol=2e-6)


@pytest.mark.parametrize("kind,param,alpha", [KINDS[0], KINDS[2], KINDS[4]])
def test_pipeline_takes_the_pooled_step_and_the_loss_falls(kind, param, alpha, monkeypatch, capsys):
    """Pipeline.learn on CountriesS1, two epochs: every (model, loss) cell is routed to PooledLossStep
    (profiles/r17_loss_family_speed.txt), the loss stays finite and the second epoch's mean is below the first's."""
    from mkb_amd import compose, datasets, evaluation, fused, models, sampling

    seen = []
    inner = fused.PooledLossStep.__call__

    def spy(self, *args, **kwargs):
        out = inner(self, *args, **kwargs)
        seen.append(out.detach())
        return out

    monkeypatch.setattr(fused.PooledLossStep, "__call__", spy)
    ds = datasets.CountriesS1(batch_size=64, shuffle=False, seed=42, num_workers=0)
    torch.manual_seed(5)
    m = models.TransE(hidden_dim=20, entities=ds.entities, relations=ds.relations, gamma=6.0).cuda()
    ns = sampling.NegativeSampling(size=16, train_triples=ds.train, entities=ds.entities, relations=ds.relations, seed=42)
    opt = torch.optim.Adam([m.entity_embedding, m.relation_embedding], lr=2e-2)
    pipe = compose.Pipeline(epochs=2, eval_every=100, device="cuda")
    loss = _loss_object(kind, param, alpha)
    assert type(pipe._fused_step_for(m, ds, ns, opt, loss)) is fused.PooledLossStep
    pipe.learn(model=m, dataset=ds, sampling=ns, optimizer=opt, loss=loss,
               evaluation=evaluation.Evaluation(true_triples=ds.true_triples, entities=ds.entities, relations=ds.relations,
                                                batch_size=64, device="cuda"))
    values = torch.stack(seen).cpu().numpy()
    assert len(values) >= 4 and len(values) % 2 == 0 and np.isfinite(values).all()
    first, second = values[: len(values) // 2].mean(), values[len(values) // 2:].mean()
    print("pipeline", kind, "epoch means", first, second)
    assert second < first
