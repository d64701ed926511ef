"""-m gpu: the KvsAll step of ComplEx / DistMult (mkb_amd/csrc/score_all.hip: all_bce_kernel; fused.KvsAllStep, losses.KvsAll)
over the case table of tests/util_onevsall.py -- every kernel family of the three products, the forward's lane fallback, every
N % 4, rows of 5000 columns -- on both sides, with the label sets of tests/util_kvsall.py: no label, one, 255 / 256 / 257, every
entity, columns 0 and N - 1, a shared query, neighbours owning the adjacent keys, the owners of the first and the last key, a target
that is no label.

  kernel     mkb_all_bce on a block with ld > N: loss, pos and dS against float64 on the block's own float32 values within
             8 x err_ref (util_kvsall.bound), pad columns exactly 0, the floats behind the block untouched, two runs the same bits;
             label smoothing 0 and 0.1, both reductions, weights on and off, a given weight sum;
  stability  scores of +-300 in label and non-label columns: finite, within the same bound;
  step       KvsAllStep: loss, positive_score, g_ent, g_rel against float64; for N % 4 != 0 a float64 model of "the forward's pad
             columns entered the row sums" moves the loss by more than its tolerance, so the check tells that defect from rounding;
  exact      two runs the same bits, prefilled gradient buffers end as prefill + result;
  autograd   losses.KvsAll(...)(model.score_all(...), sample, mode, w).backward() against the step, with and without the N3 term;
  own target every row labelled by its own target alone (the products of 1vsAll, another dS);
  pipeline   compose.Pipeline.learn with losses.KvsAll(): two epochs, both sides, no negatives drawn, every batch through KvsAllStep,
             losses against a float64 replica, under optim.Adagrad and optim.Adam(lazy_rows=True);
  refusals   the C ABI answers MKB_ERR_INVALID and leaves block and outputs as they were.
"""
import numpy as np
import pytest
import torch

import util_kvsall as K
import util_onevsall as U

pytestmark = pytest.mark.gpu


def _model(pb):
    from util_gpu import make_model

    return make_model(pb.model, pb.ent, pb.rel, pb.hidden, 6.0)


def _dev(a, dtype=None):
    t = torch.as_tensor(a)
    return (t if dtype is None else t.to(dtype)).cuda()


def _mode_id(mode):
    from mkb_amd import _hip

    return _hip.mode_id(mode)


def _held(tag, name, mode, what, got, f64, err, term):
    """Print error / err_ref of one quantity, -> (error, bound)."""
    e = float(np.abs(np.asarray(got, dtype=np.float64) - f64[what]).max())
    tol = K.bound(name, what, err[what], term)
    print(f"kvsall-error {tag} {name} {mode} {what}: error {e:.3e} err_ref {err[what]:.3e} ratio {e / err[what]:.2f} tolerance {tol:.3e}")
    return e, tol


def _bce_block(S32, N, sample, mode, keys, weight, weight_sum, eps, reduction, guard=64, fill=7.25):
    """mkb_all_bce through the C ABI on a [B, ld] block with ld > N inside a larger buffer -> (rc, loss, pos, block, guard floats).
    The pad columns hold the last entity's score again, as the forward leaves them."""
    from mkb_amd import _hip

    B = S32.shape[0]
    ld = ((N + 3) & ~3) + 4
    buf = torch.full((B * ld + guard,), fill, dtype=torch.float32, device="cuda")
    block = buf[: B * ld].view(B, ld)
    block[:, :N] = _dev(S32)
    block[:, N:] = block[:, N - 1: N]
    loss = torch.full((1,), fill, device="cuda")
    pos = torch.full((B,), fill, device="cuda")
    scratch = torch.empty(B + 1, device="cuda")
    s, k = _dev(sample), _dev(keys)
    w = None if weight is None else _dev(weight)
    W = None if weight_sum is None else _dev(np.float32(weight_sum)).reshape(1)
    rc = _hip.lib().mkb_all_bce(_hip.ptr(block), B, N, ld, _hip.ptr(s), _mode_id(mode), K.R, _hip.ptr(k), k.numel(), _hip.ptr(w), _hip.ptr(W),
                                eps, int(reduction == "sum"), _hip.ptr(loss), _hip.ptr(pos), _hip.ptr(scratch), _hip.stream_ptr())
    torch.cuda.synchronize()
    return rc, loss.cpu().numpy()[0], pos.cpu().numpy(), block.cpu().numpy(), buf[B * ld:].cpu().numpy()


# (label smoothing, reduction, weights, a given weight sum as a multiple of the weights' own)
BLOCK_SETTINGS = ((0.0, "mean", True, None), (0.1, "mean", False, None), (0.0, "sum", False, None), (0.1, "sum", True, 2.0))


def _check_block(tag, name, S32, N, sample, mode, keys, weight_all, de, settings=BLOCK_SETTINGS):
    failures = []
    for eps, reduction, weighted, wsum in settings:
        w = weight_all if weighted else None
        W = None if wsum is None else np.float32(wsum * np.float32(weight_all).sum())
        f64, err = K.block_expected(S32, sample, mode, keys, w, W, eps, reduction)
        rc, loss, pos, block, guard = _bce_block(S32, N, sample, mode, keys, w, W, eps, reduction)
        assert rc == 0
        assert np.isfinite(loss) and np.isfinite(block).all()
        assert not block[:, N:].any(), "pad columns of dS must be exactly 0"
        assert (guard == 7.25).all(), "the floats behind the block were written"
        again = _bce_block(S32, N, sample, mode, keys, w, W, eps, reduction)
        assert np.array_equal(np.float32(loss).view(np.int32), np.float32(again[1]).view(np.int32)) and np.array_equal(block, again[3])
        for what, got in (("loss", loss), ("pos", pos), ("dS", block[:, :N])):
            e, tol = _held(f"{tag} eps={eps} {reduction} w={int(weighted)} W={wsum}", name, mode, what, got, f64, err,
                           K.typical_term(f64, len(sample), de, what))
            if not e <= tol:
                failures.append((mode, eps, reduction, what, e, tol))
    return failures


@pytest.mark.parametrize("case", U.CASES, ids=U.CASE_IDS)
def test_kernel_on_a_block(case):
    pb = U.problem(case)
    failures = []
    for mode in U.MODES:
        L = K.labels(case, mode)
        S32 = K.expected(case, mode)[0]["S"].astype(np.float32)
        failures += _check_block("block", case[0], S32, pb.N, L.sample, mode, L.keys, pb.weight, U.entity_dim(pb.model, pb.hidden))
    assert not failures, failures


@pytest.mark.parametrize("B", [8192, 8193])
def test_kernel_on_a_block_on_each_side_of_the_weight_sum_limit(B):
    """One batch on each side of the limit up to which every workgroup reduces the weight sum itself: the 32-row batch, labels and
    weights of one case repeated cyclically; once with weights and no weight sum, once with a given weight sum."""
    case = U.CASES[U.CASE_IDS.index("t64-n130-d16")]
    pb = U.problem(case)
    rows = np.arange(B) % pb.B
    settings = ((0.1, "mean", True, None), (0.1, "mean", True, 2.0))
    failures = []
    for mode in U.MODES:
        L = K.labels(case, mode)
        S32 = K.expected(case, mode)[0]["S"].astype(np.float32)[rows]
        failures += _check_block(f"limit B={B}", case[0], S32, pb.N, np.asarray(L.sample)[rows], mode, L.keys, np.asarray(pb.weight)[rows],
                                 U.entity_dim(pb.model, pb.hidden), settings)
    assert not failures, failures


def test_scores_of_300_stay_finite_and_within_tolerance():
    case = U.CASES[U.CASE_IDS.index("t64-n131-d16")]
    pb = U.problem(case)
    for mode in U.MODES:
        L = K.labels(case, mode)
        S32 = np.random.RandomState(3).normal(0, 2, size=(pb.B, pb.N)).astype(np.float32)
        Y = K.multi_hot(L.sample, mode, L.keys, pb.N)
        for row in (L.rows["one"], L.rows["k1"], L.rows["edge"], L.rows["all"], 9):
            lab, non = np.flatnonzero(Y[row] == 1), np.flatnonzero(Y[row] == 0)
            S32[row, lab[0]] = 300.0
            if len(lab) > 1:
                S32[row, lab[-1]] = -300.0
            if len(non):
                S32[row, non[0]], S32[row, non[-1]] = 300.0, -300.0
        settings = ((0.1, "mean", True, None), (0.0, "sum", False, None))
        assert not _check_block("extreme", case[0], S32, pb.N, L.sample, mode, L.keys, pb.weight, 16, settings)


def _step(pb, L, mode, eps, reduction, weight="own", prefill=None, reg=None, triples=None, sample=None):
    """One KvsAllStep on a fresh model -> (loss, pos, g_ent, g_rel) as numpy.  prefill: (g_ent, g_rel) device tensors put into .grad."""
    from mkb_amd import fused

    m = _model(pb)
    if prefill is not None:
        m.entity_embedding.grad, m.relation_embedding.grad = prefill[0].clone(), prefill[1].clone()
    w = _dev(pb.weight) if weight == "own" else weight
    step = fused.KvsAllStep(m, L.triples if triples is None else triples, eps, reduction, regularizer=reg)
    loss = step(_dev(L.sample if sample is None else sample), w, mode)
    torch.cuda.synchronize()
    return (loss.cpu().numpy(), step.positive_score.cpu().numpy()[:, 0], m.entity_embedding.grad.cpu().numpy(),
            m.relation_embedding.grad.cpu().numpy())


STEP_SETTINGS = ((0.1, "mean"), (0.0, "sum"))


@pytest.mark.parametrize("case", U.CASES, ids=U.CASE_IDS)
def test_step_against_float64_and_the_pad_trap(case):
    pb = U.problem(case)
    de = U.entity_dim(pb.model, pb.hidden)
    failures = []
    for mode in U.MODES:
        L = K.labels(case, mode)
        for eps, reduction in STEP_SETTINGS:
            f64, err = K.expected(case, mode, eps, reduction)
            got = _step(pb, L, mode, eps, reduction)
            for what, value in zip(("loss", "pos", "g_ent", "g_rel"), got):
                e, tol = _held(f"step eps={eps} {reduction}", case[0], mode, what, value, f64, err, K.typical_term(f64, pb.B, de, what))
                if not e <= tol:
                    failures.append((mode, eps, reduction, what, e, tol))
            if pb.N % 4:
                d_loss, tol_loss = K.pad_trap(case, mode, eps, reduction), K.tolerance(case, mode, "loss", eps, reduction)
                print(f"kvsall-padtrap {case[0]} {mode} eps={eps} {reduction}: pad columns inside the row sums move the loss by {d_loss:.3e} "
                      f"({d_loss / tol_loss:.0f} x tolerance)")
                assert d_loss > tol_loss, "the case would not show the defect"
                assert abs(float(got[0]) - float(f64["loss"])) <= tol_loss
    assert not failures, failures


@pytest.mark.parametrize("case", U.CASES, ids=U.CASE_IDS)
def test_two_runs_have_the_same_bits_and_prefilled_buffers_accumulate(case):
    pb = U.problem(case)
    mode = U.MODES[U.CASES.index(case) % 2]  # (the sides alternate over the table; the tolerance test runs both on every case)
    L = K.labels(case, mode)
    first, second = _step(pb, L, mode, 0.1, "mean"), _step(pb, L, mode, 0.1, "mean")
    for a, b in zip(first, second):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    # every gradient element takes the finished result in ONE rounded fp32 addition: the expectation is that addition, made here
    g = torch.Generator().manual_seed(7)
    pre = [(torch.rand(shape, generator=g) - 0.5).float().cuda() for shape in (pb.ent.shape, pb.rel.shape)]
    filled = _step(pb, L, mode, 0.1, "mean", prefill=pre)
    for k in (2, 3):
        want = pre[k - 2].cpu().numpy() + first[k]
        assert np.array_equal(filled[k].view(np.int32), want.view(np.int32)), ("g_ent", "g_rel")[k - 2]
    assert np.array_equal(filled[0].view(np.int32), first[0].view(np.int32))
    # weight of ones = no weight
    ones, none = _step(pb, L, mode, 0.0, "sum", weight=torch.ones(pb.B, device="cuda")), _step(pb, L, mode, 0.0, "sum", weight=None)
    for a, b in zip(ones, none):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


def _autograd(pb, L, mode, eps, reduction, lam=0.0):
    from mkb_amd import losses, regularizers

    m = _model(pb)
    sample, w = _dev(L.sample), _dev(pb.weight)
    total = losses.KvsAll(L.triples, eps, reduction)(m.score_all(sample, mode), sample, mode, w, n_relation=K.R)
    if lam:
        total = total + regularizers.N3(lam)(m, sample, w)
    total.backward()
    torch.cuda.synchronize()
    return total.detach().cpu().numpy(), None, m.entity_embedding.grad.cpu().numpy(), m.relation_embedding.grad.cpu().numpy()


@pytest.mark.parametrize("case", U.CASES, ids=U.CASE_IDS)
def test_autograd_route_equals_the_step(case):
    pb = U.problem(case)
    de = U.entity_dim(pb.model, pb.hidden)
    eps, reduction = 0.1, "mean"
    for mode in U.MODES:
        L = K.labels(case, mode)
        f64, err = K.expected(case, mode, eps, reduction)
        auto, step = _autograd(pb, L, mode, eps, reduction), _step(pb, L, mode, eps, reduction)
        for k, what in ((0, "loss"), (2, "g_ent"), (3, "g_rel")):
            e, tol = _held("autograd", case[0], mode, what, auto[k], f64, err, K.typical_term(f64, pb.B, de, what))
            assert e <= tol, (mode, what, e, tol)
            assert np.abs(auto[k].astype(np.float64) - step[k]).max() <= 2 * tol, (mode, what)  # (each within tol of float64)


@pytest.mark.parametrize("name", ["ragged-complex", "t64-n130-d64", "bf16x3-distmult"])
def test_n3_joins_both_routes(name):
    from mkb_amd import regularizers

    case = U.CASES[U.CASE_IDS.index(name)]
    pb, lam = U.problem(case), 1e-2
    de = U.entity_dim(pb.model, pb.hidden)
    eps, reduction = 0.1, "mean"
    for mode in U.MODES:
        L = K.labels(case, mode)
        f64, err = K.expected(case, mode, eps, reduction, True, lam)
        f64 = dict(f64, loss=f64["total"])
        err = dict(err, loss=max(err["loss"], 2.0 ** -24 * abs(float(f64["total"]))))
        for label, got in (("step", _step(pb, L, mode, eps, reduction, reg=regularizers.N3(lam))),
                           ("autograd", _autograd(pb, L, mode, eps, reduction, lam))):
            for k, what in ((0, "loss"), (2, "g_ent"), (3, "g_rel")):
                e, tol = _held(f"n3-{label}", name, mode, what, got[k], f64, err, K.typical_term(f64, pb.B, de, what))
                assert e <= tol, (label, mode, what, e, tol)


@pytest.mark.parametrize("name", ["ragged-complex", "t64-n130-d64", "bf16x3-distmult", "long-distmult"])
def test_every_row_labelled_by_its_own_target_alone(name):
    """The batch 1vsAll trains on, as labels: the same three products, another dS."""
    from mkb_amd.losses import kvs_all

    case = U.CASES[U.CASE_IDS.index(name)]
    pb = U.problem(case)
    de = U.entity_dim(pb.model, pb.hidden)
    for mode in U.MODES:
        sample, keys, triples = K.own_target_labels(case, mode)
        f64, f32 = (K.compute(pb.model, torch.from_numpy(pb.ent).to(dt), torch.from_numpy(pb.rel).to(dt), sample, mode, keys, pb.weight)
                    for dt in (torch.float64, torch.float32))
        err = K.err_ref(f64, f32)
        loss, pos, g_ent, g_rel = _step(pb, None, mode, 0.0, "mean", triples=triples, sample=sample)
        dS = _model(pb).score_all(_dev(sample), mode).detach().contiguous().clone()
        kvs_all.launch(dS, pb.N, _dev(sample), _mode_id(mode), K.R, _dev(keys), _dev(pb.weight), None, 0.0, "mean")
        torch.cuda.synchronize()
        for what, got in (("loss", loss), ("pos", pos), ("dS", dS.cpu().numpy()), ("g_ent", g_ent), ("g_rel", g_rel)):
            e, tol = _held("own-target", name, mode, what, got, f64, err, K.typical_term(f64, pb.B, de, what))
            assert e <= tol, (mode, what, e, tol)


# ---------------------------------------------------------------------------------------------------------------- pipeline
def _adagrad64(lr):
    acc = {}

    def update(k, p, g):
        a = acc.setdefault(k, torch.zeros_like(p))
        a += g * g
        p -= lr * g / (a.sqrt() + 1e-10)

    return update


def _adam64(lr, b1=0.9, b2=0.999, eps=1e-8):
    st = {}

    def update(k, p, g):
        s = st.setdefault(k, {"m": torch.zeros_like(p), "v": torch.zeros_like(p), "n": 0})
        s["n"] += 1
        s["m"].mul_(b1).add_(g, alpha=1 - b1)
        s["v"].mul_(b2).add_(g * g, alpha=1 - b2)
        p -= (lr / (1 - b1 ** s["n"])) * s["m"] / ((s["v"] / (1 - b2 ** s["n"])).sqrt() + eps)

    return update


@pytest.mark.parametrize("which", ["adagrad", "lazy-adam"])
def test_pipeline_routes_kvsall_and_draws_no_negatives(monkeypatch, which):
    from mkb_amd import compose, datasets, fused, losses, optim
    from mkb_amd.utils.true_keys import _build
    from util_gpu import make_model

    N, hidden, B = 4100, 16, 32  # (4,096 rows or more: the table a row-lazy optimizer attaches to)
    rs = np.random.RandomState(5)
    ent = rs.uniform(-1, 1, size=(N, 2 * hidden)).astype(np.float32)
    rel = rs.uniform(-1, 1, size=(U.R, 2 * hidden)).astype(np.float32)
    # few heads and tails: most queries have several known answers
    train = sorted({(int(h), int(r), int(t)) for h, r, t in zip(rs.randint(40, size=4 * B + 40), rs.randint(U.R, size=4 * B + 40),
                                                                 rs.randint(N - 40, N, size=4 * B + 40))})[: 4 * B]
    assert len(train) == 4 * B
    ents, rels = {i: i for i in range(N)}, {i: i for i in range(U.R)}
    ds = datasets.Dataset(train=train, batch_size=B, entities=ents, relations=rels, shuffle=False, num_workers=0, seed=42)
    m = make_model("ComplEx", ent, rel, hidden, 6.0)

    class NoSampler:
        size = 16

        def generate(self, *args, **kwargs):
            raise AssertionError("the KvsAll route draws no negatives")

    seen, inner = [], fused.KvsAllStep.__call__

    def spy(self, sample, weight, mode, weight_sum=None):
        assert type(self) is fused.KvsAllStep and self.true_triples is ds.train
        out = inner(self, sample, weight, mode, weight_sum=weight_sum)
        seen.append((sample.cpu().numpy(), weight.cpu().numpy(), mode, float(out)))
        return out

    monkeypatch.setattr(fused.KvsAllStep, "__call__", spy)
    params = [m.entity_embedding, m.relation_embedding]
    eps, lr = 0.1, {"adagrad": 0.1, "lazy-adam": 1e-3}[which]
    opt = optim.Adagrad(params, lr=lr) if which == "adagrad" else optim.Adam(params, lr=lr, lazy_rows=True)
    update = _adagrad64(lr) if which == "adagrad" else _adam64(lr)
    compose.Pipeline(epochs=2, eval_every=100, device="cuda").learn(model=m, dataset=ds, sampling=NoSampler(), optimizer=opt,
                                                                      loss=losses.KvsAll(label_smoothing=eps, reduction="sum"))
    n_steps = len(seen)
    assert n_steps == 2 * len(ds) and n_steps >= 8
    assert {s[2] for s in seen} == {"head-batch", "tail-batch"}
    # the float64 replica of the same steps: util_kvsall.compute and the optimizer's rule in float64.  Per step the bound is 8 x the
    # fp32 evaluation's own error at the replica's tables, at least one ulp of the loss, times the number of steps taken so far: the
    # tables the device holds have drifted by that many steps' errors.
    keys = {mode: k.numpy() for mode, k in _build(ds.train, "cpu", N, U.R).items()}
    assert max(K.multi_hot(seen[0][0], seen[0][2], keys[seen[0][2]], N).sum(1)) > 1  # (multi-label rows)
    e64, r64 = torch.from_numpy(ent).double(), torch.from_numpy(rel).double()
    for k, (sample, weight, mode, got) in enumerate(seen):
        f64 = K.compute("ComplEx", e64, r64, sample, mode, keys[mode], weight, eps=eps, reduction="sum")
        f32 = K.compute("ComplEx", e64.float(), r64.float(), sample, mode, keys[mode], weight, eps=eps, reduction="sum")
        err_ref = max(abs(float(f32["loss"]) - float(f64["loss"])), 2.0 ** -24 * abs(float(f64["loss"])))
        tol = (k + 1) * K.ERR_FACTOR * err_ref
        e = abs(got - float(f64["loss"]))
        print(f"kvsall-pipeline {which} step {k} {mode}: loss {got:.6f} float64 {float(f64['loss']):.6f} error {e:.3e} tolerance {tol:.3e}")
        assert e <= tol, (k, e, tol)
        update("ent", e64, torch.from_numpy(f64["g_ent"]))
        update("rel", r64, torch.from_numpy(f64["g_rel"]))
    assert float(seen[-1][3]) < float(seen[0][3])  # it learns


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_block_and_outputs_untouched():
    from mkb_amd import _hip, fused

    case = U.CASES[U.CASE_IDS.index("t64-n129-d16")]
    pb, mode = U.problem(case), "tail-batch"
    L = K.labels(case, mode)
    lib, B, N, ld = _hip.lib(), pb.B, pb.N, 132
    S = torch.full((B, ld), 1.5, device="cuda")
    loss, pos, scratch = torch.full((1,), 7.25, device="cuda"), torch.full((B,), 7.25, device="cuda"), torch.zeros(B + 1, device="cuda")
    sample, keys = _dev(L.sample), _dev(L.keys)
    names = (("S", _hip.ptr(S)), ("B", B), ("N", N), ("ld", ld), ("sample", _hip.ptr(sample)), ("mode", _hip.MODE_TAIL), ("R", K.R),
             ("keys", _hip.ptr(keys)), ("n_keys", keys.numel()), ("weight", None), ("wsum", None), ("eps", 0.1), ("sum", 0),
             ("loss", _hip.ptr(loss)), ("pos", _hip.ptr(pos)), ("scratch", _hip.ptr(scratch)), ("stream", _hip.stream_ptr()))
    for bad in (dict(S=None), dict(sample=None), dict(scratch=None), dict(keys=None), dict(n_keys=-1), dict(eps=-0.01), dict(eps=1.0),
                dict(eps=float("nan")), dict(eps=float("inf")), dict(mode=_hip.MODE_DEFAULT), dict(B=0), dict(N=0), dict(ld=N - 1), dict(R=0),
                dict(B=1, N=(1 << 31) - 1, ld=(1 << 31) - 1, R=1 << 31)):
        assert lib.mkb_all_bce(*[bad.get(k, d) for k, d in names]) == _hip.ERR_INVALID, bad
    m = _model(pb)
    gr, ws = fused.grad_buffers(m), fused._all_workspace(m, B)
    step = lambda **kw: lib.mkb_all_kvs_step(kw.get("tb", m._tables()), kw.get("gr", gr), kw.get("sample", _hip.ptr(sample)), None, kw.get("B", B),
                                             kw.get("mode", _hip.MODE_TAIL), kw.get("keys", _hip.ptr(keys)), kw.get("n_keys", keys.numel()),
                                             kw.get("eps", 0.1), 0, None, _hip.ptr(loss), _hip.ptr(pos), kw.get("ws", _hip.ptr(ws)),
                                             kw.get("nb", ws.numel()), _hip.stream_ptr())
    for bad in (dict(tb=None), dict(gr=None), dict(sample=None), dict(B=0), dict(mode=_hip.MODE_DEFAULT), dict(keys=None), dict(n_keys=-1),
                dict(eps=1.0), dict(eps=float("nan")), dict(ws=None), dict(nb=ws.numel() - 1)):
        assert step(**bad) == _hip.ERR_INVALID, bad
    torch.cuda.synchronize()
    assert bool((S == 1.5).all()) and float(loss) == 7.25 and bool((pos == 7.25).all())
    assert not m.entity_embedding.grad.any() and not m.relation_embedding.grad.any()
    assert step() == 0 and bool(torch.isfinite(loss).all())  # (the same arguments, none of them bad)
