"""-m gpu: filtered 1vsAll with label smoothing (mkb_amd/csrc/score_all.hip: all_softmax_filtered_kernel; fused.OneVsAllStep and
losses.OneVsAll with label_smoothing / true_triples) on the designed batches of tests/util_onevsall_filtered.py -- no key, the target
the only key, a target that is no key, 1 / 255 / 256 / 257 filtered columns, columns 0 and N - 1 filtered, two rows of one query
filtering each other's target, every column but the target filtered, the owners of the first and the last key -- on both sides.

  kernel     mkb_all_softmax_filtered on an injected float32 block with ld > N, N = 129 / 130 / 131 (LDS staging) and 5000 (re-read
             from memory): loss, pos and dS against float64 on the block's own values within 8 x err_ref (util_onevsall_filtered.bound);
             filtered and pad columns of dS exactly 0, the floats behind the block untouched, two runs the same bits; (eps, T) in
             {(0, 1), (0.1, 1), (0.1, 0.5)}, weights on and off, a given weight sum; one row has a filtered column 1e4 above its
             largest kept score; an n_i = 1 row is all zero;
  target     a target array that is not the sample's open slot: that entity is filtered like any other key;
  stability  scores of +-300 in kept and filtered columns: finite, within the same bound;
  step       OneVsAllStep(label_smoothing, true_triples): loss, positive_score, g_ent, g_rel against float64 on four cases of
             util_onevsall.CASES (lane fallback, fp32 tiles, bf16x3 tiles, rows of 5000), gradients accumulated onto pre-filled
             buffers, two runs the same bits;
  glue       losses.OneVsAll(...)(model.score_all(...), ...) against the step; compose.Pipeline.learn with
             OneVsAll(filter_known=True) filters by its dataset's training triples; OneVsAllStep at its defaults is a direct
             mkb_all_step call bit for bit; the distance models are refused.
"""
import numpy as np
import pytest
import torch

import util_onevsall as U
import util_onevsall_filtered as V

pytestmark = pytest.mark.gpu


def _case(name):
    return U.CASES[U.CASE_IDS.index(name)]


def _model(pb):
    from util_gpu import make_model

    return make_model(pb.model, pb.ent, pb.rel, pb.hidden, 6.0)


def _dev(a, dtype=None):
    t = torch.as_tensor(a)
    return (t if dtype is None else t.to(dtype)).cuda()


def _mode_id(mode):
    from mkb_amd import _hip

    return _hip.mode_id(mode)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


def _held(tag, name, mode, what, got, f64, err, term):
    """Print error / err_ref of one quantity, -> (error, bound)."""
    e = float(np.abs(np.asarray(got, dtype=np.float64) - f64[what]).max())
    tol = V.bound(name, what, err[what], term)
    print(f"onevsall-filtered-error {tag} {name} {mode} {what}: error {e:.3e} err_ref {err[what]:.3e} ratio {e / err[what]:.2f} tolerance {tol:.3e}")
    return e, tol


def _block(S32, N, target, sample, mode, keys, weight, weight_sum, eps, T, guard=64, fill=7.25):
    """mkb_all_softmax_filtered through the C ABI on a [B, ld] block with ld > N inside a larger buffer -> (rc, loss, pos, block, guard
    floats).  The pad columns hold the last entity's score again, as the forward leaves them."""
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
    t, s, k = _dev(np.ascontiguousarray(target)), _dev(sample), _dev(keys)
    w = None if weight is None else _dev(weight)
    W = None if weight_sum is None else _dev(np.float32(weight_sum)).reshape(1)
    rc = _hip.lib().mkb_all_softmax_filtered(_hip.ptr(block), B, N, ld, _hip.ptr(t), 1, _hip.ptr(s), _mode_id(mode), V.R, _hip.ptr(k), k.numel(),
                                             _hip.ptr(w), _hip.ptr(W), T, eps, _hip.ptr(loss), _hip.ptr(pos), _hip.ptr(scratch),
                                             _hip.stream_ptr())
    torch.cuda.synchronize()
    return rc, loss.cpu().numpy()[0], pos.cpu().numpy(), block.cpu().numpy(), buf[B * ld:].cpu().numpy()


# (label smoothing, temperature, weights, a given weight sum as a multiple of the weights' own)
BLOCK_SETTINGS = ((0.0, 1.0, True, None), (0.0, 1.0, False, None), (0.1, 1.0, False, None), (0.1, 1.0, True, 2.0), (0.1, 0.5, True, None),
                  (0.1, 0.5, False, None))
assert {(s[0], s[1]) for s in BLOCK_SETTINGS} == set(V.SETTINGS)
BLOCK_B = 16


def _weights(B):
    return np.random.RandomState(11).uniform(0.5, 1.5, size=B).astype(np.float32)


def _check_block(tag, name, S32, N, sample, mode, keys, weight_all, target=None, settings=BLOCK_SETTINGS):
    failures = []
    target = V.open_slot(sample, mode) if target is None else target
    Fm = V.filtered_mask(sample, mode, keys, N, target)
    for eps, T, weighted, wsum in settings:
        w = weight_all if weighted else None
        W = None if wsum is None else np.float32(wsum * np.float32(weight_all).sum())
        f64, err = V.block_expected(S32, sample, mode, keys, w, W, eps, T, target)
        rc, loss, pos, block, guard = _block(S32, N, target, sample, mode, keys, w, W, eps, T)
        assert rc == 0
        assert np.isfinite(loss) and np.isfinite(block).all()
        assert not block[:, N:].any(), "pad columns of dS must be exactly 0"
        assert (block[:, :N][Fm] == 0.0).all(), "filtered columns of dS must be exactly 0"
        assert (guard == 7.25).all(), "the floats behind the block were written"
        for i in np.flatnonzero(f64["n"] == 1):
            assert not block[i].any(), "a row that keeps its target alone has no gradient"
        again = _block(S32, N, target, sample, mode, keys, w, W, eps, T)
        assert np.array_equal(_bits(loss), _bits(again[1])) and np.array_equal(_bits(block), _bits(again[3]))
        for what, got in (("loss", loss), ("pos", pos), ("dS", block[:, :N])):
            e, tol = _held(f"{tag} eps={eps} T={T} w={int(weighted)} W={wsum}", name, mode, what, got, f64, err,
                           V.typical_term(f64, len(sample), 16, what))
            if not e <= tol:
                failures.append((mode, eps, T, what, e, tol))
    return failures


def _injected(name, N, mode):
    """A seeded float32 block for the batch of ``V.rows(name, BLOCK_B, N, mode)``; the 255-filtered row has one filtered column 1e4
    above its largest kept score."""
    L = V.rows(name, BLOCK_B, N, mode)
    S32 = np.random.RandomState(N).normal(0, 2, size=(BLOCK_B, N)).astype(np.float32)
    Fm = V.filtered_mask(L.sample, mode, L.keys, N)
    i = L.rows["k0"]
    S32[i, np.flatnonzero(Fm[i])[3]] = S32[i, ~Fm[i]].max() + np.float32(1e4)
    return L, S32


@pytest.mark.parametrize("N", [129, 130, 131, 5000])
def test_kernel_on_an_injected_block(N):
    name = f"block-n{N}"
    failures = []
    for mode in U.MODES:
        L, S32 = _injected(name, N, mode)
        failures += _check_block("block", name, S32, N, L.sample, mode, L.keys, _weights(BLOCK_B))
    assert not failures, failures


@pytest.mark.parametrize("N", [131, 5000])
def test_a_target_that_is_not_the_open_slot(N):
    """The sample's open-slot entity is then a key like any other: filtered, unless it is the given target."""
    name = f"block-n{N}"
    for mode in U.MODES:
        L, S32 = _injected(name, N, mode)
        target = (V.open_slot(L.sample, mode) + 1) % N
        i = L.rows["only"]
        assert V.filtered_mask(L.sample, mode, L.keys, N, target)[i, V.open_slot(L.sample, mode)[i]]
        assert not _check_block("target", name, S32, N, L.sample, mode, L.keys, _weights(BLOCK_B), target, ((0.1, 0.5, True, None),))


@pytest.mark.parametrize("N", [131, 5000])
def test_scores_of_300_stay_finite_and_within_tolerance(N):
    name = f"block-n{N}"
    for mode in U.MODES:
        L, S32 = _injected(name, N, mode)
        Fm = V.filtered_mask(L.sample, mode, L.keys, N)
        for row in (L.rows["none"], L.rows["one"], L.rows["k1"], L.rows["k2"], 9):
            kept, filt = np.flatnonzero(~Fm[row]), np.flatnonzero(Fm[row])
            S32[row, kept[0]], S32[row, kept[-1]] = 300.0, -300.0
            if len(filt):
                S32[row, filt[0]] = 300.0
            if len(filt) > 1:
                S32[row, filt[-1]] = -300.0
        assert not _check_block("extreme", name, S32, N, L.sample, mode, L.keys, _weights(BLOCK_B), None, ((0.1, 0.5, True, None), (0.0, 1.0, False, None)))


# ---------------------------------------------------------------------------------------------------------------- the step
def _step(pb, L, mode, eps, T, weight="own", prefill=None):
    """One filtered OneVsAllStep on a fresh model -> (loss, pos, g_ent, g_rel) as numpy.  prefill: (g_ent, g_rel) device tensors put
    into .grad."""
    from mkb_amd import fused

    m = _model(pb)
    if prefill is not None:
        m.entity_embedding.grad, m.relation_embedding.grad = prefill[0].clone(), prefill[1].clone()
    w = _dev(pb.weight) if weight == "own" else weight
    step = fused.OneVsAllStep(m, T, label_smoothing=eps, true_triples=L.triples)
    loss = step(_dev(L.sample), w, mode)
    torch.cuda.synchronize()
    return (loss.cpu().numpy(), step.positive_score.cpu().numpy()[:, 0], m.entity_embedding.grad.cpu().numpy(),
            m.relation_embedding.grad.cpu().numpy())


STEP_SETTINGS = ((0.1, 1.0), (0.1, 0.5))


@pytest.mark.parametrize("name", V.STEP_CASES)
def test_step_against_float64(name):
    case = _case(name)
    pb = U.problem(case)
    de = U.entity_dim(pb.model, pb.hidden)
    failures = []
    for mode in U.MODES:
        L = V.case_rows(case, mode)
        for eps, T in STEP_SETTINGS:
            f64, err = V.expected(case, mode, eps, T)
            got = _step(pb, L, mode, eps, T)
            for what, value in zip(("loss", "pos", "g_ent", "g_rel"), got):
                e, tol = _held(f"step eps={eps} T={T}", name, mode, what, value, f64, err, V.typical_term(f64, pb.B, de, what))
                if not e <= tol:
                    failures.append((mode, eps, T, what, e, tol))
    assert not failures, failures


@pytest.mark.parametrize("name", V.STEP_CASES)
def test_two_runs_have_the_same_bits_and_prefilled_buffers_accumulate(name):
    case = _case(name)
    pb = U.problem(case)
    mode = U.MODES[V.STEP_CASES.index(name) % 2]  # (the sides alternate; the tolerance test runs both on every case)
    L = V.case_rows(case, mode)
    first, second = _step(pb, L, mode, 0.1, 0.5), _step(pb, L, mode, 0.1, 0.5)
    for a, b in zip(first, second):
        assert np.array_equal(_bits(a), _bits(b))
    # every gradient element takes the finished result in ONE rounded fp32 addition: the expectation is that addition, made here
    g = torch.Generator().manual_seed(7)
    pre = [(torch.rand(shape, generator=g) - 0.5).float().cuda() for shape in (pb.ent.shape, pb.rel.shape)]
    filled = _step(pb, L, mode, 0.1, 0.5, prefill=pre)
    for k in (2, 3):
        want = pre[k - 2].cpu().numpy() + first[k]
        assert np.array_equal(_bits(filled[k]), _bits(want)), ("g_ent", "g_rel")[k - 2]
    assert np.array_equal(_bits(filled[0]), _bits(first[0]))


# ---------------------------------------------------------------------------------------------------------------- glue
@pytest.mark.parametrize("name", V.STEP_CASES)
def test_autograd_route_equals_the_step(name):
    from mkb_amd import losses

    case = _case(name)
    pb = U.problem(case)
    de = U.entity_dim(pb.model, pb.hidden)
    eps, T = 0.1, 0.5
    for mode in U.MODES:
        L = V.case_rows(case, mode)
        f64, err = V.expected(case, mode, eps, T)
        m = _model(pb)
        sample, w = _dev(L.sample), _dev(pb.weight)
        loss = losses.OneVsAll(T, eps, True, L.triples)(m.score_all(sample, mode), sample[:, 0 if mode == "head-batch" else 2].contiguous(), w,
                                                        sample=sample, mode=mode, n_relation=V.R)
        loss.backward()
        torch.cuda.synchronize()
        auto = (loss.detach().cpu().numpy(), None, m.entity_embedding.grad.cpu().numpy(), m.relation_embedding.grad.cpu().numpy())
        step = _step(pb, L, mode, eps, T)
        for k, what in ((0, "loss"), (2, "g_ent"), (3, "g_rel")):
            e, tol = _held("autograd", name, mode, what, auto[k], f64, err, V.typical_term(f64, pb.B, de, what))
            assert e <= tol, (mode, what, e, tol)
            assert np.abs(auto[k].astype(np.float64) - step[k]).max() <= 2 * tol, (mode, what)  # (each within tol of float64)


def test_smoothing_alone_needs_no_sample_and_is_torchs_cross_entropy():
    from mkb_amd import losses

    case = _case("t64-n130-d64")
    pb, eps, T = U.problem(case), 0.1, 0.5
    rs = np.random.RandomState(2)
    S32 = rs.normal(0, 2, size=(pb.B, pb.N)).astype(np.float32)
    target = rs.randint(pb.N, size=pb.B)
    sample = np.stack([np.zeros(pb.B, dtype=np.int64)] * 2 + [target], 1)
    f64, err = V.block_expected(S32, sample, "tail-batch", np.zeros(0, dtype=np.int64), None, None, eps, T)
    want = torch.nn.functional.cross_entropy(torch.from_numpy(S32).double() / T, torch.from_numpy(target), label_smoothing=eps)
    assert abs(float(want) - float(f64["loss"])) <= 1e-12
    scores = _dev(S32).requires_grad_(True)
    loss = losses.OneVsAll(T, eps)(scores, _dev(target))
    loss.backward()
    torch.cuda.synchronize()
    for what, got in (("loss", loss.detach().cpu().numpy()), ("dS", scores.grad.cpu().numpy())):
        e, tol = _held("smoothing-alone", case[0], "tail-batch", what, got, f64, err, V.typical_term(f64, pb.B, 16, what))
        assert e <= tol, (what, e, tol)


def test_pipeline_filters_by_the_training_triples_of_its_dataset(monkeypatch):
    from mkb_amd import compose, datasets, fused, losses
    from util_gpu import make_model

    N, hidden, B = 131, 16, 32
    rs = np.random.RandomState(5)
    ent = rs.uniform(-1, 1, size=(N, 2 * hidden)).astype(np.float32)
    rel = rs.uniform(-1, 1, size=(U.R, 2 * hidden)).astype(np.float32)
    # few heads and tails: most queries have several known answers
    train = sorted({(int(h), int(r), int(t)) for h, r, t in zip(rs.randint(12, size=8 * B), rs.randint(U.R, size=8 * B),
                                                                 rs.randint(N - 12, N, size=8 * B))})[: 4 * B]
    assert len(train) == 4 * B
    ents, rels = {i: i for i in range(N)}, {i: i for i in range(U.R)}
    ds = datasets.Dataset(train=train, batch_size=B, entities=ents, relations=rels, shuffle=False, num_workers=0, seed=42)
    m = make_model("ComplEx", ent, rel, hidden, 6.0)

    class NoSampler:
        size = 16

        def generate(self, *args, **kwargs):
            raise AssertionError("the 1vsAll route draws no negatives")

    seen, inner = [], fused.OneVsAllStep.__call__

    def spy(self, sample, weight, mode, weight_sum=None):
        assert self.true_triples is ds.train and self.label_smoothing == 0.1 and self.temperature == 0.5
        out = inner(self, sample, weight, mode, weight_sum=weight_sum)
        seen.append((sample.cpu().numpy(), weight.cpu().numpy(), mode, out.detach().clone()))
        return out

    monkeypatch.setattr(fused.OneVsAllStep, "__call__", spy)
    opt = torch.optim.Adagrad([m.entity_embedding, m.relation_embedding], lr=0.1)
    pipe = compose.Pipeline(epochs=1, eval_every=100, device="cuda")
    pipe.device_batches = True
    pipe.learn(model=m, dataset=ds, sampling=NoSampler(), optimizer=opt, loss=losses.OneVsAll(0.5, 0.1, filter_known=True))
    assert len(seen) >= 4 and {s[2] for s in seen} == {"head-batch", "tail-batch"}
    assert all(np.isfinite(float(s[3])) for s in seen)
    assert float((m.entity_embedding.detach().cpu() - torch.from_numpy(ent)).abs().max()) > 0
    assert float((m.relation_embedding.detach().cpu() - torch.from_numpy(rel)).abs().max()) > 0
    # the first step ran on the untouched tables: its loss is the float64 formula's with THESE triples as keys, and not plain 1vsAll's
    sample, weight, mode, got = seen[0]
    keys = np.sort(np.array([((t * U.R + r) * N + h) if mode == "head-batch" else ((h * U.R + r) * N + t) for h, r, t in train], dtype=np.int64))
    assert V.filtered_mask(sample, mode, keys, N).sum(1).max() > 1
    args = ("ComplEx", torch.from_numpy(ent), torch.from_numpy(rel), sample, mode)
    f64 = V.compute(args[0], args[1].double(), args[2].double(), *args[3:], keys, weight, eps=0.1, T=0.5)
    f32 = V.compute(*args, keys, weight, eps=0.1, T=0.5)
    plain = V.compute(args[0], args[1].double(), args[2].double(), *args[3:], np.zeros(0, dtype=np.int64), weight, eps=0.1, T=0.5)
    tol = V.ERR_FACTOR * max(abs(float(f32["loss"]) - float(f64["loss"])), 2.0 ** -24 * abs(float(f64["loss"])))
    print(f"onevsall-filtered-pipeline first step {mode}: loss {float(got):.6f} float64 {float(f64['loss']):.6f} unfiltered {float(plain['loss']):.6f} tolerance {tol:.3e}")
    assert abs(float(got) - float(f64["loss"])) <= tol < abs(float(plain["loss"]) - float(f64["loss"]))


@pytest.mark.parametrize("name", ["ragged-complex", "long-complex"])
def test_the_default_step_is_a_direct_mkb_all_step_call_bit_for_bit(name):
    from mkb_amd import _hip, fused

    case = _case(name)
    pb = U.problem(case)
    for mode in U.MODES:
        sample, w = _dev(pb.sample), _dev(pb.weight)
        m = _model(pb)
        loss = fused.OneVsAllStep(m)(sample, w, mode)
        m2 = _model(pb)
        gr, ws = fused.grad_buffers(m2), fused._all_workspace(m2, pb.B)
        loss2, pos2 = torch.empty(1, device="cuda"), torch.empty(pb.B, device="cuda")
        rc = _hip.lib().mkb_all_step(m2._tables(), gr, _hip.ptr(sample), _hip.ptr(w), pb.B, _mode_id(mode), 1.0, None, _hip.ptr(loss2),
                                     _hip.ptr(pos2), _hip.ptr(ws), ws.numel(), _hip.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0
        assert np.array_equal(_bits(loss.cpu().numpy()), _bits(loss2.cpu().numpy()[0]))
        for a, b in ((m.entity_embedding.grad, m2.entity_embedding.grad), (m.relation_embedding.grad, m2.relation_embedding.grad)):
            assert np.array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy()))


@pytest.mark.parametrize("name", ["TransE", "RotatE", "pRotatE"])
def test_distance_models_are_refused(name):
    from mkb_amd import _hip, fused, models

    N, hidden, B = 129, 8, 8
    m = getattr(models, name)(hidden_dim=hidden, entities={i: i for i in range(N)}, relations={i: i for i in range(U.R)}, gamma=6.0).cuda()
    with pytest.raises(NotImplementedError, match="OneVsAllStep covers ComplEx and DistMult"):
        fused.OneVsAllStep(m, label_smoothing=0.1, true_triples=[(0, 0, 1)])
    sample = torch.zeros((B, 3), dtype=torch.int64, device="cuda")
    keys = torch.zeros(1, dtype=torch.int64, device="cuda")
    loss, pos = torch.full((1,), 7.25, device="cuda"), torch.full((B,), 7.25, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    ws = ws[(-ws.data_ptr()) % 256:]
    rc = _hip.lib().mkb_all_filtered_step(m._tables(), fused.grad_buffers(m), _hip.ptr(sample), None, B, _hip.MODE_TAIL, _hip.ptr(keys), 1, 1.0,
                                          0.1, None, _hip.ptr(loss), _hip.ptr(pos), _hip.ptr(ws), ws.numel(), _hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == _hip.ERR_UNSUPPORTED
    assert float(loss) == 7.25 and bool((pos == 7.25).all())
