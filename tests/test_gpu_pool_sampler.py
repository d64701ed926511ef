"""-m gpu tests of the pool samplers: mkb_pool_filter and mkb_pool_draw_alias against the numpy restatement of
tests/util_pool_sampler.py (bytes, not tolerances: both are integer arithmetic), the three samplers through the fused steps against
the general kernels, and compose.Pipeline's route.

Shapes of the filter: 2K = 2, 6, 64 (exactly one wave), 66, 1024 (the last size with four rows per workgroup) and 2048 (the
largest, one row per workgroup); B = 1, 5 and 257 (more than one workgroup, a last workgroup with idle waves); 37 and 14,541
entities.  The rows made on purpose are util_pool_sampler.filter_fixture's."""
import numpy as np
import pytest
import torch

import util_pool_sampler as up
from util_gpu import grad_close, make_model, random_problem

pytestmark = pytest.mark.gpu

R = 5
PAD = 64  # elements behind every output that the kernels must leave alone


def _padded(n, dtype, fill):
    return torch.full((n + PAD,), fill, dtype=dtype, device="cuda")


def run_filter(sample, mode_id, N, pool, K, keys, outputs=(True, True, True), status=None):
    """mkb_pool_filter on over-long outputs -> (rc, neg, pos, cnt, touched, status) as numpy (None for an output not asked for);
    asserts that nothing behind an output was written."""
    from mkb_amd import _hip

    B = len(sample)
    s = torch.as_tensor(np.ascontiguousarray(sample, dtype=np.int64)).cuda()
    p = torch.as_tensor(np.ascontiguousarray(pool, dtype=np.int64)).cuda()
    k = None if keys is None else torch.as_tensor(np.ascontiguousarray(keys, dtype=np.int64)).cuda()
    neg = _padded(B * K, torch.int64, -7)
    pos = _padded(B * K, torch.int32, -7) if outputs[0] else None
    cnt = _padded(B * 2 * K, torch.int16, -7) if outputs[1] else None  # (uint16 on the device: the same bytes)
    touched = _padded(2 * K + 2 * B, torch.int64, -7) if outputs[2] else None
    status = torch.zeros(2, dtype=torch.int32, device="cuda") if status is None else status
    rc = _hip.lib().mkb_pool_filter(_hip.ptr(s), B, mode_id, N, R, _hip.ptr(p), K, _hip.ptr(k), 0 if k is None else k.numel(),
                                    _hip.ptr(neg), _hip.ptr(pos), _hip.ptr(cnt), _hip.ptr(touched), _hip.ptr(status), _hip.stream_ptr())
    torch.cuda.synchronize()
    out = [rc]
    for buf, n, shape in ((neg, B * K, (B, K)), (pos, B * K, (B, K)), (cnt, B * 2 * K, (B, 2 * K)), (touched, 2 * K + 2 * B, (2 * K + 2 * B,))):
        if buf is None:
            out.append(None)
            continue
        host = buf.cpu().numpy()
        assert (host[n:] == -7).all(), "written past an output"
        host = host[:n].reshape(shape)
        out.append(host.view(np.uint16) if host.dtype == np.int16 else host)
    return out + [status.cpu().numpy()]


def _assert_filter_equals_restatement(sample, mode_id, N, pool, K, keys):
    rc, neg, pos, cnt, touched, status = run_filter(sample, mode_id, N, pool, K, keys)
    assert rc == 0 and status.tolist() == [0, 0]
    w_neg, w_pos, w_cnt, w_touched, empty = up.filter_pool(sample, mode_id, N, R, pool, K, keys)
    assert not empty
    for name, got, want in (("neg", neg, w_neg), ("pos", pos, w_pos), ("cnt", cnt, w_cnt), ("touched", touched, w_touched)):
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), name
    # the invariants, from the outputs alone
    assert (cnt.astype(np.int64).sum(1) == K).all()
    np.testing.assert_array_equal(neg, np.asarray(pool)[pos])
    for i, (h, r, t) in enumerate(np.asarray(sample).tolist()):
        fixed, target = (t, h) if mode_id == up.HEAD else (h, t)
        assert target not in neg[i] and not np.isin(neg[i], up.known_answers(keys, fixed, r, N, R)).any(), i
    again = run_filter(sample, mode_id, N, pool, K, keys)
    for a, b in zip((neg, pos, cnt, touched), again[1:5]):
        assert a.tobytes() == b.tobytes(), "two runs differ"
    return neg


@pytest.mark.parametrize("mode_id", [up.HEAD, up.TAIL], ids=["head", "tail"])
@pytest.mark.parametrize("B", [1, 5, 257])
@pytest.mark.parametrize("K", [1, 3, 32, 33, 512, 1024])
@pytest.mark.parametrize("N", [37, 14541])
def test_pool_filter_equals_the_restatement_byte_for_byte(N, K, B, mode_id):
    sample, pool, triples, safe = up.filter_fixture(N, R, B, K, mode_id, seed=1000 * K + B)
    keys = up.side_keys(triples, mode_id, N, R)
    neg = _assert_filter_equals_restatement(sample, mode_id, N, pool, K, keys)
    if B > 2:
        assert (neg[2] == safe).all()  # every pool entry but one is a known answer: that one fills the K slots
    # a pool of one entity repeated, and the same batch without any keys (only the targets are dropped)
    neg = _assert_filter_equals_restatement(sample, mode_id, N, np.full(2 * K, safe), K, keys)
    assert (neg == safe).all()
    _assert_filter_equals_restatement(sample, mode_id, N, pool, K, None)
    # the optional outputs left out: neg does not change
    rc, neg_only, pos, cnt, touched, _ = run_filter(sample, mode_id, N, pool, K, keys, outputs=(False, False, False))
    assert rc == 0 and pos is None and cnt is None and touched is None
    assert neg_only.tobytes() == up.filter_pool(sample, mode_id, N, R, pool, K, keys)[0].tobytes()


def test_pool_ids_outside_the_table_are_nobodys_answer():
    """A pool id outside [0, n_entity) is kept (it is no known answer, whatever key base + id happens to hit) and indexes nothing."""
    N, K = 37, 4
    sample = np.array([[3, 1, 5], [4, 1, 6]], dtype=np.int64)
    triples = np.array([[3, 1, 5], [3, 2, 0], [3, 2, 1], [4, 1, 6], [2, 4, 36]], dtype=np.int64)  # (3, 2, 0): key of (3, 1) + N
    pool = np.array([N, N + 1, -1, -N, 5, 6, 2 ** 40, 7], dtype=np.int64)
    for mode_id in (up.HEAD, up.TAIL):
        keys = up.side_keys(triples, mode_id, N, R)
        rc, neg, pos, cnt, touched, status = run_filter(sample, mode_id, N, pool, K, keys)
        want = up.filter_pool(sample, mode_id, N, R, pool, K, keys)
        assert rc == 0 and status.tolist() == [0, 0]
        assert neg.tobytes() == want[0].tobytes() and pos.tobytes() == want[1].tobytes() and cnt.tobytes() == want[2].tobytes()
    assert neg[0].tolist() == [N, N + 1, -1, -N]


def test_a_row_that_keeps_nothing_is_reported_lazily():
    """Rows 3 and 9 lose the whole pool: their outputs are zero, every other row is right, the status pair names row 3 (the smallest),
    and the sampler's check() raises RuntimeError with that row -- once; the sampler can be used on."""
    from mkb_amd import _hip, sampling

    N, K, B = 37, 3, 12
    sample, pool, triples, safe = up.filter_fixture(N, R, B, K, up.TAIL, seed=5)
    for i in (9, 3):  # the fixture's row 3 knows pool[0]; both now know `safe` and the rest of the pool as well
        h, r, _ = sample[i]
        triples = np.concatenate([triples, [[h, r, int(c)] for c in set(pool.tolist())]])
    keys = up.side_keys(triples, up.TAIL, N, R)
    rc, neg, pos, cnt, touched, status = run_filter(sample, up.TAIL, N, pool, K, keys)
    w_neg, w_pos, w_cnt, w_touched, empty = up.filter_pool(sample, up.TAIL, N, R, pool, K, keys)
    assert rc == 0 and empty == [3, 9] and status.tolist() == [_hip.ERR_EMPTY, 3]
    assert neg.tobytes() == w_neg.tobytes() and pos.tobytes() == w_pos.tobytes() and cnt.tobytes() == w_cnt.tobytes()
    for i in empty:
        assert not neg[i].any() and not pos[i].any() and not cnt[i].any()
    assert touched.tobytes() == w_touched.tobytes()
    # a later call with a smaller failing row lowers the row; one with a larger row leaves it
    st = torch.zeros(2, dtype=torch.int32, device="cuda")
    order = np.r_[0:3, 4:12, 3]  # row 9 moves to 8, row 3 to 11
    assert run_filter(sample[order], up.TAIL, N, pool, K, keys, status=st)[5].tolist() == [_hip.ERR_EMPTY, 8]
    assert run_filter(sample, up.TAIL, N, pool, K, keys, status=st)[5].tolist() == [_hip.ERR_EMPTY, 3]
    assert run_filter(sample[order], up.TAIL, N, pool, K, keys, status=st)[5].tolist() == [_hip.ERR_EMPTY, 3]
    # row 0 is a row like any other: the zeroed pair is told from "row 0 failed" by its code
    first = np.r_[3, 0:3, 4:12]
    assert run_filter(sample[first], up.TAIL, N, pool, K, keys, status=st)[5].tolist() == [_hip.ERR_EMPTY, 0]
    st = torch.zeros(2, dtype=torch.int32, device="cuda")
    assert run_filter(sample[first], up.TAIL, N, pool, K, keys, status=st)[5].tolist() == [_hip.ERR_EMPTY, 0]
    assert run_filter(sample, up.TAIL, N, pool, K, keys, status=st)[5].tolist() == [_hip.ERR_EMPTY, 0]

    class Given(sampling.PoolNegativeSampling):
        def _pool(self, s, mode):
            return torch.as_tensor(pool).to(s.device)

    ents, rels = {i: i for i in range(N)}, {i: i for i in range(R)}
    sampler = Given(K, [tuple(t) for t in triples.tolist()], ents, rels)
    got = sampler.generate(torch.as_tensor(sample).cuda(), "tail-batch")
    assert got.cpu().numpy().tobytes() == w_neg.tobytes()
    with pytest.raises(RuntimeError, match=r"row 3\b"):
        sampler.check()
    sampler.check()  # reported once
    keep = np.setdiff1d(np.arange(B), empty)
    got = sampler.generate(torch.as_tensor(sample[keep]).cuda(), "tail-batch")
    sampler.check()
    assert got.cpu().numpy().tobytes() == w_neg[keep].tobytes()
    assert sampler.get_state() == (42, 2)


def test_refused_arguments_are_invalid_before_any_launch():
    from mkb_amd import _hip

    lib = _hip.lib()
    N, K, B = 37, 4, 3
    s = torch.zeros((B, 3), dtype=torch.int64, device="cuda")
    pool = torch.ones(2 * K, dtype=torch.int64, device="cuda")
    sentinel = -12345
    neg = torch.full((B, K), sentinel, dtype=torch.int64, device="cuda")
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    keys = torch.arange(5, dtype=torch.int64, device="cuda") + 1000  # (keys of another query than the rows' (0, 0))
    good = dict(sample=s, B=B, mode=_hip.MODE_TAIL, N=N, R=R, pool=pool, K=K, keys=keys, n_keys=5, neg=neg, status=status[:2])

    def call(**change):
        a = dict(good, **change)
        return lib.mkb_pool_filter(_hip.ptr(a["sample"]), a["B"], a["mode"], a["N"], a["R"], _hip.ptr(a["pool"]), a["K"], _hip.ptr(a["keys"]),
                                   a["n_keys"], _hip.ptr(a["neg"]), None, None, None, _hip.ptr(a["status"]), _hip.stream_ptr())

    refused = [dict(K=0), dict(K=1025), dict(K=-1), dict(B=0), dict(B=-3), dict(N=0), dict(N=2 ** 31), dict(R=0), dict(sample=None),
               dict(pool=None), dict(neg=None), dict(status=None), dict(status=status[1:3]), dict(mode=_hip.MODE_DEFAULT), dict(mode=3),
               dict(keys=None, n_keys=5), dict(n_keys=-1)]
    for change in refused:
        assert call(**change) == _hip.ERR_INVALID, change
        assert lib.mkb_last_error()
    torch.cuda.synchronize()
    assert bool((neg == sentinel).all()) and status.tolist() == [0, 0, 0, 0]  # nothing was launched
    assert call() == 0 and call(N=2 ** 31 - 1) == 0 and call(keys=None, n_keys=0) == 0
    torch.cuda.synchronize()
    assert bool((neg == 1).all())  # (heads 0 and tails 0 know nothing about entity 1)

    accept = torch.full((N,), 1 << 32, dtype=torch.int64, device="cuda")
    alias = torch.zeros(N, dtype=torch.int32, device="cuda")
    out = torch.full((2 * K,), sentinel, dtype=torch.int64, device="cuda")

    def draw(accept=accept, alias=alias, N=N, K=K, out=out):
        return lib.mkb_pool_draw_alias(_hip.ptr(accept), _hip.ptr(alias), N, K, 1, 0, _hip.ptr(out), None, _hip.stream_ptr())

    for change in (dict(accept=None), dict(alias=None), dict(out=None), dict(K=0), dict(K=1025), dict(N=0), dict(N=2 ** 31)):
        assert draw(**change) == _hip.ERR_INVALID, change
    torch.cuda.synchronize()
    assert bool((out == sentinel).all())
    assert draw() == 0
    torch.cuda.synchronize()
    assert bool(((out >= 0) & (out < N)).all())


# ---------------------------------------------------------------------------------------------------------------- the alias draw
def run_draw(accept, alias, N, K, seed, draw, with_words=True):
    from mkb_amd import _hip

    a, b = torch.as_tensor(accept).cuda(), torch.as_tensor(alias).cuda()
    pool = _padded(2 * K, torch.int64, -7)
    words = _padded(4 * K, torch.int32, -7) if with_words else None  # (uint32 on the device: the same bytes)
    _hip.check(_hip.lib().mkb_pool_draw_alias(_hip.ptr(a), _hip.ptr(b), N, K, seed, draw, _hip.ptr(pool), _hip.ptr(words),
                                              _hip.stream_ptr()), "mkb_pool_draw_alias")
    torch.cuda.synchronize()
    assert bool((pool[2 * K:] == -7).all())
    if words is None:
        return pool[: 2 * K].cpu().numpy(), None
    w = words.cpu().numpy()
    assert (w[4 * K:] == -7).all()
    return pool[: 2 * K].cpu().numpy(), w[: 4 * K].view(np.uint32).reshape(2 * K, 2)


def _tables(N, kind):
    from mkb_amd.sampling.pool_sampling import alias_table

    w = up.skewed_weights(N, seed=N)
    if kind == "zeros":
        w[np.random.RandomState(N).rand(N) < 0.5] = 0.0
        w[N // 2] = 1.0
    if kind == "one-hot":
        w[:] = 0.0
        w[N // 3] = 2.0
    return (w,) + alias_table(w)


@pytest.mark.parametrize("K", [1, 33, 1024])
@pytest.mark.parametrize("N", [1, 2, 37, 14541])
def test_alias_draw_equals_the_host_recomputation_from_its_words(N, K):
    """The pool is the integer mapping of the kernel's own words (column word under the rejection mask, u against accept); the same
    (seed, draw) gives the same bytes, with or without the words; draw + 1 and another seed give other bytes; an entity of weight 0
    never appears; one-hot weights give a constant pool."""
    w, accept, alias = _tables(N, "zeros")
    pool, words = run_draw(accept, alias, N, K, seed=11, draw=5)
    np.testing.assert_array_equal(pool, up.alias_pick(words[:, 0], words[:, 1], accept, alias, N))
    if N == 1:
        assert not words[:, 0].any()
    assert (w[pool] > 0).all()
    again, words2 = run_draw(accept, alias, N, K, seed=11, draw=5)
    assert again.tobytes() == pool.tobytes() and words2.tobytes() == words.tobytes()
    assert run_draw(accept, alias, N, K, seed=11, draw=5, with_words=False)[0].tobytes() == pool.tobytes()
    nxt, words_next = run_draw(accept, alias, N, K, seed=11, draw=6)
    other, words_other = run_draw(accept, alias, N, K, seed=12, draw=5)
    assert words_next.tobytes() != words.tobytes() and words_other.tobytes() != words.tobytes()
    if (w > 0).sum() > 1 and K > 1:
        assert nxt.tobytes() != pool.tobytes() and other.tobytes() != pool.tobytes()
    w1, accept1, alias1 = _tables(N, "one-hot")
    assert (run_draw(accept1, alias1, N, K, seed=3, draw=0)[0] == N // 3).all()


def test_alias_draw_counter_layout():
    """Entry p of draw d is subsequence d * 2K + p: draw 3 at K = 1 (subsequences 6, 7) has the words of entries 6, 7 of draw 0
    at K = 4, and draw 1 at K = 33 continues draw 0 at K = 66."""
    N = 37
    _, accept, alias = _tables(N, "zeros")
    small, w_small = run_draw(accept, alias, N, 1, seed=8, draw=3)
    wide, w_wide = run_draw(accept, alias, N, 4, seed=8, draw=0)
    assert w_small.tobytes() == w_wide[6:8].tobytes() and small.tobytes() == wide[6:8].tobytes()
    second, w_second = run_draw(accept, alias, N, 33, seed=8, draw=1)
    both, w_both = run_draw(accept, alias, N, 66, seed=8, draw=0)
    assert w_second.tobytes() == w_both[66:].tobytes() and second.tobytes() == both[66:].tobytes()


def test_alias_draw_frequencies():
    """n_entity = 37, skewed weights, 512 draws at K = 64: n = 65,536 samples at a fixed seed.  Every entity's frequency lies within
    5 sqrt(p_e (1 - p_e) / n) of p_e -- five standard deviations of the binomial count, a two-sided tail of 5.7e-7 per entity;
    tests/test_host_pool_sampler.py confirms the bound for the restatement of the mapping fed with numpy's uniform words."""
    from mkb_amd import sampling

    N, K, draws = 37, 64, 512
    w = up.skewed_weights(N)
    ents, rels = {i: i for i in range(N)}, {i: i for i in range(R)}
    sampler = sampling.WeightedNegativeSampling(K, [(0, 0, 1)], ents, rels, seed=2024, weights=w, power=1.0)
    s = torch.zeros((1, 3), dtype=torch.int64, device="cuda")
    pools = []
    for _ in range(draws):
        pools.append(sampler._pool(s, "tail-batch"))
        sampler.draws += 1
    got = torch.cat(pools).cpu().numpy()
    n = len(got)
    assert n == 65536 and sampler.get_state() == (2024, 512)
    p = w / w.sum()
    freq = np.bincount(got, minlength=N) / n
    bound = 5 * np.sqrt(p * (1 - p) / n)
    print("frequency fraction of bound: %.3f" % float((np.abs(freq - p) / bound).max()))
    assert (np.abs(freq - p) <= bound).all()
    # the counter is the whole state: a second sampler set to (seed, 100) draws the 101st pool
    other = sampling.WeightedNegativeSampling(K, [(0, 0, 1)], ents, rels, seed=1, weights=w, power=1.0)
    other.set_state((2024, 100))
    assert torch.equal(other._pool(s, "tail-batch"), pools[100])


# ------------------------------------------------------------------------------------------------ the samplers through the steps
N5, B5, K5, HID = 37, 16, 4, 8


def _samplers(train, ents, rels):
    from mkb_amd import sampling

    class Given(sampling.PoolNegativeSampling):
        def _pool(self, sample, mode):
            ids = np.random.RandomState(self.seed + self.draws).randint(self.n_entity, size=2 * self.size)
            ids[-1] = ids[0]
            return torch.as_tensor(ids, device=sample.device)

    return {"weighted": lambda: sampling.WeightedNegativeSampling(K5, train, ents, rels, seed=3),
            "inbatch": lambda: sampling.InBatchNegativeSampling(K5, train, ents, rels, seed=3),
            "given": lambda: Given(K5, train, ents, rels, seed=3)}


def _problem5(name, seed=21):
    ent, rel, sample, _, w, modulus = random_problem(name, N5, R, HID, B5, K5, seed)
    train = [tuple(int(v) for v in row) for row in sample.tolist()]
    ents, rels = {i: i for i in range(N5)}, {i: i for i in range(R)}
    model = lambda: make_model(name, ent, rel, HID, 6.0, modulus)
    return model, _samplers(train, ents, rels), sample.cuda().contiguous(), w.cuda(), train


def _grads(m):
    out = [m.entity_embedding.grad.cpu().numpy().copy(), m.relation_embedding.grad.cpu().numpy().copy()]
    if m.name == "pRotatE":
        out.append(m.modulus.grad.cpu().numpy().copy())
    return out


@pytest.mark.parametrize("which", ["weighted", "inbatch", "given"])
@pytest.mark.parametrize("mode", ["head-batch", "tail-batch"])
@pytest.mark.parametrize("name", ["TransE", "RotatE", "ComplEx", "DistMult", "pRotatE"])
def test_samplers_through_the_pooled_steps_equal_the_general_kernels(name, mode, which, monkeypatch):
    """FusedTrainStep and PooledLossStep(MarginRanking) on a new sampler's negatives against the general kernels (mkb_score_fwd /
    mkb_score_bwd through autograd, and the loss) on the SAME negatives as a plain tensor.  Bounds: those of the existing
    pooled-against-general comparisons -- tests/test_gpu_pool.py for the Adversarial step (scores 1e-4, loss 1e-5, times max(1,
    largest |score|); grad_close on the entity table, with rtol 1e-4 on the relation table and the modulus),
    tests/test_gpu_ns_losses.py for PooledLossStep (loss 1e-5 + 1e-5 |loss|, grad_close on all three).  The in-batch pool is the
    case the uniform sampler meets only in part: every pool entity is also a tail (head) of the batch."""
    import mkb_amd.models.base as model_base
    from mkb_amd import losses
    from mkb_amd.fused import FusedTrainStep, PooledLossStep, pooled_supported

    monkeypatch.setattr(model_base, "AUTO_POOL", False)  # the plain copy of the negatives stays on the general kernels
    model, samplers, sample, w, _ = _problem5(name)
    sampler = samplers[which]()
    neg = sampler.generate(sample, mode)
    sampler.check()
    info = neg._mkb_pool
    assert neg.shape == (B5, K5) and neg.dtype == torch.int64 and info.size == K5 and info.pool.numel() == 2 * K5
    assert torch.equal(neg, info.pool[info.pos.long()]) and sampler.get_state()[:2] == (3, 1)
    if which == "inbatch":
        col = 0 if mode == "head-batch" else 2
        o = np.random.RandomState(3).randint(B5)
        assert torch.equal(info.pool, sample[(torch.arange(2 * K5, device="cuda") + o) % B5, col])
    plain = neg.clone()
    assert getattr(plain, "_mkb_pool", None) is None
    mg = model()
    assert pooled_supported(mg, B5, K5)

    def general(loss):
        mg.zero_grad(set_to_none=True)
        pos, sc = mg(sample), mg(sample, plain, mode)
        err = loss(pos, sc, w)
        err.backward()
        return pos.detach(), sc.detach(), float(err.detach()), _grads(mg)

    # ---- the Adversarial step
    pos, sc, want, g_want = general(losses.Adversarial(alpha=0.5))
    mp = model()
    step = FusedTrainStep(mp, 0.5)
    got = float(step(sample, w, neg, mode))
    g_got = _grads(mp)
    scale = max(1.0, float(sc.abs().max()))
    np.testing.assert_allclose(step.negative_score.cpu().numpy(), sc.cpu().numpy(), rtol=0, atol=1e-4 * scale)
    np.testing.assert_allclose(step.positive_score.cpu().numpy(), pos.cpu().numpy(), rtol=0, atol=1e-4 * scale)
    assert abs(got - want) <= 1e-5 * scale, (got, want)
    assert all(np.abs(g).max() > 0 for g in g_want)
    grad_close(g_got[0], g_want[0])
    grad_close(g_got[1], g_want[1], rtol=1e-4)
    if name == "pRotatE":
        np.testing.assert_allclose(g_got[2], g_want[2], rtol=1e-4)
    # the explicit sequence on the sampler's tensor takes pooled_forward
    mp.zero_grad(set_to_none=True)
    sc_pooled = mp(sample, neg, mode)
    losses.Adversarial(alpha=0.5)(mp(sample), sc_pooled, w).backward()
    np.testing.assert_allclose(sc_pooled.detach().cpu().numpy(), sc.cpu().numpy(), rtol=0, atol=1e-4 * scale)
    g_seq = _grads(mp)
    grad_close(g_seq[0], g_want[0])
    grad_close(g_seq[1], g_want[1], rtol=1e-4)
    # ---- the margin step (the margin stepped until no pair of the general route lies within 1e-3 of the kink)
    margin = 6.0
    a = sc.double() - pos.double().view(-1, 1)
    for _ in range(1000):
        if float((margin + a).abs().min()) > 1e-3:
            break
        margin += 0.01
    assert float((margin + a).abs().min()) > 1e-3
    loss = losses.MarginRanking(margin=margin)
    _, _, want, g_want = general(loss)
    mp = model()
    got = float(PooledLossStep(mp, loss)(sample, w, neg, mode))
    assert abs(got - want) <= 1e-5 + 1e-5 * abs(want), (got, want)
    for g, r in zip(_grads(mp), g_want):
        assert np.abs(r).max() > 0
        grad_close(g, r)


@pytest.mark.parametrize("which", ["weighted", "inbatch"])
def test_samplers_under_the_row_lazy_optimizer_equal_dense_adam(which):
    """Six sampled steps on a 4096-row table (the smallest that steps row-lazily) with optim.Adam(lazy_rows=True) against the same
    steps with dense torch.optim.Adam: the step catches the optimizer up on the rows the sampler listed.  DistMult and atol 2e-6, as
    tests/test_gpu_ns_losses.py compares the two optimizers (its docstring has the reason for the model)."""
    from mkb_amd import _links, optim, sampling
    from mkb_amd.fused import FusedTrainStep

    N, B, K = 4096, 32, 8
    ent, rel, _, _, w, _ = random_problem("DistMult", N, R, 16, B, K, seed=13)
    g = torch.Generator().manual_seed(4)
    train_t = torch.stack([torch.randint(N, (6 * B,), generator=g), torch.randint(R, (6 * B,), generator=g),
                           torch.randint(N, (6 * B,), generator=g)], 1)
    train = [tuple(r) for r in train_t.tolist()]
    ents, rels = {i: i for i in range(N)}, {i: i for i in range(R)}
    cls = sampling.WeightedNegativeSampling if which == "weighted" else sampling.InBatchNegativeSampling
    tables = []
    for lazy in (True, False):
        m = make_model("DistMult", ent, rel, 16, 6.0)
        ns = cls(K, train, ents, rels, seed=9)
        params = [m.entity_embedding, m.relation_embedding]
        opt = optim.Adam(params, lr=1e-3, lazy_rows=True) if lazy else torch.optim.Adam(params, lr=1e-3)
        assert (_links.owner(m.entity_embedding) is opt) == lazy
        step = FusedTrainStep(m, 1.0)
        for it in range(6):
            s = train_t[it * B:(it + 1) * B].cuda().contiguous()
            step.sampled(s, w.cuda(), ns, "head-batch" if it % 2 else "tail-batch")
            opt.step()
            opt.zero_grad()
        if lazy:
            opt.flush()
        ns.check()
        torch.cuda.synchronize()
        tables.append((m.entity_embedding.detach().cpu().numpy(), m.relation_embedding.detach().cpu().numpy()))
    (ea, ra), (eb, rb) = tables
    print("row-lazy vs dense: max |d ent| %.3g, max |d rel| %.3g" % (np.abs(ea - eb).max(), np.abs(ra - rb).max()))
    assert np.abs(eb - ent.numpy()).max() > 1e-4
    np.testing.assert_allclose(ea, eb, rtol=0, atol=2e-6)
    np.testing.assert_allclose(ra, rb, rtol=0, atol=2e-6)


# ------------------------------------------------------------------------------------------------------------- compose.Pipeline
LR, EPOCHS, BATCH, SIZE = 2e-2, 2, 64, 16


@pytest.mark.parametrize("optimizer", ["adam-lazy", "adagrad"])
@pytest.mark.parametrize("which", ["weighted", "inbatch"])
def test_pipeline_learns_with_the_pool_samplers(which, optimizer, monkeypatch):
    """Pipeline.learn on CountriesS1 (the smallest dataset the pipeline tests use), two epochs, RotatE: the pipeline takes
    FusedTrainStep for every batch and lends the sampler to nobody, the loss is finite and the second epoch's mean is below the
    first's, and the tables equal those of the same loop written out by hand with generate + step(...).

    Bound of the table comparison.  Both runs make the same launches on the same numbers; what may differ is the order of the float
    atomics in the backward kernels.  A gradient element sums at most BATCH (SIZE + 1) = 1088 terms, so two orders differ by at
    most 1088 * 2^-24 = 6.5e-5 of the sum of their magnitudes; a step of Adam or Adagrad moves an element by at most ~lr, so the
    two runs part by at most lr * 6.5e-5 a step, to first order, and over the 68 steps by 68 * 2e-2 * 6.5e-5 = 8.8e-5.  A sampler
    that drew another pool in one step would move rows by ~lr = 2e-2."""
    from mkb_amd import compose, datasets, evaluation, fused, losses, models, optim, sampling

    ds = datasets.CountriesS1(batch_size=BATCH, shuffle=False, seed=42, num_workers=0)
    cls = sampling.WeightedNegativeSampling if which == "weighted" else sampling.InBatchNegativeSampling

    def setup():
        torch.manual_seed(5)
        m = models.RotatE(hidden_dim=20, entities=ds.entities, relations=ds.relations, gamma=6.0).cuda()
        ns = cls(SIZE, ds.train, ds.entities, ds.relations, seed=42)
        params = [m.entity_embedding, m.relation_embedding]
        opt = optim.Adam(params, lr=LR, lazy_rows=True) if optimizer == "adam-lazy" else optim.Adagrad(params, lr=LR)
        return m, ns, opt

    m, ns, opt = setup()
    seen, inner = [], fused.FusedTrainStep.__call__

    def spy(self, *args, **kwargs):
        assert getattr(opt, "draw_ahead", None) is None  # only a NegativeSampling's draw can ride the optimizer's launch
        out = inner(self, *args, **kwargs)
        seen.append(out.detach())
        return out

    monkeypatch.setattr(fused.FusedTrainStep, "__call__", spy)
    pipe = compose.Pipeline(epochs=EPOCHS, eval_every=100, device="cuda")
    loss = losses.Adversarial(alpha=0.5)
    assert type(pipe._fused_step_for(m, ds, ns, opt, loss)) is fused.FusedTrainStep
    pipe._give_back(opt)
    pipe.learn(model=m, dataset=ds, sampling=ns, optimizer=opt, loss=loss,
               evaluation=evaluation.Evaluation(true_triples=ds.true_triples, entities=ds.entities, relations=ds.relations,
                                                batch_size=64, device="cuda"))
    monkeypatch.setattr(fused.FusedTrainStep, "__call__", inner)
    values = torch.stack(seen).cpu().numpy()
    steps = len(values)
    assert steps == EPOCHS * 2 * ((len(ds.train) + BATCH - 1) // BATCH) and np.isfinite(values).all()
    first, second = values[: steps // 2].mean(), values[steps // 2:].mean()
    print("pipeline", which, optimizer, "epoch means", first, second)
    assert second < first
    assert ns.get_state()[:2] == (42, steps)

    # the same loop by hand
    m2, ns2, opt2 = setup()
    step = fused.FusedTrainStep(m2, 0.5)
    for _ in range(EPOCHS):
        for data in ds:
            sample, weight = data["sample"].cuda(), data["weight"].cuda()
            negatives = ns2.generate(sample, data["mode"])
            step(sample, weight, negatives, data["mode"])
            opt2.step()
            opt2.zero_grad()
    ns2.check()
    if hasattr(opt2, "flush"):
        opt2.flush()
    torch.cuda.synchronize()
    bound = steps * LR * BATCH * (SIZE + 1) * 2.0 ** -24
    for what, a, b in (("entity", m.entity_embedding, m2.entity_embedding), ("relation", m.relation_embedding, m2.relation_embedding)):
        a, b = a.detach().cpu().numpy(), b.detach().cpu().numpy()
        print("pipeline vs hand loop", which, optimizer, what, "max |d| %.3g of bound %.3g" % (np.abs(a - b).max(), bound))
        np.testing.assert_allclose(a, b, rtol=0, atol=bound)


def test_kdmkb_style_use_from_the_host():
    """A CPU sample is moved to the device and the negatives come back to the CPU, as NegativeSampling.generate answers one
    (distillation.KdmkbModel only calls generate)."""
    from mkb_amd import sampling

    _, samplers, sample, _, train = _problem5("TransE")
    for which in ("weighted", "inbatch"):
        a, b = samplers[which](), samplers[which]()
        on_host = a.generate(sample.cpu(), "tail-batch")
        on_device = b.generate(sample, "tail-batch")
        assert not on_host.is_cuda and torch.equal(on_host, on_device.cpu())
    with pytest.raises(ValueError):
        a.generate(sample, "default")
