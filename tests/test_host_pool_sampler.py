"""CPU (-m "not gpu") tests of the pool samplers' host side: Vose's alias table, the numpy restatement of the filter that the GPU
tests compare against (tests/util_pool_sampler.py), the argument checks, the library's new symbols, and the bound the GPU frequency
test uses, confirmed here for the restatement of the mapping."""
import numpy as np
import pytest

import util_pool_sampler as up

TWO32 = 1 << 32


def _weight_cases(n):
    rs = np.random.RandomState(n)
    one_hot = np.zeros(n)
    one_hot[n // 2] = 3.0
    with_zeros = rs.rand(n) + 0.05
    with_zeros[::2] = 0.0
    if not with_zeros.sum() > 0:
        with_zeros[0] = 1.0
    return {"uniform": np.ones(n), "one-hot": one_hot, "zeros": with_zeros, "skewed": up.skewed_weights(n)}


@pytest.mark.parametrize("kind", ["uniform", "one-hot", "zeros", "skewed"])
@pytest.mark.parametrize("n", [1, 2, 37])
def test_vose_table_implies_the_distribution(n, kind):
    """q_e = (accept_e + sum_{j: alias_j = e} (2^32 - accept_j)) / (n 2^32) equals p_e within n 2^-31; an entity of weight 0 has
    accept = 0 and is nobody's alias (it cannot be drawn: probability 0 is exact)."""
    from mkb_amd.sampling.pool_sampling import alias_table

    w = _weight_cases(n)[kind]
    p = w / w.sum()
    accept, alias = alias_table(w)
    assert accept.dtype == np.int64 and alias.dtype == np.int32 and accept.shape == alias.shape == (n,)
    assert (accept >= 0).all() and (accept <= TWO32).all() and (alias >= 0).all() and (alias < n).all()
    q = up.implied_distribution(accept, alias)
    err = float(np.abs(q - p).max())
    print("alias table", n, kind, "max |q - p| = %.3g, bound %.3g" % (err, n * 2.0 ** -31))
    assert err <= n * 2.0 ** -31
    zero = w == 0
    assert (accept[zero] == 0).all() and (q[zero] == 0).all()
    assert not zero[alias[accept < TWO32]].any()  # (a column that always keeps its own entity never looks at its alias)
    if kind == "uniform":
        assert (accept == TWO32).all()


def test_weighted_sampler_weights():
    """'degree' counts occurrences as head or tail; an array is taken as it is; the power is applied; bad weights -> ValueError."""
    from mkb_amd.sampling import WeightedNegativeSampling

    ents, rels = {i: i for i in range(6)}, {0: 0, 1: 1}
    train = [(0, 0, 1), (0, 1, 2), (3, 0, 0), (4, 1, 4)]
    deg = np.array([3, 1, 1, 1, 2, 0], dtype=np.float64)
    s = WeightedNegativeSampling(2, train, ents, rels, seed=1)
    np.testing.assert_allclose(s.probabilities, deg ** 0.75 / (deg ** 0.75).sum(), rtol=1e-15)
    assert s.accept[5] == 0 and 5 not in s.alias[s.accept < TWO32] and (s.size, s.n_entity, s.n_relation) == (2, 6, 2)
    assert s.get_state() == (1, 0)
    s = WeightedNegativeSampling(2, train, ents, rels, weights="degree", power=1.0)
    np.testing.assert_allclose(s.probabilities, deg / deg.sum(), rtol=1e-15)
    s = WeightedNegativeSampling(2, train, ents, rels, weights="uniform", power=0.3)
    np.testing.assert_allclose(s.probabilities, np.full(6, 1 / 6), rtol=1e-15)
    s = WeightedNegativeSampling(2, train, ents, rels, weights=[0, 1, 16, 0, 0, 81], power=0.5)
    np.testing.assert_allclose(s.probabilities, np.array([0, 1, 4, 0, 0, 9]) / 14.0, rtol=1e-15)
    for bad in ("frequency", None, [1.0, 2.0], np.ones((6, 1)), [1, 1, 1, 1, 1, -1], [0] * 6, [1, 1, 1, 1, 1, float("nan")],
                [1, 1, 1, 1, 1, float("inf")], ["a"] * 6):
        with pytest.raises(ValueError):
            WeightedNegativeSampling(2, train, ents, rels, weights=bad)
    with pytest.raises(ValueError):
        WeightedNegativeSampling(0, train, ents, rels)
    with pytest.raises(ValueError):
        WeightedNegativeSampling(1025, train, ents, rels)


def _brute_force_filter(sample, mode, pool, K, true_head, true_tail):
    """The filter as a python loop over dictionaries of known answers, in the shape of the reference's in-batch negatives
    (mkb/text/learn.py:366-400: for every row, walk the candidates, skip the row's own, keep what is not a known answer), with
    this project's cyclic fill in place of the reference's truncation to the shortest row."""
    out = []
    for h, r, t in sample:
        fake = []
        for position, c in enumerate(pool):
            if mode == "tail-batch":
                if c == t or c in true_tail.get((h, r), ()):
                    continue
            else:
                if c == h or c in true_head.get((r, t), ()):
                    continue
            fake.append((position, c))
        out.append([fake[j % len(fake)] for j in range(K)] if fake else None)
    return out


@pytest.mark.parametrize("mode", ["head-batch", "tail-batch"])
@pytest.mark.parametrize("N,B,K", [(37, 5, 1), (37, 257, 3), (37, 40, 33), (500, 64, 32)])
def test_filter_restatement_equals_a_brute_force_loop(N, B, K, mode):
    R = 5
    mode_id = up.HEAD if mode == "head-batch" else up.TAIL
    sample, pool, triples, _ = up.filter_fixture(N, R, B, K, mode_id, seed=N + B + K)
    rs = np.random.RandomState(B)
    pool = np.where(rs.rand(2 * K) < 0.3, rs.randint(N, size=2 * K), pool)  # some rows may now lose the whole pool: covered too
    true_head, true_tail = {}, {}
    for h, r, t in triples.tolist():
        true_head.setdefault((r, t), set()).add(h)
        true_tail.setdefault((h, r), set()).add(t)
    neg, pos, cnt, touched, empty = up.filter_pool(sample, mode_id, N, R, pool, K, up.side_keys(triples, mode_id, N, R))
    want = _brute_force_filter(sample.tolist(), mode, pool.tolist(), K, true_head, true_tail)
    assert empty == [i for i, row in enumerate(want) if row is None]
    for i, row in enumerate(want):
        if row is None:
            assert not neg[i].any() and not pos[i].any() and not cnt[i].any()
            continue
        assert [p for p, _ in row] == pos[i].tolist() and [c for _, c in row] == neg[i].tolist()
        assert cnt[i].tolist() == [sum(1 for p, _ in row if p == q) for q in range(2 * K)]
    np.testing.assert_array_equal(touched, np.concatenate([pool, sample[:, 0], sample[:, 2]]))
    # keys = None: only the target is dropped
    neg0, pos0, _, _, _ = up.filter_pool(sample, mode_id, N, R, pool, K, None)
    want0 = _brute_force_filter(sample.tolist(), mode, pool.tolist(), K, {}, {})
    for i, row in enumerate(want0):
        assert row is None or [p for p, _ in row] == pos0[i].tolist()


def test_frequency_bound_holds_for_the_restated_mapping():
    """The bound of the GPU frequency test -- every entity within 5 sqrt(p (1 - p) / n) of p_e at n = 65,536 draws, from the
    binomial: five standard deviations, 6e-7 per entity and side -- holds for the restatement of the mapping fed with numpy's
    uniform words (the alias table's own error, 37 * 2^-31 = 1.7e-8, is far inside it: the smallest bound here is ~1e-3)."""
    from mkb_amd.sampling.pool_sampling import alias_table

    N, n = 37, 65536
    w = up.skewed_weights(N)
    p = w / w.sum()
    accept, alias = alias_table(w)
    rs = np.random.RandomState(2024)
    got = up.alias_pick(up.uniform_columns(rs, n, N), rs.randint(0, TWO32, size=n, dtype=np.int64), accept, alias, N)
    freq = np.bincount(got, minlength=N) / n
    bound = 5 * np.sqrt(p * (1 - p) / n)
    print("frequency fraction of bound (restatement): %.3f, smallest bound %.3g" % (float((np.abs(freq - p) / bound).max()), bound.min()))
    assert (np.abs(freq - p) <= bound).all()


def test_library_exports_the_pool_sampler_symbols():
    from mkb_amd import _hip

    lib = _hip.lib()
    for name in ("mkb_pool_filter", "mkb_pool_draw_alias"):
        assert name in _hip.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.mkb_abi_version() == 9  # new symbols, no bump


def test_in_batch_sampler_state_and_base_class():
    from mkb_amd.sampling import InBatchNegativeSampling, PoolNegativeSampling

    ents, rels = {i: i for i in range(6)}, {0: 0}
    s = InBatchNegativeSampling(4, [(0, 0, 1)], ents, rels, seed=7)
    seed, draws, state = s.get_state()
    assert (seed, draws) == (7, 0) and state[0] == "MT19937"
    with pytest.raises(ValueError):
        s.set_state((7, 3))
    s.set_state((9, 0))
    assert s.get_state()[:2] == (9, 0)
    base = PoolNegativeSampling(4, [(0, 0, 1)], ents, rels)
    with pytest.raises(NotImplementedError):
        base._pool(None, "tail-batch")
    base.check()  # nothing generated: nothing to report, no device needed
