"""-m gpu: filtered top-k entity prediction (mkb_topk, mkb_amd/csrc/rank.hip; utils.predict_top_k, Evaluation.top_k).

The expected answer is restated here independently of the kernel: a stable descending sort (numpy lexsort: NaN first, then higher
score, then lower entity id) of the device's own all-entity scores (Evaluation.ranks(..., with_scores=True): the same routes, so
the same fp32 values), with the filtered columns (oracle.ranking.candidates) removed.  Ids must match exactly, scores bit for bit.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MODELS = ["TransE", "RotatE", "ComplEx", "DistMult", "pRotatE"]
KS = (1, 10, 100, 1024)


def expected_topk(scores, excluded, k):
    """-> (ids [n, k], scores [n, k]) of a stable descending sort with NaN first, excluded columns left out, padded -1 / -inf."""
    n, N = scores.shape
    nan = np.isnan(scores)
    cls = np.where(excluded, 2, np.where(nan, 0, 1))
    neg = np.where(nan | excluded, 0.0, -scores.astype(np.float64))
    cand = np.broadcast_to(np.arange(N), (n, N))
    order = np.lexsort((cand, neg, cls), axis=-1)[:, :k]
    valid = np.take_along_axis(cls, order, axis=1) < 2
    ids = np.where(valid, order, -1)
    sc = np.where(valid, np.take_along_axis(scores, order, axis=1), -np.inf).astype(np.float32)
    if k > N:
        ids = np.concatenate([ids, np.full((n, k - N), -1)], axis=1)
        sc = np.concatenate([sc, np.full((n, k - N), -np.inf, dtype=np.float32)], axis=1)
    return ids, sc


def excluded_columns(triples, keys, N, R, mode, how):
    """how: "keep" (the filtered rank's candidate set: the other true triples go, oracle.ranking.candidates), "drop" (the target
    goes too when its own triple is true), "none"."""
    from oracle import ranking

    t = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    if how == "none":
        return np.zeros((len(t), N), dtype=bool)
    _, bias = ranking.candidates(t, keys, N, R, mode)
    other = bias != 0
    if how == "keep":
        return other
    target = t[:, 0] if mode == "head-batch" else t[:, 2]
    own = (t[:, 0] * R + t[:, 1]) * N + t[:, 2]  # the query's own triple (keys of oracle.ranking.true_key_set)
    pos = np.minimum(np.searchsorted(keys, own), len(keys) - 1)
    other[np.arange(len(t)), target] |= keys[pos] == own
    return other


def assert_topk_equal(ids, sc, want_ids, want_sc, what):
    ids, sc = ids.cpu().numpy(), sc.cpu().numpy()
    np.testing.assert_array_equal(ids, want_ids, err_msg=what)
    np.testing.assert_array_equal(sc.view(np.uint32), want_sc.view(np.uint32), err_msg=what)


def _run_exact(m, ev, triples, true, N, R, chunk=1024, ks=KS):
    from oracle import ranking
    from mkb_amd.utils import predict_top_k

    keys = ranking.true_key_set(true, N, R)
    for mode in ("head-batch", "tail-batch"):
        _, dev_scores = ev.ranks(m, triples, mode, chunk=chunk, with_scores=True)
        dev_scores = dev_scores.cpu().numpy()
        for how in ("keep", "drop", "none"):
            excl = excluded_columns(triples, keys, N, R, mode, how)
            want_ids, want_sc = expected_topk(dev_scores, excl, max(ks))
            for k in ks:
                if how == "none":
                    ids, sc = predict_top_k(m, triples, mode, k, chunk=chunk)
                elif how == "keep":
                    ids, sc = ev.top_k(m, triples, mode, k, chunk=chunk)
                else:
                    ids, sc = predict_top_k(m, triples, mode, k, true_triples=ev.true_triples, keep_target=False, chunk=chunk)
                assert ids.shape == (len(triples), k) and ids.dtype == torch.int64 and sc.dtype == torch.float32
                assert_topk_equal(ids, sc, want_ids[:, :k], want_sc[:, :k], f"{m.name} {mode} {how} k={k}")


def _fb15k237(name, seed=77):
    from util_gpu import make_model
    from util_gpu_tables import eval_tables
    from mkb_amd import datasets, evaluation

    ds = datasets.Fb15k237(batch_size=8, shuffle=False, seed=42, num_workers=0)
    ent, rel, modulus = eval_tables(name, seed=seed)
    m = make_model(name, ent, rel, 1000, 9.0, modulus).eval()
    ev = evaluation.Evaluation(true_triples=ds.true_triples, entities=ds.entities, relations=ds.relations, batch_size=64,
                               device="cuda", num_workers=0)
    test = np.asarray(ds.test, dtype=np.int64)
    triples = test[np.random.RandomState(5).choice(len(test), size=256, replace=False)]
    return ds, m, ev, triples


@pytest.mark.parametrize("name", MODELS)
def test_topk_exact_on_umls(name):
    """Umls (135 entities: k = 1024 pads), every test triple, both modes, filter kept / dropped / off."""
    from util_gpu import make_model
    from mkb_amd import datasets, evaluation

    ds = datasets.Umls(batch_size=8, shuffle=False, seed=42, num_workers=0)
    rs = np.random.RandomState(11)
    hidden = 64
    de = 2 * hidden if name in ("RotatE", "ComplEx") else hidden
    dr = 2 * hidden if name == "ComplEx" else hidden
    ent = rs.uniform(-0.2, 0.2, size=(ds.n_entity, de)).astype(np.float32)
    rel = rs.uniform(-0.2, 0.2, size=(ds.n_relation, dr)).astype(np.float32)
    modulus = np.array([[0.1]], dtype=np.float32) if name in ("RotatE", "pRotatE") else None
    m = make_model(name, ent, rel, hidden, 6.0, modulus).eval()
    ev = evaluation.Evaluation(true_triples=ds.true_triples, entities=ds.entities, relations=ds.relations, batch_size=64,
                               device="cuda", num_workers=0)
    triples = np.asarray(ds.test, dtype=np.int64)
    _run_exact(m, ev, triples, np.asarray(ds.true_triples, dtype=np.int64), ds.n_entity, ds.n_relation)


@pytest.mark.parametrize("name", MODELS)
def test_topk_exact_and_rank_consistent_on_fb15k237(name):
    """256 FB15k-237 test triples at hidden 1000 (tile route: TransE / RotatE, matrix cores: ComplEx / DistMult, lane route:
    pRotatE); then, with the target kept in: wherever the filtered rank r <= k the target sits at slot r - 1, else it is absent."""
    ds, m, ev, triples = _fb15k237(name)
    _run_exact(m, ev, triples, np.asarray(ds.true_triples, dtype=np.int64), 14541, 237)
    for mode in ("head-batch", "tail-batch"):
        ranks = ev.ranks(m, triples, mode).cpu().numpy()
        target = triples[:, 0 if mode == "head-batch" else 2]
        for k in (10, 100):
            ids = ev.top_k(m, triples, mode, k)[0].cpu().numpy()
            inside = ranks <= k
            rows = np.flatnonzero(inside)
            np.testing.assert_array_equal(ids[rows, ranks[rows] - 1], target[rows], err_msg=f"{name} {mode} k={k}")
            assert not (ids[~inside] == target[~inside, None]).any(), f"{name} {mode} k={k}: target listed past its rank"


def test_topk_against_the_oracle_at_the_headline_size():
    """RotatE hidden 1000 on FB15k-237: the filtered top-10 id set is the oracle's wherever the oracle's 10th and 11th candidates
    stand further apart than the near-tie band of test_gpu_rank_oracle.py."""
    from oracle import ranking, scoring
    from util_gpu_tables import eval_tables

    ds, m, ev, triples = _fb15k237("RotatE")
    triples = triples[:96]
    ent, rel, modulus = eval_tables("RotatE", seed=77)
    tb = scoring.Tables("RotatE", 1000, 9.0, torch.from_numpy(ent), torch.from_numpy(rel), torch.from_numpy(modulus))
    keys = ranking.true_key_set(np.asarray(ds.true_triples, dtype=np.int64), 14541, 237)
    k, eps, n_clear = 10, 2e-5, 0
    for mode in ("head-batch", "tail-batch"):
        raw, _, _ = ranking.scores_and_ranks_one_pass(tb, triples, keys, mode, chunk=8, fast_norm=True)
        excl = excluded_columns(triples, keys, 14541, 237, mode, "keep")
        srt = -np.sort(-np.where(excl, -np.inf, raw), axis=1)
        clear = srt[:, k - 1] - srt[:, k] > eps
        want = np.argsort(-np.where(excl, -np.inf, raw), axis=1, kind="stable")[:, :k]
        ids = ev.top_k(m, triples, mode, k)[0].cpu().numpy()
        for i in np.flatnonzero(clear):
            assert set(ids[i]) == set(want[i]), (mode, i)
        n_clear += int(clear.sum())
    print(f"{n_clear} of {2 * len(triples)} top-10 sets compared")
    assert n_clear >= 16, n_clear


def _model(name, ent, rel, hidden, modulus=None):
    from util_gpu import make_model

    return make_model(name, ent, rel, hidden, 6.0, modulus).eval()


def _evaluation(true, N, R):
    from mkb_amd import evaluation

    return evaluation.Evaluation(true_triples=[tuple(t) for t in np.asarray(true).tolist()], entities={i: i for i in range(N)},
                                 relations={i: i for i in range(R)}, batch_size=64, device="cuda", num_workers=0)


def test_topk_ties_and_nan():
    """Duplicate entity rows tie exactly (lower id first); a NaN entity row ranks first with a NaN score; a collapsed table (every
    score equal: more ties at the threshold than the gather buffer holds) returns the lowest unfiltered ids."""
    from mkb_amd.utils import predict_top_k

    rs = np.random.RandomState(4)
    N, R, hidden = 300, 5, 32
    true = np.stack([rs.randint(N, size=2000), rs.randint(R, size=2000), rs.randint(N, size=2000)], 1)
    for name in ("TransE", "DistMult"):
        ent = rs.uniform(-0.5, 0.5, size=(N, hidden)).astype(np.float32)
        rel = rs.uniform(-0.5, 0.5, size=(R, hidden)).astype(np.float32)
        for dup in (40, 77, 150, 299):
            ent[dup] = ent[12]
        ent[200] = np.nan
        m = _model(name, ent, rel, hidden)
        ev = _evaluation(true, N, R)
        triples = true[(true[:, 0] != 200) & (true[:, 2] != 200)][:64]
        _run_exact(m, ev, triples, true, N, R, ks=(1, 10, 300, 1024))
        for mode in ("head-batch", "tail-batch"):
            ids, sc = predict_top_k(m, triples, mode, N)
            if name == "TransE":
                assert (ids[:, 0] == 200).all() and torch.isnan(sc[:, 0]).all()
            pos = {e: (ids == e).int().argmax(dim=1) for e in (12, 40, 77, 150, 299)}
            assert all((pos[a] + 1 == pos[b]).all() for a, b in ((12, 40), (40, 77), (77, 150), (150, 299)))
    # collapsed: every entity row equal
    N = 5000
    ent = np.tile(rs.uniform(-0.5, 0.5, size=(1, hidden)).astype(np.float32), (N, 1))
    rel = rs.uniform(-0.5, 0.5, size=(R, hidden)).astype(np.float32)
    true = np.stack([rs.randint(N, size=3000), rs.randint(R, size=3000), rs.randint(N, size=3000)], 1)
    true[:200, 0], true[:200, 1], true[:200, 2] = 7, 1, np.arange(200)  # (7, 1, ?) filters tails 0..199
    true[200:, 0] = np.where(true[200:, 0] == 7, 8, true[200:, 0])
    m = _model("TransE", ent, rel, hidden)
    ev = _evaluation(true, N, R)
    triples = np.concatenate([true[:1], true[300:331]])
    _run_exact(m, ev, triples, true, N, R, ks=(1, 100, 1024))
    ids = ev.top_k(m, triples[:1], "tail-batch", 100, keep_target=False)[0].cpu().numpy()
    np.testing.assert_array_equal(ids[0], np.arange(200, 300))


def test_topk_large_and_near_total_filters():
    """N = 20,000: one (h, r) with 12,000 true tails at k = 1024, one whose filter leaves 5 candidates (slots 5.. = -1 / -inf)."""
    from mkb_amd.utils import predict_top_k

    rs = np.random.RandomState(8)
    N, R, hidden = 20000, 3, 32
    big = np.stack([np.zeros(12000, np.int64), np.zeros(12000, np.int64), rs.choice(N, 12000, replace=False)], 1)
    left = rs.choice(N, 5, replace=False)
    nearly = np.setdiff1d(np.arange(N), left)
    near = np.stack([np.ones(len(nearly), np.int64), np.ones(len(nearly), np.int64), nearly], 1)
    noise = np.stack([rs.randint(2, N, size=3000), rs.randint(R, size=3000), rs.randint(N, size=3000)], 1)
    true = np.concatenate([big, near, noise])
    ent = rs.uniform(-0.5, 0.5, size=(N, 2 * hidden)).astype(np.float32)
    rel = rs.uniform(-0.5, 0.5, size=(R, hidden)).astype(np.float32)
    m = _model("RotatE", ent, rel, hidden, np.array([[0.3]], dtype=np.float32))
    ev = _evaluation(true, N, R)
    triples = np.concatenate([big[:3], near[:3], noise[:26]])
    _run_exact(m, ev, triples, true, N, R, ks=(10, 1024))
    ids, sc = predict_top_k(m, near[:1], "tail-batch", 1024, true_triples=ev.true_triples)
    ids, sc = ids.cpu().numpy()[0], sc.cpu().numpy()[0]
    assert sorted(ids[:5].tolist()) == sorted(left.tolist())
    assert (ids[5:] == -1).all() and np.isneginf(sc[5:]).all() and np.isfinite(sc[:5]).all()


def test_topk_yago_shape_global_path():
    """YAGO3-10 shape: N = 123,182, RotatE hidden 500, B = 64, k = 100."""
    rs = np.random.RandomState(9)
    N, R, hidden = 123182, 37, 500
    r = 11.0 / hidden
    ent = rs.uniform(-r, r, size=(N, 2 * hidden)).astype(np.float32)
    rel = rs.uniform(-r, r, size=(R, hidden)).astype(np.float32)
    true = np.stack([rs.randint(N, size=200000), rs.randint(R, size=200000), rs.randint(N, size=200000)], 1)
    true[:3000, 0], true[:3000, 1] = 5, 2  # one (h, r) with ~3000 tails
    m = _model("RotatE", ent, rel, hidden, np.array([[0.5 * r]], dtype=np.float32))
    ev = _evaluation(true, N, R)
    triples = np.concatenate([true[:2], true[5000:5062]])
    _run_exact(m, ev, triples, true, N, R, ks=(100,))


@pytest.mark.parametrize("B", [30, 1037])
def test_topk_ragged_batches_cross_chunk_seams(B):
    """ComplEx at FB15k-237 size, chunk = 512: the matrix-core route's B % 4 fallback and the chunk seams."""
    from util_gpu_tables import eval_tables
    from mkb_amd import datasets

    ds = datasets.Fb15k237(batch_size=8, shuffle=False, seed=42, num_workers=0)
    ent, rel, _ = eval_tables("ComplEx", hidden=200, seed=3)
    m = _model("ComplEx", ent, rel, 200)
    ev = _evaluation(np.asarray(ds.true_triples, dtype=np.int64), 14541, 237)
    test = np.asarray(ds.test, dtype=np.int64)
    triples = test[np.random.RandomState(B).choice(len(test), size=B, replace=False)]
    _run_exact(m, ev, triples, np.asarray(ds.true_triples, dtype=np.int64), 14541, 237, chunk=512, ks=(10, 1024))


def test_topk_errors():
    """k = 0, k = 1025 and mode None: ValueError from the API, MKB_ERR_INVALID from the C ABI (nothing launched, outputs untouched)."""
    import ctypes

    from mkb_amd import _hip
    from mkb_amd.utils import predict_top_k

    rs = np.random.RandomState(1)
    N, R, hidden = 100, 3, 16
    m = _model("DistMult", rs.rand(N, hidden).astype(np.float32), rs.rand(R, hidden).astype(np.float32), hidden)
    s = torch.tensor([[1, 0, 2], [3, 1, 4]], device="cuda")
    for k, mode in ((0, "tail-batch"), (1025, "head-batch"), (5, None)):
        with pytest.raises(ValueError):
            predict_top_k(m, s, mode, k)
    with pytest.raises(ValueError, match="outside"):
        predict_top_k(m, torch.tensor([[N, 0, 0]], device="cuda"), "tail-batch", 3)
    lib, tb = _hip.lib(), m._tables()
    need = lib.mkb_topk_workspace_bytes(tb, 2, 10)
    ws = _hip.aligned_bytes(need, "cuda")
    ids = torch.full((2, 1025), 7, dtype=torch.int64, device="cuda")
    sc = torch.full((2, 1025), 7.0, device="cuda")
    for k, mode in ((0, _hip.MODE_TAIL), (1025, _hip.MODE_HEAD), (5, _hip.MODE_DEFAULT)):
        rc = lib.mkb_topk(tb, _hip.ptr(s), 2, mode, None, 0, k, 0, _hip.ptr(ids), _hip.ptr(sc), ctypes.c_void_p(ws.data_ptr()), need,
                          _hip.stream_ptr())
        assert rc == _hip.ERR_INVALID, (k, mode)
    torch.cuda.synchronize()
    assert (ids == 7).all() and (sc == 7.0).all()
    ids, sc = predict_top_k(m, s, "tail-batch", 10)
    assert ids.shape == (2, 10) and (ids >= 0).all()
