"""-m gpu: the exact squared-L2 k nearest rows (mkb_topk_nearest / mkb_topk_nearest_dists in mkb_amd/csrc/rank.hip) on both
routes: the register tile (D % 4 == 0, D >= 64, contiguous 16-byte aligned rows) and the general lane-per-candidate kernel.

The selection is checked exactly against a stable ascending sort of the device's own distance block (NaN first, then smaller
distance, then lower position in the candidate list); the block against float64 numpy to a relative 1e-5 of the distance scale;
the ids against a float64 numpy kNN wherever the k-th and (k+1)-th distances stand clearly apart."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _nearest(Q, X, cand, k):
    """-> (ids, dists, block) of mkb_topk_nearest_dists, and (ids, dists) of mkb_topk_nearest (must agree bit for bit)."""
    from mkb_amd.utils.predict_top_k import topk_nearest

    block = torch.full((Q.shape[0], cand.numel()), float("nan"), device="cuda")
    ids, d = topk_nearest(Q, X, cand, k, block=block)
    ids2, d2 = topk_nearest(Q, X, cand, k)
    assert torch.equal(ids, ids2) and torch.equal(d.view(torch.int32), d2.view(torch.int32))
    return ids.cpu().numpy(), d.cpu().numpy(), block.cpu().numpy()


def _sorted_block(block, cand, k):
    """A stable ascending sort of each row: NaN first, then smaller distance, then lower position; -1 / +inf past the row."""
    B, n = block.shape
    nan = np.isnan(block)
    order = np.lexsort((np.broadcast_to(np.arange(n), (B, n)), np.where(nan, 0.0, block), ~nan), axis=-1)[:, :k]
    ids = np.full((B, k), -1, dtype=np.int64)
    d = np.full((B, k), np.inf, dtype=np.float32)
    m = min(k, n)
    ids[:, :m] = cand[order[:, :m]]
    d[:, :m] = np.take_along_axis(block, order[:, :m], axis=1)
    return ids, d


def _f64_block(Q, X, cand):
    q, x = Q.double().cpu().numpy(), X.double().cpu().numpy()[cand]
    return np.stack([((x - row) ** 2).sum(1) for row in q]) if len(q) else np.zeros((0, len(cand)))


def _check(Q, X, cand_t, k, f64=True):
    cand = cand_t.cpu().numpy()
    ids, d, block = _nearest(Q, X, cand_t, k)
    want_ids, want_d = _sorted_block(block, cand, k)
    np.testing.assert_array_equal(ids, want_ids)
    ok = ~np.isnan(want_d)
    np.testing.assert_array_equal(np.isnan(d), ~ok)
    np.testing.assert_array_equal(d[ok].view(np.uint32), want_d[ok].view(np.uint32))
    if f64 and Q.shape[0]:
        ref = _f64_block(Q, X, cand)
        scale = max(ref.max(), 1e-30)
        np.testing.assert_allclose(block, ref, rtol=0, atol=1e-5 * scale)
        if k < cand.size:  # ids against the float64 kNN where the k-th / (k+1)-th gap is clear
            srt = np.sort(ref, axis=1)
            clear = (srt[:, k] - srt[:, k - 1]) > 1e-4 * srt[:, k]
            order = np.argsort(ref, axis=1, kind="stable")[:, :k]
            assert clear.mean() > 0.5
            np.testing.assert_array_equal(np.sort(ids[clear], axis=1), np.sort(cand[order[clear]], axis=1))
    return ids, d, block


def _data(B, n_rows, D, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    Q = (torch.rand((B, D), generator=g) * 2 - 1) * scale
    X = (torch.rand((n_rows, D), generator=g) * 2 - 1) * scale
    return Q.cuda(), X.cuda()


@pytest.mark.parametrize("D", [64, 128, 1000, 1, 3, 6, 63, 130])
@pytest.mark.parametrize("n_cand", [1, 63, 64, 65, 1000])
def test_nearest_exact_on_both_routes(D, n_cand):
    """Tile shapes (D = 64, 128, 1000) and general ones (1, 3, 6, 63, 130), candidate counts around the tile's 64, ragged B."""
    Q, X = _data(77, 1200, D, seed=D * 7 + n_cand)
    rs = np.random.RandomState(n_cand)
    cand = torch.as_tensor(rs.permutation(1200)[:n_cand]).cuda()  # unsorted
    for k in sorted({1, min(10, n_cand), n_cand, n_cand + 5}):
        _check(Q, X, cand, k)


def test_nearest_fb15k237_shape_and_max_k():
    """14,541 candidates (FB15k-237's entity count) at D = 1000 and D = 6; k = 10, 100 and MKB_TOPK_MAX_K."""
    from mkb_amd import _hip

    for D in (1000, 6):
        Q, X = _data(130, 14541, D, seed=D)
        cand = torch.arange(14541, device="cuda")
        for k in (10, 100, _hip.TOPK_MAX_K):
            _check(Q, X, cand, k, f64=D == 6 or k == 10)


def test_nearest_routes_agree_bit_for_bit():
    """A table view offset by one float (not 16-byte aligned) forces the general route at D = 128: the same ids and the same
    distance bits as the tile route on the same data; a row stride past D (a column slice) as well."""
    Q, X = _data(100, 3000, 128, seed=5)
    cand = torch.as_tensor(np.random.RandomState(3).permutation(3000)[:2000]).cuda()
    a = _nearest(Q, X, cand, 50)
    flat = torch.empty(3000 * 128 + 1, device="cuda")
    flat[1:] = X.reshape(-1)
    Xoff = flat[1:].view(3000, 128)
    assert Xoff.data_ptr() % 16 != 0
    b = _nearest(Q, Xoff, cand, 50)
    wide = torch.zeros((3000, 132), device="cuda")
    wide[:, :128] = X
    c = _nearest(Q, wide[:, :128], cand, 50)
    for other in (b, c):
        np.testing.assert_array_equal(a[0], other[0])
        np.testing.assert_array_equal(a[1].view(np.uint32), other[1].view(np.uint32))
        np.testing.assert_array_equal(a[2].view(np.uint32), other[2].view(np.uint32))


def test_nearest_duplicates_ties_and_nan():
    """Duplicate candidates and equal rows tie exactly (lower position first); a NaN query row gives NaN distances, ordered by
    position; a NaN table row comes first for every query."""
    for D in (64, 5):
        Q, X = _data(20, 50, D, seed=D)
        X[7] = X[3]
        X[9] = float("nan")
        Q[4] = float("nan")
        cand = torch.tensor([3, 7, 3, 12, 9, 40, 7, 0, 1, 2, 3, 30], device="cuda")
        ids, d, block = _check(Q, X, cand, 12, f64=False)
        assert (np.delete(ids[:, 0], 4) == 9).all() and np.isnan(d[:, 0]).all()
        assert (ids[4] == cand.cpu().numpy()).all() and np.isnan(d[4]).all()
        for i in set(range(20)) - {4}:  # the five copies of one row (positions 0, 1, 2, 6, 10) sit together in position order
            row = list(ids[i])
            j = row.index(3)
            assert row[j: j + 5] == [3, 7, 3, 7, 3] and len(set(d[i, j: j + 5].view(np.uint32))) == 1


def test_nearest_common_offset():
    """Rows near 1e3 that differ by about 1e-2: |q|^2 + |x|^2 - 2 q.x in fp32 loses the distance entirely; the difference form
    gives the float64 order."""
    rs = np.random.RandomState(0)
    for D in (64, 7):
        base = rs.uniform(999, 1001, size=(1, D))
        X = torch.as_tensor((base + rs.normal(0, 1e-2, size=(500, D))).astype(np.float32)).cuda()
        Q = torch.as_tensor((base + rs.normal(0, 1e-2, size=(40, D))).astype(np.float32)).cuda()
        cand = torch.arange(500, device="cuda")
        ids, d, block = _check(Q, X, cand, 5)
        q, x = Q.double().cpu().numpy(), X.double().cpu().numpy()
        gemm = (q * q).sum(1)[:, None] + (x * x).sum(1)[None, :] - 2 * q @ x.T
        gemm32 = ((Q * Q).sum(1)[:, None] + (X * X).sum(1)[None, :] - 2 * Q @ X.T).cpu().numpy()
        ref = _f64_block(Q, X, np.arange(500))
        assert np.abs(gemm - ref).max() < 1e-6  # (float64 is fine either way)
        assert (np.argsort(gemm32, axis=1)[:, :5] != np.argsort(ref, axis=1)[:, :5]).any()  # fp32 GEMM form: wrong order


@pytest.mark.parametrize("B", [0, 1, 70000])
def test_nearest_batch_sizes(B):
    """B = 0 (nothing launched), one query, and more queries than a grid dimension holds (65,535) at small D and n_cand."""
    Q, X = _data(B, 30, 3, seed=B)
    cand = torch.arange(0, 30, 3, device="cuda")
    if B == 0:
        from mkb_amd.utils.predict_top_k import topk_nearest

        ids, d = topk_nearest(Q, X, cand, 4)
        assert ids.shape == (0, 4) and d.shape == (0, 4)
        return
    _check(Q, X, cand, 4)


def test_nearest_many_passes():
    """n_cand large enough that one call takes several passes of 64 queries (2^24 floats per pass): the pass seams."""
    Q, X = _data(130, 270000, 64, seed=11)
    cand = torch.as_tensor(np.random.RandomState(1).permutation(270000)).cuda()
    ids, d, block = _nearest(Q, X, cand, 20)
    want_ids, want_d = _sorted_block(block, cand.cpu().numpy(), 20)
    np.testing.assert_array_equal(ids, want_ids)
    np.testing.assert_array_equal(d.view(np.uint32), want_d.view(np.uint32))


def test_nearest_rejects_bad_arguments_on_the_device():
    import ctypes

    from mkb_amd import _hip

    lib = _hip.lib()
    Q, X = _data(4, 10, 8, seed=1)
    cand = torch.arange(10, device="cuda")
    ids = torch.full((4, 3), 7, dtype=torch.int64, device="cuda")
    d = torch.zeros((4, 3), device="cuda")
    need = lib.mkb_topk_nearest_workspace_bytes(4, 10, 3)
    ws = _hip.aligned_bytes(need, torch.device("cuda"))
    p = _hip.ptr
    args = [p(Q), 8, p(X), 8, p(cand), 10, 4, 8, 3, p(ids), p(d), p(ws), need, _hip.stream_ptr()]
    assert lib.mkb_topk_nearest(*args) == 0
    for i, bad in ((1, 7), (3, 7), (5, 0), (6, -1), (7, 0), (8, 0), (8, 1025), (12, need - 1), (11, ctypes.c_void_p(ws.data_ptr() + 16))):
        a = list(args)
        a[i] = bad
        assert lib.mkb_topk_nearest(*a) == _hip.ERR_INVALID, (i, bad)
    torch.cuda.synchronize()
