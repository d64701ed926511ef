"""CPU (-m "not gpu") tests of the top-k entity prediction's host side: the C ABI (include/mkb_hip.h, since ABI 7) exports mkb_topk and
mkb_topk_workspace_bytes with the declared signatures, rejects bad arguments before any launch, and the Python API validates its
arguments and refuses a CPU model."""
import ctypes
import re

import pytest
import torch


def test_topk_symbols_and_abi():
    from conftest import ROOT
    from mkb_amd import _hip

    header = (ROOT / "include" / "mkb_hip.h").read_text()
    assert re.search(r"#define MKB_ABI_VERSION 9\b", header)
    assert re.search(r"#define MKB_TOPK_MAX_K 1024\b", header) and re.search(r"#define MKB_TOPK_KEEP_TARGET 1\b", header)
    assert _hip.ABI_VERSION == 9 and (_hip.TOPK_MAX_K, _hip.TOPK_KEEP_TARGET) == (1024, 1)
    decl = re.search(r"int64_t mkb_topk_workspace_bytes\(([^)]*)\);", header)
    assert decl and [a.split()[-1].lstrip("*") for a in decl.group(1).split(",")] == ["tb", "B", "k"]
    decl = re.search(r"\bint mkb_topk\(([^)]*)\);", header)
    assert decl
    params = [" ".join(a.split()) for a in decl.group(1).split(",")]
    assert params == ["const mkb_tables_t *tb", "const int64_t *sample", "int64_t B", "int mode", "const int64_t *true_keys",
                      "int64_t n_true", "int k", "int flags", "int64_t *ids", "float *scores", "void *ws", "int64_t ws_bytes",
                      "void *stream"], params
    c = ctypes
    assert _hip._SIGNATURES["mkb_topk_workspace_bytes"] == (c.c_int64, [c.POINTER(_hip.Tables), c.c_int64, c.c_int])
    assert _hip._SIGNATURES["mkb_topk"] == (c.c_int, [c.POINTER(_hip.Tables), c.c_void_p, c.c_int64, c.c_int, c.c_void_p, c.c_int64,
                                                      c.c_int, c.c_int, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_void_p])
    lib = ctypes.CDLL(str(ROOT / "mkb_amd" / "libmkb_hip.so"))
    assert hasattr(lib, "mkb_topk") and hasattr(lib, "mkb_topk_workspace_bytes")
    assert _hip.lib().mkb_abi_version() == 9


def _fake_tables():
    """A RotatE table description whose pointers are never dereferenced (every call below fails validation first)."""
    from mkb_amd import _hip

    fake = ctypes.c_void_p(0x10000)
    return _hip.Tables(_hip.MODEL_IDS["RotatE"], 8, 100, 3, 16, 8, fake, fake, fake, 6.0, 1.0), fake


def test_topk_abi_rejects_bad_arguments_before_any_launch():
    from mkb_amd import _hip

    lib = _hip.lib()
    tb, p = _fake_tables()
    ws_ok = lib.mkb_rank_workspace_bytes(tb, 4)
    assert ws_ok > 0
    assert lib.mkb_topk_workspace_bytes(tb, 4, 10) == ws_ok
    assert lib.mkb_topk_workspace_bytes(tb, 4, 0) == 0 and lib.mkb_topk_workspace_bytes(tb, 4, 1025) == 0
    ws = ctypes.c_void_p(0x100000)  # 256-byte aligned

    def call(B=4, mode=_hip.MODE_TAIL, keys=None, n_true=0, k=10, flags=0, ids=p, scores=p, ws=ws, ws_bytes=ws_ok, sample=p):
        return lib.mkb_topk(tb, sample, B, mode, keys, n_true, k, flags, ids, scores, ws, ws_bytes, None)

    for kw in [dict(k=0), dict(k=1025), dict(k=-3), dict(mode=_hip.MODE_DEFAULT), dict(mode=7), dict(flags=2), dict(flags=-1),
               dict(B=0), dict(B=-1), dict(B=1 << 31), dict(ws_bytes=ws_ok - 1), dict(ws=ctypes.c_void_p(0x100010)),
               dict(ids=None), dict(scores=None), dict(ws=None), dict(sample=None), dict(n_true=5)]:
        assert call(**kw) == _hip.ERR_INVALID, kw
    bad = _hip.Tables(99, 8, 100, 3, 16, 8, p, p, p, 6.0, 1.0)
    assert lib.mkb_topk(bad, p, 4, _hip.MODE_TAIL, None, 0, 10, 0, p, p, ws, ws_ok, None) == _hip.ERR_INVALID


def test_predict_top_k_validates_and_refuses_the_cpu():
    from mkb_amd import datasets, evaluation, models
    from mkb_amd.utils import predict_top_k

    m = models.RotatE(hidden_dim=4, entities={i: i for i in range(5)}, relations={0: 0}, gamma=1)
    s = torch.tensor([[0, 0, 1]])
    for k in (0, 1025, -1, 2.5, None, True):
        with pytest.raises(ValueError, match="k must"):
            predict_top_k(m, s, "tail-batch", k)
    for mode in (None, "relation-batch", "default"):
        with pytest.raises(ValueError, match="mode"):
            predict_top_k(m, s, mode, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        predict_top_k(m, s, "tail-batch", 3)
    ev = evaluation.Evaluation(entities={i: i for i in range(5)}, relations={0: 0}, batch_size=2, true_triples=[(0, 0, 1)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev.top_k(m, [(0, 0, 1)], "head-batch", 3)
    with pytest.raises(ValueError):
        ev.top_k(m, [(0, 0, 1)], None, 3)


def test_true_keys_helper_matches_the_oracle_key_set():
    import numpy as np

    from oracle import ranking
    from mkb_amd.utils import true_keys

    rs = np.random.RandomState(3)
    N, R = 50, 4
    true = [tuple(t) for t in np.stack([rs.randint(N, size=300), rs.randint(R, size=300), rs.randint(N, size=300)], 1).tolist()]
    keys = true_keys(true, "cpu", N, R)
    np.testing.assert_array_equal(keys["tail-batch"].numpy(), ranking.true_key_set(true, N, R))
    flipped = [(t, r, h) for h, r, t in true]
    np.testing.assert_array_equal(keys["head-batch"].numpy(), ranking.true_key_set(flipped, N, R))
    assert true_keys(true, "cpu", N, R) is keys  # cached per collection
    true.append((0, 0, 0))
    assert true_keys(true, "cpu", N, R) is not keys  # ... and rebuilt when it grows
