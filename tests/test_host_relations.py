"""CPU (-m "not gpu") tests of the relation side's host part: the C ABI (include/mkb_hip.h, "relation prediction", under ABI 8)
exports mkb_rel_scores / mkb_rel_rank / mkb_rel_topk and the two workspace functions with the declared signatures and refuses bad
arguments before any launch; the Python entry points validate theirs and refuse a CPU model; predict_top_k keeps refusing the
relation side; and the numpy restatements the GPU tests compare the kernels with (tests/util_relations.py) agree with the torch
formula of Evaluation._relation_ranks_torch."""
import ctypes
import re

import numpy as np
import pytest
import torch

import util_relations as ur

DECLARED = {
    "mkb_rel_scores": ("int", ["const mkb_tables_t *tb", "const int64_t *sample", "int64_t B", "const int64_t *rel_ids", "int64_t n_rel",
                               "float *scores", "int64_t ld", "void *stream"]),
    "mkb_rel_rank_workspace_bytes": ("int64_t", ["const mkb_tables_t *tb", "int64_t B"]),
    "mkb_rel_rank": ("int", ["const mkb_tables_t *tb", "const int64_t *sample", "int64_t B", "const int64_t *true_keys", "int64_t n_true",
                             "int64_t *rank", "float *scores", "void *ws", "int64_t ws_bytes", "void *stream"]),
    "mkb_rel_topk_workspace_bytes": ("int64_t", ["const mkb_tables_t *tb", "int64_t B", "int k"]),
    "mkb_rel_topk": ("int", ["const mkb_tables_t *tb", "const int64_t *sample", "int64_t B", "const int64_t *true_keys", "int64_t n_true",
                             "int k", "int flags", "int64_t *ids", "float *scores", "void *ws", "int64_t ws_bytes", "void *stream"]),
}


def test_relation_symbols_signatures_and_abi():
    from conftest import ROOT
    from mkb_amd import _hip

    header = (ROOT / "include" / "mkb_hip.h").read_text()
    assert re.search(r"#define MKB_ABI_VERSION 9\b", header) and _hip.ABI_VERSION == 9
    lib = ctypes.CDLL(str(ROOT / "mkb_amd" / "libmkb_hip.so"))
    c = ctypes

    def ctype(param):
        if param == "const mkb_tables_t *tb":
            return c.POINTER(_hip.Tables)
        return c.c_void_p if "*" in param else {"int64_t": c.c_int64, "int": c.c_int}[param.split()[0]]

    for name, (res, params) in DECLARED.items():
        decl = re.search(r"\b%s %s\(([^)]*)\);" % (res, name), header)
        assert decl, name
        assert [" ".join(a.split()) for a in decl.group(1).split(",")] == params, name
        assert _hip._SIGNATURES[name] == ({"int": c.c_int, "int64_t": c.c_int64}[res], [ctype(p) for p in params]), name
        assert hasattr(lib, name), name
    assert _hip.lib().mkb_abi_version() == 9


def _fake_tables(model="RotatE"):
    """A table description whose pointers are never dereferenced (every call below fails validation first): N = 100, R = 3."""
    from mkb_amd import _hip

    fake = ctypes.c_void_p(0x10000)
    return _hip.Tables(_hip.MODEL_IDS[model], 8, 100, 3, 16, 8, fake, fake, fake, 6.0, 1.0), fake


def test_relation_abi_rejects_bad_arguments_before_any_launch():
    from mkb_amd import _hip

    lib = _hip.lib()
    tb, p = _fake_tables()
    bad_model = _hip.Tables(99, 8, 100, 3, 16, 8, p, p, p, 6.0, 1.0)
    long_rows = _hip.Tables(_hip.MODEL_IDS["TransE"], 4096, 100, 3, 4096, 4096, p, p, p, 6.0, 1.0)
    ws_ok = lib.mkb_rel_rank_workspace_bytes(tb, 4)
    assert ws_ok >= 4 * 3 * 4 + 4 * 4  # the [B, R] block and the [B, ceil(R / 32)] mask
    assert lib.mkb_rel_topk_workspace_bytes(tb, 4, 10) == ws_ok
    for B in (0, -1, 1 << 31):
        assert lib.mkb_rel_rank_workspace_bytes(tb, B) == 0 and lib.mkb_rel_topk_workspace_bytes(tb, B, 10) == 0
    assert lib.mkb_rel_rank_workspace_bytes(None, 4) == 0 and lib.mkb_rel_topk_workspace_bytes(None, 4, 10) == 0
    assert lib.mkb_rel_topk_workspace_bytes(tb, 4, 0) == 0 and lib.mkb_rel_topk_workspace_bytes(tb, 4, 1025) == 0
    ws = ctypes.c_void_p(0x100000)  # 256-byte aligned

    def refused(rc, what):
        assert rc == _hip.ERR_INVALID, what
        assert lib.mkb_last_error(), what

    def scores(tb=tb, sample=p, B=4, rel_ids=None, n_rel=3, out=p, ld=3):
        return lib.mkb_rel_scores(tb, sample, B, rel_ids, n_rel, out, ld, None)

    for kw in [dict(tb=None), dict(tb=bad_model), dict(sample=None), dict(out=None), dict(B=-1), dict(B=1 << 31), dict(ld=2),
               dict(n_rel=0), dict(n_rel=-2, ld=5), dict(n_rel=2), dict(n_rel=4, ld=4), dict(rel_ids=p, n_rel=5, ld=4),
               dict(rel_ids=p, n_rel=0)]:
        refused(scores(**kw), ("scores", kw))
    assert scores(B=0) == 0 and scores(B=0, rel_ids=p, n_rel=7, ld=9) == 0  # a valid call that launches nothing
    assert scores(tb=long_rows) == -5  # MKB_ERR_UNSUPPORTED: the caller keeps the general forward

    def rank(tb=tb, sample=p, B=4, keys=None, n_true=0, out=p, block=None, ws=ws, ws_bytes=ws_ok):
        return lib.mkb_rel_rank(tb, sample, B, keys, n_true, out, block, ws, ws_bytes, None)

    def topk(tb=tb, sample=p, B=4, keys=None, n_true=0, k=2, flags=0, ids=p, out=p, ws=ws, ws_bytes=ws_ok):
        return lib.mkb_rel_topk(tb, sample, B, keys, n_true, k, flags, ids, out, ws, ws_bytes, None)

    common = [dict(tb=None), dict(tb=bad_model), dict(sample=None), dict(out=None), dict(B=-1), dict(B=1 << 31), dict(n_true=5),
              dict(keys=p, n_true=-1), dict(ws=None), dict(ws_bytes=ws_ok - 1), dict(ws=ctypes.c_void_p(0x100010))]
    for kw in common:
        refused(rank(**kw), ("rank", kw))
    for kw in common + [dict(ids=None), dict(k=0), dict(k=1025), dict(k=-3), dict(flags=2), dict(flags=-1)]:
        refused(topk(**kw), ("topk", kw))
    assert rank(B=0) == 0 and rank(B=0, ws=None, ws_bytes=0) == 0 and topk(B=0) == 0 and topk(B=0, ws=None, ws_bytes=0, k=1024) == 0
    big = lib.mkb_rel_rank_workspace_bytes(long_rows, 4)
    assert rank(tb=long_rows, ws_bytes=big) == -5 and topk(tb=long_rows, ws_bytes=big) == -5


def test_python_entry_points_validate_and_refuse_the_cpu():
    from mkb_amd import evaluation, models
    from mkb_amd.utils import predict_top_k, predict_top_k_relations, relation_scores

    m = models.RotatE(hidden_dim=4, entities={i: i for i in range(5)}, relations={0: 0}, gamma=1)
    s = torch.tensor([[0, 0, 1]])
    for k in (0, 1025, -1, 2.5, None, True):
        with pytest.raises(ValueError, match="k must"):
            predict_top_k_relations(m, s, k)
    for chunk in (0, -4):
        with pytest.raises(ValueError, match="chunk"):
            predict_top_k_relations(m, s, 3, chunk=chunk)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        predict_top_k_relations(m, s, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        relation_scores(m, s)
    ev = evaluation.Evaluation(entities={i: i for i in range(5)}, relations={0: 0}, batch_size=2, true_triples=[(0, 0, 1)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev.top_k_relations(m, [(0, 0, 1)], 3)
    # the relation side has entry points of its own: predict_top_k keeps refusing it
    with pytest.raises(ValueError, match="mode"):
        predict_top_k(m, s, "relation-batch", 3)
    with pytest.raises(ValueError):
        ev.top_k(m, [(0, 0, 1)], None, 3)


class _TableModel:
    """A CPU stand-in for a model in Evaluation._relation_ranks_torch: the score of (h, r, t) is an entry of a fixed table."""

    def __init__(self, table):
        self.table = table  # [N, R, N]
        self.n_entity, self.n_relation = table.shape[0], table.shape[1]
        self.entity_embedding = table

    def __call__(self, triples):
        return self.table[triples[..., 0], triples[..., 1], triples[..., 2]]


@pytest.mark.parametrize("R", [1, 3, 65])
def test_restatements_agree_with_the_torch_formula(R):
    """tests/util_relations.py against Evaluation._relation_ranks_torch on random finite blocks: N = 50, a dense true set in which
    some queries have every other relation true."""
    from mkb_amd import evaluation
    from mkb_amd.utils import true_keys

    N, B = 50, 40
    rs = np.random.RandomState(100 + R)
    table = torch.as_tensor(rs.randint(-8, 8, size=(N, R, N)).astype(np.float32) / 4)  # coarse values: ties and a bias of -1 that lands on others
    sample = np.stack([rs.randint(N, size=B), rs.randint(R, size=B), rs.randint(N, size=B)], 1).astype(np.int64)
    sample[5] = sample[4]  # a duplicate query
    true = {(int(h), int(r), int(t)) for h, r, t in sample[: B // 2]}  # half of the targets are keys themselves
    for h, _, t in sample[:6]:  # every relation of these pairs is true
        true |= {(int(h), r, int(t)) for r in range(R)}
    for h, _, t in sample[6:]:
        true |= {(int(h), int(r), int(t)) for r in np.flatnonzero(rs.rand(R) < 0.4)}
    true |= {(int(a), int(b), int(c)) for a, b, c in zip(rs.randint(N, size=200), rs.randint(R, size=200), rs.randint(N, size=200))}
    true = sorted(true)
    ev = evaluation.Evaluation(entities={i: i for i in range(N)}, relations={i: i for i in range(R)}, batch_size=8, true_triples=true)
    model = _TableModel(table)
    want, block = ev._relation_ranks_torch(model, sample, chunk=16, with_scores=True)
    keys = true_keys(true, "cpu", N, R)["tail-batch"].numpy()
    mask = ur.filter_mask(sample, keys, N, R)
    assert mask[:6].all() and not mask.all() or R == 1
    np.testing.assert_array_equal(block.numpy(), table.numpy()[sample[:, 0], :, sample[:, 2]])
    got = ur.rel_ranks(block.numpy(), sample, mask)
    np.testing.assert_array_equal(got, want.numpy())
    np.testing.assert_array_equal(got[:6], 1)  # every other relation filtered: behind the target
    # the top k with the target kept puts the target at rank - 1 wherever the rank is at most k
    for k in (1, 5, R + 7):
        ids, scores = ur.rel_topk(block.numpy(), sample, mask, k, keep_target=True)
        for i in np.flatnonzero(got <= k):
            assert ids[i, got[i] - 1] == sample[i, 1]
        assert ((ids == -1) == np.isneginf(scores)).all()
        plain, _ = ur.rel_topk(block.numpy(), sample, mask, k, keep_target=False)
        assert (plain[:6] == -1).all()
