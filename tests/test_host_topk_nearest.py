"""CPU (-m "not gpu") tests of the exact squared-L2 k nearest rows (mkb_topk_nearest) and of the TransE teacher's sampler on its
host side: declarations, argument checks before any launch, the sampler's mappings and sizes, FastTopKSampling's ImportError."""
import ctypes
import re

import pytest
import torch


def test_nearest_declarations_match_the_binding():
    from conftest import ROOT
    from mkb_amd import _hip

    header = (ROOT / "include" / "mkb_hip.h").read_text()
    common = ["const float *Q", "int64_t ldq", "const float *X", "int64_t ldx", "const int64_t *cand", "int64_t n_cand", "int64_t B",
              "int64_t D", "int k", "int64_t *ids", "float *dists"]
    tail = ["void *ws", "int64_t ws_bytes", "void *stream"]
    for name, args in (("mkb_topk_nearest", common + tail), ("mkb_topk_nearest_dists", common + ["float *block"] + tail)):
        decl = re.search(r"\bint " + name + r"\(([^)]*)\);", header)
        assert decl, name
        assert [" ".join(a.split()) for a in decl.group(1).split(",")] == args
    assert re.search(r"\bint64_t mkb_topk_nearest_workspace_bytes\(int64_t B, int64_t n_cand, int k\);", header)
    c = ctypes
    base = [c.c_void_p, c.c_int64, c.c_void_p, c.c_int64, c.c_void_p, c.c_int64, c.c_int64, c.c_int64, c.c_int, c.c_void_p, c.c_void_p]
    assert _hip._SIGNATURES["mkb_topk_nearest"] == (c.c_int, base + [c.c_void_p, c.c_int64, c.c_void_p])
    assert _hip._SIGNATURES["mkb_topk_nearest_dists"] == (c.c_int, base + [c.c_void_p, c.c_void_p, c.c_int64, c.c_void_p])
    assert _hip._SIGNATURES["mkb_topk_nearest_workspace_bytes"] == (c.c_int64, [c.c_int64, c.c_int64, c.c_int])
    lib = ctypes.CDLL(str(ROOT / "mkb_amd" / "libmkb_hip.so"))
    for name in ("mkb_topk_nearest", "mkb_topk_nearest_dists", "mkb_topk_nearest_workspace_bytes"):
        assert hasattr(lib, name)
    assert _hip.ABI_VERSION == 9


def test_nearest_rejects_bad_arguments_before_any_launch():
    from mkb_amd import _hip

    lib = _hip.lib()
    fake = ctypes.c_void_p(0x10000)
    ws_ok = lib.mkb_topk_nearest_workspace_bytes(4, 100, 10)
    assert ws_ok >= 4 * 100 * 4 and ws_ok % 256 == 0
    assert lib.mkb_topk_nearest_workspace_bytes(4, 100, 0) == 0 and lib.mkb_topk_nearest_workspace_bytes(0, 100, 10) == 0
    assert lib.mkb_topk_nearest_workspace_bytes(4, 0, 10) == 0 and lib.mkb_topk_nearest_workspace_bytes(4, 100, 1025) == 0
    # a pass holds about 2^24 distances: the workspace does not grow with B past that
    assert lib.mkb_topk_nearest_workspace_bytes(1 << 30, 14541, 10) == lib.mkb_topk_nearest_workspace_bytes(1 << 20, 14541, 10) < 1 << 27
    ws = ctypes.c_void_p(0x100000)

    def call(Q=fake, ldq=8, X=fake, ldx=8, cand=fake, n=100, B=4, D=8, k=10, ids=fake, d=fake, ws=ws, ws_bytes=ws_ok, block=None,
             dists=False):
        if dists:
            return lib.mkb_topk_nearest_dists(Q, ldq, X, ldx, cand, n, B, D, k, ids, d, block, ws, ws_bytes, None)
        return lib.mkb_topk_nearest(Q, ldq, X, ldx, cand, n, B, D, k, ids, d, ws, ws_bytes, None)

    for kw in [dict(k=0), dict(k=1025), dict(B=-1), dict(B=1 << 31), dict(n=0), dict(n=1 << 31), dict(D=0), dict(ldq=7), dict(ldx=7),
               dict(Q=None), dict(X=None), dict(cand=None), dict(ids=None), dict(d=None), dict(ws=None), dict(ws_bytes=ws_ok - 1),
               dict(ws=ctypes.c_void_p(0x100010)), dict(dists=True), dict(dists=True, block=fake, k=0)]:
        assert call(**kw) == _hip.ERR_INVALID, kw
    assert call(B=0, ws=None, ws_bytes=0) == 0  # nothing to do: no launch


def _dicts():
    t_ents = {"a": 0, "b": 1, "c": 2, "d": 3}
    s_ents = {"d": 0, "b": 7, "x": 1, "c": 2}
    t_rels = {"r": 0, "s": 1, "q": 2}
    s_rels = {"q": 0, "s": 1}
    return dict(teacher_entities=t_ents, teacher_relations=t_rels, student_entities=s_ents, student_relations=s_rels)


def test_topk_sampling_transe_mappings_and_sizes():
    from mkb_amd import distillation, models

    kw = _dicts()
    torch.manual_seed(0)
    teacher = models.TransE(hidden_dim=4, entities=kw["teacher_entities"], relations=kw["teacher_relations"], gamma=1)
    ts = distillation.TopKSamplingTransE(teacher=teacher, batch_size_entity=2, batch_size_relation=1, n_random_entities=1,
                                         n_random_relations=1, seed=3, dataset_teacher=None, device="cpu", **kw)
    assert ts.supervised is False and ts.depends_on_teacher is True
    assert list(ts.mapping_entities.items()) == [(1, 7), (2, 2), (3, 0)]
    assert list(ts.mapping_relations.items()) == [(1, 1), (2, 0)]
    assert (ts.batch_size_entity, ts.batch_size_relation) == (3, 2)
    ent_rows, ent_ids, _ = ts._index["entity"]
    rel_rows, rel_ids, _ = ts._index["relation"]
    assert ent_ids.tolist() == [1, 2, 3] and rel_ids.tolist() == [1, 2]  # the index: shared rows in ascending teacher id
    assert torch.equal(ent_rows, teacher.entity_embedding.detach()[[1, 2, 3]])
    assert torch.equal(rel_rows, teacher.relation_embedding.detach()[[1, 2]])
    tb = ts.tables("cpu")
    assert tb["ent_map"].tolist() == [-1, 7, 2, 0] and tb["rel_map"].tolist() == [-1, 1, 0]
    for k_e, k_r, n_e in ((4, 1, 0), (2, 3, 0), (0, 1, 0), (2, 1, 4)):
        with pytest.raises(ValueError):
            distillation.TopKSamplingTransE(teacher=teacher, batch_size_entity=k_e, batch_size_relation=k_r, n_random_entities=n_e,
                                            n_random_relations=0, **kw)
    rot = models.RotatE(hidden_dim=4, entities=kw["teacher_entities"], relations=kw["teacher_relations"], gamma=1)
    with pytest.raises(ValueError, match="TransE"):
        distillation.TopKSamplingTransE(teacher=rot, batch_size_entity=2, batch_size_relation=1, n_random_entities=0,
                                        n_random_relations=0, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ts.get(sample=torch.tensor([[1, 1, 2]]), teacher=teacher)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        teacher._top_k(torch.tensor([[1, 1, 2]]))
    assert "TopKSamplingTransE" in distillation.__all__


def test_fast_topk_sampling_transe_teacher_without_the_keyword_raises_import_error():
    from mkb_amd import distillation, models

    kw = _dicts()
    transe = models.TransE(hidden_dim=4, entities=kw["teacher_entities"], relations=kw["teacher_relations"], gamma=1)
    with pytest.raises(ImportError, match="faiss") as err:
        distillation.FastTopKSampling(batch_size_entity=2, batch_size_relation=1, n_random_entities=0, n_random_relations=0,
                                      dataset_teacher=[], teacher=transe, **kw)
    assert "transe_sampler" in str(err.value) and "TopKSamplingTransE" in str(err.value)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # with it: built, then the device is required
        distillation.FastTopKSampling(batch_size_entity=2, batch_size_relation=1, n_random_entities=0, n_random_relations=0,
                                      dataset_teacher=[], teacher=transe, transe_sampler=distillation.TopKSamplingTransE, **kw)
