"""CPU (-m "not gpu") tests of the candidate-masked and block top k (mkb_topk_masked, mkb_topk_block) and of the teacher top-k
samplers' host side: declarations, argument checks before any launch, predict_top_k(candidates=...) validation, the samplers'
mappings and sizes."""
import ctypes
import re

import pytest
import torch


def test_masked_and_block_declarations_match_the_binding():
    from conftest import ROOT
    from mkb_amd import _hip

    header = (ROOT / "include" / "mkb_hip.h").read_text()
    decl = re.search(r"\bint mkb_topk_masked\(([^)]*)\);", header)
    assert decl
    assert [" ".join(a.split()) for a in decl.group(1).split(",")] == [
        "const mkb_tables_t *tb", "const int64_t *sample", "int64_t B", "int mode", "const int64_t *true_keys", "int64_t n_true",
        "const uint32_t *cand_bits", "int k", "int flags", "int64_t *ids", "float *scores", "void *ws", "int64_t ws_bytes",
        "void *stream"]
    decl = re.search(r"\bint mkb_topk_block\(([^)]*)\);", header)
    assert decl
    assert [" ".join(a.split()) for a in decl.group(1).split(",")] == [
        "const float *S", "int64_t B", "int64_t N", "int64_t ld", "int k", "int64_t *ids", "float *scores", "void *stream"]
    c = ctypes
    assert _hip._SIGNATURES["mkb_topk_masked"] == (c.c_int, [c.POINTER(_hip.Tables), c.c_void_p, c.c_int64, c.c_int, c.c_void_p,
                                                             c.c_int64, c.c_void_p, c.c_int, c.c_int, c.c_void_p, c.c_void_p,
                                                             c.c_void_p, c.c_int64, c.c_void_p])
    assert _hip._SIGNATURES["mkb_topk_block"] == (c.c_int, [c.c_void_p, c.c_int64, c.c_int64, c.c_int64, c.c_int, c.c_void_p,
                                                            c.c_void_p, c.c_void_p])
    lib = ctypes.CDLL(str(ROOT / "mkb_amd" / "libmkb_hip.so"))
    assert hasattr(lib, "mkb_topk_masked") and hasattr(lib, "mkb_topk_block")
    assert _hip.ABI_VERSION == 9


def test_masked_and_block_reject_bad_arguments_before_any_launch():
    from mkb_amd import _hip

    lib = _hip.lib()
    fake = ctypes.c_void_p(0x10000)
    tb = _hip.Tables(_hip.MODEL_IDS["RotatE"], 8, 100, 3, 16, 8, fake, fake, fake, 6.0, 1.0)
    ws_ok = lib.mkb_topk_workspace_bytes(tb, 4, 10)
    ws = ctypes.c_void_p(0x100000)

    def masked(B=4, mode=_hip.MODE_TAIL, n_true=0, bits=fake, k=10, flags=0, ids=fake, scores=fake, ws=ws, ws_bytes=ws_ok,
               sample=fake):
        return lib.mkb_topk_masked(tb, sample, B, mode, None, n_true, bits, k, flags, ids, scores, ws, ws_bytes, None)

    for kw in [dict(k=0), dict(k=1025), dict(mode=_hip.MODE_DEFAULT), dict(flags=2), dict(B=0), dict(B=-1),
               dict(ws_bytes=ws_ok - 1), dict(ws=ctypes.c_void_p(0x100010)), dict(ids=None), dict(scores=None), dict(sample=None),
               dict(n_true=3), dict(bits=None, k=0)]:
        assert masked(**kw) == _hip.ERR_INVALID, kw

    def block(S=fake, B=4, N=8, ld=8, k=4, ids=fake, scores=fake):
        return lib.mkb_topk_block(S, B, N, ld, k, ids, scores, None)

    for kw in [dict(k=0), dict(k=1025), dict(B=-1), dict(B=1 << 31), dict(ld=7), dict(N=0), dict(N=1 << 31, ld=1 << 31),
               dict(ids=None), dict(scores=None), dict(S=None)]:
        assert block(**kw) == _hip.ERR_INVALID, kw
    assert block(B=0) == 0  # nothing to do: no launch


def test_candidate_bits_and_predict_top_k_validation():
    from mkb_amd import models
    from mkb_amd.utils import candidate_bits, predict_top_k

    bits = candidate_bits([0, 33, 5, 5], 40, "cpu")
    assert bits.dtype == torch.int32 and bits.tolist() == [(1 << 0) | (1 << 5), 1 << 1]
    assert candidate_bits(torch.ones(40, dtype=torch.bool), 40, "cpu").tolist() == [-1, 255]
    assert candidate_bits([], 40, "cpu").tolist() == [0, 0]
    m = models.RotatE(hidden_dim=4, entities={i: i for i in range(5)}, relations={0: 0}, gamma=1)
    s = torch.tensor([[0, 0, 1]])
    for bad in ([5], [-1], torch.ones(4, dtype=torch.bool), torch.ones((5, 1), dtype=torch.bool), [0.5, 1.0]):
        with pytest.raises(ValueError):
            predict_top_k(m, s, "tail-batch", 3, candidates=bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        predict_top_k(m, s, "tail-batch", 3, candidates=[0, 2])


def test_topk_sampling_mappings_and_sizes():
    from mkb_amd import distillation, models

    t_ents = {"a": 0, "b": 1, "c": 2, "d": 3}
    s_ents = {"d": 0, "b": 7, "x": 1, "c": 2}
    t_rels = {"r": 0, "s": 1, "q": 2}
    s_rels = {"q": 0, "s": 1}
    ts = distillation.TopKSampling(teacher_entities=t_ents, teacher_relations=t_rels, student_entities=s_ents,
                                   student_relations=s_rels, batch_size_entity=2, batch_size_relation=1, n_random_entities=1,
                                   n_random_relations=1, seed=3)
    assert ts.supervised is False and ts.depends_on_teacher is True
    assert list(ts.mapping_entities.items()) == [(1, 7), (2, 2), (3, 0)]
    assert list(ts.mapping_relations.items()) == [(1, 1), (2, 0)]
    assert (ts.batch_size_entity, ts.batch_size_relation) == (3, 2)
    tb = ts.tables("cpu")
    assert tb["ent_map"].tolist() == [-1, 7, 2, 0] and tb["rel_map"].tolist() == [-1, 1, 0]
    assert tb["rel_t"].tolist() == [1, 2] and tb["rel_s"].tolist() == [1, 0]
    assert tb["ent_bits"].tolist() == [0b1110]
    for k_e, k_r in ((4, 1), (2, 3), (0, 1)):
        with pytest.raises(ValueError):
            distillation.TopKSampling(teacher_entities=t_ents, teacher_relations=t_rels, student_entities=s_ents,
                                      student_relations=s_rels, batch_size_entity=k_e, batch_size_relation=k_r,
                                      n_random_entities=0, n_random_relations=0)
    m = models.RotatE(hidden_dim=4, entities=t_ents, relations=t_rels, gamma=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ts.get(sample=torch.tensor([[0, 1, 2]]), teacher=m)
    transe = models.TransE(hidden_dim=4, entities=t_ents, relations=t_rels, gamma=1)
    with pytest.raises(ImportError, match="faiss"):
        distillation.FastTopKSampling(teacher_entities=t_ents, teacher_relations=t_rels, student_entities=s_ents,
                                      student_relations=s_rels, batch_size_entity=2, batch_size_relation=1, n_random_entities=0,
                                      n_random_relations=0, dataset_teacher=[], teacher=transe)


@pytest.mark.parametrize("what", ["entity", "relation"])
def test_one_constructor_checks_both_sizes(what):
    """The samplers' one constructor: a top k of 0, past the shared set or past TOPK_MAX_K, and a random size below 0 or past the
    shared set, raise ValueError -- for entities and for relations."""
    from mkb_amd import _hip, distillation

    big = _hip.TOPK_MAX_K + 6  # shared labels: more than the largest k, so that only the k bound can refuse it
    dicts = {f"teacher_{w}": {f"x{i}": i for i in range(big)} for w in ("entities", "relations")}
    dicts.update({f"student_{w}": {f"x{i}": i for i in range(5, big + 5)} for w in ("entities", "relations")})  # big - 5 shared
    shared = big - 5
    ok = dict(batch_size_entity=2, batch_size_relation=2, n_random_entities=1, n_random_relations=1)
    ts = distillation.TopKSampling(**dicts, **ok)
    assert len(ts.mapping_entities) == len(ts.mapping_relations) == shared > _hip.TOPK_MAX_K
    plural = "entities" if what == "entity" else "relations"
    for bad in ({f"batch_size_{what}": 0}, {f"batch_size_{what}": shared + 1}, {f"batch_size_{what}": _hip.TOPK_MAX_K + 1},
                {f"n_random_{plural}": -1}, {f"n_random_{plural}": shared + 1}):
        with pytest.raises(ValueError):
            distillation.TopKSampling(**dicts, **{**ok, **bad})
    small = {k: ({f"x{i}": i for i in range(4)} if k.endswith(plural) else v) for k, v in dicts.items()}
    with pytest.raises(ValueError):  # within TOPK_MAX_K, past the 4 shared
        distillation.TopKSampling(**small, **{**ok, f"batch_size_{what}": 5})
