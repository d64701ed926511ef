"""CPU (-m "not gpu") tests of the grouped evaluation report (Evaluation.types_relations / detail_metrics / detail_eval; reference
evaluation/evaluation.py:282-464) against tests/golden/detail_eval.{npz,json}: the category map on numpy, and the host route of the
metrics (compute_detailled_score over the reference's candidate stream) with the oracle's CPU scoring standing in for the model."""
import ctypes

import numpy as np
import pytest
import torch

import util_detail_eval as U


class OracleModel(torch.nn.Module):
    """model(sample, negative_sample, mode) on CPU tensors by the oracle's restatement of the five forwards (not a BaseModel:
    Evaluation takes its host route)."""

    def __init__(self, name, ent, rel, hidden, gamma):
        super().__init__()
        from oracle import scoring

        self.tb = scoring.Tables(name, hidden, gamma, torch.as_tensor(ent).float(), torch.as_tensor(rel).float(), None)

    def forward(self, sample, negative_sample=None, mode=None):
        from oracle import scoring

        return scoring.score(self.tb, sample, negative_sample, mode)


def _evaluation(ds, **kw):
    from mkb_amd import evaluation

    return evaluation.Evaluation(true_triples=ds.true_triples, entities=ds.entities, relations=ds.relations, batch_size=64,
                                 num_workers=0, **kw)


def _toy(golden):
    from mkb_amd import evaluation

    g = golden("evaluation.npz")
    model = OracleModel("RotatE", g["ent"], g["rel"], 3, 1.0).eval()
    ev = evaluation.Evaluation(true_triples=U.TOY_TRUE, entities=U.TOY_ENTITIES, relations=U.TOY_RELATIONS, batch_size=2, num_workers=0)
    return model, ev


def test_metrics_symbols_are_declared_and_bound():
    import re

    from conftest import ROOT
    from mkb_amd import _hip

    header = (ROOT / "include" / "mkb_hip.h").read_text()
    decl = re.search(r"\bint mkb_relation_fanout\(([^)]*)\);", header)
    assert decl and [a.split()[-1].lstrip("*") for a in decl.group(1).split(",")] == [
        "triples", "n", "head_keys", "n_head", "tail_keys", "n_tail", "n_entity", "n_relation", "counts", "stream"]
    decl = re.search(r"\bint mkb_rank_metrics\(([^)]*)\);", header)
    assert decl and [a.split()[-1].lstrip("*") for a in decl.group(1).split(",")] == [
        "ranks", "sample", "n", "group_of_relation", "n_relation", "n_groups", "counts", "rr_sum", "stream"]
    assert len(_hip._SIGNATURES["mkb_relation_fanout"][1]) == 10 and len(_hip._SIGNATURES["mkb_rank_metrics"][1]) == 9
    lib = _hip.lib()
    assert hasattr(lib, "mkb_relation_fanout") and hasattr(lib, "mkb_rank_metrics")


def test_metrics_abi_rejects_bad_arguments_before_any_launch():
    from mkb_amd import _hip

    lib, p = _hip.lib(), ctypes.c_void_p(0x10000)  # never dereferenced: every call below fails validation first

    def fanout(triples=p, n=4, head=p, n_head=4, tail=p, n_tail=4, N=10, R=3, counts=p):
        return lib.mkb_relation_fanout(triples, n, head, n_head, tail, n_tail, N, R, counts, None)

    for kw in [dict(N=0), dict(N=-1), dict(R=0), dict(R=-5), dict(R=1 << 31), dict(n=-1), dict(n_head=-1), dict(n_tail=-1),
               dict(n=1 << 62), dict(counts=None), dict(triples=None), dict(head=None), dict(tail=None)]:
        assert fanout(**kw) == _hip.ERR_INVALID, kw

    def metrics(ranks=p, sample=p, n=4, table=p, R=3, G=4, counts=p, rr=p):
        return lib.mkb_rank_metrics(ranks, sample, n, table, R, G, counts, rr, None)

    for kw in [dict(R=0), dict(R=-1), dict(G=0), dict(G=-2), dict(n=-1), dict(n=1 << 62), dict(ranks=None), dict(sample=None),
               dict(table=None), dict(counts=None), dict(rr=None)]:
        assert metrics(**kw) == _hip.ERR_INVALID, kw
    assert b"null pointer" in lib.mkb_last_error()


def test_types_relations_docstring_case_counts_repeats(golden):
    """The reference's class docstring passes train + valid + test with repeated triples: 4 triples over 2 pairs make both
    relations M_M at threshold 1.5 only because every occurrence counts (without the repeats: 2 over 2, 1_1)."""
    from mkb_amd import evaluation

    rec = golden("detail_eval.json")["toy"]
    model, ev = _toy(golden)
    assert rec["types"] == {"r0": "M_M", "r1": "M_M"}
    assert ev.types_relations(model=model, dataset=U.TOY_TEST, threshold=1.5) == rec["types"]
    assert ev.types_relations(model=model, dataset=U.TOY_TEST, threshold=2.0 - 1e-9) == rec["types"]
    assert ev.types_relations(model=model, dataset=U.TOY_TEST, threshold=2.0) == {"r0": "1_1", "r1": "1_1"}
    once = evaluation.Evaluation(true_triples=U.TOY_TRAIN, entities=U.TOY_ENTITIES, relations=U.TOY_RELATIONS, batch_size=2)
    assert once.types_relations(model=model, dataset=U.TOY_TEST, threshold=1.5) == {"r0": "1_1", "r1": "1_1"}


@pytest.mark.parametrize("name", ["CountriesS1", "Umls"])
def test_types_relations_match_the_reference(golden, name):
    rec = golden("detail_eval.json")[f"{name}/TransE"]
    ds = U.dataset(name)
    ev = _evaluation(ds)
    for threshold in (1.5, 1.0):
        got = ev.types_relations(model=None, dataset=ds.test, threshold=threshold)
        assert got == rec["types"][str(threshold)]
        assert list(got) == sorted(got, key=ds.relations.get)  # in relation id order, like the reference's frame


def test_detail_metrics_and_frame_of_the_docstring_case(golden):
    rec = golden("detail_eval.json")["toy"]
    model, ev = _toy(golden)
    got = ev.detail_metrics(model=model, dataset=U.TOY_TEST, threshold=1.5)
    U.assert_metrics_close(got, rec["metrics"], 0.0)
    assert got["head-batch"]["M_M"] == {"MRR": 0.6667, "MR": 2.0, "HITS@1": 0.5, "HITS@3": 1.0, "HITS@10": 1.0}
    assert got["tail-batch"]["M_M"] == {"MRR": 0.4167, "MR": 2.5, "HITS@1": 0.0, "HITS@3": 1.0, "HITS@10": 1.0}
    assert got["tail-batch"]["1_1"] == dict.fromkeys(U.METRICS, 0.0) and got["frequency"]["M_M"] == 1.0
    pytest.importorskip("pandas")
    frame = ev.detail_eval(model=model, dataset=U.TOY_TEST, threshold=1.5)
    want = rec["frame"]
    assert list(frame.index) == want["index"] == list(U.TYPES)
    assert frame.index.name == "relation" and want["index_name"] is None  # the reference sets the name, its last concat drops it
    assert [list(c) for c in frame.columns] == want["columns"] and frame.columns.nlevels == 2
    assert frame.values.tolist() == want["values"]


@pytest.mark.parametrize("case", U.CASES)
def test_detail_metrics_host_route_matches_the_reference(golden, case):
    """Same stream, same running means: the rounded numbers are the reference's exactly, at both thresholds."""
    g, rec = golden("detail_eval.npz"), golden("detail_eval.json")[case]
    name, model_name = case.split("/")
    ds = U.dataset(name)
    model = OracleModel(model_name, g[f"{case}/ent"], g[f"{case}/rel"], rec["hidden"], rec["gamma"]).eval()
    ev = _evaluation(ds)
    for threshold in (1.5, 1.0):
        got = ev.detail_metrics(model=model, dataset=ds.test, threshold=threshold)
        U.assert_metrics_close(got, rec["metrics"][str(threshold)], 0.0)
    assert not model.training


def test_fixture_ranks_reproduce_the_recorded_metrics(golden):
    """The per-item ranks and the rounded table of a fixture belong together (the GPU tests compare against both)."""
    g, js = golden("detail_eval.npz"), golden("detail_eval.json")
    for case in U.CASES:
        ds = U.dataset(case.split("/")[0])
        relations = np.asarray(ds.test, dtype=np.int64)[:, 1]
        table = U.type_table(js[case]["types"]["1.5"], ds.relations)
        for mode in U.MODES:
            counts, rr = U.group_sums(g[f"{case}/{mode}/ranks"], relations, table, 4)
            assert counts[:, 0].sum() == len(ds.test)
            for k, kind in enumerate(U.TYPES):
                want = js[case]["metrics"]["1.5"][mode][kind]
                n = max(int(counts[k, 0]), 1)
                got = [rr[k] / n] + [int(c) / n for c in counts[k, 1:]]
                np.testing.assert_allclose(got, [want[m] for m in U.METRICS], rtol=0, atol=0.5e-4 + 1e-9)


def test_a_relation_absent_from_the_true_triples_is_left_out(golden):
    """Keyed by relation id: relation r1 of three never occurs among the true triples, r2 keeps its own category (the reference's
    row-keyed frame would hand r2's category to r1), and the test items of r1 belong to no category."""
    from mkb_amd import evaluation

    g = golden("evaluation.npz")
    relations = {"r0": 0, "r1": 1, "r2": 2}
    true = [(0, 0, 1), (2, 0, 3), (0, 2, 1), (0, 2, 2), (0, 2, 3)]
    rel = np.concatenate([g["rel"], g["rel"][:1] + 0.25])
    model = OracleModel("RotatE", g["ent"], rel, 3, 1.0).eval()
    ev = evaluation.Evaluation(true_triples=true, entities=U.TOY_ENTITIES, relations=relations, batch_size=2, num_workers=0)
    assert ev.types_relations(model=model, dataset=[], threshold=1.5) == {"r0": "1_1", "r2": "1_M"}
    test = [(0, 0, 1), (1, 1, 2), (0, 2, 3)]
    got = ev.detail_metrics(model=model, dataset=test, threshold=1.5)
    assert got["frequency"] == {"1_1": 0.5, "1_M": 0.5, "M_1": 0.0, "M_M": 0.0}
    alone = ev.detail_metrics(model=model, dataset=[test[0], test[2]], threshold=1.5)
    assert {m: got[m] for m in U.MODES} == {m: alone[m] for m in U.MODES}  # the item of r1 changed nothing
    assert got["head-batch"]["1_1"]["MR"] >= 1.0 and got["head-batch"]["1_M"]["MR"] >= 1.0
