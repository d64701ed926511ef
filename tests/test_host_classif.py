"""CPU (-m "not gpu") tests of triple classification (evaluation.find_threshold / accuracy and their extensions; reference
evaluation/classif.py) against tests/golden/classif.{npz,json}: the threshold rule restated from counts (util_classif), the host
route of the package on the same rule, and datasets.classification_set."""
import ctypes
import re
import warnings

import numpy as np
import pytest
import torch

import util_classif as U


class OracleModel(torch.nn.Module):
    """model(sample) on CPU tensors by the oracle's restatement of the forwards (not a BaseModel: the host route)."""

    def __init__(self, name, ent, rel, hidden, gamma, n_relation):
        super().__init__()
        from oracle import scoring

        self.tb = scoring.Tables(name, hidden, gamma, torch.as_tensor(ent).float(), torch.as_tensor(rel).float(), None)
        self.n_relation = n_relation

    def forward(self, sample, negative_sample=None, mode=None):
        from oracle import scoring

        return scoring.score(self.tb, sample, negative_sample, mode)


def test_names_are_exported_and_symbols_declared_and_bound():
    from conftest import ROOT
    from mkb_amd import _hip, datasets, evaluation

    for name in ("find_threshold", "accuracy", "find_thresholds_per_relation", "classification_report", "threshold_search",
                 "threshold_accuracy"):
        assert callable(getattr(evaluation, name)) and name in evaluation.__all__
    assert callable(datasets.classification_set)
    header = (ROOT / "include" / "mkb_hip.h").read_text()
    decl = re.search(r"\bint mkb_threshold_search\(([^)]*)\);", header)
    assert decl and [a.split()[-1].lstrip("*") for a in decl.group(1).split(",")] == [
        "score", "label", "group", "n", "n_groups", "threshold", "stats", "ws", "ws_bytes", "stream"]
    decl = re.search(r"\bint mkb_threshold_accuracy\(([^)]*)\);", header)
    assert decl and [a.split()[-1].lstrip("*") for a in decl.group(1).split(",")] == [
        "score", "label", "group", "n", "threshold", "n_groups", "counts", "stream"]
    assert re.search(r"#define MKB_THRESHOLD_SEARCH_MAX_N (\d+)", header).group(1) == str(_hip.THRESHOLD_SEARCH_MAX_N)
    assert evaluation.classif.SEARCH_CAP == _hip.THRESHOLD_SEARCH_MAX_N
    lib = _hip.lib()
    assert lib.mkb_threshold_search_workspace_bytes(1000, 3) >= 1000 * 4
    assert lib.mkb_threshold_search_workspace_bytes(_hip.THRESHOLD_SEARCH_MAX_N + 1, 1) < 0


def test_abi_rejects_bad_arguments_before_any_launch():
    from mkb_amd import _hip

    lib, p = _hip.lib(), ctypes.c_void_p(0x10000)  # never dereferenced: every call below fails validation first

    def search(score=p, label=p, group=p, n=4, G=2, thr=p, stats=p, ws=p, ws_bytes=1 << 20):
        return lib.mkb_threshold_search(score, label, group, n, G, thr, stats, ws, ws_bytes, None)

    for kw in [dict(n=-1), dict(G=0), dict(G=-3), dict(score=None), dict(label=None), dict(thr=None), dict(stats=None),
               dict(ws=None), dict(ws_bytes=8), dict(ws=ctypes.c_void_p(0x10002))]:
        assert search(**kw) == _hip.ERR_INVALID, kw
    assert search(n=_hip.THRESHOLD_SEARCH_MAX_N + 1, ws_bytes=1 << 40) == _hip.ERR_INVALID
    message = lib.mkb_last_error().decode()
    assert "cap" in message and str(_hip.THRESHOLD_SEARCH_MAX_N) in message
    assert search(n=1 << 17, G=1 << 16, ws_bytes=1 << 40) == _hip.ERR_INVALID  # 2^33 item visits by the per-group workgroups
    assert "65536 groups x 131072 items" in lib.mkb_last_error().decode()

    def accuracy(score=p, label=p, group=p, n=4, thr=p, G=2, counts=p):
        return lib.mkb_threshold_accuracy(score, label, group, n, thr, G, counts, None)

    for kw in [dict(n=1 << 20, G=1 << 13), dict(n=-1), dict(n=1 << 62), dict(G=0), dict(score=None), dict(label=None), dict(thr=None),
               dict(counts=None)]:
        assert accuracy(**kw) == _hip.ERR_INVALID, kw
    assert b"null pointer" in lib.mkb_last_error()


def test_a_library_without_a_new_symbol_says_rebuild(monkeypatch):
    from mkb_amd import _hip

    monkeypatch.setattr(_hip, "_lib", None)
    monkeypatch.setitem(_hip._SIGNATURES, "mkb_threshold_search_not_there", (ctypes.c_int, []))
    with pytest.raises(_hip.HipLibraryError, match="rebuild"):
        _hip.lib()
    assert _hip._lib is None


@pytest.mark.parametrize("model", U.MODELS)
def test_restatement_returns_the_golden_thresholds(golden, model):
    """Global and for every relation of the valid set, with ==: no case is exempt."""
    from mkb_amd.evaluation import classif

    g, n_rel = golden("classif.npz"), golden("classif.json")["n_relation"]
    score, y, relation = g[f"{model}/valid/score"], g["valid/y"], g["valid/X"][:, 1]
    assert score.dtype == np.float32
    want, want_per = g[f"{model}/threshold"], g[f"{model}/threshold_per_relation"]
    present = ~np.isnan(want_per)
    assert present.sum() == len(set(relation.tolist())) and np.isfinite(want_per[present]).sum() >= 20
    for search in (U.search, lambda s, lab, rel=None, G=1: classif.threshold_search(s, lab, relation=rel, n_relation=G if rel is not None else None)):
        thr, stats = search(score, y)
        assert thr.dtype == np.float32 and thr[0] == want
        assert stats[0, 0] + stats[0, 1] == stats[0, 5] == len(score) and stats[0, 4] == 0
        per, per_stats = search(score, y, relation, n_rel)
        assert np.all(per[present] == want_per[present]) and np.all(np.isinf(per[~present]))
        assert per_stats[:, 5].sum() == len(score) and np.all(per_stats[~present, 5] == 0)
    assert np.array_equal(classif.threshold_search(score, y, relation, n_rel)[1], U.search(score, y, relation, n_rel)[1])


@pytest.mark.parametrize("model", U.MODELS)
def test_accuracy_counts_at_the_golden_threshold(golden, model):
    from mkb_amd.evaluation import classif

    g, rec = golden("classif.npz"), golden("classif.json")["models"][model]
    thr = g[f"{model}/threshold"]
    assert repr(float(thr)) == rec["threshold"] and str(thr) == rec["threshold_str"]
    for split in ("valid", "test"):
        score, y = g[f"{model}/{split}/score"], g[f"{split}/y"]
        for counts in (U.accuracy_counts(score, y, thr), classif.threshold_accuracy(score, y, thr)):
            assert counts.shape == (1, 2) and counts[0, 1] == len(score)
            assert counts[0, 0] / counts[0, 1] == rec["accuracy"][split]
    # the threshold's own statistics give the accuracy on the set it was searched on
    _, stats = classif.threshold_search(g[f"{model}/valid/score"], g["valid/y"])
    P, N, tp, fp, _, n = stats[0].tolist()
    assert (tp + N - fp) / n == rec["accuracy"]["valid"]


def test_doctest_numbers(golden):
    """classif.py:39-66: 1.9384804, then the accuracies at the literal 1.9384804 -- a double just above the float32 threshold,
    so the item at the threshold is not >= it: 669 of 1,304; at the float32 itself: 670 (the recorded accuracy)."""
    from mkb_amd.evaluation import classif

    g, rec = golden("classif.npz"), golden("classif.json")["models"]["TransE3"]
    score, y = g["TransE3/valid/score"], g["valid/y"]
    thr = classif.threshold_search(score, y)[0][0]
    assert str(thr) == "1.9384804" and isinstance(thr, np.float32)
    assert int(classif.threshold_accuracy(score, y, 1.9384804)[0, 0]) / len(y) == 0.5130368098159509
    assert int(classif.threshold_accuracy(g["TransE3/test/score"], g["test/y"], 1.9384804)[0, 0]) / len(g["test/y"]) == 0.49924357034795763
    assert int(classif.threshold_accuracy(score, y, thr)[0, 0]) / len(y) == rec["accuracy"]["valid"] == 670 / 1304


@pytest.mark.parametrize("model", ["TransE3", "RotatE", "TransE_trained"])
def test_model_functions_on_a_cpu_model_equal_the_restatement_on_its_scores(golden, model):
    from mkb_amd import evaluation, utils

    g, js = golden("classif.npz"), golden("classif.json")
    rec, n_rel = js["models"][model], js["n_relation"]
    m = OracleModel(rec["model"], g[f"{model}/ent"], g[f"{model}/rel"], rec["hidden"], rec["gamma"], n_rel).eval()
    X, y = [tuple(t) for t in g["valid/X"].tolist()], g["valid/y"].tolist()
    Xt, yt = [tuple(t) for t in g["test/X"].tolist()], g["test/y"].tolist()
    score = utils.make_prediction(model=m, dataset=X, batch_size=500, device="cpu").numpy()
    score_t = utils.make_prediction(model=m, dataset=Xt, batch_size=500, device="cpu").numpy()
    np.testing.assert_allclose(score, g[f"{model}/valid/score"], rtol=0, atol=1e-4)
    call = dict(model=m, batch_size=500, device="cpu")
    thr = evaluation.find_threshold(X=X, y=y, num_workers=0, **call)
    assert isinstance(thr, np.float32) and thr == U.search(score, y)[0][0]
    got = evaluation.accuracy(X=Xt, y=yt, threshold=thr, num_workers=0, **call)
    assert isinstance(got, float) and got == U.accuracy_counts(score_t, yt, thr)[0, 0] / len(yt)
    per, overall = evaluation.find_thresholds_per_relation(X=X, y=y, **call)
    want, stats = U.search(score, y, g["valid/X"][:, 1], n_rel)
    fallback = (stats[:, 0] == 0) | (stats[:, 1] == 0)
    assert overall == thr and per.shape == (n_rel,) and fallback.any() and not fallback.all()
    assert np.all(per[~fallback] == want[~fallback]) and np.all(per[fallback] == thr)
    counts = U.accuracy_counts(score_t, yt, per, g["test/X"][:, 1])
    assert evaluation.accuracy(X=Xt, y=yt, threshold=per, **call) == counts[:, 0].sum() / len(yt)
    report = evaluation.classification_report(X=Xt, y=yt, threshold=per, **call)
    assert report["n"] == len(yt) and report["accuracy"] == counts[:, 0].sum() / len(yt)
    assert report["per_relation"] == {r: {"accuracy": c / k, "n": k} for r, (c, k) in enumerate(counts.tolist()) if k}
    flat = evaluation.classification_report(X=Xt, y=yt, threshold=float(thr), **call)
    assert flat["accuracy"] == got and sum(v["n"] for v in flat["per_relation"].values()) == len(yt)


def test_edge_cases():
    from mkb_amd.evaluation import classif

    f32 = lambda *v: np.asarray(v, dtype=np.float32)  # noqa: E731
    for search in (U.search, classif.threshold_search):
        for y in ([1, 1, 1], [-1, -1, -1], [0, 0, -1]):  # one class only
            thr, stats = search(f32(1, 2, 3), y)
            assert np.isposinf(thr[0]) and stats[0, 2:5].tolist() == [0, 0, 0] and stats[0, 5] == 3
        assert np.isposinf(search(f32(2), [1])[0][0]) and np.isposinf(search(f32(2), [-1])[0][0])  # n == 1
        thr, stats = search(f32(), np.zeros(0, dtype=np.int64))
        assert np.isposinf(thr[0]) and stats.tolist() == [[0] * 6]
        thr, stats = search(f32(5, 5, 5, 5), [1, -1, 1, -1])  # all scores equal: J = 0 everywhere, the first point wins
        assert np.isposinf(thr[0]) and stats[0].tolist() == [2, 2, 0, 0, 0, 4]
        thr, stats = search(f32(-0.0, 0.0, -0.0, -1, -1), [1, 1, -1, -1, -1])  # one point at zero: 2 tp, 1 fp
        assert thr[0] == 0.0 and stats[0].tolist() == [2, 3, 2, 1, 0, 5]
        thr, stats = search(f32(3, 2, 1), [1, 0, -1])  # a label of 0 is a negative
        assert thr[0] == 3.0 and stats[0].tolist() == [1, 2, 1, 0, 0, 3]
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="1 of 3 scores"):
            classif.threshold_search(f32(1, bad, 3), [1, -1, 1])
        assert U.search(f32(1, bad, 3), [-1, -1, 1])[1][0].tolist() == [1, 1, 1, 0, 1, 3]
    # accuracy: a NaN score is neither >= nor <; +-inf compare as usual
    score, y = f32(np.nan, np.nan, np.inf, -np.inf, 1, 1, -0.0), [1, -1, 1, -1, 1, -1, 1]
    for counts in (U.accuracy_counts(score, y, 0.0), classif.threshold_accuracy(score, y, 0.0)):
        assert counts.tolist() == [[4, 7]]
    assert classif.threshold_accuracy(score, y, np.inf).tolist() == U.accuracy_counts(score, y, np.inf).tolist() == [[3, 7]]
    assert classif.threshold_accuracy(f32(), [], 0.0).tolist() == [[0, 0]]
    # groups: ids outside [0, G) belong to nobody
    counts = classif.threshold_accuracy(f32(1, 2, 3, 4), [1, 1, -1, -1], [1.5, 9.0, 0.0], relation=[0, 1, -1, 3], n_relation=3)
    assert counts.tolist() == U.accuracy_counts(f32(1, 2, 3, 4), [1, 1, -1, -1], [1.5, 9.0, 0.0], [0, 1, -1, 3]).tolist() == [[0, 1], [0, 1], [0, 0]]


def test_model_functions_raise_on_scores_that_are_not_finite():
    from mkb_amd import evaluation

    class Broken(torch.nn.Module):
        def forward(self, sample, negative_sample=None, mode=None):
            out = sample[:, :1].float()
            out[sample[:, 0] == 2] = float("nan")
            return out

    X, y = [(0, 0, 1), (1, 0, 2), (2, 0, 3), (2, 0, 0), (3, 0, 0)], [1, -1, 1, -1, 1]
    with pytest.raises(ValueError, match="2 of 5 scores"):
        evaluation.find_threshold(model=Broken(), X=X, y=y, batch_size=2, device="cpu")
    assert evaluation.accuracy(model=Broken(), X=X, y=y, threshold=1.0, batch_size=2, device="cpu") == 1 / 5


def test_one_threshold_in_an_array_and_an_empty_set():
    """accuracy and classification_report read a threshold the same way: one number, however wrapped, is every triple's; and
    neither reports an accuracy of no triples."""
    from mkb_amd import evaluation

    class First(torch.nn.Module):
        n_relation = 3

        def forward(self, sample, negative_sample=None, mode=None):
            return sample[:, :1].float()

    X, y = [(0, 0, 1), (1, 1, 2), (2, 2, 3), (3, 2, 0)], [-1, -1, 1, -1]
    call = dict(model=First(), X=X, y=y, batch_size=3, device="cpu")
    for one in (2.0, np.float32(2.0), [2.0], np.array([2.0]), torch.tensor([2.0])):
        assert evaluation.accuracy(threshold=one, **call) == 0.75
        assert evaluation.classification_report(threshold=one, **call)["accuracy"] == 0.75
    per = [9.0, 0.0, 2.5]
    assert evaluation.accuracy(threshold=per, **call) == evaluation.classification_report(threshold=per, **call)["accuracy"] == 0.25
    for fn in (evaluation.accuracy, evaluation.classification_report):
        with pytest.raises(ValueError, match="X is empty"):
            fn(model=First(), X=[], y=[], threshold=1.0, batch_size=3, device="cpu")


def test_classification_set():
    from mkb_amd import datasets

    ds = U.dataset()
    true = set(map(tuple, ds.true_triples))
    got = datasets.classification_set(ds.valid, ds.true_triples, ds.entities, seed=42)
    X, y = got["X"], got["y"]
    assert len(X) == len(y) == 2 * len(ds.valid)
    assert y == [1, -1] * len(ds.valid)
    assert X[0::2] == [tuple(t) for t in ds.valid]
    assert all((h, r) == X[2 * i][:2] and (h, r, t) not in true and 0 <= t < len(ds.entities) for i, (h, r, t) in enumerate(X[1::2]))
    assert datasets.classification_set(ds.valid, ds.true_triples, ds.entities, seed=42) == got
    assert datasets.classification_set(ds.valid, ds.true_triples, ds.entities, seed=43)["X"] != X
    assert datasets.classification_set([], ds.true_triples, ds.entities) == {"X": [], "y": []}
    with pytest.raises(ValueError, match="no false tail"):
        datasets.classification_set([(0, 0, 1)], [(0, 0, 0), (0, 0, 1)], {"a": 0, "b": 1})
    both = datasets.Dataset(train=ds.train, valid=ds.valid, test=ds.test, entities=ds.entities, relations=ds.relations, batch_size=8,
                            num_workers=0, classification_valid=got, classification_test=got)
    assert both.classification_valid is got and both.classification_test is got


def test_random_tied_cases_against_sklearn():
    """The rule against roc_curve itself, where sklearn is installed: heavy ties, labels in {-1, 0, 1} (0 and -1 both negative)."""
    metrics = pytest.importorskip("sklearn.metrics")
    from mkb_amd.evaluation import classif

    rng = np.random.default_rng(5)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for case in range(3000):
            n = int(rng.integers(1, 60))
            if case % 3 == 0:
                score = rng.integers(-2, 3, n).astype(np.float32)
            elif case % 3 == 1:
                score = rng.standard_normal(n).astype(np.float32)
            else:
                score = rng.choice(rng.standard_normal(4).astype(np.float32), n)
            y = rng.integers(-1, 2, n)
            if (y > 0).all() or (y <= 0).all():
                want = np.float32(np.inf)
            else:
                fpr, tpr, thresholds = metrics.roc_curve(np.where(y > 0, 1, -1), score)
                want = thresholds[np.argmax(tpr - fpr)]
            assert U.roc_choice(score, y)[0] == want, (score, y)
            assert classif.threshold_search(score, y)[0][0] == want, (score, y)
