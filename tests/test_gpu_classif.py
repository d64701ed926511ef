"""-m gpu: triple classification on the device -- the kernels of mkb_amd/csrc/classif.hip (mkb_threshold_search,
mkb_threshold_accuracy) at their launch edges against the restatement of tests/util_classif.py with exact equality, the golden
scores of tests/golden/classif.npz, and evaluation.find_threshold / accuracy / find_thresholds_per_relation end to end."""
import numpy as np
import pytest
import torch

import util_classif as U

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _search(score, label, group, G):
    """One mkb_threshold_search call on fresh output buffers and a fresh workspace, all pre-filled with junk."""
    from mkb_amd import _hip

    lib, n = _hip.lib(), len(score)
    s = torch.as_tensor(np.asarray(score, dtype=np.float32), device=DEV)
    y = torch.as_tensor(np.asarray(label, dtype=np.int64), device=DEV)
    g = None if group is None else torch.as_tensor(np.asarray(group, dtype=np.int32), device=DEV)
    thr = torch.full((G,), 7.0, dtype=torch.float32, device=DEV)
    stats = torch.full((G, 6), -7, dtype=torch.int64, device=DEV)
    need = lib.mkb_threshold_search_workspace_bytes(n, G)
    assert need >= 0
    ws = torch.full((need // 4 + 64,), -0x35353536, dtype=torch.int32, device=DEV)
    some = (lambda t: _hip.ptr(t) if n else None)
    _hip.check(lib.mkb_threshold_search(some(s), some(y), some(g) if g is not None else None, n, G, _hip.ptr(thr), _hip.ptr(stats),
                                        some(ws), need, _hip.stream_ptr()), "mkb_threshold_search")
    tail = ws[need // 4:].cpu().numpy()
    assert (tail == -0x35353536).all()  # nothing written behind the workspace
    return thr.cpu().numpy(), stats.cpu().numpy()


def _accuracy(score, label, group, threshold):
    from mkb_amd import _hip

    n, G = len(score), len(threshold)
    s = torch.as_tensor(np.asarray(score, dtype=np.float32), device=DEV)
    y = torch.as_tensor(np.asarray(label, dtype=np.int64), device=DEV)
    g = None if group is None else torch.as_tensor(np.asarray(group, dtype=np.int32), device=DEV)
    t = torch.as_tensor(np.asarray(threshold, dtype=np.float32), device=DEV)
    counts = torch.full((G, 2), -7, dtype=torch.int64, device=DEV)
    some = (lambda x: _hip.ptr(x) if n else None)
    _hip.check(_hip.lib().mkb_threshold_accuracy(some(s), some(y), some(g) if g is not None else None, n, _hip.ptr(t), G,
                                                 _hip.ptr(counts), _hip.stream_ptr()), "mkb_threshold_accuracy")
    return counts.cpu().numpy()


def _check(score, label, group, G):
    """Both kernels against the restatement, exactly, and bit-identical from run to run."""
    score = np.asarray(score, dtype=np.float32)
    want_thr, want_stats = U.search(score, label, group, G)
    thr, stats = _search(score, label, group, G)
    assert U.same_floats(thr, want_thr), (thr, want_thr)
    np.testing.assert_array_equal(stats, want_stats)
    thr2, stats2 = _search(score, label, group, G)
    assert thr2.tobytes() == thr.tobytes() and stats2.tobytes() == stats.tobytes()
    at = np.where(np.isinf(want_thr), np.float32(0.5), want_thr).astype(np.float32)  # a finite threshold for every group
    for threshold in (at, want_thr):
        counts = _accuracy(score, label, group, threshold)
        np.testing.assert_array_equal(counts, U.accuracy_counts(score, label, threshold, group))
        assert _accuracy(score, label, group, threshold).tobytes() == counts.tobytes()
    finite = np.isfinite(want_thr) & (want_stats[:, 4] == 0)  # the statistics of the search give the accuracy at its threshold
    acc = _accuracy(score, label, group, want_thr)
    assert np.array_equal((stats[:, 2] + stats[:, 1] - stats[:, 3])[finite], acc[finite, 0])
    return thr, stats


def _groups(rs, n, G, label):
    """Group ids with one group nobody maps to and one with positives only (G > 1), and ids -1 and G on a few items."""
    group = rs.randint(G, size=n).astype(np.int32)
    empty = only_pos = -1
    if G > 1:
        empty, only_pos = G // 2, (G // 2 + 1) % G
        group[group == empty] = (empty + 2) % G if G > 2 else only_pos
        label[group == only_pos] = 1
    if n >= 63:
        group[[5, 40]], group[[6, 41]] = -1, G
    return group, empty, only_pos


@pytest.mark.parametrize("G", [1, 4, 37])
def test_search_and_accuracy_edge_shapes(G):
    """n around the 64-lane wave, the 256-item tile and several workgroups; heavy ties (5 integer scores) and randn."""
    for n in (0, 1, 2, 63, 64, 65, 255, 256, 257, 1025, 5000):
        for kind in ("ties", "randn"):
            rs = np.random.RandomState(1000 * G + n + (kind == "ties"))
            score = rs.randint(-2, 3, size=n).astype(np.float32) if kind == "ties" else rs.randn(n).astype(np.float32)
            label = rs.randint(-1, 2, size=n).astype(np.int64)
            group, empty, only_pos = _groups(rs, n, G, label)
            if G == 1 and kind == "ties" and n < 63:
                group = None  # the null group pointer: every item is of group 0
            thr, stats = _check(score, label, group, G)
            if G > 1:
                assert np.isposinf(thr[empty]) and not stats[empty].any()
                assert np.isposinf(thr[only_pos]) and stats[only_pos, 1] == 0
            if n >= 1025:
                assert np.isfinite(thr).any()


@pytest.mark.parametrize("n", [8193, 10007, 35070])
def test_search_with_several_tiles_per_workgroup(n):
    """Above 8,192 items the grid of the two pair passes has fewer splits than tiles of 256 items, so a workgroup walks several
    tiles (re-staging its LDS tile each time) and the tiles do not divide evenly among the splits: 33 tiles over 32 splits,
    40 over 26, and 137 over 8 -- the shape of FB15k-237's valid set.  None is a multiple of 256."""
    for G, kind in ((1, "ties"), (1, "randn"), (37, "ties"), (237, "randn")):
        rs = np.random.RandomState(n + G + (kind == "ties"))
        score = rs.randint(-2, 3, size=n).astype(np.float32) if kind == "ties" else rs.randn(n).astype(np.float32)
        label = rs.randint(-1, 2, size=n).astype(np.int64)
        group, empty, only_pos = _groups(rs, n, G, label)
        if G > 1 and kind == "ties":
            order = np.argsort(group, kind="stable")  # by group, as a caller that sorts by relation passes them
            score, label, group = score[order], label[order], group[order]
        thr, stats = _check(score, label, group if G > 1 else None, G)
        assert np.isfinite(thr).any() and stats[:, 5].sum() == (n if G == 1 else n - 4)
        if G > 1:
            assert np.isposinf(thr[empty]) and not stats[empty].any()


def test_search_special_scores():
    rs = np.random.RandomState(3)
    n = 600
    label = rs.randint(-1, 2, size=n).astype(np.int64)
    tiny = np.float32(1e-45)  # the smallest denormal
    denormal = (rs.randint(-3, 4, size=n) * tiny).astype(np.float32)
    denormal[::7] = -0.0
    assert (np.abs(denormal[denormal != 0]) < 1e-44).all()
    thr, _ = _check(denormal, label, None, 1)
    assert np.isfinite(thr[0])
    huge = (rs.randint(0, 2, size=n) * 2 - 1) * np.float32(3e38)
    _check(huge.astype(np.float32), label, rs.randint(4, size=n), 4)
    thr, stats = _check(np.full(n, 2.5, dtype=np.float32), label, None, 1)
    assert np.isposinf(thr[0]) and stats[0, 2:4].tolist() == [0, 0]
    score = rs.randn(n).astype(np.float32)
    above = np.where(label > 0, np.abs(score) + 1, -np.abs(score) - 1).astype(np.float32)
    thr, stats = _check(above, label, None, 1)  # separable: the lowest positive score, J = 1
    assert thr[0] == above[label > 0].min() and stats[0, 2] == stats[0, 0] and stats[0, 3] == 0
    thr, _ = _check(-above, label, None, 1)  # every positive below every negative: no threshold beats +inf
    assert np.isposinf(thr[0])
    zeros = np.where(rs.rand(n) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    zeros[::5] = -1
    label[::5] = -1
    _check(zeros, label, rs.randint(3, size=n), 3)


def test_scores_that_are_not_finite_are_counted():
    from mkb_amd.evaluation import classif

    rs = np.random.RandomState(4)
    n, G = 700, 4
    score = rs.randn(n).astype(np.float32)
    label = rs.randint(-1, 2, size=n).astype(np.int64)
    group = rs.randint(-1, G + 1, size=n)
    score[rs.rand(n) < 0.05] = np.nan
    score[3], score[300], score[699] = np.inf, -np.inf, np.nan
    _, stats = _check(score, label, group, G)
    bad = ~np.isfinite(score)
    assert stats[:, 4].tolist() == [int((bad & (group == g)).sum()) for g in range(G)] and stats[:, 4].sum() > 0
    with pytest.raises(ValueError, match=f"{int((bad & (group >= 0) & (group < G)).sum())} of {n} scores"):
        classif.threshold_search(torch.as_tensor(score, device=DEV), label, relation=group, n_relation=G)
    counts = classif.threshold_accuracy(torch.as_tensor(score, device=DEV), label, [0.0, 0.1, -0.2, 9.0], relation=group, n_relation=G)
    np.testing.assert_array_equal(counts, U.accuracy_counts(score, label, [0.0, 0.1, -0.2, 9.0], group))


@pytest.mark.parametrize("model", U.MODELS)
def test_golden_scores_on_the_device(golden, model):
    from mkb_amd.evaluation import classif

    g, js = golden("classif.npz"), golden("classif.json")
    rec, n_rel = js["models"][model], js["n_relation"]
    y, relation = g["valid/y"], g["valid/X"][:, 1]
    score = torch.as_tensor(g[f"{model}/valid/score"], device=DEV)
    thr, stats = classif.threshold_search(score, y)
    assert thr[0] == g[f"{model}/threshold"]
    P, N, tp, fp, _, n = stats[0].tolist()
    assert (tp + N - fp) / n == rec["accuracy"]["valid"]
    per, _ = classif.threshold_search(score, y, relation=relation, n_relation=n_rel)
    want = g[f"{model}/threshold_per_relation"]
    present = ~np.isnan(want)
    assert np.all(per[present] == want[present]) and np.all(np.isinf(per[~present]))
    for split in ("valid", "test"):
        s = torch.as_tensor(g[f"{model}/{split}/score"], device=DEV)
        counts = classif.threshold_accuracy(s, g[f"{split}/y"], g[f"{model}/threshold"])
        assert counts[0, 0] / counts[0, 1] == rec["accuracy"][split]
    if model == "TransE3":  # the doctest's literal, a double just above the float32 threshold (classif.py:48-66)
        assert int(classif.threshold_accuracy(score, y, 1.9384804)[0, 0]) / len(y) == 0.5130368098159509


@pytest.mark.parametrize("model", U.MODELS)
def test_end_to_end_on_the_device(golden, model, monkeypatch):
    """Device scores within the parity bound of the golden ones; thresholds and accuracies equal the restatement applied to the
    device's own scores (the threshold is one of the scores, selected among near-ties that a last-bit difference reorders: it is
    not compared with golden here)."""
    from mkb_amd import evaluation, utils
    from mkb_amd.evaluation import classif
    from util_gpu import make_model

    def no_host(*a, **k):
        raise AssertionError("the host route was taken")

    monkeypatch.setattr(classif, "_search_host", no_host)
    monkeypatch.setattr(classif, "_accuracy_host", no_host)
    g, js = golden("classif.npz"), golden("classif.json")
    rec, n_rel = js["models"][model], js["n_relation"]
    modulus = g[f"{model}/modulus"] if f"{model}/modulus" in g.files else None
    m = make_model(rec["model"], g[f"{model}/ent"], g[f"{model}/rel"], rec["hidden"], rec["gamma"], modulus).eval()
    X, y = [tuple(t) for t in g["valid/X"].tolist()], g["valid/y"].tolist()
    Xt, yt = [tuple(t) for t in g["test/X"].tolist()], g["test/y"].tolist()
    score = utils.make_prediction(model=m, dataset=X, batch_size=500, device=DEV).cpu().numpy()
    score_t = utils.make_prediction(model=m, dataset=Xt, batch_size=500, device=DEV).cpu().numpy()
    np.testing.assert_allclose(score, g[f"{model}/valid/score"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(score_t, g[f"{model}/test/score"], rtol=0, atol=1e-4)
    thr = evaluation.find_threshold(model=m, X=X, y=y, batch_size=500)
    assert isinstance(thr, np.float32) and thr == U.search(score, y)[0][0]
    for split_X, split_y, s in ((X, y, score), (Xt, yt, score_t)):
        got = evaluation.accuracy(model=m, X=split_X, y=split_y, threshold=thr, batch_size=500)
        assert got == U.accuracy_counts(s, split_y, thr)[0, 0] / len(split_y)
    per, overall = evaluation.find_thresholds_per_relation(model=m, X=X, y=y, batch_size=500)
    want, stats = U.search(score, y, g["valid/X"][:, 1], n_rel)
    fallback = (stats[:, 0] == 0) | (stats[:, 1] == 0)
    assert overall == thr and np.all(per[~fallback] == want[~fallback]) and np.all(per[fallback] == thr)
    counts = U.accuracy_counts(score_t, yt, per, g["test/X"][:, 1])
    assert evaluation.accuracy(model=m, X=Xt, y=yt, threshold=per, batch_size=500) == counts[:, 0].sum() / len(yt)
    report = evaluation.classification_report(model=m, X=Xt, y=yt, threshold=per, batch_size=500)
    assert report["accuracy"] == counts[:, 0].sum() / len(yt)
    assert report["per_relation"] == {r: {"accuracy": c / k, "n": k} for r, (c, k) in enumerate(counts.tolist()) if k}


def test_above_the_cap_the_entry_refuses_and_python_searches_on_the_host(golden, monkeypatch):
    from mkb_amd import _hip, evaluation
    from mkb_amd.evaluation import classif
    from util_gpu import make_model

    lib, n = _hip.lib(), _hip.THRESHOLD_SEARCH_MAX_N + 1
    s, y = torch.zeros(n, dtype=torch.float32, device=DEV), torch.ones(n, dtype=torch.int64, device=DEV)
    thr, stats = torch.full((1,), 7.0, device=DEV), torch.full((1, 6), -7, dtype=torch.int64, device=DEV)
    ws = torch.empty(8 * n, dtype=torch.int32, device=DEV)
    rc = lib.mkb_threshold_search(_hip.ptr(s), _hip.ptr(y), None, n, 1, _hip.ptr(thr), _hip.ptr(stats), _hip.ptr(ws), 32 * n, _hip.stream_ptr())
    assert rc == _hip.ERR_INVALID
    message = lib.mkb_last_error().decode()
    assert "cap" in message and str(n) in message and str(n - 1) in message
    torch.cuda.synchronize()
    assert thr.item() == 7.0 and (stats == -7).all()  # refused before any launch

    calls = []
    host = classif._search_host
    monkeypatch.setattr(classif, "_search_host", lambda *a: calls.append(len(a[0])) or host(*a))
    rs = np.random.RandomState(9)
    score, label, group = rs.randint(-2, 3, size=300).astype(np.float32), rs.randint(-1, 2, size=300), rs.randint(5, size=300)
    on_device = torch.as_tensor(score, device=DEV)
    want_thr, want_stats = U.search(score, label, group, 5)
    got_thr, got_stats = classif.threshold_search(on_device, label, relation=group, n_relation=5, _cap=299)
    assert calls == [300] and U.same_floats(got_thr, want_thr) and np.array_equal(got_stats, want_stats)
    got_thr, got_stats = classif.threshold_search(on_device, label, relation=group, n_relation=5, _cap=300)
    assert calls == [300] and U.same_floats(got_thr, want_thr) and np.array_equal(got_stats, want_stats)

    g, js = golden("classif.npz"), golden("classif.json")
    rec = js["models"]["TransE_trained"]
    m = make_model("TransE", g["TransE_trained/ent"], g["TransE_trained/rel"], rec["hidden"], rec["gamma"]).eval()
    X, y = [tuple(t) for t in g["valid/X"].tolist()], g["valid/y"].tolist()
    there = evaluation.find_threshold(model=m, X=X, y=y, batch_size=500)
    per_there, _ = evaluation.find_thresholds_per_relation(model=m, X=X, y=y, batch_size=500)
    assert calls == [300]
    monkeypatch.setattr(classif, "SEARCH_CAP", 1000)
    assert evaluation.find_threshold(model=m, X=X, y=y, batch_size=500) == there and calls == [300, len(X)]
    per_here, _ = evaluation.find_thresholds_per_relation(model=m, X=X, y=y, batch_size=500)
    assert np.array_equal(per_here, per_there) and calls == [300] + [len(X)] * 3
