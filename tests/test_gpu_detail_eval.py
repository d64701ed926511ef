"""-m gpu: the grouped evaluation report on the device -- the two kernels of mkb_amd/csrc/metrics.hip (mkb_rank_metrics,
mkb_relation_fanout) at their launch edges against numpy restatements written here, and Evaluation.types_relations /
detail_metrics / eval_per_relation against tests/golden/detail_eval.{npz,json} and against the same object's host route."""
import numpy as np
import pytest
import torch

import util_detail_eval as U

pytestmark = pytest.mark.gpu


def _rank_metrics(ranks, sample, table, G):
    """One mkb_rank_metrics call on fresh, dirty output buffers -> (counts [G, 5] int64, rr_sum [G] float64) on the host."""
    from mkb_amd import _hip

    dev = "cuda"
    r = torch.as_tensor(np.asarray(ranks, dtype=np.int64), device=dev)
    s = torch.as_tensor(np.asarray(sample, dtype=np.int64).reshape(-1, 3), device=dev)
    t = torch.as_tensor(np.asarray(table, dtype=np.int32), device=dev)
    counts = torch.full((G, 5), -7, dtype=torch.int64, device=dev)
    rr = torch.full((G,), float("nan"), dtype=torch.float64, device=dev)
    _hip.check(_hip.lib().mkb_rank_metrics(_hip.ptr(r) if len(r) else None, _hip.ptr(s) if len(r) else None, len(r), _hip.ptr(t),
                                           t.numel(), G, _hip.ptr(counts), _hip.ptr(rr), _hip.stream_ptr()), "mkb_rank_metrics")
    return counts.cpu().numpy(), rr.cpu().numpy()


def _check_rank_metrics(ranks, sample, table, G):
    want_counts, want_rr = U.group_sums(ranks, np.asarray(sample).reshape(-1, 3)[:, 1], table, G)
    counts, rr = _rank_metrics(ranks, sample, table, G)
    np.testing.assert_array_equal(counts, want_counts)
    np.testing.assert_allclose(rr, want_rr, rtol=1e-12, atol=0)
    again_counts, again_rr = _rank_metrics(ranks, sample, table, G)
    assert np.array_equal(again_counts, counts) and again_rr.tobytes() == rr.tobytes()  # bit-identical from run to run
    return counts, rr


@pytest.mark.parametrize("G", [1, 4, 37])
def test_rank_metrics_edge_shapes(G):
    """n around the 64-lane wave and the 256-lane workgroup, 0 and many; relations mapped to -1; a group nobody maps to (G > 1);
    relation ids outside the table; ranks up to 2^31 + 5."""
    R = 41
    for n in (0, 1, 63, 64, 65, 257, 5000):
        rs = np.random.RandomState(1000 * G + n)
        empty = G // 2 if G > 1 else -1
        table = rs.randint(G, size=R).astype(np.int32)
        table[table == empty] = (empty + 1) % G
        table[rs.rand(R) < 0.2] = -1
        table[0], table[R - 1] = -1, G - 1
        sample = np.stack([rs.randint(500, size=n), rs.randint(R, size=n), rs.randint(500, size=n)], 1).astype(np.int64)
        ranks = rs.randint(1, 200, size=n).astype(np.int64)
        big = rs.rand(n) < 0.1
        ranks[big] = (1 << 31) + 5 - rs.randint(0, 3, size=int(big.sum()))
        if n >= 63:
            sample[5, 1], sample[6, 1] = -1, R  # outside the table: in no group
            sample[7, 1] = R - 1
        counts, _ = _check_rank_metrics(ranks, sample, table, G)
        if G > 1:
            assert not counts[empty].any()
        if n == 5000:
            assert counts[:, 1].max() > 1 << 33  # the rank sum needs 64 bits


def test_rank_metrics_all_items_in_one_group():
    n, R, G = 5000, 3, 4
    sample = np.zeros((n, 3), dtype=np.int64)
    sample[:, 1] = np.arange(n) % R
    ranks = np.full(n, (1 << 31) + 5, dtype=np.int64)
    ranks[::7] = 1
    counts, rr = _check_rank_metrics(ranks, sample, np.full(R, 2, dtype=np.int32), G)
    assert counts[2, 0] == n and counts[2, 1] == int(ranks.astype(object).sum()) > 1 << 43
    assert not counts[[0, 1, 3]].any() and not rr[[0, 1, 3]].any()
    # the identity table of eval_per_relation
    counts, _ = _check_rank_metrics(ranks, sample, np.arange(R, dtype=np.int32), R)
    assert counts[:, 0].tolist() == [1667, 1667, 1666]


def _fanout_reference(triples, N, R):
    a = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    h, r, t = a[:, 0], a[:, 1], a[:, 2]
    out = np.zeros((R, 3), dtype=np.int64)
    out[:, 0] = np.bincount(r, minlength=R)
    for col, other in ((1, t), (2, h)):
        pairs = np.unique(np.stack([other, r], 1), axis=0)
        out[:, col] = np.bincount(pairs[:, 1], minlength=R)
    return out


def _fanout(triples, N, R):
    from mkb_amd import _hip
    from mkb_amd.utils import true_keys

    a = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    keys = true_keys(a, "cuda", N, R)
    head, tail = keys["head-batch"], keys["tail-batch"]
    t = torch.as_tensor(a, device="cuda")
    out = torch.full((R, 3), -7, dtype=torch.int64, device="cuda")
    args = (_hip.ptr(t) if len(a) else None, len(a), _hip.ptr(head) if head.numel() else None, head.numel(),
            _hip.ptr(tail) if tail.numel() else None, tail.numel(), N, R, _hip.ptr(out), _hip.stream_ptr())
    _hip.check(_hip.lib().mkb_relation_fanout(*args), "mkb_relation_fanout")
    first = out.cpu().numpy()
    _hip.check(_hip.lib().mkb_relation_fanout(*args), "mkb_relation_fanout")  # overwrites, does not accumulate
    np.testing.assert_array_equal(out.cpu().numpy(), first)
    return first, head.numel()


def _distinct_triples(rs, n, N, R, skip_relation=None):
    rels = np.array([r for r in range(R) if r != skip_relation])
    a = np.stack([rs.randint(N, size=4 * n), rels[rs.randint(len(rels), size=4 * n)], rs.randint(N, size=4 * n)], 1)
    a = np.unique(a, axis=0)
    assert len(a) >= n
    return a[rs.permutation(len(a))[:n]]


def test_relation_fanout_edge_shapes():
    rs = np.random.RandomState(7)
    cases = {
        "no triples": (np.zeros((0, 3), dtype=np.int64), 50, 4),
        "one triple": (np.array([[3, 2, 9]]), 50, 4),
        "one relation": (_distinct_triples(rs, 300, 20, 1), 20, 1),
        "1000 keys, relation 3 without triples": (_distinct_triples(rs, 1000, 60, 6, skip_relation=3), 60, 6),
        # 6 heads x 2 relations x 256 tails: every (h, r) pair owns 256 consecutive tail-batch keys (its boundaries fall on multiples
        # of 256, hence of 64); every (t, r) pair owns 6 head-batch keys
        "pair boundaries on multiples of 256": (np.array([(h, r, t) for h in range(6) for r in (0, 2) for t in range(256)]), 300, 3),
        # 5 tails x 64 heads: (t, r) pairs of 64 head-batch keys each
        "pair boundaries on multiples of 64": (np.array([(h, 1, t) for t in range(5) for h in range(64)]), 64, 2),
        "more relations than the LDS counters hold": (_distinct_triples(rs, 3000, 40, 5000), 40, 5000),
    }
    big = _distinct_triples(rs, 400, 123182, 37)
    big[:3] = [[123181, 36, 123181], [123181, 36, 0], [0, 36, 123181]]  # ids at N - 1 and R - 1: keys up to ~5.6e11
    cases["large ids"] = (np.unique(big, axis=0), 123182, 37)
    for what, (triples, N, R) in cases.items():
        got, n_keys = _fanout(triples, N, R)
        np.testing.assert_array_equal(got, _fanout_reference(triples, N, R), err_msg=what)
        assert n_keys == len(triples), what
        # every triple three times, shuffled: the first count triples, the pair counts stay
        thrice = np.tile(triples, (3, 1))[rs.permutation(3 * len(triples))]
        got3, n_keys3 = _fanout(thrice, N, R)
        assert n_keys3 == n_keys, what
        np.testing.assert_array_equal(got3, got * [3, 1, 1], err_msg=what)
    assert cases["1000 keys, relation 3 without triples"][0].shape == (1000, 3)
    assert not _fanout(cases["1000 keys, relation 3 without triples"][0], 60, 6)[0][3].any()


# ---------------------------------------------------------------------------------------------------------------- fixtures
def _evaluation(ds_name):
    from mkb_amd import evaluation

    ds = U.dataset(ds_name)
    return ds, evaluation.Evaluation(true_triples=ds.true_triples, entities=ds.entities, relations=ds.relations, batch_size=64,
                                     device="cuda", num_workers=0)


def _model(golden, case):
    from util_gpu import make_model

    g, rec = golden("detail_eval.npz"), golden("detail_eval.json")[case]
    return make_model(case.split("/")[1], g[f"{case}/ent"], g[f"{case}/rel"], rec["hidden"], rec["gamma"]).eval()


def test_docstring_case_on_the_device(golden):
    """The reference's class docstring: 4 entities, a filter set with repeated triples -> both relations M_M, its printed table."""
    from mkb_amd import evaluation
    from util_gpu import make_model

    g, rec = golden("evaluation.npz"), golden("detail_eval.json")["toy"]
    model = make_model("RotatE", g["ent"], g["rel"], 3, 1.0).eval()
    ev = evaluation.Evaluation(true_triples=U.TOY_TRUE, entities=U.TOY_ENTITIES, relations=U.TOY_RELATIONS, batch_size=2, device="cuda",
                               num_workers=0)
    assert ev.types_relations(model=model, dataset=U.TOY_TEST, threshold=1.5) == rec["types"] == {"r0": "M_M", "r1": "M_M"}
    U.assert_metrics_close(ev.detail_metrics(model=model, dataset=U.TOY_TEST, threshold=1.5), rec["metrics"], 1e-4)
    for mode in U.MODES:
        np.testing.assert_array_equal(ev.ranks(model, U.TOY_TEST, mode).cpu().numpy(), golden("detail_eval.npz")[f"toy/{mode}/ranks"])


@pytest.mark.parametrize("case", U.CASES)
def test_detail_metrics_match_the_reference_and_the_host_route(golden, case):
    """Device route against the fixture and against the same object's host route.  The ranks, and so every count and integer sum,
    are equal; a rounded metric may differ by one unit of its last digit (1e-4): the device's ordered double sum and the running
    mean differ by ~1e-13, which can only flip a rounding boundary."""
    g, rec = golden("detail_eval.npz"), golden("detail_eval.json")[case]
    ds, ev = _evaluation(case.split("/")[0])
    model = _model(golden, case)
    relations = np.asarray(ds.test, dtype=np.int64)[:, 1]
    for threshold in (1.5, 1.0):
        types = ev.types_relations(model=model, dataset=ds.test, threshold=threshold)
        assert types == rec["types"][str(threshold)]
        table = U.type_table(types, ds.relations)
        sums = ev._group_sums(model, ds.test, table, 4)
        for mode in U.MODES:
            want_counts, want_rr = U.group_sums(g[f"{case}/{mode}/ranks"], relations, table, 4)
            np.testing.assert_array_equal(sums[mode][0], want_counts)
            np.testing.assert_allclose(sums[mode][1], want_rr, rtol=1e-12)
        device = ev.detail_metrics(model=model, dataset=ds.test, threshold=threshold)
        U.assert_metrics_close(device, rec["metrics"][str(threshold)], 1e-4 + 1e-12)
    for mode in U.MODES:
        np.testing.assert_array_equal(ev.ranks(model, ds.test, mode).cpu().numpy(), g[f"{case}/{mode}/ranks"])
    ev.force_reference_path = True
    try:
        assert ev.types_relations(model=model, dataset=ds.test, threshold=1.5) == rec["types"]["1.5"]  # numpy on the same definition
        host = ev.detail_metrics(model=model, dataset=ds.test, threshold=1.0)
    finally:
        ev.force_reference_path = False
    U.assert_metrics_close(host, rec["metrics"]["1.0"], 1e-4 + 1e-12)
    U.assert_metrics_close(device, host, 1e-4 + 1e-12)


def test_eval_per_relation_is_consistent_with_eval(golden):
    case = "Umls/TransE"
    ds, ev = _evaluation("Umls")
    model = _model(golden, case)
    per = ev.eval_per_relation(model=model, dataset=ds.test)
    assert list(per) == list(ds.relations)
    total = ev.eval(model=model, dataset=ds.test)
    n = len(ds.test)
    for mode in U.MODES:
        assert sum(v[mode]["count"] for v in per.values()) == n
        assert list(per["location_of"][mode]) == [*U.METRICS, "count"]
    for metric in ("MRR", "MR"):  # every term is rounded to 4 places: half a unit from each side
        mean = sum(v[mode]["count"] * v[mode][metric] for v in per.values() for mode in U.MODES) / (2 * n)
        assert abs(mean - total[metric]) <= 1e-4 + 1e-9, (metric, mean, total[metric])
    absent = [name for name, v in per.items() if v["head-batch"]["count"] == 0]
    assert all(per[name]["head-batch"] == {**dict.fromkeys(U.METRICS, 0.0), "count": 0} for name in absent)


def test_detail_metrics_draws_from_the_generator_like_eval(golden):
    """One int64 from torch's CPU generator per side, as eval (and the reference's two DataLoader iterators) draw."""
    ds, ev = _evaluation("CountriesS1")
    model = _model(golden, "CountriesS1/RotatE")
    states = []
    for call in (ev.eval, ev.detail_metrics, ev.eval_per_relation):
        torch.manual_seed(5)
        call(model=model, dataset=ds.test)
        states.append(torch.get_rng_state())
    assert torch.equal(states[0], states[1]) and torch.equal(states[0], states[2])
    torch.manual_seed(5)
    assert not torch.equal(states[0], torch.get_rng_state())
