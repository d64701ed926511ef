"""Shared by the detail_eval tests: the cases of tests/golden/detail_eval.{npz,json} (tools/make_golden.py::gen_detail_eval) and
a numpy restatement of the grouped metrics."""
import math

import numpy as np

MODES = ("head-batch", "tail-batch")
TYPES = ("1_1", "1_M", "M_1", "M_M")
METRICS = ("MRR", "MR", "HITS@1", "HITS@3", "HITS@10")
CASES = ("CountriesS1/TransE", "CountriesS1/RotatE", "Umls/TransE", "Umls/RotatE")

TOY_TRAIN = [(0, 0, 1), (0, 1, 1), (2, 0, 3), (2, 1, 3)]
TOY_TEST = [(0, 0, 1), (2, 1, 3)]
TOY_TRUE = TOY_TRAIN + TOY_TEST + TOY_TEST  # train + valid + test of the reference's class docstring: repeats included
TOY_ENTITIES = {f"e{i}": i for i in range(4)}
TOY_RELATIONS = {"r0": 0, "r1": 1}

_DATASETS = {}


def dataset(name):
    from mkb_amd import datasets

    if name not in _DATASETS:
        _DATASETS[name] = getattr(datasets, name)(batch_size=8, shuffle=False, seed=42, num_workers=0)
    return _DATASETS[name]


def group_sums(ranks, relations, group_of_relation, n_groups):
    """What mkb_rank_metrics computes: (int64 [G, 5], float64 [G] by math.fsum)."""
    ranks, relations = np.asarray(ranks, dtype=np.int64), np.asarray(relations, dtype=np.int64)
    table = np.asarray(group_of_relation, dtype=np.int64)
    ok = (relations >= 0) & (relations < len(table))
    group = np.full(len(ranks), -1, dtype=np.int64)
    group[ok] = table[relations[ok]]
    counts, rr = np.zeros((n_groups, 5), dtype=np.int64), np.zeros(n_groups, dtype=np.float64)
    for g in range(n_groups):
        r = ranks[group == g]
        counts[g] = [len(r), sum(int(v) for v in r), int((r <= 1).sum()), int((r <= 3).sum()), int((r <= 10).sum())]
        rr[g] = math.fsum(1.0 / int(v) for v in r)
    return counts, rr


def type_table(types, relations):
    """int32 [R]: the category index of every relation id, -1 where ``types`` ({name: category}) has none."""
    table = np.full(len(relations), -1, dtype=np.int32)
    for name, kind in types.items():
        table[relations[name]] = TYPES.index(kind)
    return table


def assert_metrics_close(got, want, atol):
    assert set(got) == set(want) == {*MODES, "frequency"}
    for mode in MODES:
        assert list(got[mode]) == list(TYPES)
        for kind in TYPES:
            assert list(got[mode][kind]) == list(METRICS)
            for metric in METRICS:
                assert abs(got[mode][kind][metric] - want[mode][kind][metric]) <= atol, (mode, kind, metric, got[mode][kind], want[mode][kind])
    for kind in TYPES:
        assert abs(got["frequency"][kind] - want["frequency"][kind]) <= 1e-12, (kind, got["frequency"], want["frequency"])
