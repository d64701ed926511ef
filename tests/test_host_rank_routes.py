"""Host checks of the route tests' own material (tests/util_rank_routes.py): the case table reaches every route, instantiation
and selection edge of ``run_rank``; the tolerance is tight enough to see one dropped or doubled dimension; the planted duplicates
tie exactly; and the float64 expectation agrees with the pinned fp32 reference ranking wherever nothing is within the near-tie band.
No GPU."""
import numpy as np
import pytest
import torch

import util_rank_routes as U
from oracle import ranking, scoring


def _has(**want):
    """Cases of the table whose fields match ``want`` (model, hidden, N, B, route, inst; a set means any of its members)."""
    names = ("model", "hidden", "N", "R", "B", "n_true", "route", "inst")
    out = []
    for case in U.CASES:
        row = dict(zip(names, case))
        if all(row[k] in v if isinstance(v, (set, frozenset, tuple)) else row[k] == v for k, v in want.items()):
            out.append(case)
    return out


def test_route_of_agrees_with_the_table():
    for case in U.CASES:
        assert U.route_of(case) == (case[6], case[7]), U.case_id(case)
    assert len({U.case_id(c) for c in U.CASES}) == len(U.CASES)


def test_cases_cover_routes_instantiations_and_edges():
    routes = {U.route_of(c) for c in U.CASES}
    assert {r for r, _ in routes} == {"lane", "tile", "matrix"}
    assert {i for r, i in routes if r == "lane"} == {"kpt1", "kpt2w8", "kpt2w16", "kpt4"}
    assert {i for r, i in routes if r == "matrix"} == {"f32tile64", "bf16x3"}
    # the lane instantiations by model, as the issue lists them
    lane = {
        "kpt1": [("pRotatE", 3), ("RotatE", 31), ("TransE", 63), ("DistMult", 512)],
        "kpt2w8": [("pRotatE", 513), ("RotatE", 1022), ("ComplEx", 300), ("TransE", 1023)],
        "kpt2w16": [("pRotatE", 1025), ("RotatE", 2046), ("ComplEx", 1024), ("DistMult", 2048), ("TransE", 2047)],
        "kpt4": [("pRotatE", 2049), ("pRotatE", 4096), ("RotatE", 2050), ("RotatE", 4094), ("ComplEx", 1025), ("ComplEx", 2048),
                 ("DistMult", 4096), ("TransE", 4095)],
    }
    for inst, pairs in lane.items():
        for model, hidden in pairs:
            assert _has(model=model, hidden=hidden, route="lane", inst=inst), (inst, model, hidden)
    assert _has(model="DistMult", hidden=512, B=5) and _has(model="ComplEx", hidden=300, B=7)
    assert _has(model="ComplEx", hidden=1024, B=31) and _has(model="DistMult", hidden=2048, B=30) and _has(model="DistMult", hidden=4096, B=9)
    assert all(c[4] < 32 for c in _has(model="ComplEx", hidden=(1025, 2048)))
    wide_lane = [c for c in _has(route="lane") if c[1] >= 3 and c[4] <= 31]
    assert {1, 5, 8, 9} <= {c[4] for c in wide_lane} and {1, 2, 17, 33, 130} <= {c[2] for c in wide_lane}
    assert _has(route="lane", N=512) and _has(route="lane", N=513)
    # both sides of every selection edge
    for hidden, route in ((31, "lane"), (32, "tile"), (36, "tile"), (2052, "tile"), (4096, "tile")):
        assert _has(model="RotatE", hidden=hidden, route=route), hidden
    for hidden, route in ((63, "lane"), (64, "tile"), (68, "tile"), (4096, "tile")):
        assert _has(model="TransE", hidden=hidden, route=route), hidden
    assert {1, 63, 64, 65, 130} <= {c[2] for c in _has(route="tile")} and {1, 63, 64, 65} <= {c[4] for c in _has(route="tile")}
    assert _has(model="ComplEx", hidden=8, route="matrix") and _has(model="DistMult", hidden=16, route="matrix")
    assert _has(model="DistMult", hidden=4096, B=32, route="matrix")
    assert {32, 36} <= {c[4] for c in _has(route="matrix")} and {1, 2, 3, 5, 127, 128, 129} <= {c[2] for c in _has(route="matrix")}
    assert _has(model=("ComplEx", "DistMult"), B=28, route="lane") and _has(model="DistMult", hidden=12, B=32, route="lane")
    # the lane route's grid: fewer entities than slices (one entity per slice) and slices that cross the 16-candidate slab
    per = {U.lane_slices(c)[1] for c in _has(route="lane")}
    assert 1 in per and {15, 16, 17, 19} <= per, sorted(per)
    # size limits: tables of at most ~5 MB
    for model, hidden, N, R, B, *_ in U.CASES:
        de = scoring.dims(model, hidden)[0]
        assert 2 <= R <= 7 and N <= (130 if de > 1024 else 1030) and N * de * 4 <= 5.5e6, (model, hidden, N)


@pytest.mark.parametrize("model,hidden,route", sorted({(c[0], c[1], c[6]) for c in U.CASES}))
def test_tolerance_sees_one_dimension(model, hidden, route):
    """The tolerance -- 8 x err_ref, or twice the route's measured ratio -- is at most a quarter of the typical single term of a
    score: a dropped or doubled dimension fails the score check."""
    err_ref, term = U.calibration(model, hidden)
    tol = U.tolerance(model, hidden, route)
    print(f"{model} hidden {hidden} {route}: err_ref {err_ref:.3e}  tolerance {tol:.3e}  typical term {term:.3e}  term / err_ref {term / max(err_ref, 1e-300):.1f}")
    assert err_ref > 0 and 8.0 * err_ref <= 0.25 * term, (model, hidden, err_ref, term)
    assert tol == 8.0 * err_ref if route == "lane" else 8.0 * err_ref <= tol <= 2.0 * U.MEASURED_RATIO[route] * err_ref
    assert tol <= 0.25 * term, (model, hidden, tol, term)


def test_planted_duplicates_tie_exactly_and_the_filter_is_as_planned():
    n = 0
    for case in U.CASES:
        pb = U.problem(case)
        exp = U.expected(case)
        # every query filters at least one candidate on each side (N = 1 has none)
        for mode in U.MODES:
            f = exp[mode][2]
            assert not f[np.arange(pb.B), pb.target(mode)].any()
            if pb.N >= 2:
                assert f.any(axis=1).all(), (U.case_id(case), mode)
        if pb.planted is None:
            assert pb.N < 8
            continue
        pl = pb.planted
        assert pl["c1"] < pl["c2"] < pl["t"] < pl["c3"] < pl["c4"] and pl["p"] < pl["q"]
        for mode in U.MODES:
            s, ranks, f = exp[mode]
            for c in ("c1", "c2", "c3", "c4"):
                np.testing.assert_array_equal(s[:, pl[c]], s[:, pl["t"]])
            np.testing.assert_array_equal(s[:, pl["p"]], s[:, pl["q"]])
            ties = pb.tie_queries[mode]
            assert ties and (pb.target(mode)[ties] == pl["t"]).all()
            for i in ties:
                assert not f[i, pl["c1"]] and f[i, pl["c2"]] and f[i, pl["c3"]] and not f[i, pl["c4"]]
                above = int(((s[i] > s[i, pl["t"]]) & ~f[i]).sum())
                assert ranks[i] == 1 + above + 1  # c1 and nothing else of the group
                n += 1
    assert n >= 2 * sum(1 for c in U.CASES if c[2] >= 8)


def test_expected_ranks_agree_with_the_pinned_reference_outside_near_ties():
    """``oracle.ranking.scores_and_ranks`` (fp32, the reference's argsort) against the float64 expectation on every query whose
    band is one rank wide (no duplicate of the target, no candidate within 2 x tolerance of it)."""
    compared = 0
    for case in U.CASES:
        pb = U.problem(case)
        if pb.B > 400:  # (the many-query cases repeat a 17-entity table: the first 400 queries say the same)
            rows = np.arange(400)
        else:
            rows = np.arange(pb.B)
        tb = pb.tables(torch.float32)
        chunk = 4 if scoring.dims(pb.model, pb.hidden)[0] > 1024 else 64
        for mode in U.MODES:
            _, _, ref = ranking.scores_and_ranks(tb, pb.triples[rows], pb.keys, mode, chunk=chunk, fast_norm=True, want_raw=False)
            lo, hi = U.band(case, mode)
            want = U.expected(case)[mode][1]
            assert ((lo <= want) & (want <= hi)).all()
            clear = (lo == hi)[rows]
            np.testing.assert_array_equal(ref[clear], want[rows][clear], err_msg=f"{U.case_id(case)} {mode}")
            assert ((lo[rows] <= ref) & (ref <= hi[rows])).all(), (U.case_id(case), mode)
            compared += int(clear.sum())
    assert compared >= 1000, compared


def test_clear_rank_share_per_route_family():
    """At least one third of the (query, side) pairs of each route family have a band of one rank, so the band check on the device
    pins most ranks exactly."""
    share = U.clear_share()
    print({k: round(v, 3) for k, v in share.items()})
    for fam, s in share.items():
        assert s >= 1.0 / 3.0, (fam, s)
