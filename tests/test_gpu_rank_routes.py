"""-m gpu: mkb_rank, mkb_rank_scores and mkb_topk (mkb_amd/csrc/rank.hip) on every route of ``run_rank`` and every row width of its
lane route, at the smallest shapes that select them (tests/util_rank_routes.py: the case table, seeded tables with planted exact
duplicates, float64 expectations from oracle.scoring, and a tolerance measured against the reference arithmetic's own fp32 error).

Per case and side:
  scores  the whole exported [B, N] block within ``tolerance`` of float64: 8 x err_ref on the lane route, twice the measured ratio
          on the two others (below); everywhere at most a quarter of one term of the sum, so a dropped or doubled dimension fails;
  rank    every rank equals the rank recounted on the host from the device's own exported block (stable descending order, lower id
          first, filtered candidates removed): no band -- the rank kernel finishes its scores with the fp32 operation of the export;
  ties    the planted copies of the target score bit-equal; the lower unfiltered copy counts before the target, the higher one and
          both filtered copies do not;
  band    every rank inside oracle.ranking.rank_bounds on the float64 scores with eps = 2 x tolerance (one rank wide for more than
          four fifths of the queries of each route: test_host_rank_routes.py);
  mkb_rank (no score hand-out) returns the ranks of mkb_rank_scores;
  top k   test_gpu_topk._run_exact at k = 1 and 10: filter kept / dropped / off, ids exact and scores bit for bit.

Largest device error / err_ref measured on the MI355X, per route (profiles/r22_rank_routes_errors.txt has every case and side):
  lane    1.55  (ComplEx hidden 1024, N = 130; every lane case stays below 8)
  tile    11.59 (RotatE hidden 4096, N = 130: 1.55e-5 against err_ref 1.34e-6; hidden 2052: 6.0; hidden <= 68: at most 1.5;
                 TransE at most 0.5)
  matrix  16.18 (DistMult hidden 4096 on the 64-row fp32 tiles, N = 129: 9.5e-5 against err_ref 5.9e-6; ComplEx hidden 256 on the
                 bf16x3 tiles: 8.7; entity_dim 16: at most 1.3)
The two routes above 8 sum a row's terms one after the other in fp32 (two running sums per pair in the register tile, the matrix
instruction's accumulator in the products), torch's blocked sums -- what err_ref measures -- do not: the error grows with the
row width as such a sum's does and no defect stands behind it.  These two routes are therefore held to twice their
measured ratio (util_rank_routes.MEASURED_RATIO), capped at a quarter of the typical term (the cap binds for TransE hidden 4096).
"""
import numpy as np
import pytest

import util_rank_routes as U

pytestmark = pytest.mark.gpu

CASE_IDS = [U.case_id(c) for c in U.CASES]


def _device_side(case):
    from util_gpu import dirty_device_memory, make_model
    from mkb_amd import evaluation

    pb = U.problem(case)
    dirty_device_memory()
    m = make_model(pb.model, pb.ent, pb.rel, pb.hidden, U.GAMMA, pb.modulus).eval()
    ev = evaluation.Evaluation(true_triples=[tuple(t) for t in pb.true.tolist()], entities={i: i for i in range(pb.N)},
                               relations={i: i for i in range(pb.R)}, batch_size=64, device="cuda", num_workers=0)
    return pb, m, ev


@pytest.mark.parametrize("case", U.CASES, ids=CASE_IDS)
def test_scores_ranks_ties_and_band(case):
    pb, m, ev = _device_side(case)
    tol = U.tolerance(pb.model, pb.hidden, case[6])
    err_ref = U.calibration(pb.model, pb.hidden)[0]
    rows = np.arange(pb.B)
    for mode in U.MODES:
        dev_ranks, dev_scores = ev.ranks(m, pb.triples, mode, chunk=pb.B, with_scores=True)
        plain_ranks = ev.ranks(m, pb.triples, mode, chunk=pb.B)
        dev_ranks, dev_scores, plain_ranks = dev_ranks.cpu().numpy(), dev_scores.cpu().numpy(), plain_ranks.cpu().numpy()
        want, _, filtered = U.expected(case)[mode]
        target = pb.target(mode)
        lo, hi = U.band(case, mode)
        what = f"{U.case_id(case)} {mode}"
        assert dev_scores.shape == (pb.B, pb.N) and dev_scores.dtype == np.float32
        # scores
        err = float(np.abs(dev_scores.astype(np.float64) - want).max())
        print(f"{what}: err_ref {err_ref:.3e}  device error {err:.3e}  ratio {err / err_ref:.2f}  (tolerance {tol:.3e})  "
              f"clear ranks {int((lo == hi).sum())} / {pb.B}")
        assert np.isfinite(dev_scores).all(), what
        assert err <= tol, f"{what}: [B, N] score block off by {err:.3e} > {tol:.3e} at {np.unravel_index(np.abs(dev_scores - want).argmax(), want.shape)}"
        # exact rank on the device's own scores
        np.testing.assert_array_equal(dev_ranks, U.ranks_from_scores(dev_scores, filtered, target), err_msg=f"{what}: rank vs the exported scores")
        # ties
        if pb.planted is not None:
            pl = pb.planted
            bits = dev_scores.view(np.uint32)
            for c in ("c1", "c2", "c3", "c4"):
                np.testing.assert_array_equal(bits[:, pl[c]], bits[:, pl["t"]], err_msg=f"{what}: copy {c} of the target's row")
            np.testing.assert_array_equal(bits[:, pl["q"]], bits[:, pl["p"]], err_msg=f"{what}: duplicated pair")
            for i in pb.tie_queries[mode]:
                assert target[i] == pl["t"]
                s = dev_scores[i]
                above = int(((s > s[pl["t"]]) & ~filtered[i]).sum())
                # c1 (lower id, a candidate) counts; c2 (lower, filtered), c3 (higher, filtered) and c4 (higher) do not
                assert dev_ranks[i] == above + 2, (what, i, int(dev_ranks[i]), above)
        # band around the float64 ranking
        inside = (lo <= dev_ranks) & (dev_ranks <= hi)
        assert inside.all(), (what, rows[~inside], lo[~inside], dev_ranks[~inside], hi[~inside])
        # mkb_rank == mkb_rank_scores
        np.testing.assert_array_equal(plain_ranks, dev_ranks, err_msg=f"{what}: mkb_rank vs mkb_rank_scores")


@pytest.mark.parametrize("case", U.CASES, ids=CASE_IDS)
def test_topk_exact(case):
    """mkb_topk over the same row strides and finishers: keep / drop / none, bit-exact against the device's own scores."""
    from test_gpu_topk import _run_exact

    pb, m, ev = _device_side(case)
    _run_exact(m, ev, pb.triples, pb.true, pb.N, pb.R, chunk=pb.B, ks=(1, 10))


def test_clear_rank_share():
    """The band check above is one rank wide for at least a third of the queries of every route family."""
    for fam, share in U.clear_share().items():
        assert share >= 1.0 / 3.0, (fam, share)


def test_width_limit_is_refused_and_eval_takes_the_reference_path():
    """4097 units: mkb_rank refuses with its documented message; Evaluation.eval never calls it and agrees with itself under
    force_reference_path."""
    from util_gpu import make_model
    from mkb_amd import _hip, evaluation

    rs = np.random.RandomState(4097)
    N, R, hidden = 20, 3, 4097
    rng = (U.GAMMA + 2.0) / hidden
    ent = rs.uniform(-rng, rng, size=(N, hidden)).astype(np.float32)
    rel = rs.uniform(-rng, rng, size=(R, hidden)).astype(np.float32)
    m = make_model("pRotatE", ent, rel, hidden, U.GAMMA, np.array([[0.5 * rng]], dtype=np.float32)).eval()
    true = np.stack([rs.randint(N, size=40), rs.randint(R, size=40), rs.randint(N, size=40)], 1)
    triples = [tuple(t) for t in true[:6].tolist()]
    ev = evaluation.Evaluation(true_triples=[tuple(t) for t in true.tolist()], entities={i: i for i in range(N)},
                               relations={i: i for i in range(R)}, batch_size=4, device="cuda", num_workers=0)
    for with_scores in (False, True):
        with pytest.raises(_hip.HipLibraryError, match="rows of more than 4096 units are not supported"):
            ev.ranks(m, triples, "tail-batch", with_scores=with_scores)
    assert not ev._device_ok(m)

    def refuse(*a, **k):
        raise AssertionError("Evaluation.eval took the device path at 4097 units")

    ev.ranks = refuse
    got = ev.eval(m, triples)
    ev.force_reference_path = True
    assert ev.eval(m, triples) == got
    assert set(got) == {"MRR", "MR", "HITS@1", "HITS@3", "HITS@10"} and 1.0 <= got["MR"] <= N
