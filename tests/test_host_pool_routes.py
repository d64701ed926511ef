"""CPU (-m "not gpu") tests of the pooled step's case table (tests/util_pool_routes.py), the table tests/test_gpu_pool_routes.py runs
on the device:

  leaves    every case selects the leaves of plan_pool it claims, under the folds of each entry point: a host program built on the
            library's own planning code (mkb_amd/csrc/score_pool_plan.h, compiled host-only with the compiler of csrc/build.py)
            prints the plan; the table reaches every leaf of util_pool_routes.LEAVES and both sides of every edge in EDGES;
  pools     the hand-built pools have the properties they are built for;
  reference the torch formulation of the step agrees with oracle.closed.train_step_grads wherever that fits the host;
  defects   float64 models of plausible defects move every case they apply to by at least 10 x the tolerance of some compared
            quantity (profiles/r26_pool_routes_sensitivity.txt keeps the smallest figure per defect).
"""
import pathlib
import subprocess

import numpy as np
import pytest
import torch

import util_pool_routes as U

ROOT = pathlib.Path(__file__).resolve().parent.parent

PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "score_pool_plan.h"
using namespace mkb;
static const char *family(const GemmPlan &p) {
    return p.kernel == GemmKernel::Bf16x3Tile128 ? "bf16x3" : p.kernel == GemmKernel::F32Tile128 ? "f32tile128" : "f32tile64";
}
static void product(const char *name, const GemmPlan &p) {
    printf(" %s=%s,tm%d,tn%d,ks%d,%s,%s", name, family(p), p.tm, p.tn, p.ks,
           p.tail == GemmTailKind::Reduce ? "reduce" : p.tail == GemmTailKind::Scatter ? "scatter" : "notail",
           p.dest == GemmDest::Slices ? "slices" : p.dest == GemmDest::Partials ? "partials" : "final");
}
// model hidden B K n_entity n_relation aligned no_mfma dense no128 no_pair bf16x3 fold_s fold_x -> one line of key=value words
int main(int argc, char **argv) {
    if (argc != 15) return 2;
    const char *names[] = {"TransE", "DistMult", "ComplEx", "RotatE", "pRotatE"};
    const int ids[] = {MKB_TRANSE, MKB_DISTMULT, MKB_COMPLEX, MKB_ROTATE, MKB_PROTATE};
    int model = -1;
    for (int i = 0; i < 5; ++i) if (!strcmp(argv[1], names[i])) model = ids[i];
    if (model < 0) return 2;
    const int hidden = atoi(argv[2]);
    const int64_t B = atoll(argv[3]), K = atoll(argv[4]);
    mkb_tables_t tb{};
    tb.model = model;
    tb.hidden_dim = hidden;
    tb.n_entity = atoll(argv[5]);
    tb.n_relation = atoll(argv[6]);
    tb.entity_dim = (model == MKB_ROTATE || model == MKB_COMPLEX) ? 2 * hidden : hidden;
    tb.relation_dim = model == MKB_COMPLEX ? 2 * hidden : hidden;
    tb.ent = (const float *)(uintptr_t)(atoi(argv[7]) ? 0x40000000 : 0x40000004);  // (only its alignment is looked at)
    const int dense = atoi(argv[9]);
    const PoolSwitches sw{atoi(argv[8]) != 0, dense < 0 ? PoolSwitches::kDenseDefault : (dense ? PoolSwitches::kDenseOn : PoolSwitches::kDenseOff),
                          GemmSwitches{atoi(argv[10]) != 0, atoi(argv[11]) != 0, atoi(argv[12]) != 0}};
    const PoolFolds folds{atoi(argv[13]) != 0, atoi(argv[14]) != 0};
    PoolPlan L;
    if (2 * K > kMaxP || !plan_pool(&tb, B, 2 * K, sw, folds, L)) { printf("supported=0\n"); return 0; }
    printf("supported=1 kpt=%d nw=%d rel_copies=%d dq_parts=%d", L.kpt, L.nw, L.rel_copies, L.dq_parts);
    switch (L.fwd) {
        case FwdRoute::Matrix: printf(" fwd=Matrix"); product("s", L.gemm); break;
        case FwdRoute::Tile: printf(" fwd=Tile fkpt=%d kd=%d ks=%d", L.tile.kpt, L.tile.kd, L.tile.ks); break;
        case FwdRoute::RowTile: printf(" fwd=RowTile fkpt=%d fnw=%d fslices=%d", L.rows.kpt, L.rows.nw, L.rows.slices); break;
    }
    switch (L.bwd) {
        case BwdRoute::Matrix:
            printf(" bwd=Matrix pair=%d", (int)L.products.pair);
            product("dq", L.products.dq);
            product("dx", L.products.dx);
            break;
        case BwdRoute::SinglePass:
            printf(" bwd=SinglePass blocks=%d halves=%d dim_slices=%d bkpt=%d nc=%d tiles_per_wave=%d row_groups=%d dense_lanes=%d grid=%u",
                   L.single.blocks, L.single.halves, L.single.dim_slices, L.single.kpt, L.single.nc(), L.single.tiles_per_wave,
                   L.single.row_groups, L.single.dense_lanes, L.single.grid());
            break;
        case BwdRoute::Wave: printf(" bwd=Wave bkpt=%d chunks=%d slices=%d", L.wave.kpt, L.wave.chunks, L.wave.slices); break;
        case BwdRoute::TwoPass: printf(" bwd=TwoPass q_slices=%d x_slices=%d", L.two.q_slices, L.two.x_slices); break;
    }
    printf("\n");
    return 0;
}
"""

# What the three entry-point families pass as PoolFolds (score_pool.hip) at the shapes of this table: mkb_pool_step, mkb_pool_step_fwd /
# bwd, mkb_pool_score_fwd / bwd.  mkb_pool_step folds the score product only up to 2K = 1024 positions, and its backward half only
# when the forward really left a tail; only matrix-route plans read the folds, and those cases have K <= 512 (asserted below).
FOLDS = {"step": (1, 1), "half": (0, 1), "score": (0, 0)}


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    from mkb_amd.csrc import build

    d = tmp_path_factory.mktemp("pool_plan")
    (d / "main.cc").write_text(PROGRAM)
    exe = d / "pool_plan"
    subprocess.run([build.HIPCC, "--cuda-host-only", "-std=c++17", "-O1", "-Wno-unused-function", "-I", str(ROOT / "mkb_amd" / "csrc"),
                    str(d / "main.cc"), "-o", str(exe)], check=True, capture_output=True)

    def ask(case, entry="step"):
        _, model, hidden, B, K, N, R = case[:7]
        sw = U.switches(case)
        args = [model, hidden, B, K, N, R, 0 if "misaligned" in sw else 1, int(sw.get("MKB_POOL_NO_MFMA") == "1"),
                {None: -1, "0": 0, "1": 1}[sw.get("MKB_POOL_DENSE")], int("MKB_GEMM_NO128" in sw), int("MKB_GEMM_NO_PAIR" in sw),
                int(sw.get("MKB_GEMM_BF16X3", "1") != "0"), *FOLDS[entry]]
        return subprocess.run([str(exe)] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout.split()

    return ask


@pytest.mark.parametrize("case", U.CASES, ids=U.CASE_IDS)
def test_the_case_selects_the_leaves_it_claims(planner, case):
    plans = {entry: planner(case, entry) for entry in FOLDS}
    for entry, words in plans.items():
        print(f"pool-plan {case[0]} {entry}: {' '.join(words)}")
        assert "supported=1" in words, (case[0], entry)
    for claim in case[8]:
        entry, word = claim.split(":", 1) if ":" in claim else ("step", claim)
        assert word in plans[entry], (case[0], claim, plans[entry])


def test_the_table_reaches_every_leaf_and_both_sides_of_every_edge(planner):
    claims = [set(c[8]) for c in U.CASES]
    for leaf in U.LEAVES:
        assert any(leaf <= c for c in claims), f"no case claims {sorted(leaf)}"
    for below, above, word_below, word_above in U.EDGES:  # the word the edge is about flips between the two cases
        lo, hi = planner(U.case_named(below)), planner(U.case_named(above))
        assert word_below in lo and word_below not in hi and word_above in hi and word_above not in lo, (below, above, lo, hi)
    # riders: a misaligned table on a VALU and on the matrix route, B = 1, B no multiple of 8, few and many relations, pRotatE
    sw = [U.switches(c) for c in U.CASES]
    assert sum("misaligned" in s for s in sw) >= 2
    assert {1} <= {c[3] for c in U.CASES} and any(c[3] % 8 for c in U.CASES)
    assert any(c[6] == 2 and c[3] >= 32 for c in U.CASES) and any(c[6] >= 5000 for c in U.CASES)
    assert any(c[1] == "pRotatE" for c in U.CASES)
    assert any(c[1] in ("ComplEx", "DistMult") and c[3] < 2 * c[4] and "fwd=Matrix" in c[8] for c in U.CASES)  # B < 2K on the matrix route
    # the entry points plan differently somewhere in the table: a folding product takes another K split
    assert any(planner(c, "step") != planner(c, "score") for c in U.CASES)
    # every switch of the plan is thrown by some case
    thrown = set().union(*[set(s) for s in sw])
    assert thrown >= {"MKB_POOL_NO_MFMA", "MKB_POOL_DENSE", "MKB_GEMM_BF16X3", "MKB_GEMM_NO_PAIR", "MKB_GEMM_NO128", "misaligned"}
    # the folds restated in FOLDS hold for every case that reads them
    assert all(c[4] <= 512 for c in U.CASES if "fwd=Matrix" in planner(c))


@pytest.mark.parametrize("case", U.CASES, ids=U.CASE_IDS)
def test_the_pools_have_the_patterns_they_are_built_for(case):
    _, model, hidden, B, K, N, R = case[:7]
    for scale in U.SCALES:
        s, a = U.problem(case, scale, "sampler"), U.problem(case, scale, "adversarial")
        for pb in (s, a):
            assert pb.pos.shape == (B, K) and pb.cnt.shape == (B, 2 * K) and (pb.cnt.sum(1) == K).all() and pb.cnt.max() < 1 << 16
            assert np.array_equal(pb.neg, pb.pool[pb.pos]) and pb.pool.min() >= 0 and pb.pool.max() < N
            assert pb.weight.min() >= 0.5 and pb.weight.max() <= 1.5 and pb.cnt[B - 1].any()
        assert a.pos[0].min() >= K and a.cnt[:, 2 * K - 1].any()              # a row off the dense prefix; position P - 1 in use
        if B >= 2:
            assert a.cnt[1].max() == K                                       # one position taken K times
        if K >= 4:
            assert len(a.unused()) >= 2 and a.pool[2] == a.pool[K + 2]       # unused positions; one entity at two positions
            assert a.cnt[:, K].any()                                         # the first position past K in use
        assert a.shared in a.pool and a.shared in a.sample[:, 0] and a.shared in a.sample[:, 2]
        if B >= 3:
            assert a.cnt[:, 3 % (2 * K)].any()                               # ... at a position some row uses
    if model not in ("ComplEx", "DistMult") and U.units(model, hidden) >= 63 and U.terms(case) <= U.DEFECT_TERMS:
        big = np.abs(U.expected(case, "tail-batch", "trained", "sampler")[0]["S"]).max()
        assert 15 <= big <= 150, big                                         # |score| of a trained model, not of an initialised one


HOST_CASES = [c for c in U.CASES if U.on_host(c)]


@pytest.mark.parametrize("case", HOST_CASES, ids=[c[0] for c in HOST_CASES])
def test_the_torch_formulation_is_the_closed_form(case):
    """util_pool_routes.step (float64, the pooled form) against oracle.closed.train_step_grads on the [B, K] negatives: they are
    two float64 evaluations of one formula, so they agree to a few float64 roundings per term, relative to each quantity's size."""
    n = 0
    for scale in U.SCALES:
        for pattern in U.PATTERNS:
            mode = U.MODES[n % 2]
            n += 1
            pb = U.problem(case, scale, pattern)
            mine = U.run_step(pb, mode, torch.float64)
            ref, _ = U.closed_step(pb, mode)
            used = pb.cnt > 0
            for q in U.QUANTITIES:
                a, b = (mine[q] * used, ref[q] * used) if q == "S" else (mine[q], ref[q])
                size = max(float(np.abs(b).max()), 1e-300)
                assert float(np.abs(a - b).max()) <= 2.0 ** -40 * size, (case[0], scale, pattern, mode, q)
            # the |term| sums bound the gradients they stand behind
            assert (np.abs(ref["g_ent"]) <= mine["a_ent"] * (1 + 1e-9) + 1e-300).all()
            assert (np.abs(ref["g_rel"]) <= mine["a_rel"] * (1 + 1e-9) + 1e-300).all()


def test_the_expectation_of_a_large_case_is_the_same_formulation():
    """Cases too large for oracle.closed take ``step`` itself in float64 (and in float32 for err_ref): the very function pinned
    above, on the same kind of problem."""
    large = [c for c in U.CASES if not U.on_host(c)]
    assert large and all(U.terms(c) > U.HOST_TERMS for c in large)
    case = min(large, key=U.terms)
    f64, err, rows = U.expected(case, "head-batch", "trained", "adversarial")
    pb = U.problem(case, "trained", "adversarial")
    mine = U.run_step(pb, "head-batch", torch.float64)
    assert all(np.array_equal(f64[q], mine[q]) for q in U.QUANTITIES)
    assert all(err[q] > 0 for q in U.QUANTITIES) and (rows["g_ent"] > 0).all()


# (the bilinear models' float64 step is three matrix products whatever the size; of the distance cases only tile-ks4 / 2 / 1, 5.5e8 .. 2.2e9 terms,
# are too large for the host: its route's smaller siblings tile-rotate and sp-h2-rotate are evaluated)
DEFECT_CASES = [c for c in U.CASES if U.terms(c) <= U.DEFECT_TERMS or c[1] in ("ComplEx", "DistMult")]
assert sorted(c[0] for c in U.CASES if c not in DEFECT_CASES) == ["tile-ks1", "tile-ks2", "tile-ks4"]


@pytest.mark.parametrize("case", DEFECT_CASES, ids=[c[0] for c in DEFECT_CASES])
def test_every_defect_model_moves_the_case(case):
    mode = U.MODES[U.CASES.index(case) % 2]
    weak = []
    for defect in U.DEFECTS:
        if not U.applies(case, defect):
            continue
        for side in (mode, U.MODES[1 - U.MODES.index(mode)]):  # (the device test runs both sides: the other one is asked where the first is weak)
            ratio, where = U.defect_move(case, side, "trained", defect)
            print(f"pool-routes-sensitivity {case[0]} {side} {defect}: move / tolerance {ratio:.3g} in {where}")
            if ratio >= 10:
                break
        else:
            weak.append((defect, ratio, where))
    assert not weak, weak


def test_a_measured_ratio_is_listed_only_above_the_factor():
    for (name, quantity), ratio in U.MEASURED_RATIO.items():
        assert name in U.CASE_IDS and quantity in U.QUANTITIES + ("g_ent/rows", "g_rel/rows") and ratio > U.ERR_FACTOR
