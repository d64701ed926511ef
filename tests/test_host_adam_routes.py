"""CPU (-m "not gpu") tests of the Adam launches' case table (tests/util_adam_routes.py), the table tests/test_gpu_adam_routes.py runs
on the device:

  leaves    every case selects the leaves of plan_adam_rows it claims: a host program built on the library's own planning code
            (mkb_amd/csrc/adam_plan.h, compiled host-only with the compiler of csrc/build.py) prints the plan; the table reaches every
            leaf of util_adam_routes.LEAVES and the claimed word flips across every pair of EDGES;
  schedule  the id lists and the replays they cause have the properties they are built for;
  reference the float64 restatement of the element rule is torch.optim.Adam on float64 tensors;
  defects   float64 models of plausible defects move every case they apply to by at least 10 x the tolerance of some compared
            quantity (profiles/r27_adam_routes_sensitivity.txt keeps the smallest figure per defect);
  cap       err_ref is the one-ulp floor for p in at most a quarter of a case's rows that took a non-zero gradient (the other rows
            hold their initial bits on both sides and sit on the floor by construction).
"""
import pathlib
import subprocess

import numpy as np
import pytest
import torch

import util_adam_routes as U

ROOT = pathlib.Path(__file__).resolve().parent.parent

PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "adam_plan.h"
using namespace mkb;
// call D aligned rows n_table step listed forced_sweep rider_n -> one line of key=value words
int main(int argc, char **argv) {
    if (argc != 10) return 2;
    if (!strcmp(argv[1], "dense")) {  // dense n threads max_blocks: the workgroups of a dense launch
        printf("blocks=%lld\n", (long long)adam_dense_blocks(atoll(argv[2]), atoi(argv[3]), atoll(argv[4])));
        return 0;
    }
    const AdamRowsCall call = !strcmp(argv[1], "step") ? AdamRowsCall::Step : AdamRowsCall::Advance;
    const AdamRowsShape s{atoll(argv[2]), atoi(argv[3]) != 0, atoll(argv[4]), atoll(argv[5]), atoll(argv[6]), atoi(argv[7]) != 0, atoi(argv[8]),
                          atoll(argv[9])};
    const AdamRowsPlan P = plan_adam_rows(call, s);
    const char *kernel = P.kernel == AdamRowsKernel::CatchupUnroll ? "unroll" : P.kernel == AdamRowsKernel::CatchupLean ? "lean"
                         : P.kernel == AdamRowsKernel::Flush ? "flush" : "step";
    printf("kernel=%s unroll=%d threads=%d vec4=%d epl=%d access=%d rpb=%d lanes=%d passes=%d sweep=%lld sweep_start=%lld rows_listed=%lld "
           "row_blocks=%lld rider_blocks=%lld table_bound=%lld caps=%lld,%lld\n",
           kernel, P.kernel == AdamRowsKernel::CatchupUnroll ? kReplayUnroll : 1, P.threads, P.vec4, P.epl, P.access, P.rows_per_block,
           P.lanes_per_row, P.passes, (long long)P.sweep_rows, (long long)P.sweep_start, (long long)P.rows_listed, (long long)P.row_blocks,
           (long long)P.rider_blocks, (long long)P.table_bound, (long long)kAdamDenseMaxBlocks, (long long)kAdamRiderMaxBlocks);
    return 0;
}
"""


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    from mkb_amd.csrc import build

    d = tmp_path_factory.mktemp("adam_plan")
    (d / "main.cc").write_text(PROGRAM)
    exe = d / "adam_plan"
    subprocess.run([build.HIPCC, "--cuda-host-only", "-std=c++17", "-O1", "-Wno-unused-function", "-I", str(ROOT / "mkb_amd" / "csrc"),
                    str(d / "main.cc"), "-o", str(exe)], check=True, capture_output=True)

    def ask(*args):
        args = list(args) + [0] * (9 - len(args))
        return subprocess.run([str(exe)] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout.split()

    return ask


def _plans(planner, case, rows=None, step=7):
    """The plan words of the case's three launches, prefixed: the catch-up over ``rows`` listed ids (default L), the closing flush,
    mkb_adam_rows_step."""
    forced = -1 if case.sweep is None else int(case.sweep)
    rows = case.L if rows is None else rows
    words = {"catch": planner("advance", case.D, int(case.off == 0), rows, case.N, step, 1, forced, case.rider),
             "flush": planner("advance", case.D, int(case.off == 0), case.N, case.N, case.T, 0, forced, case.rider),
             "step": planner("step", case.D, int(case.off == 0), rows, case.N, step, 1, forced, case.rider)}
    return {f"{k}:{w}" for k, ws in words.items() for w in ws}


@pytest.mark.parametrize("case", U.CASES, ids=U.CASE_IDS)
def test_the_case_selects_the_leaves_it_claims(planner, case):
    words = _plans(planner, case)
    print(f"adam-plan {case.name}: {' '.join(sorted(words))}")
    assert {"catch:threads=512", "flush:kernel=flush", "flush:threads=256", "step:kernel=step", "step:threads=256", "flush:unroll=1",
            "catch:caps=2048,1024"} <= words
    for claim in case.claims - {"own"}:
        assert claim in words, (case.name, claim, sorted(words))
    # what util_adam_routes restates of the plan (the extra id lists, the second-chunk defect and the model of `last` build on it)
    epl, lanes, rpb = U.geometry(case)
    assert {f"catch:epl={epl}", f"catch:lanes={lanes}", f"catch:rpb={rpb}"} <= words
    for t in (1, 7, case.T):
        for rows in (1, rpb + 1, case.L):
            w = _plans(planner, case, rows, t)
            window = U.sweep_window(case, rows, t)
            assert f"catch:sweep={len(window)}" in w and (len(window) == 0 or f"catch:sweep_start={window[0]}" in w), (case.name, t, rows)
    assert "catch:unroll=4" in words or "catch:kernel=lean" in words


def test_the_table_reaches_every_leaf_and_both_sides_of_every_edge(planner):
    claims = [set(c.claims) for c in U.CASES]
    for leaf in U.LEAVES:
        assert any(leaf <= c for c in claims), f"no case claims {sorted(leaf)}"
    for below, above, word_below, word_above in U.EDGES:  # the word the edge is about flips between the two cases
        lo, hi = _plans(planner, U.case_named(below)), _plans(planner, U.case_named(above))
        assert word_below in lo and word_below not in hi and word_above in hi and word_above not in lo, (below, above)
    # the widths the issue names, each side of each edge
    have = {c.D for c in U.CASES}
    assert have >= {256, 260, 512, 516, 1024, 1028, 2000, 2048, 2052, 4100, 126, 130, 510, 514, 1022, 1026, 2050, 1, 3, 33, 1023, 1025, 255, 257}
    assert any(c.off == 1 and c.D % 4 == 0 for c in U.CASES)
    # 12 x listed rows | one fewer; the switch at 0; a forced period with short gaps
    assert all(c.N in (12 * c.L, 12 * c.L - 1) for c in U.CASES)
    assert {c.rider for c in U.CASES} >= {0, 4, 5, 37 * 64 + 3, 1024 * 256 * 4 + 5, 1024 * 512 * 4 + 5}
    assert any(c.betas == (0.4, 0.9) for c in U.CASES) and any(c.own and c.D > 2048 for c in U.CASES)
    # the dense launches: one workgroup (the tail elements ride its lanes) up to 1025 floats, the grid-stride cap of 2048 past it
    assert [planner("dense", n, 256, 2048)[0] for n in U.DENSE_NS] == ["blocks=1"] * 8 + ["blocks=2048"]
    assert sorted(n for n, _ in U.MULTI)[:4] == [1, 3, 4, 5] and {1, 3, 1025} <= {n for n, _ in U.MULTI} and len(U.MULTI) == 8
    assert len({s for _, s in U.MULTI}) == 8


@pytest.mark.parametrize("case", U.CASES, ids=U.CASE_IDS)
def test_the_schedule_has_the_patterns_it_is_built_for(case):
    rpb = U.geometry(case)[2]
    extra_lengths = set()
    for t, (ids, extras) in enumerate(U.schedule(case), start=1):
        assert ids.shape == (case.L,) and (ids < 0).sum() == 1 and (ids >= case.N).sum() == 1
        assert len(U.valid_rows(case, ids)) <= case.L - 5, "at least three duplicates"
        extra_lengths |= {len(e) for e in extras}
    if case.T >= max(U.EXTRA_STEPS):
        assert extra_lengths == {1, rpb - 1, rpb + 1} - {0}
    touched = np.unique(np.concatenate([U.valid_rows(case, ids) for ids, _ in U.schedule(case)]))
    assert 0 in touched and case.N - 1 in touched and len(touched) < case.N // 4  # most rows are never touched
    zero_rows = sum(int((vals.abs().sum(1) == 0).sum()) for _, vals in U.gradients(case))
    assert zero_rows >= case.T // 2, "touched rows with an all-zero gradient"
    scales = {r % 4 for rows, _ in U.gradients(case) for r in rows}
    assert scales == {0, 1, 2, 3} and {(r // 4) % 2 for r in touched} == {0, 1}
    assert U.lr_of(case, case.T // 2) != U.lr_of(case, case.T // 2 + 1)
    for form in ("plain", "advance"):
        seen, last = U.replay_counts(case, form)
        assert (last == case.T).all()
        if case.T < 40:
            continue
        catch = {n for kind, n, first in seen if kind == "catch" and first == (form == "advance")}
        if not len(U.sweep_window(case, case.L, 7)):  # without a window the gaps are the schedule's own
            assert set(U.GAPS[:-1]) <= catch and max(catch) >= 33, (form, sorted(catch))
        else:  # the window splits them: every remainder class of the four-wide loop, and a group, still occur
            assert {n % 4 for n in catch} == {0, 1, 2, 3} and max(catch) >= 4, (form, sorted(catch))
        assert {n % 4 for kind, n, _ in seen if kind == "flush"} == {0, 1, 2, 3}
    if case.sweep == "7":  # the forced window wraps past the end of the table in mid-window, and overlaps listed ids
        windows = [U.sweep_window(case, case.L, t - 1) for t in range(2, case.T + 1)]
        assert any(w[0] > w[-1] for w in windows)
        assert any(np.intersect1d(w, U.valid_rows(case, U.schedule(case)[t - 1][0])).size for t, w in enumerate(windows, start=2))
    if case.own:
        for ids, _ in U.schedule(case):
            glob, local = U.own_split(case, ids)
            mine = glob[glob % 3 == 1] // 3
            assert (glob % 3 != 1).any() and len(glob) and len(local)
            assert set(U.valid_rows(case, np.concatenate([mine, local])).tolist()) == set(U.valid_rows(case, ids).tolist())
            assert not set((glob[glob % 3 != 1] // 3).tolist()) & set(U.valid_rows(case, ids).tolist())


@pytest.mark.parametrize("name", ["f4-256", "odd-33", "f2-1026", "betas-130"])
def test_the_float64_rule_is_torch_adam_on_float64(name):
    """util_adam_routes.run64 against torch.optim.Adam on float64 CPU tensors, at default and at changed betas, across the change of
    the learning rate: two float64 evaluations of one rule, equal to 2^-40 of each quantity's size."""
    case = U.case_named(name)
    mine, ref = U.run64(case), U.run_torch(case, torch.float64)
    for q in U.QUANTITIES:
        size = np.abs(ref[q]).max(1, keepdims=True)  # per row: the rows' scales span twelve orders of magnitude
        assert (np.abs(mine[q] - ref[q]) <= 2.0 ** -40 * np.maximum(size, 1e-300)).all(), (name, q)
    p0, grads = U.dense_stream(1025)
    f64, err = U.dense_reference(p0, grads, first_step=7, betas=case.betas)
    q = torch.nn.Parameter(p0.double())
    opt = torch.optim.Adam([q], lr=U.LRS[0], betas=case.betas, eps=U.EPS)
    opt.state[q] = {"step": torch.tensor(6.0), "exp_avg": torch.zeros_like(q), "exp_avg_sq": torch.zeros_like(q)}
    for g in grads:
        q.grad = g.double()
        opt.step()
    assert np.abs(f64["p"] - q.detach().numpy()).max() <= 2.0 ** -40 * np.abs(f64["p"]).max()
    assert all((err[k] > 0).all() for k in U.QUANTITIES)


@pytest.mark.parametrize("case", U.CASES, ids=U.CASE_IDS)
def test_every_defect_model_moves_the_case(case):
    weak = []
    for defect in U.DEFECTS:
        if not U.applies(case, defect):
            continue
        ratio, where = U.defect_move(case, defect)
        print(f"adam-routes-sensitivity {case.name} {defect}: move / tolerance {ratio:.3g} in {where}")
        if ratio < 10:
            weak.append((defect, ratio, where))
    assert not weak, weak


def test_every_defect_model_applies_somewhere():
    for defect in U.DEFECTS:
        assert sum(U.applies(c, defect) for c in U.CASES) >= 3, defect


@pytest.mark.parametrize("case", U.CASES, ids=U.CASE_IDS)
def test_err_ref_is_rarely_the_one_ulp_floor(case):
    """Where torch's float32 result is within one ulp of float64 over a whole row, the tolerance is ERR_FACTOR ulps and says little.
    Among the rows that took a non-zero gradient (every other row holds its initial bits on both sides, deviation zero) that is the
    case for at most a quarter, for p; the reference alone decides this."""
    ref = U.reference(case)
    floored = ref.floored["p"][ref.real]
    print(f"adam-routes-floor {case.name}: {int(floored.sum())} of {len(floored)} rows")
    assert len(floored) >= 20 and floored.mean() <= 0.25
    never = ~ref.real
    assert all((ref.f64[q][never] == 0).all() for q in ("m", "v"))
    assert (ref.f64["p"][never] == U.initial(case)[ref.live[never]].double().numpy()).all()


def test_a_measured_ratio_names_a_group_and_a_quantity():
    groups = {c.group for c in U.CASES} | {"dense", "multi"}
    for (group, quantity), ratio in U.MEASURED_RATIO.items():
        assert group in groups and quantity in U.QUANTITIES and 0 <= ratio
