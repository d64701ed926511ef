"""CPU (-m "not gpu") tests of the 1vsAll training step's host part: the C ABI (include/mkb_hip.h, "1vsAll", under ABI 8) exports
mkb_all_step_workspace_bytes / mkb_all_score_fwd / mkb_all_softmax / mkb_all_score_bwd / mkb_all_step with the declared signatures
and refuses bad arguments before any launch; the Python surface (losses.OneVsAll, fused.OneVsAllStep, model.score_all) checks its
arguments, refuses the distance models and has no CPU fallback; and the case table of the GPU tests (tests/util_onevsall.py) really
selects the kernel families it claims: a host program built on the planner's own headers (gemm_plan.h, all_plan.h) is asked."""
import os
import pathlib
import re
import subprocess

import pytest
import torch

import util_onevsall as U

ROOT = pathlib.Path(__file__).resolve().parent.parent
SYMBOLS = ("mkb_all_step_workspace_bytes", "mkb_all_score_fwd", "mkb_all_softmax", "mkb_all_score_bwd", "mkb_all_step")


def _tables(model="ComplEx", hidden=8, n_entity=129, n_relation=3, ent=0x40000000):
    from mkb_amd import _hip

    de = 2 * hidden if model in ("RotatE", "ComplEx") else hidden
    dr = 2 * hidden if model == "ComplEx" else hidden
    return _hip.Tables(_hip.MODEL_IDS[model], hidden, n_entity, n_relation, de, dr, ent, 0x50000000, 0x50100000, 6.0, 0.5)


def test_symbols_are_declared_exported_and_bound_under_abi_8():
    from mkb_amd import _hip

    header = (ROOT / "include" / "mkb_hip.h").read_text()
    assert re.search(r"#define\s+MKB_ABI_VERSION\s+9\b", header) and _hip.ABI_VERSION == 9
    lib = _hip.lib()
    assert lib.mkb_abi_version() == 9
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _hip.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _hip._SIGNATURES[name][1]
    # the header's parameter counts are the binding's
    for name in SYMBOLS:
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, header, re.S).group(1)
        assert len(decl.split(",")) == len(_hip._SIGNATURES[name][1]), name


def test_names_are_public():
    import mkb_amd
    from mkb_amd import fused, losses

    assert "OneVsAll" in losses.__all__ and callable(losses.OneVsAll)
    assert "OneVsAllStep" in fused.__all__ and callable(fused.OneVsAllStep)
    assert callable(mkb_amd.models.ComplEx.score_all)
    assert repr(losses.OneVsAll(2.0)) == "OneVsAll(temperature=2.0)"


def _model(name, hidden=4, N=9):
    from mkb_amd import models

    return getattr(models, name)(hidden_dim=hidden, entities={i: i for i in range(N)}, relations={i: i for i in range(2)}, gamma=6.0)


@pytest.mark.parametrize("T", [0.0, -1.0, float("nan"), float("inf")])
def test_bad_temperature_is_refused(T):
    from mkb_amd import fused, losses

    with pytest.raises(ValueError):
        losses.OneVsAll(T)
    with pytest.raises(ValueError):
        fused.OneVsAllStep(_model("DistMult"), temperature=T)


@pytest.mark.parametrize("name", ["TransE", "RotatE", "pRotatE"])
def test_distance_models_are_refused_with_the_alternative_named(name):
    from mkb_amd import fused

    m = _model(name)
    with pytest.raises(NotImplementedError, match=r"losses\.CrossEntropy"):
        fused.OneVsAllStep(m)
    with pytest.raises(NotImplementedError, match=r"with_scores=True"):
        m.score_all(torch.zeros((2, 3), dtype=torch.int64), "tail-batch")


def test_there_is_no_cpu_fallback():
    from mkb_amd import fused, losses

    m = _model("ComplEx")
    sample = torch.zeros((2, 3), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.score_all(sample, "tail-batch")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fused.OneVsAllStep(m)(sample, None, "tail-batch")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        losses.OneVsAll()(torch.zeros(2, 9), torch.zeros(2, dtype=torch.int64))


def test_wrong_shapes_and_modes_are_refused():
    from mkb_amd import fused

    step = fused.OneVsAllStep(_model("DistMult"))
    good = torch.zeros((2, 3), dtype=torch.int64)
    with pytest.raises(ValueError, match="head-batch"):
        step(good, None, None)
    with pytest.raises(ValueError, match=r"\[B, 3\]"):
        step(torch.zeros((2, 4), dtype=torch.int64), None, "tail-batch")
    with pytest.raises(ValueError, match=r"\[B, 3\]"):
        step(torch.zeros((0, 3), dtype=torch.int64), None, "tail-batch")
    with pytest.raises(ValueError, match="weight"):
        step(good, torch.ones(3), "tail-batch")
    with pytest.raises(ValueError, match="head-batch"):
        _model("DistMult").score_all(good, "default")


class _FakeDevice(torch.Tensor):
    """A CPU tensor that says it is on the device: the shape checks behind require_device are reached without one."""

    @property
    def is_cuda(self):
        return True


def test_the_loss_checks_its_shapes():
    from mkb_amd import losses

    fake = lambda t: t.as_subclass(_FakeDevice)
    loss = losses.OneVsAll()
    with pytest.raises(ValueError, match=r"\[B, N\]"):
        loss(fake(torch.zeros(4)), fake(torch.zeros(4, dtype=torch.int64)))
    with pytest.raises(ValueError, match="target"):
        loss(fake(torch.zeros(4, 5)), fake(torch.zeros(3, dtype=torch.int64)))
    with pytest.raises(ValueError, match="target"):
        loss(fake(torch.zeros(4, 5)), fake(torch.zeros(4, dtype=torch.int32)))
    with pytest.raises(ValueError, match="weight"):
        loss(fake(torch.zeros(4, 5)), fake(torch.zeros(4, dtype=torch.int64)), fake(torch.ones(5)))


def test_invalid_c_arguments_are_refused_before_any_launch():
    """Every call below would fault (the pointers are made up) or fail with MKB_ERR_HIP (no device here) if it got as far as a launch."""
    from mkb_amd import _hip

    lib, P = _hip.lib(), 0x60000000  # (256-byte aligned, never dereferenced)
    tb = _tables()
    n = lib.mkb_all_step_workspace_bytes(tb, 32)
    gr = _hip.Grads(P, P, None)
    soft = lambda **kw: lib.mkb_all_softmax(*[kw.get(k, d) for k, d in (("S", P), ("B", 4), ("N", 9), ("ld", 12), ("target", P), ("stride", 1),
                                                                         ("weight", None), ("wsum", None), ("T", 1.0), ("loss", P),
                                                                         ("pos", P), ("scratch", P), ("stream", None))])
    for bad in (dict(S=None), dict(target=None), dict(loss=None), dict(pos=None), dict(scratch=None), dict(T=0.0), dict(T=-2.0),
                dict(T=float("nan")), dict(T=float("inf")), dict(B=0), dict(B=-1), dict(N=0), dict(ld=8), dict(stride=0),
                dict(B=1 << 16, N=1 << 15, ld=1 << 15)):  # B * ld = 2^31
        assert soft(**bad) == _hip.ERR_INVALID, bad
        assert lib.mkb_last_error()
    step = lambda tb_=tb, gr_=gr, sample=P, B=32, mode=_hip.MODE_TAIL, T=1.0, loss=P, pos=P, ws=P, nb=n: lib.mkb_all_step(
        tb_, gr_, sample, None, B, mode, T, None, loss, pos, ws, nb, None)
    for bad in (dict(tb_=None), dict(gr_=None), dict(gr_=_hip.Grads(None, P, None)), dict(gr_=_hip.Grads(P, None, None)), dict(sample=None),
                dict(B=0), dict(mode=_hip.MODE_DEFAULT), dict(T=0.0), dict(T=float("nan")), dict(loss=None), dict(pos=None), dict(ws=None),
                dict(nb=n - 1), dict(ws=P + 16), dict(B=1 << 25)):
        assert step(**bad) == _hip.ERR_INVALID, bad
    assert lib.mkb_all_score_fwd(tb, P, 32, _hip.MODE_TAIL, None, P, n, None) == _hip.ERR_INVALID
    assert lib.mkb_all_score_fwd(tb, P, 32, _hip.MODE_DEFAULT, P, P, n, None) == _hip.ERR_INVALID
    assert lib.mkb_all_score_bwd(tb, gr, P, 32, _hip.MODE_TAIL, None, 132, P, n, None) == _hip.ERR_INVALID
    assert lib.mkb_all_score_bwd(tb, gr, P, 32, _hip.MODE_TAIL, P, 128, P, n, None) == _hip.ERR_INVALID  # ld < n_entity
    for name in ("TransE", "RotatE", "pRotatE"):  # another model: unsupported, and the message names the alternative
        other = _tables(name)
        assert step(tb_=other) == _hip.ERR_UNSUPPORTED, name
        assert b"losses.CrossEntropy" in lib.mkb_last_error()
        assert lib.mkb_all_step_workspace_bytes(other, 32) == 0


def test_workspace_is_positive_and_monotone_in_the_batch():
    from mkb_amd import _hip

    lib = _hip.lib()
    for model, hidden, N in (("ComplEx", 8, 129), ("DistMult", 37, 129), ("ComplEx", 500, 14541), ("DistMult", 768, 1537)):
        tb = _tables(model, hidden, N)
        # (batches of a few hundred rows at most: the radix sort's size query answers larger ones only with a device present)
        sizes = [lib.mkb_all_step_workspace_bytes(tb, B) for B in (1, 2, 7, 32, 37, 128, 256)]
        assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1], (model, sizes)
        assert all(s % 256 == 0 for s in sizes)
        # it holds at least Q, the padded score block, the id list and dQ
        de = 2 * hidden if model == "ComplEx" else hidden
        assert sizes[-1] >= 256 * de * 8 + 256 * ((N + 3) & ~3) * 4 + N * 8
    assert lib.mkb_all_step_workspace_bytes(_tables(), 0) == 0 and lib.mkb_all_step_workspace_bytes(None, 8) == 0
    assert lib.mkb_all_step_workspace_bytes(_tables(n_entity=14541), 1 << 20) == 0  # B * Npad past 2^31: the calls refuse it


PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include "all_plan.h"
using namespace mkb;
static const char *family(const GemmPlan &p) {
    return p.kernel == GemmKernel::Bf16x3Tile128 ? "bf16x3" : p.kernel == GemmKernel::F32Tile128 ? "f32tile128" : "f32tile64";
}
int main(int argc, char **argv) {  // B N De bf16x3 -> "forward dQ dE  ks of each  whether dQ's K runs over the padded id list"
    const int64_t B = atoll(argv[1]), N = atoll(argv[2]), De = atoll(argv[3]);
    const GemmSwitches sw{false, false, atoi(argv[4]) != 0};
    const bool gemm = all_fwd_on_gemm(B, N, De, true, true);
    const GemmPlan f = plan_gemm(all_fwd_shape(B, N, De), all_fwd_limits(), sw);
    const int64_t ld = gemm ? all_npad(N) : N;  // what the forward's route leaves behind (run_rank)
    const GemmPlan q = plan_gemm(all_dq_shape(B, N, De, ld, ld > N, true), all_dq_limits(), sw);
    const GemmPlan e = plan_gemm(all_de_shape(B, N, De, ld, true), all_de_limits(N, De), sw);
    printf("%s %s %s %d %d %d %d %zu %zu\n", gemm ? family(f) : "lane", family(q), family(e), gemm ? f.ks : 0, q.ks, e.ks, (int)(ld > N),
           q.lds, e.lds);
    return 0;
}
"""


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    d = tmp_path_factory.mktemp("all_plan")
    (d / "main.cc").write_text(PROGRAM)
    exe = d / "all_plan"
    subprocess.run([os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-I", str(ROOT / "mkb_amd" / "csrc"), str(d / "main.cc"), "-o", str(exe)],
                   check=True, capture_output=True)

    def ask(B, N, De, bf16x3=1):
        out = subprocess.run([str(exe), str(B), str(N), str(De), str(bf16x3)], check=True, capture_output=True, text=True).stdout.split()
        return tuple(out[:3]), [int(x) for x in out[3:]]

    return ask


@pytest.mark.parametrize("case", U.CASES, ids=U.CASE_IDS)
def test_the_case_table_selects_the_kernel_families_it_claims(planner, case):
    name, model, hidden, B, N, claim = case
    families, (ks_f, ks_q, ks_e, gathered, lds_q, lds_e) = planner(B, N, U.entity_dim(model, hidden))
    assert families == claim, (name, families)
    assert ks_f <= 1  # the forward is never split
    if name.startswith("bf16x3"):
        assert ks_e == 2 and gathered == 1  # the accumulating product goes through partials here; dQ runs over the padded id list
    if name.startswith("long"):
        assert N > U.STAGE_COLS and ks_q > 1


def test_the_table_covers_every_family_each_product_can_take(planner):
    seen = [set(), set(), set()]
    for case in U.CASES:
        for s, f in zip(seen, case[5]):
            s.add(f)
    assert seen[0] == {"lane", "f32tile64", "bf16x3"} and seen[1] == seen[2] == {"f32tile64", "bf16x3"}
    assert {c[4] % 4 for c in U.CASES} >= {1, 2, 3}  # every pad width of the forward's id list


def test_the_headline_shape_and_a_large_graph_stay_launchable(planner):
    """FB15k-237 (14,541 entities, hidden 1000, B = 1024): the three products on the 128-row bf16x3 tiles, dE unsplit (the epilogue
    itself accumulates).  A graph of a million entities: the row ids of dQ's K range do not fit the LDS, the planner falls back to
    the 64-row tiles instead of planning a launch that cannot start."""
    for de in (1000, 2000):
        families, (_, ks_q, ks_e, _, lds_q, lds_e) = planner(1024, 14541, de)
        assert families == ("bf16x3",) * 3 and ks_e == 1 and max(lds_q, lds_e) <= 160 * 1024
    families, (_, _, _, _, lds_q, lds_e) = planner(1024, 1000001, 1000)
    assert families[1] == "f32tile64" and max(lds_q, lds_e) <= 160 * 1024
    # without the bf16 split an entity count that is no multiple of 4 cannot keep the 128-row fp32 tiles for dE (float4 along m)
    assert planner(512, 1537, 768, bf16x3=0)[0][2] == "f32tile64"
    assert planner(512, 1540, 768, bf16x3=0)[0][2] == "f32tile128"
