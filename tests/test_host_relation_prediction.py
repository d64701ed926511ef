"""CPU (-m "not gpu") tests of the relation-prediction term's host part: the C ABI (include/mkb_hip.h, "relation prediction", under
ABI 9) exports mkb_rel_step_workspace_bytes / mkb_rel_score_bwd / mkb_rel_step with the declared signatures and refuses bad
arguments before any launch; losses.RelationPrediction validates its arguments and has no CPU fallback; the five steps and
compose.Pipeline take it; every case of tests/util_relation_prediction.py has a kink-clear batch with the rows the issue asks for;
and the replica the GPU tests compare against agrees with finite differences in float64."""
import ctypes
import inspect
import re
import types

import numpy as np
import pytest
import torch

import util_relation_prediction as up

DECLARED = {
    "mkb_rel_step_workspace_bytes": ("int64_t", ["const mkb_tables_t *tb", "int64_t B"]),
    "mkb_rel_score_bwd": ("int", ["const mkb_tables_t *tb", "const mkb_grads_t *gr", "const int64_t *sample", "int64_t B",
                                  "const float *dscore", "int64_t ld", "void *ws", "int64_t ws_bytes", "void *stream"]),
    "mkb_rel_step": ("int", ["const mkb_tables_t *tb", "const mkb_grads_t *gr", "const int64_t *sample", "const float *weight", "int64_t B",
                             "float temperature", "float lambda", "const float *weight_sum", "float *loss", "float *pos", "void *ws",
                             "int64_t ws_bytes", "void *stream"]),
}


def test_symbols_signatures_and_abi():
    from conftest import ROOT
    from mkb_amd import _hip

    header = (ROOT / "include" / "mkb_hip.h").read_text()
    assert re.search(r"#define MKB_ABI_VERSION 9\b", header) and _hip.ABI_VERSION == 9
    lib = ctypes.CDLL(str(ROOT / "mkb_amd" / "libmkb_hip.so"))
    c = ctypes

    def ctype(param):
        if param == "const mkb_tables_t *tb":
            return c.POINTER(_hip.Tables)
        if param == "const mkb_grads_t *gr":
            return c.POINTER(_hip.Grads)
        return c.c_void_p if "*" in param else {"int64_t": c.c_int64, "int": c.c_int, "float": c.c_float}[param.split()[0]]

    for name, (res, params) in DECLARED.items():
        decl = re.search(r"\b%s %s\(([^)]*)\);" % (res, name), header)
        assert decl, name
        assert [" ".join(a.split()) for a in decl.group(1).split(",")] == params, name
        assert _hip._SIGNATURES[name] == ({"int": c.c_int, "int64_t": c.c_int64}[res], [ctype(p) for p in params]), name
        assert hasattr(lib, name) and name in _hip.EXPORTED_SYMBOLS, name
    assert _hip.lib().mkb_abi_version() == 9


def test_abi_rejects_bad_arguments_before_any_launch():
    """Pointers that are never dereferenced: every call fails validation first, or has B == 0."""
    from mkb_amd import _hip

    lib = _hip.lib()
    p = ctypes.c_void_p(0x10000)
    ids = _hip.MODEL_IDS
    tb = _hip.Tables(ids["RotatE"], 8, 100, 3, 16, 8, p, p, p, 6.0, 1.0)
    protate = _hip.Tables(ids["pRotatE"], 8, 100, 3, 8, 8, p, p, p, 6.0, 1.0)
    bad_model = _hip.Tables(99, 8, 100, 3, 16, 8, p, p, p, 6.0, 1.0)
    bad_dims = _hip.Tables(ids["RotatE"], 8, 100, 3, 8, 8, p, p, p, 6.0, 1.0)
    many = _hip.Tables(ids["TransE"], 8, 1 << 33, 3, 8, 8, p, p, p, 6.0, 1.0)       # n_entity past the int32 sort
    long_rows = _hip.Tables(ids["TransE"], 2800, 100, 3, 2800, 2800, p, p, p, 6.0, 1.0)  # (2 + 4) rows of 2800 floats > 64 KB of LDS
    grads = _hip.Grads(p, p, None)
    B = 4
    need = lib.mkb_rel_step_workspace_bytes(tb, B)
    # the block, dH and dT, one relation partial, the occurrence list four times, the loss scratch
    assert need >= 4 * (B * 3 + 2 * B * 16 + 3 * 8 + 4 * 2 * B + B + 1) and need % 256 == 0
    for args in [(None, B), (tb, 0), (tb, -1), (tb, 1 << 31), (tb, 1 << 40), (many, B)]:
        assert lib.mkb_rel_step_workspace_bytes(*args) == 0, args[1:]
    ws = ctypes.c_void_p(0x100000)  # 256-byte aligned
    inf, nan = float("inf"), float("nan")

    def step(tb=tb, gr=grads, sample=p, weight=None, B=B, T=0.5, lam=0.25, weight_sum=None, loss=p, pos=p, ws=ws, ws_bytes=need):
        return lib.mkb_rel_step(tb, gr, sample, weight, B, T, lam, weight_sum, loss, pos, ws, ws_bytes, None)

    def bwd(tb=tb, gr=grads, sample=p, B=B, dscore=p, ld=3, ws=ws, ws_bytes=need):
        return lib.mkb_rel_score_bwd(tb, gr, sample, B, dscore, ld, ws, ws_bytes, None)

    common = [dict(tb=None), dict(tb=bad_model), dict(tb=bad_dims), dict(tb=many), dict(gr=None), dict(gr=_hip.Grads(None, p, None)),
              dict(gr=_hip.Grads(p, None, None)), dict(tb=protate), dict(sample=None), dict(B=-1), dict(B=1 << 31), dict(B=1 << 40),
              dict(ws=None), dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws=ctypes.c_void_p(0x100010))]
    for kw in common + [dict(loss=None), dict(pos=None), dict(T=0.0), dict(T=-1.0), dict(T=inf), dict(T=nan), dict(lam=0.0),
                        dict(lam=-0.25), dict(lam=inf), dict(lam=nan)]:
        assert step(**kw) == _hip.ERR_INVALID, kw
        assert lib.mkb_last_error(), kw
    for kw in common + [dict(dscore=None), dict(ld=2), dict(ld=0), dict(ld=-3), dict(ld=1 << 31)]:
        assert bwd(**kw) == _hip.ERR_INVALID, kw
        assert lib.mkb_last_error(), kw
    assert step(tb=long_rows) == _hip.ERR_UNSUPPORTED and bwd(tb=long_rows, ld=3) == _hip.ERR_UNSUPPORTED
    assert step(tb=long_rows, B=0) == _hip.ERR_UNSUPPORTED
    # valid calls that launch nothing
    assert step(B=0) == 0 and step(B=0, ws=None, ws_bytes=0) == 0 and bwd(B=0) == 0 and bwd(B=0, ws=None, ws_bytes=0) == 0
    # pRotatE with a modulus gradient passes the pointer checks (and stops at the workspace)
    assert step(tb=protate, gr=_hip.Grads(p, p, p), ws_bytes=0) == _hip.ERR_INVALID
    assert "workspace" in lib.mkb_last_error().decode()


def test_class_is_public_validates_its_arguments_and_refuses_cpu_tensors():
    import mkb_amd
    from mkb_amd import losses, models

    assert "RelationPrediction" in losses.__all__ and mkb_amd.losses.RelationPrediction is losses.RelationPrediction
    term = losses.RelationPrediction()
    assert (term.weight, term.temperature) == (1.0, 1.0)
    term = losses.RelationPrediction(0.25, temperature=0.5)
    assert (term.weight, term.temperature) == (0.25, 0.5)
    assert repr(term) == "RelationPrediction(weight=0.25, temperature=0.5)"
    for bad in (0.0, -0.25, float("inf"), float("nan"), "x"):
        with pytest.raises(ValueError):
            losses.RelationPrediction(bad)
        with pytest.raises(ValueError):
            losses.RelationPrediction(0.25, temperature=bad)
    m = models.ComplEx(hidden_dim=4, entities={0: 0, 1: 1}, relations={0: 0}, gamma=1)
    sample = torch.tensor([[0, 0, 1]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        term(m, sample)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        term.launch(m, sample, torch.ones(1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.score_relations(sample)
    assert list(inspect.signature(term.launch).parameters) == ["model", "sample", "weight", "weight_sum", "grads"]
    assert list(inspect.signature(term.__call__).parameters) == ["model", "sample", "weight", "weight_sum"]


def test_step_classes_take_the_term():
    from mkb_amd import fused, losses, models

    te = models.TransE(hidden_dim=4, entities={0: 0, 1: 1}, relations={0: 0}, gamma=1)
    cx = models.ComplEx(hidden_dim=4, entities={0: 0, 1: 1}, relations={0: 0}, gamma=1)
    term = losses.RelationPrediction(0.25)
    triples = [(0, 0, 1)]
    make = [lambda **kw: fused.FusedTrainStep(te, 1.0, **kw), lambda **kw: fused.PooledLossStep(te, losses.CrossEntropy(), **kw),
            lambda **kw: fused.OneVsAllStep(cx, **kw), lambda **kw: fused.KvsAllStep(cx, triples, **kw),
            lambda **kw: fused.DistanceAllStep(te, losses.OneVsAll(), **kw)]
    for f in make:
        step = f()
        assert step.relation_prediction is None and step.relation_prediction_loss is None and step.regularizer is None
        step = f(relation_prediction=term)
        assert step.relation_prediction is term and step.relation_prediction_loss is None and step.regularizer is None


def test_pipeline_hands_the_term_to_each_kind_of_step(monkeypatch):
    from mkb_amd import compose, fused, losses, models, sampling
    from mkb_amd.compose import pipeline as pipeline_module
    from mkb_amd.models.base import BaseModel

    pipe = compose.Pipeline(epochs=1)
    assert pipe.relation_prediction is None
    term = pipe.relation_prediction = losses.RelationPrediction(0.25)
    dataset = types.SimpleNamespace(train=[(0, 0, 1)], batch_size=4)
    te = models.TransE(hidden_dim=4, entities={0: 0, 1: 1}, relations={0: 0}, gamma=1)
    cx = models.ComplEx(hidden_dim=4, entities={0: 0, 1: 1}, relations={0: 0}, gamma=1)
    opt = types.SimpleNamespace()
    wanted = [(te, losses.OneVsAll(), fused.DistanceAllStep), (te, losses.KvsAll(), fused.DistanceAllStep), (cx, losses.OneVsAll(), fused.OneVsAllStep),
              (cx, losses.KvsAll(), fused.KvsAllStep)]
    for model, loss, kind in wanted:
        step = pipe._fused_step_for(model, dataset, None, opt, loss)
        assert type(step) is kind and step.relation_prediction is term and step.regularizer is None
    # the two pooled steps want a device model the pooled kernels cover: a stand-in that says so
    monkeypatch.setattr(pipeline_module, "pooled_supported", lambda *a: True)

    class OnDevice(BaseModel):
        def __init__(self):  # (no tables: the step classes only keep the model)
            pass

    stand_in = OnDevice.__new__(OnDevice)
    stand_in.__dict__["entity_embedding"] = types.SimpleNamespace(is_cuda=True)
    sampler = sampling.NegativeSampling.__new__(sampling.NegativeSampling)
    sampler.size = 4
    for loss, kind in ((losses.Adversarial(alpha=0.5), fused.FusedTrainStep), (losses.CrossEntropy(), fused.PooledLossStep)):
        step = pipe._fused_step_for(stand_in, dataset, sampler, opt, loss)
        assert type(step) is kind and step.relation_prediction is term and step.regularizer is None
    # ... and the explicit sequence adds term(model, sample, weight) to the loss
    assert "self.relation_prediction(model, sample, weight)" in inspect.getsource(compose.Pipeline._run_epoch)


@pytest.mark.parametrize("case", up.CASES, ids=up.CASE_IDS)
def test_every_case_has_a_kink_clear_batch_with_the_rows_the_shapes_need(case):
    pb = up.problem(case)
    assert up.kink_clear(pb)
    de, dr = up.dims(pb.model, pb.hidden)
    assert pb.ent.shape == (up.N, de) and pb.rel.shape == (pb.R, dr) and pb.sample.shape == (pb.B, 3)
    s = pb.sample
    assert s[:, 1].min() >= 0 and s[:, 1].max() < pb.R and s[:, [0, 2]].max() < up.N
    if pb.B >= 7:
        assert (s[:, 0] == s[:, 2]).any()                                     # a row with h == t
        assert len(np.intersect1d(s[:, 0], s[:, 2])) > 0                      # an entity that is a head here and a tail there
        assert len(np.unique(s, axis=0)) < pb.B                               # two identical rows
        assert (s[:, 1] == 0).any() and (s[:, 1] == pb.R - 1).any()           # the first and the last relation as targets
        assert len(np.unique(s[:, [0, 2]])) < 2 * pb.B                        # entities repeat


def test_case_table_covers_the_shapes():
    hidden, R, B = ({c[k] for c in up.CASES} for k in (2, 3, 4))
    assert {4, 37, 130, 300} <= hidden and {1, 3, 5, 37, 130} <= R and {1, 7, 37, 130} <= B
    assert {c[0] for c in up.CASES} == set(up.MODELS) and len(up.MODELS) == 5
    assert up.ERR_FACTOR == 8.0
    for (name, quantity), (ratio, cause) in up.MEASURED_RATIO.items():
        assert name in up.CASE_IDS and quantity in up.QUANTITIES and ratio > up.ERR_FACTOR and cause


@pytest.mark.parametrize("model", up.MODELS)
@pytest.mark.parametrize("mode", ["term", "block"])
def test_replica_gradients_agree_with_finite_differences(model, mode):
    """The float64 replica's autograd against central differences of its own value on the smallest case, for entries of both tables
    that the batch uses and for pRotatE's modulus: step 1e-7 (inside the kink margin of 2 float32 ulps of the largest argument),
    truncation ~1e-14, rounding ~1e-16 / 1e-7 = 1e-9 of the value."""
    case = (model,) + up.SMALLEST
    pb = up.problem(case)
    kw = dict(dblock=up.seed_block(pb)) if mode == "block" else dict(weighted=True, weight_sum=9.5)
    ref = up.replica(pb, torch.float64, **kw)
    eps = 1e-7

    def value(ent, rel, modulus=pb.modulus):
        return float(up.replica(pb._replace(modulus=modulus), torch.float64, tables=(ent, rel), **kw)["loss"])

    rs = np.random.RandomState(5)
    used = np.unique(pb.sample[:, [0, 2]])
    checked = 0
    for which, table, grad in (("ent", pb.ent.astype(np.float64), ref["g_ent"]), ("rel", pb.rel.astype(np.float64), ref["g_rel"])):
        for _ in range(6):
            row = int(rs.choice(used)) if which == "ent" else int(rs.randint(pb.R))
            col = int(rs.randint(table.shape[1]))
            hi, lo = table.copy(), table.copy()
            hi[row, col] += eps
            lo[row, col] -= eps
            other = pb.rel.astype(np.float64) if which == "ent" else pb.ent.astype(np.float64)
            fd = ((value(hi, other) - value(lo, other)) if which == "ent" else (value(other, hi) - value(other, lo))) / (2 * eps)
            assert abs(fd - grad[row, col]) <= 1e-7 * max(1.0, abs(fd)), (which, row, col, fd, grad[row, col])
            checked += abs(fd) > 1e-6
    assert checked >= 6
    # rows outside the batch take no gradient
    outside = np.setdiff1d(np.arange(up.N), used)
    assert len(outside) and not ref["g_ent"][outside].any()
    if model == "pRotatE":
        ent, rel = pb.ent.astype(np.float64), pb.rel.astype(np.float64)
        fd = (value(ent, rel, pb.modulus + eps) - value(ent, rel, pb.modulus - eps)) / (2 * eps)
        assert abs(fd - float(ref["g_mod"].reshape(-1)[0])) <= 1e-7 * max(1.0, abs(fd)) and abs(fd) > 1e-6
    else:
        assert ref["g_mod"] is None
