"""CPU (-m "not gpu") tests of the embedding regularisers' host part: the C ABI (include/mkb_hip.h, "embedding regularisers", under
ABI 8) exports mkb_reg_rows_workspace_bytes / mkb_reg_rows with the declared signatures and refuses bad arguments before any launch;
mkb_amd.regularizers validates its arguments and has no CPU fallback; the step classes take ``regularizer=None``; and the float64
reference the GPU tests compare against (tests/util_regularizers.py) agrees with torch's float64 autograd and with hand-computed
values."""
import ctypes
import re

import numpy as np
import pytest
import torch

import util_regularizers as ur

DECLARED = {
    "mkb_reg_rows_workspace_bytes": ("int64_t", ["const mkb_tables_t *tb", "int64_t B"]),
    "mkb_reg_rows": ("int", ["const mkb_tables_t *tb", "const mkb_grads_t *gr", "const int64_t *sample", "const float *weight", "int64_t B",
                             "int p", "float lambda_ent", "float lambda_rel", "const float *weight_sum", "const float *scale",
                             "float *value", "void *ws", "int64_t ws_bytes", "void *stream"]),
}


def test_regulariser_symbols_signatures_and_abi():
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


def test_regulariser_abi_rejects_bad_arguments_before_any_launch():
    """Pointers that are never dereferenced: every call fails validation first (or has B == 0, with no value to write)."""
    from mkb_amd import _hip

    lib = _hip.lib()
    p = ctypes.c_void_p(0x10000)
    tb = _hip.Tables(_hip.MODEL_IDS["RotatE"], 8, 100, 3, 16, 8, p, p, p, 6.0, 1.0)
    bad_model = _hip.Tables(99, 8, 100, 3, 16, 8, p, p, p, 6.0, 1.0)
    huge = _hip.Tables(_hip.MODEL_IDS["TransE"], 8, (1 << 31) - 2, 3, 8, 8, p, p, p, 6.0, 1.0)  # n_entity + n_relation > 2^31 - 1
    grads = _hip.Grads(p, p, None)
    B = 4
    need = lib.mkb_reg_rows_workspace_bytes(tb, B)
    assert need >= 4 * 3 * B * 4 + 3 * B * 4 and need % 256 == 0  # the occurrence list twice (keys, values) and the value slots
    for args in [(None, B), (tb, 0), (tb, -1), (tb, 1 << 30), (tb, 1 << 40), (huge, B)]:
        assert lib.mkb_reg_rows_workspace_bytes(*args) == 0, args[1:]
    ws = ctypes.c_void_p(0x100000)  # 256-byte aligned
    inf, nan = float("inf"), float("nan")

    def call(tb=tb, gr=grads, sample=p, weight=None, B=B, p_=3, le=0.1, lr=0.1, weight_sum=None, scale=None, value=p, ws=ws, ws_bytes=need):
        return lib.mkb_reg_rows(tb, gr, sample, weight, B, p_, le, lr, weight_sum, scale, value, ws, ws_bytes, None)

    for kw in [dict(p_=1), dict(p_=4), dict(p_=0), dict(p_=-3), dict(le=-0.1), dict(lr=-1e-9), dict(le=inf), dict(lr=inf), dict(le=nan),
               dict(lr=nan), dict(tb=None), dict(tb=bad_model), dict(tb=huge), dict(sample=None), dict(gr=None, value=None), dict(B=-1),
               dict(B=1 << 30), dict(B=1 << 40), dict(ws=None), dict(ws_bytes=need - 1), dict(ws_bytes=0),
               dict(ws=ctypes.c_void_p(0x100010)), dict(gr=_hip.Grads(None, p, None)), dict(gr=_hip.Grads(p, None, None))]:
        assert call(**kw) == _hip.ERR_INVALID, kw
        assert lib.mkb_last_error(), kw
    # a valid call that launches nothing (gradient only: there is no value to write either)
    assert call(B=0, value=None) == 0 and call(B=0, value=None, ws=None, ws_bytes=0) == 0
    # a table whose weight is 0 is not touched: its gradient buffer may be missing -- but the call still needs a workspace
    assert call(gr=_hip.Grads(None, p, None), le=0.0, ws_bytes=0) == _hip.ERR_INVALID


def test_classes_validate_their_arguments_and_refuse_cpu_tensors():
    import mkb_amd
    from mkb_amd import models, regularizers

    assert mkb_amd.regularizers is regularizers and set(regularizers.__all__) == {"Lp", "N3", "L2"}
    n3, l2, lp = regularizers.N3(0.25), regularizers.L2(0.5), regularizers.Lp()
    assert (n3.p, n3.entity_weight, n3.relation_weight) == (3, 0.25, 0.25)
    assert (l2.p, l2.entity_weight, l2.relation_weight) == (2, 0.5, 0.5)
    assert (lp.p, lp.entity_weight, lp.relation_weight) == (3, 0.0, 0.0)
    assert isinstance(n3, regularizers.Lp) and isinstance(l2, regularizers.Lp)
    for bad in [dict(p=1), dict(p=4), dict(p=2.5), dict(p="3"), dict(p=True), dict(entity_weight=-1.0), dict(relation_weight=-1e-9),
                dict(entity_weight=float("inf")), dict(relation_weight=float("nan")), dict(entity_weight="0.1"), dict(entity_weight=None)]:
        with pytest.raises(ValueError):
            regularizers.Lp(**bad)
    for cls in (regularizers.N3, regularizers.L2):
        for bad in (-0.5, float("nan"), float("inf"), "x"):
            with pytest.raises(ValueError):
                cls(bad)
    m = models.ComplEx(hidden_dim=4, entities={0: 0, 1: 1}, relations={0: 0}, gamma=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        n3(m, torch.tensor([[0, 0, 1]]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        n3.launch(m, torch.tensor([[0, 0, 1]]), torch.ones(1))


def test_step_classes_take_a_regulariser():
    import inspect

    from mkb_amd import compose, fused, losses, models, parallel, regularizers, table_rows

    m = models.TransE(hidden_dim=4, entities={0: 0, 1: 1}, relations={0: 0}, gamma=1)
    n3 = regularizers.N3(0.1)
    for step in (fused.FusedTrainStep(m, 1.0), fused.FusedTrainStep(m, 1.0, regularizer=None), fused.FusedTrainStep(m, 1.0, None),
                 fused.PooledLossStep(m, losses.CrossEntropy()), fused.PooledLossStep(m, losses.CrossEntropy(), regularizer=None)):
        assert step.regularizer is None and step.regularization is None
    assert fused.FusedTrainStep(m, 1.0, regularizer=n3).regularizer is n3
    assert fused.PooledLossStep(m, losses.MarginRanking(), n3).regularizer is n3
    pipe = compose.Pipeline(epochs=1)
    assert pipe.regularizer is None
    assert list(inspect.signature(pipe.learn).parameters) == ["model", "dataset", "sampling", "optimizer", "loss", "evaluation"]
    # the sharded steps are out of scope: they say so before touching anything else
    with pytest.raises(NotImplementedError):
        parallel.DimShardedStep(None, 1.0, regularizer=n3)
    with pytest.raises(NotImplementedError):
        table_rows.TableRowShardedStep(None, None, 1.0, regularizer=n3)


def _torch_expression(name, ent, rel, sample, p, le, lr, w, W):
    """The penalty as a user writes it in torch (float64), for autograd."""
    pe, pr = ur.PAIRED[name]

    def f(rows, paired):
        if not paired:
            return (rows.abs() ** p).sum(1)
        d = rows.shape[1] // 2
        m2 = rows[:, :d] ** 2 + rows[:, d:] ** 2
        return (m2 ** 1.5).sum(1) if p == 3 else m2.sum(1)  # (m2 ** 1.5: a finite derivative at m2 = 0, unlike sqrt(m2) ** 3)

    per_row = le * (f(ent[sample[:, 0]], pe) + f(ent[sample[:, 2]], pe)) + lr * f(rel[sample[:, 1]], pr)
    return (w / W * per_row).sum()


@pytest.mark.parametrize("p", [2, 3])
@pytest.mark.parametrize("name", ["TransE", "RotatE", "ComplEx"])
@pytest.mark.parametrize("weighted", [False, True])
def test_reference_agrees_with_torch_float64_autograd(name, p, weighted):
    g = torch.Generator().manual_seed(7 + p)
    N, R, d, B = 9, 3, 5, 14
    de, dr = ur.DIMS[name]
    ent = (torch.rand(N, de * d, generator=g, dtype=torch.float64) - 0.5).requires_grad_()
    rel = (torch.rand(R, dr * d, generator=g, dtype=torch.float64) - 0.5).requires_grad_()
    with torch.no_grad():
        ent[2] = 0.0  # a row of exact zeros that the batch uses
    sample = torch.stack([torch.randint(N, (B,), generator=g), torch.randint(R, (B,), generator=g), torch.randint(N, (B,), generator=g)], 1)
    sample[0, 0] = 2
    sample[3, 2] = sample[3, 0]  # h == t
    w = torch.rand(B, generator=g, dtype=torch.float64) + 0.1 if weighted else torch.ones(B, dtype=torch.float64)
    W = 3.7 if weighted else float(B)
    le, lr = 0.3, 0.7
    want = _torch_expression(name, ent, rel, sample, p, le, lr, w, W)
    want.backward()
    reg, g_ent, g_rel = ur.reference(name, ent.detach().numpy(), rel.detach().numpy(), sample.numpy(), p, le, lr,
                                     w.numpy() if weighted else None, W if weighted else None)
    np.testing.assert_allclose(reg, float(want.detach()), rtol=1e-13)
    np.testing.assert_allclose(g_ent, ent.grad.numpy(), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(g_rel, rel.grad.numpy(), rtol=1e-12, atol=1e-15)
    assert not g_ent[2].any() and not np.isnan(g_ent).any()  # (the zero row: gradient exactly 0 for either p)


def test_reference_agrees_with_hand_computed_values():
    """Two triples that share their head; h == t in the second.  Real table, p = 3: f(x) = sum |x|^3; paired, p = 3: f = sum m^3."""
    ent = np.array([[1.0, -2.0], [3.0, 4.0], [0.0, 0.0]])
    rel = np.array([[2.0, -1.0]])
    sample = np.array([[0, 0, 1], [0, 0, 0]])
    w, le, lr = np.array([1.0, 3.0]), 0.5, 2.0
    # real: f(E0) = 1 + 8 = 9, f(E1) = 27 + 64 = 91, f(R0) = 8 + 1 = 9;  W = 4
    reg, g_ent, g_rel = ur.reference("TransE", ent, rel, sample, 3, le, lr, w)
    want = 0.25 * (le * (9 + 91) + lr * 9) + 0.75 * (le * (9 + 9) + lr * 9)
    assert abs(reg - want) < 1e-12 and want == 37.25
    # E0 occurs with coefficient 1/4 + 2 * 3/4 = 7/4, E1 with 1/4, R0 with 1; f'(x) = 3 x |x|
    np.testing.assert_allclose(g_ent, [[le * 1.75 * 3.0, -le * 1.75 * 12.0], [le * 0.25 * 27.0, le * 0.25 * 48.0], [0.0, 0.0]], rtol=1e-14)
    np.testing.assert_allclose(g_rel, [[lr * 12.0, -lr * 3.0]], rtol=1e-14)
    # paired (ComplEx, hidden_dim 1): m(E0) = sqrt 5, m(E1) = 5, m(R0) = sqrt 5; f = m^3, f' = 3 m (re, im)
    reg, g_ent, g_rel = ur.reference("ComplEx", ent, rel, sample, 3, le, lr, w)
    f0, f1 = 5.0 ** 1.5, 125.0
    want = 0.25 * (le * (f0 + f1) + lr * f0) + 0.75 * (le * 2 * f0 + lr * f0)
    assert abs(reg - want) < 1e-12
    s5 = 5.0 ** 0.5
    np.testing.assert_allclose(g_ent, [[le * 1.75 * 3 * s5 * 1.0, -le * 1.75 * 3 * s5 * 2.0], [le * 0.25 * 15 * 3.0, le * 0.25 * 15 * 4.0], [0, 0]], rtol=1e-14)
    np.testing.assert_allclose(g_rel, [[lr * 3 * s5 * 2.0, -lr * 3 * s5 * 1.0]], rtol=1e-14)
    # RotatE pairs the entity table only: the relation row keeps the real form
    _, _, g_rel = ur.reference("RotatE", ent, np.array([[2.0]]), sample, 3, le, lr, w)
    np.testing.assert_allclose(g_rel, [[lr * 12.0]], rtol=1e-14)
    # a zero row, p = 3, paired: exactly 0, no NaN
    f, df = ur.row_term(np.zeros(4), 3, True)
    assert f == 0.0 and not df.any() and not np.isnan(df).any()
    # p = 2: the paired and the real form are the same sum
    a = ur.reference("ComplEx", ent, rel, sample, 2, le, lr, w)
    b = ur.reference("TransE", ent, rel, sample, 2, le, lr, w)
    assert abs(a[0] - b[0]) < 1e-12 and np.allclose(a[1], b[1], rtol=1e-14) and np.allclose(a[2], b[2], rtol=1e-14)
