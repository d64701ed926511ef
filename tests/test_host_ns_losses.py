"""CPU (-m "not gpu") tests of the negative-sampling loss family's host part: the C ABI (include/mkb_hip.h, under ABI 8) exports
mkb_ns_loss with the declared signature and refuses bad arguments before any launch; the three classes import, validate their
parameters and refuse CPU tensors; and the float64 reference the GPU tests compare the kernel with (tests/util_ns_losses.py)
agrees with closed-form values on a 2x2 case written out by hand."""
import ctypes
import math
import re

import numpy as np
import pytest
import torch

import util_ns_losses as un

PARAMS = ["int kind", "const float *pos", "const float *neg", "const float *weight", "const uint16_t *cnt", "int64_t B", "int64_t K",
          "float param", "float alpha", "const float *weight_sum", "float *loss", "float *dpos", "float *dneg", "float *scratch",
          "void *stream"]


def test_symbol_signature_and_abi():
    from conftest import ROOT
    from mkb_amd import _hip

    header = (ROOT / "include" / "mkb_hip.h").read_text()
    assert re.search(r"#define MKB_ABI_VERSION 9\b", header) and _hip.ABI_VERSION == 9
    assert re.search(r"typedef enum \{ MKB_LOSS_MARGIN = 0, MKB_LOSS_PAIR_LOGISTIC = 1, MKB_LOSS_SOFTMAX = 2 \} mkb_loss_t;", header)
    decl = re.search(r"\bint mkb_ns_loss\(([^)]*)\);", header)
    assert decl
    assert [" ".join(a.split()) for a in decl.group(1).split(",")] == PARAMS
    c = ctypes

    def ctype(param):
        return c.c_void_p if "*" in param else {"int64_t": c.c_int64, "int": c.c_int, "float": c.c_float}[param.split()[0]]

    assert _hip._SIGNATURES["mkb_ns_loss"] == (c.c_int, [ctype(p) for p in PARAMS])
    assert hasattr(ctypes.CDLL(str(ROOT / "mkb_amd" / "libmkb_hip.so")), "mkb_ns_loss")
    assert (_hip.LOSS_MARGIN, _hip.LOSS_PAIR_LOGISTIC, _hip.LOSS_SOFTMAX) == (un.MARGIN, un.PAIR_LOGISTIC, un.SOFTMAX) == (0, 1, 2)
    assert _hip.lib().mkb_abi_version() == 9


def test_abi_rejects_bad_arguments_before_any_launch():
    """Every refusal of the header comment, on a machine without a GPU: the pointers are never dereferenced."""
    from mkb_amd import _hip

    lib = _hip.lib()
    p = ctypes.c_void_p(0x10000)

    def call(kind=0, pos=p, neg=p, weight=p, cnt=p, B=4, K=3, param=1.0, alpha=0.0, weight_sum=None, loss=p, dpos=p, dneg=p,
             scratch=p):
        return lib.mkb_ns_loss(kind, pos, neg, weight, cnt, B, K, param, alpha, weight_sum, loss, dpos, dneg, scratch, None)

    cases = [dict(pos=None), dict(neg=None), dict(loss=None), dict(dpos=None), dict(dneg=None), dict(scratch=None),
             dict(kind=3), dict(kind=-1), dict(kind=99),
             dict(B=0), dict(B=-1), dict(K=0), dict(K=-5), dict(B=1 << 31, K=1), dict(B=1, K=1 << 31), dict(B=1 << 16, K=1 << 15),
             dict(B=(1 << 31) - 1, K=2),
             dict(alpha=-0.5), dict(alpha=-1e-30), dict(alpha=float("nan")), dict(kind=1, alpha=-1.0),
             dict(kind=2, param=0.0), dict(kind=2, param=-1.0),
             dict(param=float("nan")), dict(param=float("inf")), dict(kind=1, param=float("-inf")), dict(kind=2, param=float("inf")),
             dict(kind=2, param=float("nan"))]
    for kw in cases:
        assert call(**kw) == _hip.ERR_INVALID, kw
        assert lib.mkb_last_error(), kw


def test_classes_import_validate_and_refuse_the_cpu():
    from mkb_amd import losses

    assert {"MarginRanking", "PairwiseLogistic", "CrossEntropy"} <= set(losses.__all__)
    m, p, c = losses.MarginRanking(), losses.PairwiseLogistic(), losses.CrossEntropy()
    assert (m.margin, m.alpha, p.margin, p.alpha, c.temperature) == (1.0, 0.0, 0.0, 0.0, 1.0)
    assert (m.kind, p.kind, c.kind) == (un.MARGIN, un.PAIR_LOGISTIC, un.SOFTMAX)
    assert (m.param, p.param, c.param, c.alpha) == (1.0, 0.0, 1.0, 0.0)
    for bad in (dict(alpha=-1.0), dict(margin=float("nan")), dict(alpha=float("inf"))):
        with pytest.raises(ValueError):
            losses.MarginRanking(**bad)
        with pytest.raises(ValueError):
            losses.PairwiseLogistic(**bad)
    for T in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            losses.CrossEntropy(temperature=T)
    pos, neg, w = torch.zeros(4, 1), torch.zeros(4, 3), torch.ones(4)
    for loss in (m, p, c):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            loss(pos, neg, w)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            loss(pos, neg)


def test_pooled_step_refuses_other_losses():
    from mkb_amd import fused, losses

    with pytest.raises(TypeError):
        fused.PooledLossStep(None, losses.Adversarial(0.5))
    with pytest.raises(TypeError):
        fused.PooledLossStep(None, lambda p, n, w: 0)


def test_reference_agrees_with_closed_forms_on_a_2x2_case():
    pos, neg, w = [1.0, 0.0], [[0.0, 1.0], [-1.0, 0.0]], [1.0, 3.0]  # W = 4
    e = math.e
    # margin 0.5, alpha 0: a = [[-.5, .5], [-.5, .5]], rows = [.25, .25]
    loss, dpos, dneg = un.reference(un.MARGIN, pos, neg, w, param=0.5)
    assert loss == pytest.approx(0.25, abs=1e-15)
    np.testing.assert_allclose(dneg, [[0, 0.125], [0, 0.375]], atol=1e-15)
    np.testing.assert_allclose(dpos, [-0.125, -0.375], atol=1e-15)
    # pairwise logistic, margin 0, alpha = ln 2: both rows weigh their negatives 1/3, 2/3; a = [[-1, 0], [-1, 0]]
    sp1 = math.log1p(1 / e)
    loss, dpos, dneg = un.reference(un.PAIR_LOGISTIC, pos, neg, w, param=0.0, alpha=math.log(2))
    assert loss == pytest.approx(sp1 / 3 + 2 * math.log(2) / 3, abs=1e-15)
    g = np.array([1 / 3 / (1 + e), 2 / 3 * 0.5])
    np.testing.assert_allclose(dneg, [0.25 * g, 0.75 * g], atol=1e-15)
    np.testing.assert_allclose(dpos, [-0.25 * g.sum(), -0.75 * g.sum()], atol=1e-15)
    # softmax, T = 2: Z0 = e^.5 + 1 + e^.5, Z1 = 1 + e^-.5 + 1
    z0, z1 = 2 * e ** 0.5 + 1, 2 + e ** -0.5
    loss, dpos, dneg = un.reference(un.SOFTMAX, pos, neg, w, param=2.0)
    assert loss == pytest.approx((1 * (math.log(z0) - 0.5) + 3 * math.log(z1)) / 4, abs=1e-15)
    np.testing.assert_allclose(dneg, [[1 / 8 / z0, e ** 0.5 / 8 / z0], [3 * e ** -0.5 / 8 / z1, 3 / 8 / z1]], atol=1e-15)
    np.testing.assert_allclose(dpos, [(e ** 0.5 / z0 - 1) / 8, 3 * (1 / z1 - 1) / 8], atol=1e-15)
    # multiplicities [[2, 1], [0, 3]], NaN where the multiplicity is 0, the caller's weight sum 8 instead of 4
    cnt, neg_nan = [[2, 1], [0, 3]], [[0.0, 1.0], [float("nan"), 0.0]]
    z0, z1 = e ** 0.5 + 2 + e ** 0.5, 1 + 3
    loss, dpos, dneg = un.reference(un.SOFTMAX, pos, neg_nan, w, cnt=cnt, param=2.0, weight_sum=8.0)
    assert loss == pytest.approx((1 * (math.log(z0) - 0.5) + 3 * math.log(z1)) / 8, abs=1e-15)
    np.testing.assert_allclose(dneg, [[2 / 16 / z0, e ** 0.5 / 16 / z0], [0, 3 * 3 / 16 / z1]], atol=1e-15)
    # margin with the same multiplicities: row 0 = (2 * 0 + 1 * .5) / 3, row 1 = .5
    loss, dpos, dneg = un.reference(un.MARGIN, pos, neg_nan, w, cnt=cnt, param=0.5)
    assert loss == pytest.approx((0.5 / 3 + 3 * 0.5) / 4, abs=1e-15)
    np.testing.assert_allclose(dneg, [[0, 0.25 / 3], [0, 0.75]], atol=1e-15)
    # a row that uses no position contributes 0 (pairwise) / its positive term only, exactly 0 (softmax)
    for kind in (un.MARGIN, un.PAIR_LOGISTIC, un.SOFTMAX):
        loss, dpos, dneg = un.reference(kind, pos, neg_nan, w, cnt=[[0, 0], [0, 0]], param=1.0)
        assert loss == 0.0 and not dpos.any() and not dneg.any()
    # multiplicities are repeated columns
    for kind, param, alpha in ((un.MARGIN, 0.5, 0.7), (un.PAIR_LOGISTIC, 0.2, 0.3), (un.SOFTMAX, 0.5, 0.0)):
        a = un.reference(kind, [1.0], [[0.3, 7.0, -0.4]], None, cnt=[[2, 0, 3]], param=param, alpha=alpha)
        b = un.reference(kind, [1.0], [un.expand_row([0.3, 7.0, -0.4], [2, 0, 3])], None, param=param, alpha=alpha)
        assert a[0] == pytest.approx(b[0], abs=1e-15) and a[1] == pytest.approx(b[1], abs=1e-15)
        np.testing.assert_allclose(a[2][0], [b[2][0][:2].sum(), 0, b[2][0][2:].sum()], atol=1e-15)
