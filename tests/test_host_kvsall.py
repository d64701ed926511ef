"""CPU (-m "not gpu") tests of the KvsAll training step's host part: the C ABI (include/mkb_hip.h, "KvsAll", under ABI 8) exports
mkb_all_bce / mkb_all_kvs_step with the declared signatures and refuses bad arguments before any launch; the Python surface
(losses.KvsAll, fused.KvsAllStep) checks its arguments, refuses the distance models and has no CPU fallback; the float64 reference
of the GPU tests (tests/util_kvsall.py) is torch's binary_cross_entropy_with_logits on the dense multi-hot matrix; and its label
construction yields every kind of label set it claims, for every case."""
import pathlib
import re

import numpy as np
import pytest
import torch

import util_kvsall as K
import util_onevsall as U

ROOT = pathlib.Path(__file__).resolve().parent.parent
SYMBOLS = ("mkb_all_bce", "mkb_all_kvs_step")


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
    for name, count in zip(SYMBOLS, (17, 16)):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _hip.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _hip._SIGNATURES[name][1]
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, header, re.S).group(1)  # the header's parameter count is the binding's
        assert len(decl.split(",")) == len(_hip._SIGNATURES[name][1]) == count, name


def test_names_are_public():
    from mkb_amd import fused, losses

    assert "KvsAll" in losses.__all__ and callable(losses.KvsAll)
    assert "KvsAllStep" in fused.__all__ and callable(fused.KvsAllStep)
    assert repr(losses.KvsAll()) == "KvsAll(label_smoothing=0.0, reduction='mean')"
    assert repr(losses.KvsAll([(0, 0, 1)], 0.1, "sum")) == "KvsAll(label_smoothing=0.1, reduction='sum')"
    assert issubclass(fused.KvsAllStep, fused._AllEntityStep) and issubclass(fused.OneVsAllStep, fused._AllEntityStep)  # written once


def _model(name, hidden=4, N=9):
    from mkb_amd import models

    return getattr(models, name)(hidden_dim=hidden, entities={i: i for i in range(N)}, relations={i: i for i in range(2)}, gamma=6.0)


TRIPLES = [(0, 0, 1), (0, 0, 2), (3, 1, 4)]


@pytest.mark.parametrize("eps", [-0.1, 1.0, 1.5, float("nan"), float("inf")])
def test_bad_smoothing_is_refused(eps):
    from mkb_amd import fused, losses

    with pytest.raises(ValueError, match="label_smoothing"):
        losses.KvsAll(TRIPLES, label_smoothing=eps)
    with pytest.raises(ValueError, match="label_smoothing"):
        fused.KvsAllStep(_model("DistMult"), TRIPLES, label_smoothing=eps)


def test_bad_reduction_and_missing_triples_are_refused():
    from mkb_amd import fused, losses

    with pytest.raises(ValueError, match="reduction"):
        losses.KvsAll(TRIPLES, reduction="none")
    with pytest.raises(ValueError, match="reduction"):
        fused.KvsAllStep(_model("ComplEx"), TRIPLES, reduction="batchmean")
    with pytest.raises(ValueError, match="true_triples"):
        fused.KvsAllStep(_model("ComplEx"), None)


@pytest.mark.parametrize("name", ["TransE", "RotatE", "pRotatE"])
def test_distance_models_are_refused_with_the_alternative_named(name):
    from mkb_amd import fused

    with pytest.raises(NotImplementedError, match=r"KvsAllStep covers ComplEx and DistMult.*losses\.CrossEntropy"):
        fused.KvsAllStep(_model(name), TRIPLES)


def test_there_is_no_cpu_fallback():
    from mkb_amd import fused, losses

    sample = torch.zeros((2, 3), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fused.KvsAllStep(_model("ComplEx"), TRIPLES)(sample, None, "tail-batch")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        losses.KvsAll(TRIPLES)(torch.zeros(2, 9), sample, "tail-batch")


def test_wrong_shapes_and_modes_are_refused_by_the_step():
    from mkb_amd import fused

    step = fused.KvsAllStep(_model("DistMult"), TRIPLES)
    good = torch.zeros((2, 3), dtype=torch.int64)
    with pytest.raises(ValueError, match="head-batch"):
        step(good, None, None)
    with pytest.raises(ValueError, match=r"\[B, 3\]"):
        step(torch.zeros((2, 4), dtype=torch.int64), None, "tail-batch")
    with pytest.raises(ValueError, match="weight"):
        step(good, torch.ones(3), "tail-batch")


class _FakeDevice(torch.Tensor):
    """A CPU tensor that says it is on the device: the shape checks behind require_device are reached without one."""

    @property
    def is_cuda(self):
        return True


def test_the_loss_checks_its_arguments():
    from mkb_amd import losses

    fake = lambda t: t.as_subclass(_FakeDevice)
    loss = losses.KvsAll(TRIPLES)
    sample = fake(torch.zeros((4, 3), dtype=torch.int64))
    with pytest.raises(ValueError, match="true_triples"):
        losses.KvsAll()(fake(torch.zeros(4, 5)), sample, "tail-batch")
    with pytest.raises(ValueError, match="head-batch"):
        loss(fake(torch.zeros(4, 5)), sample, "default")
    with pytest.raises(ValueError, match=r"\[B, N\]"):
        loss(fake(torch.zeros(4)), sample, "tail-batch")
    with pytest.raises(ValueError, match="sample"):
        loss(fake(torch.zeros(4, 5)), fake(torch.zeros((3, 3), dtype=torch.int64)), "tail-batch")
    with pytest.raises(ValueError, match="sample"):
        loss(fake(torch.zeros(4, 5)), fake(torch.zeros((4, 3), dtype=torch.int32)), "head-batch")
    with pytest.raises(ValueError, match="weight"):
        loss(fake(torch.zeros(4, 5)), sample, "tail-batch", fake(torch.ones(5)))


def test_invalid_c_arguments_are_refused_before_any_launch():
    """Every call below would fault (the pointers are made up) or fail with MKB_ERR_HIP (no device here) if it got as far as a launch."""
    from mkb_amd import _hip

    lib, P = _hip.lib(), 0x60000000  # (256-byte aligned, never dereferenced)
    tb = _tables()
    n = lib.mkb_all_step_workspace_bytes(tb, 32)
    gr = _hip.Grads(P, P, None)
    names = (("S", P), ("B", 4), ("N", 9), ("ld", 12), ("sample", P), ("mode", _hip.MODE_TAIL), ("R", 3), ("keys", P), ("n_keys", 5),
             ("weight", None), ("wsum", None), ("eps", 0.1), ("sum", 0), ("loss", P), ("pos", P), ("scratch", P), ("stream", None))
    bce = lambda **kw: lib.mkb_all_bce(*[kw.get(k, d) for k, d in names])
    big = 1 << 31
    for bad in (dict(S=None), dict(sample=None), dict(loss=None), dict(pos=None), dict(scratch=None), dict(keys=None), dict(n_keys=-1),
                dict(eps=-0.01), dict(eps=1.0), dict(eps=float("nan")), dict(eps=float("inf")), dict(mode=_hip.MODE_DEFAULT), dict(mode=7),
                dict(B=0), dict(B=-1), dict(N=0), dict(ld=8), dict(R=0), dict(B=1 << 16, N=1 << 15, ld=1 << 15),  # B * ld = 2^31
                dict(B=1, N=big - 1, ld=big - 1, R=big)):  # (N R + R) N past 2^63
        assert bce(**bad) == _hip.ERR_INVALID, bad
        assert lib.mkb_last_error()
    step = lambda tb_=tb, gr_=gr, sample=P, B=32, mode=_hip.MODE_TAIL, keys=P, n_keys=5, eps=0.1, loss=P, pos=P, ws=P, nb=n: lib.mkb_all_kvs_step(
        tb_, gr_, sample, None, B, mode, keys, n_keys, eps, 0, None, loss, pos, ws, nb, None)
    for bad in (dict(tb_=None), dict(gr_=None), dict(gr_=_hip.Grads(None, P, None)), dict(gr_=_hip.Grads(P, None, None)), dict(sample=None),
                dict(B=0), dict(mode=_hip.MODE_DEFAULT), dict(keys=None), dict(n_keys=-1), dict(eps=1.0), dict(eps=-1.0),
                dict(eps=float("nan")), dict(loss=None), dict(pos=None), dict(ws=None), dict(nb=n - 1), dict(ws=P + 16), dict(B=1 << 25)):
        assert step(**bad) == _hip.ERR_INVALID, bad
    for name in ("TransE", "RotatE", "pRotatE"):  # another model: unsupported
        assert step(tb_=_tables(name)) == _hip.ERR_UNSUPPORTED, name


def test_the_reference_is_torchs_bce_with_logits_on_the_multi_hot_matrix():
    for case in (U.CASES[0], U.CASES[5]):
        pb = U.problem(case)
        for mode in U.MODES:
            L = K.labels(case, mode)
            f64, _ = K.expected(case, mode, 0.0, "mean", weighted=False)
            S = torch.from_numpy(f64["S"]).requires_grad_(True)
            Y = torch.from_numpy(K.multi_hot(L.sample, mode, L.keys, pb.N))
            want = torch.nn.functional.binary_cross_entropy_with_logits(S, Y)
            want.backward()
            assert abs(float(want.detach()) - float(f64["loss"])) <= 1e-12 * abs(float(want.detach()))
            assert np.abs(S.grad.numpy() - f64["dS"]).max() <= 1e-12 * np.abs(f64["dS"]).max()


@pytest.mark.parametrize("case", U.CASES, ids=U.CASE_IDS)
def test_the_label_construction_yields_every_kind(case):
    from mkb_amd.utils.true_keys import _build

    N = case[4]
    for mode in U.MODES:
        L = K.labels(case, mode)
        assert L.sample.shape == (case[3], 3) and (np.diff(L.keys) > 0).all()
        assert (L.sample >= 0).all() and (L.sample[:, [0, 2]] < N).all() and (L.sample[:, 1] < K.R).all()
        found = K.label_kinds(L.sample, mode, L.keys, N)
        assert K.required_kinds(N) <= found, (case[0], mode, K.required_kinds(N) - found)
        # the designed rows are where the table says, and the keys are what the library builds from the triples
        n = K.multi_hot(L.sample, mode, L.keys, N).sum(1).astype(int)
        assert [n[L.rows[k]] for k in K.KINDS] == [0, 1, *K.lane_counts(N), 2, N, N]
        assert np.array_equal(_build(L.triples, "cpu", N, K.R)[mode].numpy(), L.keys)


def test_own_target_labels_are_one_per_row():
    for case in U.CASES:
        for mode in U.MODES:
            s, keys, triples = K.own_target_labels(case, mode)
            Y = K.multi_hot(s, mode, keys, case[4])
            assert (Y.sum(1) == 1).all() and (Y[np.arange(len(s)), s[:, 0 if mode == "head-batch" else 2]] == 1).all()
