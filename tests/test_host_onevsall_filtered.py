"""CPU (-m "not gpu") tests of the filtered 1vsAll step's host part: the C ABI (include/mkb_hip.h, "filtered 1vsAll", under ABI 8)
exports mkb_all_softmax_filtered / mkb_all_filtered_step with the declared signatures and refuses bad arguments before any launch;
the Python surface (losses.OneVsAll, fused.OneVsAllStep) takes the new settings, checks them, and is unchanged at its defaults; the
float64 reference of the GPU tests (tests/util_onevsall_filtered.py) is torch's cross entropy with label smoothing -- on the whole
row without keys, on the row with its filtered columns physically deleted with keys; and its batches hold every kind of row they
claim, for every shape the GPU tests use."""
import pathlib
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import util_onevsall as U
import util_onevsall_filtered as V

ROOT = pathlib.Path(__file__).resolve().parent.parent
SYMBOLS = ("mkb_all_softmax_filtered", "mkb_all_filtered_step")
TRIPLES = [(0, 0, 1), (0, 0, 2), (3, 1, 4)]


def _case(name):
    return U.CASES[U.CASE_IDS.index(name)]


def _tables(model="ComplEx", hidden=8, n_entity=129, n_relation=3, ent=0x40000000):
    from mkb_amd import _hip

    de = 2 * hidden if model in ("RotatE", "ComplEx") else hidden
    dr = 2 * hidden if model == "ComplEx" else hidden
    return _hip.Tables(_hip.MODEL_IDS[model], hidden, n_entity, n_relation, de, dr, ent, 0x50000000, 0x50100000, 6.0, 0.5)


def _model(name, hidden=4, N=9):
    from mkb_amd import models

    return getattr(models, name)(hidden_dim=hidden, entities={i: i for i in range(N)}, relations={i: i for i in range(2)}, gamma=6.0)


def test_symbols_are_declared_exported_and_bound_under_abi_8():
    from mkb_amd import _hip

    header = (ROOT / "include" / "mkb_hip.h").read_text()
    assert re.search(r"#define\s+MKB_ABI_VERSION\s+9\b", header) and _hip.ABI_VERSION == 9
    lib = _hip.lib()
    assert lib.mkb_abi_version() == 9
    for name, count in zip(SYMBOLS, (19, 16)):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _hip.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _hip._SIGNATURES[name][1]
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, header, re.S).group(1)  # the header's parameter count is the binding's
        assert len(decl.split(",")) == len(_hip._SIGNATURES[name][1]) == count, name


def test_the_defaults_are_unchanged():
    from mkb_amd import fused, losses

    loss = losses.OneVsAll()
    assert repr(loss) == "OneVsAll(temperature=1.0)" and repr(losses.OneVsAll(0.5)) == "OneVsAll(temperature=0.5)"
    assert loss.temperature == 1.0 and loss.label_smoothing == 0.0 and loss.filter_known is False and loss.true_triples is None
    assert loss.kind is None
    step = fused.OneVsAllStep(_model("ComplEx"))
    assert step.temperature == 1.0 and step.label_smoothing == 0.0 and step.true_triples is None and step.regularizer is None


def test_the_new_settings_are_kept_and_shown():
    from mkb_amd import fused, losses

    loss = losses.OneVsAll(temperature=0.5, label_smoothing=0.1, filter_known=True, true_triples=TRIPLES)
    assert (loss.temperature, loss.label_smoothing, loss.filter_known, loss.true_triples) == (0.5, 0.1, True, TRIPLES)
    assert repr(loss) == "OneVsAll(temperature=0.5, label_smoothing=0.1, filter_known=True)"
    step = fused.OneVsAllStep(_model("DistMult"), 2.0, None, 0.2, TRIPLES)
    assert (step.temperature, step.label_smoothing, step.true_triples) == (2.0, 0.2, TRIPLES)


@pytest.mark.parametrize("eps", [-0.1, 1.0, 1.5, float("nan"), float("inf")])
def test_bad_smoothing_is_refused(eps):
    from mkb_amd import fused, losses

    with pytest.raises(ValueError, match="label_smoothing"):
        losses.OneVsAll(label_smoothing=eps)
    with pytest.raises(ValueError, match="label_smoothing"):
        fused.OneVsAllStep(_model("DistMult"), label_smoothing=eps)


class _FakeDevice(torch.Tensor):
    """A CPU tensor that says it is on the device: the checks behind require_device are reached without one."""

    @property
    def is_cuda(self):
        return True


def test_filtering_asks_for_its_arguments_at_call_time():
    from mkb_amd import losses

    fake = lambda t: t.as_subclass(_FakeDevice)
    scores, target = fake(torch.zeros(4, 5)), fake(torch.zeros(4, dtype=torch.int64))
    sample = fake(torch.zeros((4, 3), dtype=torch.int64))
    with pytest.raises(ValueError, match="true_triples"):
        losses.OneVsAll(filter_known=True)(scores, target, sample=sample, mode="tail-batch")
    loss = losses.OneVsAll(filter_known=True, true_triples=TRIPLES)
    with pytest.raises(ValueError, match="sample and mode"):
        loss(scores, target)
    with pytest.raises(ValueError, match="sample and mode"):
        loss(scores, target, sample=sample)
    with pytest.raises(ValueError, match="head-batch"):
        loss(scores, target, sample=sample, mode="default")
    with pytest.raises(ValueError, match="sample"):
        loss(scores, target, sample=fake(torch.zeros((3, 3), dtype=torch.int64)), mode="tail-batch")
    with pytest.raises(ValueError, match="target"):
        loss(scores, fake(torch.zeros(3, dtype=torch.int64)), sample=sample, mode="tail-batch")


def test_there_is_no_cpu_fallback():
    from mkb_amd import fused, losses

    sample = torch.zeros((2, 3), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fused.OneVsAllStep(_model("ComplEx"), label_smoothing=0.1, true_triples=TRIPLES)(sample, None, "tail-batch")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        losses.OneVsAll(label_smoothing=0.1)(torch.zeros(2, 9), sample[:, 2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        losses.OneVsAll(filter_known=True, true_triples=TRIPLES)(torch.zeros(2, 9), sample[:, 2], sample=sample, mode="tail-batch")


@pytest.mark.parametrize("name", ["TransE", "RotatE", "pRotatE"])
def test_distance_models_are_refused(name):
    from mkb_amd import fused

    with pytest.raises(NotImplementedError, match=r"OneVsAllStep covers ComplEx and DistMult"):
        fused.OneVsAllStep(_model(name), label_smoothing=0.1, true_triples=TRIPLES)


def test_invalid_c_arguments_are_refused_before_any_launch():
    """Every call below would fault (the pointers are made up) or fail with MKB_ERR_HIP (no device here) if it got as far as a launch."""
    from mkb_amd import _hip

    lib, P = _hip.lib(), 0x60000000  # (256-byte aligned, never dereferenced)
    tb = _tables()
    n = lib.mkb_all_step_workspace_bytes(tb, 32)
    gr = _hip.Grads(P, P, None)
    names = (("S", P), ("B", 4), ("N", 9), ("ld", 12), ("target", P), ("tstride", 1), ("sample", P), ("mode", _hip.MODE_TAIL), ("R", 3),
             ("keys", P), ("n_keys", 5), ("weight", None), ("wsum", None), ("T", 1.0), ("eps", 0.1), ("loss", P), ("pos", P), ("scratch", P),
             ("stream", None))
    call = lambda **kw: lib.mkb_all_softmax_filtered(*[kw.get(k, d) for k, d in names])
    big = 1 << 31
    for bad in (dict(S=None), dict(target=None), dict(sample=None), dict(loss=None), dict(pos=None), dict(scratch=None), dict(keys=None),
                dict(n_keys=-1), dict(T=0.0), dict(T=-1.0), dict(T=float("nan")), dict(T=float("inf")), dict(eps=-0.01), dict(eps=1.0),
                dict(eps=float("nan")), dict(eps=float("inf")), dict(mode=_hip.MODE_DEFAULT), dict(mode=7), dict(B=0), dict(B=-1), dict(N=0),
                dict(ld=8), dict(tstride=0), dict(R=0), dict(B=1 << 16, N=1 << 15, ld=1 << 15),  # B * ld = 2^31
                dict(B=1, N=big - 1, ld=big - 1, R=big)):  # (N R + R) N past 2^63
        assert call(**bad) == _hip.ERR_INVALID, bad
        assert lib.mkb_last_error()
    step = lambda tb_=tb, gr_=gr, sample=P, B=32, mode=_hip.MODE_TAIL, keys=P, n_keys=5, T=1.0, eps=0.1, loss=P, pos=P, ws=P, nb=n: \
        lib.mkb_all_filtered_step(tb_, gr_, sample, None, B, mode, keys, n_keys, T, eps, None, loss, pos, ws, nb, None)
    for bad in (dict(tb_=None), dict(gr_=None), dict(gr_=_hip.Grads(None, P, None)), dict(gr_=_hip.Grads(P, None, None)), dict(sample=None),
                dict(B=0), dict(mode=_hip.MODE_DEFAULT), dict(keys=None), dict(n_keys=-1), dict(T=0.0), dict(T=float("nan")), dict(eps=1.0),
                dict(eps=-1.0), dict(eps=float("nan")), dict(loss=None), dict(pos=None), dict(ws=None), dict(nb=n - 1), dict(ws=P + 16),
                dict(B=1 << 25)):
        assert step(**bad) == _hip.ERR_INVALID, bad
    for name in ("TransE", "RotatE", "pRotatE"):  # another model: unsupported
        assert step(tb_=_tables(name)) == _hip.ERR_UNSUPPORTED, name


@pytest.mark.parametrize("eps,T", V.SETTINGS)
def test_without_keys_the_reference_is_torchs_smoothed_cross_entropy(eps, T):
    none = np.zeros(0, dtype=np.int64)
    for case in (_case("ragged-complex"), _case("t64-n130-d64")):
        pb = U.problem(case)
        for mode in U.MODES:
            f64 = V.compute(pb.model, torch.from_numpy(pb.ent).double(), torch.from_numpy(pb.rel).double(), pb.sample, mode, none, None,
                            eps=eps, T=T)
            S = torch.from_numpy(f64["S"]).requires_grad_(True)
            want = F.cross_entropy(S / T, torch.from_numpy(pb.target(mode)), label_smoothing=eps)
            want.backward()
            assert abs(float(want.detach()) - float(f64["loss"])) <= 1e-12 * abs(float(want.detach()))
            assert np.abs(S.grad.numpy() - f64["dS"]).max() <= 1e-12 * np.abs(f64["dS"]).max()
            if eps == 0.0 and T == 1.0:  # ... and today's 1vsAll reference
                plain = U.compute(pb.model, torch.from_numpy(pb.ent).double(), torch.from_numpy(pb.rel).double(), pb.sample, mode, None)
                assert abs(float(plain["loss"]) - float(f64["loss"])) <= 1e-12 * abs(float(plain["loss"]))
                assert np.abs(plain["g_ent"] - f64["g_ent"]).max() <= 1e-12 * np.abs(plain["g_ent"]).max()


@pytest.mark.parametrize("eps,T", V.SETTINGS)
def test_with_keys_the_reference_is_the_cross_entropy_of_the_row_with_its_filtered_columns_deleted(eps, T):
    case = _case("t64-n130-d64")
    pb = U.problem(case)
    for mode in U.MODES:
        L = V.case_rows(case, mode)
        f64, _ = V.expected(case, mode, eps, T, weighted=False)
        Fm = V.filtered_mask(L.sample, mode, L.keys, pb.N)
        target = V.open_slot(L.sample, mode)
        assert Fm.any(1).sum() >= 7
        for i in range(pb.B):
            keep = np.flatnonzero(~Fm[i])
            s = torch.from_numpy(f64["S"][i, keep]).requires_grad_(True)
            want = F.cross_entropy(s[None] / T, torch.tensor([int(np.searchsorted(keep, target[i]))]), label_smoothing=eps)
            want.backward()
            assert abs(float(want.detach()) - f64["rows"][i]) <= 1e-12 * max(1.0, abs(float(want.detach()))), (mode, i)
            assert np.abs(s.grad.numpy() / pb.B - f64["dS"][i, keep]).max() <= 1e-12, (mode, i)
            assert not f64["dS"][i, Fm[i]].any() and f64["n"][i] == len(keep)
        for kind in ("all", "same"):  # n_i = 1: the row is 0 and so is its gradient
            i = L.rows[kind]
            assert f64["n"][i] == 1 and abs(f64["rows"][i]) <= 1e-12 and np.abs(f64["dS"][i]).max() <= 1e-15


SHAPES = sorted({(c[0], c[3], c[4]) for c in U.CASES if c[0] in V.STEP_CASES} | {(f"block-n{N}", 16, N) for N in (129, 130, 131, 5000)})


@pytest.mark.parametrize("name,B,N", SHAPES, ids=[s[0] for s in SHAPES])
def test_the_batches_hold_every_kind_of_row(name, B, N):
    from mkb_amd.utils.true_keys import _build

    for mode in U.MODES:
        L = V.rows(name, B, N, mode)
        assert L.sample.shape == (B, 3) and (np.diff(L.keys) > 0).all()
        assert (L.sample >= 0).all() and (L.sample[:, [0, 2]] < N).all() and (L.sample[:, 1] < V.R).all()
        found = V.kinds(L.sample, mode, L.keys, N)
        assert V.required_kinds(N) <= found, (name, mode, V.required_kinds(N) - found)
        # the designed rows are where the table says, and the keys are what the library builds from the triples
        nF = V.filtered_mask(L.sample, mode, L.keys, N).sum(1)
        assert [int(nF[L.rows[k]]) for k in V.KINDS] == [0, 0, 1, *V.lane_counts(N), N - 1, N - 1]
        assert np.array_equal(_build(L.triples, "cpu", N, V.R)[mode].numpy(), L.keys)
        # a target that is not the sample's open slot: that entity is then filtered like any other key
        shifted = (V.open_slot(L.sample, mode) + 1) % N
        Fs = V.filtered_mask(L.sample, mode, L.keys, N, shifted)
        i = L.rows["only"]
        assert Fs[i, V.open_slot(L.sample, mode)[i]] and not Fs[np.arange(B), shifted].any()
