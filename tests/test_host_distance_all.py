"""CPU (-m "not gpu") tests of the host part of the all-entity losses of the distance models: the C ABI (include/mkb_hip.h, "all-entity
losses, distance models", under ABI 9) exports the six mkb_dist_all_* calls with the declared signatures and refuses bad arguments
before any launch; the Python surface (fused.DistanceAllStep, fused.distance_score_all) checks its arguments, refuses ComplEx and
DistMult and has no CPU fallback; the case table and the float64 replica of the GPU tests (tests/util_distance_all.py) are what they
claim to be."""
import pathlib
import re

import numpy as np
import pytest
import torch

import util_distance_all as U

ROOT = pathlib.Path(__file__).resolve().parent.parent
SYMBOLS = ("mkb_dist_all_workspace_bytes", "mkb_dist_all_score_fwd", "mkb_dist_all_score_bwd", "mkb_dist_all_step",
           "mkb_dist_all_filtered_step", "mkb_dist_all_kvs_step")


def _tables(model="RotatE", hidden=8, n_entity=129, n_relation=3, ent=0x40000000):
    from mkb_amd import _hip

    de = 2 * hidden if model in ("RotatE", "ComplEx") else hidden
    dr = 2 * hidden if model == "ComplEx" else hidden
    return _hip.Tables(_hip.MODEL_IDS[model], hidden, n_entity, n_relation, de, dr, ent, 0x50000000, 0x50100000, 6.0, 0.5)


def test_symbols_are_declared_exported_and_bound_under_abi_9():
    from mkb_amd import _hip

    header = (ROOT / "include" / "mkb_hip.h").read_text()
    assert re.search(r"#define\s+MKB_ABI_VERSION\s+9\b", header) and _hip.lib().mkb_abi_version() == 9
    lib = _hip.lib()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _hip.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _hip._SIGNATURES[name][1]
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, header, re.S).group(1)
        assert len(decl.split(",")) == len(_hip._SIGNATURES[name][1]), name  # the header's parameter counts are the binding's
    # ... and argument for argument those of the call each one mirrors
    for new, old in (("workspace_bytes", "step_workspace_bytes"), ("score_fwd", "score_fwd"), ("score_bwd", "score_bwd"), ("step", "step"),
                     ("filtered_step", "filtered_step"), ("kvs_step", "kvs_step")):
        assert _hip._SIGNATURES["mkb_dist_all_" + new] == _hip._SIGNATURES["mkb_all_" + old]


def test_names_are_public():
    from mkb_amd import fused

    assert "DistanceAllStep" in fused.__all__ and callable(fused.DistanceAllStep)
    assert "distance_score_all" in fused.__all__ and callable(fused.distance_score_all)
    assert fused.DISTANCE_MODELS == U.MODELS


def _model(name, hidden=4, N=9):
    from mkb_amd import models

    return getattr(models, name)(hidden_dim=hidden, entities={i: i for i in range(N)}, relations={i: i for i in range(2)}, gamma=6.0)


@pytest.mark.parametrize("name", ["ComplEx", "DistMult"])
def test_product_models_are_refused_with_their_own_steps_named(name):
    from mkb_amd import fused, losses

    m = _model(name)
    with pytest.raises(NotImplementedError, match=r"OneVsAllStep.*KvsAllStep"):
        fused.DistanceAllStep(m, losses.OneVsAll())
    with pytest.raises(NotImplementedError, match=r"model\.score_all"):
        fused.distance_score_all(m, torch.zeros((2, 3), dtype=torch.int64), "tail-batch")


@pytest.mark.parametrize("name", U.MODELS)
def test_the_old_steps_name_the_new_one(name):
    from mkb_amd import fused

    with pytest.raises(NotImplementedError, match=r"DistanceAllStep"):
        fused.OneVsAllStep(_model(name))
    with pytest.raises(NotImplementedError, match=r"DistanceAllStep"):
        fused.KvsAllStep(_model(name), [(0, 0, 1)])


def test_argument_errors_of_the_step_are_raised():
    from mkb_amd import fused, losses

    m = _model("RotatE")
    with pytest.raises(TypeError, match="OneVsAll or losses.KvsAll"):
        fused.DistanceAllStep(m, losses.CrossEntropy())
    with pytest.raises(ValueError, match="true_triples"):
        fused.DistanceAllStep(m, losses.KvsAll())
    with pytest.raises(ValueError, match="true_triples"):
        fused.DistanceAllStep(m, losses.OneVsAll(filter_known=True))
    assert fused.DistanceAllStep(m, losses.KvsAll(), true_triples=[(0, 0, 1)]).true_triples == [(0, 0, 1)]
    assert fused.DistanceAllStep(m, losses.KvsAll([(1, 0, 2)]), true_triples=[(0, 0, 1)]).true_triples == [(1, 0, 2)]  # the marker's own win
    step = fused.DistanceAllStep(m, losses.OneVsAll())
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
        fused.distance_score_all(m, good, "default")


@pytest.mark.parametrize("name", U.MODELS)
def test_there_is_no_cpu_fallback(name):
    from mkb_amd import fused, losses

    m = _model(name)
    sample = torch.zeros((2, 3), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fused.distance_score_all(m, sample, "tail-batch")
    for marker in (losses.OneVsAll(), losses.OneVsAll(label_smoothing=0.1), losses.KvsAll([(0, 0, 1)])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fused.DistanceAllStep(m, marker)(sample, None, "tail-batch")


def test_invalid_c_arguments_are_refused_before_any_launch():
    """Every call below would fault (the pointers are made up) or fail with MKB_ERR_HIP (no device here) if it got as far as a launch."""
    from mkb_amd import _hip

    lib, P = _hip.lib(), 0x60000000  # (256-byte aligned, never dereferenced)
    tb = _tables()
    n = lib.mkb_dist_all_workspace_bytes(tb, 32)
    assert n > 0
    gr = _hip.Grads(P, P, None)
    nan, inf = float("nan"), float("inf")

    def step(tb_=tb, gr_=gr, sample=P, B=32, mode=_hip.MODE_TAIL, T=1.0, loss=P, pos=P, ws=P, nb=n):
        return lib.mkb_dist_all_step(tb_, gr_, sample, None, B, mode, T, None, loss, pos, ws, nb, None)

    def filtered(tb_=tb, gr_=gr, sample=P, B=32, mode=_hip.MODE_TAIL, keys=P, n_keys=4, T=1.0, eps=0.1, loss=P, pos=P, ws=P, nb=n):
        return lib.mkb_dist_all_filtered_step(tb_, gr_, sample, None, B, mode, keys, n_keys, T, eps, None, loss, pos, ws, nb, None)

    def kvs(tb_=tb, gr_=gr, sample=P, B=32, mode=_hip.MODE_TAIL, keys=P, n_keys=4, eps=0.1, loss=P, pos=P, ws=P, nb=n):
        return lib.mkb_dist_all_kvs_step(tb_, gr_, sample, None, B, mode, keys, n_keys, eps, 0, None, loss, pos, ws, nb, None)

    common = (dict(tb_=None), dict(gr_=None), dict(gr_=_hip.Grads(None, P, None)), dict(gr_=_hip.Grads(P, None, None)), dict(sample=None),
              dict(B=0), dict(B=-1), dict(mode=_hip.MODE_DEFAULT), dict(loss=None), dict(pos=None), dict(ws=None), dict(nb=n - 1),
              dict(ws=P + 16), dict(B=1 << 25))  # (129 + 3) 2^25 > 2^31
    temperature = (dict(T=0.0), dict(T=-1.0), dict(T=nan), dict(T=inf))
    smoothing = (dict(eps=-0.1), dict(eps=1.0), dict(eps=nan), dict(keys=None), dict(n_keys=-1))
    for call, bads in ((step, common + temperature), (filtered, common + temperature + smoothing), (kvs, common + smoothing)):
        for bad in bads:
            assert call(**bad) == _hip.ERR_INVALID, (call.__name__, bad)
            assert lib.mkb_last_error()
    assert filtered(keys=None, n_keys=0, ws=None) == _hip.ERR_INVALID  # (no keys is legal: it is the workspace that is refused)
    # B * Npad at 2^31 exactly: 2^15 - 1 entities pad to 2^15 columns, B = 2^16
    big = _tables(n_entity=(1 << 15) - 1)
    assert step(tb_=big, B=1 << 16, nb=1 << 40) == _hip.ERR_INVALID and lib.mkb_dist_all_workspace_bytes(big, 1 << 16) == 0
    fwd = lambda scores=P, mode=_hip.MODE_TAIL, B=32, ws=P, nb=n: lib.mkb_dist_all_score_fwd(tb, P, B, mode, scores, ws, nb, None)
    for bad in (dict(scores=None), dict(mode=_hip.MODE_DEFAULT), dict(B=0), dict(ws=None), dict(nb=n - 1), dict(ws=P + 16)):
        assert fwd(**bad) == _hip.ERR_INVALID, bad
    bwd = lambda gr_=gr, d=P, ld=129, mode=_hip.MODE_TAIL, B=32, ws=P, nb=n: lib.mkb_dist_all_score_bwd(tb, gr_, P, B, mode, d, ld, ws, nb, None)
    for bad in (dict(gr_=None), dict(d=None), dict(ld=128), dict(mode=_hip.MODE_DEFAULT), dict(B=0), dict(nb=n - 1), dict(ws=P + 16)):
        assert bwd(**bad) == _hip.ERR_INVALID, bad
    for name in ("ComplEx", "DistMult"):  # the product models: unsupported, and the message names their own calls
        other = _tables(name)
        for call in (step, filtered, kvs):
            assert call(tb_=other) == _hip.ERR_UNSUPPORTED, name
            assert b"mkb_all_" in lib.mkb_last_error()
        assert lib.mkb_dist_all_workspace_bytes(other, 32) == 0
    # pRotatE without its modulus is no valid table
    no_mod = _tables("pRotatE")
    no_mod.modulus = None
    assert step(tb_=no_mod) == _hip.ERR_INVALID


def test_workspace_is_positive_aligned_and_monotone_in_the_batch():
    from mkb_amd import _hip

    lib = _hip.lib()
    batches = (1, 2, 7, 16, 17, 32, 37, 64, 100, 128, 130, 200, 256)  # (the radix sort's size query answers larger ones only with a device)
    for model in U.MODELS:
        for hidden, N in ((4, 9), (37, 129), (130, 1030), (300, 129), (1000, 14541)):
            tb = _tables(model, hidden, N)
            sizes = [lib.mkb_dist_all_workspace_bytes(tb, B) for B in batches]
            assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1], (model, hidden, N, sizes)
            assert all(s % 256 == 0 for s in sizes)
            de = U.entity_dim(model, hidden)
            assert sizes[-1] >= 256 * de * 4 * 3 + 256 * N * 4 + N * 8  # at least Q, dQ, the stash, the score block and the id list
    assert lib.mkb_dist_all_workspace_bytes(_tables(), 0) == 0 and lib.mkb_dist_all_workspace_bytes(None, 8) == 0
    assert lib.mkb_dist_all_workspace_bytes(_tables(n_entity=14541), 1 << 20) == 0  # B * Npad past 2^31: the calls refuse it


# ---------------------------------------------------------------------------------------------------- the GPU tests' own tools
def test_the_case_table_has_every_value_of_every_axis_for_every_model_and_side():
    for model in U.MODELS:
        for mode in U.MODES:
            mine = [c for c in U.CASES if c[0] == model and c[1] == mode]
            assert {c[3] for c in mine} >= {4, 37, 130} and {c[4] for c in mine} >= {9, 129, 1030} and {c[5] for c in mine} >= {1, 7, 37, 130}
            assert any(U.entity_dim(model, c[3]) > 256 or c[3] > 256 for c in mine)  # a second unit slice
            assert any(c[3] % 4 == 0 and c[3] >= 64 for c in mine)                   # the forward's register tile
    assert len(set(U.CASE_IDS)) == len(U.CASES)


@pytest.mark.parametrize("model", U.MODELS)
@pytest.mark.parametrize("mode", U.MODES)
def test_the_replica_states_the_closed_form_scores(model, mode):
    """The [B, N, De] expression of the replica against oracle/closed.py's float64 scores of the same candidates."""
    from oracle import closed

    pb = U.problem((model, mode, "h37-n129-b7", 37, 129, 7))
    with torch.no_grad():
        S, _ = U.score_block(model, torch.tensor(pb.ent, dtype=torch.float64), torch.tensor(pb.rel, dtype=torch.float64),
                             torch.tensor([[pb.modulus]], dtype=torch.float64), torch.as_tensor(pb.sample), mode, pb.gamma,
                             closed.emb_range_over_pi(pb.gamma, pb.hidden))
    cand = np.tile(np.arange(pb.N), (pb.B, 1))
    want = closed.scores(model, pb.ent, pb.rel, pb.sample, cand, mode, pb.gamma, pb.hidden, modulus=pb.modulus)
    assert np.abs(S.numpy() - want).max() <= 1e-12


def test_the_replica_losses_are_torchs():
    """softmax: F.cross_entropy at the temperature; kvs: BCEWithLogitsLoss on the smoothed multi-hot labels; filtered: cross entropy
    over the kept columns with the smoothed one-hot label -- on the replica's own float64 scores."""
    F = torch.nn.functional
    pb = U.problem(("TransE", "tail-batch", "h37-n129-b7", 37, 129, 7))
    pb = pb._replace(weight=None)
    f64 = U.replica(pb, "softmax", torch.float64)
    S, target = torch.from_numpy(f64["S"]), torch.from_numpy(pb.sample[:, 2])
    assert abs(float(F.cross_entropy(S / 0.5, target)) - float(f64["loss"])) <= 1e-12
    A = torch.from_numpy(U.label_mask(pb.sample, pb.mode, pb.triples, pb.N))
    assert A[torch.arange(pb.B), target].all() and int(A.sum()) > pb.B  # the batch's own triples are known, and more
    f64 = U.replica(pb, "kvs", torch.float64)
    y = 0.9 * A.double() + 0.1 / pb.N
    assert abs(float(F.binary_cross_entropy_with_logits(S, y)) - float(f64["loss"])) <= 1e-12
    f64 = U.replica(pb, "filtered", torch.float64)
    rows = []
    for i in range(pb.B):
        kept = ~A[i]
        kept[target[i]] = True
        cols = torch.nonzero(kept)[:, 0]
        rows.append(F.cross_entropy(S[i, cols][None] / 0.5, (cols == target[i]).nonzero()[0], label_smoothing=0.1))
        assert (f64["dS"][i][~kept.numpy()] == 0).all()
    assert abs(float(torch.stack(rows).mean()) - float(f64["loss"])) <= 1e-12
