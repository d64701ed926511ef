"""-m gpu: the pooled negative-sampling step on every route of plan_pool (the case table of tests/util_pool_routes.py; its claims
are checked on the CPU by tests/test_host_pool_routes.py) against float64, through each of its entry points:

  step      fused.FusedTrainStep                                   (mkb_pool_step: both product tails fold)
  halves    mkb_pool_step_fwd + mkb_pool_step_bwd                  (one tail folds)
  autograd  model(sample, negative, mode) + losses.Adversarial     (mkb_pool_score_fwd / bwd: nothing folds)

for both modes, tables at the initialisation range and at a trained model's scale, and pools in the sampler's pattern and in an
adversarial one (a row off the dense prefix, one position taken K times, unused positions, one entity at two positions, a pool
entity that is also a head and a tail).  Positive scores, every pool score with cnt > 0, the loss and all gradients are held to
8 x err_ref (util_pool_routes.tolerance), the two table gradients per row as well; every error / err_ref is printed, failures
are collected before the assertion.  Per case once more: prefilled gradient buffers end as prefill + result, a run on dirtied
memory and a workspace of 0xFF bytes gives the same answers, and a given weight sum scales loss and gradients.
The ratios measured on the MI355X are in profiles/r26_pool_routes_errors.txt.
"""
import contextlib
import os

import numpy as np
import pytest
import torch

import util_pool_routes as U

pytestmark = pytest.mark.gpu

ENTRIES = ("step", "halves", "autograd")


@contextlib.contextmanager
def _switches(case):
    """The case's run-time switches in the environment (the library reads them once per call)."""
    names = ("MKB_POOL_NO_MFMA", "MKB_POOL_DENSE", "MKB_GEMM_BF16X3", "MKB_GEMM_NO_PAIR", "MKB_GEMM_NO128")
    saved = {k: os.environ.get(k) for k in names}
    try:
        for k in names:
            os.environ.pop(k, None)
        for k, v in U.switches(case).items():
            if k in names:
                os.environ[k] = v
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _model(pb):
    from util_gpu import make_model

    m = make_model(pb.model, pb.ent, pb.rel, pb.hidden, U.GAMMA, pb.modulus)
    if "misaligned" in U.switches(pb.case):  # a view one float into a larger allocation
        big = torch.empty(pb.ent.size + 8, dtype=torch.float32, device="cuda")
        view = big[1:1 + pb.ent.size].view(pb.ent.shape)
        view.copy_(torch.from_numpy(pb.ent))
        m.entity_embedding = torch.nn.Parameter(view)
        assert m.entity_embedding.data_ptr() % 16 == 4
    return m


class _Batch:
    def __init__(self, pb, mode):
        from mkb_amd import _hip
        from mkb_amd.sampling.negative_sampling import PoolInfo

        dev = lambda a, dt: torch.as_tensor(a).to(dt).cuda().contiguous()
        self.sample, self.weight = dev(pb.sample, torch.int64), dev(pb.weight, torch.float32)
        self.neg = dev(pb.neg, torch.int64)
        self.info = PoolInfo(dev(pb.pool, torch.int64), dev(pb.pos, torch.int32), dev(pb.cnt, torch.int32).to(torch.uint16), pb.K,
                             _hip.mode_id(mode), self.sample)
        self.neg._mkb_pool = self.info


def _grads(m, prefill=None):
    out = {}
    for q, p in (("g_ent", m.entity_embedding), ("g_rel", m.relation_embedding)):
        g = p.grad.detach().double().cpu().numpy()
        out[q] = g if prefill is None else g - prefill[q].double().cpu().numpy()
    if m.name == "pRotatE":
        g = m.modulus.grad.detach().double().cpu().numpy().reshape(())
        out["g_modulus"] = g if prefill is None else g - prefill["g_modulus"].double().cpu().numpy().reshape(())
    else:
        out["g_modulus"] = np.zeros(())
    return out


def _set_grads(m, prefill):
    m.zero_grad(set_to_none=True)
    if prefill is not None:
        m.entity_embedding.grad, m.relation_embedding.grad = prefill["g_ent"].clone(), prefill["g_rel"].clone()
        if m.name == "pRotatE":
            m.modulus.grad = prefill["g_modulus"].clone()


def _run(entry, m, pb, bt, mode, weight_sum=None, prefill=None):
    """One step through an entry point -> the quantities of util_pool_routes.compare as float64 numpy.  A HIP error (the library's
    MKB_ERR_HIP, or torch's own report of one) ends the session: nothing more is started on a device that has faulted.  Any other
    error -- a refused argument, an unsupported shape -- fails this test alone."""
    from mkb_amd import _hip

    try:
        return _run_entry(entry, m, pb, bt, mode, weight_sum, prefill)
    except RuntimeError as e:
        text = str(e)
        if (isinstance(e, _hip.HipLibraryError) and "(status -2)" in text) or "HIP error" in text or "hipError" in text:
            pytest.exit(f"device error in {pb.case[0]} {mode} {entry}: {e}", returncode=3)
        raise


def _run_entry(entry, m, pb, bt, mode, weight_sum, prefill):
    from mkb_amd import _hip, fused, losses

    B, K = pb.B, pb.K
    _set_grads(m, prefill)
    W = None if weight_sum is None else torch.tensor([weight_sum], dtype=torch.float32, device="cuda")
    if entry == "step":
        step = fused.FusedTrainStep(m, alpha=U.ALPHA)
        loss = step(bt.sample, bt.weight, bt.neg, mode, weight_sum=W)
        pos, S = step.positive_score[:, 0], step._S
    elif entry == "halves":
        lib, tb, gr, ws = _hip.lib(), m._tables(), fused.grad_buffers(m), fused._workspace(m, B, K)
        pos = torch.empty(B, dtype=torch.float32, device="cuda")
        S = torch.empty((B, 2 * K), dtype=torch.float32, device="cuda")
        loss = torch.empty(1, dtype=torch.float32, device="cuda")
        mid, info = _hip.mode_id(mode), bt.info
        with _hip.on_device(bt.sample.device):
            _hip.check(lib.mkb_pool_step_fwd(tb, _hip.ptr(bt.sample), _hip.ptr(info.pool), _hip.ptr(info.cnt), B, K, mid, _hip.ptr(pos),
                                             _hip.ptr(S), _hip.ptr(ws), _hip.stream_ptr()), "mkb_pool_step_fwd")
            _hip.check(lib.mkb_pool_step_bwd(tb, gr, _hip.ptr(bt.sample), _hip.ptr(bt.weight), _hip.ptr(info.pool), _hip.ptr(info.cnt), B, K,
                                             mid, U.ALPHA, _hip.ptr(W), _hip.ptr(pos), _hip.ptr(S), _hip.ptr(loss), _hip.ptr(ws),
                                             _hip.stream_ptr()), "mkb_pool_step_bwd")
    else:
        assert weight_sum is None and bt.info.usable_for(m, bt.sample, _hip.mode_id(mode)), "the pooled scoring path must take this batch"
        sc = m(bt.sample, bt.neg, mode)
        loss = losses.Adversarial(alpha=U.ALPHA)(m(bt.sample), sc, bt.weight)
        loss.backward()
        pos = m(bt.sample).detach()[:, 0]
        S = torch.zeros((B, 2 * K), dtype=torch.float32, device="cuda")
        S.scatter_(1, bt.info.pos.long(), sc.detach())  # (the [B, K] view back onto its pool positions)
    torch.cuda.synchronize()
    out = _grads(m, prefill)
    out.update(pos=pos.double().cpu().numpy(), S=S.double().cpu().numpy(), loss=loss.detach().double().cpu().numpy().reshape(()))
    return out


def _hold(failures, case, tag, f64, err, rows, got, cnt, scale_by=1.0):
    for q, e, e_ref, tol in U.compare(case, f64, err, rows, got, cnt, scale_by):
        print(f"pool-routes-error {case[0]} {tag} {q}: error {e:.3e} err_ref {e_ref:.3e} ratio {e / e_ref:.2f} tolerance {tol:.3e}")
        if not e <= tol:
            failures.append((tag, q, e, tol))


@pytest.mark.parametrize("case", U.CASES, ids=U.CASE_IDS)
def test_every_entry_point_against_float64(case):
    from mkb_amd import fused

    failures = []
    with _switches(case):
        for scale in U.SCALES:
            for pattern in U.PATTERNS:
                pb = U.problem(case, scale, pattern)
                m = _model(pb)
                for mode in U.MODES:
                    f64, err, rows = U.expected(case, mode, scale, pattern, device="cuda")
                    bt = _Batch(pb, mode)
                    for entry in ENTRIES:
                        got = _run(entry, m, pb, bt, mode)
                        _hold(failures, case, f"{mode} {scale} {pattern} {entry}", f64, err, rows, got, pb.cnt)
        fused.check_workspace_guards()
    assert not failures, failures


@pytest.mark.parametrize("case", U.CASES, ids=U.CASE_IDS)
def test_prefill_dirty_memory_and_a_given_weight_sum(case):
    from mkb_amd import fused
    from util_gpu import dirty_device_memory

    mode, scale, pattern = U.MODES[U.CASES.index(case) % 2], "trained", "adversarial"
    failures = []
    with _switches(case):
        pb = U.problem(case, scale, pattern)
        f64, err, rows = U.expected(case, mode, scale, pattern, device="cuda")
        m, bt = _model(pb), _Batch(pb, mode)
        # prefilled buffers end as prefill + result.  A touched row is prefilled at the size of its own |term| sum (adding to a
        # value a million times larger would round the result away: that is fp32, not a defect); an untouched row keeps its
        # prefill exactly, whatever it is.
        mine = U.run_step(pb, mode, torch.float64, "cpu" if U.on_host(case) else "cuda")
        g = torch.Generator().manual_seed(7)
        prefill = {}
        for q, a in (("g_ent", mine["a_ent"]), ("g_rel", mine["a_rel"])):
            size = torch.from_numpy(a.max(1, keepdims=True))
            size = torch.where(size > 0, size, torch.ones_like(size))
            prefill[q] = ((torch.rand(a.shape, generator=g, dtype=torch.float64) * 2 - 1) * size).float().cuda()
        prefill["g_modulus"] = torch.full((1, 1), float(abs(f64["g_modulus"])), dtype=torch.float32, device="cuda")
        for entry in ("step", "halves"):
            got = _run(entry, m, pb, bt, mode, prefill=prefill)
            _hold(failures, case, f"{mode} {scale} {pattern} {entry}+prefill", f64, err, rows, got, pb.cnt)
            for q, a in (("g_ent", mine["a_ent"]), ("g_rel", mine["a_rel"])):
                assert not got[q][a.max(1) == 0].any(), f"{entry}: a {q} row nothing contributes to changed"
        # dirty memory: the cached workspace full of 0xFF bytes (always), and freed blocks full of NaN where MKB_TEST_DIRTY_MEMORY
        # asks for them (tests/conftest.py sets it for the -m gpu suite by default)
        dirty_device_memory()
        fused._workspace(m, pb.B, pb.K).fill_(0xFF)
        for entry in ENTRIES:
            got = _run(entry, m, pb, bt, mode)
            _hold(failures, case, f"{mode} {scale} {pattern} {entry}+dirty", f64, err, rows, got, pb.cnt)
        # a given weight sum (a data-parallel shard's): loss and gradients scale by sum(w) / W, the scores stay
        W = 1.75 * float(pb.weight.astype(np.float64).sum())
        ratio = float(np.float32(pb.weight).astype(np.float64).sum()) / float(np.float32(W))
        for entry in ("step", "halves"):
            got = _run(entry, m, pb, bt, mode, weight_sum=W)
            _hold(failures, case, f"{mode} {scale} {pattern} {entry}+weightsum", f64, err, rows, got, pb.cnt, scale_by=ratio)
        fused.check_workspace_guards()
    assert not failures, failures
