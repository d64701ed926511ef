"""The Adam launches (mkb_amd/csrc/adam.hip) on every leaf of their plan (mkb_amd/csrc/adam_plan.h), driven through the C ABI over
the case table of tests/util_adam_routes.py (tests/test_host_adam_routes.py shows on the host that each case takes the leaves it
claims, and that the measure used here bites).

Bit for bit.  The same hand-made stream runs through dense ``mkb_adam_step`` and through the row-lazy forms -- plain catch-up +
``mkb_adam_rows_step``, the advance form, the advance form with a flush in mid-run, the ownership form where claimed.  Each must end
with the bits of the dense run; rows read before a step hold the dense run's bits of that moment; ``last`` follows a host model of
it launch by launch; the gradient buffer ends all zero; never-touched rows keep their bits; the guard bands around every array keep
their sentinel; a rider ends with the bits of its own ``mkb_adam_step`` launches.

Float64.  Dense and row-lazy kernels share ``adam_one`` / ``adam_pair``, so the comparison above is blind to an error both make.
The dense result is therefore held against the element rule in float64 (util_adam_routes.run64, pinned to torch's float64 Adam on
the host), per table row and per quantity, within ERR_FACTOR = 4 x err_ref, the distance torch.optim.Adam on float32 CPU tensors
keeps from the same float64 result.  Derivation of the factor: m and v are formed with torch's operations, each rounded once.  The
update term takes v_sqrt_f32 and two v_rcp_f32 (1 ulp each) where torch has correctly rounded operations, so it carries about twice
torch's rounding -- of a term that is lr-sized, 1e-2 or less of the parameter's own final rounding, which both sides share.  Ratios
near 1 to 2 are expected; 4 leaves a factor two.  util_adam_routes.MEASURED_RATIO and profiles/r27_adam_routes_errors.txt keep what
an MI355X gave.
"""
import functools

import numpy as np
import pytest
import torch

import util_adam_routes as U

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 64  # elements of sentinel in front of and behind every array (256 bytes: a view behind it keeps the allocation's alignment)
SENTINEL = {torch.float32: 12345.678, torch.int32: -77}
WORLD, RANK = 3, 1


class Banded:
    """A tensor between two guard bands, ``off`` elements off the allocation's 16-byte grid."""

    def __init__(self, shape, dtype=torch.float32, off=0, init=None):
        n = int(np.prod(shape))
        self.raw = torch.full((GUARD + off + n + GUARD,), SENTINEL[dtype], dtype=dtype, device=DEV)
        self.lo, self.hi = GUARD + off, GUARD + off + n
        self.t = self.raw[self.lo:self.hi].view(shape)
        if init is None:
            self.t.zero_()
        else:
            self.t.copy_(init)
        assert self.t.data_ptr() % 16 == (4 * off) % 16

    def intact(self):
        s = SENTINEL[self.raw.dtype]
        return bool((self.raw[:self.lo] == s).all()) and bool((self.raw[self.hi:] == s).all())


class Table:
    """p, g, m, v, last, consts of one run, each between guard bands."""

    def __init__(self, case, off=None):
        off = case.off if off is None else off
        self.case = case
        self.P = Banded((case.N, case.D), off=off, init=U.initial(case))
        self.G, self.M, self.V = (Banded((case.N, case.D), off=off) for _ in range(3))
        self.LAST = Banded((case.N,), torch.int32)
        self.CONSTS = Banded((case.T + 2, 2))
        self.p, self.g, self.m, self.v, self.last = self.P.t, self.G.t, self.M.t, self.V.t, self.LAST.t
        self.rider = Rider(case) if case.rider else None

    def intact(self):
        return all(b.intact() for b in (self.P, self.G, self.M, self.V, self.LAST, self.CONSTS)) and (self.rider is None or self.rider.intact())


class Rider:
    def __init__(self, case):
        p0, base = U.rider_initial(case)
        self.n = case.rider
        self.P = Banded((self.n,), init=p0)
        self.G, self.M, self.V = (Banded((self.n,)) for _ in range(3))
        self.base = base.to(DEV)
        self.p, self.g, self.m, self.v = self.P.t, self.G.t, self.M.t, self.V.t

    def write_gradient(self, t):
        self.g.copy_(U.rider_gradient(self.base, t))

    def struct(self, t):
        from mkb_amd import _hip
        return _hip.AdamDense(self.p.data_ptr(), self.g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.n, t + U.RIDER_STEP_OFFSET)

    def intact(self):
        return all(b.intact() for b in (self.P, self.G, self.M, self.V))


def _dense_step(p, g, m, v, step, lr, betas):
    from mkb_amd import _hip
    _hip.check(_hip.lib().mkb_adam_step(_hip.ptr(p), _hip.ptr(g), _hip.ptr(m), _hip.ptr(v), p.numel(), step, lr, betas[0], betas[1], U.EPS, 1,
                                        _hip.stream_ptr()), "mkb_adam_step")


def _table_args(tb, grad):
    from mkb_amd import _hip
    return (_hip.ptr(tb.p), _hip.ptr(tb.g) if grad else None, _hip.ptr(tb.m), _hip.ptr(tb.v), _hip.ptr(tb.last), _hip.ptr(tb.CONSTS.t),
            tb.case.N, tb.case.D)


def _rows_step(tb, ids, step, lr, rider):
    from mkb_amd import _hip
    b = tb.case.betas
    _hip.check(_hip.lib().mkb_adam_rows_step(*_table_args(tb, True), _hip.ptr(ids), ids.numel(), step, lr, b[0], b[1], U.EPS, rider,
                                             _hip.stream_ptr()), "mkb_adam_rows_step")


def _advance(tb, grad, ids, upto, lr, rider, own=None):
    """ids: int64 device tensor, or None for the whole table; own: (global ids,) of the ownership form in front of ids."""
    from mkb_amd import _hip
    b = tb.case.betas
    rows = (_hip.ptr(own), own.numel(), WORLD, RANK) if own is not None else (None, 0, 0, 0)
    rows += (_hip.ptr(ids), 0 if ids is None else ids.numel())
    _hip.check(_hip.lib().mkb_adam_rows_advance(*_table_args(tb, grad), *rows, upto, lr, b[0], b[1], U.EPS, rider, None, _hip.stream_ptr()),
               "mkb_adam_rows_advance")


def _set_sweep(monkeypatch, case):
    if case.sweep is None:
        monkeypatch.delenv("MKB_ADAM_SWEEP", raising=False)
    else:
        monkeypatch.setenv("MKB_ADAM_SWEEP", case.sweep)


@functools.lru_cache(maxsize=1)
def _dense_run(case):
    """The stream through mkb_adam_step on the whole table (16-byte aligned whatever the case's offset: the rule is element-wise).
    -> the table, what a reader of step t must see (the listed rows after t - 1 steps), the state after T // 2 steps."""
    tb = Table(case, off=0)
    n = case.N * case.D
    reads, mid = [], None
    for t, (rows, vals) in enumerate(U.gradients(case), start=1):
        rows = torch.as_tensor(rows, device=DEV)
        reads.append(tb.p[rows].clone())
        tb.g[rows] = vals.to(DEV)
        _dense_step(tb.p, tb.g, tb.m, tb.v, t, U.lr_of(case, t), case.betas)
        if tb.rider is not None:
            r = tb.rider
            r.write_gradient(t)
            _dense_step(r.p, r.g, r.m, r.v, t + U.RIDER_STEP_OFFSET, U.lr_of(case, t), case.betas)
        if t == case.T // 2:
            mid = (tb.p.clone(), tb.m.clone(), tb.v.clone())
    assert n == tb.p.numel() and not tb.g.any() and tb.intact()
    return tb, reads, mid


def _run_form(case, form, dense):
    """form: "plain" | "advance" | "advance-flush" | "own" (the advance form with the ownership split of every step's id list)."""
    ref, reads, mid = dense
    tb = Table(case)
    expect_last = np.zeros(case.N, dtype=np.int32)
    deferred, pending_rider = False, None  # advance forms: a deferred step waits in the gradient rows | its rider

    def check_last(where):
        assert torch.equal(tb.last, torch.as_tensor(expect_last, device=DEV)), (case.name, form, where)

    for t in range(1, case.T + 1):
        ids, extras = U.schedule(case)[t - 1]
        rows = torch.as_tensor(U.valid_rows(case, ids), device=DEV)
        if t >= 2:
            for k, lst in enumerate([ids] + list(extras)):
                own = None
                if form == "own" and k == 0:
                    glob, lst = U.own_split(case, lst, WORLD, RANK)
                    own = torch.as_tensor(glob, device=DEV)
                n_listed = len(lst) + (0 if own is None else own.numel())
                if form == "plain":
                    _advance(tb, False, torch.as_tensor(lst, device=DEV), t - 1, 0.0, None, own)
                else:
                    _advance(tb, deferred, torch.as_tensor(lst, device=DEV), t - 1, U.lr_of(case, t - 1) if deferred else 0.0,
                             pending_rider if deferred else None, own)
                    pending_rider = None
                visited = U.valid_rows(case, ids if k == 0 else lst)
                expect_last[np.concatenate([visited, U.sweep_window(case, n_listed, t - 1)]).astype(np.int64)] = t - 1
            check_last(f"catch-up before step {t}")
        assert torch.equal(tb.p[rows], reads[t - 1]), (case.name, form, f"rows read at step {t} are not current")
        assert not tb.g[rows].any(), (case.name, form, f"a gradient row of step {t} was not cleared")
        grad_rows, vals = U.gradients(case)[t - 1]
        tb.g[torch.as_tensor(grad_rows, device=DEV)] = vals.to(DEV)
        if tb.rider is not None:
            tb.rider.write_gradient(t)
        if form == "plain" or t == 1:
            _rows_step(tb, torch.as_tensor(ids, device=DEV), t, U.lr_of(case, t), tb.rider.struct(t) if tb.rider is not None else None)
            expect_last[U.valid_rows(case, ids)] = t
            check_last(f"step {t}")
        else:
            deferred, pending_rider = True, tb.rider.struct(t) if tb.rider is not None else None
        if form == "advance-flush" and t == case.T // 2:
            _advance(tb, deferred, None, t, U.lr_of(case, t), pending_rider)
            pending_rider = None
            expect_last[:] = t
            check_last("flush in mid-run")
            assert all(torch.equal(a, b) for a, b in zip((tb.p, tb.m, tb.v), mid)), (case.name, form, "the flush in mid-run differs from dense Adam")
            assert not tb.g.any()
    _advance(tb, deferred, None, case.T, U.lr_of(case, case.T) if deferred else 0.0, pending_rider)
    expect_last[:] = case.T
    check_last("closing flush")
    for q in U.QUANTITIES:
        a, b = getattr(tb, q), getattr(ref, q)
        assert torch.equal(a, b), (case.name, form, q, f"{int((a != b).sum())} elements differ from dense Adam")
    assert not tb.g.any(), (case.name, form, "the gradient buffer is not all zero")
    never = np.ones(case.N, dtype=bool)
    never[U.live_rows(case)] = False
    never = torch.as_tensor(never, device=DEV)
    assert torch.equal(tb.p[never], U.initial(case).to(DEV)[never]) and not tb.m[never].any() and not tb.v[never].any()
    assert tb.intact(), (case.name, form, "a guard band was written")
    if tb.rider is not None:
        for q in U.QUANTITIES:
            assert torch.equal(getattr(tb.rider, q), getattr(ref.rider, q)), (case.name, form, "rider", q)
        assert not tb.rider.g.any()
    # the constants every step recorded are the ones a launch of that step computes: (-lr / (1 - b1^s), sqrt(1 - b2^s)), rounded once
    s = np.arange(1, case.T + 1, dtype=np.float64)
    lr = np.asarray([U.lr_of(case, int(k)) for k in s])
    want = np.stack([-(lr / (1 - case.betas[0] ** s)), np.sqrt(1 - case.betas[1] ** s)], 1).astype(np.float32)
    assert np.array_equal(tb.CONSTS.t[1:case.T + 1].cpu().numpy(), want), (case.name, form, "recorded constants")


@pytest.mark.parametrize("case", U.CASES, ids=U.CASE_IDS)
def test_every_row_lazy_form_is_dense_adam_bit_for_bit(case, monkeypatch):
    _set_sweep(monkeypatch, case)
    dense = _dense_run(case)
    for form in ("plain", "advance", "advance-flush") + (("own",) if case.own else ()):
        _run_form(case, form, dense)


@pytest.mark.parametrize("case", U.CASES, ids=U.CASE_IDS)
def test_dense_adam_stays_within_four_times_torchs_distance_from_float64(case):
    tb, _, _ = _dense_run(case)
    live = torch.as_tensor(U.reference(case).live, device=DEV)
    ratios = U.ratios(case, {q: getattr(tb, q)[live].cpu().numpy() for q in U.QUANTITIES})
    print(f"adam-routes-ratio {case.name} ({case.group}): " + "  ".join(f"{q} {ratios[q]:.3f}" for q in U.QUANTITIES))
    assert all(r <= U.ERR_FACTOR for r in ratios.values()), (case.name, ratios)


def _dense_tensors(n, p0, grads, first_step):
    """DENSE_STEPS launches of mkb_adam_step on a banded tensor of n floats -> the four Banded arrays."""
    P = Banded((n,), init=p0[:n])
    G, M, V = (Banded((n,)) for _ in range(3))
    for k, g in enumerate(grads):
        G.t.copy_(g[:n])
        _dense_step(P.t, G.t, M.t, V.t, first_step + k, U.LRS[0], (0.9, 0.999))
    return P, G, M, V


def _assert_dense_close(name, got, f64, err):
    for q, b in zip(U.QUANTITIES, got):
        ratio = float((np.abs(b.t.double().cpu().numpy() - f64[q]) / err[q]).max())
        print(f"adam-routes-ratio {name}: {q} {ratio:.3f}")
        assert ratio <= U.ERR_FACTOR, (name, q, ratio)


def test_dense_step_at_every_tail_and_past_the_grid_stride_cap():
    small = max(n for n in U.DENSE_NS if n <= 4096)
    p0, grads = U.dense_stream(small)
    f64, err = U.dense_reference(p0, grads)
    whole = None
    for n in sorted((n for n in U.DENSE_NS if n <= small), reverse=True):
        P, G, M, V = _dense_tensors(n, p0, grads, 1)
        assert not G.t.any() and all(b.intact() for b in (P, G, M, V)), n
        if whole is None:
            whole = (P, M, V)
            _assert_dense_close(f"dense n={n}", (P, M, V), f64, err)
        for a, b in zip((P, M, V), whole):  # a shorter tensor's float4 body and scalar tail give the bits of the longer one's prefix
            assert torch.equal(a.t, b.t[:n]), n
    big = max(U.DENSE_NS)
    p0, grads = U.dense_stream(big)
    f64, err = U.dense_reference(p0, grads)
    P, G, M, V = _dense_tensors(big, p0, grads, 1)
    assert not G.t.any() and all(b.intact() for b in (P, G, M, V))
    _assert_dense_close(f"dense n={big}", (P, M, V), f64, err)


def test_multi_tensor_step_is_eight_single_steps():
    """mkb_adam_step_multi over eight tensors, each with its own step count, three launches: the bits of eight mkb_adam_step launch
    sequences, which are held against float64."""
    from mkb_amd import _hip

    p0, grads = U.dense_stream(max(n for n, _ in U.MULTI), seed=4)
    grads = grads[:3]
    multi = [(Banded((n,), init=p0[:n]),) + tuple(Banded((n,)) for _ in range(3)) for n, _ in U.MULTI]
    for k, g in enumerate(grads):
        for (n, _), (P, G, M, V) in zip(U.MULTI, multi):
            G.t.copy_(g[:n])
        arr = (_hip.AdamDense * len(multi))(*[_hip.AdamDense(P.t.data_ptr(), G.t.data_ptr(), M.t.data_ptr(), V.t.data_ptr(), n, s + k)
                                              for (n, s), (P, G, M, V) in zip(U.MULTI, multi)])
        _hip.check(_hip.lib().mkb_adam_step_multi(arr, len(multi), U.LRS[0], 0.9, 0.999, U.EPS, 1, None, _hip.stream_ptr()), "mkb_adam_step_multi")
    for (n, s), (P, G, M, V) in zip(U.MULTI, multi):
        single = _dense_tensors(n, p0, grads, s)
        assert not G.t.any() and all(b.intact() for b in (P, G, M, V)), n
        for a, b in zip((P, M, V), (single[0], single[2], single[3])):
            assert torch.equal(a.t, b.t), (n, s)
        f64, err = U.dense_reference(p0[:n], [g[:n] for g in grads], first_step=s, width=64)
        _assert_dense_close(f"multi n={n} step={s}", (P, M, V), f64, err)


@pytest.mark.parametrize("defer", [False, True])
def test_the_constants_table_grows_at_step_65536(defer):
    """mkb_amd.optim.Adam itself on a 4,096 x 36 table: a row-lazy and a dense twin start from one state at step 65,530 with non-zero
    moments and take twelve steps whose row gaps straddle 65,535 | 65,536, where ``_consts`` doubles the per-step constants table
    and copies it.  The replays read constants on both sides of the old table's end: the bits of the dense twin."""
    from mkb_amd import _links, optim

    N, D, start = 4096, 36, 65530
    g = torch.Generator(device="cpu").manual_seed(9)
    p0, m0, v0 = torch.randn(N, D, generator=g), torch.randn(N, D, generator=g) * 0.1, torch.rand(N, D, generator=g) * 0.01 + 1e-4
    state = {"state": {0: {"step": start, "exp_avg": m0.to(DEV), "exp_avg_sq": v0.to(DEV)}},
             "param_groups": [{"lr": 1e-3, "betas": (0.9, 0.999), "eps": U.EPS, "params": [0]}], "step_count": start}
    # rows 0 .. 5 are visited at steps start + 1 + (their list): the gaps 65,532 -> 65,537 -> 65,541 and 65,535 -> 65,536 straddle the end
    visits = {0: (1, 2, 7, 11), 1: (2, 7, 12), 2: (5, 6, 12), 3: (3, 9), 4: (1, 12), 5: tuple(range(1, 13))}
    out = []
    for lazy in (True, False):
        ent = torch.nn.Parameter(p0.clone().to(DEV))
        ent.grad = torch.zeros_like(ent)
        opt = optim.Adam([ent], lr=1e-3, lazy_rows=lazy, defer_step=defer if lazy else None)
        opt.load_state_dict(state)
        assert (_links.owner(ent) is opt) == lazy
        if lazy:
            assert opt.state[ent]["consts"].shape[0] == 1 << 16
        for k in range(1, 13):
            rows = [r for r, ks in visits.items() if k in ks] + [100 + k, 100 + k]  # (and a fresh row, listed twice)
            ids = torch.tensor(rows, device=DEV)
            if lazy:
                opt.catch_up(ent, ids)
            uniq = torch.unique(ids)
            gg = torch.Generator(device="cpu").manual_seed(100 + k)
            ent.grad[uniq] += torch.randn(uniq.numel(), D, generator=gg).to(DEV)
            if lazy:
                _links.mark_touched(ent, ids)
            opt.step()
            opt.zero_grad()
        if lazy:
            assert opt.state[ent]["n"] == start + 12 and opt.state[ent]["consts"].shape[0] == 1 << 17
            assert bool(opt.state[ent].get("defer")) == defer
            opt.flush()
            assert not ent.grad.any()
        out.append((ent.detach().clone(), opt.state[ent]["m"].clone(), opt.state[ent]["v"].clone()))
    for q, a, b in zip(U.QUANTITIES, *out):
        assert torch.equal(a, b), (q, f"{int((a != b).sum())} elements differ from the dense twin")
    assert not torch.equal(out[0][0], p0.to(DEV))
