"""CPU (-m "not gpu") tests of ``mkb_amd.optim.Adagrad`` and ``mkb_adagrad_step``: the symbol through header, library and binding,
argument checking before any launch, the constructor's refusals, the checkpoint layout and the attributes ``compose.Pipeline``
looks at."""
import ctypes
import re

import pytest
import torch


def test_adagrad_step_is_declared_exported_and_bound_at_abi_8():
    from conftest import ROOT
    from mkb_amd import _hip

    header = (ROOT / "include" / "mkb_hip.h").read_text()
    assert re.search(r"\bint\s+mkb_adagrad_step\s*\(", header) and "mkb_adagrad_dense_t" in header
    assert re.search(r"#define\s+MKB_ABI_VERSION\s+9\b", header) and _hip.ABI_VERSION == 9
    raw = ctypes.CDLL(str(ROOT / "mkb_amd" / "libmkb_hip.so"))
    assert hasattr(raw, "mkb_adagrad_step")
    assert "mkb_adagrad_step" in _hip.EXPORTED_SYMBOLS
    lib = _hip.lib()
    assert lib.mkb_abi_version() == 9
    assert len(lib.mkb_adagrad_step.argtypes) == 15
    assert [name for name, _ in _hip.AdagradDense._fields_] == ["param", "grad", "sum", "n"]
    assert ctypes.sizeof(_hip.AdagradDense) == 32


def test_invalid_adagrad_arguments_are_reported_before_any_launch():
    """Every case fails in the argument checks: nothing is launched, so the made-up addresses are never touched."""
    from mkb_amd import _hip

    lib = _hip.lib()
    P = ctypes.c_void_p(4096)  # a non-null address that no check dereferences
    one = (_hip.AdagradDense * 1)(_hip.AdagradDense(4096, 4096, 4096, 4))

    def call(param=P, grad=P, acc=P, last=P, n_rows=10, D=4, ids=P, n_ids=1, step=1, dense=None, n_dense=0):
        rc = lib.mkb_adagrad_step(param, grad, acc, last, n_rows, D, ids, n_ids, step, 0.1, 1e-10, dense, n_dense, None, None)
        return rc, lib.mkb_last_error()

    for kwargs, word in (
        (dict(grad=None), b"grad"), (dict(acc=None), b"sum"), (dict(last=None), b"last"),  # a table without its arrays
        (dict(D=0), b"D"), (dict(D=-4), b"D"),
        (dict(step=0), b"step"), (dict(step=-3), b"step"),
        (dict(n_dense=9, dense=one), b"dense"), (dict(n_dense=-1), b"dense"), (dict(n_dense=1, dense=None), b"dense"),
        (dict(param=None), b"nothing to step"),           # the dense-only form needs n_dense > 0
        (dict(ids=None, n_ids=3), b"n_ids"),               # the all-rows form is ids == null AND n_ids == 0
        (dict(n_ids=-1), b"n_ids"),
        (dict(param=None, n_dense=1, dense=(_hip.AdagradDense * 1)(_hip.AdagradDense(4096, None, 4096, 4))), b"dense tensor 0"),
    ):
        rc, msg = call(**kwargs)
        assert rc == _hip.ERR_INVALID and word in msg, (kwargs, rc, msg)


def test_constructor_refuses_what_it_cannot_do_row_sparsely_and_what_torch_refuses():
    from mkb_amd import optim

    p = [torch.nn.Parameter(torch.zeros(8, 4))]
    with pytest.raises(ValueError, match="regularizers.L2"):
        optim.Adagrad(p, weight_decay=1e-4)
    with pytest.raises(ValueError, match="learning rate"):
        optim.Adagrad(p, lr=-0.1)
    for bad in (dict(lr_decay=-1e-3), dict(eps=-1e-10), dict(initial_accumulator_value=-0.1), dict(weight_decay=-1.0)):
        with pytest.raises(ValueError):
            optim.Adagrad(p, **bad)
        with pytest.raises(ValueError):
            torch.optim.Adagrad(p, **bad)  # (torch refuses the same)
    assert optim.__all__ == ["Adam", "Adagrad"]


def test_state_dict_has_torchs_layout_and_building_it_needs_no_device():
    from mkb_amd import _links, optim

    big, small = torch.nn.Parameter(torch.randn(5000, 6)), torch.nn.Parameter(torch.randn(7, 6))
    opt = optim.Adagrad([big, small], lr=0.1, lr_decay=1e-3, initial_accumulator_value=0.1, eps=1e-9)
    assert _links.owner(big) is opt and _links.owner(small) is None  # the 4,096-row rule of Adam(lazy_rows=True)
    sd = opt.state_dict()
    ref = torch.optim.Adagrad([big, small], lr=0.1, lr_decay=1e-3, initial_accumulator_value=0.1, eps=1e-9).state_dict()
    assert set(sd) == set(ref) == {"state", "param_groups"}
    assert set(sd["state"]) == set(ref["state"]) == {0, 1}
    for i, p in enumerate((big, small)):
        assert set(sd["state"][i]) == set(ref["state"][i]) == {"step", "sum"}
        assert torch.equal(sd["state"][i]["step"], ref["state"][i]["step"]) and sd["state"][i]["step"].dtype == ref["state"][i]["step"].dtype
        assert torch.equal(sd["state"][i]["sum"], ref["state"][i]["sum"])
        assert sd["state"][i]["sum"].shape == p.shape
    assert len(sd["param_groups"]) == 1
    group = sd["param_groups"][0]
    assert {"lr", "lr_decay", "eps", "weight_decay", "initial_accumulator_value", "params"} <= set(ref["param_groups"][0])
    assert set(group) == {"lr", "lr_decay", "eps", "weight_decay", "initial_accumulator_value", "params"}
    assert group == {k: ref["param_groups"][0][k] for k in group}
    # the stamps of a row-sparse table; a load leaves every one of them below the next step
    last = opt.state[big]["last"]
    assert last.dtype == torch.int32 and last.shape == (5000,) and not last.any()
    sd["state"][0]["step"] = torch.tensor(6.0)
    opt.load_state_dict(sd)
    assert opt.state[big]["n"] == 6 and int(opt.state[big]["last"].max()) < 7 and opt.step_count == 6
    assert set(opt.state_dict()["state"][0]) == {"step", "sum"}


def test_attributes_the_pipeline_and_the_steps_look_at():
    from mkb_amd import optim

    p = [torch.nn.Parameter(torch.zeros(8, 4))]
    opt = optim.Adagrad(p)
    assert not hasattr(opt, "defer_step")  # compose.Pipeline must not try to defer
    assert opt.lazy_rows is True and opt.draw_ahead is None and opt.direct_grads is True
    assert opt.rows_always_current is True and not hasattr(optim.Adam(p), "rows_always_current")  # fused.sampled_step's route
    assert (opt.lr, opt.lr_decay, opt.weight_decay, opt.initial_accumulator_value, opt.eps) == (1e-2, 0.0, 0.0, 0.0, 1e-10)  # torch's
    with pytest.raises(NotImplementedError, match="single-device"):
        opt.catch_up_sharded(p[0], None, 2, 0, None)
    with pytest.raises(NotImplementedError, match="single-device"):
        opt.catch_up_with_sampler(p[0], None, None, None, 0, ())
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # a missing device is an error, not a quiet torch step
        p[0].grad = torch.ones(8, 4)
        opt.step()
