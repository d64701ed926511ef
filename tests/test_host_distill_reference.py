"""Runs anywhere: the float64 reference of tests/util_distill.py against the captures of the live reference
(tests/golden/distill.npz, tools/make_golden.py::gen_distill), before tests/test_gpu_distill_shapes.py trusts the device
against it; and the assertions of ``grid_tables`` at every (model, hidden, gamma) that file uses."""
import numpy as np
import pytest
import torch

import util_distill as U
from util_gpu import grad_close


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_kl_reference_reproduces_the_captures(golden, tag):
    """The captures are float32 torch: 1e-6 is the bound tests/test_gpu_distill.py holds the kernel to against them."""
    g = golden("distill.npz")
    loss, ds, _ = U.kl_reference(g[f"kl/{tag}/student"], g[f"kl/{tag}/teacher"], float(g[f"kl/{tag}/T"]))
    np.testing.assert_allclose(loss.item(), float(g[f"kl/{tag}/loss"]), rtol=0, atol=1e-6)
    np.testing.assert_allclose(ds.numpy(), g[f"kl/{tag}/dstudent"], rtol=0, atol=1e-6)


def _cpu_model(cls, ent, rel, hidden, gamma, ents, rels):
    from mkb_amd import models

    m = getattr(models, cls)(hidden_dim=hidden, entities=ents, relations=rels, gamma=gamma)
    return m._set_params(torch.as_tensor(ent), torch.as_tensor(rel))


def test_distill_reference_reproduces_the_umls_doctest(golden):
    """distillation/distillation.py:452-498: Umls, RotatE hidden 3, UniformSampling(3, 3, seed 42) -> loss 1.3066.  The index
    tensors come from ``Distillation.distillation_tensors`` on the CPU (plain torch indexing: no kernel involved)."""
    from mkb_amd import datasets, distillation

    g, gj = golden("distill.npz"), golden("distill.json")
    ds = datasets.Umls(batch_size=3, shuffle=False, seed=42, num_workers=0)
    teacher = _cpu_model("RotatE", g["umls/teacher_ent"], g["umls/teacher_rel"], 3, 6, ds.entities, ds.relations)
    student = _cpu_model("RotatE", g["umls/student_ent"], g["umls/student_rel"], 3, 6, ds.entities, ds.relations)
    proc = distillation.Distillation(teacher_entities=ds.entities, student_entities=ds.entities, teacher_relations=ds.relations,
                                     student_relations=ds.relations,
                                     sampling=distillation.UniformSampling(batch_size_entity=3, batch_size_relation=3, seed=42))
    ref = U.distill_reference(proc, teacher, student, torch.as_tensor(g["umls/sample"]))
    assert round(ref["loss"].item(), 4) == gj["umls_doctest_loss"] == 1.3066
    np.testing.assert_allclose(ref["loss"].item(), float(g["umls/loss"]), rtol=0, atol=1e-5)
    grad_close(ref["g_ent"].numpy(), g["umls/g_ent"])
    grad_close(ref["g_rel"].numpy(), g["umls/g_rel"])
    assert ref["g_modulus"] is None and set(ref["student_scores"]) == set(U.PARTS)
    assert all(s.dtype == torch.float64 and s.shape[1] == 3 for s in ref["student_scores"].values())


def test_distill_reference_reproduces_the_partial_overlap_capture(golden):
    from mkb_amd import distillation

    g = golden("distill.npz")
    t_ents = {f"e{i}": i for i in range(6)}
    s_ents = {f"e{i}": j for j, i in enumerate([7, 3, 8, 5, 4, 6])}
    t_rels = {f"r{i}": i for i in range(3)}
    s_rels = {"r3": 0, "r1": 1, "r2": 2}
    teacher = _cpu_model("TransE", g["part/teacher_ent"], g["part/teacher_rel"], 4, 3, t_ents, t_rels)
    student = _cpu_model("DistMult", g["part/student_ent"], g["part/student_rel"], 5, 3, s_ents, s_rels)
    proc = distillation.Distillation(teacher_entities=t_ents, student_entities=s_ents, teacher_relations=t_rels,
                                     student_relations=s_rels,
                                     sampling=distillation.UniformSampling(batch_size_entity=2, batch_size_relation=2, seed=5))
    ref = U.distill_reference(proc, teacher, student, torch.as_tensor(g["part/sample"]))
    np.testing.assert_allclose(ref["loss"].item(), float(g["part/loss"]), rtol=0, atol=1e-5)
    grad_close(ref["g_ent"].numpy(), g["part/g_ent"])
    grad_close(ref["g_rel"].numpy(), g["part/g_rel"])


def test_drop_columns_equals_a_teacher_that_rules_the_columns_out():
    """n = 3, m = 9, k = 2: a teacher score of -1e30 has probability exactly 0 in float64, so the plain formula gives the same
    loss and student gradient (to 1e-12).  The plain call's teacher gradient is not compared: torch's softmax backward
    multiplies kl_div's -inf (the log of a zero target) by that zero and returns NaN for the whole row, which is why masked
    rows need ``drop_columns`` at all."""
    g = torch.Generator().manual_seed(11)
    n, m, k, T = 3, 9, 2, 1.5
    s, t = torch.randn(n, m, generator=g, dtype=torch.float64) * 3, torch.randn(n, m, generator=g, dtype=torch.float64) * 3
    ruled_out = t.clone()
    ruled_out[:, m - k:] = -1e30
    loss, ds, dt = U.kl_reference(s, t, T, drop_columns=k)
    loss_plain, ds_plain, _ = U.kl_reference(s, ruled_out, T)
    assert abs(loss.item() - loss_plain.item()) <= 1e-12
    np.testing.assert_allclose(ds.numpy(), ds_plain.numpy(), rtol=0, atol=1e-12)
    assert ds.shape == dt.shape == (n, m) and not dt[:, m - k:].any() and dt[:, :m - k].abs().min() > 0
    p = torch.softmax(s / T, dim=1)  # a dropped column's student gradient: p / (n m T), from the softmax over the whole row
    np.testing.assert_allclose(ds[:, m - k:].numpy(), (p[:, m - k:] / (n * m * T)).numpy(), rtol=0, atol=1e-15)
    # (and the sum is divided by n * m, not by n * (m - k): not the plain call on the narrower matrices)
    narrow, _, _ = U.kl_reference(s[:, :m - k], t[:, :m - k], T)
    assert abs(loss.item() - narrow.item()) > 1e-3


def test_kl_reference_dtype_argument():
    g = torch.Generator().manual_seed(12)
    s, t = torch.randn(4, 6, generator=g), torch.randn(4, 6, generator=g)
    loss32, ds32, dt32 = U.kl_reference(s, t, 2.0, dtype=torch.float32)
    loss64, ds64, dt64 = U.kl_reference(s, t, 2.0)
    assert loss32.dtype == ds32.dtype == dt32.dtype == torch.float32 and loss64.dtype == ds64.dtype == torch.float64
    want = torch.mean(torch.nn.functional.kl_div(torch.log_softmax(s / 2.0, 1), torch.softmax(t / 2.0, 1), reduction="none"))
    assert loss32.item() == want.item()
    np.testing.assert_allclose(ds32.numpy(), ds64.numpy(), rtol=0, atol=1e-7)
    np.testing.assert_allclose(dt32.numpy(), dt64.numpy(), rtol=0, atol=1e-7)


@pytest.mark.parametrize("name,hidden,gamma", sorted(set(U.GRID_STUDENTS) | {("pRotatE", 65, 9.0), ("pRotatE", 300, 9.0),
                                                                        ("pRotatE", 1000, 9.0), ("pRotatE", 257, 6.0)}))
def test_grid_tables_hold_their_assertions(name, hidden, gamma):
    """Every (model, hidden, gamma) the end-to-end cases put on grid tables, and the four pRotatE shapes the helper was
    checked at when it was written.  The tables themselves: odd multiples of 2**-14 in range, every h + r - t a non-zero
    multiple that float32 holds exactly and that stays 1e-5 clear of pRotatE's kinks."""
    ent, rel = U.grid_tables(name, 40, 7, hidden, gamma, seed=3)
    assert ent.shape == (40, hidden) and rel.shape == (7, hidden) and ent.dtype == rel.dtype == torch.float32
    rng = U.scoring.Tables(name, hidden, gamma, None, None).embedding_range
    for table in (ent, rel):
        q = table.double() * 2.0 ** 14
        assert (q == q.round()).all() and (q.long() % 2 == 1).all() and table.abs().max() <= rng
    assert len(torch.unique(ent)) > min(8, int(rng * 2 ** 14) // 2)  # (spread over the grid, not a constant)
    x32 = (ent[:20, None, None, :] + rel[None, :, None, :]) - ent[None, None, 20:, :]
    x64 = (ent.double()[:20, None, None, :] + rel.double()[None, :, None, :]) - ent.double()[None, None, 20:, :]
    assert (x32.double() == x64).all() and (x64 != 0).all()
    if name == "pRotatE":
        assert min(float((x64.abs() - j * rng).abs().min()) for j in (1, 2, 3)) >= 1e-5
    again = U.grid_tables(name, 40, 7, hidden, gamma, seed=3)
    assert torch.equal(again[0], ent) and torch.equal(again[1], rel)


def test_grid_tables_refuse_a_grid_that_meets_a_kink():
    """hidden 4, gamma 1: the range is 0.75, itself an odd multiple of 2**-2, so h + r - t can sit on the first kink."""
    with pytest.raises(AssertionError, match="kink"):
        U.grid_tables("pRotatE", 4, 2, 4, 1.0, seed=0, bits=2)
    U.grid_tables("TransE", 4, 2, 4, 1.0, seed=0, bits=2)  # (TransE's only kink is 0, which no odd multiple is)
