"""-m gpu: the distillation path at training shapes against the float64 reference of tests/util_distill.py (anchored to the
live reference's captures by tests/test_host_distill_reference.py).

  * ``mkb_kl_divergence`` through the C ABI at the edges of its launches -- 4 rows per workgroup, the 64-lane loop over the
    candidates, the finish kernel's stride of 256 rows -- with bounds RELATIVE to the gradients' size (at a training shape the
    entries are ~1e-5: an absolute 1e-6 would pass a kernel that is wrong by 10 %), underflowing and -inf teacher entries, and
    ``losses.KlDivergence`` for the autograd wiring;
  * ``Distillation.distill`` end to end on two partly overlapping synthetic graphs with several hundred rows per KL call and
    hidden sizes on the one-pass backward's strides, teacher -> student across the five models.

Every case prints its error as a fraction of its bound (``-s``; a line starting with ``r15``): profiles/r15_distill_parity_vs_float64.txt
is one run of this file."""
import numpy as np
import pytest
import torch

import util_distill as U

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS32 = float(np.finfo(np.float32).eps)  # 2**-23
JUNK = -7.0e33


# ---------------------------------------------------------------------------------------------- the KL kernel
def _kl_call(student, teacher, T, with_dteacher=True):
    """One mkb_kl_divergence call on fresh buffers pre-filled with junk, 64 floats longer than the kernel may touch.
    -> (loss float32 scalar, dstudent [n, m], dteacher [n, m] or None) as numpy."""
    from mkb_amd import _hip

    n, m = student.shape
    s = student.to(DEV, torch.float32).contiguous()
    t = teacher.to(DEV, torch.float32).contiguous()
    loss = torch.full((1 + 64,), JUNK, dtype=torch.float32, device=DEV)
    ds = torch.full((n * m + 64,), JUNK, dtype=torch.float32, device=DEV)
    dt = torch.full((n * m + 64,), JUNK, dtype=torch.float32, device=DEV) if with_dteacher else None
    scratch = torch.full((n + 64,), JUNK, dtype=torch.float32, device=DEV)
    _hip.check(_hip.lib().mkb_kl_divergence(_hip.ptr(s), _hip.ptr(t), n, m, float(T), _hip.ptr(loss), _hip.ptr(ds), _hip.ptr(dt),
                                            _hip.ptr(scratch), _hip.stream_ptr()), "mkb_kl_divergence")
    for name, buf, used in (("loss", loss, 1), ("dstudent", ds, n * m), ("dteacher", dt, n * m), ("scratch", scratch, n)):
        if buf is not None:
            assert bool((buf[used:] == JUNK).all()), f"{name}: written behind its {used} floats"
            assert not bool((buf[:used] == JUNK).any()), f"{name}: an element was left unwritten"
    return (loss[:1].cpu().numpy()[0], ds[:n * m].reshape(n, m).cpu().numpy(),
            None if dt is None else dt[:n * m].reshape(n, m).cpu().numpy())


def _logit_size(student, teacher, T):
    """L: the largest finite logit |s| / T, |t| / T of the case."""
    both = torch.cat([student.reshape(-1), teacher.reshape(-1)]).double().abs()
    return float(both[torch.isfinite(both)].max()) / T


def _fraction(got, ref, L):
    """max |got - ref| as a fraction of the gradient bound 4 eps32 (1 + L) max|ref|.  The model: a float32 logit of size L
    carries an absolute error of about eps32 L, which passes through exp as a relative error of that size; 4 is the margin for
    the device's expf / logf being within an ulp where the host rounds correctly."""
    ref = np.asarray(ref, dtype=np.float64)
    err = float(np.abs(np.asarray(got, dtype=np.float64) - ref).max())
    bound = 4 * EPS32 * (1 + L) * float(np.abs(ref).max())
    return err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))


def _loss_fraction(loss, loss64):
    """|loss - loss64| as a fraction of 1e-6 max(1, |loss64|), the bound mkb_amd/csrc/kl.hip's header names."""
    return abs(float(loss) - float(loss64)) / (1e-6 * max(1.0, abs(float(loss64))))


def _check_kl(student, teacher, T, tag, drop_columns=0):
    """The checks every KL case gets.  -> (loss, dstudent, dteacher) of the kernel and the float64 reference's."""
    ref = U.kl_reference(student, teacher, T, drop_columns=drop_columns)
    assert all(bool(torch.isfinite(r).all()) for r in ref), "the float64 reference itself is not finite"
    assert _well_conditioned(student, teacher, T, ref)
    loss, ds, dt = _kl_call(student, teacher, T)
    L = _logit_size(student, teacher, T)
    fl, fs, ft = _loss_fraction(loss, ref[0]), _fraction(ds, ref[1].numpy(), L), _fraction(dt, ref[2].numpy(), L)
    print(f"r15 kl {tag} shape=({student.shape[0]}, {student.shape[1]}) T={T} L={L:.0f} |loss|={abs(float(ref[0])):.3g} "
          f"fraction of bound: loss={fl:.3f} dstudent={fs:.3f} dteacher={ft:.3f}")
    assert np.isfinite(ds).all() and np.isfinite(dt).all()
    assert fl <= 1, f"loss {loss!r} against {float(ref[0])!r}: {fl:.2f} of 1e-6 max(1, |loss|)"
    assert fs <= 1, f"dstudent at {fs:.2f} of 4 eps32 (1 + L) max|ref|"
    assert ft <= 1, f"dteacher at {ft:.2f} of 4 eps32 (1 + L) max|ref|"
    # run to run: fixed-order sums, so a second identical call is bit-identical
    loss2, ds2, dt2 = _kl_call(student, teacher, T)
    assert loss2.tobytes() == loss.tobytes() and ds2.tobytes() == ds.tobytes() and dt2.tobytes() == dt.tobytes()
    # a teacher without gradient passes a null dteacher: same loss, same dstudent, bit for bit
    loss0, ds0, dt0 = _kl_call(student, teacher, T, with_dteacher=False)
    assert dt0 is None and loss0.tobytes() == loss.tobytes() and ds0.tobytes() == ds.tobytes()
    return (loss, ds, dt), ref


KL_SHAPES = [(1, 1), (1, 2),                            # the smallest
             (4, 64), (5, 65), (3, 63),                 # 4 rows per workgroup, 64 lanes per row
             (255, 7), (256, 7), (257, 7), (513, 3),    # the finish kernel's stride of 256 rows
             (1027, 130),                               # both at once
             (2, 1000),                                 # many trips of the lane loop
             (1300, 20)]                                # a training shape


def _well_conditioned(student, teacher, T, ref=None):
    """Whether a bound relative to the LARGEST reference entry of each gradient is one a float32 kernel can meet and the float64
    reference can judge.  Read off the float64 reference alone, never off the kernel's output.

      * dstudent = (p - t) / (n m T).  The float32 inputs alone (s * (1 / T), rounded) move p and t by a relative eps32 L each:
        where p ~ t in every entry, nothing in float32 meets a bound relative to |p - t|.  Asked for: somewhere the two
        distributions differ by half of the larger probability, max |p - t| >= max(p, t) / 2.  For a single row of two
        candidates this also keeps the teacher gradient t1 t2 (y1 - y2) off its own cancellation (|p1 - t1| >= 1/4 implies
        |y1 - y2| >= 1).
      * dteacher = t (d - KL_i) / (n m T), d = log t - log p.  Autograd evaluates it in that form, so where every teacher row
        is peaked (t_r ~ 1, KL_i ~ d_r) float64 itself is left with an absolute error of about eps64 (1 + L) / (n m T) -- on
        a row of two candidates 59 logits apart it returned 0.0 for an entry that is 5.05e-20.  Asked for: that error is below
        1 % of the bound 4 eps32 (1 + L) max|ref|, i.e. max|ref| >= 100 (eps64 / eps32) / (n m T).

    Any case with more than a handful of rows holds both at its first draw.  (One candidate: both gradients are exactly 0.)"""
    n, m = student.shape
    if m == 1:
        return True
    if ref is None:
        ref = U.kl_reference(student, teacher, T)
    p = torch.softmax(student.double() / T, dim=1)
    t = torch.softmax(torch.nan_to_num(teacher.double(), neginf=-1e300) / T, dim=1)
    eps64 = float(np.finfo(np.float64).eps)
    return (float((p - t).abs().max()) >= 0.5 * float(torch.maximum(p, t).max())
            and float(ref[2].abs().max()) >= 100 * (eps64 / EPS32) / (n * m * T))


def _randn_scores(n, m, T, scale):
    """student, teacher = randn * scale, redrawn from the same stream until ``_well_conditioned``."""
    g = torch.Generator().manual_seed(100003 * n + 101 * m + int(10 * T) + scale)
    for _ in range(200):
        student, teacher = torch.randn(n, m, generator=g) * scale, torch.randn(n, m, generator=g) * scale
        if _well_conditioned(student, teacher, T):
            return student, teacher
    raise AssertionError("no well-conditioned draw")


@pytest.mark.parametrize("n,m", KL_SHAPES)
def test_kl_kernel_vs_float64(n, m):
    from mkb_amd import losses

    for T in (0.5, 1.0, 2.5):
        for scale in (3, 40):
            student, teacher = _randn_scores(n, m, T, scale)
            (loss, ds, dt), _ = _check_kl(student, teacher, T, f"randn*{scale}")
            # the autograd wiring: losses.KlDivergence hands out the same numbers (an upstream gradient of 1 changes no bit)
            s, t = student.to(DEV).requires_grad_(True), teacher.to(DEV).requires_grad_(True)
            out = losses.KlDivergence()(student_score=s, teacher_score=t, T=T)
            out.backward()
            assert out.dtype == torch.float32 and out.shape == () and out.item() == loss
            assert s.grad.cpu().numpy().tobytes() == ds.tobytes() and t.grad.cpu().numpy().tobytes() == dt.tobytes()
            s2 = student.to(DEV).requires_grad_(True)  # a teacher that needs no gradient gets none
            t2 = teacher.to(DEV)
            out2 = losses.KlDivergence()(student_score=s2, teacher_score=t2, T=T)
            out2.backward()
            assert out2.item() == loss and s2.grad.cpu().numpy().tobytes() == ds.tobytes() and t2.grad is None


EDGE_SHAPES = [(257, 70), (5, 130)]


@pytest.mark.parametrize("n,m", EDGE_SHAPES)
def test_kl_kernel_underflowing_teacher(n, m):
    """Teacher rows whose spread (max - min) / T lies between 120 and 600: softmax underflows to exactly 0 in float32 for many
    entries (exp(-104) is below the smallest denormal) and in float64 for none (exp(-600) ~ 1e-261).  torch's float32 autograd
    returns NaN for such a teacher on the CPU, so float64 is the only usable reference."""
    for T in (1.0, 2.5):
        g = torch.Generator().manual_seed(7 * n + m + int(10 * T))
        student = torch.randn(n, m, generator=g) * 3
        u = torch.rand(n, m, generator=g)
        u[:, 0], u[:, m - 1] = 0.0, 1.0  # (the row's extremes, wherever the random ones fell)
        spread = 130 + 450 * torch.rand(n, 1, generator=g)  # 130 .. 580, per row
        teacher = ((u - 0.5) * spread * T).float()
        seen = (teacher.double().max(dim=1).values - teacher.double().min(dim=1).values) / T
        assert bool((seen >= 120).all() and (seen <= 600).all())
        (loss, ds, dt), ref = _check_kl(student, teacher, T, "underflow")
        t64 = torch.softmax(teacher.double() / T, dim=1)
        assert bool((t64 > 0).all())  # float64 keeps every entry
        # the kernel's own float32 t: exp(logt) with logt = t / T - max - log(sum).  Wherever the same float32 arithmetic on the
        # host gives logt < -104.5, it is 0 on the device too (expf rounds to 0 below -103.98; logt's own rounding error at
        # this size is ~1e-4), and the gradient there is exactly 0.0 -- not a NaN from 0 * inf, not a denormal.
        logit = teacher * np.float32(1.0 / T)
        shifted = logit - logit.max(dim=1, keepdim=True).values
        logt = shifted - torch.log(torch.exp(shifted).sum(dim=1, keepdim=True))
        surely_zero = (logt < -104.5).numpy()
        assert surely_zero.sum() >= n * m // 10 and (torch.exp(logt).numpy()[surely_zero] == 0).all()
        assert (dt[surely_zero] == 0.0).all()
        assert np.isfinite(dt).all() and np.isfinite(ds).all() and np.isfinite(loss)


@pytest.mark.parametrize("n,m", EDGE_SHAPES)
def test_kl_kernel_masked_candidates(n, m):
    """The last 3 teacher columns are -inf in every row (candidates the teacher rules out): t is 0 there, the entries add
    nothing to the loss, and the student is still pushed away from them by p / (n m T)."""
    k = 3
    for T in (1.0, 2.5):
        g = torch.Generator().manual_seed(11 * n + m + int(10 * T))
        student, teacher = torch.randn(n, m, generator=g) * 3, torch.randn(n, m, generator=g) * 3
        teacher[:, m - k:] = float("-inf")
        (loss, ds, dt), ref = _check_kl(student, teacher, T, "masked", drop_columns=k)
        assert (dt[:, m - k:] == 0.0).all() and not ref[2][:, m - k:].any()
        p = torch.softmax(student.double() / T, dim=1)[:, m - k:] / (n * m * T)
        L = _logit_size(student, teacher, T)
        assert np.abs(ds[:, m - k:] - p.numpy()).max() <= 4 * EPS32 * (1 + L) * float(ref[1].abs().max())
        assert (ds[:, m - k:] > 0).all()


def test_kl_divergence_non_contiguous_student():
    """A student that is a column slice of a wider matrix: the gradient lands in the slice's columns, the others get 0, and
    an upstream gradient of 2 doubles it (exactly: a power of two)."""
    from mkb_amd import losses

    n, m, lo, wide_m, T = 37, 70, 3, 83, 1.5
    g = torch.Generator().manual_seed(5)
    wide0, teacher = torch.randn(n, wide_m, generator=g) * 3, torch.randn(n, m, generator=g) * 3
    _, ref_ds, _ = U.kl_reference(wide0[:, lo:lo + m], teacher, T)
    L = _logit_size(wide0[:, lo:lo + m], teacher, T)
    grads = []
    for factor in (1, 2):
        wide = wide0.to(DEV).requires_grad_(True)
        student = wide[:, lo:lo + m]
        assert not student.is_contiguous()
        loss = losses.KlDivergence()(student_score=student, teacher_score=teacher.to(DEV), T=T)
        (factor * loss).backward()
        grad = wide.grad.cpu().numpy()
        assert not grad[:, :lo].any() and not grad[:, lo + m:].any()
        assert _fraction(grad[:, lo:lo + m], factor * ref_ds.numpy(), L) <= 1
        grads.append(grad)
    assert (2 * grads[0]).tobytes() == grads[1].tobytes()


# ---------------------------------------------------------------------------------------------- Distillation.distill
N_TEACHER, N_STUDENT, N_SHARED, R_TEACHER, R_STUDENT, R_SHARED, ROWS = 400, 350, 300, 23, 19, 15, 330
M_ENTITY, M_RELATION = 70, 12


class RowwiseSampling:
    """An unsupervised candidate sampler: independent random shared candidates for every row (with repeats), no ground truth
    in the lists.  ``Distillation`` then selects the rows of each part on its own rule (head: r and t shared, relation: h and
    t, tail: h and r)."""
    supervised = False
    depends_on_teacher = False

    def __init__(self, batch_size_entity, batch_size_relation, seed):
        self.batch_size_entity, self.batch_size_relation = batch_size_entity, batch_size_relation
        self._g = torch.Generator().manual_seed(seed)

    def _draw(self, mapping, n, size):
        keys, values = torch.tensor(list(mapping.keys())), torch.tensor(list(mapping.values()))
        pick = torch.randint(len(keys), (n, size), generator=self._g)
        return keys[pick], values[pick]

    def get(self, mapping_entities, mapping_relations, positive_sample_size, **kwargs):
        head_t, head_s = self._draw(mapping_entities, positive_sample_size, self.batch_size_entity)
        rel_t, rel_s = self._draw(mapping_relations, positive_sample_size, self.batch_size_relation)
        tail_t, tail_s = self._draw(mapping_entities, positive_sample_size, self.batch_size_entity)
        return head_t, rel_t, tail_t, head_s, rel_s, tail_s


@pytest.fixture(scope="module")
def graphs():
    """Two synthetic graphs.  The teacher knows 400 entities and 23 relations; the student 350 entities, 300 of them shared
    under permuted ids, and 19 relations, 15 shared.  ``sample``: 330 teacher triples, 50 of them (15 %) with one unshared
    part -- head, relation and tail in turn."""
    rs = np.random.RandomState(2024)
    t_ents = {f"e{i}": i for i in range(N_TEACHER)}
    t_rels = {f"r{i}": i for i in range(R_TEACHER)}
    shared_e, shared_r = rs.permutation(N_TEACHER)[:N_SHARED], rs.permutation(R_TEACHER)[:R_SHARED]
    labels_e = [f"e{i}" for i in shared_e] + [f"only_student_e{i}" for i in range(N_STUDENT - N_SHARED)]
    labels_r = [f"r{i}" for i in shared_r] + [f"only_student_r{i}" for i in range(R_STUDENT - R_SHARED)]
    s_ents = {label: int(j) for label, j in zip(labels_e, rs.permutation(N_STUDENT))}
    s_rels = {label: int(j) for label, j in zip(labels_r, rs.permutation(R_STUDENT))}
    alone_e, alone_r = np.setdiff1d(np.arange(N_TEACHER), shared_e), np.setdiff1d(np.arange(R_TEACHER), shared_r)
    sample = np.stack([rs.choice(shared_e, ROWS), rs.choice(shared_r, ROWS), rs.choice(shared_e, ROWS)], axis=1)
    broken = rs.permutation(ROWS)[:50]
    for i, row in enumerate(broken):
        sample[row, i % 3] = rs.choice(alone_r if i % 3 == 1 else alone_e)
    return {"t_ents": t_ents, "s_ents": s_ents, "t_rels": t_rels, "s_rels": s_rels, "sample": torch.as_tensor(sample),
            "shared_e": shared_e, "shared_r": shared_r, "alone_e": alone_e, "alone_r": alone_r}


def _models(pair, seed):
    from util_gpu import make_model

    (t_name, t_hidden, t_gamma), (s_name, s_hidden, s_gamma) = U.PAIRS[pair]
    teacher = make_model(t_name, *U.uniform_tables(t_name, N_TEACHER, R_TEACHER, t_hidden, t_gamma, seed), t_hidden, t_gamma)
    tables = U.grid_tables if s_name in ("TransE", "pRotatE") else U.uniform_tables
    student = make_model(s_name, *tables(s_name, N_STUDENT, R_STUDENT, s_hidden, s_gamma, seed + 1), s_hidden, s_gamma)
    return teacher, student


def _proc(graphs, sampler, seed):
    from mkb_amd import distillation

    if sampler == "uniform":
        sampling = distillation.UniformSampling(batch_size_entity=M_ENTITY, batch_size_relation=M_RELATION, seed=seed)
    else:
        sampling = RowwiseSampling(M_ENTITY, M_RELATION, seed)
    return distillation.Distillation(teacher_entities=graphs["t_ents"], student_entities=graphs["s_ents"],
                                     teacher_relations=graphs["t_rels"], student_relations=graphs["s_rels"], sampling=sampling)


def _grad_fraction(got, ref):
    """max |got - ref| as a fraction of util_gpu.grad_close's default bound, min(1e-5, 2e-4 max|ref|)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max()) / min(1e-5, 2e-4 * max(float(np.abs(ref).max()), 1e-30))


def _distill_and_check(graphs, pair, sampler, sample, seed, expect_parts=U.PARTS, min_rows=257):
    from util_gpu import grad_close

    teacher, student = _models(pair, seed)
    sample_dev = sample.to(DEV)
    # a sampler draws from its own stream: one fresh, equally seeded Distillation per pass gives each the same candidates
    tensors = _proc(graphs, sampler, seed).distillation_tensors(sample_dev, teacher=teacher)
    assert tuple(tensors) == tuple(expect_parts)
    for part, (teacher_x, student_x) in tensors.items():
        assert teacher_x.shape == student_x.shape and teacher_x.shape[0] >= min_rows
        assert teacher_x.shape[1] == (M_RELATION if part == "relation" else M_ENTITY)
    ref = U.distill_reference(None, teacher, student, sample, tensors=tensors)

    score_err = 0.0  # scores: the project's parity bound, 1e-4 absolute, on the same index tensors
    with torch.no_grad():
        for part, (teacher_x, student_x) in tensors.items():
            for model, x, want in ((teacher, teacher_x, ref["teacher_scores"][part]), (student, student_x, ref["student_scores"][part])):
                got = model.distill(x.contiguous()).cpu().numpy()
                score_err = max(score_err, float(np.abs(got - want.numpy()).max()))
                np.testing.assert_allclose(got, want.numpy(), rtol=0, atol=1e-4)

    runs = []
    for _ in range(2):  # the second pass: grads zeroed, a bit-identical loss
        student.zero_grad(set_to_none=True)
        loss = _proc(graphs, sampler, seed).distill(teacher=teacher, student=student, sample=sample_dev)
        loss.backward()
        runs.append((loss.item(), student.entity_embedding.grad.cpu().numpy().copy(), student.relation_embedding.grad.cpu().numpy().copy(),
                     student.modulus.grad.cpu().numpy().copy() if student.name == "pRotatE" else None))
        assert all(p.grad is None for p in teacher.parameters())
    (loss, g_ent, g_rel, g_mod), (loss_again, g_ent_again, g_rel_again, g_mod_again) = runs
    fe, fr = _grad_fraction(g_ent, ref["g_ent"].numpy()), _grad_fraction(g_rel, ref["g_rel"].numpy())
    line = (f"r15 distill {pair} sampler={sampler} parts={'/'.join(f'{p}:{x[0].shape[0]}' for p, x in tensors.items())} "
            f"max score err={score_err:.2e} loss err={abs(loss - ref['loss'].item()):.2e} (loss {ref['loss'].item():.4g}) "
            f"fraction of grad_close's bound: g_ent={fe:.3f} g_rel={fr:.3f}")
    if g_mod is not None:
        line += f" g_modulus rel err={abs(g_mod.item() - ref['g_modulus'].item()) / abs(ref['g_modulus'].item()):.2e}"
    print(line)
    np.testing.assert_allclose(loss, ref["loss"].item(), rtol=0, atol=1e-5)
    grad_close(g_ent, ref["g_ent"].numpy())
    grad_close(g_rel, ref["g_rel"].numpy())
    if g_mod is not None:
        np.testing.assert_allclose(g_mod, ref["g_modulus"].numpy(), rtol=1e-4)
    elif hasattr(student, "modulus"):
        assert student.modulus.grad is None  # RotatE's unused parameter
    assert loss_again == loss  # bit-identical (a python float holds the float32 exactly)
    # the table gradients are sums of float atomics, whose order varies from run to run: close, not bitwise equal
    grad_close(g_ent_again, g_ent)
    grad_close(g_rel_again, g_rel)
    grad_close(g_ent_again, ref["g_ent"].numpy())
    grad_close(g_rel_again, ref["g_rel"].numpy())
    if g_mod is not None:
        np.testing.assert_allclose(g_mod_again, ref["g_modulus"].numpy(), rtol=1e-4)
    return ref


def test_graphs_fixture(graphs):
    """Runs on the device like the rest of the file, but checks the fixture alone: at least 257 fully shared rows, so every KL
    call of the uniform sampler crosses the finish kernel's stride, and about 15 % rows with an unshared part."""
    from mkb_amd import distillation

    proc = distillation.Distillation(graphs["t_ents"], graphs["s_ents"], graphs["t_rels"], graphs["s_rels"],
                                     sampling=distillation.UniformSampling(2, 2, seed=0))
    assert len(proc.mapping_entities) == N_SHARED and len(proc.mapping_relations) == R_SHARED
    assert any(t != s for t, s in proc.mapping_entities.items())  # permuted ids
    available = [proc.available(*row) for row in graphs["sample"].tolist()]
    full = sum(a["head"] for a in available)
    assert full == ROWS - 50 and full >= 257


@pytest.mark.parametrize("pair", list(U.PAIRS))
def test_distill_uniform_sampler(graphs, pair):
    _distill_and_check(graphs, pair, "uniform", graphs["sample"], seed=31 + list(U.PAIRS).index(pair))


@pytest.mark.parametrize("pair", ["TransE300-RotatE257", "DistMult100-pRotatE300"])
def test_distill_rowwise_unsupervised_sampler(graphs, pair):
    """Per-row distinct candidates, and each part over its own rows: a row with an unshared head still distils its head."""
    ref = _distill_and_check(graphs, pair, "rowwise", graphs["sample"], seed=57)
    rows = {part: s.shape[0] for part, s in ref["student_scores"].items()}
    assert rows == {"head": ROWS - 33, "relation": ROWS - 33, "tail": ROWS - 34}  # 50 broken rows: 17 heads, 17 relations, 16 tails


def test_distill_skips_a_part_without_rows(graphs):
    """Unsupervised rule: the relation list of a row needs its head and tail shared.  With an unshared head or tail in every
    row no relation can be distilled, ``distill`` skips that part, and the loss is the sum over the two that remain (rows with
    an unshared head still distil their head, and likewise the tails).  With an unshared relation in every row only the
    relation part remains."""
    rs = np.random.RandomState(9)
    sample = graphs["sample"].clone()
    sample[:, 0], sample[:, 2] = torch.as_tensor(rs.choice(graphs["shared_e"], ROWS)), torch.as_tensor(rs.choice(graphs["shared_e"], ROWS))
    sample[:, 1] = torch.as_tensor(rs.choice(graphs["shared_r"], ROWS))
    no_relation = sample.clone()
    no_relation[:165, 0] = torch.as_tensor(rs.choice(graphs["alone_e"], 165))
    no_relation[165:, 2] = torch.as_tensor(rs.choice(graphs["alone_e"], 165))
    ref = _distill_and_check(graphs, "RotatE130-ComplEx130", "rowwise", no_relation, seed=77, expect_parts=("head", "tail"), min_rows=165)
    assert ref["student_scores"]["head"].shape == ref["student_scores"]["tail"].shape == (165, M_ENTITY)
    only_relation = sample.clone()
    only_relation[:, 1] = torch.as_tensor(rs.choice(graphs["alone_r"], ROWS))
    ref = _distill_and_check(graphs, "RotatE130-ComplEx130", "rowwise", only_relation, seed=78, expect_parts=("relation",))
    assert ref["student_scores"]["relation"].shape == (ROWS, M_RELATION)
