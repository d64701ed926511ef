"""The float64 reference of the distillation path, in plain torch on the CPU (TEST INFRASTRUCTURE ONLY): ``losses.KlDivergence``
(``kl_reference``), ``distillation.Distillation.distill`` (``distill_reference``), and tables on which a float32 kernel and a
float64 reference cannot disagree about the side of a kink (``grid_tables``).  tests/test_host_distill_reference.py anchors
the first two to the captures of the live reference before anything on the device is compared with them."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import scoring

PARTS = ("head", "relation", "tail")


def kl_reference(student, teacher, T, dtype=torch.float64, drop_columns=0):
    """-> (loss, dstudent, dteacher) of ``mean(kl_div(log_softmax(s / T, 1), softmax(t / T, 1), reduction="none"))`` by autograd
    on copies of the inputs in ``dtype``.

    ``drop_columns=k``: the reference for rows whose last ``k`` teacher entries are -inf (candidates the teacher rules out).
    The teacher's distribution is the softmax of the remaining columns and the dropped ones contribute nothing (their t is 0);
    the student's log-softmax still runs over the whole row, and the sum is still divided by n * m.  The gradients keep the
    inputs' shape: dteacher is zero in the dropped columns, dstudent is p / (n m T) there."""
    s = torch.as_tensor(student).detach().cpu().to(dtype).clone().requires_grad_(True)
    t = torch.as_tensor(teacher).detach().cpu().to(dtype).clone().requires_grad_(True)
    n, m = s.shape
    keep = m - int(drop_columns)
    assert 0 < keep <= m
    terms = F.kl_div(torch.log_softmax(s / T, dim=1)[:, :keep], torch.softmax(t[:, :keep] / T, dim=1), reduction="none")
    loss = terms.sum() / (n * m)  # (= torch.mean(terms) without dropped columns)
    loss.backward()
    return loss.detach(), s.grad, t.grad


def _leaves(model, grad):
    """float64 copies of a model's float32 tables (and modulus): autograd leaves when ``grad``."""
    leaf = lambda p: p.detach().cpu().to(torch.float64).clone().requires_grad_(grad)
    modulus = getattr(model, "modulus", None)
    tb = scoring.Tables(model.name, model.hidden_dim, float(model.gamma.item()), None, None, None)
    return tb, leaf(model.entity_embedding), leaf(model.relation_embedding), None if modulus is None else leaf(modulus)


def distill_reference(proc, teacher, student, sample, tensors=None):
    """``proc.distill(teacher, student, sample)`` in float64 on the CPU, from the index tensors the device path builds
    (``proc.distillation_tensors``: deterministic; pass ``tensors`` to reuse the ones of an earlier call -- a sampler with a
    random stream gives other candidates on its next call).  Scores by ``oracle.scoring.score`` on float64 leaves made from the
    models' float32 tables, the formula of ``kl_reference`` per part, the parts summed.

    -> dict(loss, g_ent, g_rel, g_modulus (pRotatE students, else None), teacher_scores / student_scores {part: [n, m]})."""
    if tensors is None:
        tensors = proc.distillation_tensors(sample, teacher=teacher)
    tb_t, ent_t, rel_t, mod_t = _leaves(teacher, False)
    tb_s, ent_s, rel_s, mod_s = _leaves(student, True)
    loss, teacher_scores, student_scores = 0, {}, {}
    for part, (teacher_x, student_x) in tensors.items():
        with torch.no_grad():
            ts = scoring.score(tb_t, teacher_x.cpu(), ent=ent_t, rel=rel_t, modulus=mod_t)
        ss = scoring.score(tb_s, student_x.cpu(), ent=ent_s, rel=rel_s, modulus=mod_s)
        loss = loss + torch.mean(F.kl_div(torch.log_softmax(ss, dim=1), torch.softmax(ts, dim=1), reduction="none"))
        teacher_scores[part], student_scores[part] = ts, ss.detach()
    if tensors:
        loss.backward()
    zero = lambda leaf: torch.zeros_like(leaf) if leaf.grad is None else leaf.grad
    return {"loss": torch.as_tensor(loss, dtype=torch.float64).detach(), "g_ent": zero(ent_s), "g_rel": zero(rel_s),
            "g_modulus": zero(mod_s) if student.name == "pRotatE" else None,
            "teacher_scores": teacher_scores, "student_scores": student_scores}


def uniform_tables(name, N, R, hidden, gamma, seed):
    """The usual tables: uniform in the model's embedding range (models/base.py), float32."""
    g = torch.Generator().manual_seed(seed)
    de, dr = scoring.dims(name, hidden)
    rng = scoring.Tables(name, hidden, gamma, None, None).embedding_range
    return (torch.rand(N, de, generator=g) * 2 - 1) * rng, (torch.rand(R, dr, generator=g) * 2 - 1) * rng


def grid_tables(name, N, R, hidden, gamma, seed, bits=14):
    """Entity and relation tables for a TransE or pRotatE student whose entries are random odd multiples of 2**-bits inside the
    model's embedding range.  Every element h + r - t is then an odd multiple of 2**-bits as well: never 0, and exact in
    float32 (as are both partial sums), so TransE's |.| never sits at its kink and float32 and float64 see the same sign.
    pRotatE's |sin(x / (range / pi))| has its kinks at x = j * range: asserted here, in float64, that every reachable odd
    multiple keeps at least 1e-5 from them (j = 1 .. 3; |x| <= 3 * range).

    Why: on ordinary random tables a float32 sign flip at a kink is expected about once per 1e7 elements, and one flip moves a
    gradient element by 2 |dscore| -- thousands of times the gradient tolerance -- so a correct kernel would fail by chance.
    (RotatE's kink needs both components of a complex difference within rounding of 0 at once: negligible, no grid needed.
    DistMult and ComplEx have none.)"""
    assert name in ("TransE", "pRotatE"), name
    step = 2.0 ** -bits
    rng = scoring.Tables(name, hidden, gamma, None, None).embedding_range  # the float32 value the model holds, as a double
    K = int((rng / step + 1) // 2)  # odd multiples (2k + 1) * step, k in [-K, K): the largest is (2K - 1) * step <= rng
    assert K >= 2 and (2 * K - 1) * step <= rng, (hidden, gamma, bits)
    reach = np.arange(1, 3 * (2 * K - 1) + 1, 2, dtype=np.float64) * step  # |h + r - t|, by symmetry the positive ones
    assert reach.min() > 0
    if name == "pRotatE":
        gap = min(float(np.abs(reach - j * rng).min()) for j in (1, 2, 3))
        assert gap >= 1e-5, f"an element can come within {gap:.3g} of a kink of |sin| (hidden {hidden}, gamma {gamma})"
    rs = np.random.RandomState(seed)
    ent = (2 * rs.randint(-K, K, size=(N, hidden)) + 1) * step
    rel = (2 * rs.randint(-K, K, size=(R, hidden)) + 1) * step
    ent32, rel32 = ent.astype(np.float32), rel.astype(np.float32)
    assert (ent32 == ent).all() and (rel32 == rel).all() and np.abs(ent).max() <= rng and np.abs(rel).max() <= rng
    return torch.from_numpy(ent32), torch.from_numpy(rel32)


# The teacher -> student pairs of the end-to-end cases (tests/test_gpu_distill_shapes.py): (model, hidden, gamma) each.  The
# hidden sizes sit on the one-pass backward's stride of 256 elements (257, 513, 1000, 300; De = 260 for ComplEx 130) and on
# both sides of its De % 4 vector path.  TransE and pRotatE students take grid tables.
PAIRS = {
    "TransE300-RotatE257": (("TransE", 300, 9.0), ("RotatE", 257, 6.0)),
    "RotatE130-ComplEx130": (("RotatE", 130, 6.0), ("ComplEx", 130, 6.0)),
    "ComplEx64-DistMult513": (("ComplEx", 64, 6.0), ("DistMult", 513, 6.0)),
    "DistMult100-pRotatE300": (("DistMult", 100, 6.0), ("pRotatE", 300, 9.0)),
    "pRotatE65-TransE1000": (("pRotatE", 65, 9.0), ("TransE", 1000, 9.0)),
}
GRID_STUDENTS = sorted({student for _, student in PAIRS.values() if student[0] in ("TransE", "pRotatE")})
