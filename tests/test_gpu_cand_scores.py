"""-m gpu: ``BaseModel.score_candidates`` / ``mkb_cand_score_fwd`` / ``mkb_cand_score_bwd`` -- candidate lists in any one slot of a
triple -- against the route they replace (``model(block)`` on the substituted ``[B, M, 3]`` block: bit-equal scores) and against
autograd of ``oracle.scoring.score`` on float64 leaves (gradients, ``util_gpu.grad_close``'s default bound), the buffers of the C
calls, the fallback for rows too long for the kernels, the row-lazy optimizer's protocol, and ``Distillation.distill`` on top.

Tables stay small (<= 400 entities, <= 23 relations) except in the row-lazy test: ``mkb_amd.optim.Adam(lazy_rows=True)`` steps a
table row-lazily only from 4096 rows on, so that test takes an entity table of exactly 4096 rows of 16 floats."""
import numpy as np
import pytest
import torch

import util_distill as U
from oracle import scoring
from test_gpu_distill_shapes import M_ENTITY, M_RELATION, _models, _proc, graphs  # noqa: F401  (graphs: the module's fixture)
from util_gpu import grad_close, make_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODELS = ["TransE", "RotatE", "ComplEx", "DistMult", "pRotatE"]
PARTS = ["head", "relation", "tail"]
COL = {"head": 0, "relation": 1, "tail": 2}
JUNK = -7.0e33


def _block(sample, cand, part):
    block = sample.unsqueeze(1).repeat(1, cand.shape[1], 1)
    block[:, :, COL[part]] = cand
    return block


def _problem(rs, N, R, B, M, part, pattern="random"):
    """sample [B, 3] and cand [B, M] (CPU int64).  Always: rows with h == t.  ``random``: repeats within a row, the row's own id
    in the list and -- head part -- a candidate equal to the row's tail.  ``one``: a single candidate id for every pair.
    ``distinct``: no two pairs share a candidate where the table has that many rows, else no two candidates of a row do (and M
    is at most the table's size).  ``same_ht``: every row has the same head and tail."""
    n_table = R if part == "relation" else N
    sample = np.stack([rs.randint(N, size=B), rs.randint(R, size=B), rs.randint(N, size=B)], 1).astype(np.int64)
    sample[::3, 2] = sample[::3, 0]
    if pattern == "same_ht":  # (two different entities: with h == t in every row TransE's and pRotatE's entity gradient is 0)
        sample[:, 0], sample[:, 2] = sample[1 % B, 0], (sample[1 % B, 0] + 1 + rs.randint(N - 1)) % N
    cand = rs.randint(n_table, size=(B, M)).astype(np.int64)
    if pattern == "one":
        cand[:] = rs.randint(n_table)
    elif pattern == "distinct":
        if B * M <= n_table:
            cand = rs.permutation(n_table)[: B * M].reshape(B, M).astype(np.int64)
        else:
            assert M <= n_table
            cand = np.stack([rs.permutation(n_table)[:M] for _ in range(B)]).astype(np.int64)
    else:
        if M > 1:
            cand[::2, M - 1] = cand[::2, 0]                 # a repeat within the row
        cand[1::2, M // 2] = sample[1::2, COL[part]]        # the row's own id
        if part == "head":
            cand[::4, 0] = sample[::4, 2]                   # a candidate head that is the row's tail
    return torch.as_tensor(sample), torch.as_tensor(cand)


def _tables(name, N, R, hidden, seed):
    gamma = 9.0 if name in ("TransE", "pRotatE") else 6.0
    make = U.grid_tables if name in ("TransE", "pRotatE") else U.uniform_tables  # no float32 sign flips at a kink (util_distill)
    return make_model(name, *make(name, N, R, hidden, gamma, seed), hidden, gamma)


# ---------------------------------------------------------------------------------------------- forward bits
HIDDEN = [1, 3, 64, 65, 130, 257]                       # both sides of the De % 4 vector path and of the 256-lane stride
SHAPES = [(1, 1), (2, 3), (3, 4), (5, 5), (7, 9), (33, 70)]  # the turns of 4 waves
RELATIONS = [1, 5, 19]


@pytest.mark.parametrize("name", MODELS)
def test_forward_bits_equal_the_block_route(name):
    rs = np.random.RandomState(MODELS.index(name))
    for hi, hidden in enumerate(HIDDEN):
        for bi, (B, M) in enumerate(SHAPES):
            R, N = RELATIONS[(hi + bi) % 3], 37 + 11 * bi
            gamma = 6.0
            model = make_model(name, *U.uniform_tables(name, N, R, hidden, gamma, 100 * hi + bi), hidden, gamma)
            for part in PARTS:
                sample, cand = _problem(rs, N, R, B, M, part)
                with torch.no_grad():
                    want = model(_block(sample, cand, part).to(DEV))
                    unread = sample.clone()
                    unread[:, COL[part]] = 0  # the part's own column is not read
                    got = model.score_candidates(unread.to(DEV), cand.to(DEV), part)
                assert got.shape == (B, M) and got.dtype == torch.float32
                assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes(), (name, hidden, B, M, R, part)
            model.check_ids()


def test_empty_batch_and_out_of_range_candidates():
    model = make_model("TransE", *U.uniform_tables("TransE", 20, 3, 8, 6.0, 1), 8, 6.0)
    out = model.score_candidates(torch.zeros((0, 3), dtype=torch.int64, device=DEV), torch.zeros((0, 4), dtype=torch.int64, device=DEV), "head")
    assert out.shape == (0, 4) and out.requires_grad
    out.sum().backward()
    sample = torch.tensor([[1, 0, 2], [3, 2, 4]], device=DEV)
    good = {"head": [[5, 19], [0, 7]], "relation": [[0, 2], [1, 1]], "tail": [[5, 19], [0, 7]]}
    bad = {"head": ([[5, 20], [0, 7]], "candidate entity id"), "relation": ([[0, 3], [1, 1]], "candidate relation id"),
           "tail": ([[5, 19], [20, 7]], "candidate entity id")}
    with torch.no_grad():
        for part in PARTS:
            model.score_candidates(sample, torch.tensor(good[part], device=DEV), part)
            model.check_ids()  # nothing flagged
            model.score_candidates(sample, torch.tensor(bad[part][0], device=DEV), part)
            with pytest.raises(IndexError, match=bad[part][1]):
                model.check_ids()
            model.check_ids()  # the flags were cleared
        unread = sample.clone()
        unread[:, 1] = 99  # the relation column is not read by the relation part, so not checked either
        model.score_candidates(unread, torch.tensor(good["relation"], device=DEV), "relation")
        model.check_ids()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- backward
BWD_HIDDEN = {"TransE": 257, "RotatE": 257, "ComplEx": 130, "DistMult": 513, "pRotatE": 513}
PAIR_SHAPES = [(9, 7), (16, 4), (13, 5), (43, 3), (107, 3)]  # B * M = 63, 64, 65, 129, 321: the edges of the 64-pair chunks
PATTERNS = ["random", "one", "distinct", "same_ht"]
N_BWD, R_BWD = 400, 23


def _seed(B, M, g):
    """A random dscore of size ~1/16.  ``grad_close``'s bound is absolute, 1e-5, wherever the largest reference entry exceeds
    0.05; a float32 sum of n terms of size s is exact to about sqrt(n) * eps32 * (n ** 0.5 * s), so with up to 321 pairs adding
    into one row (the ``one`` pattern) the entries must stay below ~9 for ANY float32 route to meet it -- standard normal seeds
    put them at ~20 (the block route misses the bound there too), seeds of 1/16 at ~1.  Distillation's own seeds are far smaller
    still (KL gradients, 1e-5 .. 1e-3)."""
    return torch.randn(B, M, generator=g) / 16


def _reference_grads(model, block, dscore):
    """Autograd of oracle.scoring.score on float64 leaves (tests/util_distill.py::_leaves) with the seed ``dscore``."""
    tb, ent, rel, mod = U._leaves(model, True)
    score = scoring.score(tb, block.cpu(), ent=ent, rel=rel, modulus=mod)
    (score * dscore.double().cpu()).sum().backward()
    return ent.grad.numpy(), rel.grad.numpy(), None if mod is None or mod.grad is None else mod.grad.numpy()


def _grads(model):
    g_mod = getattr(model, "modulus", None)
    return (model.entity_embedding.grad.cpu().numpy().copy(), model.relation_embedding.grad.cpu().numpy().copy(),
            None if g_mod is None or g_mod.grad is None else g_mod.grad.cpu().numpy().copy())


def _check_against(model, got, ref):
    grad_close(got[0], ref[0])
    grad_close(got[1], ref[1])
    if model.name == "pRotatE":
        np.testing.assert_allclose(got[2], ref[2], rtol=1e-4)
    else:
        assert got[2] is None  # RotatE's modulus is not used: its .grad stays None


@pytest.mark.parametrize("part", PARTS)
@pytest.mark.parametrize("name", MODELS)
def test_backward_vs_float64_and_the_block_route(name, part):
    hidden = BWD_HIDDEN[name]
    model = _tables(name, N_BWD, R_BWD, hidden, seed=7 + MODELS.index(name))
    rs = np.random.RandomState(31 * MODELS.index(name) + COL[part])
    g = torch.Generator().manual_seed(5)
    for si, (B, M) in enumerate(PAIR_SHAPES):
        for pattern in PATTERNS:
            sample, cand = _problem(rs, N_BWD, R_BWD, B, M, part, pattern)
            dscore = _seed(B, M, g)
            block = _block(sample, cand, part)
            ref = _reference_grads(model, block, dscore)
            model.zero_grad(set_to_none=True)
            score = model.score_candidates(sample.to(DEV), cand.to(DEV), part)
            (score * dscore.to(DEV)).sum().backward()
            got = _grads(model)
            _check_against(model, got, ref)
            if pattern == "random":  # accumulation: a second backward without zero_grad doubles the gradient
                (model.score_candidates(sample.to(DEV), cand.to(DEV), part) * dscore.to(DEV)).sum().backward()
                twice = _grads(model)
                grad_close(twice[0], 2 * ref[0])
                grad_close(twice[1], 2 * ref[1])
                if name == "pRotatE":
                    np.testing.assert_allclose(twice[2], 2 * ref[2], rtol=1e-4)
            # the wiring: the same gradients from the block route on the device
            model.zero_grad(set_to_none=True)
            model(block.to(DEV)).backward(dscore.to(DEV))
            old = _grads(model)
            grad_close(got[0], old[0])
            grad_close(got[1], old[1])
            if name == "pRotatE":
                np.testing.assert_allclose(got[2], old[2], rtol=1e-4)


# ---------------------------------------------------------------------------------------------- buffers, through the C ABI
@pytest.mark.parametrize("part", PARTS)
@pytest.mark.parametrize("name", ["RotatE", "pRotatE"])
def test_buffers_of_the_c_calls(name, part):
    """Score buffer and workspace pre-filled with junk and 64 floats / 256 bytes longer than needed: every score is written,
    nothing behind either is, with a workspace of exactly ``mkb_cand_score_bwd_workspace_bytes`` bytes; the gradient buffers
    are added to, not overwritten."""
    from mkb_amd import _hip

    N, R, hidden = 150, 7, 65
    model = _tables(name, N, R, hidden, seed=3)
    lib, tb = _hip.lib(), model._tables()
    rs = np.random.RandomState(4)
    for B, M in [(1, 1), (5, 5), (33, 70)]:
        sample, cand = _problem(rs, N, R, B, M, part)
        s, c = sample.to(DEV), cand.to(DEV)
        score = torch.full((B * M + 64,), JUNK, dtype=torch.float32, device=DEV)
        _hip.check(lib.mkb_cand_score_fwd(tb, _hip.ptr(s), _hip.ptr(c), B, M, COL[part], _hip.ptr(score), _hip.stream_ptr()), "fwd")
        assert bool((score[B * M:] == JUNK).all()) and not bool((score[:B * M] == JUNK).any())
        with torch.no_grad():
            assert score[:B * M].cpu().numpy().tobytes() == model(_block(sample, cand, part).to(DEV)).cpu().numpy().tobytes()
        need = lib.mkb_cand_score_bwd_workspace_bytes(tb, B, M, COL[part])
        assert need >= 0 and need % 256 == 0
        raw = torch.full((need + 512,), 0x5A, dtype=torch.uint8, device=DEV)
        off = (-raw.data_ptr()) % 256
        ws = raw[off: off + need + 256]
        tails = lambda n: torch.cat([torch.zeros(n, dtype=torch.float32, device=DEV), torch.full((64,), JUNK, dtype=torch.float32, device=DEV)])
        g_ent, g_rel, g_mod = tails(N * model.entity_dim), tails(R * model.relation_dim), tails(1)
        dscore = _seed(B, M, torch.Generator().manual_seed(B)).to(DEV)
        gr = _hip.Grads(g_ent.data_ptr(), g_rel.data_ptr(), g_mod.data_ptr())
        _hip.check(lib.mkb_cand_score_bwd(tb, gr, _hip.ptr(s), _hip.ptr(c), B, M, COL[part], _hip.ptr(dscore), _hip.ptr(ws), need,
                                          _hip.stream_ptr()), "bwd")
        assert bool((ws[need:] == 0x5A).all()), "written behind the workspace"
        assert bool((g_ent[-64:] == JUNK).all() and (g_rel[-64:] == JUNK).all() and (g_mod[1:] == JUNK).all())
        ref = _reference_grads(model, _block(sample, cand, part), dscore)
        grad_close(g_ent[:-64].reshape(N, -1).cpu().numpy(), ref[0])
        grad_close(g_rel[:-64].reshape(R, -1).cpu().numpy(), ref[1])
        if name == "pRotatE":
            np.testing.assert_allclose(g_mod[0].item(), ref[2].item(), rtol=1e-4)
        else:
            assert g_mod[0].item() == 0.0  # RotatE's modulus gets nothing


# ---------------------------------------------------------------------------------------------- fallback
@pytest.mark.parametrize("part", PARTS)
def test_rows_too_long_for_the_kernel_fall_back_to_the_block_route(part):
    """(2 + 4) * 2731 * 4 bytes > 64 KB: ``mkb_cand_score_fwd`` answers MKB_ERR_UNSUPPORTED and ``score_candidates`` scores the
    substituted block with the general kernels: their bits, their gradients."""
    from mkb_amd import _hip

    N, R, hidden, B, M = 8, 2, 2731, 3, 5
    model = _tables("TransE", N, R, hidden, seed=11)
    rs = np.random.RandomState(12)
    sample, cand = _problem(rs, N, R, B, M, part)
    s, c = sample.to(DEV), cand.to(DEV)
    out = torch.empty((B, M), dtype=torch.float32, device=DEV)
    assert _hip.lib().mkb_cand_score_fwd(model._tables(), _hip.ptr(s), _hip.ptr(c), B, M, COL[part], _hip.ptr(out), _hip.stream_ptr()) == _hip.ERR_UNSUPPORTED
    dscore = _seed(B, M, torch.Generator().manual_seed(1)).to(DEV)
    block = _block(sample, cand, part).to(DEV)
    want = model(block)
    want.backward(dscore)
    old = _grads(model)
    model.zero_grad(set_to_none=True)
    got = model.score_candidates(s, c, part)
    assert got.detach().cpu().numpy().tobytes() == want.detach().cpu().numpy().tobytes()
    got.backward(dscore)
    new = _grads(model)
    grad_close(new[0], old[0])
    grad_close(new[1], old[1])
    ref = _reference_grads(model, block, dscore)
    grad_close(new[0], ref[0])
    grad_close(new[1], ref[1])


# ---------------------------------------------------------------------------------------------- row-lazy Adam
def test_three_steps_with_the_row_lazy_optimizer():
    """loss = sum over the parts of (score_candidates(...) * w).sum(), three steps, ``mkb_amd.optim.Adam`` with and without
    ``lazy_rows``: the same scores of a probe block afterwards, an entity and a relation that occur only as candidates have
    moved in both runs, and the lazy optimizer is still on its row-lazy route (observed as in
    tests/test_gpu_defer.py::test_readme_loop_keeps_the_row_lazy_route)."""
    from mkb_amd import _links, optim

    N, R, hidden, B, Me, Mr = 4096, 23, 16, 32, 6, 4
    only_e, only_r = N - 1, R - 1  # never a head, relation or tail of a sample
    rs = np.random.RandomState(8)
    steps = []
    for _ in range(3):
        sample = torch.as_tensor(np.stack([rs.randint(N - 1, size=B), rs.randint(R - 1, size=B), rs.randint(N - 1, size=B)], 1))
        ce, cr, ct = (torch.as_tensor(rs.randint(N - 1, size=(B, Me))), torch.as_tensor(rs.randint(R - 1, size=(B, Mr))),
                      torch.as_tensor(rs.randint(N - 1, size=(B, Me))))
        ce[3, 2], cr[5, 1], ct[7, 0] = only_e, only_r, only_e
        w = {p: torch.as_tensor(rs.rand(B, Mr if p == "relation" else Me).astype(np.float32) + 0.5) for p in PARTS}
        steps.append((sample.to(DEV), {"head": ce.to(DEV), "relation": cr.to(DEV), "tail": ct.to(DEV)}, {p: x.to(DEV) for p, x in w.items()}))
    probe = torch.as_tensor(np.stack([rs.randint(N, size=64), rs.randint(R, size=64), rs.randint(N, size=64)], 1))
    probe[0] = torch.tensor([only_e, only_r, 5])
    probe = probe.to(DEV)

    def run(lazy):
        model = make_model("RotatE", *U.uniform_tables("RotatE", N, R, hidden, 6.0, 21), hidden, 6.0)
        before = model.entity_embedding[only_e].detach().clone(), model.relation_embedding[only_r].detach().clone()
        opt = optim.Adam([model.entity_embedding, model.relation_embedding], lr=1e-2, lazy_rows=lazy)
        for sample, cands, w in steps:
            opt.zero_grad()
            loss = sum((model.score_candidates(sample, cands[p], p) * w[p]).sum() for p in PARTS)
            loss.backward()
            opt.step()
        if lazy:
            st = opt.state[model.entity_embedding]
            assert "last" in st and _links.owner(model.entity_embedding) is opt, "the optimizer fell back to the dense kernel"
            assert not _links.autograd_wrote(model.entity_embedding)
            opt.flush()
        model.check_ids()
        assert float((model.entity_embedding[only_e].detach() - before[0]).abs().max()) > 1e-3
        assert float((model.relation_embedding[only_r].detach() - before[1]).abs().max()) > 1e-3
        with torch.no_grad():
            return model(probe).cpu().numpy()

    np.testing.assert_allclose(run(True), run(False), rtol=0, atol=1e-4)


# ---------------------------------------------------------------------------------------------- Distillation.distill
SAMPLER = {"TransE300-RotatE257": "rowwise", "RotatE130-ComplEx130": "uniform", "ComplEx64-DistMult513": "rowwise",
           "DistMult100-pRotatE300": "uniform", "pRotatE65-TransE1000": "uniform"}  # one PAIRS entry per student model


@pytest.mark.parametrize("routes", ["kernel", "shipped"])
@pytest.mark.parametrize("pair", list(U.PAIRS))
def test_distill_keeps_its_loss_bits_and_meets_float64(graphs, pair, routes, monkeypatch):  # noqa: F811
    """``Distillation.distill`` with every part on ``score_candidates`` (``kernel``) and with the routing as shipped: the loss is
    bit-equal to the sum of ``KlDivergence`` over ``model.distill(block)`` scores, the student's gradients meet ``grad_close``
    against ``util_distill.distill_reference``."""
    from mkb_amd import distillation, losses

    if routes == "kernel":
        monkeypatch.setattr(distillation.Distillation, "SLOT_KERNEL_ROUTES", {name: tuple(PARTS) for name in MODELS})
    seed, sampler = 41 + list(U.PAIRS).index(pair), SAMPLER[pair]
    teacher, student = _models(pair, seed)
    sample = graphs["sample"]
    sample_dev = sample.to(DEV)
    tensors = _proc(graphs, sampler, seed).distillation_tensors(sample_dev, teacher=teacher)
    assert tuple(tensors) == tuple(PARTS)
    with torch.no_grad():
        kl = losses.KlDivergence()
        want = 0
        for teacher_x, student_x in tensors.values():
            want = want + kl(teacher_score=teacher.distill(teacher_x.contiguous()), student_score=student.distill(student_x.contiguous()))
    student.zero_grad(set_to_none=True)
    loss = _proc(graphs, sampler, seed).distill(teacher=teacher, student=student, sample=sample_dev)
    assert loss.item() == want.item()
    loss.backward()
    assert all(p.grad is None for p in teacher.parameters())
    ref = U.distill_reference(None, teacher, student, sample, tensors=tensors)
    grad_close(student.entity_embedding.grad.cpu().numpy(), ref["g_ent"].numpy())
    grad_close(student.relation_embedding.grad.cpu().numpy(), ref["g_rel"].numpy())
    if student.name == "pRotatE":
        np.testing.assert_allclose(student.modulus.grad.cpu().numpy(), ref["g_modulus"].numpy(), rtol=1e-4)
    elif hasattr(student, "modulus"):
        assert student.modulus.grad is None
