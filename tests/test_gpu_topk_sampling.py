"""-m gpu: the candidate mask and block selection of the top-k kernel (mkb_topk_masked, mkb_topk_block in mkb_amd/csrc/rank.hip)
and the teacher top-k samplers built on them (distillation.TopKSampling / FastTopKSampling).

Kernel answers are restated independently: a stable descending sort (NaN first, then higher score, then lower id) of the device's
own all-entity scores with the non-candidate and filtered columns removed (test_gpu_topk.expected_topk).  Sampler answers are
compared with captures of the live reference (tools/make_golden.py::gen_topk_sampling), whose recorded k-th / (k+1)-th score
gaps are all above 1e-4, so that an fp32 near-tie cannot reorder them."""
import collections
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_topk import MODELS, _fb15k237, assert_topk_equal, excluded_columns, expected_topk  # noqa: E402
from util_gpu import grad_close, make_model  # noqa: E402


def _call(m, triples, mode, k, keys, flags, bits, masked=True):
    """mkb_topk_masked (masked=True; bits may be None = a null mask) or mkb_topk on all rows at once."""
    from mkb_amd import _hip

    s = torch.as_tensor(np.asarray(triples, dtype=np.int64)).cuda().contiguous()
    B = s.shape[0]
    ids = torch.empty((B, k), dtype=torch.int64, device="cuda")
    sc = torch.empty((B, k), dtype=torch.float32, device="cuda")
    lib, tb = _hip.lib(), m._tables()
    need = lib.mkb_topk_workspace_bytes(tb, B, k)
    ws = torch.empty(need + 256, dtype=torch.uint8, device="cuda")
    w = ctypes.c_void_p(ws.data_ptr() + (-ws.data_ptr()) % 256)
    kp = _hip.ptr(keys) if keys is not None else None
    nk = keys.numel() if keys is not None else 0
    if masked:
        rc = lib.mkb_topk_masked(tb, _hip.ptr(s), B, _hip.mode_id(mode), kp, nk, _hip.ptr(bits), k, flags, _hip.ptr(ids), _hip.ptr(sc),
                                 w, need, _hip.stream_ptr())
    else:
        rc = lib.mkb_topk(tb, _hip.ptr(s), B, _hip.mode_id(mode), kp, nk, k, flags, _hip.ptr(ids), _hip.ptr(sc), w, need,
                          _hip.stream_ptr())
    _hip.check(rc, "topk")
    return ids, sc


def _umls(name):
    from mkb_amd import datasets, evaluation

    ds = datasets.Umls(batch_size=8, shuffle=False, seed=42, num_workers=0)
    rs = np.random.RandomState(11)
    hidden = 64
    de = 2 * hidden if name in ("RotatE", "ComplEx") else hidden
    dr = 2 * hidden if name == "ComplEx" else hidden
    ent = rs.uniform(-0.2, 0.2, size=(ds.n_entity, de)).astype(np.float32)
    rel = rs.uniform(-0.2, 0.2, size=(ds.n_relation, dr)).astype(np.float32)
    modulus = np.array([[0.1]], dtype=np.float32) if name in ("RotatE", "pRotatE") else None
    m = make_model(name, ent, rel, hidden, 6.0, modulus).eval()
    ev = evaluation.Evaluation(true_triples=ds.true_triples, entities=ds.entities, relations=ds.relations, batch_size=64,
                               device="cuda", num_workers=0)
    return ds, m, ev, np.asarray(ds.test, dtype=np.int64)


@pytest.mark.parametrize("graph", ["umls", "fb15k237"])
@pytest.mark.parametrize("name", MODELS)
def test_null_mask_is_mkb_topk_bit_for_bit(name, graph):
    """A null mask and an all-ones mask give mkb_topk's ids and scores, bit for bit: five models, the three routes, with and
    without the filter and KEEP_TARGET."""
    from mkb_amd import _hip
    from mkb_amd.utils import candidate_bits, true_keys

    ds, m, ev, triples = _umls(name) if graph == "umls" else _fb15k237(name)
    ones = candidate_bits(torch.ones(m.n_entity, dtype=torch.bool), m.n_entity, "cuda")
    for mode in ("head-batch", "tail-batch"):
        keys = true_keys(ds.true_triples, torch.device("cuda"), m.n_entity, m.n_relation)[mode]
        for kk, flags in ((None, 0), (keys, 0), (keys, _hip.TOPK_KEEP_TARGET)):
            for k in (1, 10, 100):
                ref = _call(m, triples, mode, k, kk, flags, None, masked=False)
                for bits in (None, ones):
                    got = _call(m, triples, mode, k, kk, flags, bits)
                    what = f"{name} {graph} {mode} k={k} flags={flags} filter={kk is not None} mask={bits is not None}"
                    assert torch.equal(got[0], ref[0]), what
                    assert torch.equal(got[1].view(torch.int32), ref[1].view(torch.int32)), what


def _check_masks(m, ev, triples, true, N, R, masks, ks=(1, 5, 40)):
    from mkb_amd.utils import predict_top_k
    from oracle import ranking

    keys = ranking.true_key_set(true, N, R) if true is not None else None
    for mode in ("head-batch", "tail-batch"):
        _, dev_scores = ev.ranks(m, triples, mode, with_scores=True)
        dev_scores = dev_scores.cpu().numpy()
        for how in (("keep", "none") if true is not None else ("none",)):
            excl = excluded_columns(triples, keys, N, R, mode, how)
            for label, mask in masks.items():
                want_ids, want_sc = expected_topk(dev_scores, excl | ~mask[None, :], max(ks))
                for k in ks:
                    ids, sc = predict_top_k(m, triples, mode, k, true_triples=ev.true_triples if how == "keep" else None,
                                            keep_target=how == "keep", candidates=torch.as_tensor(mask))
                    assert_topk_equal(ids, sc, want_ids[:, :k], want_sc[:, :k], f"{m.name} {mode} {how} {label} k={k}")


@pytest.mark.parametrize("name", MODELS)
def test_masked_topk_exact_on_umls(name):
    """Umls (135 entities), every test triple: a random 50 % mask, a single candidate, an empty mask (all -1 / -inf), and k past
    the candidates left (padded)."""
    ds, m, ev, triples = _umls(name)
    N = ds.n_entity
    rs = np.random.RandomState(4)
    masks = {"half": rs.rand(N) < 0.5, "one": np.arange(N) == 17, "none": np.zeros(N, dtype=bool), "six": np.isin(np.arange(N), [3, 9, 40, 41, 90, 134])}
    _check_masks(m, ev, triples, np.asarray(ds.true_triples, dtype=np.int64), N, ds.n_relation, masks)
    ids, sc = _call(m, triples, "tail-batch", 3, None, 0, torch.zeros((N + 31) // 32, dtype=torch.int32, device="cuda"))
    assert (ids == -1).all() and torch.isneginf(sc).all()


@pytest.mark.parametrize("name", MODELS)
def test_masked_topk_exact_on_fb15k237(name):
    """256 FB15k-237 test triples at hidden 1000 (all three routes) with a random 50 % mask and a 200-entity mask."""
    ds, m, ev, triples = _fb15k237(name)
    rs = np.random.RandomState(6)
    small = np.zeros(14541, dtype=bool)
    small[rs.choice(14541, 200, replace=False)] = True
    _check_masks(m, ev, triples, np.asarray(ds.true_triples, dtype=np.int64), 14541, 237, {"half": rs.rand(14541) < 0.5, "200": small},
                 ks=(10, 100))


def test_mask_overrides_keep_target():
    """KEEP_TARGET keeps the target past the filter, but not past the mask: a target outside the mask is never returned."""
    from mkb_amd import _hip
    from mkb_amd.utils import candidate_bits, predict_top_k

    ds, m, ev, triples = _umls("RotatE")
    N = ds.n_entity
    for mode, col in (("head-batch", 0), ("tail-batch", 2)):
        target = triples[:, col]
        mask = np.ones(N, dtype=bool)
        mask[np.unique(target)] = False
        ids, _ = predict_top_k(m, triples, mode, 20, true_triples=ds.true_triples, keep_target=True, candidates=torch.as_tensor(mask))
        ids = ids.cpu().numpy()
        assert not (ids == target[:, None]).any()
        assert mask[ids[ids >= 0]].all()
        ids2, _ = _call(m, triples, mode, 20, None, _hip.TOPK_KEEP_TARGET, candidate_bits(torch.as_tensor(mask), N, "cuda"))
        assert not (ids2.cpu().numpy() == target[:, None]).any()


def test_masked_topk_yago_shape():
    """YAGO3-10 shape (N = 123,182: a 15 KB mask), RotatE hidden 64, 48 queries, a random 30 % mask, k = 100."""
    from mkb_amd import evaluation

    N, R, hidden = 123182, 37, 64
    rs = np.random.RandomState(8)
    ent = rs.uniform(-0.2, 0.2, size=(N, 2 * hidden)).astype(np.float32)
    rel = rs.uniform(-0.2, 0.2, size=(R, hidden)).astype(np.float32)
    m = make_model("RotatE", ent, rel, hidden, 6.0, np.array([[0.1]], dtype=np.float32)).eval()
    triples = np.stack([rs.randint(N, size=48), rs.randint(R, size=48), rs.randint(N, size=48)], 1).astype(np.int64)
    ev = evaluation.Evaluation(true_triples=[tuple(t) for t in triples.tolist()], entities={i: i for i in range(N)},
                               relations={i: i for i in range(R)}, batch_size=64, device="cuda", num_workers=0)
    _check_masks(m, ev, triples, None, N, R, {"30": rs.rand(N) < 0.3}, ks=(100,))


def _np_block_topk(S, k):
    B, N = S.shape
    nan = np.isnan(S)
    key = np.where(nan, 0.0, -S.astype(np.float64))
    key = np.where(key == 0.0, 0.0, key)  # -0 and +0 tie
    order = np.lexsort((np.broadcast_to(np.arange(N), (B, N)), key, ~nan), axis=-1)[:, :k]
    ids = np.full((B, k), -1, dtype=np.int64)
    sc = np.full((B, k), -np.inf, dtype=np.float32)
    n = min(k, N)
    ids[:, :n] = order[:, :n]
    sc[:, :n] = np.take_along_axis(S, order[:, :n], axis=1)
    return ids, sc


@pytest.mark.parametrize("B,N,ld,k", [(7, 50, 50, 5), (5, 300, 333, 40), (3, 1, 1, 4), (4, 6, 9, 10), (65, 2000, 2000, 1024),
                                      (2, 5000, 5003, 1)])
def test_block_topk_against_a_numpy_stable_sort(B, N, ld, k):
    """mkb_topk_block on random blocks with NaN, +-0, +-inf, many ties, a row stride past N, N = 1 and N < k."""
    from mkb_amd.utils import topk_block

    rs = np.random.RandomState(B * 1000 + N)
    full = rs.randint(-20, 20, size=(B, ld)).astype(np.float32) / 4  # ties everywhere
    full[rs.rand(B, ld) < 0.05] = np.nan
    full[rs.rand(B, ld) < 0.05] = -0.0
    full[rs.rand(B, ld) < 0.05] = 0.0
    full[rs.rand(B, ld) < 0.02] = np.inf
    full[rs.rand(B, ld) < 0.02] = -np.inf
    dev = torch.as_tensor(full).cuda()
    S = dev[:, :N]
    ids, sc = topk_block(S, k)
    want_ids, want_sc = _np_block_topk(full[:, :N], k)
    np.testing.assert_array_equal(ids.cpu().numpy(), want_ids)
    got = sc.cpu().numpy()
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want_sc))
    ok = ~np.isnan(want_sc)
    np.testing.assert_array_equal(got[ok].view(np.uint32), want_sc[ok].view(np.uint32))  # the block's own values (-0 stays -0)


def test_block_topk_rejects_bad_arguments():
    from mkb_amd import _hip

    lib = _hip.lib()
    S = torch.zeros((4, 8), device="cuda")
    ids = torch.empty((4, 4), dtype=torch.int64, device="cuda")
    sc = torch.empty((4, 4), device="cuda")
    p = _hip.ptr
    assert lib.mkb_topk_block(p(S), 4, 8, 8, 4, p(ids), p(sc), None) == 0
    for args in [(4, 8, 7, 4), (-1, 8, 8, 4), (4, 8, 8, 0), (4, 8, 8, 1025), (4, 0, 8, 4)]:
        assert lib.mkb_topk_block(p(S), *args, p(ids), p(sc), None) == _hip.ERR_INVALID, args
    assert lib.mkb_topk_block(p(S), 4, 8, 8, 4, None, p(sc), None) == _hip.ERR_INVALID
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- samplers
def _model(cls, ent, rel, hidden, gamma, ents, rels):
    from mkb_amd import models

    m = getattr(models, cls)(hidden_dim=hidden, entities=ents, relations=rels, gamma=gamma)
    m._set_params(torch.as_tensor(ent), torch.as_tensor(rel))
    return m.cuda()


def test_capture_gaps_are_clear(golden):
    gj = golden("topk_sampling.json")
    assert min(gj["gaps"].values()) > 1e-4, gj["gaps"]


@pytest.mark.parametrize("cls,hid", [("RotatE", 6), ("ComplEx", 6), ("DistMult", 8)])
def test_topk_sampling_get_vs_reference(golden, cls, hid):
    """CountriesS1, teacher and student the same graph, top 5 entities + 3 random, top 1 relation + 1 random, four batches:
    all six tensors equal the reference's."""
    from mkb_amd import datasets, distillation

    g = golden("topk_sampling.npz")
    ds = datasets.CountriesS1(batch_size=6, seed=42, shuffle=False, num_workers=0)
    teacher = _model(cls, g[f"get/{cls}/ent"], g[f"get/{cls}/rel"], hid, 4, ds.entities, ds.relations)
    sampler = distillation.TopKSampling(teacher_entities=ds.entities, teacher_relations=ds.relations, student_entities=ds.entities,
                                        student_relations=ds.relations, batch_size_entity=5, batch_size_relation=1,
                                        n_random_entities=3, n_random_relations=1, seed=7, device="cuda")
    assert (sampler.batch_size_entity, sampler.batch_size_relation) == (8, 2)
    for j, b in enumerate(g["get/samples"]):
        got = sampler.get(sample=torch.as_tensor(b).cuda(), teacher=teacher)
        for name, x in zip(("head_t", "rel_t", "tail_t", "head_s", "rel_s", "tail_s"), got):
            assert x.dtype == torch.int64 and x.is_cuda
            np.testing.assert_array_equal(x.cpu().numpy(), g[f"get/{cls}/{j}/{name}"], err_msg=f"{cls} batch {j} {name}")


def test_topk_sampling_partly_shared_graphs():
    """Teacher and student share part of their entities / relations under different ids: every returned id is shared, teacher
    ids are in teacher space, student ids are their mapping, and the top k equals a torch sort of the device's own scores."""
    from mkb_amd import distillation

    rs = np.random.RandomState(2)
    t_ents = {f"e{i}": i for i in range(40)}
    s_ents = {f"e{i}": j for j, i in enumerate(rs.permutation(np.arange(10, 55)))}  # e10..e39 shared, other ids
    t_rels = {f"r{i}": i for i in range(6)}
    s_rels = {"r9": 0, "r4": 1, "r1": 2, "r5": 3, "r2": 4}
    teacher = _model("RotatE", rs.uniform(-1, 1, (40, 16)).astype(np.float32), rs.uniform(-1, 1, (6, 8)).astype(np.float32), 8, 4,
                     t_ents, t_rels)
    sampler = distillation.TopKSampling(teacher_entities=t_ents, teacher_relations=t_rels, student_entities=s_ents,
                                        student_relations=s_rels, batch_size_entity=6, batch_size_relation=3, n_random_entities=2,
                                        n_random_relations=1, seed=1)
    sample = torch.as_tensor(np.stack([rs.randint(40, size=9), rs.randint(6, size=9), rs.randint(40, size=9)], 1)).cuda()
    ht, rt, tt, hs, rsd, ts = sampler.get(sample=sample, teacher=teacher)
    shared_e, shared_r = sampler.mapping_entities, sampler.mapping_relations
    for t_ids, s_ids, mapping in ((ht, hs, shared_e), (tt, ts, shared_e), (rt, rsd, shared_r)):
        for a, b in zip(t_ids.cpu().numpy().ravel(), s_ids.cpu().numpy().ravel()):
            assert int(a) in mapping and mapping[int(a)] == int(b)
    e_ids = torch.tensor(sorted(shared_e), device="cuda")
    r_ids = torch.tensor(sorted(shared_r), device="cuda")
    with torch.no_grad():
        for mode, got in (("head-batch", ht), ("tail-batch", tt)):
            sc = teacher(sample, e_ids.view(1, -1).expand(9, -1).contiguous(), mode)
            order = torch.sort(sc, dim=1, descending=True, stable=True).indices[:, :6]
            assert torch.equal(got[:, :6], e_ids[order]), mode
        n = r_ids.numel()  # r1, r2, r4, r5
        blk = torch.stack([sample[:, 0:1].expand(-1, n), r_ids.view(1, -1).expand(9, -1), sample[:, 2:3].expand(-1, n)], -1)
        order = torch.sort(teacher(blk.contiguous()), dim=1, descending=True, stable=True).indices[:, :3]
        assert torch.equal(rt[:, :3], r_ids[order])
    assert ht.shape == (9, 8) and rt.shape == (9, 4)


def test_distill_with_topk_sampling_vs_reference(golden):
    """Distillation.distill with TopKSampling (unsupervised: each part distilled where the other two are shared) on Umls,
    RotatE teaching DistMult: loss and student gradients."""
    from mkb_amd import datasets, distillation

    g = golden("topk_sampling.npz")
    ds = datasets.Umls(batch_size=5, shuffle=False, seed=42, num_workers=0)
    teacher = _model("RotatE", g["distill/teacher_ent"], g["distill/teacher_rel"], 6, 6, ds.entities, ds.relations)
    student = _model("DistMult", g["distill/student_ent"], g["distill/student_rel"], 8, 6, ds.entities, ds.relations)
    sampler = distillation.TopKSampling(teacher_entities=ds.entities, teacher_relations=ds.relations, student_entities=ds.entities,
                                        student_relations=ds.relations, batch_size_entity=4, batch_size_relation=3,
                                        n_random_entities=2, n_random_relations=2, seed=9)
    proc = distillation.Distillation(teacher_entities=ds.entities, student_entities=ds.entities, teacher_relations=ds.relations,
                                     student_relations=ds.relations, sampling=sampler)
    sample = next(iter(ds))["sample"]
    np.testing.assert_array_equal(sample.numpy(), g["distill/sample"])
    loss = proc.distill(teacher=teacher, student=student, sample=sample.cuda())
    np.testing.assert_allclose(loss.item(), float(g["distill/loss"]), rtol=0, atol=1e-5)
    loss.backward()
    grad_close(student.entity_embedding.grad.cpu().numpy(), g["distill/g_ent"])
    grad_close(student.relation_embedding.grad.cpu().numpy(), g["distill/g_rel"], rtol=1e-4)
    assert teacher.entity_embedding.grad is None


def test_kdmkb_with_fast_topk_sampling_vs_reference(golden):
    """kdmkb_model.py with the reference's own default sampler (FastTopKSampling), two RotatE models of different sizes teaching
    each other over CountriesS1 copies, three steps: per-step losses and the tables afterwards."""
    from mkb_amd import datasets, distillation

    g, gj = golden("topk_sampling.npz"), golden("topk_sampling.json")
    torch.manual_seed(42)
    d1 = datasets.CountriesS1(batch_size=8, seed=42)
    d2 = datasets.CountriesS1(batch_size=8, seed=42)
    m1 = _model("RotatE", g["kd/m1_ent"], g["kd/m1_rel"], 6, 3, d1.entities, d1.relations)
    m2 = _model("RotatE", g["kd/m2_ent"], g["kd/m2_rel"], 4, 3, d2.entities, d2.relations)
    mods, dsets = collections.OrderedDict(a=m1, b=m2), collections.OrderedDict(a=d1, b=d2)
    kd = distillation.KdmkbModel(models=mods, datasets=dsets, lr={"a": 1e-2, "b": 1e-2}, alpha_kl={"a": 0.3, "b": 0.6},
                                 alpha_adv={"a": 0.5, "b": 0.5}, negative_sampling_size={"a": 4, "b": 4},
                                 batch_size_entity={"a": 4, "b": 4}, batch_size_relation={"a": 1, "b": 1},
                                 n_random_entities={"a": 3, "b": 2}, n_random_relations={"a": 1, "b": 1}, device="cuda", seed=42,
                                 sampling_method=distillation.FastTopKSampling)
    assert all(isinstance(d.sampling, distillation.FastTopKSampling) for d in kd.distillation.values())
    for want in gj["kd_step_losses"]:
        kd.forward(dsets, mods, {"a": 0.3, "b": 0.6})
        got = {k: kd.metrics[k]._w[-1] for k in mods}
        assert got == pytest.approx(want, abs=2e-5), (got, want)
    for key, m in (("m1", m1), ("m2", m2)):
        np.testing.assert_allclose(m.entity_embedding.detach().cpu().numpy(), g[f"kd/{key}_ent_after"], rtol=0, atol=3e-5)
        np.testing.assert_allclose(m.relation_embedding.detach().cpu().numpy(), g[f"kd/{key}_rel_after"], rtol=0, atol=3e-5)


def test_fast_topk_sampling_errors_and_lookup():
    """A TransE teacher raises ImportError (the reference's faiss index); a top k past the shared set raises ValueError; a key
    outside the teacher's training triples raises KeyError; known keys return the precomputed rows plus random columns."""
    from mkb_amd import datasets, distillation, models

    ds = datasets.CountriesS1(batch_size=64, seed=42, shuffle=False, num_workers=0)
    kw = dict(teacher_entities=ds.entities, teacher_relations=ds.relations, student_entities=ds.entities,
              student_relations=ds.relations, dataset_teacher=ds, seed=3)
    transe = models.TransE(hidden_dim=4, entities=ds.entities, relations=ds.relations, gamma=3).cuda()
    with pytest.raises(ImportError, match="faiss"):
        distillation.FastTopKSampling(teacher=transe, batch_size_entity=3, batch_size_relation=1, n_random_entities=0,
                                      n_random_relations=0, **kw)
    torch.manual_seed(0)
    rot = models.RotatE(hidden_dim=4, entities=ds.entities, relations=ds.relations, gamma=3).cuda()
    with pytest.raises(ValueError):
        distillation.FastTopKSampling(teacher=rot, batch_size_entity=3, batch_size_relation=3, n_random_entities=0,
                                      n_random_relations=0, **kw)
    with pytest.raises(ValueError):
        distillation.TopKSampling(batch_size_entity=len(ds.entities) + 1, batch_size_relation=1, n_random_entities=0,
                                  n_random_relations=0, **kw)
    fast = distillation.FastTopKSampling(teacher=rot, batch_size_entity=3, batch_size_relation=1, n_random_entities=2,
                                         n_random_relations=1, **kw)
    slow = distillation.TopKSampling(batch_size_entity=3, batch_size_relation=1, n_random_entities=2, n_random_relations=1, **kw)
    train = torch.as_tensor(np.asarray(ds.train, dtype=np.int64)[:50]).cuda()
    a, b = fast.get(sample=train), slow.get(sample=train, teacher=rot)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    seen = {(h, r, t) for h, r, t in ds.train}
    h = next(e for e in range(len(ds.entities)) if all((e, 0, t) not in seen for t in range(len(ds.entities))))
    with pytest.raises(KeyError):
        fast.get(sample=torch.tensor([[h, 0, 0]], device="cuda"))


@pytest.mark.parametrize("cls", ["RotatE", "TransE"])
def test_fast_topk_sampling_chunk_seams(cls):
    """The one precompute loop at its chunk seams: chunk = 7 (it divides none of CountriesS1's 192 / 1110 / 432 head / relation /
    tail keys, so every part ends on a ragged chunk) against chunk = 1024 (one chunk, but two for the relations) -- the same keys,
    teacher ids and student ids for all three parts, for a RotatE teacher (TopKSampling.side) and a TransE teacher
    (TopKSamplingTransE.side)."""
    from mkb_amd import datasets, distillation, models

    ds = datasets.CountriesS1(batch_size=64, seed=42, shuffle=False, num_workers=0)
    torch.manual_seed(5)
    teacher = getattr(models, cls)(hidden_dim=6, entities=ds.entities, relations=ds.relations, gamma=3).cuda()
    kw = dict(teacher_entities=ds.entities, teacher_relations=ds.relations, student_entities=ds.entities,
              student_relations=ds.relations, dataset_teacher=ds, teacher=teacher, batch_size_entity=3, batch_size_relation=2,
              n_random_entities=1, n_random_relations=1, seed=3, device="cuda", transe_sampler=distillation.TopKSamplingTransE)
    small, whole = (distillation.FastTopKSampling(chunk=chunk, **kw) for chunk in (7, 1024))
    for part in ("head", "relation", "tail"):
        n = whole._keys[part][0].numel()
        assert n > 7 and n % 7 != 0, (part, n)
        assert whole._keys[part][1].shape == (n, 2 if part == "relation" else 3)
        for a, b in zip(small._keys[part], whole._keys[part]):
            assert torch.equal(a, b), part


def test_samplers_share_one_constructor():
    """FastTopKSampling and TopKSamplingTransE refuse the sizes TopKSampling refuses (tests/test_host_topk_sampling.py), and a
    FastTopKSampling over no triples holds empty [0, k] lists."""
    from mkb_amd import datasets, distillation, models

    ds = datasets.CountriesS1(batch_size=64, seed=42, shuffle=False, num_workers=0)
    n_e, n_r = len(ds.entities), len(ds.relations)
    kw = dict(teacher_entities=ds.entities, teacher_relations=ds.relations, student_entities=ds.entities,
              student_relations=ds.relations, dataset_teacher=[], seed=3, device="cuda")
    ok = dict(batch_size_entity=3, batch_size_relation=1, n_random_entities=1, n_random_relations=1)
    teachers = {distillation.FastTopKSampling: models.RotatE(hidden_dim=4, entities=ds.entities, relations=ds.relations, gamma=3).cuda(),
                distillation.TopKSamplingTransE: models.TransE(hidden_dim=4, entities=ds.entities, relations=ds.relations, gamma=3).cuda()}
    for sampler, teacher in teachers.items():
        for bad in (dict(batch_size_entity=0), dict(batch_size_entity=n_e + 1), dict(batch_size_relation=0),
                    dict(batch_size_relation=n_r + 1), dict(n_random_entities=-1), dict(n_random_entities=n_e + 1),
                    dict(n_random_relations=-1), dict(n_random_relations=n_r + 1)):
            with pytest.raises(ValueError):
                sampler(teacher=teacher, **kw, **{**ok, **bad})
    empty = distillation.FastTopKSampling(teacher=teachers[distillation.FastTopKSampling], **kw, **ok)
    assert (empty.batch_size_entity, empty.batch_size_relation) == (4, 2)
    for part, k in (("head", 3), ("relation", 1), ("tail", 3)):
        assert [tuple(x.shape) for x in empty._keys[part]] == [(0,), (0, k), (0, k)]
    with pytest.raises(KeyError):
        empty.get(sample=torch.tensor([[0, 0, 1]], device="cuda"))
