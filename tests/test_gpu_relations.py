"""-m gpu: the relation side of link prediction on the device (mkb_amd/csrc/score_relation.hip): mkb_rel_scores against the general
forward bit for bit, mkb_rel_rank against Evaluation._relation_ranks_torch and against the numpy restatement of the contract
(tests/util_relations.py), mkb_rel_topk against the restatement, and the Python entry points built on them.  Score bits are
compared through ``.view(torch.int32)`` so that NaN equals NaN."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import util_relations as ur  # noqa: E402
from util_gpu import make_model  # noqa: E402

MODELS = ["TransE", "RotatE", "ComplEx", "DistMult", "pRotatE"]
N = 50


def _tables(name, hidden, R, seed, n_entity=N):
    rs = np.random.RandomState(seed)
    de = 2 * hidden if name in ("RotatE", "ComplEx") else hidden
    dr = 2 * hidden if name == "ComplEx" else hidden
    ent = rs.uniform(-0.3, 0.3, size=(n_entity, de)).astype(np.float32)
    rel = rs.uniform(-0.3, 0.3, size=(R, dr)).astype(np.float32)
    modulus = np.array([[0.1]], dtype=np.float32) if name in ("RotatE", "pRotatE") else None
    return ent, rel, modulus


def _model(name, hidden, R, seed, n_entity=N):
    ent, rel, modulus = _tables(name, hidden, R, seed, n_entity)
    return make_model(name, ent, rel, hidden, 6.0, modulus).eval()


def _pairs(rs, B, R, n_entity=N):
    return np.stack([rs.randint(n_entity, size=B), rs.randint(R, size=B), rs.randint(n_entity, size=B)], 1).astype(np.int64)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _ws(need):
    raw = torch.empty(need + 256, dtype=torch.uint8, device="cuda")
    return raw, ctypes.c_void_p(raw.data_ptr() + (-raw.data_ptr()) % 256)


def _general(m, s, rel):
    """The existing path: model(block [B, n_rel, 3]), one general-forward workgroup per triple."""
    from mkb_amd.utils.predict_relations import general_relation_scores

    with torch.no_grad():
        return general_relation_scores(m, s, rel)


def _scores(m, s, rel=None, pad=0, fill=-123.0):
    """mkb_rel_scores into a pre-filled block of row stride n_rel + pad -> the whole [B, n_rel + pad] block."""
    from mkb_amd import _hip

    n_rel = m.n_relation if rel is None else rel.numel()
    out = torch.full((s.shape[0], n_rel + pad), fill, dtype=torch.float32, device="cuda")
    _hip.check(_hip.lib().mkb_rel_scores(m._tables(), _hip.ptr(s), s.shape[0], _hip.ptr(rel), n_rel, _hip.ptr(out), n_rel + pad,
                                         _hip.stream_ptr()), "mkb_rel_scores")
    return out


def _rank(m, s, keys, with_scores=True, rank_fill=-5):
    from mkb_amd import _hip

    lib, tb, B = _hip.lib(), m._tables(), s.shape[0]
    # (buffers of max(B, 1) rows, passed by their base pointer: torch reports a null pointer for an empty tensor, which the ABI refuses)
    rank = torch.full((max(B, 1),), rank_fill, dtype=torch.int64, device="cuda")
    block = torch.full((max(B, 1), m.n_relation), float("nan"), dtype=torch.float32, device="cuda") if with_scores else None
    sample = s if B else torch.zeros((1, 3), dtype=torch.int64, device="cuda")
    need = lib.mkb_rel_rank_workspace_bytes(tb, B)
    raw, w = _ws(need)
    _hip.check(lib.mkb_rel_rank(tb, _hip.ptr(sample), B, _hip.ptr(keys) if keys is not None and keys.numel() else None,
                                keys.numel() if keys is not None else 0, _hip.ptr(rank), _hip.ptr(block), w if B else None, need,
                                _hip.stream_ptr()), "mkb_rel_rank")
    if B == 0:  # nothing was launched: nothing was written
        torch.cuda.synchronize()
        assert bool((rank == rank_fill).all()) and (block is None or bool(torch.isnan(block).all()))
    rank, block = rank[:B], (block[:B] if with_scores else None)
    torch.cuda.synchronize()
    return rank, block


def _topk(m, s, keys, k, keep, fill=7):
    from mkb_amd import _hip

    lib, tb, B = _hip.lib(), m._tables(), s.shape[0]
    ids = torch.full((B, k), fill, dtype=torch.int64, device="cuda")  # dirty output buffers
    sc = torch.full((B, k), float(fill), dtype=torch.float32, device="cuda")
    need = lib.mkb_rel_topk_workspace_bytes(tb, B, k)
    raw, w = _ws(need)
    raw.fill_(0xA5 if fill == 7 else 0x3C)  # ... and a dirty workspace
    _hip.check(lib.mkb_rel_topk(tb, _hip.ptr(s), B, _hip.ptr(keys) if keys is not None and keys.numel() else None,
                                keys.numel() if keys is not None else 0, k, _hip.TOPK_KEEP_TARGET if keep else 0, _hip.ptr(ids),
                                _hip.ptr(sc), w, need, _hip.stream_ptr()), "mkb_rel_topk")
    torch.cuda.synchronize()
    return ids, sc


def _keys(true, R, n_entity=N):
    a = np.asarray(sorted(true), dtype=np.int64).reshape(-1, 3)
    return np.unique((a[:, 0] * R + a[:, 1]) * n_entity + a[:, 2])


def _true_set(rs, sample, R, dense=0.4, n_all=3):
    """Other true relations for the pairs of ``sample``: the first n_all pairs have EVERY relation true, half of the targets are
    keys themselves, the rest get a random ~dense share."""
    true = {(int(h), int(r), int(t)) for h, r, t in sample[: len(sample) // 2]}
    for i, (h, _, t) in enumerate(sample):
        rels = range(R) if i < n_all else np.flatnonzero(rs.rand(R) < dense)
        true |= {(int(h), int(r), int(t)) for r in rels if i < n_all or r != sample[i, 1] or i < len(sample) // 2}
    return true


RS = [1, 3, 4, 5, 63, 64, 65, 237]
BS = [1, 3, 4, 5, 257]


@pytest.mark.parametrize("hidden", [3, 37, 64, 260])
@pytest.mark.parametrize("name", MODELS)
def test_scores_are_the_general_forward_bit_for_bit(name, hidden):
    """hidden 3: fewer units than lanes; 37: an odd length on the scalar route; 64: the vec4 route; 260: the vec4 route with a
    second, ragged stride.  Every R meets four of the five batch sizes over the four hidden sizes (B around the waves per
    workgroup; R around the waves' turns).  The relation column of sample is out of range: it must not be read."""
    hi = [3, 37, 64, 260].index(hidden)
    for idx, R in enumerate(RS):
        B = BS[(idx + hi) % len(BS)]
        rs = np.random.RandomState(1000 * hi + R)
        m = _model(name, hidden, R, seed=R + hi)
        pairs = _pairs(rs, B, R)
        s = torch.as_tensor(pairs).cuda()
        unread = s.clone()
        unread[:, 1] = 10 ** 12
        every = torch.arange(R, device="cuda")
        got = _scores(m, unread, None, pad=3)
        want = _general(m, s, every)
        what = f"{name} hidden={hidden} R={R} B={B}"
        assert torch.equal(_bits(got[:, :R]), _bits(want)), what
        assert bool((got[:, R:] == -123.0).all()), what  # the padding columns are untouched
        # a list with duplicates, in reversed order, n_rel != R
        rel = torch.as_tensor(np.concatenate([np.arange(R)[::-1], rs.randint(R, size=3), [0, 0]]).astype(np.int64)).cuda()
        got = _scores(m, unread, rel, pad=3)
        assert torch.equal(_bits(got[:, : rel.numel()]), _bits(_general(m, s, rel))), what
        assert torch.equal(_bits(got[:, : rel.numel()]), _bits(want[:, rel])), what
        assert bool((got[:, rel.numel():] == -123.0).all()), what


def test_relation_scores_entry_point():
    from mkb_amd.utils import relation_scores

    m = _model("ComplEx", 37, 9, seed=5)
    pairs = _pairs(np.random.RandomState(2), 11, 9)
    s = torch.as_tensor(pairs).cuda()
    assert torch.equal(_bits(relation_scores(m, pairs)), _bits(_general(m, s, torch.arange(9, device="cuda"))))
    rel = [8, 8, 0, 3]
    assert torch.equal(_bits(relation_scores(m, pairs.tolist(), relations=rel)), _bits(_general(m, s, torch.tensor(rel).cuda())))
    assert relation_scores(m, np.empty((0, 3), dtype=np.int64)).shape == (0, 9)
    for bad in ([[N, 0, 1]], [[0, 0, -1]]):
        with pytest.raises(ValueError, match="outside"):
            relation_scores(m, bad)
    for bad in ([9], [-1], []):
        with pytest.raises(ValueError, match="relation"):
            relation_scores(m, pairs, relations=bad)


@pytest.mark.parametrize("hidden", [37, 64])
@pytest.mark.parametrize("name", MODELS)
def test_rank_equals_the_torch_route_on_umls(name, hidden):
    from mkb_amd import datasets, evaluation, models

    ds = datasets.Umls(batch_size=8, shuffle=False, seed=42, num_workers=0)
    torch.manual_seed(3)
    m = getattr(models, name)(hidden_dim=hidden, entities=ds.entities, relations=ds.relations, gamma=6).cuda().eval()
    ev = evaluation.Evaluation(true_triples=ds.true_triples, entities=ds.entities, relations=ds.relations, batch_size=64,
                               device="cuda", num_workers=0)
    test = ds.test[:150]
    with torch.no_grad():
        want, want_block = ev._relation_ranks_torch(m, test, with_scores=True)
        got, block = ev._relation_ranks_kernel(m, test, chunk=64, with_scores=True)  # three chunks, the last ragged
        assert bool(torch.isfinite(block).all())
        assert torch.equal(got, want), (name, hidden)
        assert torch.equal(_bits(block), _bits(want_block))
        s = torch.as_tensor(np.asarray(test, dtype=np.int64)).cuda()
        assert torch.equal(_bits(block), _bits(_scores(m, s)))
        assert torch.equal(ev._relation_ranks_kernel(m, test), want)
        found = ev.relation_ranks(m, test, with_scores=True)  # whichever route is this model's default
        assert torch.equal(found[0], want) and torch.equal(_bits(found[1]), _bits(want_block))


@pytest.mark.parametrize("R", [1, 5, 65])
def test_rank_equals_the_restatement_on_crafted_sets(R):
    m = _model("RotatE", 37, R, seed=40 + R)
    rs = np.random.RandomState(R)
    sample = _pairs(rs, 41, R)
    sample[7] = sample[6]  # duplicate queries
    sample[8] = sample[6]
    true = _true_set(rs, sample, R)  # pairs 0-2: every other relation is a key; the second half's targets are not keys
    s = torch.as_tensor(sample).cuda()
    want_block = _scores(m, s)
    for keys in (np.empty(0, dtype=np.int64), _keys(true, R)):  # n_true = 0 filters nothing
        rank, block = _rank(m, s, torch.as_tensor(keys).cuda())
        assert torch.equal(_bits(block), _bits(want_block))
        mask = ur.filter_mask(sample, keys, N, R)
        np.testing.assert_array_equal(rank.cpu().numpy(), ur.rel_ranks(block.cpu().numpy(), sample, mask))
        if len(keys):
            assert mask[:3].all() and bool((rank[:3] == 1).all())
            own = mask[np.arange(41), sample[:, 1]]
            assert own[:20].all() and not own[20:].all()  # targets that are keys, and targets that are not
            assert torch.equal(rank[6], rank[7]) and torch.equal(rank[6], rank[8])
        rank2, _ = _rank(m, s, torch.as_tensor(keys).cuda(), with_scores=False, rank_fill=99)
        assert torch.equal(rank, rank2)  # without the block, on other dirty buffers: the same ranks
    empty = torch.empty((0, 3), dtype=torch.int64, device="cuda")
    rank, block = _rank(m, empty, torch.as_tensor(_keys(true, R)).cuda())  # B = 0 launches nothing
    assert rank.shape == (0,) and block.shape == (0, R)


def _spoiled(name, hidden, R):
    """Tables with a NaN relation row (1), one whose scores overflow (2), and two equal rows (3 == 4): NaN, +-inf and ties."""
    ent, rel, modulus = _tables(name, hidden, R, seed=77)
    rel[1] = np.nan
    rel[2] = 3e38
    rel[4] = rel[3]
    if name in ("ComplEx", "DistMult"):
        ent[:, 0] = 30.0  # h * r overflows in this unit
    return make_model(name, ent, rel, hidden, 6.0, modulus).eval()


@pytest.mark.parametrize("name", MODELS)
def test_nan_inf_and_ties_follow_the_restatement(name):
    R = 7
    m = _spoiled(name, 37, R)
    rs = np.random.RandomState(9)
    sample = _pairs(rs, 60, R)
    sample[:14, 1] = np.repeat(np.arange(R), 2)  # every kind of relation is a target, with and without its own key
    true = _true_set(rs, sample, R, dense=0.3, n_all=0)
    s = torch.as_tensor(sample).cuda()
    for keys in (np.empty(0, dtype=np.int64), _keys(true, R)):
        kt = torch.as_tensor(keys).cuda()
        rank, block = _rank(m, s, kt)
        b = block.cpu().numpy()
        assert np.isnan(b[:, 1]).all() and (b[:, 3] == b[:, 4]).all(), name
        if name in ("TransE", "ComplEx", "DistMult"):  # (the rotations take the row as phases: nothing overflows there)
            assert not np.isfinite(b[:, 2]).any(), name
        if name == "TransE":
            assert np.isneginf(b[:, 2]).all()
        mask = ur.filter_mask(sample, keys, N, R)
        np.testing.assert_array_equal(rank.cpu().numpy(), ur.rel_ranks(b, sample, mask))
        for k, keep in ((1, True), (3, False), (R, True), (R + 2, False)):
            ids, sc = _topk(m, s, kt, k, keep)
            want_ids, want_sc = ur.rel_topk(b, sample, mask, k, keep)
            np.testing.assert_array_equal(ids.cpu().numpy(), want_ids)
            np.testing.assert_array_equal(sc.cpu().numpy().view(np.int32), want_sc.view(np.int32))


@pytest.mark.parametrize("name", ["TransE", "ComplEx"])
def test_a_collapsed_model_does_not_rank_its_targets_first(name):
    R = 9
    ent, rel, modulus = _tables(name, 37, R, seed=1)
    ent[:], rel[:] = ent[0], rel[0]
    m = make_model(name, ent, rel, 37, 6.0, modulus).eval()
    rs = np.random.RandomState(4)
    sample = _pairs(rs, 30, R)
    true = _true_set(rs, sample, R, n_all=0)
    keys = _keys(true, R)
    mask = ur.filter_mask(sample, keys, N, R)
    rank, block = _rank(m, torch.as_tensor(sample).cuda(), torch.as_tensor(keys).cuda())
    assert bool((block == block[0, 0]).all())
    want = np.array([1 + int((~mask[i, :r]).sum()) for i, r in enumerate(sample[:, 1])])  # the unfiltered relations of lower id
    np.testing.assert_array_equal(rank.cpu().numpy(), want)
    assert (want > 1).any()


@pytest.mark.parametrize("R", [3, 65, 237])
@pytest.mark.parametrize("name", MODELS)
def test_topk_equals_the_restatement(name, R):
    m = _model(name, 37, R, seed=R)
    rs = np.random.RandomState(R + 1)
    sample = _pairs(rs, 37, R)
    true = _true_set(rs, sample, R)
    s = torch.as_tensor(sample).cuda()
    block = _scores(m, s).cpu().numpy()
    for keys in (np.empty(0, dtype=np.int64), _keys(true, R)):
        kt = torch.as_tensor(keys).cuda()
        mask = ur.filter_mask(sample, keys, N, R)
        rank = _rank(m, s, kt, with_scores=False)[0].cpu().numpy()
        for k in sorted({1, 5, R, R + 7, 1024}):
            for keep in (False, True):
                ids, sc = _topk(m, s, kt, k, keep)
                want_ids, want_sc = ur.rel_topk(block, sample, mask, k, keep)
                what = f"{name} R={R} k={k} keep={keep} keys={len(keys)}"
                np.testing.assert_array_equal(ids.cpu().numpy(), want_ids, err_msg=what)
                np.testing.assert_array_equal(sc.cpu().numpy().view(np.int32), want_sc.view(np.int32), err_msg=what)
                left = (~mask).sum(1) + (mask[np.arange(len(sample)), sample[:, 1]] if keep else 0)
                assert ((ids.cpu().numpy() >= 0).sum(1) == np.minimum(left, k)).all(), what  # -1 / -inf past the candidates
                if keep:  # wherever the rank is at most k, the target sits at position rank - 1
                    hit = np.flatnonzero(rank <= k)
                    assert (ids.cpu().numpy()[hit, rank[hit] - 1] == sample[hit, 1]).all(), what
                again = _topk(m, s, kt, k, keep, fill=-9)  # a second run on other dirty buffers: the same bits
                assert torch.equal(ids, again[0]) and torch.equal(_bits(sc), _bits(again[1])), what


def test_topk_sampling_relation_side_equals_the_general_route():
    """A teacher and a student that share about half their relations under a different numbering."""
    from mkb_amd.distillation import TopKSampling

    R = 11
    ents = {f"e{i}": i for i in range(N)}
    t_rels = {f"r{i}": i for i in range(R)}
    shared = [1, 2, 4, 7, 8, 10]
    s_rels = {f"r{i}": j for j, i in enumerate(reversed(shared))}
    s_rels.update({"only_student": len(shared)})
    pairs = torch.as_tensor(_pairs(np.random.RandomState(3), 70, R)).cuda()
    for name in MODELS:
        teacher = _model(name, 64, R, seed=8)
        for k in (1, 4, len(shared)):
            sampler = TopKSampling(teacher_entities=ents, teacher_relations=t_rels, student_entities=ents, student_relations=s_rels,
                                   batch_size_entity=3, batch_size_relation=k, n_random_entities=0, n_random_relations=0, device="cuda")
            sampler.RELATION_KERNEL_MODELS = frozenset(MODELS)  # the kernel's route, whatever this model's default is
            with torch.no_grad():
                got = sampler.side("relation", pairs, teacher, chunk=32)
                want = sampler._relation_side_general(pairs, teacher, chunk=32)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (name, k)
            assert set(got[0].unique().tolist()) <= set(shared)
            assert torch.equal(got[1], torch.tensor([s_rels.get(f"r{i}", -1) for i in range(R)]).cuda()[got[0]])


def test_evaluation_wiring_on_umls():
    from mkb_amd import datasets, evaluation, models
    from mkb_amd.utils import predict_top_k_relations

    ds = datasets.Umls(batch_size=8, shuffle=False, seed=42, num_workers=0)
    ev = evaluation.Evaluation(true_triples=ds.true_triples, entities=ds.entities, relations=ds.relations, batch_size=64,
                               device="cuda", num_workers=0)
    test = ds.test[:150]
    torch.manual_seed(5)
    m = models.RotatE(hidden_dim=64, entities=ds.entities, relations=ds.relations, gamma=6).cuda().eval()
    for keep in (True, False):
        got = ev.top_k_relations(m, test, 5, keep_target=keep, chunk=64)
        want = predict_top_k_relations(m, test, 5, true_triples=ds.true_triples, keep_target=keep)
        assert torch.equal(got[0], want[0]) and torch.equal(_bits(got[1]), _bits(want[1]))
    ids, _ = ev.top_k_relations(m, test, 5)
    rank = ev.relation_ranks(m, test)
    hit = torch.nonzero(rank <= 5).flatten()
    target = torch.as_tensor(np.asarray(test, dtype=np.int64)[:, 1]).cuda()
    assert len(hit) and torch.equal(ids[hit, rank[hit] - 1], target[hit])
    with pytest.raises(ValueError, match="outside"):
        predict_top_k_relations(m, [[0, ds.n_relation, 1]], 3, keep_target=True)
    predict_top_k_relations(m, [[0, ds.n_relation, 1]], 3)  # without keep_target the relation column is not read
    assert predict_top_k_relations(m, [], 3)[0].shape == (0, 3)


@pytest.mark.parametrize("name", MODELS)
def test_eval_relations_equals_the_reference_route_at_hidden_260(name):
    from mkb_amd import datasets, evaluation, models

    ds = datasets.Umls(batch_size=8, shuffle=False, seed=42, num_workers=0)
    torch.manual_seed(3)
    m = getattr(models, name)(hidden_dim=260, entities=ds.entities, relations=ds.relations, gamma=6).cuda().eval()
    ev = evaluation.Evaluation(true_triples=ds.true_triples, entities=ds.entities, relations=ds.relations, batch_size=64,
                               device="cuda", num_workers=0)
    test = ds.test[:150]
    fast = ev.eval_relations(model=m, dataset=test)
    with torch.no_grad():
        assert torch.equal(ev._relation_ranks_kernel(m, test), ev._relation_ranks_torch(m, test))
    ev.force_reference_path = True
    assert fast == ev.eval_relations(model=m, dataset=test)
