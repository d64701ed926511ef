"""-m gpu: the TransE teacher's top-k samplers (distillation.TopKSamplingTransE, FastTopKSampling(transe_sampler=...)) on the
exact squared-L2 k nearest rows (mkb_topk_nearest), against captures of the live reference run around an exact flat L2 index
(tools/make_golden.py::gen_topk_sampling_transe).  The captures' k-th / (k+1)-th relative distance gaps (and the RotatE
teacher's score gap) are all above 1e-4, so an fp32 near-tie cannot reorder them."""
import collections
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_topk_sampling import _model  # noqa: E402

NAMES = ("head_t", "rel_t", "tail_t", "head_s", "rel_s", "tail_s")


def test_capture_gaps_are_clear(golden):
    gj = golden("topk_sampling_transe.json")
    assert min(gj["gaps"].values()) > 1e-4, gj["gaps"]


def test_transe_top_k_queries():
    """TransE._top_k: t - r, t - h, h + r as [B, 1, D], bit for bit the reference's -r + t, -h + t, h + r."""
    from mkb_amd import models

    torch.manual_seed(0)
    m = models.TransE(hidden_dim=6, entities={i: i for i in range(30)}, relations={i: i for i in range(4)}, gamma=3).cuda()
    s = torch.tensor([[0, 1, 2], [5, 3, 29], [7, 0, 7]], device="cuda")
    head, rel, tail = m._top_k(s)
    E, R = m.entity_embedding.detach(), m.relation_embedding.detach()
    h, r, t = E[s[:, 0]], R[s[:, 1]], E[s[:, 2]]
    for got, want in ((head, -r + t), (rel, -h + t), (tail, h + r)):
        assert got.shape == (3, 1, 6)
        assert torch.equal(got.reshape(3, 6), want)


def _get_setup(g, gj):
    from mkb_amd import datasets

    ds = datasets.CountriesS1(batch_size=6, seed=42, shuffle=False, num_workers=0)
    d = {name: collections.OrderedDict((k, v) for k, v in gj["get"][name]) for name in ("t_ents", "s_ents", "t_rels", "s_rels")}
    teacher = _model("TransE", g["get/ent"], g["get/rel"], 8, 4, ds.entities, ds.relations)
    return d, teacher


def test_topk_sampling_transe_get_vs_reference(golden):
    """CountriesS1, the teacher dict shuffled, a student dict that renumbers and drops labels, top 5 entities + 3 random, top 1
    relation + 1 random, four batches: all six tensors equal the reference's."""
    from mkb_amd import distillation

    g, gj = golden("topk_sampling_transe.npz"), golden("topk_sampling_transe.json")
    d, teacher = _get_setup(g, gj)
    sampler = distillation.TopKSamplingTransE(teacher_entities=d["t_ents"], teacher_relations=d["t_rels"],
                                              student_entities=d["s_ents"], student_relations=d["s_rels"], teacher=teacher,
                                              batch_size_entity=5, batch_size_relation=1, n_random_entities=3, n_random_relations=1,
                                              seed=7, device="cuda")
    assert sampler.supervised is False and sampler.depends_on_teacher is True
    assert (sampler.batch_size_entity, sampler.batch_size_relation) == (8, 2)
    for j, b in enumerate(g["get/samples"]):
        got = sampler.get(sample=torch.as_tensor(b).cuda(), teacher=teacher)
        for name, x in zip(NAMES, got):
            assert x.dtype == torch.int64 and x.is_cuda
            np.testing.assert_array_equal(x.cpu().numpy(), g[f"get/{j}/{name}"], err_msg=f"batch {j} {name}")


def test_topk_sampling_transe_edges(golden):
    """An empty sample gives [0, k] tensors; a non-TransE teacher and a top k past the shared set raise ValueError."""
    from mkb_amd import distillation, models

    g, gj = golden("topk_sampling_transe.npz"), golden("topk_sampling_transe.json")
    d, teacher = _get_setup(g, gj)
    kw = dict(teacher_entities=d["t_ents"], teacher_relations=d["t_rels"], student_entities=d["s_ents"], student_relations=d["s_rels"],
              n_random_entities=2, n_random_relations=0)
    sampler = distillation.TopKSamplingTransE(teacher=teacher, batch_size_entity=4, batch_size_relation=2, **kw)
    out = sampler.get(sample=torch.empty((0, 3), dtype=torch.int64, device="cuda"), teacher=teacher)
    assert [tuple(x.shape) for x in out] == [(0, 6), (0, 2), (0, 6), (0, 6), (0, 2), (0, 6)]
    rot = models.RotatE(hidden_dim=4, entities={i: i for i in range(271)}, relations={0: 0, 1: 1}, gamma=3).cuda()
    with pytest.raises(ValueError):
        distillation.TopKSamplingTransE(teacher=rot, batch_size_entity=4, batch_size_relation=1, **kw)
    with pytest.raises(ValueError):
        sampler.get(sample=torch.tensor([[0, 0, 1]], device="cuda"), teacher=rot)
    with pytest.raises(ValueError):
        distillation.TopKSamplingTransE(teacher=teacher, batch_size_entity=len(d["s_ents"]) + 1, batch_size_relation=1, **kw)
    with pytest.raises(ValueError):
        distillation.TopKSamplingTransE(teacher=teacher, batch_size_entity=2, batch_size_relation=3, **kw)


def test_fast_topk_sampling_transe_vs_reference(golden):
    """FastTopKSampling(transe_sampler=TopKSamplingTransE) over the CountriesS1 training split: looked-up rows equal the
    reference's; an unseen key raises KeyError; without the keyword a TransE teacher still raises ImportError."""
    from mkb_amd import datasets, distillation

    g = golden("topk_sampling_transe.npz")
    ds = datasets.CountriesS1(batch_size=16, seed=42, shuffle=False, num_workers=0)
    teacher = _model("TransE", g["fast/ent"], g["fast/rel"], 8, 4, ds.entities, ds.relations)
    kw = dict(teacher_entities=ds.entities, teacher_relations=ds.relations, student_entities=ds.entities,
              student_relations=ds.relations, batch_size_entity=4, batch_size_relation=1, n_random_entities=2, n_random_relations=1,
              dataset_teacher=ds, teacher=teacher, seed=3, device="cuda")
    with pytest.raises(ImportError, match="faiss"):
        distillation.FastTopKSampling(**kw)
    fast = distillation.FastTopKSampling(transe_sampler=distillation.TopKSamplingTransE, **kw)
    for j, b in enumerate(g["fast/samples"]):
        got = fast.get(sample=torch.as_tensor(b).cuda())
        for name, x in zip(NAMES, got):
            np.testing.assert_array_equal(x.cpu().numpy(), g[f"fast/{j}/{name}"], err_msg=f"batch {j} {name}")
    seen = {(h, r, t) for h, r, t in ds.train}
    h = next(e for e in range(len(ds.entities)) if all((e, 0, t) not in seen for t in range(len(ds.entities))))
    with pytest.raises(KeyError):
        fast.get(sample=torch.tensor([[h, 0, 0]], device="cuda"))


def test_kdmkb_with_transe_teacher_vs_reference(golden):
    """kdmkb_model.py with the reference's default sampler (FastTopKSampling, which sends the TransE teacher to its faiss
    sampler): a TransE and a RotatE model teaching each other over CountriesS1 copies, three steps: per-step losses and tables.

    The first step's losses match to 2e-5.  Adam's first update lr * g / (|g| + 1e-8) turns the fp32 rounding of gradients near
    1e-8 (most likely what a few TransE rows get from the distillation's softmax tails) into differences of up to lr = 1e-2 on
    those rows (measured: 2e-3 on three rows after step 1), which the later losses carry at ~1e-4; they are checked at that size, the
    tables at about one Adam step."""
    from mkb_amd import datasets, distillation

    g, gj = golden("topk_sampling_transe.npz"), golden("topk_sampling_transe.json")
    d1 = datasets.CountriesS1(batch_size=8, seed=42)
    d2 = datasets.CountriesS1(batch_size=8, seed=42)
    torch.manual_seed(61)
    m1 = _model("TransE", g["kd/m1_ent"], g["kd/m1_rel"], 8, 3, d1.entities, d1.relations)
    m2 = _model("RotatE", g["kd/m2_ent"], g["kd/m2_rel"], 4, 3, d2.entities, d2.relations)
    mods, dsets = collections.OrderedDict(a=m1, b=m2), collections.OrderedDict(a=d1, b=d2)
    kd = distillation.KdmkbModel(models=mods, datasets=dsets, lr={"a": 1e-2, "b": 1e-2}, alpha_kl={"a": 0.3, "b": 0.6},
                                 alpha_adv={"a": 0.5, "b": 0.5}, negative_sampling_size={"a": 4, "b": 4},
                                 batch_size_entity={"a": 4, "b": 4}, batch_size_relation={"a": 1, "b": 1},
                                 n_random_entities={"a": 3, "b": 2}, n_random_relations={"a": 1, "b": 1}, device="cuda", seed=42,
                                 sampling_method=functools.partial(distillation.FastTopKSampling,
                                                                   transe_sampler=distillation.TopKSamplingTransE))
    for step, want in enumerate(gj["kd_step_losses"]):
        kd.forward(dsets, mods, {"a": 0.3, "b": 0.6})
        got = {k: kd.metrics[k]._w[-1] for k in mods}
        assert got == pytest.approx(want, abs=2e-5 if step == 0 else 1e-3), (step, got, want)
    for key, m in (("m1", m1), ("m2", m2)):
        np.testing.assert_allclose(m.entity_embedding.detach().cpu().numpy(), g[f"kd/{key}_ent_after"], rtol=0, atol=1e-2)
        np.testing.assert_allclose(m.relation_embedding.detach().cpu().numpy(), g[f"kd/{key}_rel_after"], rtol=0, atol=3e-5)


def test_fast_equals_slow_for_a_transe_teacher():
    """FastTopKSampling(transe_sampler=TopKSamplingTransE).get equals TopKSamplingTransE.get on the first 50 CountriesS1
    training triples, all six tensors, with one seed on both: the two score the same query rows against the same index rows with
    the same kernel, so the lists are equal exactly."""
    from mkb_amd import datasets, distillation, models

    ds = datasets.CountriesS1(batch_size=64, seed=42, shuffle=False, num_workers=0)
    torch.manual_seed(0)
    teacher = models.TransE(hidden_dim=8, entities=ds.entities, relations=ds.relations, gamma=3).cuda()
    kw = dict(teacher_entities=ds.entities, teacher_relations=ds.relations, student_entities=ds.entities,
              student_relations=ds.relations, teacher=teacher, batch_size_entity=3, batch_size_relation=1, n_random_entities=2,
              n_random_relations=1, seed=3, device="cuda")
    fast = distillation.FastTopKSampling(dataset_teacher=ds, transe_sampler=distillation.TopKSamplingTransE, **kw)
    slow = distillation.TopKSamplingTransE(**kw)
    train = torch.as_tensor(np.asarray(ds.train, dtype=np.int64)[:50]).cuda()
    for name, x, y in zip(NAMES, fast.get(sample=train), slow.get(sample=train, teacher=teacher)):
        assert x.shape == y.shape == (50, 2 if name.startswith("rel") else 5)
        assert torch.equal(x, y), name
