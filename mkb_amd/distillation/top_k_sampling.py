"""Teacher top-k candidate samplers for distillation (reference mkb/distillation/top_k_sampling.py:9-662): ``TopKSampling`` picks,
for every positive triple, the k entities / relations the teacher scores highest among those both graphs share;
``FastTopKSampling`` precomputes those lists over the teacher's training triples once and looks them up.  Unsupervised: the
ground truth is not put into the lists, so ``Distillation`` distils each part of a triple whose other two parts are shared.

The reference loops over the triples on the host with three ``argsort``s per triple.  Here one base class holds what every
sampler shares (the mappings, sizes, checks, device tables, the random columns and the one ``get``), and each live sampler
answers one question, ``side(part, sample, teacher)``: the k candidates of one part ("head", "relation" or "tail") of these
triples, in teacher and in student ids.  ``TopKSampling.side`` is one ``mkb_topk_masked`` launch per entity side and batch (the
all-entity score block, restricted to the shared entities by a bitmask), and for the relation side one ``mkb_rel_scores`` of the
``[b, shared relations]`` block (the scores ``Evaluation.relation_ranks`` counts on) and one ``mkb_topk_block``.
``TopKSamplingTransE.side`` is the reference's sampler for a TransE teacher: the shared entities / relations nearest in L2 to
the teacher's translated queries, with the device's exact squared-L2 k nearest rows (``mkb_topk_nearest``) in place of the
reference's faiss ``IndexFlatL2``.  ``FastTopKSampling`` runs one loop over the distinct keys of the three parts and asks the
``side`` of ``TopKSampling`` -- or, for a TransE teacher, of ``transe_sampler=TopKSamplingTransE`` -- ``chunk`` keys at a time."""
import collections

import numpy as np
import torch

from .. import _hip
from ..utils.predict_relations import rel_scores_launch
from ..utils.predict_top_k import _launch, candidate_bits, topk_block, topk_nearest

__all__ = ["FastTopKSampling", "TopKSampling", "TopKSamplingTransE"]

PARTS = ("head", "relation", "tail")


def _shared(teacher, student):
    """teacher id -> student id of the labels both know, in the teacher dict's order (the reference's mapping)."""
    return collections.OrderedDict((i, student[label]) for label, i in teacher.items() if label in student)


def _check_k(k, n_shared, what):
    if not 1 <= k <= _hip.TOPK_MAX_K:
        raise ValueError(f"batch_size_{what} must lie in [1, {_hip.TOPK_MAX_K}], got {k}")
    if k > n_shared:
        raise ValueError(f"batch_size_{what} = {k} is larger than the {n_shared} {what} teacher and student share")


class _Sampler:
    """What the three samplers share: the teacher id -> student id mappings of the shared entities / relations, the top-k and
    random sizes with their checks, the device tables, the random columns, and ``get``.  A live sampler adds ``side``."""

    supervised = False  # the ground truth is not part of the distributions
    depends_on_teacher = True  # KdmkbModel.learn rebuilds it as the teacher trains

    def __init__(self, teacher_entities, teacher_relations, student_entities, student_relations, batch_size_entity,
                 batch_size_relation, n_random_entities, n_random_relations, device="cpu", seed=None, **kwargs):
        self.batch_size_entity_top_k, self.batch_size_relation_top_k = batch_size_entity, batch_size_relation
        self.n_random_entities, self.n_random_relations = n_random_entities, n_random_relations
        self.device = device
        self._rng = np.random.RandomState(seed)
        self.mapping_entities = _shared(teacher_entities, student_entities)
        self.mapping_relations = _shared(teacher_relations, student_relations)
        self.n_teacher_entities, self.n_teacher_relations = len(teacher_entities), len(teacher_relations)
        _check_k(batch_size_entity, len(self.mapping_entities), "entity")
        _check_k(batch_size_relation, len(self.mapping_relations), "relation")
        for what, n, shared in (("entities", n_random_entities, self.mapping_entities),
                                ("relations", n_random_relations, self.mapping_relations)):
            if n < 0 or n > len(shared):
                raise ValueError(f"n_random_{what} = {n} must lie in [0, {len(shared)}]")
        self._tables = {}

    def tables(self, device):
        """-> dict of device tables: ``ent_bits`` (the shared teacher entities as an mkb_topk_masked bitmask), ``ent_map`` /
        ``rel_map`` (teacher id -> student id, -1 = not shared), ``rel_t`` / ``rel_s`` (the shared relations, ascending teacher
        id, and their student ids)."""
        device = torch.device(device)
        tb = self._tables.get(device)
        if tb is None:
            def lookup(mapping, n):
                out = torch.full((n,), -1, dtype=torch.int64)
                out[torch.tensor(list(mapping.keys()), dtype=torch.int64)] = torch.tensor(list(mapping.values()), dtype=torch.int64)
                return out.to(device)
            rel_t = torch.tensor(sorted(self.mapping_relations), dtype=torch.int64)
            tb = self._tables[device] = {
                "ent_bits": candidate_bits(torch.tensor(list(self.mapping_entities), dtype=torch.int64), self.n_teacher_entities, device),
                "ent_map": lookup(self.mapping_entities, self.n_teacher_entities),
                "rel_map": lookup(self.mapping_relations, self.n_teacher_relations),
                "rel_t": rel_t.to(device),
                "rel_s": torch.tensor([self.mapping_relations[int(r)] for r in rel_t], dtype=torch.int64).to(device),
            }
        return tb

    def _check_teacher(self, teacher):
        if teacher.n_entity != self.n_teacher_entities or teacher.n_relation != self.n_teacher_relations:
            raise ValueError(f"the teacher's tables ({teacher.n_entity} entities, {teacher.n_relation} relations) do not match "
                             f"teacher_entities / teacher_relations ({self.n_teacher_entities}, {self.n_teacher_relations})")

    def _sync(self, teacher):
        """What ``get`` does to the teacher before it is scored: rows a row-lazy Adam has not brought current yet."""
        teacher.sync_parameters()

    def _k(self, part):
        return self.batch_size_relation_top_k if part == "relation" else self.batch_size_entity_top_k

    def _random_columns(self, b, dev, outs):
        """The random columns of the reference's ``_randomize_distribution`` (top_k_sampling.py:877-960): one draw of entities,
        then one of relations, per call, from the sampler's ``RandomState``; the same draw goes to every row."""
        head_t, rel_t, tail_t, head_s, rel_s, tail_s = outs

        def draw(mapping, n):
            t = self._rng.choice(list(mapping.keys()), size=n, replace=False)
            s = [mapping[i] for i in t]
            return (torch.as_tensor(np.asarray(x, dtype=np.int64)).to(dev).view(1, -1).expand(b, -1) for x in (t, s))

        if self.n_random_entities > 0:
            t, s = draw(self.mapping_entities, self.n_random_entities)
            head_t, tail_t = torch.cat([head_t, t], dim=1), torch.cat([tail_t, t], dim=1)
            head_s, tail_s = torch.cat([head_s, s], dim=1), torch.cat([tail_s, s], dim=1)
        if self.n_random_relations > 0:
            t, s = draw(self.mapping_relations, self.n_random_relations)
            rel_t, rel_s = torch.cat([rel_t, t], dim=1), torch.cat([rel_s, s], dim=1)
        return head_t, rel_t, tail_t, head_s, rel_s, tail_s

    @property
    def batch_size_entity(self):
        return self.batch_size_entity_top_k + self.n_random_entities

    @property
    def batch_size_relation(self):
        return self.batch_size_relation_top_k + self.n_random_relations

    def get(self, sample, teacher, **kwargs):
        """-> (head, relation, tail distributions of the teacher, then of the student): int64 on ``sample``'s device."""
        _hip.require_device(teacher.entity_embedding)
        self._check_teacher(teacher)
        out_dev = sample.device
        dev = teacher.entity_embedding.device
        self._sync(teacher)
        with torch.no_grad():
            s = sample.to(device=dev, dtype=torch.int64).reshape(-1, 3).contiguous()
            b = s.shape[0]
            if b:
                t_ids, s_ids = zip(*(self.side(part, s, teacher) for part in PARTS))
                outs = t_ids + s_ids
            else:
                outs = tuple(torch.empty((0, self._k(part)), dtype=torch.int64, device=dev) for part in PARTS + PARTS)
            outs = self._random_columns(b, dev, outs)
        return tuple(x.contiguous().to(out_dev) for x in outs)


class TopKSampling(_Sampler):
    """The teacher's top ``batch_size_entity`` heads and tails and top ``batch_size_relation`` relations of every triple of
    ``sample``, among the entities / relations teacher and student share, followed by ``n_random_entities`` /
    ``n_random_relations`` random shared ones (reference top_k_sampling.py:267-662).

    ``get(sample, teacher)`` -> six int64 tensors on ``sample``'s device: head, relation and tail candidates in teacher ids,
    then the same in student ids, ``[b, batch_size_entity]`` / ``[b, batch_size_relation]``.

    Two differences from the reference, both where it is ill-defined:
      - equal teacher scores are ordered by lower teacher id (the reference's ``argsort`` leaves their order unspecified);
      - the teacher relation list holds teacher relation ids.  The reference returns student ids there
        (``relations_student[rank_relations]``): the same list whenever both graphs number their shared relations alike;
        where they do not, it scores the teacher on the wrong relations or indexes out of its table.
    A top k larger than the number of shared entities / relations raises ``ValueError`` (the reference would return fewer
    columns and fail later)."""

    # The teachers whose relation side runs on mkb_rel_scores: where it was measured faster at B = 1024 by more than the general
    # route's spread (profiles/r14_relation_side_speed.txt).  A RotatE teacher keeps the general forward (0.404 against 0.376 ms:
    # 1,024 workgroups that each rebuild 237 rotated queries do not fill the device; the general forward's 242 k do).
    RELATION_KERNEL_MODELS = frozenset({"TransE", "ComplEx", "DistMult", "pRotatE"})

    def side(self, part, sample, teacher, chunk=1024):
        """-> (teacher ids, student ids) [b, k] of one part ("head", "relation" or "tail") for ``sample`` [b, 3] int64 on the
        teacher's device, ``chunk`` rows per launch: the teacher's k best shared entities / relations in that place.  No random
        columns, no synchronisation."""
        dev = teacher.entity_embedding.device
        tb = self.tables(dev)
        b, k = sample.shape[0], self._k(part)
        ids = torch.empty((b, k), dtype=torch.int64, device=dev)
        if part != "relation":  # the shared entities only, nothing filtered
            _launch(teacher, sample, f"{part}-batch", k, torch.empty(0, dtype=torch.int64, device=dev), 0, tb["ent_bits"], chunk, ids,
                    torch.empty((b, k), dtype=torch.float32, device=dev))
            return ids, tb["ent_map"][ids]
        rel_t, n_rel = tb["rel_t"], tb["rel_t"].numel()
        if teacher.name not in self.RELATION_KERNEL_MODELS:
            return self._relation_side_general(sample, teacher, chunk)
        score = torch.empty((min(b, chunk), n_rel), dtype=torch.float32, device=dev)
        for lo in range(0, b, chunk):  # mkb_rel_scores of [b, R_shared], then the block selection
            s = sample[lo: lo + chunk].contiguous()
            if not rel_scores_launch(teacher, s, rel_t, score[: s.shape[0]]):
                return self._relation_side_general(sample, teacher, chunk)
            topk_block(score[: s.shape[0]], k, ids=ids[lo: lo + chunk])
        return rel_t[ids], tb["rel_s"][ids]

    def _relation_side_general(self, sample, teacher, chunk=1024):
        """The relation side through the general forward of the ``[b, R_shared, 3]`` block: the route of teachers
        ``mkb_rel_scores`` does not support or was not measured faster for, and what the tests compare the kernel's route with."""
        dev = teacher.entity_embedding.device
        tb = self.tables(dev)
        b, k = sample.shape[0], self._k("relation")
        ids = torch.empty((b, k), dtype=torch.int64, device=dev)
        rel_t, n_rel = tb["rel_t"], tb["rel_t"].numel()
        for lo in range(0, b, chunk):  # the general forward of [b, R_shared, 3], then the block selection
            s = sample[lo: lo + chunk]
            block = torch.stack([s[:, 0:1].expand(-1, n_rel), rel_t.view(1, -1).expand(s.shape[0], -1),
                                 s[:, 2:3].expand(-1, n_rel)], dim=-1)
            score = teacher(block.contiguous()).reshape(s.shape[0], n_rel).float().contiguous()
            topk_block(score, k, ids=ids[lo: lo + chunk])
        return rel_t[ids], tb["rel_s"][ids]

    def top_k(self, sample, teacher, chunk=1024):
        """-> (heads, relations, tails) in teacher ids, then the same in student ids: the top-k columns only, on the teacher's
        device, for ``sample`` [b, 3] int64 on that device.  No random columns, no synchronisation."""
        t_ids, s_ids = zip(*(self.side(part, sample, teacher, chunk) for part in PARTS))
        return t_ids + s_ids


class TopKSamplingTransE(_Sampler):
    """The reference's sampler for a TransE teacher (top_k_sampling.py:680-875): for every triple of ``sample`` the
    ``batch_size_entity`` shared entities nearest in L2 to the teacher's translated queries ``t - r`` (heads) and ``h + r``
    (tails), the ``batch_size_relation`` shared relations nearest to ``t - h`` (``TransE._top_k``), then ``n_random_entities`` /
    ``n_random_relations`` random shared ones.  ``get(sample, teacher)`` -> the six int64 tensors of ``TopKSampling.get``.

    The reference's faiss ``IndexFlatL2`` is the device's exact squared-L2 k nearest rows (``mkb_topk_nearest``).  As in the
    reference, the index holds the shared rows of the teacher's tables as they are when the sampler is built, while the queries
    use the teacher's current tables (``KdmkbModel.learn`` rebuilds its samplers every ``update_distillation_every`` steps).

    One deviation: equal distances go to the lower teacher id (the index holds the shared rows in ascending teacher id).  The
    reference's index holds them in the teacher dict's order, and faiss leaves the order of equal distances unspecified.  A top k
    larger than the number of shared entities / relations raises ``ValueError``, as in ``TopKSampling``; so does a teacher that
    is not a TransE."""

    def __init__(self, teacher_entities, teacher_relations, student_entities, student_relations, teacher, batch_size_entity,
                 batch_size_relation, n_random_entities, n_random_relations, seed=None, device="cpu", **kwargs):
        super().__init__(teacher_entities, teacher_relations, student_entities, student_relations, batch_size_entity,
                         batch_size_relation, n_random_entities, n_random_relations, device=device, seed=seed)
        self._check_teacher(teacher)
        teacher.sync_parameters()
        with torch.no_grad():
            dev = teacher.entity_embedding.device
            shared = {"entity": torch.tensor(sorted(self.mapping_entities), dtype=torch.int64, device=dev),
                      "relation": torch.tensor(sorted(self.mapping_relations), dtype=torch.int64, device=dev)}
            tables = {"entity": teacher.entity_embedding, "relation": teacher.relation_embedding}
            # part -> (the index: the shared rows, ascending teacher id; their teacher ids; positions 0 .. n - 1)
            self._index = {part: (tables[part].detach()[ids].contiguous(), ids, torch.arange(ids.numel(), device=dev))
                           for part, ids in shared.items()}

    def _check_teacher(self, teacher):
        if teacher.name != "TransE":
            raise ValueError(f"TopKSamplingTransE needs a TransE teacher, got {teacher.name}")
        super()._check_teacher(teacher)

    def _sync(self, teacher):
        """Nothing: the constructor synchronised the teacher when it cut the index; ``get`` reads its tables as they are."""

    def side(self, part, sample, teacher):
        """-> (teacher ids, student ids) [b, k] of one part ("head", "relation" or "tail") for ``sample`` [b, 3] int64 on the
        teacher's device: the shared rows nearest to the part's translated query.  No random columns, no synchronisation."""
        index, t_ids, pos = self._index["relation" if part == "relation" else "entity"]
        q = teacher._top_k(sample)[PARTS.index(part)]
        near, _ = topk_nearest(q.reshape(sample.shape[0], -1).contiguous(), index, pos, self._k(part))
        t = t_ids[near]
        tb = self.tables(sample.device)
        return t, (tb["rel_map"] if part == "relation" else tb["ent_map"])[t]


class FastTopKSampling(_Sampler):
    """``TopKSampling`` precomputed over the teacher's training triples when it is built (reference top_k_sampling.py:9-264):
    for every distinct (r, t) of ``dataset_teacher``'s triples the teacher's top heads, for every distinct (h, t) its top
    relations, for every distinct (h, r) its top tails -- on the device, ``chunk`` queries at a time.  ``get`` looks the rows of
    a sample up (``KeyError`` for a key that was not precomputed, like the reference's dicts) and appends the random columns.

    Building it walks ``dataset_teacher`` once as the reference does (its loaders draw their seeds from torch's global generator
    when their iterators are created), so a seeded run keeps the reference's batch order.  A TransE teacher takes the sampler the
    reference hands it to, ``TopKSamplingTransE``, when ``transe_sampler=distillation.TopKSamplingTransE`` is passed; without
    it a TransE teacher raises ``ImportError``, as the reference does without faiss.  Other teachers ignore ``transe_sampler``."""

    def __init__(self, teacher_entities, teacher_relations, student_entities, student_relations, batch_size_entity,
                 batch_size_relation, n_random_entities, n_random_relations, dataset_teacher, teacher, device="cpu", seed=None,
                 chunk=1024, transe_sampler=None, **kwargs):
        transe = teacher.name == "TransE"
        if transe and transe_sampler is None:
            raise ImportError("FastTopKSampling with a TransE teacher needs the faiss L2 index of the reference's "
                              "TopKSamplingTransE (No module named 'faiss'); pass transe_sampler=distillation.TopKSamplingTransE "
                              "for the device's exact L2 index, or use another teacher or TopKSampling")
        kw = dict(teacher_entities=teacher_entities, teacher_relations=teacher_relations, student_entities=student_entities,
                  student_relations=student_relations, batch_size_entity=batch_size_entity, batch_size_relation=batch_size_relation,
                  device=device, seed=seed)
        super().__init__(n_random_entities=n_random_entities, n_random_relations=n_random_relations, **kw)
        # whose ``side`` answers "the k candidates of this part for these queries"
        base = (transe_sampler if transe else TopKSampling)(teacher=teacher, n_random_entities=0, n_random_relations=0, **kw)
        _hip.require_device(teacher.entity_embedding)
        base._check_teacher(teacher)
        # the reference's pass over the teacher's training batches (its dicts are filled from the head-batch ones)
        batches = [data["sample"] for data in dataset_teacher if data["mode"] == "head-batch"]
        dev = teacher.entity_embedding.device
        N, R = teacher.n_entity, teacher.n_relation
        tri = torch.cat(batches).to(device=dev, dtype=torch.int64) if batches else torch.empty((0, 3), dtype=torch.int64, device=dev)
        h, r, t = tri[:, 0], tri[:, 1], tri[:, 2]
        teacher.sync_parameters()
        self._keys = {}
        self._N, self._R = N, R
        zero = torch.zeros_like
        with torch.no_grad():  # per part: its distinct keys, a query row per key (the part's own column is a placeholder)
            for part, key, row in (("head", r * N + t, lambda u: (zero(u), u // N, u % N)),
                                   ("relation", h * N + t, lambda u: (u // N, zero(u), u % N)),
                                   ("tail", h * R + r, lambda u: (u // R, u % R, zero(u)))):
                u = torch.unique(key)
                q = torch.stack(row(u), 1).contiguous()
                t_ids, s_ids = (torch.empty((u.numel(), self._k(part)), dtype=torch.int64, device=dev) for _ in range(2))
                for lo in range(0, u.numel(), chunk):
                    t_ids[lo: lo + chunk], s_ids[lo: lo + chunk] = base.side(part, q[lo: lo + chunk], teacher)
                self._keys[part] = (u, t_ids, s_ids)

    def _rows(self, part, key):
        keys, t, s = self._keys[part]
        if keys.numel() == 0:
            raise KeyError(f"no {part} distribution was precomputed")
        key = key.to(keys.device)
        pos = torch.searchsorted(keys, key).clamp_(max=keys.numel() - 1)
        missing = keys[pos] != key
        if bool(missing.any()):
            raise KeyError(f"{part} distribution of a triple whose key was not among the teacher's training triples")
        return t[pos], s[pos]

    def get(self, sample, **kwargs):
        """-> (head, relation, tail distributions of the teacher, then of the student): int64 on ``sample``'s device."""
        out_dev = sample.device
        dev = self._keys["head"][0].device
        s = sample.to(device=dev, dtype=torch.int64).reshape(-1, 3)
        h, r, t = s[:, 0], s[:, 1], s[:, 2]
        (head_t, head_s), (rel_t, rel_s), (tail_t, tail_s) = (
            self._rows(part, key) for part, key in zip(PARTS, (r * self._N + t, h * self._N + t, h * self._R + r)))
        outs = self._random_columns(s.shape[0], dev, (head_t, rel_t, tail_t, head_s, rel_s, tail_s))
        return tuple(x.contiguous().to(out_dev) for x in outs)
