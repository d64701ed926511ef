"""``Evaluation`` -- filtered link-prediction metrics MRR / MR / HITS@1/3/10 (reference
mkb/evaluation/evaluation.py:137-279) with the same constructor and return dictionaries.

``eval`` on a ROCm device runs ``mkb_rank``: every test triple is scored against ALL entity rows by a tiled HIP
kernel (no ``[B, N, D]`` gather, no per-item python loop over ``n_entity`` candidates as in
``datasets.base.TestDataset``, base.py:196-241) and the filtered rank is counted on the device; exact score ties
count in the target's favour.  ``eval_relations`` runs ``mkb_rel_rank`` the same way (``relation_ranks``).
``force_reference_path = True`` takes the reference's route instead: ``TestDataset`` candidate lists + filter bias,
``model(sample, negative_sample, mode)`` through the general HIP forward, rank read off a descending argsort
(evaluation.py:245-262).
"""
import collections

import numpy as np
import torch
from torch.utils import data

from .. import _hip
from ..datasets import base
from ..models.base import BaseModel
from ..utils import Bar, Mean, predict_top_k, predict_top_k_relations, true_keys

__all__ = ["Evaluation"]


def _metrics():
    return collections.OrderedDict({m: Mean() for m in ["MRR", "MR", "HITS@1", "HITS@3", "HITS@10"]})


def _update(metrics, ranks):
    """Add the 1-based ``ranks`` (a list) to the five running means."""
    for ranking in ranks:
        metrics["MRR"].update(1.0 / ranking)
        metrics["MR"].update(ranking)
        metrics["HITS@1"].update(1.0 if ranking <= 1 else 0.0)
        metrics["HITS@3"].update(1.0 if ranking <= 3 else 0.0)
        metrics["HITS@10"].update(1.0 if ranking <= 10 else 0.0)


def _report(metrics, suffix=""):
    return {f"{name}{suffix}": round(metric.get(), 4) for name, metric in metrics.items()}


_MODES = ("head-batch", "tail-batch")
_TYPES = ("1_1", "1_M", "M_1", "M_M")
_METRICS = ("MRR", "MR", "HITS@1", "HITS@3", "HITS@10")
# the models whose relation_ranks runs on mkb_rel_rank by default: all five were measured faster on FB15k-237's test split by more
# than the torch route's spread (profiles/r14_relation_side_speed.txt)
RELATION_KERNEL_MODELS = frozenset({"TransE", "RotatE", "ComplEx", "DistMult", "pRotatE"})
_FANOUT_CACHE = []  # [(true_triples, len, device or None, n_entity, n_relation, counts)], most recent first


def _from_sums(counts, rr_sum):
    """The five rounded metrics of one group from ``mkb_rank_metrics``' sums (items, rank sum, ranks <= 1, <= 3, <= 10; sum of
    1 / rank); 0.0 for a group without items, like a fresh ``Mean``."""
    n = int(counts[0])
    means = [float(rr_sum) / n] + [int(c) / n for c in counts[1:]] if n else [0.0] * 5
    return {name: round(value, 4) for name, value in zip(_METRICS, means)}


class Evaluation:
    def __init__(self, entities, relations, batch_size, true_triples=[], device="cpu", num_workers=1):
        self.entities = entities
        self.relations = relations
        self.true_triples = true_triples
        self.batch_size = batch_size
        self.device = device
        self.num_workers = num_workers

    def _get_test_loader(self, triples, mode):
        test_dataset = base.TestDataset(triples=triples, true_triples=self.true_triples, entities=self.entities,
                                        relations=self.relations, mode=mode)
        return data.DataLoader(dataset=test_dataset, batch_size=self.batch_size, num_workers=self.num_workers,
                               collate_fn=base.TestDataset.collate_fn)

    def get_entity_stream(self, dataset):
        return [self._get_test_loader(dataset, "head-batch"), self._get_test_loader(dataset, "tail-batch")]

    def get_relation_stream(self, dataset):
        test_dataset = base.TestDatasetRelation(triples=dataset, true_triples=self.true_triples,
                                                entities=self.entities, relations=self.relations)
        return data.DataLoader(dataset=test_dataset, batch_size=self.batch_size, num_workers=self.num_workers,
                               collate_fn=base.TestDatasetRelation.collate_fn)

    # ------------------------------------------------------------------ device ranking (mkb_rank)
    def ranks(self, model, dataset, mode, chunk=1024, with_scores=False):
        """Filtered rank (1-based) of every triple of ``dataset`` in ``mode``, computed on the device: int64 tensor.
        ``with_scores=True`` -> ``(ranks, scores [n, n_entity])``: the scores of every triple against all entities the ranks
        were counted on (``mkb_rank_scores``; what ``model(sample, all entities, mode)`` returns at evaluation.py:237, before the
        filter bias)."""
        dev = model.entity_embedding.device
        _hip.require_device(model.entity_embedding)
        model.sync_parameters()
        keys = true_keys(self.true_triples, dev, model.n_entity, model.n_relation)[mode]
        triples = torch.as_tensor(np.asarray(dataset, dtype=np.int64).reshape(-1, 3), device=dev)
        out = torch.empty(len(triples), dtype=torch.int64, device=dev)
        scores = torch.empty((len(triples), model.n_entity), dtype=torch.float32, device=dev) if with_scores else None
        lib, tb, ws = _hip.lib(), model._tables(), _hip.Workspace(dev)
        name = "mkb_rank_scores" if with_scores else "mkb_rank"
        fn = getattr(lib, name)
        with _hip.on_device(dev):
            for lo in range(0, len(triples), chunk):
                s = triples[lo: lo + chunk].contiguous()
                need = lib.mkb_rank_workspace_bytes(tb, s.shape[0])
                block = (_hip.ptr(scores[lo: lo + chunk]),) if with_scores else ()  # (the score rows follow the ranks)
                _hip.check(fn(tb, _hip.ptr(s), s.shape[0], _hip.mode_id(mode), _hip.ptr(keys), keys.numel(),
                              _hip.ptr(out[lo: lo + chunk]), *block, ws.ptr(need), need, _hip.stream_ptr()), name)
        return (out, scores) if with_scores else out

    def top_k(self, model, dataset, mode, k, keep_target=True, chunk=1024):
        """The k best candidates of every triple of ``dataset`` in ``mode`` on the device, filtered by ``true_triples`` (with
        ``keep_target=True`` the candidate set ``ranks`` counts on: wherever the target's rank is at most k, it sits at that
        position) -> ``(ids [n, k], scores [n, k])``; see ``utils.predict_top_k``."""
        return predict_top_k(model, dataset, mode, k, true_triples=self.true_triples, keep_target=keep_target, chunk=chunk)

    def _device_ok(self, model):
        units = model.hidden_dim if model.name == "RotatE" else model.entity_dim
        return (isinstance(model, BaseModel) and model.entity_embedding.is_cuda and str(self.device) != "cpu"
                and units <= 4096 and len(self.true_triples) > 0)

    def eval(self, model, dataset):
        metrics = _metrics()
        if self._device_ok(model) and not getattr(self, "force_reference_path", False):
            with torch.no_grad():
                for mode in ("head-batch", "tail-batch"):  # same order as get_entity_stream
                    # The reference creates one DataLoader iterator per side here, and each creation draws one int64
                    # from torch's global CPU generator (the workers' base seed).  Draw it too, so that a training
                    # run interleaved with evaluations keeps shuffling its batches exactly like the reference.
                    torch.empty((), dtype=torch.int64).random_()
                    _update(metrics, self.ranks(model, dataset, mode).tolist())
            return _report(metrics)
        with torch.no_grad():
            for test_set in self.get_entity_stream(dataset):
                metrics = self.compute_score(model=model, test_set=test_set, metrics=metrics, device=self.device)
        return _report(metrics)

    def top_k_relations(self, model, dataset, k, keep_target=True, chunk=4096):
        """The k best relations of every ``(h, ?, t)`` of ``dataset`` on the device, filtered by ``true_triples`` (with
        ``keep_target=True`` the candidate set ``relation_ranks`` counts on: wherever the target's rank is at most k, it sits at
        that position) -> ``(ids [n, k], scores [n, k])``; see ``utils.predict_top_k_relations``."""
        return predict_top_k_relations(model, dataset, k, true_triples=self.true_triples, keep_target=keep_target, chunk=chunk)

    def relation_ranks(self, model, dataset, chunk=4096, with_scores=False):
        """Filtered rank (1-based) of the true relation of every triple among all relations, on the device: what
        ``compute_score`` does with the ``relation-batch`` stream (datasets/base.py:254-305: the other true relations of
        (h, ., t) are replaced by the target relation and biased by -1), without the per-item host loop.  One ``mkb_rel_rank``
        call per ``chunk`` triples (csrc/score_relation.hip: one workgroup per (h, ?, t) scores all relations, the filter is a
        bitmask, one wave counts the rank); the scores, and so the ranks, are those of ``_relation_ranks_torch``, which stays
        the route of shapes the kernel does not support.  ``with_scores=True`` -> ``(ranks, scores [n, n_relation])``: the block
        the ranks were counted on, before the filter.

        ``RELATION_KERNEL_MODELS`` names the models whose default route the kernel is (where it was measured faster, DESIGN
        section 5); the others keep ``_relation_ranks_torch``.  Both give the same ranks."""
        found = self._relation_ranks_kernel(model, dataset, chunk, with_scores) if model.name in RELATION_KERNEL_MODELS else None
        return self._relation_ranks_torch(model, dataset, chunk, with_scores) if found is None else found

    def _relation_ranks_kernel(self, model, dataset, chunk=4096, with_scores=False):
        """``relation_ranks`` on ``mkb_rel_rank``; None when the library does not support the model's rows."""
        dev = model.entity_embedding.device
        _hip.require_device(model.entity_embedding)
        model.sync_parameters()
        n_ent, n_rel = model.n_entity, model.n_relation
        triples = torch.as_tensor(np.asarray(dataset, dtype=np.int64).reshape(-1, 3), device=dev).contiguous()
        limits = torch.tensor([n_ent, n_rel, n_ent], device=dev)
        if len(triples) and bool(((triples < 0) | (triples >= limits)).any()):
            raise ValueError("dataset holds an entity or relation id outside the model's tables")
        keys = true_keys(self.true_triples, dev, n_ent, n_rel)["tail-batch"]  # sorted (h * R + r) * N + t
        out = torch.empty(len(triples), dtype=torch.int64, device=dev)
        scores = torch.empty((len(triples), n_rel), dtype=torch.float32, device=dev) if with_scores else None
        lib, tb, ws = _hip.lib(), model._tables(), _hip.Workspace(dev)
        with _hip.on_device(dev):
            for lo in range(0, len(triples), chunk):
                s = triples[lo: lo + chunk]
                need = lib.mkb_rel_rank_workspace_bytes(tb, s.shape[0])
                rc = lib.mkb_rel_rank(tb, _hip.ptr(s), s.shape[0], _hip.ptr(keys), keys.numel(), _hip.ptr(out[lo: lo + chunk]),
                                      _hip.ptr(scores[lo: lo + chunk]) if with_scores else None, ws.ptr(need), need,
                                      _hip.stream_ptr())
                if rc == _hip.ERR_UNSUPPORTED:  # rows too long for the kernel: nothing was launched
                    return None
                _hip.check(rc, "mkb_rel_rank")
        return (out, scores) if with_scores else out

    def _relation_ranks_torch(self, model, dataset, chunk=4096, with_scores=False):
        """``relation_ranks`` as torch glue around the general forward of the ``[b, R, 3]`` block of every chunk: the route of
        shapes ``mkb_rel_rank`` does not support, and the device oracle of its tests."""
        dev = model.entity_embedding.device
        n_ent, n_rel = model.n_entity, model.n_relation
        keys = true_keys(self.true_triples, dev, n_ent, n_rel)["tail-batch"]  # sorted (h * R + r) * N + t
        triples = torch.as_tensor(np.asarray(dataset, dtype=np.int64).reshape(-1, 3), device=dev)
        cand = torch.arange(n_rel, device=dev)
        out, blocks = [], []
        for lo in range(0, len(triples), chunk):
            s = triples[lo: lo + chunk]
            h, r, t = s[:, 0:1], s[:, 1:2], s[:, 2:3]
            k = (h * n_rel + cand) * n_ent + t                       # [b, R] keys of (h, r', t)
            pos = torch.searchsorted(keys, k.reshape(-1)).clamp_(max=keys.numel() - 1).view_as(k)
            true = keys[pos] == k
            rel = torch.where(true, r.expand_as(k), cand.expand_as(k))
            bias = torch.where(true & (cand != r), -1.0, 0.0)
            neg = torch.stack([h.expand_as(k), rel, t.expand_as(k)], dim=-1)  # [b, R, 3]
            score = model(neg.contiguous()) + bias
            if with_scores:  # the block before the filter: one more forward, of (h, r', t) itself
                blocks.append(model(torch.stack([h.expand_as(k), cand.expand_as(k), t.expand_as(k)], dim=-1).contiguous()))
            # position in a stable descending sort with NaN first (see ranks_before in csrc/rank.hip): a collapsed or
            # diverged model must not rank its targets first
            key = torch.nan_to_num(score, nan=float("inf"), posinf=float("inf"))
            target = key.gather(1, r)
            before = (key > target) | ((key == target) & (cand < r))
            out.append(1 + before.sum(dim=1))
        ranks = torch.cat(out) if out else torch.empty(0, dtype=torch.int64, device=dev)
        if with_scores:
            return ranks, (torch.cat(blocks) if blocks else torch.empty((0, n_rel), dtype=torch.float32, device=dev))
        return ranks

    def eval_relations(self, model, dataset):
        metrics = _metrics()
        if self._device_ok(model) and not getattr(self, "force_reference_path", False) and len(dataset) > 0:
            with torch.no_grad():
                torch.empty((), dtype=torch.int64).random_()  # the reference's DataLoader iterator draws its base seed
                _update(metrics, self.relation_ranks(model, dataset).tolist())
            return _report(metrics, "_relations")
        with torch.no_grad():
            metrics = self.compute_score(model=model, test_set=self.get_relation_stream(dataset), metrics=metrics,
                                         device=self.device)
        return _report(metrics, "_relations")

    @classmethod
    def compute_score(cls, model, test_set, metrics, device):
        training = model.training
        if training:
            model = model.eval()
        bar = Bar(dataset=test_set, update_every=1)
        bar.set_description("Evaluation")
        for batch in bar:
            sample = batch["sample"].to(device)
            negative_sample = batch["negative_sample"].to(device)
            filter_bias = batch["filter_bias"].to(device)
            mode = batch["mode"]
            if mode == "relation-batch":
                score = model(negative_sample)
                positive_arg = sample[:, 1]
            else:
                score = model(sample=sample, negative_sample=negative_sample, mode=mode)
                positive_arg = sample[:, 0] if mode == "head-batch" else sample[:, 2]
            score = score + filter_bias
            argsort = torch.argsort(score, dim=1, descending=True)
            hit = argsort == positive_arg.unsqueeze(1)
            assert bool((hit.sum(dim=1) == 1).all())
            _update(metrics, (hit.float().argmax(dim=1) + 1).tolist())  # one D2H copy per batch
        if training:
            model = model.train()
        return metrics

    # ------------------------------------------------------------------ grouped report (reference evaluation.py:282-464)
    def _grouped_on_device(self, model):
        return isinstance(model, BaseModel) and self._device_ok(model) and not getattr(self, "force_reference_path", False)

    def _fanout(self, model):
        """``int64 [R, 3]`` per relation id: its true triples (with multiplicity), its distinct (tail, relation) pairs, its
        distinct (head, relation) pairs -- the three counts the reference's two pandas group-bys reduce to.  On the device from
        ``mkb_relation_fanout`` over the triples and the sorted keys of ``utils.true_keys``; otherwise numpy on the same
        definition.  Cached like the keys: per triple collection (the same object with the same length), device and table size."""
        n_ent, n_rel = len(self.entities), len(self.relations)
        dev = model.entity_embedding.device if self._grouped_on_device(model) else None
        n = len(self.true_triples)
        for j, (obj, length, d, ne, nr, counts) in enumerate(_FANOUT_CACHE):
            if obj is self.true_triples and length == n and d == dev and ne == n_ent and nr == n_rel:
                _FANOUT_CACHE.insert(0, _FANOUT_CACHE.pop(j))
                return counts
        a = np.asarray(self.true_triples, dtype=np.int64).reshape(-1, 3)
        if dev is not None:
            keys = true_keys(self.true_triples, dev, n_ent, n_rel)
            head, tail = keys["head-batch"], keys["tail-batch"]
            triples = torch.as_tensor(a, device=dev)
            out = torch.empty((n_rel, 3), dtype=torch.int64, device=dev)
            with _hip.on_device(dev):
                _hip.check(_hip.lib().mkb_relation_fanout(_hip.ptr(triples), len(a), _hip.ptr(head), head.numel(), _hip.ptr(tail),
                                                          tail.numel(), n_ent, n_rel, _hip.ptr(out), _hip.stream_ptr()),
                           "mkb_relation_fanout")
            counts = out.cpu().numpy()
        else:
            a = a[(a[:, 1] >= 0) & (a[:, 1] < n_rel)]
            h, r, t = a[:, 0], a[:, 1], a[:, 2]
            counts = np.stack([np.bincount(r, minlength=n_rel), np.bincount(np.unique(t * n_rel + r) % n_rel, minlength=n_rel),
                               np.bincount(np.unique(h * n_rel + r) % n_rel, minlength=n_rel)], axis=1).astype(np.int64)
        _FANOUT_CACHE.insert(0, (self.true_triples, n, dev, n_ent, n_rel, counts))
        del _FANOUT_CACHE[4:]
        return counts

    def types_relations(self, model, dataset, threshold=1.5):
        """``{relation name: "1_1" | "1_M" | "M_1" | "M_M"}`` over ``true_triples`` (Bordes et al. 2013; reference
        evaluation.py:342-383).  The first character is "1" when a (relation, tail) pair has at most ``threshold`` heads on
        average -- the relation's triples, each occurrence counted, over its distinct (tail, relation) pairs -- and "M"
        otherwise; the second character says the same of the tails per (head, relation) pair.

        The result is keyed by relation id: a relation that never occurs in ``true_triples`` is left out.  The reference keys
        its frame by the row index after ``reset_index()``, which is the relation id only when every relation id occurs: then
        the two agree; otherwise the reference shifts the categories onto the wrong relations."""
        counts = self._fanout(model)
        name_of = {value: key for key, value in self.relations.items()}
        out = {}
        for r in np.flatnonzero(counts[:, 0] > 0).tolist():
            n, per_tail, per_head = (float(c) for c in counts[r])
            out[name_of[r]] = ("1" if n / per_tail <= threshold else "M") + "_" + ("1" if n / per_head <= threshold else "M")
        return out

    def _group_sums(self, model, dataset, group_of_relation, n_groups):
        """Per mode ``(int64 [G, 5], float64 [G])``: the items of each group, their rank sum, the ranks <= 1, <= 3, <= 10, and
        the sum of 1 / rank.  ``ranks`` per mode as ``eval`` computes them (with its generator draw per side), then one
        ``mkb_rank_metrics`` launch on the whole rank tensor and one read-back of ``6 G`` numbers."""
        dev = model.entity_embedding.device
        table = torch.as_tensor(np.asarray(group_of_relation, dtype=np.int32), device=dev)
        triples = torch.as_tensor(np.asarray(dataset, dtype=np.int64).reshape(-1, 3), device=dev)
        out = {}
        with torch.no_grad():
            for mode in _MODES:  # same order as get_entity_stream
                torch.empty((), dtype=torch.int64).random_()  # see eval: the reference's DataLoader iterator draws its base seed
                ranks = self.ranks(model, dataset, mode)
                buf = torch.empty(6 * n_groups, dtype=torch.int64, device=dev)  # counts [G, 5] int64, then sum of 1 / rank [G] double
                with _hip.on_device(dev):
                    _hip.check(_hip.lib().mkb_rank_metrics(_hip.ptr(ranks), _hip.ptr(triples), len(triples), _hip.ptr(table),
                                                           table.numel(), n_groups, _hip.ptr(buf), _hip.ptr(buf[5 * n_groups:]),
                                                           _hip.stream_ptr()), "mkb_rank_metrics")
                host = buf.cpu().numpy()
                out[mode] = (host[: 5 * n_groups].reshape(n_groups, 5), host[5 * n_groups:].view(np.float64))
        return out

    @classmethod
    def compute_detailled_score(cls, model, test_set, metrics, types_relations, device):
        """The reference's method (evaluation.py:281-340): ``compute_score`` with the five means kept per
        ``metrics[mode][types_relations[relation id]]``.  An item whose relation has no category (it never occurs in
        ``true_triples``; the reference raises ``KeyError``) is left out."""
        training = model.training
        if training:
            model = model.eval()
        bar = Bar(dataset=test_set, update_every=1)
        bar.set_description("Evaluation")
        for batch in bar:
            sample = batch["sample"].to(device)
            negative_sample = batch["negative_sample"].to(device)
            filter_bias = batch["filter_bias"].to(device)
            mode = batch["mode"]
            score = model(sample=sample, negative_sample=negative_sample, mode=mode) + filter_bias
            argsort = torch.argsort(score, dim=1, descending=True)
            positive_arg = sample[:, 0] if mode == "head-batch" else sample[:, 2]
            hit = argsort == positive_arg.unsqueeze(1)
            assert bool((hit.sum(dim=1) == 1).all())
            found = torch.stack([hit.float().argmax(dim=1) + 1, sample[:, 1]], dim=1).tolist()  # one D2H copy per batch
            for ranking, relation in found:
                if relation in types_relations:
                    _update(metrics[mode][types_relations[relation]], [ranking])
        if training:
            model = model.train()
        return metrics

    def detail_metrics(self, model, dataset, threshold=1.5):
        """``detail_eval`` as a plain nested dict: ``{"head-batch" | "tail-batch": {"1_1" | "1_M" | "M_1" | "M_M": {"MRR", "MR",
        "HITS@1", "HITS@3", "HITS@10"}}}`` of the items of ``dataset`` whose relation is of that category (``types_relations``),
        rounded to 4 places, 0.0 for a category without items, plus ``"frequency": {category: share of the relations}``.

        On a ROCm device (the conditions of ``eval``) the ranks stay on the device and ``mkb_rank_metrics`` reduces them per
        category; otherwise (or with ``force_reference_path = True``) ``compute_detailled_score`` walks the reference's stream."""
        type_of = {self.relations[name]: kind for name, kind in self.types_relations(model, dataset, threshold).items()}
        if self._grouped_on_device(model):
            table = np.full(len(self.relations), -1, dtype=np.int32)
            for relation, kind in type_of.items():
                table[relation] = _TYPES.index(kind)
            sums = self._group_sums(model, dataset, table, len(_TYPES))
            out = {mode: {kind: _from_sums(sums[mode][0][g], sums[mode][1][g]) for g, kind in enumerate(_TYPES)} for mode in _MODES}
        else:
            metrics = {mode: {kind: _metrics() for kind in _TYPES} for mode in _MODES}
            with torch.no_grad():
                for test_set in self.get_entity_stream(dataset):
                    metrics = self.compute_detailled_score(model=model, test_set=test_set, metrics=metrics, types_relations=type_of,
                                                           device=self.device)
            out = {mode: {kind: _report(metrics[mode][kind]) for kind in _TYPES} for mode in _MODES}
        kinds = list(type_of.values())
        out["frequency"] = {kind: kinds.count(kind) / len(kinds) if kinds else 0.0 for kind in _TYPES}
        return out

    def detail_eval(self, model, dataset, threshold=1.5):
        """The reference's table (evaluation.py:385-464): a ``pandas.DataFrame`` with the categories ``1_1 .. M_M`` as index
        (named ``relation``), the column blocks ``head`` / ``tail`` x MRR, MR, HITS@1, HITS@3, HITS@10 and
        ``("metadata", "frequency")``; the numbers of ``detail_metrics``.  (The reference names the index too, but its last
        ``concat`` with the unnamed frequency frame drops the name again; here it stays.)"""
        import pandas as pd  # here only: the package imports without pandas

        found = self.detail_metrics(model, dataset, threshold)
        columns = [(side, metric) for side in ("head", "tail") for metric in _METRICS] + [("metadata", "frequency")]
        rows = [[found[mode][kind][metric] for mode in _MODES for metric in _METRICS] + [found["frequency"][kind]] for kind in _TYPES]
        return pd.DataFrame(rows, index=pd.Index(_TYPES, name="relation"), columns=pd.MultiIndex.from_tuples(columns))

    def eval_per_relation(self, model, dataset):
        """``{relation name: {"head-batch": {MRR, MR, HITS@1, HITS@3, HITS@10, "count"}, "tail-batch": {...}}}``: the filtered
        metrics of ``eval`` for the items of each relation (``mkb_rank_metrics`` with one group per relation); on a ROCm device
        only."""
        _hip.require_device(model.entity_embedding)
        n_rel = len(self.relations)
        sums = self._group_sums(model, dataset, np.arange(n_rel, dtype=np.int32), n_rel)
        return {name: {mode: {**_from_sums(sums[mode][0][r], sums[mode][1][r]), "count": int(sums[mode][0][r][0])} for mode in _MODES}
                for name, r in self.relations.items()}
