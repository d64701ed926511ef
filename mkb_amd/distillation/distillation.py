"""``Distillation`` -- knowledge distillation between two KGE models that share part of their entities / relations
(reference mkb/distillation/distillation.py:12-683; called from ``KdmkbModel.forward``, kdmkb_model.py:337-349).

For every positive triple of the teacher's batch whose parts both graphs know, three candidate lists are scored by teacher
and student -- P(head | r, t), P(relation | h, t), P(tail | h, r) -- and the student is pulled towards the teacher with
``losses.KlDivergence``.  The reference assembles the ``[n, candidates, 3]`` index tensors triple by triple on the host
(``.item()`` per element, deep copies, ``torch.stack`` of python lists); here they are built for the whole batch with a few
tensor operations on the device, from the same sampled candidates (``distillation_tensors``).  ``distill`` does not write them
out: a part is its rows ``[n, 3]`` and its lists ``[n, m]`` (``distillation_candidates``), scored by
``BaseModel.score_candidates`` (``mkb_cand_score_fwd`` / ``mkb_cand_score_bwd``), which reads the two rows a row's candidates
share once and has the bits of the 3-D sample (models/base.py:146-151) through ``mkb_score_fwd``.  Same numbers: tests pin the
tensors and the loss to captures of the reference.
"""
import collections

import torch

from ..losses import KlDivergence
from ..models.base import PARTS, BaseModel

__all__ = ["Distillation"]


class Distillation:
    # model name -> the parts ``distill`` scores with ``BaseModel.score_candidates``: the (model, part) cells in which that route
    # was measured ahead of the block route by more than the block route's own spread (profiles/r16_distill_slot_routes.txt)
    SLOT_KERNEL_ROUTES = {name: ("head", "relation", "tail") for name in ("TransE", "RotatE", "ComplEx", "DistMult", "pRotatE")}

    def __init__(self, teacher_entities, student_entities, teacher_relations, student_relations, sampling, device="cpu"):
        self.teacher_entities, self.student_entities = teacher_entities, student_entities
        self.teacher_relations, self.student_relations = teacher_relations, student_relations
        self.sampling, self.device = sampling, device
        shared = lambda t, s: collections.OrderedDict((i, s[label]) for label, i in t.items() if label in s)
        self.mapping_entities = shared(teacher_entities, student_entities)      # teacher id -> student id
        self.mapping_relations = shared(teacher_relations, student_relations)
        self._tables = {}

    # ------------------------------------------------------------------ which parts of a triple can be distilled
    def available(self, head, relation, tail):
        h, r, t = head in self.mapping_entities, relation in self.mapping_relations, tail in self.mapping_entities
        if self.sampling.supervised:  # the ground truth sits in every list: all three parts must be shared
            return dict.fromkeys(("head", "relation", "tail"), h and r and t)
        return {"head": r and t, "relation": h and t, "tail": h and r}

    def _lookup(self, device):
        """teacher id -> student id as dense device tables (-1 = not shared)."""
        tb = self._tables.get(device)
        if tb is None:
            def table(mapping, n):
                out = torch.full((n,), -1, dtype=torch.int64)
                if mapping:
                    out[torch.tensor(list(mapping.keys()))] = torch.tensor(list(mapping.values()))
                return out.to(device)
            tb = self._tables[device] = (table(self.mapping_entities, len(self.teacher_entities)),
                                         table(self.mapping_relations, len(self.teacher_relations)))
        return tb

    def distillation_candidates(self, sample, teacher=None):
        """-> {"head" | "relation" | "tail": (teacher rows [n, 3], teacher candidates [n, m], student rows, student candidates)}
        int64 on ``sample``'s device, for the rows of ``sample`` (teacher ids) each part is available for; parts without rows are
        absent.  Row i of a part stands for the m triples that put ``candidates[i, j]`` into the part's column of ``rows[i]``
        (``distillation_tensors`` writes them out); the other two columns are the same for all m."""
        dev = sample.device
        ent_map, rel_map = self._lookup(dev)
        drawn = self.sampling.get(sample=sample, mapping_entities=self.mapping_entities, mapping_relations=self.mapping_relations,
                                  positive_sample_size=sample.shape[0], teacher=teacher)
        head_t, rel_t, tail_t, head_s, rel_s, tail_s = (d.to(device=dev, dtype=torch.int64) for d in drawn)
        h, r, t = sample[:, 0], sample[:, 1], sample[:, 2]
        hs, rs, ts = ent_map[h], rel_map[r], ent_map[t]
        ok_h, ok_r, ok_t = hs >= 0, rs >= 0, ts >= 0
        if self.sampling.supervised:
            every = ok_h & ok_r & ok_t
            rows = {"head": every, "relation": every, "tail": every}
        else:
            rows = {"head": ok_r & ok_t, "relation": ok_h & ok_t, "tail": ok_h & ok_r}
        out = {}
        for part, cand_t, cand_s, truth_t, truth_s in (("head", head_t, head_s, h, hs), ("relation", rel_t, rel_s, r, rs),
                                                       ("tail", tail_t, tail_s, t, ts)):
            keep = rows[part]
            if not bool(keep.any()):
                continue
            ct, cs = cand_t[keep].clone(), cand_s[keep].clone()
            if self.sampling.supervised:  # the ground truth takes the last slot (distillation.py:313-314, 331-333)
                ct[:, -1], cs[:, -1] = truth_t[keep], truth_s[keep]
            out[part] = (torch.stack([h[keep], r[keep], t[keep]], dim=1), ct, torch.stack([hs[keep], rs[keep], ts[keep]], dim=1), cs)
        return out

    @staticmethod
    def _block(rows, cand, part):
        """The ``[n, m, 3]`` triples of a part: ``rows`` with the part's column replaced by each candidate."""
        block = rows.unsqueeze(1).expand(-1, cand.shape[1], -1).clone()
        block[:, :, PARTS[part]] = cand
        return block

    def distillation_tensors(self, sample, teacher=None):
        """-> {"head" | "relation" | "tail": (teacher [n, m, 3], student [n, m, 3])} int64 on ``sample``'s device, for the
        rows of ``sample`` (teacher ids) each part is available for; parts without rows are absent."""
        return {part: (self._block(rows_t, cand_t, part), self._block(rows_s, cand_s, part))
                for part, (rows_t, cand_t, rows_s, cand_s) in self.distillation_candidates(sample, teacher=teacher).items()}

    @classmethod
    def _scores(cls, model, rows, cand, part):
        """A model's scores of a part's candidate lists: ``score_candidates`` where it was measured ahead for the model and the
        part (``SLOT_KERNEL_ROUTES``), else ``model.distill`` on the written-out block -- always for a model whose class has a
        ``distill`` of its own or that is not a ``BaseModel``.  The same bits either way."""
        if (isinstance(model, BaseModel) and type(model).distill is BaseModel.distill
                and part in cls.SLOT_KERNEL_ROUTES.get(model.name, ())):
            return model.score_candidates(rows, cand, part)
        return model.distill(cls._block(rows, cand, part))

    def distill(self, teacher, student, sample):
        """KL(teacher || student) summed over the three candidate lists; differentiable w.r.t. the student only."""
        dev = student.entity_embedding.device
        sample = sample.to(dev)
        loss = 0
        kl = KlDivergence()
        for part, (rows_t, cand_t, rows_s, cand_s) in self.distillation_candidates(sample, teacher=teacher).items():
            with torch.no_grad():
                teacher_score = self._scores(teacher, rows_t, cand_t, part)
            loss = loss + kl(teacher_score=teacher_score, student_score=self._scores(student, rows_s, cand_s, part))
        return loss
