"""TransE (reference mkb/models/transe.py:11-84): score = gamma - || h + r - t ||_1."""
import torch

from .. import _hip
from .base import BaseModel

__all__ = ["TransE"]


class TransE(BaseModel):
    def __init__(self, hidden_dim, entities, relations, gamma):
        super().__init__(hidden_dim=hidden_dim, relation_dim=hidden_dim, entity_dim=hidden_dim, entities=entities,
                         relations=relations, gamma=gamma)

    def _top_k(self, sample):
        """The translated queries of ``distillation.TopKSamplingTransE`` (transe.py:78-84), each ``[B, 1, D]``: ``t - r`` (the
        head a triple's (r, t) points at), ``t - h`` (the relation of its (h, t)) and ``h + r`` (the tail of its (h, r)).  Device
        tables only; a row-lazy optimizer's rows are brought current first."""
        _hip.require_device(self.entity_embedding)
        self.sync_parameters()
        sample = torch.as_tensor(sample).to(device=self.entity_embedding.device, dtype=torch.int64).reshape(-1, 3)
        head = self.entity_embedding[sample[:, 0]].unsqueeze(1)
        relation = self.relation_embedding[sample[:, 1]].unsqueeze(1)
        tail = self.entity_embedding[sample[:, 2]].unsqueeze(1)
        return -relation + tail, -head + tail, head + relation
