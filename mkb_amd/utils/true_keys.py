"""Sorted int64 keys of a set of true triples, one ordering per mode, on a device: the filter of the device ranking (``mkb_rank``)
and of the device top k (``mkb_topk``).  Tail-batch keys are ``(h * R + r) * N + t``, head-batch keys ``(t * R + r) * N + h``, so
that the filtered set of one query is a contiguous range of each array."""
import numpy as np
import torch

__all__ = ["true_keys"]

_CACHE = []  # [(true_triples, len, device, n_entity, n_relation, keys)], most recent first
_CACHE_SIZE = 4


def _build(true_triples, device, n_entity, n_relation):
    a = np.asarray(true_triples, dtype=np.int64).reshape(-1, 3)
    h, r, t = a[:, 0], a[:, 1], a[:, 2]
    tail = np.unique((h * n_relation + r) * n_entity + t)
    head = np.unique((t * n_relation + r) * n_entity + h)
    return {"head-batch": torch.as_tensor(head, device=device), "tail-batch": torch.as_tensor(tail, device=device)}


def true_keys(true_triples, device, n_entity, n_relation):
    """-> ``{"head-batch": keys, "tail-batch": keys}`` (ascending int64 tensors on ``device``).  Cached per triple collection
    (the same object with the same length), device and table size."""
    n = len(true_triples)
    for j, (obj, length, dev, ne, nr, keys) in enumerate(_CACHE):
        if obj is true_triples and length == n and dev == device and ne == n_entity and nr == n_relation:
            _CACHE.insert(0, _CACHE.pop(j))
            return keys
    keys = _build(true_triples, device, n_entity, n_relation)
    _CACHE.insert(0, (true_triples, n, device, n_entity, n_relation, keys))
    del _CACHE[_CACHE_SIZE:]
    return keys
