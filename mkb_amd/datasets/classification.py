"""``classification_set``: a labelled set for triple classification (evaluation.find_threshold / accuracy) built from a split,
the way the reference's ``classification_valid.csv`` / ``classification_test.csv`` are laid out: every true triple is followed
by one corrupted copy that is not a true triple (Socher et al. 2013).  The named datasets here ship no such files."""
import numpy as np

__all__ = ["classification_set"]


def classification_set(triples, true_triples, entities, seed=42):
    """``{"X": [(h, r, t), ...], "y": [1, -1, ...]}`` of length ``2 * len(triples)``: each triple of ``triples`` (label 1) is
    followed by itself with another tail (label -1), drawn uniformly from ``entities`` by ``numpy.random.RandomState(seed)`` and
    drawn again until the corrupted triple is not in ``true_triples`` (nor the positive itself).  The result feeds
    ``Dataset(classification_valid=..., classification_test=...)``."""
    pos = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    true = np.concatenate([np.asarray(true_triples, dtype=np.int64).reshape(-1, 3), pos])
    n_ent = len(entities)
    if n_ent <= 0 or (len(true) and (true[:, [0, 2]].min() < 0 or true[:, [0, 2]].max() >= n_ent or true[:, 1].min() < 0)):
        raise ValueError("entity ids must lie in [0, len(entities)) and relation ids must not be negative")
    n_rel = int(true[:, 1].max()) + 1 if len(true) else 1
    keys = np.unique((true[:, 0] * n_rel + true[:, 1]) * n_ent + true[:, 2])
    rng = np.random.RandomState(seed)
    tail = np.empty(len(pos), dtype=np.int64)
    todo = np.arange(len(pos))
    for _ in range(1000):
        if len(todo) == 0:
            break
        tail[todo] = rng.randint(n_ent, size=len(todo))
        drawn = (pos[todo, 0] * n_rel + pos[todo, 1]) * n_ent + tail[todo]
        todo = todo[np.isin(drawn, keys, assume_unique=False)]
    else:
        h, r, _ = pos[todo[0]].tolist()
        raise ValueError(f"no false tail found for ({h}, {r}, .): every entity seems to be a true tail")
    X = np.repeat(pos, 2, axis=0)
    X[1::2, 2] = tail
    return {"X": [tuple(row) for row in X.tolist()], "y": [1, -1] * len(pos)}
