"""``KvsAll`` -- the multi-label binary cross entropy over ALL entities (KvsAll, "1-N" training: the recipe of ConvE, TuckER and
LibKGE's ComplEx / DistMult configurations).

``loss(scores, sample, mode, weight=None, n_relation=None)`` with ``scores`` [B, N] (one column per entity, higher = more
plausible: what ``model.score_all(sample, mode)`` returns), ``sample`` [B, 3] int64 (the triples whose open slot was scored),
``mode`` ``'tail-batch'`` or ``'head-batch'`` and an optional per-row ``weight`` [B] (absent: all ones):

    y_ij  = (1 - eps) [j in A_i] + eps / N                     eps = label_smoothing
    row_i = c sum_j (softplus(scores_ij) - y_ij scores_ij)     c = 1 / N (reduction="mean") or 1 ("sum")
    loss  = sum_i w_i row_i / sum_i w_i

differentiable in ``scores``.  ``A_i`` is the set of ALL known answers of row i's query -- every ``t`` with ``(h_i, r_i, t)`` in
``true_triples`` (tail-batch; every ``h`` with ``(h, r_i, t_i)`` for head-batch) -- read on the device from the sorted key arrays
of the filtered ranking (``utils.true_keys``); no [B, N] label matrix is built.  A query without any known answer is legal.
``n_relation``: the relation count of the tables the scores came from (absent: 1 + the largest relation id of ``true_triples``).

With ``reduction="mean"``, ``label_smoothing=0`` and no weights the value is the reference's
``losses.BCEWithLogitsLoss()(scores, multi_hot)`` = ``torch.nn.BCEWithLogitsLoss()`` on the dense multi-hot label matrix (the
mean over all B N elements).

The class is also the marker ``compose.Pipeline.learn`` reads: with this loss every batch goes through ``fused.KvsAllStep`` (no
negatives are drawn; with ``true_triples=None`` the labels are the training triples of the dataset being iterated); with TransE,
RotatE or pRotatE through ``fused.DistanceAllStep``.
"""
import math

import torch

from .. import _hip
from . import _rows
from ..utils.true_keys import true_keys

__all__ = ["KvsAll"]

REDUCTIONS = ("mean", "sum")


def checked_settings(label_smoothing, reduction):
    """-> (float label_smoothing, reduction), or ValueError."""
    eps = float(label_smoothing)
    if not math.isfinite(eps) or not 0.0 <= eps < 1.0:
        raise ValueError(f"label_smoothing must be in [0, 1), not {eps}")
    if reduction not in REDUCTIONS:
        raise ValueError(f"reduction must be one of {REDUCTIONS}, not {reduction!r}")
    return eps, reduction


def launch(S, n_cols, sample, mode_id, n_relation, keys, weight, weight_sum, label_smoothing, reduction):
    """One ``mkb_all_bce`` call on a contiguous float32 device block ``S`` [B, ld] of which the first ``n_cols`` columns count;
    ``keys``: the sorted int64 device keys of ``mode_id``'s side.  ``S`` is OVERWRITTEN with the gradient seeds.
    -> (loss [1], pos [B])."""
    B, ld = S.shape
    loss, pos, scratch = _rows.block_outputs(S)
    with _hip.on_device(S.device):
        _hip.check(_hip.lib().mkb_all_bce(_hip.ptr(S), B, n_cols, ld, _hip.ptr(sample), mode_id, n_relation, _hip.ptr(keys), keys.numel(),
                                          _hip.ptr(weight), _hip.ptr(weight_sum), label_smoothing, int(reduction == "sum"),
                                          _hip.ptr(loss), _hip.ptr(pos), _hip.ptr(scratch), _hip.stream_ptr()), "mkb_all_bce")
    return loss, pos


def relation_count(loss):
    """The ``n_relation`` a loss that holds ``true_triples`` assumes when none is given: 1 + their largest relation id (kept until
    their number changes)."""
    if loss._n_relation is None or loss._n_relation[0] != len(loss.true_triples):
        loss._n_relation = (len(loss.true_triples), 1 + max((int(t[1]) for t in loss.true_triples), default=0))
    return loss._n_relation[1]


class KvsAll:
    kind = None  # (not one of mkb_ns_loss's kinds: fused.PooledLossStep refuses it)

    def __init__(self, true_triples=None, label_smoothing=0.0, reduction="mean"):
        self.label_smoothing, self.reduction = checked_settings(label_smoothing, reduction)
        self.true_triples = true_triples
        self._n_relation = None

    def __call__(self, scores, sample, mode, weight=None, n_relation=None):
        _hip.require_device(scores, sample, weight)
        mode_id = _hip.side_id(mode, "KvsAll labels")
        if self.true_triples is None:
            raise ValueError("KvsAll needs true_triples to label a score block (only compose.Pipeline fills them in from its dataset)")
        _rows.check_scores(scores)
        if sample.shape != (scores.size(0), 3) or sample.dtype != torch.int64:
            raise ValueError("sample must be an int64 tensor [B, 3]")
        _rows.check_weight(weight, scores.size(0))
        s, w = _rows.f32(scores), _rows.f32(weight)
        if s.shape[0] == 0:
            return _rows.empty_batch(w, s)
        n_relation = relation_count(self) if n_relation is None else int(n_relation)
        keys = true_keys(self.true_triples, s.device, s.size(1), n_relation)["head-batch" if mode_id == _hip.MODE_HEAD else "tail-batch"]
        sample = _hip.contiguous(sample, torch.int64)
        return _rows.SeedsInPlaceFn.apply(s, lambda S: launch(S, S.shape[1], sample, mode_id, n_relation, keys, w, None, self.label_smoothing,
                                                              self.reduction))

    def __repr__(self):
        return f"KvsAll(label_smoothing={self.label_smoothing}, reduction={self.reduction!r})"
