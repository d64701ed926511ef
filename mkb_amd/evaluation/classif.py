"""Triple classification -- ``find_threshold`` and ``accuracy`` (reference mkb/evaluation/classif.py:9-155) with the same
signatures and the same numbers, plus per-relation thresholds (the protocol of Socher et al. 2013, from which the
``classification_valid`` / ``classification_test`` files come) and a per-relation report.

``find_threshold`` returns ``thresholds[argmax(tpr - fpr)]`` of ``sklearn.metrics.roc_curve(y, score)``.  With as many positives
as negatives, several thresholds usually share the exact maximum, and which of them sklearn returns is decided by float64
rounding and by the collinear points it dropped.  So the rule is restated exactly (``mkb_threshold_search`` in
include/mkb_hip.h spells it out) rather than simplified; sklearn itself is not needed.

On a ROCm device the scores of ``utils.make_prediction`` stay there: ``mkb_threshold_search`` counts all pairs and selects per
group, ``mkb_threshold_accuracy`` counts per group, and only thresholds and counts come back.  A model that is not on a device
(or ``device="cpu"``), plain arrays, and more items than the all-pairs search takes go the host route: the same rule on numpy
with a sort and cumulative sums.
"""
import numpy as np
import torch

from .. import _hip
from ..models.base import BaseModel
from ..utils import make_prediction

__all__ = ["find_threshold", "accuracy", "find_thresholds_per_relation", "classification_report", "threshold_search",
           "threshold_accuracy"]

SEARCH_CAP = _hip.THRESHOLD_SEARCH_MAX_N  # items above which threshold_search sorts on the host: the device search is quadratic
# and measured slower than the sort from there on (profiles/r13_classif_speed.txt)


# ------------------------------------------------------------------ host route (numpy)
def _roc_choice(score, positive):
    """``(threshold, tp, fp)`` of one group of finite float32 scores: roc_curve's points (descending distinct scores, cumulative
    positives / negatives, the points where neither second difference moves dropped except the two ends, and ``+inf`` with J = 0
    first), J in float64 as ``tps / tps[-1] - fps / fps[-1]``, first maximum."""
    P = int(positive.sum())
    N = len(score) - P
    if P == 0 or N == 0:
        return np.float32(np.inf), 0, 0
    order = np.argsort(score, kind="stable")[::-1]
    s, y = score[order], positive[order]
    last = np.r_[np.flatnonzero(s[1:] != s[:-1]), len(s) - 1]  # the last item of every run of one score (-0.0 == +0.0)
    tps = np.cumsum(y)[last].astype(np.float64)
    fps = 1.0 + last - tps
    if len(last) > 2:
        kept = np.flatnonzero(np.r_[True, (np.diff(fps, 2) != 0) | (np.diff(tps, 2) != 0), True])
        last, tps, fps = last[kept], tps[kept], fps[kept]
    J = np.r_[0.0, tps / tps[-1] - fps / fps[-1]]
    k = int(np.argmax(J))
    return (np.float32(np.inf), 0, 0) if k == 0 else (s[last[k - 1]], int(tps[k - 1]), int(fps[k - 1]))


def _groups_host(group, n, n_groups):
    """Per group the indices of its items, in item order; ids outside ``[0, n_groups)`` belong to nobody."""
    if group is None:
        return [np.arange(n)] + [np.arange(0)] * (n_groups - 1)
    order = np.argsort(group, kind="stable")
    ids = group[order]
    lo, hi = np.searchsorted(ids, np.arange(n_groups), "left"), np.searchsorted(ids, np.arange(n_groups), "right")
    return [order[a:b] for a, b in zip(lo, hi)]


def _search_host(score, label, group, n_groups):
    threshold, stats = np.full(n_groups, np.inf, dtype=np.float32), np.zeros((n_groups, 6), dtype=np.int64)
    for g, idx in enumerate(_groups_host(group, len(score), n_groups)):
        s, positive = score[idx], label[idx] > 0
        finite = np.isfinite(s)
        thr, tp, fp = _roc_choice(s[finite], positive[finite])
        P = int(positive[finite].sum())
        threshold[g], stats[g] = thr, (P, int(finite.sum()) - P, tp, fp, len(idx) - int(finite.sum()), len(idx))
    return threshold, stats


def _accuracy_host(score, label, group, threshold):
    counts = np.zeros((len(threshold), 2), dtype=np.int64)
    for g, idx in enumerate(_groups_host(group, len(score), len(threshold))):
        s, positive = score[idx].astype(np.float64), label[idx] > 0
        with np.errstate(invalid="ignore"):
            counts[g] = (int((((s >= threshold[g]) & positive) | ((s < threshold[g]) & ~positive)).sum()), len(idx))
    return counts


def _ceil_float32(threshold):
    """The smallest float32 >= each float64 threshold: a float32 score is >= (or <) the one exactly when it is >= (or <) the
    other, so the device compares float32 with float32 and still decides by the threshold's exact value."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = threshold.astype(np.float32)
        low = t.astype(np.float64) < threshold
    t[low] = np.nextafter(t[low], np.float32(np.inf))
    return t


# ------------------------------------------------------------------ arrays or tensors
def _on_device(scores):
    return isinstance(scores, torch.Tensor) and scores.is_cuda


def _prepare(scores, y, relation, n_relation):
    """-> (scores float32 [n], labels int64 [n], group int32 [n] or None, n_groups), all on the device of ``scores`` when that is
    a ROCm tensor, as numpy arrays otherwise."""
    if relation is not None and n_relation is None:
        raise ValueError("n_relation is needed with relation")
    n_groups = 1 if relation is None else int(n_relation)
    if _on_device(scores):
        dev = scores.device
        s = _hip.contiguous(scores.detach().reshape(-1), torch.float32)
        lab = torch.as_tensor(y, device=dev) if isinstance(y, torch.Tensor) else torch.as_tensor(np.asarray(y).reshape(-1), device=dev)
        lab = _hip.contiguous((lab > 0) if lab.is_floating_point() else lab, torch.int64).reshape(-1)
        grp = None
        if relation is not None:
            grp = relation.to(dev) if isinstance(relation, torch.Tensor) else torch.as_tensor(np.asarray(relation).reshape(-1), device=dev)
            grp = _hip.contiguous(grp.reshape(-1), torch.int32)
    else:
        as_np = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)  # noqa: E731
        s = np.ascontiguousarray(as_np(scores).reshape(-1), dtype=np.float32)
        lab = as_np(y).reshape(-1)
        lab = (lab > 0).astype(np.int64) if lab.dtype.kind == "f" else lab.astype(np.int64)
        grp = None if relation is None else as_np(relation).reshape(-1).astype(np.int64)
    if len(lab) != len(s) or (grp is not None and len(grp) != len(s)):
        raise ValueError(f"{len(s)} scores, {len(lab)} labels" + ("" if grp is None else f", {len(grp)} relation ids"))
    return s, lab, grp, n_groups


def threshold_search(scores, y, relation=None, n_relation=None, _cap=None):
    """The threshold of ``find_threshold`` for given scores (a tensor or an array, ``[n]``) and labels (``> 0``: positive):
    ``(float32 [G], int64 [G, 6])`` -- per group the threshold and P, N, the true and false positives at the threshold, the items
    with a score that is not finite, all items.  One group without ``relation``; with ``relation`` (``[n]`` ids) and
    ``n_relation``, one per relation id.  A group without positives or without negatives gets ``+inf``.  A score that is not
    finite raises ``ValueError``, as ``roc_curve`` does.  ``(tp + N - fp) / items`` is the accuracy at the threshold on the same
    set.  Scores on a ROCm device are searched there (up to ``SEARCH_CAP`` items)."""
    s, lab, grp, n_groups = _prepare(scores, y, relation, n_relation)
    return _searches(s, lab, [(grp, n_groups)], SEARCH_CAP if _cap is None else _cap)[0]


def _searches(s, lab, groupings, cap):
    """One search per ``(group ids or None, n_groups)`` over the same prepared scores and labels -> ``[(thresholds, stats)]``.
    On the device the searches are launched one after the other and all results come back in one copy."""
    n = len(s)
    if _on_device(s) and n <= cap:
        dev, lib = s.device, _hip.lib()
        total = sum(g for _, g in groupings)
        out = torch.empty(7 * total, dtype=torch.int64, device=dev)  # per search: stats [G, 6] int64, then thresholds [G] float32
        lo = 0
        with _hip.on_device(dev):
            for grp, n_groups in groupings:
                need = lib.mkb_threshold_search_workspace_bytes(n, n_groups)
                ws = _hip.aligned_bytes(max(need, 0), dev)
                _hip.check(lib.mkb_threshold_search(_hip.ptr(s), _hip.ptr(lab), _hip.ptr(grp), n, n_groups,
                                                    _hip.ptr(out[lo + 6 * n_groups:]), _hip.ptr(out[lo:]), _hip.ptr(ws), need,
                                                    _hip.stream_ptr()), "mkb_threshold_search")
                lo += 7 * n_groups
        host, found, lo = out.cpu().numpy(), [], 0
        for _, n_groups in groupings:
            stats = host[lo: lo + 6 * n_groups].reshape(n_groups, 6)
            found.append((host[lo + 6 * n_groups: lo + 7 * n_groups].view(np.float32)[:n_groups].copy(), stats))
            lo += 7 * n_groups
    else:
        if _on_device(s):  # above the cap: one copy of the scores, then the sort
            s, lab = s.cpu().numpy(), lab.cpu().numpy()
        found = [_search_host(s, lab, grp.cpu().numpy() if isinstance(grp, torch.Tensor) else grp, g) for grp, g in groupings]
    for _, stats in found:
        bad = int(stats[:, 4].sum())
        if bad:
            raise ValueError(f"{bad} of {n} scores are NaN or infinite: no threshold separates them")
    return found


def _threshold_array(threshold):
    """A number, a sequence, an array or a tensor of thresholds as float64 ``[k]``."""
    return np.asarray(threshold.detach().cpu().numpy() if isinstance(threshold, torch.Tensor) else threshold, dtype=np.float64).reshape(-1)


def threshold_accuracy(scores, y, threshold, relation=None, n_relation=None):
    """``int64 [G, 2]``: per group the items that ``threshold[g]`` classifies correctly -- score >= threshold and label > 0, or
    score < threshold and label <= 0 (a NaN score is neither) -- and all its items.  ``threshold``: a number (one group, or
    every relation's with ``relation``) or ``[n_relation]`` numbers.  Groups as in ``threshold_search``.

    The comparison is exact: a threshold given as a Python float is not rounded to float32 first.  The reference's doctest passes
    the literal ``1.9384804``, which lies just above the float32 score it was printed from, and reports 669 of 1,304 correct;
    with the ``numpy.float32`` that ``find_threshold`` returned, the item at the threshold counts too: 670."""
    s, lab, grp, n_groups = _prepare(scores, y, relation, n_relation)
    thr = _threshold_array(threshold)
    if thr.size == 1:
        thr = np.repeat(thr, n_groups)
    if thr.size != n_groups:
        raise ValueError(f"{thr.size} thresholds for {n_groups} groups")
    if not _on_device(s):
        return _accuracy_host(s, lab, grp, thr)
    dev = s.device
    t = torch.as_tensor(_ceil_float32(thr), device=dev)
    counts = torch.empty((n_groups, 2), dtype=torch.int64, device=dev)
    with _hip.on_device(dev):
        _hip.check(_hip.lib().mkb_threshold_accuracy(_hip.ptr(s), _hip.ptr(lab), _hip.ptr(grp), len(s), _hip.ptr(t), n_groups,
                                                     _hip.ptr(counts), _hip.stream_ptr()), "mkb_threshold_accuracy")
    return counts.cpu().numpy()


# ------------------------------------------------------------------ models
def _device_ok(model, device):
    """The rule of ``Evaluation._device_ok``: the parameters are on a ROCm device and the caller did not ask for the CPU."""
    return isinstance(model, BaseModel) and model.entity_embedding.is_cuda and str(device) != "cpu"


def _scores(model, X, batch_size, num_workers, device):
    """``make_prediction`` -- a device tensor on the device route, a float32 array otherwise -- and the ``[n, 3]`` triples."""
    triples = np.asarray(X, dtype=np.int64).reshape(-1, 3)
    if _device_ok(model, device):
        model.sync_parameters()
        return make_prediction(model=model, dataset=triples, batch_size=batch_size, num_workers=num_workers,
                               device=model.entity_embedding.device), triples
    scores = make_prediction(model=model, dataset=triples, batch_size=batch_size, num_workers=num_workers, device=device)
    return scores.detach().cpu().numpy().astype(np.float32, copy=False), triples


def _n_relation(model, triples):
    n = getattr(model, "n_relation", None)
    return int(n) if n is not None else (int(triples[:, 1].max()) + 1 if len(triples) else 1)


def find_threshold(model, X, y, batch_size, num_workers=1, device="cuda"):
    """The threshold (a ``numpy.float32``, one of the scores or ``+inf``) at or above which a triple is classified as true:
    ``thresholds[argmax(tpr - fpr)]`` of ``sklearn.metrics.roc_curve(y, model's scores of X)`` (classif.py:89-124)."""
    scores, _ = _scores(model, X, batch_size, num_workers, device)
    return threshold_search(scores, y)[0][0]


def _one_threshold(threshold):
    """One threshold for every triple (a number, or a single number in an array or a list); otherwise one per relation id."""
    return _threshold_array(threshold).size == 1


def _some_triples(triples):
    if len(triples) == 0:
        raise ValueError("X is empty: there is no accuracy of no triples")


def accuracy(model, X, y, threshold, batch_size, num_workers=1, device="cuda"):
    """The share of ``X`` that ``threshold`` classifies like ``y`` (classif.py:9-86, 127-155).  ``threshold`` may also hold one
    threshold per relation id (``find_thresholds_per_relation``): every triple is then judged by its relation's.  An empty ``X``
    raises ``ValueError``."""
    scores, triples = _scores(model, X, batch_size, num_workers, device)
    _some_triples(triples)
    if _one_threshold(threshold):
        counts = threshold_accuracy(scores, y, threshold)
    else:
        counts = threshold_accuracy(scores, y, threshold, relation=triples[:, 1], n_relation=_threshold_array(threshold).size)
    return int(counts[:, 0].sum()) / len(triples)


def find_thresholds_per_relation(model, X, y, batch_size, device="cuda"):
    """``(float32 [n_relation], global threshold)``: ``find_threshold`` on the triples of each relation.  A relation that does not
    occur in ``X``, or occurs with one class only, gets the global threshold (of all of ``X``)."""
    scores, triples = _scores(model, X, batch_size, 1, device)
    s, lab, grp, n_groups = _prepare(scores, y, triples[:, 1], _n_relation(model, triples))
    (overall, _), (per, stats) = _searches(s, lab, [(None, 1), (grp, n_groups)], SEARCH_CAP)  # both searches, one read-back
    overall, per = overall[0], per.copy()
    per[(stats[:, 0] == 0) | (stats[:, 1] == 0)] = overall
    return per, overall


def classification_report(model, X, y, threshold, batch_size, device="cuda"):
    """``{"accuracy", "n", "per_relation": {relation id: {"accuracy", "n"}}}`` of ``X`` at ``threshold`` (a number, or one per
    relation id, as in ``accuracy``); relations without a triple in ``X`` are left out.  An empty ``X`` raises ``ValueError``."""
    scores, triples = _scores(model, X, batch_size, 1, device)
    _some_triples(triples)
    n_rel = _n_relation(model, triples) if _one_threshold(threshold) else _threshold_array(threshold).size
    counts = threshold_accuracy(scores, y, threshold, relation=triples[:, 1], n_relation=n_rel)
    n = len(triples)
    return {"accuracy": int(counts[:, 0].sum()) / n, "n": n,
            "per_relation": {r: {"accuracy": int(c) / int(m), "n": int(m)} for r, (c, m) in enumerate(counts.tolist()) if m}}
