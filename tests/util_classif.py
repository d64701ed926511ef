"""The threshold rule of triple classification restated on numpy from per-score counts (include/mkb_hip.h,
mkb_threshold_search), independent of both routes of mkb_amd.evaluation.classif: what sklearn.metrics.roc_curve +
argmax(tpr - fpr) return, without sklearn.  Shared by tests/test_host_classif.py and tests/test_gpu_classif.py."""
import numpy as np

MODELS = ("TransE3", "RotatE", "ComplEx", "DistMult", "pRotatE", "TransE_trained")  # the cases of tests/golden/classif.*


def roc_choice(score, label):
    """-> (threshold float32, tp, fp) of one group; ``score`` float32 and finite, ``label > 0`` positive."""
    score = np.asarray(score, dtype=np.float32)
    pos = np.asarray(label) > 0
    P, N = int(pos.sum()), int((~pos).sum())
    if P == 0 or N == 0:
        return np.float32(np.inf), 0, 0
    sp, sn = np.sort(score[pos]), np.sort(score[~pos])
    values = np.unique(score)[::-1]  # distinct, descending; -0.0 and +0.0 are one value
    tp_ge, fp_ge = P - np.searchsorted(sp, values, "left"), N - np.searchsorted(sn, values, "left")
    tp_gt, fp_gt = P - np.searchsorted(sp, values, "right"), N - np.searchsorted(sn, values, "right")
    tp_nx, fp_nx = np.r_[tp_ge[1:], P], np.r_[fp_ge[1:], N]  # counts at the next lower distinct value
    keep = (fp_nx - 2 * fp_ge + fp_gt != 0) | (tp_nx - 2 * tp_ge + tp_gt != 0)
    keep[0] = keep[-1] = True
    best, choice = 0.0, (np.float32(np.inf), 0, 0)
    for k in np.flatnonzero(keep):  # descending thresholds: a later point must be strictly better
        J = np.float64(tp_ge[k]) / np.float64(P) - np.float64(fp_ge[k]) / np.float64(N)
        if J > best:
            best, choice = J, (values[k], int(tp_ge[k]), int(fp_ge[k]))
    return choice


def search(score, label, group=None, n_groups=1):
    """-> (thresholds float32 [G], stats int64 [G, 6]) as mkb_threshold_search defines them."""
    score, label = np.asarray(score, dtype=np.float32), np.asarray(label)
    group = np.zeros(len(score), dtype=np.int64) if group is None else np.asarray(group)
    thr, stats = np.full(n_groups, np.inf, dtype=np.float32), np.zeros((n_groups, 6), dtype=np.int64)
    for g in range(n_groups):
        mine = group == g
        ok = mine & np.isfinite(score)
        thr[g], tp, fp = roc_choice(score[ok], label[ok])
        P = int((label[ok] > 0).sum())
        stats[g] = (P, int(ok.sum()) - P, tp, fp, int(mine.sum() - ok.sum()), int(mine.sum()))
    return thr, stats


def accuracy_counts(score, label, threshold, group=None):
    """-> int64 [G, 2]: (correct, items) per group, item by item as the reference's loop (classif.py:143-155)."""
    threshold = np.asarray(threshold, dtype=np.float64).reshape(-1)  # compared by exact value, like Python's float(score) >= t
    out = np.zeros((len(threshold), 2), dtype=np.int64)
    for i, (s, y) in enumerate(zip(np.asarray(score, dtype=np.float32).tolist(), np.asarray(label).tolist())):
        g = 0 if group is None else int(group[i])
        if 0 <= g < len(threshold):
            t = float(threshold[g])
            out[g] += (int((s >= t and y > 0) or (s < t and y <= 0)), 1)
    return out


def same_floats(a, b):
    """``==`` elementwise (-0.0 == +0.0, inf == inf), shapes included."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all(a == b))


_DATASET = []


def dataset():
    """Umls of the package (its ids are its own: the fixtures carry the reference's ids in their triples)."""
    from mkb_amd import datasets

    if not _DATASET:
        _DATASET.append(datasets.Umls(batch_size=8, shuffle=False, seed=42, num_workers=0))
    return _DATASET[0]
