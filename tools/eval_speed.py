"""python tools/eval_speed.py [Model ...]: seconds of one filtered evaluation (evaluation.Evaluation.eval, both corruption sides) of
FB15k-237's test split -- 40,932 queries x 14,541 entities, hidden 1000, random tables -- per model, and next to it the seconds of
the report by relation category (evaluation.Evaluation.detail_metrics) of the same model and split.

python tools/eval_speed.py classif: triple classification on sets made by datasets.classification_set from FB15k-237's valid
(35,070 items) and test (40,932 items) splits, RotatE hidden 1000: find_threshold, accuracy and find_thresholds_per_relation on
the device route and on the host route (device="cpu" after the scores: sort, cumulative sums; and the reference's own per-item
Python loop for the accuracy), the device search apart from the scoring of the same call, and the search at 32,768 .. 262,144 items.

python tools/eval_speed.py relations [Model ...]: the relation side of the same split -- evaluation.Evaluation.eval_relations as a whole
call and relation_ranks alone, 20,466 triples x 237 relations, through the general forward of the [b, 237, 3] block with torch glue
and through mkb_rel_rank.

python tools/eval_speed.py classif cap: the sweep over sizes alone.  The device search refuses more than MKB_THRESHOLD_SEARCH_MAX_N
items, so the sizes above it are measured on a build with a higher value (the measurement that placed the cap):
    python -c "import os; from mkb_amd.csrc import build; build.build(extra_flags=['-DMKB_THRESHOLD_SEARCH_MAX_N=262144'], out=os.path.abspath('variants/libmkb_hip_cap.so'), objdir=os.path.abspath('variants/obj_cap'))"
    MKB_HIP_LIB=variants/libmkb_hip_cap.so python tools/eval_speed.py classif cap"""
import sys, time, torch
sys.path.insert(0, __file__.rsplit("/", 2)[0])
from mkb_amd import datasets, evaluation, models
ds = datasets.Fb15k237(batch_size=1024, shuffle=False, seed=42, num_workers=0)


class Best(float):  # the best of the runs, with all of them for the record
    runs = ()

def timed(call, runs=5):
    call()  # warm: code objects, allocator
    times, out = [], None
    for _ in range(runs):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    best = Best(min(times))
    best.runs = tuple(times)
    return best, out

def line(what, seconds, note=""):
    runs = "  (runs: " + " ".join(f"{1e3 * t:.3f}" for t in seconds.runs) + ")" if getattr(seconds, "runs", ()) else ""
    print(f"{what:58s} {1e3 * seconds:10.3f} ms{runs}  {note}", flush=True)


def relations_speed(names):
    """eval_relations as a whole call, and relation_ranks alone, on FB15k-237's test split at hidden 1000: through the torch glue
    around the general forward (Evaluation._relation_ranks_torch) and through mkb_rel_rank (Evaluation._relation_ranks_kernel)."""
    import mkb_amd.evaluation.evaluation as ev_mod

    ev = evaluation.Evaluation(true_triples=ds.true_triples, entities=ds.entities, relations=ds.relations, batch_size=1024, device="cuda",
                               num_workers=0)
    print(f"test: {len(ds.test)} triples x {len(ds.relations)} relations, hidden 1000; best of 5 runs after one warm run, every run listed",
          flush=True)
    default = ev_mod.RELATION_KERNEL_MODELS
    for name in names:
        torch.manual_seed(1)
        m = getattr(models, name)(hidden_dim=1000, entities=ds.entities, relations=ds.relations, gamma=9.0).cuda().eval()
        with torch.no_grad():
            t_old, r_old = timed(lambda: ev._relation_ranks_torch(m, ds.test))
            t_new, r_new = timed(lambda: ev._relation_ranks_kernel(m, ds.test))
        spread = max(t_old.runs) - min(t_old.runs)
        line(f"{name} relation_ranks, general forward + torch", t_old, f"spread {1e3 * spread:.3f} ms")
        line(f"{name} relation_ranks, mkb_rel_rank", t_new,
             f"same ranks: {bool(torch.equal(r_old, r_new))}; faster by more than the spread: {bool(t_old - t_new > spread)}")
        for route, members in (("general forward + torch", frozenset()), ("mkb_rel_rank", frozenset([name]))):
            ev_mod.RELATION_KERNEL_MODELS = members
            t, out = timed(lambda: ev.eval_relations(model=m, dataset=ds.test))
            line(f"{name} eval_relations, {route}", t, str(out))
        ev_mod.RELATION_KERNEL_MODELS = default


def classif_speed(sweep_only=False):
    import numpy as np
    from mkb_amd import _hip
    from mkb_amd.evaluation import classif

    R = len(ds.relations)
    if not sweep_only:
        classif_calls(timed, line, R)
    rs = np.random.RandomState(0)
    for n in (32768, 65536, 131072, 262144):
        if _hip.lib().mkb_threshold_search_workspace_bytes(n, 1) < 0:  # above the cap of the loaded library
            continue
        s = torch.as_tensor(rs.randn(n).astype(np.float32), device="cuda")
        lab = torch.as_tensor(rs.randint(0, 2, size=n) * 2 - 1, device="cuda")
        grp = torch.as_tensor(np.sort(rs.randint(R, size=n)).astype(np.int32), device="cuda")
        t_dev, (a, _) = timed(lambda: classif.threshold_search(s, lab, _cap=n))
        t_grp, _ = timed(lambda: classif.threshold_search(s, lab, relation=grp, n_relation=R, _cap=n))
        sh, lh = s.cpu().numpy(), lab.cpu().numpy()
        t_h, (b, _) = timed(lambda: classif.threshold_search(sh, lh))
        line(f"search at n = {n}: device, one group", t_dev, f"same as host: {a[0] == b[0]}")
        line(f"search at n = {n}: device, {R} groups", t_grp)
        line(f"search at n = {n}: host, one group", t_h)


def classif_calls(timed, line, R):
    import numpy as np
    from mkb_amd import utils
    from mkb_amd.evaluation import classif

    valid = datasets.classification_set(ds.valid, ds.true_triples, ds.entities, seed=42)
    test = datasets.classification_set(ds.test, ds.true_triples, ds.entities, seed=43)
    torch.manual_seed(1)
    m = models.RotatE(hidden_dim=1000, entities=ds.entities, relations=ds.relations, gamma=9.0).cuda().eval()
    call = dict(model=m, batch_size=4096)
    X, y = np.asarray(valid["X"], dtype=np.int64), np.asarray(valid["y"], dtype=np.int64)
    Xt, yt = np.asarray(test["X"], dtype=np.int64), np.asarray(test["y"], dtype=np.int64)
    print(f"valid: {len(y)} items, test: {len(yt)} items, {R} relations; best of 5 runs after one warm run, every run listed", flush=True)
    t_thr, thr = timed(lambda: evaluation.find_threshold(X=X, y=y, **call))
    line("find_threshold, device route (whole call)", t_thr, f"threshold {thr}")
    t_score, scores = timed(lambda: utils.make_prediction(model=m, dataset=X, batch_size=4096, device="cuda"))
    line("  of which scoring (make_prediction)", t_score)
    y_dev, rel_dev = torch.as_tensor(y, device="cuda"), torch.as_tensor(X[:, 1], device="cuda")
    t_search, (thr_dev, _) = timed(lambda: classif.threshold_search(scores, y_dev))
    line("  of which threshold search (kernels + read-back)", t_search)
    s_host = scores.cpu().numpy()
    t_host, (thr_host, _) = timed(lambda: classif.threshold_search(s_host, y))
    line("threshold search, host route (sort, cumulative sums)", t_host, f"same threshold: {thr_host[0] == thr_dev[0] == thr}")
    t_per, (per, _) = timed(lambda: evaluation.find_thresholds_per_relation(X=X, y=y, **call))
    line("find_thresholds_per_relation, device route (whole call)", t_per)
    t_per_search, _ = timed(lambda: classif.threshold_search(scores, y_dev, relation=rel_dev, n_relation=R))
    line("  of which the grouped search", t_per_search)
    t_per_host, (per_host, stats) = timed(lambda: classif.threshold_search(s_host, y, relation=X[:, 1], n_relation=R))
    both = (stats[:, 0] > 0) & (stats[:, 1] > 0)
    line("grouped search, host route", t_per_host, f"same thresholds: {bool(np.all(per[both] == per_host[both]))}")
    t_acc, acc = timed(lambda: evaluation.accuracy(X=Xt, y=yt, threshold=thr, **call))
    line("accuracy, device route (whole call)", t_acc, f"accuracy {acc:.6f}")
    st = utils.make_prediction(model=m, dataset=Xt, batch_size=4096, device="cuda")
    yt_dev = torch.as_tensor(yt, device="cuda")
    t_count, counts = timed(lambda: classif.threshold_accuracy(st, yt_dev, thr))
    line("  of which the count (kernel + read-back)", t_count)
    st_host = st.cpu().numpy()
    t_count_host, counts_host = timed(lambda: classif.threshold_accuracy(st_host, yt, thr))
    line("accuracy count, host route (numpy)", t_count_host, f"same count: {counts.tolist() == counts_host.tolist()}")

    def reference_loop():  # reference evaluation/classif.py:143-155
        correct = 0
        for i in range(len(st_host)):
            if st_host[i] >= thr and yt[i] > 0:
                correct += 1
            if st_host[i] < thr and yt[i] <= 0:
                correct += 1
        return correct

    t0 = time.perf_counter(); correct = reference_loop()
    line("accuracy count, the reference's per-item loop (one run)", time.perf_counter() - t0, f"same count: {correct == int(counts[0, 0])}")


if sys.argv[1:2] == ["relations"]:
    relations_speed(sys.argv[2:] or ["TransE", "RotatE", "ComplEx", "DistMult", "pRotatE"])
    sys.exit(0)
if sys.argv[1:2] == ["classif"]:
    classif_speed(sweep_only=sys.argv[2:3] == ["cap"])
    sys.exit(0)
ev = evaluation.Evaluation(true_triples=ds.true_triples, entities=ds.entities, relations=ds.relations, batch_size=1024, device="cuda", num_workers=0)
for name in (sys.argv[1:] or ["TransE", "RotatE", "ComplEx", "DistMult", "pRotatE"]):
    torch.manual_seed(1)
    m = getattr(models, name)(hidden_dim=1000, entities=ds.entities, relations=ds.relations, gamma=9.0).cuda().eval()
    for what, call in (("eval", ev.eval), ("detail_metrics", ev.detail_metrics)):
        call(model=m, dataset=ds.test[:2048])  # warm: code objects, the true keys and the fan-out counts of the filter set
        times, out = [], None
        for _ in range(3):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            out = call(model=m, dataset=ds.test)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        if what == "detail_metrics":
            out = {mode: {kind: v["MRR"] for kind, v in out[mode].items()} for mode in ("head-batch", "tail-batch")}
        runs = " ".join(f"{t:.3f}" for t in times)
        print(f"{name:9s} {what:14s} {times[0]:.3f} s  (three runs: {runs})  {out}", flush=True)
