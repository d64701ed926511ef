"""python tools/eval_speed.py [Model ...]: seconds of one filtered evaluation (evaluation.Evaluation.eval, both corruption sides) of
FB15k-237's test split -- 40,932 queries x 14,541 entities, hidden 1000, random tables -- per model, and next to it the seconds of
the report by relation category (evaluation.Evaluation.detail_metrics) of the same model and split."""
import sys, time, torch
sys.path.insert(0, __file__.rsplit("/", 2)[0])
from mkb_amd import datasets, evaluation, models
ds = datasets.Fb15k237(batch_size=1024, shuffle=False, seed=42, num_workers=0)
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
