"""Device time of the exact squared-L2 k nearest rows and of the TransE teacher's samplers at the FB15k-237 TransE-1000 shape
(HIP events, warm-up first, median of repetitions, one MI355X):
  - one mkb_topk_nearest launch, B = 1024 queries against the 14,541 entity rows, k = 10 / 100, against mkb_topk_masked with a
    TransE-1000 teacher on the same chunk (the same register tile with the L1 term);
  - TopKSamplingTransE.get at B = 1024, split into the entity side (two launches) and the relation side (one launch over the
    237 relations), against TopKSampling.get on the same teacher;
  - building FastTopKSampling(transe_sampler=TopKSamplingTransE) over the FB15k-237 training split.

    python tools/topk_nearest_speed.py [--reps 20]

Prints one JSON line.  The tables are random (eval_tables, as in the top-k tests): the cost does not depend on the values."""
import argparse
import json
import pathlib
import statistics
import sys

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def timed(fn, reps):
    """Median over `reps` of the event time of one call, after two warm-up calls."""
    fn()
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    from util_gpu import make_model
    from util_gpu_tables import eval_tables
    from mkb_amd import datasets, distillation
    from mkb_amd.utils import candidate_bits
    from mkb_amd.utils.predict_top_k import _launch, topk_nearest

    ds = datasets.Fb15k237(batch_size=1024, shuffle=True, seed=42)
    ent, rel, _ = eval_tables("TransE", seed=77)
    teacher = make_model("TransE", ent, rel, 1000, 9.0).eval()
    train = np.asarray(ds.train, dtype=np.int64)
    sample = torch.as_tensor(train[np.random.RandomState(0).choice(len(train), 1024, replace=False)]).cuda()
    out = {"shape": "FB15k-237 TransE-1000, B = 1024, 14,541 entity rows / 237 relation rows"}
    with torch.no_grad():
        q = teacher._top_k(sample)[2].reshape(1024, -1).contiguous()
        X = teacher.entity_embedding.detach()
        cand = torch.arange(14541, device="cuda")
        bits = candidate_bits(torch.ones(14541, dtype=torch.bool), 14541, "cuda")
        none = torch.empty(0, dtype=torch.int64, device="cuda")
        for k in (10, 100):
            ids = torch.empty((1024, k), dtype=torch.int64, device="cuda")
            d = torch.empty((1024, k), dtype=torch.float32, device="cuda")
            out[f"mkb_topk_nearest_k{k}_ms"] = timed(lambda: topk_nearest(q, X, cand, k, ids=ids, dists=d), args.reps)
            out[f"mkb_topk_masked_transe_k{k}_ms"] = timed(lambda: _launch(teacher, sample, "tail-batch", k, none, 0, bits, 1024, ids, d),
                                                           args.reps)
        kw = dict(teacher_entities=ds.entities, teacher_relations=ds.relations, student_entities=ds.entities,
                  student_relations=ds.relations, batch_size_entity=10, batch_size_relation=5, n_random_entities=10,
                  n_random_relations=5, seed=1)
        l2 = distillation.TopKSamplingTransE(teacher=teacher, device="cuda", **kw)
        l1 = distillation.TopKSampling(device="cuda", **kw)
        out["transe_get_ms"] = timed(lambda: l2.get(sample=sample, teacher=teacher), args.reps)
        out["transe_get_entity_side_ms"] = timed(lambda: [l2.side(p, sample, teacher) for p in ("head", "tail")], args.reps)
        out["transe_get_relation_side_ms"] = timed(lambda: l2.side("relation", sample, teacher), args.reps)
        out["topk_sampling_get_ms"] = timed(lambda: l1.get(sample=sample, teacher=teacher), args.reps)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fast = distillation.FastTopKSampling(dataset_teacher=ds, teacher=teacher, transe_sampler=distillation.TopKSamplingTransE,
                                         device="cuda", **kw)
    b.record()
    b.synchronize()
    out["fast_build_s"] = a.elapsed_time(b) / 1000
    out["fast_keys"] = {p: int(fast._keys[p][0].numel()) for p in ("head", "relation", "tail")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
