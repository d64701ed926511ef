"""Device time of the teacher top-k samplers at the FB15k-237 RotatE-1000 shape (HIP events, one MI355X):
  - TopKSampling.get at B = 1024, split into the entity side (two mkb_topk_masked launches) and the relation side (the general
    forward of [B, 237, 3] plus mkb_topk_block);
  - building FastTopKSampling over the FB15k-237 training split;
  - mkb_topk_masked with a 50 % mask against mkb_topk on the same 1024-query chunk;
  - TopKSampling.side("relation") at B = 1024 for the five teachers at hidden 1000, through the general forward and through
    mkb_rel_scores: five measurements of --reps calls each, every one listed.

    python tools/topk_sampling_speed.py [--reps 20]

Prints one JSON line.  The tables are random (eval_tables, as in the top-k tests): the selection's cost does not depend on the
values."""
import argparse
import json
import pathlib
import sys
import time

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    from util_gpu import make_model
    from util_gpu_tables import eval_tables
    from mkb_amd import datasets, distillation
    from mkb_amd.utils import candidate_bits, topk_block
    from mkb_amd.utils.predict_top_k import _launch

    ds = datasets.Fb15k237(batch_size=1024, shuffle=True, seed=42)
    ent, rel, modulus = eval_tables("RotatE", seed=77)
    teacher = make_model("RotatE", ent, rel, 1000, 9.0, modulus).eval()
    kw = dict(teacher_entities=ds.entities, teacher_relations=ds.relations, student_entities=ds.entities,
              student_relations=ds.relations, batch_size_entity=10, batch_size_relation=5, n_random_entities=10,
              n_random_relations=5, seed=1)
    sampler = distillation.TopKSampling(**kw)
    train = np.asarray(ds.train, dtype=np.int64)
    sample = torch.as_tensor(train[np.random.RandomState(0).choice(len(train), 1024, replace=False)]).cuda()
    tb = sampler.tables("cuda")
    none = torch.empty(0, dtype=torch.int64, device="cuda")
    ids = torch.empty((1024, 10), dtype=torch.int64, device="cuda")
    sc = torch.empty((1024, 10), dtype=torch.float32, device="cuda")
    out = {"shape": "FB15k-237 RotatE-1000, B = 1024, top 10 entities / 5 relations (+ 10 / 5 random)"}
    with torch.no_grad():
        out["get_ms"] = timed(lambda: sampler.get(sample=sample, teacher=teacher), args.reps)

        def ent_side():
            for mode in ("head-batch", "tail-batch"):
                _launch(teacher, sample, mode, 10, none, 0, tb["ent_bits"], 1024, ids, sc)
        out["get_entity_side_ms"] = timed(ent_side, args.reps)
        rel_t = tb["rel_t"]
        rel_ids = torch.empty((1024, 5), dtype=torch.int64, device="cuda")

        def rel_side():
            blk = torch.stack([sample[:, 0:1].expand(-1, 237), rel_t.view(1, -1).expand(1024, -1), sample[:, 2:3].expand(-1, 237)], -1)
            topk_block(teacher(blk.contiguous()).reshape(1024, 237), 5, ids=rel_ids)
        out["get_relation_side_ms"] = timed(rel_side, args.reps)
        half = candidate_bits(torch.as_tensor(np.random.RandomState(1).rand(14541) < 0.5), 14541, "cuda")
        for k in (10, 100):
            ids_k = torch.empty((1024, k), dtype=torch.int64, device="cuda")
            sc_k = torch.empty((1024, k), dtype=torch.float32, device="cuda")
            out[f"mkb_topk_k{k}_ms"] = timed(lambda: _launch(teacher, sample, "tail-batch", k, none, 0, None, 1024, ids_k, sc_k), args.reps)
            out[f"mkb_topk_masked50_k{k}_ms"] = timed(lambda: _launch(teacher, sample, "tail-batch", k, none, 0, half, 1024, ids_k, sc_k),
                                                      args.reps)
        for name in ("TransE", "RotatE", "ComplEx", "DistMult", "pRotatE"):
            e_tab, r_tab, mod = eval_tables(name, seed=77)
            t = make_model(name, e_tab, r_tab, 1000, 9.0, mod).eval()
            sampler.RELATION_KERNEL_MODELS = frozenset([name])
            same = all(torch.equal(x, y) for x, y in zip(sampler.side("relation", sample, t), sampler._relation_side_general(sample, t)))
            for route, fn in (("general", lambda: sampler._relation_side_general(sample, t)), ("kernel", lambda: sampler.side("relation", sample, t))):
                out[f"relation_side_{name}_{route}_ms"] = [round(timed(fn, args.reps), 4) for _ in range(5)]
            out[f"relation_side_{name}_same_ids"] = same
            del t
        del sampler.RELATION_KERNEL_MODELS
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fast = distillation.FastTopKSampling(dataset_teacher=ds, teacher=teacher, **kw)
    b.record()
    b.synchronize()
    out["fast_build_s"] = a.elapsed_time(b) / 1000
    out["fast_build_wall_s"] = time.perf_counter() - t0
    out["fast_keys"] = {p: int(fast._keys[p][0].numel()) for p in ("head", "relation", "tail")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
