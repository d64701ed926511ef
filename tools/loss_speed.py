"""fused.PooledLossStep against compose.Pipeline's explicit sequence (model(sample), model(sample, negatives, mode), loss,
backward -- the pooled autograd forward) with the same loss object, per (model, loss) cell:

    python tools/loss_speed.py [--steps 200] [--reps 5] [--out FILE]

FB15k-237's tables, hidden 1000, B = 1024, K = 256; TransE, RotatE, ComplEx x MarginRanking, PairwiseLogistic, CrossEntropy.
Both routes run the same batches and negatives and are followed by the same dense mkb_amd.optim.Adam step + zero_grad, as in
Pipeline's loop.  Each repetition times `steps` steps between two device synchronisations; the routes alternate repetition by
repetition; reported: the best of `reps` and the spread (worst - best) of each route.  A cell belongs on the pooled step only
where its best is ahead of the explicit route's best by more than the explicit route's spread (compose/pipeline.py)."""
import argparse
import sys
import time

import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from mkb_amd import datasets, losses, models, optim, sampling  # noqa: E402
from mkb_amd.fused import PooledLossStep  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hidden", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--models", default="TransE,RotatE,ComplEx")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loss_speed.py measures on a ROCm device: none found")

    ds = datasets.Fb15k237(batch_size=args.batch, shuffle=True, seed=42, num_workers=0)
    batches = []
    for data in datasets.DeviceBatches(ds, "cuda", seed=42):
        if data["sample"].shape[0] == args.batch:
            batches.append((data["sample"], data["weight"], data["mode"]))
        if len(batches) == args.steps:
            break
    sampler = sampling.NegativeSampling(size=args.size, train_triples=ds.train, entities=ds.entities, relations=ds.relations, seed=42)
    negatives = [sampler.generate(sample=s, mode=mode) for s, _, mode in batches]
    sampler.check()
    loss_objects = [losses.MarginRanking(margin=6.0), losses.PairwiseLogistic(), losses.CrossEntropy()]
    lines = [f"# loss_speed: n_entity {len(ds.entities)}, n_relation {len(ds.relations)}, hidden {args.hidden}, B {args.batch}, K {args.size}, "
             f"{len(batches)} steps per repetition, best of {args.reps}; ms per step (forward, loss, backward, dense Adam step)",
             "# model loss | pooled best (spread) | explicit best (spread) | ahead by | route"]
    for name in args.models.split(","):
        for loss in loss_objects:
            torch.manual_seed(42)
            model = getattr(models, name)(hidden_dim=args.hidden, entities=ds.entities, relations=ds.relations, gamma=9.0).cuda()
            opt = optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-5)
            pooled = PooledLossStep(model, loss)

            def run_pooled():
                for (s, w, mode), neg in zip(batches, negatives):
                    pooled(s, w, neg, mode)
                    opt.step()
                    opt.zero_grad()

            def run_explicit():
                for (s, w, mode), neg in zip(batches, negatives):
                    error = loss(model(s), model(sample=s, negative_sample=neg, mode=mode), w)
                    error.backward()
                    opt.step()
                    opt.zero_grad()

            times = {"pooled": [], "explicit": []}
            for rep in range(args.reps + 1):  # repetition 0 warms both routes up (code objects, workspaces, the allocator)
                for key, fn in (("pooled", run_pooled), ("explicit", run_explicit)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    if rep:
                        times[key].append((time.perf_counter() - t0) / len(batches) * 1e3)
            pb, ps = min(times["pooled"]), max(times["pooled"]) - min(times["pooled"])
            eb, es = min(times["explicit"]), max(times["explicit"]) - min(times["explicit"])
            route = "pooled step" if eb - pb > es else "explicit sequence"
            lines.append(f"{name} {type(loss).__name__} | {pb:.3f} ({ps:.3f}) | {eb:.3f} ({es:.3f}) | {eb - pb:+.3f} | {route}")
            print(lines[-1], flush=True)
            del model, opt, pooled
            torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as handle:
            handle.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
