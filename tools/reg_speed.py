"""What an N3 regulariser costs a training step, and what the device route saves over the torch expression:

    python tools/reg_speed.py [--steps 200] [--reps 5] [--cases a,b,c] [--weight 1e-3] [--out FILE]

FB15k-237's tables, hidden 1000, B = 1024, K = 256; TransE, RotatE, ComplEx; the optimizer is always
mkb_amd.optim.Adam(lazy_rows=True, defer_step=True, draw_ahead=sampler), the sampler rides its catch-up launch where it can.
  a  fused.FusedTrainStep without a regulariser (run this case from a checkout of the parent commit for the cost of the feature:
     it needs nothing this tool's commit adds);
  b  the same step with regularizers.N3 through ``regularizer=`` (one more library call, mkb_reg_rows);
  c  what a user could do before: the explicit sequence (model(sample), model(sample, negatives, mode), Adversarial) with the N3
     penalty written in torch on gathered rows.  Autograd adds a dense table into .grad, the optimizer leaves its row-lazy route
     at the first step and stays on the dense kernel.
Each repetition times `steps` steps between two device synchronisations; the cases alternate repetition by repetition, repetition 0
warms up (code objects, workspaces, the allocator).  Reported per case: the best of `reps` and the spread (worst - best), in ms per
step; then b - a and c / b where the cases were run together."""
import argparse
import sys
import time

import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from mkb_amd import datasets, losses, models, optim, sampling  # noqa: E402
from mkb_amd.fused import FusedTrainStep  # noqa: E402

PAIRED = {"ComplEx": (True, True), "RotatE": (True, False)}  # (entity, relation) rows read as [re | im] halves


def torch_n3(model, sample, weight, lam):
    """The penalty as user code writes it: sum_i (w_i / W) lam (f(E[h_i]) + f(E[t_i]) + f(R[r_i])), f = sum |x|^3 or sum |z|^3."""
    def f(rows, paired):
        if not paired:
            return (rows.abs() ** 3).sum(1)
        d = rows.shape[1] // 2
        return ((rows[:, :d] ** 2 + rows[:, d:] ** 2) ** 1.5).sum(1)

    pe, pr = PAIRED.get(model.name, (False, False))
    ent, rel = model.entity_embedding, model.relation_embedding
    per_row = f(ent[sample[:, 0]], pe) + f(ent[sample[:, 2]], pe) + f(rel[sample[:, 1]], pr)
    return lam * (weight / weight.sum() * per_row).sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hidden", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--weight", type=float, default=1e-3)
    ap.add_argument("--models", default="TransE,RotatE,ComplEx")
    ap.add_argument("--cases", default="a,b,c")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("reg_speed.py measures on a ROCm device: none found")
    cases = args.cases.split(",")

    ds = datasets.Fb15k237(batch_size=args.batch, shuffle=True, seed=42, num_workers=0)
    batches = []
    for data in datasets.DeviceBatches(ds, "cuda", seed=42):
        if data["sample"].shape[0] == args.batch:
            batches.append((data["sample"], data["weight"], data["mode"]))
        if len(batches) == args.steps:
            break
    lines = [f"# reg_speed: n_entity {len(ds.entities)}, n_relation {len(ds.relations)}, hidden {args.hidden}, B {args.batch}, K {args.size}, "
             f"{len(batches)} steps per repetition, best of {args.reps}; ms per step (sampler, forward, loss, backward, optimizer); "
             f"N3 weight {args.weight}",
             "# model | case best (spread) ... | b - a | c / b"]
    crit = losses.Adversarial(alpha=1.0)
    for name in args.models.split(","):
        runs = {}
        for case in cases:
            torch.manual_seed(42)
            model = getattr(models, name)(hidden_dim=args.hidden, entities=ds.entities, relations=ds.relations, gamma=9.0).cuda()
            sampler = sampling.NegativeSampling(size=args.size, train_triples=ds.train, entities=ds.entities, relations=ds.relations, seed=42)
            opt = optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-5, lazy_rows=True, draw_ahead=sampler,
                             defer_step=True)
            if case == "a":
                step = FusedTrainStep(model, 1.0)
            elif case == "b":
                from mkb_amd import regularizers

                step = FusedTrainStep(model, 1.0, regularizer=regularizers.N3(args.weight))

            def run(case=case, model=model, sampler=sampler, opt=opt, step=step if case in "ab" else None):
                for s, w, mode in batches:
                    if case == "c":
                        error = crit(model(s), model(sample=s, negative_sample=sampler.generate(sample=s, mode=mode), mode=mode), w)
                        (error + torch_n3(model, s, w, args.weight)).backward()
                    else:
                        step.sampled(s, w, sampler, mode)
                    opt.step()
                    opt.zero_grad()

            runs[case] = run
        times = {case: [] for case in cases}
        for rep in range(args.reps + 1):
            for case in cases:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                runs[case]()
                torch.cuda.synchronize()
                if rep:
                    times[case].append((time.perf_counter() - t0) / len(batches) * 1e3)
        best = {case: min(t) for case, t in times.items()}
        cells = [f"{case} {best[case]:.3f} ({max(times[case]) - best[case]:.3f})" for case in cases]
        extra = [f"{best['b'] - best['a']:+.3f}" if "a" in best and "b" in best else "-",
                 f"{best['c'] / best['b']:.2f}x" if "b" in best and "c" in best else "-"]
        lines.append(" | ".join([name] + cells + extra))
        print(lines[-1], flush=True)
        del runs
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as handle:
            handle.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
