"""fused.OneVsAllStep against what a user can write without it, per (model, optimizer) cell:

    python tools/onevsall_speed.py [--steps 50] [--reps 5] [--out FILE]

FB15k-237's tables (14,541 entities), hidden 1000, B = 1024; ComplEx and DistMult x optim.Adagrad and dense optim.Adam.  Routes:
  (a) step      fused.OneVsAllStep (mkb_all_step: forward product, row softmax, the two backward products, the query chain);
  (b) torch     the query built with torch from the tables, q @ E.T, F.cross_entropy (weighted per row), backward();
  (c) sampled   for context: fused.PooledLossStep(CrossEntropy) against K = 256 sampled negatives.
Every route runs the same batches and is followed by the same optimizer's step + zero_grad.  Each repetition times `steps` steps
between two device synchronisations; the routes alternate repetition by repetition; reported: the best of `reps` and the spread
(worst - best) of each route in ms per step.  (a) is "ahead" of (b) only where its best beats (b)'s best by more than (b)'s spread."""
import argparse
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from mkb_amd import datasets, losses, models, optim, sampling  # noqa: E402
from mkb_amd.fused import OneVsAllStep, PooledLossStep  # noqa: E402


def torch_query(name, ent, rel, sample, mode):
    """q [B, De] with score(candidate x) = <q, x>, from the model's own expressions."""
    head = mode == "head-batch"
    e, r = ent[sample[:, 2 if head else 0]], rel[sample[:, 1]]
    if name == "DistMult":
        return e * r
    re_e, im_e = torch.chunk(e, 2, dim=1)
    re_r, im_r = torch.chunk(r, 2, dim=1)
    if head:
        return torch.cat([re_r * re_e + im_r * im_e, re_r * im_e - im_r * re_e], 1)
    return torch.cat([re_e * re_r - im_e * im_r, re_e * im_r + im_e * re_r], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hidden", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--models", default="ComplEx,DistMult")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("onevsall_speed.py measures on a ROCm device: none found")

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
    lines = [f"# onevsall_speed: n_entity {len(ds.entities)}, n_relation {len(ds.relations)}, hidden {args.hidden}, B {args.batch}, "
             f"{len(batches)} steps per repetition, best of {args.reps}; ms per step (forward, loss, backward, optimizer step)",
             f"# model optimizer | (a) OneVsAllStep best (spread) | (b) torch best (spread) | (a) ahead by | verdict | (c) sampled K={args.size} best (spread)"]
    for name in args.models.split(","):
        for opt_name in ("adagrad", "adam"):
            def fresh():
                torch.manual_seed(42)
                m = getattr(models, name)(hidden_dim=args.hidden, entities=ds.entities, relations=ds.relations, gamma=9.0).cuda()
                ps = [p for p in m.parameters() if p.requires_grad]
                return m, (optim.Adagrad(ps, lr=0.1) if opt_name == "adagrad" else optim.Adam(ps, lr=1e-5))

            m_a, opt_a = fresh()
            m_b, opt_b = fresh()
            m_c, opt_c = fresh()
            step_a, step_c = OneVsAllStep(m_a), PooledLossStep(m_c, losses.CrossEntropy())

            def run_a():
                for s, w, mode in batches:
                    step_a(s, w, mode)
                    opt_a.step()
                    opt_a.zero_grad()

            def run_b():
                ent, rel = m_b.entity_embedding, m_b.relation_embedding
                for s, w, mode in batches:
                    scores = torch_query(name, ent, rel, s, mode) @ ent.t()
                    rows = F.cross_entropy(scores, s[:, 0 if mode == "head-batch" else 2], reduction="none")
                    ((w * rows).sum() / w.sum()).backward()
                    opt_b.step()
                    opt_b.zero_grad()

            def run_c():
                for (s, w, mode), neg in zip(batches, negatives):
                    step_c(s, w, neg, mode)
                    opt_c.step()
                    opt_c.zero_grad()

            times = {"a": [], "b": [], "c": []}
            for rep in range(args.reps + 1):  # (the first repetition warms up: workspaces, optimizer state, LDS opt-ins)
                for key, run in (("a", run_a), ("b", run_b), ("c", run_c)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    run()
                    torch.cuda.synchronize()
                    if rep:
                        times[key].append((time.perf_counter() - t0) * 1e3 / len(batches))
            best = {k: min(v) for k, v in times.items()}
            spread = {k: max(v) - min(v) for k, v in times.items()}
            gap = best["b"] - best["a"]
            verdict = "ahead" if gap > spread["b"] else ("behind" if -gap > spread["b"] else "within (b)'s spread")
            lines.append(f"{name} {opt_name} | {best['a']:.3f} ({spread['a']:.3f}) | {best['b']:.3f} ({spread['b']:.3f}) | {gap:+.3f} | {verdict} | "
                         f"{best['c']:.3f} ({spread['c']:.3f})")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
