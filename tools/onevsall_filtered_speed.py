"""fused.OneVsAllStep with filtering and label smoothing against plain 1vsAll and against what a user could write before, per
(model, optimizer) cell:

    python tools/onevsall_filtered_speed.py [--steps 50] [--reps 5] [--out FILE]

FB15k-237's tables (14,541 entities), hidden 1000, B = 1024, label smoothing 0.1, the training triples as known answers; ComplEx
and DistMult x optim.Adagrad and dense optim.Adam.  Routes:
  (a) filtered  fused.OneVsAllStep(label_smoothing, true_triples) (mkb_all_filtered_step: forward product, the filtered softmax
                kernel reading the known answers from the sorted keys, the two backward products, the query chain);
  (b) torch     the query built with torch from the tables, q @ E.T, a dense [B, N] mask scattered on the device from the same
                sorted keys (the target's column cleared), masked_fill(-inf), a hand-written smoothed log-softmax over the kept
                columns (weighted per row), backward();
  (c) plain     fused.OneVsAllStep at its defaults (mkb_all_step, all_softmax_kernel: the code of the commit before this
                feature, untouched by it) on the same batches.
Every route runs the same batches and is followed by the same optimizer's step + zero_grad.  Each repetition times `steps` steps
between two device synchronisations; the routes alternate repetition by repetition; reported: the best of `reps` and the spread
(worst - best) of each route in ms per step.  (a) is "ahead" of (b) only where its best beats (b)'s best by more than (b)'s spread;
(a) is "slower" than (c) only where its best is behind (c)'s best by more than (a)'s own spread.
Last, the two softmax kernels alone on one [B, Npad] block: `steps` launches back to back between two device events."""
import argparse
import sys
import time

import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from mkb_amd import datasets, models, optim  # noqa: E402
from mkb_amd.fused import OneVsAllStep  # noqa: E402
from mkb_amd.losses import one_vs_all  # noqa: E402
from mkb_amd.utils.true_keys import true_keys  # noqa: E402
from kvsall_speed import multi_hot  # noqa: E402
from onevsall_speed import torch_query  # noqa: E402


def filtered_mask(sample, mode, keys, N, R):
    """F [B, N] bool on the device: the known answers of each row's query without the row's own target."""
    mask = multi_hot(sample, mode, keys, N, R) > 0
    mask[torch.arange(len(sample), device=sample.device), sample[:, 0 if mode == "head-batch" else 2]] = False
    return mask


def torch_rows(scores, target, mask, eps):
    """The smoothed cross entropy over the kept columns, per row (F.cross_entropy(label_smoothing=...) is NaN on -inf columns)."""
    logp = torch.log_softmax(scores.masked_fill(mask, float("-inf")), 1)
    n = (~mask).sum(1)
    lin = logp.masked_fill(mask, 0.0).sum(1)
    return -(1.0 - eps) * logp.gather(1, target.view(-1, 1)).squeeze(1) - (eps / n) * lin


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hidden", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--smoothing", type=float, default=0.1)
    ap.add_argument("--models", default="ComplEx,DistMult")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("onevsall_filtered_speed.py measures on a ROCm device: none found")

    ds = datasets.Fb15k237(batch_size=args.batch, shuffle=True, seed=42, num_workers=0)
    N, R, eps = len(ds.entities), len(ds.relations), args.smoothing
    batches = []
    for data in datasets.DeviceBatches(ds, "cuda", seed=42):
        if data["sample"].shape[0] == args.batch:
            batches.append((data["sample"], data["weight"], data["mode"]))
        if len(batches) == args.steps:
            break
    keys = true_keys(ds.train, torch.device("cuda", torch.cuda.current_device()), N, R)
    n_filtered = sum(float(filtered_mask(s, mode, keys[mode], N, R).sum()) for s, _, mode in batches) / (len(batches) * args.batch)
    lines = [f"# onevsall_filtered_speed: n_entity {N}, n_relation {R}, hidden {args.hidden}, B {args.batch}, label smoothing {eps}, "
             f"{n_filtered:.2f} filtered columns per row, {len(batches)} steps per repetition, best of {args.reps}; ms per step (forward, "
             "loss, backward, optimizer step)",
             "# model optimizer | (a) filtered step best (spread) | (b) torch best (spread) | (a) ahead of (b) by | verdict | "
             "(c) plain OneVsAllStep best (spread) | (a) - (c) | verdict"]
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
            step_a, step_c = OneVsAllStep(m_a, label_smoothing=eps, true_triples=ds.train), OneVsAllStep(m_c)

            def run_a():
                for s, w, mode in batches:
                    step_a(s, w, mode)
                    opt_a.step()
                    opt_a.zero_grad()

            def run_b():
                ent, rel = m_b.entity_embedding, m_b.relation_embedding
                for s, w, mode in batches:
                    scores = torch_query(name, ent, rel, s, mode) @ ent.t()
                    rows = torch_rows(scores, s[:, 0 if mode == "head-batch" else 2], filtered_mask(s, mode, keys[mode], N, R), eps)
                    ((w * rows).sum() / w.sum()).backward()
                    opt_b.step()
                    opt_b.zero_grad()

            def run_c():
                for s, w, mode in batches:
                    step_c(s, w, mode)
                    opt_c.step()
                    opt_c.zero_grad()

            times = {"a": [], "b": [], "c": []}
            for rep in range(args.reps + 1):  # (the first repetition warms up: workspaces, optimizer state, the key arrays)
                for key, run in (("a", run_a), ("b", run_b), ("c", run_c)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    run()
                    torch.cuda.synchronize()
                    if rep:
                        times[key].append((time.perf_counter() - t0) * 1e3 / len(batches))
            best = {k: min(v) for k, v in times.items()}
            spread = {k: max(v) - min(v) for k, v in times.items()}
            gap, over = best["b"] - best["a"], best["a"] - best["c"]
            verdict = "ahead" if gap > spread["b"] else ("behind" if -gap > spread["b"] else "within (b)'s spread")
            cost = "slower" if over > spread["a"] else ("faster" if -over > spread["a"] else "within (a)'s spread")
            lines.append(f"{name} {opt_name} | {best['a']:.3f} ({spread['a']:.3f}) | {best['b']:.3f} ({spread['b']:.3f}) | {gap:+.3f} | {verdict} | "
                         f"{best['c']:.3f} ({spread['c']:.3f}) | {over:+.3f} | {cost}")
            print(lines[-1], flush=True)

    # the two softmax kernels alone (each launch pair: the row kernel + the one-workgroup loss finish)
    s, w, mode = batches[0]
    ld = (N + 3) & ~3
    block = torch.randn((args.batch, ld), device="cuda") * 4.0
    target = s[:, 0 if mode == "head-batch" else 2].contiguous()
    runs = {"all_softmax_filtered_kernel": lambda S: one_vs_all.launch_filtered(S, N, target, 1, s, 1 if mode == "head-batch" else 2, R, keys[mode],
                                                                                 w, None, 1.0, eps),
            "all_softmax_kernel": lambda S: one_vs_all.launch(S, N, target, 1, w, None, 1.0)}
    kernel = {k: [] for k in runs}
    for rep in range(args.reps + 1):
        for k, run in runs.items():
            S = block.clone()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(args.steps):
                run(S)
            b.record()
            torch.cuda.synchronize()
            if rep:
                kernel[k].append(a.elapsed_time(b) / args.steps)
    lines.append(f"# loss launches alone on a [{args.batch}, {ld}] block, {args.steps} back to back between two events, ms per launch pair, "
                 "best (spread): " + ", ".join(f"{k} {min(v):.4f} ({max(v) - min(v):.4f})" for k, v in kernel.items()))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
