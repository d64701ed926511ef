"""fused.KvsAllStep against what a user can write without it, per (model, optimizer) cell:

    python tools/kvsall_speed.py [--steps 50] [--reps 5] [--out FILE]

FB15k-237's tables (14,541 entities), hidden 1000, B = 1024, label smoothing 0.1; ComplEx and DistMult x optim.Adagrad and dense
optim.Adam.  Routes:
  (a) step      fused.KvsAllStep (mkb_all_kvs_step: forward product, the multi-label BCE kernel reading the labels from the sorted
                keys, the two backward products, the query chain);
  (b) torch     the query built with torch from the tables, q @ E.T, a dense [B, N] multi-hot matrix scattered on the device from
                the same sorted keys, F.binary_cross_entropy_with_logits (weighted per row), backward();
  (c) 1vsAll    for context: fused.OneVsAllStep on the same batches.
Every route runs the same batches and is followed by the same optimizer's step + zero_grad.  Each repetition times `steps` steps
between two device synchronisations; the routes alternate repetition by repetition; reported: the best of `reps` and the spread
(worst - best) of each route in ms per step.  (a) is "ahead" of (b) only where its best beats (b)'s best by more than (b)'s spread.
Last, the two loss kernels alone on one [B, Npad] block: `steps` launches back to back between two device events."""
import argparse
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from mkb_amd import datasets, models, optim  # noqa: E402
from mkb_amd.fused import KvsAllStep, OneVsAllStep  # noqa: E402
from mkb_amd.losses import kvs_all, one_vs_all  # noqa: E402
from mkb_amd.utils.true_keys import true_keys  # noqa: E402
from onevsall_speed import torch_query  # noqa: E402


def multi_hot(sample, mode, keys, N, R):
    """Y [B, N] of 0 / 1 on the device from the sorted keys of ``mode``'s side."""
    q = sample[:, 2 if mode == "head-batch" else 0] * R + sample[:, 1]
    lo, hi = torch.searchsorted(keys, q * N), torch.searchsorted(keys, (q + 1) * N)
    n = hi - lo
    row = torch.repeat_interleave(torch.arange(len(q), device=q.device), n)
    first = torch.cumsum(n, 0) - n
    at = torch.arange(row.numel(), device=q.device) - first[row] + lo[row]
    Y = torch.zeros((len(q), N), dtype=torch.float32, device=q.device)
    Y[row, keys[at] - q[row] * N] = 1.0
    return Y


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
        raise SystemExit("kvsall_speed.py measures on a ROCm device: none found")

    ds = datasets.Fb15k237(batch_size=args.batch, shuffle=True, seed=42, num_workers=0)
    N, R, eps = len(ds.entities), len(ds.relations), args.smoothing
    batches = []
    for data in datasets.DeviceBatches(ds, "cuda", seed=42):
        if data["sample"].shape[0] == args.batch:
            batches.append((data["sample"], data["weight"], data["mode"]))
        if len(batches) == args.steps:
            break
    keys = true_keys(ds.train, torch.device("cuda", torch.cuda.current_device()), N, R)
    n_labels = sum(float(multi_hot(s, mode, keys[mode], N, R).sum()) for s, _, mode in batches) / (len(batches) * args.batch)
    lines = [f"# kvsall_speed: n_entity {N}, n_relation {R}, hidden {args.hidden}, B {args.batch}, label smoothing {eps}, "
             f"{n_labels:.2f} labels per row, {len(batches)} steps per repetition, best of {args.reps}; ms per step (forward, loss, backward, "
             "optimizer step)",
             "# model optimizer | (a) KvsAllStep best (spread) | (b) torch best (spread) | (a) ahead by | verdict | (c) OneVsAllStep best (spread)"]
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
            step_a, step_c = KvsAllStep(m_a, ds.train, label_smoothing=eps), OneVsAllStep(m_c)

            def run_a():
                for s, w, mode in batches:
                    step_a(s, w, mode)
                    opt_a.step()
                    opt_a.zero_grad()

            def run_b():
                ent, rel = m_b.entity_embedding, m_b.relation_embedding
                for s, w, mode in batches:
                    scores = torch_query(name, ent, rel, s, mode) @ ent.t()
                    y = (1.0 - eps) * multi_hot(s, mode, keys[mode], N, R) + eps / N
                    rows = F.binary_cross_entropy_with_logits(scores, y, reduction="none").mean(1)
                    ((w * rows).sum() / w.sum()).backward()
                    opt_b.step()
                    opt_b.zero_grad()

            def run_c():
                for s, w, mode in batches:
                    step_c(s, w, mode)
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

    # the two loss kernels alone (each launch pair: the row kernel + the one-workgroup loss finish)
    s, w, mode = batches[0]
    ld = (N + 3) & ~3
    block = torch.randn((args.batch, ld), device="cuda") * 4.0
    runs = {"all_bce_kernel": lambda S: kvs_all.launch(S, N, s, 1 if mode == "head-batch" else 2, R, keys[mode], w, None, eps, "mean"),
            "all_softmax_kernel": lambda S: one_vs_all.launch(S, N, s[:, 0 if mode == "head-batch" else 2].contiguous(), 1, w, None, 1.0)}
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
