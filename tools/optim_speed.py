"""What the optimizer costs a fused training step: row-sparse Adagrad against dense torch Adagrad, with row-lazy Adam for orientation:

    python tools/optim_speed.py [--steps 200] [--reps 5] [--cases d,g,n,a] [--models TransE,RotatE,ComplEx] [--out FILE]

FB15k-237's tables, hidden 1000, B = 1024, K = 256; every case runs fused.FusedTrainStep through ``step.sampled(...)``, then
``optimizer.step()`` and ``optimizer.zero_grad()``:
  d  torch.optim.Adagrad on the dense ``.grad`` (what can be written without mkb_amd.optim.Adagrad): every step streams the whole
     entity table, its gradient and its accumulator through ATen's kernels, and ``zero_grad()`` makes the next step fill a fresh
     dense gradient;
  g  mkb_amd.optim.Adagrad with the sampler's next draw riding its launch (``draw_ahead=sampler``);
  n  mkb_amd.optim.Adagrad without the draw (the sampler draws in a launch of its own);
  a  mkb_amd.optim.Adam(lazy_rows=True, defer_step=True, draw_ahead=sampler), for orientation.
Each repetition times ``steps`` steps between two device synchronisations; the cases alternate repetition by repetition, repetition
0 warms up.  Reported per case: the best of ``reps`` and the spread (worst - best) in ms per step; then d / g, and whether g is
ahead of d by more than d's spread.

Then the kernels on their own (``--kernel-reps`` launches each, hipEvents around every launch: ``_hip.profile_read("adam")``):
``mkb_adagrad_step`` and ``mkb_adam_rows_step`` over the row list of one batch (pool | heads | tails, with its duplicates) of a
[n_entity, 2 * hidden] table, every listed gradient row non-zero."""
import argparse
import sys
import time

import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from mkb_amd import _hip, datasets, models, optim, sampling  # noqa: E402
from mkb_amd.fused import FusedTrainStep  # noqa: E402


def kernel_times(ids, n_rows, D, launches, reps):
    """-> {name: (best, spread)} in us per launch."""
    lib, dev = _hip.lib(), ids.device
    p, g, a, b = (torch.zeros(n_rows, D, device=dev) for _ in range(4))
    consts = torch.zeros((launches * (reps + 1) + 2, 2), device=dev)
    uniq = torch.unique(ids)
    out = {}
    for name in ("mkb_adagrad_step", "mkb_adam_rows_step"):
        last = torch.zeros(n_rows, dtype=torch.int32, device=dev)
        a.zero_(), b.zero_()
        step, times = 0, []
        _hip.profile_enable("adam", True)
        for rep in range(reps + 1):
            _hip.profile_read("adam")
            for _ in range(launches):
                step += 1
                g[uniq] = 1e-3  # (outside the bracketed launch)
                if name == "mkb_adagrad_step":
                    rc = lib.mkb_adagrad_step(_hip.ptr(p), _hip.ptr(g), _hip.ptr(a), _hip.ptr(last), n_rows, D, _hip.ptr(ids), ids.numel(),
                                              step, 1e-3, 1e-10, None, 0, None, _hip.stream_ptr())
                else:
                    rc = lib.mkb_adam_rows_step(_hip.ptr(p), _hip.ptr(g), _hip.ptr(a), _hip.ptr(b), _hip.ptr(last), _hip.ptr(consts), n_rows, D,
                                                _hip.ptr(ids), ids.numel(), step, 1e-3, 0.9, 0.999, 1e-8, None, _hip.stream_ptr())
                _hip.check(rc, name)
            n, ms = _hip.profile_read("adam")
            if rep:
                times.append(ms / n * 1e3)
        _hip.profile_enable("adam", False)
        out[name] = (min(times), max(times) - min(times))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hidden", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--models", default="TransE,RotatE,ComplEx")
    ap.add_argument("--cases", default="d,g,n,a")
    ap.add_argument("--kernel-reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_speed.py measures on a ROCm device: none found")
    cases = args.cases.split(",")

    ds = datasets.Fb15k237(batch_size=args.batch, shuffle=True, seed=42, num_workers=0)
    batches = []
    for data in datasets.DeviceBatches(ds, "cuda", seed=42):
        if data["sample"].shape[0] == args.batch:
            batches.append((data["sample"], data["weight"], data["mode"]))
        if len(batches) == args.steps:
            break
    lines = [f"# optim_speed: n_entity {len(ds.entities)}, n_relation {len(ds.relations)}, hidden {args.hidden}, B {args.batch}, K {args.size}, "
             f"{len(batches)} steps per repetition, best of {args.reps}; ms per step (sampler, fused step, optimizer step, zero_grad)",
             "# model | case best (spread) ... | d / g | g ahead of d by more than d's spread"]
    for name in args.models.split(","):
        runs = {}
        for case in cases:
            torch.manual_seed(42)
            model = getattr(models, name)(hidden_dim=args.hidden, entities=ds.entities, relations=ds.relations, gamma=9.0).cuda()
            sampler = sampling.NegativeSampling(size=args.size, train_triples=ds.train, entities=ds.entities, relations=ds.relations, seed=42)
            params = [p for p in model.parameters() if p.requires_grad]
            if case == "d":
                opt = torch.optim.Adagrad(params, lr=args.lr)
            elif case in ("g", "n"):
                opt = optim.Adagrad(params, lr=args.lr, draw_ahead=sampler if case == "g" else None)
            else:
                opt = optim.Adam(params, lr=args.lr * 1e-2, lazy_rows=True, draw_ahead=sampler, defer_step=True)
            step = FusedTrainStep(model, 1.0)

            def run(sampler=sampler, opt=opt, step=step):
                for s, w, mode in batches:
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
        spread = {case: max(t) - min(t) for case, t in times.items()}
        cells = [f"{case} {best[case]:.3f} ({spread[case]:.3f})" for case in cases]
        extra = ["-", "-"]
        if "d" in best and "g" in best:
            extra = [f"{best['d'] / best['g']:.2f}x", "yes" if best["d"] - best["g"] > spread["d"] else "NO"]
        lines.append(" | ".join([name] + cells + extra))
        print(lines[-1], flush=True)
        del runs
        torch.cuda.empty_cache()
    if args.kernel_reps > 0:
        s, _, mode = batches[0]
        sampler = sampling.NegativeSampling(size=args.size, train_triples=ds.train, entities=ds.entities, relations=ds.relations, seed=42)
        ids = sampler.generate(s, mode)._mkb_pool.rows(s).clone()
        D = 2 * args.hidden
        kt = kernel_times(ids, len(ds.entities), D, args.kernel_reps, args.reps)
        distinct = int(torch.unique(ids).numel())
        lines.append(f"# the kernels alone: {ids.numel()} listed rows ({distinct} distinct) of a [{len(ds.entities)}, {D}] table, us per launch "
                     f"(hipEvents around each launch), best of {args.reps} x {args.kernel_reps} (spread); bytes moved: distinct rows x {4 * D} B x "
                     "6 arrays (Adagrad: p, g, sum in; p, sum, g out) or x 8 (Adam: p, g, m, v in; p, m, v, g out)")
        for kname, (b, sp) in kt.items():
            arrays = 6 if kname == "mkb_adagrad_step" else 8
            mb = distinct * 4 * D * arrays / 1e6
            lines.append(f"{kname} | {b:.2f} ({sp:.2f}) us | {mb:.1f} MB | {mb / b:.2f} TB/s")  # (MB per us)
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as handle:
            handle.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
