"""The pool samplers (sampling.WeightedNegativeSampling, sampling.InBatchNegativeSampling) inside the fused training step, against
the uniform device sampler on the same commit and against what could be written before them, per model:

    python tools/pool_sampler_speed.py [--steps 200] [--reps 5] [--out FILE]

FB15k-237's tables, hidden 1000, B = 1024, K = 256; TransE, RotatE, ComplEx; fused.FusedTrainStep (Adversarial) with
optim.Adam(lazy_rows=True, defer_step=True).  A step is: negatives for the batch, the fused step, optimizer.step(), zero_grad().
Routes:
    uniform         sampling.NegativeSampling(rng="rocrand") through step.sampled (its filter rides the optimizer's catch-up launch)
    weighted        WeightedNegativeSampling("degree", 0.75) through step.sampled (mkb_pool_draw_alias + mkb_pool_filter)
    inbatch         InBatchNegativeSampling through step.sampled (torch indexing + mkb_pool_filter)
    weighted-torch  what could be written before: torch.multinomial pool, the filter in torch (searchsorted in the sorted keys, a
                    stable argsort for the cyclic fill), PoolInfo.discover (torch.unique, a sort and a host sync), then the step
    inbatch-torch   the same with the in-batch pool
Each repetition times `steps` steps between two device synchronisations; the routes alternate repetition by repetition; reported:
the best of `reps` and the spread (worst - best) of each route.  A new sampler is ahead of its torch route where the torch route's
best exceeds its best by more than the torch route's spread.  Last, the two new kernels' own times (the library's event brackets, 200 launches each)."""
import argparse
import sys
import time

import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from mkb_amd import _hip, datasets, models, optim, sampling  # noqa: E402
from mkb_amd.fused import FusedTrainStep  # noqa: E402
from mkb_amd.sampling.negative_sampling import PoolInfo  # noqa: E402
from mkb_amd.utils.true_keys import true_keys  # noqa: E402


class TorchPoolRoute:
    """Negatives from a pool with torch alone, handed to the step through PoolInfo.discover."""

    def __init__(self, ds, size, kind, probabilities=None, seed=42):
        self.size, self.kind, self.N, self.R, self.train = size, kind, len(ds.entities), len(ds.relations), ds.train
        self.p = None if probabilities is None else torch.as_tensor(probabilities, dtype=torch.float32, device="cuda")
        self.gen = torch.Generator(device="cuda").manual_seed(seed)
        self.steps = torch.arange(2 * size, device="cuda")
        self.slots = torch.arange(size, device="cuda")

    def generate(self, sample, mode):
        K, head = self.size, mode == "head-batch"
        if self.kind == "weighted":
            pool = torch.multinomial(self.p, 2 * K, replacement=True, generator=self.gen)
        else:
            o = torch.randint(sample.shape[0], (1,), device="cuda", generator=self.gen)
            pool = sample[(self.steps + o) % sample.shape[0], 0 if head else 2]
        keys = true_keys(self.train, sample.device, self.N, self.R)[mode]
        fixed, target = (sample[:, 2], sample[:, 0]) if head else (sample[:, 0], sample[:, 2])
        want = ((fixed * self.R + sample[:, 1]) * self.N).view(-1, 1) + pool.view(1, -1)
        at = torch.searchsorted(keys, want).clamp_(max=keys.numel() - 1)
        keep = (keys[at] != want) & (pool.view(1, -1) != target.view(-1, 1))
        order = torch.argsort(~keep, dim=1, stable=True)  # kept positions first, in pool order
        pos = order.gather(1, self.slots.view(1, -1) % keep.sum(1, keepdim=True).clamp_(min=1))
        neg = pool[pos]
        neg._mkb_pool = PoolInfo.discover(neg, sample, _hip.mode_id(mode))
        return neg


def kernel_times(ds, size, batch, n=200):
    """ms per launch of mkb_pool_draw_alias and of mkb_pool_filter (head-batch and tail-batch alternating): the library's own
    event brackets around each launch (mkb_profile_enable), so the host's time between launches is not counted."""
    ws = sampling.WeightedNegativeSampling(size, ds.train, ds.entities, ds.relations, seed=1)
    sample = torch.as_tensor(ds.train[:batch], dtype=torch.int64, device="cuda")
    pool = ws._pool(sample, "tail-batch")
    out = {}
    for what, fn in (("mkb_pool_draw_alias", lambda i: ws._pool(sample, "tail-batch")),
                     ("mkb_pool_filter", lambda i: sampling.negatives_from_pool(sample, "head-batch" if i % 2 else "tail-batch", pool, size,
                                                                                 ds.train, ws.n_entity, ws.n_relation))):
        for i in range(10):
            fn(i)
        torch.cuda.synchronize()
        _hip.profile_enable("sampler", True)
        for i in range(n):
            fn(i)
        launches, total_ms = _hip.profile_read("sampler")
        _hip.profile_enable("sampler", False)
        assert launches == n, launches
        out[what] = total_ms / n
    return out


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
        raise SystemExit("pool_sampler_speed.py measures on a ROCm device: none found")

    ds = datasets.Fb15k237(batch_size=args.batch, shuffle=True, seed=42, num_workers=0)
    batches = []
    for data in datasets.DeviceBatches(ds, "cuda", seed=42):
        if data["sample"].shape[0] == args.batch:
            batches.append((data["sample"], data["weight"], data["mode"]))
        if len(batches) == args.steps:
            break
    common = dict(size=args.size, train_triples=ds.train, entities=ds.entities, relations=ds.relations, seed=42)
    weighted = sampling.WeightedNegativeSampling(**common)
    samplers = {"uniform": sampling.NegativeSampling(rng="rocrand", **common), "weighted": weighted,
                "inbatch": sampling.InBatchNegativeSampling(**common),
                "weighted-torch": TorchPoolRoute(ds, args.size, "weighted", weighted.probabilities),
                "inbatch-torch": TorchPoolRoute(ds, args.size, "inbatch")}
    lines = [f"# pool_sampler_speed: n_entity {len(ds.entities)}, n_relation {len(ds.relations)}, hidden {args.hidden}, B {args.batch}, "
             f"K {args.size}, {len(batches)} steps per repetition, best of {args.reps}; ms per step (negatives, FusedTrainStep, "
             f"optim.Adam(lazy_rows=True, defer_step=True) step, zero_grad); best (spread)",
             "# model | " + " | ".join(samplers) + " | weighted ahead of its torch route | inbatch ahead of its torch route | "
             "inbatch - uniform"]
    for name in args.models.split(","):
        times = {key: [] for key in samplers}
        runs = {}
        for key, sampler in samplers.items():
            torch.manual_seed(42)
            model = getattr(models, name)(hidden_dim=args.hidden, entities=ds.entities, relations=ds.relations, gamma=9.0).cuda()
            opt = optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-5, lazy_rows=True, defer_step=True)
            step = FusedTrainStep(model, 1.0)

            def run(step=step, opt=opt, sampler=sampler, torch_route=key.endswith("-torch")):
                for s, w, mode in batches:
                    if torch_route:
                        step(s, w, sampler.generate(s, mode), mode)
                    else:
                        step.sampled(s, w, sampler, mode)
                    opt.step()
                    opt.zero_grad()

            runs[key] = (run, model, opt)
        for rep in range(args.reps + 1):  # repetition 0 warms every route up (code objects, workspaces, the allocator)
            for key, (run, _, _) in runs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run()
                torch.cuda.synchronize()
                if rep:
                    times[key].append((time.perf_counter() - t0) / len(batches) * 1e3)
        for key in ("uniform", "weighted", "inbatch"):
            samplers[key].check()
        best = {key: min(v) for key, v in times.items()}
        spread = {key: max(v) - min(v) for key, v in times.items()}
        verdict = lambda new, old: f"{best[old] - best[new]:+.3f} ({'yes' if best[old] - best[new] > spread[old] else 'NO'})"
        lines.append(f"{name} | " + " | ".join(f"{best[key]:.3f} ({spread[key]:.3f})" for key in samplers)
                     + f" | {verdict('weighted', 'weighted-torch')} | {verdict('inbatch', 'inbatch-torch')} | "
                     f"{best['inbatch'] - best['uniform']:+.3f}")
        print(lines[-1], flush=True)
        del runs
        torch.cuda.empty_cache()
    for what, ms in kernel_times(ds, args.size, args.batch).items():
        lines.append(f"# {what}: {ms * 1e3:.1f} us per launch (B {args.batch}, K {args.size}; an event pair around every launch)")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as handle:
            handle.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
