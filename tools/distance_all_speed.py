"""Step time of the all-entity losses of the distance models (fused.DistanceAllStep) at FB15k-237's size: 14,541 entities, 237
relations, hidden 1000, B = 1024.

    python tools/distance_all_speed.py [--out profiles/r26_distance_all_speed.txt] [--rounds 5] [--steps 20]

  step      ms per step (the step + optimizer.step + zero_grad) of the 1vsAll softmax for TransE / RotatE / pRotatE with optim.Adagrad
            and optim.Adam(): best of --rounds rounds of --steps steps, with the spread of the rounds;
  split     the kernels of one RotatE step by phase (forward, loss, dQ pass, dE pass, chain), from torch.profiler's kernel records;
  sampled   the sampled softmax step (PooledLossStep, CrossEntropy, K = 256) beside it;
  torch     the same loss through torch alone, the best route this file could write: the [B, N] block chunk by chunk over the
            entities without a graph, the loss and its seeds on the block, then every chunk recomputed with a graph and back-propagated
            with its columns of the seeds (hand-made checkpointing: memory stays at one [B, chunk, De] expression);
  terms     pair terms per second of the two backward passes, against the pooled backward's (RotatE's pool_bwd1_kernel, the headline)
            (profiles/r06_kernel_trace_stats.txt: 92.44 us for 1024 rows x 512 pool positions x 1000 units, both gradients from one
            evaluation).
"""
import argparse
import sys
import time

import numpy as np
import torch

ROOT = __file__.rsplit("/", 2)[0]
sys.path.insert(0, ROOT)
from mkb_amd import fused, losses, models, optim, sampling  # noqa: E402

N, R, HIDDEN, B, K = 14541, 237, 1000, 1024, 256
POOL_BWD1_TERMS_PER_S = 1024 * 512 * 1000 / 92.44e-6


def make(name):
    torch.manual_seed(42)
    return getattr(models, name)(hidden_dim=HIDDEN, entities={i: i for i in range(N)}, relations={i: i for i in range(R)}, gamma=9.0).cuda()


def batch(seed=1):
    rs = np.random.RandomState(seed)
    sample = torch.from_numpy(np.stack([rs.randint(N, size=B), rs.randint(R, size=B), rs.randint(N, size=B)], 1)).cuda()
    return sample, torch.from_numpy(rs.uniform(0.5, 1.5, size=B).astype(np.float32)).cuda()


def timed(run, rounds, steps):
    """-> (best, worst) ms per call over the rounds, after two warm-up calls."""
    for _ in range(2):
        run()
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(steps):
            run(k)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / steps * 1e3)
    return min(out), max(out)


def all_entity(name, which, rounds, steps):
    m = make(name)
    params = [p for p in m.parameters() if p.requires_grad]
    opt = optim.Adagrad(params, lr=0.1) if which == "adagrad" else optim.Adam(params, lr=1e-4)
    step = fused.DistanceAllStep(m, losses.OneVsAll())
    sample, w = batch()

    def run(k=0):
        step(sample, w, "tail-batch" if k % 2 else "head-batch")
        opt.step()
        opt.zero_grad()

    return timed(run, rounds, steps)


def sampled(name, rounds, steps):
    m = make(name)
    train = [(int(h), int(r), int(t)) for h, r, t in batch(2)[0].cpu().numpy()]
    sampler = sampling.NegativeSampling(size=K, train_triples=train, entities={i: i for i in range(N)}, relations={i: i for i in range(R)}, seed=42)
    opt = optim.Adam([p for p in m.parameters() if p.requires_grad], lr=1e-4, lazy_rows=True, draw_ahead=sampler)
    step = fused.PooledLossStep(m, losses.CrossEntropy())
    sample, w = batch()

    def run(k=0):
        step.sampled(sample, w, sampler, "tail-batch" if k % 2 else "head-batch")
        opt.step()
        opt.zero_grad()

    return timed(run, rounds, steps)


def torch_route(name, rounds, steps, chunk=128):
    """tail-batch RotatE / TransE in torch alone (module docstring)."""
    m = make(name)
    ent, rel = m.entity_embedding, m.relation_embedding
    gamma, kd = m._constants()
    sample, w = batch()

    def block(q, x):  # [B, n] scores of the entity rows x against the queries q
        if name == "TransE":
            return gamma - (q[:, None] - x[None]).abs().sum(-1)
        d = HIDDEN
        a, b = q[:, None, :d] - x[None, :, :d], q[:, None, d:] - x[None, :, d:]
        return gamma - torch.sqrt(a * a + b * b).sum(-1)

    def query():
        h, r = ent[sample[:, 0]], rel[sample[:, 1]]
        if name == "TransE":
            return h + r
        c, s = torch.cos(r / kd), torch.sin(r / kd)
        return torch.cat([h[:, :HIDDEN] * c - h[:, HIDDEN:] * s, h[:, :HIDDEN] * s + h[:, HIDDEN:] * c], 1)

    def run(k=0):
        with torch.no_grad():
            q = query()
            S = torch.cat([block(q, ent[lo: lo + chunk]) for lo in range(0, N, chunk)], 1)
        S.requires_grad_(True)
        row = torch.logsumexp(S, 1) - S[torch.arange(B, device=S.device), sample[:, 2]]
        loss = (w * row).sum() / w.sum()
        loss.backward()
        q = query()
        for lo in range(0, N, chunk):  # (the graph of q is kept across the chunks: its backward runs once, at the end)
            block(q, ent[lo: lo + chunk]).backward(S.grad[:, lo: lo + chunk], retain_graph=True)
        ent.grad = None
        rel.grad = None

    return timed(run, rounds, steps)


PHASES = (("forward", ("query_build", "pool_fwd_tile", "all_fwd_kernel", "iota_kernel", "dist_affine")),
          ("loss", ("all_softmax", "weight_sum", "row_loss", "finish")),
          ("dQ pass", ("dist_dq",)), ("dE pass", ("dist_de", "dist_mod")),
          ("chain", ("all_chain", "all_stash", "sort", "Sort", "radix", "pair_key", "scan", "histogram")))


def split(name, steps=5):
    """{phase: ms per step} of the step's own kernels (no optimizer), from the profiler's kernel records; None if it has none."""
    from torch.profiler import ProfilerActivity, profile

    m = make(name)
    step = fused.DistanceAllStep(m, losses.OneVsAll())
    sample, w = batch()
    for _ in range(2):
        step(sample, w, "tail-batch")
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        for _ in range(steps):
            step(sample, w, "tail-batch")
        torch.cuda.synchronize()
    out, other = {p: 0.0 for p, _ in PHASES}, {}
    for ev in prof.events():
        if getattr(ev, "device_type", None) is None or "cuda" not in str(ev.device_type).lower():
            continue
        us = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
        for phase, keys in PHASES:
            if any(k in ev.name for k in keys):
                out[phase] += us / steps / 1e3
                break
        else:
            other[ev.name[:60]] = other.get(ev.name[:60], 0.0) + us / steps / 1e3
    return (out, other) if sum(out.values()) > 0 else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/r26_distance_all_speed.txt")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--torch-steps", type=int, default=2)
    args = ap.parse_args()
    lines = [f"# all-entity 1vsAll step of the distance models, {torch.cuda.get_device_name(0)}: N = {N}, R = {R}, hidden {HIDDEN}, B = {B}",
             f"# ms per step (step + optimizer.step + zero_grad), best of {args.rounds} rounds of {args.steps} steps (worst round in brackets)"]

    def say(line):
        lines.append(line)
        print(line, flush=True)
        with open(args.out, "w") as f:  # (kept current: a later phase that fails leaves the earlier ones on file)
            f.write("\n".join(lines) + "\n")

    best = {}
    for name in ("RotatE", "TransE", "pRotatE"):
        for which in ("adagrad", "adam"):
            lo, hi = all_entity(name, which, args.rounds, args.steps)
            best[name, which] = lo
            say(f"DistanceAllStep {name:8s} {which:8s} {lo:9.3f} ms ({hi:.3f})")
        lo, hi = sampled(name, args.rounds, args.steps)
        say(f"sampled softmax {name:8s} K = {K}, adam(lazy_rows) {lo:9.3f} ms ({hi:.3f})   all-entity / sampled = {best[name, 'adam'] / lo:.1f}x for {N / (K + 1):.0f}x the candidates")
    for name in ("RotatE", "TransE", "pRotatE"):
        found = split(name)
        if found is None:
            say(f"split {name}: the profiler returned no kernel records")
            continue
        out, other = found
        say(f"split {name:8s} (step alone, ms per step): " + ", ".join(f"{p} {v:.3f}" for p, v in out.items())
            + (" | not classed: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(other.items(), key=lambda kv: -kv[1])[:4]) if other else ""))
        terms = B * N * HIDDEN
        for p in ("dQ pass", "dE pass"):
            if out[p] > 0:
                rate = terms / (out[p] * 1e-3)
                say(f"terms {name:8s} {p}: {rate:.3e} pair terms / s = {rate / POOL_BWD1_TERMS_PER_S:.2f} x the {POOL_BWD1_TERMS_PER_S:.3e} of RotatE's pool_bwd1_kernel (one gradient per pass here, both there)")
    for name in ("RotatE", "TransE"):
        lo, hi = torch_route(name, 2, args.torch_steps)
        say(f"torch route     {name:8s} chunked over entities, recomputed per chunk, no optimizer: {lo:9.3f} ms ({hi:.3f}); "
            f"DistanceAllStep with adagrad is {lo / best[name, 'adagrad']:.1f}x faster, "
            + ("more" if lo - best[name, "adagrad"] > hi - lo else "NOT more") + " than that route's spread")


if __name__ == "__main__":
    main()
