"""Step time of the relation-prediction term (losses.RelationPrediction, mkb_rel_step) at FB15k-237's size: 14,541 entities, 237
relations, hidden 1000, B = 1024.

    python tools/relation_prediction_speed.py [--out profiles/r28_relation_prediction_speed.txt] [--rounds 5] [--steps 50]

  term      ms per call of ``term.launch`` alone, the five models;
  step      ms per step (the step + optimizer.step + zero_grad) of FusedTrainStep (TransE, RotatE, ComplEx; row-lazy optim.Adam, the
            sampler's draw riding it) and OneVsAllStep (ComplEx, DistMult; optim.Adagrad), without the term, with
            ``relation_prediction=`` and with the route that could be written before: ``model.score_candidates`` over all relations +
            ``F.cross_entropy`` + ``backward()`` beside the same step -- same optimizer construction; that route's dense gradients
            through autograd are what turns a row-lazy Adam dense, which is part of what it costs.  Best of --rounds rounds of
            --steps steps; the spread is worst - best round.  A cell is "ahead" when the term's step beats that route's by more than
            that route's spread;
  split     the kernels of one ``term.launch`` by phase, from torch.profiler's kernel records, and the pair terms per second of
            the two recomputing passes (B x R x hidden terms each) against the 3.1e12 / 3.4e12 of score_all_dist.hip's passes
            (profiles/r26_distance_all_speed.txt).
"""
import argparse
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = __file__.rsplit("/", 2)[0]
sys.path.insert(0, ROOT)
from mkb_amd import fused, losses, models, optim, sampling  # noqa: E402

N, R, HIDDEN, B, K = 14541, 237, 1000, 1024, 256
LAMBDA, T = 0.25, 1.0
DIST_PASSES = (3.1e12, 3.4e12)


def make(name):
    torch.manual_seed(42)
    return getattr(models, name)(hidden_dim=HIDDEN, entities={i: i for i in range(N)}, relations={i: i for i in range(R)}, gamma=9.0).cuda()


def batch(seed=1):
    rs = np.random.RandomState(seed)
    sample = torch.from_numpy(np.stack([rs.randint(N, size=B), rs.randint(R, size=B), rs.randint(N, size=B)], 1)).cuda()
    return sample, torch.from_numpy(rs.uniform(0.5, 1.5, size=B).astype(np.float32)).cuda()


def timed(run, rounds, steps):
    """-> (best, worst) ms per call over the rounds, after three warm-up calls."""
    for k in range(3):
        run(k)
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(steps):
            run(k)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / steps * 1e3)
    return min(out), max(out)


def term_alone(name, rounds, steps):
    m = make(name)
    term = losses.RelationPrediction(LAMBDA, T)
    sample, w = batch()
    return timed(lambda k=0: term.launch(m, sample, w), rounds, steps)


def torch_term(m, sample, w, all_relations):
    ce = F.cross_entropy(m.score_candidates(sample, all_relations, "relation") / T, sample[:, 1], reduction="none")
    return LAMBDA * (w * ce).sum() / w.sum()


def step_time(kind, name, route, rounds, steps):
    """route: None (the step alone), "term" (relation_prediction=) or "torch" (the autograd route beside the step)."""
    m = make(name)
    params = [p for p in m.parameters() if p.requires_grad]
    term = losses.RelationPrediction(LAMBDA, T) if route == "term" else None
    sample, w = batch()
    all_relations = torch.arange(R, device="cuda").expand(B, R).contiguous()
    if kind == "fused":
        train = [(int(h), int(r), int(t)) for h, r, t in batch(2)[0].cpu().numpy()]
        sampler = sampling.NegativeSampling(size=K, train_triples=train, entities={i: i for i in range(N)}, relations={i: i for i in range(R)}, seed=42)
        opt = optim.Adam(params, lr=1e-4, lazy_rows=True, draw_ahead=sampler)
        step = fused.FusedTrainStep(m, 1.0, relation_prediction=term)
    else:
        sampler = None
        opt = optim.Adagrad(params, lr=0.1)
        step = fused.OneVsAllStep(m, relation_prediction=term)

    def run(k=0):
        step.sampled(sample, w, sampler, "tail-batch" if k % 2 else "head-batch")
        if route == "torch":
            torch_term(m, sample, w, all_relations).backward()
        opt.step()
        opt.zero_grad()

    return timed(run, rounds, steps)


PHASES = (("forward", ("slot_score",)), ("softmax", ("all_softmax", "weight_sum", "row_loss", "rel_scale")),
          ("pair-major pass", ("rel_bwd_pair",)), ("relation-major pass", ("rel_bwd_rel", "rel_part_reduce")),
          ("entity rows", ("rel_ent_rows", "pair_keys", "sort", "Sort", "radix", "scan", "histogram", "onesweep")), ("modulus", ("rel_mod",)))


def split(name, steps=5):
    """{phase: ms per call} of ``term.launch``'s kernels, from the profiler's kernel records; None if it has none."""
    from torch.profiler import ProfilerActivity, profile

    m = make(name)
    term = losses.RelationPrediction(LAMBDA, T)
    sample, w = batch()
    for _ in range(2):
        term.launch(m, sample, w)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        for _ in range(steps):
            term.launch(m, sample, w)
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
    ap.add_argument("--out", default="profiles/r28_relation_prediction_speed.txt")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--only-term", action="store_true", help="a few term.launch calls of RotatE and ComplEx and nothing else (for a kernel trace)")
    args = ap.parse_args()
    if args.only_term:
        for name in ("RotatE", "ComplEx"):
            m, term = make(name), losses.RelationPrediction(LAMBDA, T)
            sample, w = batch()
            for _ in range(20):
                term.launch(m, sample, w)
            torch.cuda.synchronize()
        return
    lines = [f"# relation-prediction term, {torch.cuda.get_device_name(0)}: N = {N}, R = {R}, hidden {HIDDEN}, B = {B}, lambda {LAMBDA}, T {T}",
             f"# ms, best of {args.rounds} rounds of {args.steps} (spread = worst - best round in brackets)"]

    def say(line):
        lines.append(line)
        print(line, flush=True)
        with open(args.out, "w") as f:  # (kept current: a later phase that fails leaves the earlier ones on file)
            f.write("\n".join(lines) + "\n")

    for name in ("TransE", "RotatE", "ComplEx", "DistMult", "pRotatE"):
        lo, hi = term_alone(name, args.rounds, args.steps)
        say(f"term alone      {name:8s} {lo:8.3f} ms ({hi - lo:.3f})")
    for kind, names in (("fused", ("TransE", "RotatE", "ComplEx")), ("onevsall", ("ComplEx", "DistMult"))):
        for name in names:
            cell = {route: step_time(kind, name, route, args.rounds, args.steps) for route in (None, "term", "torch")}
            (a, _), (b, b_hi), (c, c_hi) = cell[None], cell["term"], cell["torch"]
            verdict = "ahead" if c - b > c_hi - c else "NOT ahead"
            say(f"{'FusedTrainStep' if kind == 'fused' else 'OneVsAllStep':15s} {name:8s} alone {a:8.3f} | with the term {b:8.3f} ({b_hi - b:.3f}), +{b - a:.3f} | "
                f"with score_candidates + cross_entropy + backward {c:8.3f} ({c_hi - c:.3f}), +{c - a:.3f} | {verdict} by {c - b:.3f} ms against a spread of {c_hi - c:.3f}")
    for name in ("RotatE", "ComplEx", "TransE", "pRotatE"):
        found = split(name)
        if found is None:
            say(f"split {name}: the profiler returned no kernel records")
            continue
        out, other = found
        say(f"split {name:8s} (term.launch, ms per call): " + ", ".join(f"{p} {v:.4f}" for p, v in out.items() if v > 0)
            + (" | not classed: " + ", ".join(f"{k} {v:.4f}" for k, v in sorted(other.items(), key=lambda kv: -kv[1])[:4]) if other else ""))
        terms = B * R * HIDDEN
        for p in ("pair-major pass", "relation-major pass"):
            if out[p] > 0:
                rate = terms / (out[p] * 1e-3)
                say(f"terms {name:8s} {p}: {rate:.3e} pair terms / s (score_all_dist.hip's passes: {DIST_PASSES[0]:.1e} / {DIST_PASSES[1]:.1e})")


if __name__ == "__main__":
    main()
