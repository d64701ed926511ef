"""Forward + backward time of the candidate lists ``Distillation.distill`` scores, ``BaseModel.score_candidates`` (the slot
kernels) against the block route (``model(block)`` on the written-out ``[n, m, 3]`` block: the general kernels in default mode),
and of ``distill`` as a whole, for the five models as students (HIP events, one MI355X):

  - tables of FB15k-237's size (14,541 entities, 237 relations), hidden 1000, B = 1024;
  - (M_entity, M_relation) = (20, 10) and (100, 50);
  - shared lists (one draw for the whole batch with the row's own id in the last slot: what ``UniformSampling`` gives) and
    per-row lists (independent draws);
  - every figure: the best of 5 measurements of ``--reps`` calls each after a warm call, the two routes alternating, with the
    spread (max - min) of the 5.

    python tools/distill_speed.py [--reps 10] [--out FILE]

A (model, part) cell keeps the slot kernels only where they are ahead of the block route by more than the block route's own
spread in all four configurations; the table's last block lists the cells, which is what ``Distillation.SLOT_KERNEL_ROUTES`` holds.
The per-part figures take the block as given (building it is charged to ``distill`` as a whole only).  The tables are random
(eval_tables): the cost does not depend on the values."""
import argparse
import pathlib
import sys

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

MODELS = ("TransE", "RotatE", "ComplEx", "DistMult", "pRotatE")
PARTS = ("head", "relation", "tail")
SIZES = ((20, 10), (100, 50))
N, R, HIDDEN, B = 14541, 237, 1000, 1024


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def alternate(fns, reps, rounds=5):
    """-> per function (best, spread) in ms over ``rounds`` measurements, taken in turn so that a drift hits every route alike."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    runs = [[] for _ in fns]
    for _ in range(rounds):
        for out, fn in zip(runs, fns):
            out.append(timed(fn, reps))
    return [(min(r), max(r) - min(r)) for r in runs]


class RowwiseSampling:
    """Independent candidates for every row (with repeats), no ground truth in the lists; ids are shared one to one."""
    supervised = False
    depends_on_teacher = False

    def __init__(self, batch_size_entity, batch_size_relation, seed):
        self.me, self.mr, self.g = batch_size_entity, batch_size_relation, torch.Generator().manual_seed(seed)

    def get(self, positive_sample_size, **kwargs):
        e = lambda: torch.randint(N, (positive_sample_size, self.me), generator=self.g)
        h, r, t = e(), torch.randint(R, (positive_sample_size, self.mr), generator=self.g), e()
        return h, r, t, h, r, t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/distill_speed.py measures on a ROCm device: none found")
    from util_gpu import make_model
    from util_gpu_tables import eval_tables
    from mkb_amd import distillation

    rs = np.random.RandomState(0)
    sample = torch.as_tensor(np.stack([rs.randint(N, size=B), rs.randint(R, size=B), rs.randint(N, size=B)], 1)).cuda()
    ids = {i: i for i in range(N)}
    rels = {i: i for i in range(R)}
    shipped = dict(distillation.Distillation.SLOT_KERNEL_ROUTES)
    every = {name: PARTS for name in MODELS}
    lines = [f"tables {N} x {R}, hidden {HIDDEN}, B = {B}; ms, best of 5 x {args.reps} calls (spread = max - min of the 5); forward + backward",
             "", f"{'model':9s}{'part':9s}{'M':>4s} {'lists':8s}{'block':>8s}{'(spread)':>9s}{'slot':>8s}{'(spread)':>9s}  ahead by more than the block route's spread"]
    ahead = {}
    whole = []
    for name in MODELS:
        ent, rel, mod = eval_tables(name, seed=77)
        student = make_model(name, ent, rel, HIDDEN, 9.0, mod)
        ent, rel, mod = eval_tables(name, seed=78)
        teacher = make_model(name, ent, rel, HIDDEN, 9.0, mod).eval()
        for me, mr in SIZES:
            for kind in ("shared", "per-row"):
                for part in PARTS:
                    n_table, m, col = (R, mr, 1) if part == "relation" else (N, me, 0 if part == "head" else 2)
                    if kind == "shared":
                        cand = torch.as_tensor(rs.choice(n_table, m, replace=False)).view(1, m).repeat(B, 1).cuda()
                        cand[:, -1] = sample[:, col]
                    else:
                        cand = torch.as_tensor(rs.randint(n_table, size=(B, m))).cuda()
                    block = sample.unsqueeze(1).repeat(1, m, 1)
                    block[:, :, col] = cand
                    w = torch.as_tensor(rs.randn(B, m).astype(np.float32)).cuda()
                    with torch.no_grad():
                        same = student(block).cpu().numpy().tobytes() == student.score_candidates(sample, cand, part).cpu().numpy().tobytes()
                    if not same:
                        raise SystemExit(f"{name} {part}: the two routes' scores differ")
                    (old, old_sp), (new, new_sp) = alternate([lambda: student(block).backward(w),
                                                             lambda: student.score_candidates(sample, cand, part).backward(w)], args.reps)
                    wins = new < old - old_sp
                    ahead[(name, part)] = ahead.get((name, part), True) and wins
                    lines.append(f"{name:9s}{part:9s}{m:4d} {kind:8s}{old:8.3f}{old_sp:9.3f}{new:8.3f}{new_sp:9.3f}  {'yes' if wins else 'no'}")
                    student.zero_grad(set_to_none=True)
                sampling = (distillation.UniformSampling(me, mr, seed=1) if kind == "shared" else RowwiseSampling(me, mr, seed=1))
                proc = distillation.Distillation(ids, ids, rels, rels, sampling=sampling)

                def distill_with(routes):
                    def fn():
                        distillation.Distillation.SLOT_KERNEL_ROUTES = routes
                        proc.distill(teacher=teacher, student=student, sample=sample).backward()
                    return fn
                res = alternate([distill_with({}), distill_with(every), distill_with(shipped)], max(2, args.reps // 2))
                distillation.Distillation.SLOT_KERNEL_ROUTES = shipped
                whole.append(f"{name:9s}({me:3d},{mr:3d}) {kind:8s}" + "".join(f"{b:9.3f}{s:9.3f}" for b, s in res))
                student.zero_grad(set_to_none=True)
        del student, teacher
    lines += ["", "Distillation.distill as a whole (teacher of the student's class under no_grad, student forward + backward, the sampler's",
              "host work and the KL kernels included), every part on the block route / on the slot kernels / routed as shipped:", "",
              f"{'student':9s}{'(Me, Mr)':10s}{'lists':8s}{'block':>9s}{'(spread)':>9s}{'slot':>9s}{'(spread)':>9s}{'shipped':>9s}{'(spread)':>9s}"] + whole
    lines += ["", "cells that keep the slot kernels (ahead in all four configurations); every other cell stays on the block route:"]
    for name in MODELS:
        lines.append(f"{name:9s}" + (", ".join(p for p in PARTS if ahead[(name, p)]) or "-"))
    lines += ["", "shipped (Distillation.SLOT_KERNEL_ROUTES when this ran):"]
    for name in MODELS:
        lines.append(f"{name:9s}" + (", ".join(shipped.get(name, ())) or "-"))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
