"""Device time of the filtered top k (mkb_topk) against the filtered rank (mkb_rank) on the same chunk, and of top-10 filtered
prediction for both sides of the FB15k-237 test split against the device-path Evaluation.eval.

    python tools/topk_speed.py [--reps 20] [--out profiles/topk_speed.jsonl]

Both calls run the same all-entity score block; mkb_topk only swaps the last launch (rank_kernel -> topk_kernel), so the
difference of the two is the selection's cost.  HIP-event timing on torch's current stream, median of --reps after two warm-ups.
Tables are the seeded draws of the GPU tests (tests/util_gpu_tables.py); the timing does not depend on the values.
"""
import argparse
import ctypes
import json
import pathlib
import sys
import time

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

from mkb_amd import _hip, datasets, evaluation, models  # noqa: E402
from mkb_amd.utils import true_keys  # noqa: E402
from util_gpu_tables import eval_tables  # noqa: E402


def make(name, ds, hidden):
    ent, rel, modulus = eval_tables(name, n_entity=ds.n_entity, n_relation=ds.n_relation, hidden=hidden, seed=77)
    m = getattr(models, name)(hidden_dim=hidden, entities=ds.entities, relations=ds.relations, gamma=9.0)
    with torch.no_grad():
        m.entity_embedding.copy_(torch.as_tensor(ent))
        m.relation_embedding.copy_(torch.as_tensor(rel))
        if modulus is not None and hasattr(m, "modulus"):
            m.modulus.copy_(torch.as_tensor(modulus))
    return m.to("cuda").eval()


def median_ms(fn, reps):
    for _ in range(2):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def chunk_ab(label, m, ds, B, ks, reps, mode="tail-batch"):
    """mkb_rank vs mkb_topk on one chunk of B test triples."""
    lib, tb = _hip.lib(), m._tables()
    keys = true_keys(ds.true_triples, m.entity_embedding.device, m.n_entity, m.n_relation)[mode]
    test = np.asarray(ds.test, dtype=np.int64)
    s = torch.as_tensor(test[np.random.RandomState(0).choice(len(test), size=B, replace=False)], device="cuda").contiguous()
    need = max(lib.mkb_rank_workspace_bytes(tb, B), lib.mkb_topk_workspace_bytes(tb, B, max(ks)))
    ws = _hip.aligned_bytes(need, "cuda")
    rank = torch.empty(B, dtype=torch.int64, device="cuda")
    mid = _hip.mode_id(mode)

    def run_rank():
        _hip.check(lib.mkb_rank(tb, _hip.ptr(s), B, mid, _hip.ptr(keys), keys.numel(), _hip.ptr(rank), ctypes.c_void_p(ws.data_ptr()),
                                need, _hip.stream_ptr()), "mkb_rank")

    rows = []
    t_rank = median_ms(run_rank, reps)
    for k in ks:
        ids = torch.empty((B, k), dtype=torch.int64, device="cuda")
        sc = torch.empty((B, k), dtype=torch.float32, device="cuda")

        def run_topk():
            _hip.check(lib.mkb_topk(tb, _hip.ptr(s), B, mid, _hip.ptr(keys), keys.numel(), k, _hip.TOPK_KEEP_TARGET, _hip.ptr(ids),
                                    _hip.ptr(sc), ctypes.c_void_p(ws.data_ptr()), need, _hip.stream_ptr()), "mkb_topk")

        t_topk = median_ms(run_topk, reps)
        rows.append({"what": "chunk", "model": label, "mode": mode, "B": B, "n_entity": m.n_entity, "k": k,
                     "mkb_rank_ms": round(t_rank, 4), "mkb_topk_ms": round(t_topk, 4), "topk_over_rank": round(t_topk / t_rank, 4)})
    return rows


def split_prediction(label, m, ds, reps):
    """Top-10 filtered prediction for both sides of the test split vs the device-path Evaluation.eval (wall time, synchronised)."""
    ev = evaluation.Evaluation(true_triples=ds.true_triples, entities=ds.entities, relations=ds.relations, batch_size=1024,
                               device="cuda", num_workers=0)

    def wall(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(max(3, reps // 4)):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts))

    t_eval = wall(lambda: ev.eval(m, ds.test))
    t_topk = wall(lambda: [ev.top_k(m, ds.test, mode, 10) for mode in ("head-batch", "tail-batch")])
    return {"what": "test_split", "model": label, "n_test": len(ds.test), "k": 10, "eval_s": round(t_eval, 4),
            "top10_s": round(t_topk, 4), "top10_over_eval": round(t_topk / t_eval, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    fb = datasets.Fb15k237(batch_size=8, shuffle=False, seed=42, num_workers=0)
    wn = datasets.Wn18rr(batch_size=8, shuffle=False, seed=42, num_workers=0)
    rows = []
    rotate = make("RotatE", fb, 1000)
    rows += chunk_ab("RotatE-1000 FB15k-237", rotate, fb, 1024, (10, 100), a.reps)
    rows += chunk_ab("ComplEx-1000 FB15k-237", make("ComplEx", fb, 1000), fb, 1024, (10, 100), a.reps)
    rows += chunk_ab("RotatE-500 WN18RR", make("RotatE", wn, 500), wn, 1024, (10, 100), a.reps)
    rows.append(split_prediction("RotatE-1000 FB15k-237", rotate, fb, a.reps))
    out = open(a.out, "w") if a.out else None
    for r in rows:
        line = json.dumps(r)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
    if out:
        out.close()


if __name__ == "__main__":
    main()
