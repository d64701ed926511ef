"""Error table of the relation-prediction term (losses.RelationPrediction, mkb_rel_step / mkb_rel_score_bwd) against the float64
replica, in units of err_ref, the float32 error of torch's own evaluation of the same expression: the case table of
tests/util_relation_prediction.py.

    python tools/relation_prediction_errors.py [--out profiles/r28_relation_prediction_errors.txt]

The device is held to ERR_FACTOR = 8 x err_ref; a (case, quantity) above 8 would go into MEASURED_RATIO there, with its cause.
"""
import argparse
import sys

import torch

ROOT = __file__.rsplit("/", 2)[0]
sys.path.insert(0, ROOT)
sys.path.insert(0, ROOT + "/tests")
import util_relation_prediction as U  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/r28_relation_prediction_errors.txt")
    args = ap.parse_args()
    lines = [f"# relation-prediction term: device error / err_ref, {torch.cuda.get_device_name(0)}",
             "# err_ref = max(|torch float32 - float64|, %g float32 ulps of the quantity's largest magnitude); T = %g, lambda = %g, N = %d entities"
             % (U.FLOOR_ULPS, U.T, U.LAMBDA, U.N),
             "# launch: term.launch (mkb_rel_step), random row weights, gradient buffers pre-filled with +-%g; S and dS: model.score_relations and"
             % U.PREFILL,
             "# lambda x the seeds of mkb_all_softmax on it; bwd: score_relations(sample).backward(random block), the largest of its three gradients",
             "%-26s " % "case" + " ".join("%8s" % q for q in U.QUANTITIES) + " %8s" % "bwd"]
    worst = {q: (0.0, "") for q in U.QUANTITIES + ("bwd",)}
    for case, name in zip(U.CASES, U.CASE_IDS):
        pb = U.problem(case)
        pre = U.prefill(pb)
        f64, yard = U.expected(pb, pre=pre)
        got = U.device_launch(pb, pre=pre)
        block = U.device_block(pb)
        got.update(S=block["S"], dS=block["dS"])
        r = U.ratios(got, f64, yard)
        dblock = U.seed_block(pb)
        b64, byard = U.expected(pb, dblock=dblock)
        m = U.device_model(pb)
        m.score_relations(torch.as_tensor(pb.sample).cuda()).backward(torch.as_tensor(dblock).cuda())
        torch.cuda.synchronize()
        r["bwd"] = max(U.ratios(U.grads_of(m, pb), b64, byard).values())
        lines.append("%-26s " % name + " ".join("%8s" % ("%.2f" % r[q] if q in r else "-") for q in U.QUANTITIES + ("bwd",)))
        print(lines[-1], flush=True)
        for q, v in r.items():
            if v > worst[q][0]:
                worst[q] = (v, name)
    lines.append("# largest ratio per quantity (the bound is %g)" % U.ERR_FACTOR)
    for q in U.QUANTITIES + ("bwd",):
        lines.append("# %-6s %8.2f   (%s)" % (q, worst[q][0], worst[q][1]))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-len(U.QUANTITIES) - 2:]))


if __name__ == "__main__":
    main()
