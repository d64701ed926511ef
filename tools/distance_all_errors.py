"""Error table of the all-entity losses of the distance models (fused.DistanceAllStep) against the float64 replica, in units of the
float32 error of torch's own evaluation of the same expression: the case table of tests/util_distance_all.py x its three losses.

    python tools/distance_all_errors.py [--out profiles/r26_distance_all_errors.txt]

The largest ratio per quantity, doubled and rounded up, is FACTOR in tests/util_distance_all.py.
"""
import argparse
import math
import sys

import torch

ROOT = __file__.rsplit("/", 2)[0]
sys.path.insert(0, ROOT)
sys.path.insert(0, ROOT + "/tests")
import util_distance_all as U  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/r26_distance_all_errors.txt")
    args = ap.parse_args()
    lines = [f"# all-entity losses of the distance models: device error / yardstick, {torch.cuda.get_device_name(0)}",
             "# yardstick = max(|torch float32 - float64|, %g float32 ulps of the quantity's largest magnitude); settings %s" % (U.FLOOR_ULPS, U.SETTINGS),
             "# gradient buffers pre-filled with +-%g, random row weights; S and dS through mkb_dist_all_score_fwd + the stand-alone loss call" % U.PREFILL,
             "%-40s %-9s " % ("case", "loss") + " ".join("%8s" % q for q in U.QUANTITIES)]
    worst = {q: (0.0, "") for q in U.QUANTITIES}
    for case, name in zip(U.CASES, U.CASE_IDS):
        pb = U.problem(case)
        pre = U.prefill(pb)
        for loss in U.LOSSES:
            f64, yard = U.expected(pb, loss, pre=pre)
            got = U.device_step(pb, loss, pre=pre)
            got.update(U.device_block(pb, loss))
            r = U.ratios(got, f64, yard)
            lines.append("%-40s %-9s " % (name, loss) + " ".join("%8s" % ("%.2f" % r[q] if q in r else "-") for q in U.QUANTITIES))
            print(lines[-1], flush=True)
            for q, v in r.items():
                if v > worst[q][0]:
                    worst[q] = (v, f"{name} {loss}")
    lines.append("# largest ratio per quantity -> FACTOR = ceil(2 x ratio)")
    for q in U.QUANTITIES:
        lines.append("# %-6s %8.2f  -> %d   (%s)" % (q, worst[q][0], max(1, math.ceil(2 * worst[q][0])), worst[q][1]))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-len(U.QUANTITIES) - 1:]))


if __name__ == "__main__":
    main()
