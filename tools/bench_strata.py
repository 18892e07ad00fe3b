"""Cost of the size-stratified counts (utils.evaluate_strata, ev_stratify_kernel + ev_strata_count_kernel of
csrc/evaluate.hip) next to the sweep and the FROC walk they follow and to the numpy twin.

    python tools/bench_strata.py [--reps 30] [--boots 0 100 1000] [--out profiles/strata_bench.json]

One data set: 100 cases x 100 detections, 5 ground-truth boxes each, 2 IoU thresholds, 4 size bins (3 edges), 10 score
cuts + the 7 default FROC rates = 17 cuts.  Per number of bootstrap rows R: the ``msl_evaluate_strata`` enqueue alone (both
launches), timed with HIP events at steady state (median and minimum of --reps calls after two warm-ups, each call
followed by a synchronise), ``msl_evaluate_froc`` and the preceding ``msl_evaluate_detections`` the same way in the same
run, and one wall-clock pass of ``strata_host`` on the same inputs at the same cuts (its matching loop, which the device
route does not repeat, is reported separately).  The device integers are compared with the twin's before anything is
timed.  Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.bench_froc import IOUS, make_set, timed  # noqa: E402

EDGES = [27.0, 125.0, 1000.0]
SCORES = [round(0.05 + 0.1 * i, 2) for i in range(10)]
VOXELS = 64.0 ** 3


def main():
    from mslesions3d_amd import utils as U
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--boots", type=int, nargs="+", default=[0, 100, 1000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "strata_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_strata needs the HIP device")
    torch.cuda.set_device(0)
    data = make_set()
    rates = list(U.DEFAULT_FP_RATES)
    g = [int((l == 1).sum()) for l in data[4]]
    plan = U.prepare_evaluation(*data, IOUS, SCORES)
    out = {"cases": 100, "detections": plan["D"], "gt_boxes": plan["G"], "ious": IOUS, "bins": len(EDGES) + 1,
           "cuts": len(SCORES) + len(rates), "reps": args.reps, "evaluate_detections": timed(plan["launch"], args.reps), "rows": []}
    t0 = time.perf_counter()
    U.strata_host(*data, VOXELS, EDGES, IOUS, None, [0])
    match_s = time.perf_counter() - t0  # R = 0, one cut: nearly all of it is the matching loop and the claim ranks
    for R in args.boots:
        w = U.bootstrap_weights(100, R, seed=0)
        f = U.prepare_froc(plan, g, w, rates)
        plan["launch"]()
        f["launch"]()
        n_iou, n_sc = len(IOUS), len(SCORES)
        kc = plan["out"][:n_iou * n_sc * U.METRIC_SUMMARY].reshape(n_iou, n_sc, U.METRIC_SUMMARY)[:, :, 6].to(torch.int64)
        k = f["out"][:(R + 1) * n_iou * len(rates) * 2].reshape(R + 1, n_iou, len(rates), 2)[..., 0]
        cuts = torch.cat([kc[None].expand(R + 1, n_iou, n_sc), k], dim=2).contiguous()
        s = U.prepare_strata(plan, VOXELS, EDGES, w, cuts)
        s["launch"]()
        host_cuts = cuts.cpu().numpy()
        dev = U.strata_ints(s["out"].cpu().numpy(), s["R1"], s["n_iou"], s["n_cuts"], s["S1"], host_cuts)
        t0 = time.perf_counter()
        host = U.strata_host(*data, VOXELS, EDGES, IOUS, w, host_cuts)
        host_s = time.perf_counter() - t0
        same = all(np.array_equal(dev[key], host[key]) for key in ("tp", "fp", "gw", "det_unbinned", "nw", "cuts"))
        row = {"R": R, "workgroups": (R + 1) * len(IOUS), "device_equals_twin": bool(same),
               "evaluate_strata": timed(s["launch"], args.reps), "evaluate_froc": timed(f["launch"], args.reps),
               "strata_host_s": round(host_s, 4), "strata_host_walk_s": round(max(host_s - match_s, 0.0), 4)}
        out["rows"].append(row)
        if not same:
            raise SystemExit(f"device and twin differ at R = {R}: {json.dumps(out)}")
    out["strata_host_matching_s"] = round(match_s, 4)
    text = json.dumps(out)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
