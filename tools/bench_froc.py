"""Cost of the FROC walk (utils.evaluate_froc, ev_froc_kernel of csrc/evaluate.hip) next to the sweep it follows and to
its numpy twin.

    python tools/bench_froc.py [--reps 30] [--boots 0 100 1000] [--out profiles/froc_bench.json]

One data set: 100 cases x 100 detections, 5 ground-truth boxes each, 2 IoU thresholds, the 7 default rates.  Per number
of bootstrap rows R: the ``msl_evaluate_froc`` enqueue alone, timed with HIP events at steady state (median and minimum
of --reps calls after two warm-ups, each call followed by a synchronise), the preceding ``msl_evaluate_detections`` the
same way, and one wall-clock pass of ``froc_host`` on the same inputs (its matching loop, which the device route does not
repeat, is reported separately).  The device integers are compared with the twin's before anything is timed.  The
weights row is gathered from global memory; staging it in LDS was not tried.  Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

IOUS = [0.1, 0.5]


def make_set(n_img=100, per=100, n_gt=5, seed=0):
    rs = np.random.RandomState(seed)

    def boxes(n):
        lo = rs.uniform(0, 0.8, (n, 3)).astype(np.float32)
        return np.concatenate([lo, lo + rs.uniform(0.02, 0.2, (n, 3)).astype(np.float32)], 1)

    gt = [boxes(n_gt) for _ in range(n_img)]
    det = np.stack([boxes(per) for _ in range(n_img)])
    hits = min(per, 3 * n_gt)
    det[:, :hits] = np.repeat(np.stack(gt), 3, axis=1)[:, :hits] + rs.uniform(-0.03, 0.03, (n_img, hits, 6)).astype(np.float32)
    sc = rs.uniform(0, 1, (n_img, per)).astype(np.float32)
    return (list(det), [np.ones(per, np.int64)] * n_img, list(sc), gt, [np.ones(n_gt, np.int64)] * n_img)


def timed(launch, reps):
    for _ in range(2):
        launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return {"median_ms": round(statistics.median(times), 4), "min_ms": round(min(times), 4)}


def main():
    from mslesions3d_amd import utils as U
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--boots", type=int, nargs="+", default=[0, 100, 1000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "froc_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_froc needs the HIP device")
    torch.cuda.set_device(0)
    data = make_set()
    rates = list(U.DEFAULT_FP_RATES)
    g = [int((l == 1).sum()) for l in data[4]]
    plan = U.prepare_evaluation(*data, IOUS, [0.0])
    out = {"cases": 100, "detections": plan["D"], "gt_boxes": plan["G"], "ious": IOUS, "rates": len(rates), "reps": args.reps,
           "weights_row": "gathered from global memory (LDS staging not measured)",
           "evaluate_detections": timed(plan["launch"], args.reps), "rows": []}
    t0 = time.perf_counter()
    U.froc_host(*data, IOUS, rates, None)
    match_s = time.perf_counter() - t0  # R = 0: nearly all of it is the matching loop of compute_metrics_per_class
    for R in args.boots:
        w = U.bootstrap_weights(100, R, seed=0)
        f = U.prepare_froc(plan, g, w, rates)
        plan["launch"]()
        f["launch"]()
        dev = U.froc_ints(f["out"].cpu().numpy(), f["R1"], f["n_iou"], f["n_rates"], None)
        t0 = time.perf_counter()
        host = U.froc_host(*data, IOUS, rates, w)
        host_s = time.perf_counter() - t0
        same = all(np.array_equal(dev[k], host[k]) for k in ("k", "tp", "gw", "nw"))
        row = {"R": R, "workgroups": (R + 1) * len(IOUS), "device_equals_twin": bool(same), "evaluate_froc": timed(f["launch"], args.reps),
               "froc_host_s": round(host_s, 4), "froc_host_walk_s": round(max(host_s - match_s, 0.0), 4)}
        out["rows"].append(row)
        if not same:
            raise SystemExit(f"device and twin differ at R = {R}: {json.dumps(out)}")
    out["froc_host_matching_s"] = round(match_s, 4)
    text = json.dumps(out)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
