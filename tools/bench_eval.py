"""Cost of the dataset-scale evaluation sweep (utils.evaluate_detections, csrc/evaluate.hip).

    python tools/bench_eval.py [--reps 20] [--sets 600x100 3000x100 4096x1024] [--host-points 1] [--e2e 40]

Per set (images x detections per image, ~5 ground-truth boxes per image, 2 IoU x 10 score thresholds): the device sweep
(one msl_evaluate_detections enqueue) timed with HIP events at steady state (median of --reps back-to-back calls after
two warm-ups), the host packing (one wall-clock pass of prepare_evaluation) and the device-to-host copy of the detail
results.  On the smallest set, one grid point of the host calculate_mAP for comparison.  With --e2e M: an artificial data
set of M subjects (64^3) with 100 predictions each is read back as eval.py does, and the split of the wall clock between
reading (prediction files + volumes for the ground truth) and the sweep is reported.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

IOUS = [0.1, 0.5]
SCORES = [round(0.1 * k, 1) for k in range(10)]


def make_set(n_img, per, seed=0, n_gt=5):
    rs = np.random.RandomState(seed)

    def boxes(n):
        lo = rs.uniform(0, 0.8, (n, 3)).astype(np.float32)
        return np.concatenate([lo, lo + rs.uniform(0.02, 0.2, (n, 3)).astype(np.float32)], 1)

    gt = [boxes(n_gt) for _ in range(n_img)]
    det = np.stack([boxes(per) for _ in range(n_img)])
    hits = min(per, 3 * n_gt)
    det[:, :hits] = np.repeat(np.stack(gt), 3, axis=1)[:, :hits] + rs.uniform(-0.03, 0.03, (n_img, hits, 6)).astype(np.float32)
    sc = rs.uniform(0, 1, (n_img, per)).astype(np.float32)
    return ([torch.from_numpy(d) for d in det], [torch.ones(per, dtype=torch.int64)] * n_img,
            [torch.from_numpy(s) for s in sc], [torch.from_numpy(g) for g in gt], [torch.ones(n_gt, dtype=torch.int64)] * n_img)


def time_set(n_img, per, reps):
    from mslesions3d_amd.utils import prepare_evaluation
    db, dl, ds, gb, gl = make_set(n_img, per)
    t0 = time.perf_counter()
    plan = prepare_evaluation(db, dl, ds, gb, gl, IOUS, SCORES)
    torch.cuda.synchronize()
    pack_ms = (time.perf_counter() - t0) * 1e3
    for _ in range(2):
        plan["launch"]()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        plan["launch"]()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    t0 = time.perf_counter()
    plan["out"].cpu()
    d2h_ms = (time.perf_counter() - t0) * 1e3
    return {"images": n_img, "detections": plan["D"], "gt_boxes": plan["G"], "grid": f"{len(IOUS)}x{len(SCORES)}",
            "device_ms": round(statistics.median(times), 4), "device_ms_min": round(min(times), 4),
            "host_pack_ms": round(pack_ms, 2), "d2h_detail_ms": round(d2h_ms, 2),
            "result_mib": round(plan["out"].numel() * 4 / 2 ** 20, 2)}, (db, dl, ds, gb, gl)


def host_point(data):
    from mslesions3d_amd.utils import calculate_mAP
    db, dl, ds, gb, gl = data
    dif = [torch.zeros(len(l), dtype=torch.bool) for l in gl]
    t0 = time.perf_counter()
    calculate_mAP(db, dl, ds, gb, gl, dif, min_overlap=0.5, return_detail=True)
    return round((time.perf_counter() - t0) * 1e3, 1)


def end_to_end(m):
    """eval.py's flow on an artificial data set, phase by phase."""
    from mslesions3d_amd import datasets as DS
    from mslesions3d_amd import eval as EV
    from mslesions3d_amd.predict import save_predictions
    from mslesions3d_amd.utils import evaluate_detections
    rs = np.random.RandomState(1)
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        DS.generate_artificial_dataset(tmp, "bench", num_images=m, image_size=(64, 64, 64))
        gen_s = time.perf_counter() - t0
        pdir = os.path.join(tmp, "preds")
        os.makedirs(pdir)
        subs = sorted(f[4:8] for f in os.listdir(os.path.join(tmp, "multiple_objects", "one_class", "bench", "images")))
        for s in subs:
            lo = rs.uniform(0, 0.8, (100, 3)).astype(np.float32)
            b = np.concatenate([lo, lo + 0.1], 1)
            save_predictions(s, (64, 64, 64), b, np.ones(100, np.int64), rs.uniform(0, 1, 100).astype(np.float32), 0.0, pdir)
        ds = DS.ExampleDataset(n_classes=1, num_workers=0, data_dir=tmp, dataset_name="bench")
        ds.setup(stage="predict_train")
        loader = ds._loader(ds.predict_dataset, False, EV.BATCH)
        t0 = time.perf_counter()
        det_b, det_l, det_s, gt_b, gt_l = EV.gather_batches(loader, pdir, min(SCORES), log=lambda *_: None)
        read_s = time.perf_counter() - t0
        dif = [torch.zeros(len(l), dtype=torch.bool) for l in gt_l]
        t0 = time.perf_counter()
        evaluate_detections(det_b, det_l, det_s, gt_b, gt_l, dif, min_overlaps=IOUS, min_scores=SCORES, return_detail=True)
        torch.cuda.synchronize()
        sweep_s = time.perf_counter() - t0
    return {"subjects": len(det_b), "generate_s": round(gen_s, 2), "read_files_and_volumes_s": round(read_s, 3),
            "evaluate_detections_s": round(sweep_s, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sets", nargs="+", default=["600x100", "3000x100", "4096x1024"])
    ap.add_argument("--host-points", type=int, default=1, help="host calculate_mAP grid points on the smallest set (0: none)")
    ap.add_argument("--e2e", type=int, default=40, help="subjects of the end-to-end split (0: skip)")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    out = {"ious": IOUS, "scores": SCORES, "sets": []}
    first = None
    for spec in args.sets:
        n_img, per = (int(v) for v in spec.split("x"))
        row, data = time_set(n_img, per, args.reps)
        out["sets"].append(row)
        first = first or data
    if args.host_points:
        out["host_calculate_mAP_ms_per_point"] = [host_point(first) for _ in range(args.host_points)]
        out["host_set"] = args.sets[0]
    if args.e2e:
        out["end_to_end"] = end_to_end(args.e2e)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
