"""Cost of msl_draw_boxes (csrc/overlay.hip) next to a device fill of the same bytes, and the wall time of the two
clinical predict routes (host-prepared cases against devicedata.LesionPredictFeed).

    python tools/bench_overlay.py [--reps 10] [--window 10] [--predict-cases 4] [--out profiles/overlay_bench.json]

Kernel (stated, fixed): one image of (250, 300, 300), K = 100 boxes of 6 .. 14 voxels a side, both planes: 90 MB
written, nothing read but the boxes.  Microseconds of one call (median, smallest and largest of --reps windows of --window
back-to-back calls between two HIP events) for both styles, alternating with a device fill (``Tensor.fill_``) of one
int16 buffer of the two planes' size in the same process.  The kernel only writes, so the fill is its yardstick:
``ratio_to_fill`` = fill time / kernel time.  The output is checked against utils.draw_boxes before anything is timed.

Predict routes (``--predict-cases`` N, 0 to skip): N synthetic cases of tools/bench_lesionprep.py's brains embedded in
(192, 256, 256) volumes, written as a LesionsDataModule tree, predicted by ``predict -dm lesions -ps train`` at
spatial_size (250, 300, 300) with an untrained checkpoint: wall seconds of ``--cache 0`` and ``--cache 1`` in three
alternating rounds after one warm-up run of each, same process.  Writes one JSON file and prints it as one line.
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

from mslesions3d_amd import _lib  # noqa: E402
from mslesions3d_amd.utils import DRAW_STYLES, draw_boxes  # noqa: E402
from tools.bench_lesionprep import CASES, FULL, TARGET, brain, spread, timed_many  # noqa: E402

K = 100


def detections(shape, k, seed=0):
    rs = np.random.RandomState(seed)
    size = rs.randint(6, 15, (k, 3))
    lo = np.stack([rs.randint(0, n - 14, k) for n in shape], 1)
    boxes = (np.concatenate([lo, lo + size], 1) / np.asarray(shape * 2, np.float64)).astype(np.float32)
    return boxes, rs.randint(1, 3, k).astype(np.int64), rs.uniform(0.5, 1.0, k).astype(np.float32)


def bench_kernel(args, dev):
    stream = torch.cuda.current_stream(dev).cuda_stream
    V = int(np.prod(TARGET))
    b, l, s = detections(TARGET, K)
    db, dl, ds = (torch.from_numpy(a).to(dev) for a in (b, l, s))
    off = np.asarray([0, K], np.int32)
    inst = torch.empty((1,) + TARGET, dtype=torch.int16, device=dev)
    cls = torch.empty((1,) + TARGET, dtype=torch.int16, device=dev)
    filled = torch.empty(2 * V, dtype=torch.int16, device=dev)

    def draw(style):
        return lambda: _lib.call("msl_draw_boxes", db.data_ptr(), dl.data_ptr(), ds.data_ptr(), off.ctypes.data, 1, *TARGET,
                                 DRAW_STYLES[style], 0.5, inst.data_ptr(), cls.data_ptr(), stream)

    for style in DRAW_STYLES:
        inst.fill_(-1)
        cls.fill_(-1)
        draw(style)()
        want = draw_boxes(b, l, s, TARGET, style, 0.5)
        assert np.array_equal(inst[0].cpu().numpy(), want[0]) and np.array_equal(cls[0].cpu().numpy(), want[1]), style
    t = timed_many([draw("edges"), draw("preds"), lambda: filled.fill_(7)], args.reps, args.window)
    nbytes = 4 * V
    out = {"shape": TARGET, "boxes": K, "box_voxels": "6 .. 14 a side", "planes": 2, "bytes_written": nbytes,
           "fill": dict(spread(t[2]), GBps=round(nbytes / t[2][0] / 1e3, 1), what="Tensor.fill_ of one int16 buffer of the same bytes")}
    for k, style in enumerate(("edges", "preds")):
        out[f"msl_draw_boxes[{style}]"] = dict(spread(t[k]), GBps=round(nbytes / t[k][0] / 1e3, 1),
                                               ratio_to_fill=round(t[2][0] / t[k][0], 3))
    return out


def bench_predict(args, dev):
    from mslesions3d_amd import predict as P
    from mslesions3d_amd.datasets import LesionsDataModule
    from mslesions3d_amd.ssd3d import LSSD3D
    root = tempfile.mkdtemp(prefix="overlay_bench_")
    data_dir = os.path.join(root, "raw")
    probe = LesionsDataModule.__new__(LesionsDataModule)
    probe.data_dir, probe.registration, probe.skullstripped = data_dir, "T2star", True
    for k in range(args.predict_cases):
        img, seg = brain(CASES[k % len(CASES)], k)
        full_img, full_seg = np.zeros(FULL, np.float32), np.zeros(FULL, np.int16)
        sl = tuple(slice(a, a + n) for a, n in zip((3, 12, 20), img.shape))
        full_img[sl], full_seg[sl] = img, seg
        os.makedirs(os.path.join(probe._get_data_dir("CENTER"), f"sub-{k:03d}"), exist_ok=True)
        for name, arr in (("FLAIR", full_img), ("labeled_lesions", full_seg)):
            path = probe._get_sequence("CENTER", f"{k:03d}", name) + ".npy"
            os.makedirs(os.path.dirname(path), exist_ok=True)
            np.save(path, arr)
    model = LSSD3D(n_classes=2, input_channels=1, input_size=TARGET, threshold=[0.1, 0.2], lr=1e-3).to(dev)
    ckpt = os.path.join(root, "untrained.ckpt")
    model.save_checkpoint(ckpt)
    del model

    def run(cache, tag):
        a = P.build_parser().parse_args(["-dm", "lesions", "-d", data_dir, "--centers", "CENTER", "-m", ckpt, "-ps", "train",
                                         "-o", os.path.join(root, tag), "-sc", "0.01", "--cache", str(cache), "-si", "1"])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        P.predict_example(a)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    times = {0: [], 1: []}
    for r in range(4):  # round 0 warms both routes up (programs recorded, files cached)
        for cache in (0, 1):
            t = run(cache, f"c{cache}_{r}")
            if r:
                times[cache].append(round(t, 3))
    n = len([f for f in os.listdir(os.path.join(root, "c1_1")) if f.endswith("_preds.npy")])
    return {"cases_in_tree": args.predict_cases, "subjects_predicted": n, "case_shape": FULL, "spatial_size": TARGET,
            "flags": "-dm lesions -ps train -si 1 -sc 0.01", "rounds": 3,
            "host_route_s": times[0], "device_route_s": times[1],
            "host_route_median_s": statistics.median(times[0]), "device_route_median_s": statistics.median(times[1])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--window", type=int, default=10)
    ap.add_argument("--predict-cases", type=int, default=4)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "overlay_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(dev), "reps": args.reps, "window": args.window, "kernel": bench_kernel(args, dev)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:  # (the kernel figures are on disk before the longer predict runs start)
        json.dump(res, f, indent=1)
    if args.predict_cases > 0:
        res["predict_routes"] = bench_predict(args, dev)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
