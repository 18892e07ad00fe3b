"""Cost of msl_binary_boxes (csrc/datapipe.hip, boxes from binary lesion masks) next to the routes that existed before it:

    python tools/bench_binary_boxes.py [--shape 250 300 300] [-N 2] [--reps 20] [--warmup 5] [--out FILE.json]

Input: N int16 masks of --shape with about 40 ellipsoidal lesions of 2 .. 12 voxels per axis each (seeded).  Routes, all in
this process on the same card, each compared with the host's boxes before anything is timed:

  msl_binary_boxes    the run-based labelling, default run_cap (262144 runs per image)
  msl_seg_boxes       the union-find over a link per voxel of the synthetic data set's route, on a uint8 copy of the mask
                      with one class (the copy is not timed): the same components
  msl_instance_boxes  on the scipy-labelled mask: no labelling at all, the floor of one dense read
  host                scipy.ndimage.label plus the host walk (datasets.boxes_from_instances, "binary"), wall clock

Timing: HIP events around the call, --reps calls after --warmup (median and minimum).  Prints one JSON line and writes it
to --out when given.
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

LESIONS_PER_IMAGE = 40


def make_masks(N, shape, seed=0):
    rs = np.random.RandomState(seed)
    out = np.zeros((N,) + tuple(shape), np.int16)
    for n in range(N):
        for _ in range(LESIONS_PER_IMAGE):
            ext = rs.randint(2, 13, 3)
            lo = [int(rs.randint(0, s - e + 1)) for s, e in zip(shape, ext)]
            g = np.meshgrid(*[(np.arange(e) - (e - 1) / 2) / (e / 2) for e in ext], indexing="ij")
            ball = (g[0] ** 2 + g[1] ** 2 + g[2] ** 2) <= 1.0
            view = out[n][tuple(slice(a, a + e) for a, e in zip(lo, ext))]
            view[ball] = 1
    return out


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4)}


def main():
    from scipy.ndimage import label

    from mslesions3d_amd import datasets as DS
    from mslesions3d_amd.devicedata import MAX_RUNS_PER_IMAGE, _BinBoxOut, _BoxOut, _InstBoxOut, _default_comp_cap
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[250, 300, 300])
    ap.add_argument("-N", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    N, shape = args.N, tuple(args.shape)
    masks = make_masks(N, shape)
    t0 = time.perf_counter()
    host = [DS.boxes_from_instances(m, [(1, np.inf)], "binary") for m in masks]
    host_ms = (time.perf_counter() - t0) * 1e3
    capacity = 1024 * N
    stream = torch.cuda.current_stream().cuda_stream
    seg16 = torch.from_numpy(masks).to(dev)
    seg8 = torch.from_numpy(masks.astype(np.uint8)).to(dev)
    lab16 = torch.from_numpy(np.stack([label(m)[0] for m in masks]).astype(np.int16)).to(dev)
    m = masks != 0
    runs = int(m[..., 0].sum() + (m[..., 1:] & ~m[..., :-1]).sum())
    routes = {"msl_binary_boxes": (_BinBoxOut(N, shape, capacity, dev), seg16),
              "msl_seg_boxes": (_BoxOut(N, shape, 1, capacity, _default_comp_cap(capacity), dev), seg8),
              "msl_instance_boxes": (_InstBoxOut(N, shape, [(1, np.inf)], capacity, dev), lab16)}
    res = {"shape": list(shape), "N": N, "lesions_per_image": LESIONS_PER_IMAGE, "foreground_voxels": int(m.sum()),
           "runs": runs, "boxes": int(sum(len(l) for _, l in host)), "run_cap": MAX_RUNS_PER_IMAGE * N, "routes": {}}
    for name, (out, seg) in routes.items():
        out.launch(seg, stream)
        off = out.obj_off.cpu().tolist()
        out.raise_on_overflow(out.flag.item())
        for n in range(N):  # the routes agree with the host before they are timed
            got = out.gb[off[n]:off[n + 1]].cpu().numpy()
            assert got.tobytes() == host[n][0].numpy().tobytes(), (name, n)
        res["routes"][name] = dict(timed(lambda: out.launch(seg, stream), args.reps, args.warmup),
                                   workspace_bytes=int(out.ws.numel()))
    res["routes"]["host_scipy_label_and_walk"] = {"wall_ms": round(host_ms, 1)}
    b, s = res["routes"]["msl_binary_boxes"], res["routes"]["msl_seg_boxes"]
    res["binary_not_above_seg_boxes"] = bool(b["median_ms"] <= s["median_ms"])
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
