"""Cost of the MR stage (msl_augment_mr, csrc/mraug.hip).

    python tools/bench_mraug.py [--reps 30] [--window 5] [--patches P.json] [--lesionprep L.json] [--step_ms MS]
                                [--out profiles/mraug_bench.json]

(4, C, 128, 128, 128) batches for C = 1 and 2.  Microseconds of one call (its two launches; median, smallest and largest of
--reps windows of --window back-to-back calls between two HIP events, after three warm-up calls):

  all_three : blur, bias and noise drawn for all four samples (sigma 1.5 on every axis: R = 6)
  blur      : blur alone, the same sigmas
  blur_r8   : blur alone at the largest radius (sigma 2.0)
  epilogue  : bias and noise without blur: one read, one write
  copy      : nothing drawn: the copy
Each is reported against the 8 B / voxel floor (one read, one write) at the bandwidth a device-to-device copy of the same
bytes reaches in the same process, and - with --patches / --lesionprep naming files that tools/bench_patches.py and
tools/bench_lesionprep.py wrote ON THE SAME BOX - against the batch-build launch the stage follows; --step_ms (bench.py's
step time on that box) adds the share of a training step.  The output is checked against the host mirror on a small batch
before anything is timed.  Writes one JSON file and prints it as one line.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mslesions3d_amd import _lib  # noqa: E402
from mslesions3d_amd import datasets as DS  # noqa: E402
from mslesions3d_amd.devicedata import MRStage, MRStageRunner, mr_tables  # noqa: E402
from tools.bench_views import windows  # noqa: E402

N, SHAPE = 4, (128, 128, 128)
KW = {"gaussiansmooth": {}, "biasfield": {"degree": 3, "lattice": 9}, "gaussiannoise": {}}


def sample(seed, smooth=None, bias=False, noise=False):
    rs = np.random.RandomState(seed)
    draws = (smooth, rs.uniform(0.0, 0.1, 20) if bias else None, (0.1, 17 + seed, 99) if noise else None)
    return (([0, 1, 2], [0, 0, 0]), [MRStage(n, d, KW[n]) for n, d in zip(DS.MR_NAMES, draws)])


CONFIGS = {"all_three": dict(smooth=(1.5, 1.5, 1.5), bias=True, noise=True), "blur": dict(smooth=(1.5, 1.5, 1.5)),
           "blur_r8": dict(smooth=(2.0, 2.0, 2.0)), "epilogue": dict(bias=True, noise=True), "copy": {}}


def bound_call(stage, src, dst, per_sample, dev):
    """The launch alone, on tables uploaded once: the timed region holds no host work but the ctypes call."""
    rows, taps, lattice = mr_tables(per_sample)
    p, t, l = (torch.from_numpy(a).to(dev) for a in (rows, taps, lattice))
    stream = torch.cuda.current_stream().cuda_stream
    args = (src.data_ptr(), p.data_ptr(), t.data_ptr(), l.data_ptr(), stage.N, stage.C, *stage.shape, lattice.shape[1],
            dst.data_ptr(), stage.ws.data_ptr(), stage.ws.numel(), stream)
    keep = (p, t, l)
    return lambda: (_lib.call("msl_augment_mr", *args), keep)[0]


def check_small(dev):
    rs = np.random.RandomState(0)
    x = rs.randn(2, 2, 9, 20, 70).astype(np.float32)
    per = [sample(1, (2.0, 0.25, 1.1), True, True), sample(2)]
    src, dst = torch.from_numpy(x).to(dev), torch.empty(x.shape, device=dev)
    MRStageRunner(2, 2, x.shape[2:], dev).run(src, per, dst, torch.cuda.current_stream().cuda_stream)
    for n, (_, stages) in enumerate(per):
        want = x[n]
        for st in stages:
            want = DS.apply_mr(st.name, want, st.draw, st.kw)
        assert np.array_equal(dst[n].cpu().numpy(), want), "msl_augment_mr != the host mirror"


def build_launch(path, key_path):
    """One "us" figure out of a bench file written on this box, or None."""
    if not path:
        return None
    node = json.load(open(path))
    for k in key_path:
        node = node[k]
    return float(node["us"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--window", type=int, default=5)
    ap.add_argument("--patches", default=None, help="tools/bench_patches.py's output of this box")
    ap.add_argument("--lesionprep", default=None, help="tools/bench_lesionprep.py's output of this box")
    ap.add_argument("--step_ms", type=float, default=None, help="bench.py's step time on this box (128^3 x 4)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mraug_bench.json"))
    args = ap.parse_args()
    if args.reps < 30:
        ap.error("--reps: at least 30 repetitions")
    dev = torch.device("cuda", 0)
    check_small(dev)
    window_us = build_launch(args.patches, ("configs", "recipe", "msl_augment_window_mc"))
    fit_us = build_launch(args.lesionprep, ("kernels", "msl_augment_fit[recipe_affine_on]"))
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "window": args.window, "batches": {},
           "batch_build_us_same_box": {"msl_augment_window_mc[recipe, 4x1x128^3]": window_us,
                                       "msl_augment_fit[recipe_affine_on, 4x1x250x300x300]": fit_us},
           "step_ms_same_box": args.step_ms}
    for C in (1, 2):
        voxels = N * C * int(np.prod(SHAPE))
        src = torch.randn((N, C) + SHAPE, device=dev)
        dst = torch.empty_like(src)
        stage = MRStageRunner(N, C, SHAPE, dev)
        calls = {name: bound_call(stage, src, dst, [sample(n, **kw) for n in range(N)], dev) for name, kw in CONFIGS.items()}
        calls["d2d_copy"] = lambda: dst.copy_(src)
        passes = [{name: windows(fn, args.reps, args.window) for name, fn in calls.items()} for _ in range(2)]
        best = {name: min((p[name] for p in passes), key=lambda r: r["us"]) for name in calls}
        floor_us = best["d2d_copy"]["us"]  # 8 B / voxel at the bandwidth a copy reaches here
        out = {"voxels": voxels, "floor_bytes": 8 * voxels, "floor_us_at_copy_bandwidth": floor_us,
               "copy_GBps": round(8 * voxels / floor_us / 1e3, 1), "configs": {}}
        for name in CONFIGS:
            r = dict(best[name])
            r["over_floor"] = round(r["us"] / floor_us, 2)
            r["GBps_of_8B_per_voxel"] = round(8 * voxels / r["us"] / 1e3, 1)
            if C == 1 and window_us:
                r["over_window_launch"] = round(r["us"] / window_us, 3)
            if args.step_ms:
                r["share_of_step"] = round(r["us"] / (1000.0 * args.step_ms), 4)
            out["configs"][name] = r
        res["batches"][f"{N}x{C}x128^3"] = out
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
