"""Cost of the patch-training window kernel (msl_augment_window_mc, csrc/datapipe.hip).

    python tools/bench_patches.py [--reps 10] [--window 10] [--out profiles/patches_bench.json]

One (1, 230, 280, 260) case in the arena -> a (4, 1, 128, 128, 128) batch.  Microseconds of one launch (median, smallest
and largest of --reps windows of --window back-to-back calls between two HIP events), every configuration alternating in
the same process with msl_augment_fit_mc on the same rows at the same output shape.  That call is the yardstick: it is
the fit's voxel-by-voxel body, which this kernel shares, and it writes the same bytes.

  identity_fit_origins : identity rows, the windows at the fit's own shifts - the two launches write the same batch
                         (checked), so the difference is the interior load path alone (the shift of the last axis is 66:
                         rows start 8 bytes off a 16-byte boundary, four 4-byte loads per thread)
  identity_aligned     : identity rows, four interior windows whose last-axis origin is a multiple of four: one 16-byte
                         load per thread and plane
  identity_odd         : the same windows moved by one voxel along the last axis
  recipe               : the train_lesions recipe (flip, three rot90s, rotating affine "border", shift / scale intensity;
                         the affine drawn for all four samples), windows from datasets.patch_origin
The output is checked against datasets.window on a small case before anything is timed.  Writes one JSON file and
prints it as one line.
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
from mslesions3d_amd.devicedata import fit_rows, sample_params  # noqa: E402
from tools.bench_views import windows  # noqa: E402

CASE, PATCH, N = (230, 280, 260), (128, 128, 128), 4
IDENT = (([0, 1, 2], [0, 0, 0]), [])


class Arena:
    def __init__(self, img, seg, dev):
        self.img, self.seg = torch.from_numpy(img.reshape(-1)).to(dev), torch.from_numpy(seg.reshape(-1)).to(dev)
        self.table = torch.tensor([[0, *seg.shape]], dtype=torch.int64, device=dev)
        self.C = img.size // seg.size

    def call(self, fn, rows, origins, patch, dst_img, dst_seg):
        p = torch.from_numpy(np.asarray(rows, dtype=np.float64)).to(self.img.device)
        w = torch.from_numpy(np.asarray(origins, dtype=np.int32)).to(self.img.device)
        stream = torch.cuda.current_stream().cuda_stream
        args = [self.img.data_ptr(), self.seg.data_ptr(), self.seg.numel(), self.C, self.table.data_ptr(), 1, p.data_ptr()]
        if fn == "msl_augment_window_mc":
            args.append(w.data_ptr())
        keep = (p, w)  # the launch reads them: they live as long as the closure
        return lambda: (_lib.call(fn, *args, len(rows), *patch, dst_img.data_ptr(), dst_seg.data_ptr(), stream), keep)[0]


def check_small(dev):
    rs = np.random.RandomState(0)
    img, seg = rs.randn(2, 21, 19, 37).astype(np.float32), rs.randint(0, 50, (21, 19, 37)).astype(np.int16)
    arena = Arena(img, seg, dev)
    patch, origins = (12, 16, 20), [(-3, 2, 5), (4, 1, 8), (10, 6, 20)]
    di = torch.empty((3, 2) + patch, device=dev)
    ds = torch.empty((3,) + patch, dtype=torch.int16, device=dev)
    arena.call("msl_augment_window_mc", fit_rows([0] * 3, [IDENT] * 3), origins, patch, di, ds)()
    for n, o in enumerate(origins):
        assert np.array_equal(di[n].cpu().numpy(), DS.window(img, o, patch)), "msl_augment_window_mc != datasets.window"
        assert np.array_equal(ds[n].cpu().numpy(), DS.window(seg, o, patch))


def recipe_rows():
    augs = DS.select_augmentations(["flip", "rotate90", "affine", "shiftintensity", "scaleintensity"])
    augs = [(n, dict(kw, prob=1.0) if n == "affine" else kw) for n, kw in augs]
    per_sample, origins = [], []
    for n in range(N):
        rs = np.random.RandomState(100 + n)
        perm, stages = sample_params(DS.draw_augmentations(augs, rs), CASE, augs, ragged=True)
        per_sample.append((perm, stages))
        origins.append(DS.patch_origin(rs, tuple(CASE[a] for a in perm[0]), PATCH, np.zeros((0, 3)), 0.0))
    return fit_rows([0] * N, per_sample), origins


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--window", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "patches_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    check_small(dev)
    rs = np.random.RandomState(1)
    img = rs.randn(*CASE).astype(np.float32)
    seg = ((rs.rand(*CASE) < 0.01) * rs.randint(1, 3000, CASE)).astype(np.int16)
    arena = Arena(img, seg, dev)
    di = [torch.empty((N, 1) + PATCH, device=dev) for _ in range(2)]
    ds = [torch.empty((N,) + PATCH, dtype=torch.int16, device=dev) for _ in range(2)]
    ident = fit_rows([0] * N, [IDENT] * N)
    fit = [DS.fit_shift(n, t) for n, t in zip(CASE, PATCH)]
    aligned = [(10, 20, 64), (90, 30, 8), (40, 150, 128), (100, 100, 40)]
    configs = {"identity_fit_origins": (ident, [fit] * N), "identity_aligned": (ident, aligned),
               "identity_odd": (ident, [(a, b, c + 1) for a, b, c in aligned]), "recipe": recipe_rows()}
    nbytes = N * int(np.prod(PATCH)) * 6
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "window": args.window, "case": [1, *CASE],
           "batch": [N, 1, *PATCH], "bytes_written": nbytes, "configs": {}}
    for name, (rows, origins) in configs.items():
        win = arena.call("msl_augment_window_mc", rows, origins, PATCH, di[0], ds[0])
        ref = arena.call("msl_augment_fit_mc", rows, origins, PATCH, di[1], ds[1])
        win(), ref()
        if name == "identity_fit_origins":
            assert torch.equal(di[0], di[1]) and torch.equal(ds[0], ds[1]), "window at the fit's shifts != fit"
        w, f = [], []
        for _ in range(2):  # alternate the two in one process
            w.append(windows(win, args.reps, args.window))
            f.append(windows(ref, args.reps, args.window))
        best = lambda rs_: min(rs_, key=lambda r: r["us"])
        w, f = best(w), best(f)
        res["configs"][name] = {"origins": [list(map(int, o)) for o in origins], "msl_augment_window_mc": w,
                                "msl_augment_fit_mc": f, "window_over_fit": round(w["us"] / f["us"], 3),
                                "GBps_written": round(nbytes / w["us"] / 1e3, 1)}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
