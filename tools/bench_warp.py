"""Cost of the separable-warp kernel (msl_augment_warp_mc, csrc/datapipe.hip).

    python tools/bench_warp.py [--reps 10] [--window 5] [--out profiles/warp_bench.json]

Four clinical-size one-sequence cases in the arena -> a (4, 1, 250, 300, 300) batch, the centred fit.  Microseconds of one
launch (median, smallest and largest of --reps windows of --window back-to-back calls between two HIP events); the five
configurations are timed in turn, twice over, in the same process, and the better pass of each is kept.

  warp_identity : msl_augment_warp_mc, rows that drew nothing ([7] = 0: the permuted copy)
  fit_identity  : msl_augment_fit_mc on the same rows - the yardstick of the copy path (it writes the same batch: checked)
  warp_zoom     : msl_augment_warp_mc, a zoom drawn for all four samples (the recipe's range 0.9 .. 1.1, "border")
  warp_grid     : msl_augment_warp_mc, a grid distortion drawn for all four (5 cells, limit 0.03, "border")
  fit_affine    : msl_augment_fit_mc, the train_lesions affine drawn for all four (rotation up to pi / 12, scale 0.1,
                  "border"): the same eight-tap gather with a dense coordinate, the yardstick of the warp rows
The output is checked against devicedata.warp_numpy on a small case before anything is timed.  Writes one JSON file and
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
from mslesions3d_amd.devicedata import WarpStage, fit_rows, sample_params, warp_numpy, warp_rows  # noqa: E402
from tools.bench_views import windows  # noqa: E402

CASES = [(230, 280, 260), (200, 260, 300), (250, 300, 300), (260, 310, 290)]
TARGET, N = (250, 300, 300), 4
IDENT = (([0, 1, 2], [0, 0, 0]), [])


class Arena:
    """One-sequence cases of ``shapes`` behind one another; ``call`` binds a launch into (N, 1) + target buffers."""

    def __init__(self, imgs, segs, dev):
        self.dev = dev
        self.img = torch.from_numpy(np.concatenate([v.reshape(-1) for v in imgs])).to(dev)
        self.seg = torch.from_numpy(np.concatenate([v.reshape(-1) for v in segs])).to(dev)
        off = np.concatenate([[0], np.cumsum([v.size for v in segs])])
        self.table = torch.tensor([[int(off[k]), *segs[k].shape] for k in range(len(segs))], dtype=torch.int64, device=dev)

    def call(self, fn, rows, coords, target, dst_img, dst_seg):
        p = torch.from_numpy(np.asarray(rows, dtype=np.float64)).to(self.dev)
        t = torch.from_numpy(np.asarray(coords if len(coords) else np.zeros(1), dtype=np.float64)).to(self.dev)
        stream = torch.cuda.current_stream().cuda_stream
        args = [self.img.data_ptr(), self.seg.data_ptr(), self.seg.numel(), 1, self.table.data_ptr(), self.table.shape[0],
                p.data_ptr()]
        if fn in ("msl_augment_warp_mc", "msl_augment_deform_mc"):  # (the deformation's lattices ride where the tables do)
            args += [t.data_ptr(), t.numel(), None]  # windows null: the centred fit
        keep = (p, t)  # the launch reads them: they live as long as the closure
        return lambda: (_lib.call(fn, *args, len(rows), *target, dst_img.data_ptr(), dst_seg.data_ptr(), stream), keep)[0]


def drawn(augs, shapes, seed):
    """-> per sample (perm, stages) with the list's one resampling stage drawn (prob 1)."""
    augs = [(n, dict(kw, prob=1.0)) for n, kw in augs]
    return [sample_params(DS.draw_augmentations(augs, np.random.RandomState(seed + n)), shapes[n], augs, ragged=True)
            for n in range(len(shapes))]


def check_small(dev):
    rs = np.random.RandomState(0)
    shapes = [(21, 19, 37), (14, 30, 22)]
    imgs = [rs.randn(*s).astype(np.float32) for s in shapes]
    segs = [rs.randint(0, 50, s).astype(np.int16) for s in shapes]
    arena = Arena(imgs, segs, dev)
    target = (24, 28, 40)
    per = [drawn([DS.WARP_AUGMENTATIONS[k]], [shapes[k]], 3)[0] for k in range(2)]
    rows, coords = warp_rows([0, 1], per)
    di = torch.empty((2, 1) + target, device=dev)
    ds = torch.empty((2,) + target, dtype=torch.int16, device=dev)
    arena.call("msl_augment_warp_mc", rows, coords, target, di, ds)()
    for n, (_, stages) in enumerate(per):
        st = next(s for s in stages if isinstance(s, WarpStage))
        want = DS.resize_with_pad_or_crop(warp_numpy(imgs[n], st.tables, 1, st.boundary), target)
        assert np.array_equal(di[n, 0].cpu().numpy(), want), "msl_augment_warp_mc != warp_numpy"
        assert np.array_equal(ds[n].cpu().numpy(), DS.resize_with_pad_or_crop(warp_numpy(segs[n], st.tables, 0, st.boundary), target))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--window", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    check_small(dev)
    rs = np.random.RandomState(1)
    imgs = [rs.randn(*s).astype(np.float32) for s in CASES]
    segs = [((rs.rand(*s) < 0.01) * rs.randint(1, 3000, s)).astype(np.int16) for s in CASES]
    arena = Arena(imgs, segs, dev)
    di = [torch.empty((N, 1) + TARGET, device=dev) for _ in range(2)]
    ds = [torch.empty((N,) + TARGET, dtype=torch.int16, device=dev) for _ in range(2)]
    cases = list(range(N))
    ident = fit_rows(cases, [IDENT] * N)
    zoom = warp_rows(cases, drawn([DS.WARP_AUGMENTATIONS[0]], CASES, 100))
    grid = warp_rows(cases, drawn([DS.WARP_AUGMENTATIONS[1]], CASES, 100))
    affine = fit_rows(cases, drawn([DS.LESIONS_AUGMENTATIONS[0]], CASES, 100))
    assert (zoom[0][:, 7] == 2).all() and (grid[0][:, 7] == 2).all() and (affine[:, 7] == 1).all()
    none = np.zeros(0)
    calls = {"warp_identity": arena.call("msl_augment_warp_mc", ident, none, TARGET, di[0], ds[0]),
             "fit_identity": arena.call("msl_augment_fit_mc", ident, none, TARGET, di[1], ds[1]),
             "warp_zoom": arena.call("msl_augment_warp_mc", *zoom, TARGET, di[0], ds[0]),
             "warp_grid": arena.call("msl_augment_warp_mc", *grid, TARGET, di[0], ds[0]),
             "fit_affine": arena.call("msl_augment_fit_mc", affine, none, TARGET, di[1], ds[1])}
    calls["warp_identity"](), calls["fit_identity"]()
    assert torch.equal(di[0], di[1]) and torch.equal(ds[0], ds[1]), "warp identity rows != msl_augment_fit_mc"
    nbytes = N * int(np.prod(TARGET)) * 6
    passes = [{name: windows(fn, args.reps, args.window) for name, fn in calls.items()} for _ in range(2)]
    best = {name: min((p[name] for p in passes), key=lambda r: r["us"]) for name in calls}
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "window": args.window, "cases": [list(s) for s in CASES],
           "batch": [N, 1, *TARGET], "bytes_written": nbytes, "configs": best,
           "GBps_written": {name: round(nbytes / r["us"] / 1e3, 1) for name, r in best.items()},
           "warp_identity_over_fit_identity": round(best["warp_identity"]["us"] / best["fit_identity"]["us"], 3),
           "warp_zoom_over_fit_affine": round(best["warp_zoom"]["us"] / best["fit_affine"]["us"], 3),
           "warp_grid_over_fit_affine": round(best["warp_grid"]["us"] / best["fit_affine"]["us"], 3)}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
