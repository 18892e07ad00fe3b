"""Cost of the free-form deformation kernel (msl_augment_deform_mc, csrc/datapipe.hip), on the
protocol of tools/bench_warp.py.

    python tools/bench_deform.py [--reps 10] [--window 5] [--out profiles/deform_bench.json]

Four clinical-size one-sequence cases in the arena -> a (4, 1, 250, 300, 300) batch, the centred fit.  Microseconds of one
launch (median, smallest and largest of --reps windows of --window back-to-back calls between two HIP events); the five
configurations are timed in turn, twice over, in the same process, and the better pass of each is kept.

  deform_identity : msl_augment_deform_mc, rows that drew nothing ([7] = 0: the permuted copy)
  fit_identity    : msl_augment_fit_mc on the same rows - the yardstick of the copy path (it writes the same batch: checked)
  deform_elastic  : msl_augment_deform_mc, an elastic3d drawn for all four samples (the recipe's 7^3 lattice, "border")
  warp_zoom       : msl_augment_warp_mc, a zoom drawn for all four (the recipe's range 0.9 .. 1.1, "border"): the same
                    eight-tap gather behind a table read
  fit_affine      : msl_augment_fit_mc, the train_lesions affine drawn for all four: the same gather behind a dense matrix
The output is checked against devicedata.deform_numpy on a small case before anything is timed.  Writes one JSON file and
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

from mslesions3d_amd import datasets as DS  # noqa: E402
from mslesions3d_amd.devicedata import DeformStage, deform_numpy, deform_rows, fit_rows, warp_rows  # noqa: E402
from tools.bench_views import windows  # noqa: E402
from tools.bench_warp import CASES, IDENT, N, TARGET, Arena, drawn  # noqa: E402


def check_small(dev):
    rs = np.random.RandomState(0)
    shapes = [(21, 19, 37), (14, 30, 22)]
    imgs = [rs.randn(*s).astype(np.float32) for s in shapes]
    segs = [rs.randint(0, 50, s).astype(np.int16) for s in shapes]
    arena = Arena(imgs, segs, dev)
    target = (24, 28, 40)
    per = [drawn(DS.DEFORM_AUGMENTATIONS, [shapes[k]], 3)[0] for k in range(2)]
    rows, lattices = deform_rows([0, 1], per)
    di = torch.empty((2, 1) + target, device=dev)
    ds = torch.empty((2,) + target, dtype=torch.int16, device=dev)
    arena.call("msl_augment_deform_mc", rows, lattices, target, di, ds)()
    for n, (_, stages) in enumerate(per):
        st = next(s for s in stages if isinstance(s, DeformStage))
        want = DS.resize_with_pad_or_crop(deform_numpy(imgs[n], st.lattice, 1, st.boundary), target)
        assert np.array_equal(di[n, 0].cpu().numpy(), want), "msl_augment_deform_mc != deform_numpy"
        assert np.array_equal(ds[n].cpu().numpy(), DS.resize_with_pad_or_crop(deform_numpy(segs[n], st.lattice, 0, st.boundary), target))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--window", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deform_bench.json"))
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
    elastic = deform_rows(cases, drawn(DS.DEFORM_AUGMENTATIONS, CASES, 100))
    zoom = warp_rows(cases, drawn([DS.WARP_AUGMENTATIONS[0]], CASES, 100))
    affine = fit_rows(cases, drawn([DS.LESIONS_AUGMENTATIONS[0]], CASES, 100))
    assert (elastic[0][:, 7] == 3).all() and (elastic[0][:, 9] == 7).all() and (zoom[0][:, 7] == 2).all() and (affine[:, 7] == 1).all()
    none = np.zeros(0)
    calls = {"deform_identity": arena.call("msl_augment_deform_mc", ident, none, TARGET, di[0], ds[0]),
             "fit_identity": arena.call("msl_augment_fit_mc", ident, none, TARGET, di[1], ds[1]),
             "deform_elastic": arena.call("msl_augment_deform_mc", *elastic, TARGET, di[0], ds[0]),
             "warp_zoom": arena.call("msl_augment_warp_mc", *zoom, TARGET, di[0], ds[0]),
             "fit_affine": arena.call("msl_augment_fit_mc", affine, none, TARGET, di[1], ds[1])}
    calls["deform_identity"](), calls["fit_identity"]()
    assert torch.equal(di[0], di[1]) and torch.equal(ds[0], ds[1]), "deform identity rows != msl_augment_fit_mc"
    nbytes = N * int(np.prod(TARGET)) * 6
    passes = [{name: windows(fn, args.reps, args.window) for name, fn in calls.items()} for _ in range(2)]
    best = {name: min((p[name] for p in passes), key=lambda r: r["us"]) for name in calls}
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "window": args.window, "cases": [list(s) for s in CASES],
           "batch": [N, 1, *TARGET], "bytes_written": nbytes, "control_points": 7, "configs": best,
           "both_passes_us": {name: [p[name]["us"] for p in passes] for name in calls},
           "GBps_written": {name: round(nbytes / r["us"] / 1e3, 1) for name, r in best.items()},
           "deform_identity_over_fit_identity": round(best["deform_identity"]["us"] / best["fit_identity"]["us"], 3),
           "deform_elastic_over_warp_zoom": round(best["deform_elastic"]["us"] / best["warp_zoom"]["us"], 3),
           "deform_elastic_over_fit_affine": round(best["deform_elastic"]["us"] / best["fit_affine"]["us"], 3)}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
