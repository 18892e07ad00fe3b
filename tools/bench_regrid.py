"""Cost of msl_regrid (csrc/datapipe.hip) next to a device-to-device copy of the same bytes, and the build time of
devicedata.LesionCache on a tree of cases on their native grid against the same tree regridded on the host beforehand.

    python tools/bench_regrid.py [--reps 10] [--window 10] [--cache-cases 4] [--out profiles/regrid_bench.json]

Kernel (stated, fixed): one case of (176, 240, 256) stored voxels, one f32 image plane and the int16 mask, four plans:
``down`` (0.8 mm isotropic, already LPI: step 1.25), ``up`` (1.2 mm: step 0.8333), ``flip`` (RAS at 1 mm: three
reversals, step 1) - all three with the stored last axis staying last, the kernel's fast path - and ``permuted`` (the
stored axes in another order at 0.9 mm: the last output axis walks the source with a stride).  Microseconds of one call
(median, smallest and largest of --reps windows of --window back-to-back calls between two HIP events), alternating with
a device-to-device copy in the same process.  ``bytes_moved`` = the source read once + the destination written, six
bytes a voxel each; the copy moves the same number (half of it read, half written).  ``ratio_to_copy`` = copy time /
kernel time.  Every output is checked against datasets.regrid before anything is timed.  No pass bar.

Cache (``--cache-cases`` N, 0 to skip): N cases of tools/bench_lesionprep.py's brains in (192, 256, 256) stored volumes
with sidecar affines (mixed spacings and orientations), and the same cases regridded by the host ``datasets.regrid`` and
stored plain; seconds to construct ``LesionCache`` on either tree (files read from disk each time), three alternating
rounds after one warm-up of each, and the host seconds the offline regridding took.  Writes one JSON file and prints it
as one line.
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
from mslesions3d_amd import datasets as DS  # noqa: E402
from mslesions3d_amd.devicedata import LesionCache, plan_row  # noqa: E402
from tools.bench_lesionprep import brain, spread, timed_many  # noqa: E402

NATIVE = (176, 240, 256)
FULL = (192, 256, 256)
CENTERS = ("A_CENTER",)


def affine_of(world, sign, zoom):
    """Stored axis j runs along world axis world[j] with direction sign[j] and spacing zoom[j] mm (RAS+)."""
    a = np.zeros((4, 4), dtype=np.float64)
    for j in range(3):
        a[world[j], j] = sign[j] * zoom[j]
    a[3, 3] = 1.0
    return a


PLANS = {"down": ((0, 1, 2), (-1, -1, -1), (0.8, 0.8, 0.8)), "up": ((0, 1, 2), (-1, -1, -1), (1.2, 1.2, 1.2)),
         "flip": ((0, 1, 2), (1, 1, 1), (1.0, 1.0, 1.0)), "permuted": ((2, 0, 1), (1, -1, 1), (0.9, 0.9, 0.9))}


def bench_kernel(args, dev):
    stream = torch.cuda.current_stream(dev).cuda_stream
    img, seg = brain(NATIVE, 0)
    di, dseg = torch.from_numpy(img).to(dev), torch.from_numpy(seg).to(dev)
    out = {"native_shape": NATIVE, "channels": 1}
    for name, spec in PLANS.items():
        plan = DS.regrid_plan(affine_of(*spec), NATIVE)
        row = plan_row(plan)
        oi = torch.empty(plan.out_shape, dtype=torch.float32, device=dev)
        oseg = torch.empty(plan.out_shape, dtype=torch.int16, device=dev)

        def call():
            _lib.call("msl_regrid", di.data_ptr(), dseg.data_ptr(), 1, *NATIVE, row.ctypes.data, *plan.out_shape,
                      oi.data_ptr(), oseg.data_ptr(), stream)

        call()
        want_i, want_s = DS.regrid(img, seg, plan)
        assert oi.cpu().numpy().tobytes() == want_i.tobytes() and np.array_equal(oseg.cpu().numpy(), want_s), name
        nbytes = 6 * (int(np.prod(NATIVE)) + int(np.prod(plan.out_shape)))
        a = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        b = torch.empty_like(a)
        t = timed_many([call, lambda: b.copy_(a)], args.reps, args.window)
        out[name] = dict(spread(t[0]), ax=plan.ax, rev=[int(r) for r in plan.rev], step=[round(s, 4) for s in plan.step],
                         out_shape=plan.out_shape, fast_path=plan.ax[2] == 2, bytes_moved=nbytes,
                         GBps=round(nbytes / t[0][0] / 1e3, 1), copy=dict(spread(t[1]), GBps=round(nbytes / t[1][0] / 1e3, 1)),
                         ratio_to_copy=round(t[1][0] / t[0][0], 3))
        del a, b, oi, oseg
    return out


def bench_cache(args, dev):
    specs = [((0, 1, 2), (1, 1, 1), (1.0, 1.0, 1.0)), ((0, 1, 2), (-1, 1, -1), (0.9, 0.9, 1.1)),
             ((0, 1, 2), (1, -1, 1), (1.2, 1.2, 0.8)), ((1, 0, 2), (1, 1, -1), (1.0, 1.0, 1.25))]
    with tempfile.TemporaryDirectory() as tmp:
        dirs = {k: os.path.join(tmp, k, "raw") for k in ("native", "regridded")}
        probe = DS.LesionsDataModule.__new__(DS.LesionsDataModule)
        probe.registration, probe.skullstripped = "T2star", True
        host_s = 0.0
        for k in range(args.cache_cases):
            core, cseg = brain((160 + 4 * k, 200, 176), k)
            img, seg = np.zeros(FULL, np.float32), np.zeros(FULL, np.int16)
            sl = tuple(slice((f - c) // 2, (f - c) // 2 + c) for f, c in zip(FULL, core.shape))
            img[sl], seg[sl] = core, cseg
            affine = affine_of(*specs[k % len(specs)])
            t0 = time.perf_counter()
            ri, rseg = DS.regrid(img, seg, DS.regrid_plan(affine, FULL))
            host_s += time.perf_counter() - t0
            for key, (a, b, aff) in (("native", (img, seg, affine)), ("regridded", (ri, rseg, None))):
                probe.data_dir = dirs[key]
                os.makedirs(os.path.join(probe._get_data_dir(CENTERS[0]), f"sub-{k:03d}"), exist_ok=True)
                for name, arr in (("FLAIR", a), ("labeled_lesions", b)):
                    path = probe._get_sequence(CENTERS[0], f"{k:03d}", name)
                    os.makedirs(os.path.dirname(path), exist_ok=True)
                    np.save(path + ".npy", np.ascontiguousarray(arr))
                    if aff is not None:
                        np.save(path + ".affine.npy", aff)

        def build(key):
            dm = DS.LesionsDataModule(data_dir=dirs[key], centers=CENTERS, batch_size=2, spatial_size=(250, 300, 300))
            dm.setup("fit")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cache = LesionCache(dm, dev)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            return dt, cache

        _, ca = build("native")
        _, cb = build("regridded")
        assert ca.full_shapes == cb.full_shapes and torch.equal(ca.img, cb.img) and torch.equal(ca.seg, cb.seg)
        del ca, cb
        times = {"native": [], "regridded": []}
        for _ in range(3):
            for key in times:
                times[key].append(round(build(key)[0], 3))
    return {"cases": args.cache_cases, "stored_shape": FULL, "specs": [list(map(list, s)) for s in specs[:args.cache_cases]],
            "native_tree_s": times["native"], "regridded_tree_s": times["regridded"],
            "native_tree_median_s": statistics.median(times["native"]),
            "regridded_tree_median_s": statistics.median(times["regridded"]),
            "host_regrid_of_the_tree_s": round(host_s, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--window", type=int, default=10)
    ap.add_argument("--cache-cases", type=int, default=4)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "regrid_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_regrid.py measures on the GPU: no device found")
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "window": args.window, "kernel": bench_kernel(args, dev)}
    if args.cache_cases > 0:
        out["cache_build"] = bench_cache(args, dev)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
