"""Cost of the three kernels behind devicedata.LesionCache (csrc/datapipe.hip) next to a device-to-device copy.

    python tools/bench_lesionprep.py [--reps 10] [--window 10] [--out profiles/lesionprep_bench.json]
    python tools/bench_lesionprep.py --channels 2 [--out profiles/lesionprep_mc_bench.json]

Case mix (stated, fixed): four cropped brains of (170, 205, 165), (185, 220, 180), (160, 200, 170) and (176, 208, 176)
voxels - ellipsoids of positive intensities, 40 instance-labelled lesions of 2 .. 9 voxels a side each - fitted to
spatial_size (250, 300, 300) at batch 4; the foreground box runs on the first brain embedded in a (192, 256, 256) volume.

Per kernel: microseconds of one call (median over --reps windows of --window back-to-back calls between two HIP events),
the bytes it must move (compulsory reads + writes), and the same figures for a device-to-device copy that moves the same
number of bytes (half read, half written), timed in the same process, windows alternating.  ``ratio_to_copy`` =
copy time / kernel time: 1.0 means the kernel moves its bytes as fast as the copy does.  Writes one JSON file and prints
it as one line.

``--channels C`` (C > 1) measures the multi-sequence entry points instead, same shapes and method: per row (identity,
recipe as drawn, affine drawn for all four) msl_augment_fit_mc on C-plane cases, C launches of msl_augment_fit on the
separate planes (each also rewrites the mask) and the device copy of the fused launch's bytes, windows of the three
alternating; and msl_foreground_box_mc on the (C, 192, 256, 256) volume.  Every figure carries the smallest and largest
window (``us_min`` / ``us_max``) so that two medians can be told apart from the spread.  The fused output is checked
bit for bit against the separate launches before anything is timed.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mslesions3d_amd import _lib  # noqa: E402
from mslesions3d_amd import datasets as DS  # noqa: E402
from mslesions3d_amd.devicedata import _InstBoxOut, fit_rows, sample_params  # noqa: E402

CASES = [(170, 205, 165), (185, 220, 180), (160, 200, 170), (176, 208, 176)]
TARGET = (250, 300, 300)
FULL = (192, 256, 256)
RECIPE = ["flip", "rotate90", "affine", "shiftintensity", "scaleintensity"]


def brain(shape, seed):
    rs = np.random.RandomState(seed)
    g = np.meshgrid(*(np.linspace(-1, 1, n) for n in shape), indexing="ij")
    inside = (g[0] ** 2 + g[1] ** 2 + g[2] ** 2) <= 1.0
    img = np.where(inside, rs.rand(*shape).astype(np.float32) * 100 + 1, 0).astype(np.float32)
    seg = np.zeros(shape, np.int16)
    for k in range(40):
        size = rs.randint(2, 10, 3)
        at = [int(rs.randint(n // 4, 3 * n // 4 - s)) for n, s in zip(shape, size)]
        seg[tuple(slice(a, a + s) for a, s in zip(at, size))] = k + 1
    return img, seg


def timed(fn, copy_fn, reps, window):
    """-> (median us of fn, median us of copy_fn), windows of each alternating."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = ([], [])
    for r in range(reps + 2):
        for k, f in enumerate((fn, copy_fn)):
            e0.record()
            for _ in range(window):
                f()
            e1.record()
            e1.synchronize()
            if r >= 2:  # two warm-up rounds
                out[k].append(e0.elapsed_time(e1) * 1e3 / window)
    return statistics.median(out[0]), statistics.median(out[1])


def timed_many(fns, reps, window):
    """-> per function (median, min, max) us of one call; windows of the functions alternating."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = [[] for _ in fns]
    for r in range(reps + 2):
        for k, f in enumerate(fns):
            e0.record()
            for _ in range(window):
                f()
            e1.record()
            e1.synchronize()
            if r >= 2:  # two warm-up rounds
                out[k].append(e0.elapsed_time(e1) * 1e3 / window)
    return [(statistics.median(o), min(o), max(o)) for o in out]


def spread(t):
    return {"us": round(t[0], 2), "us_min": round(t[1], 2), "us_max": round(t[2], 2)}


def main_mc(args):
    """The C-channel entry points next to C one-channel launches and the copy (module docstring)."""
    C = args.channels
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    cases = [brain(s, k) for k, s in enumerate(CASES)]
    rs = np.random.RandomState(7)
    # channel c of a case: the brain on another scale and with another texture (the mask is shared)
    planes = [[np.where(img > 0, img * (c + 1) + rs.rand(*img.shape).astype(np.float32) * c, 0).astype(np.float32)
               for c in range(C)] for img, _ in cases]
    sizes = [int(np.prod(s)) for s in CASES]
    off = np.concatenate([[0], np.cumsum(sizes)])
    a_mc = torch.from_numpy(np.concatenate([p.reshape(-1) for case in planes for p in case])).to(dev)
    a_one = [torch.from_numpy(np.concatenate([case[c].reshape(-1) for case in planes])).to(dev) for c in range(C)]
    a_seg = torch.from_numpy(np.concatenate([c[1].reshape(-1) for c in cases])).to(dev)
    table = torch.tensor([[int(off[k]), *CASES[k]] for k in range(4)], dtype=torch.int64, device=dev)
    N, V = 4, int(np.prod(TARGET))
    d_mc = torch.empty((N, C) + TARGET, dtype=torch.float32, device=dev)
    d_one = [torch.empty((N,) + TARGET, dtype=torch.float32, device=dev) for _ in range(C)]
    d_seg = torch.empty((N,) + TARGET, dtype=torch.int16, device=dev)
    d_seg1 = torch.empty((N,) + TARGET, dtype=torch.int16, device=dev)
    scratch = torch.empty(2 * N * V * (4 * C + 2), dtype=torch.uint8, device=dev)

    def copy_of(nbytes):
        h = int(nbytes) // 2
        src, dst = scratch[:h], scratch[scratch.numel() // 2:scratch.numel() // 2 + h]
        return lambda: dst.copy_(src)

    res = {"channels": C, "case_shapes": CASES, "spatial_size": TARGET, "batch": N, "reps": args.reps,
           "window": args.window, "device": torch.cuda.get_device_name(dev),
           "copy": "device-to-device copy moving the fused launch's bytes (half read, half written), same process",
           "separate": f"{C} launches of msl_augment_fit, one per plane arena (each rewrites the mask)", "kernels": {}}

    full = np.zeros((C,) + FULL, np.float32)
    for c in range(C):  # the second channel's support is shifted: the union is larger than either
        full[c, 11 + 3 * c:11 + 3 * c + CASES[0][0], 25:25 + CASES[0][1], 40 - 5 * c:40 - 5 * c + CASES[0][2]] = planes[0][c]
    vol = torch.from_numpy(full).to(dev)
    box = torch.zeros(6, dtype=torch.int32, device=dev)
    nbytes = vol.numel() * 4
    t = timed_many([lambda: _lib.call("msl_foreground_box_mc", vol.data_ptr(), C, *FULL, 5, box.data_ptr(), stream),
                    copy_of(nbytes)], args.reps, args.window)
    lo, hi = DS.foreground_box(full, 5)
    assert box.cpu().tolist() == list(lo) + list(hi)
    res["kernels"]["msl_foreground_box_mc"] = dict(spread(t[0]), bytes_moved=int(nbytes), copy=spread(t[1]),
                                                   GBps=round(nbytes / t[0][0] / 1e3, 1), shape=(C,) + FULL)

    src_bytes = int(off[-1]) * (4 * C + 2)
    for tag, names, prob in (("identity", [], None), ("recipe_as_drawn", RECIPE, None), ("recipe_affine_on", RECIPE, 1.0)):
        augs = DS.select_augmentations(names)
        if prob is not None:
            augs = [(n, dict(kw, prob=prob)) for n, kw in augs]
        per = [sample_params(DS.draw_augmentations(augs, np.random.RandomState(n)), CASES[n], augs, ragged=True)
               for n in range(N)]
        rows = torch.from_numpy(fit_rows(list(range(N)), per)).to(dev)

        def fused():
            _lib.call("msl_augment_fit_mc", a_mc.data_ptr(), a_seg.data_ptr(), a_seg.numel(), C, table.data_ptr(), 4,
                      rows.data_ptr(), N, *TARGET, d_mc.data_ptr(), d_seg.data_ptr(), stream)

        def separate():
            for c in range(C):
                _lib.call("msl_augment_fit", a_one[c].data_ptr(), a_seg.data_ptr(), a_seg.numel(), table.data_ptr(), 4,
                          rows.data_ptr(), N, *TARGET, d_one[c].data_ptr(), d_seg1.data_ptr(), stream)

        fused()
        separate()
        torch.cuda.synchronize()
        assert torch.equal(d_seg, d_seg1)
        for c in range(C):
            assert torch.equal(d_mc[:, c].contiguous().view(torch.int32), d_one[c].view(torch.int32)), (tag, c)
        nbytes = src_bytes + N * V * (4 * C + 2)
        t = timed_many([fused, separate, copy_of(nbytes)], args.reps, args.window)
        res["kernels"][f"msl_augment_fit_mc[{tag}]"] = dict(
            spread(t[0]), bytes_moved=int(nbytes), GBps=round(nbytes / t[0][0] / 1e3, 1), separate=spread(t[1]),
            copy=spread(t[2]), fused_over_separate=round(t[0][0] / t[1][0], 3), ratio_to_copy=round(t[2][0] / t[0][0], 3),
            affine_rows=int(sum(r[7] for r in rows.cpu().numpy())))
    out = args.out or os.path.join(ROOT, "profiles", "lesionprep_mc_bench.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def entry(us, copy_us, nbytes):
    return {"us": round(us, 2), "bytes_moved": int(nbytes), "GBps": round(nbytes / us / 1e3, 1),
            "copy_us": round(copy_us, 2), "copy_GBps": round(nbytes / copy_us / 1e3, 1),
            "ratio_to_copy": round(copy_us / us, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--window", type=int, default=10)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--channels", type=int, default=1, help="sequences per case; > 1 measures the _mc entry points")
    args = ap.parse_args()
    if not 1 <= args.channels <= 4:
        ap.error("--channels must be 1 .. 4")
    if args.channels > 1:
        return main_mc(args)
    args.out = args.out or os.path.join(ROOT, "profiles", "lesionprep_bench.json")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    cases = [brain(s, k) for k, s in enumerate(CASES)]
    off = np.concatenate([[0], np.cumsum([int(np.prod(s)) for s in CASES])])
    a_img = torch.from_numpy(np.concatenate([c[0].reshape(-1) for c in cases])).to(dev)
    a_seg = torch.from_numpy(np.concatenate([c[1].reshape(-1) for c in cases])).to(dev)
    table = torch.tensor([[int(off[k]), *CASES[k]] for k in range(4)], dtype=torch.int64, device=dev)
    N, V = 4, int(np.prod(TARGET))
    d_img = torch.empty((N,) + TARGET, dtype=torch.float32, device=dev)
    d_seg = torch.empty((N,) + TARGET, dtype=torch.int16, device=dev)
    scratch = torch.empty(2 * N * V * 6, dtype=torch.uint8, device=dev)  # source and destination of the copies

    def copy_of(nbytes):
        h = int(nbytes) // 2
        src, dst = scratch[:h], scratch[scratch.numel() // 2:scratch.numel() // 2 + h]
        return lambda: dst.copy_(src)

    res = {"case_shapes": CASES, "spatial_size": TARGET, "batch": N, "reps": args.reps, "window": args.window,
           "copy": "device-to-device copy moving the same bytes (half read, half written), same process",
           "device": torch.cuda.get_device_name(dev), "kernels": {}}

    # msl_foreground_box: reads the volume once
    full = np.zeros(FULL, np.float32)
    full[11:11 + CASES[0][0], 25:25 + CASES[0][1], 40:40 + CASES[0][2]] = cases[0][0]
    vol = torch.from_numpy(full).to(dev)
    box = torch.zeros(6, dtype=torch.int32, device=dev)
    us, cus = timed(lambda: _lib.call("msl_foreground_box", vol.data_ptr(), *FULL, 5, box.data_ptr(), stream),
                    copy_of(vol.numel() * 4), args.reps, args.window)
    lo, hi = DS.foreground_box(full, 5)
    assert box.cpu().tolist() == list(lo) + list(hi)
    res["kernels"]["msl_foreground_box"] = dict(entry(us, cus, vol.numel() * 4), shape=FULL)

    # msl_augment_fit: reads each source voxel about once (6 B), writes 6 B per output voxel
    src_bytes = int(off[-1]) * 6
    for tag, names, prob in (("identity", [], None), ("recipe_as_drawn", RECIPE, None), ("recipe_affine_on", RECIPE, 1.0)):
        augs = DS.select_augmentations(names)
        if prob is not None:
            augs = [(n, dict(kw, prob=prob)) for n, kw in augs]
        per = [sample_params(DS.draw_augmentations(augs, np.random.RandomState(n)), CASES[n], augs, ragged=True)
               for n in range(N)]
        rows = torch.from_numpy(fit_rows(list(range(N)), per)).to(dev)
        nbytes = src_bytes + N * V * 6
        us, cus = timed(lambda: _lib.call("msl_augment_fit", a_img.data_ptr(), a_seg.data_ptr(), a_img.numel(),
                                          table.data_ptr(), 4, rows.data_ptr(), N, *TARGET, d_img.data_ptr(),
                                          d_seg.data_ptr(), stream), copy_of(nbytes), args.reps, args.window)
        res["kernels"][f"msl_augment_fit[{tag}]"] = dict(entry(us, cus, nbytes),
                                                         affine_rows=int(sum(r[7] for r in rows.cpu().numpy())))

    # msl_instance_boxes: reads the int16 batch once (on the identity batch built last: the fitted masks)
    ident = [(([0, 1, 2], [0, 0, 0]), [])] * N
    rows = torch.from_numpy(fit_rows(list(range(N)), ident)).to(dev)
    _lib.call("msl_augment_fit", a_img.data_ptr(), a_seg.data_ptr(), a_img.numel(), table.data_ptr(), 4, rows.data_ptr(), N,
              *TARGET, d_img.data_ptr(), d_seg.data_ptr(), stream)
    out = _InstBoxOut(N, TARGET, [(1, np.inf)], 64 * N, dev)
    nbytes = N * V * 2 + out.ws.numel()
    us, cus = timed(lambda: out.launch(d_seg, stream), copy_of(nbytes), args.reps, args.window)
    torch.cuda.synchronize()
    n_boxes = int(out.obj_off.cpu()[-1])
    assert int(out.flag.item()) == 0 and n_boxes > 0
    res["kernels"]["msl_instance_boxes"] = dict(entry(us, cus, nbytes), boxes=n_boxes,
                                                workspace_bytes=int(out.ws.numel()))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
