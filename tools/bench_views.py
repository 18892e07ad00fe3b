"""Cost of the multi-view prediction kernels (csrc/views.hip).

    python tools/bench_views.py [--reps 10] [--window 10] [--out profiles/views_bench.json]

1. Gather (stated, fixed): a (1, 230, 280, 260) case -> the 8 views of 192^3 of ``view_plan`` at margin 8.  Microseconds
   of one msl_view_gather (median, smallest and largest of --reps windows of --window back-to-back calls between two HIP
   events), alternating in the same process with a device-to-device copy (``Tensor.copy_``) of a buffer of the gather's
   output size.  Both read and write that many bytes, so the copy is the yardstick: ``ratio_to_copy`` = copy time /
   gather time.  The output is checked against datasets.gather_views on a small case before anything is timed.
2. Merge: msl_views_merge at V = 8 and 64, top_k = 100, both modes, on random detections.
3. Overhead: ``LSSD3D.predict_views`` of the 8 views at view_batch 2 (untrained network, f32) against the same number of
   ``predict_batches`` passes of shape (2, 1, 192, 192, 192) - the baseline bench.py --mode infer times: what gather, the
   copies out of the workspace and the merge add per case, in ms and in forward passes.
Writes one JSON file and prints it as one line.
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
from mslesions3d_amd.datasets import gather_views, view_plan  # noqa: E402
from mslesions3d_amd.utils import merge_views_device, merge_views_workspace  # noqa: E402

CASE, TILE, MARGIN = (1, 230, 280, 260), (192, 192, 192), (8, 8, 8)


def windows(fn, reps, window):
    """Microseconds of one call: [median, min, max] over ``reps`` windows of ``window`` calls between two events."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(window):
            fn()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1000.0 / window)
    return {"us": round(statistics.median(us), 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2)}


def gather_call(case, views, tile, dst):
    stream = torch.cuda.current_stream().cuda_stream
    return lambda: _lib.call("msl_view_gather", case.data_ptr(), case.shape[0], *case.shape[1:], views.ctypes.data,
                             views.shape[0], *tile, dst.data_ptr(), stream)


def bench_gather(reps, window, dev):
    small = np.random.RandomState(0).randn(2, 21, 19, 37).astype(np.float32)
    sv = view_plan(small.shape[1:], (16, 16, 32), (2, 2, 2), flip_axes=(2,))
    out = torch.empty((sv.shape[0], 2, 16, 16, 32), device=dev)
    gather_call(torch.from_numpy(small).to(dev), sv, (16, 16, 32), out)()
    assert np.array_equal(out.cpu().numpy(), gather_views(small, sv, (16, 16, 32))), "msl_view_gather != gather_views"
    case = torch.randn(CASE, device=dev)
    views = view_plan(CASE[1:], TILE, MARGIN)
    dst = torch.empty((views.shape[0], CASE[0]) + TILE, device=dev)
    src_copy = torch.randn(dst.shape, device=dev)
    nbytes = dst.numel() * 4
    res = {"case": list(CASE), "tile": list(TILE), "views": int(views.shape[0]), "bytes_written": nbytes}
    g, c = [], []
    for _ in range(2):  # alternate the two in one process
        g.append(windows(gather_call(case, views, TILE, dst), reps, window))
        c.append(windows(lambda: dst.copy_(src_copy), reps, window))
    best = lambda rs: min(rs, key=lambda r: r["us"])
    res["copy"] = dict(best(c), what="Tensor.copy_ device to device of the same bytes")
    res["msl_view_gather"] = best(g)
    for k in ("copy", "msl_view_gather"):
        res[k]["GBps_written"] = round(nbytes / res[k]["us"] / 1e3, 1)
    res["msl_view_gather"]["ratio_to_copy"] = round(res["copy"]["us"] / res["msl_view_gather"]["us"], 2)
    return res


def bench_merge(reps, window, dev):
    from tests.test_views_cpu import random_detections
    res = {}
    for V in (8, 64):
        top_k = 100
        views = view_plan((200, 200, 64), (64, 64, 64), MARGIN, flip_axes=(0, 1))[:V]
        det = random_detections(np.random.RandomState(V), V, top_k)
        t = [torch.from_numpy(a).to(dev) for a in det]
        ws = merge_views_workspace(V, top_k, dev)
        for mode in ("nms", "fuse"):
            out = merge_views_device(*t, views, (64, 64, 64), (200, 200, 64), MARGIN, 0.5, mode, top_k, workspace=ws)
            fn = lambda: merge_views_device(*t, views, (64, 64, 64), (200, 200, 64), MARGIN, 0.5, mode, top_k, workspace=ws, out=out)
            res[f"V{V}_top_k{top_k}_{mode}"] = dict(windows(fn, reps, window), kept=int(out["count"].item()))
    return res


def bench_overhead(reps, dev):
    import time
    from mslesions3d_amd.ssd3d import LSSD3D
    torch.manual_seed(0)
    model = LSSD3D(n_classes=2, input_channels=1, input_size=TILE).to(dev).eval()
    model.min_score, model.top_k = 0.3, 100
    case = torch.randn(CASE, device=dev)
    views = view_plan(CASE[1:], TILE, MARGIN)
    V, vb = views.shape[0], 2
    batch = {"img": torch.randn((vb, 1) + TILE, device=dev)}

    def passes():
        for _ in model.predict_batches((batch for _ in range(V // vb)), depth=2):
            pass

    def multi():
        model.predict_views(case, views, MARGIN, merge="fuse", view_batch=vb)

    out = {}
    for name, fn in (("predict_batches", passes), ("predict_views", multi)) * 2:
        fn(), fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        out.setdefault(name, []).extend(ms)
    base, mv = statistics.median(out["predict_batches"]), statistics.median(out["predict_views"])
    return {"views": int(V), "view_batch": vb, "passes": V // vb, "predict_batches_ms": round(base, 3),
            "predict_views_ms": round(mv, 3), "added_ms": round(mv - base, 3),
            "added_forward_passes": round((mv - base) / (base / (V // vb)), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--window", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "views_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "window": args.window,
           "gather": bench_gather(args.reps, args.window, dev), "merge": bench_merge(args.reps, args.window, dev),
           "overhead": bench_overhead(args.reps, dev)}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
