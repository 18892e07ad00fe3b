"""Cost of the prior fit report (msl_prior_fit, csrc/priorfit.hip) next to the only route there was before it:
``msl_multibox_match`` per batch of 4 images plus torch counting of ``true_classes > 0`` grouped by ``matched``.

    python tools/bench_prior_fit.py [--reps 20] [--warmup 5] [--out profiles/prior_fit_bench.json]

Input: synthetic ground truth of 64 images x 40 boxes of 2 .. 12 voxels per axis against the priors of a (250,300,300) input
on layers "3 5 7" (P = 208248), one threshold (0.2, from where a prior is a positive under the default band [0.1, 0.2]).
Both routes run in this process on the same card, produce ``pos`` (G, 1, 3) and are compared before anything is timed.
Timing: HIP events around the whole route, --reps calls after --warmup (median and minimum).  Also: a five-factor scale
sweep end to end (``prepare_prior_fit`` once, then ``make_priors`` + ``run_prior_fit`` with its device-to-host copy per
factor; wall clock).  Prints one JSON line and writes it to --out.
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

SIZE, LAYERS, THR = (250, 300, 300), (3, 5, 7), 0.2
N_IMG, PER_IMG, BATCH = 64, 40, 4
FACTORS = (0.5, 0.75, 1.0, 1.5, 2.0)


def make_boxes(seed=0):
    rs = np.random.RandomState(seed)
    size = np.asarray(SIZE, np.float64)
    out = []
    for _ in range(N_IMG):
        ext = rs.randint(2, 13, (PER_IMG, 3))
        lo = (rs.uniform(0, 1, (PER_IMG, 3)) * (size - ext)).round()
        out.append(np.concatenate([lo / size, (lo + ext) / size], 1).astype(np.float32))
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
    from mslesions3d_amd import _lib
    from mslesions3d_amd import utils as U
    from mslesions3d_amd.ssd3d import LSSD3D, MultiBoxLoss
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prior_fit_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_prior_fit needs the HIP device")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    model = LSSD3D(n_classes=2, input_channels=1, input_size=SIZE, threshold=[0.1, THR], aspect_ratios={l: [1.] for l in LAYERS})
    pri, ranges = model.priors_cxcycz, model.prior_ranges()
    P, S = int(pri.shape[0]), len(ranges)
    boxes = make_boxes()
    G = N_IMG * PER_IMG

    # route (ii): one call
    plan = U.prepare_prior_fit(boxes, dev)
    off = U.prior_fit_ranges(ranges, P)
    thr = np.asarray([THR], dtype=np.float32)
    ws_bytes = _lib.load().msl_prior_fit_workspace_bytes(G)
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
    out = torch.empty(G * (3 + S), dtype=torch.int32, device=dev)
    b = out.data_ptr()

    def route_fit():
        _lib.call("msl_prior_fit", plan["gb"].data_ptr(), plan["off"].data_ptr(), N_IMG, G, pri.data_ptr(), P, off.ctypes.data, S,
                  thr.ctypes.data, 1, ws.data_ptr(), ws_bytes, b, b + 4 * G, b + 8 * G, b + 12 * G, st)

    # route (i): the matcher per batch of 4 + torch counting
    scale_of_prior = torch.from_numpy(np.searchsorted(off, np.arange(P), side="right") - 1).to(dev)
    packs = []
    for i in range(0, N_IMG, BATCH):
        bb = [torch.from_numpy(x) for x in boxes[i:i + BATCH]]
        gb, gl, go, T = MultiBoxLoss.pack_targets(bb, [torch.ones(x.shape[0], dtype=torch.int64) for x in bb], dev)
        packs.append((gb, gl, go, T, go[:-1].to(torch.int64)))
    buf = {"overlap": torch.empty((BATCH, P), dtype=torch.float32, device=dev), "obj": torch.empty((BATCH, P), dtype=torch.int32, device=dev),
           "pfo": torch.empty(BATCH * PER_IMG, dtype=torch.int32, device=dev), "tc": torch.empty((BATCH, P), dtype=torch.int64, device=dev),
           "tl": torch.empty((BATCH, P, 6), dtype=torch.float32, device=dev), "matched": torch.empty((BATCH, P), dtype=torch.int64, device=dev)}
    pos_match = torch.zeros((G, S), dtype=torch.int64, device=dev)

    def route_match():
        g0 = 0
        for gb, gl, go, T, first in packs:
            _lib.call("msl_multibox_match", gb.data_ptr(), gl.data_ptr(), go.data_ptr(), T, pri.data_ptr(), BATCH, P, THR, 0.0, 0,
                      buf["overlap"].data_ptr(), buf["obj"].data_ptr(), buf["pfo"].data_ptr(), buf["tc"].data_ptr(),
                      buf["tl"].data_ptr(), buf["matched"].data_ptr(), st)
            idx = (buf["matched"] + first[:, None]) * S + scale_of_prior[None, :]
            pos_match[g0:g0 + T] = torch.bincount(idx[buf["tc"] > 0], minlength=T * S).reshape(T, S)
            g0 += T

    route_fit()
    route_match()
    torch.cuda.synchronize()
    pos_fit = out[3 * G:].reshape(G, S).to(torch.int64)
    same = bool(torch.equal(pos_fit, pos_match))
    res = {"images": N_IMG, "boxes": G, "priors": P, "ranges": {str(k): list(v) for k, v in ranges.items()}, "threshold": THR,
           "tile": _lib.PRIOR_FIT_TILE, "chunk": _lib.PRIOR_FIT_CHUNK, "pos_equal": same,
           "orphaned": int((pos_fit.sum(1) == 0).sum()), "reps": args.reps, "warmup": args.warmup,
           "bytes_written": {"match_route": N_IMG * P * 48 + G * 4, "prior_fit": G * 8 + G * (3 + S) * 4}}
    if not same:
        raise SystemExit(f"the two routes differ: {json.dumps(res)}")
    res["prior_fit"] = timed(route_fit, args.reps, args.warmup)
    res["match_route"] = timed(route_match, args.reps, args.warmup)
    res["speedup_median"] = round(res["match_route"]["median_ms"] / res["prior_fit"]["median_ms"], 2)

    def sweep():
        pl = U.prepare_prior_fit(boxes, dev)
        return [U.run_prior_fit(pl, model.make_priors({f: float(model.scales[f]) * k for f in ranges}), [0.1, THR], ranges) for k in FACTORS]
    sweep()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sweep()
    torch.cuda.synchronize()
    res["sweep_5_factors_s"] = round(time.perf_counter() - t0, 4)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
