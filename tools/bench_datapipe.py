"""Cost of the device data pipeline (devicedata.DeviceCache, csrc/datapipe.hip) against the host pipeline it replaces.

    python tools/bench_datapipe.py [--reps 20] [--host-reps 2] [--epoch-cases 16] [--skip-epoch]
                                   [--augment example|train_lesions] [--stages]

Per configuration (64^3 x 8 and 128^3 x 4, without augmentation and with ``flip rotate90 translate scale``): one device
batch (gather + resample stages + connected components -> packed boxes) timed with HIP events at steady state (median
of --reps batches after two warm-ups; every augmentation draw of the batch on the host included, since it is enqueued
in the same interval), and one host batch (``ExampleDataset.train_dataloader()``, num_workers 0: load, normalise,
augment with scipy, label, collate; wall clock, median of --host-reps batches).  Then the whole-run wall time of
``train.py`` on a generated toy64 data set, ``-c 0`` against ``-c 1`` (2 epochs, batch 2, each in a fresh process).
Prints one JSON line.

``--augment train_lesions`` runs the same with ``flip rotate90 affine shiftintensity scaleintensity`` (the rotating
affine and the intensity pair of the clinical recipe).  ``--stages`` adds a "stages" entry: the time of ONE resample
launch at 128^3 x 4 and 64^3 x 8, msl_augment_resample on a drawn diagonal matrix next to msl_augment_affine on a drawn
rotating matrix (+-15 degrees, the recipe's ranges), on the same diagonal matrix, and as an intensity-only permuted
copy; each figure is the median over --reps windows of 50 back-to-back launches between two HIP events, the entry
points alternating window by window in one process.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mslesions3d_amd import datasets as DS  # noqa: E402
from mslesions3d_amd.devicedata import DeviceCache  # noqa: E402

AUG = ["flip", "rotate90", "translate", "scale"]
AUG_SETS = {"example": AUG, "train_lesions": ["flip", "rotate90", "affine", "shiftintensity", "scaleintensity"]}
STAGE_WINDOW = 50  # launches per timed window


def bench_stages(size, batch, reps, dev):
    """Median microseconds of one launch per entry point / parameter kind, on the same random source volumes."""
    import numpy as np

    from mslesions3d_amd import _lib
    from mslesions3d_amd.devicedata import (OP_ADD, OP_MUL, PARAM_STRIDE, IntensityOp, affine_row, sample_params)
    shape = (size,) * 3
    g = torch.Generator().manual_seed(0)
    img = torch.randn((batch,) + shape, generator=g).to(dev)
    seg = (torch.rand((batch,) + shape, generator=g) < 0.3).to(torch.uint8).to(dev)
    oi, os_ = torch.empty_like(img), torch.empty_like(seg)
    scale = [("affine", dict(DS.select_augmentations(["scale"])[0][1], prob=1.0))]
    rot = [("affine", dict(DS.select_augmentations(["affine"])[0][1], prob=1.0))]
    ops = [IntensityOp(OP_ADD, np.float32(0.05)), IntensityOp(OP_MUL, np.float32(1.03))]
    rows = {"resample_diagonal": [], "affine_rotating": [], "affine_diagonal": [], "affine_intensity_only": []}
    for n in range(batch):
        _, (diag,) = sample_params(DS.draw_augmentations(scale, np.random.RandomState(n)), shape, scale)
        _, (dense,) = sample_params(DS.draw_augmentations(rot, np.random.RandomState(n)), shape, rot)
        r = np.zeros(PARAM_STRIDE)
        r[0], r[1:4], r[7], r[8:11], r[11:14] = n, (0, 1, 2), 1.0, diag[0], diag[1]
        rows["resample_diagonal"].append(r)
        rows["affine_rotating"].append(affine_row(n, stage=dense))
        rows["affine_diagonal"].append(affine_row(n, stage=diag))
        rows["affine_intensity_only"].append(affine_row(n, ops=ops))
    par = {k: torch.from_numpy(np.stack(v)).to(dev) for k, v in rows.items()}
    stream = torch.cuda.current_stream(dev).cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {k: [] for k in rows}
    for rep in range(reps + 2):  # two warm-up rounds
        for k in rows:
            fn = "msl_augment_resample" if k.startswith("resample") else "msl_augment_affine"
            e0.record()
            for _ in range(STAGE_WINDOW):
                _lib.call(fn, img.data_ptr(), seg.data_ptr(), batch, par[k].data_ptr(), batch, *shape, oi.data_ptr(),
                          os_.data_ptr(), stream)
            e1.record()
            e1.synchronize()
            if rep >= 2:
                times[k].append(e0.elapsed_time(e1) * 1e3 / STAGE_WINDOW)
    out = {"size": size, "batch": batch, "window": STAGE_WINDOW, "reps": reps}
    for k, v in times.items():
        out[k + "_us"] = round(statistics.median(v), 2)
        out[k + "_us_min_max"] = [round(min(v), 2), round(max(v), 2)]
    # bytes one stage has to move: image + mask read once and written once
    out["min_bytes"] = batch * size ** 3 * 10
    return out


def bench_config(root, size, batch, augment, reps, host_reps, dev):
    ds = DS.ExampleDataset(data_dir=root, dataset_name=f"b{size}", batch_size=batch,
                           augmentations=DS.select_augmentations(augment))
    ds.setup("fit")
    cache = DeviceCache(ds, dev)
    times, epoch = [], 0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    while len(times) < reps + 2:
        it = cache.train_batches(epoch)
        while True:
            e0.record()
            b = next(it, None)
            if b is None:
                break
            e1.record()
            e1.synchronize()
            if b["img"].shape[0] == batch:
                times.append(e0.elapsed_time(e1))
        epoch += 1
    dev_ms = statistics.median(times[2:])
    host = []
    it = iter(ds.train_dataloader())
    for _ in range(host_reps):
        t0 = time.perf_counter()
        next(it)
        host.append((time.perf_counter() - t0) * 1e3)
    return {"size": size, "batch": batch, "augment": augment, "device_ms": round(dev_ms, 4),
            "host_ms": round(statistics.median(host), 2), "cache": cache.footprint()}


def bench_epoch(cases, aug=AUG):
    with tempfile.TemporaryDirectory() as tmp:
        DS.generate_artificial_dataset(tmp, "toy64", num_images=cases, image_size=(64, 64, 64))
        out = {}
        for c in (0, 1):
            cmd = [sys.executable, "-m", "mslesions3d_amd.train", "-d", tmp, "-dn", "toy64", "-b", "2", "-me", "2",
                   "-ld", os.path.join(tmp, "logs"), "-en", f"c{c}", "-c", str(c), "-a", *aug]
            t0 = time.perf_counter()
            subprocess.run(cmd, cwd=ROOT, check=True, capture_output=True, timeout=900)
            out[f"c{c}_s"] = round(time.perf_counter() - t0, 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--epoch-cases", type=int, default=16)
    ap.add_argument("--skip-epoch", action="store_true")
    ap.add_argument("--augment", choices=sorted(AUG_SETS), default="example")
    ap.add_argument("--stages", action="store_true")
    args = ap.parse_args()
    aug = AUG_SETS[args.augment]
    dev = torch.device("cuda", 0)
    res = {"configs": []}
    with tempfile.TemporaryDirectory() as tmp:
        for size, batch in ((64, 8), (128, 4)):
            DS.generate_artificial_dataset(tmp, f"b{size}", num_images=2 * batch + batch // 2 + 1,
                                           image_size=(size,) * 3)
            root = os.path.join(tmp)
            for augment in ([], aug):
                res["configs"].append(bench_config(root, size, batch, augment, args.reps, args.host_reps, dev))
                print(json.dumps(res["configs"][-1]), file=sys.stderr, flush=True)
    if not args.skip_epoch:
        res["train_py_2_epochs"] = dict(bench_epoch(args.epoch_cases, aug), cases=args.epoch_cases, batch=2, size=64,
                                        augment=aug)
    if args.stages:
        res["stages"] = [bench_stages(size, batch, args.reps, dev) for size, batch in ((128, 4), (64, 8))]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
