"""Cost of the device data pipeline (devicedata.DeviceCache, csrc/datapipe.hip) against the host pipeline it replaces.

    python tools/bench_datapipe.py [--reps 20] [--host-reps 2] [--epoch-cases 16] [--skip-epoch]

Per configuration (64^3 x 8 and 128^3 x 4, without augmentation and with ``flip rotate90 translate scale``): one device
batch (gather + resample stages + connected components -> packed boxes) timed with HIP events at steady state (median
of --reps batches after two warm-ups; every augmentation draw of the batch on the host included, since it is enqueued
in the same interval), and one host batch (``ExampleDataset.train_dataloader()``, num_workers 0: load, normalise,
augment with scipy, label, collate; wall clock, median of --host-reps batches).  Then the whole-run wall time of
``train.py`` on a generated toy64 data set, ``-c 0`` against ``-c 1`` (2 epochs, batch 2, each in a fresh process).
Prints one JSON line.
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


def bench_epoch(cases):
    with tempfile.TemporaryDirectory() as tmp:
        DS.generate_artificial_dataset(tmp, "toy64", num_images=cases, image_size=(64, 64, 64))
        out = {}
        for c in (0, 1):
            cmd = [sys.executable, "-m", "mslesions3d_amd.train", "-d", tmp, "-dn", "toy64", "-b", "2", "-me", "2",
                   "-ld", os.path.join(tmp, "logs"), "-en", f"c{c}", "-c", str(c), "-a", *AUG]
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
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"configs": []}
    with tempfile.TemporaryDirectory() as tmp:
        for size, batch in ((64, 8), (128, 4)):
            DS.generate_artificial_dataset(tmp, f"b{size}", num_images=2 * batch + batch // 2 + 1,
                                           image_size=(size,) * 3)
            root = os.path.join(tmp)
            for augment in ([], AUG):
                res["configs"].append(bench_config(root, size, batch, augment, args.reps, args.host_reps, dev))
                print(json.dumps(res["configs"][-1]), file=sys.stderr, flush=True)
    if not args.skip_epoch:
        res["train_py_2_epochs"] = dict(bench_epoch(args.epoch_cases), cases=args.epoch_cases, batch=2, size=64,
                                        augment=AUG)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
