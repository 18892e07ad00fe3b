"""Cost of the training metrics in the fused training loop (FusedTrainer.step(..., metrics=True)).

    python tools/bench_train_metrics.py [--steps 50] [--blocks 3] [--size 128] [--batch 4]

128^3 x 4 with resident inputs (the pool of bench.py), fp32 and bf16 in one process.  Blocks of `--steps` steps with the
metrics off and on alternate; each block is timed with HIP events on the trainer's stream (steps enqueued back to back,
fence=False).  For comparison the host route of LSSD3D._metrics (detect_objects + two host calculate_mAP calls) is timed
with the wall clock on the same forward outputs.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def run_dtype(dtype, args, dev):
    from mslesions3d_amd.ssd3d import LSSD3D, MultiBoxLoss
    from mslesions3d_amd.synth import make_batch_on_device
    from mslesions3d_amd.trainer import FusedTrainer
    from mslesions3d_amd.utils import calculate_mAP
    size = (args.size,) * 3
    torch.manual_seed(970205)
    model = LSSD3D(n_classes=2, input_channels=1, input_size=size, threshold=[0.1, 0.2], alpha=1.0, lr=1e-3,
                   batch_size=args.batch).to(dev).train()
    model.compute_dtype = dtype
    trainer = FusedTrainer(model)
    pool = []
    for k in range(4):
        x, boxes, labels = make_batch_on_device(args.batch, size, dev, 1, seed=k)
        pool.append((x,) + MultiBoxLoss.pack_targets(boxes, labels, dev) + (boxes, labels))

    def block(n, metrics):
        for s in range(n):
            x, gb, gl, off, T = pool[s % len(pool)][:5]
            trainer.step_packed(x, gb, gl, off, T, sync=False, resident=True, fence=False, metrics=metrics)

    # set-up: record / compile every program and allocate the metric buffers outside the timed blocks
    block(2 * len(pool), False)
    block(2 * len(pool), True)
    torch.cuda.synchronize()
    trainer.metric_sums(reset=True)
    times = {False: [], True: []}
    for _ in range(args.blocks):
        for metrics in (False, True):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(trainer._stream)
            block(args.steps, metrics)
            e1.record(trainer._stream)
            torch.cuda.synchronize()
            times[metrics].append(e0.elapsed_time(e1) / args.steps)
    avg = trainer.training_metrics()
    # NMS load of the last metric step: candidates above min_score per image (capped at 10 * top_k by the detector)
    ws = next(iter(trainer._met.values()))["ws"]
    ncand = ws["ncand"].tolist()
    # host route on the last step's forward outputs (what LSSD3D._metrics does)
    pl = trainer.last_plan
    locs, scores = pl.locs.clone(), pl.scores.clone()
    boxes, labels = pool[(2 * len(pool) + args.blocks * 2 * args.steps - 1) % len(pool)][5:]
    boxes = [b.to(dev) for b in boxes]
    labels = [l.to(dev) for l in labels]
    dif = [torch.zeros(len(l), dtype=torch.bool) for l in labels]
    host = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        db, dl, ds = model.detect_objects(locs, scores, model.min_score, model.max_overlap, model.top_k)
        calculate_mAP(db, dl, ds, boxes, labels, dif, min_overlap=0.1, return_detail=True)
        calculate_mAP(db, dl, ds, boxes, labels, dif, min_overlap=0.5, return_detail=True)
        host.append((time.perf_counter() - t0) * 1e3)
    plain, met = statistics.median(times[False]), statistics.median(times[True])
    return {"plain_ms_per_step": round(plain, 4), "metric_ms_per_step": round(met, 4),
            "overhead_ms_per_step": round(met - plain, 4), "plain_blocks_ms": [round(v, 4) for v in times[False]],
            "metric_blocks_ms": [round(v, 4) for v in times[True]], "candidates_per_image": ncand,
            "detections_per_image": ws["oc"][:args.batch].tolist(),
            "host_route_ms": round(statistics.median(host), 3), "epoch_means": avg}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--dtype", nargs="+", default=["f32", "bf16"])
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    out = {"workload": f"{args.size}^3 x {args.batch}, resident inputs", "steps_per_block": args.steps, "blocks": args.blocks}
    for dt in args.dtype:
        out[dt] = run_dtype(dt, args, dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
