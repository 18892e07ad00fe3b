"""Cost of the per-tensor histograms (FusedTrainer.step(..., stats=True), diagnostics.TensorStats / msl_tensor_stats).

    python tools/bench_tensor_stats.py [--steps 50] [--blocks 5] [--size 128] [--batch 4] [--reps 200]

Two numbers, both from HIP events on the trainer's stream, medians of repeated runs in one process:
  pass alone        `--reps` passes enqueued back to back on an otherwise idle GPU (after a real step, so the arena holds a
                    real gradient), per pass, `--blocks` times; for 1, 2 and 3 sources
  extra step time   128^3 x 4 fp32 with resident inputs (the pool of bench.py), steps enqueued back to back (fence=False):
                    blocks of `--steps` steps with stats off and with stats on EVERY step alternate; the difference of the
                    two medians (train.py --grad_histograms 25 pays a 25th of it)
Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    from mslesions3d_amd.diagnostics import TensorStats
    from mslesions3d_amd.ssd3d import LSSD3D, MultiBoxLoss
    from mslesions3d_amd.synth import make_batch_on_device
    from mslesions3d_amd.trainer import FusedTrainer
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    size = (args.size,) * 3
    torch.manual_seed(970205)
    model = LSSD3D(n_classes=2, input_channels=1, input_size=size, threshold=[0.1, 0.2], alpha=1.0, lr=1e-3,
                   batch_size=args.batch).to(dev).train()
    trainer = FusedTrainer(model)
    pool = []
    for k in range(4):
        x, boxes, labels = make_batch_on_device(args.batch, size, dev, 1, seed=k)
        pool.append((x,) + MultiBoxLoss.pack_targets(boxes, labels, dev))

    def block(n, stats):
        for s in range(n):
            x, gb, gl, off, T = pool[s % len(pool)]
            trainer.step_packed(x, gb, gl, off, T, sync=False, resident=True, fence=False, stats=stats)

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(trainer._stream)
        fn()
        e1.record(trainer._stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    # set-up outside the timed blocks: record / compile every program, build the statistics tables
    block(2 * len(pool), False)
    block(2 * len(pool), True)
    torch.cuda.synchronize()
    arena = model._engine.arena
    stream = trainer._stream.cuda_stream
    alone = {}
    for sources in (("grad",), ("grad", "param"), ("grad", "param", "exp_avg")):
        ts = TensorStats(arena, sources, optimizer=trainer.opt)

        def passes():
            with torch.cuda.stream(trainer._stream):
                for _ in range(args.reps):
                    ts.enqueue(stream)
        passes()
        runs = [timed(passes) / args.reps * 1e3 for _ in range(args.blocks)]
        alone["+".join(sources)] = {"us_per_pass": round(statistics.median(runs), 2), "runs_us": [round(v, 2) for v in runs],
                                    "workgroups": ts.n_blocks * len(sources), "bytes_read": 4 * arena.n_trainable * len(sources)}
    times = {False: [], True: []}
    for _ in range(args.blocks):
        for stats in (False, True):
            times[stats].append(timed(lambda: block(args.steps, stats)) / args.steps)
    plain, with_stats = statistics.median(times[False]), statistics.median(times[True])
    snapshot = trainer.last_stats()
    worst = max(snapshot["tensors"].items(), key=lambda kv: kv[1]["grad"]["rms"])
    print(json.dumps({"workload": f"{args.size}^3 x {args.batch} fp32, resident inputs", "steps_per_block": args.steps,
                      "blocks": args.blocks, "tensors": len(snapshot["tensors"]), "elements": arena.n_trainable,
                      "pass_alone": alone, "plain_ms_per_step": round(plain, 4), "stats_ms_per_step": round(with_stats, 4),
                      "extra_us_per_stats_step": round((with_stats - plain) * 1e3, 2),
                      "plain_blocks_ms": [round(v, 4) for v in times[False]],
                      "stats_blocks_ms": [round(v, 4) for v in times[True]],
                      "largest_grad_rms": [worst[0], worst[1]["grad"]["rms"]]}))


if __name__ == "__main__":
    main()
