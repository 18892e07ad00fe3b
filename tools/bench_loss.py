"""Cost of the IoU-family localisation losses (msl_multibox_loss_iou, MultiBoxLoss.set_loc_loss).

    python tools/bench_loss.py [--rounds 2] [--blocks 3] [--steps 800] [--reps 40000] [--size 128] [--batch 4]

Every configuration is measured in a PROCESS OF ITS OWN (a fresh child per configuration and round; the parent never opens
the GPU): a FusedTrainer owns a priority stream and its engine two side streams, and several trainers in one process share
the few hardware queues, so that the slot a trainer was created in shows up in its step time.  The rounds visit the
configurations in rotated order; per configuration the result is the median over all blocks of all rounds, and every block
is listed so that the spread can be read.  All times are HIP events around windows of at least half a second.

  step:*   --size^3 x --batch fp32 with resident inputs (the pool of bench.py), `--steps` steps enqueued back to back
           (fence=False) per block: l1 (the one-launch pack form of the loss), smooth_l1 (the variant route: the launches of
           an IoU kind), iou, giou, diou, and smooth_l1 a second time as a control of the method
  call:*   one call with gradients at N = --batch, P = 9344 (the priors of 128^3), two classes, ~5 % positives with boxes
           near their priors, `--reps` calls back to back per block: msl_multibox_loss_var(flags 0) and the three kinds
Prints one JSON line.  `--config NAME` measures that one configuration in this process (what the children run).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STEP_CONFIGS = {"step:l1": ({}, "l1"), "step:smooth_l1": ({"smooth_l1": True}, "l1"), "step:iou": ({}, "iou"),
                "step:giou": ({}, "giou"), "step:diou": ({}, "diou"), "step:smooth_l1_control": ({"smooth_l1": True}, "l1")}
CALL_CONFIGS = {"call:l1_var_flags0": 0, "call:iou": 1, "call:giou": 2, "call:diou": 3}


def timed(stream, fn):
    import torch
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def measure_call(args, kind, dev):
    """-> ms per block of --reps calls."""
    import torch
    from mslesions3d_amd import _lib
    from mslesions3d_amd._lib import ptr
    L = _lib.load()
    N, P, ncls = args.batch, 9344, 2
    g = torch.Generator().manual_seed(970205)
    tc = (torch.rand((N, P), generator=g) < 0.05).long()
    u = lambda lo, hi: lo + (hi - lo) * torch.rand((N, P, 3), generator=g)  # noqa: E731
    locs = torch.cat([10.0 * u(-0.6, 0.6), 5.0 * u(-0.7, 0.7)], dim=2)
    tl = torch.cat([10.0 * u(-0.3, 0.3), 5.0 * u(-0.5, 0.5)], dim=2)
    pri = torch.cat([0.1 + 0.8 * torch.rand((P, 3), generator=g), 0.05 + 0.2 * torch.rand((P, 3), generator=g)], dim=1)
    scores = torch.randn((N, P, ncls), generator=g) * 2.0
    locs, tl, pri, scores, tc = (t.to(dev).contiguous() for t in (locs, tl, pri, scores, tc))
    ws = torch.zeros(L.msl_multibox_loss_workspace_bytes() // 8, dtype=torch.float64, device=dev)
    var_ws = torch.zeros((L.msl_multibox_loss_var_workspace_bytes(N, P) + 7) // 8, dtype=torch.float64, device=dev)
    loss, up = torch.zeros(3, device=dev), torch.ones(2, device=dev)
    dlocs, dscores = torch.zeros_like(locs), torch.zeros_like(scores)
    stream = torch.cuda.current_stream()
    sm = stream.cuda_stream
    head = [ptr(locs), ptr(scores), ptr(tc), ptr(tl)]
    tail = [ptr(ws), ptr(var_ws), ptr(loss), ptr(up), ptr(dlocs), ptr(dscores), None, N, P, ncls, 0, 3]
    if kind == 0:
        fn, a = getattr(L, "msl_multibox_loss_var"), head + tail + [sm]
    else:
        fn, a = getattr(L, "msl_multibox_loss_iou"), head + [ptr(pri)] + tail + [kind, sm]

    def calls(n):
        for _ in range(n):
            if fn(*a) != 0:
                raise SystemExit("the loss call failed")
    calls(100)  # set-up outside the timed windows: code objects loaded
    runs = [timed(stream, lambda: calls(args.reps)) for _ in range(args.blocks)]
    traffic = N * P * (2 * 6 * 4 + 2 * ncls * 4 + 8 + 6 * 4) + P * 24  # locs, targets, scores, classes in; both gradients out
    return {"per": "call", "n": args.reps, "blocks_ms": runs, "positives": int(tc.sum()), "bytes_per_call": traffic}


def measure_step(args, kw, kind, dev):
    """-> ms per block of --steps steps."""
    import torch
    from mslesions3d_amd.ssd3d import LSSD3D, MultiBoxLoss
    from mslesions3d_amd.synth import make_batch_on_device
    from mslesions3d_amd.trainer import FusedTrainer
    size = (args.size,) * 3
    pool = []
    for k in range(4):
        x, boxes, labels = make_batch_on_device(args.batch, size, dev, 1, seed=k)
        pool.append((x,) + MultiBoxLoss.pack_targets(boxes, labels, dev))
    torch.manual_seed(970205)
    model = LSSD3D(n_classes=2, input_channels=1, input_size=size, threshold=[0.1, 0.2], alpha=1.0, lr=1e-3,
                   batch_size=args.batch, **kw).to(dev).train()
    model.set_loc_loss(kind)
    tr = FusedTrainer(model)

    def block(n):
        for s in range(n):
            x, gb, gl, off, T = pool[s % len(pool)]
            tr.step_packed(x, gb, gl, off, T, sync=False, resident=True, fence=False)
    block(4 * len(pool))  # record and compile every program outside the timed windows
    runs = [timed(tr._stream, lambda: block(args.steps)) for _ in range(args.blocks)]
    return {"per": "step", "n": args.steps, "blocks_ms": runs, "programs": len(tr._programs)}


def measure(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_loss.py measures on the GPU: no device found")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.config in CALL_CONFIGS:
        return measure_call(args, CALL_CONFIGS[args.config], dev)
    return measure_step(args, *STEP_CONFIGS[args.config], dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--steps", type=int, default=800)
    ap.add_argument("--reps", type=int, default=40000)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--config", choices=list(STEP_CONFIGS) + list(CALL_CONFIGS), default=None)
    args = ap.parse_args()
    if args.config is not None:
        print("RESULT " + json.dumps(measure(args)))
        return
    names = list(STEP_CONFIGS) + list(CALL_CONFIGS)
    per, extra = {n: [] for n in names}, {}
    for r in range(args.rounds):
        k = (r * 3) % len(names)
        for name in names[k:] + names[:k]:
            cmd = [sys.executable, os.path.abspath(__file__), "--config", name] + [
                f"--{o}={getattr(args, o)}" for o in ("blocks", "steps", "reps", "size", "batch")]
            out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600).stdout
            res = json.loads([l for l in out.splitlines() if l.startswith("RESULT ")][-1][7:])
            scale = 1e3 if res["per"] == "call" else 1.0  # calls in us, steps in ms
            per[name] += [round(v / res["n"] * scale, 4) for v in res["blocks_ms"]]
            print(f"round {r} {name}: {per[name][-args.blocks:]}", file=sys.stderr, flush=True)
            extra[name] = {k2: v for k2, v in res.items() if k2 not in ("blocks_ms", "per")}
    med = {n: round(statistics.median(v), 4) for n, v in per.items()}
    print(json.dumps({"workload": f"{args.size}^3 x {args.batch} fp32, resident inputs; calls at N={args.batch} P=9344 C=2",
                      "units": {"step": "ms per step", "call": "us per call"}, "rounds": args.rounds, "blocks_per_round": args.blocks,
                      "median": med, "blocks": per, "windows": extra,
                      "giou_minus_smooth_l1_us": round((med["step:giou"] - med["step:smooth_l1"]) * 1e3, 2),
                      "control_minus_smooth_l1_us": round((med["step:smooth_l1_control"] - med["step:smooth_l1"]) * 1e3, 2),
                      "smooth_l1_minus_l1_us": round((med["step:smooth_l1"] - med["step:l1"]) * 1e3, 2)}))


if __name__ == "__main__":
    main()
