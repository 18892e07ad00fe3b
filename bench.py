"""Headline benchmark: training volumes/s of the 3D-SSD step at 128^3, batch 4 per GPU, fp32 (BASELINE.json).

    python bench.py --gpus 1 --steps 20 --warmup 5
    python bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs bench_outputs   # + the last step's results as .npy
    python bench.py --full                # + roofline, depthwise aggregate, CPU baseline and checks
    python bench.py --dtype bf16          # BASELINE configs[2]: the same step with bf16 activations
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

One "step" = forward + matching + MultiBox loss + backward + (RCCL gradient all-reduce) + fused Adam + cosine LR
step on one resident synthetic batch (``mslesions3d_amd.trainer.FusedTrainer.step_packed``) — nothing is skipped.
Prints ONE JSON line on rank 0 with the whole-job throughput.  A plain run only sets up, warms up and times the
steps.  With ``--full`` the line also holds the roofline of the dominant kernel (the stride-2 depthwise forward of
block 1, timed with HIP events on its launch stream inside the timed steps) and a CPU baseline (the oracle's train
step on the host cores, a bounded sample), and the run checks the losses and (N > 1) the replicas.
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (/opt/skills/guides/MI355X_MICROARCH.md); ~6300 achievable


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="timed steps (train: 100, infer: 50 passes)")
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--size", type=int, default=None, help="volume edge (train: 128, infer: 192)")
    ap.add_argument("--batch", type=int, default=None, help="volumes per GPU (train: 4, infer: 2)")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check what the headline figure does not need: the roofline kernel's HIP-event pairs "
                         "inside the timed steps, the depthwise aggregate, the host enqueue cost, the CPU baseline, the "
                         "finite-loss / replica checks and (infer) the synthetic mAP.  A plain run sets up, warms up, times "
                         "the steps and prints the headline line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step handed its caller as DIR/<name>.npy "
                         "(train: loss.npy = [conf, loc, n_positives], state.npy = the model's floating-point state_dict "
                         "entries flattened in key order; infer: the last pass's detections)")
    ap.add_argument("--channels", type=int, default=1)
    ap.add_argument("--dtype", choices=["f32", "bf16"], default="f32",
                    help="f32: the headline configuration (BASELINE configs[1]); bf16: activations and activation gradients "
                         "stored as bf16, fp32 weights / accumulators / optimiser (BASELINE configs[2])")
    ap.add_argument("--mode", choices=["train", "infer"], default="train",
                    help="train: the headline metric (training volumes/s, 128^3 x 4).  infer: BASELINE configs[3] - predict_step "
                         "(eval forward + decode + 3-D NMS) at 192^3 x 2, volumes/s + kept boxes/s + mAP on synthetic cases")
    ap.add_argument("--train-steps", type=int, default=3, help="infer mode: optimisation steps before the timed inference, outside "
                    "the timed region.  A few steps move the running statistics off their initial values and leave the foreground "
                    "scores near 0.5: every image then reaches the 10*top_k candidate cap, i.e. the NMS kernels do their maximum "
                    "work (a longer run of the reference's live loss first drives every prior to background - 2500 steps: one "
                    "placeholder box per volume, no NMS work at all)")
    ap.add_argument("--event-every", type=int, default=2,
                    help="the roofline kernel's HIP-event pair is recorded on every N-th step / pass of the timed region")
    ap.add_argument("--infer-depth", type=int, default=2,
                    help="--mode infer: batches in flight in LSSD3D.predict_batches (what predict.py uses); 1 = one predict_step "
                         "(enqueue, synchronise, build the lists) after the other")
    ap.add_argument("--map-cases", type=int, default=8, help="infer mode: synthetic cases scored for mAP@0.1 / 0.5")
    ap.add_argument("--opt", action="append", default=[], metavar="NAME=VALUE",
                    help="set a schedule option of the engine / trainer / launch-program replayer for A/B runs, e.g. --opt "
                         "fold_np_max=64 --opt match_after=5 (plain attributes of mslesions3d_amd.engine.Engine, trainer.FusedTrainer, "
                         "_lib; echoed under 'knobs').  The library itself reads no tuning environment variables.")
    ap.add_argument("--fence", action="store_true", help="bracket every step with stream hand-offs to the caller's stream (default: "
                    "the steps of the timed region are enqueued back to back on the trainer's stream)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--cpu-steps", type=int, default=25)  # ~10 s of CPU work
    ap.add_argument("--no-aggregate", action="store_true",
                    help="--full without the two extra all-depthwise-layer passes after the timed region (rocprofv3 runs: keeps "
                         "the kernel statistics those of the training step alone)")
    ap.add_argument("--no-events", action="store_true",
                    help="--full without the HIP-event pair around the roofline kernel inside the timed steps")
    ap.add_argument("--profile-all", action="store_true", help="HIP-event time every launch and print a table (stderr)")
    return ap.parse_args()


def dump_outputs(path, arrays):
    """--dump-outputs: one DIR/<name>.npy per array (float32 / float64 only)."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    for name, a in arrays.items():
        a = np.ascontiguousarray(a)
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        np.save(os.path.join(path, name + ".npy"), a)


def apply_opts(opts, *targets):
    """--opt name=value -> setattr on the first target that has the attribute (int / float / bool / 'a,b' set / string)."""
    done = {}
    for item in opts:
        name, _, raw = item.partition("=")
        if raw.lower() in ("true", "false"):
            val = raw.lower() == "true"
        elif raw.lower() == "none":
            val = None
        else:
            try:
                val = int(raw)
            except ValueError:
                try:
                    val = float(raw)
                except ValueError:
                    val = {int(v) for v in raw.split(",")} if "," in raw and raw.replace(",", "").isdigit() else raw
        for t in targets:
            if hasattr(t, name):
                setattr(t, name, val)
                done[name] = raw
                break
        else:
            raise SystemExit(f"--opt {name}: no such option on {[type(t).__name__ for t in targets]}")
    return done


def cpu_baseline(size, batch, channels, steps):
    """The oracle (CPU restatement of the reference, kind 'port') timed on the host cores: 1 warm-up + `steps`."""
    from oracle.network import OracleSSD3D
    from oracle.train_step import make_optimizer, train_step
    from mslesions3d_amd.synth import make_case
    import numpy as np
    torch.manual_seed(970205)
    # the GPU box exposes every host core but a 1-GPU job owns a 16-core share: more threads only thrash
    cores = min(len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1), 16)
    torch.set_num_threads(cores)
    model = OracleSSD3D(2, channels, (size,) * 3, emulate_reference_init=False).train()
    opt, sch = make_optimizer(model, 1e-3)
    imgs, boxes, labels = [], [], []
    for i in range(batch):
        img, _, b, l = make_case(i, (size,) * 3)
        imgs.append(np.stack([img] * channels))
        boxes.append(torch.from_numpy(b))
        labels.append(torch.from_numpy(l))
    x = torch.from_numpy(np.stack(imgs))
    train_step(model, opt, sch, x, boxes, labels, [0.1, 0.2])
    t0 = time.perf_counter()
    for _ in range(steps):
        train_step(model, opt, sch, x, boxes, labels, [0.1, 0.2])
    dt = time.perf_counter() - t0
    return {"value": round(batch * steps / dt, 3), "unit": "volumes/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": f"{steps} timed train steps (+1 warm-up) of the same {size}^3 batch-{batch} fp32 workload, "
                      f"oracle (plain torch CPU ops), {dt / steps * 1e3:.0f} ms/step"}


def cpu_baseline_infer(model, x, steps, kw):
    """The oracle's predict path (eval forward + detect_objects, kind 'port') on the host cores, on the batch the GPU timed,
    with the GPU model's weights.  Also returns its detections (prior indices per image) for the parity field."""
    from oracle import detect as OD
    from oracle.network import OracleSSD3D
    cores = min(len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1), 16)
    torch.set_num_threads(cores)
    size = tuple(x.shape[2:])
    om = OracleSSD3D(model.n_classes, x.shape[1], size, emulate_reference_init=False)
    om.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()})
    om.eval()
    xc = x.detach().cpu()

    def once():
        with torch.no_grad():
            ol, osc = om(xc)
            return OD.detect_objects(ol, osc, om.priors_cxcycz, kw["min_score"], kw["max_overlap"], kw["top_k"], return_prior_index=True)
    det = once()
    t0 = time.perf_counter()
    for _ in range(steps):
        once()
    dt = time.perf_counter() - t0
    n = x.shape[0]
    return ({"value": round(n * steps / dt, 3), "unit": "volumes/s", "cores": torch.get_num_threads(), "kind": "port",
             "sample": f"{steps} timed predict passes (+1 warm-up) of the same {size[0]}^3 batch-{n} fp32 workload: oracle eval "
                       f"forward + detect_objects (plain torch CPU ops), {dt / steps * 1e3:.0f} ms per batch"}, det)


def main_infer(args):
    """BASELINE configs[3]: 192^3, batch 2, predict.py path (LSSD3D.predict_step = eval forward + softmax / decode + per-class
    candidate selection + 3-D NMS + top-k, ssd3d.py:344-460,692-702) on inputs resident in HBM.  One JSON line."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    backend = os.environ.get("MSL_BENCH_BACKEND", "nccl")
    local = local % max(torch.cuda.device_count(), 1) if backend != "nccl" else local
    if world > 1:  # replicas only: no collective on the data path; the process group carries the timing barrier
        from mslesions3d_amd.parallel import init_distributed
        init_distributed(backend, rank=rank, world_size=world, device=torch.device("cuda", local) if backend == "nccl" else None)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    from mslesions3d_amd.ssd3d import LSSD3D
    from mslesions3d_amd.synth import make_batch_on_device
    from mslesions3d_amd.trainer import FusedTrainer
    from mslesions3d_amd.utils import calculate_mAP
    size = (args.size,) * 3
    torch.manual_seed(970205)
    model = LSSD3D(n_classes=2, input_channels=args.channels, input_size=size, threshold=[0.1, 0.2], alpha=1.0, lr=1e-3,
                   batch_size=args.batch).to(dev).train()
    from mslesions3d_amd import _lib
    # a short optimisation run so that scores and running statistics are not the initial ones (fp32, outside the timed region)
    tr = FusedTrainer(model)
    opts = apply_opts(args.opt, model._engine, tr, _lib)  # (--opt used to be ignored in this mode)
    t_tr = time.perf_counter()
    for s in range(args.train_steps):
        x, boxes, labels = make_batch_on_device(args.batch, size, dev, args.channels, seed=5000 + s % 64)
        tr.step(x, boxes, labels, sync=(s == args.train_steps - 1))
    torch.cuda.synchronize()
    t_tr = time.perf_counter() - t_tr
    model.eval()
    model.compute_dtype = args.dtype
    kw = dict(min_score=0.3, max_overlap=0.3, top_k=50)
    model.min_score, model.max_overlap, model.top_k = kw["min_score"], kw["max_overlap"], kw["top_k"]
    x, gt_boxes, gt_labels = make_batch_on_device(args.batch, size, dev, args.channels, seed=1000 * rank + 3)
    for _ in range(max(args.warmup, 2)):
        model.predict_step({"img": x})
    buf = model.predict_input_buffer(x.shape)  # inputs resident in HBM: the batch lives in predict_step's staging buffer
    buf.copy_(x)
    torch.cuda.synchronize()
    eng = model._engine
    events = args.full and not args.no_events
    if events:
        eng.start_profile({"stem_fwd"})
        for _ in range(2):  # set-up: compile the replay variant that carries the stem's event pair (not inside the timed region)
            model.predict_step({"img": buf})
        eng.stop_profile()
        eng.start_profile({"stem_fwd"})
    sink = eng.prof

    def feed():
        for s in range(args.steps):
            if sink is not None:  # the event pair rides on every `--event-every`-th pass (measurement overhead, not workload)
                eng.prof = sink if s % args.event_every == 0 else None
            yield {"img": buf}

    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    nboxes = 0
    last = None
    # predict.py's loop: LSSD3D.predict_batches keeps `--infer-depth` batches in flight (1 = predict_step batch by batch)
    for out in model.predict_batches(feed(), depth=args.infer_depth):
        nboxes += sum(len(b) for b in out[0])
        last = out
    eng.prof = sink
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    prof = eng.stop_profile() if events else {}
    tmax = torch.tensor([dt, 0.0], dtype=torch.float64, device=dev)
    tsum = torch.tensor([float(nboxes)], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dist.all_reduce(tsum, op=dist.ReduceOp.SUM)
    dt, nboxes = float(tmax[0].item()), float(tsum.item())
    if args.dump_outputs and rank == 0:
        # the last timed pass's detections as predict_step hands them over (per image: boxes, labels, scores), concatenated
        # over the images of the batch; counts.npy says how many rows belong to each image
        import numpy as np
        b, l, s_ = last[:3]
        flat = lambda ts: np.concatenate([t.detach().cpu().double().numpy().reshape(-1) for t in ts])
        dump_outputs(args.dump_outputs, {"boxes": flat(b).astype(np.float32).reshape(-1, 6), "labels": flat(l),
                                         "scores": flat(s_).astype(np.float32),
                                         "counts": np.array([len(t) for t in b], dtype=np.float64)})
    maps = None
    if args.full:
        # mAP on synthetic cases (rank 0; detections of this dtype against the generator's ground truth)
        det_b, det_l, det_s, tb, tl = [], [], [], [], []
        for c in range(0, args.map_cases, args.batch):
            xs, bs, ls = make_batch_on_device(args.batch, size, dev, args.channels, seed=9000 + c)
            b, l, s_ = model.predict_step({"img": xs})
            det_b += [t.cpu() for t in b]
            det_l += [t.cpu() for t in l]
            det_s += [t.cpu() for t in s_]
            tb += [t.cpu() for t in bs]
            tl += [t.cpu() for t in ls]
        dif = [torch.zeros(len(t), dtype=torch.bool) for t in tl]
        maps = {}
        for iou in (0.1, 0.5):
            d = calculate_mAP(det_b, det_l, det_s, tb, tl, dif, min_overlap=iou, return_detail=True)
            maps[str(iou)] = {k: round(float(d[k]), 6) for k in ("mAP", "precision", "recall", "f1_score")}
    if rank == 0:
        pl = eng.plan_for(buf, False)
        d0 = pl.dims[0]
        esz = 4.0 if args.dtype == "f32" else 2.0
        vol = lambda d: d[0] * d[1] * d[2]
        alg_bytes = 4.0 * args.batch * args.channels * vol(size) + esz * args.batch * 32 * vol(d0) + 4.0 * 32 * 27 * args.channels
        ms = prof.get("stem_fwd", [])
        avg_ms = sum(ms) / max(len(ms), 1)
        achieved = alg_bytes / (avg_ms * 1e-3) / 1e9 if ms else None
        out = {
            "metric": "inference volumes/sec at 192^3 batch-2 (predict_step: eval forward + decode + 3-D NMS), replicas over N MI355X",
            "value": round(world * args.batch * args.steps / dt, 2), "unit": "volumes/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "boxes_per_s": round(nboxes / dt, 1),
            "config": {"workload": f"{args.size}^3 synthetic volumes, batch {args.batch}/GPU, {args.channels} channel(s), "
                                   f"{'fp32' if args.dtype == 'f32' else 'bf16 activations / fp32 weights and accumulators'}, SSD3D+MobileNet3D "
                                   f"predict_step with 3-D NMS (BASELINE configs[3]), min_score {kw['min_score']}, max_overlap "
                                   f"{kw['max_overlap']}, top_k {kw['top_k']}; weights: random init + {args.train_steps} fp32 optimisation "
                                   f"steps on synthetic batches ({t_tr:.1f} s, untimed)",
                       "global_batch": world * args.batch, "parallelism": f"replicas x{world}", "priors": pl.P},
            "knobs": dict({k: v for k, v in sorted(os.environ.items()) if k.startswith("MSL_")}, **opts),
        }
        if args.full:
            out["mAP_synthetic"] = {"cases": args.map_cases, "IoU": maps,
                                    "note": "detections of this run's dtype against the generator's cube boxes (synth.make_batch_on_device)"}
            out["roofline"] = {"bound": "hbm", "kernel": "stem forward (dense 3x3x3 s2, 1->32 channels; the longest launch of the pass)",
                               "achieved": None if achieved is None else round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                               "frac": None if achieved is None else round(achieved / HBM_PEAK_GBS, 4),
                               "frac_basis": f"HIP-event pair around the launch inside the timed predict passes, on every {args.event_every}. pass",
                               "traffic": None, "algorithmic_bytes_per_launch": alg_bytes, "avg_launch_us": round(avg_ms * 1e3, 2),
                               "launches_timed": len(ms)}
            if getattr(pl, "stem_dw_eval", False) and avg_ms:
                # eval mode runs stem + BatchNorm + ReLU + block-1 depthwise convolution as ONE launch that never writes the stem
                # activation (csrc/stemdw.hip): x and z1 are all it moves (85 MB at 192^3 x 2), so it is bound by the fp32 matrix
                # pipe - algorithmic FLOPs (no recomputed halo) over the MI355X's fp32 MFMA peak
                d1 = pl.dims[1]
                flops = 2.0 * 27 * args.channels * 32 * args.batch * vol(d0) + 2.0 * 27 * 32 * args.batch * vol(d1)
                tf = flops / (avg_ms * 1e-3) / 1e12
                out["roofline"].update({"bound": "mfma", "kernel": "stem + BatchNorm + ReLU + block-1 depthwise forward in one launch "
                                        "(stem_dw_eval_kernel; the longest launch of the pass)", "achieved": round(tf, 2),
                                        "peak": 157.3, "unit": "TFLOP/s", "frac": round(tf / 157.3, 4), "algorithmic_flops_per_launch": flops,
                                        "algorithmic_bytes_per_launch": 4.0 * args.batch * args.channels * vol(size) + esz * args.batch * 32 * vol(d1)})
            if world == 1 and not args.no_cpu_baseline:
                cb, odet = cpu_baseline_infer(model, x, max(1, min(args.cpu_steps, 10)), kw)
                out["cpu_baseline"] = cb
                model_det = model.detect_objects(*model(x), return_prior_index=True, **kw) if args.dtype == "f32" else None
                if model_det is not None:
                    same = all(torch.equal(model_det[3][i].cpu(), odet[3][i]) for i in range(args.batch))
                    out["cpu_baseline"]["keep_lists_equal_oracle"] = bool(same)
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


def main():
    args = parse()
    if args.mode == "infer" and args.size is None and args.batch is None:
        args.size, args.batch = 192, 2  # configs[3]
    args.size = 128 if args.size is None else args.size
    args.batch = 4 if args.batch is None else args.batch
    if args.steps is None:
        args.steps = 50 if args.mode == "infer" else 100
    if args.mode == "infer":
        return main_infer(args)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # MSL_BENCH_BACKEND=gloo rehearses the N > 1 path on a box with fewer GPUs than ranks (ranks then share devices;
    # functional check only - the driver's scaling run uses RCCL, one rank per GPU)
    backend = os.environ.get("MSL_BENCH_BACKEND", "nccl")
    local = local % max(torch.cuda.device_count(), 1) if backend != "nccl" else local
    rehearse = world == 1 and os.environ.get("MSL_DP_REHEARSE") == "1"  # one-rank RCCL group: DP host/launch cost on 1 GPU
    if rehearse:
        os.environ.setdefault("MASTER_PORT", "29577")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
    if world > 1 or rehearse:
        from mslesions3d_amd.parallel import init_distributed
        # finite collective timeout + watchdog tear-down (see init_distributed): a lost rank ends the run with an error
        init_distributed(backend, rank=rank, world_size=world, device=torch.device("cuda", local) if backend == "nccl" else None)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)

    from mslesions3d_amd import _lib
    from mslesions3d_amd.parallel import broadcast_model
    from mslesions3d_amd.ssd3d import LSSD3D, MultiBoxLoss
    from mslesions3d_amd.synth import make_batch_on_device
    from mslesions3d_amd.trainer import FusedTrainer

    size = (args.size,) * 3
    torch.manual_seed(970205)  # train.py:61
    model = LSSD3D(n_classes=2, input_channels=args.channels, input_size=size, threshold=[0.1, 0.2], alpha=1.0, lr=1e-3,
                   batch_size=args.batch).to(dev).train()
    model.compute_dtype = args.dtype
    model._ensure_device_state(dev)
    model._engine.ensure_arena(dev)
    broadcast_model(model)
    trainer = FusedTrainer(model)
    opts = apply_opts(args.opt, model._engine, trainer, _lib)

    # a small pool of resident batches (different volumes per rank: weak scaling, independent shards)
    pool = []
    for k in range(4):
        x, boxes, labels = make_batch_on_device(args.batch, size, dev, args.channels, seed=1000 * rank + k)
        pool.append((x,) + MultiBoxLoss.pack_targets(boxes, labels, dev))

    def run(nsteps):
        sink = model._engine.prof  # (None outside the timed region)
        for s in range(nsteps):
            x, gb, gl, off, T = pool[s % len(pool)]
            # the roofline kernel's HIP-event pair rides on every `--event-every`-th step of the timed region (a pair costs
            # its stream ~5 us: measurement overhead, not workload); the other steps replay the program without it
            if sink is not None and not args.profile_all:
                model._engine.prof = sink if s % args.event_every == 0 else None
            # the steps of a run are enqueued back to back on the trainer's stream (fence=False: no per-step round trip
            # through the caller's stream); torch.cuda.synchronize() on both sides of the timed region orders everything else
            trainer.step_packed(x, gb, gl, off, T, sync=False, resident=True, fence=args.fence)
        model._engine.prof = sink

    # Set-up, before the warm-up: record the launch program of each resident batch (its first step runs through the Python
    # executor) and compile both replay variants (plain / with the roofline kernel's event pair), so that neither the W
    # warm-up steps nor the K timed steps contain a one-time host-side compilation (with --warmup 5 three of the four
    # programs used to be compiled inside the timed region: -5 % on a 20-step run)
    eng = model._engine
    events = not args.no_events and (args.full or args.profile_all)
    run(2 * len(pool))
    if events and not args.profile_all:
        eng.start_profile({"dw_fwd1"})
        run(2 * len(pool))
        eng.stop_profile()
    torch.cuda.synchronize()
    run(args.warmup)
    torch.cuda.synchronize()
    if events:
        eng.start_profile(None if args.profile_all else {"dw_fwd1"})
    if world > 1 or rehearse:  # the rehearsal runs every collective of the N > 1 path on one rank
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(args.steps)
    t_host = time.perf_counter() - t0  # host-side enqueue time (diagnostic only)
    torch.cuda.synchronize()
    if world > 1 or rehearse:  # the rehearsal runs every collective of the N > 1 path on one rank
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    prof = eng.stop_profile() if events else {}
    tmax = torch.tensor([dt], dtype=torch.float64, device=dev)
    if world > 1 or rehearse:  # the rehearsal runs every collective of the N > 1 path on one rank
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    dt = float(tmax.item())
    # what the last timed step handed its caller (one sync, outside the timed region): loss_out and the model's state
    pl = trainer.last_plan
    loss_out = model.loss_fn._state(args.batch, pl.P, 2, 0, dev)["loss_out"]
    conf, loc, npos = loss_out.tolist()
    if args.dump_outputs and rank == 0:
        state = [v.detach().reshape(-1).float() for v in model.state_dict().values() if v.is_floating_point()]
        dump_outputs(args.dump_outputs, {"loss": loss_out.double().cpu().numpy(), "state": torch.cat(state).cpu().numpy()})
    dw_all, dw_alone, t_host1 = None, {}, None
    if args.full:
        # SURVEY 8(d)'s aggregate over ALL seven depthwise forwards, timed in situ in a short pass of its own (14 more
        # event records per step would perturb the timed region above): outside the timed region, not part of `value`
        if not args.profile_all and not args.no_aggregate:
            eng.start_profile({f"dw_fwd{i}" for i in range(1, 8)})
            run(20)
            dw_all = eng.stop_profile()
        # ... and the same seven launches re-issued alone from the recorded launch program (the step's own buffers and
        # arguments), 50 back to back per layer between one event pair: kernel + dependent dispatch, without the ~5 us an
        # event pair adds around a single 5 us kernel.  Idempotent launches (they rewrite the same outputs and partials).
        progs = list(getattr(trainer, "_programs", {}).values())
        if progs and not args.profile_all and not args.no_aggregate:
            by_tag = {tag: (fn, a) for fn, a, tag in progs[-1]["prog"] if fn is not None and str(tag).startswith("dw_fwd")}
            with torch.cuda.stream(trainer._stream):
                for i in range(1, 8):
                    if f"dw_fwd{i}" not in by_tag:
                        continue
                    fn, a = by_tag[f"dw_fwd{i}"]
                    for _ in range(5):
                        fn(*a)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(50):
                        fn(*a)
                    e1.record()
                    e1.synchronize()
                    dw_alone[i] = e0.elapsed_time(e1) / 50 * 1e3
            torch.cuda.synchronize()
        # diagnostic: pure host cost of enqueueing one step (GPU idle, empty queues -> no back-pressure)
        t_enq = []
        for _ in range(5):
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            run(1)
            t_enq.append(time.perf_counter() - t1)
        torch.cuda.synchronize()
        t_host1 = sorted(t_enq)[len(t_enq) // 2]
        # sanity: the last step produced finite losses
        eng.check_nan(pl)
        assert conf == conf and loc == loc and npos > 0, (conf, loc, npos)
        if world > 1 or rehearse:  # the rehearsal runs every collective of the N > 1 path on one rank
            # data-parallel invariant (outside the timed region): every replica holds the same parameters
            flat = model._engine.arena.flat
            ref = flat.detach().clone()
            dist.broadcast(ref, src=0)
            same = torch.tensor([1.0 if torch.equal(ref, flat) else 0.0], device=dev)
            dist.all_reduce(same, op=dist.ReduceOp.MIN)
            assert float(same.item()) == 1.0, "replicas diverged: the gradient all-reduce is not reaching every parameter"

    if rank == 0:
        value = world * args.batch * args.steps / dt
        out = {
            "metric": "training volumes/sec at 128^3 batch-4 (fwd+loss+bwd+Adam), data-parallel over N MI355X",
            "value": round(value, 2), "unit": "volumes/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(dt / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": f"{args.size}^3 synthetic volumes, batch {args.batch}/GPU, {args.channels} channel(s), "
                                   + ("fp32, SSD3D+MobileNet3D full train step (BASELINE configs[1])" if args.dtype == "f32" else
                                      "bf16 activations + activation gradients / fp32 weights, accumulators and Adam, "
                                      "SSD3D+MobileNet3D full train step (BASELINE configs[2])"),
                       "global_batch": world * args.batch, "parallelism": f"dp{world}", "priors": pl.P,
                       "setup": "before the W warm-up steps: the launch program of each of the 4 resident batches recorded (one "
                                "step through the Python executor) and its replay compiled"
                                + (" in both variants, plain and with the roofline kernel's event pair (untimed)" if events
                                   else " (untimed)"),
                       "last_loss": {"conf": conf, "loc": loc, "n_positives": npos}},
            "knobs": dict({k: v for k, v in sorted(os.environ.items()) if k.startswith("MSL_")}, **opts),
        }
        if args.full:
            # dominant kernel: depthwise forward of block 1 (stride 2): input (N,32,S0) read once + output written once + weights
            C1 = 32
            d0 = pl.dims[0]
            d1 = pl.dims[1]
            esz = 4.0 if args.dtype == "f32" else 2.0  # bytes per activation element in HBM
            alg_bytes = esz * args.batch * C1 * (d0[0] * d0[1] * d0[2] + d1[0] * d1[1] * d1[2]) + 4.0 * C1 * 27
            ms = prof.get("dw_fwd1", [])
            avg_ms = sum(ms) / max(len(ms), 1)
            achieved = alg_bytes / (avg_ms * 1e-3) / 1e9 if ms else None
            if args.dtype == "f32":
                variant = _lib.load().msl_dwconv_fwd_variant(args.batch, C1, *d0, 2)
                dw1_kernel = {3: "dw_s2_wave_kernel<4,5,4>", 1: "dw_fwd_stream_kernel<2,1,4,0>"}.get(variant, f"dwconv variant {variant}")
            else:
                dw1_kernel = "dw_s2_wave_kernel<4,5,4,bf16>"  # the fp32 wave kernel templated on the storage type
            # committed rocprofv3 measurements of THIS kernel on this workload (tools/summarize_profiles.py): PMC bytes per
            # launch and the kernel-trace duration.  Constants of the named profile, not something this run measured.
            traffic, traffic_src, frac_rocprof, agg_rocprof = None, None, None, None
            tpath = os.path.join(ROOT, "profiles", "dw_fwd1_traffic.json" if args.dtype == "f32" else "dw_fwd1_traffic_bf16.json")
            default_shape = args.size == 128 and args.batch == 4 and args.channels == 1
            if os.path.exists(tpath) and default_shape:
                tj = json.load(open(tpath))
                if tj.get("kernel", "").replace(" ", "") == dw1_kernel:
                    traffic = tj.get("hbm_bytes_per_launch")
                    traffic_src = f"profiles/{tj.get('profile')}_pmc_summary.csv (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE of this " \
                                  f"command, committed; not measured by this run)"
                    if tj.get("avg_launch_us_rocprof"):
                        us = float(tj["avg_launch_us_rocprof"])
                        frac_rocprof = {"frac": round(alg_bytes / (us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4), "avg_launch_us": us,
                                        "profile": f"profiles/{tj.get('profile')}_kernel_stats.csv"}
                    agg_rocprof = tj.get("depthwise_fwd_all_layers_rocprof")
            out["roofline"] = {"bound": "hbm", "kernel": dw1_kernel + " (depthwise 3x3x3 s2 forward, block 1)",
                               "achieved": None if achieved is None else round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                               "frac": None if achieved is None else round(achieved / HBM_PEAK_GBS, 4),
                               "frac_basis": f"HIP-event pair around the launch inside the timed steps, on every "
                                             f"{args.event_every}. step (includes the dispatch gap; "
                                             "conservative against the kernel-trace duration in frac_rocprof)",
                               "frac_rocprof": frac_rocprof,
                               "traffic": traffic, "traffic_source": traffic_src, "algorithmic_bytes_per_launch": alg_bytes,
                               "avg_launch_us": round(avg_ms * 1e3, 2), "launches_timed": len(ms)}
            if dw_all and all(dw_all.get(f"dw_fwd{i}") for i in range(1, 8)):
                # block i reads (N, C_i, dims[i-1]) and writes (N, C_i, dims[i]) once, plus its taps
                chans = [32, 64, 128, 128, 256, 256, 512]
                vol = lambda d: d[0] * d[1] * d[2]
                lay_b = [esz * args.batch * c * (vol(pl.dims[i]) + vol(pl.dims[i + 1])) + 4.0 * c * 27 for i, c in enumerate(chans)]
                lay_us = [1e3 * sum(dw_all[f"dw_fwd{i}"]) / len(dw_all[f"dw_fwd{i}"]) for i in range(1, 8)]
                tot_gbs = sum(lay_b) / (sum(lay_us) * 1e-6) / 1e9
                agg = {"algorithmic_bytes": sum(lay_b),
                       "in_step_event_pairs": {"sum_launch_us": round(sum(lay_us), 2), "achieved": round(tot_gbs, 1),
                                               "frac": round(tot_gbs / HBM_PEAK_GBS, 4),
                                               "per_layer_us": [round(u, 2) for u in lay_us]},
                       "rocprof_kernel_trace": agg_rocprof,
                       "note": "SURVEY 8(d): all seven depthwise forwards, algorithmic bytes / sum(t) / peak, three accountings "
                               "under fixed keys.  rocprof_kernel_trace: kernel durations of the committed profile (null when "
                               "this is not the profiled shape).  in_step_event_pairs: a HIP "
                               "event pair around each of the seven launches inside the replayed step (20-step pass after "
                               "the timed region; each pair adds ~5 us of event/dispatch overhead to a ~5 us kernel).  "
                               "back_to_back: each launch re-issued 50x alone from the recorded program on the step's "
                               "buffers, one event pair per layer (kernel + dependent dispatch).  rocprofv3 kernel "
                               "durations of the step: profiles/"}
                if len(dw_alone) == 7:
                    alone = [dw_alone[i] for i in range(1, 8)]
                    gbs = sum(lay_b) / (sum(alone) * 1e-6) / 1e9
                    agg["back_to_back"] = {"sum_launch_us": round(sum(alone), 2), "achieved": round(gbs, 1),
                                           "frac": round(gbs / HBM_PEAK_GBS, 4), "per_layer_us": [round(u, 2) for u in alone]}
                out["roofline"]["depthwise_fwd_all_layers"] = agg
            print(f"host enqueue {t_host / args.steps * 1e3:.3f} ms/step of {dt / args.steps * 1e3:.3f} ms/step wall; "
                  f"one step into empty queues: {t_host1 * 1e3:.3f} ms", file=sys.stderr)
        if args.profile_all:
            rows = sorted(((sum(v) / len(v), t, len(v)) for t, v in prof.items()), reverse=True)
            tot = sum(r[0] for r in rows)
            print(f"per-launch HIP-event times (avg ms per step), total {tot:.3f} ms", file=sys.stderr)
            for a, t, n in rows:
                print(f"  {t:40s} {a * 1e3:9.1f} us  x{n}", file=sys.stderr)
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(args.size, args.batch, args.channels, args.cpu_steps)
        print(json.dumps(out))
    if world > 1 or rehearse:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
