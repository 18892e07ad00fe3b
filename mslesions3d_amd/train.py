"""Training entry point — the flags of the reference's ``lesions3d/train.py:27-64`` and the flow of its
``example()`` (``train.py:128-188``) without Lightning / wandb / MONAI:

    python -m mslesions3d_amd.train -d DATA -dn NAME -b 2 -me 2 -ld LOGS

dataset -> LSSD3D(n_classes + 1, input_channels=len(input_images), ...) -> loop {training_step-equivalent fused step, validation at
epoch end} -> metrics as JSONL with the reference's scalar names -> top-3 checkpoints by ``avg_val_loss`` ->
early stopping on the validation loss (patience 5) -> stop at ``max_iterations`` / ``max_epochs``.

Data parallel (BASELINE north_star; the reference is single-GPU, train.py:182 ``devices=1``):

    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 -m mslesions3d_amd.train ...
"""
import argparse
import json
import os
from os.path import join as pjoin

import torch


def build_parser():
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('-d', '--dataset_path', type=str, default=r'../data/artificial_dataset')
    p.add_argument('-dn', '--dataset_name', type=str, default="#3k_64_n1-5_s6-14")
    p.add_argument('-su', '--subject', type=str, default=None)
    p.add_argument('-p', '--percentage', type=float, default=1.)
    p.add_argument('--n_classes', type=int, default=1)
    p.add_argument('-b', '--batch_size', type=int, default=8)
    p.add_argument('-lr', '--learning_rate', type=float, default=0.001)
    p.add_argument('-sr', '--scheduler', type=str, default="CosineAnnealingLR")
    p.add_argument('-th', '--threshold', type=float, default=[0.1, 0.2], nargs='+')
    p.add_argument('-pl', '--prediction_layers', type=str, default="3 5 7")
    p.add_argument('-cfg', '--base_network_config', type=str, default="mobilenet")
    p.add_argument('-sc', '--scales', type=json.loads, default="{}")
    p.add_argument('-bpl', '--boxes_per_location', type=int, default=2)
    p.add_argument('-minos', '--min_object_size', type=int, default=6)
    p.add_argument('-maxos', '--max_object_size', type=int, default=14)
    p.add_argument('--alpha', type=float, default=1.)
    p.add_argument('-a', '--augmentations', type=str, nargs='*', default=[],
                   help='flip rotate90 translate scale (example recipe); affine shiftintensity scaleintensity (train_lesions); '
                        'zoom griddistortion (separable warps) elastic3d (free-form deformation): one resampling stage '
                        'per run with -dm lesions -c 1; '
                        'lesionpaste (-dm lesions: copy-paste of lesions of the training cases on to the finished sample); '
                        'gaussiansmooth biasfield gaussiannoise (the MR stage, applied last to the finished sample)')
    p.add_argument('--paste_max_volume', type=float, default=None, metavar='V',
                   help="lesionpaste: only lesions whose bounding-box volume is at most V voxels enter the bank "
                        "(the measure of eval --size_bins; default: no limit)")
    p.add_argument('-ld', '--logdir', type=str, default=r'../logs/artificial_dataset')
    p.add_argument('-nw', '--num_workers', type=int, default=0)
    p.add_argument('-wm', '--width_mult', type=float, default=1.)
    p.add_argument('-en', '--experiment_name', type=str, default="multiple_subjects_64")
    p.add_argument('-me', '--max_epochs', type=int, default=None)
    p.add_argument('-mi', '--max_iterations', type=int, default=4000)
    p.add_argument('-cp', '--checkpoint', type=str, default=None)
    p.add_argument('-rs', '--seed', type=int, default=970205)
    p.add_argument('-es', '--early_stopping', type=int, default=1)
    p.add_argument('-cm', '--compute_metric_every_n_epochs', type=int, default=1)
    p.add_argument('-coms', '--comments', type=str, default="")
    # not in the reference's CLI: the loss variants it keeps as commented code (MultiBoxLoss docstring); default off
    p.add_argument('--hard_negative_mining', action='store_true')
    p.add_argument('--smooth_l1', action='store_true')
    p.add_argument('--focal_loss', action='store_true')
    # not in the reference either: the localisation loss.  l1 is the reference's (mean |.| of encoded offsets); iou / giou / diou
    # score the decoded boxes of the positive priors (MultiBoxLoss.set_loc_loss).  Not with --smooth_l1 (parse_args, loc_loss_of)
    p.add_argument('--loc_loss', choices=["l1", "iou", "giou", "diou"], default=None,
                   help="localisation loss; not given: l1 for a new model, the checkpoint's own kind with -cp "
                        "(given, it replaces the checkpoint's; a checkpoint trained with --smooth_l1 takes l1 only)")
    # build-side extension (the reference trains in fp32): activations and activation gradients stored as bf16
    p.add_argument('--dtype', choices=["f32", "bf16"], default="f32")
    # train.py:51 of the reference (MONAI CacheDataset): 1 = cases normalised once into HBM, every batch augmented and
    # labelled into boxes on the device (devicedata.DeviceCache)
    p.add_argument('-c', '--cache', type=int, default=0)
    # train_lesions() (train.py:191-241 of the reference): the clinical data module instead of the synthetic cubes; -d is its
    # data_dir, -c 1 keeps the cropped cases in HBM (devicedata.LesionCache)
    p.add_argument('-dm', '--data_module', choices=["example", "lesions"], default="example")
    p.add_argument('--centers', type=str, nargs='+', default=['CHUV_RIM_OK', 'BASEL_INSIDER_OK'])
    p.add_argument('--spatial_size', type=int, nargs=3, default=[250, 300, 300], metavar=('D', 'H', 'W'))
    # the MR sequences of a clinical case, one input channel each (1 .. 4); the synthetic cases have one channel
    p.add_argument('-ii', '--input_images', type=str, nargs='+', default=["FLAIR"])
    # the mask of a clinical case: a name with "labeled" in it is instance-labelled, any other name is a binary mask whose
    # 6-connected components are the lesions (the reference's BoundingBoxesGeneratord "binary" mode)
    p.add_argument('--segmentation', type=str, default=DEFAULT_SEGMENTATION, metavar='NAME')
    # patch training (-dm lesions only): one sampled window of this size per case and epoch
    # instead of the fit to --spatial_size, validation on the tiles `predict --views tiles` shows the network
    p.add_argument('--patch_size', type=int, nargs=3, default=None, metavar=('D', 'H', 'W'))
    p.add_argument('--patch_foreground', type=float, default=0.67, metavar='P',
                   help='probability that a training window is placed on a lesion (else uniformly)')
    p.add_argument('--tile_margin', type=int, nargs=3, default=[8, 8, 8], metavar=('D', 'H', 'W'))
    # on_after_backward of the reference (ssd3d.py:729-738: a gradient histogram per parameter every 25 steps), on the
    # device: every N-th step appends one record to LOGDIR/EXPERIMENT/grad_hist.jsonl (mslesions3d_amd.diagnostics prints it)
    p.add_argument('--grad_histograms', type=int, default=0, metavar='N',
                   help='per-parameter gradient / weight histograms every N steps (0: off; the reference logs every 25)')
    return p


def parse_args(argv=None):
    """The command line of this module: ``build_parser().parse_args`` plus the flags that exclude each other, as an
    argparse error (exit status 2)."""
    p = build_parser()
    args = p.parse_args(argv)
    try:
        loc_loss_of(args)
    except ValueError as e:
        p.error(str(e))
    return args


def loc_loss_of(args):
    """The kind named by --loc_loss, or None (not given: a new model trains with l1, a resumed one with its checkpoint's
    kind).  An IoU kind replaces the localisation term, so together with --smooth_l1 it is an error."""
    kind = getattr(args, "loc_loss", None)
    if kind not in (None, "l1") and getattr(args, "smooth_l1", False):
        raise ValueError(f"--loc_loss {kind} replaces the localisation loss: it cannot be combined with --smooth_l1")
    return kind


class GradHistogramLog:
    """``--grad_histograms N``: the steps that start from a ``global_step`` divisible by N run with ``stats=True``, and rank 0
    appends their records to ``grad_hist.jsonl``.  A record is read back at the NEXT logging point (or at ``close``), never
    right after its own step, so the read never waits for the pass it asked for."""

    def __init__(self, every, path):
        self.every, self.path = int(every), path
        self.pending = None  # epoch of the stats step whose record is still on the device

    def wanted(self, global_step):
        return self.every > 0 and global_step % self.every == 0

    def flush(self, trainer):
        if self.pending is None:
            return
        from .diagnostics import to_record
        stats = trainer.last_stats()
        if self.path is not None:
            with open(self.path, "a") as f:
                f.write(json.dumps(to_record(stats, stats["step"], self.pending)) + "\n")
        self.pending = None

    def before_step(self, trainer, global_step, epoch):
        """-> the ``stats`` argument of this step (flushes the previous record first: this step overwrites the snapshot)."""
        if not self.wanted(global_step):
            return False
        self.flush(trainer)
        self.pending = epoch
        return True

    close = flush


def input_images_of(args):
    """The sequences named by -ii; more than one with the synthetic data module is an error (its cases have one channel)."""
    names = tuple(getattr(args, "input_images", None) or ("FLAIR",))
    if getattr(args, "data_module", "example") != "lesions" and len(names) > 1:
        raise ValueError(f"-dm example generates one-channel cases; {len(names)} input images were named: {' '.join(names)}")
    return names


DEFAULT_SEGMENTATION = "labeled_lesions"


def segmentation_of(args):
    """The mask named by --segmentation; another name than the default with the synthetic data module is an error (its
    cases carry class masks of their own)."""
    name = getattr(args, "segmentation", None) or DEFAULT_SEGMENTATION
    if getattr(args, "data_module", "example") != "lesions" and name != DEFAULT_SEGMENTATION:
        raise ValueError(f"--segmentation names the mask of clinical cases: it needs -dm lesions, got {name!r}")
    return name


def patch_options_of(args):
    """--patch_size / --patch_foreground / --tile_margin as LesionsDataModule keywords; {} without --patch_size.  Patch
    training with the synthetic data module is an error (its cubes are the network's input already)."""
    patch = getattr(args, "patch_size", None)
    if patch is None:
        return {}
    if getattr(args, "data_module", "example") != "lesions":
        raise ValueError("--patch_size samples windows of clinical cases: it needs -dm lesions")
    return {"patch_size": tuple(patch), "patch_foreground": getattr(args, "patch_foreground", 0.67),
            "tile_margin": tuple(getattr(args, "tile_margin", (8, 8, 8)))}


def paste_options_of(args, augmentations):
    """-> (the augmentation list with --paste_max_volume bound to its lesionpaste entry, whether it names one).
    lesionpaste with the synthetic data module, or --paste_max_volume without lesionpaste, is an error."""
    volume = getattr(args, "paste_max_volume", None)
    pasting = any(n == "lesionpaste" for n, _ in augmentations)
    if pasting and getattr(args, "data_module", "example") != "lesions":
        raise ValueError("lesionpaste pastes lesions of clinical training cases: it needs -dm lesions")
    if volume is not None and not pasting:
        raise ValueError("--paste_max_volume bounds the lesions lesionpaste copies: name lesionpaste in -a")
    if volume is not None:
        augmentations = [(n, dict(kw, max_volume=volume) if n == "lesionpaste" else kw) for n, kw in augmentations]
    return augmentations, pasting


def check_input_channels(model, input_images, checkpoint):
    """A checkpoint's network reads as many channels as it was trained with: refuse another number of sequences."""
    if int(model.input_channels) != len(input_images):
        raise ValueError(f"{checkpoint} holds a network with input_channels={model.input_channels}, but "
                         f"{len(input_images)} input image(s) were named: {' '.join(input_images)}")


def _dist_env():
    """(world, rank, local rank) of a `python -m torch.distributed.run` launch; (1, 0, 0) for a plain run."""
    return int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))


def dist_barrier():
    import torch.distributed as dist
    dist.barrier()


def _mean_over_ranks(sums, count, device, on):
    """[sum of per-batch values ...] / number of batches, over every rank's validation shard: one all-reduce, so every
    rank holds bit-identical averages (early stopping and checkpoint ranking then need no broadcast)."""
    import torch.distributed as dist
    t = torch.tensor(list(sums) + [float(count)], dtype=torch.float64, device=device)
    if on:
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
    n = max(float(t[-1].item()), 1.0)
    return [float(v) / n for v in t[:-1].tolist()]


def example(args):
    """The reference's ``example()`` (train.py:128-188) as a data-parallel loop: under
    ``python -m torch.distributed.run --nproc-per-node N -m mslesions3d_amd.train ...`` every rank owns one GPU, trains on
    its shard of the cases (``datasets.ShardSampler``; BatchNorm statistics and the loss normaliser per replica), exchanges
    gradients through ``FusedTrainer``'s bucketed RCCL all-reduce overlapped with the backward pass, validates its shard of
    the validation cases, and rank 0 writes metrics and checkpoints.  N = 1 is the reference's single-GPU run."""
    from .datasets import ExampleDataset, LesionsDataModule, select_training_augmentations
    from .ssd3d import LSSD3D
    from .trainer import FusedTrainer
    input_images = input_images_of(args)  # before the first GPU call: a refused command line touches no device
    patch_options = patch_options_of(args)
    segmentation = segmentation_of(args)
    loc_loss = loc_loss_of(args)
    world, rank, local = _dist_env()
    dp = world > 1
    if dp:  # join the job BEFORE the first GPU call of this process (RCCL binds the communicator to the device)
        from .parallel import broadcast_model, init_distributed
        backend = os.environ.get("MSL_DP_BACKEND", "nccl")  # gloo: functional rehearsal with ranks sharing a GPU
        if backend != "nccl":
            local = local % max(torch.cuda.device_count(), 1)
        init_distributed(backend, rank=rank, world_size=world, device=torch.device("cuda", local) if backend == "nccl" else None)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    torch.manual_seed(args.seed)  # same seed on every rank: identical initial weights even before the broadcast
    layers = [int(x) for x in args.prediction_layers.split()]
    aspect_ratios = {l: [1.] for l in layers}
    scales = {int(k): v for k, v in args.scales.items()}
    augmentations = select_training_augmentations(args.augmentations)  # train.py:132-145, :196-205, + the warps
    lesions = getattr(args, "data_module", "example") == "lesions"
    augmentations, pasting = paste_options_of(args, augmentations)
    if lesions:
        dataset = LesionsDataModule(data_dir=args.dataset_path, centers=tuple(args.centers), subject=args.subject,
                                    input_images=input_images, segmentation=segmentation,
                                    classes=("lesion",) if args.n_classes == 1 else ("lesion", "lesion_2"),
                                    percentage=args.percentage, num_workers=args.num_workers, batch_size=args.batch_size,
                                    augmentations=augmentations, random_state=970205,
                                    spatial_size=tuple(args.spatial_size), rank=rank, world_size=world, **patch_options)
    else:
        dataset = ExampleDataset(n_classes=args.n_classes, subject=args.subject, percentage=args.percentage,
                                 num_workers=args.num_workers, batch_size=args.batch_size, data_dir=args.dataset_path,
                                 dataset_name=args.dataset_name, augmentations=augmentations, random_state=970205,
                                 rank=rank, world_size=world)
    dataset.setup(stage="fit")
    input_size = tuple(dataset.train_dataset[0]["img"].shape)[1:]
    threshold = args.threshold if len(args.threshold) > 1 else [args.threshold[0]]
    if args.checkpoint:
        model = LSSD3D.load_from_checkpoint(args.checkpoint)
        check_input_channels(model, input_images, args.checkpoint)
    else:
        model = LSSD3D(n_classes=args.n_classes + 1, input_channels=len(input_images), lr=args.learning_rate, width_mult=args.width_mult,
                       scheduler=args.scheduler, batch_size=args.batch_size, comments=args.comments, input_size=input_size,
                       compute_metric_every_n_epochs=args.compute_metric_every_n_epochs, use_wandb=False,
                       aspect_ratios=aspect_ratios, scales=scales, alpha=args.alpha, threshold=threshold,
                       min_object_size=args.min_object_size, max_object_size=args.max_object_size,
                       base_network_config=args.base_network_config, boxes_per_location=args.boxes_per_location,
                       hard_negative_mining=args.hard_negative_mining, smooth_l1=args.smooth_l1,
                       focal_loss=args.focal_loss)
    if loc_loss is not None:  # given: it replaces the kind a checkpoint carries (ValueError on a smooth_l1 checkpoint)
        model.set_loc_loss(loc_loss)
    model.init()
    model = model.to(dev)
    model.compute_dtype = args.dtype
    if dp:  # rank 0's weights and BatchNorm buffers everywhere (one flat broadcast of the parameter arena)
        model._ensure_device_state(dev)
        model._engine.ensure_arena(dev)
        broadcast_model(model)
    trainer = FusedTrainer(model)
    cache = None
    if args.cache:
        from .devicedata import DeviceCache, LesionCache
        cache = LesionCache(dataset, dev) if lesions else DeviceCache(dataset, dev)
        if rank == 0:
            print(cache.footprint())
    first_epoch = 0
    best, bad_epochs = [], 0
    if args.checkpoint:
        # resume_from_checkpoint (train.py:185): weights above; here the optimiser moments / step count, the scheduler phase,
        # the epoch counter and the loop's own bookkeeping (top-3 list, early-stopping counter).  Shuffle order and
        # augmentation draws are functions of (seed, epoch, subject), so the resumed run sees what the interrupted one would
        # have seen from epoch `epoch + 1` on.  A run continues exactly only from a `last.ckpt` (written every epoch); a
        # top-3 checkpoint restarts from ITS epoch.
        ckpt = LSSD3D.read_checkpoint(args.checkpoint)
        if ckpt.get("optimizer_states"):
            trainer.load_state_dict({"optimizer": ckpt["optimizer_states"][0],
                                     "scheduler": (ckpt.get("lr_schedulers") or [None])[0]})
            first_epoch = int(ckpt.get("epoch", -1)) + 1
        loop = ckpt.get("loop_state") or {}
        best = [(float(v), str(p)) for v, p in loop.get("best", [])]
        bad_epochs = int(loop.get("bad_epochs", 0))
    logdir = pjoin(args.logdir, args.experiment_name)
    log = shard_log = None
    if rank == 0:
        os.makedirs(logdir, exist_ok=True)
        log = open(pjoin(logdir, "metrics.jsonl"), "a")
    # rank 0 alone runs the statistics pass (it reads this rank's arena: the reduced gradient is the same on every rank)
    ghist = GradHistogramLog(args.grad_histograms, pjoin(logdir, "grad_hist.jsonl")) \
        if rank == 0 and getattr(args, "grad_histograms", 0) > 0 else None
    if dp:  # every rank's own shard: which subjects it trained on and what they cost (rank 0's losses are in metrics.jsonl too)
        dist_barrier()
        shard_log = open(pjoin(logdir, f"shard_rank{rank}.jsonl"), "a")
    done = False
    max_epochs = args.max_epochs if args.max_epochs else 10 ** 9
    max_iters = -1 if args.max_epochs else args.max_iterations
    for epoch in range(first_epoch, max_epochs):
        model.current_epoch = epoch
        model.train()
        dataset.set_epoch(epoch)
        # training metrics (ssd3d.py:497-515): detection + mAP on every step's own forward outputs, on the device
        train_metrics = epoch % (2 * max(int(model.compute_metric_every_n_epochs), 1)) == 0
        pastes = [0, 0]  # lesionpaste on the host route: rows tested / accepted in this rank's samples of the epoch
        for batch in (cache.train_batches(epoch) if cache else dataset.train_dataloader()):
            if pasting and not cache:
                flat = [v for report in batch["paste_report"] for v in report]
                pastes = [pastes[0] + sum(v > -2 for v in flat), pastes[1] + sum(v >= 0 for v in flat)]
            stats = ghist.before_step(trainer, model.global_step, epoch) if ghist is not None else False
            if cache:
                out = cache.step(trainer, batch, metrics=train_metrics, stats=stats)
            else:
                out = trainer.step(batch["img"].to(dev), batch["boxes"], batch["labels"], metrics=train_metrics, stats=stats)
            if shard_log is not None:
                shard_log.write(json.dumps({"step": model.global_step, "epoch": epoch, "subjects": list(batch["subject"]),
                                            "total_loss/training": out["loss"]}) + "\n")
            if log is not None:  # rank 0's shard losses (the reference logs one process's batch)
                log.write(json.dumps({"step": model.global_step, "epoch": epoch, "total_loss/training": out["loss"],
                                      "confidence_loss/training": out["conf"], "localization_loss/training": out["loc"],
                                      "hp_metric/lr": trainer.sch.get_last_lr()[1] if trainer.sch else model.lr}) + "\n")
            if 0 < max_iters <= model.global_step:
                done = True
                break
        if trainer.sch is not None:
            # Lightning steps a scheduler returned by configure_optimizers once per epoch (interval="epoch") on top of
            # the manual per-step call inside training_step: one extra cosine step per epoch
            trainer.sch.step()
        if pasting:  # the device route keeps its counters in HBM: one read per epoch
            asked, accepted = cache.paste_counts() if cache else pastes
            if log is not None:
                log.write(json.dumps({"step": model.global_step, "epoch": epoch, "lesionpaste/asked": asked,
                                      "lesionpaste/accepted": accepted}) + "\n")
                print(f"epoch {epoch}: lesionpaste accepted {accepted} of {asked} pastes")
        if train_metrics:
            # training_epoch_end (ssd3d.py:657-690): epoch means of the per-step values, summed over every rank's steps
            # (the vector length depends on the epoch alone, so every rank joins the same all-reduce)
            msums, msteps = trainer.metric_sums(reset=True)
            mavg = _mean_over_ranks(msums, msteps, dev, dp)
            mrec = {"step": model.global_step, "epoch": epoch}
            for i, tag in enumerate(("0.1", "0.5")):
                for k, name in enumerate(("mAP", "precision", "recall", "f1_score")):
                    mrec[f"{name}/training_IoU_{tag}"] = mavg[4 * i + k]
            mrec["hp_metric/parameter_sizes"] = float(model.compute_parameters_median_size())
            if rank == 0:
                log.write(json.dumps(mrec) + "\n")
        model.eval()
        vals = [model.validation_step(b, i) for i, b in enumerate(cache.val_batches() if cache else dataset.test_dataloader())]
        keys = ("val_total_loss", "val_conf_loss", "val_loc_loss")
        sums = [float(sum(float(v["log"][k]) for v in vals)) for k in keys]
        # (decided from the epoch, not from this rank's batches: every rank must contribute a vector of the same length)
        with_metrics = epoch % max(int(model.compute_metric_every_n_epochs), 1) == 0 and all("metrics_50" in v["log"] for v in vals)
        mkeys = [(tag, key, m) for tag, key in (("0.1", "metrics_10"), ("0.5", "metrics_50"))
                 for m in ("mAP", "precision", "recall", "f1_score")] if with_metrics else []
        sums += [float(sum(float(v["log"][key][m]) for v in vals)) for _, key, m in mkeys]
        avg = _mean_over_ranks(sums, len(vals), dev, dp)
        rec = {"step": model.global_step, "epoch": epoch, "avg_val_loss": avg[0],
               "total_loss/validation": avg[0], "confidence_loss/validation": avg[1],
               "localization_loss/validation": avg[2]}
        for (tag, _, m), v in zip(mkeys, avg[3:]):
            rec[f"{m}/validation_IoU_{tag}"] = v
        # ModelCheckpoint(monitor="avg_val_loss", save_top_k=3, mode="min")  (train.py:171-176); every rank ranks the same
        # all-reduced value, rank 0 touches the files
        path = pjoin(logdir, f"checkpoint-epoch={epoch:03d}-avg_val_loss={rec['avg_val_loss']:.4f}.ckpt")
        best.append((rec["avg_val_loss"], path))
        best.sort()
        keep, drop = best[:3], best[3:]
        # EarlyStopping('total_loss/validation', patience=5)  (train.py:180)
        bad_epochs = 0 if rec["avg_val_loss"] <= keep[0][0] else bad_epochs + 1
        loop_state = {"best": [[v, p] for v, p in keep], "bad_epochs": bad_epochs}
        if rank == 0:
            log.write(json.dumps(rec) + "\n")
            log.flush()
            print(rec)
            if (rec["avg_val_loss"], path) in keep:
                model.save_checkpoint(path, trainer, loop_state=loop_state)
            model.save_checkpoint(pjoin(logdir, "last.ckpt"), trainer, loop_state=loop_state)  # exact continuation point
            for _, p in drop:
                if os.path.exists(p):
                    os.remove(p)
        best = keep
        if done or (args.early_stopping and bad_epochs >= 5):
            break
    if ghist is not None:
        ghist.close(trainer)
    if log is not None:
        log.close()
    if shard_log is not None:
        shard_log.close()
    if dp:
        import torch.distributed as dist
        if os.environ.get("MSL_DP_CHECK_REPLICAS", "1") == "1":  # the data-parallel invariant, once, at the end of the run
            flat = model._engine.arena.flat
            ref = flat.detach().clone()
            dist.broadcast(ref, src=0)
            same = torch.tensor([1.0 if torch.equal(ref, flat) else 0.0], device=dev)
            dist.all_reduce(same, op=dist.ReduceOp.MIN)
            if float(same.item()) != 1.0:
                raise RuntimeError("data-parallel replicas diverged: the gradient all-reduce is not reaching every parameter")
        dist.barrier()
        dist.destroy_process_group()
    return model


if __name__ == "__main__":
    example(parse_args())
