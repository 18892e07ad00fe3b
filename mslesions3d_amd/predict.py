"""Prediction entry point — flags of the reference's ``lesions3d/predict.py:29-44`` and the flow of
``predict_example`` (``predict.py:235-281``): load checkpoint -> predict every subject -> write
``sub-XXXX_preds.json`` (``{j+1: [box_frac(6), box_voxel(6), label, score]}``, ``predict.py:149,222-232``) and
``sub-XXXX_preds.csv`` (``label_id,score``) -> per-subject mAP at IoU 0.5 and 0.1 (``predict.py:87-152``).
With ``-si 1`` the box overlay the reference saves as ``sub-XXXX_preds.nii.gz`` (``predict.py:176-226``) is written as
``sub-XXXX_preds.npy`` (int16; NIfTI is out of scope).  For clinical cases (``-dm lesions``) the overlay
is drawn in the CASE's own frame, and ``sub-XXXX_preds_case.json`` holds the detections in that frame
(``datasets.fit_to_case_frame``); ``--cache 1`` prepares the cases on the device (``devicedata.LesionPredictFeed``) and
maps and draws there too (msl_boxes_to_case, msl_draw_boxes).  DESIGN.md §4.9.  A case that carries an affine was put on
the LPI 1 mm grid first (``datasets.regrid_plan``): its ``_preds_case.json`` gains a ``"native"`` block with the boxes on
the stored grid (``datasets.regrid_to_native``) and ``-si 1`` also writes ``sub-XXXX_preds_native.npy`` at the stored
shape.  DESIGN.md §4.10.  ``--views tiles`` and / or ``--flip_views AXES`` show the network several views of every case
(tiles of the input size where the case is larger, mirrored copies) and merge their detections in the case's own frame
(``LSSD3D.predict_views``; ``sub-XXXX_preds_views.json`` records the views and every detection's support).  DESIGN.md §4.11.

    python -m mslesions3d_amd.predict -d DATA -dn NAME -m CKPT -o OUT
    python -m mslesions3d_amd.predict -dm lesions -d RAW -m CKPT -o OUT --cache 1 -si 1
    python -m mslesions3d_amd.predict -dm lesions -d RAW -m CKPT -o OUT --cache 1 --views tiles --flip_views 2 --merge fuse
"""
import argparse
import json
import collections
import os
import warnings
from os.path import join as pjoin

import numpy as np
import torch


def build_parser():
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('-d', '--dataset_path', type=str, default=r'../data/artificial_dataset')
    p.add_argument('-dn', '--dataset_name', type=str, default=None)
    p.add_argument('-m', '--model_path', type=str, default=r'model_final.ckpt')
    p.add_argument('-p', '--percentage', type=float, default=1.)
    p.add_argument('-su', '--subject', type=str, default=None)
    p.add_argument('-c', '--n_classes', type=int, default=1)
    p.add_argument('-nw', '--num_workers', type=int, default=0)
    p.add_argument('-ps', '--predict_subset', type=str, choices=['train', 'validation', 'test', 'all'], default='train')
    p.add_argument('-sc', '--min_score', type=float, default=0.5)
    p.add_argument('-k', '--top_k', type=int, default=100)
    p.add_argument('-o', '--output_dir', type=str, default=r"../data/predictions/")
    # not in the reference's CLI: bf16 activations for the eval forward (fp32 is the reference's precision)
    p.add_argument('--dtype', type=str, choices=['f32', 'bf16'], default='f32')
    # the clinical data module (datasets.LesionsDataModule): -d is its data_dir; files are named <center>_<subject>
    p.add_argument('-dm', '--data_module', choices=["example", "lesions"], default="example")
    p.add_argument('--centers', type=str, nargs='+', default=['CHUV_RIM_OK', 'BASEL_INSIDER_OK'])
    p.add_argument('--spatial_size', type=int, nargs=3, default=[250, 300, 300], metavar=('D', 'H', 'W'))
    # the MR sequences of a clinical case, one input channel each: the ones the checkpoint was trained with, in order
    p.add_argument('-ii', '--input_images', type=str, nargs='+', default=["FLAIR"])
    p.add_argument('-mn', '--model_name', type=str, default=None, help="sub-directory of the output path (predict.py:241)")
    p.add_argument('-si', '--save_images', type=int, default=0,
                   help="1: write the box overlay of every subject as sub-XXXX_preds.npy (with -dm lesions in the case's own "
                        "frame, plus sub-XXXX_preds_case.json; for a case with an affine also sub-XXXX_preds_native.npy at "
                        "the stored shape).  The reference's default is 1; it is 0 here so that no "
                        "existing command starts writing volumes")
    # the reference's (and this parser's) -c is --n_classes, so the device feed has the long spelling only
    p.add_argument('--cache', type=int, default=0,
                   help="with -dm lesions, 1: prepare every case on the device (devicedata.LesionPredictFeed) and map and "
                        "draw the overlays there; ignored with a warning for the example module")
    # multi-view prediction (not in the reference).  A flag that is not given leaves NO attribute behind (SUPPRESS), so the
    # namespace of a command without them is the one every caller of the single-view route has always seen; the route
    # reads them through view_options(), where the defaults (VIEW_DEFAULTS) live
    S = argparse.SUPPRESS
    p.add_argument('--segmentation', type=str, default=S, metavar='NAME',
                   help="the mask of a clinical case, as train.py: a name without 'labeled' in it is a binary mask "
                        "(default: labeled_lesions)")
    p.add_argument('--views', choices=["fit", "tiles"], default=S,
                   help="tiles: a case larger than the input size is covered by overlapping tiles instead of being "
                        "centre-cropped; their detections are merged in the case's own frame (default: fit)")
    p.add_argument('--tile_margin', type=int, nargs=3, default=S, metavar=('D', 'H', 'W'),
                   help="a tile owns the detections centred at least this far inside it; neighbours overlap by twice this "
                        "(default: 8 8 8)")
    p.add_argument('--flip_views', type=int, nargs='*', default=S, metavar='AXIS',
                   help="flip test-time augmentation: every view is also shown mirrored along each subset of these axes "
                        "(default: none)")
    p.add_argument('--merge', choices=["nms", "fuse"], default=S,
                   help="how overlapping detections of several views become one: the best one, or their score-weighted mean "
                        "(default: nms)")
    p.add_argument('--view_batch', type=int, default=S, help="views per forward pass of the multi-view route (default: 2)")
    return p


VIEW_DEFAULTS = {"views": "fit", "tile_margin": (8, 8, 8), "flip_views": (), "merge": "nms", "view_batch": 2}


def view_options(args):
    """The multi-view flags of a namespace with their defaults filled in -> a namespace of exactly those five."""
    return argparse.Namespace(**{k: (d if getattr(args, k, None) is None else getattr(args, k))
                                 for k, d in VIEW_DEFAULTS.items()})


def multi_view(args):
    """--views tiles or a non-empty --flip_views select the multi-view route."""
    o = view_options(args)
    return o.views == "tiles" or bool(o.flip_views)


def views_of(case_shape, tile, args):
    """The view table of one case: ``datasets.view_plan`` for --views tiles; for the fitted view, that one window with
    its mirrored copies."""
    from .datasets import fit_shift, view_plan
    args = view_options(args)
    flips = tuple(args.flip_views)
    if args.views == "tiles":
        return view_plan(case_shape, tile, tuple(args.tile_margin), flips)
    views = view_plan(tile, tile, (0, 0, 0), flips)
    views[:, :3] = [fit_shift(int(n), int(t)) for n, t in zip(case_shape, tile)]
    return views


def merge_margin(args):
    """--tile_margin between tiles; the fitted window and its mirrored copies own all of the window."""
    args = view_options(args)
    return tuple(args.tile_margin) if args.views == "tiles" else (0, 0, 0)


def predict_case_views(model, case, views, args, on_device):
    """One case through the multi-view route -> (boxes, labels, scores, support) tensors in the case's frame.
    ``on_device``: ``LSSD3D.predict_views`` (msl_view_gather, msl_views_merge); else their host twins around
    ``predict_step``: ``gather_views``, the views ``--view_batch`` at a time (the last chunk filled up with the last view,
    as on the device), ``merge_views``.  Both give the same bits."""
    margin, args = merge_margin(args), view_options(args)
    vb = max(1, int(args.view_batch))
    if on_device:
        return model.predict_views(case.to(model.device), views, margin, merge=args.merge, view_batch=vb)
    from .datasets import gather_views
    from .utils import merge_views
    tile, V, k = tuple(model.input_size), views.shape[0], int(model.top_k)
    x = gather_views(case.numpy(), views, tile)
    x = np.concatenate([x, np.repeat(x[-1:], -V % vb, axis=0)])
    boxes, scores = np.zeros((V, k, 6), np.float32), np.zeros((V, k), np.float32)
    labels, counts = np.zeros((V, k), np.int64), np.zeros(V, np.int32)
    for v0 in range(0, V, vb):
        b, l, s = model.predict_step({"img": torch.from_numpy(x[v0:v0 + vb])})
        for i in range(min(vb, V - v0)):
            n = counts[v0 + i] = b[i].shape[0]
            boxes[v0 + i, :n], labels[v0 + i, :n], scores[v0 + i, :n] = b[i].cpu().numpy(), l[i].cpu().numpy(), s[i].cpu().numpy()
    out = merge_views(boxes, scores, labels, counts, views, tile, case.shape[1:], margin, model.max_overlap, args.merge, k)
    if out[0].shape[0] == 0:  # ssd3d.py:437-440
        out = (np.asarray([[0, 0, 0, 1, 1, 1]], np.float32), np.zeros(1, np.int64), np.zeros(1, np.float32), np.zeros(1, np.int32))
    return tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in out)


def output_dir_of(args):
    """predict.py:240-241: the model's name, when given, is a sub-directory of the output path."""
    name = getattr(args, "model_name", None)
    return args.output_dir if name is None else pjoin(args.output_dir, name)


def prediction_infos(boxes, labels, scores, min_score, img_shape):
    """``{j + 1: (box_frac(6), box_voxel(6), label, score)}`` of the detections the reference keeps (predict.py:186-222)."""
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 6)
    scores = np.asarray(scores, dtype=np.float32).reshape(-1)
    shape2 = np.asarray(tuple(img_shape) * 2, dtype=np.float32)
    infos = {}
    for j in range(boxes.shape[0]):
        score = float(scores[j])
        if score < min_score or int(labels[j]) == 0:
            continue
        frac = [float(v) for v in boxes[j]]
        vox = (np.clip(boxes[j], np.float32(0), np.float32(1)) * shape2).astype(int).tolist()
        infos[j + 1] = (frac, vox, int(labels[j]), score)
    return infos


def save_case_predictions(subject, record, target, min_score, output_dir):
    """``sub-XXXX_preds_case.json``: the schema of ``sub-XXXX_preds.json`` with the boxes in the case's own frame -
    ``fit_to_case_frame`` of the fitted-frame boxes, fractional and as voxels of ``full_shape``.  For a case that had an
    affine (``record["plan"]``) the case frame is the regridded one and the file gains
    ``"native": {"shape": stored shape, "boxes": [box_frac(6) of every kept detection, in key order]}``, the case-frame
    boxes mapped on to the stored grid by ``regrid_to_native``."""
    from .datasets import fit_to_case_frame, regrid_to_native
    case = fit_to_case_frame(np.asarray(record["boxes"], np.float32), target, record["crop_shape"], record["crop_origin"],
                             record["full_shape"])
    infos = prediction_infos(case, record["labels"], record["scores"], min_score, record["full_shape"])
    plan = record.get("plan")
    if plan is not None:
        native = regrid_to_native(case, plan)
        infos["native"] = {"shape": [int(n) for n in plan.src_shape],
                           "boxes": [[float(v) for v in native[j - 1]] for j in list(infos)]}
    with open(pjoin(output_dir, f"sub-{subject}_preds_case.json"), "w") as f:
        json.dump(infos, f)


def save_predictions(subject, img_shape, boxes, labels, scores, min_score, output_dir):
    """predict.py:155-232 without the NIfTI overlay; file contents byte-identical to the reference's on the same detections
    (tests/golden/preds/*): the voxel box is the fp32 product ``clip(box, 0, 1) * shape`` truncated to int, and the CSV's
    score column holds what pandas prints for the 0-dim tensors the reference stores there (``tensor(0.9700)``)."""
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 6)
    scores = np.asarray(scores, dtype=np.float32).reshape(-1)
    shape2 = np.asarray(tuple(img_shape) * 2, dtype=np.float32)
    infos, scores_map = {}, []
    for j in range(boxes.shape[0]):
        score = float(scores[j])
        scores_map.append((j + 1, scores[j]))
        if score < min_score or int(labels[j]) == 0:
            continue
        frac = [float(v) for v in boxes[j]]
        vox = (np.clip(boxes[j], np.float32(0), np.float32(1)) * shape2).astype(int).tolist()
        infos[j + 1] = (frac, vox, int(labels[j]), score)
    with open(pjoin(output_dir, f"sub-{subject}_preds.json"), "w") as f:
        json.dump(infos, f)
    with open(pjoin(output_dir, f"sub-{subject}_preds.csv"), "w") as f:
        f.write(",label_id,score\n")
        for i, (lid, sc) in enumerate(scores_map):
            f.write(f"{i},{lid},{str(torch.tensor(sc))}\n")


def gather_detections(records, world, rank):
    """SURVEY section 8(e), inference: replicas only - every rank predicts its share of the subjects, no collective on the
    data path; the per-subject detections (a few KB of plain lists each) are gathered on rank 0 for the metrics.
    ``records``: list of (position in the data set, subject, record dict).  Returns the merged list in data-set order on rank 0,
    None elsewhere."""
    if world == 1:
        return sorted(records, key=lambda r: r[0])
    import torch.distributed as dist
    bucket = [None] * world if rank == 0 else None
    dist.gather_object(records, bucket, dst=0)
    if rank != 0:
        return None
    seen, merged = set(), []
    for part in bucket:
        for rec in part:
            if rec[0] not in seen:  # (the wrap-around padding of the shards predicts a few subjects twice)
                seen.add(rec[0])
                merged.append(rec)
    return sorted(merged, key=lambda r: r[0])


def predict_example(args):
    """predict.py:235-281.  Under ``python -m torch.distributed.run --nproc-per-node N -m mslesions3d_amd.predict ...`` the
    subjects are dealt round-robin over N replicas (one GPU each) and rank 0 writes the files and the metrics."""
    from .datasets import ExampleDataset, LesionsDataModule, ShardSampler
    from .ssd3d import LSSD3D
    from .train import check_input_channels, input_images_of, segmentation_of
    from .utils import calculate_mAP
    input_images = input_images_of(args)
    segmentation = segmentation_of(args)
    world, rank, local = (int(os.environ.get(k, d)) for k, d in (("WORLD_SIZE", "1"), ("RANK", "0"), ("LOCAL_RANK", "0")))
    if world > 1:
        from .parallel import init_distributed
        backend = os.environ.get("MSL_DP_BACKEND", "nccl")
        if backend != "nccl":
            local = local % max(torch.cuda.device_count(), 1)
        init_distributed(backend, rank=rank, world_size=world, device=torch.device("cuda", local) if backend == "nccl" else None)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    output_dir = output_dir_of(args)
    save_images = bool(getattr(args, "save_images", 0))
    if rank == 0 or save_images:  # (every rank writes the overlays of its own subjects)
        os.makedirs(output_dir, exist_ok=True)
    lesions = getattr(args, "data_module", "example") == "lesions"
    cache = bool(getattr(args, "cache", 0))
    if cache and not lesions and not multi_view(args):
        warnings.warn("--cache 1 prepares clinical cases on the device (-dm lesions); ignored for the example module")
        cache = False
    if lesions:
        dataset = LesionsDataModule(data_dir=args.dataset_path, centers=tuple(args.centers), batch_size=1,
                                    input_images=input_images, segmentation=segmentation,
                                    classes=("lesion",) if args.n_classes == 1 else ("lesion", "lesion_2"),
                                    num_workers=args.num_workers, subject=args.subject, percentage=args.percentage,
                                    spatial_size=tuple(args.spatial_size))
    else:
        dataset = ExampleDataset(n_classes=args.n_classes, batch_size=1, num_workers=args.num_workers, subject=args.subject,
                                 percentage=args.percentage, data_dir=args.dataset_path, dataset_name=args.dataset_name)
    dataset.setup(stage="predict_train" if args.predict_subset == "train" else "predict")
    model = LSSD3D.load_from_checkpoint(args.model_path, min_score=args.min_score)
    if lesions:
        check_input_channels(model, input_images, args.model_path)
    model = model.to(dev).eval()
    model.top_k, model.min_score = args.top_k, args.min_score  # predict.py:259-260
    model.compute_dtype = getattr(args, "dtype", "f32")
    ds = dataset.predict_dataset
    mine = ShardSampler(len(ds), rank, world, shuffle=False).indices().tolist()
    records = []
    queued = collections.deque()  # (position, batch) of the passes in flight: predict_batches yields results in order

    def feed():
        if cache:  # cropped, normalised and fitted on the device, one case ahead of the pass
            from .devicedata import LesionPredictFeed
            source = zip(mine, LesionPredictFeed(dataset, dev).batches(mine))
        else:
            source = ((pos, collate([ds[pos]])) for pos in mine)
        for pos, batch in source:
            # (the device feed reuses its image buffer: only what the records need is kept)
            queued.append((pos, {k: (tuple(v.shape[2:]) if k == "img" else v) for k, v in batch.items() if k != "seg"}))
            yield batch

    multi = multi_view(args)
    tile = tuple(model.input_size)
    if multi and lesions and tuple(args.spatial_size) != tile:
        raise ValueError(f"--spatial_size {tuple(args.spatial_size)} is the tile of the multi-view route: it must be the "
                         f"checkpoint's input size {tile}")
    for pos in (mine if multi else ()):
        # the case frame: the image itself (example module) or the normalised foreground crop, not fitted (lesions)
        batch = collate([ds.case_sample(pos) if lesions else ds[pos]])
        case = batch["img"][0].float()
        views = views_of(tuple(case.shape[1:]), tile, args)
        boxes, labels, scores, support = predict_case_views(model, case, views, args, on_device=cache)
        subj = batch["subject"][0]
        subj = subj if isinstance(subj, str) else "_".join(subj)
        rec = {"shape": tuple(case.shape[1:]), "boxes": boxes.cpu().numpy().tolist(), "labels": labels.cpu().numpy().tolist(),
               "scores": scores.cpu().numpy().tolist(), "gt_boxes": batch["boxes"][0].numpy().tolist(),
               "gt_labels": batch["labels"][0].numpy().tolist(),
               "views": {"views": views.tolist(), "tile": list(tile), "margin": list(merge_margin(args)), "merge": view_options(args).merge,
                         "support": support.cpu().numpy().tolist()}}
        if lesions:
            rec.update({k: tuple(batch[k][0]) for k in ("crop_origin", "crop_shape", "full_shape")})
            plan = ds.native_plan(pos)
            if plan is not None:
                rec["plan"] = plan
        if save_images:  # the case frame IS the crop: fit_to_case_frame with target = crop_shape has d = 0
            on_dev = boxes.is_cuda
            np.save(pjoin(output_dir, f"sub-{subj}_preds.npy"),
                    overlay_volume(rec, boxes, labels, scores, rec["crop_shape"] if lesions else None, args.min_score,
                                   on_device=on_dev))
            if "plan" in rec:
                np.save(pjoin(output_dir, f"sub-{subj}_preds_native.npy"),
                        overlay_volume(rec, boxes, labels, scores, rec["crop_shape"], args.min_score, on_device=on_dev,
                                       native=True))
        records.append((pos, subj, rec))
    for boxes, labels, scores in model.predict_batches(feed() if not multi else (), depth=2):
        pos, batch = queued.popleft()
        subj = batch["subject"][0]
        subj = subj if isinstance(subj, str) else "_".join(subj)
        rec = {"shape": batch["img"], "boxes": boxes[0].cpu().numpy().tolist(),
               "labels": labels[0].cpu().numpy().tolist(), "scores": scores[0].cpu().numpy().tolist(),
               "gt_boxes": batch["boxes"][0].numpy().tolist(), "gt_labels": batch["labels"][0].numpy().tolist()}
        if lesions:
            rec.update({k: tuple(batch[k][0]) for k in ("crop_origin", "crop_shape", "full_shape")})
            # the plan the case was regridded with: the device feed hands it out, the host data set kept it at the load
            plan = batch["plan"][0] if "plan" in batch else (None if cache else ds.native_plan(pos))
            if plan is not None:
                rec["plan"] = plan
        if save_images:
            np.save(pjoin(output_dir, f"sub-{subj}_preds.npy"),
                    overlay_volume(rec, boxes[0], labels[0], scores[0], tuple(args.spatial_size) if lesions else None,
                                   args.min_score, on_device=cache))
            if "plan" in rec:
                np.save(pjoin(output_dir, f"sub-{subj}_preds_native.npy"),
                        overlay_volume(rec, boxes[0], labels[0], scores[0], tuple(args.spatial_size), args.min_score,
                                       on_device=cache, native=True))
        records.append((pos, subj, rec))
    merged = gather_detections(records, world, rank)
    metrics = {"0.5": {}, "0.1": {}}
    if merged is not None:
        for _, subj, r in merged:
            save_predictions(subj, r["shape"], np.asarray(r["boxes"], np.float32), np.asarray(r["labels"]),
                             np.asarray(r["scores"], np.float32), args.min_score, output_dir)
            if save_images and lesions:
                save_case_predictions(subj, r, r["crop_shape"] if multi else tuple(args.spatial_size), args.min_score, output_dir)
            if multi:
                with open(pjoin(output_dir, f"sub-{subj}_preds_views.json"), "w") as f:
                    json.dump(r["views"], f)
            det_b = [torch.tensor(r["boxes"], dtype=torch.float32).reshape(-1, 6)]
            det_l = [torch.tensor(r["labels"], dtype=torch.long)]
            det_s = [torch.tensor(r["scores"], dtype=torch.float32)]
            gt_b = [torch.tensor(r["gt_boxes"], dtype=torch.float32).reshape(-1, 6)]
            gt_l = [torch.tensor(r["gt_labels"], dtype=torch.long)]
            dif = [torch.zeros(len(l), dtype=torch.bool) for l in gt_l]
            for iou in (0.5, 0.1):
                d = calculate_mAP(det_b, det_l, det_s, gt_b, gt_l, dif, min_overlap=iou, return_detail=True)
                metrics[str(iou)][subj] = {k: float(d[k]) for k in ("mAP", "precision", "recall", "f1_score")}
        for iou, m in metrics.items():
            with open(pjoin(output_dir, f"aa_metrics_per_subject_(min_IoU={iou}).json"), "w") as f:
                json.dump(m, f, indent=4)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    return metrics


def overlay_volume(rec, boxes, labels, scores, target, min_score, on_device=False, native=False):
    """The "preds"-style instance volume of one subject (``utils.draw_boxes``), int16 on the host.  ``target`` None: in
    the image's own frame (the example module; what the reference's NIfTI holds).  Otherwise the boxes are fractions of
    the fitted ``target`` volume of a clinical case and the volume is drawn in the case's own frame at ``full_shape``:
    on the host by ``fit_to_case_frame`` + ``draw_boxes``, or with ``on_device`` by msl_boxes_to_case + msl_draw_boxes on
    the detections where ``predict_batches`` left them, behind the pass on its stream, and read back once.  ``native``
    (a case that had an affine, ``rec["plan"]``): the case-frame boxes are mapped on to the stored grid by
    ``regrid_to_native`` (host f64 on both routes) and drawn at the stored shape, by the same two drawing routes."""
    from .utils import draw_boxes, draw_boxes_device
    if target is None:
        return draw_boxes(boxes.cpu(), labels.cpu(), scores.cpu(), rec["shape"], "preds", min_score)[0]
    shape = tuple(rec["plan"].src_shape) if native else rec["full_shape"]
    if not on_device:
        from .datasets import fit_to_case_frame, regrid_to_native
        case = fit_to_case_frame(boxes.cpu().numpy(), target, rec["crop_shape"], rec["crop_origin"], rec["full_shape"])
        if native:
            case = regrid_to_native(case, rec["plan"])
        return draw_boxes(case, labels.cpu(), scores.cpu(), shape, "preds", min_score)[0]
    from .devicedata import boxes_to_case_device
    case = boxes_to_case_device(boxes, target, rec["crop_shape"], rec["crop_origin"], rec["full_shape"])
    if native:
        from .datasets import regrid_to_native
        case = torch.from_numpy(regrid_to_native(case.cpu().numpy(), rec["plan"])).to(case.device)
    inst, _ = draw_boxes_device(case, labels, scores, shape, "preds", min_score, classes=False)
    return inst[0].cpu().numpy()


def collate(samples):
    from .datasets import collate_fn
    return collate_fn(samples)


if __name__ == "__main__":
    predict_example(build_parser().parse_args())
