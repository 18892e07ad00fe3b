"""Evaluation entry point — flags of the reference's ``lesions3d/eval.py:17-36`` and the flow of its ``evaluate``
(``eval.py:61-151``): read back the ``sub-XXXX_preds.json`` files that ``predict`` wrote at min_score 0.0, keep the
detections at or above ``-sc``, compute one dataset-level ``calculate_mAP`` at ``-iou`` and write
``metrics_(min_IoU=<iou>_min_score=<score>).json`` next to the predictions (the files the reference's ``plots.py`` reads).

One extension: ``-sc`` and ``-iou`` take comma-separated lists; the whole grid comes from one device sweep
(``utils.evaluate_detections``), every grid point bit-identical to the host ``calculate_mAP`` on the filtered detections.

    python -m mslesions3d_amd.eval -d DATA -dn NAME -pd PREDICTIONS -sc 0.1,0.5 -iou 0.1,0.5

Not in the reference: ``--froc`` adds the FROC curve of ALL predictions in the files (sensitivity at ``--froc_rates`` false
positives per case, their mean CPM, ``--bootstrap R`` resamples of the cases for a 95 % interval; DESIGN.md "FROC") as
``froc_(min_IoU=<iou>).json`` per ``-iou``; ``-dm lesions`` scores the predictions of clinical cases
(``datasets.LesionsDataModule``) in the frame ``predict`` wrote them in.

    python -m mslesions3d_amd.eval -dm lesions -d RAW --centers C1 C2 --spatial_size 96 96 96 -pd PREDICTIONS --froc --bootstrap 1000

``--size_bins 27,125,1000`` (ascending bounding-box volumes in voxels of the frame the boxes are fractions of; mm3 at 1 mm)
adds ``strata_(min_IoU=<iou>).json`` per ``-iou``: lesions, sensitivity and false positives per case in every size bin, at
each ``-sc`` threshold and, with ``--froc``, at each FROC rate, with ``--bootstrap`` intervals (DESIGN.md "Eval by lesion
size").

``--ignore_below V`` scores the way lesion-detection studies do: a ground-truth lesion whose size
(what ``--size_bins`` measures: f32 bounding-box volume times the voxels of its image) is below ``V`` is neither hit nor
miss - missing it is no false negative, a detection on it no false positive.  It applies to the grid, ``--froc``,
``--bootstrap`` and ``--size_bins`` (a bin wholly below ``V`` is reported empty); every output file gains an ``"ignored"``
block.  Without the flag the files are what they have always been.

    python -m mslesions3d_amd.eval -dm lesions -d RAW -pd PREDICTIONS --froc --size_bins 27,125,1000 --ignore_below 3
"""
import argparse
import json
import os
from os.path import join as pjoin

import torch

BATCH = 32  # eval.py:79


def float_list(text):
    """``0.5`` -> [0.5]; ``0.1,0.5`` -> [0.1, 0.5] (each entry parsed by ``float`` as the reference's flag is)."""
    vals = [float(v) for v in str(text).split(",") if v.strip() != ""]
    if not vals:
        raise argparse.ArgumentTypeError(f"expected one or more comma-separated numbers, got {text!r}")
    return vals


def build_parser():
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('-d', '--dataset_path', type=str, default=r'../data/artificial_dataset')
    p.add_argument('-dn', '--dataset_name', type=str, default=None)
    p.add_argument('-mn', '--model_name', type=str, default=None)
    p.add_argument('-p', '--percentage', type=float, default=1.)
    p.add_argument('-c', '--n_classes', type=int, default=1)
    p.add_argument('-nw', '--num_workers', type=int, default=8)
    p.add_argument('-ps', '--predict_subset', type=str, choices=['train', 'validation', 'test', 'all'], default=r'train')
    p.add_argument('-sc', '--min_score', type=float_list, default=0.5,
                   help="minimum score(s) for a candidate box to be kept; comma-separated list for a sweep")
    p.add_argument('-iou', '--min_iou', type=float_list, default=0.5,
                   help="minimum overlap(s) between a candidate box and a ground-truth box; comma-separated list for a sweep")
    p.add_argument('-k', '--top_k', type=int, default=100)
    p.add_argument('-pd', '--prediction_dir', type=str, default=r"../data/predictions/")
    # not in the reference.  A flag that is not given leaves NO attribute behind (SUPPRESS, as predict.view_options): the
    # namespace of a command without them is the one it has always been; eval_options() fills in the defaults
    S = argparse.SUPPRESS
    p.add_argument('--froc', action="store_true", default=S,
                   help="also write froc_(min_IoU=<iou>).json: sensitivity at fixed false positives per case, CPM")
    p.add_argument('--froc_rates', type=rate_list, default=S,
                   help="false positives per case of the FROC curve, comma-separated exact rationals (default: "
                        "0.125,0.25,0.5,1,2,4,8)")
    p.add_argument('--bootstrap', type=int, default=S, help="bootstrap resamples of the cases for the 95 %% interval (default: 0)")
    p.add_argument('--bootstrap_seed', type=int, default=S, help="seed of the resampling (default: 0)")
    p.add_argument('--size_bins', type=size_bin_list, default=S,
                   help="also write strata_(min_IoU=<iou>).json: sensitivity and false positives per case by lesion size; "
                        "comma-separated ascending bounding-box volumes in voxels, e.g. 27,125,1000")
    p.add_argument('--ignore_below', type=ignore_size, default=S, metavar='V',
                   help="ground-truth lesions smaller than V (bounding-box volume in voxels, as --size_bins) are neither "
                        "hit nor miss; every output file gains an \"ignored\" block")
    p.add_argument('-dm', '--data_module', choices=["example", "lesions"], default=S,
                   help="lesions: the clinical data module, -d is its data_dir (default: example)")
    p.add_argument('--centers', type=str, nargs='+', default=S, help="as predict.py (default: CHUV_RIM_OK BASEL_INSIDER_OK)")
    p.add_argument('--spatial_size', type=int, nargs=3, default=S, metavar=('D', 'H', 'W'),
                   help="as predict.py (default: 250 300 300)")
    p.add_argument('-ii', '--input_images', type=str, nargs='+', default=S, help="as predict.py (default: FLAIR)")
    p.add_argument('--segmentation', type=str, default=S, metavar='NAME', help="as predict.py (default: labeled_lesions)")
    return p


def rate_list(text):
    """``0.125,1/4,2`` -> [(1, 8), (1, 4), (2, 1)]: every entry parsed exactly by ``fractions.Fraction``."""
    from fractions import Fraction
    try:
        vals = [Fraction(v.strip()) for v in str(text).split(",") if v.strip() != ""]
    except (ValueError, ZeroDivisionError):
        raise argparse.ArgumentTypeError(f"expected comma-separated rationals, got {text!r}")
    if not vals or any(v <= 0 for v in vals):
        raise argparse.ArgumentTypeError(f"expected one or more positive rates, got {text!r}")
    return [(v.numerator, v.denominator) for v in vals]


def size_bin_list(text):
    """``27,125,1000`` -> [27.0, 125.0, 1000.0]: 1 .. 15 finite, strictly ascending bin edges."""
    import math
    try:
        vals = [float(v) for v in str(text).split(",") if v.strip() != ""]
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected comma-separated numbers, got {text!r}")
    if not 1 <= len(vals) <= 15 or not all(math.isfinite(v) for v in vals) or any(a >= b for a, b in zip(vals, vals[1:])):
        raise argparse.ArgumentTypeError(f"expected 1 .. 15 finite, strictly ascending sizes, got {text!r}")
    return vals


def ignore_size(text):
    """``3`` -> 3.0: one finite size > 0."""
    import math
    try:
        v = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected a number, got {text!r}")
    if not math.isfinite(v) or v <= 0:
        raise argparse.ArgumentTypeError(f"expected a finite size > 0, got {text!r}")
    return v


EVAL_DEFAULTS = {"ignore_below": None, "size_bins": None, "froc": False, "froc_rates": None, "bootstrap": 0, "bootstrap_seed": 0, "data_module": "example",
                 "centers": ('CHUV_RIM_OK', 'BASEL_INSIDER_OK'), "spatial_size": (250, 300, 300), "input_images": ("FLAIR",),
                 "segmentation": "labeled_lesions"}


def eval_options(args):
    """The flags the reference does not have, with their defaults filled in -> a namespace of exactly those."""
    o = argparse.Namespace(**{k: (d if getattr(args, k, None) is None else getattr(args, k)) for k, d in EVAL_DEFAULTS.items()})
    if o.froc_rates is None:
        from .utils import DEFAULT_FP_RATES
        o.froc_rates = list(DEFAULT_FP_RATES)
    return o


def as_list(v):
    return list(v) if isinstance(v, (list, tuple)) else [float(v)]


def retrieve_boxes(path_to_dir, subject, confidence_threshold=0.5):
    """eval.py:42-58: an entry is kept iff ``score >= confidence_threshold`` (two Python floats)."""
    with open(pjoin(path_to_dir, f"sub-{subject}_preds.json"), "r") as json_file:
        infos = json.load(json_file).values()
    det_boxes, det_labels, det_scores = [], [], []
    for det_box_frac, _, det_label, det_score in infos:
        if det_score >= confidence_threshold:
            det_boxes.append(det_box_frac)
            det_labels.append(det_label)
            det_scores.append(det_score)
    return torch.FloatTensor(det_boxes), torch.LongTensor(det_labels), torch.FloatTensor(det_scores)


def resolve_prediction_dir(prediction_dir, dataset_name=None, model_name=None, predict_subset="train"):
    """eval.py:84-90: ``pd[/dn][/mn]/<subset>_set/min_score_0.0``; else ``pd`` itself when it holds ``sub-*_preds.json``
    files (the flat layout of ``predict -o``)."""
    d = prediction_dir if dataset_name is None else pjoin(prediction_dir, dataset_name)
    d = d if model_name is None else pjoin(d, model_name)
    d = pjoin(d, f"{predict_subset}_set", "min_score_0.0")
    if os.path.exists(d):
        return d
    if os.path.isdir(prediction_dir) and any(f.startswith("sub-") and f.endswith("_preds.json")
                                             for f in os.listdir(prediction_dir)):
        return prediction_dir
    raise FileNotFoundError("Prediction directory does not exist: Predictions at min_score=0.0 must be done beforehand.")


def metrics_file_name(min_iou, min_score):
    return f"metrics_(min_IoU={min_iou}_min_score={min_score}).json"


def froc_file_name(min_iou):
    return f"froc_(min_IoU={min_iou}).json"


def strata_file_name(min_iou):
    return f"strata_(min_IoU={min_iou}).json"


def convert_tensor(tensor):
    """eval.py:134-138 under the torch of the reference's era: a one-element tensor becomes a number, any other tensor
    (the empty one included) a list."""
    t = tensor.cpu().detach()
    return t.item() if t.numel() == 1 else t.tolist()


def convert_metrics(metrics):
    """eval.py:140-147: the JSON form of a calculate_mAP detail dict."""
    metrx = {}
    for key, value in metrics.items():
        if type(value) in [int, float, str]:
            metrx[key] = value
        elif type(value) == dict:
            metrx[key] = {k: convert_tensor(v) for k, v in value.items()}
        else:
            metrx[key] = convert_tensor(value)
    return metrx


def batch_voxels(batch):
    """The voxel count of every image of a collated batch (the frame its boxes are fractions of)."""
    if "voxels" in batch:
        return list(batch["voxels"])
    n = 1
    for v in batch["img"].shape[2:]:
        n *= int(v)
    return [n] * len(batch["subject"])


def gather_batches(batches, prediction_dir, confidence_threshold, log=print, frames=None):
    """eval.py:99-120 over an iterable of collated batches: the detections at or above ``confidence_threshold`` and the
    ground truth of every batch whose subjects all have a prediction file.  A batch with a missing file is skipped whole
    (the reference's behaviour); its subjects are reported through ``log``.  ``frames``: a list that receives the voxel
    count of every gathered image."""
    det_b, det_l, det_s, gt_b, gt_l = [], [], [], [], []
    for batch in batches:
        subjects = list(batch["subject"])
        missing = [s for s in subjects if not os.path.exists(pjoin(prediction_dir, f"sub-{s}_preds.json"))]
        if missing:
            log(f"skipped batch of {len(subjects)} subjects {subjects}: no prediction file for {missing}")
            continue
        preds = [retrieve_boxes(prediction_dir, s, confidence_threshold=confidence_threshold) for s in subjects]
        det_b.extend(b for b, _, _ in preds)
        det_l.extend(l for _, l, _ in preds)
        det_s.extend(s for _, _, s in preds)
        gt_b.extend(batch["boxes"])
        gt_l.extend(batch["labels"])
        if frames is not None:
            frames.extend(batch_voxels(batch))
    return det_b, det_l, det_s, gt_b, gt_l


def gather_lesion_cases(cases, prediction_dir, confidence_threshold, log=print, frames=None):
    """``gather_batches`` for the predict data set of a ``LesionsDataModule`` (``cases``, un-augmented): the detections at
    or above ``confidence_threshold`` of every case with a ``sub-<center>_<subject>_preds.json`` and its ground truth in
    the frame ``predict`` wrote those detections in - the case frame (the foreground crop, not fitted: the boxes of
    ``case_sample``) when a ``sub-*_preds_views.json`` lies beside the file (``predict --views`` / ``--flip_views``), else
    the fitted sample's.  A case without a prediction file is skipped and reported through ``log``.  Host only: the
    ground truth comes from ``cases.case_boxes``, which loads and crops the mask without preparing the image.  ``frames``: a
    list that receives the voxel count of the frame every gathered case is scored in."""
    det_b, det_l, det_s, gt_b, gt_l = [], [], [], [], []
    for pos in range(len(cases)):
        subj = cases.subjects[pos]
        subj = subj if isinstance(subj, str) else "_".join(subj)
        if not os.path.exists(pjoin(prediction_dir, f"sub-{subj}_preds.json")):
            log(f"skipped subject {subj}: no prediction file")
            continue
        b, l, s = retrieve_boxes(prediction_dir, subj, confidence_threshold=confidence_threshold)
        case_frame = os.path.exists(pjoin(prediction_dir, f"sub-{subj}_preds_views.json"))
        boxes, labels = cases.case_boxes(pos, fit=not case_frame)
        det_b.append(b), det_l.append(l), det_s.append(s), gt_b.append(boxes), gt_l.append(labels)
        if frames is not None:
            shape = cases.crop_shape(pos) if case_frame else cases.module.spatial_size
            frames.append(int(shape[0]) * int(shape[1]) * int(shape[2]))
    return det_b, det_l, det_s, gt_b, gt_l


def froc_json(summary):
    """The JSON form of one IoU threshold's ``utils.froc_summary`` dict: the same keys; an infinite score threshold (no
    detection kept at that rate) and a NaN sensitivity (no ground truth at all) become null."""
    import math

    def conv(v):
        if isinstance(v, (list, tuple)):
            return [conv(x) for x in v]
        return None if isinstance(v, float) and not math.isfinite(v) else v
    return {k: conv(v) for k, v in summary.items()}


def strata_json(summary):
    """The JSON form of one IoU threshold's ``utils.strata_summary`` dict: the same keys; a NaN (the sensitivity of a bin
    without lesions) becomes null."""
    import math

    def conv(v):
        if isinstance(v, dict):
            return {k: conv(x) for k, x in v.items()}
        if isinstance(v, (list, tuple)):
            return [conv(x) for x in v]
        return None if isinstance(v, float) and not math.isfinite(v) else v
    return conv(summary)


def ignored_block(below, true_ignore, absorbed):
    """The ``"ignored"`` block of an output file: the threshold, the number of ignored lesions (flags on class-1 boxes are
    the only ones that count, and ``gather`` hands over class-1 boxes only where it matters: the count is of set flags), and
    the absorbed detections - one number for a grid point, a list (one per rate / cut) otherwise."""
    return {"below": float(below), "n_ignored": int(sum(int(f.sum()) for f in true_ignore)),
            "absorbed": [int(v) for v in absorbed] if isinstance(absorbed, (list, tuple)) else int(absorbed)}


def with_ignored(d, below, true_ignore):
    """The JSON dict of an output file under ``--ignore_below``: its ``absorbed`` entry (what ``true_ignore`` added to the
    summary: a tensor / list per rank for a grid point, a list per rate / cut otherwise) becomes the ``"ignored"`` block.
    Without the flag (``true_ignore`` None) ``d`` is returned as it is."""
    if true_ignore is None:
        return d
    ab = d.pop("absorbed")
    if "TP" in d:  # a grid point: convert_metrics made a number of a one-element vector, a list of any other
        ab = int(sum(ab)) if isinstance(ab, list) else int(ab)
    d["ignored"] = ignored_block(below, true_ignore, ab)
    return d


def lesion_ignore_flags(gt_boxes, gt_labels, frames, below):
    """``--ignore_below``: per image, the class-1 boxes whose size is below ``below`` (``utils.ignore_below``; a flag is
    only set on a class-1 box, so the count of set flags is the count of ignored lesions).  ``below`` None -> None."""
    if below is None:
        return None
    import numpy as np
    from .utils import _np, ignore_below
    flags = ignore_below(gt_boxes, frames, below)
    return [f & (_np(l, np.int64).reshape(-1) == 1) for f, l in zip(flags, gt_labels)]


def evaluate(prediction_dir, dataset_path, model_name, dataset_name=None, num_workers=8, predict_subset="train",
             n_classes=1, percentage=1., confidence_threshold=0.5, min_iou=0.5, options=None):
    """eval.py:61-151 for every (min_iou, confidence_threshold) pair of the given values (a number or a list each).
    Returns ``{(iou, score): detail dict}``.  ``options``: an ``eval_options`` namespace (FROC, clinical cases)."""
    from .datasets import ExampleDataset
    from .train import segmentation_of
    from .utils import evaluate_detections
    opt = eval_options(argparse.Namespace() if options is None else options)
    segmentation_of(opt)  # before the first GPU call: a refused command line touches no device
    if not torch.cuda.is_available():
        raise RuntimeError("mslesions3d_amd.eval needs the HIP device (no host fallback)")
    ious, scores = as_list(min_iou), as_list(confidence_threshold)
    lesions = opt.data_module == "lesions"
    if lesions:
        from .datasets import LesionsDataModule
        dataset = LesionsDataModule(data_dir=dataset_path, centers=tuple(opt.centers), batch_size=1,
                                    input_images=tuple(opt.input_images), segmentation=opt.segmentation,
                                    classes=("lesion",) if n_classes == 1 else ("lesion", "lesion_2"),
                                    num_workers=num_workers, percentage=percentage, spatial_size=tuple(opt.spatial_size))
    else:
        dataset = ExampleDataset(n_classes=n_classes, percentage=percentage, cache=False, num_workers=num_workers,
                                 objects="multiple", batch_size=1, data_dir=dataset_path, dataset_name=dataset_name)
    dataset.setup(stage="predict_train" if predict_subset == "train" else "predict")
    loader = None if lesions else dataset._loader(dataset.predict_dataset, False, BATCH)
    prediction_dir = resolve_prediction_dir(prediction_dir, dataset_name, model_name, predict_subset)
    print(f"Prediction directory: {prediction_dir}")
    if (opt.froc or opt.size_bins) and not lesions:  # two passes over the prediction files, one over the volumes
        loader = [dict({k: b[k] for k in ("subject", "boxes", "labels")}, voxels=batch_voxels(b)) for b in loader]

    def gather(threshold, log=print, frames=None):
        if lesions:
            return gather_lesion_cases(dataset.predict_dataset, prediction_dir, threshold, log=log, frames=frames)
        return gather_batches(loader, prediction_dir, threshold, log=log, frames=frames)

    if opt.froc:
        from .utils import evaluate_froc
        # every prediction in the files counts (NaN scores fail the compare and stay out)
        voxels = []
        det_b, det_l, det_s, gt_b, gt_l = gather(float("-inf"), log=lambda *_: None,
                                                 frames=voxels if opt.ignore_below is not None else None)
        if not gt_l:
            raise RuntimeError("FROC: no case with a prediction file")
        ign = lesion_ignore_flags(gt_b, gt_l, voxels, opt.ignore_below)
        froc = evaluate_froc(det_b, det_l, det_s, gt_b, gt_l, min_overlaps=ious, fp_rates=opt.froc_rates,
                             n_boot=opt.bootstrap, seed=opt.bootstrap_seed, **({} if ign is None else {"true_ignore": ign}))
        for iou in ious:
            d = with_ignored(froc_json(froc[iou]), opt.ignore_below, ign)
            print(f"\nFROC for IoU = {iou}: CPM {d['cpm']}  sensitivity {d['sensitivity']} at {d['rates']} FP / case")
            with open(pjoin(prediction_dir, froc_file_name(iou)), "w") as json_file:
                json.dump(d, json_file, indent=4)

    if opt.size_bins:
        from .utils import evaluate_strata
        voxels = []
        det_b, det_l, det_s, gt_b, gt_l = gather(float("-inf"), log=lambda *_: None, frames=voxels)
        if not gt_l:
            raise RuntimeError("size bins: no case with a prediction file")
        ign = lesion_ignore_flags(gt_b, gt_l, voxels, opt.ignore_below)
        strata = evaluate_strata(det_b, det_l, det_s, gt_b, gt_l, voxels, opt.size_bins, min_overlaps=ious, min_scores=scores,
                                 fp_rates=opt.froc_rates if opt.froc else None, n_boot=opt.bootstrap, seed=opt.bootstrap_seed,
                                 **({} if ign is None else {"true_ignore": ign}))
        for iou in ious:
            d = with_ignored(strata_json(strata[iou]), opt.ignore_below, ign)
            print(f"\nLesions by size for IoU = {iou}: edges {d['edges']} lesions {d['n_lesions']}")
            for cut in d["cuts"]:
                at = f"min score {cut['min_score']}" if "min_score" in cut else f"{cut['fp_rate']} FP / case"
                print(f"  at {at}: sensitivity {cut['sensitivity']}  FP / case {cut['fp_per_case']}")
            with open(pjoin(prediction_dir, strata_file_name(iou)), "w") as json_file:
                json.dump(d, json_file, indent=4)

    with torch.no_grad():
        voxels = []
        det_b, det_l, det_s, gt_b, gt_l = gather(min(scores), frames=voxels if opt.ignore_below is not None else None)
        dif = [torch.zeros(len(l), dtype=torch.bool) for l in gt_l]
        ign = lesion_ignore_flags(gt_b, gt_l, voxels, opt.ignore_below)
        print("\n+-+-+- Computing metrics! +-+-+-+")
        grid = evaluate_detections(det_b, det_l, det_s, gt_b, gt_l, dif, min_overlaps=ious, min_scores=scores,
                                   return_detail=True, **({} if ign is None else {"true_ignore": ign}))
    for iou in ious:
        for sc in scores:
            metrics = grid[(iou, sc)]
            print(f"\n\n_________________________AP for IoU = {iou} / min score = {sc}_________________________\n")
            print("mAP: ", metrics["mAP"])
            print("precision: ", metrics["precision"])
            print("recall: ", metrics["recall"])
            print("f1_score: ", metrics["f1_score"])
            print()
            metrx = with_ignored(convert_metrics(metrics), opt.ignore_below, ign)
            print(metrx)
            with open(pjoin(prediction_dir, metrics_file_name(iou, sc)), "w") as json_file:
                json.dump(metrx, json_file, indent=4)
    return grid


def main(argv=None):
    args = build_parser().parse_args(argv)
    print(f"Confidence threshold set to {args.min_score}")
    return evaluate(args.prediction_dir, args.dataset_path, dataset_name=args.dataset_name, model_name=args.model_name,
                    num_workers=args.num_workers, predict_subset=args.predict_subset, n_classes=args.n_classes,
                    percentage=args.percentage, confidence_threshold=args.min_score, min_iou=args.min_iou,
                    options=eval_options(args))


if __name__ == "__main__":
    main()
