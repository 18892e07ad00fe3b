"""Evaluation entry point — flags of the reference's ``lesions3d/eval.py:17-36`` and the flow of its ``evaluate``
(``eval.py:61-151``): read back the ``sub-XXXX_preds.json`` files that ``predict`` wrote at min_score 0.0, keep the
detections at or above ``-sc``, compute one dataset-level ``calculate_mAP`` at ``-iou`` and write
``metrics_(min_IoU=<iou>_min_score=<score>).json`` next to the predictions (the files the reference's ``plots.py`` reads).

One extension: ``-sc`` and ``-iou`` take comma-separated lists; the whole grid comes from one device sweep
(``utils.evaluate_detections``), every grid point bit-identical to the host ``calculate_mAP`` on the filtered detections.

    python -m mslesions3d_amd.eval -d DATA -dn NAME -pd PREDICTIONS -sc 0.1,0.5 -iou 0.1,0.5
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
    return p


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


def gather_batches(batches, prediction_dir, confidence_threshold, log=print):
    """eval.py:99-120 over an iterable of collated batches: the detections at or above ``confidence_threshold`` and the
    ground truth of every batch whose subjects all have a prediction file.  A batch with a missing file is skipped whole
    (the reference's behaviour); its subjects are reported through ``log``."""
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
    return det_b, det_l, det_s, gt_b, gt_l


def evaluate(prediction_dir, dataset_path, model_name, dataset_name=None, num_workers=8, predict_subset="train",
             n_classes=1, percentage=1., confidence_threshold=0.5, min_iou=0.5):
    """eval.py:61-151 for every (min_iou, confidence_threshold) pair of the given values (a number or a list each).
    Returns ``{(iou, score): detail dict}``."""
    from .datasets import ExampleDataset
    from .utils import evaluate_detections
    if not torch.cuda.is_available():
        raise RuntimeError("mslesions3d_amd.eval needs the HIP device (no host fallback)")
    ious, scores = as_list(min_iou), as_list(confidence_threshold)
    dataset = ExampleDataset(n_classes=n_classes, percentage=percentage, cache=False, num_workers=num_workers,
                             objects="multiple", batch_size=1, data_dir=dataset_path, dataset_name=dataset_name)
    dataset.setup(stage="predict_train" if predict_subset == "train" else "predict")
    loader = dataset._loader(dataset.predict_dataset, False, BATCH)
    prediction_dir = resolve_prediction_dir(prediction_dir, dataset_name, model_name, predict_subset)
    print(f"Prediction directory: {prediction_dir}")

    with torch.no_grad():
        det_b, det_l, det_s, gt_b, gt_l = gather_batches(loader, prediction_dir, min(scores))
        dif = [torch.zeros(len(l), dtype=torch.bool) for l in gt_l]
        print("\n+-+-+- Computing metrics! +-+-+-+")
        grid = evaluate_detections(det_b, det_l, det_s, gt_b, gt_l, dif, min_overlaps=ious, min_scores=scores,
                                   return_detail=True)
    for iou in ious:
        for sc in scores:
            metrics = grid[(iou, sc)]
            print(f"\n\n_________________________AP for IoU = {iou} / min score = {sc}_________________________\n")
            print("mAP: ", metrics["mAP"])
            print("precision: ", metrics["precision"])
            print("recall: ", metrics["recall"])
            print("f1_score: ", metrics["f1_score"])
            print()
            metrx = convert_metrics(metrics)
            print(metrx)
            with open(pjoin(prediction_dir, metrics_file_name(iou, sc)), "w") as json_file:
                json.dump(metrx, json_file, indent=4)
    return grid


def main(argv=None):
    args = build_parser().parse_args(argv)
    print(f"Confidence threshold set to {args.min_score}")
    return evaluate(args.prediction_dir, args.dataset_path, dataset_name=args.dataset_name, model_name=args.model_name,
                    num_workers=args.num_workers, predict_subset=args.predict_subset, n_classes=args.n_classes,
                    percentage=args.percentage, confidence_threshold=args.min_score, min_iou=args.min_iou)


if __name__ == "__main__":
    main()
