"""The host side of ``python -m mslesions3d_amd.eval`` (the reference's lesions3d/eval.py): flags and defaults, the f64
score filter of retrieve_boxes, the JSON form of calculate_mAP detail dicts, output names, the prediction-directory
layouts and the batch-of-32 skip.  CPU only (the sweep itself: tests/test_gpu_eval.py)."""
import json
import os

import numpy as np
import pytest
import torch

from mslesions3d_amd import eval as EV


def test_parser_flags_and_defaults():
    a = EV.build_parser().parse_args([])
    assert (a.dataset_path, a.dataset_name, a.model_name, a.percentage, a.n_classes, a.num_workers, a.predict_subset,
            a.min_score, a.min_iou, a.top_k, a.prediction_dir) == \
        ('../data/artificial_dataset', None, None, 1., 1, 8, 'train', 0.5, 0.5, 100, "../data/predictions/")
    a = EV.build_parser().parse_args(["-d", "D", "-dn", "N", "-mn", "M", "-p", "0.5", "-c", "2", "-nw", "0", "-ps", "test",
                                      "-sc", "0.3", "-iou", "0.1", "-k", "50", "-pd", "P"])
    assert (a.dataset_path, a.dataset_name, a.model_name, a.percentage, a.n_classes, a.num_workers, a.predict_subset,
            a.min_score, a.min_iou, a.top_k, a.prediction_dir) == ("D", "N", "M", 0.5, 2, 0, "test", [0.3], [0.1], 50, "P")
    for long_form in ("--dataset_path", "--dataset_name", "--model_name", "--percentage", "--n_classes", "--num_workers",
                      "--predict_subset", "--min_score", "--min_iou", "--top_k", "--prediction_dir"):
        assert long_form in EV.build_parser().format_help()
    with pytest.raises(SystemExit):
        EV.build_parser().parse_args(["-ps", "everything"])


def test_score_and_iou_lists():
    a = EV.build_parser().parse_args(["-sc", "0.1,0.5,0.9", "-iou", "0.1,0.5"])
    assert a.min_score == [0.1, 0.5, 0.9] and a.min_iou == [0.1, 0.5]
    assert EV.as_list(0.5) == [0.5] and EV.as_list([0.1, 0.2]) == [0.1, 0.2]
    assert EV.build_parser().parse_args(["-sc", "1e-1"]).min_score == [0.1]
    with pytest.raises(SystemExit):
        EV.build_parser().parse_args(["-sc", "a,b"])


def _write_preds(path, subject, scores, labels=None):
    infos = {j + 1: ([0.1, 0.1, 0.1, 0.2, 0.2, 0.2], [6, 6, 6, 12, 12, 12], int(1 if labels is None else labels[j]), float(s))
             for j, s in enumerate(scores)}
    with open(os.path.join(path, f"sub-{subject}_preds.json"), "w") as f:
        json.dump(infos, f)


@pytest.mark.parametrize("c", [0.7, 0.9, 0.1, 0.3])
def test_retrieve_boxes_compares_python_floats(tmp_path, c):
    """c is not an f32 value: the f32 neighbours of c (as predict writes them, Python floats of f32 scores) fall on
    either side of it, which an f32 compare would get wrong for float32(c) < c."""
    f = np.float32(c)
    below, above = np.nextafter(f, np.float32(0)), np.nextafter(f, np.float32(1))
    scores = [float(below), float(f), float(above), 1.0, 0.0]
    _write_preds(str(tmp_path), "0001", scores)
    b, l, s = EV.retrieve_boxes(str(tmp_path), "0001", confidence_threshold=c)
    want = [x for x in scores if x >= c]
    assert s.tolist() == [float(np.float32(x)) for x in want] and len(l) == len(want) == b.shape[0]
    assert (float(f) >= c) == (float(f) > c)  # c itself is never an f32 value
    assert b.dtype == torch.float32 and l.dtype == torch.int64 and s.dtype == torch.float32
    if not want:
        assert b.shape == (0,)


def test_retrieve_boxes_empty_selection_is_a_flat_empty_tensor(tmp_path):
    _write_preds(str(tmp_path), "0002", [0.1, 0.2])
    b, l, s = EV.retrieve_boxes(str(tmp_path), "0002", confidence_threshold=0.5)
    assert b.shape == (0,) and l.shape == (0,) and s.shape == (0,)


def _detail(n_det, hit):
    from mslesions3d_amd.utils import calculate_mAP
    gt = [torch.tensor([[0.1, 0.1, 0.1, 0.3, 0.3, 0.3]])]
    boxes = torch.tensor([[0.1, 0.1, 0.1, 0.3, 0.3, 0.3] if hit else [0.6, 0.6, 0.6, 0.7, 0.7, 0.7]] * n_det).reshape(-1, 6)
    labels = torch.ones(n_det, dtype=torch.int64) if n_det else torch.zeros(1, dtype=torch.int64)
    if not n_det:
        boxes = torch.tensor([[0., 0., 0., 1., 1., 1.]])
    scores = torch.linspace(0.9, 0.5, max(n_det, 1))
    return calculate_mAP([boxes], [labels], [scores], gt, [torch.ones(1, dtype=torch.int64)], [torch.zeros(1, dtype=torch.bool)],
                         min_overlap=0.5, return_detail=True)


def test_json_conversion_rules():
    one = EV.convert_metrics(_detail(1, True))  # one-element TP / FP / scores / found volumes
    assert one["TP"] == 1.0 and one["FP"] == 0.0 and isinstance(one["TP"], float)
    assert one["sorted_det_scores"] == {1: float(np.float32(0.9))}
    assert isinstance(one["found_boxes_volumes_per_class"], float)  # one found box: a number
    assert one["not_found_boxes_volumes_per_class"] == []  # the empty tensor becomes a list
    assert isinstance(one["n_true_boxes"], int) and isinstance(one["mAP"], float)
    two = EV.convert_metrics(_detail(2, True))
    assert two["TP"] == [1.0, 0.0] and two["FP"] == [0.0, 1.0] and isinstance(two["sorted_det_scores"][1], list)
    none = EV.convert_metrics(_detail(0, True))  # nothing detected: empty TP, empty scores dict
    assert none["TP"] == [] and none["FP"] == [] and none["sorted_det_scores"] == {}
    assert isinstance(none["not_found_boxes_volumes_per_class"], float)  # one ground-truth box: a number
    text = json.dumps(one, indent=4)
    assert list(json.loads(text).keys()) == ["APs", "mAP", "precision", "recall", "f1_score", "sorted_det_scores", "TP", "FP",
                                             "n_true_boxes", "found_boxes_volumes_per_class",
                                             "not_found_boxes_volumes_per_class"]
    assert '"sorted_det_scores": {\n        "1": ' in text


def test_output_file_names():
    assert EV.metrics_file_name(0.5, 0.5) == "metrics_(min_IoU=0.5_min_score=0.5).json"
    a = EV.build_parser().parse_args(["-sc", "0.10,0.5", "-iou", ".1"])
    names = [EV.metrics_file_name(i, s) for i in a.min_iou for s in a.min_score]
    assert names == ["metrics_(min_IoU=0.1_min_score=0.1).json", "metrics_(min_IoU=0.1_min_score=0.5).json"]


def test_prediction_directory_layouts(tmp_path):
    nested = tmp_path / "pd" / "ds" / "model" / "validation_set" / "min_score_0.0"
    nested.mkdir(parents=True)
    assert EV.resolve_prediction_dir(str(tmp_path / "pd"), "ds", "model", "validation") == str(nested)
    plain = tmp_path / "pd2" / "train_set" / "min_score_0.0"
    plain.mkdir(parents=True)
    assert EV.resolve_prediction_dir(str(tmp_path / "pd2")) == str(plain)
    flat = tmp_path / "flat"
    flat.mkdir()
    _write_preds(str(flat), "0003", [0.5])
    assert EV.resolve_prediction_dir(str(flat), "ds", "model", "train") == str(flat)
    empty = tmp_path / "empty"
    empty.mkdir()
    (empty / "notes.txt").write_text("no predictions here")
    for pd in (str(empty), str(tmp_path / "missing")):
        with pytest.raises(FileNotFoundError, match="Predictions at min_score=0.0 must be done beforehand"):
            EV.resolve_prediction_dir(pd, "ds", None, "train")


def _batch(subjects):
    return {"subject": subjects, "boxes": [torch.full((1, 6), float(i)) for i, _ in enumerate(subjects)],
            "labels": [torch.ones(1, dtype=torch.int64) for _ in subjects]}


def test_batch_with_a_missing_file_is_skipped_whole(tmp_path):
    first = [f"{k:04d}" for k in range(32)]
    second = [f"{k:04d}" for k in range(32, 40)]
    for s in first + second:
        if s != "0035":
            _write_preds(str(tmp_path), s, [0.2, 0.8], labels=[1, 2])
    logged = []
    det_b, det_l, det_s, gt_b, gt_l = EV.gather_batches([_batch(first), _batch(second)], str(tmp_path), 0.5, log=logged.append)
    assert len(det_b) == len(det_l) == len(det_s) == len(gt_b) == len(gt_l) == 32
    assert all(s.tolist() == [float(np.float32(0.8))] and l.tolist() == [2] for s, l in zip(det_s, det_l))
    assert len(logged) == 1 and "0035" in logged[0] and all(s in logged[0] for s in second)
    assert EV.BATCH == 32


def test_evaluate_needs_the_device(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="HIP device"):
        EV.evaluate("nowhere", "nowhere", None)


def test_capacity_is_checked_on_the_host():
    """The workspace query is host arithmetic: past the 4096 cap of msl_detection_metrics it plans, past int32 indexing
    it refuses before anything is launched."""
    from mslesions3d_amd import _lib
    from mslesions3d_amd.utils import evaluate_capacity_check
    assert evaluate_capacity_check(2 ** 22, 2 ** 16, 2 ** 20, 2, 10) > 2 ** 22 * 4 * 7
    assert evaluate_capacity_check(0, 1, 0, 1, 1) > 0
    for bad in ((2 ** 29, 1, 0, 1, 1), (2 ** 28, 1, 0, 16, 1), (10, 0, 0, 1, 1), (10, 1, 0, 0, 1), (10, 1, 0, 1, 0)):
        with pytest.raises(_lib.HipKernelError):
            evaluate_capacity_check(*bad)
