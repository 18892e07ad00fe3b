"""Evaluation with ignored ground truth on the host: the loop-form reference tests/ignore_ref.py
reproduces the oracle when no flag is set; the extended host mirrors ``utils.froc_host`` / ``utils.strata_host`` /
``utils.strata_cuts_host`` give the reference's integers on every case of tests/ignore_cases.py; the builders' own
assertions hold; the host-only parts of ``eval.py --ignore_below`` produce the ``"ignored"`` block and leave the files
alone without the flag.  CPU only."""
import json

import numpy as np
import pytest

from mslesions3d_amd import eval as EV
from mslesions3d_amd import utils as U
from oracle import metrics as OM
from tests import ignore_cases as C
from tests import ignore_ref as R
from tests.golden import cases as golden_cases

NO_NAN = [n for n in list(C.SMALL) + list(C.LARGE) if n != "odd_scores"]  # FROC and strata refuse NaN scores


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", sorted(golden_cases.map_cases()))
@pytest.mark.parametrize("thr", [0.5, 0.1])
def test_reference_without_flags_is_the_oracle(name, thr):
    c = golden_cases.map_cases()[name]
    none = [np.zeros(len(l), bool) for l in c["true_labels"]]
    case = (c["det_boxes"], c["det_labels"], c["det_scores"], c["true_boxes"], c["true_labels"], none)
    want = OM.calculate_map(*case[:5], none, min_overlap=thr)
    m = R.match(case, thr)
    sm, absorbed = R.summary(m, float("-inf"))
    assert absorbed == 0 and not m["ab"].any() and m["n_ignored"] == 0
    for i, key in ((0, "APs"), (1, "mAP"), (2, "precision"), (3, "recall"), (4, "f1_score")):
        assert np.array_equal(_bits(sm[i]), _bits(want[key])), (key, sm[i], want[key])
    assert int(sm[5]) == want["n_true_boxes"]
    if m["K"]:
        assert np.array_equal(m["tp"], want["TP"]) and np.array_equal(m["fp"], want["FP"])
        assert np.array_equal(_bits(m["score"]), _bits(want["sorted_det_scores"][1]))
        found, lost = R.volumes(m, float("-inf"))
        assert np.array_equal(_bits(found), _bits(want["found_boxes_volumes_per_class"]))
        assert np.array_equal(_bits(lost), _bits(want["not_found_boxes_volumes_per_class"]))


@pytest.mark.parametrize("name", list(C.SMALL) + list(C.LARGE))
def test_builders_hold(name):
    c = C.get(name)  # a failing builder assertion is a bug in the builder
    for thr in c["ious"]:
        m = C.match(c["case"], thr)
        assert m["ab"].sum() >= 1 and m["n_ignored"] >= 1


def test_host_matching_is_the_reference():
    for name in NO_NAN:
        c = C.get(name)
        cl = U._froc_class1(*c["case"][:5], c["case"][5])
        for thr in c["ious"]:
            m = C.match(c["case"], thr)
            tp, ab, claim = U.match_with_ignore(cl, thr)
            assert np.array_equal(tp, m["tp"]) and np.array_equal(ab, m["ab"]), (name, thr)
            assert np.array_equal(claim, m["claim"][m["t_lab"] == 1]), (name, thr)
            assert np.array_equal(cl["g"], m["g"])


def _weights(c):
    N = len(c["case"][4])
    if "weights" in c:
        return c["weights"]
    w = U.bootstrap_weights(N, 2, seed=N)
    w[1, 0] = 0
    return w


@pytest.mark.parametrize("name", NO_NAN)
def test_froc_host_is_the_reference(name):
    c = C.get(name)
    rates, w = c.get("rates", [(1, 2), (2, 1)]), _weights(c)
    if name in C.LARGE:
        w = w[:1]
    got = U.froc_host(*c["case"][:5], c["ious"], rates, w, true_ignore=c["case"][5])
    want = R.froc(c["case"], c["ious"], rates, w, match=C.match)
    for k in ("k", "tp", "gw", "nw", "absorbed"):
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), (name, k, got[k], want[k])
    assert np.array_equal(_bits(got["scores"]), _bits(want["scores"]))


@pytest.mark.parametrize("name", NO_NAN)
def test_strata_host_is_the_reference(name):
    c = C.get(name)
    w = _weights(c)[:1] if name in C.LARGE else _weights(c)
    edges, vox = c.get("edges", [27.0, 125.0, 1000.0]), c.get("voxels", 1000.0)
    K = C.match(c["case"], c["ious"][0])["K"]
    cuts = c.get("cuts", sorted({0, 1, K // 2, K, K + 3}))
    got = U.strata_host(*c["case"][:5], vox, edges, c["ious"], w, cuts, true_ignore=c["case"][5])
    want = R.strata(c["case"], vox, edges, c["ious"], w, cuts, match=C.match)
    for k in ("tp", "fp", "gw", "det_unbinned", "nw", "cuts", "absorbed"):
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), (name, k, got[k], want[k])


def test_strata_edge_bins():
    """The ignored boxes on and beside the edge are in no bin; the non-ignored box on the edge is in the bin above it."""
    c = C.get("strata")
    s = R.strata(c["case"], c["voxels"], c["edges"], c["ious"], c["weights"], c["cuts"], match=C.match)
    assert s["gw"][0].tolist() == [1, 1, 1, 0, 0]  # tiny | beside (image 1) | on2 | whole-frame bin | unbinned
    assert s["absorbed"][0, 0].tolist() == [0, 1, 1, 2, 3]


def test_cuts_host_and_none_path():
    c = C.get("random_3")
    w = _weights(c)
    cuts = U.strata_cuts_host(*c["case"][:5], c["ious"], c["scores"], c["rates"], w, true_ignore=c["case"][5])
    k = R.froc(c["case"], c["ious"], c["rates"], w, match=C.match)["k"]
    assert np.array_equal(cuts[:, :, len(c["scores"]):], k)
    # None is the path without flags; all-false flags give its integers
    none = [np.zeros(len(f), bool) for f in c["case"][5]]
    a = U.froc_host(*c["case"][:5], c["ious"], c["rates"], w)
    b = U.froc_host(*c["case"][:5], c["ious"], c["rates"], w, true_ignore=none)
    assert "absorbed" not in a and not b["absorbed"].any()
    for key in ("k", "tp", "gw", "nw"):
        assert np.array_equal(a[key], b[key])
    sa = U.strata_host(*c["case"][:5], 1000.0, [27.0, 125.0], c["ious"], w, [0, 5, 50])
    sb = U.strata_host(*c["case"][:5], 1000.0, [27.0, 125.0], c["ious"], w, [0, 5, 50], true_ignore=none)
    for key in ("tp", "fp", "gw", "det_unbinned", "nw", "cuts"):
        assert np.array_equal(sa[key], sb[key])


def test_wrong_length_flags_are_refused():
    c = C.get("multiple_absorbed")["case"]
    with pytest.raises(ValueError, match="true_ignore"):
        U.froc_host(*c[:5], [0.5], [(1, 1)], None, true_ignore=[np.zeros(3, bool)])
    with pytest.raises(ValueError, match="true_ignore"):
        U.ignore_flags([], c[4])


def test_difficult_flags_point_at_true_ignore():
    import torch
    c = C.get("multiple_absorbed")["case"]
    dif = [torch.ones(len(l), dtype=torch.bool) for l in c[4]]
    with pytest.raises(NotImplementedError, match="true_ignore"):
        U.evaluate_detections(*c[:5], dif)
    with pytest.raises(NotImplementedError, match="true_ignore"):
        U.calculate_mAP_device(*c[:5], dif)


# ---- eval.py --ignore_below, host-only ----------------------------------------------------------------------------------

def _prediction_dir(tmp_path):
    """Two subjects in a 10^3 frame: lesions of 125 and 1 voxels | 64 and 0.5 voxels; detections on each and a miss."""
    from mslesions3d_amd.predict import save_predictions
    big, tiny = C.box([0, 0, 0], 0.5), C.box([0.6, 0.6, 0.6], 0.1)
    mid, speck = C.box([0.5, 0.5, 0.5], 0.4), np.array([0.1, 0.1, 0.1, 0.2, 0.2, 0.15], np.float32)
    gts = {"a": np.stack([big, tiny]), "b": np.stack([mid, speck])}
    for s, gt in gts.items():
        b = np.concatenate([gt, C.FAR[None]]).astype(np.float32)
        save_predictions(s, (10, 10, 10), b, np.ones(3, np.int64), np.array([0.9, 0.8, 0.3], np.float32), 0.0, str(tmp_path))
    import torch
    batches = [{"subject": [s], "boxes": [torch.from_numpy(gt)], "labels": [torch.ones(2, dtype=torch.int64)], "voxels": [1000]}
               for s, gt in gts.items()]
    return batches


def test_eval_ignore_below_block(tmp_path):
    opt = EV.eval_options(EV.build_parser().parse_args(["--ignore_below", "3", "--froc"]))
    assert opt.ignore_below == 3.0 and EV.eval_options(EV.build_parser().parse_args([])).ignore_below is None
    assert "ignore_below" not in vars(EV.build_parser().parse_args([]))
    batches = _prediction_dir(tmp_path)
    frames = []
    det_b, det_l, det_s, gt_b, gt_l = EV.gather_batches(batches, str(tmp_path), float("-inf"), log=lambda *_: None, frames=frames)
    ign = EV.lesion_ignore_flags(gt_b, gt_l, frames, opt.ignore_below)
    assert [f.tolist() for f in ign] == [[False, True], [False, True]]  # 1 voxel and 0.5 voxels are below 3
    rates, w = [(1, 2), (1, 1)], U.bootstrap_weights(2, 0)
    ints = U.froc_host(det_b, det_l, det_s, gt_b, gt_l, [0.5], rates, w, true_ignore=ign)
    s = U.froc_summary(ints, [0.5], rates)[0.5]
    s["absorbed"] = U.ignored_summary(ints, 0)
    d = EV.with_ignored(EV.froc_json(s), opt.ignore_below, ign)
    assert d["ignored"] == {"below": 3.0, "n_ignored": 2, "absorbed": [2, 2]} and "absorbed" not in d
    assert d["n_lesions"] == 2 and d["sensitivity"] == [1.0, 1.0]
    json.dumps(d)
    # a size bin wholly below the threshold is reported, empty
    st = U.strata_host(det_b, det_l, det_s, gt_b, gt_l, frames, [2.0, 100.0], [0.5], w, [6], true_ignore=ign)
    sm = U.strata_summary(st, [2.0, 100.0], [0.5], [{"min_score": 0.0}])[0.5]
    # (the two far misses are under 2 voxels themselves: real false positives of that bin; the absorbed ones are in none)
    assert sm["n_lesions"] == [0, 1, 1] and sm["cuts"][0]["fp_per_case"] == [1.0, 0.0, 0.0]
    assert sm["cuts"][0]["sensitivity"][1:] == [1.0, 1.0] and sm["cuts"][0]["sensitivity"][0] != sm["cuts"][0]["sensitivity"][0]
    # a grid point: the per-rank vector becomes a count
    g = EV.with_ignored({"TP": [1.0, 0.0], "absorbed": [0.0, 1.0], "n_ignored_boxes": 2}, 3.0, ign)
    assert g["ignored"] == {"below": 3.0, "n_ignored": 2, "absorbed": 1}


def test_eval_without_the_flag_is_unchanged(tmp_path):
    batches = _prediction_dir(tmp_path)
    det_b, det_l, det_s, gt_b, gt_l = EV.gather_batches(batches, str(tmp_path), float("-inf"), log=lambda *_: None)
    assert EV.lesion_ignore_flags(gt_b, gt_l, [], None) is None
    rates, w = [(1, 2), (1, 1)], U.bootstrap_weights(2, 0)
    s = U.froc_summary(U.froc_host(det_b, det_l, det_s, gt_b, gt_l, [0.5], rates, w), [0.5], rates)[0.5]
    before = json.dumps(EV.froc_json(s), indent=4)
    d = EV.with_ignored(EV.froc_json(s), None, None)
    assert json.dumps(d, indent=4) == before and "ignored" not in d and "absorbed" not in d
    assert d["n_lesions"] == 4
