"""FROC on the host (DESIGN.md "FROC"): the numpy twin ``utils.froc_host`` against a hand-worked case and against a
brute-force restatement of the definition on top of the oracle's ``calculate_map``; weights as repetition; the bootstrap
plumbing; the host pieces of ``python -m mslesions3d_amd.eval --froc`` / ``-dm lesions``.  CPU only (the kernel:
tests/test_gpu_froc.py)."""
import json
import os
import re

import numpy as np
import pytest
import torch

from mslesions3d_amd import eval as EV
from mslesions3d_amd import utils as U
from tests import lesion_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = U.DEFAULT_FP_RATES


def _box(lo, size=0.2):
    return [lo, lo, lo, lo + size, lo + size, lo + size]


def _arr(rows):
    return np.asarray(rows, np.float32).reshape(-1, 6)


def test_exported_constants_mirror_the_kernel():
    src = open(os.path.join(ROOT, "mslesions3d_amd", "csrc", "evaluate.hip")).read()
    threads = int(re.search(r"constexpr int EV_THREADS = (\d+);", src).group(1))
    per = int(re.search(r"constexpr int EV_FROC_PER = (\d+);", src).group(1))
    assert U.FROC_TILE == threads * per
    assert U.FROC_MAX_RATES == int(re.search(r"constexpr int EV_FROC_MAX_RATES = (\d+);", src).group(1))
    assert RATES == ((1, 8), (1, 4), (1, 2), (1, 1), (2, 1), (4, 1), (8, 1))


# ---- C1 ---------------------------------------------------------------------------------------------------------------

def _hand_case():
    """Four images.  Ground truth: image 0 has A and B, image 1 none, image 2 has C (and no detection), image 3 has E.
    Class-1 detections (a hit is the ground-truth box itself, IoU 1):
        image 0: A 0.9 (TP), a miss 0.75 (FP), B 0.5 (TP), and a label-0 placeholder row that does not count
        image 1: a box 0.75 (FP: no ground truth) - tied with image 0's miss
        image 3: E 0.6 (TP), E again 0.4 (FP: already claimed)
    Rank order (stable): 0.9 TP img0 | 0.75 FP img0 | 0.75 FP img1 | 0.6 TP img3 | 0.5 TP img0 | 0.4 FP img3;  K = 6.
    Admissible prefix lengths: 0 1 3 4 5 6 (2 cuts the tie at 0.75).
    Unit weights, N = 4, G = 4:   k      0 1 2 3 4 5 6
                                  TP(k)  0 1 1 1 2 3 3
                                  FP(k)  0 0 1 2 2 2 3
      rate 1/8: FP*8 <= 4 -> FP = 0 -> k* = 1, TP 1        rate 1/4: FP <= 1 -> k = 2 is not admissible -> k* = 1, TP 1
      rate 1/2: FP <= 2 -> k* = 5, TP 3                    rates 1, 2, 4, 8: FP <= 4 .. 32 -> k* = 6, TP 3
    Weights (2, 0, 1, 1): Nw = 4, Gw = 2*2 + 0 + 1 + 1 = 6; the ranks weigh 2 2 0 1 2 1:
                                  TPw(k) 0 2 2 2 3 5 5
                                  FPw(k) 0 0 2 2 2 2 3
      1/8 and 1/4: FPw <= 0 / 1 -> k* = 1, TPw 2;  1/2: FPw <= 2 -> k* = 5, TPw 5;  1 and up: k* = 6, TPw 5."""
    A, B, C, E = _box(0.0), _box(0.5), _box(0.3), _box(0.1)
    tb = [_arr([A, B]), _arr([]), _arr([C]), _arr([E])]
    tl = [np.ones(2, np.int64), np.zeros(0, np.int64), np.ones(1, np.int64), np.ones(1, np.int64)]
    db = [_arr([A, _box(0.75), B, [0, 0, 0, 1, 1, 1]]), _arr([_box(0.4)]), _arr([]), _arr([E, E])]
    dl = [np.array([1, 1, 1, 0]), np.array([1]), np.zeros(0, np.int64), np.array([1, 1])]
    ds = [np.array([0.9, 0.75, 0.5, 0.0], np.float32), np.array([0.75], np.float32), np.zeros(0, np.float32),
          np.array([0.6, 0.4], np.float32)]
    return db, dl, ds, tb, tl


def test_hand_worked_case():
    case = _hand_case()
    w = np.array([[1, 1, 1, 1], [2, 0, 1, 1]], np.int32)
    ints = U.froc_host(*case, [0.5, 0.1], RATES, w)
    for t in range(2):  # every hit has IoU 1 and every miss IoU 0: both thresholds agree
        assert ints["k"][0, t].tolist() == [1, 1, 5, 6, 6, 6, 6]
        assert ints["tp"][0, t].tolist() == [1, 1, 3, 3, 3, 3, 3]
        assert ints["k"][1, t].tolist() == [1, 1, 5, 6, 6, 6, 6]
        assert ints["tp"][1, t].tolist() == [2, 2, 5, 5, 5, 5, 5]
    assert ints["gw"].tolist() == [4, 6] and ints["nw"].tolist() == [4, 4]
    assert ints["scores"].tolist() == [float(np.float32(v)) for v in (0.9, 0.75, 0.75, 0.6, 0.5, 0.4)]
    s = U.froc_summary(ints, [0.5, 0.1], RATES)[0.5]
    assert s["rates"] == [0.125, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0]
    assert s["sensitivity"] == [0.25, 0.25, 0.75, 0.75, 0.75, 0.75, 0.75]
    assert s["score_threshold"] == [float(np.float32(v)) for v in (0.9, 0.9, 0.5, 0.4, 0.4, 0.4, 0.4)]
    assert s["cpm"] == sum([0.25, 0.25, 0.75, 0.75, 0.75, 0.75, 0.75]) / 7
    assert (s["n_cases"], s["n_lesions"], s["n_boot"], s["dropped"]) == (4, 4, 1, 0)
    assert s["ci_low"] == [float(v) for v in np.percentile([[2 / 6, 2 / 6, 5 / 6, 5 / 6, 5 / 6, 5 / 6, 5 / 6]], 2.5, axis=0)]
    # weights (0, 1, 1, 1) and the rate 2^-20: FPw * 2^20 <= 3 -> FPw = 0.  The ranks weigh 0 0 1 1 0 1, so FPw(1) =
    # FPw(2) = 0 and FPw(3) = 1; k = 2 cuts the tie, which leaves k* = 1 with TPw 0 (image 0's hit weighs nothing)
    z = U.froc_host(*case, [0.5], [(1, 1 << 20)], np.array([[0, 1, 1, 1]], np.int32))
    assert z["k"][0, 0].tolist() == [1] and z["tp"][0, 0].tolist() == [0]
    s = U.froc_summary(z, [0.5], [(1, 1 << 20)])[0.5]
    assert s["sensitivity"] == [0.0] and s["n_lesions"] == 2


def test_nan_scores_and_bad_arguments_are_rejected():
    db, dl, ds, tb, tl = _hand_case()
    ds[3] = np.array([np.nan, 0.4], np.float32)
    with pytest.raises(ValueError, match="NaN"):
        U.froc_host(db, dl, ds, tb, tl, [0.5], RATES, None)
    case = _hand_case()
    for bad in ([(0, 1)], [(1, (1 << 20) + 1)], [(1, 1)] * 17, []):
        with pytest.raises(ValueError):
            U.froc_host(*case, [0.5], bad, None)
    for bad in (np.ones((1, 3), np.int32), -np.ones((1, 4), np.int32), np.ones((1, 4), np.float32)):
        with pytest.raises(ValueError):
            U.froc_host(*case, [0.5], RATES, bad)
    assert U.froc_rates([0.125, "1/3", (2, 4)]) == [(1, 8), (1, 3), (1, 2)]


# ---- C2 ---------------------------------------------------------------------------------------------------------------

def _boxes(rs, n):
    lo = rs.uniform(0, 0.8, (n, 3)).astype(np.float32)
    return np.concatenate([lo, lo + rs.uniform(0.05, 0.25, (n, 3)).astype(np.float32)], 1)


def _draw(seed, n_img=6, per=8):
    """Hits with jitter, duplicates, misses, label 0 / 2 rows, scores quantised to 1/8, an image without ground truth, an
    image without detections."""
    rs = np.random.RandomState(seed)
    tb, tl, db, dl, ds = [], [], [], [], []
    for i in range(n_img):
        ng = 0 if i == seed % n_img else int(rs.randint(1, 5))
        nd = 0 if i == (seed + 2) % n_img else int(rs.randint(1, per + 1))
        t, d = _boxes(rs, ng), _boxes(rs, nd)
        if ng and nd:
            k = min(nd, 2 * ng)
            d[:k] = t[rs.randint(0, ng, k)] + rs.uniform(-0.03, 0.03, (k, 6)).astype(np.float32)
        lab = np.ones(ng, np.int64)
        lab[rs.rand(ng) < 0.15] = 2
        lb = np.ones(nd, np.int64)
        lb[rs.rand(nd) < 0.1] = 2
        lb[rs.rand(nd) < 0.1] = 0
        sc = (np.round(rs.uniform(0, 1, nd) * 8) / 8).astype(np.float32)
        tb.append(t), tl.append(lab), db.append(d), dl.append(lb), ds.append(sc)
    return db, dl, ds, tb, tl


def _brute_force(case, ious, rates):
    """The definition through score thresholds: for every distinct class-1 score c the oracle's calculate_map on the
    detections with score >= c gives (sum TP, sum FP); the result at a rate is the largest sum TP among the points with
    sum FP * den <= num * N, the point (0, 0) included."""
    from oracle import metrics as OM
    db, dl, ds, tb, tl = case
    N = len(tl)
    dif = [np.zeros(len(l), bool) for l in tl]
    cuts = sorted({float(v) for sc, lb in zip(ds, dl) for v in sc[lb == 1]})
    out = np.zeros((len(ious), len(rates)), np.int64)
    for t, ov in enumerate(ious):
        points = [(0, 0)]
        for c in cuts:
            keep = [s >= np.float32(c) for s in ds]
            d = OM.calculate_map([b[k] for b, k in zip(db, keep)], [l[k] for l, k in zip(dl, keep)],
                                 [s[k] for s, k in zip(ds, keep)], tb, tl, dif, min_overlap=ov)
            points.append((int(d["TP"].sum()), int(d["FP"].sum())))
        for ci, (num, den) in enumerate(rates):
            out[t, ci] = max(tp for tp, fp in points if fp * den <= num * N)
    return out


@pytest.mark.parametrize("seed", range(24))
def test_unit_weights_equal_the_brute_force_definition(seed):
    case = _draw(seed)
    ious = [0.1, 0.5]
    ints = U.froc_host(*case, ious, RATES, None)
    assert ints["k"].shape == (1, 2, 7)
    assert np.array_equal(ints["tp"][0], _brute_force(case, ious, RATES))
    assert ints["nw"].tolist() == [6] and ints["gw"].tolist() == [sum(int((l == 1).sum()) for l in case[4])]


# ---- C3 ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(6))
def test_weights_mean_repetition(seed):
    """froc_host with weights w == froc_host with unit weights on the data set in which image n appears w[n] times.  The
    copies of an image are adjacent, so the stable rank order of the repeated set keeps tied copies together, and
    admissibility depends on scores only - k differs (every rank counts w times), TPw, Gw, Nw must not."""
    case = _draw(100 + seed)
    rs = np.random.RandomState(seed)
    w = rs.randint(0, 4, 6).astype(np.int32)
    w[seed % 6] = 0
    if w.sum() == 0:
        w[(seed + 1) % 6] = 2
    rep = [[x[n] for n in range(6) for _ in range(int(w[n]))] for x in case]
    ious = [0.1, 0.5]
    a = U.froc_host(*case, ious, RATES, w[None])
    b = U.froc_host(*rep, ious, RATES, None)
    assert np.array_equal(a["tp"], b["tp"]) and a["gw"].tolist() == b["gw"].tolist() and a["nw"].tolist() == b["nw"].tolist()
    # prefix lengths: k* of the repeated set is the weighted length of the weighted set's prefix
    img = np.concatenate([np.full(int((l == 1).sum()), n) for n, l in enumerate(case[1])])
    sc = np.concatenate([s[l == 1] for s, l in zip(case[2], case[1])])
    order = np.lexsort((np.arange(len(sc)), -sc.astype(np.float64)))
    cum = np.concatenate([[0], np.cumsum(w[img[order]])])
    assert np.array_equal(cum[a["k"]], b["k"])


# ---- C4 ---------------------------------------------------------------------------------------------------------------

def test_bootstrap_plumbing():
    N, R, seed = 6, 40, 3
    w = U.bootstrap_weights(N, R, seed)
    assert w.dtype == np.int32 and w.shape == (R + 1, N) and (w[0] == 1).all() and (w.sum(1) == N).all()
    draws = np.random.default_rng(seed).integers(0, N, size=(R, N))
    assert np.array_equal(w[1:], np.stack([np.bincount(d, minlength=N) for d in draws]))
    assert U.bootstrap_weights(N, 0).shape == (1, N)
    db, dl, ds, tb, tl = _draw(7)
    for n in range(N):  # every image carries class-1 ground truth: no resample is empty
        if not (tl[n] == 1).any():
            tb[n], tl[n] = _boxes(np.random.RandomState(n), 2), np.ones(2, np.int64)
    ious = [0.1, 0.5]
    ints = U.froc_host(db, dl, ds, tb, tl, ious, RATES, w)
    s = U.froc_summary(ints, ious, RATES)
    for t, ov in enumerate(ious):
        d = s[ov]
        assert list(d) == ["rates", "sensitivity", "score_threshold", "cpm", "ci_low", "ci_high", "cpm_ci", "n_cases",
                           "n_lesions", "n_boot", "dropped"]
        assert d["dropped"] == 0 and d["n_boot"] == R and d["n_cases"] == N
        sens = ints["tp"][1:, t, :] / ints["gw"][1:, None]
        lo, hi = np.percentile(sens, [2.5, 97.5], axis=0)
        assert d["ci_low"] == lo.tolist() and d["ci_high"] == hi.tolist()
        assert all(a <= b for a, b in zip(d["ci_low"], d["ci_high"]))
        assert d["cpm_ci"] == np.percentile(sens.mean(1), [2.5, 97.5]).tolist() and d["cpm_ci"][0] <= d["cpm_ci"][1]
        assert d["sensitivity"] == (ints["tp"][0, t] / ints["gw"][0]).tolist()
    # resamples without ground truth are dropped and counted; without resamples there is no interval
    tl2 = [np.zeros(0, np.int64)] * (N - 1) + [tl[-1]]
    tb2 = [np.zeros((0, 6), np.float32)] * (N - 1) + [tb[-1]]
    i2 = U.froc_host(db, dl, ds, tb2, tl2, [0.5], RATES, w)
    d = U.froc_summary(i2, [0.5], RATES)[0.5]
    assert d["dropped"] == int((w[1:, -1] == 0).sum()) > 0
    d = U.froc_summary(U.froc_host(db, dl, ds, tb, tl, [0.5], RATES, None), [0.5], RATES)[0.5]
    assert d["ci_low"] is None and d["ci_high"] is None and d["cpm_ci"] is None and d["n_boot"] == 0


# ---- C5 ---------------------------------------------------------------------------------------------------------------

def test_rate_parsing_and_new_flags():
    assert EV.rate_list("0.125,0.25,0.5,1,2,4,8") == list(RATES)
    assert EV.rate_list("1/3, 2.5") == [(1, 3), (5, 2)]
    a = EV.build_parser().parse_args(["--froc", "--froc_rates", "0.125,1/3", "--bootstrap", "16", "--bootstrap_seed", "5",
                                      "-dm", "lesions", "--centers", "A", "B", "--spatial_size", "8", "9", "10", "-ii",
                                      "FLAIR", "acq-mag_T2star"])
    o = EV.eval_options(a)
    assert (o.froc, o.froc_rates, o.bootstrap, o.bootstrap_seed, o.data_module, o.centers, o.spatial_size, o.input_images) == \
        (True, [(1, 8), (1, 3)], 16, 5, "lesions", ["A", "B"], [8, 9, 10], ["FLAIR", "acq-mag_T2star"])
    for bad in (["--froc_rates", "a"], ["--froc_rates", "0"], ["--froc_rates", "-1"], ["--froc_rates", "1/0"], ["-dm", "x"]):
        with pytest.raises(SystemExit):
            EV.build_parser().parse_args(bad)


def test_parser_without_new_flags_yields_the_old_namespace():
    a = EV.build_parser().parse_args([])
    assert sorted(vars(a)) == sorted(["dataset_path", "dataset_name", "model_name", "percentage", "n_classes", "num_workers",
                                      "predict_subset", "min_score", "min_iou", "top_k", "prediction_dir"])
    o = EV.eval_options(a)
    assert (o.froc, o.froc_rates, o.bootstrap, o.bootstrap_seed, o.data_module) == (False, list(RATES), 0, 0, "example")
    assert tuple(o.centers) == ('CHUV_RIM_OK', 'BASEL_INSIDER_OK') and tuple(o.spatial_size) == (250, 300, 300)


def test_froc_file_name_and_json_schema():
    assert EV.froc_file_name(0.5) == "froc_(min_IoU=0.5).json"
    ints = U.froc_host(*_hand_case(), [0.5], [(1, 1 << 20), (1, 1)], np.array([[1, 1, 1, 1], [0, 1, 0, 0]], np.int32))
    d = EV.froc_json(U.froc_summary(ints, [0.5], [(1, 1 << 20), (1, 1)])[0.5])
    text = json.dumps(d, indent=4)
    back = json.loads(text)
    assert list(back) == ["rates", "sensitivity", "score_threshold", "cpm", "ci_low", "ci_high", "cpm_ci", "n_cases",
                          "n_lesions", "n_boot", "dropped"]
    assert back["dropped"] == 1 and back["ci_low"] is None and "Infinity" not in text and "NaN" not in text
    assert back["sensitivity"] == [0.25, 0.75] and back["score_threshold"] == [float(np.float32(0.9)), float(np.float32(0.4))]
    empty = ([_arr([])], [np.zeros(0, np.int64)], [np.zeros(0, np.float32)], [_arr([_box(0.1)])], [np.ones(1, np.int64)])
    d = EV.froc_json(U.froc_summary(U.froc_host(*empty, [0.5], RATES, None), [0.5], RATES)[0.5])
    assert d["score_threshold"] == [None] * 7 and d["sensitivity"] == [0.0] * 7  # k* = 0: no threshold keeps anything


def _write_preds(path, subject, boxes, scores):
    infos = {j + 1: ([float(v) for v in b], [0] * 6, 1, float(s)) for j, (b, s) in enumerate(zip(boxes, scores))}
    with open(os.path.join(path, f"sub-{subject}_preds.json"), "w") as f:
        json.dump(infos, f)


def test_gather_lesion_cases_picks_the_frame_of_the_prediction(tmp_path):
    from mslesions3d_amd import datasets as DS
    shapes = [(40, 44, 50), (52, 48, 46), (44, 70, 52)]
    data_dir = lesion_tree.make_tree(tmp_path, shapes)
    dm = DS.LesionsDataModule(data_dir=data_dir, centers=lesion_tree.CENTERS, spatial_size=(32, 32, 32))
    cases = DS._LesionCases(dm, dm.subjects_list)
    pdir = tmp_path / "preds"
    pdir.mkdir()
    names = ["_".join(cs) for cs in cases.subjects]
    _write_preds(str(pdir), names[0], [_box(0.1), _box(0.3)], [0.9, 0.2])
    _write_preds(str(pdir), names[1], [_box(0.2)], [0.7])
    (pdir / f"sub-{names[1]}_preds_views.json").write_text("{}")  # written by predict --views: the case frame
    logged = []
    det_b, det_l, det_s, gt_b, gt_l = EV.gather_lesion_cases(cases, str(pdir), 0.5, log=logged.append)
    assert len(det_b) == len(gt_b) == 2 and len(logged) == 1 and names[2] in logged[0]
    assert det_s[0].tolist() == [float(np.float32(0.9))] and det_s[1].tolist() == [float(np.float32(0.7))]
    fitted, case = cases[0], cases.case_sample(1)
    assert torch.equal(gt_b[0], fitted["boxes"]) and torch.equal(gt_l[0], fitted["labels"])
    assert torch.equal(gt_b[1], case["boxes"]) and torch.equal(gt_l[1], case["labels"])
    # the two frames differ for a case larger than the fit, and case_boxes gives each sample's own boxes
    for pos in range(3):
        for fit, sample in ((True, cases[pos]), (False, cases.case_sample(pos))):
            b, l = cases.case_boxes(pos, fit=fit)
            assert torch.equal(b, sample["boxes"]) and torch.equal(l, sample["labels"])
    assert not torch.equal(cases[1]["boxes"], case["boxes"])
    assert len(EV.gather_lesion_cases(cases, str(pdir), float("-inf"), log=lambda *_: None)[2][0]) == 2
