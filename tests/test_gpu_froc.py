"""FROC on the device (csrc/evaluate.hip, ev_froc_kernel): ``msl_evaluate_froc`` on the workspace of a completed
``msl_evaluate_detections`` call writes exactly the integers of the numpy twin ``utils.froc_host`` (itself pinned to the
oracle's matching rule by tests/test_froc_cpu.py); the sweep's own outputs are untouched; ``python -m mslesions3d_amd.eval
--froc`` writes the twin's values for the synthetic data set and for clinical cases."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from mslesions3d_amd import utils as U
from tests import lesion_tree

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = U.DEFAULT_FP_RATES
T = U.FROC_TILE


def _boxes(rs, n, lo_max=0.8, ext=(0.05, 0.25)):
    lo = rs.uniform(0, lo_max, (n, 3)).astype(np.float32)
    return np.concatenate([lo, lo + rs.uniform(*ext, (n, 3)).astype(np.float32)], 1)


def _split(total, n_img, rs):
    """``total`` detections dealt over ``n_img`` images, the last image left without any when there are enough images."""
    cuts = np.sort(rs.randint(0, total + 1, max(n_img - 2, 0)))
    counts = np.diff(np.concatenate([[0], cuts, [total]])).tolist() + ([0] if n_img > 1 else [])
    return counts[:n_img] if n_img > 1 else [total]


def _case(seed, n_img, total, n_gt=3, quant=8, label0=0.0, no_gt=(1,)):
    """``total`` detections in all: hits with jitter, duplicates, misses; scores quantised to 1/quant (ties); image(s)
    ``no_gt`` without ground truth; a share ``label0`` of label-0 rows."""
    rs = np.random.RandomState(seed)
    tb, tl, db, dl, ds = [], [], [], [], []
    for i, nd in enumerate(_split(total, n_img, rs)):
        ng = 0 if i in no_gt else n_gt
        t, d = _boxes(rs, ng), _boxes(rs, nd)
        if ng and nd:
            k = min(nd, 3 * ng)
            d[:k] = t[rs.randint(0, ng, k)] + rs.uniform(-0.03, 0.03, (k, 6)).astype(np.float32)
        sc = rs.uniform(0, 1, nd)
        sc = (np.round(sc * quant) / quant if quant else sc).astype(np.float32)
        lb = np.ones(nd, np.int64)
        lb[rs.rand(nd) < label0] = 0
        tb.append(t), tl.append(np.ones(ng, np.int64)), db.append(d), dl.append(lb), ds.append(sc)
    return db, dl, ds, tb, tl


def _dense_case(seed, n_img, total):
    """``total`` detections, nearly all of them true positives (one small ground-truth box each, 1 % replaced by misses),
    so that the operating points lie deep in the ranking: image 1 has up to 3 detections and no ground truth, the last
    image no detection, the others share the rest and have two boxes nobody finds."""
    rs = np.random.RandomState(seed)
    counts = [0] * n_img
    counts[1] = min(total, 3)
    for j in range(total - counts[1]):
        counts[(0, *range(2, n_img - 1))[j % (n_img - 2)]] += 1
    tb, tl, db, dl, ds = [], [], [], [], []
    for i, nd in enumerate(counts):
        ng = 0 if i == 1 else nd + 2
        t = _boxes(rs, ng, lo_max=0.9, ext=(0.02, 0.05))
        d = _boxes(rs, nd, lo_max=0.9, ext=(0.02, 0.05))
        if ng:
            hit = rs.rand(nd) >= 0.01
            d[hit] = (t[:nd] + rs.uniform(-0.002, 0.002, (nd, 6)).astype(np.float32))[hit]
        sc = (np.round(rs.uniform(0, 1, nd) * 64) / 64).astype(np.float32)
        tb.append(t), tl.append(np.ones(ng, np.int64)), db.append(d), dl.append(np.ones(nd, np.int64)), ds.append(sc)
    return db, dl, ds, tb, tl


def _same_ints(a, b, what):
    for k in ("k", "tp", "gw", "nw"):
        assert a[k].dtype == b[k].dtype == np.int64 and np.array_equal(a[k], b[k]), (what, k, a[k], b[k])
    assert np.array_equal(a["scores"].view(np.uint32), b["scores"].view(np.uint32)), what


def _both(case, ious, rates, w, what):
    dev = U.evaluate_froc_ints(*case, ious, rates, w)
    host = U.froc_host(*case, ious, rates, w)
    _same_ints(dev, host, what)
    return host


# ---- G1 ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", [0, 1, T - 1, T, T + 1, 2 * T + 1])
def test_tile_boundaries(D):
    N = 7
    case = _dense_case(D, N, D)
    assert sum(len(s) for s in case[2]) == D and len(case[2][-1]) == 0 and len(case[4][1]) == 0
    w = U.bootstrap_weights(N, 3, seed=D)
    w[1, 0] = w[2, 3] = w[3, 5] = 0
    assert (w[1:] == 0).any() and (w[0] == 1).all()
    host = _both(case, [0.1, 0.5], RATES, w, f"D={D}")
    assert host["k"].shape == (4, 2, 7) and host["k"].max() <= D
    if D == 0:
        assert not host["k"].any() and not host["tp"].any()
    if D > T:  # operating points in every tile
        assert host["k"][0].max() > 2 * (D // 2) >= 2 * (T // 2) and (host["k"][0] < T).any() and len(np.unique(host["k"])) > 8


# ---- G2 ---------------------------------------------------------------------------------------------------------------

def test_one_image():
    case = _case(1, 1, 300, no_gt=())
    _both(case, [0.1, 0.5], RATES, np.array([[1], [3], [0]], np.int32), "N=1")


def test_no_ground_truth_at_all():
    case = _case(2, 5, 200, no_gt=(0, 1, 2, 3, 4))
    host = _both(case, [0.5], RATES, U.bootstrap_weights(5, 2, 1), "G=0")
    assert not host["gw"].any() and not host["tp"].any() and host["k"].any()


def test_all_scores_equal():
    db, dl, ds, tb, tl = _case(3, 6, T + 37)
    ds = [np.full_like(s, 0.5) for s in ds]
    host = _both((db, dl, ds, tb, tl), [0.1, 0.5], RATES, U.bootstrap_weights(6, 3, 2), "ties")
    K = T + 37
    assert set(np.unique(host["k"]).tolist()) <= {0, K} and (host["k"] == 0).any()  # the only realisable cuts


def test_label_zero_rows_shorten_the_ranking():
    case = _case(4, 6, T + 200, label0=0.3)
    K = sum(int((l == 1).sum()) for l in case[1])
    assert K < T + 200
    host = _both(case, [0.1, 0.5], RATES, U.bootstrap_weights(6, 3, 3), "K<D")
    assert host["scores"].shape == (K,) and host["k"].max() <= K


def test_extreme_rates_and_sixteen_rates():
    case = _case(5, 6, 500, quant=0)
    K = 500
    tiny, huge = (1, 1 << 20), (1 << 20, 1)
    sixteen = [tiny, huge] + [(n, d) for n, d in ((1, 16), (1, 8), (3, 16), (1, 4), (1, 3), (1, 2), (2, 3), (1, 1), (3, 2), (2, 1),
                                                  (3, 1), (4, 1), (8, 1), (1000, 7))]
    assert len(sixteen) == U.FROC_MAX_RATES
    w = U.bootstrap_weights(6, 3, 4)
    host = _both(case, [0.1, 0.5], sixteen, w, "16 rates")
    assert (host["k"][0, :, 1] == K).all()  # every false positive is allowed: the whole ranking
    # rank 0 made a false positive (a far-away box with the top score): nothing but the empty prefix has FP = 0
    db, dl, ds, tb, tl = case
    db[1], dl[1], ds[1] = np.concatenate([[[0.9, 0.9, 0.9, 0.95, 0.95, 0.95]], db[1]]).astype(np.float32), \
        np.concatenate([[1], dl[1]]), np.concatenate([[2.0], ds[1]]).astype(np.float32)
    host = _both((db, dl, ds, tb, tl), [0.5], [tiny, huge], np.ones((1, 6), np.int32), "k* = 0")
    assert host["k"][0, 0].tolist() == [0, K + 1] and host["tp"][0, 0, 0] == 0
    s = U.froc_summary(host, [0.5], [tiny, huge])[0.5]
    assert s["score_threshold"][0] == float("inf") and s["sensitivity"][0] == 0.0


def test_argument_checks():
    from mslesions3d_amd import _lib
    lib = _lib.load()
    case = _case(6, 3, 50)
    plan = U.prepare_evaluation(*case, [0.5], [0.0])
    f = U.prepare_froc(plan, [3, 0, 3], np.ones((1, 3), np.int32), list(RATES))
    ws, n, sc, out = U.ptr(plan["ws"]), plan["ws_bytes"], U.ptr(plan["sorted_scores"]), U.ptr(f["out"])
    some = U.ptr(f["keep"][0])
    call = lambda *a: lib.msl_evaluate_froc(*a, None)
    assert call(ws, n, sc, 50, 3, plan["G"], 1, some, some, 1, some, 17, out) == -2      # more than 16 rates
    assert call(ws, n, sc, 50, 3, plan["G"], 1, some, some, 1, some, 0, out) == -1
    assert call(ws, n, sc, 50, 0, plan["G"], 1, some, some, 1, some, 7, out) == -1
    assert call(ws, n, sc, 50, 3, plan["G"], 1, some, some, 0, some, 7, out) == -1
    assert call(None, n, sc, 50, 3, plan["G"], 1, some, some, 1, some, 7, out) == -1
    assert call(ws, n - 1, sc, 50, 3, plan["G"], 1, some, some, 1, some, 7, out) == -1   # not that call's workspace
    assert call(ws, n, None, 50, 3, plan["G"], 1, some, some, 1, some, 7, out) == -1
    assert call(ws, n, sc, 2 ** 29, 3, plan["G"], 1, some, some, 1, some, 7, out) == -2  # beyond int32 indexing
    with pytest.raises(ValueError, match="NaN"):
        bad = [s.copy() for s in case[2]]
        bad[0][0] = np.nan
        U.evaluate_froc(case[0], case[1], bad, case[3], case[4])


# ---- G3 ---------------------------------------------------------------------------------------------------------------

def test_froc_leaves_the_sweep_outputs_alone():
    case = _case(7, 9, 2 * T + 5, label0=0.05)
    ious, scs = [0.1, 0.5], [0.0, 0.5]
    alone = U.prepare_evaluation(*case, ious, scs)
    alone["launch"]()
    want = alone["out"].cpu().numpy().view(np.uint32)
    plan = U.prepare_evaluation(*case, ious, scs)
    g = [int((l == 1).sum()) for l in case[4]]
    f = U.prepare_froc(plan, g, U.bootstrap_weights(9, 5, 0), list(RATES))
    plan["launch"]()
    before = plan["out"].cpu().numpy().view(np.uint32)
    ws_before = plan["ws"].cpu().numpy()
    f["launch"]()
    ints = U.froc_ints(f["out"].cpu().numpy(), f["R1"], f["n_iou"], f["n_rates"], None)
    assert np.array_equal(plan["out"].cpu().numpy().view(np.uint32), before) and np.array_equal(before, want)
    assert np.array_equal(plan["ws"].cpu().numpy(), ws_before)  # the workspace is read, not written
    host = U.froc_host(*case, ious, RATES, U.bootstrap_weights(9, 5, 0))
    assert np.array_equal(ints["k"], host["k"]) and np.array_equal(ints["tp"], host["tp"])
    a = U.evaluate_detections(*case, [torch.zeros(len(l), dtype=torch.bool) for l in case[4]], min_overlaps=ious,
                              min_scores=scs)
    plan["launch"]()  # the sweep again on the same workspace, after FROC has read it
    assert np.array_equal(plan["out"].cpu().numpy().view(np.uint32), want) and len(a) == 4


# ---- G4 ---------------------------------------------------------------------------------------------------------------

def test_end_to_end_equals_the_twin_and_repeats():
    rs = np.random.RandomState(8)
    n_img, per = 40, 100
    tb = [_boxes(rs, 0 if i % 13 == 12 else int(rs.randint(1, 7))) for i in range(n_img)]
    tl = [np.ones(len(t), np.int64) for t in tb]
    db, dl, ds = [], [], []
    for t in tb:
        d = _boxes(rs, per)
        if len(t):
            d[:3 * len(t)] = np.repeat(t, 3, axis=0) + rs.uniform(-0.03, 0.03, (3 * len(t), 6)).astype(np.float32)
        db.append(d), dl.append(np.ones(per, np.int64)), ds.append((np.round(rs.uniform(0, 1, per) * 256) / 256).astype(np.float32))
    ious = [0.1, 0.5]
    a = U.evaluate_froc(db, dl, ds, tb, tl, min_overlaps=ious, n_boot=64, seed=11)
    b = U.evaluate_froc(db, dl, ds, tb, tl, min_overlaps=ious, n_boot=64, seed=11)
    want = U.froc_summary(U.froc_host(db, dl, ds, tb, tl, ious, RATES, U.bootstrap_weights(n_img, 64, 11)), ious, RATES)
    assert list(a) == list(want) == ious
    for ov in ious:
        assert list(a[ov]) == list(want[ov])
        for k in want[ov]:
            assert a[ov][k] == want[ov][k] and b[ov][k] == a[ov][k], (ov, k, a[ov][k], want[ov][k])
        assert a[ov]["n_boot"] == 64 and a[ov]["n_cases"] == n_img and a[ov]["ci_low"][3] <= a[ov]["ci_high"][3]
        assert 0.0 < a[ov]["cpm"] <= 1.0
    other = U.evaluate_froc(db, dl, ds, tb, tl, min_overlaps=ious, n_boot=64, seed=12)
    assert other[0.5]["sensitivity"] == a[0.5]["sensitivity"] and other[0.5]["ci_low"] != a[0.5]["ci_low"]


# ---- G5 ---------------------------------------------------------------------------------------------------------------

def _run_eval(args):
    r = subprocess.run([sys.executable, "-m", "mslesions3d_amd.eval"] + args, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return r.stdout


def _read_all(pdir, subjects):
    from mslesions3d_amd import eval as EV
    preds = [EV.retrieve_boxes(pdir, s, confidence_threshold=float("-inf")) for s in subjects]
    return [p[0] for p in preds], [p[1] for p in preds], [p[2] for p in preds]


def _want_files(det, gt_b, gt_l, ious, n_boot, seed):
    from mslesions3d_amd import eval as EV
    w = U.bootstrap_weights(len(gt_l), n_boot, seed)
    s = U.froc_summary(U.froc_host(*det, gt_b, gt_l, ious, RATES, w), ious, RATES)
    return {EV.froc_file_name(ov): json.dumps(EV.froc_json(s[ov]), indent=4) for ov in ious}


def test_eval_entry_point_writes_the_twin_froc(tmp_path):
    from mslesions3d_amd import datasets as DS
    from mslesions3d_amd.predict import save_predictions
    data = str(tmp_path / "data")
    DS.generate_artificial_dataset(data, "toy", num_images=20, image_size=(32, 32, 32), object_size=(4, 8))
    ds = DS.ExampleDataset(n_classes=1, percentage=1., num_workers=0, data_dir=data, dataset_name="toy")
    ds.setup(stage="predict_train")
    subjects = [s for b in ds._loader(ds.predict_dataset, False, 32) for s in zip(b["subject"], b["boxes"], b["labels"])]
    flat = tmp_path / "flat"
    flat.mkdir()
    rs = np.random.RandomState(5)
    for subj, gt, _ in subjects:
        t = gt.numpy().reshape(-1, 6)
        nd = int(rs.randint(0, 12))
        b = _boxes(rs, nd, lo_max=0.7)
        k = min(nd, len(t))
        b[:k] = np.clip(t[:k] + rs.uniform(-0.04, 0.04, (k, 6)).astype(np.float32), 0, 1)
        s = (np.round(rs.uniform(0, 1, nd) * 10) / 10).astype(np.float32)
        save_predictions(subj, (32, 32, 32), b, np.where(rs.rand(nd) < 0.1, 2, 1), s, 0.0, str(flat))
    base = ["-d", data, "-dn", "toy", "-pd", str(flat), "-sc", "0.5", "-iou", "0.1,0.5", "-nw", "0", "-ps", "train"]
    from mslesions3d_amd import eval as EV
    EV.evaluate(str(flat), data, None, dataset_name="toy", num_workers=0, confidence_threshold=[0.5], min_iou=[0.1, 0.5])  # no new flag
    plain = {f: (flat / f).read_text() for f in os.listdir(flat) if f.startswith("metrics_")}
    assert len(plain) == 2 and not [f for f in os.listdir(flat) if f.startswith("froc_")]
    out = _run_eval(base + ["--froc", "--bootstrap", "16"])
    assert "FROC for IoU = 0.5" in out
    assert plain == {f: (flat / f).read_text() for f in os.listdir(flat) if f.startswith("metrics_")}  # as without --froc
    want = _want_files(_read_all(str(flat), [s for s, _, _ in subjects]), [g for _, g, _ in subjects],
                       [l for _, _, l in subjects], [0.1, 0.5], 16, 0)
    assert len(want) == 2
    for fname, text in want.items():
        assert (flat / fname).read_text() == text, fname
    assert json.loads(want["froc_(min_IoU=0.5).json"])["n_boot"] == 16


def test_eval_entry_point_on_clinical_cases(tmp_path):
    from mslesions3d_amd import datasets as DS
    from mslesions3d_amd.predict import save_predictions
    size = (32, 32, 32)
    data_dir = lesion_tree.make_tree(tmp_path, [(40, 44, 50), (52, 48, 46), (44, 70, 52), (60, 50, 72), (48, 64, 64)])
    dm = DS.LesionsDataModule(data_dir=data_dir, centers=lesion_tree.CENTERS, spatial_size=size)
    dm.setup(stage="predict_train")
    cases = dm.predict_dataset
    pdir = tmp_path / "preds"
    pdir.mkdir()
    rs = np.random.RandomState(2)
    gt_b, gt_l, names = [], [], []
    for pos in range(len(cases)):
        views = pos % 2 == 1  # every other case was predicted through the multi-view route: the case frame
        sample = cases.case_sample(pos) if views else cases[pos]
        t = sample["boxes"].numpy().reshape(-1, 6)
        b = np.concatenate([t + rs.uniform(-0.02, 0.02, t.shape).astype(np.float32), _boxes(rs, 4)]).astype(np.float32)
        name = "_".join(cases.subjects[pos])
        save_predictions(name, size, b, np.ones(len(b), np.int64), rs.uniform(0.05, 1, len(b)).astype(np.float32), 0.0, str(pdir))
        if views:
            (pdir / f"sub-{name}_preds_views.json").write_text("{}")
        gt_b.append(sample["boxes"]), gt_l.append(sample["labels"]), names.append(name)
    assert len(names) == 4
    _run_eval(["-dm", "lesions", "-d", data_dir, "--centers", *lesion_tree.CENTERS, "--spatial_size", "32", "32", "32",
               "-pd", str(pdir), "-sc", "0.5", "-iou", "0.1", "-nw", "0", "-ps", "train", "--froc", "--bootstrap", "8",
               "--bootstrap_seed", "3", "--froc_rates", "0.5,1,2"])
    w = U.bootstrap_weights(4, 8, 3)
    rates = [(1, 2), (1, 1), (2, 1)]
    from mslesions3d_amd import eval as EV
    s = U.froc_summary(U.froc_host(*_read_all(str(pdir), names), gt_b, gt_l, [0.1], rates, w), [0.1], rates)[0.1]
    assert (pdir / "froc_(min_IoU=0.1).json").read_text() == json.dumps(EV.froc_json(s), indent=4)
    assert s["n_lesions"] > 0 and s["n_cases"] == 4 and (pdir / "metrics_(min_IoU=0.1_min_score=0.5).json").exists()
