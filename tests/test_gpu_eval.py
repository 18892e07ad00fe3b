"""Dataset-scale evaluation on the device (csrc/evaluate.hip): every grid point of ``utils.evaluate_detections`` is
bit-identical to the host ``calculate_mAP`` on the detections with score >= min_score (itself pinned to the reference by
tests/test_host_cpu.py), well past the 4096-detection cap of the single-workgroup kernel, and ``python -m
mslesions3d_amd.eval`` writes the reference's metrics files with exactly the host's values."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.golden import cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b, what):
    """Bit-equal, NaN-equal."""
    if isinstance(a, dict):
        assert isinstance(b, dict) and sorted(a) == sorted(b), what
        for k in a:
            _same(a[k], b[k], f"{what}.{k}")
        return
    if torch.is_tensor(a) or torch.is_tensor(b):
        assert torch.is_tensor(a) and torch.is_tensor(b) and a.dtype == b.dtype, (what, a, b)
        x, y = a.numpy(), b.numpy()
        assert x.shape == y.shape, (what, x.shape, y.shape)
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (what, x, y)
        return
    assert type(a) is type(b), (what, type(a), type(b))
    assert a == b or (a != a and b != b), (what, a, b)
    if isinstance(a, float):
        assert np.float64(a).tobytes() == np.float64(b).tobytes(), (what, a, b)


def _filtered(c, sc):
    """eval.py's retrieve_boxes per image: keep iff float(score) >= float(min_score)."""
    keep = [np.asarray(s, np.float32).astype(np.float64) >= float(sc) for s in c["det_scores"]]
    return ([np.asarray(b, np.float32).reshape(-1, 6)[k] for b, k in zip(c["det_boxes"], keep)],
            [np.asarray(l, np.int64).reshape(-1)[k] for l, k in zip(c["det_labels"], keep)],
            [np.asarray(s, np.float32).reshape(-1)[k] for s, k in zip(c["det_scores"], keep)])


def _host(c, ov, sc, detail=True):
    from mslesions3d_amd.utils import calculate_mAP
    db, dl, ds = _filtered(c, sc)
    H = lambda xs: [torch.as_tensor(np.asarray(x)) for x in xs]
    dif = [torch.zeros(len(x), dtype=torch.bool) for x in c["true_labels"]]
    return calculate_mAP(H(db), H(dl), H(ds), H(c["true_boxes"]), H(c["true_labels"]), dif, min_overlap=ov,
                         return_detail=detail)


def _device(c, ious, scs, detail=True):
    from mslesions3d_amd.utils import evaluate_detections
    D = lambda xs: [torch.as_tensor(np.asarray(x)).to(DEV) for x in xs]
    dif = [torch.zeros(len(x), dtype=torch.bool) for x in c["true_labels"]]
    return evaluate_detections(D(c["det_boxes"]), D(c["det_labels"]), D(c["det_scores"]), D(c["true_boxes"]),
                               D(c["true_labels"]), dif, min_overlaps=ious, min_scores=scs, return_detail=detail)


def _check(c, ious, scs, what):
    got = _device(c, ious, scs)
    got_short = _device(c, ious, scs, detail=False)
    assert set(got) == {(i, s) for i in ious for s in scs}
    for ov in ious:
        for sc in scs:
            want = _host(c, ov, sc)
            _same(got[(ov, sc)], want, f"{what} IoU {ov} score {sc}")
            aps, m = _host(c, ov, sc, detail=False)
            _same(got_short[(ov, sc)][0], aps, f"{what} IoU {ov} score {sc} APs")
            _same(got_short[(ov, sc)][1], m, f"{what} IoU {ov} score {sc} mAP")


@pytest.mark.parametrize("name", list(cases.map_cases().keys()))
def test_evaluate_matches_host_on_map_fixtures(name):
    c = cases.map_cases()[name]
    scores = sorted({float(s) for x in c["det_scores"] for s in np.asarray(x).ravel()})
    scs = sorted({0.0, scores[len(scores) // 2]})  # a threshold equal to an existing score
    _check(c, [0.1, 0.5], scs, name)


def _boxes(rs, n, lo_max=0.8, ext=(0.02, 0.25)):
    lo = rs.uniform(0, lo_max, (n, 3)).astype(np.float32)
    return np.concatenate([lo, lo + rs.uniform(*ext, (n, 3)).astype(np.float32)], 1)


def _stress(seed, n_img, per_img, n_gt=5, quant=None, fixed_gt=False):
    """Hits with jitter, duplicates competing for one box, misses, label 0 / 2 detections, images without detections
    or without ground truth."""
    rs = np.random.RandomState(seed)
    tb, tl, db, dl, ds = [], [], [], [], []
    for i in range(n_img):
        ng = n_gt if fixed_gt else int(rs.randint(0, 2 * n_gt + 1))
        t = _boxes(rs, ng)
        lab = np.ones(ng, np.int64)
        if ng > 2:
            lab[rs.rand(ng) < 0.1] = 2
        nd = 0 if i % 17 == 16 else per_img
        d = _boxes(rs, nd)
        if ng and nd:
            k = min(nd, 3 * ng)
            d[:k] = t[rs.randint(0, ng, k)] + rs.uniform(-0.03, 0.03, (k, 6)).astype(np.float32)
        sc = rs.uniform(0, 1, nd).astype(np.float32)
        if quant:
            sc = (np.round(sc * quant) / quant).astype(np.float32)
        lb = np.ones(nd, np.int64)
        lb[rs.rand(nd) < 0.08] = 2
        lb[rs.rand(nd) < 0.04] = 0
        tb.append(t), tl.append(lab), db.append(d), dl.append(lb), ds.append(sc)
    return dict(det_boxes=db, det_labels=dl, det_scores=ds, true_boxes=tb, true_labels=tl)


def test_evaluate_matches_host_40x100():
    _check(_stress(1, 40, 100, quant=16), [0.1, 0.5], [0.0, 0.3, 0.5, 0.9], "40x100")


def test_evaluate_matches_host_300x100():
    c = _stress(2, 300, 100)
    assert sum(len(x) for x in c["det_labels"]) > 4096
    _check(c, [0.1, 0.5], [0.0, 0.7], "300x100")


def test_evaluate_matches_host_one_long_image():
    """20 k detections and 300 ground-truth boxes in one image: five lane chunks and a long serial walk."""
    c = _stress(3, 1, 20000, n_gt=300, quant=64, fixed_gt=True)
    assert len(c["true_labels"][0]) == 300
    _check(c, [0.1, 0.5], [0.0, 0.5], "one image")


def _hard_case():
    rs = np.random.RandomState(7)
    tb = [_boxes(rs, 6), _boxes(rs, 0), _boxes(rs, 4), _boxes(rs, 3), _boxes(rs, 5)]
    tb[0][2] = [.5, .5, .5, .5, .6, .6]  # zero-volume ground truth
    tl = [np.ones(len(t), np.int64) for t in tb]
    tl[4][1] = 2  # another class: ignored, but "not found" when nothing is detected
    db, dl, ds = [], [], []
    for i, t in enumerate(tb):
        if i == 3:  # no detections at all
            db.append(np.zeros((0, 6), np.float32)), dl.append(np.zeros(0, np.int64)), ds.append(np.zeros(0, np.float32))
            continue
        d = np.concatenate([t + rs.uniform(-0.02, 0.02, t.shape).astype(np.float32), t[:1], _boxes(rs, 6)]) if len(t) \
            else _boxes(rs, 8)
        n = len(d)
        s = rs.choice(np.array([0.0, -0.0, 0.25, 0.5, 0.75, 1.0, np.inf, -np.inf, np.nan, 0.7, 0.9], np.float32), n)
        lab = np.ones(n, np.int64)
        lab[rs.rand(n) < 0.15] = 0
        lab[rs.rand(n) < 0.15] = 2
        db.append(d.astype(np.float32)), dl.append(lab), ds.append(s.astype(np.float32))
    db[0][3] = [.5, .5, .5, .5, .6, .6]  # zero-volume detection: NaN IoU against the zero-volume box
    ds[0][:4] = np.array([0.5, 0.5, -0.0, 0.0], np.float32)  # ties within an image, +0.0 / -0.0
    ds[2][:2] = np.array([0.5, 0.0], np.float32)  # ties across images
    ds[4][0] = np.float32(np.nan)
    ds[4][1] = np.float32(-np.nan)
    return dict(det_boxes=db, det_labels=dl, det_scores=ds, true_boxes=tb, true_labels=tl)


def test_evaluate_hard_inputs():
    c = _hard_case()
    scs = [-np.inf, -1.0, 0.0, 0.5, 0.7, 0.9, float(np.float32(0.7)), 1.0, np.inf, 2.0]  # 2.0: above every finite score
    _check(c, [0.0, 0.1, 0.5], scs, "hard")


def test_evaluate_nothing_detected_branch():
    c = _hard_case()
    for s in c["det_scores"]:
        s[np.isposinf(s)] = 1.0
    got = _device(c, [0.5], [1.5])[(0.5, 1.5)]
    assert got["sorted_det_scores"] == {} and got["n_true_boxes"] == sum(int((l == 1).sum()) for l in c["true_labels"])
    assert got["not_found_boxes_volumes_per_class"].numel() == sum(len(t) for t in c["true_boxes"])
    _same(got, _host(c, 0.5, 1.5), "nothing detected")


def test_evaluate_grid_equals_independent_host_calls():
    c = _stress(4, 25, 60, quant=8)
    ious, scs = [0.1, 0.3, 0.5], [0.0, 0.125, 0.25, 0.5, 0.75, 0.875]
    got = _device(c, ious, scs)
    assert len(got) == 18
    for ov in ious:
        for sc in scs:
            _same(got[(ov, sc)], _host(c, ov, sc), f"grid {ov} {sc}")


def test_evaluate_four_million_detections_is_reproducible():
    """>= 2^22 class-1 detections (the host loop is far too slow to compare at this size): two calls agree bit for bit,
    and at every grid point the TP count equals the number of ground-truth boxes claimed."""
    n_img, per = 4096, 1032
    rs = np.random.RandomState(11)
    gt = [_boxes(rs, 5) for _ in range(n_img)]
    det_b = np.repeat(np.stack(gt), per // 5 + 1, axis=1)[:, :per] + rs.uniform(-0.05, 0.05, (n_img, per, 6)).astype(np.float32)
    det_s = (np.round(rs.uniform(0, 1, (n_img, per)) * 1024) / 1024).astype(np.float32)
    c = dict(det_boxes=list(det_b.astype(np.float32)), det_labels=[np.ones(per, np.int64)] * n_img, det_scores=list(det_s),
             true_boxes=gt, true_labels=[np.ones(5, np.int64)] * n_img)
    assert n_img * per >= 2 ** 22
    ious, scs = [0.1, 0.5], [0.0, 0.5, 0.9]
    a, b = _device(c, ious, scs), _device(c, ious, scs)
    for k in a:
        _same(a[k], b[k], f"repeat {k}")
        d = a[k]
        n_tp = int(d["TP"].sum())
        assert n_tp == d["found_boxes_volumes_per_class"].numel() <= 5 * n_img, k
        assert d["TP"].numel() == d["sorted_det_scores"][1].numel() == int((det_s.astype(np.float64) >= k[1]).sum())
        assert np.isclose(d["recall"], n_tp / (5 * n_img))
    assert a[(0.1, 0.0)]["found_boxes_volumes_per_class"].numel() > 0


# ---- python -m mslesions3d_amd.eval --------------------------------------------------------------------------------

def _loader(data, name, subset):
    from mslesions3d_amd.datasets import ExampleDataset
    ds = ExampleDataset(n_classes=1, percentage=1., num_workers=0, data_dir=data, dataset_name=name)
    ds.setup(stage="predict_train" if subset == "train" else "predict")
    return ds._loader(ds.predict_dataset, False, 32)


def _convert(metrics):
    """eval.py:134-147 restated: int / float / str kept, dicts per value, a one-element tensor a number, else a list."""
    def conv(t):
        return t.item() if t.numel() == 1 else t.tolist()
    return {k: (v if type(v) in (int, float, str) else {a: conv(b) for a, b in v.items()} if type(v) == dict else conv(v))
            for k, v in metrics.items()}


def _host_files(data, name, subset, pdir, ious, scs):
    from mslesions3d_amd.utils import calculate_mAP
    out = {}
    for sc in scs:
        db, dl, ds, gb, gl = [], [], [], [], []
        for batch in _loader(data, name, subset):
            try:
                preds = []
                for s in batch["subject"]:
                    with open(os.path.join(pdir, f"sub-{s}_preds.json")) as f:
                        infos = json.load(f).values()
                    keep = [(b, l, x) for b, _, l, x in infos if x >= sc]
                    preds.append((torch.FloatTensor([b for b, _, _ in keep]), torch.LongTensor([l for _, l, _ in keep]),
                                  torch.FloatTensor([x for _, _, x in keep])))
            except FileNotFoundError:
                continue
            db += [p[0] for p in preds]
            dl += [p[1] for p in preds]
            ds += [p[2] for p in preds]
            gb += list(batch["boxes"])
            gl += list(batch["labels"])
        dif = [torch.BoolTensor([False] * len(x)) for x in gl]
        for ov in ious:
            m = calculate_mAP(db, dl, ds, gb, gl, dif, min_overlap=ov, return_detail=True)
            out[f"metrics_(min_IoU={ov}_min_score={sc}).json"] = json.dumps(_convert(m), indent=4)
    return out


def test_eval_entry_point_writes_the_host_values(tmp_path):
    from mslesions3d_amd import datasets as DS
    from mslesions3d_amd.predict import save_predictions
    data = str(tmp_path / "data")
    DS.generate_artificial_dataset(data, "toy", num_images=44, image_size=(32, 32, 32), object_size=(4, 8))
    subjects = [s for b in _loader(data, "toy", "train") for s in zip(b["subject"], b["boxes"], b["labels"])]
    assert len(subjects) > 32  # two batches: the skip of the second one leaves the first
    flat = tmp_path / "flat"
    nested = tmp_path / "preds" / "toy" / "m1" / "train_set" / "min_score_0.0"
    rs = np.random.RandomState(5)
    for d in (flat, nested):
        d.mkdir(parents=True)
    for i, (subj, gt, lab) in enumerate(subjects):
        t = gt.numpy().reshape(-1, 6)
        nd = int(rs.randint(0, 12))
        b = _boxes(rs, nd, lo_max=0.7)
        k = min(nd, len(t))
        b[:k] = np.clip(t[:k] + rs.uniform(-0.04, 0.04, (k, 6)).astype(np.float32), 0, 1)
        s = (np.round(rs.uniform(0, 1, nd) * 10) / 10).astype(np.float32)
        lb = np.where(rs.rand(nd) < 0.1, 2, 1)
        for d in (flat, nested):
            save_predictions(subj, (32, 32, 32), b, lb, s, 0.0, str(d))
    os.remove(nested / f"sub-{subjects[-1][0]}_preds.json")  # the last batch of the nested layout is skipped
    ious, scs = [0.1, 0.5], [0.1, 0.5]
    env = dict(os.environ, PYTHONPATH=ROOT)
    for pd, extra, d in ((str(flat), [], flat), (str(tmp_path / "preds"), ["-mn", "m1"], nested)):
        cmd = [sys.executable, "-m", "mslesions3d_amd.eval", "-d", data, "-dn", "toy", "-pd", pd, "-sc", "0.1,0.5",
               "-iou", "0.1,0.5", "-nw", "0", "-ps", "train"] + extra
        r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
        assert f"Prediction directory: {d}" in r.stdout
        want = _host_files(data, "toy", "train", str(d), ious, scs)
        assert len(want) == 4
        for fname, text in want.items():
            assert (d / fname).read_text() == text, (d, fname)
    assert subjects[-1][0] in r.stdout  # the skipped subjects are named


def test_evaluate_without_any_detection():
    """Every image's detections are empty CPU tensors of shape (0,): the 'nothing detected' dict at every grid point."""
    rs = np.random.RandomState(9)
    tb = [_boxes(rs, 3), _boxes(rs, 0), _boxes(rs, 2)]
    tl = [np.array([1, 2, 1]), np.zeros(0, np.int64), np.ones(2, np.int64)]
    c = dict(det_boxes=[torch.zeros(0)] * 3, det_labels=[torch.zeros(0, dtype=torch.int64)] * 3,
             det_scores=[torch.zeros(0)] * 3, true_boxes=tb, true_labels=tl)
    got = _device(c, [0.1, 0.5], [0.0, 0.5])
    for k, d in got.items():
        _same(d, _host(c, k[0], k[1]), f"empty {k}")
        assert d["n_true_boxes"] == 4 and d["not_found_boxes_volumes_per_class"].numel() == 5
