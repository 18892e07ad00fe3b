"""Eval by lesion size on the device (csrc/evaluate.hip, ev_stratify_kernel + ev_strata_count_kernel):
``msl_evaluate_strata`` on the buffers of a completed ``msl_evaluate_detections`` call writes exactly the integers of the
numpy twin ``utils.strata_host`` (itself pinned to the definitions by tests/test_strata_cpu.py); the sweep's and FROC's
buffers are untouched; ``python -m mslesions3d_amd.eval --size_bins`` writes the twin's values."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from mslesions3d_amd import utils as U
from tests import strata_cases as SC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = U.DEFAULT_FP_RATES
IOUS = [0.1, 0.5]
SCORES = [0.0, 0.5, 0.7, 2.0]
MAP_NAMES = ["mixed", "no_detections", "image_without_gt"]


def _voxels(N, seed):
    return (np.random.RandomState(seed).randint(20, 41, N) ** 3).astype(np.float64)


def _device(case, voxels, edges, ious, w, cuts, scores=(0.0,)):
    """One sweep and one ``msl_evaluate_strata`` call at host-given cuts -> the integers, like ``strata_host``."""
    plan = U.prepare_evaluation(*case, ious, list(scores))
    s = U.prepare_strata(plan, voxels, edges, w, cuts)
    plan["launch"]()
    s["launch"]()
    K = int(plan["ws"][:8].view(torch.int32)[1].item())
    got = U.strata_ints(s["out"].cpu().numpy(), s["R1"], s["n_iou"], s["n_cuts"], s["S1"],
                        np.clip(s["cuts"].cpu().numpy(), 0, K))
    return got


def _both(case, voxels, edges, ious, w, cuts, what):
    host = U.strata_host(*case, voxels, edges, ious, w, cuts)
    SC.same_ints(_device(case, voxels, edges, ious, w, cuts), host, what)
    return host


def _cpu_cases():
    return [("map:" + n, SC.map_case(n)) for n in MAP_NAMES] + [(f"seed{s}", SC.random_case(s)) for s in range(8)]


@pytest.mark.parametrize("name,case", _cpu_cases(), ids=[n for n, _ in _cpu_cases()])
def test_the_cpu_cases_through_the_public_route(name, case):
    """Sweep, FROC and strata chained on the device, the cuts never leaving it, against the twin at the host's cuts."""
    N = len(case[4])
    w = U.bootstrap_weights(N, 2, seed=N)
    w[1, 0] = 0
    vox = _voxels(N, 1)
    dev = U.evaluate_strata_ints(*case, vox, SC.EDGES, IOUS, SCORES, RATES, w)
    cuts = U.strata_cuts_host(*case, IOUS, SCORES, RATES, w)
    SC.same_ints(dev, U.strata_host(*case, vox, SC.EDGES, IOUS, w, cuts), name)
    dev = U.evaluate_strata_ints(*case, vox, SC.EDGES, IOUS, SCORES, None, w)  # without FROC: the score cuts alone
    SC.same_ints(dev, U.strata_host(*case, vox, SC.EDGES, IOUS, w, cuts[:, :, :len(SCORES)]), name)


def test_edge_values_zero_volume_and_nan_boxes():
    case = SC.edge_case()
    w = np.array([[1, 1, 1], [2, 0, 3]], np.int32)
    host = _both(case, 1000.0, SC.EDGES, IOUS, w, np.array([0, 1, 2, 3, 4, 5]), "edge")
    assert host["gw"].tolist() == [[1, 1, 1, 1, 1], [2, 0, 2, 2, 3]] and host["det_unbinned"].tolist() == [1, 3]


@pytest.mark.parametrize("R", [0, 32])
def test_forty_by_hundred(R):
    case = SC.grid_case(8, 40, 100)
    w = U.bootstrap_weights(40, R, seed=5)
    assert w.shape[0] in (1, 33)
    vox = _voxels(40, 3)
    cuts = U.strata_cuts_host(*case, IOUS, [0.1, 0.5, 0.9], RATES, w)
    host = _both(case, vox, SC.EDGES, IOUS, w, cuts, f"R={R}")
    assert (host["gw"][0, :4] > 0).sum() >= 3 and host["tp"][0].any() and host["fp"][0].any()
    if R:
        assert len({tuple(c) for c in cuts[:, 1, 3:].tolist()}) > 1  # the rows cut at different ranks


def test_one_large_image_several_rank_tiles_and_ground_truth_chunks():
    rs = np.random.RandomState(4)
    t = SC.boxes(rs, 300, lo_max=0.9, ext=(0.01, 0.09))
    d = SC.boxes(rs, 5000, lo_max=0.9, ext=(0.01, 0.09))
    d[:900] = np.repeat(t, 3, axis=0) + rs.uniform(-0.004, 0.004, (900, 6)).astype(np.float32)
    case = ([d, SC.boxes(rs, 7)], [np.ones(5000, np.int64), np.ones(7, np.int64)],
            [(np.round(rs.uniform(0, 1, 5000) * 512) / 512).astype(np.float32), rs.uniform(0, 1, 7).astype(np.float32)],
            [t, np.zeros((0, 6), np.float32)], [np.ones(300, np.int64), np.zeros(0, np.int64)])
    w = np.array([[1, 1], [3, 0], [0, 2]], np.int32)
    cuts = np.array([5007, 0, 4096, 1, 255, 256, 257, 1023, 1024, 1025, 2500, 4999, 5000, 5006], np.int64)
    host = _both(case, [64.0 ** 3, 32.0 ** 3], SC.EDGES, IOUS, w, cuts, "5000")
    assert host["tp"][0, 0, 0, :4].sum() > 200 and (host["gw"][0, :4] > 0).sum() >= 3


@pytest.mark.parametrize("n_cuts", [1, 32])
def test_cuts_unsorted_and_repeated(n_cuts):
    case = SC.random_case(11)
    N = len(case[4])
    K = sum(int((l == 1).sum()) for l in case[1])
    rs = np.random.RandomState(n_cuts)
    cuts = rs.randint(0, K + 1, (3, 2, n_cuts)).astype(np.int64)
    if n_cuts > 1:
        cuts[:, :, 5] = cuts[:, :, 2]           # repeats
        cuts[0, 0, :4] = [K, 0, K, 0]
        cuts[1, 1, 7:9] = [K + 50, -3]          # clamped to K and to 0
        assert (np.diff(cuts, axis=2) < 0).any()
    _both(case, _voxels(N, 5), SC.EDGES, IOUS, U.bootstrap_weights(N, 2, 1), cuts, f"n_cuts={n_cuts}")


@pytest.mark.parametrize("edges", [[100.0], [float(2 ** j) for j in range(15)]], ids=["S=2", "S=16"])
def test_two_and_sixteen_strata(edges):
    case = SC.random_case(3, max_det=30)
    N = len(case[4])
    w = U.bootstrap_weights(N, 3, 0)
    host = _both(case, _voxels(N, 2), edges, IOUS, w, U.strata_cuts_host(*case, IOUS, [0.25], RATES, w), str(len(edges)))
    assert host["tp"].shape[-1] == len(edges) + 2


def test_heavy_score_ties():
    case = SC.grid_case(9, 20, 60, quant=2)  # three distinct scores
    w = U.bootstrap_weights(20, 4, 2)
    cuts = np.concatenate([U.strata_cuts_host(*case, IOUS, [0.5, 1.0], RATES, w),
                           np.broadcast_to(np.array([7, 600, 601, 1199]), (5, 2, 4))], axis=2)  # cuts inside the runs of ties
    _both(case, _voxels(20, 7), SC.EDGES, IOUS, w, cuts, "ties")


def test_nan_scores_are_refused():
    db, dl, ds, tb, tl = SC.random_case(2)
    ds = [np.where(np.arange(len(s)) == 0, np.nan, s).astype(np.float32) for s in ds]
    with pytest.raises(ValueError, match="NaN"):
        U.evaluate_strata(db, dl, ds, tb, tl, 1000.0, SC.EDGES)


def test_strata_leaves_the_sweep_and_froc_outputs_alone():
    case = SC.grid_case(7, 9, 250)
    scs = [0.0, 0.5]
    w = U.bootstrap_weights(9, 5, 0)
    g = [int((l == 1).sum()) for l in case[4]]
    plan = U.prepare_evaluation(*case, IOUS, scs)
    f = U.prepare_froc(plan, g, w, list(RATES))
    plan["launch"]()
    f["launch"]()
    cuts = f["out"][:6 * 2 * 7 * 2].reshape(6, 2, 7, 2)[..., 0].contiguous()
    s = U.prepare_strata(plan, _voxels(9, 1), SC.EDGES, w, cuts)
    out0, ws0, froc0 = plan["out"].cpu().numpy().view(np.uint32), plan["ws"].cpu().numpy(), f["out"].cpu().numpy()
    s["launch"]()
    a = s["out"].cpu().numpy()
    assert np.array_equal(plan["out"].cpu().numpy().view(np.uint32), out0)
    assert np.array_equal(plan["ws"].cpu().numpy(), ws0) and np.array_equal(f["out"].cpu().numpy(), froc0)
    s["launch"]()  # two runs are bit-equal
    assert np.array_equal(s["out"].cpu().numpy(), a)
    host = U.strata_host(*case, _voxels(9, 1), SC.EDGES, IOUS, w, cuts.cpu().numpy())
    SC.same_ints(U.strata_ints(a, 6, 2, 7, 5, host["cuts"]), host, "after froc")
    plan["launch"]()  # the sweep again on the same workspace, after strata has read it
    assert np.array_equal(plan["out"].cpu().numpy().view(np.uint32), out0)


def test_refused_arguments_and_guard_bands():
    from mslesions3d_amd import _lib
    lib = _lib.load()
    case = SC.random_case(6)
    N = len(case[4])
    plan = U.prepare_evaluation(*case, IOUS, [0.0])
    w = U.bootstrap_weights(N, 2, 0)
    s = U.prepare_strata(plan, 1000.0, SC.EDGES, w, np.array([3, 50, 0]))
    plan["launch"]()
    n, guard = s["out"].numel(), 64
    pattern = torch.full((n + 2 * guard,), -0x0123456789ABCDEF, dtype=torch.int64, device=s["out"].device)
    args = list(s["args"])
    OUT = 19
    args[OUT] = pattern.data_ptr() + 8 * guard
    names = ["ws", "ws_bytes", "eval_out", "D", "N", "G", "n_iou", "n_sc", "det_rows", "obj_off", "voxels", "edges", "n_edges",
             "weights", "R1", "cuts", "n_cuts", "sws", "sws_bytes", "out"]
    at = {k: i for i, k in enumerate(names)}

    def call(**kw):
        a = list(args)
        for k, v in kw.items():
            a[at[k]] = v
        return lib.msl_evaluate_strata(*a, None)

    assert call(n_edges=16) == -2 and call(n_cuts=33) == -2 and call(D=2 ** 29) == -2
    for kw in (dict(ws=None), dict(eval_out=None), dict(det_rows=None), dict(obj_off=None), dict(voxels=None), dict(edges=None),
               dict(weights=None), dict(cuts=None), dict(sws=None), dict(out=None), dict(N=0), dict(R1=0), dict(n_edges=0),
               dict(n_cuts=0), dict(n_iou=0), dict(n_sc=0), dict(D=-1), dict(ws_bytes=args[at["ws_bytes"]] - 1),
               dict(sws_bytes=args[at["sws_bytes"]] - 1)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert bool((pattern == -0x0123456789ABCDEF).all())  # nothing launched, nothing written
    assert call() == 0
    got = pattern.cpu().numpy()
    assert (got[:guard] == -0x0123456789ABCDEF).all() and (got[-guard:] == -0x0123456789ABCDEF).all()
    host = U.strata_host(*case, 1000.0, SC.EDGES, IOUS, w, np.array([3, 50, 0]))
    SC.same_ints(U.strata_ints(got[guard:guard + n], 3, 2, 3, 5, host["cuts"]), host, "guarded")


# ---- entry point --------------------------------------------------------------------------------------------------------

def _run_eval(args):
    r = subprocess.run([sys.executable, "-m", "mslesions3d_amd.eval"] + args, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return r.stdout


def test_eval_entry_point_writes_the_twin_strata(tmp_path):
    import argparse

    from mslesions3d_amd import datasets as DS
    from mslesions3d_amd import eval as EV
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
        b = SC.boxes(rs, nd, lo_max=0.7)
        k = min(nd, len(t))
        b[:k] = np.clip(t[:k] + rs.uniform(-0.04, 0.04, (k, 6)).astype(np.float32), 0, 1)
        s = (np.round(rs.uniform(0, 1, nd) * 10) / 10).astype(np.float32)
        save_predictions(subj, (32, 32, 32), b, np.where(rs.rand(nd) < 0.1, 2, 1), s, 0.0, str(flat))
    ious, scs, edges = [0.1, 0.5], [0.3, 0.5], [27.0, 125.0, 1000.0]
    # the command without --size_bins, in this process: the files it has always written, and no other
    EV.evaluate(str(flat), data, None, dataset_name="toy", num_workers=0, confidence_threshold=scs, min_iou=ious,
                options=argparse.Namespace(froc=True, bootstrap=20))
    listing = lambda: sorted(f for f in os.listdir(flat) if not f.startswith("sub-"))
    plain = {f: (flat / f).read_bytes() for f in listing()}
    assert sorted(plain) == sorted([EV.metrics_file_name(i, s) for i in ious for s in scs] + [EV.froc_file_name(i) for i in ious])
    out = _run_eval(["-d", data, "-dn", "toy", "-pd", str(flat), "-sc", "0.3,0.5", "-iou", "0.1,0.5", "-nw", "0", "-ps", "train",
                     "--froc", "--bootstrap", "20", "--size_bins", "27,125,1000"])
    assert "Lesions by size for IoU = 0.5" in out
    assert {f: (flat / f).read_bytes() for f in listing() if not f.startswith("strata_")} == plain
    assert [f for f in listing() if f.startswith("strata_")] == [EV.strata_file_name(i) for i in ious]
    preds = [EV.retrieve_boxes(str(flat), s, confidence_threshold=float("-inf")) for s, _, _ in subjects]
    case = ([p[0] for p in preds], [p[1] for p in preds], [p[2] for p in preds], [g for _, g, _ in subjects],
            [l for _, _, l in subjects])
    N = len(subjects)  # the training split of the 20 generated images
    w = U.bootstrap_weights(N, 20, 0)
    voxels = [32 ** 3] * N
    ints = U.strata_host(*case, voxels, edges, ious, w, U.strata_cuts_host(*case, ious, scs, RATES, w))
    want = U.strata_summary(ints, edges, ious, U.strata_cut_labels(scs, RATES))
    for iou in ious:
        text = (flat / EV.strata_file_name(iou)).read_text()
        assert text == json.dumps(EV.strata_json(want[iou]), indent=4), iou
        d = json.loads(text)
        assert d["n_boot"] == 20 and d["n_cases"] == N and len(d["cuts"]) == 2 + 7 and sum(d["n_lesions"]) > 0
