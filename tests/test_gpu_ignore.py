"""Evaluation with ignored ground truth on the device (csrc/evaluate.hip): through the Python API
and the raw C ABI, every case of tests/ignore_cases.py gives the loop-form reference tests/ignore_ref.py - flags, claim
ranks, counts, FROC and strata integers exactly, summary floats bit for bit; without flags (``true_ignore`` all false,
``gt_ignore`` null) every output of the old entry point is reproduced bit for bit."""
import numpy as np
import pytest
import torch

from mslesions3d_amd import _lib
from mslesions3d_amd import utils as U
from tests import ignore_cases as C
from tests import ignore_ref as R

pytestmark = pytest.mark.gpu
ALL = list(C.SMALL) + list(C.LARGE)
NO_NAN = [n for n in ALL if n != "odd_scores"]  # FROC and strata refuse NaN scores


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _sweep(case, ious, scs, true_ignore):
    """One sweep -> host views of everything it writes."""
    plan = U.prepare_evaluation(*case[:5], ious, scs, true_ignore=true_ignore)
    plan["launch"]()
    torch.cuda.synchronize()
    return plan, _views(plan, plan["out"].cpu().numpy(), None if plan["absorbed"] is None else plan["absorbed"].cpu().numpy())


def _views(plan, host, absorbed):
    n_iou, n_sc, D, G = len(plan["ious"]), len(plan["scores"]), plan["D"], plan["G"]
    n_sum = n_iou * n_sc * U.METRIC_SUMMARY
    v = {"summary": host[:n_sum].reshape(n_iou, n_sc, U.METRIC_SUMMARY), "scores": host[n_sum:n_sum + D],
         "tp": host[n_sum + D:n_sum + D + n_iou * D].reshape(n_iou, D),
         "claim": host[n_sum + D + n_iou * D:n_sum + D + n_iou * (D + G)].view(np.int32).reshape(n_iou, G),
         "vol": host[n_sum + D + n_iou * (D + G):]}
    if absorbed is not None:
        v["abs"] = absorbed[:n_iou * n_sc].reshape(n_iou, n_sc)
        v["ab"] = absorbed[n_iou * n_sc:].reshape(n_iou, D)
    return v


@pytest.mark.parametrize("name", ALL)
def test_sweep_is_the_reference(name):
    c = C.get(name)
    case, ious, scs = c["case"], c["ious"], c["scores"]
    plan, v = _sweep(case, ious, scs, case[5])
    for t, thr in enumerate(ious):
        m = C.match(case, thr)
        K = m["K"]
        assert np.array_equal(_bits(v["scores"][:K]), _bits(m["score"])), (name, "rank order")
        assert np.array_equal(v["tp"][t, :K], m["tp"].astype(np.float32)) and not v["tp"][t, K:].any(), (name, thr, "TP")
        assert np.array_equal(v["ab"][t, :K], m["ab"]) and not v["ab"][t, K:].any(), (name, thr, "absorbed")
        assert np.array_equal(v["claim"][t], m["claim"]), (name, thr, "claim")
        for ci, sc in enumerate(scs):
            want, absorbed = R.summary(m, sc)
            print(name, thr, sc, v["summary"][t, ci], want, v["abs"][t, ci], absorbed)
            assert np.array_equal(_bits(v["summary"][t, ci]), _bits(want)), (name, thr, sc, v["summary"][t, ci], want)
            assert v["abs"][t, ci] == absorbed, (name, thr, sc)


@pytest.mark.parametrize("name", ["multiple_absorbed", "all_ignored", "random_3", "boxes_130"])
def test_detail_dict(name):
    c = C.get(name)
    case, ious, scs = c["case"], c["ious"], c["scores"] + [2.0]  # 2.0: nothing kept
    dif = [torch.zeros(len(l), dtype=torch.bool) for l in case[4]]
    got = U.evaluate_detections(*case[:5], dif, min_overlaps=ious, min_scores=scs, return_detail=True, true_ignore=case[5])
    short = U.evaluate_detections(*case[:5], dif, min_overlaps=ious, min_scores=scs, true_ignore=case[5])
    for thr in ious:
        m = C.match(case, thr)
        for sc in scs:
            d, (want, absorbed) = got[(thr, sc)], R.summary(m, sc)
            Kc = int(want[6])
            assert d["n_true_boxes"] == m["n_easy"] and d["n_ignored_boxes"] == m["n_ignored"]
            assert np.array_equal(d["TP"].numpy(), m["tp"][:Kc].astype(np.float32))
            assert np.array_equal(d["FP"].numpy(), m["fp"][:Kc].astype(np.float32))
            assert np.array_equal(d["absorbed"].numpy(), m["ab"][:Kc].astype(np.float32)) and int(d["absorbed"].sum()) == absorbed
            for i, key in ((0, "APs"), (1, "mAP"), (2, "precision"), (3, "recall"), (4, "f1_score")):
                assert np.array_equal(_bits(d[key]), _bits(want[i])), (name, thr, sc, key)
            found, lost = R.volumes(m, sc)
            assert np.array_equal(_bits(d["found_boxes_volumes_per_class"].numpy()), _bits(found))
            assert np.array_equal(_bits(d["not_found_boxes_volumes_per_class"].numpy()), _bits(lost))
            assert np.array_equal(_bits(short[(thr, sc)][1]), _bits(want[1]))


def _weights(c, name):
    N = len(c["case"][4])
    w = c["weights"] if "weights" in c else U.bootstrap_weights(N, 2, seed=N)
    if "weights" not in c:
        w[1, 0] = 0
    return w[:1] if name in C.LARGE else w


@pytest.mark.parametrize("name", NO_NAN)
def test_froc_is_the_reference(name):
    c = C.get(name)
    rates, w = c.get("rates", [(1, 2), (2, 1)]), _weights(c, name)
    got = U.evaluate_froc_ints(*c["case"][:5], c["ious"], rates, w, true_ignore=c["case"][5])
    want = R.froc(c["case"], c["ious"], rates, w, match=C.match)
    for k in ("k", "tp", "gw", "nw", "absorbed"):
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), (name, k, got[k], want[k])


@pytest.mark.parametrize("name", NO_NAN)
def test_strata_is_the_reference(name):
    c = C.get(name)
    w = _weights(c, name)
    edges, vox = c.get("edges", [27.0, 125.0, 1000.0]), c.get("voxels", 1000.0)
    rates = c.get("rates", [(1, 2), (2, 1)])
    got = U.evaluate_strata_ints(*c["case"][:5], vox, edges, c["ious"], c["scores"], rates, w, true_ignore=c["case"][5])
    want = R.strata(c["case"], vox, edges, c["ious"], w, got["cuts"], match=C.match)
    # the cuts themselves: K_c of every score threshold, then the reference's k* of every rate
    kc = [int(R.summary(C.match(c["case"], c["ious"][0]), s)[0][6]) for s in c["scores"]]
    k = R.froc(c["case"], c["ious"], rates, w, match=C.match)["k"]
    assert np.array_equal(got["cuts"][:, :, :len(kc)], np.broadcast_to(kc, got["cuts"][:, :, :len(kc)].shape))
    assert np.array_equal(got["cuts"][:, :, len(kc):], k)
    for key in ("tp", "fp", "gw", "det_unbinned", "nw", "cuts", "absorbed"):
        assert got[key].dtype == np.int64 and np.array_equal(got[key], want[key]), (name, key, got[key], want[key])


def test_flag_on_another_label_changes_nothing():
    c = C.get("other_label")
    _, a = _sweep(c["case"], c["ious"], c["scores"], c["case"][5])
    _, b = _sweep(c["same"], c["ious"], c["scores"], c["same"][5])
    for k in a:
        assert np.array_equal(a[k].view(np.uint32) if a[k].dtype == np.float32 else a[k],
                              b[k].view(np.uint32) if b[k].dtype == np.float32 else b[k]), k


@pytest.mark.parametrize("name", ["random_11", "boxes_130", "tile_boundary", "odd_scores"])
def test_no_flags_is_the_old_entry_point(name):
    c = C.get(name)
    case, ious, scs = c["case"], c["ious"], c["scores"]
    old, _ = _sweep(case, ious, scs, None)
    want = old["out"].cpu().numpy().view(np.uint32)
    # true_ignore all false
    none = [np.zeros(len(f), bool) for f in case[5]]
    plan, v = _sweep(case, ious, scs, none)
    assert np.array_equal(plan["out"].cpu().numpy().view(np.uint32), want) and not v["abs"].any() and not v["ab"].any()
    # the raw C ABI with gt_ignore null: the old workspace size suffices; `absorbed`, when given, is zeroed
    lib = _lib.load()
    ws = torch.empty_like(old["ws"])
    for absorbed in (None, torch.full((len(ious) * len(scs) + len(ious) * old["D"],), 7, dtype=torch.int32, device=ws.device)):
        out = torch.full_like(old["out"], float("nan"))
        a = list(old["args"])
        a[13], a[15] = U.ptr(ws), U.ptr(out)
        assert lib.msl_evaluate_detections_ign(*a, None, U.ptr(absorbed), None) == 0
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want)
        assert absorbed is None or not absorbed.any()
    if name != "odd_scores":  # the consumers of a workspace without flags
        w = U.bootstrap_weights(len(case[4]), 2, seed=1)
        a, b = U.evaluate_froc_ints(*case[:5], ious, [(1, 2), (2, 1)], w), \
            U.evaluate_froc_ints(*case[:5], ious, [(1, 2), (2, 1)], w, true_ignore=none)
        for k in ("k", "tp", "gw", "nw"):
            assert np.array_equal(a[k], b[k]), k
        sa = U.evaluate_strata_ints(*case[:5], 1000.0, [27.0, 125.0], ious, scs, None, w)
        sb = U.evaluate_strata_ints(*case[:5], 1000.0, [27.0, 125.0], ious, scs, None, w, true_ignore=none)
        for k in ("tp", "fp", "gw", "det_unbinned", "nw", "cuts"):
            assert np.array_equal(sa[k], sb[k]), k


def test_workspace_sizes_and_argument_checks():
    lib = _lib.load()
    sizes = [(0, 1, 0, 1, 1), (10, 3, 5, 2, 4), (16400, 5, 20, 2, 2), (2 ** 29, 3, 5, 1, 1), (10, 0, 5, 1, 1), (10, 3, 5, 0, 1),
             (10, 3, 5, 1, 0), (-1, 3, 5, 1, 1), (10, 3, 2 ** 30, 4, 1), (100, 3, 5, 65536, 1), (2 ** 27, 3, 5, 1, 1), (2 ** 28, 3, 5, 1, 1)]
    for s in sizes:
        old, new = lib.msl_evaluate_workspace_bytes(*s), lib.msl_evaluate_workspace_bytes_ign(*s)
        assert (old == 0) == (new == 0), s
        assert new == 0 or new > old, s
    assert [lib.msl_evaluate_workspace_bytes(*s) == 0 for s in sizes].count(True) >= 6
    c = C.get("multiple_absorbed")
    plan = U.prepare_evaluation(*c["case"][:5], [0.5], [0.0], true_ignore=c["case"][5])
    a = list(plan["args"])
    gi, ab = U.ptr(plan["gt_ignore"]), U.ptr(plan["absorbed"])
    assert lib.msl_evaluate_detections_ign(*a, gi, None, None) == -1          # flags without a place for the absorbed counts
    small = list(a)
    small[14] = lib.msl_evaluate_workspace_bytes(plan["D"], plan["N"], plan["G"], 1, 1)
    assert lib.msl_evaluate_detections_ign(*small, gi, ab, None) == -1        # flags need the larger workspace
    assert lib.msl_evaluate_detections_ign(*small, None, None, None) == 0     # no flags: the old size suffices
    assert lib.msl_evaluate_detections_ign(*a, gi, ab, None) == 0
    torch.cuda.synchronize()


def test_wrong_length_flags_are_refused_before_any_launch(monkeypatch):
    c = C.get("multiple_absorbed")["case"]
    calls = []
    monkeypatch.setattr(_lib, "call", lambda *a, **k: calls.append(a))
    dif = [torch.zeros(len(l), dtype=torch.bool) for l in c[4]]
    for bad in ([np.zeros(3, bool)], [np.zeros(2, bool), np.zeros(0, bool)], []):
        with pytest.raises(ValueError, match="true_ignore"):
            U.evaluate_detections(*c[:5], dif, true_ignore=bad)
        with pytest.raises(ValueError, match="true_ignore"):
            U.evaluate_froc(*c[:5], true_ignore=bad)
        with pytest.raises(ValueError, match="true_ignore"):
            U.evaluate_strata(*c[:5], 1000.0, [27.0], true_ignore=bad)
    assert not calls
