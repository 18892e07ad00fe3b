"""Eval by lesion size on the host (DESIGN.md "Eval by lesion size"): the numpy twin ``utils.strata_host`` against a
brute-force restatement of the definitions on top of the oracle's matching rule, the identities that tie it to FROC, the
reference's found / not-found volume lists, the edge cases of the binning, ``strata_summary`` and the host pieces of
``python -m mslesions3d_amd.eval --size_bins``.  CPU only (the kernel: tests/test_gpu_strata.py)."""
import json
import os
import re

import numpy as np
import pytest
import torch

from mslesions3d_amd import eval as EV
from mslesions3d_amd import utils as U
from tests import strata_cases as SC
from tests.util import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = U.DEFAULT_FP_RATES
IOUS = [0.1, 0.5]
SCORES = [0.0, 0.5, 0.7, 2.0]
MAP_NAMES = ["mixed", "no_detections", "image_without_gt"]


def test_exported_constants_mirror_the_kernel():
    src = open(os.path.join(ROOT, "mslesions3d_amd", "csrc", "evaluate.hip")).read()
    assert U.STRATA_MAX_EDGES == int(re.search(r"constexpr int EV_STRATA_MAX_EDGES = (\d+);", src).group(1)) == 15
    assert U.STRATA_MAX_CUTS == int(re.search(r"constexpr int EV_STRATA_MAX_CUTS = (\d+);", src).group(1)) == 32
    assert U._NEVER == int(re.search(r"constexpr int NEVER = (0x[0-9A-Fa-f]+);", src).group(1), 16)


def _cases():
    return [("map:" + n, SC.map_case(n)) for n in MAP_NAMES] + [(f"seed{s}", SC.random_case(s)) for s in range(8)]


def _voxels(N, seed):
    """A different frame per image: 20^3 .. 40^3 voxels."""
    return (np.random.RandomState(seed).randint(20, 41, N) ** 3).astype(np.float64)


@pytest.mark.parametrize("name,case", _cases(), ids=[n for n, _ in _cases()])
def test_twin_equals_the_brute_force_definition_and_ties_in_with_froc(name, case):
    N = len(case[4])
    w = U.bootstrap_weights(N, 2, seed=N)
    w[1, 0] = 0
    vox = _voxels(N, 1)
    cuts = U.strata_cuts_host(*case, IOUS, SCORES, RATES, w)
    K = sum(int((np.asarray(l) == 1).sum()) for l in case[1])
    assert cuts.shape == (3, 2, len(SCORES) + len(RATES)) and cuts.min() >= 0 and cuts.max() <= K
    assert (cuts[:, :, 0] == K).all() and (cuts[:, :, 3] == 0).all()  # a cut of K (score 0.0) and a cut of 0 (score 2.0)
    ints = U.strata_host(*case, vox, SC.EDGES, IOUS, w, cuts)
    want = SC.brute_force(case, vox, SC.EDGES, IOUS, w, cuts)
    SC.same_ints(ints, want, name)
    # the identities: the strata and the unbinned slot add up to FROC's pooled counts at FROC's own cuts
    froc = U.froc_host(*case, IOUS, RATES, w)
    n_sc = len(SCORES)
    assert np.array_equal(ints["tp"][:, :, n_sc:, :].sum(-1), froc["tp"])
    assert np.array_equal(ints["gw"].sum(-1), froc["gw"]) and np.array_equal(ints["nw"], froc["nw"])
    for t, ov in enumerate(IOUS):
        ranked, _ = SC.matching(case, ov)
        for r in range(3):
            for q in range(cuts.shape[2]):
                k = int(cuts[r, t, q])
                assert ints["fp"][r, t, q].sum() == sum(int(w[r, n]) * (1 - tp) for n, _, tp in ranked[:k]), (name, r, t, q)


def _bin_counts(volumes, voxels, edges):
    """Counts per stratum (last slot: unbinned) of a list of f32 volumes in one frame."""
    s = U.size_stratum(np.asarray(volumes, np.float32), float(voxels), np.asarray(edges, np.float64))
    return np.bincount(np.where(s < 0, len(edges) + 1, s), minlength=len(edges) + 2)


@pytest.mark.parametrize("name,case", _cases(), ids=[n for n, _ in _cases()])
def test_row_zero_at_a_score_cut_bins_the_found_and_not_found_lists_of_calculate_map(name, case):
    """At unit weights and the cut K_c of a score threshold, TP per bin counts ``found_boxes_volumes_per_class`` of
    ``calculate_mAP`` on the detections with score >= that threshold, and Gw_s - TP ``not_found_boxes_volumes_per_class``,
    both scaled by the one frame's voxel count.  (Without any class-1 detection the reference lists every ground-truth
    volume as not found, whatever its label: the boxes that are not class 1 are added for that comparison.)"""
    db, dl, ds, tb, tl = case
    N, voxels = len(tl), 32.0 ** 3
    ints = U.strata_host(*case, voxels, SC.EDGES, IOUS, None, U.strata_cuts_host(*case, IOUS, SCORES, None, None))
    dif = [torch.zeros(len(l), dtype=torch.bool) for l in tl]
    T = lambda xs: [torch.from_numpy(np.asarray(x)) for x in xs]
    other = np.concatenate([SC.volume_f32(np.asarray(b, np.float32).T)[np.asarray(l) != 1] for b, l in zip(tb, tl) if len(l)]
                           or [np.zeros(0, np.float32)])
    for t, ov in enumerate(IOUS):
        for q, sc in enumerate(SCORES):
            keep = [np.asarray(s, np.float32).astype(np.float64) >= sc for s in ds]
            d = U.calculate_mAP(T([np.asarray(b)[k] for b, k in zip(db, keep)]), T([np.asarray(l)[k] for l, k in zip(dl, keep)]),
                                T([np.asarray(s)[k] for s, k in zip(ds, keep)]), T(tb), T(tl), dif, min_overlap=ov,
                                return_detail=True)
            found = _bin_counts(d["found_boxes_volumes_per_class"].numpy(), voxels, SC.EDGES)
            lost = _bin_counts(d["not_found_boxes_volumes_per_class"].numpy(), voxels, SC.EDGES)
            if len(d["sorted_det_scores"]) == 0:
                lost = lost - _bin_counts(other, voxels, SC.EDGES)
            assert np.array_equal(ints["tp"][0, t, q], found), (name, ov, sc)
            assert np.array_equal(ints["gw"][0] - ints["tp"][0, t, q], lost), (name, ov, sc)


@pytest.mark.parametrize("name", MAP_NAMES)
@pytest.mark.parametrize("ov", [0.1, 0.5])
def test_full_ranking_bins_the_reference_volume_lists(name, ov):
    """The same against the lists the reference itself wrote for the fixtures (tests/golden/map.npz), at the cut K."""
    case, g = SC.map_case(name), golden("map")
    voxels = 48.0 ** 3
    ints = U.strata_host(*case, voxels, SC.EDGES, [ov], None, [1 << 40])
    assert np.array_equal(ints["tp"][0, 0, 0], _bin_counts(g[f"{name}__{ov}__found_boxes_volumes_per_class"], voxels, SC.EDGES))
    assert np.array_equal(ints["gw"][0] - ints["tp"][0, 0, 0],
                          _bin_counts(g[f"{name}__{ov}__not_found_boxes_volumes_per_class"], voxels, SC.EDGES))


def test_edge_values_zero_volume_and_nan_boxes():
    case = SC.edge_case()
    w = np.array([[1, 1, 1], [2, 0, 3]], np.int32)
    cuts = np.array([0, 1, 2, 3, 4, 5], np.int64)
    ints = U.strata_host(*case, 1000.0, SC.EDGES, IOUS, w, cuts)
    SC.same_ints(ints, SC.brute_force(case, 1000.0, SC.EDGES, IOUS, w, np.broadcast_to(cuts, (2, 2, 6))), "edge")
    # bins: [0, 27) | [27, 125) | [125, 1000) | [1000, inf) | unbinned
    assert ints["gw"].tolist() == [[1, 1, 1, 1, 1], [2, 0, 2, 2, 3]]  # flat | 64 voxels | 125 on the edge | 1000 | NaN
    assert ints["det_unbinned"].tolist() == [1, 3] and ints["nw"].tolist() == [3, 5]
    for t in range(2):
        assert ints["tp"][0, t].tolist() == [[0, 0, 0, 0, 0], [0, 0, 1, 0, 0], [0, 0, 1, 0, 0], [0, 0, 1, 0, 0],
                                             [0, 0, 1, 1, 0], [0, 0, 1, 1, 0]]
        assert ints["fp"][0, t].tolist() == [[0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [1, 0, 0, 0, 0], [1, 0, 0, 0, 1],
                                             [1, 0, 0, 0, 1], [2, 0, 0, 0, 1]]
        assert ints["tp"][1, t, 5].tolist() == [0, 0, 2, 2, 0] and ints["fp"][1, t, 5].tolist() == [4, 0, 0, 0, 3]
    # one ulp below the edge falls into the bin below it
    below = np.nextafter(np.float32(0.125), np.float32(0))
    assert U.size_stratum([np.float32(0.125), below, np.float32(np.nan), np.float32(np.inf), np.float32(-1)], 1000.0,
                          np.asarray(SC.EDGES)).tolist() == [2, 1, -1, 3, 0]


def test_one_edge_and_fifteen_edges():
    case = SC.random_case(3)
    N = len(case[4])
    w = U.bootstrap_weights(N, 1, 0)
    cuts = U.strata_cuts_host(*case, [0.5], [0.25], None, w)
    for edges in ([100.0], [float(2 ** j) for j in range(15)]):
        vox = _voxels(N, 2)
        ints = U.strata_host(*case, vox, edges, [0.5], w, cuts)
        assert ints["tp"].shape == (2, 1, 1, len(edges) + 2)
        SC.same_ints(ints, SC.brute_force(case, vox, edges, [0.5], w, cuts), str(len(edges)))
    assert (U.strata_host(*case, vox, [float(2 ** j) for j in range(15)], [0.5], w, cuts)["gw"][0] > 0).sum() > 3


def test_bad_arguments_are_rejected():
    case = SC.random_case(1)
    N = len(case[4])
    ok = dict(voxels=1000.0, size_edges=[1.0, 2.0], min_overlaps=[0.5], weights=None, cuts=[0])
    call = lambda **kw: U.strata_host(*case, **{**ok, **kw})
    call()
    for bad in ([], [2.0, 1.0], [1.0, 1.0], [np.nan], [np.inf], list(range(16))):
        with pytest.raises(ValueError):
            call(size_edges=bad)
    for bad in (0.0, -1.0, np.nan, np.ones(N + 1), np.inf):
        with pytest.raises(ValueError):
            call(voxels=bad)
    for bad in ([], list(range(33)), [0.5], np.zeros((1, 1), np.int64)):
        with pytest.raises(ValueError):
            call(cuts=bad)
    db, dl, ds, tb, tl = case
    ds = [np.where(np.arange(len(s)) == 0, np.nan, s).astype(np.float32) for s in ds]
    with pytest.raises(ValueError, match="NaN"):
        U.strata_host(db, dl, ds, tb, tl, **ok)


def test_summary_ratios_intervals_and_dropped_rows():
    S1 = 4  # two edges: three bins and the unbinned slot
    tp = np.zeros((4, 1, 2, S1), np.int64)
    fp = np.zeros_like(tp)
    gw = np.array([[4, 0, 2, 1], [8, 0, 0, 0], [2, 0, 4, 0], [4, 0, 2, 3]], np.int64)
    tp[:, 0, 1] = [[2, 0, 1, 1], [2, 0, 0, 0], [2, 0, 1, 0], [1, 0, 2, 0]]
    fp[:, 0, 1] = [[3, 1, 0, 2], [6, 0, 0, 0], [0, 2, 0, 0], [3, 1, 1, 0]]
    ints = {"tp": tp, "fp": fp, "gw": gw, "det_unbinned": np.array([5, 0, 0, 0]), "nw": np.array([4, 4, 4, 4]),
            "cuts": np.array([0, 9])[None, None].repeat(4, 0)}
    s = U.strata_summary(ints, [10.0, 20.0], [0.5], [{"min_score": 0.9}, {"fp_rate": 0.25}])[0.5]
    assert list(s) == ["edges", "n_lesions", "cuts", "dropped", "unbinned", "n_cases", "n_boot"]
    assert s["edges"] == [10.0, 20.0] and s["n_lesions"] == [4, 0, 2] and s["n_cases"] == 4 and s["n_boot"] == 3
    assert s["dropped"] == [0, 3, 1] and s["unbinned"] == {"n_lesions": 1, "detections": 5}
    a, b = s["cuts"]
    assert a["min_score"] == 0.9 and a["k"] == 0 and a["sensitivity"][0] == 0.0 and np.isnan(a["sensitivity"][1])
    assert b["fp_rate"] == 0.25 and b["k"] == 9
    assert b["sensitivity"][0] == 0.5 and np.isnan(b["sensitivity"][1]) and b["sensitivity"][2] == 0.5
    assert b["fp_per_case"] == [0.75, 0.25, 0.0] and (b["unbinned_tp"], b["unbinned_fp"]) == (1, 2)
    lo, hi = np.percentile([2 / 8, 2 / 2, 1 / 4], [2.5, 97.5])
    assert (b["ci_low"][0], b["ci_high"][0]) == (float(lo), float(hi))
    assert b["ci_low"][1] is None and b["ci_high"][1] is None  # no bootstrap row has a lesion in that bin
    lo, hi = np.percentile([1 / 4, 2 / 2], [2.5, 97.5])  # the row with Gw_s = 0 is dropped
    assert (b["ci_low"][2], b["ci_high"][2]) == (float(lo), float(hi))
    lo, hi = np.percentile([6 / 4, 0.0, 3 / 4], [2.5, 97.5])
    assert (b["fp_ci_low"][0], b["fp_ci_high"][0]) == (float(lo), float(hi))
    # without bootstrap rows there is no interval
    one = {k: (v[:1] if isinstance(v, np.ndarray) else v) for k, v in ints.items()}
    c = U.strata_summary(one, [10.0, 20.0], [0.5], [{"min_score": 0.9}, {"fp_rate": 0.25}])[0.5]
    assert c["n_boot"] == 0 and c["dropped"] == [0, 0, 0] and c["cuts"][1]["ci_low"] == [None] * 3
    assert c["cuts"][1]["fp_ci_high"] == [None] * 3
    # JSON: NaN becomes null, every key survives
    text = json.dumps(EV.strata_json(s), indent=4)
    back = json.loads(text)
    assert "NaN" not in text and back["cuts"][1]["sensitivity"] == [0.5, None, 0.5] and list(back) == list(s)


def test_size_bins_flag_and_file_name():
    assert EV.size_bin_list("27,125,1000") == [27.0, 125.0, 1000.0] and EV.size_bin_list("8") == [8.0]
    a = EV.build_parser().parse_args(["--size_bins", "27,125,1000"])
    assert EV.eval_options(a).size_bins == [27.0, 125.0, 1000.0]
    assert EV.eval_options(EV.build_parser().parse_args([])).size_bins is None
    assert "size_bins" not in vars(EV.build_parser().parse_args([]))
    for bad in ("", "a", "2,1", "1,1", "nan", "inf", ",".join(str(v) for v in range(16))):
        with pytest.raises(SystemExit):
            EV.build_parser().parse_args(["--size_bins", bad])
    assert EV.strata_file_name(0.5) == "strata_(min_IoU=0.5).json"
    assert U.strata_cut_labels([0.5], [(1, 8)]) == [{"min_score": 0.5}, {"fp_rate": 0.125}]
    assert U.strata_cut_labels([0.5, 0.7], None) == [{"min_score": 0.5}, {"min_score": 0.7}]


def test_batch_voxels():
    assert EV.batch_voxels({"img": torch.zeros(2, 1, 4, 5, 6), "subject": ["a", "b"]}) == [120, 120]
    assert EV.batch_voxels({"voxels": [7, 8], "subject": ["a", "b"]}) == [7, 8]
