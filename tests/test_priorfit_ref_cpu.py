"""The prior fit report without a GPU: the reference (tests/priorfit_ref.py) on hand-made cases against values derived by
hand, the numpy restatement of the priors against the golden fixtures, ``utils.prior_fit_summary`` on a fixed fit against
written-out counts, and the argument errors of ``python -m mslesions3d_amd.insight``."""
import os

import numpy as np
import pytest

from tests import priorfit_cases as C
from tests.priorfit_ref import reference

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "priors.npz")


def _run(name):
    images, thr = C.HAND_CASES[name]
    pri, off = C.prior_set("a")
    return reference(images, pri, thr, off), pri


def test_numpy_priors_match_the_golden_fixture():
    z = np.load(GOLDEN)
    dims = C.fmap_dims((64, 64, 64))
    assert [list(dims[f]) for f in range(8)] == z["fmap_dims_64"].tolist()
    assert [list(C.fmap_dims((48, 64, 64))[f]) for f in range(8)] == z["fmap_dims_48x64x64"].tolist()
    pri, off = C.priors_numpy((64, 64, 64), (3, 5, 7), dict(zip((3, 5, 7), z["scales_64"])))
    assert np.array_equal(pri.view(np.uint32), z["full_64"].view(np.uint32))
    assert np.allclose(list(C.default_scales((64, 64, 64), (3, 5, 7)).values()), z["scales_64"], rtol=0, atol=0)
    pri, off = C.priors_numpy((48, 64, 64), (3, 5, 7), dict(zip((3, 5, 7), z["scales_48x64x64"])))
    assert pri.shape[0] == int(z["n_48x64x64"]) == off[-1]
    assert np.array_equal(pri[:4], z["head_48x64x64"]) and np.array_equal(pri[-4:], z["tail_48x64x64"])


def test_prior_sets_have_the_sizes_the_case_list_states():
    for name, s in C.PRIOR_SETS.items():
        pri, off = C.prior_set(name)
        assert pri.shape == (s["P"], 6) and off[0] == 0 and off[-1] == s["P"] and off.size == len(s["layers"]) + 1
    pri, off = C.prior_set("a")
    assert off.tolist() == [0, 128, 144, 146]
    # the rows the hand-made cases name
    assert pri[54].tolist() == [0.625, 0.375, 0.875, 0.1875, 0.1875, 0.1875]
    assert pri[55].tolist() == [0.625, 0.375, 0.875, 0.375, 0.375, 0.375]
    assert pri[50].tolist()[:3] == [0.625, 0.375, 0.375] and pri[52].tolist()[:3] == [0.625, 0.375, 0.625]


def test_object_equal_to_a_prior():
    """The box IS prior 54: IoU v / (v + v - v) = 1.  Prior 55 (same centre, size 0.375) contains it: IoU =
    0.1875^3 / 0.375^3 = 1/8 exactly.  Every other prior is below 0.1 (the best: the size-0.3125 prior of feature 5 at
    (0.75, 0.25, 0.75), inter 0.125^3 = 1/512, union 27/4096 + 125/4096 - 8/4096 -> 8/144 = 0.056).  So feature 3 holds
    prior 54 (forced, overlap 1) at every threshold and prior 55 up to 0.125 inclusive."""
    r, _ = _run("equal_to_prior")
    assert r["best_iou"].tolist() == [1.0] and r["best_prior"].tolist() == [54] and r["held"].tolist() == [1]
    assert r["pos"][0].tolist() == [[2, 0, 0], [2, 0, 0], [1, 0, 0], [1, 0, 0]]  # thresholds 0.1, 0.125, 0.2, 1.0


def test_tie_between_two_priors_goes_to_the_first():
    """Centre half way between rows 50 and 52 (size 0.1875, 0.25 apart): the overlap along z is 0.0625 for both, inter =
    0.1875^2 * 0.0625 = 9/4096, union (27 + 27 - 9)/4096 -> IoU 9/45 = 0.2 for both, bit for bit; row 50 wins.  Their
    size-0.375 partners 51 and 53 overlap 0.15625 along z: inter 22.5/4096, union (27 + 216 - 22.5)/4096 -> 0.10204.  The
    next best is the size-0.4375 prior of feature 7, which contains the box: 27/4096 / 0.4375^3 = 0.0787."""
    r, _ = _run("tie_first_index")
    assert r["best_prior"].tolist() == [50] and r["held"].tolist() == [1]
    assert r["best_iou"].view(np.uint32).tolist() == [int(np.float32(0.2).view(np.uint32))]
    # thresholds 0.1: rows 50 (forced), 52, 51, 53;  0.15 and 0.2: 50 and 52 (0.2 >= float32(0.2));  0.25: the forced one
    assert r["pos"][0].tolist() == [[4, 0, 0], [2, 0, 0], [2, 0, 0], [1, 0, 0]]


def test_identical_pair_orphans_the_first():
    """Both boxes are prior 54.  Every prior's first maximum is box 0; the force-match gives prior 54 to the LAST claimant,
    box 1.  Box 0 keeps prior 55 (IoU 1/8) alone: nothing above 0.125, although its best IoU is 1."""
    r, _ = _run("identical_pair")
    assert r["best_iou"].tolist() == [1.0, 1.0] and r["best_prior"].tolist() == [54, 54] and r["held"].tolist() == [0, 1]
    assert r["pos"][0].tolist() == [[1, 0, 0], [0, 0, 0], [0, 0, 0]]  # thresholds 0.1, 0.2, 1.0
    assert r["pos"][1].tolist() == [[1, 0, 0], [1, 0, 0], [1, 0, 0]]


def test_zero_volume_boxes_all_claim_prior_zero():
    """IoU = 0 / (0 + v - 0) = 0 everywhere: every box's first maximum is prior 0 and every prior's first maximum is box 0.
    Only the last box holds prior 0 (overlap 1).  At threshold 0 every prior is a positive: box 0 owns all but prior 0."""
    r, _ = _run("zero_volume")
    assert r["best_iou"].tolist() == [0.0] * 3 and r["best_prior"].tolist() == [0] * 3 and r["held"].tolist() == [0, 0, 1]
    assert r["pos"][0].tolist() == [[127, 16, 2], [0, 0, 0], [0, 0, 0]]  # thresholds 0, 0.5, 1
    assert r["pos"][1].tolist() == [[0, 0, 0]] * 3
    assert r["pos"][2].tolist() == [[1, 0, 0]] * 3


def test_forced_prior_is_taken_from_its_first_max_owner():
    """Box 0 is prior 54 (IoU 1).  Box 1, a 0.0625 cube at the same centre, has its best IoU with prior 54 too: 1/27
    (prior 55: 1/216; the feature-5 prior that contains it: 1/125).  The force-match hands prior 54 to box 1, the last
    claimant, with overlap 1.  Box 0 is left with prior 55 (1/8): orphaned at 0.2 with a best IoU of 1."""
    r, _ = _run("forced_prior_taken")
    assert r["best_prior"].tolist() == [54, 54] and r["held"].tolist() == [0, 1]
    assert r["best_iou"][0] == 1.0 and abs(float(r["best_iou"][1]) - 1 / 27) < 1e-7
    assert r["pos"][0].tolist() == [[1, 0, 0], [0, 0, 0]]  # thresholds 0.1, 0.2
    assert r["pos"][1].tolist() == [[1, 0, 0], [1, 0, 0]]


def test_summary_on_a_fixed_fit():
    """Two images of 64 voxels (4^3), four boxes: volumes 1/64, 8/64 -> sizes 1, 8 voxels; bins at 2 and 10."""
    from mslesions3d_amd.utils import prior_fit_summary
    u = 0.25
    boxes = [np.array([[0, 0, 0, u, u, u], [0, 0, 0, 2 * u, 2 * u, 2 * u], [u, u, u, 2 * u, 2 * u, 2 * u]], np.float32),
             np.zeros((0, 6), np.float32),
             np.array([[0, 0, 0, 2 * u, 2 * u, 4 * u]], np.float32)]  # 16 voxels
    fit = {"best_iou": np.array([0.05, 0.6, 0.15, 0.3], np.float32), "best_prior": np.array([3, 3, 7, 9]),
           "best_scale": np.array([0, 0, 0, 1]), "held": np.array([0, 1, 1, 1]), "image": np.array([0, 0, 0, 2]),
           # (G, thresholds 0.1 / 0.2, two scale ranges)
           "pos": np.array([[[0, 0], [0, 0]], [[3, 1], [2, 0]], [[1, 0], [1, 0]], [[2, 5], [0, 1]]])}
    s = prior_fit_summary(fit, boxes, 64, [2, 10], [0.1, 0.2], shapes=(4, 4, 4), scale_names=[3, 5])
    assert s["n_images"] == 3 and s["n_lesions"] == 4 and s["scales"] == ["3", "5"] and s["edges"] == [2.0, 10.0]
    t0, t1 = s["thresholds"]
    assert [t0["threshold"], t1["threshold"]] == [float(np.float32(0.1)), float(np.float32(0.2))]
    assert t0["positives_per_image"] == 12 / 3 and t1["positives_per_image"] == 4 / 3
    names = [r["stratum"] for r in t0["strata"]]
    assert names == ["all", "[0, 2)", "[2, 10)", "[10, inf)"]
    get = lambda t, k: [r[k] for r in t["strata"]]
    assert get(t0, "lesions") == [4, 2, 1, 1] and sum(get(t0, "lesions")[1:]) == 4
    assert get(t0, "matchable") == [3, 1, 1, 1]     # best_iou >= 0.1: boxes 1, 2, 3
    assert get(t1, "matchable") == [2, 0, 1, 1]     # >= 0.2: boxes 1, 3
    assert get(t0, "orphaned") == [1, 1, 0, 0]      # box 0
    assert get(t1, "orphaned") == [1, 1, 0, 0]
    assert get(t0, "forced_only") == [0, 0, 0, 0]   # box 0 is below the threshold but does not hold its prior
    assert get(t1, "forced_only") == [1, 1, 0, 0]   # box 2: 0.15 < 0.2, held, one positive
    assert t0["strata"][0]["positives"] == {"mean": 3.0, "median": 2.5, "max": 7}
    assert t0["strata"][0]["positives_per_scale"] == {"3": 6, "5": 6}
    assert t1["strata"][3]["positives_per_scale"] == {"3": 0, "5": 1}
    assert t0["strata"][0]["best_iou"]["min"] == float(np.float32(0.05))
    assert s["extent"]["unit"] == "voxels"
    assert [a["min"] for a in s["extent"]["axes"]] == [1.0, 1.0, 1.0] and [a["max"] for a in s["extent"]["axes"]] == [2.0, 2.0, 4.0]
    # no bins: the "all" row alone; no shapes: fractions
    s = prior_fit_summary(fit, boxes, 64, (), [0.1, 0.2])
    assert [r["stratum"] for r in s["thresholds"][0]["strata"]] == ["all"] and s["extent"]["unit"] == "fraction"


def test_prior_fit_refuses_bad_boxes_before_any_gpu_call(monkeypatch):
    from mslesions3d_amd import _lib, utils

    def no_gpu(*a, **k):
        raise AssertionError("a GPU call was made")
    monkeypatch.setattr(_lib, "call", no_gpu)
    good = np.array([[0.1, 0.1, 0.1, 0.2, 0.2, 0.2]], np.float32)
    for bad in (np.array([[0.1, 0.1, 0.1, np.nan, 0.2, 0.2]], np.float32), np.array([[0.1, 0.1, 0.1, np.inf, 0.2, 0.2]], np.float32),
                np.array([[0.3, 0.1, 0.1, 0.2, 0.2, 0.2]], np.float32)):
        with pytest.raises(ValueError):
            utils.prior_fit([good, bad], None, [0.5], {3: (0, 10)})
    with pytest.raises(ValueError):
        utils.prior_fit_ranges({3: (0, 10), 5: (12, 20)}, 20)
    with pytest.raises(ValueError):
        utils.prior_fit_ranges({f: (f, f + 1) for f in range(9)}, 9)
    assert utils.prior_fit_ranges({3: (0, 128), 5: (128, 144), 7: (144, 146)}, 146).tolist() == [0, 128, 144, 146]


@pytest.mark.parametrize("argv", [
    ["--patch_size", "32", "32", "32"],                      # windows of clinical cases: needs -dm lesions
    ["-ii", "FLAIR", "acq-mag_T2star"],                      # the synthetic cases have one channel
    ["-th", "0.3", "0.1"], ["-th", "0.1", "0.2", "0.3"], ["-th", "1.5"],
    ["--scale_factors", "1,0"], ["--scale_factors", "1,1"],
    ["-pl", "5 3"], ["-pl", "3 5", "-sc", '{"3": 0.1}'],
])
def test_insight_argument_errors_come_before_any_gpu_call(argv, monkeypatch):
    import torch
    from mslesions3d_amd import insight

    def no_gpu(*a, **k):
        raise AssertionError("the device was asked for")
    monkeypatch.setattr(torch.cuda, "is_available", no_gpu)
    with pytest.raises(ValueError):
        insight.main(argv + ["-d", "/nonexistent", "-o", "/nonexistent/out"])


def test_insight_parser_reuses_the_flag_parsers():
    from mslesions3d_amd import insight
    a = insight.build_parser().parse_args(["--size_bins", "27,125", "--scale_factors", "0.5,1,2", "-th", "0.1", "0.2"])
    assert a.size_bins == [27.0, 125.0] and a.scale_factors == [0.5, 1.0, 2.0] and a.threshold == [0.1, 0.2]
    with pytest.raises(SystemExit):
        insight.build_parser().parse_args(["--size_bins", "125,27"])
