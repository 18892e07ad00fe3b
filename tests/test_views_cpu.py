"""Multi-view prediction, host side: ``datasets.view_plan`` / ``gather_views`` and
``utils.merge_views``.  No GPU.  The crafted merge cases use coordinates that are multiples of 1/64 with tile = case = 64^3,
so every mapping is exact in f32; ``merge_cases()`` is shared with tests/test_gpu_views.py."""
import numpy as np
import pytest

from mslesions3d_amd.datasets import fit_shift, gather_views, resize_with_pad_or_crop, view_plan
from mslesions3d_amd.utils import merge_views

F32 = np.float32
T64 = (64, 64, 64)
IDENT = [[0, 0, 0, 0, 0, 0]]


# ---- view_plan --------------------------------------------------------------------------------------------------------
def test_single_tile_is_the_fit():
    plan = view_plan((50, 64, 61), (64, 64, 64))
    assert plan.dtype == np.int32 and plan.tolist() == [[fit_shift(50, 64), 0, fit_shift(61, 64), 0, 0, 0]]
    assert fit_shift(50, 64) < 0


def _axis_origins(plan, k):
    return sorted(set(plan[:, k].tolist()))


@pytest.mark.parametrize("case", [(70, 64, 100), (200, 129, 64)])
def test_tiles_cover_the_case(case):
    t, m = 64, 8
    plan = view_plan(case, (t,) * 3, (m,) * 3)
    count = 1
    for k, n in enumerate(case):
        o = _axis_origins(plan, k)
        count *= len(o)
        if n <= t:
            assert o == [fit_shift(n, t)]
            continue
        assert o[0] == 0 and o[-1] == n - t
        assert all(a + t - b >= 2 * m for a, b in zip(o, o[1:]))  # neighbours overlap by at least 2m
        core = np.zeros(n, dtype=bool)  # every voxel lies in some view's core (a tile at the border owns out to it)
        for a in o:
            core[(a + m if a > 0 else 0):(a + t - m if a + t < n else n)] = True
        assert core.all()
    assert plan.shape == (count, 6) and not plan[:, 3:].any()
    # the product of the three axes, axis 0 slowest
    expect = [[a, b, c] for a in _axis_origins(plan, 0) for b in _axis_origins(plan, 1) for c in _axis_origins(plan, 2)]
    assert plan[:, :3].tolist() == expect


def test_flip_ordering():
    plan = view_plan((70, 64, 64), T64, flip_axes=(2, 0))
    assert plan.shape == (8, 6)
    flips = [[0, 0, 0], [0, 0, 1], [1, 0, 0], [1, 0, 1]]  # subsets of (2, 0), the unflipped one first
    assert plan[:4, 3:].tolist() == flips and plan[4:, 3:].tolist() == flips  # tile-major, flip-minor
    assert plan[:4, 0].tolist() == [0] * 4 and plan[4:, 0].tolist() == [6] * 4


def test_plan_limits():
    assert view_plan((200, 200, 64), T64, flip_axes=(0, 1)).shape[0] == 64  # 4 x 4 x 1 tiles x 4 flips: at capacity
    with pytest.raises(ValueError, match="flip_views"):
        view_plan((200, 200, 64), T64, flip_axes=(0, 1, 2))
    with pytest.raises(ValueError, match="spatial_size"):
        view_plan((200, 200, 250), T64)
    with pytest.raises(ValueError, match="tile_margin"):
        view_plan((70, 64, 64), (16, 64, 64), margin=(8, 8, 8))
    assert view_plan((10, 64, 64), (16, 64, 64), margin=(8, 8, 8)).shape[0] == 1  # no tiling on that axis: no core needed


# ---- gather_views -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 2])
def test_fit_view_is_resize_with_pad_or_crop(C):
    case = np.random.RandomState(C).randn(C, 5, 70, 9).astype(F32)
    tile = (8, 64, 6)
    fit = [[fit_shift(n, t) for n, t in zip(case.shape[1:], tile)] + [0, 0, 0]]  # pad, crop, crop
    out = gather_views(case, fit, tile)
    assert out.shape == (1, C) + tile and out.dtype == F32
    np.testing.assert_array_equal(out[0], resize_with_pad_or_crop(case, tile))


def test_flipped_view_is_np_flip():
    case = np.random.RandomState(3).randn(2, 20, 18, 70).astype(F32)
    tile = (16, 16, 32)
    for mask in range(8):
        f = [(mask >> k) & 1 for k in range(3)]
        plain, flipped = gather_views(case, [[-3, 1, 38, 0, 0, 0], [-3, 1, 38] + f], tile)
        np.testing.assert_array_equal(flipped, np.flip(plain, axis=tuple(1 + k for k in range(3) if f[k])))


# ---- merge_views ------------------------------------------------------------------------------------------------------
def det(rows, top_k):
    """One view's detections [(box6 in 1/64 units, score, label)] in msl_detect_objects' layout."""
    b, s, l = np.zeros((top_k, 6), F32), np.zeros(top_k, F32), np.zeros(top_k, np.int64)
    for j, (box, score, label) in enumerate(rows):
        b[j], s[j], l[j] = np.asarray(box, F32) / F32(64), score, label
    return b, s, l, len(rows)


def pack(per_view, top_k=4):
    parts = [det(rows, top_k) for rows in per_view]
    return tuple(np.stack([p[i] for p in parts]) for i in range(3)) + (np.asarray([p[3] for p in parts], np.int32),)


A, B, C_ = [8, 8, 8, 16, 16, 16], [40, 40, 40, 48, 52, 56], [9, 8, 8, 17, 16, 16]


def mirror(box, axes):
    box = list(box)
    for k in axes:
        box[k], box[3 + k] = 64 - box[3 + k], 64 - box[k]
    return box


def merge_cases():
    """name -> kwargs of merge_views (without mode)."""
    one = dict(views=IDENT, tile=T64, case_shape=T64, margin=(8, 8, 8), max_overlap=0.5)
    cases = {}
    cases["identity"] = dict(one, det=pack([[(A, 0.5, 1), (B, 0.75, 1)]]))
    flip = dict(one, views=[[0, 0, 0, 0, 0, 0], [0, 0, 0, 1, 0, 1]])
    cases["mirror"] = dict(flip, det=pack([[(B, 0.75, 1)], [(mirror(B, (0, 2)), 0.5, 1)]]))
    cases["twice"] = dict(flip, views=flip["views"] * 2,
                          det=pack([[(B, 0.75, 1), (A, 0.5, 1)], [(mirror(B, (0, 2)), 0.5, 1)]] * 2))
    cases["placeholder"] = dict(one, det=pack([[(A, 0.5, 0), (B, 0.25, 1)]]))
    cases["empty"] = dict(flip, det=pack([[], []]))
    cases["ties"] = dict(flip, det=pack([[(A, 0.5, 1), (B, 0.5, 1)], [(mirror(C_, (0, 2)), 0.5, 1)]]))
    return cases


def run(case, mode="nms", **kw):
    b, s, l, c = case["det"]
    args = {k: v for k, v in case.items() if k != "det"}
    args.update(kw)
    return merge_views(b, s, l, c, mode=mode, **args)


def test_identity_view_returns_its_detections_in_score_order():
    boxes, labels, scores, support = run(merge_cases()["identity"])
    np.testing.assert_array_equal(boxes, np.asarray([B, A], F32) / 64)
    assert scores.tolist() == [0.75, 0.5] and labels.tolist() == [1, 1] and support.tolist() == [1, 1]
    assert boxes.dtype == F32 and scores.dtype == F32 and labels.dtype == np.int64 and support.dtype == np.int32


@pytest.mark.parametrize("mode", ["nms", "fuse"])
def test_mirror_image_maps_to_the_same_box(mode):
    boxes, labels, scores, support = run(merge_cases()["mirror"], mode)
    np.testing.assert_array_equal(boxes, np.asarray([B], F32) / 64)
    assert support.tolist() == [2] and scores.tolist() == [0.75 if mode == "nms" else 0.625]


def test_every_view_twice_doubles_support_only():
    once, twice = merge_cases()["mirror"], merge_cases()["twice"]
    once = dict(once, det=pack([[(B, 0.75, 1), (A, 0.5, 1)], [(mirror(B, (0, 2)), 0.5, 1)]]))
    b1, l1, s1, u1 = run(once, "fuse")
    b2, l2, s2, u2 = run(twice, "fuse")
    np.testing.assert_array_equal(b1, b2)
    np.testing.assert_array_equal(s1, s2)
    assert u2.tolist() == (2 * u1).tolist() == [4, 2]
    assert s1.tolist() == [0.625, 0.25]  # A: one of two covering views saw it


def test_ownership_takes_an_overlap_box_from_one_tile():
    case, margin = (64, 64, 100), (8, 8, 8)
    views = view_plan(case, T64, margin)  # W origins 0 and 36: overlap [36, 64), cores end / start at 56 / 44
    assert views[:, 2].tolist() == [0, 36]
    for lo, owner in ((30, 0), (36, 0), (52, 1), (54, 1)):  # centres lo + 4: below 44 tile 0 alone, from 56 tile 1 alone
        box = [8, 8, lo, 16, 16, lo + 8]
        second = [8, 8, lo - 36, 16, 16, lo - 28]
        d = pack([[(box, 0.5, 1)], [(second, 0.75, 1)]])
        boxes, labels, scores, support = merge_views(*d, views, T64, case, margin, 0.5)
        assert scores.tolist() == [0.75 if owner else 0.5] and support.tolist() == [1]
        np.testing.assert_array_equal(boxes[0], np.asarray(box, F32) / np.asarray([64, 64, 100] * 2, F32))
    # centre 48 lies in [44, 56), both cores: both copies are candidates and NMS keeps the better one
    d = pack([[([8, 8, 44, 16, 16, 52], 0.5, 1)], [([8, 8, 8, 16, 16, 16], 0.75, 1)]])
    boxes, labels, scores, support = merge_views(*d, views, T64, case, margin, 0.5)
    assert scores.tolist() == [0.75] and support.tolist() == [2]


def test_core_intervals_do_not_double_count():
    """Margin m: the cores of neighbouring tiles are [.., o_a + T - m) and [o_b + m, ..); a centre in the margin of one
    tile belongs to the other alone."""
    case, margin = (64, 64, 100), (8, 8, 8)
    views = view_plan(case, T64, margin)
    d = pack([[([8, 8, 54, 16, 16, 62], 0.5, 1)], []])  # centre 58 >= 56: tile 0 does not own it
    assert merge_views(*d, views, T64, case, margin, 0.5)[2].shape == (0,)
    d = pack([[], [([8, 8, 0, 16, 16, 8], 0.5, 1)]])  # view 1 voxel 4 = case 40 < 44: tile 1 does not own it
    assert merge_views(*d, views, T64, case, margin, 0.5)[2].shape == (0,)


def test_placeholders_never_become_candidates():
    boxes, labels, scores, support = run(merge_cases()["placeholder"])
    assert labels.tolist() == [1] and scores.tolist() == [0.25]


@pytest.mark.parametrize("mode", ["nms", "fuse"])
def test_all_views_empty_gives_count_zero(mode):
    boxes, labels, scores, support = run(merge_cases()["empty"], mode)
    assert boxes.shape == (0, 6) and labels.shape == scores.shape == support.shape == (0,)


def test_ties_resolve_by_view_then_slot():
    boxes, labels, scores, support = run(merge_cases()["ties"])
    # A (view 0, slot 0) outranks its equal-score overlap C (view 1); B (view 0, slot 1) follows A
    np.testing.assert_array_equal(boxes, np.asarray([A, B], F32) / 64)
    assert support.tolist() == [2, 1]
    boxes, _, scores, _ = run(merge_cases()["ties"], out_top_k=1)
    np.testing.assert_array_equal(boxes, np.asarray([A], F32) / 64)


BASES = np.asarray([[0.4, 0.4, 0.4, 0.6, 0.6, 0.6], [0.2, 0.45, 0.45, 0.3, 0.55, 0.55]], F32)


def random_detections(rs, V, top_k, n_fg=1, empty=()):
    """Random detections of V views in the detect layout: boxes of 4 .. 20 % of the view, a third of them jittered copies
    of two fixed boxes (so that clusters form within and across views), scores on a coarse grid (so that ties occur),
    counts below top_k, 0 for the views in ``empty``."""
    lo = rs.uniform(0, 0.8, (V, top_k, 3))
    boxes = np.concatenate([lo, lo + rs.uniform(0.04, 0.2, (V, top_k, 3))], -1).astype(F32)
    copies = BASES[rs.randint(0, 2, (V, top_k))] + rs.uniform(-0.01, 0.01, (V, top_k, 6)).astype(F32)
    boxes = np.where(rs.rand(V, top_k, 1) < 1 / 3, copies, boxes).astype(F32)
    scores = (rs.randint(1, 64, (V, top_k)) / 64).astype(F32)
    labels = rs.randint(1, n_fg + 1, (V, top_k)).astype(np.int64)
    counts = rs.randint(max(1, top_k // 2), top_k + 1, V).astype(np.int32)
    counts[list(empty)] = 0
    return boxes, scores, labels, counts


def _iou(a, b):
    e = np.maximum(np.minimum(a[3:], b[3:]) - np.maximum(a[:3], b[:3]), F32(0))
    inter = e[0] * e[1] * e[2]
    va, vb = np.prod(a[3:] - a[:3], dtype=F32), np.prod(b[3:] - b[:3], dtype=F32)
    return inter / (va + vb - inter)


def test_matches_brute_force_nms():
    rs = np.random.RandomState(7)
    V, top_k = 4, 50
    boxes, scores, labels, counts = random_detections(rs, V, top_k)
    counts[:] = top_k  # 200 boxes
    views = [[0, 0, 0, 0, 0, 0]] * V  # four identity views: the map is exact, every box is owned
    got = merge_views(boxes, scores, labels, counts, views, T64, T64, (8, 8, 8), 0.3)
    flat_b, flat_s = boxes.reshape(-1, 6), scores.reshape(-1)
    order = sorted(range(V * top_k), key=lambda i: (-flat_s[i], i))
    kept = []
    for i in order:
        if all(not _iou(flat_b[k], flat_b[i]) > F32(0.3) for k in kept):
            kept.append(i)
    assert 10 < len(kept) < 200
    np.testing.assert_array_equal(got[0], flat_b[kept])
    np.testing.assert_array_equal(got[2], flat_s[kept])
    sup = [len({k // top_k} | {i // top_k for i in order if i not in kept and
                               next(j for j in kept if _iou(flat_b[j], flat_b[i]) > F32(0.3)) == k}) for k in kept]
    assert got[3].tolist() == sup


# ---- predict.py flags ---------------------------------------------------------------------------------------------------
def test_view_flags_select_the_route_and_leave_the_default_namespace_alone():
    from mslesions3d_amd.predict import build_parser, merge_margin, multi_view, view_options
    plain = build_parser().parse_args([])
    assert not multi_view(plain) and not {"views", "tile_margin", "flip_views", "merge", "view_batch"} & set(vars(plain))
    o = view_options(plain)
    assert (o.views, tuple(o.tile_margin), tuple(o.flip_views), o.merge, o.view_batch) == ("fit", (8, 8, 8), (), "nms", 2)
    assert not multi_view(build_parser().parse_args(["--views", "fit", "--flip_views"]))
    tiles = build_parser().parse_args(["--views", "tiles", "--tile_margin", "4", "5", "6", "--merge", "fuse", "--view_batch", "3"])
    o = view_options(tiles)
    assert multi_view(tiles) and (o.tile_margin, o.merge, o.view_batch) == ([4, 5, 6], "fuse", 3) and merge_margin(tiles) == (4, 5, 6)
    flips = build_parser().parse_args(["--flip_views", "2", "0"])
    assert multi_view(flips) and view_options(flips).flip_views == [2, 0] and merge_margin(flips) == (0, 0, 0)
