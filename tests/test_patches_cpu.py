"""Patch training on the host: datasets.window, lesion_centres, patch_origin, the patch mode of
_LesionCases and the validation tiles of LesionsDataModule.  Every comparison is bit for bit.  CPU only."""
import numpy as np
import pytest
import torch

from mslesions3d_amd import datasets as DS
from mslesions3d_amd.devicedata import sample_params
from tests import lesion_tree

SHAPES = [(40, 44, 50), (52, 48, 46), (44, 70, 52), (60, 50, 72), (48, 64, 64), (42, 42, 42), (50, 45, 58),
          (46, 66, 49), (41, 51, 61), (55, 47, 43)]
PATCH = (32, 32, 32)
P1 = {"prob": 1.0}
AUGS = [("flip", {"spatial_axis": (0, 2), "prob": 1.0}), ("rotate90", {"spatial_axes": (0, 1), "prob": 1.0}),
        ("affine", {"mode": ("bilinear", "nearest"), "rotate_range": (0.2, 0.2, 0.2), "scale_range": (0.1, 0.1, 0.1),
                    "padding_mode": "border", "prob": 1.0})]


# ---- window ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,size", [((10, 21, 16), (15, 16, 16)), ((11, 20, 9), (16, 13, 12))])
def test_window_is_the_fit_at_its_shifts_and_a_gathered_view(shape, size):
    rs = np.random.RandomState(1)
    vol = rs.randn(2, *shape).astype(np.float32)
    seg = rs.randint(0, 9, (1,) + shape).astype(np.int16)
    fit = [DS.fit_shift(n, t) for n, t in zip(shape, size)]
    assert any(d < 0 for d in fit) and any(d > 0 for d in fit)  # one axis pads, one crops
    for v in (vol, seg, vol[0]):
        out = DS.window(v, fit, size)
        assert out.dtype == v.dtype and out.shape == v.shape[:-3] + tuple(size)
        assert np.array_equal(out, DS.resize_with_pad_or_crop(v, size))
    for origin in (fit, (-3, 7, -2), (4, -5, 3), (-20, 30, 1), tuple(n - 2 for n in shape)):  # negative, overhanging
        assert any(o < 0 or o + t > n for o, t, n in zip(origin, size, shape))
        want = DS.gather_views(vol, [list(origin) + [0, 0, 0]], size)[0]
        assert np.array_equal(DS.window(vol, origin, size), want)
        idx = [np.clip(np.arange(t) + o, 0, n - 1) for o, t, n in zip(origin, size, shape)]
        assert np.array_equal(DS.window(seg, origin, size), seg[:, idx[0]][:, :, idx[1]][:, :, :, idx[2]])
    with pytest.raises(ValueError):
        DS.window(vol, (0, 0), size)


# ---- lesion_centres ----------------------------------------------------------------------------------------------------
def test_lesion_centres_follow_the_kept_boxes():
    seg = np.zeros((20, 24, 28), np.int16)
    seg[2:5, 3:9, 4:6] = 7       # extents (2..4, 3..8, 4..5): centre (3, 5.5, 4.5)
    seg[10:12, 10:11, 3:9] = 5   # flat along axis 1: dropped
    seg[15:20, 20:24, 0:2] = 3
    thr = [(1, np.inf)]
    c = DS.lesion_centres(seg[None], thr)
    boxes, _ = DS.boxes_from_instances(seg[None], thr)
    assert c.dtype == np.float64 and c.shape == (2, 3) == (boxes.shape[0], 3)
    assert c.tolist() == [[17.0, 21.5, 0.5], [3.0, 5.5, 4.5]]  # ascending id: 3, then 7
    size = np.array(seg.shape * 2, np.float64)
    ext = np.rint(boxes.numpy().astype(np.float64) * size)  # the device route's recovery of the integer extents
    assert np.array_equal((ext[:, :3] + ext[:, 3:]) / 2, c)
    two = DS.lesion_centres(seg + 1000 * (seg > 0) + 1000 * (seg == 3), [(1000, 2000), (2000, np.inf)])
    assert two.tolist() == [[3.0, 5.5, 4.5], [17.0, 21.5, 0.5]]  # pair order first
    assert DS.lesion_centres(np.zeros((4, 4, 4), np.int16), thr).shape == (0, 3)


# ---- normalize_nonzero_device --------------------------------------------------------------------------------------------
def test_normalize_nonzero_device_is_the_kernels_arithmetic_written_out():
    rs = np.random.RandomState(2)
    for shape in ((13, 17, 19), (3, 5, 7), (8, 16, 32)):  # 4199 and 105 voxels: no multiple of 1024, fewer than 1024; 4096
        vol = (rs.rand(*shape) * 100 + 1).astype(np.float32) * (rs.rand(*shape) < 0.7)
        vol.flat[5] = -3.5
        x = vol.reshape(-1)

        def lane_sum(f):  # lane t walks t, t + 1024, ...; then the tree over the lanes
            red = []
            for t in range(1024):
                s = 0.0
                for i in range(t, x.size, 1024):
                    if x[i] != 0:
                        s += f(float(x[i]))
                red.append(s)
            s = 512
            while s:
                for t in range(s):
                    red[t] = red[t] + red[t + s]
                s //= 2
            return red[0]

        count = int((x != 0).sum())
        mean = lane_sum(lambda v: v) / count
        std = np.float32(np.sqrt(lane_sum(lambda v: (v - mean) * (v - mean)) / count))
        want = np.where(vol != 0, (vol - np.float32(mean)) / std, vol).astype(np.float32)
        got = DS.normalize_nonzero_device(vol)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32))
        np.testing.assert_allclose(got, DS.normalize_nonzero(vol), rtol=1e-5, atol=1e-5)  # the bound of DESIGN.md 4.7
        assert not got[vol == 0].any()
    zero = np.zeros((4, 4, 4), np.float32)
    assert np.array_equal(DS.normalize_nonzero_device(zero), zero)
    flat = np.full((4, 4, 4), 2.5, np.float32)
    assert not DS.normalize_nonzero_device(flat).any()  # deviation 0 is taken as 1: (v - mean) / 1


# ---- patch_origin ------------------------------------------------------------------------------------------------------
def test_patch_origin_consumes_eight_draws_on_either_branch():
    centres = [[10.0, 20.5, 30.0], [50.0, 60.0, 40.0]]
    for fg, cs in ((1.0, centres), (0.0, centres), (1.0, np.zeros((0, 3))), (0.67, centres)):
        for seed in range(5):
            rs, ref = np.random.RandomState(seed), np.random.RandomState(seed)
            DS.patch_origin(rs, (60, 70, 50), (24, 32, 32), cs, fg)
            ref.random_sample(8)
            assert rs.random_sample() == ref.random_sample(), (fg, seed)


def test_patch_origin_on_a_lesion_shows_it():
    shape, patch = (60, 70, 50), (24, 32, 32)
    centres = np.array([[0.0, 0.5, 49.0], [59.0, 69.0, 0.0], [30.5, 35.0, 25.5], [11.0, 58.5, 40.0]])
    chosen = set()
    for seed in range(200):
        rs = np.random.RandomState(seed)
        u, ku = np.random.RandomState(seed).random_sample(2)
        k = min(int(ku * len(centres)), len(centres) - 1)
        chosen.add(k)
        o = DS.patch_origin(rs, shape, patch, centres, 1.0)
        assert all(isinstance(v, int) for v in o)
        for a in range(3):
            assert 0 <= o[a] <= shape[a] - patch[a]
            assert o[a] <= np.floor(centres[k][a]) < o[a] + patch[a], (seed, a)
    assert chosen == {0, 1, 2, 3}


def test_patch_origin_uniform_branch_and_small_cases():
    shape, patch = (60, 70, 50), (24, 32, 32)
    seen = [set() for _ in range(3)]
    for seed in range(400):
        o = DS.patch_origin(np.random.RandomState(seed), shape, patch, [[30.0, 30.0, 30.0]], 0.0)
        r = np.random.RandomState(seed).random_sample(8)[5:]
        assert list(o) == [int(np.floor(r[a] * (shape[a] - patch[a] + 1))) for a in range(3)]
        for a in range(3):
            assert 0 <= o[a] <= shape[a] - patch[a]
            seen[a].add(o[a])
    assert {0, shape[2] - patch[2]} <= seen[2]  # both extreme origins of the 19-position axis occur
    for seed in range(20):  # no lesion: the uniform branch whatever the probability
        a = DS.patch_origin(np.random.RandomState(seed), shape, patch, np.zeros((0, 3)), 1.0)
        b = DS.patch_origin(np.random.RandomState(seed), shape, patch, [[30.0, 30.0, 30.0]], 0.0)
        assert a == b
    # an axis no longer than the patch takes the fit's shift on either branch
    for fg in (0.0, 1.0):
        o = DS.patch_origin(np.random.RandomState(3), (20, 70, 32), patch, [[5.0, 30.0, 9.0]], fg)
        assert o[0] == DS.fit_shift(20, 24) == -2 and o[2] == 0 and 0 <= o[1] <= 38
    with pytest.raises(ValueError):
        DS.patch_origin(np.random.RandomState(0), (20, 70), patch, [], 0.5)


def test_centres_follow_the_signed_permutation_and_the_affine():
    rs = np.random.RandomState(5)
    shape = (9, 12, 7)
    vol = np.zeros(shape, np.float32)
    pts = np.array([[1, 2, 3], [8, 0, 6], [4, 11, 0]])
    for k, p in enumerate(pts):
        vol[tuple(p)] = k + 1
    draws = DS.draw_augmentations(AUGS[:2], rs)
    perm, stages = sample_params(draws, shape, AUGS[:2], ragged=True)
    x = vol[None]
    rs = np.random.RandomState(5)
    for name, kw in AUGS[:2]:
        x, _ = DS.AUGMENTATIONS[name](x, x, rs, **kw)
    moved = DS.centres_to_augmented(pts, shape, perm, stages)
    for k, q in enumerate(moved):  # the marked voxel is where the centre went
        assert x[0][tuple(int(v) for v in q)] == k + 1
    M, off = DS.affine_matrix(x.shape[1:], [1.1, 0.9, 1.0], [0.5, -1.0, 2.0], [0.1, -0.2, 0.3])
    from mslesions3d_amd.devicedata import AffineStage
    q = DS.centres_to_augmented(pts, shape, perm, [AffineStage(M, off, 1), None])
    np.testing.assert_allclose(q @ M.T + off, moved, rtol=0, atol=1e-12)  # output voxel q samples at M q + offset
    assert DS.centres_to_augmented(np.zeros((0, 3)), shape, perm, [AffineStage(M, off, 1)]).shape == (0, 3)


# ---- _LesionCases in patch mode ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return lesion_tree.make_tree(tmp_path_factory.mktemp("patches"), SHAPES)


def _module(tree, augmentations=None, **kw):
    dm = DS.LesionsDataModule(data_dir=tree, centers=lesion_tree.CENTERS, batch_size=2, spatial_size=(48, 64, 64),
                              augmentations=augmentations, **kw)
    dm.setup("fit")
    return dm


def test_a_patch_sample_equals_the_explicit_steps(tree):
    dm = _module(tree, AUGS, patch_size=PATCH, patch_foreground=0.8)
    plain = _module(tree, AUGS)
    tr = dm.train_dataset
    branches = set()
    for epoch in (0, 1):
        dm.set_epoch(epoch)
        plain.set_epoch(epoch)
        for i in range(len(tr)):
            got = tr[i]
            crop, seg = DS.crop_foreground(*tr.load(i), 5)
            img, seg = DS.normalize_nonzero_device(crop)[None], seg[None]  # patch mode: the device route's arithmetic
            shape = img.shape[1:]
            centres = DS.lesion_centres(seg, dm.thresholds)
            rs = tr.sample_rng(i)
            draws = DS.draw_augmentations(AUGS, tr.sample_rng(i))
            flip, (k, rot_ax), (zoom, shift, angles) = (d for _, d in draws)
            # flip + rot90 + affine, written out
            x, m = np.flip(img, [a + 1 for a in flip]), np.flip(seg, [a + 1 for a in flip])
            x, m = np.rot90(x, k, [a + 1 for a in rot_ax]), np.rot90(m, k, [a + 1 for a in rot_ax])
            c = centres.copy()
            for a in flip:
                c[:, a] = shape[a] - 1 - c[:, a]
            c = _rot90_points(c, k, rot_ax, shape)
            M, off = DS.affine_matrix(x.shape[1:], zoom, shift, angles)
            q = np.linalg.solve(M, (c - off).T).T if len(c) else c
            for name, kw in AUGS:  # the host transforms on the same generator
                img, seg = DS.AUGMENTATIONS[name](img, seg, rs, **kw)
            assert img.shape[1:] == x.shape[1:]
            u = np.random.RandomState(0)
            u.set_state(rs.get_state())
            branches.add(bool(len(q)) and u.random_sample() < 0.8)
            origin = DS.patch_origin(rs, img.shape[1:], PATCH, q, 0.8)
            assert got["patch_origin"] == origin
            assert np.array_equal(got["img"].numpy().view(np.int32), DS.window(img, origin, PATCH).view(np.int32))
            boxes, labels = DS.boxes_from_instances(DS.window(seg, origin, PATCH), dm.thresholds)
            assert torch.equal(got["boxes"], boxes) and torch.equal(got["labels"], labels)
            assert tuple(got["img"].shape) == (1,) + PATCH
            # the same sample without patches: the augmentation did not move (its image is normalize_nonzero's)
            fitted = plain.train_dataset[i]
            assert "patch_origin" not in fitted
            pimg, prs = DS.normalize_nonzero(crop)[None], tr.sample_rng(i)
            for name, kw in AUGS:
                pimg, _ = DS.AUGMENTATIONS[name](pimg, pimg, prs, **kw)
            assert np.array_equal(fitted["img"].numpy().view(np.int32),
                                  DS.resize_with_pad_or_crop(pimg, (48, 64, 64)).view(np.int32))
            fb, fl = DS.boxes_from_instances(DS.resize_with_pad_or_crop(seg, (48, 64, 64)), dm.thresholds)
            assert torch.equal(fitted["boxes"], fb) and torch.equal(fitted["labels"], fl)
    assert branches == {True, False}


def _rot90_points(c, k, ax, shape):
    """Where np.rot90(m, k, ax) of an array of ``shape`` puts the points ``c`` (K, 3) of m, from numpy's definition:
    k = 1: out[i, j] = m[j, n_b - 1 - i]; k = 2: out[i, j] = m[n_a - 1 - i, n_b - 1 - j]; k = 3: out[i, j] =
    m[n_a - 1 - j, i] on the axes (a, b)."""
    a, b = ax
    na, nb = shape[a], shape[b]
    out = np.array(c, dtype=np.float64).reshape(-1, 3)
    pa, pb = out[:, a].copy(), out[:, b].copy()
    k %= 4
    if k == 1:
        out[:, a], out[:, b] = nb - 1 - pb, pa
    elif k == 2:
        out[:, a], out[:, b] = na - 1 - pa, nb - 1 - pb
    elif k == 3:
        out[:, a], out[:, b] = pb, na - 1 - pa
    return out


def test_rot90_points_is_numpys_rot90():
    shape = (5, 7, 6)
    pts = np.array([[0, 0, 0], [4, 6, 5], [1, 5, 2]])
    m = np.zeros(shape, np.int32)
    for n, p in enumerate(pts):
        m[tuple(p)] = n + 1
    for ax in ((0, 1), (1, 2), (0, 2)):
        for k in (1, 2, 3):
            r = np.rot90(m, k, ax)
            for n, q in enumerate(_rot90_points(pts, k, ax, shape)):
                assert r[tuple(int(v) for v in q)] == n + 1


def test_the_augmentation_draws_do_not_depend_on_patch_mode(tree):
    augs = DS.select_augmentations(["flip", "rotate90", "affine", "shiftintensity", "scaleintensity"])
    dm, plain = _module(tree, augs, patch_size=PATCH), _module(tree, augs)
    for i in range(3):
        a, b = dm.train_dataset.sample_rng(i), plain.train_dataset.sample_rng(i)
        assert repr(DS.draw_augmentations(augs, a)) == repr(DS.draw_augmentations(augs, b))
    batches = list(dm.train_dataloader())
    assert all(tuple(b["img"].shape[1:]) == (1,) + PATCH and len(b["patch_origin"]) == len(b["subject"]) for b in batches)
    assert not any("patch_origin" in b for b in plain.train_dataloader())
    none = _module(tree, None, patch_size=PATCH)  # no augmentation: the window's draws are the generator's first eight
    s = none.train_dataset[0]
    img, seg = DS.crop_foreground(*none.train_dataset.load(0), 5)
    want = DS.patch_origin(none.train_dataset.sample_rng(0), seg.shape, PATCH, DS.lesion_centres(seg, none.thresholds), 0.67)
    assert s["patch_origin"] == want


def test_validation_tiles_enumerate_the_view_plan_and_cover_the_crops(tree):
    margin = (4, 6, 8)
    dm = _module(tree, None, patch_size=PATCH, tile_margin=margin)
    te = dm.test_dataset
    cases = te.cases
    want = []
    for i in range(len(cases)):
        img, seg = DS.crop_foreground(*cases.load(i), 5)
        plan = DS.view_plan(seg.shape, PATCH, margin)
        assert len(plan) > 1
        want += [(i, tuple(int(v) for v in row[:3])) for row in plan]
        covered = np.zeros(seg.shape, bool)
        for row in plan:
            covered[tuple(slice(max(o, 0), o + t) for o, t in zip(row[:3], PATCH))] = True
        assert covered.all()
    assert te.tiles == want and len(te) == len(want)
    norm = {i: DS.normalize_nonzero_device(DS.crop_foreground(*cases.load(i), 5)[0]) for i in range(len(cases))}
    batches = list(dm.test_dataloader())
    assert sum(len(b["subject"]) for b in batches) == len(want) and all(len(b["subject"]) <= 2 for b in batches)
    k = 0
    for b in batches:
        for n in range(len(b["subject"])):
            i, origin = want[k]
            k += 1
            seg = DS.crop_foreground(*cases.load(i), 5)[1]
            assert b["subject"][n] == cases.subjects[i] and b["patch_origin"][n] == origin
            assert b["crop_shape"][n] == seg.shape
            assert np.array_equal(b["img"][n, 0].numpy().view(np.int32), DS.window(norm[i], origin, PATCH).view(np.int32))
            boxes, labels = DS.boxes_from_instances(DS.window(seg, origin, PATCH), dm.thresholds)
            assert torch.equal(b["boxes"][n], boxes) and torch.equal(b["labels"][n], labels)


def test_the_module_and_the_entry_point_refuse_bad_patch_options(tree):
    from mslesions3d_amd import train as T
    for kw in ({"patch_size": (32, 32)}, {"patch_size": (32, 0, 32)}, {"patch_size": PATCH, "patch_foreground": 1.5},
               {"patch_size": PATCH, "tile_margin": (8, -1, 8)}):
        with pytest.raises(ValueError):
            DS.LesionsDataModule(data_dir=tree, centers=lesion_tree.CENTERS, **kw)
    args = T.build_parser().parse_args([])
    assert args.patch_size is None and args.patch_foreground == 0.67 and args.tile_margin == [8, 8, 8]
    assert T.patch_options_of(args) == {}
    args = T.build_parser().parse_args(["--patch_size", "32", "32", "32"])
    with pytest.raises(ValueError, match="-dm lesions"):  # raised before the first GPU call
        T.example(args)
    args = T.build_parser().parse_args(["-dm", "lesions", "--patch_size", "24", "32", "40", "--patch_foreground", "0.5",
                                        "--tile_margin", "4", "4", "6"])
    assert T.patch_options_of(args) == {"patch_size": (24, 32, 40), "patch_foreground": 0.5, "tile_margin": (4, 4, 6)}
