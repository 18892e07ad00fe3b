"""Separable warps on the host: datasets.zoom_table / grid_table, the draws and transforms of
'zoom' / 'griddistortion', select_training_augmentations, the lesion-centre map, devicedata.warp_numpy (the f64 mirror of
msl_augment_warp_mc) against scipy, and the lowering of the draws in devicedata.sample_params.  CPU only; every array
comparison is bit for bit."""
import numpy as np
import pytest
from scipy.ndimage import map_coordinates

from mslesions3d_amd import datasets as DS
from mslesions3d_amd import devicedata as DD
from tests import lesion_tree

SHAPES = [(9, 14, 11), (17, 30, 21)]
PADS = ("reflection", "border", "zeros")
GRID = {"num_cells": 5, "distort_limit": 0.3, "prob": 1.0}  # strong enough to leave the axis
ZOOM = {"min_zoom": 0.7, "max_zoom": 0.7, "prob": 1.0}
GRID_SEEDS = {(9, 14, 11): 1, (17, 30, 21): 0}  # chosen on the CPU: >= 5 % of the voxels sample outside the case


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(a, b):
    a, b = _bits(a), _bits(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


class Recorder:
    """A generator that notes every call made on it."""

    def __init__(self, seed=0):
        self.rs, self.calls = np.random.RandomState(seed), []

    def rand(self, *a):
        self.calls.append(("rand",) + a)
        return self.rs.rand(*a)

    def uniform(self, *a):
        self.calls.append(("uniform",) + a)
        return self.rs.uniform(*a)


# ---- tables ------------------------------------------------------------------------------------------------------------
def test_zoom_table_is_the_centred_scaling():
    for n in (1, 2, 9, 32, 250):
        assert np.array_equal(DS.zoom_table(n, 1.0), np.arange(n, dtype=np.float64))
    t = DS.zoom_table(11, 2.0)
    assert t.dtype == np.float64 and t[5] == 5.0 and t[0] == 2.5 and t[10] == 7.5  # z > 1 magnifies
    c = (14 - 1) / 2
    assert np.array_equal(DS.zoom_table(14, 0.7), (np.arange(14.0) - c) / 0.7 + c)


@pytest.mark.parametrize("n", [10, 35, 250])
def test_grid_table_with_unit_steps_steps_by_cell_over_cell_minus_one(n):
    cell = n // 5
    t = DS.grid_table(n, 5, np.ones(6))
    for s in range(5):
        seg = t[s * cell:(s + 1) * cell]
        assert seg[0] == s * cell and seg[-1] == (s + 1) * cell  # the border coordinate is written twice
        np.testing.assert_allclose(np.diff(seg), cell / (cell - 1), rtol=0, atol=1e-12)
        assert np.array_equal(seg, np.linspace(float(s * cell), float((s + 1) * cell), cell))


@pytest.mark.parametrize("n", [9, 11, 32, 250, 3, 1])
def test_grid_table_covers_every_index_and_decreases_in_no_full_segment(n):
    rs = np.random.RandomState(n)
    for _ in range(20):
        steps = 1.0 + rs.uniform(-0.3, 0.3, 6)
        t = DS.grid_table(n, 5, steps)
        assert t.shape == (n,) and t.dtype == np.float64 and np.isfinite(t).all()
        cell = max(n // 5, 1)
        full = n - n % cell  # the full segments end here; behind them the remainder segment runs to n
        assert t[0] == 0.0 and (np.diff(t[:full]) >= 0).all()
        if full == n or t[full - 1] <= n:
            assert (np.diff(t) >= 0).all()
        else:  # the rule as stated: a remainder segment that starts beyond n runs back to it
            assert t[-1] <= t[full - 1] and (t[-1] == n or full == n - 1)
        prev, want = 0.0, np.full(n, np.nan)
        for s in range(-(-n // cell)):  # the rule, segment by segment
            start, end = s * cell, min(s * cell + cell, n)
            cur = float(n) if start + cell > n else prev + cell * steps[min(s, 5)]
            want[start:end] = np.linspace(prev, cur, end - start)
            prev = cur
        assert np.array_equal(t, want)
    with pytest.raises(ValueError):
        DS.grid_table(9, 5, np.ones(5))
    with pytest.raises(ValueError):
        DS.grid_table(9, 5, [1, 1, 1, 0.0, 1, 1])


# ---- draws -------------------------------------------------------------------------------------------------------------
def test_draws_make_the_documented_calls_in_order():
    r = Recorder()
    assert DS._draw_zoom(r, prob=0.0) is None and r.calls == [("rand",)]
    r = Recorder()
    z = DS._draw_zoom(r, 0.8, 1.3, prob=1.0)
    assert r.calls == [("rand",), ("uniform", 0.8, 1.3)] and isinstance(z, float) and 0.8 <= z <= 1.3
    r = Recorder()
    assert DS._draw_griddistortion(r, prob=0.0) is None and r.calls == [("rand",)]
    r = Recorder(3)
    steps = DS._draw_griddistortion(r, num_cells=4, distort_limit=0.2, prob=1.0)
    assert r.calls == [("rand",)] + [("uniform", -0.2, 0.2, 5)] * 3  # a number f means (-f, f); axes 0, 1, 2
    ref = np.random.RandomState(3)
    ref.rand()
    for s in steps:
        assert s.shape == (5,) and np.array_equal(s, 1.0 + ref.uniform(-0.2, 0.2, 5))
    r = Recorder()
    DS._draw_griddistortion(r, distort_limit=(-0.01, 0.05), prob=1.0)
    assert r.calls[1:] == [("uniform", -0.01, 0.05, 6)] * 3
    for bad in (1.0, (-1.5, 0.1), (-0.1, 1.0)):
        with pytest.raises(ValueError):
            DS._draw_griddistortion(Recorder(), distort_limit=bad, prob=1.0)
    draws = DS.draw_augmentations(DS.WARP_AUGMENTATIONS, np.random.RandomState(5))
    assert [n for n, _ in draws] == ["zoom", "griddistortion"] and set(DS.DRAWS) == set(DS.AUGMENTATIONS)


# ---- warp_numpy against scipy ------------------------------------------------------------------------------------------
def _volume(shape, seed=0):
    rs = np.random.RandomState(seed)
    return rs.randn(*shape).astype(np.float32), ((rs.rand(*shape) < 0.4) * rs.randint(1, 3000, shape)).astype(np.int16)


def _tables(kind, shape):
    if kind == "zoom":
        return DS.warp_tables("zoom", DS._draw_zoom(np.random.RandomState(0), **ZOOM), shape, ZOOM)
    draw = DS._draw_griddistortion(np.random.RandomState(GRID_SEEDS[shape]), **GRID)
    return DS.warp_tables("griddistortion", draw, shape, GRID)


def _outside_share(tables, shape):
    grids = np.meshgrid(*tables, indexing="ij")
    out = np.zeros(shape, bool)
    for g, n in zip(grids, shape):
        out |= (g < 0) | (g > n - 1)
    return float(out.mean())


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("kind", ["zoom", "griddistortion"])
@pytest.mark.parametrize("shape", SHAPES)
def test_warp_numpy_is_map_coordinates_bit_for_bit(shape, kind, pad):
    img, seg = _volume(shape)
    tables = _tables(kind, shape)
    share = _outside_share(tables, shape)
    print(f"{kind} {shape}: {share:.3f} of the output voxels sample outside the case")
    assert share >= 0.05
    grids = np.meshgrid(*tables, indexing="ij")
    want_i = map_coordinates(img, grids, order=1, mode=DS.SCIPY_BOUNDARY[pad])
    want_s = map_coordinates(seg.astype(np.float32), grids, order=0, mode=DS.SCIPY_BOUNDARY[pad]).astype(np.int16)
    got_i = DD.warp_numpy(img, tables, 1, DD.BOUNDARY[pad])
    got_s = DD.warp_numpy(seg, tables, 0, DD.BOUNDARY[pad])
    assert _same(got_i, want_i) and _same(got_s, want_s)
    assert not np.array_equal(got_i, img) and want_s.any()


@pytest.mark.parametrize("pad", PADS)
def test_the_transforms_are_the_warp_of_their_tables(pad):
    shape = SHAPES[1]
    img, seg = _volume(shape, 2)
    img, seg = np.stack([img, img * 2 + 1]), seg[None]
    for name, kw, seed in (("zoom", ZOOM, 0), ("griddistortion", GRID, GRID_SEEDS[shape])):
        kw = dict(kw, padding_mode=pad)
        oi, os_ = DS.AUGMENTATIONS[name](img, seg, np.random.RandomState(seed), **kw)
        tables = DS.warp_tables(name, DS.DRAWS[name](np.random.RandomState(seed), **kw), shape, kw)
        assert oi.dtype == np.float32 and os_.dtype == np.int16 and oi.shape == img.shape and os_.shape == seg.shape
        for c in range(2):
            assert _same(oi[c], DD.warp_numpy(img[c], tables, 1, DD.BOUNDARY[pad]))
        assert _same(os_[0], DD.warp_numpy(seg[0], tables, 0, DD.BOUNDARY[pad]))
        a, b = DS.AUGMENTATIONS[name](img, seg, np.random.RandomState(seed), **dict(kw, prob=0.0))
        assert a is img and b is seg


def test_warp_numpy_refuses_tables_of_another_shape():
    img, _ = _volume((5, 6, 7))
    with pytest.raises(ValueError):
        DD.warp_numpy(img, [np.arange(5.0), np.arange(6.0), np.arange(6.0)], 1, 1)


# ---- selection ---------------------------------------------------------------------------------------------------------
def test_select_training_augmentations_puts_the_warps_between_affines_and_intensity():
    names = ["scaleintensity", "griddistortion", "flip", "zoom", "affine", "shiftintensity", "rotate90", "translate"]
    got = DS.select_training_augmentations(names)
    assert [n for n, _ in got] == ["flip", "rotate90", "rotate90", "rotate90", "affine", "affine", "zoom",
                                   "griddistortion", "shiftintensity", "scaleintensity"]
    assert got[6][1] is DS.WARP_AUGMENTATIONS[0][1] and got[7][1] is DS.WARP_AUGMENTATIONS[1][1]
    plain = ["flip", "rotate90", "affine", "shiftintensity"]
    assert DS.select_training_augmentations(plain) == DS.select_augmentations(plain)  # the reference's names unchanged
    assert [n for n, _ in DS.select_training_augmentations(["griddistortion"])] == ["griddistortion"]
    assert [n for n, _ in DS.select_training_augmentations(["zoom", "flip"])] == ["flip", "zoom"]
    assert DS.select_training_augmentations([]) == []
    assert DS.WARP_AUGMENTATIONS == [
        ("zoom", {"min_zoom": 0.9, "max_zoom": 1.1, "padding_mode": "border", "prob": 0.5}),
        ("griddistortion", {"num_cells": 5, "distort_limit": 0.03, "padding_mode": "border", "prob": 0.5})]
    with pytest.raises(ValueError):
        DS.select_training_augmentations(["flip", "elastic"])
    for name in ("zoom", "griddistortion"):  # the mirror of the reference's lists keeps refusing them
        with pytest.raises(ValueError):
            DS.select_augmentations([name])


# ---- lesion centres ----------------------------------------------------------------------------------------------------
def _interp(t, q):
    lo = np.clip(np.floor(q).astype(int), 0, len(t) - 2)
    return t[lo] + (q - lo) * (t[lo + 1] - t[lo])


@pytest.mark.parametrize("kind", ["zoom", "griddistortion", "magnify"])
def test_centres_to_augmented_inverts_the_tables(kind):
    shape = (20, 30, 25)  # no remainder segment: the grid tables are sorted at any distortion
    if kind == "magnify":
        tables = [DS.zoom_table(n, 1.4) for n in shape]
    elif kind == "zoom":
        tables = [DS.zoom_table(n, 0.7) for n in shape]
    else:
        steps = DS._draw_griddistortion(np.random.RandomState(2), **GRID)
        tables = DS.warp_tables("griddistortion", steps, shape, GRID)
        assert all((np.diff(t) >= 0).all() and (np.diff(t) == 0).sum() == 4 for t in tables)
    stage = DD.WarpStage(tables, 1)
    rs = np.random.RandomState(1)
    lo, hi = np.array([t[0] for t in tables]), np.array([t[-1] for t in tables])
    c = np.maximum(lo, 0) + rs.rand(40, 3) * (np.minimum(hi, np.array(shape) - 1.0) - np.maximum(lo, 0))
    c[0] = np.minimum(np.ceil(c[0]), np.floor(np.minimum(hi, np.array(shape) - 1.0)))  # whole voxels inside the range
    for a in range(3):
        c[1 + a] = [t[len(t) // 2] for t in tables]  # exactly a table value (grid: maybe a doubled one)
    ident = ((0, 1, 2), (0, 0, 0))
    q = DS.centres_to_augmented(c, shape, ident, [None, stage, DD.IntensityOp(DD.OP_ADD, np.float32(1))])
    assert q.shape == c.shape and (q >= 0).all() and (q <= np.array(shape) - 1.0).all()
    for a in range(3):
        assert np.abs(_interp(tables[a], q[:, a]) - c[:, a]).max() <= 1e-9
        i = np.searchsorted(tables[a], c[:, a], "left")  # the smallest such q: it lies in the first interval that reaches c'
        assert (q[:, a] <= i).all() and (q[:, a] >= i - 1).all()
    # outside the table's range the point is clamped onto the axis
    far = np.array([[-100.0, 5.0, 1000.0]])
    q = DS.centres_to_augmented(far, shape, ident, [stage])
    assert q[0, 0] == 0.0 and q[0, 2] == shape[2] - 1.0
    # behind a signed permutation the tables belong to the permuted shape
    perm = ((2, 0, 1), (1, 0, 0))
    pshape = tuple(shape[a] for a in perm[0])
    st = DD.WarpStage([DS.zoom_table(n, 0.8) for n in pshape], 1)
    pt = np.array([[3.0, 20.0, 10.0]])
    moved = DS.centres_to_augmented(pt, shape, perm, [st])
    plain = DS.centres_to_augmented(pt, shape, perm, [])
    for a in range(3):
        assert abs(_interp(st.tables[a], moved[:, a])[0] - plain[0, a]) <= 1e-9


# ---- sample_params -----------------------------------------------------------------------------------------------------
def test_sample_params_lowers_a_drawn_warp_for_the_permuted_shape():
    shape = (9, 14, 11)
    augs = [("rotate90", {"spatial_axes": (0, 1), "prob": 1.0, "max_k": 1}),  # a quarter turn: the shape changes
            ("griddistortion", dict(GRID, padding_mode="zeros")), ("shiftintensity", {"offsets": 0.1, "prob": 1.0})]
    draws = DS.draw_augmentations(augs, np.random.RandomState(4))
    perm, stages = DD.sample_params(draws, shape, augs, ragged=True)
    pshape = tuple(shape[a] for a in perm[0])
    assert pshape != shape and len(stages) == 2
    st = stages[0]
    assert isinstance(st, DD.WarpStage) and st.boundary == DD.BOUNDARY["zeros"] and isinstance(stages[1], DD.IntensityOp)
    assert [len(t) for t in st.tables] == list(pshape)
    for t, n, s in zip(st.tables, pshape, draws[1][1]):
        assert np.array_equal(t, DS.grid_table(n, 5, s))
    zoom = [("zoom", dict(ZOOM))]  # the padding of an entry without one is "border"
    perm, stages = DD.sample_params(DS.draw_augmentations(zoom, np.random.RandomState(0)), shape, zoom, ragged=True)
    assert stages[0].boundary == DD.BOUNDARY["border"] and np.array_equal(stages[0].tables[1], DS.zoom_table(14, 0.7))
    perm, stages = DD.sample_params([("zoom", None), ("griddistortion", None)], shape, None, ragged=True)
    assert stages == [None, None]
    # the rows of a launch: [7] = 2, the tables' offset, the boundary; the tables behind one another
    per = [DD.sample_params(DS.draw_augmentations(augs, np.random.RandomState(s)), shape, augs, ragged=True) for s in (4, 5)]
    per.insert(1, (([0, 1, 2], [0, 0, 0]), []))
    rows, coords = DD.warp_rows([0, 1, 0], per)
    assert rows.shape == (3, DD.AFFINE_STRIDE) and coords.dtype == np.float64 and coords.size == 2 * sum(shape)
    assert rows[:, 7].tolist() == [2.0, 0.0, 2.0] and rows[:, 8].tolist() == [0.0, 0.0, float(sum(shape))]
    assert rows[0, 20] == DD.BOUNDARY["zeros"] and rows[0, 21] == 1 and rows[1, 21] == 0
    assert np.array_equal(coords[sum(shape):], np.concatenate(per[2][1][0].tables))
    assert np.array_equal(DD.warp_rows([0], [per[1]])[0], DD.fit_rows([0], [per[1]])) and DD.warp_rows([0], [per[1]])[1].size == 0
    with pytest.raises(ValueError):
        DD.fit_rows([0, 1, 0], per)


def test_orderings_and_the_two_stage_refusal():
    zoom, grid = ("zoom", dict(ZOOM)), ("griddistortion", dict(GRID))
    flip, shift = ("flip", {"prob": 1.0}), ("shiftintensity", {"offsets": 0.1, "prob": 1.0})
    affine = ("affine", {"scale_range": (0.1, 0.1, 0.1), "padding_mode": "border", "prob": 1.0})

    def lower(augs, ragged=True):
        return DD.sample_params(DS.draw_augmentations(augs, np.random.RandomState(0)), (9, 14, 11), augs, ragged=ragged)

    lower([flip, zoom, shift])
    with pytest.raises(NotImplementedError, match="after an affine stage"):
        lower([zoom, flip])
    with pytest.raises(NotImplementedError, match="after an intensity operation"):
        lower([shift, grid])
    with pytest.raises(NotImplementedError, match="zoom / griddistortion on the example cache"):
        lower([grid], ragged=False)
    DD.check_ragged_pipeline([flip, grid, shift])
    for two in ([affine, zoom], [zoom, grid], [grid, affine], [grid, grid]):
        with pytest.raises(NotImplementedError, match="two affine stages on cases of unequal shape"):
            DD.check_ragged_pipeline([flip] + two + [shift])
        with pytest.raises(NotImplementedError, match="two affine stages on cases of unequal shape"):
            DD.warp_rows([0], [lower(two)])
    with pytest.raises(NotImplementedError, match="after an affine stage"):
        DD.check_ragged_pipeline([grid, flip])

    class _Example:  # DeviceCache refuses the names before it touches the device
        class train_dataset:
            augmentations = [flip, grid]
        n_classes, batch_size = 1, 2

    with pytest.raises(NotImplementedError, match="device pipeline: zoom / griddistortion on the example cache"):
        DD.DeviceCache(_Example, "cpu")


# ---- the data set ------------------------------------------------------------------------------------------------------
TREE = [(40, 44, 50), (52, 48, 46), (44, 70, 52)]


@pytest.mark.parametrize("name,kw", [("griddistortion", dict(GRID, distort_limit=0.15)),
                                     ("zoom", {"min_zoom": 0.75, "max_zoom": 1.3, "prob": 1.0})])
def test_lesion_cases_box_the_warped_mask(tmp_path, name, kw):
    data_dir = lesion_tree.make_tree(tmp_path, TREE)
    augs = [("flip", {"spatial_axis": (0, 1, 2), "prob": 0.5}), (name, kw)]
    target = (36, 48, 40)
    dm = DS.LesionsDataModule(data_dir=data_dir, centers=lesion_tree.CENTERS, batch_size=2, spatial_size=target,
                              augmentations=augs, subject=None)
    dm.setup("fit")
    tr = dm.train_dataset
    plain = DS._LesionCases(dm, tr.subjects)
    moved = seen = 0
    for i in range(len(tr)):
        got = tr[i]
        img, seg = tr.cropped(i)[:2]
        rs = tr.sample_rng(i)
        for n, k in augs:
            img, seg = DS.AUGMENTATIONS[n](img, seg, rs, **k)
        want_i = DS.resize_with_pad_or_crop(img, target)
        boxes, labels = DS.boxes_from_instances(DS.resize_with_pad_or_crop(seg, target), dm.thresholds)
        assert _same(got["img"].numpy(), want_i) and _same(got["boxes"].numpy(), boxes.numpy())
        assert got["labels"].tolist() == labels.tolist()
        seen += len(labels)
        base = plain[i]["boxes"].numpy()
        moved += base.shape != boxes.numpy().shape or not np.array_equal(np.sort(base, 0), np.sort(boxes.numpy(), 0))
    assert moved == len(tr) and seen >= 3  # every case's boxes moved with its mask


def test_patches_find_their_lesion_behind_a_warp(tmp_path):
    data_dir = lesion_tree.make_tree(tmp_path, TREE)
    augs = [("rotate90", {"spatial_axes": (0, 1), "prob": 1.0}), ("griddistortion", dict(GRID, distort_limit=0.15))]
    patch = (16, 16, 16)
    dm = DS.LesionsDataModule(data_dir=data_dir, centers=lesion_tree.CENTERS, batch_size=2, augmentations=augs,
                              patch_size=patch, patch_foreground=1.0)
    dm.setup("fit")
    tr = dm.train_dataset
    for epoch in (0, 1):
        tr.set_epoch(epoch)
        for i in range(len(tr)):
            got = tr[i]
            img, seg = tr.cropped(i)[:2]
            rs = tr.sample_rng(i)
            for n, k in augs:
                img, seg = DS.AUGMENTATIONS[n](img, seg, rs, **k)
            origin = got["patch_origin"]
            assert _same(got["img"].numpy(), DS.window(img, origin, patch))
            # the window was aimed at a lesion's centre mapped through the warp: it holds lesion voxels
            assert DS.window(seg, origin, patch).any(), (epoch, i, origin)
