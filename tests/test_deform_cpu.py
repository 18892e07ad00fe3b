"""The free-form deformation on the host: datasets.deform_lattice / deform_coords against the
contract written out as a scalar loop, the cap and what it guarantees, the draw and transform of 'elastic3d',
select_training_augmentations, the lesion-centre map, devicedata.deform_numpy (the f64 mirror of msl_augment_deform_mc)
against scipy, and the lowering of the draw in devicedata.sample_params.  CPU only; every array comparison is bit for
bit unless a bound is stated."""
import functools
import math

import numpy as np
import pytest
from scipy.ndimage import map_coordinates

from mslesions3d_amd import datasets as DS
from mslesions3d_amd import devicedata as DD
from tests import lesion_tree

SHAPES = [(9, 14, 11), (17, 30, 21)]
PADS = ("reflection", "border", "zeros")
BIG = 100.0  # a max_displacement the cap always undercuts on these shapes
# chosen on the CPU: >= 2 % of the voxels sample outside the case and >= half of them move by more than 0.25 voxel
SEEDS = {((9, 14, 11), 4): 0, ((9, 14, 11), 5): 0, ((17, 30, 21), 4): 0, ((17, 30, 21), 5): 0}


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


def _lattice(shape, L, seed=0, max_displacement=BIG):
    draw = DS._draw_elastic3d(np.random.RandomState(seed), control_points=L, max_displacement=max_displacement, prob=1.0)
    return DS.deform_lattice(shape, draw, max_displacement)


# ---- the contract, written out -------------------------------------------------------------------------------------------
def _axis(q, n, L):
    """One axis of one voxel: (cell, t, [b0 .. b3]) in Python floats (IEEE doubles, one rounding per operation)."""
    u = q * (L - 3) / (n - 1) if n > 1 else 0.0
    cell = min(int(math.floor(u)), L - 4)
    t = u - cell
    t2 = t * t
    t3 = t2 * t
    s = 1.0 - t
    return cell, t, [((s * s) * s) / 6.0,
                     (((3.0 * t3) - (6.0 * t2)) + 4.0) / 6.0,
                     ((((-3.0 * t3) + (3.0 * t2)) + (3.0 * t)) + 1.0) / 6.0,
                     t3 / 6.0]


def _coords_by_the_loop(shape, P):
    L = P.shape[1]
    Pl = P.tolist()
    out = np.empty((3,) + tuple(shape))
    for q0 in range(shape[0]):
        c0, _, b0 = _axis(float(q0), shape[0], L)
        for q1 in range(shape[1]):
            c1, _, b1 = _axis(float(q1), shape[1], L)
            R = [[0.0] * L for _ in range(3)]
            for m in range(3):
                for k2 in range(L):
                    r = 0.0
                    for j in range(4):
                        inner = 0.0
                        for i in range(4):
                            inner = inner + (b0[i] * Pl[m][c0 + i][c1 + j][k2])
                        r = r + (b1[j] * inner)
                    R[m][k2] = r
            for q2 in range(shape[2]):
                c2, _, b2 = _axis(float(q2), shape[2], L)
                q = (q0, q1, q2)
                for m in range(3):
                    d = 0.0
                    for k in range(4):
                        d = d + (b2[k] * R[m][c2 + k])
                    out[m, q0, q1, q2] = float(q[m]) + d
    return out


@pytest.mark.parametrize("L", [4, 7])
def test_deform_coords_is_the_contract_written_out(L):
    shape = SHAPES[0]
    P = _lattice(shape, L, seed=3)
    got = DS.deform_coords(shape, P)
    want = _coords_by_the_loop(shape, P)
    assert len(got) == 3 and all(g.dtype == np.float64 and g.shape == shape for g in got)
    for m in range(3):
        assert np.array_equal(got[m], want[m]), m
    grid = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    assert any(not np.array_equal(g, i) for g, i in zip(got, grid))
    # at whole voxels the point form is the same spline
    q = np.stack([g.reshape(-1) for g in grid], 1)
    d = DS.deform_displacement(shape, P, q)
    for m in range(3):
        assert np.array_equal(q[:, m] + d[:, m], got[m].reshape(-1))


@pytest.mark.parametrize("L", [4, 5, 7, 16])
def test_a_zero_lattice_is_the_index_grid_and_the_weights_sum_to_one(L):
    for shape in SHAPES + [(1, 6, 1), (5, 7, 130)]:
        got = DS.deform_coords(shape, np.zeros((3, L, L, L)))
        for g, i in zip(got, np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")):
            assert np.array_equal(g, i)
        for n in shape:
            cell, b = DS._spline_taps(np.arange(n), n, L)
            assert np.abs((b[0] + b[1]) + (b[2] + b[3]) - 1.0).max() <= 2.0 ** -52
            assert cell.min() == 0 and cell.max() <= L - 4
            for q in range(n):  # the vector form against the scalar one
                c, t, bs = _axis(float(q), n, L)
                assert c == cell[q] and [x[q] for x in b] == bs
            c, t, bs = _axis(float(n - 1), n, L)
            if n > 1:  # the last voxel lies at the far end of the last cell
                assert c == L - 4 and t == 1.0 and bs[0] == 0.0 and bs[3] == 1.0 / 6.0
            else:
                assert c == 0 and t == 0.0


# ---- the cap -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [4, 5, 7])
@pytest.mark.parametrize("shape", SHAPES)
def test_the_cap_bounds_the_displacement_and_keeps_the_map_from_folding(shape, L):
    draw = np.random.RandomState(1).uniform(-1.0, 1.0, (3, L, L, L))
    spacing = min((n - 1) / (L - 3) for n in shape)
    for md in (BIG, 0.3):
        P = DS.deform_lattice(shape, draw, md)
        A = min(md, spacing / 4)
        assert P.dtype == np.float64 and np.array_equal(P, draw * A)
    P = DS.deform_lattice(shape, draw, BIG)
    A = spacing / 4
    coords = DS.deform_coords(shape, P)
    grid = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    for c, g in zip(coords, grid):
        assert np.abs(c - g).max() <= A
    # the Jacobian of q -> q + d(q) by differences between neighbouring voxels: positive determinant at every voxel
    J = np.stack([np.stack(np.gradient(c), -1) for c in coords], -2)  # (..., m, a) = d c_m / d q_a
    det = np.linalg.det(J)
    print(f"{shape} L={L}: A = {A}, det in [{det.min():.3f}, {det.max():.3f}]")
    assert det.shape == shape and (det > 0).all()


def test_an_axis_of_one_voxel_is_left_out():
    draw = np.random.RandomState(2).uniform(-1.0, 1.0, (3, 5, 5, 5))
    P = DS.deform_lattice((9, 1, 11), draw, BIG)
    assert not P[1].any() and np.array_equal(P[0], draw[0] * (8 / 2 / 4)) and np.array_equal(P[2], draw[2] * 1.0)
    c = DS.deform_coords((9, 1, 11), P)
    assert not c[1].any() and (c[0] != np.arange(9.0).reshape(-1, 1, 1)).any()
    assert not DS.deform_lattice((1, 1, 1), draw, BIG).any()
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            DS.deform_lattice((9, 14, 11), draw, bad)
    for L in (3, 17):
        with pytest.raises(ValueError):
            DS.deform_lattice((9, 14, 11), np.zeros((3, L, L, L)), 1.0)


# ---- the draw ------------------------------------------------------------------------------------------------------------
def test_the_draw_makes_the_documented_calls_in_order():
    r = Recorder()
    assert DS._draw_elastic3d(r, prob=0.0) is None and r.calls == [("rand",)]
    r = Recorder(3)
    d = DS._draw_elastic3d(r, control_points=5, max_displacement=2.0, prob=1.0)
    assert r.calls == [("rand",), ("uniform", -1.0, 1.0, (3, 5, 5, 5))]
    ref = np.random.RandomState(3)
    ref.rand()
    assert d.dtype == np.float64 and np.array_equal(d, ref.uniform(-1.0, 1.0, (3, 5, 5, 5)))
    r = Recorder()
    assert DS._draw_elastic3d(r, prob=1.0).shape == (3, 7, 7, 7)  # the default lattice
    img = np.zeros((1, 4, 5, 6), np.float32)
    seg = np.zeros((1, 4, 5, 6), np.int16)
    r = Recorder()
    a, b = DS.AUGMENTATIONS["elastic3d"](img, seg, r, prob=0.0)
    assert a is img and b is seg and r.calls == [("rand",)]
    for kw in ({"control_points": 3}, {"control_points": 17}, {"max_displacement": 0.0}, {"max_displacement": -2.0}):
        for prob in (0.0, 1.0):  # refused whether drawn or not, on the host route as on the device route's lowering
            with pytest.raises(ValueError):
                DS._draw_elastic3d(Recorder(), prob=prob, **kw)
            with pytest.raises(ValueError):
                DS.AUGMENTATIONS["elastic3d"](img, seg, Recorder(), prob=prob, **kw)
    draws = DS.draw_augmentations(DS.DEFORM_AUGMENTATIONS, np.random.RandomState(5))
    assert [n for n, _ in draws] == ["elastic3d"] and set(DS.DRAWS) == set(DS.AUGMENTATIONS)


# ---- deform_numpy against scipy ------------------------------------------------------------------------------------------
def _volume(shape, seed=0):
    rs = np.random.RandomState(seed)
    return rs.randn(*shape).astype(np.float32), ((rs.rand(*shape) < 0.4) * rs.randint(1, 3000, shape)).astype(np.int16)


@functools.lru_cache(maxsize=None)
def _case(shape, L):
    P = _lattice(shape, L, SEEDS[(shape, L)])
    coords = DS.deform_coords(shape, P)
    for c in coords:
        c.setflags(write=False)
    return P, coords


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("L", [4, 5])
@pytest.mark.parametrize("shape", SHAPES)
def test_deform_numpy_is_map_coordinates_bit_for_bit(shape, L, pad):
    img, seg = _volume(shape)
    P, coords = _case(shape, L)
    assert np.abs(P).max() <= min((n - 1) / (L - 3) for n in shape) / 4 < BIG  # the cap binds
    grid = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    outside = np.zeros(shape, bool)
    for c, n in zip(coords, shape):
        outside |= (c < 0) | (c > n - 1)
    moved = np.sqrt(sum((c - g) ** 2 for c, g in zip(coords, grid))) > 0.25
    print(f"{shape} L={L}: {outside.mean():.3f} of the voxels sample outside the case, {moved.mean():.3f} move by more "
          f"than 0.25 voxel")
    assert outside.mean() >= 0.02 and moved.mean() >= 0.5
    want_i = map_coordinates(img, coords, order=1, mode=DS.SCIPY_BOUNDARY[pad])
    want_s = map_coordinates(seg.astype(np.float32), coords, order=0, mode=DS.SCIPY_BOUNDARY[pad]).astype(np.int16)
    got_i = DD.deform_numpy(img, P, 1, DD.BOUNDARY[pad])
    got_s = DD.deform_numpy(seg, P, 0, DD.BOUNDARY[pad])
    assert _same(got_i, want_i) and _same(got_s, want_s)
    assert not np.array_equal(got_i, img) and want_s.any()
    if np.abs(P).max() > 1.5:  # (a nearest-neighbour tap moves once a component passes half a voxel)
        assert not np.array_equal(got_s, seg)


@pytest.mark.parametrize("pad", PADS)
def test_the_transform_is_the_deformation_of_its_lattice(pad):
    shape = SHAPES[1]
    img, seg = _volume(shape, 2)
    img, seg = np.stack([img, img * 2 + 1]), seg[None]
    kw = {"control_points": 5, "max_displacement": 1.5, "padding_mode": pad, "prob": 1.0}
    oi, os_ = DS.AUGMENTATIONS["elastic3d"](img, seg, np.random.RandomState(4), **kw)
    P = DS.deform_lattice(shape, DS.DRAWS["elastic3d"](np.random.RandomState(4), **kw), 1.5)
    assert np.abs(P).max() > 1.4  # max_displacement binds here, not the cap
    assert oi.dtype == np.float32 and os_.dtype == np.int16 and oi.shape == img.shape and os_.shape == seg.shape
    for c in range(2):
        assert _same(oi[c], DD.deform_numpy(img[c], P, 1, DD.BOUNDARY[pad]))
    assert _same(os_[0], DD.deform_numpy(seg[0], P, 0, DD.BOUNDARY[pad]))


# ---- selection -------------------------------------------------------------------------------------------------------------
def test_select_training_augmentations_puts_the_deformation_behind_the_warps():
    names = ["scaleintensity", "elastic3d", "griddistortion", "flip", "zoom", "affine", "shiftintensity", "gaussiannoise"]
    got = DS.select_training_augmentations(names)
    assert [n for n, _ in got] == ["flip", "affine", "zoom", "griddistortion", "elastic3d", "shiftintensity",
                                   "scaleintensity", "gaussiannoise"]
    assert got[4][1] is DS.DEFORM_AUGMENTATIONS[0][1]
    assert [n for n, _ in DS.select_training_augmentations(["elastic3d", "rotate90", "flip"])] == \
        ["flip"] + ["rotate90"] * 3 + ["elastic3d"]
    assert [n for n, _ in DS.select_training_augmentations(["elastic3d"])] == ["elastic3d"]
    for plain in (["flip", "rotate90", "affine", "shiftintensity"], ["scale", "translate"], []):
        assert DS.select_training_augmentations(plain) == DS.select_augmentations(plain)
    without = ["scaleintensity", "griddistortion", "flip", "zoom", "biasfield"]
    assert DS.select_training_augmentations(without + ["elastic3d"]) == \
        [e for e in DS.select_training_augmentations(without)][:3] + DS.DEFORM_AUGMENTATIONS + \
        DS.select_training_augmentations(without)[3:]
    assert DS.DEFORM_AUGMENTATIONS == [
        ("elastic3d", {"control_points": 7, "max_displacement": 7.5, "padding_mode": "border", "prob": 0.2})]
    assert DS.WARP_AUGMENTATIONS == [
        ("zoom", {"min_zoom": 0.9, "max_zoom": 1.1, "padding_mode": "border", "prob": 0.5}),
        ("griddistortion", {"num_cells": 5, "distort_limit": 0.03, "padding_mode": "border", "prob": 0.5})]
    assert DD.WARP_NAMES == ("zoom", "griddistortion")
    with pytest.raises(ValueError):
        DS.select_augmentations(["elastic3d"])
    with pytest.raises(ValueError):
        DS.select_training_augmentations(["flip", "elastic"])
    assert set(DS.DRAWS) == set(DS.AUGMENTATIONS) and "elastic3d" in DS.DRAWS


# ---- lesion centres --------------------------------------------------------------------------------------------------------
def test_centres_to_augmented_inverts_the_deformation():
    shape, L = (17, 30, 21), 5
    P = _lattice(shape, L, 7)
    assert np.abs(P).max() > 1.9  # A = 2: the cap binds
    stage = DD.DeformStage(P, 1)
    rs = np.random.RandomState(1)
    hi = np.array(shape) - 1.0
    c = 3.0 + rs.rand(50, 3) * (hi - 6.0)  # interior: further from every face than the displacement reaches
    ident = ((0, 1, 2), (0, 0, 0))
    q = DS.centres_to_augmented(c, shape, ident, [None, stage, DD.IntensityOp(DD.OP_ADD, np.float32(1))])
    assert q.shape == c.shape and (q >= 0).all() and (q <= hi).all()
    err = np.abs(q + DS.deform_displacement(shape, P, q) - c).max()
    print(f"centre map: |q + d(q) - c'| <= {err:.3e} voxel, points moved by up to {np.abs(q - c).max():.3f}")
    assert err <= 1e-6 and np.abs(q - c).max() > 0.5
    # behind a signed permutation the lattice belongs to the permuted shape
    perm = ((2, 0, 1), (1, 0, 0))
    pshape = tuple(shape[a] for a in perm[0])
    st = DD.DeformStage(_lattice(pshape, L, 8), 1)
    pt = np.array([[8.0, 14.0, 10.0]])
    moved = DS.centres_to_augmented(pt, shape, perm, [st])
    plain = DS.centres_to_augmented(pt, shape, perm, [])
    assert np.abs(moved + DS.deform_displacement(pshape, st.lattice, moved) - plain).max() <= 1e-6
    assert DS.centres_to_augmented(np.zeros((0, 3)), shape, ident, [stage]).shape == (0, 3)


# ---- sample_params -----------------------------------------------------------------------------------------------------------
ELASTIC = {"control_points": 5, "max_displacement": BIG, "prob": 1.0}


def test_sample_params_lowers_a_drawn_deformation_for_the_permuted_shape():
    shape = (9, 14, 11)
    augs = [("rotate90", {"spatial_axes": (0, 1), "prob": 1.0, "max_k": 1}),  # a quarter turn: the shape changes
            ("elastic3d", dict(ELASTIC, padding_mode="zeros")), ("shiftintensity", {"offsets": 0.1, "prob": 1.0})]
    draws = DS.draw_augmentations(augs, np.random.RandomState(4))
    perm, stages = DD.sample_params(draws, shape, augs, ragged=True)
    pshape = tuple(shape[a] for a in perm[0])
    assert pshape == (14, 9, 11) and len(stages) == 2
    st = stages[0]
    assert isinstance(st, DD.DeformStage) and st.boundary == DD.BOUNDARY["zeros"] and isinstance(stages[1], DD.IntensityOp)
    assert np.array_equal(st.lattice, DS.deform_lattice(pshape, draws[1][1], BIG)) and st.lattice.shape == (3, 5, 5, 5)
    plain = [("elastic3d", {"prob": 1.0})]  # the entry's defaults: border, 7 points, 7.5 voxels
    perm, stages = DD.sample_params(DS.draw_augmentations(plain, np.random.RandomState(0)), (200, 210, 220), plain, ragged=True)
    assert stages[0].boundary == DD.BOUNDARY["border"] and stages[0].lattice.shape == (3, 7, 7, 7)
    assert np.abs(stages[0].lattice).max() > 7.0
    perm, stages = DD.sample_params([("elastic3d", None)], shape, None, ragged=True)
    assert stages == [None]
    # the rows of a launch: [7] = 3, the lattice's offset, L, the boundary; the lattices behind one another
    per = [DD.sample_params(DS.draw_augmentations(augs, np.random.RandomState(s)), shape, augs, ragged=True) for s in (4, 5)]
    per.insert(1, (([0, 1, 2], [0, 0, 0]), []))
    rows, lat = DD.deform_rows([0, 1, 0], per)
    assert rows.shape == (3, DD.AFFINE_STRIDE) and lat.dtype == np.float64 and lat.size == 2 * 375
    assert rows[:, 7].tolist() == [3.0, 0.0, 3.0] and rows[:, 8].tolist() == [0.0, 0.0, 375.0]
    assert rows[:, 9].tolist() == [5.0, 0.0, 5.0]
    assert rows[0, 20] == DD.BOUNDARY["zeros"] and rows[0, 21] == 1 and rows[1, 21] == 0
    assert np.array_equal(lat[375:], per[2][1][0].lattice.reshape(-1))
    assert np.array_equal(DD.deform_rows([0], [per[1]])[0], DD.fit_rows([0], [per[1]])) and DD.deform_rows([0], [per[1]])[1].size == 0
    for other in (DD.fit_rows, DD.warp_rows):  # a launch without a lattice argument cannot carry the stage
        with pytest.raises(ValueError):
            other([0, 1, 0], per)
    warp = [("zoom", {"min_zoom": 0.7, "max_zoom": 0.7, "prob": 1.0})]
    with pytest.raises(ValueError):
        DD.deform_rows([0], [DD.sample_params(DS.draw_augmentations(warp, np.random.RandomState(0)), shape, warp, ragged=True)])


def test_orderings_and_the_refusals():
    elastic, zoom = ("elastic3d", dict(ELASTIC)), ("zoom", {"min_zoom": 0.7, "max_zoom": 0.7, "prob": 1.0})
    flip, shift = ("flip", {"prob": 1.0}), ("shiftintensity", {"offsets": 0.1, "prob": 1.0})
    affine = ("affine", {"scale_range": (0.1, 0.1, 0.1), "padding_mode": "border", "prob": 1.0})
    noise = ("gaussiannoise", {"std": 0.1, "prob": 1.0})

    def lower(augs, ragged=True):
        return DD.sample_params(DS.draw_augmentations(augs, np.random.RandomState(0)), (9, 14, 11), augs, ragged=ragged)

    _, stages = lower([flip, elastic, shift, noise])  # the MR stage still runs behind the deformation
    assert [type(s).__name__ for s in stages] == ["DeformStage", "IntensityOp", "MRStage"]
    with pytest.raises(NotImplementedError, match="after an affine stage"):
        lower([elastic, flip])
    with pytest.raises(NotImplementedError, match="after an intensity operation"):
        lower([shift, elastic])
    with pytest.raises(NotImplementedError, match="after an MR transform"):
        lower([noise, elastic])
    with pytest.raises(NotImplementedError, match="device pipeline: elastic3d on the example cache"):
        lower([elastic], ragged=False)
    with pytest.raises(ValueError):  # the parameters are checked on the device route's lowering too, drawn or not
        lower([("elastic3d", dict(ELASTIC, control_points=17, prob=0.0))])
    DD.check_ragged_pipeline([flip, elastic, shift, noise])
    for two in ([affine, elastic], [elastic, zoom], [elastic, elastic]):
        with pytest.raises(NotImplementedError, match="two affine stages on cases of unequal shape"):
            DD.check_ragged_pipeline([flip] + two + [shift])
        with pytest.raises(NotImplementedError, match="two affine stages on cases of unequal shape"):
            DD.deform_rows([0], [lower(two)])
    with pytest.raises(NotImplementedError, match="after an affine stage"):
        DD.check_ragged_pipeline([elastic, flip])


def test_the_example_cache_refuses_the_name_before_it_touches_the_device(monkeypatch):
    from mslesions3d_amd import _lib

    def no_device(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(_lib, "load", no_device)
    monkeypatch.setattr(_lib, "call", no_device)

    class _Example:
        class train_dataset:
            augmentations = [("flip", {"prob": 1.0}), ("elastic3d", dict(ELASTIC))]
        n_classes, batch_size = 1, 2

    with pytest.raises(NotImplementedError, match="device pipeline: elastic3d on the example cache"):
        DD.DeviceCache(_Example, "cpu")


# ---- the data set ----------------------------------------------------------------------------------------------------------
TREE = [(40, 44, 50), (52, 48, 46), (44, 70, 52)]


def test_lesion_cases_box_the_deformed_mask(tmp_path):
    data_dir = lesion_tree.make_tree(tmp_path, TREE)
    augs = [("flip", {"spatial_axis": (0, 1, 2), "prob": 0.5}), ("elastic3d", {"control_points": 5, "max_displacement": 4.0,
                                                                                "prob": 1.0})]
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


def test_patches_find_their_lesion_behind_a_deformation(tmp_path):
    data_dir = lesion_tree.make_tree(tmp_path, TREE)
    augs = [("rotate90", {"spatial_axes": (0, 1), "prob": 1.0}), ("elastic3d", {"control_points": 5, "max_displacement": 4.0,
                                                                                "prob": 1.0})]
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
            # the window was aimed at a lesion's centre mapped through the deformation: it holds lesion voxels
            assert DS.window(seg, origin, patch).any(), (epoch, i, origin)
