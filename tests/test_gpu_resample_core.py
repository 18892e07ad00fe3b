"""The six resampling kernels of csrc/datapipe.hip share one sampling core (csrc/resample.hpp): wherever two entry
points of the C ABI are handed the same sampling problem in their own parameters, they return the same bytes, image and
mask.  Each kernel is tested against scipy or its numpy mirror elsewhere; these tests pin the kernels to each other."""
import functools

import numpy as np
import pytest
import torch

from mslesions3d_amd import _lib
from mslesions3d_amd.devicedata import AFFINE_STRIDE, BOUNDARY, OP_ADD, OP_MUL, PARAM_STRIDE

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
IDENT = ((0, 1, 2), (0, 0, 0))
FLIP = ((0, 1, 2), (1, 0, 1))
ROT = ((1, 2, 0), (0, 1, 0))  # keeps the shape of a cube only
OPS = ((OP_ADD, 0.25), (OP_MUL, 1.5))
ZOOM = (0.83, 1.21, 0.64)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a, dtype):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).to(DEV)  # a writable copy


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Two image planes and a mask (values below 256: msl_augment_affine's masks are bytes) of one shape, read-only."""
    rs = np.random.RandomState(sum(shape))
    img = rs.randn(2, *shape).astype(np.float32)
    seg = ((rs.rand(*shape) < 0.4) * rs.randint(1, 200, shape)).astype(np.int16)
    img.setflags(write=False)
    seg.setflags(write=False)
    return img, seg


def _row(perm, on, matrix=None, offset=(0, 0, 0), boundary=0, ops=(), source=0):
    r = np.zeros(AFFINE_STRIDE, dtype=np.float64)
    r[0], r[1:4], r[4:7], r[7] = source, perm[0], perm[1], on
    if matrix is not None:
        r[8:17] = np.asarray(matrix, dtype=np.float64).reshape(9)
    r[17:20], r[20], r[21] = offset, boundary, len(ops)
    for k, (kind, value) in enumerate(ops):
        r[22 + 2 * k], r[23 + 2 * k] = kind, np.float32(value)
    return r


def _fixed(fn, stride, vols, segs, rows):
    """msl_augment_resample / msl_augment_affine on n_src volumes of one shape -> (image (N,) + shape f32, mask int64)."""
    shape, N = vols.shape[1:], len(rows)
    p = _dev(np.stack(rows)[:, :stride], np.float64)
    si, ss = _dev(vols, np.float32), _dev(segs, np.uint8)
    di = torch.empty((N,) + shape, dtype=torch.float32, device=DEV)
    ds = torch.empty((N,) + shape, dtype=torch.uint8, device=DEV)
    _lib.call(fn, si.data_ptr(), ss.data_ptr(), vols.shape[0], p.data_ptr(), N, *shape, di.data_ptr(), ds.data_ptr(),
              _stream())
    return di.cpu().numpy(), ds.cpu().numpy().astype(np.int64)


def _ragged(fn, C, shape, rows, target, windows=None, coords=None):
    """msl_augment_fit_mc / _window_mc / _warp_mc / _deform_mc on an arena that holds ``_case(shape)`` as its single case
    -> (image (N, C) + target f32, mask (N,) + target int64).  ``coords``: the f64 table of the last two (coordinate
    tables / lattices).  The outputs start out non-zero, so a row of zeros was written."""
    img, seg = _case(shape)
    N, target = len(rows), tuple(target)
    ai, asg = _dev(img[:C].reshape(-1), np.float32), _dev(seg.reshape(-1), np.int16)
    table = torch.tensor([[0, *shape]], dtype=torch.int64, device=DEV)
    p = _dev(np.stack(rows), np.float64)
    w = None if windows is None else _dev(np.asarray(windows).reshape(N, 3), np.int32)
    t = None if coords is None else _dev(coords, np.float64)
    di = torch.full((N, C) + target, 7.0, dtype=torch.float32, device=DEV)
    ds = torch.full((N,) + target, 7, dtype=torch.int16, device=DEV)
    args = [ai.data_ptr(), asg.data_ptr(), asg.numel(), C, table.data_ptr(), 1, p.data_ptr()]
    if fn in ("msl_augment_warp_mc", "msl_augment_deform_mc"):
        args += [t.data_ptr(), t.numel()]
    if fn != "msl_augment_fit_mc":
        args.append(None if w is None else w.data_ptr())
    _lib.call(fn, *args, N, *target, di.data_ptr(), ds.data_ptr(), _stream())
    return di.cpu().numpy(), ds.cpu().numpy().astype(np.int64)


def _same(a, b):
    """Byte equality of two (image f32, mask) pairs."""
    assert a[0].dtype == np.float32 and b[0].dtype == np.float32 and a[0].shape == b[0].shape
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), "image bytes differ"
    assert np.array_equal(a[1], b[1]), "mask values differ"


def _rotation(shape):
    """A dense rotation (12 degrees about axis 0, 9 about axis 2) about the volume's centre: every matrix entry but one
    is non-zero, and the corners of the output leave the volume, so every boundary rule has work."""
    a, b = np.deg2rad(12.0), np.deg2rad(9.0)
    r0 = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    r2 = np.array([[np.cos(b), -np.sin(b), 0], [np.sin(b), np.cos(b), 0], [0, 0, 1]])
    m = r0 @ r2
    c = (np.asarray(shape, dtype=np.float64) - 1) / 2
    return m, c - m @ c


def _permuted(shape, perm):
    return tuple(shape[a] for a in perm[0])


def _centred_shift(dims, target):
    return [-((t - n) // 2) if n < t else n // 2 - t // 2 for n, t in zip(dims, target)]


@pytest.mark.parametrize("shape,perms", [((5, 6, 7), (IDENT, FLIP)), ((6, 6, 6), (IDENT, FLIP, ROT)), ((5, 6, 8), (FLIP,))])
def test_resample_is_affine_with_a_diagonal_matrix(shape, perms):
    """msl_augment_resample (zoom, offset) == msl_augment_affine (diag(zoom), that offset, reflect, no operations).  The
    offsets put coordinates below -2 len and above 2 len on some axis of every row, and between on the others: both fold
    branches of the reflect map and its plain branch run."""
    img, seg = _case(shape)
    n = np.asarray(shape, dtype=np.float64)
    offsets = [(-2.6 * n[0] + 0.3, 0.4, 2.2 * n[2] + 0.7), (2.4 * n[0] + 0.1, -2.3 * n[1] - 0.2, -0.6),
               (0.0, 1.3 * n[1] + 0.5, -1.4 * n[2] + 0.25)]
    rows = [_row(perm, 1, np.diag(ZOOM), off, BOUNDARY["reflection"], source=k % 2)
            for k, (perm, off) in enumerate((p, o) for p in perms for o in offsets)]
    rows.append(_row(FLIP, 0, source=1))  # the permuted copy
    res = []
    for r in rows:  # the same row in msl_augment_resample's layout
        q = r[:PARAM_STRIDE].copy()
        q[8:11], q[11:14], q[14:] = ZOOM, r[17:20], 0.0
        res.append(q)
    segs = np.stack([seg, seg[::-1, ::-1, ::-1]])
    _same(_fixed("msl_augment_resample", PARAM_STRIDE, img, segs, res), _fixed("msl_augment_affine", AFFINE_STRIDE, img, segs, rows))


@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("shape,perms", [((5, 7, 6), (IDENT, FLIP)), ((6, 6, 6), (ROT,)), ((5, 6, 8), (IDENT, FLIP))])
def test_affine_is_fit_of_a_single_case_at_its_own_shape(shape, perms, C):
    """msl_augment_affine on a volume == msl_augment_fit_mc with that volume as the arena's single case and target ==
    shape (the fit's shift is 0): a dense rotation under the three boundaries with two intensity operations, and the
    permuted copy.  Every channel of the fit is the affine of its plane."""
    img, seg = _case(shape)
    m, off = _rotation(shape)
    rows = [_row(perm, 1, m, off, b, OPS) for perm in perms for b in sorted(BOUNDARY.values())]
    rows.append(_row(perms[-1], 0, ops=OPS))
    fit = _ragged("msl_augment_fit_mc", C, shape, rows, shape)
    for c in range(C):
        aff = _fixed("msl_augment_affine", AFFINE_STRIDE, img[c:c + 1], seg[None], rows)
        _same((np.ascontiguousarray(fit[0][:, c]), fit[1]), aff)


@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("shape,target", [((5, 6, 7), (4, 5, 6)), ((5, 6, 7), (8, 7, 8)), ((6, 6, 6), (7, 4, 8)),
                                          ((6, 6, 6), (5, 9, 6))])
def test_fit_is_window_at_the_centred_shifts(shape, target, C):
    """msl_augment_fit_mc == msl_augment_window_mc handed the centred fit's own shifts as window origins: targets smaller
    and larger than the case (crop and pad), with and without an affine."""
    m, off = _rotation(shape)
    perms = (IDENT, FLIP, ROT)
    rows = [_row(perm, 1, m, off, b, OPS) for perm, b in zip(perms, sorted(BOUNDARY.values()))]
    rows += [_row(perm, 0, ops=OPS) for perm in perms]
    windows = [_centred_shift(_permuted(shape, perm), target) for perm in perms] * 2
    _same(_ragged("msl_augment_fit_mc", C, shape, rows, target), _ragged("msl_augment_window_mc", C, shape, rows, target, windows))


def _tables(dims, step, start):
    """Per axis t[q] = (0.0 + q * step) + start in f64, in that order: the coordinate row of a diagonal matrix."""
    return np.concatenate([(0.0 + np.arange(n, dtype=np.float64) * s) + o for n, s, o in zip(dims, step, start)])


@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("shape,target", [((5, 6, 7), (6, 5, 6)), ((6, 6, 6), (5, 7, 8))])
def test_warp_by_linear_tables_is_fit_with_a_diagonal_matrix(shape, target, C):
    """msl_augment_warp_mc with tables t_a[q] = (0.0 + q z_a) + off_a == msl_augment_fit_mc with diag(z) and that offset,
    under reflect and constant.  (Under boundary 1 the two differ by design: the warp's rule is scipy's own "nearest".)
    The offsets carry coordinates past both ends of an axis."""
    off = (-1.7, 0.6, 2.3)
    perms = (IDENT, FLIP, ROT)
    bounds = (BOUNDARY["reflection"], BOUNDARY["zeros"])
    fit_rows = [_row(perm, 1, np.diag(ZOOM), off, b, OPS) for perm in perms for b in bounds]
    warp_rows, coords = [], []
    for r, perm in zip(fit_rows, (p for p in perms for _ in bounds)):
        w = r.copy()
        w[7], w[8:17] = 2, 0.0
        w[8] = sum(len(t) for t in coords)
        w[17:20] = 0.0
        warp_rows.append(w)
        coords.append(_tables(_permuted(shape, perm), ZOOM, off))
    _same(_ragged("msl_augment_warp_mc", C, shape, warp_rows, target, coords=np.concatenate(coords)),
          _ragged("msl_augment_fit_mc", C, shape, fit_rows, target))


@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("shape", [(5, 7, 6), (6, 6, 6), (5, 6, 8)])
def test_regrid_is_warp_under_the_unclamped_nearest_rule(shape, C):
    """msl_regrid (identity orientation, output shape == source shape) == msl_augment_warp_mc with boundary 1 and tables
    (0.0 + o step) + start: both sample by scipy's own "nearest".  Steps of 0.5 and 2.5 make half-integer coordinates,
    where the f32 ties sit; the starts carry them past both ends."""
    img, seg = _case(shape)
    for step, start in [((0.5, 2.5, 0.5), (-1.5, 0.5, 1.0)), ((2.5, 0.5, 2.5), (0.5, -2.0, -3.5))]:
        plan = np.ascontiguousarray(np.concatenate([[0, 1, 2], [0, 0, 0], step, start]), dtype=np.float64)
        si, ss = _dev(img[:C], np.float32), _dev(seg, np.int16)
        di = torch.empty((C,) + shape, dtype=torch.float32, device=DEV)
        ds = torch.empty(shape, dtype=torch.int16, device=DEV)
        _lib.call("msl_regrid", si.data_ptr(), ss.data_ptr(), C, *shape, plan.ctypes.data, *shape, di.data_ptr(),
                  ds.data_ptr(), _stream())
        row = _row(IDENT, 2, boundary=BOUNDARY["border"])
        warp = _ragged("msl_augment_warp_mc", C, shape, [row], shape, coords=_tables(shape, step, start))
        _same((di.cpu().numpy()[None], ds.cpu().numpy().astype(np.int64)[None]), warp)


SHAPE_TARGET = [((5, 6, 7), (4, 5, 6)), ((5, 6, 7), (8, 7, 8)), ((6, 6, 6), (4, 5, 6)), ((6, 6, 6), (8, 7, 8))]
OFF_BOTH_ENDS = (-2, 1, 3)  # a window origin: with the larger target it leaves the case at both ends of axis 0


def _identity_tables(dims):
    return np.concatenate([np.arange(n, dtype=np.float64) for n in dims])


@pytest.mark.parametrize("origin", [None, OFF_BOTH_ENDS])
@pytest.mark.parametrize("L", [4, 16])
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("shape,target", SHAPE_TARGET)
def test_deform_with_a_zero_lattice_is_warp_with_identity_tables(shape, target, C, L, origin):
    """msl_augment_deform_mc with a zero lattice (q + d(q) is q exactly) == msl_augment_warp_mc with tables t_a[q] =
    float(q): the three permutations (a ragged case may change shape under one) with two operations under the three
    boundaries, the smallest and the largest lattice, the centred fit and window origins that run off both ends."""
    perms = [perm for perm in (IDENT, FLIP, ROT) for _ in BOUNDARY]
    bounds = sorted(BOUNDARY.values()) * 3
    deform_rows, warp_rows, coords = [], [], []
    for perm, b in zip(perms, bounds):
        d = _row(perm, 3, boundary=b, ops=OPS)
        d[8], d[9] = 0, L  # every sample reads the one zero lattice
        w = _row(perm, 2, boundary=b, ops=OPS)
        w[8] = sum(len(t) for t in coords)
        coords.append(_identity_tables(_permuted(shape, perm)))
        deform_rows.append(d)
        warp_rows.append(w)
    windows = None if origin is None else [origin] * len(perms)
    _same(_ragged("msl_augment_deform_mc", C, shape, deform_rows, target, windows, np.zeros(3 * L ** 3)),
          _ragged("msl_augment_warp_mc", C, shape, warp_rows, target, windows, np.concatenate(coords)))


@pytest.mark.parametrize("origin", [None, OFF_BOTH_ENDS])
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("target", [(4, 5, 6), (8, 7, 8)])
def test_copied_and_rejected_rows_are_the_same_in_every_row_kernel(target, C, origin):
    """The rows warp_kernel and deform_kernel do not sample: a kind-0 row (the permuted copy, with operations) is the fit's (the window's, given origins) byte for byte in both, and a row of a foreign kind, a row
    whose table offset lies past the table and a row whose case is out of range are zeros in both."""
    shape, L = (5, 6, 7), 4
    sides = {"msl_augment_warp_mc": (2, _identity_tables(shape)), "msl_augment_deform_mc": (3, np.zeros(3 * L ** 3))}
    m, off = _rotation(shape)
    windows = None if origin is None else [origin] * 4
    copied, foreign, no_case = _row(FLIP, 0, ops=OPS), _row(IDENT, 1, m, off, BOUNDARY["reflection"]), _row(IDENT, 0, source=1)
    out = {}
    for fn, (kind, side) in sides.items():
        past = _row(IDENT, kind, boundary=BOUNDARY["border"])
        past[8], past[9] = side.size + 5, L
        out[fn] = _ragged(fn, C, shape, [copied, foreign, past, no_case], target, windows, side)
        assert not out[fn][0][1:].view(np.uint32).any() and not out[fn][1][1:].any(), f"{fn}: a rejected row is not zeros"
    # the same batch through the fit (the row past its table left out: the fit has no table and takes any non-zero kind
    # for its affine): only the kind-0 row is comparable
    fit = _ragged("msl_augment_fit_mc" if origin is None else "msl_augment_window_mc", C, shape, [copied, foreign, no_case],
                  target, None if origin is None else windows[:3])
    for o in out.values():
        _same((o[0][:1], o[1][:1]), (fit[0][:1], fit[1][:1]))
