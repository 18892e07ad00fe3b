"""MONAI-free synthetic data path — host-side mirror of the parts of the reference's
``lesions3d/datasets.py:50-95,359-485`` and ``generate_artificial_dataset.py`` that the example pipeline uses.

Same directory layout (``<root>/multiple_objects/one_class/<name>/{images,labels}/sub-XXXX_{image,seg}.*``), same
80/20 split (``train_test_split(random_state=970205)``), same per-sample pipeline (add channel ->
NormalizeIntensity(nonzero=True) -> boxes from connected components of the mask, ``utils.py:450-513``) and the same
batch dict from ``collate_fn`` (``datasets.py:86-94``).  Files are ``.npy`` because nibabel is not installed here
(``.nii.gz`` is read when nibabel is importable).  This is data plumbing in front of the hot path, on the host, as in
the reference; MONAI's exact NormalizeIntensity arithmetic is not pinned (MONAI absent) — population mean/std over
the non-zero voxels is used.
"""
import collections
import itertools
import os
from os.path import join as pjoin

import numpy as np
import torch
from scipy.ndimage import label as cc_label
import zlib

from torch.utils.data import DataLoader, Dataset, Sampler

from .synth import generate_volume, make_case  # noqa: F401


def generate_artificial_dataset(output_dir, dataset_name, num_images=20, image_size=(64, 64, 64), num_objects=(1, 5),
                                object_size=(6, 14), random_seed=0):
    """generate_artificial_dataset.py:63-111 (n_classes = 1, noise on), one file pair per case."""
    root = pjoin(output_dir, "multiple_objects", "one_class", dataset_name)
    os.makedirs(pjoin(root, "images"), exist_ok=True)
    os.makedirs(pjoin(root, "labels"), exist_ok=True)
    for idx in range(num_images):
        data, mask, _ = generate_volume(idx, image_size, num_objects, object_size, random_seed)
        np.save(pjoin(root, "images", f"sub-{str(idx).zfill(4)}_image.npy"), data.astype(np.float32))
        np.save(pjoin(root, "labels", f"sub-{str(idx).zfill(4)}_seg.npy"), mask.astype(np.uint8))
    return root


def boxes_from_segmentation(seg, n_classes=1):
    """BoundingBoxesGeneratord, 'classes' mode (utils.py:450-513): per class, connected components -> inclusive
    [min, max] voxel index per axis / image size; zero-volume boxes dropped."""
    seg = np.squeeze(seg)
    size = np.array(seg.shape * 2, dtype=np.float32)
    boxes, labels = [], []
    for c in range(1, n_classes + 1):
        comp, n = cc_label(seg == c)
        for k in range(1, n + 1):
            idx = np.where(comp == k)
            b = [idx[0].min(), idx[1].min(), idx[2].min(), idx[0].max(), idx[1].max(), idx[2].max()]
            boxes.append(b)
            labels.append(c)
    boxes = torch.from_numpy(np.asarray(boxes, dtype=np.float32).reshape(-1, 6) / size)
    labels = torch.tensor(labels, dtype=torch.long)
    if boxes.numel():
        keep = ((boxes[:, 3] - boxes[:, 0]) * (boxes[:, 4] - boxes[:, 1]) * (boxes[:, 5] - boxes[:, 2])) != 0
        boxes, labels = boxes[keep], labels[keep]
    return boxes, labels


# ---- augmentations (reference train.py:132-145 -> datasets.py:99-122 registry; train pipeline only) -----------------
# The reference applies MONAI's RandFlipd / RandRotate90d / RandAffined to the (image, segmentation) pair BEFORE the boxes
# are extracted, so boxes always follow from the transformed mask.  Same here, on numpy arrays with a channel axis in
# front.  flip / rotate90 are index permutations (exact; MONAI calls the same flip / rot90).  translate / scale are the
# two RandAffined uses: resampling with bilinear (image) / nearest (mask) interpolation and reflection padding.  MONAI is
# absent, so its random-number stream and its affine grid convention are NOT pinned (documented in DESIGN.md); the
# transforms are drawn from ``np.random.RandomState(seed)``.  The same holds for the rotating affine of train_lesions()
# (``rotate_range``: R = Rx Ry Rz about the volume's centre) and for its shiftintensity / scaleintensity.

def _draw_flip(rs, spatial_axis=(0, 1, 2), prob=0.1):
    """The random draws of ``_aug_flip`` -> flipped spatial axes, or None (no flip)."""
    if rs.rand() >= prob:
        return None
    return tuple((spatial_axis,) if np.isscalar(spatial_axis) else spatial_axis)


def _aug_flip(img, seg, rs, spatial_axis=(0, 1, 2), prob=0.1):
    ax = _draw_flip(rs, spatial_axis, prob)
    if ax is None:
        return img, seg
    ax = tuple(a + 1 for a in ax)
    return np.flip(img, ax), np.flip(seg, ax)


def _draw_rotate90(rs, spatial_axes=(0, 1), prob=0.1, max_k=3):
    """The random draws of ``_aug_rotate90`` -> (k, spatial axes), or None."""
    if rs.rand() >= prob:
        return None
    return int(rs.randint(max_k)) + 1, tuple(spatial_axes)


def _aug_rotate90(img, seg, rs, spatial_axes=(0, 1), prob=0.1, max_k=3):
    d = _draw_rotate90(rs, spatial_axes, prob, max_k)
    if d is None:
        return img, seg
    k, ax = d[0], tuple(a + 1 for a in d[1])
    return np.rot90(img, k, ax), np.rot90(seg, k, ax)


def _rand_range(rs, rng, n=3):
    """MONAI's per-axis parameter draw: a (lo, hi) pair draws uniform(lo, hi), a number f draws uniform(-f, f);
    axes beyond the given entries get 0."""
    out = []
    for f in tuple(rng)[:n]:
        out.append(rs.uniform(f[0], f[1]) if isinstance(f, (tuple, list)) else rs.uniform(-f, f))
    return out + [0.0] * (n - len(out))


def _draw_affine(rs, mode=("bilinear", "nearest"), translate_range=None, scale_range=None, padding_mode="reflection",
                 prob=0.1, rotate_range=None):
    """The random draws of ``_aug_affine`` -> (zoom, shift) per spatial axis, or None.  With a ``rotate_range`` the
    angles are drawn first (then translate, then scale) and the result is (zoom, shift, angles)."""
    if rs.rand() >= prob:
        return None
    angles = _rand_range(rs, rotate_range) if rotate_range is not None else None
    shift = _rand_range(rs, translate_range) if translate_range is not None else [0.0] * 3
    zoom = [1.0 + v for v in _rand_range(rs, scale_range)] if scale_range is not None else [1.0] * 3
    return (zoom, shift) if angles is None else (zoom, shift, angles)


def affine_offset(shape, zoom, shift):
    """Output voxel o of ``_aug_affine`` samples input voxel diag(zoom) o + offset (f64, the host's arithmetic)."""
    centre = (np.array(shape, dtype=np.float64) - 1) / 2
    return centre - np.diag(zoom) @ centre + np.array(shift, dtype=np.float64)


def rotation_matrix(angles):
    """R = Rx(a0) Ry(a1) Rz(a2): rotations about array axes 0, 1, 2 (f64)."""
    c, s = np.cos(np.asarray(angles, dtype=np.float64)), np.sin(np.asarray(angles, dtype=np.float64))
    rx = np.array([[1.0, 0.0, 0.0], [0.0, c[0], -s[0]], [0.0, s[0], c[0]]])
    ry = np.array([[c[1], 0.0, s[1]], [0.0, 1.0, 0.0], [-s[1], 0.0, c[1]]])
    rz = np.array([[c[2], -s[2], 0.0], [s[2], c[2], 0.0], [0.0, 0.0, 1.0]])
    return rx @ ry @ rz


def affine_matrix(shape, zoom, shift, angles=None):
    """-> (M, offset): output voxel o of ``_aug_affine`` samples input position M o + offset, which is
    centre + R diag(zoom) (o - centre) + shift with centre = (shape - 1) / 2.  Without angles M is diag(zoom) and the
    offset is ``affine_offset``'s, bit for bit."""
    if angles is None:
        return np.diag(zoom), affine_offset(shape, zoom, shift)
    centre = (np.array(shape, dtype=np.float64) - 1) / 2
    mat = rotation_matrix(angles) @ np.diag(np.asarray(zoom, dtype=np.float64))
    return mat, centre - mat @ centre + np.array(shift, dtype=np.float64)


SCIPY_BOUNDARY = {"reflection": "reflect", "border": "nearest", "zeros": "constant"}


def _aug_affine(img, seg, rs, mode=("bilinear", "nearest"), translate_range=None, scale_range=None,
                padding_mode="reflection", prob=0.1, rotate_range=None):
    from scipy.ndimage import affine_transform
    d = _draw_affine(rs, mode, translate_range, scale_range, padding_mode, prob, rotate_range)
    if d is None:
        return img, seg
    pad = SCIPY_BOUNDARY[padding_mode]
    mat, off = affine_matrix(img.shape[1:], *d)  # output voxel o samples input voxel M o + off
    outs = []
    for a, m in ((img, mode[0]), (seg, mode[1])):
        order = 1 if m == "bilinear" else 0
        outs.append(np.stack([affine_transform(c.astype(np.float32), mat, offset=off, order=order, mode=pad) for c in a]).astype(a.dtype))
    return outs[0], outs[1]


# RandShiftIntensityd / RandScaleIntensityd: image only, one f32 operation; zeros do not stay zero (as in MONAI)
def _draw_intensity(rs, rng, prob):
    if rs.rand() >= prob:
        return None
    return float(rs.uniform(rng[0], rng[1]) if isinstance(rng, (tuple, list)) else rs.uniform(-rng, rng))


def _draw_shiftintensity(rs, offsets=0.1, prob=0.1):
    """The random draws of ``_aug_shiftintensity`` -> the offset (f64), or None."""
    return _draw_intensity(rs, offsets, prob)


def _aug_shiftintensity(img, seg, rs, offsets=0.1, prob=0.1):
    off = _draw_shiftintensity(rs, offsets, prob)
    return (img, seg) if off is None else (img + np.float32(off), seg)


def _draw_scaleintensity(rs, factors=0.1, prob=0.1):
    """The random draws of ``_aug_scaleintensity`` -> the factor f of img * (1 + f) (f64), or None."""
    return _draw_intensity(rs, factors, prob)


def _aug_scaleintensity(img, seg, rs, factors=0.1, prob=0.1):
    f = _draw_scaleintensity(rs, factors, prob)
    return (img, seg) if f is None else (img * np.float32(1.0 + f), seg)


# RandZoomd / RandGridDistortiond (the registry's 'zoom' / 'griddistortion'): separable warps.  A warp of a (n0, n1, n2)
# volume is three f64 tables t_a of length n_a; output voxel o samples the input at (t_0[o_0], t_1[o_1], t_2[o_2]) with
# bilinear (image) / nearest (mask) interpolation.  MONAI is absent: the tables below are this project's contract,
# restated from memory and NOT pinned.

def zoom_table(n, z):
    """RandZoom(keep_size=True) on one axis of n voxels: t[o] = (o - c) / z + c about the centre c = (n - 1) / 2, each
    operation one rounded f64 operation; z > 1 magnifies."""
    c = (n - 1) / 2
    return (np.arange(n, dtype=np.float64) - c) / float(z) + c


def grid_table(n, num_cells, steps):
    """RandGridDistortion on one axis of n voxels: ``steps`` holds num_cells + 1 positive f64 values.  With cell =
    max(n // num_cells, 1) and prev = 0.0, segments s = 0, 1, ... run while start = s * cell < n, with end =
    min(start + cell, n): cur = float(n) where start + cell > n, else prev + cell * steps[min(s, num_cells)];
    t[start:end] = np.linspace(prev, cur, end - start); prev = cur.  Every index is written (on a short axis too, where
    MONAI's rule would leave a tail) and the last coordinate of a segment is the first of the next one.  The table is
    non-decreasing on an axis without a remainder segment (n % cell == 0) and, with one, as long as the full segments end
    at or below n; where they end beyond n the remainder segment runs backwards to n (MONAI's rule does the same, and
    the rule is kept as it is: the resampling takes any table, only ``centres_to_augmented`` assumes a sorted one)."""
    n, num_cells = int(n), int(num_cells)
    steps = np.asarray(steps, dtype=np.float64).reshape(-1)
    if n < 1 or num_cells < 1 or steps.size != num_cells + 1 or not (steps > 0).all():
        raise ValueError(f"grid_table: n >= 1, num_cells >= 1 and num_cells + 1 positive steps expected, got {n}, "
                         f"{num_cells}, {steps.tolist()}")
    cell = max(n // num_cells, 1)
    t = np.empty(n, dtype=np.float64)
    prev, s = 0.0, 0
    while s * cell < n:
        start = s * cell
        end = min(start + cell, n)
        cur = float(n) if start + cell > n else prev + cell * steps[min(s, num_cells)]
        t[start:end] = np.linspace(prev, cur, end - start)
        prev = cur
        s += 1
    return t


def _draw_zoom(rs, min_zoom=0.9, max_zoom=1.1, mode=("bilinear", "nearest"), padding_mode="border", prob=0.1):
    """The random draws of ``_aug_zoom`` -> the zoom factor (f64, one for all axes), or None."""
    if rs.rand() >= prob:
        return None
    return float(rs.uniform(min_zoom, max_zoom))


def _draw_griddistortion(rs, num_cells=5, distort_limit=(-0.03, 0.03), mode=("bilinear", "nearest"),
                         padding_mode="border", prob=0.1):
    """The random draws of ``_aug_griddistortion`` -> the steps of axes 0, 1, 2 (three f64 arrays of num_cells + 1
    values, 1 + uniform(lo, hi)), or None.  A number f as ``distort_limit`` means (-f, f)."""
    lo, hi = distort_limit if isinstance(distort_limit, (tuple, list)) else (-distort_limit, distort_limit)
    if abs(lo) >= 1 or abs(hi) >= 1:
        raise ValueError(f"griddistortion: |distort_limit| must stay below 1 (steps are positive), got {distort_limit}")
    if rs.rand() >= prob:
        return None
    return tuple(1.0 + rs.uniform(lo, hi, num_cells + 1) for _ in range(3))


def _warp(img, seg, tables, mode, padding_mode):
    """The (image, mask) pair sampled at ``np.meshgrid(t0, t1, t2, indexing="ij")``: per channel
    ``scipy.ndimage.map_coordinates`` of the f32 channel, order 1 (bilinear) / 0 (nearest), cast back as ``_aug_affine``
    casts."""
    return _sample_at(img, seg, np.meshgrid(*tables, indexing="ij"), mode, padding_mode)


def _sample_at(img, seg, coords, mode, padding_mode):
    """The (image, mask) pair sampled at three dense f64 coordinate arrays, as ``_warp`` states it."""
    from scipy.ndimage import map_coordinates
    pad = SCIPY_BOUNDARY[padding_mode]
    outs = []
    for a, m in ((img, mode[0]), (seg, mode[1])):
        order = 1 if m == "bilinear" else 0
        outs.append(np.stack([map_coordinates(c.astype(np.float32), coords, order=order, mode=pad) for c in a]).astype(a.dtype))
    return outs[0], outs[1]


def _aug_zoom(img, seg, rs, min_zoom=0.9, max_zoom=1.1, mode=("bilinear", "nearest"), padding_mode="border", prob=0.1):
    z = _draw_zoom(rs, min_zoom, max_zoom, mode, padding_mode, prob)
    if z is None:
        return img, seg
    return _warp(img, seg, [zoom_table(n, z) for n in img.shape[1:]], mode, padding_mode)


def _aug_griddistortion(img, seg, rs, num_cells=5, distort_limit=(-0.03, 0.03), mode=("bilinear", "nearest"),
                        padding_mode="border", prob=0.1):
    steps = _draw_griddistortion(rs, num_cells, distort_limit, mode, padding_mode, prob)
    if steps is None:
        return img, seg
    return _warp(img, seg, [grid_table(n, num_cells, s) for n, s in zip(img.shape[1:], steps)], mode, padding_mode)


def warp_tables(name, draw, shape, kw):
    """The three tables of a drawn 'zoom' / 'griddistortion' (``DRAWS[name]``'s result) on a volume of ``shape``."""
    if name == "zoom":
        return [zoom_table(n, draw) for n in shape]
    return [grid_table(n, kw.get("num_cells", 5), s) for n, s in zip(shape, draw)]


# Rand3DElasticd / RandomElasticDeformation ('elastic3d'): a dense, smooth, non-rigid deformation (DESIGN.md section
# 4.15).  MONAI and TorchIO are absent: the contract below is this project's own and its parity is NOT pinned.  A lattice
# P of (3, L, L, L) f64 coefficients spans the volume with one control point of margin at either end; output voxel q
# samples the input at q + d(q), d_m the cubic B-spline of P[m].  Every operation is one rounded f64 operation in a fixed
# order, so that msl_augment_deform_mc (csrc/datapipe.hip) forms the same coordinates.

DEFORM_POINTS = (4, 16)  # control points per axis: a cubic needs four, the kernel's row buffer holds sixteen


def _check_elastic3d(control_points, max_displacement):
    lo, hi = DEFORM_POINTS
    if int(control_points) != control_points or not lo <= control_points <= hi:
        raise ValueError(f"elastic3d: control_points must be one of {lo} .. {hi}, got {control_points}")
    if not (np.isfinite(max_displacement) and max_displacement > 0):
        raise ValueError(f"elastic3d: max_displacement must be positive and finite, got {max_displacement}")


def _draw_elastic3d(rs, control_points=7, max_displacement=7.5, mode=("bilinear", "nearest"), padding_mode="border",
                    prob=0.1):
    """The random draws of ``_aug_elastic3d`` -> uniform(-1, 1) of shape (3, L, L, L) (f64), or None."""
    _check_elastic3d(control_points, max_displacement)
    if rs.rand() >= prob:
        return None
    L = int(control_points)
    return rs.uniform(-1.0, 1.0, (3, L, L, L))


def deform_lattice(shape, draw, max_displacement):
    """A draw of ``_draw_elastic3d`` on a volume of ``shape`` -> the lattice P = draw * A (f64, (3, L, L, L); component m
    displaces along axis m).  A = min(max_displacement, min_a spacing_a / 4) with spacing_a = (n_a - 1) / (L - 3) over
    the axes of two voxels or more; an axis of one voxel has its component zeroed, and A = 0 without any other axis.
    The cap keeps the map q -> q + d(q) from folding: a cubic B-spline of coefficients bounded by A has derivatives
    bounded by A / spacing <= 1 / 4 per axis (sup_t sum_i |B_i'(t)| = 1), so the gradient of d has norm below 1."""
    draw = np.asarray(draw, dtype=np.float64)
    shape = tuple(int(n) for n in shape)
    if draw.ndim != 4 or draw.shape[0] != 3 or len(set(draw.shape[1:])) != 1 or len(shape) != 3 or min(shape) < 1:
        raise ValueError(f"deform_lattice: a (3, L, L, L) draw and three positive sizes expected, got {draw.shape}, {shape}")
    L = draw.shape[1]
    _check_elastic3d(L, max_displacement)
    spacing = [(n - 1) / (L - 3) for n in shape if n >= 2]
    A = min(float(max_displacement), min(spacing) / 4) if spacing else 0.0
    P = draw * A
    for m, n in enumerate(shape):
        if n == 1:
            P[m] = 0.0
    return P


def _spline_taps(q, n, L):
    """One axis of the deformation's contract at the positions ``q`` (f64 array; whole voxels or not) of an axis of n
    voxels -> (cell, [b0, b1, b2, b3]): u = q * (L - 3) / (n - 1) (the product first; 0.0 where n == 1), cell =
    min(floor(u), L - 4) (and at least 0), t = u - cell (1.0 exactly at the last voxel), then the four cubic B-spline
    weights, operation by operation as written."""
    q = np.asarray(q, dtype=np.float64)
    u = q * float(L - 3) / float(n - 1) if n > 1 else np.zeros_like(q)
    cell = np.clip(np.floor(u), 0, L - 4).astype(np.int64)
    t = u - cell
    t2 = t * t
    t3 = t2 * t
    s = 1.0 - t
    return cell, [((s * s) * s) / 6.0,
                  (((3.0 * t3) - (6.0 * t2)) + 4.0) / 6.0,
                  ((((-3.0 * t3) + (3.0 * t2)) + (3.0 * t)) + 1.0) / 6.0,
                  t3 / 6.0]


def deform_coords(shape, P):
    """-> the three f64 coordinate arrays of ``shape``: voxel q samples at c_m = q_m + d_m(q) with, per component m,
    R_m[k2] = sum_j b1[j] * (sum_i b0[i] * P[m][cell0 + i][cell1 + j][k2]) (a function of the row (q_0, q_1) alone) and
    d_m = sum_k b2[k] * R_m[cell2 + k]; every sum starts at 0.0 and ascends, each term as sum = sum + (weight * value)."""
    P = np.asarray(P, dtype=np.float64)
    shape = tuple(int(n) for n in shape)
    L = P.shape[1]
    (c0, b0), (c1, b1), (c2, b2) = [_spline_taps(np.arange(n), n, L) for n in shape]
    out = []
    for m in range(3):
        R = np.zeros((shape[0], shape[1], L))
        for j in range(4):
            inner = np.zeros((shape[0], shape[1], L))
            for i in range(4):
                inner = inner + b0[i][:, None, None] * P[m][c0 + i][:, c1 + j, :]
            R = R + b1[j][None, :, None] * inner
        d = np.zeros(shape)
        for k in range(4):
            d = d + b2[k][None, None, :] * R[:, :, c2 + k]
        out.append(np.arange(shape[m], dtype=np.float64).reshape([-1 if a == m else 1 for a in range(3)]) + d)
    return out


def deform_displacement(shape, P, q):
    """d(q) (K, 3) f64 at the positions ``q`` (K, 3) f64 of a volume of ``shape``, whole voxels or not: the spline of
    ``deform_coords`` in the same nesting (at whole voxels, its values)."""
    P = np.asarray(P, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64).reshape(-1, 3)
    L = P.shape[1]
    (c0, b0), (c1, b1), (c2, b2) = [_spline_taps(q[:, a], shape[a], L) for a in range(3)]
    d = np.zeros_like(q)
    for m in range(3):
        for k in range(4):
            R = np.zeros(q.shape[0])
            for j in range(4):
                inner = np.zeros(q.shape[0])
                for i in range(4):
                    inner = inner + b0[i] * P[m][c0 + i, c1 + j, c2 + k]
                R = R + b1[j] * inner
            d[:, m] = d[:, m] + b2[k] * R
    return d


def _aug_elastic3d(img, seg, rs, control_points=7, max_displacement=7.5, mode=("bilinear", "nearest"),
                   padding_mode="border", prob=0.1):
    d = _draw_elastic3d(rs, control_points, max_displacement, mode, padding_mode, prob)
    if d is None:
        return img, seg
    shape = img.shape[1:]
    return _sample_at(img, seg, deform_coords(shape, deform_lattice(shape, d, max_displacement)), mode, padding_mode)


# RandGaussianSmoothd / RandBiasFieldd / RandGaussianNoised (the MR stage): resolution loss, coil
# inhomogeneity and thermal noise, on the image only.  MONAI is absent: parameter names and default ranges follow it as
# remembered, the arithmetic below is this project's contract and its parity is NOT pinned.  Every operation is exact
# integer arithmetic, an f64 sum of exact products in a fixed order or one rounded f32 operation, so that msl_augment_mr
# (csrc/mraug.hip) computes the same bits.  All channels of a sample share one blur and one bias field; the noise differs
# per channel.  The three act on the FINISHED sample: ``_LesionCases`` draws them in list order and applies them behind
# its fit / window, where the device route applies them to the built batch.

MR_MAX_RADIUS = 8  # taps reach 4 sigma: sigma <= 2.0
PHILOX_M0, PHILOX_M1, PHILOX_W0, PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
# the eight 16-bit halves of a Philox block are uniform on 0 .. 65535: mean 32767.5, variance (2^32 - 1) / 12 each
NOISE_MEAN = 262140
NOISE_SCALE = np.float32(1.0 / np.sqrt(8.0 * (2.0 ** 32 - 1.0) / 12.0))


def gaussian_radius(sigma):
    """R = int(4 sigma + 0.5); a sigma outside (0, 2.0] (R > 8) raises ValueError."""
    sigma = float(sigma)
    if not 0.0 < sigma <= 2.0:
        raise ValueError(f"gaussiansmooth: sigma must lie in (0, 2.0] (a radius of at most {MR_MAX_RADIUS}), got {sigma}")
    return int(4.0 * sigma + 0.5)


def gaussian_taps(sigma):
    """-> the 2R + 1 f32 taps of one axis: e[k] = exp(-k^2 / (2 sigma^2)) in f64 for k = -R .. R, divided by their sum
    (accumulated one after the other in ascending k) and rounded to f32."""
    R = gaussian_radius(sigma)
    k = np.arange(-R, R + 1, dtype=np.float64)
    e = np.exp(-(k * k) / (2.0 * float(sigma) * float(sigma)))
    s = 0.0
    for v in e:
        s += float(v)
    return (e / s).astype(np.float32)


def blur_axis(vol, taps, axis):
    """One pass of the blur over ``axis`` of an f32 array: acc = 0.0 (f64); for k ascending acc += f64(w[k]) *
    f64(v[i + k - R]), a tap outside the axis contributing nothing; the result rounded to f32 once."""
    vol = np.asarray(vol, dtype=np.float32)
    taps = np.asarray(taps, dtype=np.float32)
    R, n = (taps.size - 1) // 2, vol.shape[axis]
    pad = [(0, 0)] * vol.ndim
    pad[axis] = (R, R)
    padded = np.pad(vol.astype(np.float64), pad)  # (a zero product adds +0.0, which changes no partial sum)
    acc = np.zeros(vol.shape, dtype=np.float64)
    for k in range(taps.size):
        sl = [slice(None)] * vol.ndim
        sl[axis] = slice(k, k + n)
        acc = acc + np.float64(taps[k]) * padded[tuple(sl)]
    return acc.astype(np.float32)


def gaussian_smooth(img, sigmas):
    """The blur of a (C, D, H, W) f32 image: three passes, over axis 0, then 1, then 2 of every channel, each rounding
    to f32 once."""
    for a, s in enumerate(sigmas):
        img = blur_axis(img, gaussian_taps(s), a + 1)
    return img


def bias_terms(degree):
    """The exponents (i, j, k) with i + j + k <= degree in the order their coefficients are drawn: lexicographic, i
    slowest."""
    degree = int(degree)
    return [(i, j, k) for i in range(degree + 1) for j in range(degree + 1 - i) for k in range(degree + 1 - i - j)]


def _legendre(degree, u):
    """P_0 .. P_degree at the f64 points u by the recurrence (m + 1) P_{m+1} = (2m + 1) u P_m - m P_{m-1}."""
    u = np.asarray(u, dtype=np.float64)
    P = [np.ones_like(u), u]
    for m in range(1, degree):
        P.append(((2 * m + 1) * u * P[m] - m * P[m - 1]) / (m + 1))
    return P[:degree + 1]


def bias_polynomial(coeffs, degree, u0, u1, u2):
    """sum c_ijk P_i(u0) P_j(u1) P_k(u2) on the grid u0 x u1 x u2 in f64: the terms in ``bias_terms`` order, each
    ((c P_i) P_j) P_k, added one after the other from 0.0."""
    terms = bias_terms(degree)
    coeffs = np.asarray(coeffs, dtype=np.float64).reshape(-1)
    if coeffs.size != len(terms):
        raise ValueError(f"biasfield: degree {degree} takes {len(terms)} coefficients, got {coeffs.size}")
    P0, P1, P2 = (_legendre(int(degree), u) for u in (u0, u1, u2))
    s = np.zeros((len(P0[0]), len(P1[0]), len(P2[0])), dtype=np.float64)
    for c, (i, j, k) in zip(coeffs, terms):
        s = s + ((c * P0[i])[:, None, None] * P1[j][None, :, None]) * P2[k][None, None, :]
    return s


def bias_lattice(coeffs, degree=3, lattice=9):
    """-> (L, L, L) f32: F = exp(``bias_polynomial``) at the lattice points u_j = -1 + 2 j / (L - 1) of every axis,
    rounded to f32."""
    L = int(lattice)
    if L < 2:
        raise ValueError(f"biasfield: a lattice of at least 2 points per axis, got {lattice}")
    u = -1.0 + 2.0 * np.arange(L, dtype=np.float64) / (L - 1)
    return np.exp(bias_polynomial(coeffs, degree, u, u, u)).astype(np.float32)


def bias_field(lattice, shape):
    """The (L, L, L) f32 lattice sampled on a volume of ``shape`` -> f32 field.  Output voxel o samples at x_a = o_a *
    (L - 1) / (n_a - 1) in f64 (0 where n_a == 1) with the trilinear arithmetic of ``devicedata.affine_numpy`` /
    csrc/resample.hpp: taps floor(x), floor(x) + 1 clamped to L - 1, weights w0 = 1 - (x - floor(x)), w1 = 1 - w0, the
    eight corners accumulated axis 0 slowest, each ((F w_0) w_1) w_2; the sum rounded to f32."""
    F = np.asarray(lattice, dtype=np.float32).astype(np.float64)
    L = F.shape[0]
    idx, w = [], []
    for n in shape:
        o = np.arange(int(n), dtype=np.float64)
        x = o * (L - 1) / (n - 1) if n > 1 else np.zeros(int(n))
        fl = np.floor(x)
        w0 = 1.0 - (x - fl)
        w.append((w0, 1.0 - w0))
        idx.append((np.minimum(fl, L - 1).astype(np.int64), np.minimum(fl + 1, L - 1).astype(np.int64)))
    t = np.zeros(tuple(int(n) for n in shape), dtype=np.float64)
    for a in range(2):
        for b in range(2):
            for d in range(2):
                coeff = F[idx[0][a][:, None, None], idx[1][b][None, :, None], idx[2][d][None, None, :]]
                coeff = coeff * w[0][a][:, None, None]
                coeff = coeff * w[1][b][None, :, None]
                coeff = coeff * w[2][d][None, None, :]
                t = t + coeff
    return t.astype(np.float32)


def philox4x32(counter, key, rounds=10):
    """Philox4x32-10 (Salmon et al., Random123) in numpy uint64: ``counter`` four and ``key`` two 32-bit words (arrays
    broadcast against each other) -> the four output words as uint64 arrays holding 32-bit values."""
    mask = np.uint64(0xFFFFFFFF)
    c = [np.asarray(v, dtype=np.uint64) & mask for v in counter]
    k = [np.asarray(v, dtype=np.uint64) & mask for v in key]
    for r in range(rounds):
        if r:
            k = [(k[0] + np.uint64(PHILOX_W0)) & mask, (k[1] + np.uint64(PHILOX_W1)) & mask]
        p0, p1 = np.uint64(PHILOX_M0) * c[0], np.uint64(PHILOX_M1) * c[2]  # 32 x 32 bits: no overflow in 64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & mask]
    return c


def philox_normal(index, channel, k0, k1):
    """The eight-term Irwin-Hall normal of voxel ``index`` (the spatial linear index) and ``channel``: the Philox block
    of counter (index, channel, 0, 0) under key (k0, k1), its four words split into eight 16-bit halves with sum S;
    z = f32(S - 262140) * f32(1 / sqrt(8 (2^32 - 1) / 12)), one f32 multiply.  Mean 0, variance 1, tails end at
    +-4.9."""
    words = philox4x32((index, channel, 0, 0), (k0, k1))
    S = np.zeros(np.broadcast(*words).shape, dtype=np.int64)
    for wd in words:
        S = S + (wd & np.uint64(0xFFFF)).astype(np.int64) + (wd >> np.uint64(16)).astype(np.int64)
    return (S - NOISE_MEAN).astype(np.float32) * NOISE_SCALE


def gaussian_noise(img, std, k0, k1):
    """(C, D, H, W) f32 image + noise: n = z * f32(std) with z = ``philox_normal`` of (d H W + h W + w, channel), then
    v + n: three separately rounded f32 operations.  D H W >= 2^32 raises ValueError."""
    img = np.asarray(img, dtype=np.float32)
    V = int(np.prod(img.shape[1:]))
    if V >= 2 ** 32:
        raise ValueError(f"gaussiannoise: {V} voxels per channel do not fit the 32-bit counter word")
    index = np.arange(V, dtype=np.uint64).reshape(img.shape[1:])
    out = np.empty_like(img)
    for c in range(img.shape[0]):
        out[c] = img[c] + philox_normal(index, c, k0, k1) * np.float32(std)
    return out


def _draw_gaussiansmooth(rs, sigma=(0.25, 1.5), prob=0.1):
    """The random draws of ``_aug_gaussiansmooth`` -> the sigmas of axes 0, 1, 2 (f64), or None."""
    if rs.rand() >= prob:
        return None
    return tuple(float(rs.uniform(sigma[0], sigma[1])) for _ in range(3))


def _draw_biasfield(rs, degree=3, coeff_range=(0.0, 0.1), lattice=9, prob=0.1):
    """The random draws of ``_aug_biasfield`` -> the f64 coefficients in ``bias_terms`` order, or None."""
    if rs.rand() >= prob:
        return None
    return rs.uniform(coeff_range[0], coeff_range[1], len(bias_terms(degree)))


def _draw_gaussiannoise(rs, std=0.1, prob=0.1):
    """The random draws of ``_aug_gaussiannoise`` -> (std f64, k0, k1), or None."""
    if rs.rand() >= prob:
        return None
    s = float(rs.uniform(0, std))
    k0, k1 = rs.randint(0, 2 ** 32, 2, dtype=np.uint32)
    return s, int(k0), int(k1)


def apply_mr(name, img, draw, kw):
    """A drawn MR transform (``DRAWS[name]``'s result, None: not drawn) on a (C, D, H, W) f32 image."""
    if draw is None:
        return img
    if name == "gaussiansmooth":
        return gaussian_smooth(img, draw)
    if name == "biasfield":
        field = bias_field(bias_lattice(draw, kw.get("degree", 3), kw.get("lattice", 9)), img.shape[1:])
        return np.asarray(img, dtype=np.float32) * field[None]  # one f32 multiply
    if name == "gaussiannoise":
        return gaussian_noise(img, *draw)
    raise ValueError(f"not an MR transform: {name!r}")


def _aug_gaussiansmooth(img, seg, rs, **kw):
    return apply_mr("gaussiansmooth", img, _draw_gaussiansmooth(rs, **kw), kw), seg


def _aug_biasfield(img, seg, rs, **kw):
    return apply_mr("biasfield", img, _draw_biasfield(rs, **kw), kw), seg


def _aug_gaussiannoise(img, seg, rs, **kw):
    return apply_mr("gaussiannoise", img, _draw_gaussiannoise(rs, **kw), kw), seg


# ---- lesionpaste: copy-paste of cached lesions on to the finished sample -----------------------
# The draws are a fixed number of uniforms; ``lower_pastes`` turns them into integer rows before anything touches a voxel,
# and ``paste_lesions`` applies the rows: integer arithmetic throughout, apart from the rim blend (two rounded f32 products
# and one rounded sum), so that msl_paste_lesions (csrc/lesionpaste.hip) computes the same bits.
PASTE_NAME = "lesionpaste"
PASTE_MAX_EXTENT = 32      # voxels per axis of a donor lesion's box
PASTE_MAX_LESIONS = 8      # pastes per sample one msl_paste_lesions launch walks
PASTE_MAX_CANDIDATES = 16  # destination candidates per paste
PASTE_HEAD = 13            # ints of a paste row in front of its candidates
PASTE_MAX_VALUE = 32767    # the mask is int16 on the device: msl_instance_boxes labels ids 1 .. 32767

# rows (R, 8) int64: [case, label, min0..2, max0..2] (inclusive extents in the cropped case; ``case`` counts the training
# cases in ``train_dataset.subjects`` order); max_ids (n_cases, n_classes) int64: per case and class the largest id
# present, lo - 1 where the class holds none (instances mode; unused in binary mode); shapes: the cropped shapes
LesionBank = collections.namedtuple("LesionBank", "rows max_ids shapes")


def check_lesionpaste(prob=0.5, max_lesions=4, candidates=8, max_volume=None):
    """The keyword limits of ``lesionpaste``: ValueError."""
    if not 1 <= int(max_lesions) <= PASTE_MAX_LESIONS or int(max_lesions) != max_lesions:
        raise ValueError(f"lesionpaste: max_lesions of 1 .. {PASTE_MAX_LESIONS}, got {max_lesions}")
    if not 1 <= int(candidates) <= PASTE_MAX_CANDIDATES or int(candidates) != candidates:
        raise ValueError(f"lesionpaste: candidates of 1 .. {PASTE_MAX_CANDIDATES}, got {candidates}")
    if max_volume is not None and not max_volume > 0:
        raise ValueError(f"lesionpaste: max_volume is a number of voxels > 0 or None, got {max_volume}")


def paste_draw_count(max_lesions=4, candidates=8):
    return 2 + int(max_lesions) * (4 + 3 * int(candidates))


def _draw_lesionpaste(rs, prob=0.5, max_lesions=4, candidates=8, max_volume=None):
    """The random draws of ``lesionpaste``: always ``paste_draw_count`` uniforms in ONE ``rs.random_sample`` call,
    whatever they say and whatever the bank holds - [0] apply (u < prob), [1] the count K = 1 + floor(u max_lesions),
    then per paste k < max_lesions: the donor, three flip bits (u >= 0.5 mirrors the axis) and ``candidates`` triples.
    -> None (not applied) or K tuples (donor u, (f0, f1, f2), (candidates, 3) f64)."""
    check_lesionpaste(prob, max_lesions, candidates, max_volume)
    u = rs.random_sample(paste_draw_count(max_lesions, candidates))
    if u[0] >= prob:
        return None
    K = min(1 + int(np.floor(u[1] * max_lesions)), int(max_lesions))
    per = u[2:].reshape(int(max_lesions), 4 + 3 * int(candidates))
    return [(float(r[0]), tuple(int(v >= 0.5) for v in r[1:4]), r[4:].reshape(int(candidates), 3).copy()) for r in per[:K]]


def _aug_lesionpaste(img, seg, rs, **kw):
    raise NotImplementedError("lesionpaste pastes lesions of a LesionsDataModule's bank on to the finished sample: it runs "
                              "inside _LesionCases._sample / LesionCache, not as a transform of its own (-dm lesions)")


def class_max_ids(seg, thresholds, mode):
    """Per class the largest id of a mask inside the class's threshold pair [lo, hi), lo - 1 where it holds none; zeros
    in binary mode (unused there).  -> list of ints."""
    if mode == "binary":
        return [0] * len(thresholds)
    seg = np.asarray(seg)
    out = []
    for lo, hi in thresholds:
        inside = seg[(seg >= lo) & (seg < hi)]
        out.append(int(inside.max()) if inside.size else int(lo) - 1)
    return out


def bank_from_lesions(per_case, max_volume=None):
    """``per_case``: per training case (extents (K, 6) ints [min..., max...] of the boxes its box stage keeps, labels (K,),
    the cropped shape, ``class_max_ids``) -> ``LesionBank``.  A lesion enters when every extent e_a = max_a - min_a + 1 is
    at most PASTE_MAX_EXTENT, its box dilated by one voxel and clamped to the case intersects the box of no other kept
    lesion of the case, and its bounding-box volume prod(max_a - min_a) - the measure of ``eval --size_bins`` - is at
    most ``max_volume`` (None: no limit)."""
    rows, max_ids, shapes = [], [], []
    for case, (extents, labels, shape, ids) in enumerate(per_case):
        ext = np.asarray(extents, dtype=np.int64).reshape(-1, 6)
        shapes.append(tuple(int(n) for n in shape))
        max_ids.append([int(v) for v in ids])
        for k in range(ext.shape[0]):
            lo, hi = ext[k, :3], ext[k, 3:]
            if (hi - lo + 1).max() > PASTE_MAX_EXTENT:
                continue
            if max_volume is not None and int(np.prod(hi - lo)) > max_volume:
                continue
            dlo, dhi = np.maximum(lo - 1, 0), np.minimum(hi + 1, np.asarray(shape) - 1)
            others = np.delete(ext, k, axis=0)
            if ((others[:, :3] <= dhi) & (others[:, 3:] >= dlo)).all(1).any():
                continue
            rows.append([case, int(labels[k]), *lo.tolist(), *hi.tolist()])
    return LesionBank(np.asarray(rows, dtype=np.int64).reshape(-1, 8), np.asarray(max_ids, dtype=np.int64).reshape(len(shapes), -1),
                      shapes)


def lower_pastes(draw, bank, case, target, thresholds, mode, max_lesions, candidates):
    """One sample's ``_draw_lesionpaste`` result -> (max_lesions, PASTE_HEAD + 3 candidates) int32 rows, the layout of
    msl_paste_lesions (include/mslesions3d_hip.h): [0] active, [1] donor case, [2..4] min, [5..7] extents e, [8] flips
    (bit a mirrors axis a), [9] the mask value, [10..12] where the donor box's centre floor((min + max) / 2) lands inside
    the destination box (mirrored), [13 + 3 j ..] corner of candidate j, floor(u_a (t_a - e_a + 1)).  ``case`` is the
    target's position in the bank's case order, ``target`` the sample's size.  Rows past the drawn count, a paste with
    some e_a > t_a and, in instances mode, one whose id (the target case's largest id of the donor's class + 1 + the
    earlier active pastes of that class) reaches min(hi, 32768) are inactive: all zeros.  ``draw`` None: all inactive."""
    rows = np.zeros((int(max_lesions), PASTE_HEAD + 3 * int(candidates)), dtype=np.int32)
    if draw is None:
        return rows
    if not len(bank.rows):
        raise ValueError("lesionpaste: the lesion bank is empty")
    t = np.asarray(target, dtype=np.int64)
    used = {}
    for k, (u, flips, cand) in enumerate(draw):
        row = bank.rows[min(int(np.floor(u * len(bank.rows))), len(bank.rows) - 1)]
        donor, label, lo, hi = int(row[0]), int(row[1]), row[2:5], row[5:8]
        e = hi - lo + 1
        if (e > t).any():
            continue
        value = 1
        if mode != "binary":
            value = int(bank.max_ids[case][label - 1]) + 1 + used.get(label, 0)
            if value >= min(thresholds[label - 1][1], PASTE_MAX_VALUE + 1):
                continue
            used[label] = used.get(label, 0) + 1
        centre = (lo + hi) // 2 - lo
        centre = np.where(np.asarray(flips) != 0, e - 1 - centre, centre)
        rows[k, 0], rows[k, 1], rows[k, 2:5], rows[k, 5:8] = 1, donor, lo, e
        rows[k, 8], rows[k, 9], rows[k, 10:13] = flips[0] + 2 * flips[1] + 4 * flips[2], value, centre
        rows[k, PASTE_HEAD:] = np.floor(np.asarray(cand, dtype=np.float64) * (t - e + 1)).astype(np.int64).reshape(-1)
    return rows


def _paste_row_ok(r, donors, target):
    """What msl_paste_lesions refuses (report -2): an inactive row, a case out of range, a donor box outside the case, an
    extent outside 1 .. PASTE_MAX_EXTENT, a value outside 1 .. 32767, a centre outside the box, a candidate outside the
    sample."""
    if r[0] == 0 or not 0 <= r[1] < len(donors):
        return False
    lo, e = r[2:5], r[5:8]
    if (e < 1).any() or (e > PASTE_MAX_EXTENT).any() or not 1 <= r[9] <= PASTE_MAX_VALUE:
        return False
    if (lo < 0).any() or (lo + e > np.asarray(donors[int(r[1])][1].shape[-3:])).any():
        return False
    if (r[10:13] < 0).any() or (r[10:13] >= e).any():
        return False
    cand = r[PASTE_HEAD:].reshape(-1, 3)
    return bool((cand >= 0).all() and (cand + e <= np.asarray(target)).all())


def paste_lesions(img, seg, pastes, donors):
    """Apply one sample's paste rows (``lower_pastes``) IN PLACE to ``img`` (C, T0, T1, T2) f32 and ``seg`` (T0, T1, T2) or
    (1, T0, T1, T2), both C-contiguous numpy arrays; ``donors[case]`` -> (image (C, n0, n1, n2) f32, mask (n0, n1, n2) or
    (1, ...)) of a cached case.  -> report, one int per row: the accepted candidate's index, -1 none accepted, -2 an
    inactive or refused row (``_paste_row_ok``).

    Rows are applied in order, each on the mask the earlier ones left.  The first candidate j passes whose (a)
    destination box, dilated by one voxel and clamped to the sample, holds no non-zero mask voxel and (b) image voxel at
    the destination of the donor box's centre is non-zero in every channel.  Writing, donor coordinates mirrored per
    flip bit: where the donor mask inside its box is non-zero, image = the donor's value in every channel and mask = the
    row's value; a rim voxel - inside the dilated box and the sample, not written, a 6-neighbour of a written voxel, its
    donor coordinate inside the donor case - gets image = 0.5f * dst + 0.5f * donor (two rounded products, one rounded sum)
    and keeps its mask."""
    img = np.asarray(img)
    mask = seg[0] if seg.ndim == 4 else seg
    T = np.asarray(mask.shape)
    half = np.float32(0.5)
    report = []
    for r in np.asarray(pastes, dtype=np.int64):
        if not _paste_row_ok(r, donors, T):
            report.append(-2)
            continue
        dimg, dseg = donors[int(r[1])]
        dseg = dseg[0] if dseg.ndim == 4 else dseg
        dimg = dimg[None] if dimg.ndim == 3 else dimg
        lo_d, e, flips, value, centre = r[2:5], r[5:8], [(r[8] >> a) & 1 for a in range(3)], r[9], r[10:13]
        accepted = -1
        for j, c in enumerate(r[PASTE_HEAD:].reshape(-1, 3)):
            a, b = np.maximum(c - 1, 0), np.minimum(c + e + 1, T)
            if mask[a[0]:b[0], a[1]:b[1], a[2]:b[2]].any():
                continue
            at = tuple(c + centre)
            if not all(img[ch][at] != 0 for ch in range(img.shape[0])):
                continue
            accepted = j
            break
        report.append(accepted)
        if accepted < 0:
            continue
        c = r[PASTE_HEAD + 3 * accepted:PASTE_HEAD + 3 * accepted + 3]
        # the dilated box in destination order, p = -1 .. e per axis; its donor coordinate, mirrored where flipped
        n = np.asarray(dseg.shape)
        idx, inside = [], []
        for ax in range(3):
            p = np.arange(-1, e[ax] + 1)
            d = lo_d[ax] + (e[ax] - 1 - p if flips[ax] else p)
            idx.append(np.clip(d, 0, n[ax] - 1))
            inside.append((d >= 0) & (d < n[ax]))
        grid = np.ix_(*idx)
        in_case = inside[0][:, None, None] & inside[1][None, :, None] & inside[2][None, None, :]
        in_box = np.zeros(tuple(e + 2), dtype=bool)
        in_box[1:-1, 1:-1, 1:-1] = True
        written = (dseg[grid] != 0) & in_box
        near = np.zeros_like(written)
        near[1:] |= written[:-1]
        near[:-1] |= written[1:]
        near[:, 1:] |= written[:, :-1]
        near[:, :-1] |= written[:, 1:]
        near[:, :, 1:] |= written[:, :, :-1]
        near[:, :, :-1] |= written[:, :, 1:]
        rim = near & ~written & in_case
        # clip the dilated box to the sample
        a, b = np.maximum(c - 1, 0), np.minimum(c + e + 1, T)
        cut = tuple(slice(a[k] - (c[k] - 1), b[k] - (c[k] - 1)) for k in range(3))
        dst = tuple(slice(a[k], b[k]) for k in range(3))
        written, rim = written[cut], rim[cut]
        for ch in range(img.shape[0]):
            src = dimg[ch][grid][cut].astype(np.float32)
            view = img[ch][dst]
            view[rim] = (half * view[rim]) + (half * src[rim])
            view[written] = src[written]
        mask[dst][written] = value
    return report


AUGMENTATIONS = {"flip": _aug_flip, "rotate90": _aug_rotate90, "affine": _aug_affine,
                 "zoom": _aug_zoom, "griddistortion": _aug_griddistortion, "elastic3d": _aug_elastic3d,
                 "shiftintensity": _aug_shiftintensity, "scaleintensity": _aug_scaleintensity,
                 "gaussiansmooth": _aug_gaussiansmooth, "biasfield": _aug_biasfield, "gaussiannoise": _aug_gaussiannoise,
                 PASTE_NAME: _aug_lesionpaste}
DRAWS = {"flip": _draw_flip, "rotate90": _draw_rotate90, "affine": _draw_affine,
         "zoom": _draw_zoom, "griddistortion": _draw_griddistortion, "elastic3d": _draw_elastic3d,
         "shiftintensity": _draw_shiftintensity, "scaleintensity": _draw_scaleintensity,
         "gaussiansmooth": _draw_gaussiansmooth, "biasfield": _draw_biasfield, "gaussiannoise": _draw_gaussiannoise,
         PASTE_NAME: _draw_lesionpaste}
MR_NAMES = ("gaussiansmooth", "biasfield", "gaussiannoise")


def transform_name(t):
    return t if isinstance(t, str) else t[0]


def check_mr_last(augmentations):
    """The MR transforms act on the finished sample: an entry of another kind behind one of them raises
    NotImplementedError (``devicedata.sample_params`` refuses the same lists).  ``lesionpaste`` acts there as well, in
    front of them: it stands once, behind every other entry and in front of the MR transforms, or the list is refused."""
    names = [transform_name(t) for t in augmentations]
    seen = pasted = False
    for n in names:
        if n in MR_NAMES:
            seen = True
        elif seen:
            raise NotImplementedError(f"{n} placed behind an MR transform ({' / '.join(MR_NAMES)} come last)")
        elif pasted:  # lesionpaste acts on the finished sample too: once, behind every entry that is not an MR transform
            raise NotImplementedError(f"{n} placed behind {PASTE_NAME} (only {' / '.join(MR_NAMES)} follow it)")
        elif n == PASTE_NAME:
            pasted = True


def draw_augmentations(augmentations, rs):
    """The draws the host transforms make for one sample, in their call order: [(name, draw or None), ...]."""
    out = []
    for t in augmentations:
        name, kw = (t, {}) if isinstance(t, str) else t
        out.append((name, DRAWS[name](rs, **kw)))
    return out

# train.py:132-143: the names the CLI accepts and the parameters the reference binds to them
REFERENCE_AUGMENTATIONS = [("flip", {"spatial_axis": (0, 1, 2), "prob": .5}),
                           ("rotate90", {"spatial_axes": (1, 2), "prob": .5}),
                           ("rotate90", {"spatial_axes": (0, 1), "prob": .5}),
                           ("rotate90", {"spatial_axes": (0, 2), "prob": .5}),
                           ("translate", {"mode": ("bilinear", "nearest"), "translate_range": (-3, 3), "prob": .7}),
                           ("scale", {"mode": ("bilinear", "nearest"), "scale_range": (0.15, 0.15, 0.15),
                                      "padding_mode": "reflection", "prob": .7})]


# train.py:196-205, train_lesions(): the entries of the clinical recipe that the example's list lacks (its flip / rotate90
# go by the same CLI names as the example's and keep the example's parameters)
LESIONS_AUGMENTATIONS = [("affine", {"mode": ("bilinear", "nearest"), "rotate_range": (np.pi / 12, np.pi / 12, np.pi / 12),
                                     "scale_range": (0.1, 0.1, 0.1), "padding_mode": "border"}),
                         ("shiftintensity", {"offsets": 0.1, "prob": 1.0}),
                         ("scaleintensity", {"factors": 0.1, "prob": 1.0})]


def select_augmentations(names):
    """train.py:145: keep the reference's entries whose name was asked for, each list in its own order (the example's
    first, then train_lesions()'s); translate / scale both become 'affine'."""
    known = [n for n, _ in REFERENCE_AUGMENTATIONS + LESIONS_AUGMENTATIONS]
    unknown = set(names) - set(known)
    if unknown:
        raise ValueError(f"unknown augmentation(s) {sorted(unknown)}; known: {' '.join(dict.fromkeys(known))}")
    out = [(n.replace("translate", "affine").replace("scale", "affine"), kw) for n, kw in REFERENCE_AUGMENTATIONS if n in names]
    return out + [(n, kw) for n, kw in LESIONS_AUGMENTATIONS if n in names]


# the registry's two spatial transforms that neither list of train.py binds (datasets.py:99-119): parameters of this
# project's choosing, MONAI's defaults for the ranges
WARP_AUGMENTATIONS = [("zoom", {"min_zoom": 0.9, "max_zoom": 1.1, "padding_mode": "border", "prob": 0.5}),
                      ("griddistortion", {"num_cells": 5, "distort_limit": 0.03, "padding_mode": "border", "prob": 0.5})]
# the free-form deformation: a 7^3 lattice, at most 7.5 voxels (the cap of ``deform_lattice``
# binds first on axes shorter than 121 voxels)
DEFORM_AUGMENTATIONS = [("elastic3d", {"control_points": 7, "max_displacement": 7.5, "padding_mode": "border", "prob": 0.2})]
INTENSITY_NAMES = ("shiftintensity", "scaleintensity")
# the MR acquisition stage, in acquisition order: resolution loss, coil inhomogeneity, thermal
# noise; MONAI's names and default ranges as remembered
MR_AUGMENTATIONS = [("gaussiansmooth", {"sigma": (0.25, 1.5), "prob": 0.1}),
                    ("biasfield", {"degree": 3, "coeff_range": (0.0, 0.1), "lattice": 9, "prob": 0.1}),
                    ("gaussiannoise", {"std": 0.1, "prob": 0.1})]
# copy-paste of cached lesions on to the finished sample: -dm lesions only
PASTE_AUGMENTATIONS = [(PASTE_NAME, {"prob": 0.5, "max_lesions": 4, "candidates": 8, "max_volume": None})]


def select_training_augmentations(names):
    """What ``train.py -a`` binds: ``select_augmentations`` for the reference's names, unchanged, plus the entries of
    ``WARP_AUGMENTATIONS`` that were asked for, in that list's order, behind the flips / rot90s / affines and in front of
    the intensity operations (the order ``devicedata.sample_params`` takes), the entry of ``DEFORM_AUGMENTATIONS`` behind
    those, plus the entries of ``MR_AUGMENTATIONS`` that were asked for, in that list's order, behind everything else.
    ``lesionpaste`` (``PASTE_AUGMENTATIONS``) stands behind every entry that is not an MR transform and in front of those.
    Unknown names raise ValueError."""
    resample = WARP_AUGMENTATIONS + DEFORM_AUGMENTATIONS
    own = [n for n, _ in resample] + [PASTE_NAME] + list(MR_NAMES)
    known = [n for n, _ in REFERENCE_AUGMENTATIONS + LESIONS_AUGMENTATIONS] + own
    unknown = set(names) - set(known)
    if unknown:
        raise ValueError(f"unknown augmentation(s) {sorted(unknown)}; known: {' '.join(dict.fromkeys(known))}")
    out = select_augmentations([n for n in names if n not in own])
    at = next((k for k, (n, _) in enumerate(out) if n in INTENSITY_NAMES), len(out))
    out = out[:at] + [(n, kw) for n, kw in resample if n in names] + out[at:]
    return out + [(n, kw) for n, kw in PASTE_AUGMENTATIONS + MR_AUGMENTATIONS if n in names]


def _load(path_noext):
    if os.path.exists(path_noext + ".npy"):
        return np.load(path_noext + ".npy")
    import nibabel as nib  # only when .nii.gz data is supplied
    return np.asarray(nib.load(path_noext + ".nii.gz").dataobj)


def _load_affine(path_noext):
    """The voxel -> world affine of a stored volume (4 x 4 f64, RAS+ mm, the NIfTI convention), or None: the sidecar
    ``PATH.affine.npy`` of ``PATH.npy``, or ``img.affine`` of ``PATH.nii.gz`` when nibabel is importable.  No sidecar
    means no affine: the volume is taken as already LPI at 1 mm."""
    if os.path.exists(path_noext + ".npy"):
        if not os.path.exists(path_noext + ".affine.npy"):
            return None
        affine = np.asarray(np.load(path_noext + ".affine.npy"), dtype=np.float64)
        if affine.shape != (4, 4):
            raise ValueError(f"{path_noext}.affine.npy: a 4 x 4 affine expected, got shape {affine.shape}")
        return affine
    import nibabel as nib
    return np.asarray(nib.load(path_noext + ".nii.gz").affine, dtype=np.float64)


class ShardSampler(Sampler):
    """Data-parallel shard of one epoch (BASELINE north_star: "data-parallel training shards synthetic volumes across the
    8 GPUs"): every rank draws the SAME permutation of the cases from (seed, epoch), pads it by wrapping around to a
    multiple of the world size - every rank runs the same number of steps, each of which contains collectives - and takes
    every world-th entry from its rank on.  Shards of one epoch are disjoint (up to the wrap-around padding) and cover the
    data set; ``set_epoch`` re-deals them.  world = 1 is the plain seeded shuffle, so a resumed run (train.py --checkpoint)
    sees the order the interrupted one would have seen."""

    def __init__(self, n, rank=0, world=1, shuffle=True, seed=0):
        if not 0 <= rank < world:
            raise ValueError(f"rank {rank} outside world {world}")
        self.n, self.rank, self.world, self.shuffle, self.seed, self.epoch = n, rank, world, shuffle, seed, 0

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def indices(self):
        order = (np.random.RandomState((self.seed * 1000003 + self.epoch) % (2 ** 31 - 1)).permutation(self.n) if self.shuffle
                 else np.arange(self.n))
        if self.n == 0:
            return order
        per = -(-self.n // self.world)
        order = np.resize(order, per * self.world)  # wrap-around padding
        return order[self.rank::self.world]

    def __iter__(self):
        return iter(self.indices().tolist())

    def __len__(self):
        return -(-self.n // self.world) if self.n else 0


def sample_rng(seed, epoch, subject):
    """The augmentation generator of one sample: a function of (seed, epoch, subject) alone."""
    return np.random.RandomState(zlib.crc32(f"{seed}:{epoch}:{subject}".encode()) & 0x7FFFFFFF)


class _Cases(Dataset):
    def __init__(self, root, subjects, n_classes, augmentations=None, seed=0):
        self.root, self.subjects, self.n_classes = root, subjects, n_classes
        self.augmentations = list(augmentations or [])
        for t in self.augmentations:
            if (t if isinstance(t, str) else t[0]) not in AUGMENTATIONS:
                raise ValueError(f"unknown transform {t!r}")
            if transform_name(t) == PASTE_NAME:  # uint8 class masks, no instances, no bank
                raise NotImplementedError(f"{PASTE_NAME} needs the lesion bank of a LesionsDataModule (-dm lesions)")
        # augmentation randomness is drawn per SAMPLE from (seed, epoch, subject): DataLoader workers are forked copies of
        # this object, so a generator stored here would hand every worker - and every epoch - the same stream
        self.seed, self.epoch = seed, 0

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def sample_rng(self, i):
        return sample_rng(self.seed, self.epoch, self.subjects[i])

    def __len__(self):
        return len(self.subjects)

    def __getitem__(self, i):
        s = self.subjects[i]
        img = _load(pjoin(self.root, "images", f"sub-{s}_image")).astype(np.float32)
        seg = _load(pjoin(self.root, "labels", f"sub-{s}_seg"))
        nz = img != 0
        if nz.any():
            std = img[nz].std()
            img[nz] = (img[nz] - img[nz].mean()) / (std if std != 0 else 1.0)
        img, seg = img[None], np.asarray(seg)[None]  # add_channel
        rs = self.sample_rng(i) if self.augmentations else None
        for t in self.augmentations:  # between normalizeintensity and bounding_boxes_generator (datasets.py:417-430)
            name, kw = (t, {}) if isinstance(t, str) else t
            img, seg = AUGMENTATIONS[name](img, seg, rs, **kw)
        img = np.ascontiguousarray(img)
        boxes, labels = boxes_from_segmentation(seg, self.n_classes)
        return {"img": torch.from_numpy(img), "boxes": boxes, "labels": labels, "seg": [boxes, labels], "subject": s,
                "img_meta_dict": {"affine": np.eye(4)}, "seg_meta_dict": {}, "img_transforms": [], "seg_transforms": []}


GEOMETRY_KEYS = ("crop_origin", "crop_shape", "full_shape")


def collate_fn(batch):
    """datasets.py:50-95: images stacked, ragged boxes / labels kept as lists."""
    boxes = [b["boxes"] for b in batch]
    labels = [b["labels"] for b in batch]
    out = {"img": torch.stack([b["img"] for b in batch], 0), "seg": [boxes, labels], "boxes": boxes, "labels": labels,
           "subject": [b["subject"] for b in batch], "img_meta_dict": [b["img_meta_dict"] for b in batch],
           "seg_meta_dict": [b["seg_meta_dict"] for b in batch], "img_transforms": [b["img_transforms"] for b in batch],
           "seg_transforms": [b["seg_transforms"] for b in batch]}
    for key in GEOMETRY_KEYS + ("native_shape", "patch_origin", "paste_report"):  # LesionsDataModule samples carry them; passed through as lists
        if all(key in b for b in batch):
            out[key] = [b[key] for b in batch]
    return out


class ExampleDataset:
    """datasets.py:359-485 surface: ``setup(stage)``, ``train_dataloader()``, ``test_dataloader()``,
    ``predict_dataloader()``, ``train_dataset`` / ``test_dataset``."""

    def __init__(self, n_classes=1, objects="multiple", percentage=1., augmentations=None, batch_size=8, num_workers=0,
                 verbose=False, random_state=970205, cache=False, subject=None,
                 data_dir="../data/artificial_dataset", dataset_name=None, rank=0, world_size=1):
        """``rank`` / ``world_size`` (not in the reference, which is single-GPU): this process's data-parallel shard of
        the train and validation cases (``ShardSampler``)."""
        assert n_classes == 1 or n_classes == 2
        d = data_dir + "/multiple_objects" if objects == "multiple" else data_dir
        d = pjoin(d, "one_class") if n_classes == 1 else pjoin(d, "double_class")
        self.data_dir = d if dataset_name is None else pjoin(d, dataset_name)
        self.batch_size, self.num_workers, self.random_state = batch_size, num_workers, random_state
        self.n_classes, self.subject, self.percentage = n_classes, subject, percentage
        self.augmentations = augmentations
        self.rank, self.world_size, self.epoch = rank, world_size, 0
        subs = sorted(s.replace("sub-", "")[:4] for s in os.listdir(pjoin(self.data_dir, "images")) if "sub-" in s)
        self.subjects_list = subs[:int(percentage * len(subs))] if percentage > 0 else subs
        self.train_dataset = self.test_dataset = self.predict_dataset = None

    def setup(self, stage=None):
        from sklearn.model_selection import train_test_split
        if self.subject is not None:
            train, test = [self.subject], [self.subject]
        else:
            train, test = train_test_split(self.subjects_list, test_size=0.2, random_state=self.random_state)
        self.train_dataset = _Cases(self.data_dir, train, self.n_classes, self.augmentations, self.random_state)
        self.test_dataset = _Cases(self.data_dir, test, self.n_classes)
        self.predict_dataset = _Cases(self.data_dir, train if stage == "predict_train" else test, self.n_classes)

    def set_epoch(self, epoch):
        """Call before ``train_dataloader()`` of every epoch: re-deals the shards and the augmentation draws."""
        self.epoch = int(epoch)
        if self.train_dataset is not None:
            self.train_dataset.set_epoch(epoch)

    def _loader(self, ds, shuffle, bs=None, shard=False):
        sampler = None
        if shard:
            sampler = ShardSampler(len(ds), self.rank, self.world_size, shuffle, self.random_state)
            sampler.set_epoch(self.epoch)
        return DataLoader(ds, batch_size=bs or self.batch_size, shuffle=shuffle if sampler is None else False, sampler=sampler,
                          num_workers=self.num_workers, collate_fn=collate_fn, drop_last=False)

    def train_dataloader(self):
        return self._loader(self.train_dataset, True, shard=True)

    def test_dataloader(self):
        return self._loader(self.test_dataset, False, shard=self.world_size > 1)

    def predict_dataloader(self):
        return self._loader(self.predict_dataset, False, 1)


# ---- clinical cases: instance masks, foreground crop, fixed-size fit (reference datasets.py:125-335) ----------------
# crop_foreground and resize_with_pad_or_crop restate MONAI's CropForegroundd / ResizeWithPadOrCropd, which are not
# installed here: their parity is NOT pinned; the formulas in the docstrings are the contract.

def foreground_box(img, margin=5):
    """CropForegroundd(source_key="img", margin): F = {v : img[v] > 0}; per axis lo = max(min(F) - margin, 0),
    hi = min(max(F) + margin + 1, n); an empty F keeps the whole volume.  -> (lo, hi), three ints each.  A channel-first
    (C, D, H, W) image gives the box of the union F = {v : img[c, v] > 0 for any c} (CropForegroundd with
    channel_indices=None), still three ints each."""
    img = np.asarray(img)
    if img.ndim == 4:
        img = (img > 0).any(0)
    fg = np.argwhere(img > 0)
    if fg.shape[0] == 0:
        return (0,) * img.ndim, tuple(img.shape)
    lo = np.maximum(fg.min(0) - margin, 0)
    hi = np.minimum(fg.max(0) + margin + 1, img.shape)
    return tuple(int(v) for v in lo), tuple(int(v) for v in hi)


def crop_foreground(img, seg, margin=5):
    """Image (D, H, W) or (C, D, H, W) and mask (D, H, W) cropped to ``foreground_box(img, margin)``: one box for every
    channel and the mask."""
    lo, hi = foreground_box(img, margin)
    sl = tuple(slice(a, b) for a, b in zip(lo, hi))
    return img[(slice(None),) * (np.ndim(img) - 3) + sl], seg[sl]


def fit_shift(n, t):
    """resize_with_pad_or_crop on one axis of size n with target t: output index o reads source index
    clamp(o + d, 0, n - 1) with d = -((t - n) // 2) when padding and d = n // 2 - t // 2 when cropping."""
    return -((t - n) // 2) if n < t else n // 2 - t // 2


def resize_with_pad_or_crop(vol, spatial_size):
    """ResizeWithPadOrCropd(spatial_size, mode="replicate") on the trailing len(spatial_size) axes of ``vol``: per
    axis, n < t pads by edge replication with before = (t - n) // 2, after = t - n - before; n > t keeps
    [start, start + t) with start = n // 2 - t // 2."""
    vol = np.asarray(vol)
    first = vol.ndim - len(spatial_size)
    for k, t in enumerate(spatial_size):
        n = vol.shape[first + k]
        idx = np.clip(np.arange(t) + fit_shift(n, t), 0, n - 1)
        vol = np.take(vol, idx, axis=first + k)
    return vol


def window(vol, origin, size):
    """The window of ``size`` voxels at ``origin`` of the trailing three axes of ``vol``: output index p of axis k reads
    source index clamp(p + origin_k, 0, n_k - 1) - edge replication; origins may be negative and windows may overhang.
    ``window(v, [fit_shift(n, t) ...], t)`` is ``resize_with_pad_or_crop(v, t)``, and it is the unflipped row
    (origin, 0, 0, 0) of ``gather_views``.  ``msl_augment_window_mc`` (csrc/datapipe.hip) takes the same origins."""
    vol = np.asarray(vol)
    if len(origin) != 3 or len(size) != 3 or vol.ndim < 3:
        raise ValueError("window: three origins and three sizes on an array of at least three axes")
    first = vol.ndim - 3
    for k in range(3):
        n = vol.shape[first + k]
        vol = np.take(vol, np.clip(np.arange(int(size[k])) + int(origin[k]), 0, n - 1), axis=first + k)
    return vol


def fit_to_case_frame(boxes, target, crop_shape, crop_origin, full_shape):
    """Corner boxes, fractional in the fitted frame of ``target`` voxels -> the same boxes, fractional in the case's own
    frame of ``full_shape`` voxels.  ``boxes`` (K, 6) float32; ``crop_shape`` / ``crop_origin`` are the shape and the ``lo``
    of the case's ``foreground_box`` crop.  Per axis, with t, n, lo, s from the four shape arguments and d =
    ``fit_shift(n, t)``, fitted voxel o shows cropped voxel o + d, which is voxel o + d + lo of the case, so a
    coordinate c becomes ``(c * t + (d + lo)) / s``: in float32, one multiply, one add of the integer d + lo, one divide.
    Boxes are not clamped (``detect_objects`` returns unclamped boxes; the drawing clips).

    This inverts the crop and the fit (steps 1 and 4 of ``_LesionCases``) only: it is defined for the un-augmented
    pipeline, i.e. the predict and validation data sets.  Where the fit CROPS an axis, a lesion outside the kept window
    is not in the fitted mask and a lesion across its border maps back as its part inside the window.
    ``msl_boxes_to_case`` (csrc/overlay.hip) computes the same values on the device, bit for bit."""
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 6)
    t = np.asarray(target, dtype=np.int64)
    n = np.asarray(crop_shape, dtype=np.int64)
    add = np.asarray([fit_shift(int(a), int(b)) for a, b in zip(n, t)], dtype=np.int64) + np.asarray(crop_origin, dtype=np.int64)
    s = np.asarray(full_shape, dtype=np.int64)
    if not (t.shape == n.shape == add.shape == s.shape == (3,)):
        raise ValueError("fit_to_case_frame: target, crop_shape, crop_origin and full_shape are three ints each")
    t2, add2, s2 = (np.tile(v, 2).astype(np.float32) for v in (t, add, s))
    return (boxes * t2 + add2) / s2


# ---- multi-view prediction: tiled and flipped views of one case ------------------------------
MAX_VIEWS = 64  # msl_views_merge's capacity


def view_plan(case_shape, tile, margin=(8, 8, 8), flip_axes=()):
    """The views prediction shows the network of one case of ``case_shape``: windows of ``tile`` voxels, optionally
    mirrored -> int32 (V, 6), rows ``o0, o1, o2, f0, f1, f2`` (origin in case voxels, 0 / 1 flip flags).  Per axis with
    case size n, tile t, margin m: n <= t gives the one origin ``fit_shift(n, t)`` (<= 0: the view pads by edge
    replication as the fit does); n > t gives K = ceil((n - t) / (t - 2m)) + 1 origins o_i = (i * (n - t)) // (K - 1),
    the first 0, the last n - t, neighbours overlapping by at least 2m (t <= 2m raises ValueError).  Tiles are the product
    of the three axes, axis 0 slowest; every tile is followed by its flipped copies, one per subset of ``flip_axes``
    (subset i holds flip_axes[b] for every set bit b of i, so the unflipped one comes first): tile-major, flip-minor.
    More than 64 views raise ValueError."""
    case_shape, tile, margin = (tuple(int(v) for v in x) for x in (case_shape, tile, margin))
    flip_axes = tuple(int(a) for a in flip_axes)
    if not (len(case_shape) == len(tile) == len(margin) == 3) or min(case_shape + tile) < 1 or min(margin) < 0:
        raise ValueError("view_plan: case_shape, tile and margin are three ints each (sizes >= 1, margins >= 0)")
    if len(set(flip_axes)) != len(flip_axes) or any(a not in (0, 1, 2) for a in flip_axes):
        raise ValueError(f"view_plan: flip_axes {flip_axes} must be distinct axes out of 0, 1, 2")
    origins = []
    for n, t, m in zip(case_shape, tile, margin):
        if n <= t:
            origins.append([fit_shift(n, t)])
            continue
        if t <= 2 * m:
            raise ValueError(f"view_plan: a tile of {t} voxels has no core left inside a margin of {m} (--tile_margin)")
        K = -(-(n - t) // (t - 2 * m)) + 1
        origins.append([(i * (n - t)) // (K - 1) for i in range(K)])
    flips = []
    for sub in range(1 << len(flip_axes)):
        f = [0, 0, 0]
        for b, a in enumerate(flip_axes):
            if (sub >> b) & 1:
                f[a] = 1
        flips.append(f)
    V = len(origins[0]) * len(origins[1]) * len(origins[2]) * len(flips)
    if V > MAX_VIEWS:
        raise ValueError(f"view_plan: {V} views of a {case_shape} case exceed the merge capacity of {MAX_VIEWS}: a larger "
                         "--spatial_size, a smaller --tile_margin or fewer --flip_views axes reduce it")
    rows = [[a, b, c] + f for a in origins[0] for b in origins[1] for c in origins[2] for f in flips]
    return np.asarray(rows, dtype=np.int32).reshape(-1, 6)


def check_views(views):
    """(V, 6) int32 view table with 0 / 1 flip flags, V >= 1 (ValueError otherwise)."""
    views = np.ascontiguousarray(np.asarray(views, dtype=np.int32))
    if views.ndim != 2 or views.shape[1] != 6 or views.shape[0] < 1 or not np.isin(views[:, 3:], (0, 1)).all():
        raise ValueError("views: (V, 6) rows o0, o1, o2, f0, f1, f2 with V >= 1 and 0 / 1 flip flags")
    return views


def gather_views(case, views, tile):
    """The views of a (C, n0, n1, n2) case as one (V, C, T0, T1, T2) float32 batch: output voxel p of view v reads
    ``case[c][s]`` with q_k = T_k - 1 - p_k where the view is flipped along k (else p_k) and s_k = clamp(o_k + q_k, 0,
    n_k - 1).  One unflipped view at the ``fit_shift`` origins is ``resize_with_pad_or_crop(case, tile)``.
    ``msl_view_gather`` (csrc/views.hip) computes the same values on the device, bit for bit."""
    case = np.asarray(case, dtype=np.float32)
    views = check_views(views)
    if case.ndim != 4 or len(tile) != 3:
        raise ValueError("gather_views: case is (C, n0, n1, n2) and tile three ints")
    out = np.empty((views.shape[0], case.shape[0]) + tuple(int(t) for t in tile), dtype=np.float32)
    for v, row in enumerate(views):
        vol = case
        for k in range(3):
            n, t = case.shape[1 + k], int(tile[k])
            vol = np.take(vol, np.clip(np.arange(t) + int(row[k]), 0, n - 1), axis=1 + k)
            if row[3 + k]:
                vol = np.flip(vol, axis=1 + k)
        out[v] = vol
    return out


def _instance_extents(seg, thresholds, mode):
    """The walk of ``boxes_from_instances`` -> (inclusive integer extents [min..., max...] as a list of rows, labels,
    the mask's shape), flat boxes still in."""
    seg = np.squeeze(np.asarray(seg))
    if mode == "binary":
        seg, _ = cc_label(seg)
        thresholds = [(1, np.inf)]
    elif mode != "instances":
        raise ValueError(f"unknown segmentation mode {mode!r}")
    ids = np.unique(seg)[1:]
    extents, labels = [], []
    for c, (lo, hi) in enumerate(thresholds):
        for l in ids[(ids >= lo) & (ids < hi)]:
            idx = np.where(seg == l)
            extents.append([idx[0].min(), idx[1].min(), idx[2].min(), idx[0].max(), idx[1].max(), idx[2].max()])
            labels.append(c + 1)
    return extents, labels, seg.shape


def _fractional_boxes(extents, shape):
    """Integer extents / image size in f32 -> ((K, 6) boxes, keep mask of the boxes with a volume)."""
    size = np.array(tuple(shape) * 2, dtype=np.float32)
    boxes = torch.from_numpy(np.asarray(extents, dtype=np.float32).reshape(-1, 6) / size)
    keep = ((boxes[:, 3] - boxes[:, 0]) * (boxes[:, 4] - boxes[:, 1]) * (boxes[:, 5] - boxes[:, 2])) != 0
    return boxes, keep


def boxes_from_instances(seg, thresholds, mode="instances"):
    """BoundingBoxesGeneratord, 'instances' mode (utils.py:442-443, 472-481, 485-513) on an instance-labelled mask: the
    ids are the sorted unique values with the FIRST one discarded (the background - on a mask without background the
    smallest id is lost, as in the reference); per threshold pair (lo, hi) in order, the ids with lo <= id < hi give
    the inclusive voxel extents [min..., max...] and the label is the pair's position + 1; ids outside every pair are
    dropped; extents / image size in f32; zero-volume boxes removed.  ``mode="binary"`` (utils.py:445-448): connected
    components of the mask first, then thresholds [(1, inf)]."""
    extents, labels, shape = _instance_extents(seg, thresholds, mode)
    boxes, keep = _fractional_boxes(extents, shape)
    labels = torch.tensor(labels, dtype=torch.long)
    if boxes.numel():
        boxes, labels = boxes[keep], labels[keep]
    return boxes, labels


# ---- patch training: one sampled window per case and epoch -----------------------------------
def lesion_centres(seg, thresholds, mode="instances"):
    """-> f64 (K, 3): per box ``boxes_from_instances`` keeps, in its order, the centre (min + max) / 2 of the inclusive
    integer voxel extents (so a lesion of an even number of voxels along an axis has a half-integer centre there)."""
    extents, _, shape = _instance_extents(seg, thresholds, mode)
    ext = np.asarray(extents, dtype=np.float64).reshape(-1, 6)
    if ext.shape[0]:
        ext = ext[_fractional_boxes(extents, shape)[1].numpy()]
    return (ext[:, :3] + ext[:, 3:]) / 2


def centres_to_augmented(centres, shape, perm, stages=()):
    """Voxel positions (K, 3) f64 of a case of ``shape`` -> the same points in the frame of the augmented case.  ``perm``
    = (ax, rev) and ``stages`` come from ``devicedata.sample_params(..., ragged=True)``, the parameters both routes share.
    Signed permutation: c'_a = n'_a - 1 - c[ax_a] where rev_a, else c[ax_a], with n'_a = shape[ax_a].  Then per affine
    stage, in order, q = solve(M, c' - offset): the inverse of "output voxel q samples at M q + offset" (f64).  Per warp
    stage (``tables``: output voxel q samples at t_a[q_a]), per axis the smallest real q in [0, n' - 1] with t(q) = c',
    t being the table under linear interpolation: i = np.searchsorted(t, c', "left"), q = i - 1 + (c' - t[i - 1]) /
    (t[i] - t[i - 1]), and 0 / n' - 1 where c' lies at or below t[0] / above t[n' - 1].  Per deformation stage
    (``lattice``: output voxel q samples at q + d(q)) the fixed point of ``_deform_inverse``.  Stages without a matrix,
    tables or a lattice (None, intensity operations) do not move a point."""
    c = np.asarray(centres, dtype=np.float64).reshape(-1, 3)
    ax, rev = perm
    out = np.empty_like(c)
    for a in range(3):
        out[:, a] = (shape[ax[a]] - 1) - c[:, ax[a]] if rev[a] else c[:, ax[a]]
    for st in stages:
        if hasattr(st, "matrix") and out.shape[0]:
            out = np.linalg.solve(np.asarray(st.matrix, dtype=np.float64),
                                  (out - np.asarray(st.offset, dtype=np.float64)).T).T
        elif hasattr(st, "tables") and out.shape[0]:
            out = np.stack([_table_inverse(st.tables[a], out[:, a]) for a in range(3)], 1)
        elif hasattr(st, "lattice") and out.shape[0]:
            out = _deform_inverse(st.lattice, tuple(shape[ax[a]] for a in range(3)), out)
    return out


def _deform_inverse(P, shape, c):
    """``centres_to_augmented``'s rule for a deformation stage: the q with q + d(q) = c', by q_0 = c' and q_{k+1} =
    clip(c' - d(q_k), 0, n' - 1), 30 times (f64).  ``deform_lattice``'s cap makes d a contraction, so the iteration
    converges to the one solution."""
    hi = np.asarray(shape, dtype=np.float64) - 1.0
    q = c
    for _ in range(30):
        q = np.clip(c - deform_displacement(shape, P, q), 0.0, hi)
    return q


def _table_inverse(table, c):
    """``centres_to_augmented``'s rule on one axis: the smallest q in [0, n - 1] with t(q) = c, clamped."""
    t = np.asarray(table, dtype=np.float64)
    n = t.size
    if n == 1:
        return np.zeros(c.shape[0])
    i = np.searchsorted(t, c, "left")  # t[i - 1] < c <= t[i]
    k = np.clip(i, 1, n - 1)
    with np.errstate(divide="ignore", invalid="ignore"):  # (a flat interval is only met where the clamp decides)
        q = (k - 1) + (c - t[k - 1]) / (t[k] - t[k - 1])
    return np.clip(np.where(i == 0, 0.0, np.where(i >= n, n - 1.0, q)), 0.0, n - 1.0)


def patch_origin(rs, shape, patch, centres, foreground):
    """The origin (three ints) of one training window of ``patch`` voxels in a case of ``shape`` (the augmented case's n');
    ``centres`` (K, 3) are lesion centres in that frame.  Always eight draws, in this order, whichever branch is taken:
    ``u, ku = rs.random_sample(2)``, ``j = rs.random_sample(3)``, ``r = rs.random_sample(3)``.  With K > 0 and
    u < foreground the window goes on lesion k = min(int(ku * K), K - 1): per axis o = floor(c_k) - t // 2 +
    floor((j - 0.5) * (t // 2)), a jitter of up to a quarter patch either way; otherwise o = floor(r * (n' - t + 1)),
    uniform over the positions inside the case.  Then per axis: n' <= t gives ``fit_shift(n', t)`` (the whole axis,
    padded as the fit pads it), else o is clamped to [0, n' - t].  On the lesion branch with the centre inside the case,
    floor(c) lies in [o, o + t) on every axis: the jitter leaves it between t // 4 and 3 t // 4 + 1 voxels in, and a
    clamp moves the window towards it."""
    u, ku = rs.random_sample(2)
    j = rs.random_sample(3)
    r = rs.random_sample(3)
    centres = np.asarray(centres, dtype=np.float64).reshape(-1, 3)
    K = centres.shape[0]
    shape, patch = [int(n) for n in shape], [int(t) for t in patch]
    if len(shape) != 3 or len(patch) != 3 or min(shape + patch) < 1:
        raise ValueError(f"patch_origin: three positive sizes each, got {shape} and {patch}")
    if K > 0 and u < foreground:
        c = centres[min(int(ku * K), K - 1)]
        o = [int(np.floor(c[a])) - patch[a] // 2 + int(np.floor((j[a] - 0.5) * (patch[a] // 2))) for a in range(3)]
    else:
        o = [int(np.floor(r[a] * (shape[a] - patch[a] + 1))) for a in range(3)]
    return tuple(fit_shift(n, t) if n <= t else min(max(v, 0), n - t) for v, n, t in zip(o, shape, patch))


# ---- native grid -> LPI at 1 mm (reference datasets.py:199-205: orientation(axcodes="LPI"), spacing(pixdim=(1, 1, 1))) --
# Orientationd / Spacingd are MONAI's (through nibabel's orientation codes); neither library is installed here, so the
# rule below is this project's own and its parity is NOT pinned.  The map is axis-aligned: a
# signed axis permutation plus one step per axis; the obliquity of an acquisition is kept, as Spacingd keeps it.

RegridPlan = collections.namedtuple("RegridPlan", "ax rev step start src_shape out_shape out_affine identity")


def regrid_plan(affine, shape, pixdim=(1., 1., 1.)):
    """The axis-aligned map of a native volume of ``shape`` with voxel -> world ``affine`` (4 x 4, RAS+ mm) onto the LPI
    grid of ``pixdim`` mm, all in f64 -> ``RegridPlan``:

    orientation: R = affine[:3, :3], z_j = |R[:, j]|, cos = R / z.  ``ax`` is the permutation maximising
    sum_k |cos[k, ax[k]]| (ties: the lexicographically smallest): source axis ax[k] becomes reoriented axis k.
    ``rev[k] = cos[k, ax[k]] > 0``: LPI axes point along -x, -y, -z of RAS+ world, so a source axis that increases towards
    R / A / S is reversed.  The reoriented volume has spacing z'_k = z[ax[k]] and shape n'_k = shape[ax[k]].

    spacing: z'_k snaps to p_k = pixdim[k] when |z'_k - p_k| <= 1e-4 p_k.  Output voxel o reads the reoriented volume
    at ``step * o + start`` with step_k = p_k / z'_k and start_k = 0 (the centres of voxel 0 coincide), and
    ``out_shape[k] = max(1, round((n'_k - 1) z'_k / p_k + 1))``.

    ``identity``: ax == (0, 1, 2), nothing reversed, every step exactly 1.  ``out_affine``: columns
    +-R[:, ax[k]] / z[ax[k]] * p_k (minus where reversed); the translation is the world position of the source voxel
    that becomes output voxel 0.  A singular R, a zero or non-finite z -> ValueError."""
    affine = np.asarray(affine, dtype=np.float64)
    shape = tuple(int(n) for n in shape)
    p = np.asarray(pixdim, dtype=np.float64)
    if affine.shape != (4, 4) or len(shape) != 3 or min(shape) < 1 or p.shape != (3,):
        raise ValueError(f"regrid_plan: a 4 x 4 affine, three positive sizes and three spacings expected, got "
                         f"{affine.shape}, {shape}, {p.shape}")
    if not (np.isfinite(p).all() and (p > 0).all()):
        raise ValueError(f"regrid_plan: pixdim must be positive and finite, got {pixdim}")
    R = affine[:3, :3]
    if not np.isfinite(affine).all():
        raise ValueError("regrid_plan: the affine holds a non-finite value")
    z = np.sqrt((R * R).sum(0))
    if not (np.isfinite(z).all() and (z > 0).all()) or np.linalg.matrix_rank(R) < 3:
        raise ValueError(f"regrid_plan: the affine's 3 x 3 part is singular (column norms {z.tolist()})")
    cos = R / z
    best, ax = -1.0, None
    for perm in itertools.permutations(range(3)):  # lexicographic order; a strict > keeps the first of equals
        score = sum(abs(cos[k, perm[k]]) for k in range(3))
        if score > best:
            best, ax = score, perm
    rev = tuple(bool(cos[k, ax[k]] > 0) for k in range(3))
    zr = np.array([z[ax[k]] for k in range(3)])
    nr = np.array([shape[ax[k]] for k in range(3)], dtype=np.int64)
    zr = np.where(np.abs(zr - p) <= 1e-4 * p, p, zr)
    step = p / zr
    start = np.zeros(3, dtype=np.float64)
    out_shape = tuple(max(1, int(np.round((nr[k] - 1) * zr[k] / p[k] + 1.0))) for k in range(3))
    out_affine = np.eye(4, dtype=np.float64)
    first = np.zeros(3, dtype=np.float64)  # the source voxel that becomes output voxel 0
    for k in range(3):
        out_affine[:3, k] = (-1.0 if rev[k] else 1.0) * R[:, ax[k]] / z[ax[k]] * p[k]
        first[ax[k]] = shape[ax[k]] - 1 if rev[k] else 0
    out_affine[:3, 3] = R @ first + affine[:3, 3]
    identity = ax == (0, 1, 2) and not any(rev) and bool((step == 1.0).all())
    return RegridPlan(ax, rev, tuple(float(v) for v in step), tuple(float(v) for v in start), shape, out_shape,
                      out_affine, identity)


def reorient(vol, plan):
    """The trailing three axes of ``vol`` in the plan's reoriented order: np.transpose, then np.flip (a view)."""
    lead = vol.ndim - 3
    vol = np.transpose(vol, tuple(range(lead)) + tuple(lead + a for a in plan.ax))
    flip = tuple(lead + k for k in range(3) if plan.rev[k])
    return np.flip(vol, flip) if flip else vol


def regrid(img, seg, plan):
    """Image (D, H, W) or (C, D, H, W) and mask (D, H, W) of a native case on the plan's grid (either may be None).  An
    identity plan returns the inputs untouched.  Otherwise: ``reorient``, then per channel and for the mask
    ``scipy.ndimage.affine_transform(a.astype(float32), diag(step), offset=start, output_shape=out_shape, order=1
    (image) / 0 (mask), mode="nearest")``, cast back to the input's dtype as ``_aug_affine`` does.  ``msl_regrid``
    (csrc/datapipe.hip) computes the same arrays on the device, bit for bit."""
    if plan.identity:
        return img, seg
    from scipy.ndimage import affine_transform
    mat, off = np.diag(np.asarray(plan.step, dtype=np.float64)), np.asarray(plan.start, dtype=np.float64)

    def one(a, order):
        return affine_transform(np.ascontiguousarray(a).astype(np.float32), mat, offset=off, output_shape=plan.out_shape,
                                order=order, mode="nearest").astype(a.dtype)

    if img is not None:
        img = np.asarray(img)
        if img.shape[-3:] != tuple(plan.src_shape) or img.ndim not in (3, 4):
            raise ValueError(f"regrid: image of shape {img.shape} on a plan for {plan.src_shape}")
        r = reorient(img, plan)
        img = one(r, 1) if img.ndim == 3 else np.stack([one(ch, 1) for ch in r])
    if seg is not None:
        seg = np.asarray(seg)
        if seg.shape != tuple(plan.src_shape):
            raise ValueError(f"regrid: mask of shape {seg.shape} on a plan for {plan.src_shape}")
        seg = one(reorient(seg, plan), 0)
    return img, seg


def regrid_to_native(boxes, plan):
    """Corner boxes, fractional in the plan's regridded frame -> the same boxes, fractional in the native frame, computed
    in f64 and returned as (K, 6) f32.  Per regridded axis k a coordinate c is voxel r = step_k * (c * out_shape_k) of
    the reoriented volume, which is v = r, or v = (n'_k - 1) - r where the axis is reversed (min and max then swap), of
    source axis ax[k]; v / n'_k is the native fraction.  Nothing is clamped."""
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 6)
    out = np.empty_like(b)
    for k in range(3):
        a, n = plan.ax[k], float(plan.src_shape[plan.ax[k]])
        lo = plan.step[k] * (b[:, k] * plan.out_shape[k])
        hi = plan.step[k] * (b[:, 3 + k] * plan.out_shape[k])
        if plan.rev[k]:
            lo, hi = (n - 1.0) - hi, (n - 1.0) - lo
        out[:, a], out[:, 3 + a] = lo / n, hi / n
    return out.astype(np.float32)


def normalize_nonzero(img):
    """NormalizeIntensity(nonzero=True) as ``_Cases`` applies it: population mean / std over the non-zero voxels of the
    whole array (``_LesionCases`` calls it once per channel)."""
    img = np.array(img, dtype=np.float32)
    nz = img != 0
    if nz.any():
        std = img[nz].std()
        img[nz] = (img[nz] - img[nz].mean()) / (std if std != 0 else 1.0)
    return img


NORM_LANES = 1024  # NORM_THREADS of csrc/datapipe.hip


def _lane_sum(values):
    """f64 sum of a flat f64 array in msl_normalize_nonzero's order: lane t adds elements t, t + 1024, ... one after the
    other from 0.0, then the lanes fold as a tree, lane t += lane t + s for s = 512 .. 1."""
    pad = (-values.size) % NORM_LANES
    rows = np.concatenate([values, np.zeros(pad)]).reshape(-1, NORM_LANES)
    acc = np.zeros(NORM_LANES, dtype=np.float64)
    for row in rows:
        acc = acc + row
    s = NORM_LANES // 2
    while s:
        acc = acc[:s] + acc[s:2 * s]
        s //= 2
    return float(acc[0])


def normalize_nonzero_device(img):
    """NormalizeIntensity(nonzero=True) with the arithmetic of msl_normalize_nonzero (csrc/datapipe.hip), bit for bit:
    the sum of the non-zero voxels and, with mean = sum / count, the sum of their (v - mean)^2, both in f64 in the
    kernel's fixed order (``_lane_sum``; a zero voxel adds 0.0, which changes nothing); then (v - f32(mean)) /
    f32(sqrt(q / count)) in f32 on the non-zero voxels, a deviation of 0 taken as 1.  Within the bound of DESIGN.md section
    4.7 of ``normalize_nonzero``, whose f32 sums are numpy's.  Patch training normalises with it on the host, so that the
    host and the device route train on the same bits."""
    img = np.array(img, dtype=np.float32)
    nz = img != 0
    count = int(nz.sum())
    if count == 0:
        return img
    flat = img.reshape(-1).astype(np.float64)
    mean = _lane_sum(flat) / float(count)
    dev = np.where(nz.reshape(-1), flat - mean, 0.0)
    std = np.float32(np.sqrt(_lane_sum(dev * dev) / float(count)))
    if std == 0:
        std = np.float32(1.0)
    img[nz] = (img[nz] - np.float32(mean)) / std
    return img


def _same_affine(affine, other, case, name):
    """Image(s) and mask of one case share one affine (or none of them has one): ValueError otherwise."""
    if (affine is None) != (other is None) or (affine is not None and not np.allclose(affine, other, rtol=0.0, atol=1e-4)):
        raise ValueError(f"case {case}: image {name} and the mask carry different affines")


class _DonorCases:
    """``paste_lesions``'s donors on the host route: ``self[j]`` -> (image, mask) of ``cases.cropped(j)``, the last
    ``keep`` cases held, so that the samples of one batch do not load the same donor twice."""

    def __init__(self, cases, keep=8):
        self.cases, self.keep, self._held = cases, int(keep), collections.OrderedDict()

    def __len__(self):
        return len(self.cases)

    def __getitem__(self, j):
        if j in self._held:
            self._held.move_to_end(j)
        else:
            self._held[j] = self.cases.cropped(j)[:2]
            while len(self._held) > self.keep:
                self._held.popitem(last=False)
        return self._held[j]


class _LesionCases(Dataset):
    """The per-sample pipeline of LesionsDataModule (datasets.py:199-236): load -> orientation("LPI") + spacing(1 mm)
    for a case that carries an affine (``regrid_plan`` / ``regrid``) -> crop_foreground(margin 5) ->
    NormalizeIntensity(nonzero) -> training augmentations at the cropped shape -> resize_with_pad_or_crop(replicate) ->
    boxes ('instances' / 'binary' mode).  With C = len(input_images) > 1 the image is channel-first throughout: the crop
    box is the union of the channels' foregrounds, every channel is normalised over its own non-zero voxels, and one set
    of augmentation draws moves all channels and the mask (the intensity operands are shared, as in MONAI).  The MR
    transforms (``MR_NAMES``) are drawn in list order with the others but applied to the fitted / windowed sample, where
    the device route applies them; they must come last (``check_mr_last``).  ``lesionpaste`` is
    drawn in list order too and applied to the fitted / windowed sample in front of them: ``lower_pastes`` on the data
    set's ``bank``, ``paste_lesions`` with the donors ``cropped(j)`` gives; the sample then carries "paste_report"."""

    def __init__(self, module, subjects, augmentations=None, seed=0, patch=None):
        self.module, self.subjects = module, list(subjects)
        self.root = module.data_dir  # the key DeviceCache-style caches file a case under, with its subject
        self.augmentations = list(augmentations or [])
        for t in self.augmentations:
            if (t if isinstance(t, str) else t[0]) not in AUGMENTATIONS:
                raise ValueError(f"unknown transform {t!r}")
        check_mr_last(self.augmentations)  # they are applied behind the fit / window
        self.seed, self.epoch = seed, 0
        self.patch = None if patch is None else tuple(int(t) for t in patch)  # training windows instead of the fit
        self._plans = {}  # position -> the RegridPlan of the case's last load (None: no affine); native_plan
        self.paste_kw = next((dict(PASTE_AUGMENTATIONS[0][1], **({} if isinstance(t, str) else t[1]))
                              for t in self.augmentations if transform_name(t) == PASTE_NAME), None)
        if self.paste_kw is not None:
            check_lesionpaste(**self.paste_kw)
        self.bank = None  # LesionBank of a list that names lesionpaste: build_bank, at set-up
        self.donors = _DonorCases(self)

    def build_bank(self):
        """The lesion bank of this data set's cases, in ``subjects`` order: per case the extents
        and labels its box stage gives on the cropped, un-augmented mask.  Every case is loaded once.  An empty bank
        raises ValueError."""
        m = self.module
        per_case = []
        for i in range(len(self)):
            seg = self.cropped(i)[1]
            extents, labels, shape = _instance_extents(seg, m.thresholds, m.segmentation_mode)
            keep = _fractional_boxes(extents, shape)[1].numpy() if extents else np.zeros(0, dtype=bool)
            per_case.append((np.asarray(extents, dtype=np.int64).reshape(-1, 6)[keep], np.asarray(labels, dtype=np.int64)[keep],
                             shape, class_max_ids(seg, m.thresholds, m.segmentation_mode)))
        self.bank = bank_from_lesions(per_case, self.paste_kw.get("max_volume"))
        if not len(self.bank.rows):
            raise ValueError(f"{PASTE_NAME}: the lesion bank is empty: no lesion of the {len(self)} training cases is at most "
                             f"{PASTE_MAX_EXTENT} voxels wide, clear of its neighbours and within max_volume")
        return self.bank

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def sample_rng(self, i):
        return sample_rng(self.seed, self.epoch, self.subjects[i])

    def __len__(self):
        return len(self.subjects)

    def load_native(self, i):
        """-> (image f32, mask, affine or None) of case i as stored, on its native grid: (D, H, W) each; with C > 1
        sequences the image is (C, D, H, W), stacked in ``input_images`` order.  The affine is the one the image(s) and
        the mask share (np.allclose at atol 1e-4, else ValueError); None when no file of the case carries one."""
        m = self.module
        c, s = self.subjects[i]
        seg = np.asarray(_load(m._get_sequence(c, s, m.segmentation)))
        affine = _load_affine(m._get_sequence(c, s, m.segmentation))
        imgs = []
        for name in m.input_images:
            img = _load(m._get_sequence(c, s, name)).astype(np.float32)
            if img.ndim != 3 or seg.shape != img.shape:
                raise ValueError(f"case {(c, s)}: image {name} {img.shape} and mask {seg.shape} must be one 3-D shape")
            _same_affine(affine, _load_affine(m._get_sequence(c, s, name)), (c, s), name)
            imgs.append(img)
        return (imgs[0] if len(imgs) == 1 else np.stack(imgs)), seg, affine

    def native_plan(self, i):
        """The ``RegridPlan`` case i was put on the LPI 1 mm grid with, or None for a case without an affine: the one its
        last load made (``__getitem__`` and ``load`` leave it behind); a case not loaded yet in this process is loaded."""
        if i not in self._plans:
            self.load_regridded(i)
        return self._plans[i]

    def load_regridded(self, i):
        """-> (image, mask, plan or None): ``load_native`` put on the LPI 1 mm grid by the host ``regrid``; a case without
        an affine is returned as stored."""
        img, seg, affine = self.load_native(i)
        plan = self._plans[i] = None if affine is None else regrid_plan(affine, seg.shape)
        return (img, seg, None) if plan is None else regrid(img, seg, plan) + (plan,)

    def load(self, i):
        """-> (image f32, mask) of case i on the LPI 1 mm grid (``load_regridded``); as stored for a case without an
        affine."""
        return self.load_regridded(i)[:2]

    def __getitem__(self, i):
        return self._sample(i, True)

    def case_sample(self, i):
        """The sample of case i WITHOUT the fit (multi-view prediction): "img" is the normalised
        foreground crop (C,) + crop_shape, whatever its size, and the ground-truth boxes are taken on the cropped mask, as
        fractions of crop_shape.  Un-augmented data sets only."""
        if self.augmentations:
            raise ValueError("case_sample: the case frame is defined for the un-augmented pipeline")
        return self._sample(i, False)

    def case_boxes(self, i, fit=True):
        """-> (boxes, labels) of the un-augmented case i: those of ``self[i]`` (``fit``) or of ``case_sample(i)``, from
        the mask alone - loaded, regridded and cropped as the sample's is, without normalising the image."""
        if self.augmentations or self.patch is not None:
            raise ValueError("case_boxes: defined for the un-augmented, un-windowed pipeline")
        m = self.module
        img, seg, _ = self.load_regridded(i)
        lo, hi = foreground_box(img, m.margin)
        seg = seg[tuple(slice(a, b) for a, b in zip(lo, hi))][None]
        if fit:
            seg = resize_with_pad_or_crop(seg, m.spatial_size)
        return boxes_from_instances(seg, m.thresholds, m.segmentation_mode)

    def cropped(self, i):
        """Steps 1-3 of case i -> (image (C,) + crop_shape f32 normalised, mask (1,) + crop_shape, plan or None, crop
        origin, crop_shape, full_shape)."""
        m = self.module
        img, seg, plan = self.load_regridded(i)
        full_shape = tuple(int(v) for v in seg.shape)
        lo, hi = foreground_box(img, m.margin)
        sl = tuple(slice(a, b) for a, b in zip(lo, hi))  # crop_foreground
        img, seg = img[(slice(None),) * (img.ndim - 3) + sl], seg[sl]
        crop_shape = tuple(int(b - a) for a, b in zip(lo, hi))
        # patch training: the device route's arithmetic, so that both routes train on the same bits
        norm = normalize_nonzero if getattr(m, "patch_size", None) is None else normalize_nonzero_device
        if img.ndim == 3:
            img = norm(img)[None]  # add_channel
        else:
            img = np.stack([norm(ch) for ch in img])  # channel_wise: each sequence on its own scale
        return img, seg[None], plan, lo, crop_shape, full_shape

    def crop_shape(self, i):
        """The shape of case i's foreground crop (the case is loaded for it)."""
        lo, hi = foreground_box(self.load(i)[0], self.module.margin)
        return tuple(int(b - a) for a, b in zip(lo, hi))

    def _sample(self, i, fit, origin=None, cropped=None):
        """``origin``: window the un-augmented case there at the module's patch size instead of fitting it (a validation
        tile of patch training); ``cropped``: the case's ``cropped(i)`` where the caller holds it already."""
        m = self.module
        img, seg, plan, lo, crop_shape, full_shape = self.cropped(i) if cropped is None else cropped
        patch = self.patch if origin is None else m.patch_size
        centres = None
        if patch is not None and origin is None:  # on the cropped mask, before it moves
            centres = lesion_centres(seg, m.thresholds, m.segmentation_mode)
        rs = self.sample_rng(i) if self.augmentations or centres is not None else None
        mr = []  # drawn in list order, applied to the finished sample (the device route runs them on the built batch)
        paste = None  # lesionpaste's draw: applied there too, in front of the MR transforms
        for t in self.augmentations:
            name, kw = (t, {}) if isinstance(t, str) else t
            if name in MR_NAMES:
                mr.append((name, DRAWS[name](rs, **kw), kw))
                continue
            if name == PASTE_NAME:
                paste = DRAWS[name](rs, **kw)
                continue
            img, seg = AUGMENTATIONS[name](img, seg, rs, **kw)
        if centres is not None:
            # the window's draws follow every augmentation draw: a sample's augmentation does not depend on patch mode
            from .devicedata import sample_params  # (devicedata imports this module)
            draws = draw_augmentations(self.augmentations, self.sample_rng(i))
            perm, stages = sample_params(draws, crop_shape, self.augmentations, ragged=True)
            origin = patch_origin(rs, img.shape[1:], patch, centres_to_augmented(centres, crop_shape, perm, stages),
                                  m.patch_foreground)
        if origin is not None:
            img, seg = window(img, origin, patch), window(seg, origin, patch)
        elif fit:
            img, seg = resize_with_pad_or_crop(img, m.spatial_size), resize_with_pad_or_crop(seg, m.spatial_size)
        report = None
        if self.paste_kw is not None:
            if self.bank is None:
                raise ValueError(f"{PASTE_NAME}: no lesion bank (LesionsDataModule.setup builds it)")
            rows = lower_pastes(paste, self.bank, i, img.shape[1:], m.thresholds, m.segmentation_mode,
                                self.paste_kw["max_lesions"], self.paste_kw["candidates"])
            report = [-2] * len(rows)
            if paste is not None:  # in place, on copies of its own: the fit / window may have returned views of the case
                img, seg = np.array(img, dtype=np.float32, order="C"), np.array(seg, order="C")
                report = paste_lesions(img, seg, rows, self.donors)
        for name, draw, kw in mr:
            img = apply_mr(name, img, draw, kw)
        img = np.ascontiguousarray(img)
        boxes, labels = boxes_from_instances(seg, m.thresholds, m.segmentation_mode)
        out = {"img": torch.from_numpy(img), "boxes": boxes, "labels": labels, "seg": [boxes, labels],
               "subject": self.subjects[i], "img_meta_dict": {"affine": np.eye(4)}, "seg_meta_dict": {},
               "img_transforms": [], "seg_transforms": [],
               # the geometry fit_to_case_frame needs: the crop's lo and shape, the case's shape
               "crop_origin": lo, "crop_shape": crop_shape, "full_shape": full_shape}
        if origin is not None:  # of the window, in the (augmented) cropped case's voxels
            out["patch_origin"] = tuple(int(v) for v in origin)
        if report is not None:  # per paste row: the accepted candidate, -1 none, -2 inactive or refused
            out["paste_report"] = report
        if plan is not None:  # a case with an affine: full_shape is the regridded shape, the stored one rides along
            out["img_meta_dict"] = {"affine": plan.out_affine}
            out["native_shape"] = tuple(plan.src_shape)
        return out


class _LesionTiles(Dataset):
    """The validation set of patch training: case-major, tile-minor, the unflipped tiles of ``view_plan(crop_shape, patch,
    margin)`` of every case of an un-augmented ``_LesionCases`` - the windows ``predict.py --views tiles`` shows the
    network.  A sample is the case windowed at the tile's origin, with the boxes of the windowed mask.  ``tiles`` lists
    (case position, origin); it needs every case's crop shape, so the first use loads each case once.  The last case
    prepared is kept, so walking the tiles in order prepares every case once more, not once per tile."""

    def __init__(self, cases, patch, margin):
        self.cases, self.patch, self.margin = cases, tuple(patch), tuple(margin)
        self._tiles, self._held = None, (None, None)

    @property
    def tiles(self):
        if self._tiles is None:
            self._tiles = [(i, tuple(int(v) for v in row[:3])) for i in range(len(self.cases))
                           for row in view_plan(self.cases.crop_shape(i), self.patch, self.margin)]
        return self._tiles

    def __len__(self):
        return len(self.tiles)

    def __getitem__(self, k):
        i, origin = self.tiles[k]
        if self._held[0] != i:
            self._held = (i, self.cases.cropped(i))
        return self.cases._sample(i, False, origin=origin, cropped=self._held[1])


class LesionsDataModule(ExampleDataset):
    """datasets.py:125-335 surface, the ``ExampleDataset`` way: ``setup(stage)``, ``set_epoch``, ``train_dataloader()``,
    ``test_dataloader()``, ``predict_dataloader()``, ``train_dataset`` / ``test_dataset`` / ``predict_dataset``.

    Files follow the reference's BIDS layout (``_get_data_dir`` / ``_get_sequence``) and are read through ``_load``
    (``.npy`` first, ``.nii.gz`` with nibabel).  Subjects are the sorted (center, subject) pairs (the reference's
    ``os.listdir`` order is not portable), split 80 / 20 by ``train_test_split(random_state)``.  A segmentation name
    with "labeled" in it is instance-labelled ('instances' mode, thresholds [(1, inf)] for one class and
    [(1000, 2000), (2000, inf)] for two); any other name is a binary mask ('binary' mode, one class).

    ``input_images`` names 1 .. 4 sequences (the stem's limit); the reference refuses more than one
    (datasets.py:155-156), so the multi-sequence contract is this one: samples are (C,) + spatial_size in
    ``input_images`` order; the foreground crop is the union of the channels' positive voxels (CropForegroundd with
    channel_indices=None); and - a deviation from the reference's transform, which would pool the channels - each
    sequence is normalised over its OWN non-zero voxels (NormalizeIntensity(channel_wise=True)): the mean and deviation of
    two MR contrasts pooled describe neither.  At C = 1 both rules are the reference's.  With C > 1 every name must be an
    MR sequence ``_get_sequence`` knows (anything else would be looked up among the lesion masks): NotImplementedError.

    ``orientation`` / ``spacing``: a stored volume ``PATH.npy`` may have a sidecar ``PATH.affine.npy`` (4 x 4 f64, voxel ->
    world, RAS+ mm; ``img.affine`` for ``.nii.gz``); such a case is reoriented to LPI and resampled to 1 mm by the
    axis-aligned ``regrid_plan`` / ``regrid`` (bilinear image, nearest mask) in front of the crop, its samples carry the
    regridded grid's affine and ``native_shape``, and ``full_shape`` is the regridded shape.  A case without an affine is
    taken as already LPI at 1 mm.  Left out: ``fold`` (the reference indexes a list with an index array there and cannot
    run) and the rotational resampling of oblique acquisitions (the obliquity is kept).  Not in the reference:
    ``spatial_size`` (its fixed (250, 300, 300)), ``rank`` / ``world_size`` (this process's data-parallel shard).

    ``patch_size`` (patch training; not in the reference): every training sample is one window
    of that size of the cropped, normalised, augmented case at ``patch_origin`` (with probability ``patch_foreground`` on
    a lesion, else uniform) instead of the fit, and carries "patch_origin"; a lesion the window cuts is labelled by its
    visible part, as the fit's crop labels it.  The validation set becomes ``_LesionTiles``: the un-augmented tiles of
    ``view_plan(crop_shape, patch_size, tile_margin)`` of every validation case.  ``spatial_size`` is then not used (the
    prediction data set still fits to it).  Cases are normalised by ``normalize_nonzero_device``, the arithmetic of the
    device route, so ``-c 0`` and ``-c 1`` train on the same bits.  The augmentation list must be in the order ``devicedata.sample_params``
    takes (the lesion centres follow the sample through its parameters)."""

    margin = 5  # crop_foreground
    SEQUENCES = ("FLAIR", "acq-phase_T2star", "acq-mag_T2star")  # the images of _get_sequence; other names are masks

    def __init__(self, data_dir="../data/raw", centers=("CHUV_RIM_OK", "BASEL_INSIDER_OK"), input_images=("FLAIR",),
                 segmentation="labeled_lesions", classes=("lesion",), registration="T2star", skullstripped=True,
                 augmentations=None, subject=None, batch_size=8, percentage=1., num_workers=0, random_state=970205,
                 cache=False, spatial_size=(250, 300, 300), rank=0, world_size=1, patch_size=None, patch_foreground=0.67,
                 tile_margin=(8, 8, 8)):
        input_images = (input_images,) if isinstance(input_images, str) else tuple(input_images)
        if not 1 <= len(input_images) <= 4:
            raise ValueError(f"1 .. 4 input sequences (the stem's limit), got {len(input_images)}: {input_images}")
        if len(set(input_images)) != len(input_images):
            raise ValueError(f"duplicate input sequences: {input_images}")
        unknown = [n for n in input_images if n not in self.SEQUENCES]
        if len(input_images) > 1 and unknown:
            raise NotImplementedError(f"input sequence(s) {unknown} are not among the MR sequences {self.SEQUENCES} whose "
                                      f"files _get_sequence locates")
        self.data_dir, self.centers, self.registration = data_dir, tuple(centers), registration
        self.input_images, self.segmentation, self.skullstripped = tuple(input_images), segmentation, skullstripped
        self.classes, self.n_classes = tuple(classes), len(classes)
        self.batch_size, self.num_workers, self.random_state = batch_size, num_workers, random_state
        self.augmentations, self.subject, self.percentage, self.cache = augmentations, subject, percentage, cache
        self.spatial_size = tuple(int(t) for t in spatial_size)
        if len(self.spatial_size) != 3 or min(self.spatial_size) <= 0:
            raise ValueError(f"spatial_size must be three positive sizes, got {spatial_size}")
        self.patch_size = None if patch_size is None else tuple(int(t) for t in patch_size)
        self.patch_foreground, self.tile_margin = float(patch_foreground), tuple(int(v) for v in tile_margin)
        if self.patch_size is not None and (len(self.patch_size) != 3 or min(self.patch_size) <= 0):
            raise ValueError(f"patch_size must be three positive sizes, got {patch_size}")
        if not 0.0 <= self.patch_foreground <= 1.0:
            raise ValueError(f"patch_foreground is a probability, got {patch_foreground}")
        if len(self.tile_margin) != 3 or min(self.tile_margin) < 0:
            raise ValueError(f"tile_margin must be three margins >= 0, got {tile_margin}")
        self.rank, self.world_size, self.epoch = rank, world_size, 0
        self.segmentation_mode = "instances" if "labeled" in segmentation else "binary"
        if self.segmentation_mode == "binary":
            if self.n_classes != 1:
                raise ValueError("a binary mask carries one class")
            self.thresholds = [(1, np.inf)]
        elif self.n_classes == 1:
            self.thresholds = [(1, np.inf)]
        elif self.n_classes == 2:
            self.thresholds = [(1000, 2000), (2000, np.inf)]
        else:
            raise ValueError(f"one or two classes, got {self.n_classes}")
        subs = []
        for c in self.centers:
            subs += [(c, s.replace("sub-", "")) for s in os.listdir(self._get_data_dir(c)) if "sub-" in s]
        subs = sorted(subs)
        self.subjects_list = subs[:int(percentage * len(subs))] if percentage > 0 else subs
        self.train_dataset = self.test_dataset = self.predict_dataset = None

    def _get_data_dir(self, center):
        """The BIDS directory of a center (datasets.py:238-243)."""
        dd = pjoin(self.data_dir, center)
        if self.registration is not None:
            dd = pjoin(dd, "derivatives", "registrations", f"registrations_to_{self.registration}")
        return dd

    def _get_sequence(self, center, subject, img_name):
        """Path of an image or a segmentation without its extension (datasets.py:245-259)."""
        if img_name in self.SEQUENCES:
            if not self.skullstripped:
                return pjoin(self._get_data_dir(center), f"sub-{subject}", "ses-01", "anat",
                             f"sub-{subject}_ses-01_{img_name}")
            return pjoin(self._get_data_dir(center), "derivatives", "skullstripped", f"sub-{subject}", "ses-01",
                         f"sub-{subject}_ses-01_{img_name}")
        return pjoin(self._get_data_dir(center), "derivatives", "lesionmasks", f"sub-{subject}", "ses-01",
                     f"sub-{subject}_ses-01_{img_name}")

    def setup(self, stage=None):
        from sklearn.model_selection import train_test_split
        if self.subject is not None:
            one = tuple(self.subject) if not isinstance(self.subject, str) else \
                next(cs for cs in self.subjects_list if cs[1] == self.subject)
            train, test = [one], [one]
        else:
            train, test = train_test_split(self.subjects_list, train_size=0.8, test_size=0.2,
                                           random_state=self.random_state)
        self.train_dataset = _LesionCases(self, train, self.augmentations, self.random_state, patch=self.patch_size)
        if self.train_dataset.paste_kw is not None:  # lesionpaste: the bank, once, over the training cases (every rank's)
            self.train_dataset.build_bank()
        self.test_dataset = _LesionCases(self, test)
        if self.patch_size is not None:
            self.test_dataset = _LesionTiles(self.test_dataset, self.patch_size, self.tile_margin)
        self.predict_dataset = _LesionCases(self, train if stage == "predict_train" else test)
