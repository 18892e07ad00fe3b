"""Device-resident training data (``train.py -c 1``; the reference's ``-c/--cache``, MONAI ``CacheDataset``): the cases
are loaded and normalised ONCE into HBM, and every batch is gathered, augmented, labelled into boxes and packed into
``FusedTrainer.step_packed``'s target layout on the device (csrc/datapipe.hip).  Host mirror: ``datasets._Cases`` and
``datasets.boxes_from_segmentation``; the per-sample random draws are the host's own (``datasets.draw_augmentations``
on ``datasets.sample_rng``), so a batch holds the same subjects, the same masks and bit-identical boxes as the host
loader's, and images within the normalisation bound of DESIGN.md §4.7.  Against the host transforms applied to the
CACHED (device-normalised) volume the images are bit-identical too: every resample restates scipy's arithmetic and the
intensity operations are single f32 roundings.

Limits: rot90 on an axis pair of unequal sizes (a shape-changing rotation) raises NotImplementedError.  The supported
order is the reference's - flips / rot90s, then affines, then shiftintensity / scaleintensity: a flip / rot90 placed
after an affine stage or an intensity operation, an affine placed after an intensity operation and more than
AFFINE_MAX_OPS intensity operations raise NotImplementedError.

``LesionCache`` is the counterpart for ``datasets.LesionsDataModule``: cases of unequal shape, cropped to their
foreground, in one flat arena; shape-changing rot90s allowed; every batch padded / cropped to one fixed size and its
instance-labelled masks turned into boxes (msl_foreground_box_mc, msl_augment_fit_mc, msl_instance_boxes); binary masks
(``segmentation_mode == "binary"``) are labelled per batch by msl_binary_boxes instead.  A module with
C > 1 input sequences is cached channel-planar; every C, one sequence included, goes through the same entry points.  A case that
carries an affine is uploaded on its native grid and put on the LPI 1 mm grid by msl_regrid (``regrid_device``, the
device form of ``datasets.regrid``, bit for bit) in front of the foreground box.  A module with a ``patch_size`` (patch
training) gets one sampled window per case and epoch instead of the fit, and validation tiles
(msl_augment_window_mc with the origins ``datasets.patch_origin`` / ``datasets.view_plan`` give on the host).  A batch in
which some sample drew a zoom / griddistortion (a ``WarpStage``: three per-axis coordinate tables, DESIGN.md section
4.13) goes through msl_augment_warp_mc instead, on either route; ``DeviceCache`` refuses the two names.  A batch in
which some sample drew an elastic3d (a ``DeformStage``: a cubic B-spline lattice) goes through
msl_augment_deform_mc in the same way.  An augmentation
list that names gaussiansmooth / biasfield / gaussiannoise (the MR stage) adds msl_augment_mr
(csrc/mraug.hip) behind the batch build of either cache: ``mr_tables`` lowers the draws, ``MRStageRunner`` launches.
A list that names lesionpaste adds msl_paste_lesions (csrc/lesionpaste.hip) between the two on
``LesionCache``: copy-paste of lesions of the cached training cases, lowered to integer rows by ``datasets.lower_pastes``.
"""
from collections import namedtuple

import numpy as np
import torch
from os.path import join as pjoin

from . import _lib
from ._lib import ptr
from .datasets import (MR_MAX_RADIUS, MR_NAMES, PASTE_AUGMENTATIONS, PASTE_HEAD, PASTE_NAME, SCIPY_BOUNDARY, ShardSampler,
                       _load, affine_matrix, affine_offset, bank_from_lesions, bias_lattice, centres_to_augmented,
                       check_lesionpaste, deform_coords, deform_lattice, draw_augmentations, gaussian_taps, lower_pastes,
                       patch_origin, regrid_plan, sample_rng, transform_name, view_plan, warp_tables)

PARAM_STRIDE = 16  # f64 per sample of msl_augment_resample
AFFINE_STRIDE = 32  # f64 per sample of msl_augment_affine
AFFINE_MAX_OPS = 4  # intensity operations one msl_augment_affine row carries
BOUNDARY = {"reflection": 0, "border": 1, "zeros": 2}  # msl_augment_affine's code of a padding_mode
OP_ADD, OP_MUL = 1, 2
NEAREST_UNCLAMPED = 3  # affine_numpy only: the boundary rule of msl_regrid (scipy's "nearest", exactly)

# a stage msl_augment_affine runs: dense matrix / offset (f64, as the host computed them) and the boundary code
AffineStage = namedtuple("AffineStage", "matrix offset boundary")
# kind (OP_ADD / OP_MUL) and the np.float32 operand of the host's one f32 operation
IntensityOp = namedtuple("IntensityOp", "kind value")
# a stage msl_augment_warp_mc runs (zoom / griddistortion): three f64 coordinate tables, one per axis of the permuted
# case (output voxel q samples at t_a[q_a]), and the boundary code
WarpStage = namedtuple("WarpStage", "tables boundary")
WARP_NAMES = ("zoom", "griddistortion")
# a stage msl_augment_deform_mc runs (elastic3d): the (3, L, L, L) f64 lattice of ``datasets.deform_lattice`` for the
# permuted case (output voxel q samples at q + d(q)) and the boundary code
DeformStage = namedtuple("DeformStage", "lattice boundary")
DEFORM_NAMES = ("elastic3d",)
ROW_COPY, ROW_AFFINE, ROW_WARP, ROW_DEFORM = 0.0, 1.0, 2.0, 3.0  # field [7] of a parameter row
# The resampling transforms, by name: the stage type a drawn one becomes, ``fields(draw, permuted shape, kw)`` -> that
# stage's fields in front of the boundary, the default padding mode, what ``sample_params``'s order error calls it, and
# whether only the ragged cache runs it
_Resampler = namedtuple("_Resampler", "stage fields pad what ragged_only")
RESAMPLERS = {"affine": _Resampler(AffineStage, lambda d, shape, kw: affine_matrix(shape, *d), "reflection",
                                   "an affine stage", False),
              "zoom": _Resampler(WarpStage, lambda d, shape, kw: (warp_tables("zoom", d, shape, kw),), "border",
                                 "a warp stage", True),
              "griddistortion": _Resampler(WarpStage, lambda d, shape, kw: (warp_tables("griddistortion", d, shape, kw),),
                                           "border", "a warp stage", True),
              "elastic3d": _Resampler(DeformStage,
                                      lambda d, shape, kw: (deform_lattice(shape, d, kw.get("max_displacement", 7.5)),),
                                      "border", "a deformation stage", True)}
assert all((RESAMPLERS[n].stage is WarpStage) == (n in WARP_NAMES) and (RESAMPLERS[n].stage is DeformStage) == (n in DEFORM_NAMES)
           for n in RESAMPLERS)


def _example_cache_refusal(name):
    """The error of a ragged-only transform on the example cache: it names every transform of that stage type."""
    kin = [n for n, rs in RESAMPLERS.items() if rs.stage is RESAMPLERS[name].stage]
    return NotImplementedError(f"device pipeline: {' / '.join(kin)} on the example cache")


def transform_kw(t):
    """The keyword arguments of an augmentation list's entry (``datasets.transform_name``'s counterpart)."""
    return {} if isinstance(t, str) else t[1]
# an MR transform of the augmentation list (gaussiansmooth / biasfield / gaussiannoise): its name,
# its draw (``datasets.DRAWS[name]``'s result; None: not drawn) and its keyword arguments.  msl_augment_mr runs them on
# the built batch; the batch build itself does not see them
MRStage = namedtuple("MRStage", "name draw kw")
MR_STRIDE = 8  # f64 per sample of msl_augment_mr
MR_TAPS = 2 * MR_MAX_RADIUS + 1  # f32 per axis of its taps table
MR_LATTICE = 9  # points per axis of its lattice table
MR_BLUR, MR_BIAS, MR_NOISE = 1, 2, 4  # bits of field [0] of its parameter row
# lesionpaste of the augmentation list: its draw (``datasets._draw_lesionpaste``'s result; None: not
# applied) and its keyword arguments.  msl_paste_lesions runs it on the built batch in front of the MR stage; like an
# ``MRStage`` it moves no point and the batch build does not see it
PasteStage = namedtuple("PasteStage", "draw kw")
POST_STAGES = (MRStage, PasteStage)  # what runs on the built batch


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


class _BoxStage:
    """Packed targets + workspace of one box entry point for (N,) + shape masks and ``capacity`` rows.  Every entry
    point takes (mask, N, D, H, W, its own arguments, workspace, workspace bytes, gb, gl, obj_off, flag, stream); a
    subclass names it (``entry``), sizes its workspace, and supplies ``_args()`` (those own arguments) and ``_errors()``
    ([(flag bit, message)] in the order the bits are tested)."""

    def __init__(self, N, shape, capacity, dev, nbytes, unsupported):
        """``nbytes``: the entry point's workspace size, 0 for sizes it refuses (``unsupported`` says which)."""
        self.N, self.shape, self.capacity = N, tuple(shape), capacity
        if nbytes == 0:
            raise _lib.HipKernelError(f"{self.entry}: unsupported {unsupported}")
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.gb = torch.zeros((max(capacity, 1), 6), dtype=torch.float32, device=dev)
        self.gl = torch.ones(max(capacity, 1), dtype=torch.int64, device=dev)
        self.obj_off = torch.zeros(N + 1, dtype=torch.int32, device=dev)
        self.flag = torch.zeros(1, dtype=torch.int32, device=dev)
        self.flag_host = torch.zeros(1, dtype=torch.int32, pin_memory=True)

    def launch(self, seg, stream):
        _lib.call(self.entry, ptr(seg), self.N, *self.shape, *self._args(), ptr(self.ws), self.ws.numel(), ptr(self.gb),
                  ptr(self.gl), ptr(self.obj_off), ptr(self.flag), stream)
        self.flag_host.copy_(self.flag, non_blocking=True)  # read after the next synchronising read: no sync of its own

    def raise_on_overflow(self, flag=None):
        f = int(self.flag_host.item() if flag is None else flag)
        for bit, message in self._errors() if f else ():
            if f & bit:
                raise _lib.HipKernelError(f"{self.entry}: {message}")

    def boxes(self, seg):
        """Launch on ``seg`` -> (boxes list, labels list, (gb, gl, obj_off, capacity)): per-image device views and the
        packed form.  One host synchronisation (obj_off); the flag is read behind it."""
        self.launch(seg, _stream(seg.device))
        off = self.obj_off.cpu().tolist()
        self.raise_on_overflow(self.flag.item())
        return ([self.gb[off[n]:off[n + 1]] for n in range(self.N)], [self.gl[off[n]:off[n + 1]] for n in range(self.N)],
                (self.gb, self.gl, self.obj_off, self.capacity))


class _BoxOut(_BoxStage):
    """``_BoxStage`` of msl_seg_boxes for one (N, D, H, W, n_classes, capacity)."""

    entry = "msl_seg_boxes"

    def __init__(self, N, shape, n_classes, capacity, comp_cap, dev):
        self.n_classes, self.comp_cap = n_classes, comp_cap
        nbytes = _lib.load().msl_seg_boxes_workspace_bytes(N, *shape, n_classes, comp_cap)
        super().__init__(N, shape, capacity, dev, nbytes, f"sizes N={N} shape={tuple(shape)} n_classes={n_classes}")

    def _args(self):
        return self.n_classes, self.capacity, self.comp_cap

    def _errors(self):
        return [(1, f"a batch holds more ground-truth boxes than the capacity of {self.capacity} rows"),
                (2, f"a batch holds more connected components than comp_cap = {self.comp_cap}")]


def _default_comp_cap(capacity):
    return max(65536, 4 * capacity)


def boxes_from_segmentation_device(seg, n_classes=1, capacity=None, comp_cap=None):
    """``datasets.boxes_from_segmentation`` for every image of a device uint8 (N, 1, D, H, W) or (N, D, H, W) mask.

    -> (boxes list[(n_i, 6) f32], labels list[(n_i,) i64], (gb, gl, obj_off, capacity)): the per-image lists the host
    function returns (device views) and the packed form ``msl_multibox_match`` reads.  Default capacity: 1024 rows per
    image.  More boxes than the capacity raise HipKernelError.  One host synchronisation (obj_off)."""
    if not seg.is_cuda or seg.dtype != torch.uint8:
        raise _lib.HipKernelError("boxes_from_segmentation_device takes a uint8 tensor on the HIP device")
    if seg.dim() == 5:
        if seg.shape[1] != 1:
            raise ValueError(f"one mask channel expected, got {seg.shape[1]}")
        seg = seg[:, 0]
    if seg.dim() != 4:
        raise ValueError(f"(N, 1, D, H, W) or (N, D, H, W) expected, got {tuple(seg.shape)}")
    seg = seg.contiguous()
    N = seg.shape[0]
    capacity = 1024 * N if capacity is None else int(capacity)
    return _BoxOut(N, seg.shape[1:], int(n_classes), capacity, comp_cap or _default_comp_cap(capacity),
                   seg.device).boxes(seg)


def sample_params(draws, shape, augmentations=None, ragged=False):
    """One sample's draws (``datasets.draw_augmentations``) -> (signed axis permutation, [stages]).

    The permutation is (axis, rev): output axis a reads source axis axis[a], reversed iff rev[a]; it composes the flips
    and rot90s exactly as np.flip / np.rot90 index.  ``augmentations`` is the transform list the draws were made from (it
    holds each affine's ``padding_mode``; without it, reflection).  There is one stage per affine / intensity entry, in
    list order: None (not drawn), (zoom, offset) in f64 for a diagonal affine with reflection padding (the stage
    msl_augment_resample runs), ``AffineStage`` for a rotating affine or another boundary, ``IntensityOp``.
    ``ragged`` (msl_augment_fit): a rot90 may change the shape, and every affine stage is an ``AffineStage`` computed
    for the permuted shape.  A drawn zoom / griddistortion is a ``WarpStage`` with the tables of the permuted shape
    (``ragged`` only; padding "border" unless the entry says otherwise); it is a resampling stage like an affine: behind
    the flips / rot90s, in front of the intensity operations.  A drawn elastic3d is a ``DeformStage`` with the lattice of
    the permuted shape, under the same rules.  gaussiansmooth / biasfield / gaussiannoise are the last
    group: each appends an ``MRStage`` (drawn or not), which moves no point and which the batch build skips
    (``mr_tables`` lowers them for msl_augment_mr); any other entry behind one of them raises NotImplementedError.
    lesionpaste appends a ``PasteStage`` (drawn or not) under the same terms: ``ragged`` only, once, behind every entry
    that is not an MR transform and in front of those; any other position raises NotImplementedError."""
    axis, rev = [0, 1, 2], [0, 0, 0]
    stages = []
    n_ops = 0

    def swap(a, b):
        axis[a], axis[b] = axis[b], axis[a]
        rev[a], rev[b] = rev[b], rev[a]

    n_mr = 0
    pasted = False
    for k, (name, d) in enumerate(draws):
        kw = transform_kw(augmentations[k]) if augmentations is not None else {}
        if name == PASTE_NAME:  # once, behind every other entry, in front of the MR transforms: a PasteStage, drawn or not
            if pasted or n_mr:
                raise NotImplementedError(f"device pipeline: {PASTE_NAME} once, in front of the MR transforms "
                                          f"({' / '.join(MR_NAMES)})")
            if not ragged:
                raise NotImplementedError(f"device pipeline: {PASTE_NAME} on the example cache (no lesion bank)")
            pasted = True
            stages.append(PasteStage(d, dict(PASTE_AUGMENTATIONS[0][1], **kw)))
            continue
        if pasted and name not in MR_NAMES:
            raise NotImplementedError(f"device pipeline: {name} after {PASTE_NAME} (only {' / '.join(MR_NAMES)} follow it)")
        if name in MR_NAMES:  # the last group: an MRStage each, drawn or not
            stages.append(MRStage(name, d, kw))
            if MR_NAMES.index(name) < n_mr:  # one launch carries blur, then bias, then noise
                raise NotImplementedError(f"device pipeline: {' / '.join(MR_NAMES)} once each, in that order")
            n_mr = MR_NAMES.index(name) + 1
            continue
        if n_mr:
            raise NotImplementedError(f"device pipeline: {name} after an MR transform ({' / '.join(MR_NAMES)} come last)")
        if name in RESAMPLERS:
            rs = RESAMPLERS[name]
            if n_ops:
                raise NotImplementedError(f"device pipeline: {rs.what} after an intensity operation")
            if rs.ragged_only and not ragged:
                raise _example_cache_refusal(name)
            pad = kw.get("padding_mode", rs.pad)
            if d is None:
                stages.append(None)
            elif name == "affine" and len(d) == 2 and pad == "reflection" and not ragged:
                stages.append((list(d[0]), list(affine_offset(shape, *d))))
            else:  # flips / rot90s come first: the permutation is final, and it keeps the shape unless ragged
                stages.append(rs.stage(*rs.fields(d, tuple(shape[a] for a in axis), kw), BOUNDARY[pad]))
            continue
        if name in ("shiftintensity", "scaleintensity"):
            n_ops += 1
            if n_ops > AFFINE_MAX_OPS:
                raise NotImplementedError(f"device pipeline: more than {AFFINE_MAX_OPS} intensity operations")
            if d is None:
                stages.append(None)
            elif name == "shiftintensity":
                stages.append(IntensityOp(OP_ADD, np.float32(d)))
            else:
                stages.append(IntensityOp(OP_MUL, np.float32(1.0 + d)))
            continue
        if n_ops:
            raise NotImplementedError("device pipeline: a flip / rot90 after an intensity operation")
        if stages:
            raise NotImplementedError("device pipeline: a flip / rot90 after an affine stage")  # (a warp stage counts)
        if d is None:
            continue
        if name == "flip":
            for a in d:
                rev[a] ^= 1
        else:  # np.rot90(m, k, (a, b)): k=1 transpose(flip(m, b)), k=2 flip both, k=3 flip(transpose(m), b)
            k, (a, b) = d[0] % 4, d[1]
            if not ragged and shape[axis[a]] != shape[axis[b]]:
                raise NotImplementedError(f"device pipeline: rot90 over axes {(a, b)} of sizes {shape[a]} != {shape[b]}")
            if k == 1:
                rev[b] ^= 1
                swap(a, b)
            elif k == 2:
                rev[a] ^= 1
                rev[b] ^= 1
            elif k == 3:
                swap(a, b)
                rev[b] ^= 1
    return (axis, rev), stages


def affine_row(source, perm=((0, 1, 2), (0, 0, 0)), stage=None, ops=()):
    """One msl_augment_affine parameter row (AFFINE_STRIDE f64; layout in include/mslesions3d_hip.h).  ``stage``: None, a
    (zoom, offset) pair (reflection) or an ``AffineStage``; ``ops``: the drawn ``IntensityOp``s in order."""
    if len(ops) > AFFINE_MAX_OPS:
        raise NotImplementedError(f"device pipeline: more than {AFFINE_MAX_OPS} intensity operations")
    r = np.zeros(AFFINE_STRIDE, dtype=np.float64)
    r[0], r[1:4], r[4:7] = source, perm[0], perm[1]
    if stage is not None:
        if not isinstance(stage, AffineStage):
            stage = AffineStage(np.diag(stage[0]), stage[1], BOUNDARY["reflection"])
        r[7], r[8:17], r[17:20], r[20] = 1.0, np.asarray(stage.matrix, dtype=np.float64).reshape(9), stage.offset, stage.boundary
    r[21] = len(ops)
    for k, op in enumerate(ops):
        r[22 + 2 * k], r[23 + 2 * k] = op.kind, np.float32(op.value)
    return r


def affine_numpy(vol, matrix, offset, order, boundary, output_shape=None):
    """Host mirror of msl_augment_affine's resample of one (D, H, W) volume, operation by operation in f64 (scipy 1.15's
    NI_GeometricTransform): per axis cc = 0, cc += o[k] * M[h][k] (k = 0, 1, 2), cc += offset[h]; the boundary's
    map_coordinate; order 1: taps floor(cc), floor(cc) + 1 with weights w0 = 1 - (cc - floor(cc)), w1 = 1 - w0, the eight
    corners accumulated axis 0 slowest, each as ((value * w_0) * w_1) * w_2; order 0: tap floor(cc + 0.5).  Boundary 2
    (constant) writes 0 wherever an axis maps outside [0, len - 1].  ``output_shape`` (msl_regrid, ``datasets.regrid``):
    the output grid where it is not the volume's own.  Boundary ``NEAREST_UNCLAMPED`` (3) is msl_regrid's: "nearest" as
    scipy 1.15 computes it, the taps clamped into the axis but the weights taken from the coordinate as it is, so past
    either end both taps are the end voxel with weights (1 - x, x).  Boundary 1 clamps the coordinate itself, which
    gives (1, 0) there: the same value up to the last f64 bit of the sum, and so another f32 wherever that sum is a tie
    (half-integer coordinates: a step of 0.5 or 2.5).  msl_augment_affine is boundary 1; DESIGN.md section 4.10."""
    odims = vol.shape if output_shape is None else tuple(int(n) for n in output_shape)
    o = [x.astype(np.float64) for x in np.meshgrid(*(np.arange(n) for n in odims), indexing="ij")]
    M, off = np.asarray(matrix, dtype=np.float64), np.asarray(offset, dtype=np.float64)
    coords = []
    for h in range(3):
        c = np.zeros(odims)
        for k in range(3):
            c = c + o[k] * M[h, k]
        coords.append(c + off[h])
    return _sample_numpy(vol, coords, order, boundary)


def warp_numpy(vol, tables, order, boundary):
    """Host mirror of msl_augment_warp_mc's resample of one (D, H, W) volume, operation by operation in f64: output voxel
    o has the coordinate (t_0[o_0], t_1[o_1], t_2[o_2]); from there the boundary map, the taps and the weights of
    ``affine_numpy`` (scipy 1.15's NI_GeometricTransform, which ``scipy.ndimage.map_coordinates`` runs as well).
    ``boundary`` is a ``BOUNDARY`` code; "border" (1) is computed as scipy computes "nearest", ``affine_numpy``'s
    ``NEAREST_UNCLAMPED``: a zoom's tables hold half-integer coordinates, the ties at which the clamped form of
    msl_augment_affine rounds to another f32."""
    tables = [np.asarray(t, dtype=np.float64) for t in tables]
    if tuple(t.shape for t in tables) != tuple((n,) for n in vol.shape):
        raise ValueError(f"warp_numpy: one table per axis of {vol.shape} expected, got {[t.shape for t in tables]}")
    return _sample_numpy(vol, np.meshgrid(*tables, indexing="ij"), order,
                         NEAREST_UNCLAMPED if boundary == BOUNDARY["border"] else boundary)


def deform_numpy(vol, P, order, boundary):
    """Host mirror of msl_augment_deform_mc's resample of one (D, H, W) volume, operation by operation in f64: output
    voxel q has the coordinates ``datasets.deform_coords(vol.shape, P)``; from there ``warp_numpy``'s sampling, "border"
    (1) as scipy computes "nearest"."""
    return _sample_numpy(vol, deform_coords(vol.shape, P), order,
                         NEAREST_UNCLAMPED if boundary == BOUNDARY["border"] else boundary)


def _sample_numpy(vol, coords, order, boundary):
    """The tail ``affine_numpy``, ``warp_numpy`` and ``deform_numpy`` share: ``vol`` sampled at the three f64 coordinate arrays (one output
    grid), from the boundary map on."""
    dims = vol.shape
    odims = coords[0].shape

    def reflect(c, n):
        c = np.array(c, dtype=np.float64)
        if n <= 1:
            return np.zeros_like(c)
        sz2 = 2.0 * n
        x = np.where(c < -sz2, sz2 * np.trunc(-c / sz2) + c, c)
        lo = np.where(x < -n, x + sz2, np.where(x > -1e-15, 1e-15, -x) - 1.0)
        y = c - sz2 * np.trunc(c / sz2)
        hi = np.where(y >= n, (sz2 - y) - 1.0, y)
        return np.where(c < 0, lo, np.where(c > n - 1, hi, c))

    def tap(i, n):
        m = reflect(i, n) if boundary == 0 else i
        return np.clip(np.where((i >= 0) & (i < n), i, np.trunc(m)), 0, n - 1).astype(np.int64)

    cc, outside = [], np.zeros(odims, dtype=bool)
    for h in range(3):
        c = coords[h]
        n = dims[h]
        if boundary == 0:
            c = reflect(c, n)
        elif boundary == NEAREST_UNCLAMPED:
            pass
        elif boundary == 1:
            c = np.where(c < 0, 0.0, np.where(c > n - 1, float(n - 1), c))
        else:
            outside |= (c < 0) | (c > n - 1)
            c = np.where((c < 0) | (c > n - 1), -1.0, c)
        cc.append(c)
    if order == 0:
        out = vol[tuple(tap(np.floor(c + 0.5), n) for c, n in zip(cc, dims))]
        return np.where(outside, 0, out).astype(vol.dtype)
    idx, w = [], []
    for c, n in zip(cc, dims):
        fl = np.floor(c)
        w0 = 1.0 - (c - fl)
        w.append((w0, 1.0 - w0))
        idx.append((tap(fl, n), tap(fl + 1, n)))
    t = np.zeros(odims)
    for a in range(2):
        for b in range(2):
            for d in range(2):
                coeff = vol[idx[0][a], idx[1][b], idx[2][d]].astype(np.float64)
                coeff = coeff * w[0][a]
                coeff = coeff * w[1][b]
                coeff = coeff * w[2][d]
                t = t + coeff
    return np.where(outside, 0.0, t).astype(np.float32)


def batch_launches(slots, per_sample):
    """-> [(entry point, (N, stride) f64 rows)]: one launch per affine stage some sample of the batch drew (a resample
    of a resample is not one resample), or one plain gather.  The first launch reads the cache through the sample's
    permutation; the last one carries the intensity operations.  A launch whose stages are all diagonal with
    reflection padding and that carries no operation stays on msl_augment_resample."""
    N = len(slots)
    geo = [[st for st in stages if not isinstance(st, (IntensityOp,) + POST_STAGES)] for _, stages in per_sample]
    ops = [[st for st in stages if isinstance(st, IntensityOp)] for _, stages in per_sample]
    n_geo = max((len(g) for g in geo), default=0)
    used = [j for j in range(n_geo) if any(j < len(g) and g[j] is not None for g in geo)] or [None]
    out = []
    for k, j in enumerate(used):
        first, last = k == 0, k == len(used) - 1
        st = [g[j] if j is not None and j < len(g) else None for g in geo]
        dense = any(isinstance(x, AffineStage) for x in st) or (last and any(ops))
        rows = np.zeros((N, AFFINE_STRIDE if dense else PARAM_STRIDE), dtype=np.float64)
        for n in range(N):
            src = slots[n] if first else n
            perm = per_sample[n][0] if first else ((0, 1, 2), (0, 0, 0))
            if dense:
                rows[n] = affine_row(src, perm, st[n], ops[n] if last else ())
            else:
                rows[n, 0], rows[n, 1:4], rows[n, 4:7] = src, perm[0], perm[1]
                if st[n] is not None:
                    rows[n, 7], rows[n, 8:11], rows[n, 11:14] = 1.0, st[n][0], st[n][1]
        out.append(("msl_augment_affine" if dense else "msl_augment_resample", rows))
    return out


def train_batch_order(dataset, epoch):
    """The index chunks of ``dataset.train_dataloader()`` in ``epoch``: ShardSampler order of this rank, batch_size
    chunks, the last one short (drop_last=False)."""
    sampler = ShardSampler(len(dataset.train_dataset), dataset.rank, dataset.world_size, True, dataset.random_state)
    sampler.set_epoch(epoch)
    order = sampler.indices().tolist()
    return [order[i:i + dataset.batch_size] for i in range(0, len(order), dataset.batch_size)]


def permute_numpy(vol, perm):
    """Host form of the kernel's gather: out[q] = vol[s] with s[axis[a]] = rev[a] ? n - 1 - q[a] : q[a]."""
    axis, rev = perm
    out = np.transpose(vol, axis)  # out axis a <- source axis axis[a]
    flip = tuple(a for a in range(3) if rev[a])
    return np.flip(out, flip) if flip else out


# ---- what the two caches share: free functions on a batch's buffer set b and its sample_params results ----------------
def _drew_mr(per_sample):
    """Does the batch carry MR draws?  (Validation batches carry none.)  msl_augment_mr runs behind the build of a batch
    that does and whose buffer set has the stage ("mr" in b: the list names an MR transform)."""
    return any(isinstance(st, MRStage) for _, stages in per_sample for st in stages)


def _batch_nbytes(b):
    """Device bytes of one batch buffer set."""
    n = sum(t.numel() * t.element_size() for t in (b["img"], b["seg"], *b.get("tmp", ()), b["box"].ws, b["box"].gb,
                                                    b["box"].gl))
    return n + (b["built"].numel() * 4 + b["mr"].ws.numel() if "mr" in b else 0)


def _val_batch(b, subjects):
    """The ``validation_step`` batch of a launched buffer set: one host synchronisation (obj_off, the flag behind it),
    the image and the per-image box lists cloned out of the fixed buffers.  The callers add their geometry keys."""
    box = b["box"]
    off = box.obj_off.cpu().tolist()
    box.raise_on_overflow(box.flag.item())
    boxes = [box.gb[off[n]:off[n + 1]].clone() for n in range(len(subjects))]
    labels = [box.gl[off[n]:off[n + 1]].clone() for n in range(len(subjects))]
    return {"img": b["img"].clone(), "seg": [boxes, labels], "boxes": boxes, "labels": labels, "subject": list(subjects)}


class DeviceCache:
    """The cases of a ``setup()`` ``ExampleDataset`` in HBM (image f32 normalised, mask u8), and the device pipeline that
    turns them into training / validation batches.

    ``train_batches(epoch)`` yields the batches of ``dataset.train_dataloader()`` for that epoch (same ShardSampler order,
    same chunks, same per-sample draws) as dicts {"img", "seg", "gb", "gl", "obj_off", "capacity", "subject"}: the
    tensors are FIXED buffers, one set per batch shape, rewritten by the next batch.  Feed them to ``step(trainer, batch)``
    (``FusedTrainer.step_packed(..., resident=True)`` with total_objects = capacity: one recorded launch program per
    shape).  ``val_batches()`` yields ``validation_step`` batches of this rank's validation shard, without augmentation."""

    def __init__(self, dataset, device, max_objects_per_image=64, comp_cap=None):
        if dataset.train_dataset is None:
            raise ValueError("DeviceCache needs a dataset after setup()")
        self.dataset, self.device = dataset, torch.device(device)
        self.n_classes, self.batch_size = int(dataset.n_classes), int(dataset.batch_size)
        self.augmentations = list(dataset.train_dataset.augmentations)
        names = [transform_name(t) for t in self.augmentations]
        refused = [n for n, rs in RESAMPLERS.items() if rs.ragged_only and n in names]
        if refused:  # before anything is loaded
            raise _example_cache_refusal(refused[0])
        tr, te = dataset.train_dataset, dataset.test_dataset
        if dataset.world_size > 1:
            val_idx = ShardSampler(len(te), dataset.rank, dataset.world_size, False, dataset.random_state).indices()
        else:
            val_idx = np.arange(len(te))
        # every rank may draw any training case in a later epoch; validation shards are fixed
        keys = [(tr.root, s) for s in tr.subjects] + [(te.root, te.subjects[i]) for i in val_idx]
        self.slot = {}
        for k in keys:
            self.slot.setdefault(k, len(self.slot))
        self.train_slots = [self.slot[(tr.root, s)] for s in tr.subjects]
        self.val_order = [(te.subjects[i], self.slot[(te.root, te.subjects[i])]) for i in val_idx]
        cases = list(self.slot)
        first = _load(pjoin(cases[0][0], "images", f"sub-{cases[0][1]}_image"))
        self.shape = tuple(first.shape)
        if len(self.shape) != 3:
            raise ValueError(f"DeviceCache: 3-D volumes expected, got shape {self.shape}")
        V = int(np.prod(self.shape))
        self.cache_bytes = len(cases) * V * 5
        free, _ = torch.cuda.mem_get_info(self.device)
        if self.cache_bytes > 0.8 * free:
            raise MemoryError(f"DeviceCache: {len(cases)} cases of {self.shape} need {self.cache_bytes / 2**30:.2f} GiB, "
                              f"{free / 2**30:.2f} GiB free on {self.device}")
        self.img = torch.empty((len(cases),) + self.shape, dtype=torch.float32, device=self.device)
        self.seg = torch.empty((len(cases),) + self.shape, dtype=torch.uint8, device=self.device)
        for k, (root, s) in enumerate(cases):
            img = _load(pjoin(root, "images", f"sub-{s}_image")).astype(np.float32)
            seg = np.asarray(_load(pjoin(root, "labels", f"sub-{s}_seg")))
            if img.shape != self.shape or seg.shape != self.shape:
                raise ValueError(f"DeviceCache: case {s} has shape {img.shape} / {seg.shape}, the first case "
                                 f"{self.shape}: every cached case must have the same shape")
            seg8 = seg.astype(np.uint8)
            if not np.array_equal(seg8, seg):
                raise ValueError(f"DeviceCache: mask of case {s} is not integer-valued in [0, 255]")
            self.img[k].copy_(torch.from_numpy(img))
            self.seg[k].copy_(torch.from_numpy(seg8))
        _lib.call("msl_normalize_nonzero", ptr(self.img), len(cases), V, _stream(self.device))
        self.capacity = int(max_objects_per_image) * self.batch_size
        self.comp_cap = comp_cap or _default_comp_cap(self.capacity)
        self._bufs = {}
        for t in self.augmentations:
            if transform_name(t) == "rotate90":
                a, b = transform_kw(t).get("spatial_axes", (0, 1))
                if self.shape[a] != self.shape[b]:
                    raise NotImplementedError(f"device pipeline: rot90 over axes {(a, b)} of sizes "
                                              f"{self.shape[a]} != {self.shape[b]} changes the volume's shape")
        self.n_affine = names.count("affine")
        # the order limits of sample_params hold for the list itself, drawn or not: refuse it here, not at the first batch
        sample_params([(n, None) for n in names], self.shape, self.augmentations)

    # ---- footprint ----------------------------------------------------------------------------------------------------
    def nbytes(self):
        """Device bytes held: the cached cases plus every batch buffer set allocated so far."""
        return self.cache_bytes + sum(_batch_nbytes(b) for b in self._bufs.values())

    def footprint(self):
        return (f"DeviceCache: {self.img.shape[0]} cases of {self.shape} on {self.device}: "
                f"{self.cache_bytes / 2**20:.1f} MiB cached, {self.nbytes() / 2**20:.1f} MiB with batch buffers")

    # ---- the pipeline -------------------------------------------------------------------------------------------------
    def _buffers(self, N):
        b = self._bufs.get(N)
        if b is None:
            dev = self.device
            tmp = [(torch.empty((N,) + self.shape, dtype=torch.float32, device=dev),
                    torch.empty((N,) + self.shape, dtype=torch.uint8, device=dev)) for _ in range(min(self.n_affine, 2))]
            b = self._bufs[N] = {"img": torch.empty((N, 1) + self.shape, dtype=torch.float32, device=dev),
                                 "seg": torch.empty((N,) + self.shape, dtype=torch.uint8, device=dev),
                                 "tmp": [t for pair in tmp for t in pair],
                                 "box": _BoxOut(N, self.shape, self.n_classes, self.capacity, self.comp_cap, dev)}
            if names_mr(self.augmentations):  # msl_augment_mr works out of place
                b["built"] = torch.empty_like(b["img"])
                b["mr"] = MRStageRunner(N, 1, self.shape, dev)
        return b

    def _run(self, slots, per_sample, b):
        dev = self.device
        stream = _stream(dev)
        launches = batch_launches(slots, per_sample)
        pd = torch.from_numpy(np.concatenate([rows.reshape(-1) for _, rows in launches])).pin_memory().to(dev, non_blocking=True)
        N = len(slots)
        src_img, src_seg, n_src = self.img, self.seg, self.img.shape[0]
        # with the MR stage behind it the build writes the stage's source; "img" stays the batch's fixed output
        mr = "mr" in b and _drew_mr(per_sample)
        at = 0
        for k, (fn, rows) in enumerate(launches):
            last = k == len(launches) - 1
            dst_img, dst_seg = (b["built"] if mr else b["img"], b["seg"]) if last else \
                (b["tmp"][2 * (k % 2)], b["tmp"][2 * (k % 2) + 1])
            _lib.call(fn, ptr(src_img), ptr(src_seg), n_src, ptr(pd[at:]), N, *self.shape, ptr(dst_img), ptr(dst_seg), stream)
            at += rows.size
            src_img, src_seg, n_src = dst_img, dst_seg, N
        if mr:
            b["mr"].run(b["built"], per_sample, b["img"], stream)
        b["box"].launch(b["seg"], stream)

    def train_batches(self, epoch):
        tr = self.dataset.train_dataset
        for idx in train_batch_order(self.dataset, epoch):
            per_sample = []
            for i in idx:
                draws = draw_augmentations(self.augmentations, sample_rng(tr.seed, epoch, tr.subjects[i])) \
                    if self.augmentations else []
                per_sample.append(sample_params(draws, self.shape, self.augmentations))
            b = self._buffers(len(idx))
            self._run([self.train_slots[i] for i in idx], per_sample, b)
            yield {"img": b["img"], "seg": b["seg"], "gb": b["box"].gb, "gl": b["box"].gl, "obj_off": b["box"].obj_off,
                   "capacity": self.capacity, "subject": [tr.subjects[i] for i in idx], "_box": b["box"]}

    def step(self, trainer, batch, metrics=False, stats=False):
        """One ``FusedTrainer.step_packed`` on a ``train_batches`` batch; raises HipKernelError if the batch overflowed
        the capacity (checked after the step's own loss read: no extra synchronisation)."""
        out = trainer.step_packed(batch["img"], batch["gb"], batch["gl"], batch["obj_off"], batch["capacity"],
                                  resident=True, metrics=metrics, stats=stats)
        batch["_box"].raise_on_overflow()
        return out

    def val_batches(self):
        """``validation_step`` batches (device tensors, per-image box lists) of this rank's validation shard."""
        ident = (([0, 1, 2], [0, 0, 0]), [])
        for i0 in range(0, len(self.val_order), self.batch_size):
            chunk = self.val_order[i0:i0 + self.batch_size]
            b = self._buffers(len(chunk))
            self._run([slot for _, slot in chunk], [ident] * len(chunk), b)
            yield _val_batch(b, [s for s, _ in chunk])


# ---- clinical cases: ragged sources, instance masks (datasets.LesionsDataModule) ---------------------------------------
INT_MAX = 2 ** 31 - 1
INST_MAX_IDS = 32767  # msl_instance_boxes labels ids 1 .. 32767: no image holds more boxes


def threshold_table(thresholds):
    """[(lo, hi), ...] with hi possibly inf -> (n, 2) int32 array for msl_instance_boxes (inf = INT_MAX)."""
    t = np.array([[min(float(lo), INT_MAX), min(float(hi), INT_MAX)] for lo, hi in thresholds], dtype=np.float64)
    if t.ndim != 2 or t.shape[0] < 1 or not np.array_equal(t, np.floor(t)):
        raise ValueError(f"integer threshold pairs expected, got {thresholds}")
    return np.ascontiguousarray(t.astype(np.int32))


class _InstBoxOut(_BoxStage):
    """``_BoxStage`` of msl_instance_boxes for one (N, D, H, W, thresholds, capacity)."""

    entry = "msl_instance_boxes"

    def __init__(self, N, shape, thresholds, capacity, dev):
        self.thr = threshold_table(thresholds)  # host table, read during every call
        nbytes = _lib.load().msl_instance_boxes_workspace_bytes(N)
        super().__init__(N, shape, capacity, dev, nbytes, f"batch size N={N}")

    def _args(self):
        return self.thr.ctypes.data, self.thr.shape[0], self.capacity

    def _errors(self):
        return [(1, f"a batch holds more ground-truth boxes than the capacity of {self.capacity} rows"),
                (4, "a mask holds a negative value")]


def boxes_from_instances_device(seg, thresholds, capacity=None):
    """``datasets.boxes_from_instances`` ('instances' mode) for every image of a device int16 (N, D, H, W) mask ->
    (boxes list, labels list, (gb, gl, obj_off, capacity)) as ``boxes_from_segmentation_device`` returns them."""
    if not seg.is_cuda or seg.dtype != torch.int16 or seg.dim() != 4:
        raise _lib.HipKernelError("boxes_from_instances_device takes an int16 (N, D, H, W) tensor on the HIP device")
    seg = seg.contiguous()
    N = seg.shape[0]
    capacity = 1024 * N if capacity is None else int(capacity)
    return _InstBoxOut(N, seg.shape[1:], thresholds, capacity, seg.device).boxes(seg)


MAX_RUNS_PER_IMAGE = 262144  # msl_binary_boxes: runs of non-zero voxels per image (about ten times a 50 mL lesion load)


class _BinBoxOut(_BoxStage):
    """``_BoxStage`` of msl_binary_boxes for one (N, D, H, W, capacity, run_cap): ``_InstBoxOut``'s attributes, for
    binary masks (their 6-connected components are the lesions)."""

    entry = "msl_binary_boxes"

    def __init__(self, N, shape, capacity, dev, max_runs_per_image=MAX_RUNS_PER_IMAGE):
        self.run_cap = int(max_runs_per_image) * N
        nbytes = _lib.load().msl_binary_boxes_workspace_bytes(N, *shape, self.run_cap) if self.run_cap > 0 else 0
        super().__init__(N, shape, capacity, dev, nbytes,
                         f"sizes N={N} shape={tuple(shape)} max_runs_per_image={max_runs_per_image}")

    def _args(self):
        return self.capacity, self.run_cap

    def _errors(self):  # the run overflow is reported before the row overflow
        return [(8, f"a batch holds more runs of lesion voxels than max_runs_per_image = {self.run_cap // self.N} per "
                    f"image allows: raise max_runs_per_image"),
                (1, f"a batch holds more ground-truth boxes than the capacity of {self.capacity} rows: raise "
                    f"max_objects_per_image")]


def boxes_from_binary_device(seg, capacity=None, max_runs_per_image=MAX_RUNS_PER_IMAGE):
    """``datasets.boxes_from_instances(seg[n], [(1, inf)], mode="binary")`` for every image of a device int16
    (N, D, H, W) mask -> (boxes list, labels list, (gb, gl, obj_off, capacity)) as ``boxes_from_instances_device``
    returns them."""
    if not seg.is_cuda or seg.dtype != torch.int16 or seg.dim() != 4:
        raise _lib.HipKernelError("boxes_from_binary_device takes an int16 (N, D, H, W) tensor on the HIP device")
    seg = seg.contiguous()
    N = seg.shape[0]
    capacity = 1024 * N if capacity is None else int(capacity)
    return _BinBoxOut(N, seg.shape[1:], capacity, seg.device, max_runs_per_image).boxes(seg)


def _box_stage(dataset, N, shape, capacity, dev, max_runs_per_image=MAX_RUNS_PER_IMAGE, who="device pipeline"):
    """The box stage of a data module's segmentation mode for (N,) + shape masks: msl_instance_boxes on instance-labelled
    masks, msl_binary_boxes on binary ones."""
    mode = dataset.segmentation_mode
    if mode == "instances":
        return _InstBoxOut(N, shape, dataset.thresholds, capacity, dev)
    if mode == "binary":
        return _BinBoxOut(N, shape, capacity, dev, max_runs_per_image)
    raise NotImplementedError(f"{who}: no device box stage for segmentation mode {mode!r}")


def fit_rows(cases, per_sample):
    """-> (N, AFFINE_STRIDE) f64 rows of one msl_augment_fit launch: per sample its case and the (perm, stages) of
    ``sample_params(..., ragged=True)``: at most one affine stage, then the intensity operations."""
    rows, tables = _stage_rows(cases, per_sample, ())
    return rows


def warp_rows(cases, per_sample):
    """-> ((N, AFFINE_STRIDE) f64 rows, f64 coords) of one msl_augment_warp_mc launch: ``fit_rows``'s rows, where a
    sample whose one resampling stage is a ``WarpStage`` has [7] = ROW_WARP, at [8] the offset of its three tables in
    ``coords`` (concatenated, axis 0 first) and at [20] the boundary.  Without a warp drawn ``coords`` is empty and the rows
    are those of msl_augment_fit_mc / msl_augment_window_mc."""
    return _stage_rows(cases, per_sample, (WarpStage,))


def deform_rows(cases, per_sample):
    """-> ((N, AFFINE_STRIDE) f64 rows, f64 lattices) of one msl_augment_deform_mc launch: ``fit_rows``'s rows, where a
    sample whose one resampling stage is a ``DeformStage`` has [7] = ROW_DEFORM, at [8] the offset of its 3 L^3
    coefficients in ``lattices`` (concatenated, C order), at [9] L and at [20] the boundary.  Without a deformation drawn
    ``lattices`` is empty and the rows are those of msl_augment_fit_mc / msl_augment_window_mc."""
    return _stage_rows(cases, per_sample, (DeformStage,))


def _stage_rows(cases, per_sample, own):
    """The rows of one launch and the f64 table that rides with them: the tables of the ``WarpStage``s or the lattices of
    the ``DeformStage``s, whichever of the two ``own`` names.  A stage with a table that is not the launch's own raises
    ValueError."""
    rows = np.zeros((len(cases), AFFINE_STRIDE), dtype=np.float64)
    coords, at = [], 0
    for n, (case, (perm, stages)) in enumerate(zip(cases, per_sample)):
        geo = [st for st in stages if not isinstance(st, (IntensityOp,) + POST_STAGES)]
        if len(geo) > 1:
            raise NotImplementedError("device pipeline: two affine stages on cases of unequal shape")
        st = geo[0] if geo else None
        ops = [x for x in stages if isinstance(x, IntensityOp)]
        if isinstance(st, (WarpStage, DeformStage)) and not isinstance(st, own):
            raise ValueError(f"a sample drew a {type(st).__name__}: warp_rows / deform_rows return its table with the rows")
        if isinstance(st, WarpStage):
            rows[n] = affine_row(case, perm, None, ops)
            rows[n, 7], rows[n, 8], rows[n, 20] = ROW_WARP, at, st.boundary
            coords += [np.asarray(t, dtype=np.float64) for t in st.tables]
            at += sum(len(t) for t in st.tables)
        elif isinstance(st, DeformStage):
            P = np.ascontiguousarray(st.lattice, dtype=np.float64)
            rows[n] = affine_row(case, perm, None, ops)
            rows[n, 7], rows[n, 8], rows[n, 9], rows[n, 20] = ROW_DEFORM, at, P.shape[1], st.boundary
            coords.append(P.reshape(-1))
            at += P.size
        else:
            rows[n] = affine_row(case, perm, st, ops)
    return rows, (np.concatenate(coords) if coords else np.zeros(0, dtype=np.float64))


def pack_launch(rows, table, windows=None):
    """The one f64 upload of a ragged launch -> (packed, table offset, windows offset), the offsets in f64 elements:
    the (N, AFFINE_STRIDE) ``rows``, then the f64 ``table`` that rides with them (``warp_rows`` / ``deform_rows``; may be
    empty), then, where ``windows`` is given, its (N, 3) int32 origins in the doubles behind them (N odd: a last int of
    0).  Pure numpy; with an empty table and no windows the upload is ``rows.reshape(-1)``."""
    at_table, at_windows = rows.size, rows.size + table.size
    n_int = 0 if windows is None else 3 * rows.shape[0]
    packed = np.zeros(at_windows + (n_int + 1) // 2, dtype=np.float64)
    packed[:at_table] = rows.reshape(-1)
    packed[at_table:at_windows] = table
    if windows is not None:
        packed[at_windows:].view(np.int32)[:n_int] = np.asarray(windows, dtype=np.int32).reshape(-1)
    return packed, at_table, at_windows


def pack_ints(packed, ints):
    """An int32 table behind a ``pack_launch`` upload -> (packed, offset in f64 elements): the ints ride in the doubles
    behind what is there (an odd count: a last int of 0), as the windows do.  msl_paste_lesions's rows travel this way."""
    ints = np.ascontiguousarray(ints, dtype=np.int32).reshape(-1)
    out = np.zeros(packed.size + (ints.size + 1) // 2, dtype=np.float64)
    out[:packed.size] = packed
    out[packed.size:].view(np.int32)[:ints.size] = ints
    return out, packed.size


def paste_kw(augmentations):
    """The keyword arguments of the list's lesionpaste entry over the defaults, or None where it names none."""
    for t in augmentations:
        if transform_name(t) == PASTE_NAME:
            return dict(PASTE_AUGMENTATIONS[0][1], **transform_kw(t))
    return None


def names_mr(augmentations):
    """Does the augmentation list name gaussiansmooth, biasfield or gaussiannoise?"""
    return any(transform_name(t) in MR_NAMES for t in augmentations)


def mr_tables(per_sample):
    """The ``MRStage``s of a batch's ``sample_params`` results -> (rows (N, MR_STRIDE) f64, taps (N, 3, MR_TAPS) f32,
    lattice (N, L, L, L) f32), the three tables msl_augment_mr reads.  Row: [0] the sum of MR_BLUR / MR_BIAS / MR_NOISE
    for what the sample drew, [1..3] the blur radii R_0..R_2, [4] the noise deviation as an f32, [5] [6] the key words
    k0, k1.  Taps: ``datasets.gaussian_taps`` of axis a in [n, a, 0 .. 2 R_a].  Lattice: ``datasets.bias_lattice``.  Both
    are the host's own values: the device computes no exponential.  A sigma above 2.0 raises ValueError, a lattice of
    more than MR_LATTICE points per axis NotImplementedError."""
    N = len(per_sample)
    L = MR_LATTICE
    for _, stages in per_sample:
        for st in stages:
            if isinstance(st, MRStage) and st.name == "biasfield":
                L = int(st.kw.get("lattice", 9))
    if not 2 <= L <= MR_LATTICE:
        raise NotImplementedError(f"device pipeline: a bias lattice of 2 .. {MR_LATTICE} points per axis, got {L}")
    rows = np.zeros((N, MR_STRIDE), dtype=np.float64)
    taps = np.zeros((N, 3, MR_TAPS), dtype=np.float32)
    lattice = np.ones((N, L, L, L), dtype=np.float32)
    for n, (_, stages) in enumerate(per_sample):
        for st in stages:
            if not isinstance(st, MRStage) or st.draw is None:
                continue
            if st.name == "gaussiansmooth":
                rows[n, 0] += MR_BLUR
                for a, sigma in enumerate(st.draw):
                    w = gaussian_taps(sigma)
                    rows[n, 1 + a] = (w.size - 1) // 2
                    taps[n, a, :w.size] = w
            elif st.name == "biasfield":
                rows[n, 0] += MR_BIAS
                lattice[n] = bias_lattice(st.draw, st.kw.get("degree", 3), L)
            else:
                rows[n, 0] += MR_NOISE
                rows[n, 4], rows[n, 5], rows[n, 6] = np.float32(st.draw[0]), st.draw[1], st.draw[2]
    return rows, taps, lattice


class MRStageRunner:
    """msl_augment_mr for (N, C) + shape f32 batches: the workspace, and one launch per batch behind the batch build.
    ``run`` uploads the three tables of ``mr_tables`` in one pinned copy and writes ``dst`` from ``src`` (out of place) on
    the current stream; a sample that drew nothing is copied."""

    def __init__(self, N, C, shape, dev):
        self.N, self.C, self.shape, self.device = int(N), int(C), tuple(int(n) for n in shape), dev
        nbytes = _lib.load().msl_augment_mr_workspace_bytes(self.N, self.C, *self.shape)
        if nbytes == 0:
            raise _lib.HipKernelError(f"msl_augment_mr: unsupported sizes N={N} C={C} shape={self.shape}")
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def run(self, src, per_sample, dst, stream):
        rows, taps, lattice = mr_tables(per_sample)
        if rows.shape[0] != self.N:
            raise ValueError(f"msl_augment_mr: {rows.shape[0]} samples on a stage for {self.N}")
        packed = np.zeros(rows.size + (taps.size + lattice.size + 1) // 2, dtype=np.float64)
        packed[:rows.size] = rows.reshape(-1)
        f32 = packed[rows.size:].view(np.float32)  # the f32 tables ride in the doubles behind the rows
        f32[:taps.size] = taps.reshape(-1)
        f32[taps.size:taps.size + lattice.size] = lattice.reshape(-1)
        pd = torch.from_numpy(packed).pin_memory().to(self.device, non_blocking=True)
        at = pd.data_ptr() + 8 * rows.size
        _lib.call("msl_augment_mr", ptr(src), ptr(pd), at, at + 4 * taps.size, self.N, self.C, *self.shape,
                  lattice.shape[1], ptr(dst), ptr(self.ws), self.ws.numel(), stream)


def check_ragged_pipeline(augmentations):
    """What ``LesionCache`` refuses at construction, drawn or not: more than one resampling stage (affine / zoom /
    griddistortion / elastic3d: a resample of a resample of a ragged case would need a ragged intermediate) and the order limits of
    ``sample_params``.  NotImplementedError."""
    names = [transform_name(t) for t in augmentations]
    if sum(n in RESAMPLERS for n in names) > 1:
        raise NotImplementedError("device pipeline: two affine stages on cases of unequal shape")
    sample_params([(n, None) for n in names], (1, 1, 1), augmentations, ragged=True)


def plan_row(plan):
    """The 12 f64 msl_regrid reads on the host: ax[3], rev[3], step[3], start[3] of a ``datasets.RegridPlan``."""
    return np.ascontiguousarray(np.concatenate([plan.ax, [int(r) for r in plan.rev], plan.step, plan.start]),
                                dtype=np.float64)


def regrid_device(img, seg, plan):
    """``datasets.regrid`` on the HIP device (msl_regrid, current stream, no synchronisation), bit for bit: ``img`` f32
    (n0, n1, n2) or (C, n0, n1, n2) and ``seg`` int16 (n0, n1, n2) device tensors on the plan's native grid (either may
    be None) -> the pair on the plan's output grid.  An identity plan returns the inputs untouched."""
    if plan.identity:
        return img, seg
    ref = img if img is not None else seg
    if ref is None or not ref.is_cuda:
        raise _lib.HipKernelError("regrid_device takes tensors on the HIP device (no CPU fallback)")
    if (img is not None and (img.dtype != torch.float32 or tuple(img.shape[-3:]) != tuple(plan.src_shape)
                             or img.dim() not in (3, 4))) or \
            (seg is not None and (seg.dtype != torch.int16 or tuple(seg.shape) != tuple(plan.src_shape))):
        raise ValueError(f"regrid_device: f32 image / int16 mask of the plan's native shape {plan.src_shape} expected")
    C = img.shape[0] if img is not None and img.dim() == 4 else 1
    img = img.contiguous() if img is not None else None
    seg = seg.contiguous() if seg is not None else None
    out_shape = tuple(plan.out_shape)
    di = None if img is None else torch.empty((out_shape if img.dim() == 3 else (C,) + out_shape), dtype=torch.float32,
                                              device=ref.device)
    dseg = None if seg is None else torch.empty(out_shape, dtype=torch.int16, device=ref.device)
    row = plan_row(plan)  # host table, read during the call
    _lib.call("msl_regrid", ptr(img), ptr(seg), C, *plan.src_shape, row.ctypes.data, *out_shape, ptr(di), ptr(dseg),
              _stream(ref.device))
    return di, dseg


def _case_on_device(ds, i, dev, who, check_memory=None):
    """Case i of a ``_LesionCases`` data set on the device, on the LPI 1 mm grid: uploaded as stored and, where it
    carries an affine with a non-identity plan, regridded there -> (image f32 (n) / (C, n), mask int16 (n), plan or
    None).  ``check_memory(nbytes, what)`` is asked for the native copy plus the regridded one."""
    img, seg, affine = ds.load_native(i)
    seg16 = seg.astype(np.int16)
    if not np.array_equal(seg16, seg) or (seg16.size and seg16.min() < 0):
        raise ValueError(f"{who}: mask of case {ds.subjects[i]} is not integer-valued in [0, 32767]")
    plan = None if affine is None else regrid_plan(affine, seg.shape)
    per_voxel = 4 * (img.shape[0] if img.ndim == 4 else 1) + 2
    nbytes = seg.size * per_voxel
    if plan is not None and not plan.identity:
        nbytes += int(np.prod(plan.out_shape)) * per_voxel
    if check_memory is not None:
        check_memory(nbytes, f"case {ds.subjects[i]} of {img.shape}")
    vol, mask = torch.from_numpy(img).to(dev), torch.from_numpy(seg16).to(dev)
    if plan is not None:
        vol, mask = regrid_device(vol, mask, plan)
    return vol, mask, plan


def _foreground_box(vol, margin, box, stream):
    """msl_foreground_box_mc on the image ``_case_on_device`` returned -> the six ints in ``box`` (device): a
    one-sequence image has no channel axis and is the C = 1 launch."""
    C = vol.shape[0] if vol.dim() == 4 else 1
    _lib.call("msl_foreground_box_mc", ptr(vol), C, *vol.shape[-3:], int(margin), ptr(box), stream)


class LesionCache:
    """The cases of a ``setup()`` ``datasets.LesionsDataModule`` in HBM, cropped to their foreground and normalised: one
    flat arena of f32 images and one of int16 masks with a per-case (offset, shape) table, and the device pipeline that
    turns them into fixed-size training / validation batches (msl_augment_fit_mc, msl_instance_boxes).

    Same semantics as ``DeviceCache``: ``train_batches(epoch)`` yields the batches of ``dataset.train_dataloader()`` for
    that epoch (same subjects, same draws) in fixed buffers, ``step(trainer, batch)`` trains on one, ``val_batches()``
    yields ``validation_step`` batches.  At construction every case is uploaded once (a case with an affine on its
    native grid, then regridded by msl_regrid: ``plans`` holds its ``RegridPlan``, None otherwise), boxed by
    msl_foreground_box_mc (the six ints are the build's only read-back), cropped into the arena and normalised there; the
    cropped cases are staged in tensors of their own until the arena's size is known.  A pipeline with two resampling
    stages (affine / zoom / griddistortion entries, ``check_ragged_pipeline``) raises NotImplementedError (a resample of
    a resample of a ragged case would need a ragged intermediate).  A batch in which a sample drew a warp is written by
    msl_augment_warp_mc (the tables ride behind the rows in the batch's one pinned upload), one in which a sample drew an
    elastic3d by msl_augment_deform_mc (the lattices ride there); every other batch by the launch it always had.

    With C = len(dataset.input_images) a case is C contiguous f32 planes starting at element C * offset of the image
    arena (the mask arena and the table are the same for every C): boxed as the union of the channels by
    msl_foreground_box_mc, every plane normalised on its own (one msl_normalize_nonzero call over the case's C planes),
    batches written as (N, C) + target by msl_augment_fit_mc.  One sequence is C = 1 of the same calls.

    Patch mode (``dataset.patch_size`` set): the batch shape is the patch.  ``train_batches`` makes the host's draws for
    every sample - the augmentation's, then ``datasets.patch_origin``'s eight from the same generator - and
    msl_augment_window_mc cuts the window out of the augmented case in the launch that augments it; the batch carries
    "patch_origin".  The lesion centres ``patch_origin`` aims at are taken once per training case at construction
    (``centres``).  ``val_batches`` yields the tiles of ``datasets._LesionTiles`` (every validation case is cached on every
    rank: the tile list, not the case list, is what the ranks share out), ``batch_size`` tiles at a time.

    lesionpaste: a list that names it gets the lesion bank at construction (``bank``, the host's
    ``_LesionCases.build_bank`` from the device's own box stage); ``train_batches`` lowers every sample's draw with
    ``datasets.lower_pastes`` and, in a batch where some sample drew one, msl_paste_lesions (csrc/lesionpaste.hip) runs on
    the built batch in front of the MR stage and the box stage.  The batch carries "paste_report" (N, max_lesions) i32;
    ``paste_counts()`` reads the epoch's totals once."""

    def __init__(self, dataset, device, max_objects_per_image=64, max_runs_per_image=MAX_RUNS_PER_IMAGE):
        if dataset.train_dataset is None:
            raise ValueError("LesionCache needs a data module after setup()")
        self.dataset, self.device = dataset, torch.device(device)
        self.patch = getattr(dataset, "patch_size", None)
        self.batch_size = int(dataset.batch_size)
        self.target = tuple(dataset.spatial_size) if self.patch is None else tuple(self.patch)
        self.channels = C = len(dataset.input_images)
        self.augmentations = list(dataset.train_dataset.augmentations)
        check_ragged_pipeline(self.augmentations)
        if dataset.segmentation_mode not in ("instances", "binary"):
            raise NotImplementedError(f"LesionCache: no device box stage for segmentation mode "
                                      f"{dataset.segmentation_mode!r}")
        self.max_runs_per_image = int(max_runs_per_image)
        tr, te = dataset.train_dataset, dataset.test_dataset
        if self.patch is not None:
            te = te.cases  # datasets._LesionTiles: its tiles are dealt to the ranks below, once the crop shapes are known
            val_idx = np.arange(len(te))
        elif dataset.world_size > 1:
            val_idx = ShardSampler(len(te), dataset.rank, dataset.world_size, False, dataset.random_state).indices()
        else:
            val_idx = np.arange(len(te))
        self.slot = {}
        loaders = []
        for ds, idx in ((tr, range(len(tr))), (te, val_idx)):
            for i in idx:
                if ds.subjects[i] not in self.slot:
                    self.slot[ds.subjects[i]] = len(self.slot)
                    loaders.append((ds, int(i)))
        self.train_slots = [self.slot[s] for s in tr.subjects]
        self.val_order = [(te.subjects[i], self.slot[te.subjects[i]]) for i in val_idx]
        dev, stream = self.device, _stream(self.device)
        box = torch.zeros(6, dtype=torch.int32, device=dev)
        staged, self.shapes, self.origins, self.full_shapes, self.plans = [], [], [], [], []
        for ds, i in loaders:
            vol, mask, plan = _case_on_device(ds, i, dev, "LesionCache", self._check_memory)
            _foreground_box(vol, dataset.margin, box, stream)
            b = box.cpu().tolist()  # the one read that sizes the crop
            sl = tuple(slice(b[a], b[3 + a]) for a in range(3))
            staged.append((vol[(...,) + sl].contiguous(), mask[sl].contiguous()))
            self.shapes.append(tuple(b[3 + a] - b[a] for a in range(3)))
            self.origins.append(tuple(b[:3]))  # the crop's lo: datasets.fit_to_case_frame maps boxes back with it
            self.full_shapes.append(tuple(int(v) for v in mask.shape))  # the regridded shape of a case with an affine
            self.plans.append(plan)  # datasets.regrid_to_native maps case-frame boxes on to the stored grid with it
            del vol, mask
        sizes = [int(np.prod(s)) for s in self.shapes]
        self.offsets = [0] + np.cumsum(sizes).tolist()
        self.cache_bytes = self.offsets[-1] * (4 * C + 2)
        self._check_memory(self.cache_bytes, f"{len(sizes)} cropped cases")
        self.img = torch.empty(C * max(self.offsets[-1], 1), dtype=torch.float32, device=dev)
        self.seg = torch.empty(max(self.offsets[-1], 1), dtype=torch.int16, device=dev)
        for k in range(len(sizes)):
            ci, cs = staged[k]
            staged[k] = None
            self.img[C * self.offsets[k]:C * self.offsets[k + 1]].copy_(ci.reshape(-1))
            self.seg[self.offsets[k]:self.offsets[k + 1]].copy_(cs.reshape(-1))
            if sizes[k]:  # C contiguous volumes, each over its own non-zero voxels
                _lib.call("msl_normalize_nonzero", self.img.data_ptr() + 4 * C * self.offsets[k], C, sizes[k], stream)
        self.table = torch.tensor([[self.offsets[k], *self.shapes[k]] for k in range(len(sizes))],
                                  dtype=torch.int64, device=dev).reshape(-1, 4)
        self.capacity = int(max_objects_per_image) * self.batch_size
        self._bufs = {}
        self.paste = paste_kw(self.augmentations)
        if self.paste is not None:  # lesionpaste: the bank over the training cases, in train_dataset.subjects order
            check_lesionpaste(**self.paste)
            self.bank = self._lesion_bank()
            self._paste_counts = torch.zeros(2, dtype=torch.int64, device=dev)  # rows that were tested / accepted
        if self.patch is not None:
            self.centres = {k: self._case_centres(k) for k in sorted(set(self.train_slots))}
            tiles =[(s, k, tuple(int(v) for v in row[:3])) for s, k in self.val_order
                     for row in view_plan(self.shapes[k], self.patch, dataset.tile_margin)]
            if dataset.world_size > 1:
                own = ShardSampler(len(tiles), dataset.rank, dataset.world_size, False, dataset.random_state).indices()
                tiles = [tiles[i] for i in own]
            self.val_tiles = tiles  # (subject, slot, origin): this rank's share of dataset.test_dataset.tiles

    def _case_lesions(self, slot):
        """The boxes the box stage keeps on a cached case -> (inclusive integer extents f64 (K, 6) [min..., max...], labels
        i64 (K,)), in its order: one msl_instance_boxes call (msl_binary_boxes on a binary mask: the components of the
        cropped, un-augmented mask) on the cropped mask, read back once.  The kernel writes f32(e / n) for an inclusive
        integer extent e on an axis of n voxels; the extent
        is recovered as rint(f32(e / n) * n) in f64.  The division's relative error is at most 2^-24 and the f64 product
        adds 2^-53, so the product is within e * 2^-23 of e: exact while e < 2^22, and the arena refuses axes of 2^20
        voxels or more."""
        shape = self.shapes[slot]
        if not int(np.prod(shape)):
            return np.zeros((0, 6), dtype=np.float64), np.zeros(0, dtype=np.int64)
        out = _box_stage(self.dataset, 1, shape, INST_MAX_IDS, self.device, self.max_runs_per_image, "LesionCache")
        out.launch(self.case(slot)[1], _stream(self.device))
        n = out.obj_off.cpu().tolist()[1]  # (synchronises: the flag and the rows are there too)
        out.raise_on_overflow(out.flag.item())
        ext = np.rint(out.gb[:n].cpu().numpy().astype(np.float64) * np.asarray(shape * 2, dtype=np.float64))
        return ext, out.gl[:n].cpu().numpy().astype(np.int64)

    def _case_centres(self, slot):
        """``datasets.lesion_centres`` of a cached case -> f64 (K, 3), from ``_case_lesions``'s extents."""
        ext, _ = self._case_lesions(slot)
        return (ext[:, :3] + ext[:, 3:]) / 2

    def _lesion_bank(self):
        """``datasets.bank_from_lesions`` over the training cases in ``train_dataset.subjects`` order, the bank
        ``_LesionCases.build_bank`` makes on the host: per case the extents and labels of ``_case_lesions`` and, in
        instances mode, the largest id of every class's threshold pair on the cached mask (torch; set-up plumbing)."""
        thr = self.dataset.thresholds
        per_case = []
        for slot in self.train_slots:
            ext, labels = self._case_lesions(slot)
            ids = [0] * len(thr)
            if self.dataset.segmentation_mode == "instances":
                seg = self.case(slot)[1]
                for c, (lo, hi) in enumerate(thr):
                    inside = seg[(seg >= int(lo)) & (seg < min(float(hi), 32768.0))]
                    ids[c] = int(inside.max().item()) if inside.numel() else int(lo) - 1
            per_case.append((ext.astype(np.int64), labels, self.shapes[slot], ids))
        bank = bank_from_lesions(per_case, self.paste.get("max_volume"))
        if not len(bank.rows):
            raise ValueError(f"{PASTE_NAME}: the lesion bank is empty: no lesion of the {len(per_case)} training cases is "
                             f"small enough and clear of its neighbours")
        return bank

    def paste_counts(self, reset=True):
        """-> (pastes tested, pastes accepted) since the last reset: ONE read of the device counters (train.py reads them
        at the end of an epoch); (0, 0) without lesionpaste."""
        if self.paste is None:
            return 0, 0
        asked, accepted = self._paste_counts.cpu().tolist()
        if reset:
            self._paste_counts.zero_()
        return int(asked), int(accepted)

    def _check_memory(self, nbytes, what):
        free, _ = torch.cuda.mem_get_info(self.device)
        if nbytes > 0.8 * free:
            raise MemoryError(f"LesionCache: {what} need {nbytes / 2**30:.2f} GiB, {free / 2**30:.2f} GiB free on "
                              f"{self.device}")

    def case(self, slot):
        """-> (image f32, mask int16) views of a cached case, shaped; the image is (C, n0, n1, n2) for C > 1."""
        a, b, C = self.offsets[slot], self.offsets[slot + 1], self.channels
        shape = tuple(self.shapes[slot])
        return self.img[C * a:C * b].view(shape if C == 1 else (C,) + shape), self.seg[a:b].view(shape)

    # ---- footprint ----------------------------------------------------------------------------------------------------
    def nbytes(self):
        """Device bytes held: the cached cases plus every batch buffer set allocated so far."""
        return self.cache_bytes + sum(_batch_nbytes(b) for b in self._bufs.values())

    def footprint(self):
        lo, hi = np.min(self.shapes, 0).tolist(), np.max(self.shapes, 0).tolist()
        how = f"fitted to {self.target}" if self.patch is None else \
            f"in patches of {self.target} ({len(self.val_tiles)} validation tiles)"
        return (f"LesionCache: {len(self.shapes)} cases of {tuple(lo)} .. {tuple(hi)} {how} on "
                f"{self.device}: {self.cache_bytes / 2**20:.1f} MiB cached, {self.nbytes() / 2**20:.1f} MiB with batch "
                f"buffers")

    # ---- the pipeline -------------------------------------------------------------------------------------------------
    def _buffers(self, N):
        b = self._bufs.get(N)
        if b is None:
            dev = self.device
            b = self._bufs[N] = {"img": torch.empty((N, self.channels) + self.target, dtype=torch.float32, device=dev),
                                 "seg": torch.empty((N,) + self.target, dtype=torch.int16, device=dev),
                                 "box": _box_stage(self.dataset, N, self.target, self.capacity, dev,
                                                   self.max_runs_per_image, "LesionCache")}
            if names_mr(self.augmentations):  # msl_augment_mr works out of place
                b["built"] = torch.empty_like(b["img"])
                b["mr"] = MRStageRunner(N, self.channels, self.target, dev)
            if self.paste is not None:  # msl_paste_lesions's report: -2 where nothing was asked
                b["paste_report"] = torch.full((N, int(self.paste["max_lesions"])), -2, dtype=torch.int32, device=dev)
        return b

    def _run(self, slots, per_sample, b, windows=None, pastes=None):
        """``pastes``: the (N, K, stride) int32 rows of ``datasets.lower_pastes`` for a training batch in which some
        sample drew a lesionpaste; they ride in the batch's one pinned upload behind the build's rows."""
        stream, N = _stream(self.device), len(slots)
        # one resampling entry per pipeline: a batch holds warp stages or deformation stages, never both
        deform = any(isinstance(st, DeformStage) for _, stages in per_sample for st in stages)
        rows, table = (deform_rows if deform else warp_rows)(slots, per_sample)
        packed, at_table, at_windows = pack_launch(rows, table, windows)
        if pastes is not None:
            packed, at_pastes = pack_ints(packed, pastes)
        pd = torch.from_numpy(packed).pin_memory().to(self.device, non_blocking=True)
        origins = None if windows is None else pd.data_ptr() + 8 * at_windows
        if table.size:  # some sample drew a warp / deformation; every other batch keeps the launch it always had
            entry, own = "msl_augment_deform_mc" if deform else "msl_augment_warp_mc", \
                (pd.data_ptr() + 8 * at_table, table.size, origins)
        else:
            entry, own = ("msl_augment_fit_mc", ()) if windows is None else ("msl_augment_window_mc", (origins,))
        # with the MR stage behind it the build writes the stage's source; "img" stays the batch's fixed output
        built = b["built"] if "mr" in b and _drew_mr(per_sample) else b["img"]
        _lib.call(entry, ptr(self.img), ptr(self.seg), self.seg.numel(), self.channels, ptr(self.table), len(self.shapes),
                  ptr(pd), *own, N, *self.target, ptr(built), ptr(b["seg"]), stream)
        self._finish(b, per_sample, stream, built, None if pastes is None else (pd, at_pastes, pastes.shape))

    def _finish(self, b, per_sample, stream, built=None, pastes=None):
        """Behind the batch build: the paste stage on the built batch (only where some sample drew one; ``pastes``: the
        upload, the rows' offset in it in f64 elements and their (N, K, stride) shape), then the MR stage on the built
        images, then the box stage."""
        if "paste_report" in b:
            b["paste_report"].fill_(-2)
        if pastes is not None:
            pd, at, (N, K, stride) = pastes
            _lib.call("msl_paste_lesions", ptr(self.img), ptr(self.seg), self.seg.numel(), self.channels, ptr(self.table),
                      len(self.shapes), pd.data_ptr() + 8 * at, N, K, (stride - PASTE_HEAD) // 3, *self.target, ptr(built),
                      ptr(b["seg"]), ptr(b["paste_report"]), stream)
            rep = b["paste_report"]  # the epoch's counters stay on the device: train.py reads them once per epoch
            self._paste_counts += torch.stack([(rep > -2).sum(), (rep >= 0).sum()])
        if "mr" in b and _drew_mr(per_sample):
            b["mr"].run(b["built"], per_sample, b["img"], stream)
        b["box"].launch(b["seg"], stream)

    def train_batches(self, epoch):
        tr = self.dataset.train_dataset
        for idx in train_batch_order(self.dataset, epoch):
            per_sample = []
            windows = None if self.patch is None else []
            for i in idx:
                slot = self.train_slots[i]
                rs = sample_rng(tr.seed, epoch, tr.subjects[i])
                draws = draw_augmentations(self.augmentations, rs) if self.augmentations else []
                per_sample.append(sample_params(draws, self.shapes[slot], self.augmentations, ragged=True))
                if windows is not None:  # the host's eight draws, behind the augmentation's, in the augmented frame
                    perm, stages = per_sample[-1]
                    centres = centres_to_augmented(self.centres[slot], self.shapes[slot], perm, stages)
                    windows.append(patch_origin(rs, tuple(self.shapes[slot][a] for a in perm[0]), self.patch, centres,
                                                self.dataset.patch_foreground))
            pastes = None
            if self.paste is not None:  # the host's lowering, sample by sample; a launch only where some sample drew one
                drawn = [next(st.draw for st in stages if isinstance(st, PasteStage)) for _, stages in per_sample]
                if any(d is not None for d in drawn):
                    pastes = np.stack([lower_pastes(d, self.bank, i, self.target, self.dataset.thresholds,
                                                    self.dataset.segmentation_mode, self.paste["max_lesions"],
                                                    self.paste["candidates"]) for d, i in zip(drawn, idx)])
                    pastes[:, :, 1] = np.asarray(self.train_slots, dtype=np.int32)[pastes[:, :, 1]]  # bank case -> arena slot
            b = self._buffers(len(idx))
            self._run([self.train_slots[i] for i in idx], per_sample, b, windows, pastes)
            out = {"img": b["img"], "seg": b["seg"], "gb": b["box"].gb, "gl": b["box"].gl, "obj_off": b["box"].obj_off,
                   "capacity": self.capacity, "subject": [tr.subjects[i] for i in idx], "_box": b["box"]}
            if windows is not None:
                out["patch_origin"] = windows
            if self.paste is not None:
                out["paste_report"] = b["paste_report"]
            yield out

    step = DeviceCache.step

    def _geometry(self, slots):
        """The keys ``datasets.fit_to_case_frame`` maps a validation batch's boxes back to the case with."""
        return {"crop_origin": [self.origins[k] for k in slots], "crop_shape": [tuple(self.shapes[k]) for k in slots],
                "full_shape": [self.full_shapes[k] for k in slots]}

    def _val_tile_batches(self):
        ident = (([0, 1, 2], [0, 0, 0]), [])
        for i0 in range(0, len(self.val_tiles), self.batch_size):
            chunk = self.val_tiles[i0:i0 + self.batch_size]
            b = self._buffers(len(chunk))
            self._run([slot for _, slot, _ in chunk], [ident] * len(chunk), b, [o for _, _, o in chunk])
            yield {**_val_batch(b, [s for s, _, _ in chunk]), "patch_origin": [o for _, _, o in chunk],
                   **self._geometry([slot for _, slot, _ in chunk])}

    def val_batches(self):
        """``validation_step`` batches (device tensors, per-image box lists) of this rank's validation shard; in patch
        mode, of this rank's share of the validation tiles."""
        if self.patch is not None:
            yield from self._val_tile_batches()
            return
        ident = (([0, 1, 2], [0, 0, 0]), [])
        for i0 in range(0, len(self.val_order), self.batch_size):
            chunk = self.val_order[i0:i0 + self.batch_size]
            b = self._buffers(len(chunk))
            self._run([slot for _, slot in chunk], [ident] * len(chunk), b)
            yield {**_val_batch(b, [s for s, _ in chunk]), **self._geometry([slot for _, slot in chunk])}


def boxes_to_case_device(boxes, target, crop_shape, crop_origin, full_shape):
    """``datasets.fit_to_case_frame`` on the HIP device (msl_boxes_to_case, current stream, no synchronisation), bit for
    bit.  ``boxes``: a (K, 6) device tensor with one geometry, or a list of N of them with a list of N geometries each."""
    single = torch.is_tensor(boxes)
    if single:
        boxes, target, crop_shape, crop_origin, full_shape = [boxes], [target], [crop_shape], [crop_origin], [full_shape]
    if not all(b.is_cuda for b in boxes):
        raise _lib.HipKernelError("boxes_to_case_device takes tensors on the HIP device (no CPU fallback)")
    flat = [b.contiguous().float().reshape(-1, 6) for b in boxes]
    off = np.concatenate([[0], np.cumsum([b.shape[0] for b in flat])]).astype(np.int32)
    geo = np.ascontiguousarray(np.asarray([list(t) + list(n) + list(lo) + list(s) for t, n, lo, s in
                                           zip(target, crop_shape, crop_origin, full_shape)], dtype=np.int32).reshape(-1, 12))
    packed = flat[0] if single else torch.cat(flat)
    out = torch.empty_like(packed)
    _lib.call("msl_boxes_to_case", ptr(packed), off.ctypes.data, geo.ctypes.data, len(flat), ptr(out), _stream(packed.device))
    return out if single else [out[off[n]:off[n + 1]] for n in range(len(flat))]


class LesionPredictFeed:
    """``dataset.predict_dataset`` of a ``setup()`` ``datasets.LesionsDataModule`` as batches of one, prepared on the
    device case by case: upload (a case with an affine on its native grid, then msl_regrid), msl_foreground_box_mc,
    crop, msl_normalize_nonzero, msl_augment_fit_mc with the identity row into a (1, C) + spatial_size batch,
    msl_instance_boxes on the fitted mask - the kernels ``LesionCache`` runs, on one case at a time, so nothing but the
    case being prepared and the batches handed out is resident.  A batch of a case with an affine also carries
    "native_shape" and "plan" (its ``RegridPlan``), as lists.

    ``batches(indices)`` yields ``{"img", "subject", "boxes", "labels", "crop_origin", "crop_shape", "full_shape"}`` (and
    "seg": [boxes, labels]) in the order of ``indices`` (default: every case): "img" a device tensor, valid until the
    next batch is drawn (``predict_batches`` copies it into its own buffer at once); "boxes" / "labels" the ground truth of the host data set on the host, bit for bit; the
    geometry keys as lists, as ``collate_fn`` passes them.  The six ints of the foreground box are the only host round
    trip per case: the ground-truth counts of case k come over in pinned memory and are read after case k + 1's box read
    has synchronised the stream, so the feed prepares one case ahead of the one it hands out.  With
    ``LSSD3D.predict_batches(feed.batches(), depth)`` at most depth + 1 cases are resident."""

    def __init__(self, dataset, device, max_objects_per_image=64, max_runs_per_image=MAX_RUNS_PER_IMAGE):
        if dataset.predict_dataset is None:
            raise ValueError("LesionPredictFeed needs a data module after setup()")
        self.dataset, self.device = dataset, torch.device(device)
        self.target, self.channels = tuple(dataset.spatial_size), len(dataset.input_images)
        self.capacity = int(max_objects_per_image)
        dev, C = self.device, self.channels
        self._box = torch.zeros(6, dtype=torch.int32, device=dev)
        self._row = torch.from_numpy(fit_rows([0], [(([0, 1, 2], [0, 0, 0]), [])]).reshape(-1)).to(dev)  # the identity row
        self._slots = [{"img": torch.empty((1, C) + self.target, dtype=torch.float32, device=dev),
                        "seg": torch.empty((1,) + self.target, dtype=torch.int16, device=dev),
                        "box": _box_stage(dataset, 1, self.target, self.capacity, dev, max_runs_per_image,
                                          "LesionPredictFeed"),
                        "gb": torch.zeros((max(self.capacity, 1), 6), dtype=torch.float32, pin_memory=True),
                        "gl": torch.zeros(max(self.capacity, 1), dtype=torch.int64, pin_memory=True),
                        "off": torch.zeros(2, dtype=torch.int32, pin_memory=True)} for _ in range(2)]

    def __len__(self):
        return len(self.dataset.predict_dataset)

    def __iter__(self):
        return self.batches()

    def _start(self, pos, k):
        """Everything of case ``pos`` enqueued; the box read is the one wait."""
        ds, dev, C, stream = self.dataset.predict_dataset, self.device, self.channels, _stream(self.device)
        vol, mask, plan = _case_on_device(ds, pos, dev, "LesionPredictFeed")
        full_shape = tuple(int(v) for v in mask.shape)
        _foreground_box(vol, self.dataset.margin, self._box, stream)
        b = self._box.cpu().tolist()  # the one read that sizes the crop
        sl = tuple(slice(b[a], b[3 + a]) for a in range(3))
        shape = tuple(b[3 + a] - b[a] for a in range(3))
        ci = vol[(...,) + sl].contiguous()
        cs = mask[sl].contiguous()
        del vol, mask
        size = int(np.prod(shape))
        slot = self._slots[k % 2]
        if size:
            _lib.call("msl_normalize_nonzero", ptr(ci), C, size, stream)
        table = torch.tensor([[0, *shape]], dtype=torch.int64).to(dev)
        _lib.call("msl_augment_fit_mc", ptr(ci), ptr(cs), max(size, 1), C, ptr(table), 1, ptr(self._row), 1,
                  *self.target, ptr(slot["img"]), ptr(slot["seg"]), stream)
        box = slot["box"]
        box.launch(slot["seg"], stream)
        slot["gb"].copy_(box.gb, non_blocking=True)
        slot["gl"].copy_(box.gl, non_blocking=True)
        slot["off"].copy_(box.obj_off, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        # (ci, cs and table are released on return: the caching allocator hands a freed block to this stream's later work
        #  only, which is ordered behind these launches)
        return {"slot": slot, "subject": ds.subjects[pos], "crop_origin": tuple(b[:3]), "crop_shape": shape,
                "full_shape": full_shape, "plan": plan, "done": done}

    def _finish(self, h):
        slot = h["slot"]
        slot["box"].raise_on_overflow()
        n = int(slot["off"][1])
        boxes, labels = [slot["gb"][:n].clone()], [slot["gl"][:n].clone()]
        out = {"img": slot["img"], "seg": [boxes, labels], "boxes": boxes, "labels": labels, "subject": [h["subject"]],
               "crop_origin": [h["crop_origin"]], "crop_shape": [h["crop_shape"]], "full_shape": [h["full_shape"]]}
        if h["plan"] is not None:  # as the host samples of a case with an affine
            out["native_shape"], out["plan"] = [tuple(h["plan"].src_shape)], [h["plan"]]
        return out

    def batches(self, indices=None):
        pending = None
        for k, pos in enumerate(range(len(self)) if indices is None else indices):
            cur = self._start(int(pos), k)  # (its box read has waited for everything of the pending case)
            if pending is not None:
                yield self._finish(pending)
            pending = cur
        if pending is not None:
            pending["done"].synchronize()
            yield self._finish(pending)
