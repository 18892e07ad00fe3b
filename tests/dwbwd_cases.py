"""Case tables of tests/test_gpu_dwbwd.py (shared with tests/test_dwbwd_ref_cpu.py, which proves at the same shapes that every
bound of tests/dwbwd_ref.py accepts honest fp32 and rejects eight kinds of wrong kernel).  Plain data, nothing here imports the
package.  A case is ``(id, entry, bf16, N, C, (D, H, W), stride, accumulate, opts)``; the id starts with the kernel path the shape
must reach, and ``opts["kind"]`` is the DwKind msl_dwconv_route_kind has to answer for it (the patch kernels have no route: their
``blocks`` - workgroups per image and channel - are asserted through the *_num_partials queries instead).

opts: kind (route), op (route query's op), path (key of dwbwd_ref.BWW_DEPTH / SUMS_DEPTH), blocks, yprev (bf16 patch kernel with
BatchNorm sums), taps_t (one-pass: ask for the (27, C) weight transpose), cond (ill-conditioned operands), nan ((n, c, od, oh, ow)
of one NaN in dy), affine (weight gradient with the input's BatchNorm folded in), dw (immediate fold into dw)."""
import zlib

import torch

from tests import bn_ref as R
from tests.dwbwd_ref import OP_BWD_DATA, OP_BWD_WEIGHT, bf16_round, num_blocks, out_dims


def _c(id_, entry, bf16, N, C, dims, stride, acc=0, **opts):
    return (id_, entry, bf16, N, C, dims, stride, acc, opts)


def _both(id_, entry, bf16, N, C, dims, stride, **opts):
    return [_c(f"{id_}-acc{a}", entry, bf16, N, C, dims, stride, a, **opts) for a in (0, 1)]


def _shape(N, C, dims):
    return f"{N}x{C}x" + "x".join(str(d) for d in dims)


# ------------------------------------------------------------------------------------------------- msl_dwconv_bwd_data (fp32)
BWD_DATA_CASES = []
# Wave, stride 1: every slab length (D = 5: SLAB 2, ragged last slab; 3: SLAB 1; 9: SLAB 4, ragged; 17: SLAB 8, ragged) and 4 / 1 / 1 / 1
# channels per wave
for _N, _C, _d in ((2, 16, (5, 4, 4)), (1, 4, (3, 8, 8)), (1, 2, (9, 16, 16)), (1, 1, (17, 16, 16))):
    BWD_DATA_CASES += _both(f"wave-s1:{_shape(_N, _C, _d)}", "bwd_data", 0, _N, _C, _d, 1, kind="wave", op=OP_BWD_DATA)
# Resident, stride 1; the second is a wave-shaped plane whose channel count (3, not a multiple of 4) the wave kernel refuses
for _N, _C, _d in ((1, 4, (6, 12, 16)), (1, 3, (4, 4, 4))):
    BWD_DATA_CASES += _both(f"resident-s1:{_shape(_N, _C, _d)}", "bwd_data", 0, _N, _C, _d, 1, kind="resident", op=OP_BWD_DATA)
BWD_DATA_CASES += _both("datavec:1x2x3x32x32", "bwd_data", 0, 1, 2, (3, 32, 32), 1, kind="datavec", op=OP_BWD_DATA)
BWD_DATA_CASES += _both("datanaive-s1:1x3x5x7x9", "bwd_data", 0, 1, 3, (5, 7, 9), 1, kind="datanaive", op=OP_BWD_DATA)
BWD_DATA_CASES += _both("datanaive-s2:1x3x5x7x9", "bwd_data", 0, 1, 3, (5, 7, 9), 2, kind="datanaive", op=OP_BWD_DATA)
# the patch kernel: one patch; odd D and H (patches half outside); 576 patches = three workgroups, the last a quarter full; even
S2PATCH_SHAPES = ((2, 2, (1, 1, 4)), (1, 3, (5, 7, 8)), (1, 2, (7, 18, 64)), (2, 4, (8, 8, 8)))
for _N, _C, _d in S2PATCH_SHAPES:
    BWD_DATA_CASES += _both(f"s2patch:{_shape(_N, _C, _d)}", "bwd_data", 0, _N, _C, _d, 2, kind="s2patch", op=OP_BWD_DATA,
                            blocks=num_blocks(_d, 256))
BWD_DATA_CASES.append(_c("s2patch:cond:1x3x5x7x8", "bwd_data", 0, 1, 3, (5, 7, 8), 2, 1, kind="s2patch", op=OP_BWD_DATA, cond=True,
                         blocks=1))
BWD_DATA_CASES.append(_c("wave-s1:cond:1x4x3x8x8", "bwd_data", 0, 1, 4, (3, 8, 8), 1, 0, kind="wave", op=OP_BWD_DATA, cond=True))

# ------------------------------------------------------------------------------------------------- msl_dwconv_bwd_data_bf16
BWD_DATA_BF16_CASES = []
for _p, _k, _N, _C, _d, _s in (("wave", "wave", 2, 16, (5, 4, 4), 1), ("tiled-s1", "tiled", 1, 3, (3, 9, 33), 1),
                               ("tiled-s2", "tiled_s2", 1, 2, (5, 9, 66), 2), ("tiled-s2", "tiled_s2", 1, 3, (5, 7, 9), 2),
                               ("s2patch", "s2patch", 1, 3, (5, 7, 8), 2)):
    BWD_DATA_BF16_CASES += _both(f"bf16-{_p}:{_shape(_N, _C, _d)}", "bwd_data_bf16", 1, _N, _C, _d, _s, kind=_k, op=OP_BWD_DATA)

# ------------------------------------------------------------------------------------------------- patch kernel + BatchNorm sums
# (2, 3, (5, 7, 8)) joins the list: C = 3 with N = 2, so p = (nc / C) gridDim.x + blockIdx.x differs from every wrong spelling
PATCH_BN_SHAPES = S2PATCH_SHAPES + ((2, 3, (5, 7, 8)), (2, 3, (7, 18, 64)))
PATCH_BN_CASES = []
for _N, _C, _d in PATCH_BN_SHAPES:
    _o = dict(path="patch", blocks=num_blocks(_d, 256))
    PATCH_BN_CASES += _both(f"patch-bn:{_shape(_N, _C, _d)}", "patch_bn", 0, _N, _C, _d, 2, **_o)
    PATCH_BN_CASES += _both(f"patch-bn-bf16:{_shape(_N, _C, _d)}", "patch_bf16", 1, _N, _C, _d, 2, yprev=True, **_o)
    PATCH_BN_CASES += _both(f"patch-bf16:{_shape(_N, _C, _d)}", "patch_bf16", 1, _N, _C, _d, 2, yprev=False, **_o)
PATCH_BN_CASES.append(_c("patch-bn:nan:1x3x5x7x8", "patch_bn", 0, 1, 3, (5, 7, 8), 2, 1, path="patch", blocks=1, nan=(0, 1, 1, 2, 1)))
PATCH_BN_CASES.append(_c("patch-bn:cond:1x3x5x7x8", "patch_bn", 0, 1, 3, (5, 7, 8), 2, 0, path="patch", blocks=1, cond=True))

# ------------------------------------------------------------------------------------------------- the one-pass kernel
# one patch; odd D and H with N = 2, C = 3; odd D and H, three columns of patches; 1100 patches: the second workgroup has 76 live
# threads in its first pass and none after; even extents
ONEPASS_SHAPES = ((1, 2, (1, 1, 4)), (2, 3, (5, 7, 8)), (1, 4, (7, 7, 12)), (1, 1, (10, 22, 80)), (2, 8, (8, 8, 8)))
ONEPASS_CASES = []
for _N, _C, _d in ONEPASS_SHAPES:
    _o = dict(path="onepass", blocks=num_blocks(_d, 1024))
    ONEPASS_CASES += _both(f"onepass-data:{_shape(_N, _C, _d)}", "onepass_data", 0, _N, _C, _d, 2, **_o)
    for _t in (False, True):
        _n = "-taps" if _t else ""
        ONEPASS_CASES.append(_c(f"onepass{_n}:{_shape(_N, _C, _d)}", "onepass", 0, _N, _C, _d, 2, 0, taps_t=_t, **_o))
        ONEPASS_CASES.append(_c(f"onepass-bf16{_n}:{_shape(_N, _C, _d)}", "onepass_bf16", 1, _N, _C, _d, 2, 0, taps_t=_t, **_o))
ONEPASS_CASES.append(_c("onepass-data:nan:2x3x5x7x8", "onepass_data", 0, 2, 3, (5, 7, 8), 2, 0, path="onepass", blocks=1,
                        nan=(1, 2, 1, 1, 2)))
ONEPASS_CASES.append(_c("onepass-data:cond:1x4x7x7x12", "onepass_data", 0, 1, 4, (7, 7, 12), 2, 1, path="onepass", blocks=1, cond=True))

# ------------------------------------------------------------------------------------------------- msl_dwconv_bwd_weight (+ _bf16)
BWW_CASES = []
for _p, _k, _path, _N, _C, _d, _s in (
        ("chunks-via-naive", "chunks", "chunks", 1, 2, (5, 15, 30), 1),   # W % 4 != 0 -> Naive -> Chunks; 2250 outputs: three chunks
        ("chunks-via-naive", "chunks", "chunks", 2, 64, (4, 4, 5), 1),    # a tail volume: one short chunk, 64 channels, two images
        # a plane lds_plan takes (W % 4 == 0, not square: no wave) with 16 items per channel: G = 16 > 4 sends it to Chunks
        ("chunks-via-G>4", "chunks", "chunks", 1, 16, (2, 4, 8), 1),
        ("resident-G<=4", "resident", "resident", 1, 4, (6, 12, 16), 1),
        ("resident-G<=4", "resident", "resident", 1, 3, (5, 12, 16), 2),
        # Stream: planes of >= 1024 voxels; (1, 4) while an output plane has <= 256 items and an input plane <= 1024 float4
        ("stream<2,1,4>", "stream", "stream", 1, 3, (9, 40, 48), 2),     # 120 items, 480 float4
        ("stream<1,1,4>", "stream", "stream", 1, 2, (5, 32, 32), 1),     # 256 items: the last shape of (1, 4) at stride 1
        ("stream<1,4,12>", "stream", "stream", 1, 2, (3, 40, 48), 1),    # 480 items
        ("stream<2,4,12>", "stream", "stream", 1, 2, (5, 68, 64), 2),    # 272 items, 1088 float4 (in place of 7 x 96 x 96)
        ("wave-s1", "wave", "wave_s1", 2, 16, (9, 4, 4), 1),
        ("wave-s2", "wave", "wave_s2", 1, 4, (7, 16, 16), 2),
        ("wave-s2-split-plane", "wave", "wave_s2", 1, 2, (6, 64, 64), 2)):
    for _dw in (True, False):
        BWW_CASES.append(_c(f"bww:{_p}:{_shape(_N, _C, _d)}-s{_s}-{'dw' if _dw else 'deferred'}", "bww", 0, _N, _C, _d, _s, 0, kind=_k,
                            op=OP_BWD_WEIGHT, path=_path, dw=_dw, affine=True))
BWW_CASES.append(_c("bww:chunks:cond:1x2x5x15x30-s1", "bww", 0, 1, 2, (5, 15, 30), 1, 0, kind="chunks", op=OP_BWD_WEIGHT, path="chunks",
                    dw=True, affine=False, cond=True))
# bf16: one shape per route of tests/test_gpu_bf16.py::test_dw_bwd_bf16, and a ragged tile
for _p, _k, _path, _N, _C, _d, _s in (("tiled-s2", "tiled", "tiled_bf16", 1, 4, (10, 40, 40), 2),
                                      ("tiled-s1", "tiled", "tiled_bf16", 1, 3, (7, 6, 6), 1),
                                      ("wave-s1", "wave", "wave_s1", 2, 16, (16, 16, 16), 1),
                                      ("wave-s2", "wave", "wave_s2", 1, 8, (7, 32, 32), 2),
                                      ("tiled-s1-ragged", "tiled", "tiled_bf16", 1, 3, (3, 9, 33), 1)):
    BWW_CASES.append(_c(f"bww-bf16:{_p}:{_shape(_N, _C, _d)}-s{_s}", "bww_bf16", 1, _N, _C, _d, _s, 0, kind=_k, op=OP_BWD_WEIGHT,
                        path=_path, dw=False, affine=True))

FINALIZE_NP = (1, 63, 64, 65, 448, 449, 512, 513, 1100)  # the 8-way unrolled loop starts at NP = 449; 64-lane tails on both sides

ALL_CASES = BWD_DATA_CASES + BWD_DATA_BF16_CASES + PATCH_BN_CASES + ONEPASS_CASES + BWW_CASES


def ids(cases):
    return [c[0] for c in cases]


# ------------------------------------------------------------------------------------------------- data of a case
def gen(seed):
    return torch.Generator().manual_seed(seed)


def make_data(case):
    """Host tensors of a case (CPU, fp32; rounded to bf16 values on bf16 storage): dy, w (C, 27), y (the producer's raw output /
    the weight gradient's input x), vec (4, C) [scale, shift, mean, invstd] of y's batch statistics, old (the gradient already in
    g_in when ``accumulate``)."""
    id_, entry, bf16, N, C, dims, stride, acc, o = case
    g = gen(zlib.crc32(id_.split(":")[0].encode() + repr((N, C, dims, stride)).encode()))
    od = out_dims(dims, stride)
    dy = torch.randn((N, C) + od, generator=g)
    w = torch.randn((C, 27), generator=g) * 0.4
    y = torch.randn((N, C) + tuple(dims), generator=g) * 1.5 + 0.3
    y[..., -1] = y[..., -1].abs() + 2.0  # the last column is alive behind the ReLU: an error at the W edge reaches the sums
    y[..., 0] = 0.05                     # the first is positive and below the mean: y > 0 and fma(y, sc, sh) > 0 disagree there
    old = torch.randn((N, C) + tuple(dims), generator=g)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    if o.get("cond"):
        # operands of a large common offset and weights that sum to zero: |result| << absdot
        dy = 100.0 + torch.randn(dy.shape, generator=g) * 1e-2
        w = w - w.mean(1, keepdim=True)
        if entry == "bww":
            y = y - y.mean((0, 2, 3, 4), keepdim=True)
    if bf16:
        dy, y, old = bf16_round(dy), bf16_round(y), bf16_round(old)
    if o.get("nan"):
        dy[o["nan"]] = float("nan")
    vec = R.host_vectors(y, gamma, beta)
    return dict(dy=dy, w=w, y=y, old=old if acc else None, vec=vec)
