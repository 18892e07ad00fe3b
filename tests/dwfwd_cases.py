"""Case tables of tests/test_gpu_dwfwd.py (shared with tests/test_dwfwd_ref_cpu.py, which proves at the same shapes that every
bound of tests/dwfwd_ref.py accepts honest fp32 and rejects ten kinds of wrong kernel).  Plain data, nothing here imports the
package.  A case is ``(id, entry, bf16, N, C, (D, H, W), stride, opts)``; the id starts with the kernel path the shape must reach.

entry: "train" (a forward WITH statistics: msl_dwconv_fwd / msl_dwconv_fwd_bf16), "eval" (the same entries without partials),
"small_bf16" (msl_dwconv_fwd_small_eval_bf16), "fold" (msl_dwconv_fwd_fold / msl_dwconv_fwd_wave_bf16_fold).
opts: route (wave, stream, resident, naive, tiled, rows_eval, small_eval), force_naive, ipt (the stream instantiation), in_np (fold:
producer partial count, 6 = serial fold, 70 = wave-tree fold).  Every train / eval case runs with and without the input affine."""
import zlib

import torch

from tests import bn_ref as R
from tests.dwfwd_ref import bf16_rne


def _c(id_, entry, bf16, N, C, dims, stride, **opts):
    return (id_, entry, bf16, N, C, dims, stride, opts)


def _shape(N, C, dims, stride):
    return f"{N}x{C}x" + "x".join(str(d) for d in dims) + f"-s{stride}"


# planes 4^2, 8^2, 16^2; slab lengths 2 (4 x 4 x 4), 4 with a ragged last slab (D = 9), 2 ragged (5), 8 ragged (20), 1 (D = 1, 3)
WAVE_S1 = ((2, 64, (4, 4, 4)), (2, 16, (9, 4, 4)), (1, 8, (5, 8, 8)), (1, 8, (20, 8, 8)), (1, 2, (1, 16, 16)), (1, 4, (3, 16, 16)))
# planes 8^2 (8 channels a wave), 16^2 (2), 32^2 (two waves a plane), 64^2 (eight waves: one partial per four); OD 1, 3, 4, 9 (slab 4,
# ragged), 3, and 5 (slab 2, ragged)
WAVE_S2 = ((3, 8, (2, 8, 8)), (1, 8, (5, 8, 8)), (1, 4, (7, 16, 16)), (1, 2, (18, 32, 32)), (1, 2, (6, 64, 64)), (1, 4, (9, 16, 16)))
FOLD = (((2, 16, (9, 4, 4)), 1), ((1, 8, (5, 8, 8)), 1), ((3, 8, (2, 8, 8)), 2), ((1, 2, (18, 32, 32)), 2))  # four channels / one / eight / one per wave
# (shape, stride, items and prefetch registers per thread): both instantiations at both strides, SLAB = 4 not dividing OD = 9 / 5 / 5
STREAM = (((1, 3, (9, 40, 48)), 1, 4), ((1, 4, (10, 40, 40)), 2, 1), ((1, 2, (7, 96, 96)), 2, 4), ((1, 2, (5, 32, 32)), 1, 1))
RESIDENT = (((1, 4, (6, 12, 16)), 1), ((2, 8, (12, 24, 24)), 2), ((2, 16, (32, 16, 32)), 2))  # G = 1, 2, 4
# W % 4 != 0; OW % 4 != 0; one voxel; 4500 outputs an image: two statistics chunks, the second a tenth full
NAIVE = (((1, 4, (5, 7, 9)), 2), ((2, 4, (6, 6, 6)), 1), ((1, 1, (1, 1, 1)), 1), ((1, 2, (5, 30, 30)), 1))
# rows of 2, 3, 10, 64, 5 and 2 lanes; D = 2; odd H at stride 1
ROWS_EVAL = (((2, 3, (2, 6, 8)), 2), ((1, 3, (5, 12, 12)), 2), ((1, 2, (6, 20, 40)), 2), ((1, 2, (17, 10, 256)), 2), ((1, 3, (5, 7, 20)), 1),
             ((2, 4, (2, 5, 8)), 1), ((1, 4, (7, 24, 24)), 2), ((2, 8, (9, 24, 24)), 1))  # and 6 lanes, at both strides
# one voxel; odd everything; stride 2; 420 voxels; an image of exactly 1024 LDS cells
SMALL_EVAL = (((1, 2, (1, 1, 1)), 1), ((1, 5, (3, 5, 7)), 1), ((2, 7, (6, 6, 6)), 2), ((1, 9, (5, 6, 14)), 1), ((1, 2, (6, 6, 14)), 1))
# 16-byte staging with two W tiles; scalar staging with two W tiles (W = 36: % 4 == 0 but % 8 != 0, 35: odd, 67 at stride 2: OW = 34);
# several H and D tiles with ragged ends; one voxel; C = 3
TILED = (((1, 2, (3, 10, 40)), 1), ((1, 2, (5, 9, 72)), 2), ((1, 2, (3, 9, 36)), 1), ((1, 2, (3, 9, 35)), 1), ((1, 2, (4, 7, 67)), 2),
         ((1, 3, (5, 19, 12)), 1), ((2, 2, (7, 21, 10)), 2), ((1, 1, (1, 1, 1)), 1), ((2, 3, (7, 6, 6)), 1))

TRAIN_CASES, EVAL_CASES, FOLD_CASES = [], [], []
for _N, _C, _d in WAVE_S1:
    for _b in (0, 1):
        TRAIN_CASES.append(_c(f"wave-s1{'-bf16' * _b}:{_shape(_N, _C, _d, 1)}", "train", _b, _N, _C, _d, 1, route="wave"))
for _N, _C, _d in WAVE_S2:
    for _b in (0, 1):
        TRAIN_CASES.append(_c(f"wave-s2{'-bf16' * _b}:{_shape(_N, _C, _d, 2)}", "train", _b, _N, _C, _d, 2, route="wave"))
for (_N, _C, _d), _s, _ipt in STREAM:
    TRAIN_CASES.append(_c(f"stream<{_s},{_ipt},{4 if _ipt == 1 else 12}>:{_shape(_N, _C, _d, _s)}", "train", 0, _N, _C, _d, _s,
                          route="stream", ipt=_ipt))
for (_N, _C, _d), _s in RESIDENT:
    TRAIN_CASES.append(_c(f"resident:{_shape(_N, _C, _d, _s)}", "train", 0, _N, _C, _d, _s, route="resident"))
for (_N, _C, _d), _s in NAIVE:
    TRAIN_CASES.append(_c(f"naive:{_shape(_N, _C, _d, _s)}", "train", 0, _N, _C, _d, _s, route="naive"))
# the generic kernel forced on shapes with a route of their own (resident, wave)
TRAIN_CASES.append(_c("naive-forced:1x4x6x12x16-s1", "train", 0, 1, 4, (6, 12, 16), 1, route="naive", force_naive=1))
TRAIN_CASES.append(_c("naive-forced:1x8x5x8x8-s2", "train", 0, 1, 8, (5, 8, 8), 2, route="naive", force_naive=1))
for (_N, _C, _d), _s in TILED:
    TRAIN_CASES.append(_c(f"tiled-bf16:{_shape(_N, _C, _d, _s)}", "train", 1, _N, _C, _d, _s, route="tiled"))

for (_N, _C, _d), _s in ROWS_EVAL:
    for _b in (0, 1):
        EVAL_CASES.append(_c(f"rows-eval{'-bf16' * _b}:{_shape(_N, _C, _d, _s)}", "eval", _b, _N, _C, _d, _s, route="rows_eval"))
for (_N, _C, _d), _s in SMALL_EVAL:
    for _b in (0, 1):
        EVAL_CASES.append(_c(f"small-eval{'-bf16' * _b}:{_shape(_N, _C, _d, _s)}", "eval", _b, _N, _C, _d, _s, route="small_eval"))
    EVAL_CASES.append(_c(f"small-eval-bf16-own-entry:{_shape(_N, _C, _d, _s)}", "small_bf16", 1, _N, _C, _d, _s, route="small_eval"))

for (_N, _C, _d), _s in FOLD:
    for _b in (0, 1):
        for _np in (6, 70):
            FOLD_CASES.append(_c(f"fold-wave-s{_s}{'-bf16' * _b}-np{_np}:{_shape(_N, _C, _d, _s)}", "fold", _b, _N, _C, _d, _s, route="wave",
                                 in_np=_np))
# the fp32 fold entry takes every route: stream (the workgroup folds one channel), resident (G = 2 channels), naive
for _r, (_N, _C, _d), _s, _np in (("stream", (1, 4, (10, 40, 40)), 2, 70), ("resident", (2, 8, (12, 24, 24)), 2, 6), ("naive", (1, 4, (5, 7, 9)), 2, 70)):
    FOLD_CASES.append(_c(f"fold-{_r}-np{_np}:{_shape(_N, _C, _d, _s)}", "fold", 0, _N, _C, _d, _s, route=_r, in_np=_np))

ALL_CASES = TRAIN_CASES + EVAL_CASES + FOLD_CASES
FOLD_COUNT = 1000.0  # element count of the producer's statistics
EPS = 1e-5


def ids(cases):
    return [c[0] for c in cases]


def gen(seed):
    return torch.Generator().manual_seed(seed)


def make_data(case):
    """Host tensors of a case (CPU, fp32; x rounded to bf16 values on bf16 storage): x, w (C, 27), sc / sh (the explicit input
    affine), and for a fold case the producer's partials (2, C, in_np) fp64 with gamma and beta."""
    id_, entry, bf16, N, C, dims, stride, o = case
    g = gen(zlib.crc32(repr((bf16, N, C, dims, stride)).encode()))
    x = torch.randn((N, C) + tuple(dims), generator=g) * 1.5 + 0.3
    w = torch.randn((C, 27), generator=g) * 0.4
    sc = torch.rand(C, generator=g) + 0.5
    sh = torch.randn(C, generator=g) * 0.3
    sh[0] = 0.25  # act(0) > 0 on one channel at least: a halo that holds act(0) differs from a zero halo
    # the first voxel is alive behind the ReLU on even channels and dead on odd ones, so that a map of one voxel shows both
    x[:, 0::2, 0, 0, 0] = x[:, 0::2, 0, 0, 0].abs() + 0.5
    x[:, 1::2, 0, 0, 0] = -x[:, 1::2, 0, 0, 0].abs() - 3.0
    if bf16:
        x = bf16_rne(x)
    d = dict(x=x, w=w, sc=sc, sh=sh)
    if entry == "fold":
        n = o["in_np"]
        ps = torch.randn((C, n), generator=g, dtype=torch.float64) * 3.0
        pq = ps.abs() * 2.0 + torch.rand((C, n), generator=g, dtype=torch.float64) * 40.0 + 20.0
        d.update(part_in=torch.stack([ps, pq]).contiguous(), gamma=torch.rand(C, generator=g) + 0.5,
                 beta=torch.randn(C, generator=g) * 0.3 + 0.2)
    return d


def host_fold_vectors(d):
    """(scale, shift) fp32 of a fold case made on the host in float64 (the CPU test's stand-in for msl_bn_finalize's vectors)."""
    p = d["part_in"]
    r = R.finalize_ref(R.exact_sum(p[0]), R.exact_sum(p[1]), FOLD_COUNT, d["gamma"], d["beta"], EPS, 0.0)
    return R.f32(r["scale"]), R.f32(r["shift"])
