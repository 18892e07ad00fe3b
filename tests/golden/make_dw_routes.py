"""Mint ``dw_routes.npz``: what every host-only depthwise query answers for a fixed list of shapes, taken at the commit
BEFORE the depthwise host code got its single route (so the file pins the kernel choice and the partial counts of the old
cascades):

    python -m tests.golden.make_dw_routes

``shapes`` is an int32 (n, 6) array of (N, C, D, H, W, stride), ``answers`` an int32 (n, len(QUERIES)) array, one column per
query in the order of QUERIES (the two stride-2-only queries take no stride and are asked for every row).  No GPU is needed:
the queries are host arithmetic.  ``tests/test_dw_routes_cpu.py`` asks the library under test the same questions and
compares.  Re-mint only when a shape is meant to change its kernel.
"""
import os

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dw_routes.npz")

QUERIES = (  # name, takes a stride
    ("msl_dwconv_fwd_variant", True),
    ("msl_dwconv_fwd_num_partials", True),
    ("msl_dwconv_fwd_bf16_num_partials", True),
    ("msl_dwconv_wave_num_partials", True),
    ("msl_dwconv_fwd_eval_rows_ok", True),
    ("msl_dwconv_bwd_weight_num_partials", True),
    ("msl_dwconv_bwd_data_bnreduce_num_partials", False),
    ("msl_dwconv_s2_bwd_bnreduce_bww_num_partials", False),
)

# (N, C, (D, H, W), stride): the depthwise parametrisations of tests/test_gpu_kernels.py and tests/test_gpu_bf16.py
TEST_SHAPES = [
    # DW_CASES
    (1, 4, (10, 40, 40), 2), (1, 3, (9, 40, 48), 1), (1, 2, (7, 96, 96), 2), (2, 16, (32, 16, 32), 2), (1, 4, (6, 12, 16), 1),
    (2, 8, (12, 24, 24), 2), (1, 2, (6, 64, 64), 2), (2, 8, (16, 16, 16), 2), (2, 64, (8, 8, 8), 2), (2, 16, (32, 32, 32), 2),
    (1, 4, (7, 16, 16), 2), (1, 8, (5, 8, 8), 2), (1, 2, (18, 32, 32), 2), (3, 8, (2, 8, 8), 2), (2, 8, (16, 16, 16), 1),
    (2, 64, (4, 4, 4), 1), (1, 8, (5, 8, 8), 1), (1, 4, (3, 16, 16), 1), (2, 16, (9, 4, 4), 1), (1, 8, (20, 8, 8), 1),
    (1, 2, (1, 16, 16), 1), (3, 32, (2, 4, 4), 1), (2, 4, (6, 6, 6), 1), (2, 4, (4, 4, 4), 2), (1, 4, (5, 7, 9), 2),
    # test_dw_fwd_eval_rows (+ the two shapes it asserts are refused), test_dw_fwd_eval_rows_bf16
    (2, 8, (10, 96, 96), 2), (1, 16, (10, 48, 48), 2), (1, 4, (7, 24, 24), 2), (1, 3, (5, 12, 12), 2), (1, 2, (6, 20, 40), 2),
    (2, 3, (2, 6, 8), 2), (1, 2, (17, 10, 256), 2), (1, 5, (9, 96, 24), 2), (2, 8, (9, 24, 24), 1), (1, 16, (12, 12, 12), 1),
    (1, 3, (5, 7, 20), 1), (1, 2, (3, 33, 96), 1), (2, 4, (2, 5, 8), 1), (1, 2, (6, 9, 256), 1), (1, 2, (6, 12, 6), 1),
    # test_dw_fwd_eval_small_maps (fp32 and bf16)
    (2, 512, (6, 6, 6), 1), (2, 7, (6, 6, 6), 2), (1, 5, (3, 5, 7), 1), (3, 3, (8, 8, 6), 2), (1, 2, (1, 1, 1), 1),
    (1, 9, (5, 6, 14), 1), (1, 1, (16, 16, 16), 1),
    # test_dw_fwd_fold_matches_explicit_affine
    (2, 8, (8, 8, 8), 1), (2, 32, (4, 4, 4), 1), (1, 16, (5, 4, 4), 1), (2, 4, (6, 12, 16), 1), (2, 16, (8, 8, 8), 2),
    (2, 4, (8, 16, 16), 2), (1, 2, (8, 32, 32), 2), (1, 2, (5, 96, 96), 2),
    # test_dw_bwd
    (2, 4, (8, 16, 16), 1), (1, 3, (5, 7, 9), 2), (1, 3, (5, 7, 9), 1), (1, 2, (9, 12, 20), 2),
    # test_dw_s2_bwd_data_bnreduce_bww_matches_autograd, test_dw_s2_bwd_data_with_bn_reduce_bf16
    (2, 16, (8, 8, 8), 2), (1, 8, (10, 14, 20), 2), (3, 4, (6, 6, 36), 2), (2, 64, (32, 32, 32), 2), (1, 4, (32, 32, 32), 2),
    (2, 4, (6, 10, 12), 2),
    # test_dw_fwd_bf16, test_dw_bwd_bf16
    (1, 3, (7, 6, 6), 1), (2, 16, (12, 12, 12), 2), (1, 2, (5, 7, 9), 2), (1, 2, (3, 96, 96), 2), (1, 4, (64, 64, 64), 2),
    (2, 8, (32, 32, 32), 2), (2, 16, (16, 16, 16), 1), (2, 16, (16, 16, 16), 2), (2, 32, (8, 8, 8), 1), (2, 32, (8, 8, 8), 2),
    (1, 8, (5, 16, 16), 1), (1, 8, (7, 32, 32), 2), (2, 32, (16, 16, 16), 2), (2, 64, (8, 8, 8), 1), (1, 2, (4, 128, 128), 2),
    (1, 4, (6, 10, 12), 2),
]

# planes (H, W) on both sides of every threshold of the planners:
#  square 4 .. 260: the wave kernels' 4/8/16 (stride 1) and 8/16/32/64 (stride 2) and their neighbours 32 / 128, rows up to 256
#  H*W = 1024 (stream / resident), Lp = 1024 / 1088 items (ipt 4 / 5), 12288 / 12544 cells at stride 2 (lpt 12 / 13),
#  W % 4 != 0, odd H, rows of 256 / 260
PLANES = [(s, s) for s in (2, 4, 6, 8, 12, 16, 24, 28, 32, 40, 48, 64, 96, 112, 128, 192, 256, 260)] + [
    (16, 32), (32, 16), (31, 32), (16, 64), (15, 64), (8, 124), (40, 48), (64, 68), (96, 128), (28, 32), (4, 8), (8, 4),
    (12, 16), (7, 9), (5, 8), (9, 12), (33, 96), (10, 256), (9, 260), (6, 10), (3, 1024), (2, 512)]
DEPTHS = (1, 2, 3, 4, 8, 15, 31, 63)  # every slab length; odd depths keep the resident slab whole (its LDS limits)
BATCH_CHANNELS = ((1, 1), (2, 3), (1, 4), (2, 8), (1, 12), (4, 64), (2, 512))  # C % cpw != 0, G 1 .. 64 (G > 4)

# maps around the 512-voxel / 1024-cell limits of the small-map kernel
SMALL_MAPS = [(8, 8, 6), (9, 9, 6), (10, 10, 5), (10, 10, 6), (7, 11, 6), (14, 6, 6), (16, 6, 5), (21, 4, 6), (8, 8, 8), (1, 8, 8),
              (1, 22, 22), (1, 23, 22), (2, 16, 16), (4, 11, 11), (8, 9, 7)]

# arguments an entry point refuses (the count queries that do not check them still answer from the planners)
BAD_ARGS = [(0, 4, 8, 8, 8, 1), (-1, 4, 8, 8, 8, 2), (2, 0, 8, 8, 8, 1), (2, -2, 16, 16, 16, 2), (2, 4, 0, 8, 8, 2),
            (2, 4, 8, 0, 0, 1), (2, 4, 8, 8, 0, 1), (2, 4, 8, 0, 8, 2), (2, 4, 8, 8, 8, 3), (1, 2, 6, 64, 64, 3),
            (2, 8, 9, 24, 24, 3), (1, 4, 10, 40, 40, 3), (1, 3, 5, 7, 9, 3), (4, 32, 64, 64, 64, 3)]


def shapes():
    """The fixed list of (N, C, D, H, W, stride), without repeats, in a fixed order."""
    out = []
    for size in (64, 128, 192):  # the seven depthwise layers of a cubic input, batch 1 / 2 / 4
        for n in (1, 2, 4):
            for c, div, stride in ((32, 2, 2), (64, 4, 2), (128, 8, 1), (128, 8, 2), (256, 16, 1), (256, 16, 2), (512, 32, 1)):
                out.append((n, c, size // div, size // div, size // div, stride))
    out += [(n, c) + tuple(d) + (s,) for n, c, d, s in TEST_SHAPES]
    for stride in (1, 2):
        for h, w in PLANES:
            for d in DEPTHS:
                out += [(n, c, d, h, w, stride) for n, c in BATCH_CHANNELS]
        out += [(n, c) + m + (stride,) for m in SMALL_MAPS for n, c in ((1, 2), (2, 16))]
    out += BAD_ARGS
    return list(dict.fromkeys(out))


def answers(lib, shape_list):
    """int32 (n, len(QUERIES)): every query's answer for every shape."""
    out = np.empty((len(shape_list), len(QUERIES)), dtype=np.int32)
    for i, (n, c, d, h, w, s) in enumerate(shape_list):
        for j, (name, strided) in enumerate(QUERIES):
            out[i, j] = getattr(lib, name)(n, c, d, h, w, s) if strided else getattr(lib, name)(n, c, d, h, w)
    return out


def main():
    from mslesions3d_amd import _lib
    sl = shapes()
    ans = answers(_lib.load(), sl)
    np.savez_compressed(OUT, shapes=np.asarray(sl, dtype=np.int32), answers=ans)
    print(f"{OUT}: {len(sl)} shapes x {len(QUERIES)} queries, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
