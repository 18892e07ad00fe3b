"""Mint ``pw_routes.npz``: what every host-only pointwise query answers for a fixed list of shapes, taken at the commit BEFORE
the pointwise host code got its single route (so the file pins the kernel choice, the partial counts and the slab counts of the
old free functions):

    python -m tests.golden.make_pw_routes

``shapes`` is an int32 (n, 4) array of (N, Cin, Cout, S), ``answers`` an int64 (n, len(COLUMNS)) array, one column per query in
the order of COLUMNS (``msl_pwconv_fwd_bf16_num_partials`` takes (N, S) only; ``msl_pwconv_bwd_weight_workspace_bytes`` returns a
size_t, hence the int64 columns).  No GPU is needed: the queries are host arithmetic.  ``tests/test_pw_routes_cpu.py`` asks the
library under test the same questions and compares.  Re-mint only when a shape is meant to change its kernel.
"""
import os

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pw_routes.npz")

QUERIES = (
    "msl_pwconv_fwd_num_partials",
    "msl_pwconv_bwd_weight_nslabs",
    "msl_pwconv_bwd_weight_workspace_bytes",
    "msl_pwconv_bwd_weight_batchable",
    "msl_pwconv_fwd_bf16_num_partials",
    "msl_pwconv_bwd_weight_bf16_nslabs",
    "msl_pwconv_bwd_fused_num_partials",
)
# the eighth recorded answer: msl_pwconv_fwd_num_partials with the roles swapped, (Cin, Cout) -> (Cout, Cin) - the count of the
# bwd-data GEMM's route, which the old code could only be asked for by swapping the arguments by hand
SWAPPED = "msl_pwconv_fwd_num_partials(swapped)"
COLUMNS = QUERIES + (SWAPPED,)
# the queries that count (batchable is yes / no, the fused count is 0 or one workgroup count): each takes >= 6 values on the list
COUNTING = ("msl_pwconv_fwd_num_partials", "msl_pwconv_bwd_weight_nslabs", "msl_pwconv_bwd_weight_workspace_bytes",
            "msl_pwconv_fwd_bf16_num_partials", "msl_pwconv_bwd_weight_bf16_nslabs", SWAPPED)

CHANNELS = (4, 32, 36, 64, 68, 96, 128, 160, 256, 384, 512, 768, 1024)
# lane / tile / strip / chunk boundaries: 8-position groups (bf16 tr), 32- and 64-position chunks (weight gradients), 64 / 128 / 256
# column strips and tiles, the 128-strip and 256-tile thresholds of blocks 1-3, the 4096 waves at which a wave takes two column tiles
SPATIAL = (1, 8, 31, 32, 33, 64, 65, 100, 127, 128, 129, 130, 192, 256, 512, 2048, 4032, 4096, 4100, 8132, 16256, 16384, 16388,
           21888, 32512, 32768, 65536)
# block 1 (Cin 32 -> Cout 64) around the fused backward's 512-strip threshold and S % 128
FUSED_STRIPS = (127, 128, 129, 170, 171, 255, 256, 257, 300, 400, 511, 512, 513, 600, 700, 768, 1000, 1023, 1024, 1025, 1500, 2047,
                2048, 2049, 3000, 4096, 5000, 6000, 8192, 10000, 12000, 16384, 20000, 32768, 40000, 55296)
# the seven pointwise layers of a cubic input of edge `size`: (Cin, Cout, edge divisor)
LAYERS = ((32, 64, 4), (64, 128, 8), (128, 128, 8), (128, 256, 16), (256, 256, 16), (256, 512, 32), (512, 512, 32))
# channel counts an entry point refuses (the count queries that do not check them still answer from the planners; sizes <= 0
# are not asked: the slab planners divide by the chunk count)
BAD_ARGS = [(1, 48, 64, 32), (1, 32, 48, 32), (2, 24, 40, 64), (1, 8, 8, 7), (1, 1056, 8, 8), (1, 544, 32, 64), (1, 32, 30, 64)]


def shapes():
    """The fixed list of (N, Cin, Cout, S), without repeats, in a fixed order."""
    out = []
    for size in (64, 128, 192):
        for n in (1, 2, 4):
            out += [(n, cin, cout, (size // div) ** 3) for cin, cout, div in LAYERS]
    for n in (1, 2, 3, 4):
        for cin in CHANNELS:
            for cout in CHANNELS:
                out += [(n, cin, cout, s) for s in SPATIAL]
        out += [(n, 32, 64, 128 * k + r) for k in FUSED_STRIPS for r in (0, 64)]
    out += BAD_ARGS
    return list(dict.fromkeys(out))


def answers(lib, shape_list):
    """int64 (n, len(COLUMNS)): every query's answer for every shape."""
    out = np.empty((len(shape_list), len(COLUMNS)), dtype=np.int64)
    for i, (n, cin, cout, s) in enumerate(shape_list):
        for j, name in enumerate(QUERIES):
            out[i, j] = getattr(lib, name)(n, s) if name == "msl_pwconv_fwd_bf16_num_partials" else getattr(lib, name)(n, cin, cout, s)
        out[i, len(QUERIES)] = lib.msl_pwconv_fwd_num_partials(n, cout, cin, s)
    return out


def main():
    from mslesions3d_amd import _lib
    sl = shapes()
    ans = answers(_lib.load(), sl)
    np.savez_compressed(OUT, shapes=np.asarray(sl, dtype=np.int32), answers=ans)
    print(f"{OUT}: {len(sl)} shapes x {len(COLUMNS)} answers, {os.path.getsize(OUT)} bytes")
    for j, name in enumerate(COLUMNS):
        print(f"  {name}: {len(np.unique(ans[:, j]))} distinct values")
    print(f"  fused non-zero: {int((ans[:, QUERIES.index('msl_pwconv_bwd_fused_num_partials')] != 0).sum())} shapes")


if __name__ == "__main__":
    main()
