"""Case table of tests/test_gpu_heads.py (shared with tests/test_heads_ref_cpu.py, which proves at the same shapes that every
bound of tests/heads_ref.py accepts honest fp32 and rejects thirteen kinds of wrong kernel).  Plain data; nothing here imports
the package.  A case is ``(id, N, C, (D, H, W), ncls)``; the id starts with the route the shape must reach, as
``heads_ref.route_name`` spells it:

    <forward>/<bwd-data>/<weight gradient>:<shape>
    forward          reg | lds<block width><c: cubic map, t: tiled non-cubic map> . k<K slabs> . m<16-row output tiles>
    bwd-data         reg | lds<w> . c<16-channel tiles per workgroup> x <channel groups> [r: the last group is ragged]
    weight gradient  reg . s<k-steps per wave> | lds<w> . b<blocks per workgroup>, x <slabs> [r: the last workgroup is ragged]

and for the bf16 forward ``bf16.t<k-steps of the tail loop>``.  Every fp32 case runs the forward, bwd-data (fp32 and bf16 output)
and the weight gradient (fp32 and bf16 channels-last feature map); the comments say which edge a shape is in the table for.  The
largest tensor is 3 x 64 x 11 x 16 x 16 (0.54 M elements)."""
import zlib

import torch

CASES = [
    # ---- register-fed everywhere.  S = 105: odd, % 4 = 1 (a k-step of the weight gradient partly out of range), % 16 = 9, % 32 = 9;
    # C = 16: three of the four waves of the bwd-data workgroup exit
    ("reg.k1.m1/reg.c4x1r/reg.s8x1r:1x16x3x5x7", 1, 16, (3, 5, 7), 2),
    # K split in two; two weight-gradient slabs, the second with two whole waves out of range
    ("reg.k2.m1/reg.c4x1r/reg.s8x2r:2x32x3x5x6", 2, 32, (3, 5, 6), 2),
    ("reg.k4.m1/reg.c4x1/reg.s8x1r:2x64x2x2x2", 2, 64, (2, 2, 2), 2),
    # one voxel: every tap but the centre reads the halo; 16 K slabs (two full groups of the finalize's 8-wide loop)
    ("reg.k16.m1/reg.c4x4/reg.s8x1r:1x256x1x1x1", 1, 256, (1, 1, 1), 2),
    # bwd-data with C % 64 != 0 beyond one tile: the second channel block holds one live wave
    ("reg.k1.m1/reg.c4x2r/reg.s8x1r:1x80x3x5x7", 1, 80, (3, 5, 7), 2),
    # nine k-steps per wave (steps > 8), five slabs
    ("reg.k16.m1/reg.c4x4/reg.s9x5:1x256x5x12x12", 1, 256, (5, 12, 12), 2),
    # ---- two output tiles (MT = 2): ncls = 3 (14 padded rows), K split 1 and 2; ncls = 10 (no padded row)
    ("reg.k1.m2/reg.c4x1r/reg.s8x1r:1x16x3x5x7-ncls3", 1, 16, (3, 5, 7), 3),
    ("reg.k2.m2/reg.c4x1r/reg.s8x1r:1x32x4x4x4-ncls3", 1, 32, (4, 4, 4), 3),
    ("reg.k1.m2/reg.c4x1r/reg.s8x1r:1x16x3x5x7-ncls10", 1, 16, (3, 5, 7), 10),
    # ---- ncls = 1 (two padded rows, scores one column wide) on a register-fed and on an LDS shape; the latter leaves 12 slabs
    # and a bias fold of 2 elements, which the deferred reduction takes as eight interleaved chains
    ("reg.k1.m1/reg.c4x1r/reg.s8x1r:1x16x3x5x7-ncls1", 1, 16, (3, 5, 7), 1),
    ("lds16c.k1.m1/lds16.c1x1/lds16.b1x12:1x16x3x16x16-ncls1", 1, 16, (3, 16, 16), 1),
    # ---- LDS-staged kernels on the cubic maps
    ("lds16c.k1.m1/lds16.c1x1/lds16.b1x64:1x16x16x16x16", 1, 16, (16, 16, 16), 2),
    ("lds16c.k2.m1/lds16.c1x2/lds16.b2x32:1x32x16x16x16", 1, 32, (16, 16, 16), 2),
    ("lds16c.k1.m1/lds16.c1x1/lds16.b1x4:1x16x1x16x16", 1, 16, (1, 16, 16), 2),     # D = 1 on the 16-wide kernels
    ("lds16c.k1.m1/lds16.c1x1/lds16.b1x12:1x16x3x16x16", 1, 16, (3, 16, 16), 2),
    ("lds8c.k1.m1/lds8.c1x1/lds8.b1x1:1x16x1x8x8", 1, 16, (1, 8, 8), 2),            # D = 1 on the 8-wide kernels
    ("lds8c.k1.m1/lds8.c1x3/lds8.b1x24:3x48x8x8x8", 3, 48, (8, 8, 8), 2),
    ("lds8c.k4.m1/lds8.c1x4/lds8.b1x2:1x64x2x8x8", 1, 64, (2, 8, 8), 2),
    ("lds4c.k1.m1/lds4.c1x1/lds4.b1x1:1x16x4x4x4", 1, 16, (4, 4, 4), 2),
    ("lds4c.k2.m1/lds4.c1x2/lds4.b1x2:1x32x8x4x4", 1, 32, (8, 4, 4), 2),
    ("lds4c.k16.m1/lds4.c1x16/lds4.b1x1:1x256x4x4x4", 1, 256, (4, 4, 4), 2),        # two full groups of the finalize's 8-wide loop
    # ---- tiled LDS forward on non-cubic maps (the backward is register-fed): 4-, 16- and 8-wide blocks
    ("lds4t.k1.m1/reg.c4x1r/reg.s8x3:1x16x4x8x12", 1, 16, (4, 8, 12), 2),
    ("lds4t.k1.m1/reg.c4x1r/reg.s8x3:1x16x8x12x4", 1, 16, (8, 12, 4), 2),
    ("lds16t.k1.m1/reg.c4x1r/reg.s8x6:1x16x3x8x32", 1, 16, (3, 8, 32), 2),
    ("lds16t.k1.m1/reg.c4x1r/reg.s8x3:1x16x2x4x48", 1, 16, (2, 4, 48), 2),
    ("lds8t.k1.m1/reg.c4x1r/reg.s8x8r:1x16x5x8x24", 1, 16, (5, 8, 24), 2),
    ("lds8t.k1.m1/reg.c4x1r/reg.s8x12:2x16x2x16x24", 2, 16, (2, 16, 24), 2),
    # ---- LDS bwd-data: two tiles per workgroup with a ragged last group (C / 16 = 3); four tiles per workgroup (2 x 128 x 16^3
    # reaches cts = 4 too; 3 x 64 x 11 x 16 x 16 is the smallest shape the mirror finds: 132 position blocks leave one group)
    ("lds16c.k1.m1/lds16.c2x2r/lds16.b5x26r:2x48x16x16x16", 2, 48, (16, 16, 16), 2),
    ("lds16c.k2.m1/lds16.c4x1/lds16.b7x19r:3x64x11x16x16", 3, 64, (11, 16, 16), 2),
    # ---- LDS weight gradient: three blocks per workgroup with a ragged last workgroup; more blocks than one stage holds and no
    # multiple of it (4 x 256 x 8^3 gives 7; 3 x 256 x 8^3 is smaller and gives 5 with a last workgroup of 4, and the case above 7)
    ("lds16c.k1.m1/lds16.c1x3/lds16.b3x22r:1x48x16x16x16", 1, 48, (16, 16, 16), 2),
    ("lds8c.k16.m1/lds8.c2x8/lds8.b5x5r:3x256x8x8x8", 3, 256, (8, 8, 8), 2),
]

# bf16 forward (one kernel): C = 32, 64, 96, 128 leave 3, 2, 1, 0 k-steps to the tail loop; S = 105 (ragged last tile and a
# workgroup with waves out of range), two images of 8^3, ncls 1 and 2, one voxel
BF16_CASES = [
    ("bf16.t3:1x32x3x5x7", 1, 32, (3, 5, 7), 2),
    ("bf16.t2:1x64x3x5x7", 1, 64, (3, 5, 7), 2),
    ("bf16.t1:1x96x3x5x7", 1, 96, (3, 5, 7), 2),
    ("bf16.t0:1x128x3x5x7", 1, 128, (3, 5, 7), 2),
    ("bf16.t3:2x32x8x8x8", 2, 32, (8, 8, 8), 2),
    ("bf16.t3:1x32x3x5x7-ncls1", 1, 32, (3, 5, 7), 1),
    ("bf16.t2:1x64x1x1x1", 1, 64, (1, 1, 1), 2),
]

ALL_CASES = CASES + BF16_CASES


def ids(cases):
    return [c[0] for c in cases]


def make_data(case):
    """Host inputs of a case: a = relu(randn), weights scaled 1 / sqrt(27 C), small biases, a random upstream gradient
    dO (N, 12 + 2 ncls, D, H, W) that is nonzero at the last position (a clamped read of it must show)."""
    id_, N, C, dims, ncls = case
    g = torch.Generator().manual_seed(zlib.crc32(id_.encode()))
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    a = torch.relu(r(N, C, *dims))
    lw, cw = r(12, C, 3, 3, 3) / (27 * C) ** 0.5, r(2 * ncls, C, 3, 3, 3) / (27 * C) ** 0.5
    lb, cb = 0.1 * r(12), 0.1 * r(2 * ncls)
    dO = r(N, 12 + 2 * ncls, *dims)
    last = dO[-1, :, -1, -1, -1]
    dO[-1, :, -1, -1, -1] = torch.where(last.abs() < 0.25, torch.full_like(last, 0.5), last)
    if float(a[-1, :, -1, -1, -1].max()) == 0.0:  # and the activation it would be multiplied with
        a[-1, 0, -1, -1, -1] = 1.0
    return dict(a=a, lw=lw, cw=cw, lb=lb, cb=cb, dO=dO)
