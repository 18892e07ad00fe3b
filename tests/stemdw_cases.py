"""Case table of tests/test_gpu_stemdw.py (shared with tests/test_stemdw_ref_cpu.py, which holds every row against
stemdw_ref.plan and the library's own query).  Plain data: (id, N, Cin, (D, H, W)).  The id names what the case reaches:
``c<Cin>-th<TH>-aw<AW>-sd<SD>`` = the instantiation stem_dw_eval_kernel<Cin, TH, AW, .> and the output planes per workgroup; both
are asserted on the CPU, so an edit cannot move a case silently.  Input H is 4 ZH, and ZH picks TH: 2 -> 2, 3 or 6 -> 3, 4 or
8 -> 4 - except Cin = 2 at W = 192, where TH 3 and 4 need more load slots than a workgroup has and every ZH runs TH 2.
These are the smallest shapes at which each path can still go wrong."""
import math

import torch

# ------------------------------------------------------------------------------------------------- SD = 1: every instantiation
# D = 8 / 12: two / three plane segments (first, [middle,] last); rows > 1: the recomputed halo row; one odd N
_SD1 = [
    # cin, W, TH, N, D, ZH
    (1, 64, 2, 3, 12, 2), (1, 64, 3, 2, 8, 6), (1, 64, 4, 2, 12, 4),
    (1, 128, 2, 2, 8, 2), (1, 128, 3, 1, 12, 3), (1, 128, 4, 1, 8, 8),
    (1, 192, 2, 1, 12, 2), (1, 192, 3, 1, 8, 6), (1, 192, 4, 1, 12, 4),    # (1, 4, 96): 161 056 B of LDS
    (2, 64, 2, 2, 8, 2), (2, 64, 3, 1, 12, 3), (2, 64, 4, 1, 8, 8),
    (2, 128, 2, 1, 12, 2), (2, 128, 3, 1, 8, 6), (2, 128, 4, 1, 12, 4),
    (2, 192, 2, 1, 8, 2), (2, 192, 2, 1, 12, 4), (2, 192, 2, 1, 8, 6),     # TH 3 and 4 rejected by the slot count: 1, 2, 3 row groups
]
CASES = [(f"c{c}-th{th}-aw{W // 2}-sd1:{N}x{D}x{4 * zh}x{W}", N, c, (D, 4 * zh, W)) for c, W, th, N, D, zh in _SD1]

# ------------------------------------------------------------------------------------------------- SD > 1: many small images
CASES += [(f"c1-th2-aw32-sd{sd}:256x{4 * sd}x8x64", 256, 1, (4 * sd, 8, 64)) for sd in (2, 3, 4, 6, 8)]   # SD = ZD, grid (1, 1, 256)
CASES += [
    ("c1-th2-aw32-sd8:128x64x8x64-two-segments", 128, 1, (64, 8, 64)),    # the use_b cut and the recomputed halo plane inside an image
    ("c1-th3-aw32-sd2:32x8x96x64-eight-row-groups", 32, 1, (8, 96, 64)),
    ("c1-th4-aw32-sd2:32x8x128x64-eight-row-groups", 32, 1, (8, 128, 64)),
    ("c2-th2-aw32-sd2:256x8x8x64", 256, 2, (8, 8, 64)),
    ("c1-th3-aw96-sd2:16x8x192x192-sixteen-row-groups", 16, 1, (8, 192, 192)),  # the instantiation of the 192^3 inference pass
]
MAX_VOXELS = 5_000_000  # N Cin D H W of the largest case: its float64 reference takes seconds

# ------------------------------------------------------------------------------------------------- refused shapes
# (id, N, Cin, dims, launch): launch = False where the call is only asked of msl_stem_dw_fwd_eval_supported
REFUSED = [
    ("D-30", 1, 1, (30, 32, 64), True), ("Cin-3", 1, 3, (32, 32, 64), True), ("W-96-AW-48", 1, 1, (32, 32, 96), True),
    ("W-256", 1, 1, (32, 32, 256), True), ("N-0", 0, 1, (32, 32, 64), True),
    ("c2-aw96-zh3-no-TH", 1, 2, (8, 12, 192), True),   # TH 3 needs 4410 load slots, ZH = 3 admits neither 2 nor 4
    ("D-10", 1, 1, (10, 32, 64), True), ("H-30", 1, 1, (32, 30, 64), True), ("W-62", 1, 1, (32, 32, 62), True),
    ("2^30-voxels", 1, 1, (2048, 4096, 128), False), ("2^30-voxels-two-channels", 1, 2, (1024, 4096, 128), False),
    ("Cin-0", 1, 0, (32, 32, 64), True),
]
# and the neighbour just below the 2^30 limit, which is taken (query only)
LARGEST_TAKEN = (1, 1, (2044, 4096, 128))


def ids(cases):
    return [c[0] for c in cases]


def id_parts(id_):
    """-> (Cin, TH, AW, SD) the id names."""
    c, th, aw, sd = id_.split(":")[0].split("-")[:4]
    return int(c[1:]), int(th[2:]), int(aw[2:]), int(sd[2:])


def gen(seed):
    return torch.Generator().manual_seed(seed)


def seed_of(N, cin, dims):
    return 2000 * cin + 97 * dims[0] + 31 * dims[1] + 7 * dims[2] + N


def make_data(case, variant=0, n=None):
    """The operands of a case (``variant``: another draw; ``n``: only the first n images) -> dict(x, w, sc, sh, wd) fp32.
    Scales of both signs with |sc| >= 0.5; shifts of both signs, channels 0-7 above 0.2 (relu(sh) in a padding cell is then far
    above any bound) and 8-15 below -0.1; w ~ 0.3 randn, wd ~ randn / sqrt(27)."""
    _, N, cin, dims = case
    g = gen(seed_of(N, cin, dims) + 100003 * variant)
    n = N if n is None else min(n, N)
    x = torch.randn((N, cin) + tuple(dims), generator=g)[:n].contiguous()
    w = torch.randn((32, cin, 3, 3, 3), generator=g) * 0.3
    wd = torch.randn((32, 27), generator=g) / math.sqrt(27)
    sign = torch.where(torch.rand(32, generator=g) < 0.5, -1.0, 1.0)
    sign[0], sign[1] = 1.0, -1.0
    sc = (torch.rand(32, generator=g) + 0.5) * sign
    sh = torch.randn(32, generator=g) * 0.3
    sh[:8] = 0.2 + 0.05 + torch.rand(8, generator=g) * 0.5
    sh[8:16] = -0.1 - torch.rand(8, generator=g) * 0.3
    return dict(x=x, w=w, sc=sc, sh=sh, wd=wd)
