"""Case tables of tests/test_gpu_bf16pw.py, shared with tests/test_bf16pw_ref_cpu.py: plain CPU data, nothing here imports
the package.  Every case id names the kernel instantiation of csrc/bf16.hip (BatchNorm backward: csrc/bn.hip on bf16 storage) it is
meant to reach, and carries the path that the
dispatch arithmetic mirrored below (``tile_path`` and ``bww_path`` = the bf16 branches of pw_route in csrc/pwroute.hpp,
``fused_path`` = msl_bn_relu_bwd_fused_bf16, ``apply_grid`` / ``reduce_chunks``) must give for it: ``assert_path`` fails loudly
when a changed heuristic would silently move a case to another kernel, and tests/test_bf16pw_ref_cpu.py holds the mirror against
the library's own answer (msl_pwconv_route_kind).  Every shape is the smallest that reaches its path.

forward and backward data share the tile kernels with (M, K) = (Cout, Cin) and (Cin, Cout).  J (fp32 additions that combine
K-split partial tiles) is 0 in every case: both tile kernels run the MFMA chain over K serially inside a wave (bf16.hip,
``for k0 ...`` of pw_fwd_bf16_kernel, ``for it ...`` of pw_bf16_tr_kernel - one accumulator per wave, no K split)."""
import torch

from tests import bn_ref as R


def cdiv(a, b):
    return (a + b - 1) // b


def gen(seed):
    return torch.Generator().manual_seed(seed)


def bf(t):
    return t.to(torch.bfloat16).float()


# ------------------------------------------------------------------------------------------------- dispatch mirrors
# op of msl_pwconv_route_kind per table, and the PwKind (csrc/pwroute.hpp) behind the first field of a mirrored path
ROUTE_OP = dict(fwd=0, bwd_data=1, bww=2)
ROUTE_KIND = dict(tr=7, plain=8, mfma=9, any=10)


def tile_path(N, M, K, S):
    """pw_route, bf16 forward / bwd-data: ("tr", BK, T) or ("plain", vec_ok)."""
    if S % 8 == 0 and K % 32 == 0 and K <= 1024 and M % 8 == 0:
        tiles_img, mtiles = cdiv(S, 64), cdiv(M, 64)
        T = max(1, min(min(4, tiles_img), (tiles_img * mtiles * N) // 512))
        return ("tr", 128 if K % 128 == 0 else 64 if K % 64 == 0 else 32, T)
    return ("plain", S % 8 == 0)


def bww_path(N, Cin, Cout, S):
    """pw_route, bf16 weight gradient: ("mfma", MT, nslabs, chunks per slab, total chunks) or ("any", 1, fp32 chain length)."""
    if S % 64 or Cin % 32 or Cout % 32:
        return ("any", 1, N * cdiv(S, 64) * 64)  # one accumulator per thread: N * ceil(S / 64) * 64 fmaf, zeros past S
    mt = 2 if Cout % 64 == 0 else 1
    tiles = (Cout // (32 * mt)) * (Cin // 32)
    total = N * (S // 64)
    ks = max(1, min(256 // max(1, tiles), total // 4))
    cpb = cdiv(total, ks)
    return ("mfma", mt, cdiv(total, cpb), cpb, total)


def fused_path(N, S):
    """msl_bn_relu_bwd_fused_bf16: (NT, IPT) of the register kernel or "generic"; with n_t, a thread's fp32 additions."""
    total8 = N * (S >> 3)
    if S % 8 == 0 and total8 <= 4096:
        for lim, nt, ipt in ((64, 64, 1), (256, 256, 1), (512, 256, 2), (1024, 512, 2), (2048, 1024, 2), (4096, 1024, 4)):
            if total8 <= lim:
                return (nt, ipt), 8 * ipt
    return "generic", N * cdiv(S, 256)


def apply_grid(S):
    return min(cdiv(S, 1024), 64)


def reduce_chunks(S):
    return cdiv(S, 4096)  # BWD_CHUNK (bn.hip); a thread adds at most 4096 / 256 = 16 terms


# ------------------------------------------------------------------------------------------------- GEMM cases
# (id, N, Cin, Cout, S, expected tile_path(N, Cout, Cin, S))
FWD_CASES = [
    ("tr<32>:one-group", 1, 32, 8, 8, ("tr", 32, 1)),             # 56 dead rows and columns
    ("tr<64>:M-tail-S-tail", 2, 64, 72, 136, ("tr", 64, 1)),
    ("tr<128>:one-chunk", 1, 128, 64, 64, ("tr", 128, 1)),
    ("tr<128>:two-chunks", 1, 256, 40, 200, ("tr", 128, 1)),
    ("tr<32>:three-chunks", 1, 96, 160, 128, ("tr", 32, 1)),
    ("tr<32>:T2", 4, 32, 8, 16384, ("tr", 32, 2)),
    ("tr<32>:T4-ragged-group-partial-tile", 4, 32, 8, 32840, ("tr", 32, 4)),
    ("plain:S1", 1, 32, 64, 1, ("plain", False)),
    ("plain:S27", 2, 32, 96, 27, ("plain", False)),
    ("plain:S130", 1, 64, 40, 130, ("plain", False)),
    ("plain:K1056-vec", 1, 1056, 8, 8, ("plain", True)),
    ("plain:M12-vec", 1, 32, 12, 64, ("plain", True)),
]
# the same list with the roles swapped: (M, K) = (Cin, Cout), TRANS_W; expected tile_path(N, Cin, Cout, S)
BWD_DATA_CASES = [
    ("trT<32>:one-group", 1, 8, 32, 8, ("tr", 32, 1)),
    ("trT<64>:M-tail-S-tail", 2, 72, 64, 136, ("tr", 64, 1)),
    ("trT<128>:one-chunk", 1, 64, 128, 64, ("tr", 128, 1)),
    ("trT<128>:two-chunks", 1, 40, 256, 200, ("tr", 128, 1)),
    ("trT<32>:three-chunks", 1, 160, 96, 128, ("tr", 32, 1)),
    ("trT<32>:T2", 4, 8, 32, 16384, ("tr", 32, 2)),
    ("trT<32>:T4-ragged-group-partial-tile", 4, 8, 32, 32840, ("tr", 32, 4)),
    ("plainT:S1", 1, 64, 32, 1, ("plain", False)),
    ("plainT:S27", 2, 96, 32, 27, ("plain", False)),
    ("plainT:S130", 1, 40, 64, 130, ("plain", False)),
    ("plainT:K1056-vec", 1, 8, 1056, 8, ("plain", True)),
]
BWD_DATA_REFUSED = [(1, 12, 32, 64), (1, 4, 32, 8)]  # Cin % 8 != 0 -> MSL_ERR_ARG (the forward's M12 case has no TRANS_W twin)

FOLD_CASES = [FWD_CASES[1], FWD_CASES[8]]  # one tr, one plain
FOLD_NP = (1, 7, 64)
FOLD_UNSUPPORTED = [("in_np65", 1, 32, 8, 8, 65), ("Cin1056", 1, 1056, 8, 8, 4)]  # (id, N, Cin, Cout, S, in_np)

# weight gradient: (id, N, Cin, Cout, S, expected bww_path).  L (positions one slab contracts) = chunks per slab * 64.
BWW_CASES = [
    ("bww<2>:one-chunk-one-slab", 1, 32, 64, 64, ("mfma", 2, 1, 1, 1)),
    ("bww<1>:one-chunk", 1, 32, 32, 64, ("mfma", 1, 1, 1, 1)),
    ("bww<1>:two-slabs", 2, 64, 96, 256, ("mfma", 1, 2, 4, 8)),
    ("bww<1>:three-even-slabs", 3, 32, 32, 320, ("mfma", 1, 3, 5, 15)),  # 15 chunks in slabs of 5: slabs span images, none ragged
    ("bww<1>:ragged-last-slab", 3, 32, 32, 192, ("mfma", 1, 2, 5, 9)),   # 9 chunks in slabs of 5: the last slab holds 4
    ("bww-any:S100", 2, 32, 32, 100, ("any", 1, 256)),
    ("bww-any:C24x40", 1, 24, 40, 64, ("any", 1, 64)),
    ("bww-any:C8x8-S7", 1, 8, 8, 7, ("any", 1, 64)),
]

# ------------------------------------------------------------------------------------------------- materialise, BatchNorm backward
MAT_CASES = [("mat:1x8x1", 1, 8, (1, 1, 1)), ("mat:2x16x90", 2, 16, (3, 5, 6)), ("mat:1x8x294-ragged-wg", 1, 8, (7, 6, 7))]
PAD32_CASES = [("pad32:1x3x1", 1, 3, (1, 1, 1)), ("pad32:2x3x90", 2, 3, (3, 5, 6)), ("pad32:1x3x294-ragged-wg", 1, 3, (7, 6, 7))]
PAD32_FOLD_NP = (1, 70)

BN_C = 3
REDUCE_CASES = [("reduce:1x1", 1, 1), ("reduce:2x4096", 2, 4096), ("reduce:2x4097-one-element-chunk", 2, 4097),
                ("reduce:1x100", 1, 100)]
# (id, N, S, expected gridDim.x)
APPLY_CASES = [("apply:1x1", 1, 1, 1), ("apply:2x1023", 2, 1023, 1), ("apply:1x65537-grid-saturated", 1, 65537, 64)]
# (id, N, S, expected fused_path(N, S)[0])
FUSED_CASES = [
    ("fused<64,1>:total8=1", 1, 8, (64, 1)), ("fused<64,1>:total8=64", 1, 512, (64, 1)),
    ("fused<256,1>:total8=65", 1, 520, (256, 1)), ("fused<256,1>:total8=256", 2, 1024, (256, 1)),
    ("fused<256,2>:total8=257", 1, 2056, (256, 2)), ("fused<256,2>:total8=512", 1, 4096, (256, 2)),
    ("fused<512,2>:total8=513", 1, 4104, (512, 2)), ("fused<512,2>:total8=1024", 2, 4096, (512, 2)),
    ("fused<1024,2>:total8=1025", 1, 8200, (1024, 2)), ("fused<1024,2>:total8=2048", 2, 8192, (1024, 2)),
    ("fused<1024,4>:total8=2049", 1, 16392, (1024, 4)), ("fused<1024,4>:total8=4096", 4, 8192, (1024, 4)),
    ("fused-generic:total8=4097", 1, 32776, "generic"), ("fused-generic:S100", 3, 100, "generic"),
]


def assert_path(kind, case):
    """The path a case id names, from the mirrored dispatch arithmetic."""
    if kind == "fwd":
        id_, N, Cin, Cout, S, want = case
        got = tile_path(N, Cout, Cin, S)
    elif kind == "bwd_data":
        id_, N, Cin, Cout, S, want = case
        got = tile_path(N, Cin, Cout, S)
    elif kind == "bww":
        id_, N, Cin, Cout, S, want = case
        got = bww_path(N, Cin, Cout, S)
    elif kind == "fused":
        id_, N, S, want = case
        got = fused_path(N, S)[0]
    elif kind == "apply":
        id_, N, S, want = case
        got = apply_grid(S)
    else:
        raise KeyError(kind)
    assert got == want, f"{id_}: the dispatch now gives {got}, the case was written for {want}"


# ------------------------------------------------------------------------------------------------- data
def gemm_data(N, Cin, Cout, S, seed=0):
    """z, dy: bf16 values (as fp32); w, sc, sh: fp32."""
    g = gen(900 + seed + 31 * N + 7 * Cin + 3 * Cout + S)
    z = bf(torch.randn((N, Cin, S), generator=g))
    w = torch.randn((Cout, Cin), generator=g) / Cin ** 0.5
    sc, sh = torch.randn(Cin, generator=g).abs() + 0.5, torch.randn(Cin, generator=g) * 0.3
    dy = bf(torch.randn((N, Cout, S), generator=g))
    # channel 0 tells fmaf from multiply + add in every case: z = 1 + 2**-7, scale = 1 + 2**-17, so z * scale = 1 + 2**-7 + 2**-17 +
    # 2**-24 exactly, which a separate multiply rounds (a tie, to even) to 1 + 2**-7 + 2**-17.  With shift = -(0.5 + 3 * 2**-9 +
    # 2**-17) the sum is then exactly 0.5 + 2**-9, a bf16 tie that goes to 0.5, while the single rounding of fmaf keeps
    # 0.5 + 2**-9 + 2**-24 (an fp32 value), above the tie, which goes to 0.5 + 2**-8: the MFMA operand differs by one bf16 ulp.
    z[:, 0, :], sc[0], sh[0] = 1.0 + 2.0 ** -7, 1.0 + 2.0 ** -17, -(0.5 + 3 * 2.0 ** -9 + 2.0 ** -17)
    return dict(z=z, w=w, sc=sc, sh=sh, dy=dy)


def fold_partials(Cin, in_np, count, g):
    """Host-made fp64 (2, Cin, in_np) partials of plausible statistics (mean ~ N(0, 1), var ~ 1..3), unevenly split."""
    mean = torch.randn(Cin, generator=g, dtype=torch.float64)
    var = torch.rand(Cin, generator=g, dtype=torch.float64) * 2 + 1
    s, q = mean * count, (var + mean * mean) * count
    wgt = torch.rand(in_np, generator=g, dtype=torch.float64) + 0.1
    wgt /= wgt.sum()
    return torch.stack([s[:, None] * wgt, q[:, None] * wgt]).contiguous()


def bn_data(N, S, seed=0, C=BN_C):
    """g, y: bf16 values; y32: y before its rounding; vec (6, C): rows 0-3 from bn_ref.host_vectors on the ROUNDED y, rows 4-5
    (k1, k2) the float64 sums of the reference over the count, rounded to fp32 on the host (msl_bn_relu_bwd_apply_bf16's input)."""
    gr = gen(4000 + seed + 17 * N + S)
    y32 = torch.randn((N, C, S), generator=gr) * 1.5 + 0.3
    y = bf(y32)
    g = bf(torch.randn((N, C, S), generator=gr))
    gamma, beta = torch.randn(C, generator=gr).abs() + 0.5, torch.randn(C, generator=gr) * 0.3
    v4 = R.host_vectors(y, gamma, beta)
    s, q = R.bwd_sums_ref(g, y, v4)
    k = torch.stack([R.f32(s / (N * S)), R.f32(q / (N * S))])
    return dict(g=g, y=y, y32=y32, vec=torch.cat([v4, k]).contiguous())


def mat_data(N, C, dims, seed=0):
    g = gen(6000 + seed + N + 13 * C + dims[0] * dims[1] * dims[2])
    S = dims[0] * dims[1] * dims[2]
    y = bf(torch.randn((N, C, S), generator=g))
    return dict(y=y, sc=torch.randn(C, generator=g).abs() + 0.5, sh=torch.randn(C, generator=g) * 0.3)


# ------------------------------------------------------------------------------------------------- tie cases
ONE_TIE, UP_TIE = 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -7 + 2.0 ** -8  # exactly between two bf16 values: -> 1.0 (0x3F80), 1 + 2**-6 (0x3F82)
TIE_BITS = (0x3F80, 0x3F82, 0xBF80, 0xBF82)                     # expected stored bits of the column patterns 0..3
TIE_SHAPES = [("tie:tr<32>", 1, 8, 32, 8), ("tie:plain-S12", 1, 8, 32, 12)]  # (id, N, M, K, S), M <= 8, K = 32


def tie_gemm(N, M, K, S):
    """W (M, K), A (N, K, S), all bf16-exact: row m has two non-zero weights, 1.0 at k = m and 2**-8 at k = 16 + m; column s of A
    carries pattern s % 4 = (a1, a2) in ((1, 1), (1 + 2**-7, 1), (-1, -1), (-(1 + 2**-7), -1)) in the rows 0..7 / 16..23, and
    3.0 elsewhere (met by zero weights only).  Every product and every sum is exact in fp32, so the fp32 accumulator holds
    1 + 2**-8, 1 + 2**-7 + 2**-8 or a negative of them whatever the order: ties, which round-to-nearest-even sends to TIE_BITS.
    -> (W, A, expected bits (N, M, S) int64)."""
    assert M <= 8 and K == 32
    W = torch.zeros(M, K)
    for m in range(M):
        W[m, m], W[m, 16 + m] = 1.0, 2.0 ** -8
    A = torch.full((N, K, S), 3.0)
    pat = torch.arange(S) % 4
    a1 = torch.tensor([1.0, 1.0 + 2.0 ** -7, -1.0, -(1.0 + 2.0 ** -7)])[pat]
    a2 = torch.tensor([1.0, 1.0, -1.0, -1.0])[pat]
    A[:, 0:8, :] = a1
    A[:, 16:24, :] = a2
    bits = torch.tensor(TIE_BITS, dtype=torch.int64)[pat].expand(N, M, S).contiguous()
    return W, A, bits


def tie_apply():
    """apply with k1 = k2 = 0 and scale = 1 + 2**-8 (an fp32 value), mask open everywhere (y = 1, shift = 0): dy = scale * g in one
    exact fp32 product.  g = 1 -> 1 + 2**-8, a tie -> 0x3F80; g = -1 -> 0xBF80; g = 1 + 2**-7 -> 1 + 2**-7 + 2**-8 + 2**-15, above
    the tie -> 0x3F82 (a truncating store gives 0x3F81).  -> (g, y, vec (6, 1), expected bits)."""
    g = torch.tensor([1.0, 1.0 + 2.0 ** -7, -1.0]).repeat(4).view(1, 1, 12)
    y = torch.ones_like(g)
    vec = torch.tensor([[ONE_TIE], [0.0], [0.0], [1.0], [0.0], [0.0]])
    bits = torch.tensor([0x3F80, 0x3F82, 0xBF80], dtype=torch.int64).repeat(4).view(1, 1, 12)
    return g, y, vec, bits


def tie_materialize():
    """z = 1, 1 + 2**-7, 0.5 (bf16); scale = 1, shift = 2**-8: fmaf is exact and lands on 1 + 2**-8 (tie -> 0x3F80), 1 + 2**-7 + 2**-8
    (tie -> 0x3F82) and 0.5 + 2**-8 = 0.5 (1 + 2**-7), a bf16 value (0x3F01).  8 channels x S = 3.  -> (y, sc, sh, expected bits)."""
    y = torch.tensor([1.0, 1.0 + 2.0 ** -7, 0.5]).expand(1, 8, 3).contiguous()
    bits = torch.tensor([0x3F80, 0x3F82, 0x3F01], dtype=torch.int64).expand(1, 8, 3).contiguous()
    return y, torch.ones(8), torch.full((8,), 2.0 ** -8), bits


# ------------------------------------------------------------------------------------------------- non-finite cases
NONFINITE_FWD = ("nonfinite:tr<64>", 2, 64, 72, 136)   # NaN at z[0, 5, 3], +Inf at z[1, 40, 135]
NONFINITE_APPLY = ("nonfinite:apply", 2, 1023)         # NaN at g[0, 1, 7], +Inf at g[1, 2, 1000] (both under an open mask)
NONFINITE_BWW = [("nonfinite:bww<1>", 1, 32, 32, 64), ("nonfinite:bww-any", 1, 32, 32, 100)]  # NaN at z[0, 3, 9]
