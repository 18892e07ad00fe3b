"""Case tables of tests/test_gpu_pw.py (shared with tests/test_pw_ref_cpu.py, which proves every bound at every shape with
honest fp32 on the CPU).  Plain data: (id, N, Cin, Cout, S, J).  The id names the kernel path the shape is meant to reach - the
PwKind of csrc/pwroute.hpp that ``expected_kind`` reads off it and tests/test_pw_ref_cpu.py asserts against the library's own
answer (msl_pwconv_route_kind); DESIGN.md, Appendix A, lists every kernel instantiation with its case.  J = fp32 additions that
combine K-split partial tiles: 0 serial K, NWK for the split wave form, the wave count for the K-split GEMM."""

# PwKind of csrc/pwroute.hpp, as msl_pwconv_route_kind returns it, and its ops
KIND = dict(none=0, strip=1, wave=2, ksplit=3, gemm=4, bww_wave=5, bww_tile=6, bf16_tr=7, bf16_plain=8, bf16_bww_mfma=9,
            bf16_bww_any=10, fused=11)
OP_FWD, OP_BWD_DATA, OP_BWD_WEIGHT, OP_BWD_FUSED = 0, 1, 2, 3


def expected_kind(id_):
    """The PwKind a case id spells: ``<path>[:<detail>]``, or ``<family>-declined-<why>:<path>`` where a family declines the shape."""
    head, _, tail = id_.partition(":")
    name = tail if "declined" in head else head
    for prefix, kind in (("bww-wave", "bww_wave"), ("bww-fallback", "bww_tile"), ("strip", "strip"), ("wave", "wave"),
                         ("split", "wave"), ("ksplit", "ksplit"), ("gemm", "gemm")):
        if name.startswith(prefix):
            return KIND[kind]
    raise KeyError(id_)


WAVE_S = (1, 31, 32, 33, 127, 128, 129, 130)  # lane, tile and workgroup tails; S - 1 clamp of the columns past S

FWD_CASES = [
    # the five strip instantiations at exactly 128 strips
    ("strip<32,256,2>", 2, 32, 64, 16384, 0),
    ("strip<64,128,1>", 1, 64, 32, 16384, 0),
    ("strip<64,64,4>", 2, 64, 128, 4096, 0),
    ("strip<128,64,4>", 2, 128, 128, 4096, 0),
    ("strip<128,64,2>", 2, 128, 64, 4096, 0),
    # 127 / 126 strips: declined by the count -> wave kernels
    ("strip-declined-count:wave<32,2>", 1, 32, 64, 32512, 0),
    ("strip-declined-count:wave<64,1>", 1, 64, 32, 16256, 0),
    ("strip-declined-count:wave<64,2>", 2, 64, 128, 4032, 0),
    ("strip-declined-count:split2-M128", 2, 128, 128, 4032, 2),
    ("strip-declined-count:split2-M64", 2, 128, 64, 4032, 2),
    # S % cols != 0: declined by the divisibility rule
    ("strip-declined-div:wave<32,2>", 2, 32, 64, 16388, 0),
    ("strip-declined-div:wave<64,1>", 1, 64, 32, 16388, 0),
    ("strip-declined-div:wave<64,2>", 2, 64, 128, 4100, 0),
    ("strip-declined-div:split2-M128", 2, 128, 128, 4100, 2),
    ("strip-declined-div:split2-M64", 2, 128, 64, 4100, 2),
]
# wave kernel, NWK = 1, NT = 1: K = 32 | 64, MT = 1 (Cout = 32 | 96) and MT = 2 (Cout = 64)
for _k, _m in ((32, 32), (64, 96), (32, 64), (64, 64)):
    for _i, _s in enumerate(WAVE_S):
        FWD_CASES.append((f"wave<{_k},{1 if _m % 64 else 2}>-M{_m}-S{_s}", 1 + _i % 2, _k, _m, _s, 0))
FWD_CASES += [
    ("wave-NT2<32,2>:4104-waves", 2, 32, 256, 16404, 0),  # last workgroup: 20 live columns in tile 0, tile 1 wholly past S
    ("wave-NT2<64,1>:4104-waves", 2, 64, 96, 21870, 0),
    ("wave-NT2<32,1>:4104-waves", 2, 32, 96, 21870, 0),
    ("wave-NT2<64,2>:4104-waves", 2, 64, 256, 16404, 0),
    ("wave-NT1<32,2>:4088-waves", 2, 32, 256, 16340, 0),
]
for _k in (128, 256, 512):  # wave kernel, NWK = K / 64
    for _s in (1, 33, 64, 95):
        for _n in (1, 3):
            FWD_CASES.append((f"wave-split{_k // 64}-S{_s}-N{_n}", _n, _k, 32, _s, _k // 64))
FWD_CASES += [
    ("gemm-vec", 2, 96, 160, 132, 0),
    ("gemm-vec-M4", 1, 32, 4, 128, 0),       # rows >= M read row 0 and must not be stored
    ("gemm-scalar", 2, 96, 160, 131, 0),
    ("gemm-scalar-M68", 1, 160, 68, 130, 0),
    ("ksplit4-K128", 1, 128, 36, 70, 4),
    ("ksplit4-K384", 2, 384, 64, 65, 4),
    ("ksplit8-K256", 1, 256, 36, 70, 8),           # Cout % 32 != 0: the wave form declines
    ("ksplit8-K768-noaffine", 1, 768, 40, 64, 8),  # Cin > FOLD_MAXK: the affine forms are refused
    ("ksplit-declined-256-tiles:gemm", 4, 384, 4, 8132, 0),
]

# one shape of every forward kernel family, for msl_pwconv_fwd_fold
FOLD_CASES = [
    ("strip<64,64,4>", 2, 64, 128, 4096),
    ("wave-NT1<32,2>", 2, 32, 64, 130),
    ("wave-NT2<32,2>", 2, 32, 256, 16404),
    ("wave-split4", 3, 256, 32, 95),
    ("gemm-scalar", 2, 96, 160, 131),
    ("ksplit4-K128", 1, 128, 36, 70),
]
FOLD_NP = (1, 7, 8, 9, 64, 65, 128, 515)  # serial loop: unrolled / tail parts; both sides of NP = 64; wave loop's strided tail

# backward data: the GEMM is M = Cin, K = Cout, weights read transposed (TRANS_W = true everywhere)
BWD_DATA_CASES = [
    ("strip<32,256,2>T", 2, 64, 32, 16384, 0),   # (K, M) = (32, 64) with the weights read transposed (Cin = 64, Cout = 32)
    ("strip<64,128,1>T", 1, 32, 64, 16384, 0),
    ("strip<64,64,4>T", 2, 128, 64, 4096, 0),    # (64, 128)
    ("strip<128,64,4>T", 2, 128, 128, 4096, 0),
    ("strip<128,64,2>T", 2, 64, 128, 4096, 0),
    ("strip-declined-count:wave<32,2>T", 1, 64, 32, 32512, 0),
    ("strip-declined-div:wave<64,2>T", 2, 128, 64, 4100, 0),
]
for _k, _m in ((32, 32), (64, 96), (32, 64), (64, 64)):
    for _i, _s in enumerate((1, 33, 129, 130)):
        BWD_DATA_CASES.append((f"wave<{_k},{1 if _m % 64 else 2}>T-M{_m}-S{_s}", 1 + _i % 2, _m, _k, _s, 0))
for _k in (128, 256, 512):
    for _s in (33, 95):
        BWD_DATA_CASES.append((f"wave-split{_k // 64}T-S{_s}", 3, 32, _k, _s, _k // 64))
BWD_DATA_CASES += [
    ("gemmT-vec", 2, 160, 96, 132, 0),
    ("gemmT-scalar", 2, 160, 96, 131, 0),
    ("gemmT-scalar-M68", 1, 68, 160, 130, 0),    # Cin % 64 != 0: columns >= M read column 0
    ("ksplit4T-K128", 1, 36, 128, 70, 4),
    ("ksplit4T-K384", 2, 64, 384, 65, 4),
    ("ksplit8T-K768", 1, 40, 768, 64, 8),
    ("ksplit-declined-256-tiles:gemmT", 4, 4, 384, 8132, 0),
]

# weight gradient: (id, N, Cin, Cout, S)
BWW_CASES = [
    ("bww-wave<1>:one-chunk", 1, 32, 32, 32),
    ("bww-wave<2>:7-chunks-no-split", 1, 32, 64, 224),
    ("bww-wave<2>:41-chunks-short-last-slab-odd-per-wave", 1, 32, 64, 1312),
    ("bww-wave<1>:N3-slabs-span-images", 3, 64, 96, 352),
    ("bww-wave<2>:N3-123-chunks", 3, 32, 64, 1312),
    ("bww-wave<2>:tiles8", 2, 128, 128, 96),
    ("bww-fallback<64>-S65", 2, 64, 64, 65),
    ("bww-fallback<64>-S130", 1, 128, 64, 130),
    ("bww-fallback<32>-S33", 1, 96, 64, 33),
]

FUSED_CASE = (3, 32, 64, 21888)  # 513 strips of 128 over 256 workgroups: uneven share, strips cross images
