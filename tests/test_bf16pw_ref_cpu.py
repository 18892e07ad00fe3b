"""tests/bf16pw_ref.py and tests/bf16pw_cases.py checked without a GPU: the two roundings (fmaf, fp32 -> bf16) against integer /
rational arithmetic on bit patterns, the float64 GEMM references against einsum and autograd, every case's path against the
library's own queries, and - the proof that the checks are neither violated by honest arithmetic nor vacuous - an honest fp32
emulation that passes every check at every case, and fourteen wrong kernels that are each rejected in at least one case of
every entry point they apply to.  The pinned share (elements whose rounding interval is a single bf16 value, where the test
demands exact bits) of the smallest-K case of every entry point with a bf16 output is asserted to be >= 0.9."""
import functools

import numpy as np
import pytest
import torch

from mslesions3d_amd import _lib
from tests import bf16pw_cases as C
from tests import bf16pw_ref as B
from tests import bn_ref as R
from tests import pw_ref as P
from tests.test_pw_ref_cpu import _fma_exact


# ------------------------------------------------------------------------------------------------- the roundings
def test_bf16_rne_is_round_to_nearest_even_on_bit_patterns():
    g = C.gen(3)
    x = torch.randn(20000, generator=g) * torch.exp(torch.randn(20000, generator=g) * 8)
    hard = torch.tensor([C.ONE_TIE, C.UP_TIE, -C.ONE_TIE, -C.UP_TIE, 1 + 2.0 ** -8 + 2.0 ** -23, 1 + 2.0 ** -8 - 2.0 ** -24, 0.0, -0.0,
                         2.0 ** -126, 3.3895314e38, 1.0, 65280.0, 65408.0])
    x = torch.cat([x, hard])
    want = B.round_bits(x, 16, "rne")
    assert torch.equal(B.f32bits(B.bf16_rne(x)), B.f32bits(want))
    assert torch.equal(B.bits16(B.bf16_rne(x)), B.f32bits(want) >> 16)
    # the three roundings differ where they should
    t = torch.tensor([C.ONE_TIE, C.UP_TIE])
    assert B.bits16(B.round_bits(t, 16, "rne")).tolist() == [0x3F80, 0x3F82]
    assert B.bits16(B.round_bits(t, 16, "away")).tolist() == [0x3F81, 0x3F82]
    assert B.bits16(B.round_bits(t, 16, "trunc")).tolist() == [0x3F80, 0x3F81]
    # rounded twice: 1 + 2**-8 + 2**-20 is above the tie (-> 0x3F81); 9 significant bits first lands ON it, then to even
    assert B.bits16(B.store(torch.tensor([1 + 2.0 ** -8 + 2.0 ** -20]), "twice")).tolist() == [0x3F80]
    assert B.bits16(B.store(torch.tensor([1 + 2.0 ** -8 + 2.0 ** -20]))).tolist() == [0x3F81]


def test_fma32_on_the_cases_probe_channel_and_random_bits():
    d = C.gemm_data(1, 32, 8, 8)
    x = torch.cat([d["z"][0, :, 0], torch.randn(500, generator=C.gen(4))])
    a = torch.cat([d["sc"], torch.randn(500, generator=C.gen(5))])
    b = torch.cat([d["sh"], torch.randn(500, generator=C.gen(6))])
    got = P.fma32(x, a, b).numpy()
    want = np.array([_fma_exact(*t) for t in zip(x.tolist(), a.tolist(), b.tolist())], dtype=np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # channel 0: fmaf -> 0.5 + 2**-9 + 2**-24 -> bf16 0.5 + 2**-8; multiply + add -> 0.5 + 2**-9 -> bf16 0.5
    assert float(got[0]) == 0.5 + 2.0 ** -9 + 2.0 ** -24 and float(B.bf16_rne(torch.tensor(got[:1]))) == 0.5 + 2.0 ** -8
    assert float(x[0] * a[0] + b[0]) == 0.5 + 2.0 ** -9 and float(B.bf16_rne(x[:1] * a[:1] + b[:1])) == 0.5


# ------------------------------------------------------------------------------------------------- references vs independent code
@pytest.mark.parametrize("N,Cin,Cout,S", [(2, 32, 8, 37), (1, 64, 72, 5)])
def test_gemm_refs_match_einsum_and_autograd(N, Cin, Cout, S):
    d = C.gemm_data(N, Cin, Cout, S)
    A, Wb = B.fwd_operands(d["z"], d["sc"], d["sh"], d["w"])
    a = A.double().requires_grad_(True)
    wd = Wb.double().requires_grad_(True)
    y = torch.einsum("oc,ncs->nos", wd, a)
    y.backward(d["dy"].double())
    tol = dict(rtol=0, atol=1e-12)
    assert torch.allclose(B.fwd_expect(A, Wb, Cin)["y"], y.detach(), **tol)
    assert torch.allclose(B.bwd_data_expect(d["dy"], Wb, Cout)["y"], a.grad, **tol)
    e = B.bww_expect(d["dy"], d["z"], d["sc"], d["sh"], True, 64, 1)
    assert torch.allclose(e["dw"], wd.grad, **tol)
    assert bool((B.fwd_expect(A, Wb, Cin)["B"] >= 0).all()) and bool((e["B"] >= 0).all())


# ------------------------------------------------------------------------------------------------- paths and library queries
ALL_PATHS = ([("fwd", c) for c in C.FWD_CASES] + [("bwd_data", c) for c in C.BWD_DATA_CASES] + [("bww", c) for c in C.BWW_CASES]
             + [("fused", c) for c in C.FUSED_CASES] + [("apply", c) for c in C.APPLY_CASES])


@pytest.mark.parametrize("kind,case", ALL_PATHS, ids=[f"{k}:{c[0]}" for k, c in ALL_PATHS])
def test_case_reaches_the_path_it_names(kind, case):
    C.assert_path(kind, case)
    L = _lib.load()
    if kind in ("fwd", "bwd_data", "bww"):  # the library's own route agrees with the mirror
        _, N, Cin, Cout, S, want = case
        got = L.msl_pwconv_route_kind(C.ROUTE_OP[kind], 1, N, Cin, Cout, S, 1 if kind == "fwd" else 0)
        assert got == C.ROUTE_KIND[want[0]], f"{case[0]}: route kind {got}, the mirror gives {want[0]}"
    if kind == "fwd":
        _, N, Cin, Cout, S, _ = case
        assert L.msl_pwconv_fwd_bf16_num_partials(N, S) == N * C.cdiv(S, 64) * 2
        assert Cin % 32 == 0
    elif kind == "bwd_data":
        assert case[3] % 32 == 0 and case[2] % 8 == 0
    elif kind == "bww":
        _, N, Cin, Cout, S, want = case
        assert L.msl_pwconv_bwd_weight_bf16_nslabs(N, Cin, Cout, S) == want[2 if want[0] == "mfma" else 1]
    elif kind == "fused":
        assert (case[3] == "generic") == (case[2] % 8 != 0 or case[1] * (case[2] >> 3) > 4096)


def test_ids_threshold_sides_and_refusals():
    total8 = [n * (s >> 3) for _, n, s, _ in C.FUSED_CASES[:13]]
    assert total8 == [1, 64, 65, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097]
    L = _lib.load()
    for id_, N, S in C.REDUCE_CASES:
        assert L.msl_bn_relu_bwd_bf16_num_partials(N, S) == N * C.reduce_chunks(S)
    for _, N, Cin, Cout, S, in_np in C.FOLD_UNSUPPORTED:  # no query exists for the fold: the launcher's own two limits
        assert in_np > 64 or Cin > 1024
    for N, Cin, Cout, S in C.BWD_DATA_REFUSED:
        assert Cin % 8 != 0 and Cout % 32 == 0
    for id_, N, M, K, S in C.TIE_SHAPES:
        assert (C.tile_path(N, M, K, S)[0] == "tr") == ("tr" in id_)  # forward and TRANS_W alike: (M, K) = (rows, chain)
    # the ragged last slab and the T = 4 ragged last group are what their ids say
    assert C.bww_path(3, 32, 32, 192)[4] % C.bww_path(3, 32, 32, 192)[3] != 0
    assert C.cdiv(32840, 64) % 4 != 0 and 32840 % 64 == 8


# ------------------------------------------------------------------------------------------------- one runner for emulation and mutants
@functools.lru_cache(maxsize=None)
def _gemm(case):
    id_, N, Cin, Cout, S = case[:5]
    return C.gemm_data(N, Cin, Cout, S)


@functools.lru_cache(maxsize=None)
def _fwd_expect(case):
    d = _gemm(case)
    A, Wb = B.fwd_operands(d["z"], d["sc"], d["sh"], d["w"])
    return B.fwd_expect(A, Wb, case[2])


@functools.lru_cache(maxsize=None)
def _bwd_expect(case):
    d = _gemm(case)
    return B.bwd_data_expect(d["dy"], B.bf16_rne(d["w"]), case[3])


@functools.lru_cache(maxsize=None)
def _bn(N, S):
    return C.bn_data(N, S)


def run(entry, case, mut=None):
    """The emulation of ``entry`` at ``case`` (honest, or the wrong kernel ``mut``) through the checks of the GPU test."""
    rep = B.Report(f"{case[0]}[{mut}]")
    if entry == "fwd":
        d = _gemm(case)
        y, part = B.emul_fwd(d["z"], d["sc"], d["sh"], d["w"], True, True, mut)
        B.check_fwd(rep, _fwd_expect(case), y, part)
    elif entry == "bwd_data":
        d = _gemm(case)
        B.check_fwd(rep, _bwd_expect(case), B.emul_bwd_data(d["dy"], d["w"], mut))
    elif entry == "bww":
        id_, N, Cin, Cout, S, path = case
        d = _gemm(case)
        ns, cpb = (path[2], path[3]) if path[0] == "mfma" else (1, path[2] // 64)
        for affine in (True, False):
            e = B.bww_expect(d["dy"], d["z"], d["sc"], d["sh"], affine, cpb * 64, ns)
            B.check_bww(rep, e, B.emul_bww(d["dy"], d["z"], d["sc"], d["sh"], affine, ns, cpb, mut))
    elif entry == "mat":
        id_, N, Cc, dims = case
        d = C.mat_data(N, Cc, dims)
        a, ab = B.mat_expect(d["y"], d["sc"], d["sh"])
        plain, cl = B.emul_materialize(d["y"], d["sc"], d["sh"], mut)
        rep.bits("plain", B.f32bits(plain), B.f32bits(a))
        rep.bits("pad_cl", B.f32bits(cl), B.f32bits(ab))
    elif entry == "reduce":
        id_, N, S = case
        d = _bn(N, S)
        rep.bound("partials", B.emul_reduce(d["g"], d["y"], d["vec"], mut), *B.reduce_expect(d["g"], d["y"], d["vec"]))
    elif entry == "apply":
        id_, N, S = case[:3]
        d = _bn(N, S)
        e = B.apply_expect(d["g"], d["y"], d["vec"])
        rep.interval("dy", B.emul_apply(d["g"], d["y"], d["vec"], d["y32"], mut), e["y"], e["B"])
    elif entry == "fused":
        id_, N, S, path = case
        d = _bn(N, S)
        n_t = C.fused_path(N, S)[1]
        layout = ("strided", 256) if path == "generic" else ("reg",) + path
        B.check_fused(rep, B.fused_expect(d["g"], d["y"], d["vec"], n_t), *B.emul_fused(d["g"], d["y"], d["vec"], layout, d["y32"], mut))
    else:
        raise KeyError(entry)
    return rep


CASES = dict(fwd=C.FWD_CASES, bwd_data=C.BWD_DATA_CASES, bww=C.BWW_CASES, mat=C.MAT_CASES, reduce=C.REDUCE_CASES,
             apply=C.APPLY_CASES, fused=C.FUSED_CASES)
EVERY = [(e, c) for e, cs in CASES.items() for c in cs]


@pytest.mark.parametrize("entry,case", EVERY, ids=[f"{e}:{c[0]}" for e, c in EVERY])
def test_honest_fp32_emulation_passes_every_check(entry, case):
    rep = run(entry, case)
    assert rep.failures() == [], "\n".join(rep.failures())
    if entry in ("apply", "fused", "reduce"):
        d = _bn(case[1], case[2])
        assert B.mask_is_kernels(d["y"], d["vec"])


# ------------------------------------------------------------------------------------------------- the tie cases
def _tie_run(entry, shape, mut=None):
    id_, N, M, K, S = shape
    W, A, bits = C.tie_gemm(N, M, K, S)
    rep = B.Report(f"{id_}:{entry}[{mut}]")
    if entry == "fwd":
        y, part = B.emul_fwd(A, None, None, W, False, True, mut)  # without the affine: its ReLU would clear the negative ties
        e = B.fwd_expect(*B.fwd_operands(A, None, None, W, affine=False), K)
    else:
        y, part = B.emul_bwd_data(A, W.t().contiguous(), mut), None
        e = B.bwd_data_expect(A, B.bf16_rne(W.t().contiguous()), K)
    e["B"] = torch.zeros_like(e["B"])
    B.check_fwd(rep, e, y, part, exact_bits=bits)
    return rep, e


def _tie_other(entry, mut=None):
    rep = B.Report(f"tie:{entry}[{mut}]")
    if entry == "apply":
        g, y, vec, bits = C.tie_apply()
        rep.bits("dy-bits", B.bits16(B.emul_apply(g, y, vec, None, mut)), bits)
    else:
        y, sc, sh, bits = C.tie_materialize()
        rep.bits("pad_cl-bits", B.bits16(B.emul_materialize(y, sc, sh, mut)[1]), bits)
    return rep


@pytest.mark.parametrize("shape", C.TIE_SHAPES, ids=[s[0] for s in C.TIE_SHAPES])
def test_tie_cases_are_exact_and_single_valued(shape):
    id_, N, M, K, S = shape
    W, A, bits = C.tie_gemm(N, M, K, S)
    assert torch.equal(B.bf16_rne(W), W) and torch.equal(B.bf16_rne(A), A)
    exact32 = lambda t: bool(torch.equal(t.float().double(), t))
    assert int((W != 0).sum(1).max()) == 2
    for m in range(M):  # both products and their sum are fp32 values: B == 0 whatever the order
        k1, k2 = (W[m] != 0).nonzero().flatten().tolist()
        p1, p2 = W[m, k1].double() * A[:, k1].double(), W[m, k2].double() * A[:, k2].double()
        assert exact32(p1) and exact32(p2) and exact32(p1 + p2)
    for entry in ("fwd", "bwd_data"):
        rep, e = _tie_run(entry, shape)
        assert rep.failures() == [], "\n".join(rep.failures())
        lo, hi = B.interval(e["y"], 0.0)
        assert torch.equal(lo, hi) and torch.equal(B.bits16(lo), bits)
        assert sorted(set(e["y"].reshape(-1).tolist())) == sorted([-C.UP_TIE, -C.ONE_TIE, C.ONE_TIE, C.UP_TIE][:min(4, S)])


def test_tie_cases_of_apply_and_materialize_are_exact():
    g, y, vec, bits = C.tie_apply()
    e = B.apply_expect(g, y, vec)
    assert torch.equal(e["y"].float().double(), e["y"]), "scale * g must be an fp32 value"
    assert torch.equal(B.bits16(B.bf16_rne(e["y"].float())), bits) and _tie_other("apply").failures() == []
    y, sc, sh, bits = C.tie_materialize()
    v = y.double() * sc.double().view(1, -1, 1) + sh.double().view(1, -1, 1)
    assert torch.equal(v.float().double(), v) and torch.equal(B.mat_expect(y, sc, sh)[0].double(), v)
    assert torch.equal(B.bits16(B.mat_expect(y, sc, sh)[1]), bits) and _tie_other("mat").failures() == []


# ------------------------------------------------------------------------------------------------- the wrong kernels
MUTANTS = [  # (number in the issue, name, entry points it applies to)
    (1, "trunc", ("fwd", "bwd_data", "apply", "fused", "mat")),
    (2, "twice", ("fwd", "bwd_data", "apply", "fused", "mat")),
    (4, "a_unrounded", ("fwd", "bww")),
    (5, "w_unrounded", ("fwd", "bwd_data")),
    (6, "muladd", ("fwd", "bww", "mat")),
    (7, "mask_bf16", ("reduce", "apply", "fused")),
    (8, "stats_stored", ("fwd",)),
    (9, "drop_chunk", ("fwd", "bwd_data", "bww")),
    (10, "tail_col", ("fwd", "bwd_data", "apply", "fused", "mat")),
    (11, "tail_row", ("fwd", "bwd_data", "mat")),
    (12, "slab_twice", ("bww",)),
    (13, "xhat_unrounded", ("apply", "fused")),
    (14, "swap", ("reduce", "fused")),
]
MUT_PAIRS = [(n, m, e) for n, m, es in MUTANTS for e in es]


def _size(entry, case):
    return case[1] * case[2] * (case[4] if entry in ("fwd", "bwd_data", "bww") else 1)


@pytest.mark.parametrize("num,mut,entry", MUT_PAIRS, ids=[f"{n:02d}-{m}-{e}" for n, m, e in MUT_PAIRS])
def test_wrong_kernel_is_rejected(num, mut, entry):
    """Rejected in at least one case of the entry point (the cases are tried from the smallest up)."""
    tried = []
    for case in sorted(CASES[entry], key=lambda c: _size(entry, c)):
        rep = run(entry, case, mut)
        if rep.failures():
            print(f"{mut} on {entry}: rejected by {case[0]} ({len(tried)} smaller cases accepted it): {rep.failures()[0]}")
            return
        tried.append(case[0])
    raise AssertionError(f"wrong kernel {num} ({mut}) passes every {entry} case: {tried}")


@pytest.mark.parametrize("entry", ["fwd", "bwd_data", "apply", "mat"])
@pytest.mark.parametrize("mut", ["away", "trunc", "twice"])
def test_tie_cases_reject_the_wrong_roundings(entry, mut):
    """3 (round half away from zero) shows in the tie cases only; truncation shows there too.  Rounding twice is invisible on an
    exact tie that is already a 9-bit value - it is caught by the regular cases (above) - so it must PASS here."""
    if entry in ("fwd", "bwd_data"):
        fails = [f for s in C.TIE_SHAPES for f in _tie_run(entry, s, mut)[0].failures()]
    else:
        fails = _tie_other(entry, mut).failures()
    assert (fails == []) == (mut == "twice"), fails[:2]


# ------------------------------------------------------------------------------------------------- the interval test pins bits
PINNED = [("fwd", min(C.FWD_CASES, key=lambda c: (c[2], c[1] * c[3] * c[4]))),
          ("bwd_data", min(C.BWD_DATA_CASES, key=lambda c: (c[3], c[1] * c[2] * c[4]))),
          # apply: N * S = 1 is left to the next case up.  There gm - k1 and xhat are exact zeros, the reference is 0 under a bound
          # that is not, and an interval around 0 holds more than one bf16 value however good the kernel: it cannot be pinned.
          ("apply", min((c for c in C.APPLY_CASES if c[1] * c[2] > 1), key=lambda c: c[1] * c[2])),
          ("fused", min(C.FUSED_CASES, key=lambda c: c[1] * c[2]))]


@pytest.mark.parametrize("entry,case", PINNED, ids=[f"{e}:{c[0]}" for e, c in PINNED])
def test_pinned_share_of_the_smallest_case(entry, case):
    rep = run(entry, case)
    row = [r for r in rep.rows if r["what"] in ("y", "dy")][0]
    print(f"{entry} {case[0]}: pinned share {row['pinned']:.4f}")
    assert row["pinned"] >= 0.9, row["pinned"]
