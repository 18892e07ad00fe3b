"""tests/pw_ref.py checked without a GPU: the float64 reference against float64 autograd of einsum(w, relu(z sc + sh)), the
bit-exact fmaf of ``act32`` against rational arithmetic, and - the proof that the bounds are neither vacuous nor violated by
honest arithmetic - an fp32 CPU evaluation of the same GEMMs inside every bound at every case shape of tests/test_gpu_pw.py."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from mslesions3d_amd import _lib
from tests import pw_cases as C
from tests import pw_ref as P


def gen(seed):
    return torch.Generator().manual_seed(seed)


def case_data(N, Cin, Cout, S, seed=0):
    g = gen(seed + 31 * N + 7 * Cin + 3 * Cout + S)
    z = torch.randn((N, Cin, S), generator=g)
    w = torch.randn((Cout, Cin), generator=g) / Cin ** 0.5
    sc, sh = torch.randn(Cin, generator=g).abs() + 0.5, torch.randn(Cin, generator=g) * 0.3
    dy = torch.randn((N, Cout, S), generator=g)
    return z, w, sc, sh, dy


# ------------------------------------------------------------------------------------------------- act32 / fma32
def _fma_exact(x, a, b):
    """One rounding of the exact x * a + b to fp32, by rational arithmetic."""
    v = Fraction(float(x)) * Fraction(float(a)) + Fraction(float(b))
    if v == 0:
        return np.float32(0.0)
    lo = np.float32(float(v))  # python rounds the rational to float64 correctly; fix the second rounding by hand
    cands = {lo, np.nextafter(lo, np.float32(np.inf)), np.nextafter(lo, np.float32(-np.inf))}
    best = min(cands, key=lambda c: (abs(Fraction(float(c)) - v), int(np.float32(c).view(np.uint32)) & 1))
    return np.float32(best)


def test_fma32_is_one_rounding():
    g = gen(1)
    x, a, b = (torch.randn(4000, generator=g) for _ in range(3))
    # (u + v)(u - v) = 2^-24 - 2^-60 with u = 2^-12, v = 2^-30; b = 1 + 2^-23: the exact sum lies 2^-60 BELOW the midpoint of
    # two fp32 neighbours, float64 rounds it ONTO the midpoint, and rounding that again (ties to even) goes up: fmaf goes down
    u, v = 2.0 ** -12, 2.0 ** -30
    hx = torch.tensor([u + v, -(u + v)], dtype=torch.float32)
    ha = torch.tensor([u - v, u - v], dtype=torch.float32)
    hb = torch.tensor([1.0 + 2.0 ** -23, -(1.0 + 2.0 ** -23)], dtype=torch.float32)
    x, a, b = torch.cat([x, hx]), torch.cat([a, ha]), torch.cat([b, hb])
    got = P.fma32(x, a, b).numpy()
    want = np.array([_fma_exact(*t) for t in zip(x.tolist(), a.tolist(), b.tolist())], dtype=np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    naive = (x.double() * a.double() + b.double()).float().numpy()
    assert not np.array_equal(naive.view(np.uint32), want.view(np.uint32)), "the halfway cases must exercise the double rounding"


def test_act32_keeps_nan_and_signed_zero():
    z = torch.tensor([[[-0.0, 0.0, -1.0, 1.0, float("nan"), -1.0, 2.0]]])
    got = P.act32(z, torch.tensor([1.0]), torch.tensor([-0.0]))[0, 0]
    # fmaf(-0, 1, -0) = -0 and ``-0 < 0`` is false: -0 passes; fmaf(+0, 1, -0) = +0; negatives -> +0; NaN stays
    assert torch.signbit(got[0]) and got[0] == 0 and not torch.signbit(got[1]) and not torch.signbit(got[2]) and got[2] == 0
    assert got[3] == 1 and torch.isnan(got[4]) and got[6] == 2
    z0 = torch.tensor([[[-1.0, 1.0]]])
    got0 = P.act32(z0, torch.tensor([0.0]), torch.tensor([-0.0]))[0, 0]  # -1 * 0 + -0 = -0 ; 1 * 0 + -0 = +0
    assert torch.signbit(got0[0]) and not torch.signbit(got0[1])


# ------------------------------------------------------------------------------------------------- against autograd
@pytest.mark.parametrize("N,Cin,Cout,S", [(2, 32, 8, 37), (1, 64, 96, 5)])
def test_refs_match_float64_autograd(N, Cin, Cout, S):
    z, w, sc, sh, dy = case_data(N, Cin, Cout, S)
    a32 = P.act32(z, sc, sh)
    a = a32.double().requires_grad_(True)
    wd = w.double().requires_grad_(True)
    y = torch.einsum("oc,ncs->nos", wd, a)
    y.backward(dy.double())
    tol = dict(rtol=0, atol=1e-12)
    yr, ya = P.fwd_ref(a32, w)
    assert torch.allclose(yr, y.detach(), **tol) and bool((ya >= yr.abs() - 1e-12).all())
    gr, ga = P.bwd_data_ref(dy, w)
    assert torch.allclose(gr, a.grad, **tol) and bool((ga >= gr.abs() - 1e-12).all())
    dr, da = P.bww_ref(dy, a32)
    assert torch.allclose(dr, wd.grad, **tol) and bool((da >= dr.abs() - 1e-12).all())
    # the activation itself: float64 relu(z sc + sh) rounded once more differs from fmaf's single rounding by < 1 ulp
    a64 = torch.relu(z.double() * sc.double().view(1, -1, 1) + sh.double().view(1, -1, 1))
    assert bool(((a32.double() - a64).abs() <= 2 * P.U * a64.abs() + 1e-45).all())


# ------------------------------------------------------------------------------------------------- honest fp32 inside the bounds
def _ratio(got32, ref, bound):
    r, _, bad = P.worst(got32, ref, bound)
    return r, bad


@pytest.mark.parametrize("case", C.FWD_CASES, ids=[c[0] for c in C.FWD_CASES])
def test_fp32_forward_inside_bound(case):
    _, N, Cin, Cout, S, J = case
    z, w, sc, sh, _ = case_data(N, Cin, Cout, S)
    a32 = P.act32(z, sc, sh)
    y, absdot = P.fwd_ref(a32, w)
    y32 = torch.matmul(w, a32)
    r, bad = _ratio(y32, y, P.gemm_bound(absdot, Cin, J))
    assert bad == 0 and 0 < r <= 1, r
    # statistics: an fp32 reduction in the kernels' own order at every partial width a kernel uses (the case's own among
    # them) - a lane adds its column of the W / 32 tiles one after the other, the square rounded on its own (worse than the
    # kernels' fma), then the 32 lanes meet in a 5-level tree - against the float64 sums of the same fp32 values
    tot, tb = P.stats_total_ref(y, P.gemm_bound(absdot, Cin, J))
    for W in (32, 64, 128, 256):
        ref, bnd = P.stats_ref(y32, W)
        per = (S + W - 1) // W
        yp = torch.nn.functional.pad(y32, (0, per * W - S)).view(N, Cout, per, W // 32, 32)
        s = torch.zeros((N, Cout, per, 32))
        q = torch.zeros((N, Cout, per, 32))
        for t in range(W // 32):
            a = yp[:, :, :, t]
            s = s + a
            q = q + a * a
        for m in (16, 8, 4, 2, 1):
            s = s[..., :m] + s[..., m:2 * m]
            q = q[..., :m] + q[..., m:2 * m]
        assert s.dtype == torch.float32 and q.dtype == torch.float32
        slot = lambda t: t[..., 0].permute(1, 0, 2).reshape(Cout, N * per)
        r, bad = _ratio(torch.stack([slot(s), slot(q)]), ref, bnd)
        assert bad == 0, (W, r)
        r, bad = _ratio(ref.sum(-1), tot, tb + bnd.sum(-1))
        assert bad == 0, (W, r)


@pytest.mark.parametrize("case", C.BWD_DATA_CASES, ids=[c[0] for c in C.BWD_DATA_CASES])
def test_fp32_backward_data_inside_bound(case):
    _, N, Cin, Cout, S, J = case
    _, w, _, _, dy = case_data(N, Cin, Cout, S)
    g, absdot = P.bwd_data_ref(dy, w)
    r, bad = _ratio(torch.matmul(w.t().contiguous(), dy), g, P.gemm_bound(absdot, Cout, J))
    assert bad == 0 and 0 < r <= 1, r


@pytest.mark.parametrize("case", C.BWW_CASES + [("fused",) + C.FUSED_CASE], ids=[c[0] for c in C.BWW_CASES] + ["fused-shape"])
def test_fp32_weight_gradient_inside_bound(case):
    _, N, Cin, Cout, S = case
    ns = _lib.load().msl_pwconv_bwd_weight_nslabs(N, Cin, Cout, S)
    assert ns >= 1
    z, _, sc, sh, dy = case_data(N, Cin, Cout, S)
    a32 = P.act32(z, sc, sh)
    dw, absdot = P.bww_ref(dy, a32)
    # honest fp32 in the kernels' structure: ns slabs of at most L positions each, added in fp32
    L = P.bww_slab_len(N, S, ns)
    df = dy.permute(1, 0, 2).reshape(Cout, N * S)
    af = a32.permute(1, 0, 2).reshape(Cin, N * S)
    acc = torch.zeros(Cout, Cin)
    for k in range(0, N * S, L):
        acc = acc + torch.matmul(df[:, k:k + L], af[:, k:k + L].t())
    r, bad = _ratio(acc, dw, P.bww_bound(absdot, N, S, ns))
    assert bad == 0 and 0 < r <= 1, r


# ------------------------------------------------------------------------------------------------- paths
ROUTE_CASES = ([(C.OP_FWD, c) for c in C.FWD_CASES] + [(C.OP_FWD, c) for c in C.FOLD_CASES]
               + [(C.OP_BWD_DATA, c) for c in C.BWD_DATA_CASES] + [(C.OP_BWD_WEIGHT, c) for c in C.BWW_CASES])


@pytest.mark.parametrize("op,case", ROUTE_CASES, ids=[f"op{op}:{c[0]}" for op, c in ROUTE_CASES])
def test_case_reaches_the_kernel_its_id_names(op, case):
    """The library's own route (host arithmetic) for every case of the four tables; the forward's kind holds with and without
    statistics, and the NT2 / NT1 ids name the column tiles per wave that the partial count shows."""
    id_, N, Cin, Cout, S = case[:5]
    L = _lib.load()
    want = C.expected_kind(id_)
    for stats in ((0, 1) if op == C.OP_FWD else (0,)):
        got = L.msl_pwconv_route_kind(op, 0, N, Cin, Cout, S, stats)
        assert got == want, f"{id_}: route kind {got}, the id names {want}"
    if "NT2" in id_ or "NT1" in id_:
        assert L.msl_pwconv_fwd_num_partials(N, Cin, Cout, S) == N * -(-S // (256 if "NT2" in id_ else 128))


def test_fused_case_and_route_query_refusals():
    L = _lib.load()
    N, Cin, Cout, S = C.FUSED_CASE
    assert L.msl_pwconv_route_kind(C.OP_BWD_FUSED, 0, N, Cin, Cout, S, 0) == C.KIND["fused"]
    assert L.msl_pwconv_route_kind(C.OP_BWD_FUSED, 1, N, Cin, Cout, S, 0) == C.KIND["none"]       # fp32 only
    assert L.msl_pwconv_route_kind(C.OP_BWD_FUSED, 0, 1, Cin, Cout, 65408, 0) == C.KIND["none"]   # 511 strips
    ok = (2, 32, 64, 4096, 0)
    assert L.msl_pwconv_route_kind(0, 0, *ok) == C.KIND["wave"]
    for args in ((-1, 0) + ok, (4, 0) + ok, (0, 2) + ok, (0, -1) + ok, (0, 0, 0, 32, 64, 4096, 0), (0, 0, 2, 0, 64, 4096, 0),
                 (0, 0, 2, 32, -64, 4096, 0), (0, 0, 2, 32, 64, 0, 0)):
        assert L.msl_pwconv_route_kind(*args) == -1, args

