"""The bf16 pointwise GEMM family (msl_pwconv_fwd_bf16, _fold, msl_pwconv_bwd_data_bf16, msl_pwconv_bwd_weight_slabs_bf16), the
materialise kernels of csrc/bf16.hip and the four BatchNorm+ReLU-backward kernels of csrc/bn.hip on bf16 storage, path by path,
against the float64 reference
of tests/bf16pw_ref.py (bounds derived there from the kernel text, not tuned).

bf16 outputs meet the rounding-interval test - bf16_rne(ref - B) <= stored <= bf16_rne(ref + B) - which pins most elements to
one bit pattern; the tie cases demand written-down bits.  The cases are the CPU data of tests/bf16pw_cases.py; every test first
asserts, from the dispatch arithmetic mirrored there (and the library's queries where one exists), the path its id names, and
tests/test_bf16pw_ref_cpu.py proves at the same cases that an honest fp32 emulation passes every check and fourteen wrong
kernels do not.  Every output and partial buffer is NaN-filled (a finite sentinel where NaNs are under test) between guard bands
that must come back untouched; every entry runs twice into fresh buffers and must repeat itself bit for bit; every refusal checks
the return code and that nothing was written.  With MSL_BF16PW_RATIO_LOG=<file> every comparison appends
"<case id> <what> <error / bound> <pinned share>" (DESIGN.md, Appendix D)."""
import os

import pytest
import torch

from mslesions3d_amd import _lib
from mslesions3d_amd._lib import ptr
from tests import bf16pw_cases as C
from tests import bf16pw_ref as B
from tests.test_gpu_pw import Guarded, dev, same_bits, st
from tests.test_gpu_pw import _release_kept  # noqa: F401  (autouse fixture: frees what dev() and Guarded keep alive)

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NAN = float("nan")
SENTINEL = -12288.0  # finite and a bf16 value: guard bands and pre-fill where the kernel under test may itself produce NaNs
EPS = 1e-5
ERR_ARG, ERR_UNSUPPORTED = -1, -2


def same(a, b):
    """Bit identity of two device tensors of one dtype (bf16 included)."""
    if a.element_size() == 2:
        return a.dtype == b.dtype and bool(torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16)))
    return same_bits(a, b)


def finish(rep):
    """Print and log every comparison of the case, then fail on the first bad one."""
    log = os.environ.get("MSL_BF16PW_RATIO_LOG")
    for r in rep.rows:
        line = f"{rep.id.replace(' ', '_')} {r['what']} {r['ratio']:.4f} {'-' if r['pinned'] is None else format(r['pinned'], '.4f')}"
        print(line)
        if log:
            with open(log, "a") as f:
                f.write(line + "\n")
    assert rep.failures() == [], "\n".join(rep.failures())


def twice(run):
    """run() -> list of Guarded outputs; a second run into fresh buffers must repeat the first bit for bit."""
    a, b = run(), run()
    for x, y in zip(a, b):
        if x is not None:
            assert same(x.full, y.full), "a second run into fresh buffers gave other bits"
    return a


# ------------------------------------------------------------------------------------------------- msl_pwconv_fwd_bf16
def run_fwd(z16, sc, sh, w, N, Cin, Cout, S, stats, guard=NAN, expect=0):
    L = _lib.load()
    NP = L.msl_pwconv_fwd_bf16_num_partials(N, S)
    assert NP == N * C.cdiv(S, 64) * 2
    y = Guarded(N * Cout * S, dtype=BF, guard=guard)
    part = Guarded(2 * Cout * NP, dtype=torch.float64, guard=guard) if stats else None
    rc = L.msl_pwconv_fwd_bf16(ptr(z16), ptr(sc), ptr(sh), ptr(w), ptr(y.v), ptr(part.v) if stats else None, N, Cin, Cout, S, st())
    torch.cuda.synchronize()
    assert rc == expect, f"msl_pwconv_fwd_bf16 returned {rc}, expected {expect}"
    if rc == 0:
        y.intact("y")
        if stats:
            part.intact("partials")
    return y, part


def fwd_forms(id_, d, A, N, Cin, Cout, S, guard=NAN):
    """Affine + statistics (twice), affine only, statistics only and neither (the last two on the host-activated bf16 input):
    y bit-identical across the four, the partials across the two that emit them.  -> (y, partials) of the first."""
    zd, ad, wd, scd, shd = dev(d["z"].to(BF)), dev(A.to(BF)), dev(d["w"]), dev(d["sc"]), dev(d["sh"])
    y0, p0 = twice(lambda: run_fwd(zd, scd, shd, wd, N, Cin, Cout, S, True, guard))
    for form, (x, aff, stats) in dict(affine=(zd, True, False), stats=(ad, False, True), plain=(ad, False, False)).items():
        y, p = run_fwd(x, scd if aff else None, shd if aff else None, wd, N, Cin, Cout, S, stats, guard)
        assert same(y.v, y0.v), f"{id_}: y of the {form} form differs from the affine + statistics form"
        if p is not None:
            assert same(p.v, p0.v), f"{id_}: partials of the {form} form differ"
    assert same(zd, d["z"].to(BF).to("cuda")) and same(wd, d["w"].to("cuda")), f"{id_}: inputs changed"
    NP = p0.n // (2 * Cout)
    return y0.v.float().cpu().view(N, Cout, S), p0.v.cpu().view(2, Cout, NP)


@pytest.mark.parametrize("case", C.FWD_CASES, ids=[c[0] for c in C.FWD_CASES])
def test_pw_fwd_bf16_paths(case):
    id_, N, Cin, Cout, S, _ = case
    C.assert_path("fwd", case)
    d = C.gemm_data(N, Cin, Cout, S)
    A, Wb = B.fwd_operands(d["z"], d["sc"], d["sh"], d["w"])
    y, part = fwd_forms(id_, d, A, N, Cin, Cout, S)
    rep = B.Report(id_)
    B.check_fwd(rep, B.fwd_expect(A, Wb, Cin), y, part)  # J = 0: serial K
    finish(rep)


def test_pw_fwd_bf16_nonfinite():
    """A NaN and a +Inf in z: NaN / Inf exactly where the float64 reference has them, every other element keeps the bits of the
    clean run."""
    id_, N, Cin, Cout, S = C.NONFINITE_FWD
    d = C.gemm_data(N, Cin, Cout, S)
    A0, _ = B.fwd_operands(d["z"], d["sc"], d["sh"], d["w"])
    y_clean, p_clean = fwd_forms(id_ + ":clean", d, A0, N, Cin, Cout, S, SENTINEL)
    d["z"][0, 5, 3], d["z"][1, 40, 135] = NAN, float("inf")
    A, Wb = B.fwd_operands(d["z"], d["sc"], d["sh"], d["w"])
    assert bool(torch.isnan(A[0, 5, 3])) and bool(torch.isinf(A[1, 40, 135]))
    y, part = fwd_forms(id_, d, A, N, Cin, Cout, S, SENTINEL)
    e = B.fwd_expect(A, Wb, Cin)
    assert bool(torch.isnan(e["y"][0, :, 3]).all()) and bool(torch.isinf(e["y"][1, :, 135]).all())
    assert int((~torch.isfinite(e["y"])).sum()) == 2 * Cout
    rep = B.Report(id_)
    B.check_fwd(rep, e, y, part)
    fin = torch.isfinite(e["y"])
    rep.bits("untouched-elements", B.bits16(y)[fin], B.bits16(y_clean)[fin])
    finp = torch.isfinite(B.stats_expect(e["y"], e["B"], S)[0])
    assert int((~finp).sum()) == 2 * 2 * Cout
    rep.bits("untouched-partials", part.view(torch.int64)[finp], p_clean.view(torch.int64)[finp])
    finish(rep)


@pytest.mark.parametrize("shape", C.TIE_SHAPES, ids=[s[0] for s in C.TIE_SHAPES])
def test_pw_fwd_and_bwd_data_bf16_ties(shape):
    """Exact fp32 accumulators on bf16 ties: the stored bits are the case's TIE_BITS (round to nearest even), B = 0."""
    id_, N, M, K, S = shape
    W, A, bits = C.tie_gemm(N, M, K, S)
    assert (C.tile_path(N, M, K, S)[0] == "tr") == ("tr" in id_)
    rep = B.Report(id_)
    # forward without the affine (its ReLU would clear the negative ties) ...
    y, _ = twice(lambda: run_fwd(dev(A.to(BF)), None, None, dev(W), N, K, M, S, True))
    rep.bits("fwd-bits", B.bits16(y.v.cpu().view(N, M, S)), bits)
    # ... and with scale 1, shift 0: the negative patterns' operands become zeros, the positive ties stay
    y, _ = run_fwd(dev(A.to(BF)), dev(torch.ones(K)), dev(torch.zeros(K)), dev(W), N, K, M, S, False)
    rep.bits("fwd-affine-bits", B.bits16(y.v.cpu().view(N, M, S)), torch.where(bits < 0x8000, bits, torch.zeros_like(bits)))
    g = Guarded(N * M * S, dtype=BF)
    _lib.call("msl_pwconv_bwd_data_bf16", ptr(dev(A.to(BF))), ptr(dev(W.t().contiguous())), ptr(g.v), N, M, K, S, st())
    torch.cuda.synchronize()
    g.intact("g_in")
    rep.bits("bwd-data-bits", B.bits16(g.v.cpu().view(N, M, S)), bits)
    finish(rep)


# ------------------------------------------------------------------------------------------------- msl_pwconv_fwd_bf16_fold
def finalize(parts, in_np, count, gamma, beta, Cc):
    vec = Guarded(4 * Cc)
    v = vec.v.view(4, Cc)
    _lib.call("msl_bn_finalize", ptr(parts), in_np, float(count), ptr(gamma), ptr(beta), None, None, None, 0.1, EPS, ptr(v[0]),
              ptr(v[1]), ptr(v[2]), ptr(v[3]), Cc, st())
    torch.cuda.synchronize()
    vec.intact("finalize vectors")
    return v


@pytest.mark.parametrize("in_np", C.FOLD_NP)
@pytest.mark.parametrize("case", C.FOLD_CASES, ids=[c[0] for c in C.FOLD_CASES])
def test_pw_fwd_bf16_fold_is_finalize_plus_fwd(case, in_np):
    id_, N, Cin, Cout, S, _ = case
    C.assert_path("fwd", case)
    L = _lib.load()
    g = C.gen(7100 + in_np + S)
    d = C.gemm_data(N, Cin, Cout, S)
    gamma, beta = torch.randn(Cin, generator=g).abs() + 0.5, torch.randn(Cin, generator=g) * 0.3
    parts = C.fold_partials(Cin, in_np, float(N * S), g)
    pd, gd, bd, zd, wd = dev(parts), dev(gamma), dev(beta), dev(d["z"].to(BF)), dev(d["w"])
    v = finalize(pd, in_np, N * S, gd, bd, Cin)
    y0, p0 = run_fwd(zd, v[0], v[1], wd, N, Cin, Cout, S, True)

    def fold(stats):
        y = Guarded(N * Cout * S, dtype=BF)
        p = Guarded(p0.n, dtype=torch.float64) if stats else None
        rc = L.msl_pwconv_fwd_bf16_fold(ptr(zd), ptr(pd), in_np, float(N * S), ptr(gd), ptr(bd), EPS, ptr(wd), ptr(y.v),
                                        ptr(p.v) if stats else None, N, Cin, Cout, S, st())
        torch.cuda.synchronize()
        assert rc == 0
        y.intact("fold: y")
        if stats:
            p.intact("fold: partials")
        return y, p

    y1, p1 = twice(lambda: fold(True))
    assert same(y1.v, y0.v), "fold: y differs from msl_bn_finalize + msl_pwconv_fwd_bf16"
    assert same(p1.v, p0.v), "fold: partials differ from msl_bn_finalize + msl_pwconv_fwd_bf16"
    assert same(fold(False)[0].v, y0.v), "fold without statistics: y differs"
    A, Wb = B.fwd_operands(d["z"], v[0].cpu(), v[1].cpu(), d["w"])
    rep = B.Report(f"fold{in_np}:{id_}")
    B.check_fwd(rep, B.fwd_expect(A, Wb, Cin), y1.v.float().cpu().view(N, Cout, S), p1.v.cpu().view(2, Cout, -1))
    finish(rep)


def test_pw_fwd_bf16_fold_refusals():
    L = _lib.load()
    for id_, N, Cin, Cout, S, in_np in C.FOLD_UNSUPPORTED + [("null-partials", 1, 32, 8, 8, 4), ("in_np0", 1, 32, 8, 8, 0)]:
        z, w, gb = dev(torch.ones(N * Cin * S).to(BF)), dev(torch.ones(Cout * Cin)), dev(torch.ones(Cin))
        parts = dev(torch.ones(2 * Cin * max(in_np, 1), dtype=torch.float64))
        y = Guarded(N * Cout * S, dtype=BF)
        part = Guarded(2 * Cout * L.msl_pwconv_fwd_bf16_num_partials(N, S), dtype=torch.float64)
        rc = L.msl_pwconv_fwd_bf16_fold(ptr(z), None if id_ == "null-partials" else ptr(parts), in_np, float(N * S), ptr(gb), ptr(gb),
                                        EPS, ptr(w), ptr(y.v), ptr(part.v), N, Cin, Cout, S, st())
        torch.cuda.synchronize()
        assert rc == (ERR_UNSUPPORTED if id_ in ("in_np65", "Cin1056") else ERR_ARG), (id_, rc)
        y.untouched(f"{id_}: y")
        part.untouched(f"{id_}: partials")


# ------------------------------------------------------------------------------------------------- msl_pwconv_bwd_data_bf16
@pytest.mark.parametrize("case", C.BWD_DATA_CASES, ids=[c[0] for c in C.BWD_DATA_CASES])
def test_pw_bwd_data_bf16_paths(case):
    id_, N, Cin, Cout, S, _ = case
    C.assert_path("bwd_data", case)
    d = C.gemm_data(N, Cin, Cout, S)
    dyd, wd = dev(d["dy"].to(BF)), dev(d["w"])

    def run():
        g = Guarded(N * Cin * S, dtype=BF)
        _lib.call("msl_pwconv_bwd_data_bf16", ptr(dyd), ptr(wd), ptr(g.v), N, Cin, Cout, S, st())
        torch.cuda.synchronize()
        g.intact("g_in")
        return [g]

    g, = twice(run)
    assert same(dyd, d["dy"].to(BF).to("cuda")) and same(wd, d["w"].to("cuda")), "inputs changed"
    rep = B.Report(id_)
    B.check_fwd(rep, B.bwd_data_expect(d["dy"], B.bf16_rne(d["w"]), Cout), g.v.float().cpu().view(N, Cin, S))  # J = 0
    finish(rep)


def test_pw_bwd_data_bf16_refusals():
    L = _lib.load()
    for N, Cin, Cout, S in C.BWD_DATA_REFUSED:
        dy, w = dev(torch.ones(N * Cout * S).to(BF)), dev(torch.ones(Cout * Cin))
        g = Guarded(N * Cin * S, dtype=BF)
        assert L.msl_pwconv_bwd_data_bf16(ptr(dy), ptr(w), ptr(g.v), N, Cin, Cout, S, st()) == ERR_ARG
        torch.cuda.synchronize()
        g.untouched("g_in")


# ------------------------------------------------------------------------------------------------- weight gradient
def run_bww(d, affine, N, Cin, Cout, S, ns, guard=NAN):
    """-> the Guarded (ns + 1 slabs: the last must stay untouched) output of one launch."""
    L = _lib.load()
    out = Guarded((ns + 1) * Cout * Cin, guard=guard)
    if guard == guard:
        out.v.fill_(guard)
    rc = L.msl_pwconv_bwd_weight_slabs_bf16(ptr(dev(d["dy"].to(BF))), ptr(dev(d["z"].to(BF))), ptr(dev(d["sc"])) if affine else None,
                                            ptr(dev(d["sh"])) if affine else None, ptr(out.v), N, Cin, Cout, S, st())
    torch.cuda.synchronize()
    assert rc == 0
    out.intact("slabs")
    behind = out.v[ns * Cout * Cin:]
    assert bool((torch.isnan(behind) if guard != guard else behind == guard).all()), "wrote behind its nslabs slabs"
    return out


@pytest.mark.parametrize("case", C.BWW_CASES, ids=[c[0] for c in C.BWW_CASES])
def test_pw_bwd_weight_bf16_paths(case):
    id_, N, Cin, Cout, S, path = case
    C.assert_path("bww", case)
    ns = _lib.load().msl_pwconv_bwd_weight_bf16_nslabs(N, Cin, Cout, S)
    assert ns == (path[2] if path[0] == "mfma" else 1)
    L_ = path[3] * 64 if path[0] == "mfma" else path[2]
    d = C.gemm_data(N, Cin, Cout, S)
    rep = B.Report(id_)
    for affine in (True, False):
        out, = twice(lambda: [run_bww(d, affine, N, Cin, Cout, S, ns)])
        e = B.bww_expect(d["dy"], d["z"], d["sc"], d["sh"], affine, L_, ns)
        rep.bound("dW-affine" if affine else "dW-plain", out.v[:ns * Cout * Cin].view(ns, Cout, Cin).cpu().double().sum(0), e["dw"], e["B"])
    finish(rep)


@pytest.mark.parametrize("case", C.NONFINITE_BWW, ids=[c[0] for c in C.NONFINITE_BWW])
def test_pw_bwd_weight_bf16_nan_in_z(case):
    """A NaN in z reaches dW[:, its channel] through both weight-gradient kernels, with and without the affine (msl::act keeps a
    NaN pre-activation, as the forward does), and nowhere else."""
    id_, N, Cin, Cout, S = case
    assert (C.bww_path(N, Cin, Cout, S)[0] == "any") == ("any" in id_)
    ns = _lib.load().msl_pwconv_bwd_weight_bf16_nslabs(N, Cin, Cout, S)
    path = C.bww_path(N, Cin, Cout, S)
    L_ = path[3] * 64 if path[0] == "mfma" else path[2]
    d = C.gemm_data(N, Cin, Cout, S)
    d["z"][0, 3, 9] = NAN
    rep = B.Report(id_)
    for affine in (True, False):
        out = run_bww(d, affine, N, Cin, Cout, S, ns, SENTINEL)
        e = B.bww_expect(d["dy"], d["z"], d["sc"], d["sh"], affine, L_, ns)
        nan = torch.isnan(e["dw"])
        assert bool(nan[:, 3].all()) and int(nan.sum()) == Cout
        rep.bound("dW-affine" if affine else "dW-plain", out.v[:ns * Cout * Cin].view(ns, Cout, Cin).cpu().double().sum(0), e["dw"], e["B"])
    finish(rep)


# ------------------------------------------------------------------------------------------------- materialise
def _filled(n, dtype, value):
    b = Guarded(n, dtype=dtype, guard=value)
    b.v.fill_(value)
    return b


HALO = 7.0  # finite pre-fill of the padded outputs: the kernels must not write the halo


def run_materialize(y, sc, sh, N, Cc, dims, plain):
    D, H, W = dims
    S = D * H * W
    pl = Guarded(N * Cc * S) if plain else None
    cl = _filled(N * (D + 2) * (H + 2) * (W + 2) * Cc, BF, HALO)
    _lib.call("msl_bn_relu_materialize_bf16", ptr(y), ptr(sc), ptr(sh), ptr(pl.v) if plain else None, ptr(cl.v), N, Cc, D, H, W, st())
    torch.cuda.synchronize()
    cl.intact("pad_cl")
    if plain:
        pl.intact("plain")
    return [pl, cl]


def check_cl(rep, cl, want_ncs, N, Cc, dims):
    D, H, W = dims
    got = cl.v.float().cpu().view(N, D + 2, H + 2, W + 2, Cc)
    inner = torch.zeros_like(got, dtype=torch.bool)
    inner[:, 1:-1, 1:-1, 1:-1] = True
    rep.bits("pad_cl-halo", B.bits16(got[~inner]), B.bits16(torch.full_like(got[~inner], HALO)))
    rep.bits("pad_cl-interior", B.bits16(got[:, 1:-1, 1:-1, 1:-1]), B.bits16(want_ncs.view(N, Cc, D, H, W).permute(0, 2, 3, 4, 1)))


@pytest.mark.parametrize("case", C.MAT_CASES, ids=[c[0] for c in C.MAT_CASES])
def test_materialize_bf16(case):
    id_, N, Cc, dims = case
    d = C.mat_data(N, Cc, dims)
    a, ab = B.mat_expect(d["y"], d["sc"], d["sh"])
    yd, scd, shd = dev(d["y"].to(BF)), dev(d["sc"]), dev(d["sh"])
    pl, cl = twice(lambda: run_materialize(yd, scd, shd, N, Cc, dims, True))
    _, cl2 = run_materialize(yd, scd, shd, N, Cc, dims, False)
    assert same(cl2.full, cl.full), "pad_cl differs without ``plain``"
    rep = B.Report(id_)
    rep.bits("plain", B.f32bits(pl.v), B.f32bits(a))
    check_cl(rep, cl, ab, N, Cc, dims)
    finish(rep)


def test_materialize_bf16_tie_and_refusal():
    y, sc, sh, bits = C.tie_materialize()
    _, cl = run_materialize(dev(y.to(BF)), dev(sc), dev(sh), 1, 8, (1, 1, 3), False)
    rep = B.Report("tie:materialize")
    got = cl.v.float().cpu().view(1, 3, 3, 5, 8)[:, 1, 1, 1:-1]  # (1, 3 positions, 8 channels)
    rep.bits("pad_cl-bits", B.bits16(got.permute(0, 2, 1)), bits)
    finish(rep)
    L = _lib.load()
    pl, cl = Guarded(12), Guarded(27 * 12, dtype=BF)
    x = dev(torch.ones(12).to(BF))
    assert L.msl_bn_relu_materialize_bf16(ptr(x), ptr(dev(torch.ones(12))), ptr(dev(torch.ones(12))), ptr(pl.v), ptr(cl.v), 1, 12, 1, 1,
                                          1, st()) == ERR_ARG  # C % 8 != 0
    torch.cuda.synchronize()
    pl.untouched("plain")
    cl.untouched("pad_cl")


@pytest.mark.parametrize("case", C.PAD32_CASES, ids=[c[0] for c in C.PAD32_CASES])
def test_materialize_bf16_pad32_and_fold(case):
    id_, N, Cc, dims = case
    D, H, W = dims
    S = D * H * W
    L = _lib.load()
    d = C.mat_data(N, Cc, dims)
    yd = dev(d["y"].to(BF))
    n_pad = N * Cc * (D + 2) * (H + 2) * (W + 2)
    rep = B.Report(id_)

    def check(what, pad, sc, sh):
        got = pad.v.cpu().view(N, Cc, D + 2, H + 2, W + 2)
        inner = torch.zeros_like(got, dtype=torch.bool)
        inner[:, :, 1:-1, 1:-1, 1:-1] = True
        rep.bits(what + "-halo", B.f32bits(got[~inner]), B.f32bits(torch.full_like(got[~inner], HALO)))
        rep.bits(what + "-interior", B.f32bits(got[:, :, 1:-1, 1:-1, 1:-1]), B.f32bits(B.act32(d["y"], sc, sh).view(N, Cc, D, H, W)))

    def explicit(sc, sh):
        pad = _filled(n_pad, torch.float32, HALO)
        _lib.call("msl_bn_relu_materialize_bf16_pad32", ptr(yd), ptr(sc), ptr(sh), ptr(pad.v), N, Cc, D, H, W, st())
        torch.cuda.synchronize()
        pad.intact("pad32")
        return [pad]

    scd, shd = dev(d["sc"]), dev(d["sh"])
    pad, = twice(lambda: explicit(scd, shd))
    check("pad32", pad, d["sc"], d["sh"])
    for in_np in C.PAD32_FOLD_NP:
        g = C.gen(7300 + in_np + S)
        gamma, beta = torch.randn(Cc, generator=g).abs() + 0.5, torch.randn(Cc, generator=g) * 0.3
        pd, gd, bd = dev(C.fold_partials(Cc, in_np, float(N * S), g)), dev(gamma), dev(beta)
        v = finalize(pd, in_np, N * S, gd, bd, Cc)
        p0, = explicit(v[0], v[1])

        def fold():
            p = _filled(n_pad, torch.float32, HALO)
            rc = L.msl_bn_relu_materialize_bf16_pad32_fold(ptr(yd), ptr(pd), in_np, float(N * S), ptr(gd), ptr(bd), EPS, ptr(p.v), N, Cc,
                                                           D, H, W, st())
            torch.cuda.synchronize()
            assert rc == 0
            p.intact("pad32 fold")
            return [p]

        p1, = twice(fold)
        assert same(p1.full, p0.full), f"in_np {in_np}: the fold differs from msl_bn_finalize + explicit vectors"
        check(f"pad32-fold{in_np}", p1, v[0].cpu(), v[1].cpu())
    finish(rep)


# ------------------------------------------------------------------------------------------------- BatchNorm + ReLU backward
def bn_dev(d):
    return dev(d["g"].to(BF)), dev(d["y"].to(BF)), dev(d["vec"])


@pytest.mark.parametrize("case", C.REDUCE_CASES, ids=[c[0] for c in C.REDUCE_CASES])
def test_bn_relu_bwd_reduce_bf16(case):
    id_, N, S = case
    Cc = C.BN_C
    d = C.bn_data(N, S)
    gd, yd, vd = bn_dev(d)
    NP = _lib.load().msl_bn_relu_bwd_bf16_num_partials(N, S)
    assert NP == N * C.reduce_chunks(S)

    def run():
        p = Guarded(2 * Cc * NP, dtype=torch.float64)
        _lib.call("msl_bn_relu_bwd_reduce_bf16", ptr(gd), ptr(yd), ptr(vd[0]), ptr(vd[1]), ptr(vd[2]), ptr(vd[3]), ptr(p.v), N, Cc, S, st())
        torch.cuda.synchronize()
        p.intact("partials")
        return [p]

    p, = twice(run)
    rep = B.Report(id_)
    rep.bound("partials", p.v.cpu().view(2, Cc, NP), *B.reduce_expect(d["g"], d["y"], d["vec"]))  # n_t = 16
    finish(rep)


def run_apply(gd, yd, vd, N, Cc, S, inplace, guard=NAN):
    dy = Guarded(N * Cc * S, dtype=BF, guard=guard)
    if inplace:
        dy.v.copy_(gd.reshape(-1))
    _lib.call("msl_bn_relu_bwd_apply_bf16", ptr(dy.v if inplace else gd), ptr(yd), ptr(vd), ptr(dy.v), N, Cc, S, st())
    torch.cuda.synchronize()
    dy.intact("dy")
    return [dy]


@pytest.mark.parametrize("case", C.APPLY_CASES, ids=[c[0] for c in C.APPLY_CASES])
def test_bn_relu_bwd_apply_bf16(case):
    id_, N, S, _ = case
    C.assert_path("apply", case)
    Cc = C.BN_C
    d = C.bn_data(N, S)
    gd, yd, vd = bn_dev(d)
    dy, = twice(lambda: run_apply(gd, yd, vd, N, Cc, S, False))
    dy_in, = run_apply(gd, yd, vd, N, Cc, S, True)
    assert same(dy_in.v, dy.v), "in place (dy aliasing g) differs from a separate dy"
    assert same(gd, d["g"].to(BF).to("cuda")), "g changed by the out-of-place form"
    e = B.apply_expect(d["g"], d["y"], d["vec"])
    rep = B.Report(id_)
    rep.interval("dy", dy.v.float().cpu().view(N, Cc, S), e["y"], e["B"])
    finish(rep)


def test_bn_relu_bwd_apply_bf16_tie_and_nonfinite():
    g, y, vec, bits = C.tie_apply()
    dy, = run_apply(dev(g.to(BF)), dev(y.to(BF)), dev(vec), 1, 1, 12, False)
    rep = B.Report("tie:apply")
    rep.bits("dy-bits", B.bits16(dy.v.cpu().view(1, 1, 12)), bits)
    finish(rep)
    id_, N, S = C.NONFINITE_APPLY
    Cc = C.BN_C
    d = C.bn_data(N, S)
    clean, = run_apply(*bn_dev(d), N, Cc, S, False, SENTINEL)
    op = B.fma32(d["y"], d["vec"][0].view(1, -1, 1), d["vec"][1].view(1, -1, 1)) > 0
    i0, i1 = int(op[0, 1].nonzero()[0]), int(op[1, 2].nonzero()[-1])  # under an open mask
    d["g"][0, 1, i0], d["g"][1, 2, i1] = NAN, float("inf")
    dy, = run_apply(*bn_dev(d), N, Cc, S, False, SENTINEL)
    e = B.apply_expect(d["g"], d["y"], d["vec"])
    assert bool(torch.isnan(e["y"][0, 1, i0])) and float(e["y"][1, 2, i1]) == float("inf") and int((~torch.isfinite(e["y"])).sum()) == 2
    rep = B.Report(id_)
    got = dy.v.float().cpu().view(N, Cc, S)
    rep.interval("dy", got, e["y"], e["B"])
    fin = torch.isfinite(e["y"])
    rep.bits("untouched-elements", B.bits16(got)[fin], B.bits16(clean.v.float().cpu().view(N, Cc, S))[fin])
    finish(rep)


@pytest.mark.parametrize("case", C.FUSED_CASES, ids=[c[0] for c in C.FUSED_CASES])
def test_bn_relu_bwd_fused_bf16(case):
    id_, N, S, _ = case
    C.assert_path("fused", case)
    Cc = C.BN_C
    n_t = C.fused_path(N, S)[1]
    d = C.bn_data(N, S)
    gd, yd, vd = bn_dev(d)

    def run(inplace=False):
        dy, dg, db = Guarded(N * Cc * S, dtype=BF), Guarded(Cc), Guarded(Cc)
        if inplace:
            dy.v.copy_(gd.reshape(-1))
        _lib.call("msl_bn_relu_bwd_fused_bf16", ptr(dy.v if inplace else gd), ptr(yd), ptr(vd), ptr(dg.v), ptr(db.v), ptr(dy.v), N, Cc, S,
                  st())
        torch.cuda.synchronize()
        for b, what in ((dy, "dy"), (dg, "dgamma"), (db, "dbeta")):
            b.intact(what)
        return [dy, dg, db]

    dy, dg, db = twice(run)
    for a, b in zip(run(True), (dy, dg, db)):
        assert same(a.v, b.v), "in place (dy aliasing g) differs from a separate dy"
    rep = B.Report(id_)
    B.check_fused(rep, B.fused_expect(d["g"], d["y"], d["vec"], n_t), dy.v.float().cpu().view(N, Cc, S), dg.v.cpu(), db.v.cpu())
    finish(rep)


# ------------------------------------------------------------------------------------------------- recorded bits
def test_pw_bf16_bits_are_the_recorded_ones():
    """Every output buffer of the GEMM, fold, bwd-data and weight-gradient tables has the SHA-256 that tests/golden/pw_bits.json
    recorded before the host code got its single route (make_pw_bits's docstring)."""
    import json
    from tests.golden import make_pw_bits as M
    with open(M.OUT) as f:
        want = json.load(f)["bf16"]
    got = M.digests_bf16("cuda")
    assert sorted(got) == sorted(want), "the cases are not the recorded ones"
    assert {k.split()[0] for k in want} == {"msl_pwconv_fwd_bf16", "msl_pwconv_fwd_bf16_fold", "msl_pwconv_bwd_data_bf16",
                                            "msl_pwconv_bwd_weight_slabs_bf16"}
    bad = [k for k in want if got[k] != want[k]]
    assert not bad, f"{len(bad)}/{len(want)} buffers differ from the recorded bits: {bad[:8]}"
