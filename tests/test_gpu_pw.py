"""Every fp32 pointwise-convolution entry point of csrc/pwconv.hip and csrc/pwfused.hip, path by path, against the float64
reference of tests/pw_ref.py (bounds derived there, not tuned; each failure message prints the worst error / bound).

The activation vectors are made on the host and ``pw_ref.act32`` reproduces msl::act bit for bit, so the reference GEMM takes
the kernel's own operands and its ReLU mask is the kernel's: no element is excluded anywhere and no margin around zero is
needed.  Every output is pre-filled with NaN and sits between guard bands that must come back untouched (the masked stores
at column and row tails are the thing under test).  Each case id names the kernel path it is meant to reach (tests/pw_cases.py);
DESIGN.md, Appendix A, lists every kernel instantiation with the case meant to launch it.  With MSL_PW_RATIO_LOG=<file> every comparison appends
"<path> <what> <error / bound>" to that file (for the error / bound table of DESIGN.md); MSL_PW_LAUNCH_LOG=<file> logs the
library's launch counter around every test (see ``_release_kept``)."""
import ctypes
import functools
import os

import pytest
import torch

from mslesions3d_amd import _lib
from mslesions3d_amd._lib import ptr
from tests import bn_ref as R
from tests import pw_cases as C
from tests import pw_ref as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-5
G = 64  # guard elements on each side of every output (a multiple of 4: the views stay 16-byte aligned)
NAN = float("nan")


def st():
    return torch.cuda.current_stream().cuda_stream


_KEEP = []


def dev(t):
    """Move to the GPU and keep the tensor alive until the end of the test."""
    d = t.detach().to(DEV).contiguous()
    _KEEP.append(d)
    return d


@pytest.fixture(autouse=True)
def _release_kept(request):
    """Frees the kept tensors.  With MSL_PW_LAUNCH_LOG=<file>, also appends "<test id>\t<n0>\t<n1>": the library's launch
    counter before and after the test, so the dispatches n0 .. n1 - 1 of the library in a kernel trace of this file (in order,
    every kernel that is neither torch's nor the runtime's) are this test's - how DESIGN.md ties kernels to case ids."""
    log = os.environ.get("MSL_PW_LAUNCH_LOG")
    count = _lib.load().msl_thread_launch_count
    n0 = count()
    yield
    torch.cuda.synchronize()
    _KEEP.clear()
    if log:
        with open(log, "a") as f:
            f.write(f"{request.node.nodeid}\t{n0}\t{count()}\n")


class Guarded:
    """An output buffer of n elements, NaN-filled, between two bands of G guard elements: NaN, or the finite ``guard`` where the
    kernel under test may itself produce NaNs (a stray NaN stored into a NaN band would not show)."""

    def __init__(self, n, dtype=torch.float32, guard=NAN):
        self.n, self.guard = n, guard
        self.full = torch.full((n + 2 * G,), NAN, dtype=dtype, device=DEV)
        if guard == guard:
            self.full[:G] = guard
            self.full[G + n:] = guard
        self.v = self.full[G:G + n]
        _KEEP.append(self.full)

    def intact(self, what):
        bands = torch.cat([self.full[:G], self.full[G + self.n:]])
        ok = torch.isnan(bands) if self.guard != self.guard else bands == self.guard
        assert bool(ok.all()), f"{what}: wrote outside its range"

    def untouched(self, what):
        assert bool(torch.isnan(self.full).all()), f"{what}: a refused call wrote to its output"


def check(path, what, actual, ref, bound):
    ratio, idx, bad = P.worst(actual, ref, bound)
    log = os.environ.get("MSL_PW_RATIO_LOG")
    if log:
        with open(log, "a") as f:
            f.write(f"{path} {what} {ratio:.4f}\n")
    a, r = actual.detach().cpu().double().reshape(-1), ref.double().reshape(-1)
    assert bad == 0, (f"{path} {what}: {bad}/{r.numel()} elements over their bound; worst error / bound {ratio:.3f} at idx {idx} "
                      f"(got {a[idx].item():.9e}, ref {r[idx].item():.9e})")


def same_bits(a, b):
    """Bit identity of two fp32 / fp64 device tensors (NaN payloads and zero signs included)."""
    it = torch.int32 if a.dtype == torch.float32 else torch.int64
    return bool(torch.equal(a.contiguous().view(it), b.contiguous().view(it)))


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------- data, computed once per shape
def fwd_inputs(N, Cin, Cout, S):
    """Host inputs of one forward shape (cheap; the tests that need no float64 reference take only these)."""
    g = gen(100 + 31 * N + 7 * Cin + 3 * Cout + S)
    z = torch.randn((N, Cin, S), generator=g)
    w = torch.randn((Cout, Cin), generator=g) / Cin ** 0.5
    sc, sh = torch.randn(Cin, generator=g).abs() + 0.5, torch.randn(Cin, generator=g) * 0.3
    return dict(z=z, w=w, sc=sc, sh=sh)


@functools.lru_cache(maxsize=2)
def fwd_data(N, Cin, Cout, S):
    """Host data and the float64 reference of one forward shape: computed once, shared by the four forms, never modified.
    (Every shape is asked for by exactly one test, so the cache only has to span that test.)"""
    d = fwd_inputs(N, Cin, Cout, S)
    d["a32"] = P.act32(d["z"], d["sc"], d["sh"])
    d["y"], d["absdot"] = P.fwd_ref(d["a32"], d["w"])
    return d


def run_fwd(x, sc, sh, w, N, Cin, Cout, S, stats, expect=0, guard=NAN):
    """One msl_pwconv_fwd launch into guarded NaN buffers -> (y guarded, partials guarded or None, NP)."""
    L = _lib.load()
    NP = L.msl_pwconv_fwd_num_partials(N, Cin, Cout, S)
    y = Guarded(N * Cout * S, guard=guard)
    part = Guarded(2 * Cout * NP, dtype=torch.float64, guard=guard) if stats else None
    rc = L.msl_pwconv_fwd(ptr(x), ptr(sc), ptr(sh), ptr(w), ptr(y.v), ptr(part.v) if stats else None, N, Cin, Cout, S, st())
    torch.cuda.synchronize()
    assert rc == expect, f"msl_pwconv_fwd returned {rc}, expected {expect}"
    return y, part, NP


def check_stats(path, part, NP, y_gpu, d, N, Cin, Cout, S, J):
    """Every partial against the float64 sums of the kernel's own output over that partial's columns; the folded statistics
    against those of the float64 reference output under the sum of both bounds."""
    W = P.partial_width(N, S, NP)
    ref, bnd = P.stats_ref(y_gpu.cpu().view(N, Cout, S), W)
    got = part.v.view(2, Cout, NP).cpu()
    check(path, "partials", got, ref, bnd)
    tot, tb = P.stats_total_ref(d["y"], P.gemm_bound(d["absdot"], Cin, J))
    check(path, "folded-stats", R.exact_sum(got), tot, tb + bnd.sum(-1))


# ------------------------------------------------------------------------------------------------- msl_pwconv_fwd
@pytest.mark.parametrize("case", C.FWD_CASES, ids=[c[0] for c in C.FWD_CASES])
def test_pw_fwd_four_forms(case):
    """Affine + statistics, affine only, statistics only (on the host-activated input), neither: y is bit-identical across the
    four, the partials across the two that emit them; y and the partials are inside their bounds."""
    path, N, Cin, Cout, S, J = case
    d = fwd_data(N, Cin, Cout, S)
    zd, ad, wd, scd, shd = dev(d["z"]), dev(d["a32"]), dev(d["w"]), dev(d["sc"]), dev(d["sh"])
    affine_ok = Cin <= 512
    outs = {}
    for form, (x, aff, stats) in dict(affine_stats=(zd, True, True), affine=(zd, True, False), stats=(ad, False, True),
                                      plain=(ad, False, False)).items():
        if aff and not affine_ok:
            y, part, _ = run_fwd(x, scd, shd, wd, N, Cin, Cout, S, stats, expect=-2)
            y.untouched(f"{form}: y")
            if part is not None:
                part.untouched(f"{form}: partials")
            continue
        y, part, NP = run_fwd(x, scd if aff else None, shd if aff else None, wd, N, Cin, Cout, S, stats)
        y.intact(f"{form}: y")
        if part is not None:
            part.intact(f"{form}: partials")
        outs[form] = (y, part, NP)
    base = "affine_stats" if affine_ok else "stats"
    yb, pb, NP = outs[base]
    for form, (y, part, _) in outs.items():
        assert same_bits(y.v, yb.v), f"y of the {form} form differs from the {base} form"
        if part is not None:
            assert same_bits(part.v, pb.v), f"partials of the {form} form differ from the {base} form"
    check(path, "y", yb.v.view(N, Cout, S), d["y"], P.gemm_bound(d["absdot"], Cin, J))
    check_stats(path, pb, NP, yb.v, d, N, Cin, Cout, S, J)
    assert same_bits(zd, d["z"].to(DEV)) and same_bits(wd, d["w"].to(DEV)), "inputs changed"


@pytest.mark.parametrize("N,Cin,Cout,S,affine,rc", [(1, 544, 32, 64, True, -2), (1, 48, 32, 64, True, -1), (1, 32, 30, 64, True, -1),
                                                    (0, 32, 32, 64, True, -1), (1, 48, 32, 64, False, -1), (1, 32, 32, 0, True, -1)],
                         ids=["affine-Cin544", "Cin48", "Cout30", "N0", "Cin48-plain", "S0"])
def test_pw_fwd_refusals(N, Cin, Cout, S, affine, rc):
    """A refused call returns its code and leaves a NaN-filled output NaN."""
    L = _lib.load()
    n1, s1 = max(N, 1), max(S, 1)
    z, w = dev(torch.ones(n1 * Cin * s1)), dev(torch.ones(Cout * Cin))
    sc, sh = dev(torch.ones(Cin)), dev(torch.zeros(Cin))
    y, part = Guarded(n1 * Cout * s1), Guarded(2 * Cout * 64, dtype=torch.float64)
    got = L.msl_pwconv_fwd(ptr(z), ptr(sc) if affine else None, ptr(sh) if affine else None, ptr(w), ptr(y.v), ptr(part.v), N, Cin,
                           Cout, S, st())
    torch.cuda.synchronize()
    assert got == rc
    y.untouched("y")
    part.untouched("partials")
    if Cin == 544:  # the same shape without the affine is served
        y2, _, _ = run_fwd(z, None, None, w, N, Cin, Cout, S, False)
        assert bool((y2.v == 544.0).all())


# ------------------------------------------------------------------------------------------------- msl_pwconv_fwd_fold
def fold_partials(Cin, in_np, count, g, special=False):
    """Host-made fp64 (2, Cin, in_np) partials of plausible statistics (mean ~ N(0, 1), var ~ 1..3), unevenly split.
    ``special``: channel 0 gets q / count < mean^2 (the clamped variance)."""
    mean = torch.randn(Cin, generator=g, dtype=torch.float64)
    var = torch.rand(Cin, generator=g, dtype=torch.float64) * 2 + 1
    s, q = mean * count, (var + mean * mean) * count
    if special:
        q[0] = 0.5 * mean[0] * mean[0] * count
    wgt = torch.rand(in_np, generator=g, dtype=torch.float64) + 0.1
    wgt /= wgt.sum()
    return torch.stack([s[:, None] * wgt, q[:, None] * wgt]).contiguous()


def fold_inputs(N, Cin, Cout, S, in_np, count, special=False):
    g = gen(7000 + in_np + S)
    z = torch.randn((N, Cin, S), generator=g)
    w = torch.randn((Cout, Cin), generator=g) / Cin ** 0.5
    gamma, beta = torch.randn(Cin, generator=g).abs() + 0.5, torch.randn(Cin, generator=g) * 0.3
    return z, w, gamma, beta, fold_partials(Cin, in_np, count, g, special)


def run_fold_case(path, N, Cin, Cout, S, in_np, count, special=False, order=False):
    z, w, gamma, beta, parts = fold_inputs(N, Cin, Cout, S, in_np, count, special)
    if order:  # +-B in slots 0 and 32, B far above the other slots' reach in float64: every summation order has its own sum
        parts[0, :, 0] += 1e22
        parts[0, :, 32] -= 1e22
    pd, gd, bd, zd, wd = dev(parts), dev(gamma), dev(beta), dev(z), dev(w)
    vec = Guarded(4 * Cin)
    v = vec.v.view(4, Cin)
    _lib.call("msl_bn_finalize", ptr(pd), in_np, float(count), ptr(gd), ptr(bd), None, None, None, 0.1, EPS, ptr(v[0]), ptr(v[1]),
              ptr(v[2]), ptr(v[3]), Cin, st())
    y0, p0, NP = run_fwd(zd, v[0], v[1], wd, N, Cin, Cout, S, True)
    y1, p1 = Guarded(N * Cout * S), Guarded(2 * Cout * NP, dtype=torch.float64)
    _lib.call("msl_pwconv_fwd_fold", ptr(zd), ptr(pd), in_np, float(count), ptr(gd), ptr(bd), EPS, ptr(wd), ptr(y1.v), ptr(p1.v),
              N, Cin, Cout, S, st())
    torch.cuda.synchronize()
    y1.intact("fold: y")
    p1.intact("fold: partials")
    assert same_bits(y1.v, y0.v), "msl_pwconv_fwd_fold: y differs from msl_bn_finalize + msl_pwconv_fwd"
    assert same_bits(p1.v, p0.v), "msl_pwconv_fwd_fold: partials differ from msl_bn_finalize + msl_pwconv_fwd"
    y2 = Guarded(N * Cout * S)  # the fold without statistics
    _lib.call("msl_pwconv_fwd_fold", ptr(zd), ptr(pd), in_np, float(count), ptr(gd), ptr(bd), EPS, ptr(wd), ptr(y2.v), None,
              N, Cin, Cout, S, st())
    torch.cuda.synchronize()
    y2.intact("fold, no statistics: y")
    assert same_bits(y2.v, y0.v), "msl_pwconv_fwd_fold without statistics: y differs"
    if order:
        return y1, z, w, v
    ref = R.finalize_ref(R.exact_sum(parts[0]), R.exact_sum(parts[1]), count, gamma, beta, EPS, 0.1)
    for k, key in enumerate(("scale", "shift")):
        check(path, f"fold-{key}", v[k], ref[key], R.finalize_bound(ref, key))
    if special:
        assert float(ref["var"][0]) == 0.0
    return y1, z, w, v


@pytest.mark.parametrize("in_np", C.FOLD_NP)
@pytest.mark.parametrize("case", C.FOLD_CASES, ids=[c[0] for c in C.FOLD_CASES])
def test_pw_fwd_fold_is_finalize_plus_fwd(case, in_np):
    """The five kernels' bn_fold_block prologue (serial for NP <= 64, wave tree above): y and the output partials carry the
    bits of msl_bn_finalize on the same partials followed by msl_pwconv_fwd with its vectors."""
    path, N, Cin, Cout, S = case
    run_fold_case("fold:" + path, N, Cin, Cout, S, in_np, float(N * S))


@pytest.mark.parametrize("in_np,count,special", [(9, 1.0, False), (70, 1.0, False), (5, 4096.0, True), (130, 4096.0, True)],
                         ids=["count1-serial", "count1-wave", "clamped-var-serial", "clamped-var-wave"])
def test_pw_fwd_fold_edge_statistics(in_np, count, special):
    N, Cin, Cout, S = 2, 64, 96, 130
    y, z, w, v = run_fold_case("fold:edge", N, Cin, Cout, S, in_np, count, special)
    # the values too: the kernel's y against the float64 GEMM of the activation that the finalize kernel's vectors give
    yr, absdot = P.fwd_ref(P.act32(z, v[0].cpu(), v[1].cpu()), w)
    check("fold:edge", "y", y.v.view(N, Cout, S), yr, P.gemm_bound(absdot, Cin, 0))


@pytest.mark.parametrize("in_np", [64, 65])
def test_pw_fwd_fold_keeps_the_canonical_summation_order(in_np):
    """Partials whose float64 sum depends on the order of the additions (a cancelling pair of 1e22 among slots of ~1e2): the
    serial order (NP <= 64) and the wave tree (NP > 64) each give their own sum, so the fold only matches msl_bn_finalize bit
    for bit if it takes the same order on the same side of the switch.  (No comparison with the exact sum here: neither order
    is close to it.)"""
    N, Cin, Cout, S = 2, 64, 96, 130
    run_fold_case("fold:order", N, Cin, Cout, S, in_np, float(N * S), order=True)


def test_pw_fwd_fold_refusals():
    L = _lib.load()
    N, Cin, Cout, S = 1, 32, 32, 64
    z, w, gb = dev(torch.ones(N * Cin * S)), dev(torch.ones(Cout * Cin)), dev(torch.ones(Cin))
    parts = dev(torch.ones(2 * Cin * 4, dtype=torch.float64))
    y, part = Guarded(N * Cout * S), Guarded(2 * Cout * 4, dtype=torch.float64)
    for p, np_ in ((None, 4), (ptr(parts), 0), (ptr(parts), -1)):
        rc = L.msl_pwconv_fwd_fold(ptr(z), p, np_, 64.0, ptr(gb), ptr(gb), EPS, ptr(w), ptr(y.v), ptr(part.v), N, Cin, Cout, S, st())
        torch.cuda.synchronize()
        assert rc == -1
        y.untouched("y")
        part.untouched("partials")


# ------------------------------------------------------------------------------------------------- msl_pwconv_bwd_data
def bwd_data_inputs(N, Cin, Cout, S):
    g_ = gen(300 + 31 * N + 7 * Cin + 3 * Cout + S)
    dy = torch.randn((N, Cout, S), generator=g_)
    return dy, torch.randn((Cout, Cin), generator=g_) / Cin ** 0.5


@pytest.mark.parametrize("case", C.BWD_DATA_CASES, ids=[c[0] for c in C.BWD_DATA_CASES])
def test_pw_bwd_data(case):
    path, N, Cin, Cout, S, J = case
    dy, w = bwd_data_inputs(N, Cin, Cout, S)
    ref, absdot = P.bwd_data_ref(dy, w)
    out = Guarded(N * Cin * S)
    _lib.call("msl_pwconv_bwd_data", ptr(dev(dy)), ptr(dev(w)), ptr(out.v), N, Cin, Cout, S, st())
    torch.cuda.synchronize()
    out.intact("g_in")
    check(path, "g_in", out.v.view(N, Cin, S), ref, P.gemm_bound(absdot, Cout, J))


def test_pw_bwd_data_refusals():
    L = _lib.load()
    x = dev(torch.ones(4096))
    out = Guarded(4096)
    for N, Cin, Cout, S in ((0, 32, 32, 4), (1, 32, 48, 4), (1, 30, 32, 4), (1, 32, 32, 0)):
        assert L.msl_pwconv_bwd_data(ptr(x), ptr(x), ptr(out.v), N, Cin, Cout, S, st()) == -1
        torch.cuda.synchronize()
        out.untouched("g_in")


# ------------------------------------------------------------------------------------------------- weight gradient
def bww_data(N, Cin, Cout, S, seed=0):
    g_ = gen(500 + seed + 31 * N + 7 * Cin + 3 * Cout + S)
    dy = torch.randn((N, Cout, S), generator=g_)
    z = torch.randn((N, Cin, S), generator=g_)
    sc, sh = torch.randn(Cin, generator=g_).abs() + 0.5, torch.randn(Cin, generator=g_) * 0.3
    return dy, z, sc, sh


def run_bww(path, dy, x, sc, sh, ref, absdot, N, Cin, Cout, S):
    """slabs (twice), the stand-alone entry and the workspace query for one operand pair; ``sc`` None: no affine."""
    L = _lib.load()
    ns = L.msl_pwconv_bwd_weight_nslabs(N, Cin, Cout, S)
    assert ns >= 1
    assert L.msl_pwconv_bwd_weight_workspace_bytes(N, Cin, Cout, S) == ns * Cout * Cin * 4
    dyd, xd = dev(dy), dev(x)
    scp, shp = (ptr(dev(sc)), ptr(dev(sh))) if sc is not None else (None, None)
    bound = P.bww_bound(absdot, N, S, ns)
    slabs = [Guarded(ns * Cout * Cin) for _ in range(2)]
    for s in slabs:
        _lib.call("msl_pwconv_bwd_weight_slabs", ptr(dyd), ptr(xd), scp, shp, ptr(s.v), N, Cin, Cout, S, st())
    torch.cuda.synchronize()
    for s in slabs:
        s.intact("slabs")
    assert same_bits(slabs[0].v, slabs[1].v), "two runs of msl_pwconv_bwd_weight_slabs differ"
    check(path, "slab-sum", slabs[0].v.view(ns, Cout, Cin).double().sum(0), ref, bound)
    dw, ws = Guarded(Cout * Cin), Guarded(ns * Cout * Cin)
    _lib.call("msl_pwconv_bwd_weight", ptr(dyd), ptr(xd), scp, shp, ptr(dw.v), ptr(ws.v), N, Cin, Cout, S, st())
    torch.cuda.synchronize()
    dw.intact("dw")
    ws.intact("workspace")
    check(path, "dw", dw.v.view(Cout, Cin), ref, bound)
    if ns == 1:
        assert same_bits(dw.v, slabs[0].v), "nslabs == 1: the slab is not the stand-alone result"
        ws.untouched("workspace (nslabs == 1)")
    else:
        assert same_bits(ws.v, slabs[0].v), "the stand-alone entry's workspace does not hold the slabs"
    return ns


@pytest.mark.parametrize("case", C.BWW_CASES, ids=[c[0] for c in C.BWW_CASES])
def test_pw_bwd_weight(case):
    path, N, Cin, Cout, S = case
    L = _lib.load()
    dy, z, sc, sh = bww_data(N, Cin, Cout, S)
    a32 = P.act32(z, sc, sh)
    ref, absdot = P.bww_ref(dy, a32)
    run_bww(path, dy, z, sc, sh, ref, absdot, N, Cin, Cout, S)
    ref0, absdot0 = P.bww_ref(dy, z)
    run_bww(path + ":plain", dy, z, None, None, ref0, absdot0, N, Cin, Cout, S)
    wave = S % 32 == 0
    assert L.msl_pwconv_bwd_weight_batchable(N, Cin, Cout, S) == (1 if wave and Cout % 64 == 0 else 0)


def test_pw_bwd_weight_refusals():
    L = _lib.load()
    x = dev(torch.ones(8192))
    out = Guarded(8192)
    # Cout % 64 != 0 with S % 32 != 0: neither kernel takes it; then the argument checks
    for N, Cin, Cout, S in ((1, 32, 32, 33), (1, 32, 96, 65), (0, 32, 64, 32), (1, 48, 64, 32), (1, 32, 48, 32), (1, 32, 64, 0)):
        assert L.msl_pwconv_bwd_weight_slabs(ptr(x), ptr(x), ptr(x), ptr(x), ptr(out.v), N, Cin, Cout, S, st()) == -1
        torch.cuda.synchronize()
        out.untouched("slabs")
    assert L.msl_pwconv_bwd_weight_batchable(1, 32, 96, 96) == 0 and L.msl_pwconv_bwd_weight_batchable(1, 32, 64, 65) == 0
    assert L.msl_pwconv_bwd_weight_batchable(0, 32, 64, 64) == 0


@pytest.mark.parametrize("shapes", [[(32, 64, 1312)], [(32, 64, 224), (128, 128, 96), (64, 64, 1312)]], ids=["batch1", "batch3-unequal-S"])
def test_pw_bwd_weight_batch_is_the_single_launches(shapes):
    """msl_pwconv_bwd_weight_slabs_batch writes exactly the slabs of the per-layer launches (and nothing around them)."""
    L = _lib.load()
    N, n = 3, len(shapes)
    rows, single = [], []
    for q, (Cin, Cout, S) in enumerate(shapes):
        assert L.msl_pwconv_bwd_weight_batchable(N, Cin, Cout, S) == 1
        dy, z, sc, sh = (dev(t) for t in bww_data(N, Cin, Cout, S, seed=q))
        ns = L.msl_pwconv_bwd_weight_nslabs(N, Cin, Cout, S)
        ref, out = Guarded(ns * Cout * Cin), Guarded(ns * Cout * Cin)
        _lib.call("msl_pwconv_bwd_weight_slabs", ptr(dy), ptr(z), ptr(sc), ptr(sh), ptr(ref.v), N, Cin, Cout, S, st())
        rows.append((dy, z, sc, sh, out.v, Cin, Cout, S))
        single.append((ref, out))
    Pp, I = ctypes.c_void_p * n, ctypes.c_int * n
    arrs = [Pp(*[ptr(r[c]) for r in rows]) for c in range(5)] + [I(*[r[c] for r in rows]) for c in range(5, 8)]
    _lib.call("msl_pwconv_bwd_weight_slabs_batch", *[ctypes.addressof(a) for a in arrs], n, N, st())
    torch.cuda.synchronize()
    for q, (ref, out) in enumerate(single):
        out.intact(f"layer {q}")
        assert same_bits(out.v, ref.v), f"layer {q} of a batch of {n}"


# ------------------------------------------------------------------------------------------------- msl_pwconv_bwd_fused
def fused_inputs():
    """Host operands of FUSED_CASE -> (gy, y, z, w, vy, vz, y partials (2, Cout, ynp) fp64, ynp, count)."""
    N, Cin, Cout, S = C.FUSED_CASE
    g_ = gen(900)
    gy = torch.randn((N, Cout, S), generator=g_)
    y = torch.randn((N, Cout, S), generator=g_) * 1.5 + 0.3
    z = torch.randn((N, Cin, S), generator=g_) * 2.0 + 0.5
    w = torch.randn((Cout, Cin), generator=g_) * 0.2
    gam_y, bet_y = torch.rand(Cout, generator=g_) + 0.5, torch.randn(Cout, generator=g_) * 0.3
    gam_z, bet_z = torch.rand(Cin, generator=g_) + 0.5, torch.randn(Cin, generator=g_) * 0.3
    y, _ = R.separate_preactivation(y, gam_y, bet_y, EPS)
    z, _ = R.separate_preactivation(z, gam_z, bet_z, EPS)
    vy, vz = R.host_vectors(y, gam_y, bet_y, EPS), R.host_vectors(z, gam_z, bet_z, EPS)
    dbeta, dgamma = R.bwd_sums_ref(gy, y, vy)
    ynp = 5
    wgt = torch.rand(ynp, generator=g_, dtype=torch.float64) + 0.1
    wgt /= wgt.sum()
    parts = torch.stack([dbeta[:, None] * wgt, dgamma[:, None] * wgt]).contiguous()
    return gy, y, z, w, vy, vz, parts, ynp, float(N * S)


def test_pw_bwd_fused_uneven_strips():
    """513 strips over 256 workgroups (workgroup 0 walks three, the others two; strips cross images), against the float64
    evaluation of the launches it replaces: BatchNorm2 backward applied on load (bn_ref.coef_ref), g_z = W^T dL/dy, the
    BatchNorm1-backward sums of z from the kernel's own g_z, and the weight-gradient slabs.  Then against those launches
    themselves on the same operands (msl_bn_relu_bwd_finalize_apply, msl_pwconv_bwd_data, msl_pwconv_bwd_weight_slabs,
    msl_bn_relu_bwd_reduce), under the sum of the two paths' bounds.  y and z are moved away from a zero pre-activation
    (bn_ref.separate_preactivation: |a| >= 1e-3, a thousand times what any fp32 evaluation order of y * scale + shift
    can move it by), so every kernel and the float64 reference take the same ReLU mask."""
    L = _lib.load()
    N, Cin, Cout, S = C.FUSED_CASE
    NPW = L.msl_pwconv_bwd_fused_num_partials(N, Cin, Cout, S)
    assert NPW == 256
    gy, y, z, w, vy, vz, parts, ynp, count = fused_inputs()
    gz, zpart, slabs = Guarded(N * Cin * S), Guarded(2 * Cin * NPW, dtype=torch.float64), Guarded(NPW * Cout * Cin)
    dgam, dbet = Guarded(Cout), Guarded(Cout)
    gyd, yd_, vyd, pd, wd, zd_, vzd = dev(gy), dev(y), dev(vy), dev(parts), dev(w), dev(z), dev(vz)
    args = (ptr(gyd), ptr(yd_), ptr(vyd), ptr(pd), ynp, count, ptr(dgam.v), ptr(dbet.v), ptr(wd), ptr(zd_), ptr(vzd))
    _lib.call("msl_pwconv_bwd_fused", *args, ptr(gz.v), ptr(zpart.v), ptr(slabs.v), N, Cin, Cout, S, st())
    torch.cuda.synchronize()
    for o, what in ((gz, "g_z"), (zpart, "z partials"), (slabs, "slabs"), (dgam, "dgamma"), (dbet, "dbeta")):
        o.intact(what)
    path = "fused<64,32,128>"
    # dgamma / dbeta of bn2: the float64 sum of the partials, rounded once
    fr = R.bwd_finalize_ref(parts, count)
    check(path, "dbeta_y", dbet.v, fr["dbeta"], R.bwd_finalize_bound(fr, "dbeta"))
    check(path, "dgamma_y", dgam.v, fr["dgamma"], R.bwd_finalize_bound(fr, "dgamma"))
    # dL/dy = fma(scale, gm, fma(cC, y, cE)) with the kernel's fp32 (cC, cE): two roundings -> 4 U of the terms' magnitudes,
    # plus what the coefficients' own roundings (bn_ref.coef_bound) move it by
    cC, cE = R.coef_ref(fr["dbeta"], fr["dgamma"], count, vy)
    bC, bE = R.coef_bound(fr["dbeta"], fr["dgamma"], count, vy)
    b3 = lambda v: v.double().view(1, -1, 1)
    yd = y.double()
    gm = torch.where(yd * b3(vy[0]) + b3(vy[1]) > 0, gy.double(), torch.zeros((), dtype=torch.float64))
    dy = b3(vy[0]) * gm + (b3(cC) * yd + b3(cE))
    dyb = 4 * R.U * ((b3(vy[0]) * gm).abs() + (b3(cC) * yd).abs() + b3(cE).abs()) + yd.abs() * b3(bC) + b3(bE)
    # g_z: a 64-term chain on the kernel's dL/dy
    wt_abs = w.double().abs().t()
    ref, absdot = P.bwd_data_ref(dy, w)
    check(path, "g_z", gz.v.view(N, Cin, S), ref, P.gemm_bound(absdot, Cout, 0) + torch.matmul(wt_abs, dyb))
    # BatchNorm1-backward sums of z, per workgroup, from the kernel's own g_z: workgroup b walks strips b, b + 256, b + 512.
    # fp32 roundings of a term: 3 additions of a lane (one per strip) + the 5-level DPP tree + (z - mean) * invstd (2) + the fma (1)
    gzc, zd = gz.v.view(N, Cin, S).cpu(), z.double()
    t1, t2 = R.bwd_terms_ref(gzc, z, vz)
    strips = N * (S // 128)
    per_wg = (strips + NPW - 1) // NPW
    def slot(t):
        s_ = t.view(N, Cin, S // 128, 128).sum(-1).permute(1, 0, 2).reshape(Cin, strips)
        s_ = torch.nn.functional.pad(s_, (0, per_wg * NPW - strips)).view(Cin, per_wg, NPW)
        return s_.sum(1)
    zref = torch.stack([slot(t1), slot(t2)])
    zbnd = (per_wg + 5 + 3 + 1) * R.U * torch.stack([slot(t1.abs()), slot(t2.abs())])
    check(path, "z-partials", zpart.v.view(2, Cin, NPW), zref, zbnd)
    # weight gradient: the float64 sum of the 256 slabs; a slab contracts per_wg strips of 128 positions (two column parts
    # of 64 met by one addition), and dL/dy carries its own bound
    a32 = P.act32(z, vz[0], vz[1])
    dwr, dwa = P.bww_ref(dy, a32)
    extra = torch.matmul(dyb, a32.double().abs().transpose(1, 2)).sum(0)
    dw_bound = (per_wg * 128 + 2) * R.U * dwa + extra
    dw_fused = slabs.v.view(NPW, Cout, Cin).double().sum(0).cpu()
    check(path, "slab-sum", dw_fused, dwr, dw_bound)
    # ---- the separate launches on the same operands, each within its own bound of the same float64 values: the two GPU paths
    # may differ by the sum of the bounds
    vec6 = dev(torch.cat([vy, torch.zeros(2, Cout)]))  # rows 4-5 (c1, c2) are written by the launch
    dy_s, dgam_s, dbet_s = Guarded(N * Cout * S), Guarded(Cout), Guarded(Cout)
    _lib.call("msl_bn_relu_bwd_finalize_apply", ptr(pd), ynp, count, ptr(gyd), ptr(yd_), ptr(vec6), ptr(dgam_s.v), ptr(dbet_s.v),
              ptr(dy_s.v), N, Cout, S, st())
    gz_s = Guarded(N * Cin * S)
    _lib.call("msl_pwconv_bwd_data", ptr(dy_s.v), ptr(wd), ptr(gz_s.v), N, Cin, Cout, S, st())
    ns = L.msl_pwconv_bwd_weight_nslabs(N, Cin, Cout, S)
    slabs_s = Guarded(ns * Cout * Cin)
    _lib.call("msl_pwconv_bwd_weight_slabs", ptr(dy_s.v), ptr(zd_), ptr(vzd[0]), ptr(vzd[1]), ptr(slabs_s.v), N, Cin, Cout, S, st())
    NPR = L.msl_bn_relu_bwd_num_partials(N, S)
    zpart_s = Guarded(2 * Cin * NPR, dtype=torch.float64)
    _lib.call("msl_bn_relu_bwd_reduce", ptr(gz.v), ptr(zd_), ptr(vzd[0]), ptr(vzd[1]), ptr(vzd[2]), ptr(vzd[3]), ptr(zpart_s.v),
              N, Cin, S, st())
    torch.cuda.synchronize()
    for o, what in ((dy_s, "dy"), (dgam_s, "dgamma"), (dbet_s, "dbeta"), (gz_s, "g_z"), (slabs_s, "slabs"), (zpart_s, "z partials")):
        o.intact("separate " + what)
    sep = "fused-vs-separate"
    check(sep, "dbeta_y", dbet.v, dbet_s.v.cpu().double(), 2 * R.bwd_finalize_bound(fr, "dbeta"))
    check(sep, "dgamma_y", dgam.v, dgam_s.v.cpu().double(), 2 * R.bwd_finalize_bound(fr, "dgamma"))
    # the separate dL/dy = scale (gm - c1 - xhat c2) with the launch's own fp32 c1, c2 (the float64 quotient cast: 2 U), stored
    dys_b = R.bwd_apply_bound(gy, y, vy, fr["c1"], fr["c2"], 2 * R.U * fr["c1"].abs(), 2 * R.U * fr["c2"].abs())
    check("separate", "dy", dy_s.v.view(N, Cout, S), R.bwd_apply_ref(gy, y, vy, fr["c1"], fr["c2"]), dys_b)
    gz_bound_s = P.gemm_bound(absdot, Cout, 0) + torch.matmul(wt_abs, dys_b)  # strip<64,128,1>T: a serial 64-term chain
    check(sep, "g_z", gz.v.view(N, Cin, S), gz_s.v.view(N, Cin, S).cpu().double(),
          P.gemm_bound(absdot, Cout, 0) + torch.matmul(wt_abs, dyb) + gz_bound_s)
    extra_s = torch.matmul(dys_b, a32.double().abs().transpose(1, 2)).sum(0)
    check(sep, "slab-sum", dw_fused, slabs_s.v.view(ns, Cout, Cin).double().sum(0).cpu(),
          dw_bound + P.bww_bound(dwa, N, S, ns) + extra_s)
    # the z sums of the kernel's own g_z: 16 terms per thread and chunk in msl_bn_relu_bwd_reduce (tests/test_gpu_bn.py)
    zb_s = torch.stack(R.bwd_sums_bound(gzc, z, vz, 16))
    check(sep, "z-sums", R.exact_sum(zpart.v.view(2, Cin, NPW).cpu()), R.exact_sum(zpart_s.v.view(2, Cin, NPR).cpu()),
          zbnd.sum(-1) + zb_s)
    # run-to-run bit-identical
    gz2, zpart2, slabs2 = Guarded(N * Cin * S), Guarded(2 * Cin * NPW, dtype=torch.float64), Guarded(NPW * Cout * Cin)
    _lib.call("msl_pwconv_bwd_fused", *args, ptr(gz2.v), ptr(zpart2.v), ptr(slabs2.v), N, Cin, Cout, S, st())
    torch.cuda.synchronize()
    assert same_bits(gz.v, gz2.v) and same_bits(zpart.v, zpart2.v) and same_bits(slabs.v, slabs2.v)


@pytest.mark.parametrize("N,Cin,Cout,S", [(1, 32, 64, 65408), (4, 32, 64, 16448), (2, 64, 128, 32768), (2, 64, 32, 32768), (0, 32, 64, 65536)],
                         ids=["511-strips", "S%128", "64x128", "64x32", "N0"])
def test_pw_bwd_fused_refusals(N, Cin, Cout, S):
    L = _lib.load()
    assert L.msl_pwconv_bwd_fused_num_partials(N, Cin, Cout, S) == 0
    x, xd = dev(torch.ones(1024)), dev(torch.ones(1024, dtype=torch.float64))
    outs = [Guarded(1024), Guarded(1024, dtype=torch.float64), Guarded(1024), Guarded(64), Guarded(64)]
    rc = L.msl_pwconv_bwd_fused(ptr(x), ptr(x), ptr(x), ptr(xd), 4, 64.0, ptr(outs[3].v), ptr(outs[4].v), ptr(x), ptr(x), ptr(x),
                                ptr(outs[0].v), ptr(outs[1].v), ptr(outs[2].v), N, Cin, Cout, S, st())
    torch.cuda.synchronize()
    assert rc == -2
    for o in outs:
        o.untouched("a refused msl_pwconv_bwd_fused")


# ------------------------------------------------------------------------------------------------- ill-conditioned and special values
def cancelling(rows, depth, cols, g_):
    """(w (rows, depth), a (depth, cols)): neighbouring k terms cancel - w = +-4096 r + e on a pair that shares its a - so the result
    is sum e a while absdot is 2^13 times larger: the error must track absdot, not |result|."""
    r = torch.randn((rows, depth // 2), generator=g_).repeat_interleave(2, dim=1)
    sign = torch.tensor([1.0, -1.0]).repeat(depth // 2)
    w = r * sign * 4096.0 + torch.randn((rows, depth), generator=g_)
    a = torch.randn((depth // 2, cols), generator=g_).abs().repeat_interleave(2, dim=0)
    return w, a


@pytest.mark.parametrize("path,N,Cin,Cout,S,J", [("illcond:wave<64,2>", 2, 64, 64, 130, 0), ("illcond:wave-split4", 1, 256, 32, 95, 4),
                                                 ("illcond:gemm-scalar", 1, 96, 160, 131, 0)], ids=lambda v: v if isinstance(v, str) else None)
def test_pw_fwd_ill_conditioned(path, N, Cin, Cout, S, J):
    """Alternating +- terms at 2^12 times the result.  A tolerance relative to |y| (the old tests' 1e-5) is meaningless here:
    an honest kernel misses it by orders of magnitude, and the bound that an honest kernel does meet is (K + J) U absdot."""
    g_ = gen(1200 + Cin)
    w, a = cancelling(Cout, Cin, N * S, g_)
    a32 = a.view(Cin, N, S).permute(1, 0, 2).contiguous()
    ref, absdot = P.fwd_ref(a32, w)
    assert float(absdot.median() / ref.abs().median()) > 2.0 ** 10
    y, part, NP = run_fwd(dev(a32), None, None, dev(w), N, Cin, Cout, S, True)
    y.intact("y")
    part.intact("partials")
    check(path, "y", y.v.view(N, Cout, S), ref, P.gemm_bound(absdot, Cin, J))
    ref_p, bnd_p = P.stats_ref(y.v.cpu().view(N, Cout, S), P.partial_width(N, S, NP))
    check(path, "partials", part.v.view(2, Cout, NP), ref_p, bnd_p)


@pytest.mark.parametrize("path,N,Cin,Cout,S", [("illcond:bww-wave<2>", 2, 32, 64, 672), ("illcond:bww-fallback<64>", 1, 64, 64, 130)],
                         ids=lambda v: v if isinstance(v, str) else None)
def test_pw_bwd_weight_ill_conditioned(path, N, Cin, Cout, S):
    """Neighbouring positions cancel at 2^12 times the result."""
    g_ = gen(1300 + S)
    P2 = N * S
    dyf, af = cancelling(Cout, P2, Cin, g_)  # dy (Cout, positions), a (positions, Cin)
    dy = dyf.view(Cout, N, S).permute(1, 0, 2).contiguous()
    a = af.t().contiguous().view(Cin, N, S).permute(1, 0, 2).contiguous()
    ref, absdot = P.bww_ref(dy, a)
    assert float(absdot.median() / ref.abs().median()) > 2.0 ** 8
    run_bww(path, dy, a, None, None, ref, absdot, N, Cin, Cout, S)


def test_pw_fwd_signed_zeros_through_the_relu():
    """Pre-activations that are exactly +0 and -0 (msl::act passes -0: ``-0 < 0`` is false), raw +-0 inputs and a zero scale
    with a -0 shift: the four forms still agree bit for bit (pw_ref.act32 keeps the kernel's zero signs) and y is in bound."""
    N, Cin, Cout, S = 2, 64, 64, 130
    d = fwd_inputs(N, Cin, Cout, S)
    z, sc, sh = d["z"].clone(), d["sc"].clone(), d["sh"].clone()
    z[:, :, ::3] = 0.0
    z[:, :, 1::6] = -0.0
    sh[::2] = -0.0   # fmaf(-0, s, -0) = -0, fmaf(+0, s, -0) = +0
    sh[1] = 0.0
    sc[5], sh[5] = 0.0, -0.0  # fmaf(z, 0, -0): -0 for z > 0 ... the sign of z * 0
    a32 = P.act32(z, sc, sh)
    assert bool((torch.signbit(a32) & (a32 == 0)).any()) and bool((~torch.signbit(a32) & (a32 == 0)).any())
    ref, absdot = P.fwd_ref(a32, d["w"])
    wd = dev(d["w"])
    ya, pa, NP = run_fwd(dev(z), dev(sc), dev(sh), wd, N, Cin, Cout, S, True)
    yp, pp, _ = run_fwd(dev(a32), None, None, wd, N, Cin, Cout, S, True)
    assert same_bits(ya.v, yp.v) and same_bits(pa.v, pp.v)
    check("signed-zeros", "y", ya.v.view(N, Cout, S), ref, P.gemm_bound(absdot, Cin, 0))
    # an all-zero input with signed zeros gives +0 everywhere (the accumulators start at +0), statistics included
    z0 = torch.zeros((N, Cin, S))
    z0[:, ::2] = -0.0
    y0, p0, _ = run_fwd(dev(z0), None, None, wd, N, Cin, Cout, S, True)
    assert same_bits(y0.v, torch.zeros_like(y0.v)) and same_bits(p0.v, torch.zeros_like(p0.v))


NAN_CASES = [("strip<64,64,4>", 2, 64, 128, 4096, (1, 37, 4095)), ("wave<32,2>", 2, 32, 64, 130, (0, 31, 129)),
             ("wave-NT2<32,2>", 2, 32, 256, 16404, (1, 0, 16403)), ("wave-split4", 3, 256, 32, 95, (2, 200, 64)),
             ("gemm-scalar", 2, 96, 160, 131, (1, 95, 128)), ("ksplit4-K128", 1, 128, 36, 70, (0, 127, 69))]


@pytest.mark.parametrize("case", NAN_CASES, ids=[c[0] for c in NAN_CASES])
def test_pw_fwd_one_nan_poisons_its_column_only(case):
    """One NaN input element: exactly its column of y (every row, that image) and the two statistics of every row of the
    partial that holds the column are NaN; every other value keeps the bits of the clean run."""
    path, N, Cin, Cout, S, (n0, k0, s0) = case
    d = fwd_inputs(N, Cin, Cout, S)
    wd, scd, shd = dev(d["w"]), dev(d["sc"]), dev(d["sh"])
    y0, p0, NP = run_fwd(dev(d["z"]), scd, shd, wd, N, Cin, Cout, S, True)
    z = d["z"].clone()
    z[n0, k0, s0] = NAN
    y1, p1, _ = run_fwd(dev(z), scd, shd, wd, N, Cin, Cout, S, True, guard=-12345.0)  # finite bands: a stray NaN shows
    y1.intact("y")
    p1.intact("partials")
    ynan = torch.isnan(y1.v.view(N, Cout, S))
    want = torch.zeros_like(ynan)
    want[n0, :, s0] = True
    assert torch.equal(ynan, want), f"{int(ynan.sum())} NaNs in y, expected the {Cout} of one column"
    keep = ~want
    assert same_bits(y1.v.view(N, Cout, S)[keep], y0.v.view(N, Cout, S)[keep])
    W = P.partial_width(N, S, NP)
    slot = n0 * (NP // N) + s0 // W
    pnan = torch.isnan(p1.v.view(2, Cout, NP))
    wantp = torch.zeros_like(pnan)
    wantp[:, :, slot] = True
    assert torch.equal(pnan, wantp), f"{int(pnan.sum())} NaN statistics, expected the {2 * Cout} of partial {slot}"
    assert same_bits(p1.v.view(2, Cout, NP)[~wantp], p0.v.view(2, Cout, NP)[~wantp])


# ------------------------------------------------------------------------------------------------- recorded bits
def test_pw_bits_are_the_recorded_ones():
    """Every output buffer of every case of tests/pw_cases.py has the SHA-256 that tests/golden/pw_bits.json recorded before the
    host code got its single route (make_pw_bits's docstring): a mismatch means a launch changed its kernel, its grid or its
    bits, never that the file wants minting again."""
    import json
    from tests.golden import make_pw_bits as M
    with open(M.OUT) as f:
        want = json.load(f)["fp32"]
    got = M.digests_fp32(DEV)
    assert sorted(got) == sorted(want), "the cases are not the recorded ones"
    assert {k.split()[0] for k in want} == {"msl_pwconv_fwd", "msl_pwconv_fwd_fold", "msl_pwconv_bwd_data", "msl_pwconv_bwd_weight",
                                            "msl_pwconv_bwd_weight_slabs_batch", "msl_pwconv_bwd_fused"}
    bad = [k for k in want if got[k] != want[k]]
    assert not bad, f"{len(bad)}/{len(want)} buffers differ from the recorded bits: {bad[:8]}"
