"""Every fp32 BatchNorm entry point of csrc/bn.hip, path by path, against the stage-wise float64 reference of
tests/bn_ref.py (bounds derived there, not tuned; each failure message prints the worst error / bound).

The stage-wise tests make the (scale, shift, mean, invstd) vectors on the host and hand the same fp32 vectors to the
kernel and to the reference, so the reference's ReLU mask is the kernel's (bn_ref's docstring): no element is excluded
anywhere.  Every output buffer sits between guard bands that must come back untouched.  Each case's comment names the
kernel path it reaches.  With MSL_BN_RATIO_LOG=<file> every comparison appends "<entry point> <what> <error / bound>" to
that file (how the table in DESIGN.md, Appendix A, was measured)."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

from mslesions3d_amd import _lib
from mslesions3d_amd._lib import ptr
from tests import bn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS, MOM = 1e-5, 0.1
G = 64  # guard elements on each side of every output (a multiple of 4: the views stay 16-byte aligned)


def st():
    return torch.cuda.current_stream().cuda_stream


_KEEP = []


def K(t):
    """Move to the GPU and keep the tensor alive until the end of the test (a temporary passed as
    ``ptr(K(x))`` would be freed - and its block re-used - before the kernel runs)."""
    d = t.detach().to(DEV).contiguous()
    _KEEP.append(d)
    return d


@pytest.fixture(autouse=True)
def _release_kept():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


class Guarded:
    """An output buffer of n elements between two bands of G guard elements (NaN, or ``fill`` for integers / sentinels)."""

    def __init__(self, n, dtype=torch.float32, fill=float("nan"), init=None):
        self.n, self.fill = n, fill
        self.full = torch.full((n + 2 * G,), fill, dtype=dtype, device=DEV)
        self.v = self.full[G:G + n]
        if init is not None:
            self.v.copy_(init.reshape(-1))
        _KEEP.append(self.full)

    def intact(self, what):
        torch.cuda.synchronize()
        band = torch.cat([self.full[:G], self.full[G + self.n:]]).cpu()
        ok = torch.isnan(band).all() if self.fill != self.fill else (band == self.fill).all()
        assert bool(ok), f"{what}: wrote outside its range"


def check(entry, what, actual, ref, bound):
    ratio, idx, bad = R.worst(actual, ref, bound)
    log = os.environ.get("MSL_BN_RATIO_LOG")
    if log:
        with open(log, "a") as f:
            f.write(f"{entry} {what} {ratio:.4f}\n")
    a, r = actual.detach().cpu().double().reshape(-1), ref.double().reshape(-1)
    assert bad == 0, (f"{entry} {what}: {bad}/{r.numel()} elements over their bound; worst error / bound {ratio:.3f} at idx {idx} "
                      f"(got {a[idx].item():.9e}, ref {r[idx].item():.9e})")


def gen(seed):
    return torch.Generator().manual_seed(seed)


def bwd_case(N, C, S, seed, mean=1.0, std=2.0):
    """fp32 (g, y) of shape (N, C, S), and the host-made fp32 vector block (4, C) of y's batch statistics."""
    g_ = gen(seed)
    y = torch.randn((N, C, S), generator=g_) * std + mean
    g = torch.randn((N, C, S), generator=g_)
    gamma, beta = torch.randn(C, generator=g_).abs() + 0.5, torch.randn(C, generator=g_) * 0.2
    return g, y, R.host_vectors(y, gamma, beta, EPS)


def split_partials(s, q, NP, g_):
    """(2, C, NP) fp64: the sums s, q (C,) split unevenly over NP slots (the slots of a channel add up to its sum up to
    float64 rounding; the reference re-adds them exactly)."""
    w = torch.rand(NP, generator=g_, dtype=torch.float64) + 0.1
    w /= w.sum()
    return torch.stack([s.double()[:, None] * w, q.double()[:, None] * w]).contiguous()


def stat_sums(y):
    yd = y.double()
    d = (0,) + tuple(range(2, y.dim()))
    return yd.sum(d), (yd * yd).sum(d), y.numel() // y.shape[1]


# ------------------------------------------------------------------------------------------------- msl_bn_relu_bwd_fused
def fused_nt(N, S):
    """fp32 additions of one thread, read off bn.hip: the dispatcher of msl_bn_relu_bwd_fused and its kernels' indexing."""
    total4 = N * (S // 4)
    if S % 4 == 0 and total4 <= 4096:
        return 4 * (1 if total4 <= 256 else 2 if total4 <= 2048 else 4)  # bn_relu_bwd_fused_reg_kernel<NT, IPT>
    if S % 4 == 0:
        return 4 * N * ((S + 1023) // 1024)  # generic kernel, float4 loop: i = 4 tid, step 1024, every n
    return N * ((S + 255) // 256)            # generic kernel, scalar loop


FUSED_CASES = [  # (N, S): total4 = N * S / 4 against the dispatcher thresholds 64, 256, 512, 1024, 2048, 4096
    (1, 4),       # total4 1: <64,1>, one live lane
    (1, 256),     # total4 64: <64,1> full
    (1, 260),     # total4 65: <256,1>, first past 64
    (2, 512),     # total4 256: <256,1> full, two samples
    (1, 1028),    # total4 257: <256,2>, second pass one lane
    (4, 512),     # total4 512: <256,2> full
    (1, 2052),    # total4 513: <512,2>
    (4, 1024),    # total4 1024: <512,2> full
    (1, 4100),    # total4 1025: <1024,2>
    (2, 4096),    # total4 2048: <1024,2> full
    (3, 2732),    # total4 2049: <1024,4>, sample boundary inside a thread's stride
    (4, 4096),    # total4 4096: <1024,4> full
    (1, 16388),   # total4 4097: generic kernel, float4 loop with a tail
    (4, 16384),   # total4 16384: generic kernel at the engine's limit N * S = 65536
    (3, 105),     # S % 4 != 0: generic kernel, scalar loop, S < 256
    (2, 4099),    # scalar loop with a tail
    (1, 65535),   # scalar loop at the limit
]


@pytest.mark.parametrize("inplace", [False, True], ids=["out", "inplace"])
@pytest.mark.parametrize("C", [1, 5])
@pytest.mark.parametrize("N,S", FUSED_CASES)
def test_bn_relu_bwd_fused(N, S, C, inplace):
    g, y, vec = bwd_case(N, C, S, seed=1000 + N * 7 + S)
    count = float(N * S)
    vd, yd = K(vec), K(y)
    dgam, dbet = Guarded(C), Guarded(C)
    if inplace:  # dy == g, as the engine calls it
        dy = Guarded(N * C * S, init=g)
        gp = ptr(dy.v)
    else:
        dy = Guarded(N * C * S)
        gd = K(g)
        gp = ptr(gd)
    _lib.call("msl_bn_relu_bwd_fused", gp, ptr(yd), ptr(vd[0]), ptr(vd[1]), ptr(vd[2]), ptr(vd[3]), ptr(dgam.v), ptr(dbet.v),
              ptr(dy.v), N, C, S, st())
    for o, w in ((dgam, "dgamma"), (dbet, "dbeta"), (dy, "dy")):
        o.intact(w)
    nt = fused_nt(N, S)
    dbeta, dgamma = R.bwd_sums_ref(g, y, vec)
    b_db, b_dg = R.bwd_sums_bound(g, y, vec, nt)
    check("msl_bn_relu_bwd_fused", "dbeta", dbet.v, dbeta, b_db)
    check("msl_bn_relu_bwd_fused", "dgamma", dgam.v, dgamma, b_dg)
    c1, c2 = dbeta / count, dgamma / count
    # the kernel's own c1 / c2: its sums over count, cast to fp32
    bound = R.bwd_apply_bound(g, y, vec, c1, c2, b_db / count + R.U * c1.abs(), b_dg / count + R.U * c2.abs())
    check("msl_bn_relu_bwd_fused", "dy", dy.v.view(N, C, S), R.bwd_apply_ref(g, y, vec, c1, c2), bound)
    if not inplace:
        assert torch.equal(gd.cpu(), g) and torch.equal(yd.cpu(), y), "inputs changed"


# ------------------------------------------------------------------ msl_bn_relu_bwd_reduce / _bwd_finalize / _bwd_apply / _finalize_apply
CHUNK = 4096

BWD_S = [
    1,        # scalar branch, one live thread
    105,      # scalar branch, S < 256
    4096,     # vector branch, exactly one chunk, no masked load
    4100,     # vector branch, second chunk holds one float4: clamped + masked loads
    8192,     # two full chunks
    12289,    # scalar branch, four chunks, the last holds one element
    70001,    # scalar branch; apply's grid-stride loop (S > 64 * 256)
    262144,   # 64^3, block 1: 64 chunks (NP = 256 at N = 4); apply's vector grid-stride loop (S > 64 * 1024)
]


@pytest.mark.parametrize("N", [1, 4])
@pytest.mark.parametrize("S", BWD_S)
def test_bn_relu_bwd_reduce_finalize_apply(N, S):
    L = _lib.load()
    C = 2
    g, y, vec = bwd_case(N, C, S, seed=2000 + N * 3 + S)
    count = float(N * S)
    chunks = (S + CHUNK - 1) // CHUNK
    NP = L.msl_bn_relu_bwd_num_partials(N, S)
    assert NP == N * chunks
    vd, gd, yd = K(vec), K(g), K(y)
    part = Guarded(2 * C * NP, dtype=torch.float64)
    _lib.call("msl_bn_relu_bwd_reduce", ptr(gd), ptr(yd), ptr(vd[0]), ptr(vd[1]), ptr(vd[2]), ptr(vd[3]), ptr(part.v), N, C, S, st())
    part.intact("partials")
    # every partial on its own: slot p = n * chunks + chunk holds the sums over that chunk of that sample
    t1, t2 = R.bwd_terms_ref(g, y, vec)
    pad = chunks * CHUNK - S
    per = lambda t: F.pad(t, (0, pad)).view(N, C, chunks, CHUNK)
    slot = lambda t: t.sum(-1).permute(1, 0, 2).reshape(C, NP)
    ref_p = torch.stack([slot(per(t1)), slot(per(t2))])
    bnd_p = (16 + 4) * R.U * torch.stack([slot(per(t1).abs()), slot(per(t2).abs())])  # 16 terms per thread and chunk
    got_p = part.v.view(2, C, NP)
    check("msl_bn_relu_bwd_reduce", "partials", got_p, ref_p, bnd_p)
    # finalize: against the device's own partials (2 U), and against the sums of the data
    outs = {k: Guarded(C) for k in ("dgamma", "dbeta", "c1", "c2")}
    _lib.call("msl_bn_bwd_finalize", ptr(part.v), NP, count, ptr(outs["dgamma"].v), ptr(outs["dbeta"].v), ptr(outs["c1"].v),
              ptr(outs["c2"].v), C, st())
    fr = R.bwd_finalize_ref(got_p.cpu(), count)
    for k, o in outs.items():
        o.intact(k)
        check("msl_bn_bwd_finalize", k, o.v, fr[k], R.bwd_finalize_bound(fr, k))
    dbeta, dgamma = R.bwd_sums_ref(g, y, vec)
    b_db, b_dg = R.bwd_sums_bound(g, y, vec, 16)
    check("msl_bn_relu_bwd_reduce", "dbeta", outs["dbeta"].v, dbeta, b_db)
    check("msl_bn_relu_bwd_reduce", "dgamma", outs["dgamma"].v, dgamma, b_dg)
    # apply, out of place, with the kernel's c1 / c2 as the reference's inputs
    dy = Guarded(N * C * S)
    _lib.call("msl_bn_relu_bwd_apply", ptr(gd), ptr(yd), ptr(vd[0]), ptr(vd[1]), ptr(vd[2]), ptr(vd[3]), ptr(outs["c1"].v),
              ptr(outs["c2"].v), ptr(dy.v), N, C, S, st())
    dy.intact("dy")
    c1, c2 = outs["c1"].v.cpu(), outs["c2"].v.cpu()
    check("msl_bn_relu_bwd_apply", "dy", dy.v.view(N, C, S), R.bwd_apply_ref(g, y, vec, c1, c2), R.bwd_apply_bound(g, y, vec, c1, c2))
    # msl_bn_relu_bwd_finalize_apply (NP <= 256 here): the bits of finalize + apply - same partials, same lane order;
    # in place (dy == g), as the engine calls it
    assert NP <= 256
    bv = Guarded(8 * C, init=torch.cat([vec.reshape(-1), torch.full((4 * C,), float("nan"))]))
    o2 = {k: Guarded(C) for k in ("dgamma", "dbeta")}
    dy2 = Guarded(N * C * S, init=g)
    _lib.call("msl_bn_relu_bwd_finalize_apply", ptr(part.v), NP, count, ptr(dy2.v), ptr(yd), ptr(bv.v), ptr(o2["dgamma"].v),
              ptr(o2["dbeta"].v), ptr(dy2.v), N, C, S, st())
    for o, w in ((bv, "bn_vec"), (o2["dgamma"], "dgamma"), (o2["dbeta"], "dbeta"), (dy2, "dy")):
        o.intact("finalize_apply " + w)
    rows = bv.v.view(8, C)
    assert torch.equal(rows[:4].cpu(), vec), "finalize_apply changed rows 0-3 of bn_vec"
    assert torch.isnan(rows[6:]).all(), "finalize_apply wrote rows 6-7 of bn_vec"
    assert torch.equal(rows[4], outs["c1"].v) and torch.equal(rows[5], outs["c2"].v), "finalize_apply c1 / c2 bits"
    assert torch.equal(o2["dgamma"].v, outs["dgamma"].v) and torch.equal(o2["dbeta"].v, outs["dbeta"].v), "finalize_apply dgamma / dbeta bits"
    assert torch.equal(dy2.v, dy.v), "finalize_apply dy bits"


def test_bn_relu_bwd_finalize_apply_300_partials():
    """More partials than a lane's first pass covers twice (NP = 300 > 256: lanes 0-43 add five, the rest four)."""
    N, C, S, NP = 2, 3, 1000, 300
    g, y, vec = bwd_case(N, C, S, seed=31)
    count = float(N * S)
    dbeta, dgamma = R.bwd_sums_ref(g, y, vec)
    parts = split_partials(dbeta, dgamma, NP, gen(32))
    fr = R.bwd_finalize_ref(parts, count)
    bv = Guarded(6 * C, init=torch.cat([vec.reshape(-1), torch.full((2 * C,), float("nan"))]))
    dgam, dbet, dy = Guarded(C), Guarded(C), Guarded(N * C * S)
    _lib.call("msl_bn_relu_bwd_finalize_apply", ptr(K(parts)), NP, count, ptr(K(g)), ptr(K(y)), ptr(bv.v), ptr(dgam.v),
              ptr(dbet.v), ptr(dy.v), N, C, S, st())
    for o, w in ((bv, "bn_vec"), (dgam, "dgamma"), (dbet, "dbeta"), (dy, "dy")):
        o.intact(w)
    rows = bv.v.view(6, C)
    assert torch.equal(rows[:4].cpu(), vec)
    for k, got in (("dgamma", dgam.v), ("dbeta", dbet.v), ("c1", rows[4]), ("c2", rows[5])):
        check("msl_bn_relu_bwd_finalize_apply", k, got, fr[k], R.bwd_finalize_bound(fr, k))
    bound = R.bwd_apply_bound(g, y, vec, fr["c1"], fr["c2"], R.U * fr["c1"].abs(), R.U * fr["c2"].abs())
    check("msl_bn_relu_bwd_finalize_apply", "dy", dy.v.view(N, C, S), R.bwd_apply_ref(g, y, vec, fr["c1"], fr["c2"]), bound)


# ------------------------------------------------------------------------------------------------- msl_bn_bwd_finalize[_coef]
BWD_NP = [
    1,      # one lane, tail loop only
    63,     # tail loop, one lane idle
    64,     # tail loop, every lane once
    65,     # lane 0 twice
    447,    # last NP below the unrolled loop's entry (p + 448 < NP) for every lane
    448,    # still tail only: lane 0 would need p + 448 < 448
    449,    # lane 0 alone enters the eight-way unrolled loop
    512,    # every lane takes the unrolled loop once, no tail
    513,    # unrolled once, then lane 0's tail
    1024,   # unrolled twice
    2049,   # unrolled four times + tail
]


@pytest.mark.parametrize("C", [1, 3, 64])
@pytest.mark.parametrize("NP", BWD_NP)
def test_bn_bwd_finalize_and_coef_on_synthetic_partials(NP, C):
    g_ = gen(4000 + NP * 3 + C)
    count = 1000.0
    parts = torch.stack([torch.randn((C, NP), generator=g_, dtype=torch.float64) * 0.3 + 1.0,
                         torch.randn((C, NP), generator=g_, dtype=torch.float64) * 0.3 - 0.7]).contiguous()
    fr = R.bwd_finalize_ref(parts, count)
    pd = K(parts)
    outs = {k: Guarded(C) for k in ("dgamma", "dbeta", "c1", "c2")}
    _lib.call("msl_bn_bwd_finalize", ptr(pd), NP, count, ptr(outs["dgamma"].v), ptr(outs["dbeta"].v), ptr(outs["c1"].v),
              ptr(outs["c2"].v), C, st())
    for k, o in outs.items():
        o.intact(k)
        check("msl_bn_bwd_finalize", k, o.v, fr[k], R.bwd_finalize_bound(fr, k))
    # the (8, C) vector block form: rows 0-3 are inputs and stay, rows 4-7 = c1, c2, cC, cE
    vec = torch.stack([torch.randn(C, generator=g_) * 0.5 + 1.2, torch.randn(C, generator=g_) * 0.3,
                       torch.randn(C, generator=g_) + 0.5, torch.rand(C, generator=g_) + 0.5])
    bv = Guarded(8 * C, init=torch.cat([vec.reshape(-1), torch.full((4 * C,), float("nan"))]))
    o2 = {k: Guarded(C) for k in ("dgamma", "dbeta")}
    _lib.call("msl_bn_bwd_finalize_coef", ptr(pd), NP, count, ptr(o2["dgamma"].v), ptr(o2["dbeta"].v), ptr(bv.v), C, st())
    for o, w in ((bv, "bn_vec"), (o2["dgamma"], "dgamma"), (o2["dbeta"], "dbeta")):
        o.intact("coef " + w)
    rows = bv.v.view(8, C)
    assert torch.equal(rows[:4].cpu(), vec), "msl_bn_bwd_finalize_coef wrote rows 0-3"
    assert torch.equal(rows[4], outs["c1"].v) and torch.equal(rows[5], outs["c2"].v), "coef rows 4-5 are not msl_bn_bwd_finalize's c1 / c2"
    assert torch.equal(o2["dgamma"].v, outs["dgamma"].v) and torch.equal(o2["dbeta"].v, outs["dbeta"].v)
    cC, cE = R.coef_ref(fr["dbeta"], fr["dgamma"], count, vec)
    bC, bE = R.coef_bound(fr["dbeta"], fr["dgamma"], count, vec)
    check("msl_bn_bwd_finalize_coef", "cC", rows[6], cC, bC)
    check("msl_bn_bwd_finalize_coef", "cE", rows[7], cE, bE)


# ------------------------------------------------------------------------------------------------- msl_bn_finalize
def run_finalize(parts, NP, count, gamma, beta, rm, rv, nbt, mom, eps, C):
    """-> dict of Guarded outputs (running statistics / counter included when given)."""
    o = {k: Guarded(C) for k in ("scale", "shift", "mean", "invstd")}
    if rm is not None:
        o["running_mean"], o["running_var"] = Guarded(C, init=rm), Guarded(C, init=rv)
    if nbt is not None:
        o["nbt"] = Guarded(1, dtype=torch.int64, fill=-12345, init=torch.tensor([nbt]))
    p = lambda k: ptr(o[k].v) if k in o else None
    _lib.call("msl_bn_finalize", ptr(K(parts)), NP, float(count), ptr(K(gamma)), ptr(K(beta)), p("running_mean"), p("running_var"),
              p("nbt"), mom, eps, p("scale"), p("shift"), p("mean"), p("invstd"), C, st())
    for k, g in o.items():
        g.intact(k)
    return o


def check_finalize(entry, o, ref):
    for k in ("scale", "shift", "mean", "invstd", "running_mean", "running_var"):
        if k in o:
            check(entry, k, o[k].v, ref[k], R.finalize_bound(ref, k))


@pytest.mark.parametrize("NP", [
    1,     # serial fold, tail loop only
    7,     # serial fold, tail loop, last NP below the unrolled one
    8,     # serial fold, unrolled loop once, no tail
    9,     # serial fold, unrolled + tail
    64,    # serial fold at its limit (eight unrolled passes)
    65,    # wave fold, lane 0 twice
    512,   # wave fold, eight-way unrolled loop once
    513,   # wave fold, unrolled + tail
])
def test_bn_finalize(NP):
    N, C, S = 2, 5, 60
    g_ = gen(5000 + NP)
    y = torch.randn((N, C, S), generator=g_) * 2 + 1
    gamma, beta = torch.randn(C, generator=g_).abs() + 0.5, torch.randn(C, generator=g_) * 0.2
    rm, rv = torch.randn(C, generator=g_) * 0.1, torch.randn(C, generator=g_).abs() + 0.5
    s, q, count = stat_sums(y)
    parts = split_partials(s, q, NP, g_)
    o = run_finalize(parts, NP, count, gamma, beta, rm, rv, 41, MOM, EPS, C)
    ref = R.finalize_ref(R.exact_sum(parts[0]), R.exact_sum(parts[1]), count, gamma, beta, EPS, MOM, rm, rv)
    check_finalize("msl_bn_finalize", o, ref)
    assert int(o["nbt"].v) == 42


@pytest.mark.parametrize("edge", ["count1", "clamp", "no_running", "no_counter"])
def test_bn_finalize_edges(edge):
    C = 3
    gamma, beta = torch.tensor([1.5, 0.7, 1.0]), torch.tensor([0.1, -0.2, 0.0])
    rm, rv = torch.tensor([0.3, -0.1, 0.0]), torch.tensor([0.9, 1.4, 1.0])
    v = torch.tensor([3.0, -2.0, 0.5], dtype=torch.float64)
    count = 1 if edge == "count1" else 4
    if edge == "count1":    # one element per channel: the running variance takes the BIASED value (no 1 / (count - 1))
        s, q = v, v * v + 2.0
    elif edge == "clamp":   # inconsistent partials, q / count < mean^2: variance clamped at 0, invstd = 1 / sqrt(eps)
        s, q = v * count, 0.5 * v * v * count
    else:
        s, q = v * count, (v * v + 2.0) * count
    parts = torch.stack([s[:, None], q[:, None]]).contiguous()
    with_rs, with_nbt = edge != "no_running", edge != "no_counter"
    o = run_finalize(parts, 1, count, gamma, beta, rm if with_rs else None, rv if with_rs else None, 7 if with_nbt else None,
                     MOM, EPS, C)
    ref = R.finalize_ref(s, q, count, gamma, beta, EPS, MOM, rm if with_rs else None, rv if with_rs else None)
    check_finalize("msl_bn_finalize", o, ref)
    if with_nbt:
        assert int(o["nbt"].v) == 8
    if edge == "clamp":
        assert float(ref["var"].abs().max()) == 0.0
        assert torch.equal(o["invstd"].v.cpu(), R.f32(1.0 / torch.sqrt(torch.full((C,), R.as_c_float(EPS), dtype=torch.float64))))
    if edge == "count1":
        assert float((ref["running_var"] - (0.9 * rv.double() + 0.1 * 2.0)).abs().max()) < 1e-7


@pytest.mark.parametrize("ratio", [0.0, 1.0, 1e2, 1e4])
def test_bn_finalize_materialize_conditioning(ratio):
    """|mean| / std sweep of msl_bn_finalize -> msl_bn_relu_materialize against TRUE float64 BatchNorm: folding the mean
    into an fp32 shift costs about 2^-24 |mean * scale| absolute (1e-3 at ratio 1e4) - a property of the design, bounded
    by bn_ref.conditioning_bound and recorded in DESIGN.md."""
    N, C, dims = 2, 4, (4, 6, 8)
    g_ = gen(6000 + int(ratio))
    y = torch.randn((N, C) + dims, generator=g_) + ratio  # std 1
    gamma, beta = torch.randn(C, generator=g_).abs() + 0.5, torch.randn(C, generator=g_) * 0.2
    s, q, count = stat_sums(y)
    parts = torch.stack([s[:, None], q[:, None]]).contiguous()  # NP = 1: kernel and reference start from the same two numbers
    o = run_finalize(parts, 1, count, gamma, beta, None, None, None, MOM, EPS, C)
    check_finalize("msl_bn_finalize", o, R.finalize_ref(s, q, count, gamma, beta, EPS, MOM))
    out = Guarded(y.numel())
    _lib.call("msl_bn_relu_materialize", ptr(K(y)), ptr(o["scale"].v), ptr(o["shift"].v), ptr(out.v), None, N, C, *dims, st())
    out.intact("out")
    # true BatchNorm, two-pass in float64
    yd = y.double()
    d = (0, 2, 3, 4)
    mean = yd.mean(d)
    var = ((yd - mean.view(1, -1, 1, 1, 1)) ** 2).mean(d)
    scale = gamma.double() / torch.sqrt(var + R.as_c_float(EPS))
    true = torch.relu((yd - mean.view(1, -1, 1, 1, 1)) * scale.view(1, -1, 1, 1, 1) + beta.double().view(1, -1, 1, 1, 1))
    check("msl_bn_finalize+materialize", f"ratio={ratio:g}", out.v.view(y.shape), true, R.conditioning_bound(y, mean, scale, beta))
    log = os.environ.get("MSL_BN_RATIO_LOG")
    if log:
        with open(log, "a") as f:
            f.write(f"conditioning ratio={ratio:g} max_abs_dev {float((out.v.view(y.shape).cpu().double() - true).abs().max()):.3e}\n")


# ------------------------------------------------------------------------------------------------- batched tables
def bn_table(entries):
    """entries: dicts of device tensors / numbers -> (device table, total channels); first_block = running channel count."""
    L = _lib.load()
    esz = L.msl_bn_finalize_entry_bytes()
    host = (ctypes.c_ubyte * (esz * len(entries)))()
    first = 0
    for k, e in enumerate(entries):
        _lib.check(L.msl_bn_finalize_table_set(ctypes.addressof(host), k, first, ptr(e["parts"]), e["NP"], float(e["count"]),
                                               ptr(e["gamma"]), ptr(e["beta"]), ptr(e.get("rm")), ptr(e.get("rv")), ptr(e.get("nbt")),
                                               e["mom"], e["eps"], ptr(e["scale"]), ptr(e["shift"]), ptr(e.get("mean")),
                                               ptr(e.get("invstd")), e["C"]), "msl_bn_finalize_table_set")
        first += e["C"]
    return K(torch.frombuffer(bytearray(host), dtype=torch.uint8)), first


BATCH_ENTRIES = [  # (C, NP, momentum, eps, running statistics?)
    (1, 1, 0.1, 1e-5, True),      # serial fold, one partial, one channel
    (8, 65, 0.1, 1e-5, True),     # wave fold, first NP past 64
    (32, 64, 0.3, 1e-3, False),   # serial fold at its limit; no running statistics
    (512, 7, 0.1, 1e-5, True),    # the widest layer
    (8, 513, 0.01, 1e-4, True),   # wave fold, unrolled loop + tail
    (32, 63, 0.1, 1e-5, False),   # serial, no running statistics
    (1, 200, 1.0, 1e-5, True),    # momentum 1: the running estimate is replaced
]


def test_bn_finalize_batch_is_the_single_launches_bit_for_bit():
    sets = []
    for which in range(2):  # 0: one batched launch, 1: one msl_bn_finalize per entry; same inputs, separate outputs
        g2 = gen(7001)
        entries = []
        for k, (C, NP, mom, eps, rs) in enumerate(BATCH_ENTRIES):
            count = 100.0 + 37 * k
            mean, var = torch.randn(C, generator=g2, dtype=torch.float64), torch.rand(C, generator=g2, dtype=torch.float64) + 0.5
            parts = split_partials(mean * count, (var + mean * mean) * count, NP, g2)
            gamma, beta = torch.randn(C, generator=g2).abs() + 0.5, torch.randn(C, generator=g2) * 0.2
            rm, rv = torch.randn(C, generator=g2) * 0.1, torch.randn(C, generator=g2).abs() + 0.5
            e = dict(C=C, NP=NP, count=count, mom=mom, eps=eps, parts_cpu=parts, gamma_cpu=gamma, beta_cpu=beta, rm_cpu=rm, rv_cpu=rv,
                     parts=K(parts), gamma=K(gamma), beta=K(beta), nbt0=10 * k + 3, rs=rs)
            e["g"] = {n: Guarded(C) for n in ("scale", "shift", "mean", "invstd")}
            if rs:
                e["g"]["rm"], e["g"]["rv"] = Guarded(C, init=rm), Guarded(C, init=rv)
            e["g"]["nbt"] = Guarded(1, dtype=torch.int64, fill=-12345, init=torch.tensor([e["nbt0"]]))
            for n, gd in e["g"].items():
                e[n] = gd.v
            entries.append(e)
        sets.append(entries)
    table, total = bn_table(sets[0])
    assert total == sum(c for c, *_ in BATCH_ENTRIES)
    _lib.call("msl_bn_finalize_batch", ptr(table), len(sets[0]), total, st())
    for e in sets[1]:
        _lib.call("msl_bn_finalize", ptr(e["parts"]), e["NP"], e["count"], ptr(e["gamma"]), ptr(e["beta"]), ptr(e.get("rm")),
                  ptr(e.get("rv")), ptr(e["nbt"]), e["mom"], e["eps"], ptr(e["scale"]), ptr(e["shift"]), ptr(e["mean"]),
                  ptr(e["invstd"]), e["C"], st())
    for k, (a, b) in enumerate(zip(*sets)):
        for n, gd in a["g"].items():
            gd.intact(f"entry {k} {n}")
            b["g"][n].intact(f"entry {k} {n} (single)")
            assert torch.equal(gd.v, b["g"][n].v), f"entry {k} {n}: batched launch differs from msl_bn_finalize"
        assert int(a["nbt"]) == a["nbt0"] + 1, f"entry {k}: counter"
        ref = R.finalize_ref(R.exact_sum(a["parts_cpu"][0]), R.exact_sum(a["parts_cpu"][1]), a["count"], a["gamma_cpu"], a["beta_cpu"],
                             a["eps"], a["mom"], a["rm_cpu"] if a["rs"] else None, a["rv_cpu"] if a["rs"] else None)
        o = {n: a["g"][n] for n in ("scale", "shift", "mean", "invstd")}
        if a["rs"]:
            o["running_mean"], o["running_var"] = a["g"]["rm"], a["g"]["rv"]
        check_finalize("msl_bn_finalize_batch", o, ref)


EVAL_ENTRIES = [  # (C, eps): 691 channels = 5 workgroups of 128 + 51; entries 1, 3, 5 and 6 straddle a workgroup boundary
    (100, 1e-5), (50, 1e-5), (1, 1e-3), (200, 1e-5), (8, 1e-4), (32, 1e-5), (300, 1e-5)]


def test_bn_eval_affine_batch_is_the_single_launches_bit_for_bit():
    g_ = gen(8000)
    entries, singles = [], []
    for C, eps in EVAL_ENTRIES:
        gamma, beta = torch.randn(C, generator=g_).abs() + 0.5, torch.randn(C, generator=g_) * 0.2
        rm, rv = torch.randn(C, generator=g_), torch.rand(C, generator=g_) * 2 + 0.01
        sc, sh, sc1, sh1 = Guarded(C), Guarded(C), Guarded(C), Guarded(C)
        entries.append(dict(C=C, NP=1, count=1.0, mom=MOM, eps=eps, parts=K(torch.zeros(2 * C, dtype=torch.float64)), gamma=K(gamma),
                            beta=K(beta), rm=K(rm), rv=K(rv), scale=sc.v, shift=sh.v, cpu=(gamma, beta, rm, rv), g=(sc, sh, sc1, sh1)))
    table, total = bn_table(entries)
    assert total == 691 and total % 128 != 0
    _lib.call("msl_bn_eval_affine_batch", ptr(table), len(entries), total, st())
    for k, e in enumerate(entries):
        sc, sh, sc1, sh1 = e["g"]
        _lib.call("msl_bn_eval_affine", ptr(e["gamma"]), ptr(e["beta"]), ptr(e["rm"]), ptr(e["rv"]), e["eps"], ptr(sc1.v), ptr(sh1.v),
                  e["C"], st())
        for o in e["g"]:
            o.intact(f"entry {k}")
        assert torch.equal(sc.v, sc1.v) and torch.equal(sh.v, sh1.v), f"entry {k}: batched launch differs from msl_bn_eval_affine"
        rs, rh = R.eval_affine_ref(*e["cpu"], e["eps"])
        bs, bh = R.eval_affine_bound(*e["cpu"], e["eps"])
        check("msl_bn_eval_affine_batch", "scale", sc.v, rs, bs)
        check("msl_bn_eval_affine_batch", "shift", sh.v, rh, bh)
        assert torch.equal(e["rm"].cpu(), e["cpu"][2]) and torch.equal(e["rv"].cpu(), e["cpu"][3]), "running statistics changed"


# ------------------------------------------------------------------------------------------------- msl_bn_relu_materialize
SENT = -777.0

MAT_DIMS = [
    (4, 6, 8),      # W % 4 == 0: float4 loop, one workgroup per row, 48 live threads
    (3, 5, 7),      # scalar loop, S = 105
    (1, 1, 1),      # scalar loop, one voxel
    (2, 2, 3),      # scalar loop, S = 12: S % 4 == 0 but W % 4 != 0 (the branch is on W)
    (48, 48, 32),   # float4 loop, S / 4 = 18432 > 64 * 256: grid-stride
    (30, 30, 30),   # scalar loop, S = 27000 > 64 * 256: grid-stride
]


def materialize_case(dims, seed):
    N, C = 2, 3
    g_ = gen(seed)
    y = torch.randn((N, C) + dims, generator=g_) * 2 + 1
    gamma, beta = torch.randn(C, generator=g_).abs() + 0.5, torch.randn(C, generator=g_) * 0.2
    vec = R.host_vectors(y, gamma, beta, EPS)
    y.view(-1)[y.numel() // 2] = float("nan")  # a diverged value must come out as NaN, not as 0
    return N, C, y, vec


def check_padded(pad, N, C, dims, ref, bound, entry):
    pad.intact("padded")
    p = pad.v.view((N, C) + tuple(d + 2 for d in dims))
    check(entry, "padded interior", p[:, :, 1:-1, 1:-1, 1:-1], ref, bound)
    halo = p.clone()
    halo[:, :, 1:-1, 1:-1, 1:-1] = SENT
    assert bool((halo == SENT).all()), "the halo of the padded layout was written"


@pytest.mark.parametrize("mode", ["plain", "padded", "both"])
@pytest.mark.parametrize("dims", MAT_DIMS)
def test_bn_relu_materialize(dims, mode):
    N, C, y, vec = materialize_case(dims, seed=9000 + dims[0] * dims[2])
    vd = K(vec)
    out = Guarded(y.numel()) if mode != "padded" else None
    pad = Guarded(N * C * (dims[0] + 2) * (dims[1] + 2) * (dims[2] + 2), fill=SENT) if mode != "plain" else None
    _lib.call("msl_bn_relu_materialize", ptr(K(y)), ptr(vd[0]), ptr(vd[1]), ptr(out.v) if out else None, ptr(pad.v) if pad else None,
              N, C, *dims, st())
    ref, bound = R.act_ref(y, vec[0], vec[1]), R.act_bound(y, vec[0], vec[1])
    assert int(torch.isnan(ref).sum()) == 1
    if out:
        out.intact("plain")
        check("msl_bn_relu_materialize", "plain", out.v.view(y.shape), ref, bound)
    if pad:
        check_padded(pad, N, C, dims, ref, bound, "msl_bn_relu_materialize")


@pytest.mark.parametrize("NP", [
    1,      # serial fold, one partial
    8,      # serial fold, unrolled loop
    64,     # serial fold at its limit
    65,     # wave fold (wave 0 of the workgroup)
    256,    # wave fold, four per lane
    513,    # wave fold, eight-way unrolled loop + tail
    2048,   # wave fold, unrolled four times
])
def test_bn_relu_materialize_fold_is_finalize_plus_materialize_bit_for_bit(NP):
    dims = (4, 6, 8) if NP % 2 else (3, 5, 7)  # float4 / scalar loop
    N, C = 2, 5
    g_ = gen(9500 + NP)
    y = torch.randn((N, C) + dims, generator=g_) * 2 + 1
    gamma, beta = torch.randn(C, generator=g_).abs() + 0.5, torch.randn(C, generator=g_) * 0.2
    s, q, count = stat_sums(y)
    parts = split_partials(s, q, NP, g_)
    o = run_finalize(parts, NP, count, gamma, beta, None, None, None, MOM, EPS, C)
    npad = N * C * (dims[0] + 2) * (dims[1] + 2) * (dims[2] + 2)
    a_out, a_pad, b_out, b_pad = Guarded(y.numel()), Guarded(npad, fill=SENT), Guarded(y.numel()), Guarded(npad, fill=SENT)
    yd = K(y)
    _lib.call("msl_bn_relu_materialize", ptr(yd), ptr(o["scale"].v), ptr(o["shift"].v), ptr(a_out.v), ptr(a_pad.v), N, C, *dims, st())
    _lib.call("msl_bn_relu_materialize_fold", ptr(yd), ptr(K(parts)), NP, float(count), ptr(K(gamma)), ptr(K(beta)), EPS, ptr(b_out.v),
              ptr(b_pad.v), N, C, *dims, st())
    for w in (a_out, a_pad, b_out, b_pad):
        w.intact("materialize")
    assert torch.equal(a_out.v, b_out.v), "plain output: the fold differs from msl_bn_finalize + msl_bn_relu_materialize"
    assert torch.equal(a_pad.v, b_pad.v), "padded output: the fold differs"
    ref = R.finalize_ref(R.exact_sum(parts[0]), R.exact_sum(parts[1]), count, gamma, beta, EPS, MOM)
    sc32, sh32 = o["scale"].v.cpu(), o["shift"].v.cpu()
    check_finalize("msl_bn_finalize", o, ref)
    check("msl_bn_relu_materialize_fold", "plain", b_out.v.view(y.shape), R.act_ref(y, sc32, sh32), R.act_bound(y, sc32, sh32))
    check_padded(b_pad, N, C, dims, R.act_ref(y, sc32, sh32), R.act_bound(y, sc32, sh32), "msl_bn_relu_materialize_fold")


# ------------------------------------------------------------------------------------------------- forward / backward mask
@pytest.mark.parametrize("W", [16, 15])  # float4 / scalar loops of materialize and apply
def test_forward_and_backward_agree_on_the_relu_mask(W):
    """scale 1, shift 0, mean 0, invstd 1, g = 1, c1 = c2 = 0: dy = [y > 0].  The backward must mask exactly where the
    forward output is positive; y = +-0 gives 0 in both.  Denormals are only checked for agreement between the two (the
    project does not specify flushing)."""
    tiny = 1.1754943508222875e-38  # smallest normal
    vals = [0.0, -0.0, tiny, -tiny, 1.0, -1.0, 2 * tiny, -2 * tiny, 1e-40, -1e-40, 1e-45, -1e-45, 3.0, -3.0, 0.0, -0.0]
    y = torch.tensor(vals[:W]).view(1, 1, 1, 1, W)
    denorm = (y != 0) & (y.abs() < tiny)
    vec = torch.tensor([[1.0], [0.0], [0.0], [1.0]])
    vd, yd = K(vec), K(y)
    zero = K(torch.zeros(1))
    out, dy = Guarded(W), Guarded(W)
    _lib.call("msl_bn_relu_materialize", ptr(yd), ptr(vd[0]), ptr(vd[1]), ptr(out.v), None, 1, 1, 1, 1, W, st())
    _lib.call("msl_bn_relu_bwd_apply", ptr(K(torch.ones(W))), ptr(yd), ptr(vd[0]), ptr(vd[1]), ptr(vd[2]), ptr(vd[3]), ptr(zero),
              ptr(zero), ptr(dy.v), 1, 1, W, st())
    out.intact("out")
    dy.intact("dy")
    o, d = out.v.cpu().view(y.shape), dy.v.cpu().view(y.shape)
    assert torch.equal(d != 0, o > 0), f"forward {o.flatten().tolist()} backward {d.flatten().tolist()}"
    normal = ~denorm
    assert torch.equal(o[normal], torch.relu(y)[normal]) and torch.equal(d[normal], (y > 0).float()[normal])
    assert bool((o[y == 0] == 0).all()) and bool((d[y == 0] == 0).all())


# ------------------------------------------------------------------------------------------------- the chain
@pytest.mark.parametrize("N,C,dims", [
    (3, 8, (4, 6, 8)),       # S = 192: one chunk; fused <256,1>
    (2, 4, (5, 7, 9)),       # S = 315: scalar branches everywhere; generic fused kernel
    (4, 2, (16, 32, 32)),    # S = 16384: four chunks per row; fused generic kernel at N * S = 65536
])
def test_bn_chain_matches_float64_autograd(N, C, dims):
    """finalize -> materialize -> reduce -> finalize -> apply, and the fused backward, with the vectors the KERNEL made,
    against float64 autograd of relu(batch_norm(y)).  The kernel's fp32 scale / shift move the pre-activation by ~1e-6 on
    this well-conditioned data, so every |a| is first moved out of (-1e-3, 1e-3): the masks agree and nothing is excluded."""
    L = _lib.load()
    S = dims[0] * dims[1] * dims[2]
    g_ = gen(11000 + S)
    y = torch.randn((N, C) + dims, generator=g_) * 2 + 1
    gamma, beta = torch.randn(C, generator=g_).abs() + 0.5, torch.randn(C, generator=g_) * 0.2
    rm, rv = torch.randn(C, generator=g_) * 0.1, torch.randn(C, generator=g_).abs() + 0.5
    g = torch.randn((N, C) + dims, generator=g_)
    y, amin = R.separate_preactivation(y, gamma, beta, EPS, 1e-3)
    assert amin >= 1e-3
    count = float(N * S)
    mom64, eps64 = R.as_c_float(MOM), R.as_c_float(EPS)
    yt, gt, bt = y.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rm_t, rv_t = rm.double(), rv.double()
    a = torch.relu(F.batch_norm(yt, rm_t, rv_t, gt, bt, True, mom64, eps64))
    a.backward(g.double())
    # forward: per-sample partials
    yd64 = y.double()
    parts = torch.stack([yd64.sum((2, 3, 4)).t(), (yd64 * yd64).sum((2, 3, 4)).t()]).contiguous()  # (2, C, NP = N)
    o = run_finalize(parts, N, count, gamma, beta, rm, rv, 0, MOM, EPS, C)
    ref = R.finalize_ref(R.exact_sum(parts[0]), R.exact_sum(parts[1]), count, gamma, beta, EPS, MOM, rm, rv)
    check_finalize("chain msl_bn_finalize", o, ref)
    check("chain", "running_mean vs torch", o["running_mean"].v, rm_t, R.finalize_bound(ref, "running_mean"))
    check("chain", "running_var vs torch", o["running_var"].v, rv_t, R.finalize_bound(ref, "running_var"))
    vec64 = torch.stack([ref[k] for k in ("scale", "shift", "mean", "invstd")])
    vd = [o[k].v for k in ("scale", "shift", "mean", "invstd")]
    yd, gd = K(y), K(g)
    out = Guarded(y.numel())
    _lib.call("msl_bn_relu_materialize", ptr(yd), ptr(vd[0]), ptr(vd[1]), ptr(out.v), None, N, C, *dims, st())
    out.intact("out")
    check("chain", "act", out.v.view(y.shape), a.detach(), R.conditioning_bound(y, ref["mean"], ref["scale"], beta))
    # backward, three launches
    NP = L.msl_bn_relu_bwd_num_partials(N, S)
    part = Guarded(2 * C * NP, dtype=torch.float64)
    _lib.call("msl_bn_relu_bwd_reduce", ptr(gd), ptr(yd), ptr(vd[0]), ptr(vd[1]), ptr(vd[2]), ptr(vd[3]), ptr(part.v), N, C, S, st())
    outs = {k: Guarded(C) for k in ("dgamma", "dbeta", "c1", "c2")}
    _lib.call("msl_bn_bwd_finalize", ptr(part.v), NP, count, ptr(outs["dgamma"].v), ptr(outs["dbeta"].v), ptr(outs["c1"].v),
              ptr(outs["c2"].v), C, st())
    dy = Guarded(y.numel())
    _lib.call("msl_bn_relu_bwd_apply", ptr(gd), ptr(yd), ptr(vd[0]), ptr(vd[1]), ptr(vd[2]), ptr(vd[3]), ptr(outs["c1"].v),
              ptr(outs["c2"].v), ptr(dy.v), N, C, S, st())
    # the fused launch
    dg2, db2, dy2 = Guarded(C), Guarded(C), Guarded(y.numel())
    _lib.call("msl_bn_relu_bwd_fused", ptr(gd), ptr(yd), ptr(vd[0]), ptr(vd[1]), ptr(vd[2]), ptr(vd[3]), ptr(dg2.v), ptr(db2.v),
              ptr(dy2.v), N, C, S, st())
    for w in (part, dy, dg2, db2, dy2, *outs.values()):
        w.intact("chain backward")
    extra_dg, extra_dy = R.chain_extra_bounds(g, y, vec64)
    c1, c2 = bt.grad / count, gt.grad / count
    for name, nt, dbet, dgam, dyk in (("three launches", 16, outs["dbeta"].v, outs["dgamma"].v, dy.v),
                                      ("fused", fused_nt(N, S), db2.v, dg2.v, dy2.v)):
        b_db, b_dg = R.bwd_sums_bound(g, y, vec64, nt)
        b_dg = b_dg + extra_dg
        check("chain " + name, "dbeta", dbet, bt.grad, b_db)
        check("chain " + name, "dgamma", dgam, gt.grad, b_dg)
        bound = R.bwd_apply_bound(g, y, vec64, c1, c2, b_db / count + R.U * c1.abs(), b_dg / count + R.U * c2.abs()) + extra_dy(c1, c2)
        check("chain " + name, "dy", dyk.view(y.shape), yt.grad, bound)


# ------------------------------------------------------------------------------------------------- recorded bits, both storage types
def test_bn_relu_bwd_bits_are_the_recorded_ones():
    """Every output buffer of the eight BatchNorm+ReLU-backward entry points, fp32 and bf16, has the SHA-256 that
    tests/golden/bn_bwd_bits.json recorded before the two kernel families became one (make_bn_bwd_bits's docstring): a
    mismatch means the kernels changed their bits, never that the file wants minting again."""
    import json
    from tests.golden import make_bn_bwd_bits as M
    with open(M.OUT) as f:
        want = json.load(f)
    got = M.digests(DEV)
    assert sorted(got) == sorted(want), "the cases are not the recorded ones"
    assert {k.split()[0] for k in want} == {
        "msl_bn_relu_bwd_reduce", "msl_bn_relu_bwd_apply", "msl_bn_relu_bwd_fused", "msl_bn_relu_bwd_finalize_apply",
        "msl_bn_relu_bwd_reduce_bf16", "msl_bn_relu_bwd_apply_bf16", "msl_bn_relu_bwd_fused_bf16", "msl_bn_bwd_finalize"}
    bad = [k for k in want if got[k] != want[k]]
    assert not bad, f"{len(bad)}/{len(want)} buffers differ from the recorded bits: {bad[:8]}"


def test_bn_relu_bwd_fp32_scalar_branch_and_bf16_do_the_same_fp32_operations():
    """On g and y that are bf16 values, an fp32 launch on its scalar branch (S % 4 != 0) and a bf16 launch run the same fp32
    operations in the same order: equal partials / dgamma / dbeta, and the bf16 dy is the fp32 dy rounded to nearest even."""
    BF = torch.bfloat16

    def case(N, C, S, seed):
        g, y, vec = bwd_case(N, C, S, seed)
        g, y = g.to(BF), y.to(BF)
        k = torch.randn((2, C), generator=gen(seed + 1)) * 0.1  # c1, c2: any fp32 values
        vd = K(torch.cat([vec, k]))
        return K(g.float()), K(y.float()), K(g), K(y), vd, [ptr(vd[r]) for r in range(4)]

    def bits(t):
        return t.contiguous().view(torch.int16)

    L = _lib.load()
    N, C, S = 2, 3, 4099  # two chunks, the second ragged
    g32, y32, g16, y16, vd, rows = case(N, C, S, 12000)
    NP = L.msl_bn_relu_bwd_num_partials(N, S)
    assert NP == L.msl_bn_relu_bwd_bf16_num_partials(N, S) == 4
    p32, p16 = Guarded(2 * C * NP, dtype=torch.float64), Guarded(2 * C * NP, dtype=torch.float64)
    _lib.call("msl_bn_relu_bwd_reduce", ptr(g32), ptr(y32), *rows, ptr(p32.v), N, C, S, st())
    _lib.call("msl_bn_relu_bwd_reduce_bf16", ptr(g16), ptr(y16), *rows, ptr(p16.v), N, C, S, st())
    p32.intact("fp32 partials")
    p16.intact("bf16 partials")
    assert bool(torch.isfinite(p32.v).all()) and torch.equal(p32.v, p16.v), "reduce: the partials differ between the storage types"
    dy32, dy16 = Guarded(N * C * S), Guarded(N * C * S, dtype=BF)
    _lib.call("msl_bn_relu_bwd_apply", ptr(g32), ptr(y32), *rows, ptr(vd[4]), ptr(vd[5]), ptr(dy32.v), N, C, S, st())
    _lib.call("msl_bn_relu_bwd_apply_bf16", ptr(g16), ptr(y16), ptr(vd), ptr(dy16.v), N, C, S, st())
    dy32.intact("fp32 dy")
    dy16.intact("bf16 dy")
    assert bool(torch.isfinite(dy32.v).all())
    assert torch.equal(bits(dy16.v), bits(dy32.v.to(BF))), "apply: the bf16 dy is not the rounded fp32 dy"

    N, C, S = 2, 3, 1027  # the generic fused kernel on both sides
    g32, y32, g16, y16, vd, rows = case(N, C, S, 12100)
    o32 = [Guarded(C), Guarded(C), Guarded(N * C * S)]
    o16 = [Guarded(C), Guarded(C), Guarded(N * C * S, dtype=BF)]
    _lib.call("msl_bn_relu_bwd_fused", ptr(g32), ptr(y32), *rows, ptr(o32[0].v), ptr(o32[1].v), ptr(o32[2].v), N, C, S, st())
    _lib.call("msl_bn_relu_bwd_fused_bf16", ptr(g16), ptr(y16), ptr(vd), ptr(o16[0].v), ptr(o16[1].v), ptr(o16[2].v), N, C, S, st())
    for o in o32 + o16:
        o.intact("fused")
    assert bool(torch.isfinite(o32[2].v).all())
    assert torch.equal(o32[0].v, o16[0].v), "fused: dgamma differs between the storage types"
    assert torch.equal(o32[1].v, o16[1].v), "fused: dbeta differs between the storage types"
    assert torch.equal(bits(o16[2].v), bits(o32[2].v.to(BF))), "fused: the bf16 dy is not the rounded fp32 dy"
