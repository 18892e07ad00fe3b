"""Every stem-convolution entry point of csrc/stem.hip, path by path, against the float64 reference of tests/stem_ref.py
(bounds derived there, not tuned; each failure message prints the worst error / bound and its index).

The BatchNorm vectors are made on the host and ``stem_ref.mask32`` reproduces the kernels' ReLU mask bit for bit, so no element
is excluded anywhere and no margin around zero is needed.  Every output - y, the statistics partials, dw and the WHOLE slab
workspace of msl_stem_conv_bwd_weight_workspace_bytes - is pre-filled with NaN and sits between guard bands that must come back
untouched.  Each case id names the kernel it reaches (tests/stem_cases.py; asserted per case in tests/test_stem_ref_cpu.py);
DESIGN.md, Appendix A, lists every instantiation with its case.  With MSL_STEM_RATIO_LOG=<file> every comparison appends
"<case id> <what> <error / bound>" to that file (for the error / bound table of DESIGN.md)."""
import ctypes
import os

import pytest
import torch

from mslesions3d_amd import _lib
from mslesions3d_amd._lib import ptr
from tests import stem_cases as C
from tests import stem_ref as S
from tests.bf16_emul import bf

pytestmark = pytest.mark.gpu
DEV = "cuda"
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
def _release_kept():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


class Guarded:
    """An output buffer of n elements, NaN-filled, between two bands of G NaN guard elements."""

    def __init__(self, n, dtype=torch.float32):
        self.n = n
        self.full = torch.full((n + 2 * G,), NAN, dtype=dtype, device=DEV)
        self.v = self.full[G:G + n]
        _KEEP.append(self.full)

    def intact(self, what):
        bands = torch.cat([self.full[:G], self.full[G + self.n:]])
        assert bool(torch.isnan(bands).all()), f"{what}: wrote outside its range"

    def untouched(self, what):
        assert bool(torch.isnan(self.full).all()), f"{what}: a refused call wrote to its output"

    def written(self, what, n=None):
        bad = int(torch.isnan(self.v[:n]).sum())
        assert bad == 0, f"{what}: {bad} elements were never written (or are NaN)"


def check(path, what, actual, ref, bound):
    ratio, idx, bad = S.worst(actual, ref, bound)
    log = os.environ.get("MSL_STEM_RATIO_LOG")
    if log:
        with open(log, "a") as f:
            f.write(f"{path} {what} {ratio:.4f}\n")
    a, r = actual.detach().cpu().double().reshape(-1), ref.double().reshape(-1)
    assert bad == 0, (f"{path} {what}: {bad}/{r.numel()} elements over their bound; worst error / bound {ratio:.3f} at idx {idx} "
                      f"(got {a[idx].item():.9e}, ref {r[idx].item():.9e})")


def same_bits(a, b):
    """Bit identity of two device tensors of one dtype (NaN payloads and zero signs included)."""
    it = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return a.dtype == b.dtype and bool(torch.equal(a.contiguous().view(it), b.contiguous().view(it)))


def gen(seed):
    return torch.Generator().manual_seed(seed)


def seed_of(N, cin, dims, stride):
    return 1000 * cin + 97 * dims[0] + 31 * dims[1] + 7 * dims[2] + 3 * stride[0] + 2 * stride[1] + stride[2] + N


# ------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("case", C.FWD_CASES, ids=[c[0] for c in C.FWD_CASES])
def test_stem_fwd(case):
    """msl_stem_conv_fwd: y and the statistics inside their bounds, every partial slot written, nothing else written.
    msl_stem_conv_fwd_bf16: y is round-to-nearest-even of the fp32 entry's y and the partials are its partials, bit for bit."""
    path, N, cin, dims, stride = case
    L = _lib.load()
    g = gen(seed_of(N, cin, dims, stride))
    x = torch.randn((N, cin) + dims, generator=g)
    w = torch.randn((32, cin, 3, 3, 3), generator=g) * 0.3
    yr, absdot = S.fwd_ref(x, w, stride)
    od, oh, ow = S.out_dims(dims, stride)
    OS = od * oh * ow
    plan = S.fwd_plan(cin, dims, stride)
    NP = L.msl_stem_conv_fwd_num_partials(N, od, oh, ow)
    assert NP == N * plan["nb"]
    xd, wd = dev(x), dev(w)
    y, part = Guarded(N * 32 * OS), Guarded(2 * 32 * NP, dtype=torch.float64)
    rc = L.msl_stem_conv_fwd(ptr(xd), ptr(wd), ptr(y.v), ptr(part.v), N, cin, *dims, *stride, st())
    torch.cuda.synchronize()
    assert rc == 0
    y.intact("y")
    part.intact("partials")
    y.written("y")
    part.written("partials")
    ybound = S.fwd_bound(absdot, cin)
    check(path, "y", y.v, yr, ybound)
    got = S.fold_partials(part.v.cpu(), NP)
    own, ob = S.stats_own_ref(y.v.cpu().view(N, 32, OS), plan["iters"])
    check(path, "stats-of-own-y", got, own, ob)
    tot, tb = S.stats_total_ref(yr.flatten(2), ybound.flatten(2))
    check(path, "stats-of-ref-y", got, tot, tb + ob)
    # without statistics: the same y
    y2 = Guarded(N * 32 * OS)
    assert L.msl_stem_conv_fwd(ptr(xd), ptr(wd), ptr(y2.v), None, N, cin, *dims, *stride, st()) == 0
    torch.cuda.synchronize()
    y2.intact("y, no statistics")
    assert same_bits(y2.v, y.v), "y without statistics differs"
    # bf16 output
    yb, pb = Guarded(N * 32 * OS, dtype=torch.bfloat16), Guarded(2 * 32 * NP, dtype=torch.float64)
    rc = L.msl_stem_conv_fwd_bf16(ptr(xd), ptr(wd), ptr(yb.v), ptr(pb.v), N, cin, *dims, *stride, st())
    torch.cuda.synchronize()
    assert rc == 0
    yb.intact("bf16 y")
    pb.intact("bf16 partials")
    assert same_bits(yb.v, y.v.to(torch.bfloat16)), "bf16 y is not the rounded fp32 y"
    assert same_bits(pb.v, part.v), "partials of the bf16 entry differ from the fp32 entry's"
    assert same_bits(xd, x.to(DEV)) and same_bits(wd, w.to(DEV)), "inputs changed"


# ------------------------------------------------------------------------------------------------- weight gradient
def grad_reduce_stem(slabs, ns, cin):
    """The library's own deferred reduction (msl_grad_reduce_batch, kind 2) of ns padded slabs -> guarded dw."""
    L = _lib.load()
    K, NT = cin * 27, (cin * 27 + 31) // 32
    out = Guarded(32 * K)
    host = (ctypes.c_ubyte * L.msl_grad_reduce_entry_bytes())()
    nb = L.msl_grad_reduce_table_set(ctypes.addressof(host), 0, 0, 2, ptr(slabs), ptr(out.v), None, ns, 1024 * NT, 1024 * NT, K, NT, 0)
    assert nb > 0
    table = dev(torch.frombuffer(bytearray(host), dtype=torch.uint8))
    assert L.msl_grad_reduce_batch(ptr(table), 1, nb, st()) == 0
    torch.cuda.synchronize()
    out.intact("dw of msl_grad_reduce_batch")
    return out


def run_bww(path, what, launch, ref, bound, N, cin, dims, stride, plan, deferred):
    """One weight-gradient entry point: ``launch(dw_ptr, ws_ptr) -> rc``.  dw inside its bound; exactly nslabs slabs written
    into a NaN-filled workspace of the full advertised size; with ``deferred`` also the dw == NULL form."""
    L = _lib.load()
    K, NT = cin * 27, (cin * 27 + 31) // 32
    ns = L.msl_stem_conv_bwd_weight_nslabs(N, *dims, *stride)
    assert ns == plan["ns"] and 1 <= ns <= S.BW_BLOCKS
    wsn = L.msl_stem_conv_bwd_weight_workspace_bytes(cin) // 4
    assert wsn == S.BW_BLOCKS * 1024 * NT
    dw, ws = Guarded(32 * K), Guarded(wsn)
    rc = launch(ptr(dw.v), ptr(ws.v))
    torch.cuda.synchronize()
    assert rc == 0, f"{what} returned {rc}"
    dw.intact(f"{what}: dw")
    ws.intact(f"{what}: workspace")
    dw.written(f"{what}: dw")
    used = ns * 1024 * NT
    ws.written(f"{what}: slabs", used)
    assert bool(torch.isnan(ws.v[used:]).all()), f"{what}: wrote past slab {ns}"
    check(path, f"{what}:dw", dw.v.view(32, K), ref, bound)
    if not deferred:
        return
    ws2 = Guarded(wsn)
    rc = launch(None, ptr(ws2.v))
    torch.cuda.synchronize()
    assert rc == 0, f"{what}, deferred, returned {rc}"
    ws2.intact(f"{what}: deferred workspace")
    ws2.written(f"{what}: deferred slabs", used)
    assert bool(torch.isnan(ws2.v[used:]).all()), f"{what}: the deferred form wrote past slab {ns}"
    assert same_bits(ws2.v, ws.v), f"{what}: the deferred form's slabs differ from the immediate form's"
    sl = ws2.v[:used].view(ns, 32, 32 * NT)[:, :, :K].cpu().double()
    check(path, f"{what}:slab-sum", sl.sum(0), ref, bound)
    red = grad_reduce_stem(ws2.v, ns, cin)
    # two fp32 folds of the same ns slabs, each within (ns - 1) U sum |slab| of their exact sum; msl_grad_reduce_batch adds
    # <= 16 slabs serially, more in the order of the immediate form (msl::reduce_slabs_256), which for <= 8 slabs is serial too
    check(path, f"{what}:deferred-vs-immediate", dw.v.view(32, K), red.v.view(32, K).cpu().double(), 2 * ns * S.U * sl.abs().sum(0))
    if ns <= 8 or ns > 16:
        assert same_bits(red.v, dw.v), f"{what}: msl_grad_reduce_batch of the deferred slabs is not the immediate form's dw"


def bww_inputs(N, cin, dims, stride):
    g = gen(seed_of(N, cin, dims, stride) + 50000)
    odims = S.out_dims(dims, stride)
    d = dict(x=torch.randn((N, cin) + dims, generator=g), dy=torch.randn((N, 32) + odims, generator=g),
             y=torch.randn((N, 32) + odims, generator=g) * 1.5 + 0.3, dz=torch.randn((N, 32) + S.half_dims(odims), generator=g),
             w1=torch.randn((32, 1, 3, 3, 3), generator=g) * 0.4, gamma=torch.rand(32, generator=g) + 0.5,
             beta=torch.randn(32, generator=g) * 0.3)
    d["cols"] = S.im2col(d["x"].double(), stride)
    return d


def run_modes(path, N, cin, dims, stride, modes, deferred):
    L = _lib.load()
    d = bww_inputs(N, cin, dims, stride)
    xd = dev(d["x"])
    shape = (N, cin) + dims + stride
    fl = lambda t: t.flatten(2)
    for mode, b16 in modes:
        fused = mode == 2
        plan = S.bww_plan(N, cin, dims, stride, fused)
        r = bf if b16 else (lambda t: t)
        dt = torch.bfloat16 if b16 else torch.float32
        sfx = "_bf16" if b16 else ""
        if mode == 0:
            a, ab = d["dy"].double(), None
            dyd = dev(d["dy"])
            launch = lambda dw, ws: L.msl_stem_conv_bwd_weight(ptr(dyd), ptr(xd), dw, ws, *shape, st())
            what = "plain"
        elif mode == 1:
            gq, yq = r(d["dy"]), r(d["y"])
            vec = S.host_vec(gq, yq, d["gamma"], d["beta"], 6)
            a, ab = S.mode1_operand(gq, yq, vec)
            gd, yd, vd = dev(gq.to(dt)), dev(yq.to(dt)), dev(vec)
            fn = getattr(L, "msl_stem_conv_bwd_weight_bnapply" + sfx)
            launch = lambda dw, ws: fn(ptr(gd), ptr(yd), ptr(vd), ptr(xd), dw, ws, *shape, st())
            what = "bnapply" + sfx
        else:
            zq, yq = r(d["dz"]), r(d["y"])
            g64 = S.dwconv_t(zq.double(), d["w1"].double(), S.out_dims(dims, stride))
            vec = S.host_vec(g64, yq, d["gamma"], d["beta"], 8)
            a, ab, _, _ = S.mode2_operand(zq, d["w1"], yq, vec)
            zd, yd, vd = dev(zq.to(dt)), dev(yq.to(dt)), dev(vec)
            w1t = dev(d["w1"].view(32, 27).t())  # tap-major (27, 32)
            fn = getattr(L, "msl_stem_conv_bwd_weight_fused" + sfx)
            launch = lambda dw, ws: fn(ptr(zd), ptr(w1t), ptr(yd), ptr(vd), ptr(xd), dw, ws, *shape, st())
            what = "fused" + sfx
        ref, _ = S.bww_ref(fl(a), d["cols"])
        bound = S.bww_bound(fl(a), None if ab is None else fl(ab), d["cols"], plan)
        run_bww(path, what, launch, ref, bound, N, cin, dims, stride, plan, deferred)
    assert same_bits(xd, d["x"].to(DEV)), "x changed"


ALL_MODES = ((0, False), (1, False), (2, False), (1, True), (2, True))


@pytest.mark.parametrize("case", C.BWW_CASES, ids=[c[0] for c in C.BWW_CASES])
def test_stem_bwd_weight_wave(case):
    """stem_bwd_weight_kernel<Cin, 0 | 1 | 2, fp32 | bf16> through the five entry points."""
    path, N, cin, dims, stride = case
    run_modes(path, N, cin, dims, stride, ALL_MODES, path in C.DEFERRED)


@pytest.mark.parametrize("case", C.TILE_CASES, ids=[c[0] for c in C.TILE_CASES])
def test_stem_bwd_weight_tile(case):
    """stem_bww_tile_kernel<Cin, fp32 | bf16> through msl_stem_conv_bwd_weight_fused[_bf16]."""
    path, N, cin, dims, stride = case
    run_modes(path, N, cin, dims, stride, ((2, False), (2, True)), path in C.DEFERRED)


# ------------------------------------------------------------------------------------------------- refusals
def _refusals():
    """(id, cin, dims, stride, N, rc)"""
    out = []
    for name, dims in C.REFUSAL_SHAPES:
        out += [(f"Cin5-{name}", 5, dims, C.S222, 2, -2), (f"Cin0-{name}", 0, dims, C.S222, 2, -1),
                (f"Cin-1-{name}", -1, dims, C.S222, 2, -1)]
    dims = (9, 11, 16)
    for ax in range(3):
        for s in (0, 3):
            stride = tuple(s if k == ax else 2 for k in range(3))
            out.append((f"stride{''.join(map(str, stride))}", 1, dims, stride, 2, -1))
        for v in (0, -1):
            out.append((f"dim{ax}={v}", 1, tuple(v if k == ax else dims[k] for k in range(3)), C.S222, 2, -1))
    out += [("N0", 1, dims, C.S222, 0, -1), ("N-1", 1, dims, C.S222, -1, -1)]
    return out


def _entry_points(L, b, shape):
    """name -> (call, null-pointer variants); every entry point on the same buffers."""
    s = st()
    return {
        "fwd": lambda: L.msl_stem_conv_fwd(b["x"], b["w"], b["y"], b["part"], *shape, s),
        "fwd_bf16": lambda: L.msl_stem_conv_fwd_bf16(b["x"], b["w"], b["y"], b["part"], *shape, s),
        "bww": lambda: L.msl_stem_conv_bwd_weight(b["a"], b["x"], b["dw"], b["ws"], *shape, s),
        "bnapply": lambda: L.msl_stem_conv_bwd_weight_bnapply(b["a"], b["a"], b["vec"], b["x"], b["dw"], b["ws"], *shape, s),
        "bnapply_bf16": lambda: L.msl_stem_conv_bwd_weight_bnapply_bf16(b["a"], b["a"], b["vec"], b["x"], b["dw"], b["ws"], *shape, s),
        "fused": lambda: L.msl_stem_conv_bwd_weight_fused(b["a"], b["w"], b["a"], b["vec"], b["x"], b["dw"], b["ws"], *shape, s),
        "fused_bf16": lambda: L.msl_stem_conv_bwd_weight_fused_bf16(b["a"], b["w"], b["a"], b["vec"], b["x"], b["dw"], b["ws"], *shape, s),
    }


def _refusal_buffers(dims):
    """Inputs and NaN-filled outputs large enough for 5 channels at ``dims`` with N = 2 and stride 1 - a call that is wrongly
    accepted stays inside them."""
    vol = 2 * max(dims[0], 1) * max(dims[1], 1) * max(dims[2], 1)
    outs = dict(y=Guarded(32 * vol), part=Guarded(2 * 32 * 2 * S.FWD_BLOCKS_PER_IMAGE, dtype=torch.float64), dw=Guarded(32 * 5 * 27),
                ws=Guarded(S.BW_BLOCKS * 1024 * 5))
    b = dict(x=ptr(dev(torch.ones(5 * vol))), w=ptr(dev(torch.ones(32 * 5 * 27))), a=ptr(dev(torch.ones(32 * vol))),
             vec=ptr(dev(torch.ones(8 * 32))))
    b.update({k: ptr(o.v) for k, o in outs.items()})
    return b, outs


@pytest.mark.parametrize("case", _refusals(), ids=[c[0] for c in _refusals()])
def test_stem_refusals(case):
    """Every entry point returns the code, launches nothing (msl_thread_launch_count) and leaves its outputs NaN."""
    _, cin, dims, stride, N, want = case
    L = _lib.load()
    b, outs = _refusal_buffers(dims)
    n0 = L.msl_thread_launch_count()
    for name, f in _entry_points(L, b, (N, cin) + dims + stride).items():
        assert f() == want, name
    assert L.msl_thread_launch_count() == n0, "a refused call launched a kernel"
    torch.cuda.synchronize()
    for k, o in outs.items():
        o.untouched(k)


def test_stem_null_pointer_refusals():
    """The argument checks of _fused (dz, w1_t, yraw, bn_vec) and _bnapply (yraw, bn_vec), fp32 and bf16."""
    L = _lib.load()
    dims = (9, 11, 16)
    b, outs = _refusal_buffers(dims)
    shape = (2, 1) + dims + C.S222
    n0 = L.msl_thread_launch_count()
    for sfx in ("", "_bf16"):
        fused = getattr(L, "msl_stem_conv_bwd_weight_fused" + sfx)
        for k in range(4):
            p = [b["a"], b["w"], b["a"], b["vec"]]
            p[k] = None
            assert fused(*p, b["x"], b["dw"], b["ws"], *shape, st()) == -1, (sfx, k)
        bnapply = getattr(L, "msl_stem_conv_bwd_weight_bnapply" + sfx)
        for k in (1, 2):
            p = [b["a"], b["a"], b["vec"]]
            p[k] = None
            assert bnapply(*p, b["x"], b["dw"], b["ws"], *shape, st()) == -1, (sfx, k)
    assert L.msl_thread_launch_count() == n0, "a refused call launched a kernel"
    torch.cuda.synchronize()
    for k, o in outs.items():
        o.untouched(k)
    assert L.msl_stem_conv_bwd_weight_nslabs(2, *dims, 0, 2, 2) == -1 and L.msl_stem_conv_bwd_weight_nslabs(0, *dims, 2, 2, 2) == -1
