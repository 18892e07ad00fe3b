"""tests/stem_ref.py checked without a GPU: the float64 references against float64 autograd, the transposed depthwise
convolution as the adjoint of the stride-2 one, the mask rule, the restated dispatch against the case tables and the library's
own counts, and - the proof that the bounds are neither vacuous nor violated by honest arithmetic - an fp32 CPU emulation of
every accumulation order (pw_ref.fma32 chains in the kernels' k order, the waves' LDS fold, msl::reduce_slabs_256) inside every
bound at every case shape of tests/test_gpu_stem.py.  No element is skipped anywhere."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mslesions3d_amd import _lib
from tests import stem_cases as C
from tests import stem_ref as S
from tests.bf16_emul import bf


def gen(seed):
    return torch.Generator().manual_seed(seed)


def _ratio(got32, ref, bound):
    r, _, bad = S.worst(got32, ref, bound)
    return r, bad


SUB = [0, 13, 31]  # output channels the emulations follow where all 32 would take long: every bound is per element


# ------------------------------------------------------------------------------------------------- the references themselves
@pytest.mark.parametrize("cin,dims,stride", [(3, (5, 6, 9), (2, 2, 2)), (2, (4, 7, 8), (1, 2, 2)), (1, (3, 1, 6), (2, 1, 1))])
def test_refs_match_float64_autograd(cin, dims, stride):
    g = gen(3)
    x = torch.randn((2, cin) + dims, generator=g)
    w = torch.randn((32, cin, 3, 3, 3), generator=g)
    wd = w.double().requires_grad_(True)
    y = F.conv3d(x.double(), wd, stride=stride, padding=1)
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy.double())
    tol = dict(rtol=0, atol=1e-11)
    yr, ya = S.fwd_ref(x, w, stride)
    cols = S.im2col(x.double(), stride)
    assert tuple(yr.shape[2:]) == S.out_dims(dims, stride)
    assert torch.allclose(torch.matmul(w.double().view(32, -1), cols).view(yr.shape), yr, **tol), "im2col is not conv3d's"
    assert bool((ya >= yr.abs() - 1e-11).all())
    dw, da = S.bww_ref(dy.flatten(2), cols)
    assert torch.allclose(dw.view(wd.shape), wd.grad, **tol) and bool((da >= dw.abs() - 1e-11).all())


@pytest.mark.parametrize("odims", [(5, 6, 7), (6, 5, 8), (1, 2, 3), (2, 1, 1)])
def test_dwconv_t_is_the_adjoint_of_the_stride2_depthwise_convolution(odims):
    g = gen(4)
    a = torch.randn((2, 32) + odims, generator=g, dtype=torch.float64).requires_grad_(True)
    w1 = torch.randn((32, 1, 3, 3, 3), generator=g, dtype=torch.float64)
    z = F.conv3d(a, w1, stride=2, padding=1, groups=32)
    assert tuple(z.shape[2:]) == S.half_dims(odims)
    dz = torch.randn(z.shape, generator=g, dtype=torch.float64)
    z.backward(dz)
    gt = S.dwconv_t(dz, w1, odims)
    assert gt.shape == a.shape and torch.allclose(gt, a.grad, rtol=0, atol=1e-12)
    assert abs(float((z.detach() * dz).sum() - (a.detach() * gt).sum())) < 1e-9


def test_mask_rule_is_relu_of_the_batchnorm_affine():
    g = gen(5)
    y = torch.randn((2, 32, 3, 4, 5), generator=g) * 1.5 + 0.3
    sc, sf = torch.rand(32, generator=g) + 0.5, torch.randn(32, generator=g) * 0.3
    y[0, :, 0, 0, 0], sc[:4], sf[:4] = 1.0, 1.0, -1.0           # pre-activation exactly 0: not > 0
    y[0, 4:8, 0, 0, 1] = torch.tensor(1.0) + 2.0 ** -23       # and one ulp above: > 0 in fp32 only through the fma's single rounding
    sc[4:8], sf[4:8] = 1.0 - 2.0 ** -24, -1.0
    m = S.mask32(y, sc, sf)
    pre = y.double() * sc.double().view(1, -1, 1, 1, 1) + sf.double().view(1, -1, 1, 1, 1)
    assert torch.equal(m, torch.relu(pre) > 0)
    assert not bool(m[0, :4, 0, 0, 0].any()) and bool(m[0, 4:8, 0, 0, 1].all())
    # the operand of MODE 1 is tests/bn_ref.py's dL/dy on the same vectors
    from tests import bn_ref as R
    gr = torch.randn(y.shape, generator=g)
    vec = S.host_vec(gr, y, torch.ones(32), torch.zeros(32), 6)
    a, _ = S.mode1_operand(gr, y, vec)
    assert torch.allclose(a, R.bwd_apply_ref(gr, y, vec, vec[4], vec[5]), rtol=0, atol=1e-12)


def test_mode2_operand_is_the_batchnorm_backward_of_the_rebuilt_gradient():
    """scale gm + (cC y + cE) with the float64 coefficients == scale (gm - c1 - xhat c2): what MODE 2 folds."""
    from tests import bn_ref as R
    g = gen(6)
    y = torch.randn((2, 32, 5, 6, 7), generator=g) * 1.5 + 0.3
    dz = torch.randn((2, 32, 3, 3, 4), generator=g)
    w1 = torch.randn((32, 1, 3, 3, 3), generator=g) * 0.4
    gam, bet = torch.rand(32, generator=g) + 0.5, torch.randn(32, generator=g) * 0.3
    g64 = S.dwconv_t(dz.double(), w1.double(), (5, 6, 7))
    vec = S.host_vec(g64, y, gam, bet, 8)
    a, ab, gg, gabs = S.mode2_operand(dz, w1, y, vec)
    assert torch.equal(gg, g64) and bool((gabs >= gg.abs() - 1e-12).all())
    want = R.bwd_apply_ref(g64, y, vec, vec[4], vec[5])
    assert bool((ab > 0).all()) and torch.allclose(a, want, rtol=0, atol=1e-5)  # c1, c2, cC, cE are each rounded to fp32 once


# ------------------------------------------------------------------------------------------------- dispatch
def _id_parts(path):
    head = path.split(":")[0]
    return head[:head.index("<")], int(head[head.index("<") + 1:-1]), "iters2" in path


@pytest.mark.parametrize("case", C.FWD_CASES, ids=[c[0] for c in C.FWD_CASES])
def test_fwd_case_reaches_the_kernel_its_id_names(case):
    path, N, cin, dims, stride = case
    kernel, c, two = _id_parts(path)
    plan = S.fwd_plan(cin, dims, stride)
    assert (plan["kernel"], cin) == (kernel, c) and plan["iters"] == (2 if two else 1)
    if "rows-by-shape" in path:
        assert plan["rows_by_shape"] and plan["kernel"] == "mfma"
    od, oh, ow = S.out_dims(dims, stride)
    assert _lib.load().msl_stem_conv_fwd_num_partials(N, od, oh, ow) == N * plan["nb"]
    if two:  # the walk crosses rows and planes, and some wave ends on dead chunks
        assert plan["chunks_per_n"] % 2 == 1 and plan["nb"] * 8 > plan["chunks_per_n"] > plan["nb"] * 4


@pytest.mark.parametrize("case", C.BWW_CASES + C.TILE_CASES, ids=[c[0] for c in C.BWW_CASES + C.TILE_CASES])
def test_bww_case_reaches_the_kernel_its_id_names(case):
    path, N, cin, dims, stride = case
    kernel, c, two = _id_parts(path)
    fused = S.bww_plan(N, cin, dims, stride, True)
    plain = S.bww_plan(N, cin, dims, stride, False)
    assert (fused["kernel"], cin) == (kernel, c) and plain["kernel"] == "wave"
    assert fused["iters"] == (2 if two else 1)
    if kernel == "wave":
        assert plain["iters"] == fused["iters"]
    if "remap-on" in path:
        assert fused["remap"]
    if "remap-off" in path:
        assert not fused["remap"]
    if "tile-by-shape" in path:
        assert fused["tile_by_shape"] and cin > 2
    if path == "wave<3>:3x4x128-OW64":
        assert not fused["tile_by_shape"]
    ns = _lib.load().msl_stem_conv_bwd_weight_nslabs(N, *dims, *stride)
    assert ns == fused["ns"] == plain["ns"]
    if two:
        assert fused["total"] > fused["ns"] * (4 if kernel == "wave" else 1)
    assert all(p in [c[0] for c in C.BWW_CASES + C.TILE_CASES] for p in C.DEFERRED)


# ------------------------------------------------------------------------------------------------- honest fp32: forward
@pytest.mark.parametrize("case", C.FWD_CASES, ids=[c[0] for c in C.FWD_CASES])
def test_fp32_forward_inside_bound(case):
    _, N, cin, dims, stride = case
    g = gen(7 + cin + sum(dims))
    x = torch.randn((N, cin) + dims, generator=g)
    w = torch.randn((32, cin, 3, 3, 3), generator=g) * 0.3
    yr, absdot = S.fwd_ref(x, w, stride)
    cols = S.im2col(x, stride)
    K, OS = cin * 27, cols.shape[2]
    co = list(range(32)) if N * OS * 32 * K < 2e7 else SUB
    wk = w.view(32, K)[co]
    acc = torch.zeros((N, len(co), OS))
    for k in range(K):  # the MFMA chain: k ascending (the padding step of an odd K multiplies zeros)
        acc = S.fma32(wk[:, k].view(1, -1, 1), cols[:, k:k + 1], acc)
    assert acc.dtype == torch.float32
    yb = S.fwd_bound(absdot, cin)[:, co].flatten(2)
    r, bad = _ratio(acc, yr[:, co].flatten(2), yb)
    assert bad == 0 and 0 < r <= 1, r
    # statistics in the kernels' order: wave j of an image walks chunks [j * iters, (j + 1) * iters) = 2 * iters tiles of 32
    # columns; a lane adds its column of every tile (the square inside an fma), the 32 lanes meet in a 5-level tree, then double
    plan = S.fwd_plan(cin, dims, stride)
    od, oh, ow = S.out_dims(dims, stride)
    it, cpr, cpn = plan["iters"], plan["chunks_per_row"], plan["chunks_per_n"]
    nw = S.cdiv(cpn, it)
    t = F.pad(acc.view(N, len(co), od * oh, ow), (0, cpr * 64 - ow)).reshape(N, len(co), cpn, 2, 32)
    t = F.pad(t, (0, 0, 0, 0, 0, nw * it - cpn)).reshape(N, len(co), nw, 2 * it, 32)
    s, q = torch.zeros((N, len(co), nw, 32)), torch.zeros((N, len(co), nw, 32))
    for j in range(2 * it):
        s = s + t[:, :, :, j]
        q = S.fma32(t[:, :, :, j], t[:, :, :, j], q)
    for m in (16, 8, 4, 2, 1):
        s, q = s[..., :m] + s[..., m:2 * m], q[..., :m] + q[..., m:2 * m]
    assert s.dtype == torch.float32 and q.dtype == torch.float32
    got = torch.stack([s[..., 0].double().sum((0, 2)), q[..., 0].double().sum((0, 2))])
    own, ob = S.stats_own_ref(acc, it)
    r, bad = _ratio(got, own, ob)
    assert bad == 0, r
    tot, tb = S.stats_total_ref(yr[:, co].flatten(2), yb)
    r, bad = _ratio(got, tot, tb + ob)
    assert bad == 0, r


# ------------------------------------------------------------------------------------------------- honest fp32: weight gradient
def wave_positions(N, dims, stride, plan, fused):
    """The walk of the gradient kernels restated: -> int64 (ns, 4, Lmax), the flat output positions (n * OS + o) wave wv of
    workgroup b contracts, in its accumulator's order, dead positions dropped (they add exact zeros), -1 padded."""
    OD, OH, OW = S.out_dims(dims, stride)
    OS = OD * OH * OW
    ns, iters = plan["ns"], plan["iters"]
    lists = [[[] for _ in range(4)] for _ in range(ns)]
    for b in range(ns):
        lb = S.xcd_block(b, ns, plan["remap"])
        for it in range(iters):
            if plan["kernel"] == "tile":
                T = lb * iters + it
                if T >= plan["total"]:
                    continue
                gpc = OH // 8
                g4, q = T % gpc, T // gpc
                p, q = q & 1, q >> 1
                od, n = q % OD, q // OD
                order = np.array([8 * qq + j + 4 * h for qq in range(8) for j in range(4) for h in range(2)])
                for wv in range(4):
                    lists[b][wv].append(n * OS + (od * OH + p + 2 * (4 * g4 + wv)) * OW + order)
            else:
                for wv in range(4):
                    chunk = (lb * 4 + wv) * iters + it if fused else (b * iters + it) * 4 + wv
                    if chunk >= plan["total"]:
                        continue
                    cpr = plan["chunks_per_row"]
                    seg, r = chunk % cpr, chunk // cpr
                    oh, r = r % OH, r // OH
                    od, n = r % OD, r // OD
                    lists[b][wv].append(n * OS + (od * OH + oh) * OW + seg * 64 + np.arange(min(64, OW - seg * 64)))
    flat = [[np.concatenate(l) if l else np.zeros(0, dtype=np.int64) for l in row] for row in lists]
    Lmax = max(len(a) for row in flat for a in row)
    assert Lmax <= 64 * iters
    pos = np.full((ns, 4, Lmax), -1, dtype=np.int64)
    for b in range(ns):
        for wv in range(4):
            pos[b, wv, :len(flat[b][wv])] = flat[b][wv]
    live = np.sort(pos[pos >= 0])
    assert np.array_equal(live, np.arange(N * OS)), "the restated walk does not visit every output position exactly once"
    return torch.from_numpy(pos)


def emulate_bww(a32, cols32, pos):
    """a32 (N, C, OS) fp32, cols32 (N, K, OS) fp32, pos (ns, 4, L) -> (C, K) fp32: per wave an fmaf chain over its positions, the
    four waves of a workgroup folded as the kernels do in LDS ((w3 + w2) + w1, then w0 + that), the slabs as
    msl::reduce_slabs_256 (thread group g adds slabs g, g + 8, ...; the 8 group sums are added in order)."""
    N, Cc, OS = a32.shape
    K = cols32.shape[1]
    ns, _, Lm = pos.shape
    idx = torch.where(pos < 0, torch.full_like(pos, N * OS), pos)
    af = F.pad(a32.permute(1, 0, 2).reshape(Cc, N * OS), (0, 1))[:, idx]       # (C, ns, 4, L)
    bfl = F.pad(cols32.permute(1, 0, 2).reshape(K, N * OS), (0, 1))[:, idx]    # (K, ns, 4, L)
    acc = torch.zeros((ns, 4, Cc, K))
    for l in range(Lm):
        acc = S.fma32(af[..., l].permute(1, 2, 0).unsqueeze(-1), bfl[..., l].permute(1, 2, 0).unsqueeze(-2), acc)
    red = acc[:, 3] + acc[:, 2]
    red = red + acc[:, 1]
    slab = acc[:, 0] + red
    groups = []
    for gI in range(8):
        s = torch.zeros((Cc, K))
        for k in range(gI, ns, 8):
            s = s + slab[k]
        groups.append(s)
    t = torch.zeros((Cc, K))
    for s in groups:
        t = t + s
    assert t.dtype == torch.float32
    return t


def bww_data(N, cin, dims, stride):
    g = gen(11 + cin + sum(dims))
    odims = S.out_dims(dims, stride)
    return dict(x=torch.randn((N, cin) + dims, generator=g), dy=torch.randn((N, 32) + odims, generator=g),
                y=torch.randn((N, 32) + odims, generator=g) * 1.5 + 0.3, dz=torch.randn((N, 32) + S.half_dims(odims), generator=g),
                w1=torch.randn((32, 1, 3, 3, 3), generator=g) * 0.4, gamma=torch.rand(32, generator=g) + 0.5,
                beta=torch.randn(32, generator=g) * 0.3)


def operands(d, mode, b16, odims):
    """-> (a float64, its bound or None, a32: the same operand in honest fp32 arithmetic).  a32 takes nothing from stem_ref but
    the caller's vectors: its mask is relu(fmaf(y, scale, shift)) > 0 and its rebuilt gradient is fp32 autograd through the
    stride-2 depthwise convolution, so a reference whose mask or transposed convolution is off by a voxel fails here."""
    r = bf if b16 else (lambda t: t)
    v = lambda row: row.view(1, -1, 1, 1, 1)
    relu_mask = lambda yq, vec: torch.relu(S.fma32(yq, v(vec[0]).expand_as(yq), v(vec[1]).expand_as(yq))) > 0
    if mode == 0:
        return d["dy"].double(), None, d["dy"]
    if mode == 1:
        gq, yq = r(d["dy"]), r(d["y"])
        vec = S.host_vec(gq, yq, d["gamma"], d["beta"], 6)
        a, ab = S.mode1_operand(gq, yq, vec)
        gm = torch.where(relu_mask(yq, vec), gq, torch.zeros(()))
        a32 = v(vec[0]) * (gm - v(vec[4]) - ((yq - v(vec[2])) * v(vec[3])) * v(vec[5]))  # the kernel's expression, every op rounded
        return a, ab, a32
    zq, yq = r(d["dz"]), r(d["y"])
    g64 = S.dwconv_t(zq.double(), d["w1"].double(), odims)
    vec = S.host_vec(g64, yq, d["gamma"], d["beta"], 8)
    a, ab, _, _ = S.mode2_operand(zq, d["w1"], yq, vec)
    act = torch.zeros_like(yq).requires_grad_(True)  # torch's fp32 backward-data: at most 8 terms per voxel, in its own order
    g32, = torch.autograd.grad(F.conv3d(act, d["w1"], stride=2, padding=1, groups=32), act, zq)
    gm = torch.where(relu_mask(yq, vec), g32, torch.zeros(()))
    a32 = S.fma32(v(vec[0]).expand_as(gm), gm, S.fma32(v(vec[6]).expand_as(yq), yq, v(vec[7]).expand_as(yq)))
    return a, ab, a32


ALL_MODES = ((0, False), (1, False), (2, False), (1, True), (2, True))
_BWW = [(c, ALL_MODES) for c in C.BWW_CASES] + [(c, ((2, False), (2, True))) for c in C.TILE_CASES]


@pytest.mark.parametrize("case,modes", _BWW, ids=[c[0][0] for c in _BWW])
def test_fp32_weight_gradient_inside_bound(case, modes):
    _, N, cin, dims, stride = case
    d = bww_data(N, cin, dims, stride)
    odims = S.out_dims(dims, stride)
    cols = S.im2col(d["x"].double(), stride)
    cols32 = cols.float()
    walks = {}
    for mode, b16 in modes:
        fused = mode == 2
        plan = S.bww_plan(N, cin, dims, stride, fused)
        if fused not in walks:
            walks[fused] = wave_positions(N, dims, stride, plan, fused)
        a, ab, a32 = operands(d, mode, b16, odims)
        assert a32.dtype == torch.float32
        fl = lambda t: t.flatten(2)
        ref, _ = S.bww_ref(fl(a), cols)
        bound = S.bww_bound(fl(a), None if ab is None else fl(ab), cols, plan)
        if ab is not None:  # the fp32 operand itself inside the operand bound, every element
            r, bad = _ratio(a32, a, ab)
            assert bad == 0 and 0 < r <= 1, (mode, b16, r)
        got = emulate_bww(fl(a32)[:, SUB], cols32, walks[fused])
        r, bad = _ratio(got, ref[SUB], bound[SUB])
        assert bad == 0 and 0 < r <= 1, (mode, b16, r)
