"""Float64 reference of the per-channel backward link (csrc/chanlink.hip), with derived bounds, ``link_plan`` restated and an
fp32 emulation in the kernel's own order.  Plain torch on the CPU; like tests/stem_ref.py nothing here imports the package.

One launch is judged in two stages, each evaluated in float64 on exactly the values the kernel reads.

Stage A (BatchNorm1 + ReLU backward): g, z, vec_z -> dL/dz, dgamma1, dbeta1.
Stage B (transposed depthwise 3x3x3 + head share, BatchNorm2 + ReLU backward, depthwise weight gradient): the dL/dz THE KERNEL
    STORED (read back; bf16 storage: the stored bf16 values), w, y, vec_y, head share -> dL/dy, dw, dgamma2, dbeta2.  The stored
    dL/dz is what the kernel's gather sees (``rounded(g_z, dz)`` goes to LDS), so the bf16 rounding of the intermediate needs no
    model and a stage-A error cannot hide inside a stage-B bound.

Masks.  Both ReLU masks are ``fmaf(x, scale, shift) > 0`` on fp32 vectors handed in by the caller; ``stem_ref.mask32`` reproduces
that bit for bit, so the reference masks ARE the kernel's, no element is excluded and no margin around zero is used.  The
vectors [scale, shift, mean, invstd] are made on the host; the reference does not recompute statistics.  (Vectors given in
float64 - the autograd comparison of the CPU test - take the float64 sign instead.)

Bounds, U = 2**-24, each relative to the sum of the magnitudes of the terms that enter the output.  Counted off the code:

sums (dbeta = sum gm, dgamma = sum gm xhat):  a thread adds its 4 Q elements in fp32 (Q = QO for stage A, QI for stage B:
    n_t = 4 Q <= 16), everything after is float64 (chan_sum2) and cast once; a dgamma term carries three roundings (z - mean,
    * invstd, gm * xhat)  ->  (n_t + 4) U sum |gm|  and  (n_t + 4) U sum |gm xhat|  (tests/bn_ref.py).  They are relative to the
    sums of magnitudes, not to the result: a channel whose sum cancels is judged by what was added, not by what is left.
k1, k2 = (float)(t / count):  the bound of the sum over the count, plus U |k| for the cast  (dc1, dc2).
apply  sc (gm - k1 - xhat k2):  six operations -> 8 U |sc| (|gm| + |k1| + |xhat k2|)  +  |sc| (dc1 + |xhat| dc2).
gather  acc = share + sum_k w[k] dz[(i + 1 - k) / s]:  one fmaf per tap that meets the element, at most K = 27 (stride 1) or
    K = 8 (stride 2: two taps per axis for an odd index, one for an even), the head share is the chain's exact start
    ->  b_acc = (K + 1) U (|share| + sum |w| |dz|).
bf16 storage: the kernel rounds acc to bf16 before the mask (``rounded(g_y, acc)``) and that value is never stored, so it is
    bounded: half a bf16 ulp is at most 2**-8 of the value  ->  b_g = b_acc + 2**-8 (|a| + b_acc), carried through the two sums
    (sum b_g, sum b_g |xhat|) and through scale2 into dL/dy.  fp32 storage: b_g = b_acc.
stage B sums:  sum b_g [mask] + (n_t + 4) U sum (|gm| + b_g)   and the same with |xhat|.
stage B apply: 8 U |sc| (|gm| + b_g + |k1| + |xhat k2|)  +  |sc| (b_g + dc1 + |xhat| dc2).
dw[c][k] = sum_i a[i] dz[(i + 1 - k) / s] with a = relu(fmaf(y, scale2, shift2)) reproduced bit for bit (pw_ref.act32): a
    thread's fmaf chain for one tap has n_w = 4 QI links at stride 1 (four per quad) and 2 at stride 2 (two per tap row, and a
    thread meets a tap row in one of its quads only: link_parity_class); the quarter sums are float64, one cast
    ->  (n_w + 2) U sum |a| |dz|.
Stored bf16 outputs (dL/dz, dL/dy) are judged by the rounding-interval test of tests/bf16pw_ref.py; fp32 ones by the bound.
"""
import torch
import torch.nn.functional as F

from tests import bf16pw_ref as P
from tests.bn_ref import U, _bc, worst  # noqa: F401
from tests.pw_ref import act32, fma32
from tests.stem_ref import mask32

EPS = 1e-5
LDS_CAP = 156 * 1024
UB = 2.0 ** -8  # half a bf16 ulp, relative
KEYS = ("gz", "gy", "dw", "dgam1", "dbet1", "dgam2", "dbet2")


# ------------------------------------------------------------------------------------------------- link_plan, restated
def out_dims(dims, stride):
    return tuple((d - 1) // stride + 1 for d in dims)


def plan(N, dims, stride):
    """link_plan restated -> dict(nw, qo, qi, smem) or None (refused)."""
    D, H, W = dims
    if N <= 0 or D <= 0 or H <= 0 or W <= 0 or stride not in (1, 2):
        return None
    if any(v & (v - 1) for v in dims) or W < 4:
        return None
    OD, OH, OW = out_dims(dims, stride)
    if OW < 4 or (stride == 2 and (D < 2 or H < 2)):
        return None
    tqo, tqi = N * OD * OH * OW // 4, N * D * H * W // 4
    for lim, nw in ((128, 1), (1024, 4), (2048, 8), (4096, 16)):
        if tqi <= lim:
            break
    else:
        return None
    nt = nw * 64
    up = lambda v: 1 if v <= 1 else 2 if v <= 2 else 4
    qi, qo = up(-(-tqi // nt)), up(-(-tqo // nt))
    if qo > 1:
        qo = qi
    if stride == 2 and nw == 1:
        qi = 4
    ptot = N * (OD + 2) * (OH + 2) * (OW + 8)
    smem = max(ptot, 27 * nt + 108) * 4 + 2 * nw * 8
    if smem > LDS_CAP:
        return None
    return dict(nw=nw, qo=qo, qi=qi, smem=smem, tqo=tqo, tqi=tqi)


def config(N, dims, stride):
    p = plan(N, dims, stride)
    return None if p is None else (p["nw"], p["qo"], p["qi"], stride)


CONFIGS = [(1, 1, 1, 1), (1, 2, 2, 1), (4, 1, 1, 1), (4, 2, 2, 1), (4, 4, 4, 1), (8, 4, 4, 1), (16, 4, 4, 1),
           (1, 1, 4, 2), (4, 1, 1, 2), (4, 1, 2, 2), (4, 1, 4, 2), (8, 1, 4, 2), (16, 1, 4, 2)]


# ------------------------------------------------------------------------------------------------- inputs
def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _bn_vec(x, gamma, beta):
    mean = x.mean(dim=(0, 2, 3, 4))
    inv = 1.0 / torch.sqrt(x.var(dim=(0, 2, 3, 4), unbiased=False) + EPS)
    sc = gamma * inv
    return torch.stack([sc, beta - mean * sc, mean, inv])


def chain_case(n, c, dims, stride, acc, seed=0):
    """The construction of tests/test_gpu_chanlink_paths.py::_case: y -> relu(bn2) -> depthwise conv -> z (rounded to fp32) ->
    relu(bn1) -> * G, plus relu(bn2(y)) * Hs.  -> (inp, auto): the fp32 operands the kernel gets (vectors of the batch statistics,
    rounded once; ``vz64`` / ``vy64`` the same in float64) and float64 autograd's gradients."""
    y = rnd(n, c, *dims, seed=seed + 1).double().requires_grad_(True)
    gam2, gam1 = [(torch.rand(c, generator=torch.Generator().manual_seed(seed + 10 + i)) + 0.5).double().requires_grad_(True)
                  for i in range(2)]
    bet2, bet1 = [rnd(c, seed=seed + 20 + i, scale=0.3).double().requires_grad_(True) for i in range(2)]
    w = rnd(c, 1, 3, 3, 3, seed=seed + 3, scale=0.3).double().requires_grad_(True)
    a_prev = torch.relu(F.batch_norm(y, None, None, gam2, bet2, training=True, eps=EPS))
    z = F.conv3d(a_prev, w, stride=stride, padding=1, groups=c)
    z = z + (z.detach().float().double() - z.detach())
    z.retain_grad()
    a = torch.relu(F.batch_norm(z, None, None, gam1, bet1, training=True, eps=EPS))
    G = rnd(*a.shape, seed=seed + 4)
    Hs = rnd(*a_prev.shape, seed=seed + 5) if acc else torch.zeros(a_prev.shape)
    ((a * G.double()).sum() + (a_prev * Hs.double()).sum()).backward()
    vz64 = _bn_vec(z.detach(), gam1.detach(), bet1.detach())
    vy64 = _bn_vec(y.detach(), gam2.detach(), bet2.detach())
    inp = dict(G=G, Hs=Hs, z=z.detach().float(), y=y.detach().float(), w=w.detach().float().view(c, 27),
               vz=vz64.float(), vy=vy64.float(), vz64=vz64, vy64=vy64)
    auto = dict(gz=z.grad, gy=y.grad, dw=w.grad.view(c, 27), dgam1=gam1.grad, dbet1=bet1.grad, dgam2=gam2.grad, dbet2=bet2.grad)
    return inp, auto


def as_bf16(inp):
    """The operands of the bf16 entry point: activations and their gradients rounded to bf16 (held as fp32), the rest kept."""
    return dict(inp, **{k: P.bf16_rne(inp[k]) for k in ("G", "Hs", "z", "y")})


# ------------------------------------------------------------------------------------------------- the two stages
def _mask(x, vec):
    if vec.dtype == torch.float32:
        return mask32(x, vec[0], vec[1])
    return x.double() * _bc(vec[0], x) + _bc(vec[1], x) > 0


def _bn_backward(gm, bgm, x, vec, n_t):
    """gm float64 (masked), bgm its bound (or None: exact) -> the three outputs of a BatchNorm backward and their bounds."""
    red = (0, 2, 3, 4)
    cnt = float(x.numel() // x.shape[1])
    sc, mu, is_ = (_bc(vec[k], x) for k in (0, 2, 3))
    xh = (x.double() - mu) * is_
    zero = torch.zeros_like(gm)
    bgm = zero if bgm is None else bgm
    s, q = gm.sum(red), (gm * xh).sum(red)
    k = (n_t + 4) * U
    bs = bgm.sum(red) + k * (gm.abs() + bgm).sum(red)
    bq = (bgm * xh.abs()).sum(red) + k * ((gm.abs() + bgm) * xh.abs()).sum(red)
    c1, c2 = s / cnt, q / cnt
    dc1, dc2 = bs / cnt + U * c1.abs(), bq / cnt + U * c2.abs()
    t = xh * _bc(c2, x)
    d = sc * (gm - _bc(c1, x) - t)
    bd = 8 * U * sc.abs() * (gm.abs() + bgm + _bc(c1, x).abs() + t.abs()) + sc.abs() * (bgm + _bc(dc1, x) + xh.abs() * _bc(dc2, x))
    return dict(d=d, b_d=bd, dbeta=s, b_dbeta=bs, dgamma=q, b_dgamma=bq)


def stage_a(G, z, vz, qo):
    gm = torch.where(_mask(z, vz), G.double(), torch.zeros((), dtype=torch.float64))
    return _bn_backward(gm, None, z, vz, 4 * qo)


def transposed(dz, w, stride):
    """dL/d input of the depthwise 3x3x3 convolution (padding 1) of even / power-of-two extents: (N, C, OD, OH, OW) float64."""
    c = dz.shape[1]
    return F.conv_transpose3d(dz, w.view(c, 1, 3, 3, 3), stride=stride, padding=1, output_padding=stride - 1, groups=c)


def weight_grad(a, dz, stride):
    """dw[c][k] = sum a[o * s + k - 1] dz[o] -> (C, 27) float64."""
    N, C, OD, OH, OW = dz.shape
    ap = F.pad(a, (1, 1, 1, 1, 1, 1))
    s = stride
    out = [(ap[:, :, kd:kd + s * (OD - 1) + 1:s, kh:kh + s * (OH - 1) + 1:s, kw:kw + s * (OW - 1) + 1:s] * dz).sum((0, 2, 3, 4))
           for kd in range(3) for kh in range(3) for kw in range(3)]
    return torch.stack(out, 1)


def stage_b(dz, w, y, vy, Hs, stride, qi, bf16, a_prev=None):
    """dz: the stored dL/dz (any float dtype holding the stored values); Hs: the head share or None.  ``a_prev``: the block's
    input activation for dw (default: the kernel's own fp32 relu(fmaf(y, scale2, shift2)))."""
    dzd, wd = dz.double(), w.double()
    a = transposed(dzd, wd, stride)
    aabs = transposed(dzd.abs(), wd.abs(), stride)
    if Hs is not None:
        a, aabs = a + Hs.double(), aabs + Hs.double().abs()
    K = 27 if stride == 1 else 8
    bg = (K + 1) * U * aabs
    if bf16:
        bg = bg + UB * (a.abs() + bg)
    m = _mask(y, vy)
    zero = torch.zeros((), dtype=torch.float64)
    out = _bn_backward(torch.where(m, a, zero), torch.where(m, bg, zero), y, vy, 4 * qi)
    if a_prev is None:
        a_prev = act32(y.float().flatten(2), vy[0], vy[1]).view(y.shape)
    n_w = 4 * qi if stride == 1 else 2
    ad = a_prev.double()
    out["dw"] = weight_grad(ad, dzd, stride)
    out["b_dw"] = (n_w + 2) * U * weight_grad(ad.abs(), dzd.abs(), stride)
    return out


def judge(rep, got, inp, N, dims, stride, acc, bf16, with_dw=True):
    """Every output of one launch against the two stages.  ``got``: dict of KEYS (any device), ``rep``: bf16pw_ref.Report."""
    p = plan(N, dims, stride)
    g = {k: (None if v is None else v.detach().cpu().float()) for k, v in got.items()}
    A = stage_a(inp["G"], inp["z"], inp["vz"], p["qo"])
    B = stage_b(g["gz"], inp["w"], inp["y"], inp["vy"], inp["Hs"] if acc else None, stride, p["qi"], bf16)
    for name, key, S in (("dL/dz", "gz", A), ("dL/dy", "gy", B)):
        if bf16:
            rep.interval(name, g[key], S["d"], S["b_d"])
        else:
            rep.bound(name, g[key], S["d"], S["b_d"])
    rep.bound("dbeta1", g["dbet1"], A["dbeta"], A["b_dbeta"])
    rep.bound("dgamma1", g["dgam1"], A["dgamma"], A["b_dgamma"])
    rep.bound("dbeta2", g["dbet2"], B["dbeta"], B["b_dbeta"])
    rep.bound("dgamma2", g["dgam2"], B["dgamma"], B["b_dgamma"])
    if with_dw:
        rep.bound("dw", g["dw"], B["dw"], B["b_dw"])
    return rep


# ================================================================================================= fp32 emulation
MUTATIONS = ("tap_off", "swap_eo_oe", "halo", "wrap_w", "k1_out_count", "drop_head", "masked_contrib", "dw_from_y",
             "unrounded_dz")


def slots(N, dims, stride, p, side):
    """The quads a thread holds -> (idx (Q, NT) int64: quad of the channel's population [n][quad of the image], clamped to a
    valid one as the kernel's addresses are; live (Q, NT) bool).  side 'out': z / g; 'in': y / head share (in_quad)."""
    nt = p["nw"] * 64
    tid = torch.arange(nt)
    if side == "out" or stride == 1:
        Q, tot = (p["qo"], p["tqo"]) if side == "out" else (p["qi"], p["tqi"])
        qi = tid[None, :] + torch.arange(Q)[:, None] * nt
        return qi.clamp_max(tot - 1), qi < tot
    D, H, W = dims
    lD, lH, lW = (v.bit_length() - 1 for v in dims)
    lSi, QI, lnt = lD + lH + lW, p["qi"], nt.bit_length() - 1
    idx, live = [], []
    for q in range(QI):
        cls = torch.full_like(tid, q) if QI == 4 else 2 * q + (tid >> (lnt - 1)) if QI == 2 else tid >> (lnt - 2)
        pa = cls >> 1
        pb = (cls ^ pa) & 1
        rest = tid & ((nt * QI >> 2) - 1)
        x, nn = rest & ((1 << (lSi - 4)) - 1), rest >> (lSi - 4)
        iwq = x & ((1 << (lW - 2)) - 1)
        ih = ((x >> (lW - 2)) & ((1 << (lH - 1)) - 1)) * 2 + pb
        id_ = (x >> (lW + lH - 3)) * 2 + pa
        r = (((id_ << lH) + ih) << (lW - 2)) + iwq
        idx.append((nn.clamp_max(N - 1) << (lSi - 2)) + r)
        live.append(nn < N)
    return torch.stack(idx), torch.stack(live)


def _to_slots(t, idx):
    """(N, C, ...) -> (C, Q, NT, 4)"""
    C = t.shape[1]
    return t.transpose(0, 1).reshape(C, -1, 4)[:, idx]


def _from_slots(v, idx, live, shape):
    """(C, Q, NT, 4) -> (N, C, ...); every quad is held by exactly one live slot (asserted in the CPU test)."""
    N, C = shape[:2]
    D, H, W = shape[2:]
    out = torch.full((C, N * D * H * W // 4, 4), float("nan"))
    out[:, idx[live]] = v[:, live]
    return out.view((C, N) + tuple(shape[2:])).transpose(0, 1).contiguous()


def _thread_sums(t, live):
    """fp32 terms (C, Q, NT, 4) -> float64 (C,): a thread adds its elements in fp32 (q, then e), the threads meet in double."""
    acc = torch.zeros((t.shape[0], t.shape[2]))
    for q in range(t.shape[1]):
        for e in range(4):
            acc = acc + torch.where(live[q], t[:, q, :, e], torch.zeros(()))
    return acc.double().sum(-1)


def _link_bn(gq, xq, vec, live, cnt, masked_contrib):
    """One BatchNorm + ReLU backward in slot layout, fp32 -> (d (C, Q, NT, 4), dgamma, dbeta)."""
    sc, sh, mu, is_ = (vec[k].float().view(-1, 1, 1, 1) for k in range(4))
    lv = live[None, :, :, None]
    m = fma32(xq, sc, sh) > 0
    gm = torch.where(m if masked_contrib else (m & lv), gq, torch.zeros(()))
    xh = (xq - mu) * is_
    every = torch.ones_like(live)
    t1, t2 = _thread_sums(gm, every), _thread_sums(gm * xh, every)
    k1, k2 = (t1 / cnt).float().view(-1, 1, 1, 1), (t2 / cnt).float().view(-1, 1, 1, 1)
    return sc * (gm - k1 - xh * k2), t2.float(), t1.float()


def _axis(ext, k, s):
    t = torch.arange(ext) + 1 - k
    return torch.div(t, s, rounding_mode="floor") + 1, t % s == 0


def gather_terms(dz, dims, stride, mut=None):
    """The stored dL/dz (N, C, OD, OH, OW) fp32 -> [(k, term (N, C, D, H, W))] in the kernel's order (kd, kh ascending, kw
    descending): the value tap k multiplies at every input element, zero where the tap does not meet it (an fmaf with a zero
    operand leaves the accumulator as it is)."""
    D, H, W = dims
    OD, OH, OW = dz.shape[2:]
    dzp = F.pad(dz, (1, 1, 1, 1, 1, 1))
    if mut == "halo":
        dzp[:, :, OD + 1, 1, 1] = 1.0
    if mut == "wrap_w":  # a pitch without halo columns: column -1 is the row before, column OW the row after
        src = dzp.clone()
        dzp[:, :, :, 1:, 0] = src[:, :, :, :-1, OW]
        dzp[:, :, :, :-1, OW + 1] = src[:, :, :, 1:, 1]
    par = lambda ext: torch.arange(ext) & 1
    out = []
    for kd in range(3):
        for kh in range(3):
            id_, vd = _axis(D, kd, stride)
            ih, vh = _axis(H, kh, stride)
            vdh = vd[:, None] & vh[None, :]
            if stride == 2 and mut == "tap_off" and (kd, kh) == (2, 2):  # class oo's last tap row, one LDS row too low
                ih = (ih - 1).clamp_min(0)
            if stride == 2 and mut == "swap_eo_oe" and (kd, kh) in ((0, 1), (2, 1)):  # oe's rows, run by the eo quads
                vdh = (par(D) == 0)[:, None] & (par(H) == 1)[None, :]
                id_, ih = (torch.arange(D) >> 1) + (1 if kd == 0 else 0) + 1, (torch.arange(H) >> 1) + 1
            if stride == 2 and mut == "swap_eo_oe" and (kd, kh) in ((1, 0), (1, 2)):  # eo's rows, run by the oe quads
                vdh = (par(D) == 1)[:, None] & (par(H) == 0)[None, :]
                id_, ih = (torch.arange(D) >> 1) + 1, (torch.arange(H) >> 1) + (1 if kh == 0 else 0) + 1
            rows = dzp[:, :, id_][:, :, :, ih]
            for kw in (2, 1, 0):
                iw, vw = _axis(W, kw, stride)
                valid = vdh[:, :, None] & vw[None, None, :]
                out.append((kd * 9 + kh * 3 + kw, torch.where(valid, rows[..., iw], torch.zeros(()))))
    return out


def emul(inp, N, dims, stride, acc, bf16=False, with_dw=True, mut=None):
    """The link in fp32, in the kernel's order: thread partials of the sums and of the tap gradients in fp32 (fmaf chains:
    pw_ref.fma32), combined in float64.  ``inp`` as the entry point gets it (bf16: as_bf16).  -> dict of KEYS (fp32 tensors; with
    bf16 storage dL/dz and dL/dy hold bf16 values).  ``mut``: one of MUTATIONS, a kernel that is wrong in one place."""
    assert mut is None or mut in MUTATIONS
    p = plan(N, dims, stride)
    C = inp["z"].shape[1]
    st = P.bf16_rne if bf16 else (lambda t: t)
    mc = mut == "masked_contrib"
    # ---- stage A
    io, lo = slots(N, dims, stride, p, "out")
    d, dgam1, dbet1 = _link_bn(_to_slots(inp["G"], io), _to_slots(inp["z"], io), inp["vz"], lo, float(p["tqo"] * 4), mc)
    dz = _from_slots(d, io, lo, inp["z"].shape)
    gz = st(dz)
    # ---- stage B
    terms = gather_terms(dz if mut == "unrounded_dz" else gz, dims, stride, mut)
    a = inp["Hs"].clone() if (acc and mut != "drop_head") else torch.zeros(inp["y"].shape)
    for k, t in terms:
        a = fma32(inp["w"][:, k].view(1, C, 1, 1, 1), t, a)
    a = st(a)
    ii, li = slots(N, dims, stride, p, "in")
    yq = _to_slots(inp["y"], ii)
    cnt = float((p["tqo"] if mut == "k1_out_count" else p["tqi"]) * 4)
    d, dgam2, dbet2 = _link_bn(_to_slots(a, ii), yq, inp["vy"], li, cnt, mc)
    gy = st(_from_slots(d, ii, li, inp["y"].shape))
    dw = None
    if with_dw:
        sc, sh = inp["vy"][0].view(-1, 1, 1, 1), inp["vy"][1].view(-1, 1, 1, 1)
        v = fma32(yq, sc, sh)
        av = yq if mut == "dw_from_y" else torch.where(v < 0, torch.zeros_like(v), v)
        av = torch.where(li[None, :, :, None], av, torch.zeros(()))
        order = sorted(terms, key=lambda kt: kt[0])
        tq = torch.stack([_to_slots(t, ii) for _, t in order])  # (27, C, Q, NT, 4)
        dd = torch.zeros((27, C, tq.shape[3]))
        for q in range(tq.shape[2]):
            for e in (3, 2, 1, 0):
                dd = fma32(av[None, :, q, :, e], tq[:, :, q, :, e], dd)
        dw = dd.double().sum(-1).float().t().contiguous()
    return dict(gz=gz, gy=gy, dw=dw, dgam1=dgam1, dbet1=dbet1, dgam2=dgam2, dbet2=dbet2)
