"""Float64 reference of the detection-head kernels (csrc/heads.hip), a plain-Python mirror of their launch plans, the error
bounds, the checkers and an fp32 emulation with thirteen wrong kernels.  Plain torch on the CPU; nothing here imports the
package.  The same checkers judge the GPU outputs (tests/test_gpu_heads.py) and, on the CPU, the honest emulation and the wrong
kernels (tests/test_heads_ref_cpu.py).

Plan mirror.  ``head_mt``, ``head_lds_w``, ``head_fwd_lds_bw``, ``head_ksg``, ``head_fwd_ksg``, ``head_bw_plan`` are the
functions of the same names in heads.hip line for line, ``plan`` adds the gy / cts / grid arithmetic of head_bwd_data_impl.  The
CPU test holds ``fwd_workspace_bytes``, ``bww_nslabs`` and ``bww_workspace_bytes`` against the library's three host-only queries
(every case and a sweep of shapes): a threshold moved in the library moves a case to another route and fails there.

Reference.  float64 conv3d and float64 autograd (``reference``) on the exact values a kernel reads: on the bf16 entries the
bf16-rounded activations (forward and weight gradient) and the bf16-rounded weights (forward).

Bound, per output element:   B = K[q] * 2**-24 * sum|term|
with sum|term| the same float64 convolution / autograd of the absolute operands (|a| with |w| plus |bias| forward, |dO| with |w|
for bwd-data, |dO| with |a| for the weight and |dO| alone for the bias gradient).  The number of terms n is 27 C forward,
27 * 16 MT for bwd-data and N S for the two gradients.  K is not derived from n: it is MEASURED against the honest fp32
emulation below (``emulate`` without a mutant: the kernels' coarse order - forward one 4-channel k-step per tap and channel
group in sequence, the K slabs folded in order, bias last; weight gradient one partial per position block, the slabs folded in
the order of the reduction), on the CPU, over the whole case table of tests/heads_cases.py, as the largest
|emulation - reference| / (2**-24 sum|term|), and then given a margin of x 4: the MFMA's internal order and the chain splits
(even / odd taps, two wave halves) are not emulated bit for bit, and x 4 covers any reassociation of a sum whose error grows
like sqrt(n).  The error of a sum of n signed terms relative to sum|term| does not grow with n (each partial sum is ~ sqrt(i) terms
large, the sum of their roundings ~ n / sqrt(2) ulps of a term), so one K per quantity serves n = 432 .. 8448:

    quantity   entries                              n in the table     measured max    K
    fwd        msl_head_conv_fwd                    432 .. 6912        3.11            14
    fwd_bf16   msl_head_conv_fwd_bf16               864 .. 3456        1.13            6
    bwd_data   msl_head_conv_bwd_data[_bf16]        432, 864           3.11            14
    dw         msl_head_conv_bwd_weight[_bf16]      1 .. 8448          5.24            24
    db         the same, bias rows                  1 .. 8448          0.65            4

(the maxima are over every element of every case, up to 5e5 of them, which is why they sit well above the typical 0.3; K is
4 x the maximum rounded up to the next even integer with a few percent to spare, because the emulation's own einsum / matmul
order moves the maximum by that much with the host's vector width and thread count.  tests/test_heads_ref_cpu.py prints the
ratios error / B of the honest emulation and holds every one below 1 / 4.)  The
GPU is never the source of a bound.

bf16 output (msl_head_conv_bwd_data_bf16): the rounding-interval test of tests/bf16pw_ref.py - the stored value must be
bf16_rne of some fp32 value inside [ref - B, ref + B], i.e. half a bf16 ulp on top of B, and one further ulp exactly where that
interval straddles a rounding boundary.  An element whose interval is a single bf16 value is "pinned"; only there is the
rounding mode itself tested, so the share of elements that are NOT pinned is capped: UNPINNED_CAP = 0.05 at every case, from
the reference alone (a condition on the inputs, not a measurement of a kernel: B is a few 1e-5 of a typical value, a bf16 ulp
4e-3 to 8e-3 of it, so about two elements in a hundred straddle; the CPU test prints the share of every case).

Wrong kernels (``MUTANTS``): each must be rejected at every case where it can be expressed (``applicable``).
"""
import torch
import torch.nn.functional as F

from tests import bf16pw_ref as B16
from tests.bf16pw_ref import bf16_rne

U = 2.0 ** -24
NAN = float("nan")
HEAD_FWD_CH = 16
HEAD_BWW_SB = 4
TARGET = 256  # workgroups a launch aims for (head_fwd_ksg, head_bw_plan, head_bwd_data_impl)
GR_FEW = 16   # msl_grad_reduce_batch: at most this many slabs are folded in slab order

K = dict(fwd=14.0, fwd_bf16=6.0, bwd_data=14.0, dw=24.0, db=4.0)
UNPINNED_CAP = 0.05

ENTRIES = ("fwd", "fwd_bf16", "bwd_data", "bwd_data_bf16", "bww", "bww_bf16", "pack")
MUTANTS = ("drop_tap", "swap_hw", "unflipped", "halo_origin", "bias_per_slab", "last_slab", "row12", "anchor_stride", "tail_tile",
           "clamp_counted", "bias_one_block", "ragged_group", "pad_rows")


def cdiv(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------------------------------------- the plan mirror (heads.hip)
def head_mt(ncls):
    return (12 + 2 * ncls + 15) // 16


def head_lds_w(C, D, H, W, MT=1):
    if MT != 1 or H != W or C % 16 != 0 or (D * H * W) % 64 != 0:
        return 0
    if W in (16, 8):
        return W
    if W == 4 and D % 4 == 0:
        return 4
    return 0


def head_fwd_lds_bw(N, C, D, H, W, MT=1):
    if MT != 1 or C % HEAD_FWD_CH != 0:
        return 0
    cubic = head_lds_w(C, D, H, W, MT)
    if cubic:
        return cubic
    if N * D * H * W // 64 >= 512:
        return 0
    if W % 4 == 0 and H % 4 == 0 and D % 4 == 0:
        return 4
    if W % 16 == 0 and H % 4 == 0:
        return 16
    if W % 8 == 0 and H % 8 == 0:
        return 8
    return 0


def head_ksg(N, C, S):
    blocks, ksg = cdiv(S, 32) * N, 1
    while blocks * ksg < 256 and C // (4 * ksg * 2) >= 4 and C % (4 * ksg * 2 * 4) == 0:
        ksg *= 2
    return ksg


def head_fwd_ksg(N, C, D, H, W, MT):
    S = D * H * W
    if head_fwd_lds_bw(N, C, D, H, W, MT):
        blocks, ksg = N * (S // 64), 1
        while blocks * ksg < TARGET and C // (ksg * 2) >= HEAD_FWD_CH and (C // (ksg * 2)) % HEAD_FWD_CH == 0:
            ksg *= 2
        return ksg
    return head_ksg(N, C, S)


def head_bw_plan(N, C, D, H, W, MT):
    S, tiles = D * H * W, (C // 16) * 3
    lds_w = head_lds_w(C, D, H, W, MT)
    want_blocks = max(1, TARGET // tiles)
    if lds_w:
        total = N * (S // 64)
        bpw = cdiv(total, min(want_blocks, total))
        return dict(lds_w=lds_w, steps=0, nblocks=cdiv(total, bpw), bpw=bpw)
    total_steps = cdiv(N * S, 4)
    steps = max(8, cdiv(total_steps, want_blocks * 4))
    return dict(lds_w=0, steps=steps, nblocks=cdiv(total_steps, steps * 4), bpw=0)


def plan(N, C, dims, ncls):
    """-> dict(fwd, bwd_data, bww): the kernel every fp32 entry launches for this shape and its tiling."""
    D, H, W = dims
    S, MT = D * H * W, head_mt(ncls)
    lw, cub = head_fwd_lds_bw(N, C, D, H, W, MT), head_lds_w(C, D, H, W, MT)
    fwd = dict(kernel=f"lds{lw}" if lw else "reg", cubic=bool(lw and cub), ksg=head_fwd_ksg(N, C, D, H, W, MT))
    if cub:
        blocks, ctiles = N * (S // 64), C // 16
        gy = max(1, min(ctiles, TARGET // blocks))
        cts = cdiv(ctiles, gy)
        bwd = dict(kernel=f"lds{cub}", cts=cts, groups=cdiv(ctiles, cts), ragged=ctiles % cts != 0)
    else:  # a workgroup of four waves, one 16-channel tile each
        bwd = dict(kernel="reg", cts=4, groups=cdiv(C, 64), ragged=C % 64 != 0)
    p = head_bw_plan(N, C, D, H, W, MT)
    if p["lds_w"]:
        bww = dict(kernel=f"lds{p['lds_w']}", nblocks=p["nblocks"], bpw=p["bpw"], ragged=(N * (S // 64)) % p["bpw"] != 0,
                   block=64 * p["bpw"])
    else:  # four waves of `steps` k-steps of four positions; positions at or above N S are clamped and must count as zero
        span = 4 * p["steps"]
        bww = dict(kernel="reg", nblocks=p["nblocks"], steps=p["steps"], ragged=p["nblocks"] * 4 * span != N * S, block=4 * span,
                   dead_waves=(p["nblocks"] * 4 * span - N * S) // span)
    return dict(fwd=fwd, bwd_data=bwd, bww=bww, MT=MT)


def route_name(p):
    """The string a case id starts with: "<fwd>/<bwd-data>/<weight gradient>"."""
    f, b, w = p["fwd"], p["bwd_data"], p["bww"]
    fs = f"{f['kernel']}{'c' if f['cubic'] else 't' if f['kernel'] != 'reg' else ''}.k{f['ksg']}.m{p['MT']}"
    bs = f"{b['kernel']}.c{b['cts']}x{b['groups']}{'r' if b['ragged'] else ''}"
    ws = f"{w['kernel']}.{'s%d' % w['steps'] if w['kernel'] == 'reg' else 'b%d' % w['bpw']}x{w['nblocks']}{'r' if w['ragged'] else ''}"
    return f"{fs}/{bs}/{ws}"


def bf16_route_name(C):
    """The bf16 forward has one kernel; its tail loop runs (27 C / 32) % 4 k-steps."""
    return f"bf16.t{(27 * (C // 32)) % 4}"


def fwd_workspace_bytes(N, C, dims, ncls):
    ksg, MT = head_fwd_ksg(N, C, *dims, head_mt(ncls)), head_mt(ncls)
    return ksg * N * dims[0] * dims[1] * dims[2] * 16 * MT * 4 if ksg > 1 else 0


def bww_nslabs(N, C, dims, ncls):
    return head_bw_plan(N, C, *dims, head_mt(ncls))["nblocks"]


def bww_workspace_bytes(N, C, dims, ncls):
    MT, nb = head_mt(ncls), bww_nslabs(N, C, dims, ncls)
    return (nb * (C // 16) * 27 * MT * 256 + nb * 16 * MT) * 4


def direct_fold_is_in_slab_order(nslabs, count):
    """msl_grad_reduce_batch folds at most GR_FEW slabs of a count that is a multiple of 4 in slab order, anything else as eight
    interleaved chains; the direct form of the weight gradient folds in the same order."""
    return nslabs <= GR_FEW and count % 4 == 0


# ------------------------------------------------------------------------------------------------- rows <-> channels
def to_rows(y, ncls):
    """y (N, 12 + 2 ncls, D, H, W) -> locs (N, 2 S, 6), scores (N, 2 S, ncls): row 2 P + anchor."""
    N = y.shape[0]
    S = y[0, 0].numel()
    loc = y[:, :12].reshape(N, 2, 6, S).permute(0, 3, 1, 2).reshape(N, 2 * S, 6)
    cls = y[:, 12:].reshape(N, 2, ncls, S).permute(0, 3, 1, 2).reshape(N, 2 * S, ncls)
    return loc.contiguous(), cls.contiguous()


def from_rows(loc, cls, dims, ncls):
    N, S = loc.shape[0], dims[0] * dims[1] * dims[2]
    a = loc.reshape(N, S, 2, 6).permute(0, 2, 3, 1).reshape(N, 12, *dims)
    b = cls.reshape(N, S, 2, ncls).permute(0, 2, 3, 1).reshape(N, 2 * ncls, *dims)
    return torch.cat([a, b], 1).contiguous()


def dO_padded(dO, ncls):
    """The image msl_head_grad_pack writes: (N, 16 MT, D + 2, H + 2, W + 2), zero halo, zero rows at and above 12 + 2 ncls."""
    N, co = dO.shape[:2]
    out = torch.zeros((N, 16 * head_mt(ncls)) + tuple(s + 2 for s in dO.shape[2:]), dtype=dO.dtype)
    out[:, :co, 1:-1, 1:-1, 1:-1] = dO
    return out


# ------------------------------------------------------------------------------------------------- reference
def operands(d, bf16):
    """(a, W (12 + 2 ncls, C, 3, 3, 3), bias) as fp32: what the fp32 entries read, or what the bf16 entries read."""
    W = torch.cat([d["lw"], d["cw"]], 0)
    b = torch.cat([d["lb"], d["cb"]], 0)
    return (bf16_rne(d["a"]), bf16_rne(W), b) if bf16 else (d["a"], W, b)


def reference(d, bf16):
    """float64 conv3d + autograd on the operands, and the same on their absolute values -> dict of float64 tensors."""
    a, W, b = operands(d, bf16)
    dO = d["dO"].double()
    out = {}
    for tag, f in (("", lambda t: t), ("_mag", torch.abs)):
        a_, W_, b_ = (f(t.double()).requires_grad_(True) for t in (a, W, b))
        y = F.conv3d(a_, W_, b_, padding=1)
        y.backward(f(dO))
        out.update({"y" + tag: y.detach(), "ga" + tag: a_.grad, "dW" + tag: W_.grad, "db" + tag: b_.grad})
    return out


def bound(e, what, q):
    return K[q] * U * e[what + "_mag"]


def check_fwd(case_id, e, locs, scores, ncls, bf16=False):
    """locs (N, 2 S, 6), scores (N, 2 S, ncls) as written -> Report."""
    rep = B16.Report(case_id)
    rl, rs = to_rows(e["y"], ncls)
    bl, bs = to_rows(bound(e, "y", "fwd_bf16" if bf16 else "fwd"), ncls)
    rep.bound("locs", locs, rl, bl)
    rep.bound("scores", scores, rs, bs)
    return rep


def check_bwd_data(case_id, e, ga, bf16_out=False):
    rep = B16.Report(case_id)
    if bf16_out:
        rep.interval("ga", ga, e["ga"], bound(e, "ga", "bwd_data"))
    else:
        rep.bound("ga", ga, e["ga"], bound(e, "ga", "bwd_data"))
    return rep


def check_bww(case_id, e, dlw, dcw, dlb, dcb, tag=""):
    rep = B16.Report(case_id)
    Bw, Bb = bound(e, "dW", "dw"), bound(e, "db", "db")
    rep.bound("dloc_w" + tag, dlw, e["dW"][:12], Bw[:12])
    rep.bound("dcl_w" + tag, dcw, e["dW"][12:], Bw[12:])
    rep.bound("dloc_b" + tag, dlb, e["db"][:12], Bb[:12])
    rep.bound("dcl_b" + tag, dcb, e["db"][12:], Bb[12:])
    return rep


def unpinned_share(e):
    lo, hi = B16.interval(e["ga"].reshape(-1), bound(e, "ga", "bwd_data").reshape(-1))
    return float((lo != hi).double().mean())


# ------------------------------------------------------------------------------------------------- packed weights
def _wall(lw, cw, ncls, rows=None):
    C = lw.shape[1]
    co_total = 12 + 2 * ncls
    W = torch.zeros((rows or 16 * head_mt(ncls), C, 27))
    W[:12], W[12:co_total] = lw.reshape(12, C, 27), cw.reshape(2 * ncls, C, 27)
    return W


def pack_expect(lw, cw, ncls):
    """The layouts in the comments of heads.hip, as views of Wall (16 MT, C, 27) whose rows at and above 12 + 2 ncls are zero:
    Wf [cg][tap][mt][q][j] = Wall[16 mt + j][4 cg + q][tap];  Wb [ct][cog][tap][q][j] = Wall[4 cog + q][16 ct + j][tap]."""
    C, MT = lw.shape[1], head_mt(ncls)
    W = _wall(lw, cw, ncls)
    Wf = W.view(MT, 16, C // 4, 4, 27).permute(2, 4, 0, 3, 1).reshape(-1)
    Wb = W.view(4 * MT, 4, C // 16, 16, 27).permute(2, 0, 4, 1, 3).reshape(-1)
    return Wf.contiguous(), Wb.contiguous()


def pack_bf16_expect(lw, cw, ncls):
    """Wp [tap][cg][g][co][jj] = bf16(Wall[co][32 cg + 8 g + jj][tap]), 16 rows, rows at and above 12 + 2 ncls zero (as fp32 values)."""
    C = lw.shape[1]
    W = bf16_rne(_wall(lw, cw, ncls, rows=16))
    return W.view(16, C // 32, 4, 8, 27).permute(4, 1, 2, 0, 3).reshape(-1).contiguous()


def check_pack(case_id, lw, cw, ncls, Wf, Wb):
    """Exact: a packed copy has no arithmetic."""
    rep = B16.Report(case_id)
    ef, eb = pack_expect(lw, cw, ncls)
    rep.bits("Wf", B16.f32bits(Wf), B16.f32bits(ef))
    rep.bits("Wb", B16.f32bits(Wb), B16.f32bits(eb))
    return rep


# ================================================================================================= CPU emulation
# An honest fp32 evaluation in the kernels' coarse order, and the wrong kernels:
#   drop_tap        the centre tap of the first group of the contraction (4 input channels forward, 32 on bf16, 4 output
#                   channels in bwd-data, 4 input channels of the weight gradient) is missing
#   swap_hw         kh and kw exchanged
#   unflipped       bwd-data taps not mirrored
#   halo_origin     slab origin off by one along W: the halo is read as data
#   bias_per_slab   forward: the bias added once per K slab
#   last_slab       forward: the last K slab not folded; weight gradient: the last slab (weights and bias) not folded
#   row12           output row 11 treated as a class row: never written to locs
#   anchor_stride   P*12 + co written as P*6 + co
#   tail_tile       positions at or above S - S % 16 not written
#   clamp_counted   register-fed weight gradient: positions clamped to N S - 1 contribute instead of zero
#   bias_one_block  bias gradient taken from the first position block only
#   ragged_group    LDS bwd-data: the last channel group is not written
#   pad_rows        packed weights: rows at and above 12 + 2 ncls carry the weights of row 12 + 2 ncls - 1
def applicable(mut, entry, case, p):
    """False where a mutant cannot be expressed at (entry, case), each for the reason next to it."""
    id_, N, C, dims, ncls = case
    S = dims[0] * dims[1] * dims[2]
    fwd, bwd, bww = entry.startswith("fwd"), entry.startswith("bwd_data"), entry.startswith("bww")
    ksg = p["fwd"]["ksg"] if entry == "fwd" else 1
    if mut == "drop_tap":
        return fwd or bwd or bww
    if mut == "swap_hw":                 # H = W = 1: the taps off the centre column read only the halo
        return (fwd or bwd or bww) and (dims[1] > 1 or dims[2] > 1)
    if mut == "unflipped":               # one voxel: the centre tap is its own mirror image
        return bwd and S > 1
    if mut == "halo_origin":
        return fwd or bwd or bww
    if mut == "bias_per_slab":
        return entry == "fwd" and ksg > 1
    if mut == "last_slab":
        return (entry == "fwd" and ksg > 1) or (bww and p["bww"]["nblocks"] > 1)
    if mut == "row12":
        return fwd
    if mut == "anchor_stride":           # one voxel: P = 0 is written where it belongs
        return fwd and S > 1
    if mut == "tail_tile":
        return fwd and S % 16 != 0
    if mut == "clamp_counted":
        return bww and p["bww"]["kernel"] == "reg" and p["bww"]["ragged"]
    if mut == "bias_one_block":
        return bww and p["bww"]["nblocks"] > 1
    if mut == "ragged_group":
        return bwd and p["bwd_data"]["kernel"] != "reg"
    if mut == "pad_rows":                # 12 + 2 ncls = 16 or 32: no padded row
        return entry == "pack" and (12 + 2 * ncls) % 16 != 0
    raise KeyError(mut)


def _pad(x, mut):
    """Zero halo of one voxel; the ``halo_origin`` mutant starts one voxel late along W."""
    return F.pad(x, (0, 2, 1, 1, 1, 1) if mut == "halo_origin" else (1, 1, 1, 1, 1, 1))


def _taps(W, mut):
    return W.transpose(3, 4).contiguous() if mut == "swap_hw" else W


def emul_fwd(d, p, ncls, bf16=False, mut=None):
    """-> (locs (N, 2 S, 6), scores (N, 2 S, ncls)) fp32, NaN where nothing was written."""
    a, W, b = operands(d, bf16)
    N, C, D, H, Wd = a.shape
    S, G = D * H * Wd, 32 if bf16 else 4
    W = _taps(W, mut).clone()
    if mut == "drop_tap":
        W[:, :G, 1, 1, 1] = 0.0
    x = _pad(a, mut)
    ksg = 1 if bf16 else p["fwd"]["ksg"]
    cps = C // ksg
    slabs = []
    for s in range(ksg):
        acc = torch.zeros((N, W.shape[0], D, H, Wd))
        if bf16:  # k-step = (tap, 32-channel group), tap-major
            for t in range(27):
                kd, kh, kw = t // 9, (t // 3) % 3, t % 3
                for g in range(0, C, G):
                    acc = acc + torch.einsum("ncdhw,oc->nodhw", x[:, g:g + G, kd:kd + D, kh:kh + H, kw:kw + Wd], W[:, g:g + G, kd, kh, kw])
        else:  # k-step = (channel group of 4, tap), group-major
            for g in range(s * cps, (s + 1) * cps, G):
                for t in range(27):
                    kd, kh, kw = t // 9, (t // 3) % 3, t % 3
                    acc = acc + torch.einsum("ncdhw,oc->nodhw", x[:, g:g + G, kd:kd + D, kh:kh + H, kw:kw + Wd], W[:, g:g + G, kd, kh, kw])
        slabs.append(acc)
    if mut == "last_slab":
        slabs = slabs[:-1]
    y = slabs[0]
    for sl in slabs[1:]:
        y = y + sl
    for _ in range(ksg if mut == "bias_per_slab" else 1):
        y = y + b.view(1, -1, 1, 1, 1)
    locs, scores = to_rows(y, ncls)
    if mut == "row12":
        locs[:, 1::2, 5] = NAN
    if mut == "anchor_stride":
        flat, new = locs.reshape(N, S, 12), torch.full((N, S * 12), NAN)
        new[:, :S * 6] = flat[:, :, :6].reshape(N, S * 6)
        new[:, S * 6:S * 6 + 6] = flat[:, S - 1, 6:]
        locs = new.view(N, 2 * S, 6)
    if mut == "tail_tile":
        locs[:, 2 * (S - S % 16):] = NAN
        scores[:, 2 * (S - S % 16):] = NAN
    return locs, scores


def emul_bwd_data(d, p, ncls, bf16_out=False, mut=None):
    """-> g_a (N, C, D, H, W): fp32, or bf16 values held as fp32; one k-step per group of 4 output channels and tap."""
    _, W, _ = operands(d, False)
    dO = d["dO"]
    N, CO, D, H, Wd = dO.shape
    C = W.shape[1]
    W = _taps(W, mut).clone()
    if mut == "unflipped":
        W = W.flip(2, 3, 4)
    if mut == "drop_tap":
        W[:4, :, 1, 1, 1] = 0.0
    x = _pad(dO, mut)
    acc = torch.zeros((N, C, D, H, Wd))
    for g in range(0, CO, 4):
        for t in range(27):
            kd, kh, kw = t // 9, (t // 3) % 3, t % 3
            src = x[:, g:g + 4, 2 - kd:2 - kd + D, 2 - kh:2 - kh + H, 2 - kw:2 - kw + Wd]
            acc = acc + torch.einsum("nodhw,oc->ncdhw", src, W[g:g + 4, :, kd, kh, kw])
    if bf16_out:
        acc = bf16_rne(acc)
    if mut == "ragged_group":
        acc[:, (p["bwd_data"]["groups"] - 1) * p["bwd_data"]["cts"] * 16:] = NAN
    return acc


def emul_bww(d, p, ncls, bf16=False, mut=None, order="direct"):
    """-> (dloc_w, dcl_w, dloc_b, dcl_b) fp32: one partial per position block, the slabs folded in the reduction's order."""
    a, _, _ = operands(d, bf16)
    dO = d["dO"]
    N, C, D, H, Wd = a.shape
    CO, S = dO.shape[1], D * H * Wd
    x = _pad(a, mut)
    cols = []
    for t in range(27):
        kd, kh, kw = t // 9, (t // 3) % 3, t % 3
        if mut == "swap_hw":
            kh, kw = kw, kh
        cols.append(x[:, :, kd:kd + D, kh:kh + H, kw:kw + Wd].reshape(N, C, S).permute(0, 2, 1).reshape(N * S, C))
    A = torch.stack(cols, 2).reshape(N * S, C * 27)                    # [position][ci][tap]
    G = dO.reshape(N, CO, S).permute(1, 0, 2).reshape(CO, N * S)       # [co][position]
    w, blk, nb = p["bww"], p["bww"]["block"], p["bww"]["nblocks"]
    ws, bs = [], []
    for k in range(nb):
        lo, hi = k * blk, min(N * S, (k + 1) * blk)
        ws.append(G[:, lo:hi] @ A[lo:hi])
        bs.append(G[:, lo:hi].sum(1))
    if mut == "clamp_counted":
        extra = nb * blk - N * S
        ws[-1] = ws[-1] + float(extra) * torch.outer(G[:, -1], A[-1])
        bs[-1] = bs[-1] + float(extra) * G[:, -1]
    if mut == "last_slab":
        ws, bs = ws[:-1], bs[:-1]
    if mut == "bias_one_block":
        bs = bs[:1]

    def fold(parts, few):
        if few:
            chains = [parts]
        else:
            chains = [parts[g::8] for g in range(8)]
        tot = torch.zeros_like(parts[0])
        for ch in chains:
            s = torch.zeros_like(parts[0])
            for v in ch:
                s = s + v
            tot = tot + s
        return tot

    dW = fold(ws, len(ws) <= GR_FEW).view(CO, C, 3, 3, 3).clone()
    if mut == "drop_tap":
        dW[:, :4, 1, 1, 1] = 0.0
    bias = torch.stack(bs)  # [block][co]
    dlb = fold(list(bias[:, :12]), direct_fold_is_in_slab_order(len(bs), 12))
    dcb = fold(list(bias[:, 12:]), direct_fold_is_in_slab_order(len(bs), CO - 12))
    return dW[:12].contiguous(), dW[12:].contiguous(), dlb, dcb


def emul_pack(d, ncls, mut=None):
    """-> (Wf, Wb) by the index arithmetic of head_pack_weights_kernel, element by element."""
    lw, cw = d["lw"], d["cw"]
    C, MT, co_total = lw.shape[1], head_mt(ncls), 12 + 2 * ncls
    W = _wall(lw, cw, ncls)
    if mut == "pad_rows":
        W[co_total:] = W[co_total - 1]
    i = torch.arange(C // 4 * 27 * MT * 64)
    lane, r = i & 63, i >> 6
    mt, r2 = r % MT, r // MT
    tap, cg = r2 % 27, r2 // 27
    Wf = W[mt * 16 + (lane & 15), 4 * cg + (lane >> 4), tap]
    tap, r2 = r % 27, r // 27
    cog, ct = r2 % (4 * MT), r2 // (4 * MT)
    Wb = W[4 * cog + (lane >> 4), 16 * ct + (lane & 15), tap]
    return Wf, Wb


def emulate(case, entry, d, p, mut=None):
    """The output tuple of one entry for one case (``d`` = heads_cases.make_data(case), ``p`` = plan of the case)."""
    ncls = case[4]
    if entry in ("fwd", "fwd_bf16"):
        return emul_fwd(d, p, ncls, entry == "fwd_bf16", mut)
    if entry in ("bwd_data", "bwd_data_bf16"):
        return (emul_bwd_data(d, p, ncls, entry == "bwd_data_bf16", mut),)
    if entry in ("bww", "bww_bf16"):
        return emul_bww(d, p, ncls, entry == "bww_bf16", mut)
    if entry == "pack":
        return emul_pack(d, ncls, mut)
    raise KeyError(entry)


def check(case, entry, e, out, d=None):
    """-> Report of ``out`` (what ``emulate`` returns, or the same tuple read back from the GPU) for one entry."""
    id_, ncls = case[0], case[4]
    if entry in ("fwd", "fwd_bf16"):
        return check_fwd(id_, e, out[0], out[1], ncls, entry == "fwd_bf16")
    if entry in ("bwd_data", "bwd_data_bf16"):
        return check_bwd_data(id_, e, out[0], entry == "bwd_data_bf16")
    if entry in ("bww", "bww_bf16"):
        return check_bww(id_, e, *out)
    if entry == "pack":
        return check_pack(id_, d["lw"], d["cw"], ncls, out[0], out[1])
    raise KeyError(entry)
