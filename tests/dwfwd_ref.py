"""Float64 reference of the depthwise-convolution FORWARD kernels (csrc/dwconv.hip and dw_fwd_bf16_kernel of csrc/bf16.hip), with
derived error bounds, the per-slot map of their statistics partials, and the checkers.  Plain torch on the CPU; like
tests/dwbwd_ref.py (whose helpers it reuses) nothing here imports the package.  The same checkers judge the GPU outputs
(tests/test_gpu_dwfwd.py) and, on the CPU, an honest fp32 emulation and ten wrong kernels (tests/test_dwfwd_ref_cpu.py); both
emulations live at the end of this file.

    y[n,c,o] = sum_k w[c,k] a[n,c, s o - 1 + k]      a = relu(fma(x, scale, shift)) or x itself; zero outside the volume

evaluated as 27 strided slice products (``fwd_ref``; the slices are dwbwd_ref._axis).  No F.conv3d: the reference shares no code
with the torch op the older tests of these kernels compare with (tests/test_dwfwd_ref_cpu.py checks it against that op).  The
activation is reproduced, not bounded: ``act32`` of tests/pw_ref.py is msl::act bit for bit, so no element is excluded and no
margin around zero is needed; the padding is zero AFTER the activation.  On bf16 storage x is the bf16 value widened exactly.

Value bound (``U = 2**-24``, ``gamma(n) = n U / (1 - n U)``):  B = gamma(n) absdot,  absdot = sum_k |w_k| |a_k|,  n = the element's
own number of in-volume taps (at most 27).  Whatever the order, and with or without fma contraction, a term passes at most one
rounding per NON-zero term it meets (the argument of dwbwd_ref); a tap over the zero halo adds an exact zero.  Every forward
kernel keeps ONE fmaf chain per output and nothing else (line numbers of the parent of this file's first commit):

    kernel                              the chain                                             what else touches the accumulator
    dw_fwd_stream_kernel                dwconv.hip :305-306, :333 (stride 2), :352-354 (1)    :320, :369-370 move registers
    dw_fwd_resident_kernel              :529                                                  (:536 only with accumulate)
    dw_s1_wave_kernel                   :683                                                  (:697 only with accumulate)
    dw_s2_wave_kernel                   :842-843                                              -
    dw_s2_rows_eval_kernel              :989-990                                              -
    dw_s1_rows_eval_kernel              :1083                                                 -
    dw_fwd_naive_kernel                 :1365 (in-volume taps only)                           -
    dw_small_eval_kernel                :1413                                                 -
    dw_fwd_bf16_kernel                  bf16.hip :112                                         (:115 only with accumulate)

No kernel splits an accumulator and merges the parts afterwards, and none uses a ``dot4``-style partial product (dot4, :105, is the
weight gradient's); so there is no table of depths: n is the tap count for all of them.

* fp32 outputs: |y - y64| <= B elementwise (``worst``).
* bf16 outputs (msl::f2bf, common.hpp :213, in st4 / st2 :241-251, dwconv.hip :1414, bf16.hip :116): the rounding-interval test
  ``bf16pw_ref.check_interval(stored, y64, B)`` - no relative tolerance.  ``pinned_share`` is the share of elements whose interval is
  a single bf16 value; the CPU test demands more than one half on every bf16 case, from the reference alone.

Statistics partials[2][C][NP], slot by slot.  ``slots(route, N, C, dims, stride)`` reproduces which outputs slot p sums:

    route      slot within an image                          read from                                     per image
    wave       od / SLAB                                     :595, :721 (stride 1); :761, :901 (stride 2)  ceil(OD' / SLAB)
    wave, split planes (stride 2, more than four waves per plane: 64 x 64)
               (od / SLAB) GPP + (oh W/4) / 256              cell :758-759, part / WPG :877                 nslabs GPP
    stream     od / SLAB                                     :133-136, :393                                 nslabs
    resident   od / SLAB                                     :410-414, :550                                 nslabs
    naive      o / 4096 (o the flat output index)            channel_stats_kernel :1425, :1432              ceil(OS / 4096)
    tiled      ((od / 2) tiles_h + oh / 8) tiles_w + ow / 32 bf16.hip :58-60, :126                          tiles

with p = n (slots per image) + slot everywhere.  SLAB and G are the planners' (``wave_plan`` and ``lds_plan`` below are
dwroute.hpp :65-88 and :101-140 line for line; the CPU test holds their partial counts against the library's queries).

Every slot is compared with the float64 sum of y64 over exactly its outputs - on bf16 storage too: the kernels sum their
UNROUNDED fp32 accumulators (dwconv.hip :700-707, :855-858; bf16.hip :117-118), not the stored values.
    sum:             sum B + d U sum |y64|
    sum of squares:  sum (2 |y64| B + B^2) + (d + 1) U sum y64^2
d = SUMS_DEPTH[route]: the fp32 additions a term passes before the value becomes a double.  (The first addition of a chain adds to
zero and is exact, so a chain of d additions rounds d - 1 times: the spare U sum |y64| is what covers the second-order terms
d U sum B that the formula does not carry.  The squares: ``fmaf(v, v, q)`` rounds once per link, the first included - d roundings -
and the stride-2 wave kernel's ``fmaf(b, b, a * a)`` twice; (d + 1) covers both.)
"""
import torch

from tests import bf16pw_ref as B16
from tests.bf16pw_ref import bf16_rne, check_interval, round_bits  # noqa: F401  (re-exported for the tests)
from tests.bn_ref import U, _bc, exact_sum, worst  # noqa: F401
from tests.dwbwd_ref import KIND, _axis, gamma, out_dims  # noqa: F401
from tests.pw_ref import act32, fma32  # noqa: F401

NAN = float("nan")
VARIANT = dict(naive=0, stream=1, resident=2, wave=3)  # what msl_dwconv_fwd_variant answers

# fp32 additions a term of the statistics passes in one thread before the value becomes a double
SUMS_DEPTH = {
    # dw_s1_wave_kernel :700-707: ``s += acc[o][v]`` over the lane's 4 outputs, then ``ds += (double)s``
    "wave_s1": 4,
    # dw_s2_wave_kernel :855-858: ``s = acc[o][0] + acc[o][1]``, then ``ds += (double)s``
    "wave_s2": 1,
    # dw_fwd_resident_kernel :539-546: 4 outputs of an item, ``it_s[item] = s``; emit_stats adds ``(double)it_s[..]`` (:87)
    "resident": 4,
    # dw_fwd_stream_kernel :315-316 / :363-364: ``st_s[t] += acc_a[t][v]`` for the 4 outputs of the item in EVERY output plane of
    # the slab (at most SLAB of them), written to LDS once (:388) and cast by emit_stats: see sums_depth()
    "stream": None,
    # channel_stats_kernel :1427-1431: thread t adds y[lo + t], y[lo + t + 256], .. of a 4096-output chunk: 16, then block_sum of doubles
    "naive": 16,
    # dw_fwd_bf16_kernel bf16.hip :117-118: ``s += (double)acc; q += (double)acc * (double)acc``
    "tiled": 0,
}


def cdiv(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------------------------------------- the planners (dwroute.hpp)
def wave_plan(N, C, dims, stride):
    """dwroute.hpp :65-88 -> dict(SLAB, nslabs, cpw, wpp) or None."""
    D, H, W = dims
    if H != W:
        return None
    if stride == 2:
        if W not in (8, 16, 32, 64):
            return None
        cells, OD = (H // 2) * (W // 4), (D - 1) // 2 + 1
        cpw, wpp = (1, cells // 64) if cells >= 64 else (64 // cells, 1)
        if C % cpw:
            return None
        SLAB = 4 if OD >= 8 else 2 if OD >= 4 else 1
        return dict(SLAB=SLAB, nslabs=cdiv(OD, SLAB), cpw=cpw, wpp=wpp)
    if W not in (4, 8, 16):
        return None
    cpw = 64 // (H * W // 4)
    if C % cpw:
        return None
    SLAB = 8 if D >= 16 else 4 if D >= 8 else 2 if D >= 4 else 1
    return dict(SLAB=SLAB, nslabs=cdiv(D, SLAB), cpw=cpw, wpp=1)


def lds_plan(N, C, dims, stride):
    """dwroute.hpp :101-140 -> dict(kind = "stream" | "resident" | "naive", SLAB, nslabs, G, ipt)."""
    D, H, W = dims
    OD, OH, OW = out_dims(dims, stride)
    if not (W % 4 == 0 and OW % 4 == 0 and (stride == 1 or (H % 2 == 0 and W % 2 == 0))):
        return dict(kind="naive")
    RS = W + 8 if stride == 1 else ((OW + 3) & ~3) + ((OW + 4) & ~3)
    PS = (H + 2) * RS
    Lp = OH * (OW // 4)
    if H * W >= 1024:
        ipt, lpt = cdiv(Lp, 256), cdiv(H * (W // 4), 256)
        if ipt > 4 or lpt > 12 or max(PS * 4, 2 * Lp * 4) > 160 * 1024:
            return dict(kind="naive")
        slabs = max(1, min(OD, 1024 // max(1, N * C)))
        SLAB = cdiv(OD, slabs)
        if SLAB < 4:
            SLAB = min(4, OD)
        return dict(kind="stream", SLAB=SLAB, nslabs=cdiv(OD, SLAB), G=1, ipt=1 if (ipt <= 1 and lpt <= 4) else 4)
    SLAB = OD
    while (SLAB > 2 and (N * C * cdiv(OD, SLAB) < 1024 or (stride * SLAB + 2) * PS * 4 > 40 * 1024) and SLAB % 2 == 0
           and SLAB // 2 >= 2):
        SLAB //= 2
    NPL = stride * SLAB + (1 if stride == 2 else 2)
    per_ch = NPL * PS * 4 + 2 * SLAB * Lp * 4
    if per_ch > 150 * 1024:
        return dict(kind="naive")
    G = max(1, 256 // max(1, SLAB * Lp))
    p = 1
    while p * 2 <= G:
        p *= 2
    G = min(p, 64)
    while G > 1 and (C % G != 0 or per_ch * G > 60 * 1024):
        G //= 2
    return dict(kind="resident", SLAB=SLAB, nslabs=cdiv(OD, SLAB), G=G, ipt=0)


def train_route(bf16, N, C, dims, stride, force_naive=False):
    """The route of a forward WITH statistics (dw_route, dwroute.hpp :152-223): (name, plan)."""
    if not force_naive:
        p = wave_plan(N, C, dims, stride)
        if p:
            return "wave", p
    if bf16:
        return "tiled", {}
    if force_naive:
        return "naive", {}
    p = lds_plan(N, C, dims, stride)
    return p["kind"], p


def sums_path(route, stride):
    return f"wave_s{stride}" if route == "wave" else route


def sums_depth(route, plan, stride):
    """SUMS_DEPTH of a route; the stream kernel's chain runs over the output planes of its slab."""
    if route == "stream":
        return 4 * plan["SLAB"]
    return SUMS_DEPTH[sums_path(route, stride)]


# ------------------------------------------------------------------------------------------------- which slot sums which output
def slots(route, plan, dims, stride):
    """-> (slot (OD, OH, OW) int64: the slot within an image that sums the output, slots per image)."""
    D, H, W = dims
    OD, OH, OW = out_dims(dims, stride)
    od = torch.arange(OD).view(OD, 1, 1).expand(OD, OH, OW)
    oh = torch.arange(OH).view(1, OH, 1).expand(OD, OH, OW)
    ow = torch.arange(OW).view(1, 1, OW).expand(OD, OH, OW)
    if route == "wave":
        gpp = plan["wpp"] // 4 if plan["wpp"] > 4 else 1  # one partial per workgroup of four waves of a split plane
        s = od // plan["SLAB"]
        if gpp > 1:  # cell = oh (W / 4) + ow / 2, 64 cells a wave, 4 waves a workgroup
            s = s * gpp + (oh * (W // 4) + ow // 2) // 256
        return s.contiguous(), plan["nslabs"] * gpp
    if route in ("stream", "resident"):
        return (od // plan["SLAB"]).contiguous(), plan["nslabs"]
    if route == "naive":
        return (((od * OH + oh) * OW + ow) // 4096).contiguous(), cdiv(OD * OH * OW, 4096)
    if route == "tiled":
        th, tw = cdiv(OH, 8), cdiv(OW, 32)
        return (((od // 2) * th + oh // 8) * tw + ow // 32).contiguous(), cdiv(OD, 2) * th * tw
    raise KeyError(route)


def slot_sums(t, slot, per):
    """t (N, C, OD, OH, OW) float64 -> (C, N * per): sums per slot, partial index p = n * per + slot."""
    N, C = t.shape[:2]
    out = torch.zeros((N, C, per), dtype=t.dtype)
    out.index_add_(2, slot.reshape(-1), t.reshape(N, C, -1))
    return out.permute(1, 0, 2).reshape(C, N * per)


# ------------------------------------------------------------------------------------------------- the convolution
def fwd_ref(a32, w, stride):
    """a32 (N, C, D, H, W): the activated input (fp32 or bf16 values), w (C, 27) -> (y64, absdot, taps): float64
    (N, C, OD, OH, OW) twice and the number of in-volume taps (OD, OH, OW)."""
    N, C, D, H, W = a32.shape
    OD, OH, OW = out_dims((D, H, W), stride)
    ad, wd = a32.double(), w.double()
    y = torch.zeros((N, C, OD, OH, OW), dtype=torch.float64)
    absdot = torch.zeros_like(y)
    taps = torch.zeros((OD, OH, OW), dtype=torch.float64)
    for kd in range(3):
        xd = _axis(D, OD, stride, kd)
        for kh in range(3):
            xh = _axis(H, OH, stride, kh)
            for kw in range(3):
                xw = _axis(W, OW, stride, kw)
                if xd is None or xh is None or xw is None:
                    continue
                wk = wd[:, kd * 9 + kh * 3 + kw].view(1, C, 1, 1, 1)
                src = ad[:, :, xd[1], xh[1], xw[1]]
                y[:, :, xd[0], xh[0], xw[0]] += wk * src
                absdot[:, :, xd[0], xh[0], xw[0]] += wk.abs() * src.abs()
                taps[xd[0], xh[0], xw[0]] += 1
    return y, absdot, taps


def expect(x, w, stride, sc=None, sh=None):
    """x (N, C, D, H, W) as stored (fp32, or bf16 values), w (C, 27), optional per-channel affine -> dict(y, B, absdot, taps)."""
    a = act32(x.float(), sc, sh) if sc is not None else x.float()
    y, absdot, taps = fwd_ref(a, w, stride)
    return dict(y=y, B=gamma(taps) * absdot, absdot=absdot, taps=taps)


def stats_expect(e, route, plan, dims, stride):
    """-> (ref, bound, per): float64 (2, C, NP) of the statistics partials from the reference output (NOT the stored one)."""
    slot, per = slots(route, plan, dims, stride)
    d = sums_depth(route, plan, stride)
    y, Bv = e["y"], e["B"]
    ay, yy = y.abs(), y * y
    s = lambda t: slot_sums(t, slot, per)  # noqa: E731
    ref = torch.stack([s(y), s(yy)])
    bnd = torch.stack([s(Bv) + d * U * s(ay), s(2 * ay * Bv + Bv * Bv) + (d + 1) * U * s(yy)])
    return ref, bnd, per


def pinned_share(e):
    """Share of elements whose rounding interval is a single bf16 value: a property of the reference and its bound alone."""
    lo, hi = B16.interval(e["y"].reshape(-1), e["B"].reshape(-1))
    return float((lo == hi).double().mean())


def check(case_id, e, y, bf16, partials=None, route=None, plan=None, dims=None, stride=None):
    """-> bf16pw_ref.Report of one forward: y (N, C, OD, OH, OW) as stored, partials (2, C, NP) fp64 or None."""
    rep = B16.Report(case_id)
    if bf16:
        rep.interval("y", y, e["y"], e["B"])
    else:
        rep.bound("y", y, e["y"], e["B"])
    if partials is not None:
        ref, bnd, _ = stats_expect(e, route, plan, dims, stride)
        if tuple(partials.shape) != tuple(ref.shape):
            rep._add("partials", 1, float("inf"), 0, None, f"shape {tuple(partials.shape)}, the slot map has {tuple(ref.shape)}")
        else:
            rep.bound("sum", partials[0], ref[0], bnd[0])
            rep.bound("sumsq", partials[1], ref[1], bnd[1])
    return rep


# ================================================================================================= CPU emulations
# An honest fp32 evaluation of every forward kernel - one fmaf chain in tap order over the zero-padded activated input, one
# bf16_rne at the end on bf16 storage, the statistics in the kernels' own fp32 chains - and the wrong kernels of the CPU test:
#   drop_tap     the centre tap (always inside the volume) is missing at the last face along W
#   halo_act     the halo holds act(0) = relu(shift) instead of 0 (affine only)
#   reversed     taps reversed (w[26 - k])
#   origin       stride 2: input index s o + k instead of s o - 1 + k
#   trunc        bf16: truncation instead of round-to-nearest-even
#   twice        bf16: the accumulator goes through bf16 before the last add (the centre tap, added last)
#   stats_stored bf16: both statistics from the stored values
#   slot_later   every partial one slot later (slot 0 keeps the NaN the buffer was filled with)
#   sq_rounded   bf16: the sum of squares from the stored values, the sum from the accumulators
#   abs          |fma(x, scale, shift)| instead of relu (affine only)
MUTANTS = ("drop_tap", "halo_act", "reversed", "origin", "trunc", "twice", "stats_stored", "slot_later", "sq_rounded", "abs")


def _activated(x, sc, sh, mut):
    if sc is None:
        return x.float()
    if mut == "abs":
        return fma32(x.float(), _bc(sc, x).float(), _bc(sh, x).float()).abs()
    return act32(x.float(), sc, sh)


def _padded(a, sh, mut):
    """Zero halo of one voxel before and two behind every axis (the ``origin`` mutant reads one further)."""
    p = torch.nn.functional.pad(a, (1, 2, 1, 2, 1, 2))
    if mut == "halo_act" and sh is not None:
        h = torch.where(sh < 0, torch.zeros_like(sh), sh).float().view(1, -1, 1, 1, 1).expand_as(p).clone()
        h[:, :, 1:-2, 1:-2, 1:-2] = a
        p = h
    return p


def emul_acc(x, w, stride, sc=None, sh=None, mut=None, centre_last=False):
    """-> fp32 accumulators (N, C, OD, OH, OW); with ``centre_last`` (acc without the centre tap, the centre tap's operands)."""
    N, C, D, H, W = x.shape
    OD, OH, OW = out_dims((D, H, W), stride)
    p = _padded(_activated(x, sc, sh, mut), sh, mut)
    w = w.flip(1) if mut == "reversed" else w
    off = 1 if mut == "origin" and stride == 2 else 0
    acc = torch.zeros((N, C, OD, OH, OW))
    centre = None
    for k in range(27):
        kd, kh, kw = k // 9, (k // 3) % 3, k % 3
        src = p[:, :, kd + off:kd + off + stride * (OD - 1) + 1:stride, kh + off:kh + off + stride * (OH - 1) + 1:stride,
                kw + off:kw + off + stride * (OW - 1) + 1:stride]
        wk = w[:, k].view(1, C, 1, 1, 1).expand_as(src)
        if mut == "drop_tap" and k == 13:
            src = src.clone()
            src[..., OW - 1] = 0.0
        if centre_last and k == 13:
            centre = (wk, src)
            continue
        acc = fma32(wk, src, acc)
    return (acc, centre) if centre_last else acc


def emul_stats(acc, route, plan, dims, stride):
    """fp32 accumulators -> fp64 (2, C, NP): the statistics in the kernels' own fp32 chains, then doubles per slot."""
    N, C, OD, OH, OW = acc.shape
    slot, per = slots(route, plan, dims, stride)
    zero = torch.zeros(())
    if route == "tiled":
        s, q, sl = acc.double(), acc.double() * acc.double(), slot
    elif route == "naive":  # thread t of a chunk: t, t + 256, ..
        OS, ch = OD * OH * OW, cdiv(OD * OH * OW, 4096)
        v = torch.nn.functional.pad(acc.reshape(N, C, OS), (0, ch * 4096 - OS)).view(N, C, ch, 16, 256)
        s, q = torch.zeros((N, C, ch, 256)), torch.zeros((N, C, ch, 256))
        for i in range(16):
            s, q = s + v[:, :, :, i], fma32(v[:, :, :, i], v[:, :, :, i], q)
        out = torch.stack([s.double().sum(-1), q.double().sum(-1)])  # (2, N, C, ch)
        return out.permute(0, 2, 1, 3).reshape(2, C, N * ch)
    elif route == "wave" and stride == 2:  # a lane's two outputs
        a0, a1 = acc[..., 0::2], acc[..., 1::2]
        s, q, sl = a0 + a1, fma32(a1, a1, a0 * a0), slot[..., 0::2]
    elif route == "stream":  # an item's four outputs in every output plane of the slab
        SLAB, ns = plan["SLAB"], plan["nslabs"]
        s, q = torch.zeros((N, C, ns, OH, OW // 4)), torch.zeros((N, C, ns, OH, OW // 4))
        for od in range(OD):
            for v in range(4):
                t = acc[:, :, od, :, v::4]
                s[:, :, od // SLAB] = s[:, :, od // SLAB] + t
                q[:, :, od // SLAB] = fma32(t, t, q[:, :, od // SLAB])
        out = torch.stack([s.double().sum((3, 4)), q.double().sum((3, 4))])  # (2, N, C, ns)
        return out.permute(0, 2, 1, 3).reshape(2, C, N * ns)
    else:  # wave stride 1, resident: a lane's / an item's four outputs
        s, q = zero, zero
        for v in range(4):
            t = acc[..., v::4]
            s, q = s + t, fma32(t, t, q)
        sl = slot[..., 0::4]
    return torch.stack([slot_sums(s.double(), sl, per), slot_sums(q.double(), sl, per)])


def emulate(x, w, stride, bf16, sc=None, sh=None, stats=None, mut=None):
    """-> (y as stored: fp32, or bf16 values held as fp32; partials (2, C, NP) fp64 or None).  stats = (route, plan, dims)."""
    if bf16 and mut == "twice":
        part, (wk, src) = emul_acc(x, w, stride, sc, sh, centre_last=True)
        acc = fma32(wk, src, bf16_rne(part))
    else:
        acc = emul_acc(x, w, stride, sc, sh, mut)
    y = acc
    if bf16:
        y = round_bits(acc, 16, "trunc") if mut == "trunc" else bf16_rne(acc)
    part = None
    if stats is not None:
        route, plan, dims = stats
        part = emul_stats(y if mut == "stats_stored" else acc, route, plan, dims, stride)
        if mut == "sq_rounded":
            part[1] = emul_stats(y, route, plan, dims, stride)[1]
        if mut == "slot_later":
            part = torch.cat([torch.full_like(part[..., :1], NAN), part[..., :-1]], -1)
    return y, part
