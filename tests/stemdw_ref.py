"""Float64 reference of the fused eval stem + depthwise kernel (stem_dw_eval_kernel of csrc/stemdw.hip: msl_stem_dw_fwd_eval and
msl_stem_dw_fwd_eval_bf16), with derived error bounds, the planner restated, an honest fp32 emulation in the kernel's own order
and the wrong kernels of the CPU test.  Plain torch on the CPU; like tests/stem_ref.py and tests/dwfwd_ref.py (whose helpers it
reuses) nothing here imports the package.  Line numbers are those of csrc/stemdw.hip at this file's first commit.

    z[n,c,o] = sum_k wd[c,k] a[n,c, 2 o - 1 + k],   a = relu(sc y + sh) inside the activation map and 0 outside it,
    y = conv3d(x, w, stride 2, pad 1)               (on bf16 storage: y rounded to bf16 before the affine, :153)

Two checks judge every output.

End to end, from x (``ref``).  The roundings the code can apply, stage by stage:
  stem     one accumulator per output runs through KS = ceil(27 Cin / 2) MFMAs of two k each (:183 / :192, the operand layout of
           stem_fwd_rows_kernel): stem_ref.k_pad(Cin) fmaf roundings and nothing afterwards ->  E_y = k_pad(Cin) U conv(|x|, |w|).
           bf16 entry: ``v = bf2f(f2bf(v))`` (:153) adds the bf16 rounding of the raw value: half a bf16 ulp of its binade,
           ``bf16_half_ulp(|y64| + E_y)`` = 2^(e-8) for a value in [2^e, 2^(e+1)) - between 2^-9 |v| at the top of a binade and
           2^-8 |v| at its bottom.  (A flat 2^-9 |y64| is NOT a bound of round-to-nearest to 8 significant bits: 1 + 2^-8 moves by
           2^-8.  The exact emulation below leaves it at c1-th4-aw64-sd1, error / bound 1.048, and the CPU test keeps that figure.)
  affine   msl::act (:156) is ONE fmaf and a compare:  E_a = |sc| E_y + 2 U (|sc y64| + |sh|)  (U for the fmaf's rounding, the
           second U pays for its operand being y64 + E_y rather than y64).  ReLU is 1-Lipschitz, so E_a holds behind it, no element
           near zero is excluded and no margin is taken.  A padding cell is an exact 0 (:60, :169, the p >= 0 test of :211): E_a = 0.
  dw       one fmaf chain per output in (kd, kh, kw) order over two or three plane steps (:234, :238), a tap over the zero halo
           adds an exact zero:  B = sum_k |wd_k| E_a,k + gamma(n) sum_k |wd_k| (|a64_k| + E_a,k),  n = the in-volume taps.
  fp32 output: |z - z64| <= B.   bf16 output (msl::f2bf, :242): bf16pw_ref.check_interval(stored, z64, B).

Second stage alone, from the stored stem output (``ref_from_y``).  msl_stem_conv_fwd[_bf16] has its own float64 suite
(tests/test_gpu_stem.py) and the fused kernel issues the same 14 (27) MFMAs on the same operands in the same order (header of
stemdw.hip), so its raw values are those that kernel stores.  pw_ref.act32 is msl::act bit for bit, the depthwise convolution runs
in float64, and the bound is gamma(n) absdot ALONE: a wrong plane, parity slot, tap or halo cell is orders of magnitude outside
it, and on bf16 storage almost every rounding interval is a single bf16 value (``pinned_share``).

``plan`` is sdw_plan (:269-295) line for line; ``emulate`` follows the kernel workgroup by workgroup (see there), and MUTANTS
lists what it can do wrong.
"""
import torch

from tests import bf16pw_ref as B16
from tests import stem_ref
from tests.bf16pw_ref import bf16_rne, check_interval  # noqa: F401  (re-exported for the tests)
from tests.bn_ref import U, _bc, worst  # noqa: F401
from tests.dwbwd_ref import _axis, gamma
from tests.dwfwd_ref import pinned_share  # noqa: F401
from tests.pw_ref import act32, fma32
from tests.stem_ref import k_pad

COUT = 32          # SDW_C
NCG = 3            # SDW_NCG
NT = 512           # SDW_NT
NLD = 8            # SDW_NLD
LDS_MAX = 160 * 1024
S222 = (2, 2, 2)
ERR_UNSUPPORTED = -2


def cdiv(a, b):
    return (a + b - 1) // b


def act_dims(dims):
    return tuple(d // 2 for d in dims)


def z_dims(dims):
    return tuple(d // 4 for d in dims)


# ------------------------------------------------------------------------------------------------- the planner (sdw_plan)
def plan(N, cin, dims):
    """sdw_plan, :269-295 -> None (refused) or dict(th, sd, lds, slots, grid, aw)."""
    D, H, W = dims
    if N <= 0 or cin < 1 or cin > 2 or D < 4 or H < 4 or W < 4 or D % 4 or H % 4 or W % 4:
        return None
    AW, ZD, ZH = W // 2, D // 4, H // 4
    if AW % 32 != 0 or AW > 32 * NCG:
        return None
    if cin * D * H * W >= 1 << 30:
        return None
    ap, xp = AW + 4, W + 8
    th = lds = slots = 0
    for t in (3, 4, 2):
        if ZH % t:
            continue
        nrw = 2 * t + 1
        nxr = 2 * nrw + 1
        lds_t = (cin * 3 * nxr * xp + COUT * nrw * ap + 2 * COUT) * 4
        slots_t = cin * 3 * nxr * (W // 4 + 1)
        if lds_t <= LDS_MAX and slots_t <= NLD * NT:
            th, lds, slots = t, lds_t, slots_t
            break
    if not th:
        return None
    sd = 1
    for s in (8, 6, 4, 3, 2, 1):
        if ZD % s:
            continue
        sd = s
        if N * (ZH // th) * (ZD // s) >= 256:
            break
    return dict(th=th, sd=sd, lds=lds, slots=slots, grid=(ZH // th, ZD // sd, N), aw=AW)


# ------------------------------------------------------------------------------------------------- the float64 reference
def dw64(a, Ea, wd):
    """a (N, 32, AD, AH, AW) float64 (zero outside is implied), Ea its elementwise error or None, wd (32, 27) ->
    (z64, absdot = sum |wd| |a|, prop = sum |wd| Ea (or None), taps (ZD, ZH, ZW)): 27 strided slice products."""
    N, C, D, H, W = a.shape
    OD, OH, OW = (D - 1) // 2 + 1, (H - 1) // 2 + 1, (W - 1) // 2 + 1
    w64 = wd.double().view(C, 27)
    z = torch.zeros((N, C, OD, OH, OW), dtype=torch.float64)
    absdot = torch.zeros_like(z)
    prop = torch.zeros_like(z) if Ea is not None else None
    taps = torch.zeros((OD, OH, OW), dtype=torch.float64)
    for kd in range(3):
        xd = _axis(D, OD, 2, kd)
        for kh in range(3):
            xh = _axis(H, OH, 2, kh)
            for kw in range(3):
                xw = _axis(W, OW, 2, kw)
                if xd is None or xh is None or xw is None:
                    continue
                wk = w64[:, kd * 9 + kh * 3 + kw].view(1, C, 1, 1, 1)
                src = a[:, :, xd[1], xh[1], xw[1]]
                z[:, :, xd[0], xh[0], xw[0]] += wk * src
                absdot[:, :, xd[0], xh[0], xw[0]] += wk.abs() * src.abs()
                if prop is not None:
                    prop[:, :, xd[0], xh[0], xw[0]] += wk.abs() * Ea[:, :, xd[1], xh[1], xw[1]]
                taps[xd[0], xh[0], xw[0]] += 1
    return z, absdot, prop, taps


def bf16_half_ulp(t):
    """Half a bf16 ulp of the binade of |t| (float64, > 0): 2^(floor(log2 t) - 8)."""
    e = torch.frexp(t)[1].to(torch.int64)  # t = m 2^e, 0.5 <= m < 1
    return torch.ldexp(torch.ones_like(t), e - 9)


def stem64(x, w):
    """-> (y64, conv(|x|, |w|)) of the stem: stem_ref.fwd_ref at stride 2."""
    return stem_ref.fwd_ref(x, w, S222)


def ref(x, w, sc, sh, wd, bf16, stem=None, flat_bf16=None):
    """The composition in float64 from x -> dict(y = z64, B, taps, absdot).  ``stem``: a cached stem64(x, w).  ``flat_bf16``: take
    flat_bf16 |y64| for the bf16 rounding of the raw stem value (only the CPU test does, to show that 2^-9 |y64| is no bound)."""
    y64, yabs = stem if stem is not None else stem64(x, w)
    Ey = k_pad(x.shape[1]) * U * yabs
    if bf16:
        Ey = Ey + (bf16_half_ulp(y64.abs() + Ey) if flat_bf16 is None else flat_bf16 * y64.abs())
    s, t = _bc(sc, y64), _bc(sh, y64)
    a64 = torch.relu(s * y64 + t)
    Ea = s.abs() * Ey + 2 * U * ((s * y64).abs() + t.abs())
    z, absdot, prop, taps = dw64(a64, Ea, wd)
    return dict(y=z, B=prop + gamma(taps) * (absdot + prop), taps=taps, absdot=absdot)


def ref_from_y(y_stored, sc, sh, wd):
    """The second stage from the raw stem output as msl_stem_conv_fwd[_bf16] stores it (fp32, or bf16 values in any float dtype)
    -> dict(y = z64, B = gamma(n) absdot, taps, absdot)."""
    a = act32(y_stored.float(), sc, sh)
    z, absdot, _, taps = dw64(a.double(), None, wd)
    return dict(y=z, B=gamma(taps) * absdot, taps=taps, absdot=absdot)


def check(case_id, what, e, z, bf16):
    """-> bf16pw_ref.Report with one row: z (N, 32, ZD, ZH, ZW) as stored against e = ref(..) or ref_from_y(..)."""
    rep = B16.Report(case_id)
    if bf16:
        rep.interval(what, z, e["y"], e["B"])
    else:
        rep.bound(what, z, e["y"], e["B"])
    return rep


# ================================================================================================= the kernel, emulated in fp32
# ``emulate`` does what stem_dw_eval_kernel does, in its order, vectorised over the images and the row groups (workgroups of one
# plane segment differ only in oh0; each gets its own tile of 2 TH + 1 activation rows, the halo row recomputed):
#   stem      an fmaf chain over k = ci 27 + kd 9 + kh 3 + kw ascending (:62-72, :183), the padding k of an odd 27 Cin multiplying zeros;
#   affine    bf16 entry: bf16_rne of the raw value first (:153); act32 (:156); the tile's column 0 and a row above the map are 0;
#   planes    workgroup (oh0, od_begin) walks p = 2 od_begin - 1 .. 2 od_begin + 2 SD - 1, plane -1 skipped (:137-143, :211);
#   dw        p even: kd = 1 of output plane p / 2 into slot (p / 2) & 1; p odd: kd = 2 of plane (p - 1) / 2 into its slot - which is
#             then stored and reset (:240-245) - and kd = 0 of plane (p + 1) / 2 into the other slot, unless that plane belongs to
#             the next workgroup (use_b, :215); each a chain of nine fmaf in (kh, kw) order (:234, :238).
MUTANTS = (
    "slots_swapped",       # case 3 of the switch (:256) instantiated with slot 0, as case 1 is
    "no_reset",            # ``acc[SA] = 0`` (:244) missing: the plane two further on starts from the stored one
    "use_a_uncut",         # use_a (:214) without ``od_a >= od_begin``: the first plane stores kd = 2 alone over the previous segment's plane
    "plane_m1",            # plane -1 is computed (from a zero tile: relu(sh)) and feeds kd = 0 of output plane 0
    "halo_row_act",        # the row above the map holds relu(sh) (``continue`` of :169 missing)
    "halo_col_act",        # the left padding column holds relu(sh)
    "row_wrong_side",      # the halo row of a row group below the first holds activation row 2 oh0 + 1 for 2 oh0 - 1
    "kd_swapped",          # odd planes: kd = 0 to the plane they complete, kd = 2 to the plane they open
    "drop_tap",            # tap (2, 2, 2) missing in the last column group (g = ncg - 1)
    "ci1_dropped",         # Cin = 2: the chain stops at k = 27
    "pad_k_live",          # Cin = 1: the A operand of the padding k = 27 is w[c * 27 + 27] (the next channel's first weight), not 0
    "no_y_round",          # bf16: the raw stem value is not rounded to bf16
    "round_after_affine",  # bf16: bf16 rounding after the affine + ReLU instead of before
)
# what the code could do differently WITHOUT changing a bit of the output: use_b (:215) not cut at the workgroup's last plane adds
# that plane's kd = 0 taps into a slot the workgroup never stores again.  The CPU test asserts the equality; the mutant that
# mirrors it at the first plane (use_a_uncut) is the observable one.
NEUTRAL = ("use_b_uncut",)


def emul_stem(x, w, mut=None):
    """-> the raw stem values (N, 32, AD, AH, AW) fp32: one fmaf chain in k order."""
    N, cin = x.shape[:2]
    AD, AH, AW = stem_ref.out_dims(tuple(x.shape[2:]), S222)
    cols = stem_ref.im2col(x.float(), S222)  # (N, 27 cin, OS)
    K = 27 * cin
    wk = w.float().reshape(COUT, K)
    acc = torch.zeros((N, COUT, cols.shape[2]))
    for k in range(27 if mut == "ci1_dropped" else K):
        acc = fma32(wk[:, k].view(1, -1, 1), cols[:, k:k + 1], acc)
    if mut == "pad_k_live" and cin == 1:  # k = 27 = tap (0, 0, 0, 0) of LDS offset 0 (:71); channel 31 reads past w: here w[0]
        nxt = wk.reshape(-1)[(torch.arange(COUT) * K + K) % (COUT * K)]
        acc = fma32(nxt.view(1, -1, 1), cols[:, 0:1], acc)
    return acc.view(N, COUT, AD, AH, AW)


def emul_act(y, sc, sh, bf16, mut=None):
    if bf16 and mut == "round_after_affine":
        return bf16_rne(act32(y, sc, sh))
    if bf16 and mut != "no_y_round":
        y = bf16_rne(y)
    return act32(y, sc, sh)


def emul_dw(a, sh, wd, p, bf16, mut=None):
    """a (N, 32, AD, AH, AW) fp32 activation, p = plan(..) of the WHOLE case -> z as stored (fp32; bf16 values held as fp32)."""
    N, C, AD, AH, AW = a.shape
    TH, SD = p["th"], p["sd"]
    ZD, ZH, ZW = AD // 2, AH // 2, AW // 2
    G, NRW, ncg = ZH // TH, 2 * TH + 1, ZW // 16
    wk = wd.float().view(C, 27)
    relu_sh = torch.where(sh < 0, torch.zeros_like(sh), sh).float().view(1, C, 1, 1)
    # tile row hr of row group g = activation row 2 TH g - 1 + hr = row 2 TH g + hr of the plane padded by one row and one column
    rows = (2 * TH * torch.arange(G).view(G, 1) + torch.arange(NRW).view(1, NRW))
    if mut == "row_wrong_side":
        rows[1:, 0] += 2

    def tiles(pl):
        """-> (N, C, G, NRW, AW + 1): the activation plane as every row group holds it in LDS."""
        t = torch.zeros((N, C, AH + 1, AW + 1))
        if pl >= 0:
            t[:, :, 1:, 1:] = a[:, :, pl]
        else:  # plane_m1: the stem of a zero tile is 0, its activation relu(sh)
            t[:, :, 1:, 1:] = relu_sh
        if mut == "halo_row_act":
            t[:, :, 0, 1:] = relu_sh[:, :, 0]
        if mut == "halo_col_act":
            t[:, :, 1:, 0] = relu_sh[:, :, 0]
        return t[:, :, rows]

    def taps9(t):
        """tap (kh, kw) of output (r, ow) at t[2 r + kh][2 ow + kw] -> nine (N, C, G, TH, ZW)."""
        return [t[:, :, :, kh:kh + 2 * TH - 1:2, kw:kw + 2 * ZW - 1:2] for kh in range(3) for kw in range(3)]

    def chain(acc, kd, t9):
        for k in range(9):
            nxt = fma32(wk[:, kd * 9 + k].view(1, C, 1, 1, 1), t9[k], acc)
            if mut == "drop_tap" and kd == 2 and k == 8:
                nxt = torch.cat([nxt[..., :16 * (ncg - 1)], acc[..., 16 * (ncg - 1):]], -1)
            acc = nxt
        return acc

    z = torch.full((N, C, ZD, ZH, ZW), float("nan"))
    for od_begin in range(0, ZD, SD):
        acc = [torch.zeros((N, C, G, TH, ZW)) for _ in range(2)]
        p_first = 2 * od_begin - 1
        pi0 = 1 if (p_first < 0 and mut != "plane_m1") else 0
        for pl in range(p_first + pi0, p_first + 2 * SD + 1):
            odd = bool(pl & 1)
            od_a, od_b = pl >> 1, (pl + 1) >> 1
            use_a = (od_a >= od_begin or mut == "use_a_uncut") and od_a < od_begin + SD and od_a >= 0
            use_b = odd and od_b >= od_begin and (od_b < od_begin + SD or mut == "use_b_uncut")
            SA = (pl >> 1) & 1
            if mut == "slots_swapped" and (pl & 3) == 3:
                SA = 0
            SB = 1 - SA
            kda, kdb = (2, 0) if odd else (1, 0)
            if mut == "kd_swapped" and odd:
                kda, kdb = 0, 2
            t9 = taps9(tiles(pl))
            if use_a:
                acc[SA] = chain(acc[SA], kda, t9)
            if use_b:
                acc[SB] = chain(acc[SB], kdb, t9)
            if odd and use_a:
                out = acc[SA].reshape(N, C, ZH, ZW)
                z[:, :, od_a] = bf16_rne(out) if bf16 else out
                if mut != "no_reset":
                    acc[SA] = torch.zeros_like(acc[SA])
    return z


def emulate(x, w, sc, sh, wd, p, bf16, mut=None, stem=None):
    """-> (z as stored, y as msl_stem_conv_fwd[_bf16] stores it - always the honest one).  ``stem``: a cached emul_stem(x, w)."""
    y = stem if stem is not None else emul_stem(x, w)
    ym = emul_stem(x, w, mut) if mut in ("ci1_dropped", "pad_k_live") else y
    z = emul_dw(emul_act(ym, sc, sh, bf16, mut), sh, wd, p, bf16, mut)
    return z, (bf16_rne(y) if bf16 else y)


def expressible(mut, cin, p, bf16, dims):
    """False where a case cannot show a mutant, each for the reason written next to it."""
    ZD = dims[0] // 4
    if mut == "no_reset":            # a slot is used again two output planes on, inside the same workgroup
        return p["sd"] >= 3
    if mut == "use_a_uncut":         # the plane written over belongs to an earlier segment
        return ZD // p["sd"] >= 2
    if mut == "row_wrong_side":      # only a row group below the first has a recomputed halo row
        return p["grid"][0] >= 2
    if mut == "ci1_dropped":
        return cin == 2
    if mut == "pad_k_live":
        return cin == 1
    if mut in ("no_y_round", "round_after_affine"):
        return bool(bf16)
    return True
