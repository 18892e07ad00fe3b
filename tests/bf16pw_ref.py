"""Float64 reference, derived bounds and checkers of the bf16 pointwise GEMM family, the materialise kernels and the four
BatchNorm+ReLU-backward kernels of csrc/bf16.hip.  Plain torch on the CPU: nothing here imports the package.  The same checkers
judge the GPU outputs (tests/test_gpu_bf16pw.py) and, on the CPU, an honest fp32 emulation and fourteen wrong kernels
(tests/test_bf16pw_ref_cpu.py); both emulations live at the end of this file.

Operands are reproduced, not bounded (bf16.hip line numbers of the parent of this file's first commit):
* forward (pw_fwd_bf16_kernel :184-207, pw_bf16_tr_kernel :331, :342): A = bf16_rne(act32(z, sc, sh)), Wb = bf16_rne(w);
* backward data (TRANS_W, no affine): dy as given, Wb;
* weight gradient (pw_bww_bf16_kernel :497, pw_bww_bf16_any_kernel :546): dy and bf16_rne(act32(z, ..)), or z itself.
``pw_ref.act32`` is msl::act bit for bit, so no element is excluded and no margin around zero is needed.

GEMM bound.  y64 = Wb . A in float64, absdot = |Wb| . |A|; the products of two bf16 values are exact in fp32, the fp32
accumulator meets at most one rounding per term: B = (K + J) U absdot (pw_ref.gemm_bound), J = 0 in both tile kernels (the MFMA
chain over K is serial in a wave: ``acc = mfma(a, b, acc)`` :214 / :361, one accumulator, no K split).  Weight gradient:
(L + ns) U absdot with L = chunks per slab * 64 (bww_route of csrc/pwroute.hpp; the four waves of a workgroup interleave the slab's
chunks and meet in three additions :517-520, L / 4 + 3 <= L) and ns = msl_pwconv_bwd_weight_bf16_nslabs; the any-kernel is one
fmaf chain over N * ceil(S / 64) * 64 positions (:536-554), one slab.

bf16 outputs: the rounding-interval test.  The kernel stores RNE_bf16(acc) of an fp32 acc with |acc - y64| <= B.  Rounding is
monotonic, so  bf16_rne(y64 - B) <= stored <= bf16_rne(y64 + B)  as values.  The ends are first rounded to fp32 (to nearest):
acc is an fp32 value, so y64 - B <= acc implies RN32(y64 - B) <= acc, and the interval stays valid (and is never wider).  Where
both ends coincide the element is pinned to one bf16 value.  No element is left out; a NaN passes only where the reference is
NaN, and an infinite reference demands itself.

Statistics partials of msl_pwconv_fwd_bf16 (:219-231, :364-376): slot (n * ceil(S / 64) + tile) * 2 + wn holds the sums over the
32 columns tile * 64 + wn * 32 .. + 31 of the UNROUNDED fp32 accumulators - the same layout in both kernels.  They are compared
with the float64 sums of y64 over those columns: sum B + 5 U sum |y64| (half32_sum: five fp32 additions, common.hpp :124-128)
and sum (2 |y64| B + B^2) + 6 U sum y64^2 (one more rounding for ``v * v``).

BatchNorm backward (:684-823) reuses tests/bn_ref.py: the mask is ``fmaf(y, sc, sh) > 0`` (bn_ref._masked evaluates it in
float64, which has the same sign; the CPU test asserts that against pw_ref.fma32 for every case).  A thread's fp32 additions
n_t: reduce 4096 / 256 = 16 (:696), generic fused N * ceil(S / 256) (:735-742), register form 8 * IPT (:791-801); everything
after is double.  dy: the rounding-interval test with bwd_apply_bound as B (six fp32 operations :721 / :760 / :820; contraction
to fma only removes roundings); for the fused kernels the error of their own k1 = (float)(t1 / count), k2 is propagated through
dc1 / dc2.  dgamma / dbeta of the fused kernels: the sums bound plus U |sum| for the cast.

Materialise (:407-450): ``plain`` and ``pad32`` are act32 bit for bit, ``pad_cl`` is bf16_rne(act32) bit for bit."""
import torch

from tests import bn_ref as R
from tests import pw_ref as P
from tests.pw_ref import act32, fma32  # noqa: F401  (re-exported)

U = R.U
NAN = float("nan")


def cdiv(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------------------------------------- bf16
def bf16_rne(t):
    """Round-to-nearest-even of fp32 to bf16, returned as fp32 (proved against ``round_bits`` in the CPU test)."""
    return t.to(torch.bfloat16).float()


def bits16(t):
    """The bf16 bit patterns (int64, 0 .. 0xFFFF) of a tensor of bf16 values held as bf16 or fp32."""
    return t.to(torch.bfloat16).contiguous().view(torch.int16).to(torch.int64) & 0xFFFF


def _i32(t):
    return t.float().contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF


def _f32(i):
    i = i & 0xFFFFFFFF
    return torch.where(i >= 2 ** 31, i - 2 ** 32, i).to(torch.int32).view(torch.float32)


def round_bits(t, drop, mode="rne"):
    """Integer rounding of finite fp32 values on their bit patterns: the low ``drop`` mantissa bits go, to nearest even
    ("rne"), half away from zero ("away") or by truncation ("trunc").  drop = 16 is the conversion to bf16."""
    i = _i32(t)
    if mode == "rne":
        i = i + ((1 << (drop - 1)) - 1) + ((i >> drop) & 1)
    elif mode == "away":
        i = i + (1 << (drop - 1))
    return _f32((i >> drop) << drop)


def interval(y64, B):
    """-> (lo, hi) fp32 holding bf16 values: bf16_rne(RN32(y64 -+ B)); a non-finite reference is its own interval."""
    fin = torch.isfinite(y64)
    B = torch.as_tensor(B, dtype=torch.float64).expand_as(y64)
    lo = torch.where(fin, y64 - B, y64).float()
    hi = torch.where(fin, y64 + B, y64).float()
    return bf16_rne(lo), bf16_rne(hi)


def check_interval(stored, y64, B):
    """stored: the kernel's bf16 output (any float dtype).  -> dict(bad, idx, pinned, ratio, lo, hi): violations, flat index of
    the worst, share of elements whose interval is one bf16 value, and max |stored - y64| / (B + half a bf16 ulp)."""
    s = stored.detach().cpu().float().reshape(-1)
    y = y64.double().reshape(-1)
    B_ = torch.as_tensor(B, dtype=torch.float64).expand_as(y64).reshape(-1)
    lo, hi = interval(y, B_)
    nan_r = torch.isnan(y)
    ok = torch.where(nan_r, torch.isnan(s), (s >= lo) & (s <= hi))
    # the figure that is logged: |stored - ref| over B plus half a bf16 ulp of the stored value's binade (2**(e - 9) for
    # |stored| = m 2**e, 0.5 <= m < 1), the most one honest rounding can add; the assertion is the interval, not this figure
    half_ulp = torch.ldexp(torch.ones_like(y), torch.frexp(s.double())[1].to(torch.int64) - 9)
    reach = torch.where(torch.isfinite(y), B_ + half_ulp, torch.zeros_like(y))
    err = (s.double() - y).abs()
    ratio = torch.where(reach > 0, err / reach, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    ratio = torch.where(ok & ~torch.isfinite(ratio), torch.zeros_like(ratio), ratio)  # NaN == NaN, inf == inf
    ratio = torch.where(~ok & ~(ratio > 1), torch.full_like(ratio, float("inf")), ratio)  # outside the interval: the worst
    k = int(ratio.argmax()) if ratio.numel() else 0
    return dict(bad=int((~ok).sum()), idx=k, pinned=float((lo == hi).double().mean()) if s.numel() else 1.0,
                ratio=float(ratio[k]) if ratio.numel() else 0.0, lo=lo, hi=hi)


def worst(actual, ref, bound):
    """bn_ref.worst, with an infinite reference demanding itself (inf - inf is no error)."""
    a, r = actual.detach().cpu().double().reshape(-1).clone(), ref.double().reshape(-1).clone()
    b = torch.as_tensor(bound, dtype=torch.float64).expand_as(ref).reshape(-1).clone()
    same_inf = torch.isinf(r) & (a == r)
    a[same_inf], r[same_inf], b[same_inf] = 0.0, 0.0, 1.0
    b[torch.isnan(b) | torch.isinf(b)] = 0.0  # a non-finite bound next to a finite reference: demand equality rather than nothing
    return R.worst(a, r, b)


class Report:
    """The comparisons of one case: ``rows`` of dict(what, bad, ratio, idx, pinned, msg); ``failures()`` the bad ones."""

    def __init__(self, case_id):
        self.id, self.rows = case_id, []

    def _add(self, what, bad, ratio, idx, pinned, msg):
        self.rows.append(dict(what=what, bad=bad, ratio=ratio, idx=idx, pinned=pinned, msg=f"{self.id} {what}: {msg}"))

    def bound(self, what, actual, ref, bound):
        ratio, idx, bad = worst(actual, ref, bound)
        a, r = actual.detach().cpu().double().reshape(-1), ref.double().reshape(-1)
        self._add(what, bad, ratio, idx, None, f"{bad}/{r.numel()} over their bound; worst error / bound {ratio:.3f} at idx {idx} "
                                               f"(got {a[idx].item():.9e}, ref {r[idx].item():.9e})")

    def interval(self, what, stored, y64, B):
        c = check_interval(stored, y64, B)
        k = c["idx"]
        s = stored.detach().cpu().float().reshape(-1)
        self._add(what, c["bad"], c["ratio"], k, c["pinned"],
                  f"{c['bad']}/{s.numel()} outside their rounding interval; worst at idx {k}: stored {s[k].item():.9e} "
                  f"(bits 0x{int(bits16(s[k:k + 1])):04X}), interval [{c['lo'][k].item():.9e}, {c['hi'][k].item():.9e}], "
                  f"ref {y64.double().reshape(-1)[k].item():.12e}; pinned share {c['pinned']:.4f}")
        return c

    def bits(self, what, got_bits, want_bits):
        g, w = got_bits.reshape(-1).cpu(), want_bits.reshape(-1).cpu()
        ne = g != w
        bad = int(ne.sum())
        k = int(ne.to(torch.int64).argmax()) if bad else 0
        self._add(what, bad, float("inf") if bad else 0.0, k, 1.0,
                  f"{bad}/{g.numel()} bit patterns differ; first at idx {k}: got 0x{int(g[k]):X}, want 0x{int(w[k]):X}")

    def failures(self):
        return [r["msg"] for r in self.rows if r["bad"]]


def f32bits(t):
    return t.detach().cpu().float().contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------- GEMM references
def fwd_operands(z, sc, sh, w, affine=True):
    """-> (A, Wb): the MFMA operands of the forward kernels, as fp32 tensors of bf16 values."""
    return (bf16_rne(act32(z, sc, sh)) if affine else z), bf16_rne(w)


def fwd_expect(A, Wb, K, J=0):
    y, absdot = P.fwd_ref(A, Wb)
    return dict(y=y, B=P.gemm_bound(absdot, K, J))


def bwd_data_expect(dy, Wb, K, J=0):
    g, absdot = P.bwd_data_ref(dy, Wb)
    return dict(y=g, B=P.gemm_bound(absdot, K, J))


def stats_slots(t, S):
    """(N, M, S) float64 -> (M, N * ceil(S / 64) * 2): sums over every slot's 32 columns (zeros past S)."""
    N, M, _ = t.shape
    per = cdiv(S, 64)
    tp = torch.nn.functional.pad(t, (0, per * 64 - S)).view(N, M, per * 2, 32)
    return tp.sum(-1).permute(1, 0, 2).reshape(M, N * per * 2)


STATS_DEPTH_SUM, STATS_DEPTH_SQ = 5, 6


def stats_expect(y64, B, S):
    """-> (ref, bound) float64 (2, M, NP) of the statistics partials, from the reference output (NOT the stored one)."""
    fin = torch.isfinite(y64)
    Bz = torch.where(fin, B, torch.zeros_like(B))
    ay = y64.abs()
    ref = torch.stack([stats_slots(y64, S), stats_slots(y64 * y64, S)])
    bnd = torch.stack([stats_slots(Bz, S) + STATS_DEPTH_SUM * U * stats_slots(ay, S),
                       stats_slots(2 * ay * Bz + Bz * Bz, S) + STATS_DEPTH_SQ * U * stats_slots(y64 * y64, S)])
    return ref, bnd


def check_fwd(rep, e, y_stored, partials=None, exact_bits=None):
    """y_stored (N, M, S) bf16 values; partials (2, M, NP) fp64 or None; e = fwd_expect / bwd_data_expect."""
    N, M, S = e["y"].shape
    rep.interval("y", y_stored, e["y"], e["B"])
    if exact_bits is not None:
        rep.bits("y-bits", bits16(y_stored), exact_bits)
    if partials is not None:
        ref, bnd = stats_expect(e["y"], e["B"], S)
        rep.bound("partials", partials, ref, bnd)
        if bool(torch.isfinite(ref).all()):
            rep.bound("folded-stats", R.exact_sum(partials.detach().cpu()), ref.sum(-1), bnd.sum(-1))


def bww_expect(dy, z, sc, sh, affine, L, ns):
    a = bf16_rne(act32(z, sc, sh)) if affine else z
    dw, absdot = P.bww_ref(dy, a)
    return dict(dw=dw, B=(L + ns) * U * absdot)


def check_bww(rep, e, slabs):
    """slabs (ns, Cout, Cin) fp32: their float64 sum against the reference."""
    rep.bound("dW", slabs.detach().cpu().double().sum(0), e["dw"], e["B"])


# ------------------------------------------------------------------------------------------------- materialise
def mat_expect(y, sc, sh):
    """-> (act32 (N, C, S) fp32, its bf16 rounding): the ``plain`` / ``pad32`` interior and the ``pad_cl`` interior."""
    a = act32(y, sc, sh)
    return a, bf16_rne(a)


def pad_interior(t, dims):
    """(N, C, S) -> the interior view's values laid into a zero-haloed (N, C, D+2, H+2, W+2) tensor, and the interior mask."""
    N, C, _ = t.shape
    D, H, W = dims
    out = torch.zeros((N, C, D + 2, H + 2, W + 2), dtype=t.dtype)
    out[:, :, 1:-1, 1:-1, 1:-1] = t.view(N, C, D, H, W)
    m = torch.zeros_like(out, dtype=torch.bool)
    m[:, :, 1:-1, 1:-1, 1:-1] = True
    return out, m


# ------------------------------------------------------------------------------------------------- BatchNorm backward
def mask_is_kernels(y, vec):
    """bn_ref._masked's float64 mask against ``fmaf(y, sc, sh) > 0`` evaluated bit-exactly."""
    sc, sh = R._bc(vec[0], y), R._bc(vec[1], y)
    return bool(torch.equal(y.double() * sc + sh > 0, fma32(y, sc.float(), sh.float()) > 0))


def reduce_expect(g, y, vec):
    """-> (ref, bound) float64 (2, C, NP): per-chunk (sum gm, sum gm xhat), slot n * chunks + ck, n_t = 16."""
    N, C, S = y.shape
    chunks = cdiv(S, 4096)
    ref, bnd = torch.zeros((2, C, N * chunks), dtype=torch.float64), torch.zeros((2, C, N * chunks), dtype=torch.float64)
    for n in range(N):
        for ck in range(chunks):
            sl = (slice(n, n + 1), slice(None), slice(ck * 4096, min(S, (ck + 1) * 4096)))
            s, q = R.bwd_sums_ref(g[sl], y[sl], vec)
            bs, bq = R.bwd_sums_bound(g[sl], y[sl], vec, 16)
            p = n * chunks + ck
            ref[0, :, p], ref[1, :, p], bnd[0, :, p], bnd[1, :, p] = s, q, bs, bq
    return ref, bnd


def apply_expect(g, y, vec):
    """vec (6, C): the kernel's own k1, k2 -> dict(y, B)."""
    return dict(y=R.bwd_apply_ref(g, y, vec, vec[4], vec[5]), B=R.bwd_apply_bound(g, y, vec, vec[4], vec[5]))


def fused_expect(g, y, vec, n_t):
    """-> dict(dbeta, dgamma, b_dbeta, b_dgamma, y, B): the kernel forms k1, k2 itself, so their error (sums bound over the
    count, the fp32 cast of the sum and of the quotient) is propagated into dy."""
    N, _, S = y.shape
    count = float(N * S)
    s, q = R.bwd_sums_ref(g, y, vec)
    bs, bq = R.bwd_sums_bound(g, y, vec, n_t)
    c1, c2 = s / count, q / count
    dc1, dc2 = bs / count + U * c1.abs(), bq / count + U * c2.abs()
    return dict(dbeta=s, dgamma=q, b_dbeta=bs + U * s.abs(), b_dgamma=bq + U * q.abs(),
                y=R.bwd_apply_ref(g, y, vec, c1, c2), B=R.bwd_apply_bound(g, y, vec, c1, c2, dc1, dc2))


def check_fused(rep, e, dy, dgamma, dbeta):
    rep.bound("dbeta", dbeta, e["dbeta"], e["b_dbeta"])
    rep.bound("dgamma", dgamma, e["dgamma"], e["b_dgamma"])
    rep.interval("dy", dy, e["y"], e["B"])


# ================================================================================================= CPU emulations
# An honest fp32 evaluation of every entry point, and the wrong kernels of the CPU test (``mut``).  Mutant names:
#   trunc, twice, away (the store); a_unrounded, w_unrounded, muladd (operands); mask_bf16 (BatchNorm mask from bf16-rounded
#   scale / shift); stats_stored; drop_chunk; tail_col; tail_row; slab_twice; xhat_unrounded; swap.
# ``mask_bf16``: rounding the VALUE of the pre-activation to bf16 cannot change its sign (bf16 has fp32's exponent range), so a
# kernel that did only that is the same kernel; the wrong kernel that can exist is one whose pre-activation is evaluated from
# bf16-rounded operands, and that is what is emulated.
def store(acc, mut=None):
    if mut == "trunc":
        return round_bits(acc, 16, "trunc")
    if mut == "twice":
        return bf16_rne(round_bits(acc, 15, "rne"))
    if mut == "away":
        return round_bits(acc, 16, "away")
    return bf16_rne(acc)


def _act_mut(z, sc, sh, mut):
    if mut == "muladd":
        v = z * R._bc(sc, z).float() + R._bc(sh, z).float()  # two fp32 roundings
        return torch.where(v < 0, torch.zeros_like(v), v)
    return act32(z, sc, sh)


def _tails(y, mut):
    y = y.clone()
    if mut == "tail_col" and y.shape[-1] > 1:
        y[..., -1] = y[..., -2]
    if mut == "tail_row":
        y[:, -1] = NAN  # the NaN the buffer was filled with
    return y


def emul_gemm(Wb, A, chunk=32, drop_last=False):
    """k-ordered fp32 accumulation in chunks of ``chunk``: (M, K) x (N, K, S) -> fp32 (N, M, S)."""
    K = Wb.shape[1]
    ks = list(range(0, K, chunk))
    if drop_last:
        ks = ks[:-1]
    acc = torch.zeros((A.shape[0], Wb.shape[0], A.shape[2]))
    for k0 in ks:
        acc = acc + torch.matmul(Wb[:, k0:k0 + chunk], A[:, k0:k0 + chunk])
    return acc


def _tree32(v):
    for m in (16, 8, 4, 2, 1):
        v = v[..., :m] + v[..., m:2 * m]
    return v[..., 0]


def emul_stats(acc, S):
    """fp32 accumulators (N, M, S) -> fp64 (2, M, NP): a 5-level fp32 tree over each slot's 32 columns, squares rounded first."""
    N, M, _ = acc.shape
    per = cdiv(S, 64)
    v = torch.nn.functional.pad(acc, (0, per * 64 - S)).view(N, M, per * 2, 32)
    slot = lambda t: _tree32(t).permute(1, 0, 2).reshape(M, N * per * 2)
    return torch.stack([slot(v), slot(v * v)]).double()


def emul_fwd(z, sc, sh, w, affine=True, stats=True, mut=None):
    a = _act_mut(z, sc, sh, mut) if affine else z
    A = a if mut == "a_unrounded" else bf16_rne(a)
    Wb = w if mut == "w_unrounded" else bf16_rne(w)
    acc = emul_gemm(Wb, A, drop_last=mut == "drop_chunk")
    y = store(acc, mut)
    part = emul_stats(y if mut == "stats_stored" else acc, z.shape[-1]) if stats else None
    return _tails(y, mut), part


def emul_bwd_data(dy, w, mut=None):
    Wb = w if mut == "w_unrounded" else bf16_rne(w)
    acc = emul_gemm(Wb.t().contiguous(), dy, drop_last=mut == "drop_chunk")
    return _tails(store(acc, mut), mut)


def emul_bww(dy, z, sc, sh, affine, ns, cpb, mut=None):
    """ns slabs of cpb 64-position chunks each (positions of all images in a row), fp32 inside a slab."""
    N, Cout, S = dy.shape
    a = _act_mut(z, sc, sh, mut) if affine else z
    a = a if mut == "a_unrounded" else bf16_rne(a)
    df = dy.permute(1, 0, 2).reshape(Cout, N * S)
    af = a.permute(1, 0, 2).reshape(a.shape[1], N * S)
    L = cpb * 64
    slabs = []
    for k in range(0, N * S, L):
        hi = min(N * S, k + L)
        if mut == "drop_chunk" and hi == N * S:
            hi = max(k, hi - 64)
        slabs.append(torch.matmul(df[:, k:hi], af[:, k:hi].t()))
    if mut == "slab_twice":
        slabs[-1] = slabs[-1] * 2
    return torch.stack(slabs)


def emul_materialize(y, sc, sh, mut=None):
    """-> (plain fp32, pad_cl values)"""
    a = _act_mut(y, sc, sh, mut)
    return _tails(a, mut), _tails(store(a, mut), mut)


def _bn_terms(g, y, vec, mut):
    sc, sh, mu, is_ = (R._bc(vec[k], y).float() for k in range(4))
    pre = fma32(y, bf16_rne(sc), bf16_rne(sh)) if mut == "mask_bf16" else fma32(y, sc, sh)
    gm = torch.where(pre > 0, g, torch.zeros_like(g))
    return gm, (y - mu) * is_, sc, mu, is_


def _thread_sums(t, layout):
    """fp32 terms (N, C, S) -> float64 (C,): per-thread fp32 sums in the kernel's order, then double.
    layout = ("strided", 256): thread i adds elements i, i + 256, .. of every image in turn (reduce, generic fused);
             ("reg", NT, IPT): thread t adds the 8 elements of groups t, t + NT, .. of the channel's N * S / 8 groups."""
    N, C, S = t.shape
    if layout[0] == "strided":
        nb = cdiv(S, 256)
        v = torch.nn.functional.pad(t, (0, nb * 256 - S)).view(N, C, nb, 256)
        acc = torch.zeros((C, 256))
        for n in range(N):
            for b in range(nb):
                acc = acc + v[n, :, b]
        return acc.double().sum(-1)
    _, NT, IPT = layout
    v = t.permute(1, 0, 2).reshape(C, N * S // 8, 8)
    v = torch.nn.functional.pad(v, (0, 0, 0, NT * IPT - v.shape[1])).view(C, IPT, NT, 8)
    acc = torch.zeros((C, NT))
    for u in range(IPT):
        for k in range(8):
            acc = acc + v[:, u, :, k]
    return acc.double().sum(-1)


def emul_reduce(g, y, vec, mut=None):
    N, C, S = y.shape
    chunks = cdiv(S, 4096)
    gm, xhat, *_ = _bn_terms(g, y, vec, mut)
    out = torch.zeros((2, C, N * chunks), dtype=torch.float64)
    for n in range(N):
        for ck in range(chunks):
            sl = (slice(n, n + 1), slice(None), slice(ck * 4096, min(S, (ck + 1) * 4096)))
            out[0, :, n * chunks + ck] = _thread_sums(gm[sl], ("strided", 256))
            out[1, :, n * chunks + ck] = _thread_sums(gm[sl] * xhat[sl], ("strided", 256))
    return out.flip(0) if mut == "swap" else out


def _apply32(gm, y, sc, mu, is_, k1, k2, y32, mut):
    xh = ((y32 if mut == "xhat_unrounded" else y) - mu) * is_
    return _tails(store(sc * (gm - k1 - xh * k2), mut), mut)


def emul_apply(g, y, vec, y32=None, mut=None):
    gm, _, sc, mu, is_ = _bn_terms(g, y, vec, mut)
    return _apply32(gm, y, sc, mu, is_, R._bc(vec[4], y).float(), R._bc(vec[5], y).float(), y32, mut)


def emul_fused(g, y, vec, layout, y32=None, mut=None):
    """-> (dy, dgamma, dbeta)"""
    N, _, S = y.shape
    gm, xhat, sc, mu, is_ = _bn_terms(g, y, vec, mut)
    t1, t2 = _thread_sums(gm, layout), _thread_sums(gm * xhat, layout)
    k1, k2 = (t1 / (N * S)).float(), (t2 / (N * S)).float()
    dy = _apply32(gm, y, sc, mu, is_, R._bc(k1, y).float(), R._bc(k2, y).float(), y32, mut)
    dbeta, dgamma = t1.float(), t2.float()
    return (dy, dbeta, dgamma) if mut == "swap" else (dy, dgamma, dbeta)
