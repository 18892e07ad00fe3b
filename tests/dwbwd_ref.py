"""Float64 reference of the depthwise-convolution BACKWARD kernels (csrc/dwconv_bwd.hip, the weight-gradient and flipped-forward
kernels of csrc/dwconv.hip that it launches, and the bf16 backward kernels of csrc/bf16.hip), with derived error bounds.  Plain
torch on the CPU; like tests/pw_ref.py and tests/bn_ref.py (whose helpers it reuses) nothing here imports the package.

    bwd-data   g[n,c,i]  = sum_k w[c,k] dy[n,c,(i + 1 - k) / s]      (taps with an integral, in-range output index only)
    bwd-weight dW[c,k]   = sum_{n,o} dy[n,c,o] a[n,c,s o - 1 + k]    a = relu(fma(x, scale, shift)), zero outside the volume

Both are evaluated from ``tap_planes``: for every tap k the gradient dy laid out on the INPUT grid (T_k[i] = dy[(i + 1 - k) / s],
zero where that output does not exist), 27 strided slice copies.  No autograd and no conv_transpose3d: the reference shares no
code with the torch ops the older tests of these kernels compare with (tests/test_dwbwd_ref_cpu.py checks it against them).

Bounds (``U = 2**-24``, half an fp32 ulp, relative; ``gamma(n) = n U / (1 - n U)``).
* bwd-data: gamma(n) absdot, absdot = sum_k |w_k| |dy| (+ |old| with accumulate), n = the element's own number of contributing
  taps (1, 2, 4 or 8 by parity at stride 2, at most 27 at stride 1), plus one for ``accumulate``.  Whatever the order, and with or
  without fma contraction, a term passes at most one rounding per NON-zero term it meets (its own product included); a kernel
  that walks all 27 taps over a zero halo adds exact zeros, which round nothing.  So n is the same for every bwd-data kernel.
* bf16 storage: the fp32 result is rounded once more, to 8 significant bits: BF16_U (|result| + fp32 bound), BF16_U = 2**-8.
  (Half that, 2**-9 |result|, is the SMALLEST error a worst-placed value of a binade gets, not the largest: 1 + 2**-8 lies
  midway between the bf16 neighbours 1 and 1 + 2**-7 - tests/test_dwbwd_ref_cpu.py::test_bf16_unit_roundoff.)
* weight gradient: gamma(n) absdot with n = BWW_DEPTH[path], the longest chain of fp32 roundings a product passes before the
  value becomes a double; the table below is read off the kernels, line by line.  The fp64 fold of the partials is 2**-29 of
  this and is not counted; the final cast of msl_dwconv_bwd_weight_finalize adds U |sum|.
* BatchNorm-backward sums (sum gm, sum gm xhat) of the fused passes, per partial, against the float64 sums of the kernel's OWN
  stored gradient (bf16-rounded on bf16 storage): (n_t + 4) U sum |term| as in bn_ref.bwd_sums_bound, n_t = SUMS_DEPTH[path].
  Sums taken from the stored gradient carry only this summation bound, not the gradient's error (as test_gpu_pw.check_stats
  treats the statistics partials).  Where the gradient is not stored (the one-pass kernel without g_in) the sums are compared
  with those of the float64 gradient and the gradient's own bound is propagated: sum [mask] b and sum |xhat| [mask] b.

The activation and the ReLU mask are reproduced, not bounded: ``act32`` / ``fma32`` of tests/pw_ref.py return the very fp32 values
msl::act and ``fmaf(y, scale, shift) > 0`` produce, so no element is excluded and no margin around zero is needed.
"""
import torch

from tests.bn_ref import U, _bc, exact_sum, worst  # noqa: F401  (re-exported for the tests)
from tests.pw_ref import act32, fma32  # noqa: F401

BF16_U = 2.0 ** -8

# DwKind of csrc/dwroute.hpp, as msl_dwconv_route_kind returns it
KIND = dict(none=0, wave=1, rows_eval=2, small_eval=3, stream=4, resident=5, naive=6, tiled=7, tiled_s2=8, s2patch=9,
            datavec=10, datanaive=11, chunks=12)
OP_BWD_DATA, OP_BWD_WEIGHT = 2, 3

# Longest chain of fp32 roundings between a product dy * a and the first double, per weight-gradient kernel.
BWW_DEPTH = {
    # dw_bwd_weight_kernel (dwconv_bwd.hip): a lane walks o = lo + lane, lo + lane + 64, ... < lo + BW_CHUNK = 1024: 16 fmaf
    # into acc[k]; then ``msl::wave_sum((double)acc[k])``
    "chunks": 16,
    # dw_fwd_resident_kernel<S, 1> (dwconv.hip): ``a27[k] += dot4(dv, r.v[kw])`` - dot4 is a product and three fmaf (4), the
    # += one more per item of the thread; a thread takes ceil(G L / 256) items (``for item = threadIdx.x; ...; += 256``) and
    # emit_bww adds ``(double)red[...]``.  Items: see bww_depth().
    "resident": None,
    # dw_fwd_stream_kernel<S, IPT, LPT, 1>: the same dot4 (4) and one += per (item t < IPT, output plane of the slab): see bww_depth()
    "stream": None,
    # dw_s1_wave_bww_kernel: ``a27[k] += fmaf(d.w, .., fmaf(d.z, .., fmaf(d.y, .., d.x * ..)))`` (4 + 1) once per output plane
    # o < SL of the slab, SL <= 8 (wave_plan: SLAB = 8 from D >= 16); then ``group_sum<P4>((double)a27[k])``
    "wave_s1": 4 + 8,
    # dw_s2_wave_bww_kernel: ``a27[k] += fmaf(d.y, .., d.x * ..)`` (2 + 1) once per output plane, SL <= 4; then doubles
    "wave_s2": 2 + 4,
    # dw_s2_bwd_reduce_bww_kernel<4>: every tap meets exactly one (pd, ph, td, th) of a patch and takes two fmaf there
    # (``aw[kb + j] = fmaf(.., fmaf(.., aw[kb + j]))``): 2 * PPT = 8 per thread; ``msl::wave_sum(aw[k])`` is a FLOAT sum over 64
    # lanes (6 levels); the four waves meet as doubles
    "onepass": 2 * 4 + 6,
    # dw_bww_bf16_kernel (bf16.hip): one fmaf per output plane d < DW_TD = 2, ``msl::wave_sum(s[k])`` in float (6), then doubles
    "tiled_bf16": 2 + 6,
}

# fp32 additions a term of the BatchNorm sums passes in one thread (and wave) before the value becomes a double
SUMS_DEPTH = {
    # dw_bwd_data_s2_patch_kernel<true>: ``s1 += gm`` over the 2 x 2 x 4 voxels of the thread's patch, then
    # ``msl::block_sum((double)s1, ..)``
    "patch": 16,
    # dw_s2_bwd_reduce_bww_kernel<4>: 16 voxels x PPT = 4 patches, then ``msl::wave_sum(s1)`` in float (6 levels)
    "onepass": 16 * 4 + 6,
}
PATCHES_PER_BLOCK = {"patch": 256, "onepass": 256 * 4}  # s2_patch_blocks / s2_fused_blocks


def gamma(n):
    return n * U / (1.0 - n * U)


def out_dims(dims, stride):
    return tuple((d - 1) // stride + 1 for d in dims)


def bww_depth(path, dims, stride):
    """BWW_DEPTH of a path whose chain depends on the shape: an upper bound from the route's own arithmetic (lds_plan)."""
    if BWW_DEPTH.get(path) is not None:
        return BWW_DEPTH[path]
    OD, OH, OW = out_dims(dims, stride)
    Lp = OH * (OW // 4)  # items (4 outputs along W) per output plane
    if path == "resident":  # G L <= max(256, SLAB Lp) items per workgroup, SLAB <= OD
        return 4 + max(1, -(-OD * Lp // 256))
    if path == "stream":  # IPT = 1 or 4 items per thread (lds_plan), each meets every output plane of the slab (<= OD) once per tap
        ipt = 1 if (Lp <= 256 and dims[1] * (dims[2] // 4) <= 4 * 256) else 4
        return 4 + ipt * OD
    raise KeyError(path)


# ------------------------------------------------------------------------------------------------- the two convolutions
def _axis(I, O, s, k):
    """Outputs o in [0, O) whose tap k lands on an input index i = s o - 1 + k in [0, I): (slice of o, slice of i) or None."""
    lo = 0
    while lo < O and s * lo - 1 + k < 0:
        lo += 1
    hi = O
    while hi > lo and s * (hi - 1) - 1 + k >= I:
        hi -= 1
    if hi <= lo:
        return None
    i0 = s * lo - 1 + k
    return slice(lo, hi), slice(i0, s * (hi - 1) - 1 + k + 1, s)


def tap_planes(dy, stride, dims):
    """dy (N, C, OD, OH, OW) -> (T, cnt): T (27, N, C, D, H, W) float64 with T[k][i] = dy[(i + 1 - k) / s] where that output
    exists, else 0; cnt (D, H, W): taps that exist at i (a property of the shape, not of the values)."""
    N, C, OD, OH, OW = dy.shape
    D, H, W = dims
    dd = dy.double()
    T = torch.zeros((27, N, C, D, H, W), dtype=torch.float64)
    cnt = torch.zeros((D, H, W), dtype=torch.float64)
    for kd in range(3):
        ad = _axis(D, OD, stride, kd)
        for kh in range(3):
            ah = _axis(H, OH, stride, kh)
            for kw in range(3):
                aw = _axis(W, OW, stride, kw)
                if ad is None or ah is None or aw is None:
                    continue
                T[kd * 9 + kh * 3 + kw][:, :, ad[1], ah[1], aw[1]] = dd[:, :, ad[0], ah[0], aw[0]]
                cnt[ad[1], ah[1], aw[1]] += 1
    return T, cnt


def _wk(w):
    return w.double().reshape(w.shape[0], 27).t().reshape(27, 1, -1, 1, 1, 1)


def bwd_data_ref(dy, w, stride, dims):
    """dy (N, C, OD, OH, OW), w (C, 27) -> (g, absdot, taps): g (N, C, D, H, W) float64, absdot = sum |w| |dy|, taps (D, H, W)."""
    T, cnt = tap_planes(dy, stride, dims)
    wk = _wk(w)
    return (wk * T).sum(0), (wk.abs() * T.abs()).sum(0), cnt


def data_bound(absdot, taps, ref, old=None, bf16=False):
    """gamma(taps [+ 1]) (absdot [+ |old|]); bf16 storage: + BF16_U (|ref| + that).  ``ref`` already holds ``old``."""
    n = taps + (0 if old is None else 1)
    b = gamma(n) * (absdot if old is None else absdot + old.double().abs())
    return b + BF16_U * (ref.abs() + b) if bf16 else b


def bww_ref(dy, a32, stride):
    """dy (N, C, OD, OH, OW), a32 (N, C, D, H, W) -> (dW, absdot), float64 (C, 27)."""
    T, _ = tap_planes(dy, stride, tuple(a32.shape[2:]))
    ad = a32.double().unsqueeze(0)
    f = lambda t: t.sum((1, 3, 4, 5)).t().contiguous()
    return f(ad * T), f(ad.abs() * T.abs())


# ------------------------------------------------------------------------------------------------- partials of the patch kernels
def patch_slot(dims, per_block):
    """(D, H, W) -> workgroup (within an image and channel) that owns the voxel: patch q = (a H2 + b) W4 + cw, slot q / per_block."""
    D, H, W = dims
    H2, W4 = (H + 1) // 2, W // 4
    a = torch.arange(D).view(D, 1, 1) // 2
    b = torch.arange(H).view(1, H, 1) // 2
    cw = torch.arange(W).view(1, 1, W) // 4
    return ((a * H2 + b) * W4 + cw) // per_block


def num_blocks(dims, per_block):
    D, H, W = dims
    return (((D + 1) // 2) * ((H + 1) // 2) * (W // 4) + per_block - 1) // per_block


def slot_sums(t, slot, blocks):
    """t (N, C, D, H, W) float64 -> (C, N * blocks): sums per slot, partial index p = n * blocks + slot."""
    N, C = t.shape[:2]
    out = torch.zeros((N, C, blocks), dtype=torch.float64)
    out.index_add_(2, slot.reshape(-1), t.reshape(N, C, -1))
    return out.permute(1, 0, 2).reshape(C, N * blocks)


def bn_terms(g, y, vec32):
    """-> (gm, gm * xhat), float64: gm = g where fmaf(y, scale, shift) > 0 (the kernel's own fp32 test), xhat = (y - mean) invstd."""
    mask = fma32(y.float(), _bc(vec32[0], y).float(), _bc(vec32[1], y).float()) > 0
    gm = torch.where(mask, g.double(), torch.zeros((), dtype=torch.float64))
    return gm, gm * ((y.double() - _bc(vec32[2], y)) * _bc(vec32[3], y))


def bn_sums_ref(g_stored, y, vec32, path):
    """The partials [2][C][NP] of a fused pass from the gradient AS STORED, and their summation bound -> (ref, bound)."""
    dims = tuple(y.shape[2:])
    per = PATCHES_PER_BLOCK[path]
    slot, blocks = patch_slot(dims, per), num_blocks(dims, per)
    t1, t2 = bn_terms(g_stored, y, vec32)
    k = (SUMS_DEPTH[path] + 4) * U
    ref = torch.stack([slot_sums(t1, slot, blocks), slot_sums(t2, slot, blocks)])
    return ref, k * torch.stack([slot_sums(t1.abs(), slot, blocks), slot_sums(t2.abs(), slot, blocks)])


def bn_sums_propagated(gbound, y, vec32, path):
    """What an error of at most ``gbound`` per element of a gradient that is NOT stored moves the partials by."""
    dims = tuple(y.shape[2:])
    per = PATCHES_PER_BLOCK[path]
    slot, blocks = patch_slot(dims, per), num_blocks(dims, per)
    t1, t2 = bn_terms(gbound, y, vec32)
    return torch.stack([slot_sums(t1, slot, blocks), slot_sums(t2.abs(), slot, blocks)])


def bww_slot_ref(dy, a32, path="onepass"):
    """The weight partials [C * 27][NP] of the one-pass kernel (stride 2) and gamma(BWW_DEPTH) absdot per partial."""
    dims = tuple(a32.shape[2:])
    per = PATCHES_PER_BLOCK[path]
    slot, blocks = patch_slot(dims, per), num_blocks(dims, per)
    T, _ = tap_planes(dy, 2, dims)
    ad = a32.double()
    ref = torch.stack([slot_sums(ad * T[k], slot, blocks) for k in range(27)], 1)        # (C, 27, NP)
    mag = torch.stack([slot_sums(ad.abs() * T[k].abs(), slot, blocks) for k in range(27)], 1)
    C = ref.shape[0]
    return ref.reshape(C * 27, -1), gamma(BWW_DEPTH[path]) * mag.reshape(C * 27, -1)


def bf16_round(t):
    return t.float().to(torch.bfloat16).float()


# ------------------------------------------------------------------------------------------------- what a case must produce
HAS_G = ("bwd_data", "bwd_data_bf16", "patch_bn", "patch_bf16", "onepass_data")
HAS_W_PARTIALS = ("onepass_data", "onepass", "onepass_bf16")


def has_sums(case):
    return case[1] in ("patch_bn",) + HAS_W_PARTIALS or (case[1] == "patch_bf16" and case[8].get("yprev"))


def expected(case, d, got):
    """name -> (reference, bound) for every output of a case of tests/dwbwd_cases.py; ``got`` holds the outputs under test (the
    sums of a stored gradient are those of ``got["g_in"]``).  Names: g_in (N, C, D, H, W), bn_partials (2, C, NP), w_partials
    (C * 27, NP), w_taps_t (27, C), dw_sum (C, 27: the exact sum of the weight partials) and dw (C, 27)."""
    _, entry, bf16, N, C, dims, stride, acc, o = case
    dy, w, y, old, vec = d["dy"], d["w"], d["y"], d["old"], d["vec"]
    exp = {}
    if entry in HAS_G or entry in HAS_W_PARTIALS:
        g, absdot, taps = bwd_data_ref(dy, w, stride, dims)
        if old is not None:
            g = g + old.double()
        if entry in HAS_G:
            exp["g_in"] = (g, data_bound(absdot, taps, g, old, bool(bf16)))
        if has_sums(case):
            if entry in HAS_G:
                exp["bn_partials"] = bn_sums_ref(got["g_in"].detach().cpu(), y, vec, o["path"])
            else:  # the gradient exists in registers only: its own fp32 error moves the sums
                ref, b = bn_sums_ref(g, y, vec, o["path"])
                exp["bn_partials"] = (ref, b + bn_sums_propagated(data_bound(absdot, taps, g), y, vec, o["path"]))
    if entry in HAS_W_PARTIALS:
        exp["w_partials"] = bww_slot_ref(dy, act32(y, vec[0], vec[1]), o["path"])
        if o.get("taps_t"):
            exp["w_taps_t"] = (w.double().t(), torch.zeros(()))
    if entry in ("bww", "bww_bf16"):
        a32 = act32(y, vec[0], vec[1]) if o.get("affine") else y
        ref, absdot = bww_ref(dy, a32, stride)
        b = gamma(bww_depth(o["path"], dims, stride)) * absdot
        exp["dw_sum"] = (ref, b)
        if o.get("dw"):
            exp["dw"] = (ref, b + U * (ref.abs() + b))
    return exp
