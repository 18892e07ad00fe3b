"""Float64 reference of the stem-convolution kernels of csrc/stem.hip, with derived error bounds.  Plain torch on the CPU;
like tests/bn_ref.py and tests/pw_ref.py (whose helpers it reuses) nothing here imports the package.

All kernels contract on v_mfma_f32_32x32x2_f32, a k-ordered fmaf chain, so every bound is
(number of fp32 roundings the code can apply to a term) * U * sum |term|   with U = 2**-24.  The counts, read off the code:

forward (stem_fwd_mfma_kernel, stem_fwd_rows_kernel): one chain over KS = ceil(27 Cin / 2) MFMAs of two k each
    -> ``k_pad(Cin) = 2 KS`` fmaf roundings (the padding k of an odd 27 Cin multiplies zeros; it is counted all the same) and
    nothing afterwards (J = 0): the accumulator is stored as it is.
statistics: a lane adds one value per 32-column tile over the 2 * iters tiles of its wave (for the squares these are
    fmas, which round the square with the sum), the 32 lanes of a row meet in the 5-level tree of msl::half32_sum, and one
    spare for the square -> ``stats_depth(iters) = 2 iters + 5 + 1``.  The four waves then meet in double.
weight gradient: a wave contracts ``iters`` chunks (tile-staged kernel: one row of each of its ``iters`` tiles) of 64
    positions in ONE accumulator chain -> L = 64 iters; the four waves of a workgroup meet in 3 fp32 additions in LDS; the ns
    slabs are folded in fp32 by msl::reduce_slabs_256 (a thread adds every 8th slab, then the 8 group sums are added
    serially: ns values meet in at most ns - 1 roundings whatever the tree) -> ``(L + 3 + ns) U sum |a| |x|``.
operand of MODE 1 (BatchNorm backward applied on load): ``sc * (gm - c1 - ((y - mean) * invstd) * c2)``, six operations
    (-, *, *, -, -, *) -> 6 roundings + 2 (the margin tests/bn_ref.py takes: contraction only removes roundings)
    = 8 U |sc| (|gm| + |c1| + |xhat c2|).
operand of MODE 2 (gradient rebuilt from dL/dz of the stride-2 depthwise layer): per axis an odd voxel takes two taps, an
    even one a single tap -> at most 8 fmaf terms; then ``fmaf(sc, gm, fmaf(cC, y, cE))``: 2 more
    -> (8 + 2) U (|sc| sum |w1 dz| [mask] + |cC y| + |cE|).
An operand bound b_a enters the weight gradient as ``sum b_a |x|``; the chain bound then takes |a| + b_a for |a|.

The ReLU mask of MODE 1 / 2 is ``fmaf(y, scale, shift) > 0`` with fp32 vectors handed in by the caller: ``mask32`` reproduces
it bit for bit (pw_ref.fma32), so the reference mask IS the kernel's and no element is ever excluded.
"""
import torch
import torch.nn.functional as F

from tests.bn_ref import U, _bc, exact_sum, f32, worst  # noqa: F401  (re-exported for the tests)
from tests.pw_ref import fma32, stats_total_ref  # noqa: F401

COUT = 32
FWD_BLOCKS_PER_IMAGE = 256  # STEM_FWD_BLOCKS_PER_IMAGE
BW_BLOCKS = 512             # STEM_BW_BLOCKS


def cdiv(a, b):
    return (a + b - 1) // b


def out_dims(dims, stride):
    return tuple((d - 1) // s + 1 for d, s in zip(dims, stride))


def half_dims(odims):
    """dims of dL/dz of the stride-2 depthwise layer behind the stem."""
    return tuple((o - 1) // 2 + 1 for o in odims)


# ------------------------------------------------------------------------------------------------- dispatch, restated
def fwd_plan(cin, dims, stride):
    """stem_fwd_impl restated -> dict(kernel 'rows' | 'mfma', nb workgroups per image, iters chunks per wave, ...)."""
    (D, H, W), (sd, sh, sw) = dims, stride
    OD, OH, OW = out_dims(dims, stride)
    cpr = cdiv(OW, 64)
    cpn = OD * OH * cpr
    nb = min(FWD_BLOCKS_PER_IMAGE, cdiv(cpn, 4))
    rows = sw == 2 and W % 4 == 0 and OW % 32 == 0 and cin <= 2
    return dict(kernel="rows" if rows else "mfma", nb=nb, iters=cdiv(cpn, nb * 4), chunks_per_row=cpr, chunks_per_n=cpn,
                remap=nb % 8 == 0, rows_by_shape=sw == 2 and W % 4 == 0 and OW % 32 == 0)


def bww_plan(N, cin, dims, stride, fused):
    """stem_bww_impl restated -> dict(kernel 'tile' | 'wave', ns workgroups = slabs, iters per wave (tile: per workgroup))."""
    (D, H, W), (sd, sh, sw) = dims, stride
    OD, OH, OW = out_dims(dims, stride)
    cpr = cdiv(OW, 64)
    total = N * OD * OH * cpr
    ns = min(BW_BLOCKS, cdiv(total, 4))
    by_shape = stride == (2, 2, 2) and W == 128 and H % 16 == 0
    if fused and by_shape and cin <= 2:
        tiles = N * OD * (OH // 4)
        nb = min(BW_BLOCKS, tiles)
        return dict(kernel="tile", ns=nb, iters=cdiv(tiles, nb), total=tiles, remap=nb % 8 == 0, tile_by_shape=True)
    return dict(kernel="wave", ns=ns, iters=cdiv(total, ns * 4), total=total, chunks_per_row=cpr,
                remap=fused and ns % 8 == 0, tile_by_shape=by_shape)


def xcd_block(b, nb, remap):
    """lblock of the kernels: with a grid that is a multiple of 8, workgroup b takes the chunk range (b & 7) * (nb / 8) + (b >> 3)."""
    return (b & 7) * (nb >> 3) + (b >> 3) if remap else b


# ------------------------------------------------------------------------------------------------- im2col
def im2col(x, stride):
    """x (N, Cin, D, H, W) -> (N, 27 Cin, OD OH OW), k = ci * 27 + kd * 9 + kh * 3 + kw, pad 1 (dtype kept)."""
    N, Cin, D, H, W = x.shape
    OD, OH, OW = out_dims((D, H, W), stride)
    sd, sh, sw = stride
    xp = F.pad(x, (1, 1, 1, 1, 1, 1))
    cols = [xp[:, :, kd:kd + sd * (OD - 1) + 1:sd, kh:kh + sh * (OH - 1) + 1:sh, kw:kw + sw * (OW - 1) + 1:sw]
            for kd in range(3) for kh in range(3) for kw in range(3)]
    return torch.stack(cols, 2).reshape(N, Cin * 27, OD * OH * OW)


# ------------------------------------------------------------------------------------------------- forward
def k_pad(cin):
    return 2 * cdiv(27 * cin, 2)


def fwd_ref(x, w, stride):
    """-> (y, absdot) float64 (N, 32, OD, OH, OW): conv3d(x, w) and conv3d(|x|, |w|), pad 1."""
    xd, wd = x.double(), w.double()
    return F.conv3d(xd, wd, stride=stride, padding=1), F.conv3d(xd.abs(), wd.abs(), stride=stride, padding=1)


def fwd_bound(absdot, cin):
    """(K_pad + 0) U absdot: the chain's roundings, no addition after it."""
    return (k_pad(cin) + 0) * U * absdot


def stats_depth(iters):
    return 2 * iters + 5 + 1


def stats_own_ref(y_gpu, iters):
    """fp32 (N, 32, ...) as the kernel wrote it (a bf16 output: the fp32 entry point's) -> (ref, bound) float64 (2, 32):
    per-channel sum and sum of squares, and stats_depth(iters) U sum |term|."""
    yd = y_gpu.double().flatten(2)
    s, q = yd.sum((0, 2)), (yd * yd).sum((0, 2))
    return torch.stack([s, q]), stats_depth(iters) * U * torch.stack([yd.abs().sum((0, 2)), q])


def fold_partials(part, NP):
    """fp64 partials [2][32][NP] -> (2, 32) with no rounding but the last."""
    return exact_sum(part.double().view(2, COUT, NP))


# ------------------------------------------------------------------------------------------------- weight gradient
def bww_ref(a, cols):
    """a (N, 32, OS) float64, cols (N, K, OS) -> (dW, absdot) float64 (32, K)."""
    f = lambda p, q: torch.matmul(p, q.transpose(1, 2)).sum(0)
    cd = cols.double()
    return f(a.double(), cd), f(a.double().abs(), cd.abs())


def bww_chain(plan):
    """L + 3 + ns (module docstring)."""
    return 64 * plan["iters"] + 3 + plan["ns"]


def bww_bound(a, a_bound, cols, plan):
    """(L + 3 + ns) U sum (|a| + b_a) |x| + sum b_a |x|; ``a_bound`` None: the operand is exact (MODE 0)."""
    ca = cols.double().abs()
    f = lambda p: torch.matmul(p, ca.transpose(1, 2)).sum(0)
    if a_bound is None:
        return bww_chain(plan) * U * f(a.double().abs())
    return bww_chain(plan) * U * f(a.double().abs() + a_bound) + f(a_bound)


def mask32(y, sc32, sf32):
    """The kernels' ReLU mask, bit for bit: fmaf(y, scale, shift) > 0."""
    return fma32(y.float(), _bc(sc32, y).float(), _bc(sf32, y).float()) > 0


def mode1_operand(g, y, vec6):
    """g, y fp32 (N, 32, ...), vec6 (6, 32) fp32 [scale, shift, mean, invstd, c1, c2] -> (a, bound) float64:
    a = sc (gm - c1 - ((y - mean) invstd) c2), gm = g under the kernel's mask; 8 U |sc| (|gm| + |c1| + |xhat c2|)."""
    sc, mu, is_, c1, c2 = (_bc(vec6[k], y) for k in (0, 2, 3, 4, 5))
    gm = torch.where(mask32(y, vec6[0], vec6[1]), g.double(), torch.zeros((), dtype=torch.float64))
    t = ((y.double() - mu) * is_) * c2
    return sc * (gm - c1 - t), 8 * U * sc.abs() * (gm.abs() + c1.abs() + t.abs())


def dwconv_t(dz, w1, odims):
    """g = dwconv_s2^T(dz): dz (N, 32, OD1, OH1, OW1), w1 (32, 1, 3, 3, 3) -> (N, 32, OD, OH, OW); the output padding is what
    makes the stem's output size: odims - (2 * dz dims - 1), 0 for an odd and 1 for an even size."""
    op = tuple(o - (2 * z - 1) for o, z in zip(odims, dz.shape[2:]))
    assert all(p in (0, 1) for p in op), op
    return F.conv_transpose3d(dz, w1, stride=2, padding=1, output_padding=op, groups=COUT)


def mode2_operand(dz, w1, y, vec8):
    """dz, y fp32, w1 (32, 1, 3, 3, 3) fp32, vec8 (8, 32) fp32 [scale, shift, mean, invstd, c1, c2, cC, cE]
    -> (a, bound, g, gabs) float64: a = sc gm + (cC y + cE), gm = dwconv^T(dz) under the kernel's mask."""
    odims = tuple(y.shape[2:])
    g = dwconv_t(dz.double(), w1.double(), odims)
    gabs = dwconv_t(dz.double().abs(), w1.double().abs(), odims)
    m = mask32(y, vec8[0], vec8[1])
    zero = torch.zeros((), dtype=torch.float64)
    sc, cC, cE = (_bc(vec8[k], y) for k in (0, 6, 7))
    gm, gma = torch.where(m, g, zero), torch.where(m, gabs, zero)
    yd = y.double()
    return sc * gm + (cC * yd + cE), (8 + 2) * U * (sc.abs() * gma + (cC * yd).abs() + cE.abs()), g, gabs


# ------------------------------------------------------------------------------------------------- the caller's vectors
def host_vec(g, y, gamma, beta, rows, eps=1e-5):
    """The (rows, 32) fp32 block a caller hands to the kernels, made on the host in float64 and rounded once: rows 0-3
    [scale, shift, mean, invstd] of y's batch statistics, rows 4-5 c1 = dbeta / n, c2 = dgamma / n of the masked gradient g
    (float64 (N, 32, ...)), and with rows == 8 the folded coefficients of msl_bn_bwd_finalize_coef:
    cC = -scale invstd c2,  cE = scale invstd c2 mean - scale c1."""
    from tests import bn_ref as R
    v4 = R.host_vectors(y, gamma, beta, eps)
    n = y.numel() // y.shape[1]
    dbeta, dgamma = R.bwd_sums_ref(g, y, v4)
    out = [v4, f32(dbeta / n).view(1, -1), f32(dgamma / n).view(1, -1)]
    if rows == 8:
        cC, cE = R.coef_ref(dbeta, dgamma, n, v4)
        out += [f32(cC).view(1, -1), f32(cE).view(1, -1)]
    return torch.cat(out).contiguous()
