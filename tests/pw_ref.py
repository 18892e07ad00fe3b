"""Float64 reference of the fp32 pointwise-convolution kernels of csrc/pwconv.hip and csrc/pwfused.hip, with derived
error bounds.  Plain torch on the CPU; like tests/bn_ref.py (whose helpers it reuses) nothing here imports the package.

The kernels compute per image  Y[M x S] = W[M x K] . A[K x S]  with A = relu(fma(z, scale, shift)) re-created on load
(msl::act, common.hpp) and the contraction done by v_mfma_f32_32x32x2_f32, which is bit-equal to a k-ordered fmaf chain.

Bounds (``U = 2**-24``, half an fp32 ulp, relative).  A chain of n fp32 fused multiply-adds carries at most n roundings,
each relative to a partial sum that is no larger than ``absdot = sum_k |w_k| |a_k|``:
* forward / backward-data: ``(K + J) U absdot``; K = length of the chain, J = fp32 additions that combine K-split partial
  tiles afterwards (0 for the serial-K kernels).  J is written next to every case, not computed from the dispatch.
* weight gradient: ``(L + ns) U absdot``; ns = slabs (msl_pwconv_bwd_weight_nslabs), L = positions one slab contracts.
* statistics of one partial, against the float64 sums of the kernel's OWN fp32 output: ``stats_depth(W) U sum |term|``.

The activation is not bounded but reproduced: ``act32`` returns the very fp32 values the kernels feed the MFMAs, so the GEMM
reference takes the kernel's operands and the ReLU mask is the kernel's.
"""
import torch

from tests.bn_ref import U, _bc, exact_sum, worst  # noqa: F401  (re-exported for the tests)


# ------------------------------------------------------------------------------------------------- activation
def fma32(x, a, b):
    """fp32 fmaf(x, a, b) for fp32 tensors (broadcast), bit-exact: ONE rounding of the exact x * a + b.
    x * a is exact in float64 (48 significant bits).  s = RN64(p + b) and TwoSum's residual e give the exact value s + e;
    rounding s straight to fp32 would round twice, so s is first made "round to odd" (if e != 0 and s's last bit is even,
    step s one float64 ulp towards e): float64 carries 29 bits more than fp32, and rounding to odd followed by
    round-to-nearest at a precision at least two bits shorter equals a single round-to-nearest of the exact value."""
    p = x.double() * a.double()
    b = b.double().expand_as(p)
    s = p + b
    bb = s - p
    e = (p - (s - bb)) + (b - bb)  # TwoSum: s + e == p + b exactly
    inexact = (e != 0) & torch.isfinite(s)
    even = (s.contiguous().view(torch.int64) & 1) == 0
    toward = torch.where(e > 0, torch.full_like(s, float("inf")), torch.full_like(s, float("-inf")))
    s = torch.where(inexact & even, torch.nextafter(s, toward), s)
    return s.to(torch.float32)


def act32(z, scale32, shift32):
    """msl::act: ``v = fmaf(z, s, t); v < 0 ? 0 : v`` per channel of (N, C, S) - NaN and -0.0 survive, as in the kernel."""
    v = fma32(z, _bc(scale32, z).float(), _bc(shift32, z).float())
    return torch.where(v < 0, torch.zeros_like(v), v)


# ------------------------------------------------------------------------------------------------- GEMMs
def fwd_ref(a32, w):
    """a32 (N, K, S), w (M, K) -> (y, absdot), float64 (N, M, S):  y = W . A,  absdot = |W| . |A|."""
    ad, wd = a32.double(), w.double()
    return torch.matmul(wd, ad), torch.matmul(wd.abs(), ad.abs())


def bwd_data_ref(dy, w):
    """dy (N, M, S), w (M, K) -> (g, absdot), float64 (N, K, S):  g = W^T . dY (the chain runs over M)."""
    dd, wt = dy.double(), w.double().t()
    return torch.matmul(wt, dd), torch.matmul(wt.abs(), dd.abs())


def gemm_bound(absdot, K, J=0):
    """(K + J) U absdot: K fmaf roundings of the chain, J fp32 additions of K-split partial tiles."""
    return (K + J) * U * absdot


def bww_ref(dy, a32):
    """dy (N, M, S), a32 (N, K, S) -> (dW, absdot), float64 (M, K):  dW = sum_{n, s} dy a."""
    dd, ad = dy.double(), a32.double()
    f = lambda p, q: torch.matmul(p, q.transpose(1, 2)).sum(0)
    return f(dd, ad), f(dd.abs(), ad.abs())


def bww_slab_len(N, S, ns):
    """L: positions one slab contracts = ceil(total_chunks / ns) chunks of 32 (S % 32 == 0: the wave form) or 64 positions."""
    width = 32 if S % 32 == 0 else 64
    total = N * ((S + width - 1) // width)
    return ((total + ns - 1) // ns) * width


def bww_bound(absdot, N, S, ns):
    """(L + ns) U absdot: L roundings at most inside a slab (the four waves of a workgroup share its positions and meet in
    three more additions, L / 4 + 3 <= L for L >= 4; a one-chunk slab of 32 positions still has L = 32), ns for adding slabs."""
    return (bww_slab_len(N, S, ns) + ns) * U * absdot


# ------------------------------------------------------------------------------------------------- statistics
def partial_width(N, S, NP):
    """Columns one statistics partial covers, from the library's own NP (msl_pwconv_fwd_num_partials): the kernels emit one
    partial per image and block of W columns, W in {32, 64, 128, 256}, so NP / N = ceil(S / W).  Two widths give the same
    count only when that count is 1 (one partial per image: every W means the same)."""
    assert NP % N == 0
    per = NP // N
    for W in (32, 64, 128, 256):
        if (S + W - 1) // W == per:
            return W
    raise AssertionError(f"NP = {NP} is no ceil(S / W) * N for S = {S}, N = {N}")


def stats_depth(W):
    """fp32 roundings a term can pass before the partial becomes a double: a lane adds at most one value per 32-column
    MFMA tile of the partial's W columns (W / 32 <= 8 additions; for the sum of squares these are fmas that also round the
    square), the 32 lanes of a row meet in a 5-level DPP / shuffle tree (5), and one spare for ``a1 * a1`` / ``v * v`` where a
    kernel squares outside an fma (1).  Everything after is float64."""
    return W // 32 + 5 + 1


def stats_ref(y_gpu, W):
    """fp32 (N, M, S) as the kernel wrote it -> (ref, bound) float64 (2, M, NP): sum and sum of squares of every partial's
    own columns (slot p = n * ceil(S / W) + block), and stats_depth(W) U sum |term|."""
    N, M, S = y_gpu.shape
    per = (S + W - 1) // W
    yd = torch.nn.functional.pad(y_gpu.double(), (0, per * W - S)).view(N, M, per, W)
    slot = lambda t: t.sum(-1).permute(1, 0, 2).reshape(M, N * per)
    s, q = slot(yd), slot(yd * yd)
    return torch.stack([s, q]), stats_depth(W) * U * torch.stack([slot(yd.abs()), q])


def stats_total_ref(y64, ybound):
    """Per-channel (sum, sumsq) of the float64 reference output and what the GEMM's own error may move them by:
    sum |dy| <= sum bound,  sum |(y + dy)^2 - y^2| <= sum (2 |y| bound + bound^2)."""
    d = (0, 2)
    return (torch.stack([y64.sum(d), (y64 * y64).sum(d)]),
            torch.stack([ybound.sum(d), (2 * y64.abs() * ybound + ybound * ybound).sum(d)]))
