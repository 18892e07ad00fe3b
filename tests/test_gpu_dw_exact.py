"""Depthwise partial buffers at exactly the size the count queries return.  The engine sizes its statistics and
weight-gradient buffers from msl_dwconv_*_num_partials; a launch that writes more slots than its query counts writes past
them.  Here every buffer is [partials | 64 guard doubles] in ONE allocation: the partial region is zeroed, the guard holds a
sentinel, and after the launch the guard must be untouched bit for bit while the sums over exactly NP slots match torch.  A
wrong count lands in the guard, inside the allocation.

Cases: DW_CASES and the cases of test_dw_bwd (tests/test_gpu_kernels.py) - naive, stream (1 and 4 items per thread), resident,
wave stride 1 and stride 2 (shared and split planes).  Tolerances are those of test_dw_fwd / test_dw_bwd and of
test_dw_fwd_bf16 / test_dw_bwd_bf16."""
import functools

import pytest
import torch
import torch.nn.functional as F

from mslesions3d_amd import _lib
from mslesions3d_amd._lib import ptr
from tests import test_gpu_kernels as TK
from tests.test_gpu_kernels import K, affine_act, close, rnd, st
from tests.test_gpu_kernels import _release_kept  # noqa: F401  (autouse fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF_EPS = 2.0 ** -8  # half a bf16 ulp, relative
GUARD, SENTINEL = 64, -1.2345678e300

_BWD_CASES = next(m for m in TK.test_dw_bwd.pytestmark if m.name == "parametrize").args[1]
CASES = list(dict.fromkeys([c[:4] for c in TK.DW_CASES] + [tuple(c) for c in _BWD_CASES]))
# producer partial counts for the fold forward: the serial fold (<= 64) and the wave-tree fold
CASES = [c + ((6, 70)[i % 2],) for i, c in enumerate(CASES)]


def guarded(n):
    """n zeroed doubles followed by the guard -> (whole buffer, partial region)."""
    buf = torch.zeros(n + GUARD, dtype=torch.float64, device=DEV)
    buf[n:] = SENTINEL
    return buf, buf[:n]


def assert_guard_untouched(buf, n, what):
    tail = buf[n:].cpu().view(torch.int64)
    want = torch.full((GUARD,), SENTINEL, dtype=torch.float64).view(torch.int64)
    assert torch.equal(tail, want), f"{what}: {int((tail != want).sum())} guard doubles behind {n} partials overwritten"


@functools.lru_cache(maxsize=None)
def reference(N, C, dims, stride, bf16):
    """Inputs and the torch results of one case (computed once, never modified): x, w, sc, sh, dy, y, dw."""
    r = (lambda t: t.to(torch.bfloat16).float()) if bf16 else (lambda t: t)
    x = r(rnd(N, C, *dims, seed=4))
    w = rnd(C, 1, 3, 3, 3, seed=5, scale=0.4).requires_grad_(True)
    sc, sh = rnd(C, seed=6).abs() + 0.5, rnd(C, seed=7, scale=0.3)
    y = F.conv3d(affine_act(x, sc, sh), w, stride=stride, padding=1, groups=C)
    dy = r(rnd(*y.shape, seed=8))
    y.backward(dy)
    return x, w.detach(), sc, sh, dy, y.detach(), w.grad.detach()


def check_stats(part, C, NP, ref, rtol, what):
    p = part.view(2, C, NP).sum(-1).cpu()
    close(p[0], ref.double().sum((0, 2, 3, 4)), rtol, 1e-3, what + " sum")
    close(p[1], (ref.double() ** 2).sum((0, 2, 3, 4)), rtol, 1e-3, what + " sumsq")


@pytest.mark.parametrize("N,C,dims,stride,in_np", CASES)
def test_fp32_forward_fills_exactly_its_partials(N, C, dims, stride, in_np):
    L = _lib.load()
    x, w, sc, sh, _, ref, _ = reference(N, C, dims, stride, False)
    NP = L.msl_dwconv_fwd_num_partials(N, C, *dims, stride)
    assert NP > 0
    buf, part = guarded(2 * C * NP)
    y = torch.full(ref.shape, float("nan"), device=DEV)
    _lib.call("msl_dwconv_fwd", ptr(K(x)), ptr(K(sc)), ptr(K(sh)), ptr(K(w)), ptr(y), ptr(buf), N, C, *dims, stride, 0, st())
    assert_guard_untouched(buf, 2 * C * NP, "dw fwd")
    close(y, ref, 1e-5, 1e-5, "dw fwd")
    check_stats(part, C, NP, ref, 1e-5, "dw fwd")


@pytest.mark.parametrize("N,C,dims,stride,in_np", CASES)
def test_fp32_fold_forward_fills_exactly_its_partials(N, C, dims, stride, in_np):
    """The input BatchNorm folded in the kernel from in_np producer partials; the reference uses msl_bn_finalize's vectors."""
    L = _lib.load()
    x, w = reference(N, C, dims, stride, False)[:2]
    gamma, beta = rnd(C, seed=16).abs() + 0.5, rnd(C, seed=17, scale=0.3)
    count = 1000.0
    g = torch.Generator().manual_seed(18)
    ps = torch.randn(C, in_np, generator=g, dtype=torch.float64) * 3.0
    pq = ps.abs() * 2.0 + torch.rand(C, in_np, generator=g, dtype=torch.float64) * 40.0 + 20.0
    part_in = torch.stack([ps, pq]).contiguous().to(DEV)
    vec = torch.zeros(4 * C, device=DEV)  # scale | shift | mean | invstd
    _lib.call("msl_bn_finalize", ptr(part_in), in_np, count, ptr(K(gamma)), ptr(K(beta)), None, None, None, 0.1, 1e-5, ptr(vec),
              ptr(vec[C:]), ptr(vec[2 * C:]), ptr(vec[3 * C:]), C, st())
    ref = F.conv3d(affine_act(x, vec[:C].cpu(), vec[C:2 * C].cpu()), w, stride=stride, padding=1, groups=C)
    NP = L.msl_dwconv_fwd_num_partials(N, C, *dims, stride)
    buf, part = guarded(2 * C * NP)
    y = torch.full(ref.shape, float("nan"), device=DEV)
    _lib.call("msl_dwconv_fwd_fold", ptr(K(x)), ptr(part_in), in_np, count, ptr(K(gamma)), ptr(K(beta)), 1e-5, ptr(K(w)), ptr(y),
              ptr(buf), N, C, *dims, stride, st())
    assert_guard_untouched(buf, 2 * C * NP, "dw fwd fold")
    close(y, ref, 1e-5, 1e-5, "dw fwd fold")
    check_stats(part, C, NP, ref, 1e-5, "dw fwd fold")


@pytest.mark.parametrize("N,C,dims,stride,in_np", CASES)
def test_fp32_weight_gradient_fills_exactly_its_partials(N, C, dims, stride, in_np):
    L = _lib.load()
    x, _, sc, sh, dy, _, dw = reference(N, C, dims, stride, False)
    NP = L.msl_dwconv_bwd_weight_num_partials(N, C, *dims, stride)
    assert NP > 0
    buf, part = guarded(C * 27 * NP)
    _lib.call("msl_dwconv_bwd_weight", ptr(K(dy)), ptr(K(x)), ptr(K(sc)), ptr(K(sh)), None, ptr(buf), N, C, *dims, stride, st())
    assert_guard_untouched(buf, C * 27 * NP, "dw bwd weight")
    close(part.view(C * 27, NP).sum(1).float().view(C, 1, 3, 3, 3), dw, 1e-4, 1e-4, "dw bwd weight (partials, dw == NULL)")


@pytest.mark.parametrize("N,C,dims,stride,in_np", CASES)
def test_bf16_forward_and_weight_gradient_fill_exactly_their_partials(N, C, dims, stride, in_np):
    L = _lib.load()
    x, w, sc, sh, dy, ref, dw = reference(N, C, dims, stride, True)
    b16 = lambda t: K(t.to(torch.bfloat16))  # noqa: E731
    NP = L.msl_dwconv_fwd_bf16_num_partials(N, C, *dims, stride)
    assert NP > 0
    buf, part = guarded(2 * C * NP)
    y = torch.full(ref.shape, float("nan"), dtype=torch.bfloat16, device=DEV)
    _lib.call("msl_dwconv_fwd_bf16", ptr(b16(x)), ptr(K(sc)), ptr(K(sh)), ptr(K(w)), ptr(y), ptr(buf), N, C, *dims, stride, st())
    assert_guard_untouched(buf, 2 * C * NP, "dw fwd bf16")
    close(y.float(), ref, 2 * BF_EPS, 1e-5, "dw fwd bf16")
    check_stats(part, C, NP, ref, 1e-4, "dw fwd bf16")
    buf, part = guarded(C * 27 * NP)
    _lib.call("msl_dwconv_bwd_weight_bf16", ptr(b16(dy)), ptr(b16(x)), ptr(K(sc)), ptr(K(sh)), ptr(buf), N, C, *dims, stride, st())
    assert_guard_untouched(buf, C * 27 * NP, "dw bwd weight bf16")
    close(part.view(C * 27, NP).sum(1).float().view(C, 1, 3, 3, 3), dw, 1e-4, 1e-4, "dw bwd weight bf16")
