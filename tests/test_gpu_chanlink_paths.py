"""Every path of the per-channel backward link (csrc/chanlink.hip) against an fp64 reference on the CPU: the autograd of
relu(bn1(dwconv(relu(bn2(y))))) plus the heads' share of dL/d relu(bn2(y)), evaluated in float64 on exactly the values
the kernel reads.  The shapes are the smallest that reach each path: every wave count link_plan chooses, the stride-2
parity classes (with D == 2 or H == 2 the neighbour plane / row of the odd class is the halo only), masked quads (odd
batches, non-cubic extents), the smallest and the largest stride-1 image, both storage types.

Tolerances are those of tests/test_gpu_kernels.py::test_block_bwd_channel_link_matches_autograd (fp32 kernel) and of
tests/test_gpu_bf16.py::test_block_bwd_channel_link_bf16 (bf16 storage against the fp32 kernel on bf16-rounded operands)."""
import functools

import pytest
import torch
import torch.nn.functional as F

from mslesions3d_amd import _lib
from mslesions3d_amd._lib import ptr

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-5


def st():
    return torch.cuda.current_stream().cuda_stream


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def close(a, b, rtol, atol, what):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    err = (a - b).abs()
    bad = err > atol + rtol * b.abs()
    assert not bad.any(), (f"{what}: {int(bad.sum())}/{bad.numel()} elements off; max abs err {err.max().item():.3e}, "
                           f"max |ref| {b.abs().max().item():.3e}, worst idx {int(err.argmax())}")


def _bn_vec(x, gamma, beta):
    """[scale, shift, mean, invstd] of a train-mode BatchNorm on x (float64)."""
    mean = x.mean(dim=(0, 2, 3, 4))
    inv = 1.0 / torch.sqrt(x.var(dim=(0, 2, 3, 4), unbiased=False) + EPS)
    sc = gamma * inv
    return torch.stack([sc, beta - mean * sc, mean, inv])


@functools.lru_cache(maxsize=None)
def _case(n, c, dims, stride, acc, seed=0):
    """Inputs (float32, as the kernel gets them) and the float64 reference of one case; computed once, never modified."""
    D, H, W = dims
    y = rnd(n, c, D, H, W, seed=seed + 1).double().requires_grad_(True)
    gam2, gam1 = [(torch.rand(c, generator=torch.Generator().manual_seed(seed + 10 + i)) + 0.5).double().requires_grad_(True)
                  for i in range(2)]
    bet2, bet1 = [rnd(c, seed=seed + 20 + i, scale=0.3).double().requires_grad_(True) for i in range(2)]
    w = rnd(c, 1, 3, 3, 3, seed=seed + 3, scale=0.3).double().requires_grad_(True)
    a_prev = torch.relu(F.batch_norm(y, None, None, gam2, bet2, training=True, eps=EPS))
    z = F.conv3d(a_prev, w, stride=stride, padding=1, groups=c)
    # the kernel reads z rounded to float32: the reference continues from exactly that value (gradients pass unchanged)
    z = z + (z.detach().float().double() - z.detach())
    z.retain_grad()
    a = torch.relu(F.batch_norm(z, None, None, gam1, bet1, training=True, eps=EPS))
    G = rnd(*a.shape, seed=seed + 4)
    Hs = rnd(*a_prev.shape, seed=seed + 5) if acc else torch.zeros(a_prev.shape)
    ((a * G.double()).sum() + (a_prev * Hs.double()).sum()).backward()
    inp = dict(G=G, Hs=Hs, z=z.detach().float(), y=y.detach().float(), w=w.detach().float().view(c, 27),
               vz=_bn_vec(z.detach(), gam1.detach(), bet1.detach()).float(),
               vy=_bn_vec(y.detach(), gam2.detach(), bet2.detach()).float())
    ref = dict(gz=z.grad, gy=y.grad, dw=w.grad.view(c, 27), dgam1=gam1.grad, dbet1=bet1.grad, dgam2=gam2.grad, dbet2=bet2.grad)
    return inp, ref


def _run(inp, n, c, dims, stride, acc, with_dw=True, fill=7.0, bf16=False):
    """One launch -> dict of outputs.  Without accumulate the old content of dL/dy (``fill``) must be ignored."""
    D, H, W = dims
    act = (lambda t: t.bfloat16()) if bf16 else (lambda t: t)
    d = {k: v.to(DEV).contiguous() for k, v in inp.items()}
    gz = act(d["G"]).clone()
    gy = act(d["Hs"]).clone() if acc else act(torch.full_like(d["Hs"], fill))
    z, y = act(d["z"]), act(d["y"])
    o = [torch.zeros(c, device=DEV) for _ in range(4)]
    dw = torch.full((c, 27), 5.0, device=DEV) if with_dw else None
    _lib.call("msl_block_bwd_channel_link_bf16" if bf16 else "msl_block_bwd_channel_link", ptr(gz), ptr(z), ptr(d["vz"]),
              ptr(d["w"]), ptr(y), ptr(d["vy"]), ptr(gy), ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(o[3]),
              ptr(dw) if with_dw else None, n, c, D, H, W, stride, acc, st())
    torch.cuda.synchronize()
    return dict(gz=gz, gy=gy, dw=dw, dgam1=o[0], dbet1=o[1], dgam2=o[2], dbet2=o[3])


def _check(got, ref, with_dw=True):
    if with_dw:
        close(got["dw"], ref["dw"], 2e-4, 2e-5 * float(ref["dw"].abs().max()), "depthwise weight gradient")
    close(got["gz"], ref["gz"], 2e-4, 2e-5 * float(ref["gz"].abs().max()), "dL/dz")
    close(got["gy"], ref["gy"], 2e-4, 2e-5 * float(ref["gy"].abs().max()), "dL/dy")
    for k, what in (("dgam1", "dgamma bn1"), ("dbet1", "dbeta bn1"), ("dgam2", "dgamma bn2"), ("dbet2", "dbeta bn2")):
        close(got[k], ref[k], 2e-4, 1e-5 * float(ref[k].abs().max()), what)


def _same(a, b):
    return all((a[k] is None and b[k] is None) or torch.equal(a[k], b[k]) for k in a)


def _link_case(n, c, dims, stride, acc, waves, seed=0):
    L = _lib.load()
    assert L.msl_block_bwd_channel_link_supported(n, *dims, stride) == waves
    inp, ref = _case(n, c, dims, stride, acc, seed)
    got = _run(inp, n, c, dims, stride, acc)
    _check(got, ref)
    # fixed summation order, no atomics: two calls on equal inputs agree bit for bit, with and without the weight gradient
    assert _same(got, _run(inp, n, c, dims, stride, acc, fill=-3.0))
    plain = _run(inp, n, c, dims, stride, acc, with_dw=False)
    _check(plain, ref, with_dw=False)
    assert _same(plain, _run(inp, n, c, dims, stride, acc, with_dw=False, fill=1.0))


# (n, c, dims, stride, accumulate, waves per channel)
STRIDE2_GEOMETRY = [
    (1, 3, (2, 2, 8), 2, 0, 1),      # one wave, 4 quads per lane (the class is q); OD = OH = 1
    (1, 4, (4, 4, 8), 2, 1, 1),      # one wave, all four classes with interior neighbours
    (1, 3, (8, 8, 16), 2, 1, 4),     # four waves x 1 quad: a wave is one class
    (4, 3, (2, 8, 16), 2, 0, 4),     # four waves x 1 quad, D == 2
    (2, 3, (8, 8, 16), 2, 0, 4),     # four waves x 2 quads: classes paired ee + oo / eo + oe
    (2, 3, (16, 16, 16), 2, 1, 8),   # eight waves x 4 quads
    (8, 2, (2, 16, 32), 2, 0, 8),    # eight waves, D == 2
    (2, 2, (16, 16, 32), 2, 0, 16),  # sixteen waves x 4 quads
    (16, 2, (2, 16, 32), 2, 1, 16),  # sixteen waves, D == 2
    (2, 4, (8, 2, 16), 2, 1, 1),     # H == 2
]

MASKED_QUADS = [
    (3, 3, (2, 4, 8), 2, 0, 1),      # 12 of 64 lanes per class
    (5, 3, (4, 4, 8), 2, 1, 4),      # stride 2, 1 quad per thread: 40 of 64 lanes per wave
    (3, 3, (8, 4, 16), 2, 0, 4),     # stride 2, 2 quads per thread, non-cubic
    (5, 2, (8, 8, 16), 2, 1, 8),     # stride 2, 4 quads per thread: 5 of 8 image slots
    (3, 3, (4, 8, 16), 1, 1, 4),     # stride 1, non-cubic
    (5, 3, (4, 8, 8), 1, 0, 4),
    (3, 2, (16, 8, 16), 1, 0, 8),
]


@pytest.mark.parametrize("n,c,dims,stride,acc,waves", STRIDE2_GEOMETRY,
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_stride2_parity_classes_at_every_wave_count(n, c, dims, stride, acc, waves):
    _link_case(n, c, dims, stride, acc, waves)


@pytest.mark.parametrize("n,c,dims,stride,acc,waves", MASKED_QUADS,
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_masked_quads_odd_batches_and_non_cubic_extents(n, c, dims, stride, acc, waves):
    _link_case(n, c, dims, stride, acc, waves)


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("n,dims,waves", [(1, (2, 2, 4), 1), (4, (16, 16, 16), 16)], ids=["smallest", "largest"])
def test_stride1_halo_and_no_stale_lds_between_launches(n, dims, waves, acc):
    """The smallest and the largest stride-1 image (their halo cells are read by every border quad), and two launches in a
    row on one stream with different inputs: nothing of the first launch's LDS image may show in the second.
    (Seeds 100 / 400, not 0: with two channels the bound of a BatchNorm gradient is 1e-5 of the larger one, and at seed 0,
    16^3 x 4, the BatchNorm2 scale gradient of one channel is 0.106 beside -14.1, cancelled out of terms that sum to 6100 in
    magnitude: the fp32 rounding of the elements alone - the kernel's expressions evaluated by torch on the CPU with every sum
    in float64 - is 1.70e-4 there, 105 % of the bound, whatever the kernel; at these seeds it is below 3 % of the bound.)"""
    _link_case(n, 2, dims, 1, acc, waves, seed=100)
    first, second = _case(n, 2, dims, 1, acc, seed=100), _case(n, 2, dims, 1, acc, seed=400)
    for inp, ref in (first, second, first):
        _check(_run(inp, n, 2, dims, 1, acc), ref)


@pytest.mark.parametrize("n,c,dims,stride,acc", [(2, 4, (8, 8, 16), 2, 0), (3, 4, (4, 8, 16), 1, 1)], ids=["stride2", "stride1"])
def test_bf16_entry_point(n, c, dims, stride, acc):
    """msl_block_bwd_channel_link_bf16 against the fp32 link on the same bf16-rounded operands (they differ by the storage
    roundings of dL/dz, the intermediate dL/d relu(bn2(y)) and dL/dy only)."""
    inp, _ = _case(n, c, dims, stride, acc)
    inp = dict(inp, **{k: inp[k].bfloat16().float() for k in ("G", "Hs", "z", "y")})
    ref = _run(inp, n, c, dims, stride, acc)
    got = _run(inp, n, c, dims, stride, acc, bf16=True)
    for k in ("gz", "gy"):
        close(got[k].float(), ref[k], 1.0 / 128, 1e-2 * float(ref[k].abs().max()), k)
    for k in ("dgam1", "dbet1", "dgam2", "dbet2"):
        close(got[k], ref[k], 2e-2, 2e-2 * float(ref[k].abs().max()), k)
    close(got["dw"], ref["dw"], 2e-2, 2e-2 * float(ref["dw"].abs().max()), "depthwise weight gradient")
    assert _same(got, _run(inp, n, c, dims, stride, acc, bf16=True, fill=-3.0))
