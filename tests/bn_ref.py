"""Stage-wise float64 reference of the fp32 BatchNorm(+ReLU) kernels of csrc/bn.hip, with derived error bounds.

Plain torch on the CPU; nothing here imports the package under test.  Every function takes what the kernel of that
stage takes (fp32 tensors / vectors, fp64 partial sums) and evaluates the same expression in float64.

Why the reference can be exact about the ReLU mask.  The kernels receive ``scale``, ``shift``, ``mean`` and ``invstd``
as fp32 INPUT vectors and take the mask as ``fmaf(y, scale, shift) > 0``: one rounding of the exact value.  For fp32
inputs the product ``y * scale`` is exact in float64 (48 significant bits) and the float64 sum with ``shift`` rounds
monotonically, so ``y * scale + shift`` evaluated in float64 has the sign of the exact value (and is zero only if that
is zero); rounding the exact value to fp32 keeps the sign too, as long as a non-zero exact value is not smaller than
fp32 can hold - with |y|, |scale| >= 2**-50 it is a multiple of 2**-146, and the tests' data is far above that (the
one test that feeds tiny values uses scale = 1, shift = 0, where the fma is exact).  Hence: when a test makes the
four vectors on the host (float64 math, rounded to fp32) and hands the SAME vectors to the kernel and to this module,
the reference mask is the kernel's mask.  No element is excluded and no tie margin is needed.  (A chain test whose
vectors come from a kernel must instead keep the pre-activation away from 0: ``separate_preactivation``.)

Bounds (``U = 2**-24``, half an fp32 ulp, relative):
* elementwise: ``k * U * M`` with M the sum of the magnitudes of the expression's terms and k the number of fp32
  roundings in it plus 2 (contraction to fma only removes roundings);
* sums: every thread adds ``n_t`` terms in fp32, everything after is fp64 and rounded once: ``(n_t + 4) * U * sum|term|``
  (n_t additions, three roundings inside a dgamma term, the final cast);
* finalize: fp64 math rounded once -> ``2 * U`` relative; the running statistics are one more fp32 expression.
"""
import torch

U = 2.0 ** -24
EPS_DEFAULT = 1e-5


def f32(x):
    """Round a float64 tensor to fp32 (what the host does before it hands a vector to a kernel)."""
    return torch.as_tensor(x, dtype=torch.float64).to(torch.float32)


def as_c_float(x):
    """A python float as the fp32 value a C ``float`` argument carries, in float64."""
    return float(torch.tensor(x, dtype=torch.float32).double())


def _bc(v, like):
    """Per-channel vector -> broadcastable against (N, C, ...) ``like``, float64."""
    return v.double().view((1, -1) + (1,) * (like.dim() - 2))


def _red_dims(t):
    return (0,) + tuple(range(2, t.dim()))


def exact_sum(p):
    """Sum over the last axis of a float64 tensor with no rounding but the last (math.fsum): the reference of a kernel
    that adds fp64 partials in its own order must not carry an order of its own."""
    import math
    flat = p.double().reshape(-1, p.shape[-1])
    return torch.tensor([math.fsum(r.tolist()) for r in flat], dtype=torch.float64).view(p.shape[:-1])


# ------------------------------------------------------------------------------------------------- forward
def finalize_ref(sum_, sumsq, count, gamma, beta, eps, momentum, running_mean=None, running_var=None):
    """(sum, sum of squares) per channel -> dict(scale, shift, mean, invstd, var, running_mean, running_var), float64.
    Biased variance clamped at 0 for normalisation; the running estimate takes the unbiased one when count > 1."""
    s, q, count = sum_.double(), sumsq.double(), float(count)
    eps, m = as_c_float(eps), as_c_float(momentum)
    mean = s / count
    var = (q / count - mean * mean).clamp_min(0.0)
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma.double() * invstd
    out = dict(scale=scale, shift=beta.double() - mean * scale, mean=mean, invstd=invstd, var=var,
               running_mean=None, running_var=None)
    if running_mean is not None:
        unbiased = var * count / (count - 1.0) if count > 1.0 else var
        out["running_mean"] = (1.0 - m) * running_mean.double() + m * mean
        out["running_var"] = (1.0 - m) * running_var.double() + m * unbiased
        out["_rm_mag"] = ((1.0 - m) * running_mean.double()).abs() + (m * mean).abs()
        out["_rv_mag"] = ((1.0 - m) * running_var.double()).abs() + (m * unbiased).abs()
    return out


def finalize_bound(ref, key):
    """scale / shift / mean / invstd: float64 math rounded once -> 2 U relative.
    running_*: (1 - m) * r + m * x in fp32 with x rounded from fp64: roundings x, 1 - m, two products, the sum = 5 -> 7."""
    if key in ("running_mean", "running_var"):
        return 7 * U * ref["_rm_mag" if key == "running_mean" else "_rv_mag"]
    return 2 * U * ref[key].abs()


def eval_affine_ref(gamma, beta, running_mean, running_var, eps):
    """finalize_ref's eval form: the affine of the running statistics."""
    invstd = 1.0 / torch.sqrt(running_var.double() + as_c_float(eps))
    scale = gamma.double() * invstd
    return scale, beta.double() - running_mean.double() * scale


def eval_affine_bound(gamma, beta, running_mean, running_var, eps):
    """fp32 throughout: var + eps, sqrt, 1 / x, gamma * x = 4 roundings -> 6 U on scale;
    shift = beta - rm * scale: those 4 plus product and difference = 6 -> 8 U on |beta| + |rm * scale|."""
    scale, _ = eval_affine_ref(gamma, beta, running_mean, running_var, eps)
    return 6 * U * scale.abs(), 8 * U * (beta.double().abs() + (running_mean.double() * scale).abs())


def act_ref(y, scale32, shift32):
    """relu(y * scale + shift) per channel; NaN survives (the kernel's ``v < 0 ? 0 : v``)."""
    a = y.double() * _bc(scale32, y) + _bc(shift32, y)
    return torch.where(a < 0, torch.zeros_like(a), a)


def act_bound(y, scale32, shift32):
    """one fma: 1 rounding -> 3 U (|y * scale| + |shift|)."""
    return 3 * U * ((y.double() * _bc(scale32, y)).abs() + _bc(shift32, y).abs())


def conditioning_bound(y, mean, scale, beta):
    """relu(fma(y, scale32, shift32)) with vectors from finalize, against TRUE float64 BatchNorm (gamma * (y - mean) *
    invstd + beta): folding the mean into an fp32 shift costs about U * |mean * scale| absolute.
    U * (3 |y * scale| + 3 |mean * scale| + 2 |beta|): scale's rounding acts on y * scale (1) and the fma rounds a value
    no larger than |y sc| + |mean sc| + |beta| (1 each); shift's rounding acts on |mean sc| + |beta| (1 each); one spare
    on the two products."""
    sc, mu, be = _bc(scale, y), _bc(mean, y), _bc(beta, y)
    return U * (3 * (y.double() * sc).abs() + 3 * (mu * sc).abs() + 2 * be.abs())


# ------------------------------------------------------------------------------------------------- backward
def _masked(g, y, vec32):
    sc, sh, mu, is_ = (_bc(vec32[k], y) for k in range(4))
    yd = y.double()
    gm = torch.where(yd * sc + sh > 0, g.double(), torch.zeros((), dtype=torch.float64))
    return gm, (yd - mu) * is_, sc


def bwd_terms_ref(g, y, vec32):
    """-> (gm, gm * xhat) per element, float64: what the reduce kernels add up (for per-chunk partial sums)."""
    gm, xhat, _ = _masked(g, y, vec32)
    return gm, gm * xhat


def bwd_sums_ref(g, y, vec32):
    """-> (dbeta, dgamma): sum gm, sum gm * xhat with gm = g * [y * scale + shift > 0], xhat = (y - mean) * invstd."""
    gm, xhat, _ = _masked(g, y, vec32)
    d = _red_dims(y)
    return gm.sum(d), (gm * xhat).sum(d)


def bwd_sums_bound(g, y, vec32, n_t):
    """(n_t + 4) U sum|term| for (dbeta, dgamma); n_t = fp32 additions of one thread, read off the kernel's indexing."""
    gm, xhat, _ = _masked(g, y, vec32)
    d = _red_dims(y)
    k = (n_t + 4) * U
    return k * gm.abs().sum(d), k * (gm * xhat).abs().sum(d)


def bwd_apply_ref(g, y, vec32, c1, c2):
    """dL/dy = scale * (gm - c1 - xhat * c2)."""
    gm, xhat, sc = _masked(g, y, vec32)
    return sc * (gm - _bc(c1, y) - xhat * _bc(c2, y))


def bwd_apply_bound(g, y, vec32, c1, c2, dc1=None, dc2=None):
    """six operations (y - mean, * invstd, * c2, gm - c1, - ..., scale * ...) -> 8 U |scale| (|gm| + |c1| + |xhat c2|).
    ``dc1`` / ``dc2``: what the kernel's own c1 / c2 may differ from the ones given here by (a kernel that computes them
    itself: the bound of its sums over count, plus their cast) - propagated as |scale| (dc1 + |xhat| dc2)."""
    gm, xhat, sc = _masked(g, y, vec32)
    b = 8 * U * sc.abs() * (gm.abs() + _bc(c1, y).abs() + (xhat * _bc(c2, y)).abs())
    if dc1 is not None:
        b = b + sc.abs() * (_bc(dc1, y) + xhat.abs() * _bc(dc2, y))
    return b


def chain_extra_bounds(g, y, vec64):
    """A chain whose vectors come from msl_bn_finalize is compared with TRUE float64 BatchNorm (``vec64`` = its float64
    vectors): the kernel's scale, mean and invstd are those rounded once (U relative each).  With the mask unchanged
    (pre-activation kept away from 0) that adds, on top of the stage bounds,
      dgamma: U sum |gm| (2 |xhat| + |mean invstd|)        (invstd's rounding acts on xhat, mean's on mean * invstd, one spare)
      dy:     U |scale| (M + |c2| (|xhat| + |mean invstd|)) per unit of c2, M = |gm| + |c1| + |xhat c2|  (scale's rounding on
              everything, invstd's and mean's on the xhat term).
    -> (extra_dgamma, f) with f(c1, c2) -> extra_dy."""
    gm, xhat, sc = _masked(g, y, vec64)
    mi = (_bc(vec64[2], y) * _bc(vec64[3], y)).abs()
    extra_dgamma = U * (gm.abs() * (2 * xhat.abs() + mi)).sum(_red_dims(y))

    def extra_dy(c1, c2):
        c1b, c2b = _bc(c1, y).abs(), _bc(c2, y).abs()
        return U * sc.abs() * (gm.abs() + c1b + xhat.abs() * c2b + c2b * (xhat.abs() + mi))
    return extra_dgamma, extra_dy


def bwd_finalize_ref(partials, count):
    """fp64 partials [2][C][NP] -> dict(dbeta, dgamma, c1, c2), float64 (exact sums)."""
    s, q = exact_sum(partials[0]), exact_sum(partials[1])
    return dict(dbeta=s, dgamma=q, c1=s / float(count), c2=q / float(count))


def bwd_finalize_bound(ref, key):
    """float64 sum (and quotient) rounded once -> 2 U relative."""
    return 2 * U * ref[key].abs()


def coef_ref(s, q, count, vec32):
    """The (cC, cE) rows of msl_bn_bwd_finalize_coef: dL/dy = scale * gm + (cC * y + cE), from
    scale * (gm - c1 - (y - mean) * invstd * c2):  cC = -scale invstd c2,  cE = scale invstd c2 mean - scale c1."""
    sc, mu, is_ = vec32[0].double(), vec32[2].double(), vec32[3].double()
    c1, c2 = s.double() / float(count), q.double() / float(count)
    t = sc * is_ * c2
    return -t, t * mu - sc * c1


def coef_bound(s, q, count, vec32):
    """cC: c2's cast, scale * invstd, * c2 = 3 roundings -> 5 U |cC|.
    cE = fma(t, mean, -scale * c1): those 3, c1's cast, scale * c1, the fma = 6 -> 8 U (|t mean| + |scale c1|)."""
    sc, mu, is_ = vec32[0].double(), vec32[2].double(), vec32[3].double()
    c1, c2 = s.double() / float(count), q.double() / float(count)
    t = sc * is_ * c2
    return 5 * U * t.abs(), 8 * U * ((t * mu).abs() + (sc * c1).abs())


# ------------------------------------------------------------------------------------------------- inputs
def host_vectors(y, gamma, beta, eps=EPS_DEFAULT):
    """The (4, C) fp32 block [scale, shift, mean, invstd] of y's batch statistics, made on the host in float64."""
    yd = y.double()
    d = _red_dims(y)
    n = yd.numel() // yd.shape[1]
    r = finalize_ref(yd.sum(d), (yd * yd).sum(d), n, gamma, beta, eps, 0.0)
    return torch.stack([f32(r["scale"]), f32(r["shift"]), f32(r["mean"]), f32(r["invstd"])])


def separate_preactivation(y, gamma, beta, eps=EPS_DEFAULT, delta=1e-3, max_pass=10):
    """Move every element of fp32 ``y`` whose float64 pre-activation a = bn(y) has |a| < delta to +-2 delta on its own
    side, recompute the statistics, repeat until none is left.  -> (y, min |a|).  For a chain whose vectors come from a
    kernel: fp32 rounding of scale / shift moves a by ~1e-6 on well-conditioned data, far inside the margin."""
    y = y.clone()
    for _ in range(max_pass):
        yd = y.double()
        d = _red_dims(y)
        n = yd.numel() // yd.shape[1]
        r = finalize_ref(yd.sum(d), (yd * yd).sum(d), n, gamma, beta, eps, 0.0)
        sc, sh = _bc(r["scale"], y), _bc(r["shift"], y)
        a = yd * sc + sh
        near = a.abs() < delta
        if not near.any():
            return y, float(a.abs().min())
        tgt = torch.where(a >= 0, 2 * delta, -2 * delta)
        y = torch.where(near, ((tgt - sh) / sc).float(), y)
    raise AssertionError("separate_preactivation did not converge")


def worst(actual, ref, bound):
    """-> (max error / bound, flat index of it, number of elements over their bound).  A zero bound demands equality; a
    NaN in the reference demands a NaN."""
    a, r, b = actual.detach().cpu().double().reshape(-1), ref.double().reshape(-1), bound.double().expand_as(ref).reshape(-1)
    nan_r = torch.isnan(r)
    err = (a - r).abs()
    ratio = torch.where(b > 0, err / b, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    ratio = torch.where(nan_r, torch.where(torch.isnan(a), torch.zeros_like(err), torch.full_like(err, float("inf"))), ratio)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(err, float("inf")), ratio)
    k = int(ratio.argmax())
    return float(ratio[k]), k, int((ratio > 1).sum())
