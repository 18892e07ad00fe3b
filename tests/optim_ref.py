"""Float64 reference of csrc/optim.hip - Adam over the flat arena, the batched gradient fold, the loss fold - with derived
error bounds.  Plain numpy / torch on the CPU; like tests/bn_ref.py (whose helpers it reuses) nothing here imports the package.

Every bound is (fp32 roundings a term can go through) * U * |term| with U = 2**-24, carried through the expression as a
running error: an intermediate is a pair (exact value, bound on |computed - exact|), and each operation maps the input bounds
through its derivative (rigorously: products keep their second-order term, quotients and roots divide by the smallest
denominator the error allows) and adds U * (|value| + incoming error) for its own rounding.  optim.o is compiled with
-ffp-contract=off and without fast-math, so a * b + c is two roundings, and hipcc's default for HIP is correctly rounded fp32
division and sqrtf (-fhip-fp32-correctly-rounded-divide-sqrt): one U each, like every other operation.

adam_kernel, operation by operation (hp = [step_bias, step_other, sqrt(bc2), beta1, beta2, eps, wd, grad_scale], fp32):

     1  t1 = g * gs                  7  a  = v * b2                 11  s  = sqrtf(vi)
     2  t2 = wd * p                  8  c1 = (1 - b2) * gi          12  q  = s / bc2s
     3  gi = t1 + t2                 9  c2 = c1 * gi                13  dn = q + eps
     4  d  = gi - m                 10  vi = a + c2                 14  r  = mi / dn
     5  e  = d * (1 - b1)                                           15  u  = step * r
     6  mi = m + e                                                  16  p' = p - u
    (1 - b1 and 1 - b2 are formed in fp32 like the kernel does: exact for beta in [0.5, 1], and no operation of the count.)
    exp_avg goes through 6 roundings (1-6), exp_avg_sq through 7 (1-3 and 7-10; gi enters twice), the parameter through all
    16.  A rounding that happens to be exact (gs = 1, wd = 0) is counted all the same: the bound does not depend on which
    constants are trivial.  Where every input of an element is 0 every term is 0: the bound is 0 and demands the exact 0.

gradient fold (grad_reduce_batch_kernel):
    fp32 slabs (kinds 0, 2, 3): whatever the tree - serial over <= 16 slabs, or 8 serial group sums added serially - ns values meet
        in at most ns - 1 roundings, each of a partial sum no larger than sum |x|: (ns - 1) U sum_k |x_k| around the exact sum.
    fp64 partials (kind 1): the kernel adds in double (lanes strided, then 32 lane sums; NP values meet in at most NP - 1
        roundings of 2**-53) and rounds once to fp32: 2**-24 |exact| + (NP - 1) 2**-53 sum |x|.
    loss values (kind 4): double sums (order error (ns - 1) 2**-53 sum |x|), then ``(float)ce / f``, ``(float)l1 / (f * 6.0f)``
        in fp32 - reproduced in numpy float32, so the comparison is bit for bit once the sum is pinned (loss_fold_range).

The storage orders of kinds 2 and 3 are written as index loops over the documented layouts (stem_map, head_map): source index
of every destination element, found by walking the layout with one loop per axis, not by decoding a thread index.
"""
import functools
import math

import numpy as np
import torch

from tests.bn_ref import U, exact_sum, worst  # noqa: F401  (re-exported for the tests)

U64 = 2.0 ** -53


# ------------------------------------------------------------------------------------------------- running-error arithmetic
def _t(x):
    return torch.as_tensor(x, dtype=torch.float64)


def _rounded(val, err, u=1.0):
    """The fp32 rounding of a computed value within ``err`` of ``val``: ``u`` * U of its own magnitude on top."""
    return val, err + u * U * (val.abs() + err)


def _mul(a, b):
    (x, ex), (y, ey) = a, b
    return _rounded(x * y, x.abs() * ey + y.abs() * ex + ex * ey)


def _add(a, b, sign=1.0):
    (x, ex), (y, ey) = a, b
    return _rounded(x + sign * y, ex + ey)


def _div(a, b, u=1.0):
    """|x'/y' - x/y| = |dx y - x dy| / (|y| |y'|) <= (ex + |x/y| ey) / (|y| - ey)."""
    (x, ex), (y, ey) = a, b
    q = x / y
    return _rounded(q, (ex + q.abs() * ey) / (y.abs() - ey), u)


def _sqrt(a, u=1.0):
    """|sqrt(v') - sqrt(v)| = |v' - v| / (sqrt(v') + sqrt(v)) <= ev / (sqrt(v) + sqrt(max(v - ev, 0))); 0 where v = ev = 0."""
    v, ev = a
    s = torch.sqrt(v)
    den = s + torch.sqrt((v - ev).clamp_min(0.0))
    err = torch.where(den > 0, ev / torch.where(den > 0, den, torch.ones_like(den)), torch.sqrt(ev))
    return _rounded(s, err, u)


def make_hp(lr, betas, eps, weight_decay, step, grad_scale=1.0, bias_lr_mult=2.0, dtype=np.float32):
    """The hyper-parameter vector FusedAdam uploads before step number ``step`` (1-based): biases at ``bias_lr_mult`` * lr.
    ``dtype=np.float64`` keeps the host's doubles (for the comparison with torch.optim.Adam in float64)."""
    b1, b2 = betas
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    return np.array([bias_lr_mult * lr / bc1, lr / bc1, math.sqrt(bc2), b1, b2, eps, weight_decay, grad_scale], dtype=dtype)


def adam_step(p, g, m, v, hp, is_bias, ep=None, em=None, ev=None, div_sqrt_u=1.0):
    """One step of adam_kernel evaluated in float64 from the given inputs -> (p', m', v', bound_p, bound_m, bound_v), all float64.
    ``hp``: the 8 values the kernel reads, as they are (fp32-rounded by the caller for a GPU comparison); 1 - beta is formed in
    fp32.  ``ep / em / ev``: bounds on how far the kernel's own p / m / v inputs may be from the ones given (the bounds of the
    previous step, for a multi-step run); the gradient is exact.  ``div_sqrt_u``: roundings charged to the division and sqrtf
    (1: correctly rounded, see the module docstring; never more than 2)."""
    assert 1.0 <= div_sqrt_u <= 2.0
    hp = [float(x) for x in np.asarray(hp).tolist()]
    ss_b, ss_o, bc2s, b1, b2, eps, wd, gs = hp
    omb1 = float(np.float32(1.0) - np.float32(b1))
    omb2 = float(np.float32(1.0) - np.float32(b2))
    p, g, m, v = _t(p), _t(g), _t(m), _t(v)
    z = torch.zeros_like(p)
    P, M, V, G = (p, z if ep is None else _t(ep)), (m, z if em is None else _t(em)), (v, z if ev is None else _t(ev)), (g, z)
    c = lambda s: (_t(s), _t(0.0))  # a kernel constant: exact
    gi = _add(_mul(G, c(gs)), _mul(c(wd), P))                      # 1, 2, 3
    mi = _add(M, _mul(_add(gi, M, -1.0), c(omb1)))                 # 4, 5, 6
    vi = _add(_mul(V, c(b2)), _mul(_mul(c(omb2), gi), gi))         # 7, 8, 9, 10
    dn = _add(_div(_sqrt(vi, div_sqrt_u), c(bc2s), div_sqrt_u), c(eps))  # 11, 12, 13
    step = torch.where(torch.as_tensor(np.asarray(is_bias)).bool(), _t(ss_b), _t(ss_o))
    pn = _add(P, _mul((step, z), _div(mi, dn, div_sqrt_u)), -1.0)  # 14, 15, 16
    return pn[0], mi[0], vi[0], pn[1], mi[1], vi[1]


# ------------------------------------------------------------------------------------------------- layouts of kinds 2 and 3
@functools.lru_cache(maxsize=None)
def stem_map(K, NT):
    """Source index inside a padded stem image [32][32 * NT] of every element of dw [32][K] (K = 27 Cin <= 32 NT)."""
    idx = torch.empty(32 * K, dtype=torch.int64)
    for co in range(32):
        for k in range(K):
            idx[co * K + k] = co * (32 * NT) + k
    return idx


@functools.lru_cache(maxsize=None)
def head_map(C, MT, ncls):
    """Source index inside a head slab [ct][tap][mt][co16][ci16] (C / 16 input tiles, 27 taps, MT tiles of 16 output rows) of
    every element of dloc_w (12, C, 27) and dcl_w (2 ncls, C, 27): output row co = 16 mt + co16 is row co of the location
    head below 12, row co - 12 of the class head up to 12 + 2 ncls, padding beyond."""
    loc = torch.full((12 * C * 27,), -1, dtype=torch.int64)
    cl = torch.full((2 * ncls * C * 27,), -1, dtype=torch.int64)
    s = 0
    for ct in range(C // 16):
        for tap in range(27):
            for mt in range(MT):
                for co16 in range(16):
                    co = 16 * mt + co16
                    for ci16 in range(16):
                        ci = 16 * ct + ci16
                        if co < 12:
                            loc[(co * C + ci) * 27 + tap] = s
                        elif co < 12 + 2 * ncls:
                            cl[((co - 12) * C + ci) * 27 + tap] = s
                        s += 1
    assert s == (C // 16) * 27 * MT * 256
    return loc, cl


# ------------------------------------------------------------------------------------------------- folds
def fold_slabs(src, kind, K=None, NT=None, C=None, MT=None, ncls=None):
    """``src``: [ns][count] fp32 slabs (the columns of a slab that belong to the entry).  -> (list of exact float64 sums over
    the slabs, list of bounds (ns - 1) U sum_k |x_k|), one pair per destination: kind 0 the flat [count]; kind 2 dw [32 K] of
    the padded image; kind 3 dloc_w [12 C 27] and dcl_w [2 ncls C 27]."""
    x = _t(src)
    ns = x.shape[0]
    tot = exact_sum(x.t().contiguous())
    bound = (ns - 1) * U * exact_sum(x.abs().t().contiguous())
    if kind == 0:
        maps = [None]
    elif kind == 2:
        assert x.shape[1] == 1024 * NT
        maps = [stem_map(K, NT)]
    elif kind == 3:
        assert x.shape[1] == (C // 16) * 27 * MT * 256
        maps = list(head_map(C, MT, ncls))
    else:
        raise ValueError(kind)
    return [tot if i is None else tot[i] for i in maps], [bound if i is None else bound[i] for i in maps]


def fold_partials_f64(src):
    """``src``: [count][NP] fp64 partials -> (exact sums, 2**-24 |exact| + (NP - 1) 2**-53 sum |x|)."""
    x = _t(src)
    tot = exact_sum(x)
    return tot, U * tot.abs() + (x.shape[1] - 1) * U64 * exact_sum(x.abs())


def _loss_values(ce, l1, n_pos):
    """The kernel's last lines: ``f = (float)n_pos; (float)ce / f; (float)l1 / (f * 6.0f); f`` in numpy float32."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        f = np.float32(n_pos)
        return np.array([np.float32(ce) / f, np.float32(l1) / (f * np.float32(6.0)), f], dtype=np.float32)


def loss_fold(parts, n_pos):
    """``parts``: [ns][2] fp64 (sum ce, sum l1) per workgroup -> float32 [sum ce / f, sum l1 / (6 f), f] from the exact sums."""
    x = np.asarray(parts, dtype=np.float64).reshape(-1, 2)
    return _loss_values(math.fsum(x[:, 0].tolist()), math.fsum(x[:, 1].tolist()), n_pos)


def loss_fold_range(parts, n_pos):
    """-> (lo, hi): loss_fold of the sums moved down / up by the order error (ns - 1) 2**-53 sum |x| a double sum can carry.
    The cast and the divisions by f >= 0 are monotone, so the kernel's values lie between the two (mostly lo == hi: one bit
    pattern is right)."""
    x = np.asarray(parts, dtype=np.float64).reshape(-1, 2)
    out = []
    for sign in (-1.0, 1.0):
        s = [math.fsum(x[:, j].tolist()) + sign * (x.shape[0] - 1) * U64 * math.fsum(np.abs(x[:, j]).tolist()) for j in (0, 1)]
        out.append(_loss_values(s[0], s[1], n_pos))
    return out[0], out[1]
