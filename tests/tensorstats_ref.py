"""Reference for the per-tensor histograms and moments of csrc/tensorstats.hip / mslesions3d_amd/diagnostics.py.

The binning is spelled from the definition - ``math.floor(math.log2(abs(x)))`` clamped to [-42, 20] - value by value, on
purpose NOT through ``diagnostics.bin_of`` (which reads the bit pattern).  The moments are float64: ``math.fsum`` gives the
correctly rounded sum of the exactly representable terms (an fp32 value, its magnitude, and its square - the product of two
fp32 values is exact in fp64).

Bound for a device sum: any summation order of n float64 terms t_i has error <= (n - 1) * u * sum|t_i| to first order
(u = 2^-53); ``sum_bound`` grants n * 2^-52 * sum|t_i|, what the issue states."""
import math

import numpy as np

N_BINS = 128
FLT_MAX = float(np.finfo(np.float32).max)
TINY = float(np.finfo(np.float32).tiny)  # smallest normal


def ref_bin(x):
    """Bin of one value (a Python float holding an fp32 value)."""
    if x != x or x == math.inf or x == -math.inf:
        return 0
    if x == 0.0:
        return 1
    c = min(max(math.floor(math.log2(abs(x))), -42), 20) + 42
    return (2 if x < 0 else 65) + c


def ref_bins(values):
    v = np.asarray(values, dtype=np.float32).reshape(-1)
    with np.errstate(invalid="ignore"):  # widening a signalling NaN raises the flag; it stays a NaN
        wide = v.astype(np.float64).tolist()
    return np.fromiter(map(ref_bin, wide), dtype=np.int64, count=v.size)


def edge_values():
    """The values at which the binning changes (fp32), both signs where that means something."""
    f = np.float32
    below = np.nextafter(f(2.0 ** -42), f(0))
    pos = [f(2.0 ** -43), f(2.0 ** -42), below, f(1), np.nextafter(f(2), f(0)), f(2.0 ** 20), f(2.0 ** 21), f(FLT_MAX),
           f(TINY), f(1e-40), f(0), f(np.inf)]
    out = []
    for v in pos:
        out += [v, -v]
    out.append(f(np.nan))
    return np.array(out, dtype=np.float32)


def random_bits(rng, n):
    """n fp32 values drawn uniformly over all 2^32 bit patterns (every exponent, subnormals, a few Inf / NaN)."""
    return rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32).view(np.float32)


def ref_stats(values):
    """{"hist" int64[128], "n_finite", "sum", "sum_sq", "sum_abs", "min", "max"} of an fp32 array."""
    v = np.asarray(values, dtype=np.float32).reshape(-1)
    hist = np.bincount(ref_bins(v), minlength=N_BINS).astype(np.int64)
    d = v[np.isfinite(v)].astype(np.float64)
    return {"hist": hist, "n_finite": int(d.size), "sum": math.fsum(d.tolist()), "sum_sq": math.fsum((d * d).tolist()),
            "sum_abs": math.fsum(np.abs(d).tolist()), "min": float(d.min()) if d.size else math.inf,
            "max": float(d.max()) if d.size else -math.inf}


def sum_bound(n, sum_abs_terms):
    return n * 2.0 ** -52 * sum_abs_terms
