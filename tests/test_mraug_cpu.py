"""The host side of the MR stage: datasets.philox4x32 / philox_normal, gaussian_taps / blur_axis,
bias_lattice / bias_field, the draws of gaussiansmooth / biasfield / gaussiannoise, select_training_augmentations and the
lowering in devicedata.sample_params / mr_tables.  CPU only."""
import numpy as np
import pytest

from mslesions3d_amd import datasets as DS
from mslesions3d_amd import devicedata as DD


class Recorder:
    """Counts the calls a draw makes on the generator it is handed."""

    def __init__(self, seed=0):
        self.rs, self.calls = np.random.RandomState(seed), []

    def __getattr__(self, name):
        def call(*a, **kw):
            self.calls.append(name)
            return getattr(self.rs, name)(*a, **kw)
        return call


# ---- Philox and the normal -------------------------------------------------------------------------------------------------
KNOWN = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
          "d16cfe09 94fdcceb 5001e420 24126ea1")]


@pytest.mark.parametrize("counter,key,want", KNOWN)
def test_philox_known_answers(counter, key, want):
    assert " ".join(f"{int(w):08x}" for w in DS.philox4x32(counter, key)) == want


def test_philox_broadcasts_over_counters():
    c0 = np.array([0, 0x243F6A88, 0xFFFFFFFF], dtype=np.uint64)
    got = DS.philox4x32((c0, 0, 0, 0), (0, 0))
    assert int(got[0][0]) == 0x6627E8D5 and got[0].shape == (3,)
    for i, c in enumerate(c0):
        assert [int(w[i]) for w in got] == [int(w) for w in DS.philox4x32((int(c), 0, 0, 0), (0, 0))]


def test_eight_half_normal_moments():
    """Over 2^20 consecutive counters: |mean| <= 5 / 1024 and |variance - 1| <= 0.007, five standard errors each (the
    excess kurtosis of the eight-term Irwin-Hall sum is -0.15); the tails end at (524280 - 262140) c = 4.9."""
    z = DS.philox_normal(np.arange(2 ** 20, dtype=np.uint64), 1, 0xA4093822, 0x299F31D0)
    assert z.dtype == np.float32
    z = z.astype(np.float64)
    print("mean", z.mean(), "variance", z.var())
    assert abs(z.mean()) <= 5 / 1024
    assert abs(z.var() - 1.0) <= 0.007
    assert np.abs(z).max() <= 262140 * float(DS.NOISE_SCALE) < 4.9
    assert DS.NOISE_SCALE == np.float32(1.0 / np.sqrt(8 * (2 ** 32 - 1) / 12)) and DS.NOISE_SCALE.dtype == np.float32


def test_noise_is_three_f32_operations_per_channel():
    img = np.random.RandomState(0).randn(2, 3, 4, 5).astype(np.float32)
    out = DS.gaussian_noise(img, 0.3, 17, 18)
    idx = np.arange(60, dtype=np.uint64).reshape(3, 4, 5)
    for c in range(2):
        n = DS.philox_normal(idx, c, 17, 18) * np.float32(0.3)
        assert n.dtype == np.float32 and np.array_equal(out[c], img[c] + n)
    assert not np.array_equal(out[0] - img[0], out[1] - img[1])
    assert np.array_equal(DS.gaussian_noise(img, 0.0, 17, 18), img)  # (no -0.0 in img)


# ---- taps and blur -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0.25, 0.4, 1.0, 1.5, 1.99, 2.0])
def test_taps_sum_to_one_and_are_symmetric(sigma):
    w = DS.gaussian_taps(sigma)
    R = (w.size - 1) // 2
    assert w.dtype == np.float32 and w.size == 2 * R + 1 == 2 * int(4 * sigma + 0.5) + 1
    assert abs(float(w.astype(np.float64).sum()) - 1.0) <= 2.0 ** -23 * (2 * R + 1)
    assert np.array_equal(w, w[::-1]) and w[R] == w.max()


def test_radius_limits():
    assert DS.gaussian_radius(0.25) == 1 and DS.gaussian_radius(2.0) == 8 == DS.MR_MAX_RADIUS
    for bad in (2.01, 0.0, -1.0):
        with pytest.raises(ValueError, match="sigma"):
            DS.gaussian_taps(bad)
    with pytest.raises(ValueError, match="sigma"):
        DS.gaussian_smooth(np.zeros((1, 4, 4, 4), np.float32), (1.0, 2.01, 1.0))


def _ulp(x):
    return np.spacing(np.abs(x).astype(np.float32))


def test_blur_against_scipy_within_one_ulp():
    """scipy.ndimage.correlate1d(mode="constant") per axis, rounded to f32 between the axes; its summation order is its
    own, so the two may differ by the rounding of a different f64 sum: one f32 ulp of the result."""
    from scipy.ndimage import correlate1d
    rs = np.random.RandomState(0)
    img = rs.randn(2, 9, 20, 33).astype(np.float32)  # D shorter than 2R + 1 at R = 8
    sigmas = (2.0, 0.25, 1.3)
    got = DS.gaussian_smooth(img, sigmas)
    assert got.dtype == np.float32 and got.shape == img.shape
    want = img
    for a, s in enumerate(sigmas):
        w = DS.gaussian_taps(s).astype(np.float64)
        want = correlate1d(want.astype(np.float64), w, axis=a + 1, mode="constant", cval=0.0).astype(np.float32)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print("largest difference in ulps", float((err / _ulp(want)).max()))
    assert (err <= _ulp(want)).all()


def test_blur_pass_is_the_contract_sum():
    rs = np.random.RandomState(1)
    v = rs.randn(7).astype(np.float32)
    w = DS.gaussian_taps(2.0)  # R = 8 on an axis of 7: both halos overlap
    got = DS.blur_axis(v, w, 0)
    for i in range(7):
        acc = 0.0
        for k in range(-8, 9):
            if 0 <= i + k < 7:
                acc += float(w[k + 8]) * float(v[i + k])
        assert got[i] == np.float32(acc)


# ---- bias field --------------------------------------------------------------------------------------------------------------
def _poly_scalar(coeffs, degree, u):
    """The contract's polynomial at one point, written out in Python floats."""
    def legendre(x):
        P = [1.0, x]
        for m in range(1, degree):
            P.append(((2 * m + 1) * x * P[m] - m * P[m - 1]) / (m + 1))
        return P
    P0, P1, P2 = (legendre(float(x)) for x in u)
    s = 0.0
    for c, (i, j, k) in zip(coeffs, DS.bias_terms(degree)):
        s = s + ((float(c) * P0[i]) * P1[j]) * P2[k]
    return s


def test_bias_terms_order():
    terms = DS.bias_terms(3)
    assert len(terms) == 20 and terms == sorted(terms) and terms[0] == (0, 0, 0) and terms[-1] == (3, 0, 0)
    assert all(sum(t) <= 3 for t in terms) and len(set(terms)) == 20


def test_bias_field_is_exact_on_the_lattice_and_within_the_interpolation_error_elsewhere():
    """At a voxel that sits on a lattice point the field is f32(exp(polynomial)) bit for bit (weights 1 and 0).  Elsewhere
    trilinear interpolation of g = exp(p) on cells of h = 2 / (L - 1) errs by at most sum_a h^2 / 8 max |d^2 g / du_a^2|,
    and d^2 g / du^2 = g (p'' + p'^2).  On [-1, 1]: |P_m| <= 1, |P_m'| <= m (m + 1) / 2, |P_m''| <= (m - 1) m (m + 1)
    (m + 2) / 8, so with A = sum |c|, B_a = sum |c| max|P'_{i_a}| and C_a = sum |c| max|P''_{i_a}| the bound is
    exp(A) sum_a (C_a + B_a^2) h^2 / 8; at coeff_range 0.1 and degree 3 that is at most e^2 * 3 * (2.4 + 2.1^2) / 128 = 1.18.
    The f32 roundings of the lattice and of the field add two relative 2^-24."""
    coeffs = np.random.RandomState(3).uniform(0.0, 0.1, 20)
    L, degree = 9, 3
    F = DS.bias_lattice(coeffs, degree, L)
    u = -1.0 + 2.0 * np.arange(L) / (L - 1)
    assert F.dtype == np.float32 and F.shape == (L, L, L)
    for j in ((0, 0, 0), (8, 8, 8), (1, 5, 7), (4, 4, 4), (8, 0, 3)):
        assert F[j] == np.float32(np.exp(_poly_scalar(coeffs, degree, [u[a] for a in j])))
    from numpy.polynomial import legendre as NL
    c3 = np.zeros((4, 4, 4))
    for c, t in zip(coeffs, DS.bias_terms(degree)):
        c3[t] = c
    ref = np.exp(NL.leggrid3d(u, u, u, c3))  # an independent evaluation: equal up to the f64 rounding of the sums
    np.testing.assert_allclose(F, ref, rtol=2.0 ** -23, atol=0)
    # voxels on lattice points: n - 1 a multiple of L - 1
    shape = (17, 9, 25)
    field = DS.bias_field(F, shape)
    assert field.dtype == np.float32 and field.shape == shape
    assert np.array_equal(field[::2, ::1, ::3], F)
    # elsewhere: the derived bound
    mP1, mP2 = [0.0, 1.0, 3.0, 6.0], [0.0, 0.0, 3.0, 15.0]
    terms = DS.bias_terms(degree)
    A = float(np.abs(coeffs).sum())
    bound = 0.0
    for a in range(3):
        B = sum(abs(c) * mP1[t[a]] for c, t in zip(coeffs, terms))
        C = sum(abs(c) * mP2[t[a]] for c, t in zip(coeffs, terms))
        bound += (C + B * B) * (2.0 / (L - 1)) ** 2 / 8
    bound *= np.exp(A)
    assert bound <= np.exp(2.0) * 3 * (2.4 + 2.1 ** 2) / 128
    shape = (13, 30, 11)
    field = DS.bias_field(F, shape).astype(np.float64)
    grid = [-1.0 + 2.0 * np.arange(n) / (n - 1) for n in shape]
    exact = np.exp(DS.bias_polynomial(coeffs, degree, *grid))
    err = np.abs(field - exact).max()
    print("interpolation error", err, "bound", bound)
    assert err <= bound + 2.0 ** -22 * exact.max()
    assert np.array_equal(DS.bias_field(F, (1, 1, 5))[0, 0], DS.bias_field(F, (2, 2, 5))[0, 0])  # n = 1 samples at 0


# ---- draws, names, order -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DS.MR_NAMES)
def test_prob_zero_returns_the_inputs_and_consumes_one_draw(name):
    img, seg = np.ones((1, 3, 4, 5), np.float32), np.zeros((1, 3, 4, 5), np.int16)
    r = Recorder()
    assert DS.DRAWS[name](r, prob=0.0) is None and r.calls == ["rand"]
    r = Recorder()
    out = DS.AUGMENTATIONS[name](img, seg, r, prob=0.0)
    assert out[0] is img and out[1] is seg and r.calls == ["rand"]


def test_draws_follow_the_contract():
    r = Recorder(1)
    s = DS._draw_gaussiansmooth(r, sigma=(0.25, 1.5), prob=1.0)
    assert r.calls == ["rand", "uniform", "uniform", "uniform"] and len(s) == 3 and all(0.25 <= v <= 1.5 for v in s)
    r = Recorder(1)
    c = DS._draw_biasfield(r, prob=1.0)
    assert r.calls == ["rand", "uniform"] and c.shape == (20,) and c.dtype == np.float64 and (0 <= c).all() and (c <= 0.1).all()
    r = Recorder(1)
    std, k0, k1 = DS._draw_gaussiannoise(r, std=0.1, prob=1.0)
    assert r.calls == ["rand", "uniform", "randint"] and 0 <= std <= 0.1 and 0 <= k0 < 2 ** 32 and 0 <= k1 < 2 ** 32
    rs = np.random.RandomState(1)
    rs.rand()
    assert std == rs.uniform(0, 0.1) and [k0, k1] == rs.randint(0, 2 ** 32, 2, dtype=np.uint32).tolist()
    assert set(DS.DRAWS) == set(DS.AUGMENTATIONS) and set(DS.MR_NAMES) <= set(DS.DRAWS)


def test_the_mask_passes_through_and_channels_share_blur_and_bias():
    rs = np.random.RandomState(0)
    img = np.repeat(rs.randn(1, 6, 7, 8).astype(np.float32), 2, 0)
    seg = rs.randint(0, 3, (1, 6, 7, 8)).astype(np.int16)
    for name in DS.MR_NAMES:
        out, m = DS.AUGMENTATIONS[name](img, seg, np.random.RandomState(4), prob=1.0)
        assert m is seg and out.dtype == np.float32 and out.shape == img.shape and not np.array_equal(out, img)
        assert np.array_equal(out[0], out[1]) == (name != "gaussiannoise")


def test_select_training_augmentations_puts_the_three_last():
    today = ["flip", "rotate90", "translate", "scale", "affine", "zoom", "griddistortion", "shiftintensity", "scaleintensity"]
    for names in (today, today[:3], ["shiftintensity", "zoom"], []):
        warp = [n for n, _ in DS.WARP_AUGMENTATIONS]
        base = DS.select_augmentations([n for n in names if n not in warp])
        at = next((k for k, (n, _) in enumerate(base) if n in DS.INTENSITY_NAMES), len(base))
        want = base[:at] + [t for t in DS.WARP_AUGMENTATIONS if t[0] in names] + base[at:]
        assert DS.select_training_augmentations(names) == want  # the parent commit's rule, restated
        got = DS.select_training_augmentations(["gaussiannoise"] + names + ["gaussiansmooth", "biasfield"])
        assert got[:len(want)] == want and got[len(want):] == DS.MR_AUGMENTATIONS
    assert [n for n, _ in DS.select_training_augmentations(["gaussiannoise", "flip", "gaussiansmooth"])] == \
        ["flip", "gaussiansmooth", "gaussiannoise"]
    assert DS.MR_AUGMENTATIONS == [("gaussiansmooth", {"sigma": (0.25, 1.5), "prob": 0.1}),
                                   ("biasfield", {"degree": 3, "coeff_range": (0.0, 0.1), "lattice": 9, "prob": 0.1}),
                                   ("gaussiannoise", {"std": 0.1, "prob": 0.1})]
    with pytest.raises(ValueError, match="unknown augmentation"):
        DS.select_training_augmentations(["gaussiansmooth", "ricianoise"])
    with pytest.raises(ValueError):  # the mirror of the reference's lists keeps refusing them
        DS.select_augmentations(["biasfield"])


# ---- lowering for the device -------------------------------------------------------------------------------------------------
def test_sample_params_takes_the_three_as_a_last_group():
    augs = [("flip", {"prob": 1.0}), ("shiftintensity", {"prob": 1.0})] + [(n, dict(kw, prob=1.0)) for n, kw in DS.MR_AUGMENTATIONS]
    draws = DS.draw_augmentations(augs, np.random.RandomState(2))
    perm, stages = DD.sample_params(draws, (8, 9, 10), augs, ragged=True)
    assert perm == ([0, 1, 2], [1, 1, 1])  # the flip still reaches the permutation: an MR name is no flip
    assert [type(s).__name__ for s in stages] == ["IntensityOp"] + ["MRStage"] * 3
    assert [s.name for s in stages[1:]] == list(DS.MR_NAMES) and stages[2].kw["lattice"] == 9
    rows, coords = DD.warp_rows([0], [(perm, stages)])  # the batch build does not see them
    assert rows[0, 21] == 1 and rows[0, 7] == DD.ROW_COPY and coords.size == 0
    undrawn = DD.sample_params([(n, None) for n, _ in augs], (8, 9, 10), augs, ragged=True)[1]
    assert [s.draw for s in undrawn[1:]] == [None] * 3
    for bad in (["gaussiansmooth", "flip"], ["gaussiannoise", "shiftintensity"], ["biasfield", "affine"],
                ["gaussiansmooth", "zoom"], ["gaussiannoise", "gaussiansmooth"], ["biasfield", "biasfield"]):
        with pytest.raises(NotImplementedError):
            DD.sample_params([(n, None) for n in bad], (8, 9, 10), None, ragged=True)
    with pytest.raises(NotImplementedError):
        DS.check_mr_last(["gaussiansmooth", "flip"])
    DS.check_mr_last(["flip", "gaussiannoise", "gaussiansmooth"])  # the host applies any order of the three


def test_mr_tables_rows_taps_and_lattice():
    draws = [("gaussiansmooth", (0.25, 2.0, 1.0)), ("biasfield", np.full(20, 0.05)), ("gaussiannoise", (0.07, 5, 0xFFFFFFFF))]
    full = DD.sample_params(draws, (4, 4, 4), [(n, {}) for n, _ in draws], ragged=True)
    none = DD.sample_params([(n, None) for n, _ in draws], (4, 4, 4), None, ragged=True)
    rows, taps, lat = DD.mr_tables([none, full])
    assert rows.shape == (2, DD.MR_STRIDE) and taps.shape == (2, 3, 17) and lat.shape == (2, 9, 9, 9)
    assert rows.dtype == np.float64 and taps.dtype == np.float32 and lat.dtype == np.float32
    assert not rows[0].any() and not taps[0].any() and (lat[0] == 1).all()
    assert rows[1].tolist() == [7.0, 1.0, 8.0, 4.0, float(np.float32(0.07)), 5.0, float(0xFFFFFFFF), 0.0]
    assert np.array_equal(taps[1, 0, :3], DS.gaussian_taps(0.25)) and not taps[1, 0, 3:].any()
    assert np.array_equal(taps[1, 1], DS.gaussian_taps(2.0)) and np.array_equal(lat[1], DS.bias_lattice(np.full(20, 0.05)))
    assert DD.names_mr(["flip", ("biasfield", {})]) and not DD.names_mr(["flip", ("affine", {})])
    with pytest.raises(ValueError, match="sigma"):
        DD.mr_tables([DD.sample_params([("gaussiansmooth", (2.5, 1, 1))], (4, 4, 4), None, ragged=True)])


def test_lesion_cases_apply_the_three_behind_the_fit(tmp_path):
    """The host loader draws the three in list order and applies them to the fitted sample, where the device route applies
    them to the built batch; a run that names none of them draws and computes what it always did."""
    from tests import lesion_tree
    data_dir = lesion_tree.make_tree(tmp_path, [(30, 34, 38), (36, 30, 32)])
    target = (24, 40, 32)  # crops axis 0, pads axis 1
    base = [("flip", {"spatial_axis": (0,), "prob": 1.0}), ("shiftintensity", {"offsets": 0.1, "prob": 1.0})]
    mr = [(n, dict(kw, prob=1.0)) for n, kw in DS.MR_AUGMENTATIONS]

    def module(augs):
        dm = DS.LesionsDataModule(data_dir=data_dir, centers=lesion_tree.CENTERS, batch_size=1, spatial_size=target,
                                  augmentations=augs, subject="100")
        dm.setup("fit")
        return dm.train_dataset

    plain, full = module(base), module(base + mr)
    a, b = plain[0], full[0]
    assert a["img"].shape == b["img"].shape == (1,) + target and np.array_equal(a["boxes"], b["boxes"])
    rs = full.sample_rng(0)
    draws = DS.draw_augmentations(base + mr, rs)
    want = a["img"].numpy()
    for (name, kw), (_, d) in zip(mr, draws[2:]):
        want = DS.apply_mr(name, want, d, kw)
    assert np.array_equal(b["img"].numpy(), want) and not np.array_equal(a["img"].numpy(), want)
    with pytest.raises(NotImplementedError, match="behind an MR transform"):
        module(mr + base)
