"""tests/stemdw_ref.py checked without a GPU.  ``plan`` agrees with msl_stem_dw_fwd_eval_supported (host arithmetic) on every case,
every refused shape and a sweep; the case table reaches exactly the instantiations and SD values a sweep of ``plan`` can reach;
the float64 reference agrees with float64 F.conv3d; an honest fp32 emulation of the kernel, workgroup by workgroup, lies inside
both bounds at every case, no element excluded; on bf16 storage more than half of the second-stage intervals are a single bf16
value; and - the proof that the checks bite - every wrong kernel of stemdw_ref.MUTANTS fails at every case able to express it.

The emulation follows the first CPU_IMAGES images of a case under the plan of the WHOLE case (a workgroup never looks at another
image; N only chooses SD), so the many-image cases that reach SD > 1 are emulated too."""
import functools
import itertools

import pytest
import torch
import torch.nn.functional as F

from mslesions3d_amd import _lib
from tests import stemdw_cases as C
from tests import stemdw_ref as R

CPU_IMAGES = 2
CASE_IDS = C.ids(C.CASES)


def _plan(case):
    _, N, cin, dims = case
    return R.plan(N, cin, dims)


# ------------------------------------------------------------------------------------------------- the planner
def _sweep():
    Ns, cins = (1, 2, 3, 16, 32, 100, 128, 256, 300), (1, 2)
    Ds, Hs, Ws = (4, 8, 12, 16, 24, 32, 48, 64, 128, 192), (8, 12, 16, 24, 32, 48, 96, 128, 192), (32, 64, 128, 192, 256)
    return list(itertools.product(Ns, cins, Ds, Hs, Ws))


def test_plan_is_the_librarys():
    L = _lib.load()
    for _, N, cin, dims in C.CASES:
        assert L.msl_stem_dw_fwd_eval_supported(N, cin, *dims) == 1 and R.plan(N, cin, dims) is not None
    for id_, N, cin, dims, _ in C.REFUSED:
        assert L.msl_stem_dw_fwd_eval_supported(N, cin, *dims) == 0 and R.plan(N, cin, dims) is None, id_
    N, cin, dims = C.LARGEST_TAKEN
    assert L.msl_stem_dw_fwd_eval_supported(N, cin, *dims) == 1 and R.plan(N, cin, dims) is not None
    odd = [(N, cin, (D, H, W)) for N, cin in ((1, 1), (2, 2), (0, 1), (1, 0), (1, 3), (-1, 1))
           for D, H, W in itertools.product((0, 2, 4, 6, 8), (4, 6, 8, 12), (4, 60, 62, 64, 96, 100, 128, 160, 192, 196, 224))]
    shapes = [(N, cin, (D, H, W)) for N, cin, D, H, W in _sweep()] + odd
    assert len(shapes) > 300
    taken = 0
    for N, cin, dims in shapes:
        got = L.msl_stem_dw_fwd_eval_supported(N, cin, *dims)
        assert got == (R.plan(N, cin, dims) is not None), (N, cin, dims)
        taken += got
    assert 0 < taken < len(shapes)


def test_cases_cover_what_the_planner_can_reach():
    """Instantiations and SD values from a sweep of plan(), not typed in; the LDS and slot limits at their tightest."""
    plans = [(cin, R.plan(N, cin, (D, H, W))) for N, cin, D, H, W in _sweep()]
    reach = {(cin, p["th"], p["aw"]) for cin, p in plans if p}
    sds = {p["sd"] for _, p in plans if p}
    assert len(reach) == 16 and (2, 3, 96) not in reach and (2, 4, 96) not in reach
    assert sds == {1, 2, 3, 4, 6, 8}
    sd1 = {(c[2], _plan(c)["th"], _plan(c)["aw"]) for c in C.CASES if _plan(c)["sd"] == 1}
    assert sd1 == reach, reach - sd1
    assert {_plan(c)["sd"] for c in C.CASES} == sds
    for c in C.CASES:
        p = _plan(c)
        assert C.id_parts(c[0]) == (c[2], p["th"], p["aw"], p["sd"]), (c[0], p)
        assert p["lds"] <= R.LDS_MAX and p["slots"] <= R.NLD * R.NT
        assert c[1] * c[2] * c[3][0] * c[3][1] * c[3][2] <= C.MAX_VOXELS
        assert p["grid"] == (c[3][1] // 4 // p["th"], c[3][0] // 4 // p["sd"], c[1])
    assert len(set(CASE_IDS)) == len(CASE_IDS)
    one = [c for c in C.CASES if _plan(c)["sd"] == 1]
    assert all(c[1] <= 3 and c[3][0] in (8, 12) for c in one) and any(c[1] % 2 for c in one)
    for th in (2, 3, 4):  # the recomputed halo row
        assert any(_plan(c)["th"] == th and _plan(c)["grid"][0] >= 2 for c in one), th
    assert {c[3][1] // 4 for c in one if c[2] == 2 and c[3][2] == 192} == {2, 4, 6}
    assert max(_plan(c)["lds"] for c in C.CASES) == 161056
    many = [c for c in C.CASES if _plan(c)["sd"] > 1]
    assert any(_plan(c)["grid"][1] >= 2 for c in many), "no SD > 1 case with two plane segments in an image"
    assert {_plan(c)["th"] for c in many if _plan(c)["grid"][0] >= 2} >= {3, 4} and any(c[2] == 2 for c in many)
    # what the table of the issue says inference runs
    for shape, th, sd in (((1, 1, (192,) * 3), 3, 3), ((2, 1, (192,) * 3), 3, 6), ((2, 1, (128,) * 3), 4, 2), ((1, 2, (192,) * 3), 2, 4)):
        p = R.plan(*shape)
        assert (p["th"], p["sd"]) == (th, sd), (shape, p)


# ------------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("cin,dims", [(1, (8, 12, 16)), (2, (8, 8, 12))])
def test_reference_matches_float64_conv3d(cin, dims):
    d = C.make_data(("x", 2, cin, dims))
    e = R.ref(d["x"], d["w"], d["sc"], d["sh"], d["wd"], False)
    y = F.conv3d(d["x"].double(), d["w"].double(), stride=2, padding=1)
    a = torch.relu(y * d["sc"].double().view(1, -1, 1, 1, 1) + d["sh"].double().view(1, -1, 1, 1, 1))
    z = F.conv3d(a, d["wd"].double().view(32, 1, 3, 3, 3), stride=2, padding=1, groups=32)
    mag = F.conv3d(a.abs(), d["wd"].double().abs().view(32, 1, 3, 3, 3), stride=2, padding=1, groups=32)
    cnt = F.conv3d(torch.ones((1, 1) + R.act_dims(dims), dtype=torch.float64), torch.ones((1, 1, 3, 3, 3), dtype=torch.float64),
                   stride=2, padding=1)[0, 0]
    assert tuple(e["y"].shape[2:]) == R.z_dims(dims)
    assert torch.allclose(e["y"], z, rtol=0, atol=1e-12) and torch.allclose(e["absdot"], mag, rtol=0, atol=1e-12)
    assert torch.equal(e["taps"], cnt) and float(cnt.min()) == 8 and float(cnt.max()) == 27
    assert bool((e["B"] > 0).all())
    # the bf16 bound is the fp32 bound plus the propagated rounding of y; the second stage from the exact y has the same z
    eb = R.ref(d["x"], d["w"], d["sc"], d["sh"], d["wd"], True)
    assert torch.equal(eb["y"], e["y"]) and bool((eb["B"] > e["B"]).all())
    e2 = R.ref_from_y(y.float(), d["sc"], d["sh"], d["wd"])
    assert torch.allclose(e2["y"], z, rtol=0, atol=1e-5) and bool((e2["B"] <= e["B"]).all())


def test_bf16_rounding_of_y_is_half_an_ulp_of_its_binade():
    """|bf16(v) - v| <= bf16_half_ulp(|v|) for every v, with equality at the ties; 2^-9 |v| holds only near the top of a binade:
    1 + 2^-8 moves by 2^-8.  The end-to-end bound with a flat 2^-9 |y64| is left by exact round-to-nearest-even arithmetic."""
    g = C.gen(9)
    v = torch.cat([torch.randn(100000, generator=g) * 3, torch.tensor([1 + 2.0 ** -8, -(2 + 2.0 ** -7), 0.75 + 2.0 ** -9])])
    err = (R.bf16_rne(v).double() - v.double()).abs()
    assert bool((err <= R.bf16_half_ulp(v.double().abs())).all())
    assert float(err[-3]) == 2.0 ** -8 == float(R.bf16_half_ulp(v[-3:].double().abs())[0]) and float(err[-1]) == 2.0 ** -9
    assert bool((err > 2.0 ** -9 * v.double().abs()).any())
    idx = CASE_IDS.index("c1-th4-aw64-sd1:1x8x32x128")
    d, p, s32, s64 = _setup(idx)
    z, _ = R.emulate(d["x"], d["w"], d["sc"], d["sh"], d["wd"], p, True, stem=s32)
    flat = R.ref(d["x"], d["w"], d["sc"], d["sh"], d["wd"], True, stem=s64, flat_bf16=2.0 ** -9)
    row = R.check(CASE_IDS[idx], "end-to-end, 2^-9 |y64|", flat, z, True).rows[0]
    print(row["msg"])
    assert row["bad"] >= 1 and row["ratio"] > 1


# ------------------------------------------------------------------------------------------------- honest fp32 and the wrong kernels
@functools.lru_cache(maxsize=None)
def _setup(idx):
    """Operands of the first CPU_IMAGES images, the whole case's plan, the honest stem chain and the float64 stem."""
    case = C.CASES[idx]
    d = C.make_data(case, n=CPU_IMAGES)
    return d, _plan(case), R.emul_stem(d["x"], d["w"]), R.stem64(d["x"], d["w"])


def _judge(case, d, p, stem32, stem64, bf16, mut=None):
    """-> (failures of the two checks, their ratios, pinned share of the second stage, z) of one emulated run."""
    z, y = R.emulate(d["x"], d["w"], d["sc"], d["sh"], d["wd"], p, bf16, mut, stem=stem32)
    e1 = R.ref(d["x"], d["w"], d["sc"], d["sh"], d["wd"], bf16, stem=stem64)
    e2 = R.ref_from_y(y, d["sc"], d["sh"], d["wd"])
    r1, r2 = R.check(case[0], "end-to-end", e1, z, bf16), R.check(case[0], "from-y", e2, z, bf16)
    return r1.failures() + r2.failures(), (r1.rows[0]["ratio"], r2.rows[0]["ratio"]), R.pinned_share(e2), z


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("idx", range(len(C.CASES)), ids=CASE_IDS)
def test_honest_fp32_passes_and_every_mutant_fails(idx, bf16):
    case = C.CASES[idx]
    d, p, s32, s64 = _setup(idx)
    bad, ratios, pinned, z = _judge(case, d, p, s32, s64, bf16)
    print(f"{case[0]} {'bf16' if bf16 else 'fp32'} honest: end-to-end {ratios[0]:.4f} from-y {ratios[1]:.4f} pinned {pinned:.4f}")
    assert not bool(torch.isnan(z).any()), "the emulated walk leaves outputs unwritten"
    assert bad == [], "an honest fp32 evaluation is outside a bound:\n" + "\n".join(bad)
    assert 0 < ratios[0] <= 1 and ratios[1] <= 1
    if bf16:  # from the reference alone: a case with few pinned intervals would hide a rounding error
        assert pinned > 0.5
    for m in R.NEUTRAL:
        zn, _ = R.emulate(d["x"], d["w"], d["sc"], d["sh"], d["wd"], p, bf16, m, stem=s32)
        assert torch.equal(zn, z), f"{m} changes the output: it belongs to MUTANTS"
    for m in R.MUTANTS:
        if R.expressible(m, case[2], p, bf16, case[3]):
            badm, rm, _, _ = _judge(case, d, p, s32, s64, bf16, m)
            print(f"{case[0]} {'bf16' if bf16 else 'fp32'} {m}: end-to-end {rm[0]:.3g} from-y {rm[1]:.3g}")
            assert badm, f"mutant {m} passes both checks of {case[0]}"


def test_every_mutant_is_expressed_somewhere():
    """The pairs left out are exactly those of the rules in stemdw_ref.expressible, and none of them empties a mutant's list."""
    ran = {m: 0 for m in R.MUTANTS}
    runs = [(c, b) for c in C.CASES for b in (False, True)]
    for c, b in runs:
        for m in R.MUTANTS:
            ran[m] += R.expressible(m, c[2], _plan(c), b, c[3])
    assert all(n > 0 for n in ran.values()), ran
    always = ("slots_swapped", "plane_m1", "halo_row_act", "halo_col_act", "kd_swapped", "drop_tap")
    assert all(ran[m] == len(runs) for m in always)
    assert ran["no_y_round"] == ran["round_after_affine"] == len(C.CASES)
    assert ran["ci1_dropped"] + ran["pad_k_live"] == len(runs)
    assert ran["no_reset"] == 2 * sum(_plan(c)["sd"] >= 3 for c in C.CASES) >= 8
    assert ran["row_wrong_side"] == 2 * sum(_plan(c)["grid"][0] >= 2 for c in C.CASES)
    assert ran["use_a_uncut"] == 2 * sum(_plan(c)["grid"][1] >= 2 for c in C.CASES)
