"""tests/heads_ref.py checked without a GPU.  The plan mirror answers the library's three host-only queries exactly, at every case
of tests/heads_cases.py and on a sweep of 2500 shapes; every case reaches the route its id names and every route the mirror can
name has a case; the honest fp32 emulation lies inside every bound with a ratio below 1 / 4 (the margin heads_ref.K was given
over the measured maximum); the share of bwd-data elements whose bf16 rounding interval holds two values stays under
heads_ref.UNPINNED_CAP; and - the proof that the checks bite - each of the thirteen wrong kernels fails at every case and entry
that can express it.  The measured ratios are printed."""
import functools
import random

import pytest

from mslesions3d_amd import _lib
from tests import heads_cases as C
from tests import heads_ref as R

FP32_ENTRIES = ("fwd", "bwd_data", "bwd_data_bf16", "bww", "bww_bf16", "pack")


def entries(case):
    return ("fwd_bf16",) if case[0].startswith("bf16.") else FP32_ENTRIES


def assert_queries(N, Cc, dims, ncls):
    """The mirror against msl_head_fwd_workspace_bytes, msl_head_conv_bwd_weight_nslabs, msl_head_bwd_weight_workspace_bytes."""
    L = _lib.load()
    shape = (N, Cc, *dims, ncls)
    assert L.msl_head_fwd_workspace_bytes(*shape) == R.fwd_workspace_bytes(N, Cc, dims, ncls), shape
    assert L.msl_head_conv_bwd_weight_nslabs(*shape) == R.bww_nslabs(N, Cc, dims, ncls), shape
    assert L.msl_head_bwd_weight_workspace_bytes(*shape) == R.bww_workspace_bytes(N, Cc, dims, ncls), shape


def assert_route(case):
    """The route the id names, held against the mirror and the mirror against the library -> the plan."""
    id_, N, Cc, dims, ncls = case
    p = R.plan(N, Cc, dims, ncls)
    if id_.startswith("bf16."):
        assert Cc % 32 == 0 and 12 + 2 * ncls <= 16
        assert id_.startswith(R.bf16_route_name(Cc) + ":"), f"{id_}: the tail loop runs {R.bf16_route_name(Cc)}"
        return p
    assert id_.startswith(R.route_name(p) + ":"), f"{id_}: the mirror says {R.route_name(p)}"
    assert_queries(N, Cc, dims, ncls)
    L = _lib.load()
    ksg, S, MT = p["fwd"]["ksg"], dims[0] * dims[1] * dims[2], p["MT"]
    if ksg > 1:  # the library's own K split, read off its workspace size
        assert L.msl_head_fwd_workspace_bytes(N, Cc, *dims, ncls) == ksg * N * S * 16 * MT * 4
    assert L.msl_head_conv_bwd_weight_nslabs(N, Cc, *dims, ncls) == p["bww"]["nblocks"]
    return p


@pytest.mark.parametrize("case", C.ALL_CASES, ids=C.ids(C.ALL_CASES))
def test_case_reaches_its_route(case):
    assert_route(case)


def sweep(n=2500, seed=7):
    rng = random.Random(seed)
    for _ in range(n):
        kind = rng.random()
        if kind < 0.4:  # the shapes the LDS kernels take are rare among random extents
            w = rng.choice((4, 8, 16))
            dims = (rng.randint(1, 48), w, w)
        elif kind < 0.6:
            dims = (rng.randint(1, 12) * 4 if rng.random() < 0.5 else rng.randint(1, 48), rng.randint(1, 12) * 4, rng.randint(1, 6) * 8)
        else:
            dims = (rng.randint(1, 48), rng.randint(1, 48), rng.randint(1, 48))
        yield rng.randint(1, 6), 16 * rng.randint(1, 32), dims, rng.randint(1, 10)


def test_mirror_answers_the_queries_on_a_sweep():
    names = set()
    n = 0
    for N, Cc, dims, ncls in sweep():
        assert_queries(N, Cc, dims, ncls)
        names.add(R.route_name(R.plan(N, Cc, dims, ncls)))
        n += 1
    assert n >= 2000 and len(names) > 100


def kernel_names(p):
    f = p["fwd"]
    return {"fwd:" + f["kernel"] + ("c" if f["cubic"] else "t" if f["kernel"] != "reg" else "") + f".m{p['MT']}",
            "bwd:" + p["bwd_data"]["kernel"], "bww:" + p["bww"]["kernel"] + f".m{p['MT']}"}


def test_every_route_has_a_case():
    """Every kernel the mirror names on the sweep (forward: by block width, cubic or tiled, output tiles; bwd-data and weight
    gradient: by kernel) is reached by a case, and so is every edge the table is built for."""
    have = set()
    for c in C.CASES:
        have |= kernel_names(R.plan(*c[1:]))
    can = set()
    for s in sweep():
        can |= kernel_names(R.plan(*s))
    assert can <= have, sorted(can - have)
    plans = [R.plan(*c[1:]) for c in C.CASES]
    assert {p["fwd"]["ksg"] for p in plans} >= {1, 2, 4, 16}
    lds = [p for p in plans if p["bwd_data"]["kernel"] != "reg"]
    assert any(p["bwd_data"]["cts"] == 2 and p["bwd_data"]["ragged"] for p in lds) and any(p["bwd_data"]["cts"] >= 4 for p in lds)
    assert any(p["bwd_data"]["kernel"] == "reg" and p["bwd_data"]["groups"] == 2 and p["bwd_data"]["ragged"] for p in plans)
    w = [p["bww"] for p in plans]
    assert any(b["kernel"] != "reg" and b["bpw"] == 3 and b["ragged"] for b in w)
    assert any(b["kernel"] != "reg" and b["bpw"] > R.HEAD_BWW_SB and b["bpw"] % R.HEAD_BWW_SB for b in w)
    assert any(b["kernel"] == "reg" and b["dead_waves"] >= 1 and b["nblocks"] > 1 for b in w)
    assert any(b["kernel"] == "reg" and b["steps"] > 8 for b in w)
    assert any(c[1] * c[3][0] * c[3][1] * c[3][2] % 4 for c in C.CASES)
    assert any(b["nblocks"] > R.GR_FEW for b in w) and any(8 < b["nblocks"] <= R.GR_FEW for b in w)  # both folds of the reduction
    assert {c[4] for c in C.CASES} >= {1, 2, 3, 10} and any(c[3] == (1, 1, 1) for c in C.CASES)
    assert {R.bf16_route_name(c[2]) for c in C.BF16_CASES} == {"bf16.t0", "bf16.t1", "bf16.t2", "bf16.t3"}
    assert max(c[1] * c[2] * c[3][0] * c[3][1] * c[3][2] for c in C.ALL_CASES) <= 6e5  # small enough for well under a second each


@functools.lru_cache(maxsize=None)
def _data(idx):
    return C.make_data(C.ALL_CASES[idx])


@functools.lru_cache(maxsize=None)
def _reference(idx, bf16):
    return R.reference(_data(idx), bf16)


def ref_of(idx, entry):
    return _reference(idx, entry in ("fwd_bf16", "bww_bf16"))


RUNS = [(i, e) for i, c in enumerate(C.ALL_CASES) for e in entries(c)]
RUN_IDS = [f"{C.ALL_CASES[i][0]}-{e}" for i, e in RUNS]


@pytest.mark.parametrize("idx,entry", RUNS, ids=RUN_IDS)
def test_honest_fp32_passes_and_every_mutant_fails(idx, entry):
    case = C.ALL_CASES[idx]
    p, d, e = assert_route(case), _data(idx), ref_of(idx, entry)
    rep = R.check(case, entry, e, R.emulate(case, entry, d, p), d)
    print(f"{case[0]} {entry} honest " + " ".join(f"{r['what']}={r['ratio']:.4f}" for r in rep.rows))
    assert rep.failures() == [], "the honest fp32 emulation is outside a bound"
    # the margin K was given, the measured maximum times 4 (rows held to a bound: a bf16 row's figure is over B + half an ulp)
    assert all(r["ratio"] < 0.25 for r in rep.rows if r["pinned"] is None), [r["msg"] for r in rep.rows]
    for m in R.MUTANTS:
        if R.applicable(m, entry, case, p):
            rm = R.check(case, entry, e, R.emulate(case, entry, d, p, mut=m), d)
            print(f"{case[0]} {entry} {m} " + " ".join(f"{r['what']}={r['ratio']:.4g}" for r in rm.rows))
            assert rm.failures(), f"mutant {m} passes every check of {case[0]} ({entry})"


def test_every_mutant_runs_and_only_impossible_pairs_are_skipped():
    ran = {m: 0 for m in R.MUTANTS}
    for i, entry in RUNS:
        case = C.ALL_CASES[i]
        p = R.plan(*case[1:])
        for m in R.MUTANTS:
            ran[m] += R.applicable(m, entry, case, p)
    assert all(n > 0 for n in ran.values()), ran
    conv = sum(1 for i, e in RUNS if e != "pack")
    assert ran["drop_tap"] == conv and ran["halo_origin"] == conv
    assert ran["row12"] == sum(1 for i, e in RUNS if e.startswith("fwd"))
    assert ran["ragged_group"] == 2 * sum(1 for c in C.CASES if R.plan(*c[1:])["bwd_data"]["kernel"] != "reg")
    assert ran["pad_rows"] == sum(1 for c in C.CASES if c[4] not in (2, 10))


@pytest.mark.parametrize("idx", range(len(C.CASES)), ids=C.ids(C.CASES))
def test_unpinned_share_of_the_bf16_gradient_is_under_its_cap(idx):
    """From the reference alone: where the rounding interval of an element is one bf16 value only round-to-nearest-even of an
    accumulator inside its bound passes; a case in which many elements are free to take two values would hide a rounding error."""
    share = R.unpinned_share(_reference(idx, False))
    print(f"{C.CASES[idx][0]}: unpinned share {share:.5f}")
    assert share <= R.UNPINNED_CAP
