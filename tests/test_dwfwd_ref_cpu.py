"""tests/dwfwd_ref.py checked without a GPU.  The float64 reference agrees with float64 F.conv3d(groups = C) at every case of
tests/dwfwd_cases.py; every case reaches the route its id names and the reference's planners count the partials the library's
queries count (host arithmetic); the slot maps cover every output exactly once below NP; an honest fp32 evaluation (one fmaf chain
in tap order, one bf16_rne at the end) lies inside every bound of every case, no element excluded; on every bf16 case more than
half of the elements are pinned to a single bf16 value; and - the proof that the checks bite - ten kinds of wrong kernel fail at
every case that can express them."""
import functools

import pytest
import torch
import torch.nn.functional as F

from mslesions3d_amd import _lib
from tests import dwfwd_cases as C
from tests import dwfwd_ref as D

OP_FWD = 0


def assert_route(case):
    """The route the id names, asked of the library -> (route, plan) of the reference's own planners."""
    id_, entry, bf16, N, Cc, dims, stride, o = case
    L = _lib.load()
    shape = (N, Cc, *dims, stride)
    want = o["route"]
    if entry in ("eval", "small_bf16"):
        got = L.msl_dwconv_route_kind(OP_FWD, bf16, *shape)
        assert got == D.KIND[want], f"{id_}: route kind {got}, the case is named for {want} = {D.KIND[want]}"
        if want == "rows_eval":
            assert L.msl_dwconv_fwd_eval_rows_ok(*shape) == 1
        return want, {}
    route, plan = D.train_route(bool(bf16), N, Cc, dims, stride, bool(o.get("force_naive")))
    assert route == want, f"{id_}: the reference's planner says {route}, the case is named for {want}"
    if o.get("force_naive"):  # no query counts a forced launch; the shape has a faster route of its own
        assert L.msl_dwconv_fwd_variant(*shape) != D.VARIANT["naive"]
        return route, plan
    _, per = D.slots(route, plan, dims, stride)
    if bf16:
        wave_np = L.msl_dwconv_wave_num_partials(*shape)
        assert (wave_np > 0) == (want == "wave"), f"{id_}: msl_dwconv_wave_num_partials = {wave_np}, the case is named for {want}"
        assert L.msl_dwconv_fwd_bf16_num_partials(*shape) == N * per, f"{id_}: the slot map has {N * per} partials"
    else:
        got = L.msl_dwconv_fwd_variant(*shape)
        assert got == D.VARIANT[want], f"{id_}: variant {got}, the case is named for {want} = {D.VARIANT[want]}"
        assert L.msl_dwconv_fwd_num_partials(*shape) == N * per, f"{id_}: the slot map has {N * per} partials"
    if "ipt" in o:
        assert plan["ipt"] == o["ipt"], f"{id_}: stream instantiation ipt = {plan['ipt']}"
    return route, plan


def variants(case):
    """(affine, sc, sh) of every run of a case, from host-made vectors."""
    d = C.make_data(case)
    if case[1] == "fold":
        return d, [(1,) + C.host_fold_vectors(d)]
    return d, [(0, None, None), (1, d["sc"], d["sh"])]


@functools.lru_cache(maxsize=None)
def _expect(idx, affine):
    case = C.ALL_CASES[idx]
    d, vs = variants(case)
    _, sc, sh = next(v for v in vs if v[0] == affine)
    return D.expect(d["x"], d["w"], case[6], sc, sh)


def runs():
    return [(i, v[0]) for i, c in enumerate(C.ALL_CASES) for v in variants(c)[1]]


RUNS = runs()
RUN_IDS = [f"{C.ALL_CASES[i][0]}-aff{a}" for i, a in RUNS]


# ------------------------------------------------------------------------------------------------- routes (host arithmetic)
@pytest.mark.parametrize("case", C.ALL_CASES, ids=C.ids(C.ALL_CASES))
def test_case_reaches_its_path(case):
    assert_route(case)


def test_every_path_has_a_case():
    ids = " ".join(C.ids(C.ALL_CASES))
    for name in ("wave-s1:", "wave-s1-bf16:", "wave-s2:", "wave-s2-bf16:", "stream<1,1,4>", "stream<1,4,12>", "stream<2,1,4>",
                 "stream<2,4,12>", "resident:", "naive:", "naive-forced:", "tiled-bf16:", "rows-eval:", "rows-eval-bf16:",
                 "small-eval:", "small-eval-bf16:", "small-eval-bf16-own-entry:", "fold-wave-s1-np6", "fold-wave-s1-bf16-np70",
                 "fold-wave-s2-np70", "fold-wave-s2-bf16-np6"):
        assert name in ids, name
    # small enough to run in well under a second each: at most 2e5 outputs, and one input (resident, G = 4) of 5.2e5 elements
    assert max(c[3] * c[4] * torch.tensor(D.out_dims(c[5], c[6])).prod().item() for c in C.ALL_CASES) <= 2e5
    assert sorted(c[3] * c[4] * c[5][0] * c[5][1] * c[5][2] for c in C.ALL_CASES)[-2] <= 2e5
    split = [c for c in C.TRAIN_CASES if c[7]["route"] == "wave" and D.wave_plan(c[3], c[4], c[5], c[6])["wpp"] > 4]
    assert split, "no split-plane wave case (one partial per four waves)"
    assert {D.lds_plan(c[3], c[4], c[5], c[6])["G"] for c in C.TRAIN_CASES if c[7]["route"] == "resident"} >= {1, 2, 4}
    # both staging paths of dw_fwd_bf16_kernel with more than one tile along W
    wide = [(c[5][2] % 8 == 0) for c in C.TRAIN_CASES if c[7]["route"] == "tiled" and D.out_dims(c[5], c[6])[2] > 32]
    assert True in wide and False in wide


# ------------------------------------------------------------------------------------------------- slot maps
@pytest.mark.parametrize("case", C.TRAIN_CASES + C.FOLD_CASES, ids=C.ids(C.TRAIN_CASES + C.FOLD_CASES))
def test_slot_map_covers_every_output_once(case):
    id_, entry, bf16, N, Cc, dims, stride, o = case
    route, plan = assert_route(case)
    slot, per = D.slots(route, plan, dims, stride)
    OD, OH, OW = D.out_dims(dims, stride)
    assert tuple(slot.shape) == (OD, OH, OW) and int(slot.min()) >= 0 and int(slot.max()) < per
    assert sorted(slot.unique().tolist()) == list(range(per)), "a slot no output feeds would keep what the buffer held"
    ones = torch.ones((N, Cc, OD, OH, OW), dtype=torch.float64)
    counts = D.slot_sums(ones, slot, per)
    assert tuple(counts.shape) == (Cc, N * per) and float(counts.sum()) == N * Cc * OD * OH * OW
    L = _lib.load()
    if not o.get("force_naive"):
        q = L.msl_dwconv_fwd_bf16_num_partials if bf16 else L.msl_dwconv_fwd_num_partials
        assert N * per == q(N, Cc, *dims, stride)


# ------------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("idx,affine", RUNS, ids=RUN_IDS)
def test_reference_matches_float64_conv3d(idx, affine):
    case = C.ALL_CASES[idx]
    d, vs = variants(case)
    _, sc, sh = next(v for v in vs if v[0] == affine)
    e = _expect(idx, affine)
    a = (D.act32(d["x"], sc, sh) if affine else d["x"]).double()
    Cc = case[4]
    ref = F.conv3d(a, d["w"].double().view(Cc, 1, 3, 3, 3), stride=case[6], padding=1, groups=Cc)
    mag = F.conv3d(a.abs(), d["w"].double().abs().view(Cc, 1, 3, 3, 3), stride=case[6], padding=1, groups=Cc)
    cnt = F.conv3d(torch.ones((1, 1) + tuple(case[5]), dtype=torch.float64), torch.ones((1, 1, 3, 3, 3), dtype=torch.float64),
                   stride=case[6], padding=1)[0, 0]
    assert tuple(ref.shape[2:]) == D.out_dims(case[5], case[6])
    assert torch.allclose(e["y"], ref, rtol=0, atol=1e-12) and torch.allclose(e["absdot"], mag, rtol=0, atol=1e-12)
    assert torch.equal(e["taps"], cnt) and 1 <= float(cnt.min()) and float(cnt.max()) <= 27


# ------------------------------------------------------------------------------------------------- pinned share
@pytest.mark.parametrize("idx,affine", [r for r in RUNS if C.ALL_CASES[r[0]][2]],
                         ids=[i for r, i in zip(RUNS, RUN_IDS) if C.ALL_CASES[r[0]][2]])
def test_more_than_half_of_a_bf16_case_is_pinned(idx, affine):
    """Where the rounding interval of an element is one bf16 value, only round-to-nearest-even of an accumulator inside its
    bound passes; a case in which few elements are pinned would hide a rounding-mode error."""
    share = D.pinned_share(_expect(idx, affine))
    print(f"{C.ALL_CASES[idx][0]}-aff{affine}: pinned share {share:.4f}")
    assert share > 0.5


# ------------------------------------------------------------------------------------------------- honest fp32 and the wrong kernels
def expressible(case, affine, d, sc, sh, mutant):
    """False for the (run, mutant) pairs that are structurally impossible, each for the reason written next to it."""
    id_, entry, bf16, N, Cc, dims, stride, o = case
    stats = entry in ("train", "fold")
    if mutant == "halo_act":             # no activation without the affine; a halo of act(0) is a zero halo unless a shift is positive
        return bool(affine) and bool((sh > 0).any())
    if mutant == "abs":                  # |v| is relu(v) unless some pre-activation is negative (one voxel, one channel: it is alive)
        return bool(affine) and bool((D.fma32(d["x"], D._bc(sc, d["x"]).float(), D._bc(sh, d["x"]).float()) < 0).any())
    if mutant == "reversed":             # one voxel: the centre tap is the only one inside the volume and is its own mirror image
        return dims != (1, 1, 1)
    if mutant == "origin":               # stride 2 only
        return stride == 2
    if mutant == "trunc":                # one voxel: a single value that happens to round down is truncated to the same bits
        return bool(bf16) and dims != (1, 1, 1)
    if mutant == "twice":                # one voxel: nothing is added before the centre tap, so nothing is rounded twice
        return bool(bf16) and dims != (1, 1, 1)
    if mutant in ("stats_stored", "sq_rounded"):
        return bool(bf16) and stats
    if mutant == "slot_later":
        return stats
    return True                          # drop_tap: every run


def failures(case, e, y, part, route, plan):
    rep = D.check(case[0], e, y, case[2], part, route, plan, case[5], case[6])
    return rep.failures()


@pytest.mark.parametrize("idx,affine", RUNS, ids=RUN_IDS)
def test_honest_fp32_passes_and_every_mutant_fails(idx, affine):
    case = C.ALL_CASES[idx]
    id_, entry, bf16, N, Cc, dims, stride, o = case
    d, vs = variants(case)
    _, sc, sh = next(v for v in vs if v[0] == affine)
    route, plan = assert_route(case)
    stats = (route, plan, dims) if entry in ("train", "fold") else None
    e = _expect(idx, affine)
    y, part = D.emulate(d["x"], d["w"], stride, bf16, sc, sh, stats)
    assert (part is None) == (stats is None)
    assert failures(case, e, y, part, route, plan) == [], "an honest fp32 evaluation is outside a bound"
    for m in D.MUTANTS:
        if expressible(case, affine, d, sc, sh, m):
            ym, pm = D.emulate(d["x"], d["w"], stride, bf16, sc, sh, stats, mut=m)
            assert failures(case, e, ym, pm, route, plan), f"mutant {m} passes every check of {id_} (affine {affine})"


def test_only_structurally_impossible_pairs_are_skipped():
    """Every mutant is rejected somewhere, and the pairs left out are exactly those of the rules in ``expressible``: drop_tap runs
    everywhere, slot_later at every run with statistics, the bf16 mutants at every bf16 run (``trunc``, ``twice`` and ``reversed`` bar one voxel)."""
    ran = {m: 0 for m in D.MUTANTS}
    for i, a in RUNS:
        case = C.ALL_CASES[i]
        d, vs = variants(case)
        _, sc, sh = next(v for v in vs if v[0] == a)
        for m in D.MUTANTS:
            ran[m] += expressible(case, a, d, sc, sh, m)
    bf = sum(1 for i, a in RUNS if C.ALL_CASES[i][2])
    one_voxel_bf = sum(1 for i, a in RUNS if C.ALL_CASES[i][2] and C.ALL_CASES[i][5] == (1, 1, 1))
    with_stats = sum(1 for i, a in RUNS if C.ALL_CASES[i][1] in ("train", "fold"))
    assert all(n > 0 for n in ran.values()), ran
    assert ran["drop_tap"] == len(RUNS) and ran["slot_later"] == with_stats
    assert ran["trunc"] == bf - one_voxel_bf and ran["twice"] == bf - one_voxel_bf
    one_alive_voxel = sum(1 for i, a in RUNS if a and C.ALL_CASES[i][4:6] == (1, (1, 1, 1)))
    assert ran["halo_act"] == sum(1 for i, a in RUNS if a) and ran["abs"] == ran["halo_act"] - one_alive_voxel
    assert ran["origin"] == sum(1 for i, a in RUNS if C.ALL_CASES[i][6] == 2)
