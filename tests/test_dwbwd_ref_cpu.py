"""tests/dwbwd_ref.py checked without a GPU.  The float64 reference agrees with float64 autograd of F.conv3d(groups = C) at every
case shape of tests/dwbwd_cases.py; every case reaches the route its id names (host arithmetic: msl_dwconv_route_kind and the
*_num_partials queries); an honest fp32 evaluation of every case lies inside every bound; and - the proof that the bounds bite -
eight kinds of wrong kernel fail ``worst()`` at every case that can express them."""
import pytest
import torch
import torch.nn.functional as F

from mslesions3d_amd import _lib
from tests import dwbwd_cases as C
from tests import dwbwd_ref as D

NAN = float("nan")
MUTANTS = ("tap_swap", "parity_pair", "drop_last", "halo", "acc_twice", "mask_y", "slot_unwritten", "unrounded")
SWAP = [k + 2 if k == 12 else k - 2 if k == 14 else k for k in range(27)]  # kd * 9 + kh * 3 + 0 <-> + 2 at (kd, kh) = (1, 1)


def expressible(case, mutant):
    """False for the (case, mutant) pairs that are structurally impossible, each for the reason written next to it."""
    _, entry, bf16, N, Cc, dims, stride, acc, o = case
    if mutant == "parity_pair":     # the k = 0 / k = 2 pair of an odd index exists at stride 2 only
        return stride == 2
    if mutant == "halo":            # an out-of-range output index next to the volume: every axis at stride 1; at stride 2 only
        return stride == 1 or any(d % 2 == 0 for d in dims)  # past an EVEN extent (o = I / 2 for k = 0) - 5 x 7 x 9 has none
    if mutant == "acc_twice":       # nothing to add twice without accumulate
        return acc == 1
    if mutant == "mask_y":          # no ReLU mask where no BatchNorm sums are formed
        return D.has_sums(case)
    if mutant == "slot_unwritten":  # no partials
        return D.has_sums(case) or entry in ("bww", "bww_bf16")
    if mutant == "unrounded":       # sums of a STORED bf16 gradient only (the one-pass bf16 entry stores none)
        return entry == "patch_bf16" and bool(o.get("yprev"))
    return True                     # tap_swap, drop_last: every case


# ------------------------------------------------------------------------------------------------- reference against autograd
SHAPES = sorted({(c[3], c[4], c[5], c[6]) for c in C.ALL_CASES})


@pytest.mark.parametrize("N,Cc,dims,stride", SHAPES, ids=[f"{C._shape(s[0], s[1], s[2])}-s{s[3]}" for s in SHAPES])
def test_refs_match_float64_autograd(N, Cc, dims, stride):
    g = C.gen(N + 10 * Cc + sum(dims) + stride)
    a = torch.randn((N, Cc) + tuple(dims), generator=g, dtype=torch.float64).requires_grad_(True)
    w = torch.randn((Cc, 1, 3, 3, 3), generator=g, dtype=torch.float64).requires_grad_(True)
    out = F.conv3d(a, w, stride=stride, padding=1, groups=Cc)
    assert tuple(out.shape[2:]) == D.out_dims(dims, stride)
    dy = torch.randn(out.shape, generator=g, dtype=torch.float64)
    out.backward(dy)
    gr, ga, taps = D.bwd_data_ref(dy, w.detach().view(Cc, 27), stride, dims)
    assert torch.allclose(gr, a.grad, rtol=0, atol=1e-12) and bool((ga >= gr.abs() - 1e-12).all())
    dr, da = D.bww_ref(dy, a.detach(), stride)
    assert torch.allclose(dr, w.grad.view(Cc, 27), rtol=0, atol=1e-12) and bool((da >= dr.abs() - 1e-12).all())
    t = set(taps.unique().tolist())
    assert t <= ({1.0, 2.0, 4.0, 8.0} if stride == 2 else set(float(i) for i in range(1, 28))) and max(t) <= 27


def test_bf16_unit_roundoff():
    """One bf16 rounding costs up to 2**-8 |x| / (1 + 2**-8), not 2**-9 |x|: BF16_U is the format's, and it is attained."""
    x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.999])
    err = (D.bf16_round(x).double() - x.double()).abs() / x.double()
    assert float(err[0]) > 2.0 ** -9 and float(err[1]) > 2.0 ** -9 and bool((err <= D.BF16_U).all())
    g = C.gen(5)
    r = torch.randn(100000, generator=g)
    assert bool(((D.bf16_round(r).double() - r.double()).abs() <= D.BF16_U * r.double().abs()).all())


# ------------------------------------------------------------------------------------------------- routes (host arithmetic)
@pytest.mark.parametrize("case", C.ALL_CASES, ids=C.ids(C.ALL_CASES))
def test_case_reaches_its_path(case):
    assert_route(case)


def assert_route(case):
    id_, entry, bf16, N, Cc, dims, stride, acc, o = case
    L = _lib.load()
    if "kind" in o:
        got = L.msl_dwconv_route_kind(o["op"], bf16, N, Cc, *dims, stride)
        assert got == D.KIND[o["kind"]], f"{id_}: route kind {got}, the case is named for {o['kind']} = {D.KIND[o['kind']]}"
    if "blocks" in o:
        q = L.msl_dwconv_s2_bwd_bnreduce_bww_num_partials if o.get("path") == "onepass" else L.msl_dwconv_bwd_data_bnreduce_num_partials
        assert q(N, Cc, *dims) == N * o["blocks"], f"{id_}: {q(N, Cc, *dims)} partials, the case is named for {N} x {o['blocks']}"


def test_route_query_refuses_bad_arguments():
    L = _lib.load()
    ok = (1, 4, 4, 4, 4, 1)
    assert L.msl_dwconv_route_kind(2, 0, *ok) == D.KIND["resident"]
    for args in ((-1, 0) + ok, (4, 0) + ok, (2, 2) + ok, (2, -1) + ok, (2, 0, 0, 4, 4, 4, 4, 1), (2, 0, 1, 0, 4, 4, 4, 1),
                 (2, 0, 1, 4, 0, 4, 4, 1), (2, 0, 1, 4, 4, 4, 4, 3), (2, 0, 1, 4, 4, 4, 4, 0)):
        assert L.msl_dwconv_route_kind(*args) == -1, args
    assert L.msl_dwconv_route_kind(1, 0, 1, 4, 4, 4, 4, 2) == D.KIND["none"]  # the flipped forward is a stride-1 route


# ------------------------------------------------------------------------------------------------- fp32 emulation and its mutants
def slot_sums32(t, slot, blocks):
    N, Cc = t.shape[:2]
    out = torch.zeros((N, Cc, blocks), dtype=torch.float32)
    out.index_add_(2, slot.reshape(-1), t.reshape(N, Cc, -1))
    return out.permute(1, 0, 2).reshape(Cc, N * blocks).double()


def emulate(case, d, mutant=None):
    """The kernels' arithmetic in fp32 tensors (any order; products and sums rounded separately, which is no better than fma),
    the partial sums taken in fp32 per slot.  ``mutant``: one of MUTANTS, the wrong kernel to build instead."""
    _, entry, bf16, N, Cc, dims, stride, acc, o = case
    dy, w, y, old, vec = d["dy"], d["w"].clone(), d["y"], d["old"], d["vec"]
    Dd, H, W = dims
    if mutant == "tap_swap":        # kd * 9 + kh * 3 + 0 <-> + 2 at (kd, kh) = (1, 1): the one row every shape uses
        w[:, [12, 14]] = w[:, [14, 12]]
    if mutant == "parity_pair":     # k = 0 <-> k = 2 on the W axis
        w = w.view(Cc, 9, 3)[:, :, [2, 1, 0]].reshape(Cc, 27)
    dye = dy
    if mutant == "halo":            # the output one past the end exists and holds its neighbour's value
        ax = 4 if (stride == 1 or W % 2 == 0) else 3 if H % 2 == 0 else 2
        dye = torch.cat([dy, dy.narrow(ax, dy.shape[ax] - 1, 1)], ax)
    T, _ = D.tap_planes(dye, stride, dims)
    T = T.float()
    out = {}
    a32 = D.act32(y, vec[0], vec[1]) if (entry in D.HAS_W_PARTIALS or o.get("affine")) else y
    if mutant == "drop_last" and entry not in D.HAS_G:
        a32 = a32.clone()
        a32[:, :, Dd - 1] = 0.0     # the weight gradient loses the last input plane
    if entry in D.HAS_G or entry in D.HAS_W_PARTIALS:
        g = torch.zeros((N, Cc) + tuple(dims))
        for k in range(27):
            g = g + w[:, k].view(1, Cc, 1, 1, 1) * T[k]
        if old is not None:
            g = g + (2.0 * old if mutant == "acc_twice" else old)
        unrounded = g
        if bf16 and entry in D.HAS_G:
            g = D.bf16_round(g)
        if mutant == "drop_last" and entry in D.HAS_G:   # ``id < D`` written as ``id < D - 1``: the buffer keeps what it held
            g = g.clone()
            keep = old if old is not None else torch.zeros_like(g)
            if Dd > 1:
                g[:, :, Dd - 1] = keep[:, :, Dd - 1]
            elif H > 1:
                g[:, :, :, H - 1] = keep[:, :, :, H - 1]
            else:
                g[..., W - 4:] = keep[..., W - 4:]
        if entry in D.HAS_G:
            out["g_in"] = g
        if D.has_sums(case):
            per = D.PATCHES_PER_BLOCK[o["path"]]
            slot, blocks = D.patch_slot(dims, per), D.num_blocks(dims, per)
            bc = lambda v: v.view(1, -1, 1, 1, 1)
            mask = (y > 0) if mutant == "mask_y" else (D.fma32(y, bc(vec[0]), bc(vec[1])) > 0)
            gs = unrounded if mutant == "unrounded" else g
            gm = torch.where(mask, gs, torch.zeros(()))
            t2 = gm * ((y - bc(vec[2])) * bc(vec[3]))
            bn = torch.stack([slot_sums32(gm, slot, blocks), slot_sums32(t2, slot, blocks)])
            if mutant == "slot_unwritten":
                bn[1, 0, 0] = NAN
            out["bn_partials"] = bn
    if entry in D.HAS_W_PARTIALS:
        per = D.PATCHES_PER_BLOCK[o["path"]]
        slot, blocks = D.patch_slot(dims, per), D.num_blocks(dims, per)
        wp = torch.stack([slot_sums32(a32 * T[k], slot, blocks) for k in range(27)], 1)
        if mutant == "tap_swap":    # the weight gradient's own tap index
            wp = wp[:, SWAP]
        out["w_partials"] = wp.reshape(Cc * 27, -1)
        if o.get("taps_t"):
            out["w_taps_t"] = d["w"].t().contiguous()
    if entry in ("bww", "bww_bf16"):
        # rows of W in fp32 (a thread's chain is never longer), the rest in double like the kernels' partials
        dw = torch.stack([(a32 * T[k]).sum(-1).double().sum((0, 2, 3)) for k in range(27)], 1)
        if mutant == "tap_swap":
            dw = dw[:, SWAP]
        if mutant == "parity_pair":
            dw = dw.view(Cc, 9, 3)[:, :, [2, 1, 0]].reshape(Cc, 27)
        if mutant == "slot_unwritten":
            dw[0, 0] = NAN
        out["dw_sum"] = dw
        if o.get("dw"):
            out["dw"] = dw.float()
    return out


def failures(case, d, got):
    bad = {}
    for name, (ref, bound) in D.expected(case, d, got).items():
        ratio, _, n = D.worst(got[name], ref, bound)
        if n:
            bad[name] = ratio
    return bad


@pytest.mark.parametrize("case", C.ALL_CASES, ids=C.ids(C.ALL_CASES))
def test_honest_fp32_passes_and_every_mutant_fails(case):
    d = C.make_data(case)
    got = emulate(case, d)
    assert set(got) == set(D.expected(case, d, got)), "the emulation and the reference disagree about the outputs of the case"
    assert failures(case, d, got) == {}, "an honest fp32 evaluation is outside a bound"
    for m in MUTANTS:
        if expressible(case, m):
            assert failures(case, d, emulate(case, d, m)), f"mutant {m} passes every bound of {case[0]}"


def test_only_structurally_impossible_pairs_are_skipped():
    """The skipped (case, mutant) pairs are exactly those of the rules in ``expressible``; in particular tap_swap and drop_last
    run at every case, parity_pair at every stride-2 case, and the only stride-2 shape without a halo is 5 x 7 x 9."""
    skipped = {(c[0], m) for c in C.ALL_CASES for m in MUTANTS if not expressible(c, m)}
    assert not any(m in ("tap_swap", "drop_last") for _, m in skipped)
    assert {i for i, m in skipped if m == "parity_pair"} == {c[0] for c in C.ALL_CASES if c[6] == 1}
    assert {i for i, m in skipped if m == "halo"} == {c[0] for c in C.ALL_CASES if c[6] == 2 and c[5] == (5, 7, 9)}
    assert {i for i, m in skipped if m == "acc_twice"} == {c[0] for c in C.ALL_CASES if c[7] == 0}
    assert {i for i, m in skipped if m == "unrounded"} == {c[0] for c in C.ALL_CASES if not (c[1] == "patch_bf16" and c[8].get("yprev"))}
    no_sums = {c[0] for c in C.ALL_CASES if c[1] in ("bwd_data", "bwd_data_bf16", "bww", "bww_bf16") or (c[1] == "patch_bf16" and not c[8].get("yprev"))}
    assert {i for i, m in skipped if m == "mask_y"} == no_sums
    assert {i for i, m in skipped if m == "slot_unwritten"} == no_sums - {c[0] for c in C.ALL_CASES if c[1] in ("bww", "bww_bf16")}
