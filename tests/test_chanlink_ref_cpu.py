"""tests/chanlink_ref.py checked without a GPU: ``plan`` against the library's own host query over a sweep, the case table
against the 13 configurations, the two-stage float64 reference against float64 autograd, the restated thread slots, and - the
proof that the bounds are neither violated by honest fp32 arithmetic nor vacuous - the fp32 emulation of the kernel's order inside
every bound at every case, fp32 and bf16 storage, and nine wrong kernels outside theirs.  No element is skipped anywhere."""
import functools

import pytest
import torch

from mslesions3d_amd import _lib
from tests import bf16pw_ref as P
from tests import chanlink_cases as C
from tests import chanlink_ref as S


@functools.lru_cache(maxsize=None)
def inputs(cid):
    _, N, c, dims, stride, acc = C.BY_ID[cid]
    return S.chain_case(N, c, dims, stride, acc, seed=1 + C.CASES.index(C.BY_ID[cid]))


# ------------------------------------------------------------------------------------------------- planner
def test_plan_is_link_plan_over_a_sweep():
    L = _lib.load()
    pows = [1, 2, 4, 8, 16, 32]
    shapes = [(N, (D, H, W), s) for N in list(range(1, 34)) + [64, 128, 256, 512] for D in pows for H in pows
              for W in pows + [64] for s in (1, 2)]
    shapes += [(N, dims, s) for _, N, _, dims, s, _ in C.REFUSALS] + [(N, dims, s) for _, N, _, dims, s, _ in C.CASES]
    shapes += [(2, (D, 4, 8), s) for D in (3, 5, 6, 7, 12) for s in (1, 2)] + [(2, (4, 4, W), s) for W in (1, 2, 3, 6, 12) for s in (1, 2)]
    seen = set()
    for N, dims, s in shapes:
        p = S.plan(N, dims, s)
        assert L.msl_block_bwd_channel_link_supported(N, *dims, s) == (0 if p is None else p["nw"]), (N, dims, s)
        if p is not None:
            assert (p["nw"], p["qo"], p["qi"], s) in S.CONFIGS, (N, dims, s, p)
            seen.add((p["nw"], p["qo"], p["qi"], s))
    assert seen == set(S.CONFIGS)


def test_case_table_reaches_every_configuration():
    reached = {}
    for cid, N, c, dims, stride, acc in C.CASES:
        p = S.plan(N, dims, stride)
        assert p is not None, cid
        assert S.config(N, dims, stride) == C.config_of_id(cid), cid
        assert 2 <= c <= 4 and N * dims[0] * dims[1] * dims[2] <= 2 ** 16, cid
        # all lanes live: every input-side slot of every thread holds a quad - or, for the one-wave stride-2 form (four slots per
        # lane, at most 128 quads), as many as the configuration can hold: 32 of the 64 lanes of each class
        full = min(p["nw"] * 64 * p["qi"], {1: 128, 4: 1024, 8: 2048, 16: 4096}[p["nw"]])
        live = p["tqi"] == full
        assert live == bool(S.slots(N, dims, stride, p, "in")[1].all()) or (p["nw"], stride) == (1, 2), cid
        reached.setdefault(S.config(N, dims, stride), []).append((acc, live))
    assert set(reached) == set(S.CONFIGS)
    for cfg, rows in reached.items():
        assert {a for a, _ in rows} == {0, 1}, cfg
        assert {l for _, l in rows} == {True, False}, cfg
    assert S.plan(*_shape("s1-w16-q4-lds153856"))["smem"] == 153856
    assert S.plan(*_shape("s1-w4-q1-rows-lds110k"))["smem"] > 64 * 1024
    assert S.plan(25, (8, 8, 8), 1) is None and S.plan(25, (8, 8, 4), 1) is not None  # refused by the LDS cap alone
    for rid, N, c, dims, stride, rc in C.REFUSALS:
        assert (S.plan(N, dims, stride) is None) == (rc == -2 or N <= 0), rid  # (C is no argument of link_plan)


def _shape(cid):
    _, N, _, dims, stride, _ = C.BY_ID[cid]
    return N, dims, stride


@pytest.mark.parametrize("cid", [c[0] for c in C.CASES])
def test_every_quad_is_held_by_exactly_one_live_slot(cid):
    N, dims, stride = _shape(cid)
    p = S.plan(N, dims, stride)
    for side, tot in (("out", p["tqo"]), ("in", p["tqi"])):
        idx, live = S.slots(N, dims, stride, p, side)
        assert idx.shape == (p["qo"] if side == "out" else p["qi"], p["nw"] * 64)
        assert int(idx.min()) >= 0 and int(idx.max()) < tot
        assert sorted(idx[live].tolist()) == list(range(tot)), side


# ------------------------------------------------------------------------------------------------- reference against autograd
@pytest.mark.parametrize("n,c,dims,stride,acc", [(2, 3, (2, 4, 8), 1, 1), (3, 2, (4, 4, 4), 1, 0), (1, 2, (1, 1, 4), 1, 1),
                                                 (2, 3, (4, 4, 8), 2, 1), (3, 2, (2, 8, 8), 2, 0), (1, 4, (8, 2, 16), 2, 1)])
def test_two_stage_reference_is_float64_autograd(n, c, dims, stride, acc):
    inp, auto = S.chain_case(n, c, dims, stride, acc, seed=7)
    p = S.plan(n, dims, stride)
    A = S.stage_a(inp["G"], inp["z"], inp["vz64"], p["qo"])
    # dw of autograd is taken on the float64 activation: hand that in (the kernel's fp32 one is checked in the emulation test)
    sc, sh = (inp["vy64"][k].view(1, -1, 1, 1, 1) for k in (0, 1))
    a_prev = torch.relu(inp["y"].double() * sc + sh)
    B = S.stage_b(A["d"], inp["w"], inp["y"], inp["vy64"], inp["Hs"] if acc else None, stride, p["qi"], False, a_prev=a_prev)
    for what, got, want in (("dz", A["d"], auto["gz"]), ("dgamma1", A["dgamma"], auto["dgam1"]), ("dbeta1", A["dbeta"], auto["dbet1"]),
                            ("dy", B["d"], auto["gy"]), ("dgamma2", B["dgamma"], auto["dgam2"]), ("dbeta2", B["dbeta"], auto["dbet2"]),
                            ("dw", B["dw"], auto["dw"])):
        err = float((got - want).abs().max())
        assert err <= 1e-11 * max(1.0, float(want.abs().max())), (what, err)


def test_float64_sign_is_the_fp32_mask():
    for cid in ("s1-w4-q2-masked", "s2-w8-q4-live"):
        inp, _ = inputs(cid)
        for x, v in ((inp["z"], inp["vz"]), (inp["y"], inp["vy"])):
            assert P.mask_is_kernels(x.flatten(2), v)


# ------------------------------------------------------------------------------------------------- emulation inside the bounds
WORST = {}


def _judge(cid, bf16, out, inp):
    _, N, c, dims, stride, acc = C.BY_ID[cid]
    return S.judge(P.Report(cid), out, inp, N, dims, stride, acc, bf16, with_dw=out["dw"] is not None)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("cid", [c[0] for c in C.CASES])
def test_emulation_is_inside_every_bound(cid, bf16):
    _, N, c, dims, stride, acc = C.BY_ID[cid]
    inp = S.as_bf16(inputs(cid)[0]) if bf16 else inputs(cid)[0]
    out = S.emul(inp, N, dims, stride, acc, bf16=bf16)
    for k in S.KEYS:
        assert not bool(torch.isnan(out[k]).any()), k
    rep = _judge(cid, bf16, out, inp)
    for r in rep.rows:
        key = ("bf16 " if bf16 else "fp32 ") + r["what"]
        WORST[key] = max(WORST.get(key, 0.0), r["ratio"])
    print(cid, "bf16" if bf16 else "fp32", " ".join(f"{r['what']}={r['ratio']:.3f}" for r in rep.rows))
    assert not rep.failures(), rep.failures()


def test_print_worst_emulation_ratio():
    """(Runs after the cases above: the figures of DESIGN.md, Appendix A.3.)"""
    for k in sorted(WORST):
        print(f"worst emul error / bound  {k}: {WORST[k]:.3f}")
    assert all(v <= 1.0 for v in WORST.values())


# ------------------------------------------------------------------------------------------------- wrong kernels
S2 = [c[0] for c in C.CASES if c[4] == 2]
S1 = [c[0] for c in C.CASES if c[4] == 1]
MASKED = [c[0] for c in C.CASES if not bool(S.slots(c[1], c[3], c[4], S.plan(c[1], c[3], c[4]), "out")[1].all())
          or not bool(S.slots(c[1], c[3], c[4], S.plan(c[1], c[3], c[4]), "in")[1].all())]
# mutation -> (cases that exercise it, storage)
EXERCISED = {
    "tap_off": (S2, False),            # class oo (odd plane, odd row) exists at every stride-2 shape; its tap row (2, 2) reads data
    "swap_eo_oe": (S2, False),         # classes eo and oe exist at every stride-2 shape
    "halo": (S1 + S2, False),          # the plane behind the last one is read by the last plane's kd = 0 taps at both strides
    "wrap_w": ([c for c in S1 + S2 if C.BY_ID[c][3][1] // C.BY_ID[c][4] >= 2], False),  # needs a neighbouring row: OH >= 2
    "k1_out_count": (S2, False),       # the counts differ at stride 2 only
    "drop_head": ([c[0] for c in C.CASES if c[5] == 1], False),
    "masked_contrib": (MASKED, False),
    "dw_from_y": (S1 + S2, False),
    "unrounded_dz": (S1 + S2, True),
}


def test_every_mutation_is_listed():
    assert set(EXERCISED) == set(S.MUTATIONS) and all(len(v[0]) >= 2 for v in EXERCISED.values())


# a few cases per mutation keep the test quick; every configuration a mutation touches is among them
def _pick(ids):
    seen, out = set(), []
    for cid in ids:
        cfg = C.config_of_id(cid)
        if cfg not in seen and C.BY_ID[cid][1] * C.BY_ID[cid][3][0] * C.BY_ID[cid][3][1] * C.BY_ID[cid][3][2] <= 2 ** 14:
            seen.add(cfg)
            out.append(cid)
    return out


@pytest.mark.parametrize("mut", S.MUTATIONS)
def test_a_wrong_kernel_leaves_its_bound(mut):
    ids, bf16 = EXERCISED[mut]
    for cid in _pick(ids):
        _, N, c, dims, stride, acc = C.BY_ID[cid]
        inp = S.as_bf16(inputs(cid)[0]) if bf16 else inputs(cid)[0]
        rep = _judge(cid, bf16, S.emul(inp, N, dims, stride, acc, bf16=bf16, mut=mut), inp)
        assert rep.failures(), f"{mut} at {cid} stayed inside every bound: " + " ".join(f"{r['what']}={r['ratio']:.3f}" for r in rep.rows)
