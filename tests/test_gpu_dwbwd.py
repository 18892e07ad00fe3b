"""Every depthwise-convolution BACKWARD entry point - msl_dwconv_bwd_data (+ _bf16), msl_dwconv_bwd_data_bnreduce,
msl_dwconv_bwd_data_s2_patch_bf16, the one-pass msl_dwconv_s2_bwd_[data_]bnreduce_bww (+ _bf16), msl_dwconv_bwd_weight (+ _bf16)
and msl_dwconv_bwd_weight_finalize - path by path against the float64 reference of tests/dwbwd_ref.py (bounds derived there, not
tuned; a failure prints the worst error / bound and its index).

The cases are the CPU data of tests/dwbwd_cases.py; tests/test_dwbwd_ref_cpu.py proves at the same cases that every bound accepts
honest fp32 and rejects eight kinds of wrong kernel.  Every test first asserts the route its case id names (msl_dwconv_route_kind,
or the *_num_partials query of the route-less patch kernels).  Every output and partial buffer is pre-filled with NaN and sits
between guard bands that must come back untouched; every entry runs twice into fresh buffers and must repeat itself bit for
bit.  With MSL_DWBWD_RATIO_LOG=<file> every comparison appends "<case id> <what> <error / bound>" to that file (the table of
DESIGN.md, Appendix B)."""
import ctypes
import os

import pytest
import torch

from mslesions3d_amd import _lib
from mslesions3d_amd._lib import ptr
from tests import dwbwd_cases as C
from tests import dwbwd_ref as D
from tests.test_dwbwd_ref_cpu import assert_route
from tests.test_gpu_pw import Guarded, dev, st
from tests.test_gpu_pw import _release_kept  # noqa: F401  (autouse fixture: frees what dev() and Guarded keep alive)

pytestmark = pytest.mark.gpu
NAN = float("nan")
FINITE_GUARD = -12345.0  # where the kernel under test may itself produce NaNs
ERR_ARG, ERR_UNSUPPORTED = -1, -2


def check(case_id, what, actual, ref, bound):
    ratio, idx, bad = D.worst(actual, ref, bound)
    log = os.environ.get("MSL_DWBWD_RATIO_LOG")
    if log:
        with open(log, "a") as f:
            f.write(f"{case_id} {what} {ratio:.4f}\n")
    print(f"{case_id} {what}: error / bound {ratio:.4f}")
    a, r = actual.detach().cpu().double().reshape(-1), ref.double().reshape(-1)
    assert bad == 0, (f"{case_id} {what}: {bad}/{r.numel()} elements over their bound; worst error / bound {ratio:.3f} at idx {idx} "
                      f"(got {a[idx].item():.9e}, ref {r[idx].item():.9e})")


def same_bits(a, b):
    """Bit identity of two device tensors of one dtype (NaN payloads and zero signs included)."""
    it = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return a.dtype == b.dtype and bool(torch.equal(a.contiguous().view(it), b.contiguous().view(it)))


def grad_reduce_kind1(partials, NP, count):
    """The library's deferred fold of fp64 partials [count][NP] (msl_grad_reduce_batch, kind 1) -> guarded fp32 (count,)."""
    L = _lib.load()
    out = Guarded(count)
    host = (ctypes.c_ubyte * L.msl_grad_reduce_entry_bytes())()
    nb = L.msl_grad_reduce_table_set(ctypes.addressof(host), 0, 0, 1, ptr(partials), ptr(out.v), None, NP, count, 0, 0, 0, 0)
    assert nb > 0
    table = dev(torch.frombuffer(bytearray(host), dtype=torch.uint8))
    assert L.msl_grad_reduce_batch(ptr(table), 1, nb, st()) == 0
    torch.cuda.synchronize()
    out.intact("dw of msl_grad_reduce_batch")
    return out


class Run:
    """One launch of a case's entry point into fresh guarded, NaN-filled buffers."""

    def __init__(self, case, d, entry=None):
        id_, entry0, bf16, N, Cc, dims, stride, acc, o = case
        self.entry = entry = entry or entry0
        L = _lib.load()
        dt = torch.bfloat16 if bf16 else torch.float32
        guard = FINITE_GUARD if o.get("nan") else NAN
        S = dims[0] * dims[1] * dims[2]
        dyd, wd, yd, vec = dev(d["dy"].to(dt)), dev(d["w"]), dev(d["y"].to(dt)), dev(d["vec"])
        v = [ptr(vec[k]) for k in range(4)]
        self.bufs = {}

        def buf(name, n, dtype=torch.float32):
            self.bufs[name] = Guarded(n, dtype=dtype, guard=guard)
            return ptr(self.bufs[name].v)

        def gbuf():
            p = buf("g_in", N * Cc * S, dt)
            if acc:
                self.bufs["g_in"].v.copy_(d["old"].to(dt).reshape(-1))
            return p

        shape = (N, Cc, *dims)
        if entry in ("bwd_data", "bwd_data_bf16"):
            fn = L.msl_dwconv_bwd_data if entry == "bwd_data" else L.msl_dwconv_bwd_data_bf16
            rc = fn(ptr(dyd), ptr(wd), gbuf(), *shape, stride, acc, st())
        elif entry == "patch_bn":
            NP = self.NP = L.msl_dwconv_bwd_data_bnreduce_num_partials(*shape)
            rc = L.msl_dwconv_bwd_data_bnreduce(ptr(dyd), ptr(wd), gbuf(), ptr(yd), *v, buf("bn_partials", 2 * Cc * NP, torch.float64),
                                                *shape, stride, acc, st())
        elif entry == "patch_bf16":
            NP = self.NP = L.msl_dwconv_bwd_data_bnreduce_num_partials(*shape)
            g = gbuf()
            if o.get("yprev"):
                rc = L.msl_dwconv_bwd_data_s2_patch_bf16(ptr(dyd), ptr(wd), g, ptr(yd), ptr(vec), buf("bn_partials", 2 * Cc * NP, torch.float64),
                                                         *shape, acc, st())
            else:
                rc = L.msl_dwconv_bwd_data_s2_patch_bf16(ptr(dyd), ptr(wd), g, None, None, None, *shape, acc, st())
        elif entry in ("onepass_data", "onepass", "onepass_bf16"):
            NP = self.NP = L.msl_dwconv_s2_bwd_bnreduce_bww_num_partials(*shape)
            g = gbuf() if entry == "onepass_data" else None
            bn, wp = buf("bn_partials", 2 * Cc * NP, torch.float64), buf("w_partials", Cc * 27 * NP, torch.float64)
            tt = buf("w_taps_t", 27 * Cc) if o.get("taps_t") else None
            if entry == "onepass_data":
                rc = L.msl_dwconv_s2_bwd_data_bnreduce_bww(ptr(dyd), ptr(wd), g, ptr(yd), *v, bn, wp, *shape, acc, st())
            elif entry == "onepass":
                rc = L.msl_dwconv_s2_bwd_bnreduce_bww(ptr(dyd), ptr(wd), ptr(yd), *v, bn, wp, tt, *shape, st())
            else:
                rc = L.msl_dwconv_s2_bwd_bnreduce_bww_bf16(ptr(dyd), ptr(wd), ptr(yd), ptr(vec), bn, wp, tt, *shape, st())
        elif entry in ("bww", "bww_bf16"):
            aff = (v[0], v[1]) if o.get("affine") else (None, None)
            if entry == "bww":
                NP = self.NP = L.msl_dwconv_bwd_weight_num_partials(*shape, stride)
                dw = buf("dw", Cc * 27) if o.get("dw") else None
                rc = L.msl_dwconv_bwd_weight(ptr(dyd), ptr(yd), *aff, dw, buf("w_sum_partials", Cc * 27 * NP, torch.float64), *shape, stride, st())
            else:
                NP = self.NP = L.msl_dwconv_fwd_bf16_num_partials(*shape, stride)
                rc = L.msl_dwconv_bwd_weight_bf16(ptr(dyd), ptr(yd), *aff, buf("w_sum_partials", Cc * 27 * NP, torch.float64), *shape, stride, st())
        else:
            raise KeyError(entry)
        torch.cuda.synchronize()
        assert rc == 0, f"{id_}: {entry} returned {rc}"
        for name, b in self.bufs.items():
            b.intact(f"{id_}: {name}")
        assert same_bits(dyd, d["dy"].to(dt).to("cuda")) and same_bits(wd, d["w"].to("cuda")) and same_bits(yd, d["y"].to(dt).to("cuda")), \
            f"{id_}: inputs changed"
        self.shape, self.Cc = shape, Cc

    def got(self):
        """The outputs under the names of dwbwd_ref.expected, on the CPU."""
        g, Cc = {}, self.Cc
        for name, b in self.bufs.items():
            t = b.v.detach().cpu()
            if name == "g_in":
                g[name] = t.float().view(self.shape)
            elif name == "bn_partials":
                g[name] = t.view(2, Cc, self.NP)
            elif name == "w_partials":
                g[name] = t.view(Cc * 27, self.NP)
            elif name == "w_taps_t":
                g[name] = t.view(27, Cc)
            elif name == "w_sum_partials":
                g["dw_sum"] = D.exact_sum(t.view(Cc * 27, self.NP)).view(Cc, 27)
            elif name == "dw":
                g[name] = t.view(Cc, 27)
        return g


def run_and_check(case, d=None):
    """Route, two runs, bit identity between them, every output inside its bound -> (first run, its outputs, the expectations)."""
    assert_route(case)
    d = d or C.make_data(case)
    r1, r2 = Run(case, d), Run(case, d)
    for name in r1.bufs:
        assert same_bits(r1.bufs[name].v, r2.bufs[name].v), f"{case[0]}: two runs differ in {name}"
    got = r1.got()
    exp = D.expected(case, d, got)
    assert set(exp) <= set(got), f"{case[0]}: outputs {sorted(got)} but expectations {sorted(exp)}"
    for name, (ref, bound) in exp.items():
        check(case[0], name, got[name], ref, bound)
    return r1, got, exp, d


# ------------------------------------------------------------------------------------------------- msl_dwconv_bwd_data (+ _bf16)
@pytest.mark.parametrize("case", C.BWD_DATA_CASES, ids=C.ids(C.BWD_DATA_CASES))
def test_dw_bwd_data(case):
    run_and_check(case)


@pytest.mark.parametrize("case", C.BWD_DATA_BF16_CASES, ids=C.ids(C.BWD_DATA_BF16_CASES))
def test_dw_bwd_data_bf16(case):
    run_and_check(case)


# ------------------------------------------------------------------------------------------------- patch kernel + BatchNorm sums
@pytest.mark.parametrize("case", C.PATCH_BN_CASES, ids=C.ids(C.PATCH_BN_CASES))
def test_dw_patch_bnreduce(case):
    """msl_dwconv_bwd_data_bnreduce / msl_dwconv_bwd_data_s2_patch_bf16: g_in, the sums of the gradient as stored, and g_in bit
    for bit that of the plain bwd-data entry (the same kernel without the reduce)."""
    r, got, exp, d = run_and_check(case)
    plain = Run(case, d, entry="bwd_data_bf16" if case[2] else "bwd_data")
    assert same_bits(r.bufs["g_in"].v, plain.bufs["g_in"].v), f"{case[0]}: g_in differs from the plain bwd-data entry's"
    if case[8].get("nan"):
        n0, c0 = case[8]["nan"][:2]
        gnan = torch.isnan(got["g_in"])
        assert 1 <= int(gnan.sum()) <= 27 and int(gnan[n0, c0].sum()) == int(gnan.sum()), "the NaN left its footprint"
        pn = torch.isnan(got["bn_partials"])
        assert bool(pn[:, c0].any()) and not bool(pn[:, [c for c in range(case[4]) if c != c0]].any())


# ------------------------------------------------------------------------------------------------- the one-pass kernel
@pytest.mark.parametrize("case", C.ONEPASS_CASES, ids=C.ids(C.ONEPASS_CASES))
def test_dw_onepass(case):
    """msl_dwconv_s2_bwd_data_bnreduce_bww, msl_dwconv_s2_bwd_bnreduce_bww and its _bf16 variant: g_in (where written), the
    BatchNorm partials, the weight partials slot by slot, and the weight transpose bit for bit."""
    id_, entry, bf16, N, Cc, dims, stride, acc, o = case
    r, got, exp, d = run_and_check(case)
    if o.get("taps_t"):
        assert same_bits(r.bufs["w_taps_t"].v.view(27, Cc), d["w"].t().contiguous().to("cuda")), "w_taps_t is not w.T bit for bit"
    if entry == "onepass_data":
        # the patch kernel on the same operands: the sums of both agree within the sum of both bounds (+ what a gradient that
        # differs within its own bound may move them by; the two kernels form g_in in the same order, so this is usually 0)
        pcase = (id_, "patch_bn", 0, N, Cc, dims, 2, acc, dict(path="patch"))
        p = Run(pcase, d)
        pgot = p.got()
        pref, pb = D.bn_sums_ref(pgot["g_in"], d["y"], d["vec"], "patch")
        slack = 2 * D.bn_sums_propagated(exp["g_in"][1], d["y"], d["vec"], "onepass").sum(-1)
        check(id_, "bn-sums:onepass-vs-patch", D.exact_sum(got["bn_partials"]), D.exact_sum(pgot["bn_partials"]),
              exp["bn_partials"][1].sum(-1) + pb.sum(-1) + slack)
        check(id_, "dw:exact-fold", D.exact_sum(got["w_partials"]).view(Cc, 27), *onepass_dw(d, o))
    if o.get("nan"):
        n0, c0 = o["nan"][:2]
        gnan = torch.isnan(got["g_in"])
        assert 1 <= int(gnan.sum()) <= 27 and int(gnan[n0, c0].sum()) == int(gnan.sum()), "the NaN left its footprint"
        others = [c for c in range(Cc) if c != c0]
        assert not bool(torch.isnan(got["bn_partials"][:, others]).any())
        assert not bool(torch.isnan(got["w_partials"].view(Cc, 27, -1)[others]).any())
        assert bool(torch.isnan(got["bn_partials"][:, c0]).any()) and bool(torch.isnan(got["w_partials"].view(Cc, 27, -1)[c0]).any(-1).all())


def onepass_dw(d, o):
    ref, absdot = D.bww_ref(d["dy"], D.act32(d["y"], d["vec"][0], d["vec"][1]), 2)
    return ref, D.gamma(D.BWW_DEPTH["onepass"]) * absdot


@pytest.mark.parametrize("entry", ["onepass_data", "onepass", "onepass_bf16", "patch_bn", "patch_bf16"])
def test_dw_fused_refusals(entry):
    """W % 4 != 0 -> UNSUPPORTED; N = 0 -> ERR_ARG; g_in = NULL on the data entry -> ERR_ARG.  Every output stays untouched."""
    L = _lib.load()
    bf16 = entry.endswith("bf16")
    dt = torch.bfloat16 if bf16 else torch.float32
    x, w, vec = dev(torch.ones(4096).to(dt)), dev(torch.ones(64 * 27)), dev(torch.ones(4 * 64))
    v = [ptr(vec)] * 4
    for shape, g_null, want in (((1, 2, 5, 7, 6), False, ERR_UNSUPPORTED), ((0, 2, 4, 4, 4), False, ERR_ARG), ((1, 2, 4, 4, 4), True, ERR_ARG)):
        if g_null and entry != "onepass_data":
            continue
        outs = [Guarded(4096, dtype=dt), Guarded(2048, dtype=torch.float64), Guarded(4096, dtype=torch.float64), Guarded(27 * 64)]
        g, bn, wp, tt = (ptr(b.v) for b in outs)
        if entry == "onepass_data":
            rc = L.msl_dwconv_s2_bwd_data_bnreduce_bww(ptr(x), ptr(w), None if g_null else g, ptr(x), *v, bn, wp, *shape, 0, st())
        elif entry == "onepass":
            rc = L.msl_dwconv_s2_bwd_bnreduce_bww(ptr(x), ptr(w), ptr(x), *v, bn, wp, tt, *shape, st())
        elif entry == "onepass_bf16":
            rc = L.msl_dwconv_s2_bwd_bnreduce_bww_bf16(ptr(x), ptr(w), ptr(x), ptr(vec), bn, wp, tt, *shape, st())
        elif entry == "patch_bn":
            rc = L.msl_dwconv_bwd_data_bnreduce(ptr(x), ptr(w), g, ptr(x), *v, bn, *shape, 2, 0, st())
        else:
            rc = L.msl_dwconv_bwd_data_s2_patch_bf16(ptr(x), ptr(w), g, ptr(x), ptr(vec), bn, *shape, 0, st())
        torch.cuda.synchronize()
        assert rc == want, f"{entry}{shape}: returned {rc}, expected {want}"
        for b in outs:
            b.untouched(f"a refused {entry}")
    if entry == "onepass":
        assert L.msl_dwconv_s2_bwd_bnreduce_bww_num_partials(1, 2, 5, 7, 6) == -1
    if entry == "patch_bn":
        assert L.msl_dwconv_bwd_data_bnreduce_num_partials(1, 2, 5, 7, 6) == -1


# ------------------------------------------------------------------------------------------------- msl_dwconv_bwd_weight (+ _bf16)
@pytest.mark.parametrize("case", C.BWW_CASES, ids=C.ids(C.BWW_CASES))
def test_dw_bwd_weight(case):
    """The exact fold of the fp64 partials and, where asked for, dw; the deferred form's partials carry the immediate form's
    bits and msl_grad_reduce_batch (kind 1) folds them to within one rounding of their exact sum."""
    id_, entry, bf16, N, Cc, dims, stride, acc, o = case
    r, got, exp, d = run_and_check(case)
    if entry == "bww" and not o.get("dw"):
        red = grad_reduce_kind1(r.bufs["w_sum_partials"].v, r.NP, Cc * 27)
        s = got["dw_sum"]
        check(id_, "dw:grad-reduce-kind1", red.v.view(Cc, 27), s, D.U * s.abs() + exp["dw_sum"][1] * 2.0 ** -20)
        imm = Run((id_, entry, bf16, N, Cc, dims, stride, acc, dict(o, dw=True)), d)
        assert same_bits(imm.bufs["w_sum_partials"].v, r.bufs["w_sum_partials"].v), "deferred and immediate partials differ"


# ------------------------------------------------------------------------------------------------- msl_dwconv_bwd_weight_finalize
@pytest.mark.parametrize("NP", C.FINALIZE_NP)
def test_dw_bwd_weight_finalize(NP):
    """dw[i] = the sum of its NP fp64 partials, rounded once: U |sum| around the exact sum (math.fsum); both sides of the 8-way
    unrolled loop's start (NP = 449) and of its 64-lane tails."""
    L = _lib.load()
    Cc = 2
    g = C.gen(4000 + NP)
    parts = torch.randn((Cc * 27, NP), generator=g, dtype=torch.float64) * torch.logspace(-3, 3, NP, dtype=torch.float64) + 0.25
    outs = [Guarded(Cc * 27) for _ in range(2)]
    pd = dev(parts)
    for out in outs:
        assert L.msl_dwconv_bwd_weight_finalize(ptr(pd), NP, ptr(out.v), Cc, st()) == 0
    torch.cuda.synchronize()
    for out in outs:
        out.intact("dw")
    assert same_bits(outs[0].v, outs[1].v)
    s = D.exact_sum(parts)
    check(f"finalize:NP{NP}", "dw", outs[0].v, s, D.U * s.abs())
    assert same_bits(pd, parts.to("cuda")), "partials changed"


def test_dw_bwd_weight_finalize_refusals():
    L = _lib.load()
    pd, out = dev(torch.ones(54 * 4, dtype=torch.float64)), Guarded(54)
    for NP, Cc in ((0, 2), (-1, 2), (4, 0), (4, -3)):
        assert L.msl_dwconv_bwd_weight_finalize(ptr(pd), NP, ptr(out.v), Cc, st()) == ERR_ARG
        torch.cuda.synchronize()
        out.untouched("dw")
