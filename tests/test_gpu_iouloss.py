"""msl_multibox_loss_iou (csrc/multibox.hip) through the C ABI against tests/iouloss_ref.py (float64 torch) on the cases of
tests/iouloss_cases.py; tests/test_iouloss_ref_cpu.py proves the reference and what the cases promise.

Buffers, guard bands and pre-fills are those of tests/test_gpu_multibox.py (``Guarded``: NaN bytes in every float buffer the
call writes, guard bytes on both sides).  The tolerance is the project's rule, from the reference side alone
(``iouloss_ref.tolerance``): 8 x the deviation of fp32 torch from fp64 torch on the same case and kind, capped at 1e-4.  Each
comparison prints the kernel's measured deviation (pytest -s)."""
import functools

import pytest
import torch

from mslesions3d_amd import _lib
from mslesions3d_amd._lib import ptr
from tests import iouloss_cases as IC
from tests import iouloss_ref as IR
from tests import multibox_ref as R
from tests.test_gpu_multibox import _KEEP, ERR_ARG, ERR_UNSUPPORTED, Guarded, dev, fn, st

pytestmark = pytest.mark.gpu
KIND_IDS = list(IR.KINDS.items())


@pytest.fixture(autouse=True)
def _release_kept():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


@functools.lru_cache(maxsize=None)
def ref64(name, kind, flags):
    c = IC.case(name)
    return IR.losses_and_grads(c["locs"], c["scores"], c["true_classes"], c["true_locs"], c["priors"], kind, flags, c["ratio"],
                               *IC.UPSTREAM)


@functools.lru_cache(maxsize=None)
def bound(name, kind):
    c = IC.case(name)
    return IR.tolerance(c["locs"], c["scores"], c["true_classes"], c["true_locs"], c["priors"], kind, c["ncls"], c["ratio"],
                        *IC.UPSTREAM)


class Buffers:
    def __init__(self, c):
        L = _lib.load()
        self.c, self.N, self.P, self.ncls = c, c["N"], c["P"], c["ncls"]
        self.locs, self.scores = dev(c["locs"]), dev(c["scores"])
        self.tc, self.tl, self.pri = dev(c["true_classes"]), dev(c["true_locs"]), dev(c["priors"])
        self.up = dev(torch.tensor(IC.UPSTREAM, dtype=torch.float32))
        self.nws = L.msl_multibox_loss_workspace_bytes() // 8
        self.var_bytes = L.msl_multibox_loss_var_workspace_bytes(self.N, self.P)
        self.fresh()

    def fresh(self):
        N, P = self.N, self.P
        self.ws, self.loss = Guarded(self.nws, torch.float64), Guarded(3)
        self.dlocs, self.dscores = Guarded(N * P * 6), Guarded(N * P * self.ncls)
        self.var_ws = Guarded(self.var_bytes // 8, torch.float64)
        self.flag = Guarded(1, torch.int32)
        self.flag.v.zero_()
        return self

    def outputs(self):
        return self.ws, self.loss, self.dlocs, self.dscores, self.var_ws

    def mask(self):
        return self.var_ws.bytes[:self.N * self.P * 4].view(torch.float32).view(self.N, self.P)

    def args(self, kind, flags, grads=True, flag=True, **over):
        a = dict(locs=ptr(self.locs), scores=ptr(self.scores), tc=ptr(self.tc), tl=ptr(self.tl), pri=ptr(self.pri), ws=self.ws.p,
                 var_ws=self.var_ws.p, loss=self.loss.p, up=ptr(self.up), dlocs=self.dlocs.p if grads else None,
                 dscores=self.dscores.p if grads else None, flag=self.flag.p if flag else None, N=self.N, P=self.P,
                 ncls=self.ncls, flags=flags, ratio=self.c["ratio"], kind=kind)
        a.update(over)
        return list(a.values()) + [st()]

    def iou(self, kind, flags, grads=True, flag=True):
        _lib.call("msl_multibox_loss_iou", *self.args(kind, flags, grads, flag))

    def var(self, flags):
        _lib.call("msl_multibox_loss_var", ptr(self.locs), ptr(self.scores), ptr(self.tc), ptr(self.tl), self.ws.p, self.var_ws.p,
                  self.loss.p, ptr(self.up), self.dlocs.p, self.dscores.p, self.flag.p, self.N, self.P, self.ncls, flags,
                  self.c["ratio"], st())


def check(what, name, kind, flags, b, grads):
    """Every output of one call against the fp64 reference; -> loss_out on the host."""
    r, (tol, dev32), c = ref64(name, kind, flags), bound(name, kind), b.c
    torch.cuda.synchronize()
    b.loss.written(what)
    b.ws.written(what)
    b.var_ws.intact(what)
    b.flag.intact(what)
    assert int(b.flag.v) == 0, f"{what}: NaN flag {int(b.flag.v)} on clean input"
    got = b.loss.v.cpu()
    assert float(got[2]) == float(r["n_pos"]), f"{what}: loss_out[2] = {float(got[2])}, {r['n_pos']} positives"
    quantities = [("conf", got[0]), ("loc", got[1])]
    if grads:
        b.dlocs.written(what)
        b.dscores.written(what)
        dl, ds = b.dlocs.v.view(b.N, b.P, 6).cpu(), b.dscores.v.view(b.N, b.P, b.ncls).cpu()
        quantities += [("dlocs", dl), ("dscores", ds)]
        tc = c["true_classes"]
        assert float(dl[tc <= 0].abs().max() if (tc <= 0).any() else 0.0) == 0.0, f"{what}: box gradient off the positives"
        assert float(ds[tc < 0].abs().max() if (tc < 0).any() else 0.0) == 0.0, f"{what}: ignored priors have a score gradient"
    else:
        for o in (b.dlocs, b.dscores):
            o.untouched(f"{what} (forward only)")
    for k, g in quantities:
        d = R.deviation(g, r[k])
        print(f"{what} {k}: kernel deviation {d:.3e}, allowed {tol:.3e} (8 x fp32 torch {dev32:.3e}, cap 1e-4)")
        assert d <= tol, f"{what} {k}: deviation {d:.3e} from fp64 over {tol:.3e} (8 x fp32 torch {dev32:.3e}, cap 1e-4)"
    if flags & R.HNM:
        m = b.mask().cpu()
        assert bool(((m == 0) | (m == 1)).all()) and int(((m != 0) != r["mask"]).sum()) == 0, f"{what}: mined mask"
    return got


@pytest.mark.parametrize("kind,kid", KIND_IDS)
@pytest.mark.parametrize("name", IC.NAMES)
def test_iou_losses_against_fp64(name, kind, kid):
    """Every case x kind x confidence flag set, with gradients and forward-only (equal bits)."""
    c = IC.case(name)
    b = Buffers(c)
    for flags in IR.valid_flags(c["ncls"]):
        what = f"{name} {kind} flags {flags}"
        b.fresh().iou(kid, flags)
        both = check(what, name, kind, flags, b, True)
        b.fresh().iou(kid, flags, grads=False)
        only = check(what + " forward-only", name, kind, flags, b, False)
        assert torch.equal(only.view(torch.int32), both.view(torch.int32)), f"{what}: forward-only losses differ"


@pytest.mark.parametrize("kind,kid", KIND_IDS)
@pytest.mark.parametrize("name", IC.NAMES + [IC.NO_POSITIVE])
def test_confidence_side_has_the_bits_of_loss_var_and_runs_repeat(name, kind, kid):
    """loss_out[0], loss_out[2], dscores and the mined mask: bit-equal to msl_multibox_loss_var(flags & 5); a second call on
    the same inputs gives every output the same bits."""
    c = IC.case(name)
    a, a2, v = Buffers(c), Buffers(c), Buffers(c)
    for flags in IR.valid_flags(c["ncls"]):
        a.fresh().iou(kid, flags)
        a2.fresh().iou(kid, flags)
        v.fresh().var(flags & 5)
        torch.cuda.synchronize()
        what = f"{name} {kind} flags {flags}"
        i32 = lambda g: g.v.view(torch.int32)  # noqa: E731
        for o, o2 in zip((a.loss, a.dlocs, a.dscores, a.ws), (a2.loss, a2.dlocs, a2.dscores, a2.ws)):
            assert torch.equal(i32(o), i32(o2)), f"{what}: two runs differ"
        assert torch.equal(i32(a.loss)[[0, 2]], i32(v.loss)[[0, 2]]), f"{what}: conf / n_positives differ from loss_var"
        assert torch.equal(i32(a.dscores), i32(v.dscores)), f"{what}: dscores differ from loss_var"
        if flags & R.HNM:
            assert torch.equal(a.mask().view(torch.int32), v.mask().view(torch.int32)), f"{what}: mined mask differs from loss_var"
            assert torch.equal(a.mask().view(torch.int32), a2.mask().view(torch.int32))
        for o in a.outputs():
            o.intact(what)


@pytest.mark.parametrize("kind,kid", KIND_IDS)
def test_batch_without_a_positive_gives_nan_like_the_l1_path(kind, kid):
    """loc_loss = 0 / 0 = NaN (what MultiBoxLoss.forward turns into "Loss is NaN"), n_positives 0, dlocs exactly 0."""
    c = IC.case(IC.NO_POSITIVE)
    b, v = Buffers(c), Buffers(c)
    for flags in IR.valid_flags(c["ncls"]):
        b.fresh().iou(kid, flags)
        v.fresh().var(flags)
        torch.cuda.synchronize()
        got, l1 = b.loss.v.cpu(), v.loss.v.cpu()
        assert torch.isnan(l1[1]), "the L1 path gives NaN without a positive"
        assert torch.isnan(got[1]) and float(got[2]) == 0.0
        r = ref64(IC.NO_POSITIVE, kind, flags)
        assert torch.isnan(r["loc"]) and r["n_pos"] == 0
        b.dlocs.written("dlocs")
        assert float(b.dlocs.v.abs().max()) == 0.0


@pytest.mark.parametrize("kind,kid", KIND_IDS)
def test_identical_boxes(kind, kid):
    """locs == true_locs bit for bit: loc_loss within the case's bound of 0, finite gradients.  (The reference's loc_loss is
    0 up to fp64 rounding, so fp32 torch's RELATIVE deviation from it is huge and the rule's cap, 1e-4, is the bound.)"""
    c = IC.case(IC.IDENTICAL)
    tol, dev32 = bound(IC.IDENTICAL, kind)
    b = Buffers(c)
    b.iou(kid, 0)
    torch.cuda.synchronize()
    got = b.loss.v.cpu()
    print(f"identical boxes {kind}: loc_loss {float(got[1]):.3e}, allowed {tol:.3e} (8 x fp32 torch {dev32:.3e}, cap 1e-4)")
    assert abs(float(got[1])) <= tol
    b.dlocs.written("dlocs")
    b.dscores.written("dscores")
    assert bool(torch.isfinite(b.dlocs.v).all()) and bool(torch.isfinite(b.dscores.v).all())


NAN_CASE = "N3_P7001_C3"  # N*P = 21003: indices >= 16384 are read by the second grid-stride trip only


def test_nan_flag():
    c = IC.case(NAN_CASE)
    total = c["N"] * c["P"]
    assert total > 16384 + 256
    for where in (0, total - 1, 16384 + 77):
        for in_loc, in_score, want in ((True, False, 1), (False, True, 2), (True, True, 3)):
            locs, scores = c["locs"].clone(), c["scores"].clone()
            if in_loc:
                locs.view(-1, 6)[where, where % 6] = float("nan")
            if in_score:
                scores.view(-1, c["ncls"])[where, where % c["ncls"]] = float("nan")
            b = Buffers(dict(c, locs=locs, scores=scores))
            b.iou(2, 1)
            torch.cuda.synchronize()
            b.flag.intact("nan flag")
            assert int(b.flag.v) == want, f"NaN at prior {where} (loc {in_loc}, score {in_score}) -> flag {int(b.flag.v)}"
    b = Buffers(c)
    b.iou(2, 1)
    torch.cuda.synchronize()
    assert int(b.flag.v) == 0
    clean = b.loss.v.clone()
    b.fresh().iou(2, 1, flag=False)  # a null flag pointer is accepted and changes nothing else
    torch.cuda.synchronize()
    assert torch.equal(b.loss.v.view(torch.int32), clean.view(torch.int32)) and int(b.flag.v) == 0


def test_bad_arguments_are_refused():
    b3, b2 = Buffers(IC.case("N1_P255_C3")), Buffers(IC.case("N1_P255_C2"))
    call = lambda b, kind, flags, **over: fn("msl_multibox_loss_iou")(*b.args(kind, flags, **over))  # noqa: E731
    for kind in (0, 4, -1, 7):
        assert call(b3, kind, 0) == ERR_ARG, f"kind {kind}"
    for flags in (2, 3, 6, 7, 8, -1):
        assert call(b3, 1, flags) == ERR_ARG, f"flags {flags} (three classes)"
        assert call(b2, 1, flags) == ERR_ARG, f"flags {flags} (two classes)"
    for flags in (4, 5):
        assert call(b3, 2, flags) == ERR_UNSUPPORTED, "focal with three classes"
    for over in (dict(ncls=1), dict(ncls=17), dict(N=0), dict(P=0), dict(ratio=-1), dict(dlocs=None), dict(dscores=None),
                 dict(up=None), dict(var_ws=None), dict(pri=None)):
        assert call(b3, 3, 1, **over) == ERR_ARG, over
    torch.cuda.synchronize()
    for b in (b3, b2):
        for o in b.outputs():
            o.untouched("a refused call")
        assert int(b.flag.v) == 0
    assert call(b3, 3, 1, up=None, dlocs=None, dscores=None) == 0, "forward only needs no upstream factors"
    assert call(b2, 3, 5) == 0, "focal with two classes is accepted"
    torch.cuda.synchronize()
