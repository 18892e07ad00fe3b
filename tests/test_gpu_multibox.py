"""Every matching and MultiBox-loss entry point of csrc/multibox.hip, called through the C ABI, against tests/multibox_ref.py
(loss: float64 torch from given targets) and oracle.multibox.match_batch (matching), on the cases of tests/multibox_cases.py.
tests/test_multibox_ref_cpu.py proves the reference and what the cases promise (real ties, IoUs on a threshold, mining cuts
that do not depend on rounding).

Every output and scratch buffer lies between two guard bands and is pre-filled with a pattern no result can have (all-ones
bytes = NaN for floats, 0x5A bytes for integers): after a call the bands must be intact and everything the entry is documented
to write must have been written.

The loss tolerance is computed from the reference side alone (``multibox_ref.tolerance``): 8 x the deviation of fp32 torch
from fp64 torch on the same case, capped at 1e-4.  Each comparison prints the kernel's measured deviation (pytest -s)."""
import ctypes
import functools

import pytest
import torch

from mslesions3d_amd import _lib
from mslesions3d_amd._lib import ptr
from oracle import multibox as OMB
from tests import multibox_cases as C
from tests import multibox_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = 256  # guard bytes on each side of every buffer (the body stays 256-byte aligned)
GUARD_BYTE, NAN_BYTE, INT_BYTE = 0xA5, 0xFF, 0x5A
ERR_ARG, ERR_UNSUPPORTED = -1, -2
SENT = 12345.0  # pre-fill of the head-gradient images: halo and padding rows must keep it


def st():
    return torch.cuda.current_stream().cuda_stream


def fn(name):
    return getattr(_lib.load(), name)


_KEEP = []


def dev(t):
    d = t.detach().to(DEV).contiguous()
    _KEEP.append(d)
    return d


@pytest.fixture(autouse=True)
def _release_kept():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


class Guarded:
    """``n`` elements of ``dtype`` pre-filled with ``fill`` bytes, between two bands of guard bytes, in one allocation."""

    def __init__(self, n, dtype=torch.float32, fill=None):
        self.nbytes = n * torch.empty((), dtype=dtype).element_size()
        self.fill = fill if fill is not None else (NAN_BYTE if dtype.is_floating_point else INT_BYTE)
        self.full = torch.full((self.nbytes + 2 * G,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
        self.bytes = self.full[G:G + self.nbytes]
        self.bytes.fill_(self.fill)
        self.v = self.bytes.view(dtype)
        _KEEP.append(self.full)

    @property
    def p(self):
        return self.v.data_ptr()

    def intact(self, what):
        bands = torch.cat([self.full[:G], self.full[G + self.nbytes:]])
        assert bool((bands == GUARD_BYTE).all()), f"{what}: wrote outside its buffer"

    def written(self, what, view=None):
        """Guards intact and no element of ``view`` (default: the whole body) still holds the pre-fill."""
        self.intact(what)
        v = self.v if view is None else view
        left = v.contiguous().view(torch.uint8).view(v.numel(), -1)
        n = int((left == self.fill).all(dim=1).sum())
        assert n == 0, f"{what}: {n} of {v.numel()} elements were never written"

    def untouched(self, what):
        self.intact(what)
        assert bool((self.bytes == self.fill).all()), f"{what}: a refused call wrote to its output"


# ------------------------------------------------------------------------------------------------------- matching
@functools.lru_cache(maxsize=None)
def oracle_match(name):
    """-> (true_classes, true_locs, matched, overlap [(P,) per image with objects or None]) of the CPU oracle, computed once."""
    c = C.matching_case(name)
    tc, tl, matched = OMB.match_batch(c["boxes"], c["labels"], c["priors"], c["threshold"])
    ov = [OMB.match_image(b, l, c["priors"], c["threshold"])[2] if b.shape[0] else None
          for b, l in zip(c["boxes"], c["labels"])]
    return tc, tl, matched, ov


def pack_gt(boxes, labels):
    sizes = [int(b.shape[0]) for b in boxes]
    off = torch.tensor([0] + sizes, dtype=torch.int32).cumsum(0).to(torch.int32)
    T = int(off[-1])
    gb = torch.cat(boxes).float() if T else torch.zeros((1, 6))
    gl = torch.cat(labels).long() if T else torch.zeros(1, dtype=torch.long)
    return dev(gb), dev(gl), dev(off), T


class MatchRun:
    """One call of msl_multibox_match (npos None) or msl_multibox_match_count into fresh guarded buffers."""

    def __init__(self, c, npos=None, call=True):
        self.c, self.N, self.P = c, len(c["boxes"]), c["priors"].shape[0]
        N, P = self.N, self.P
        self.gb, self.gl, self.off, self.T = pack_gt(c["boxes"], c["labels"])
        self.pri = dev(c["priors"])
        self.overlap, self.obj = Guarded(N * P), Guarded(N * P, torch.int32)
        self.pfo = Guarded(max(self.T, 1), torch.int32)
        self.tc, self.tl, self.matched = Guarded(N * P, torch.int64), Guarded(N * P * 6), Guarded(N * P, torch.int64)
        lo, hi, soft = C.thresholds(c["threshold"])
        self.args = [ptr(self.gb), ptr(self.gl), ptr(self.off), self.T, ptr(self.pri), N, P, lo, hi, soft, self.overlap.p,
                     self.obj.p, self.pfo.p, self.tc.p, self.tl.p, self.matched.p]
        self.name = "msl_multibox_match" if npos is None else "msl_multibox_match_count"
        if npos is not None:
            self.args.append(ptr(npos))
        if call:
            _lib.call(self.name, *self.args, st())
            torch.cuda.synchronize()

    def outputs(self):
        return self.overlap, self.obj, self.pfo, self.tc, self.tl, self.matched

    def check(self, name):
        c, N, P = self.c, self.N, self.P
        tc, tl, matched, ov = oracle_match(name)
        what = f"{self.name} {name}"
        for b in (self.tc, self.tl, self.matched):
            b.written(what)
        if self.T > 0:  # the scratch of a batch without any object is not used
            self.overlap.written(what)
            self.obj.written(what)
            self.pfo.written(what, self.pfo.v[:self.T])
        else:
            for b in (self.overlap, self.obj, self.pfo):
                b.untouched(what)
        got_tc, got_m = self.tc.v.view(N, P).cpu(), self.matched.v.view(N, P).cpu()
        assert torch.equal(got_tc, tc), f"{what}: {int((got_tc != tc).sum())} true_classes differ from the oracle"
        assert torch.equal(got_m, matched), f"{what}: {int((got_m != matched).sum())} matched objects differ from the oracle"
        got_tl = self.tl.v.view(N, P, 6).cpu()
        torch.testing.assert_close(got_tl, tl, rtol=2e-6, atol=2e-6, msg=lambda m: f"{what} true_locs: {m}")
        obj, overlap = self.obj.v.view(N, P).cpu(), self.overlap.v.view(N, P).cpu()
        for n in range(N):
            if c["boxes"][n].shape[0] == 0:
                assert float(got_tl[n].abs().max()) == 0.0, f"{what}: true_locs of image {n} without objects"
            elif self.T > 0:
                assert torch.equal(obj[n].long(), matched[n]), f"{what}: obj scratch of image {n} after the force-match"
                assert torch.equal(overlap[n].view(torch.int32), ov[n].view(torch.int32)), f"{what}: overlap of image {n}"
        return int((tc > 0).sum())


@pytest.mark.parametrize("name", C.MATCH_NAMES)
def test_matching_equals_the_oracle_bit_for_bit(name):
    c = C.matching_case(name)
    MatchRun(c).check(name)
    npos = Guarded(1, torch.int32)
    npos.v.fill_(-123456789)  # garbage: the call has to reset it, also when the batch has no object at all
    want = MatchRun(c, npos.v).check(name)
    npos.intact("npos")
    assert int(npos.v) == want, f"msl_multibox_match_count {name}: counted {int(npos.v)} positives, the oracle has {want}"


def test_positives_counter_is_reset_by_every_call():
    """Three batches into one counter, one after the other: with objects, without any (the reset is then the encode
    kernel's), with objects again."""
    npos = Guarded(1, torch.int32)
    npos.v.fill_(77)
    for name in ("P1025_special_many300_one_soft", "P1024_all_empty_hardH", "P4097_special_dozen_none_hardQ", "P9223_empty_soft",
                 "P255_many300_soft"):
        want = int((oracle_match(name)[0] > 0).sum())
        MatchRun(C.matching_case(name), npos.v)
        assert int(npos.v) == want, name
    npos.intact("npos")
    assert int((oracle_match("P1024_all_empty_hardH")[0] > 0).sum()) == 0


def test_match_count_refuses_a_null_counter():
    r = MatchRun(C.matching_case("P255_special_none_dozen_soft"), npos=None, call=False)
    assert fn("msl_multibox_match_count")(*r.args, None, st()) == ERR_ARG
    torch.cuda.synchronize()
    for b in r.outputs():
        b.untouched("msl_multibox_match_count without a counter")


# ----------------------------------------------------------------------------------------------------------- loss
def _case(name):
    return C.mining_case(name) if name in C.MINING_NAMES else C.loss_case(name)


@functools.lru_cache(maxsize=None)
def ref64(name, flags):
    c = _case(name)
    return R.losses_and_grads(c["locs"], c["scores"], c["true_classes"], c["true_locs"], flags, c["ratio"], *C.UPSTREAM)


@functools.lru_cache(maxsize=None)
def bound(name):
    c = _case(name)
    return R.tolerance(c["locs"], c["scores"], c["true_classes"], c["true_locs"], c["ncls"], c["ratio"], *C.UPSTREAM)


class LossBuffers:
    def __init__(self, c):
        N, P, ncls = c["N"], c["P"], c["ncls"]
        L = _lib.load()
        self.N, self.P, self.ncls, self.c = N, P, ncls, c
        self.locs, self.scores = dev(c["locs"]), dev(c["scores"])
        self.tc, self.tl = dev(c["true_classes"]), dev(c["true_locs"])
        self.up = dev(torch.tensor(C.UPSTREAM, dtype=torch.float32))
        self.nws = L.msl_multibox_loss_workspace_bytes() // 8
        self.var_bytes = L.msl_multibox_loss_var_workspace_bytes(N, P)
        assert self.var_bytes == ((N * P * 4 + 15) & ~15) + N * 8
        self.fresh()

    def fresh(self):
        N, P = self.N, self.P
        self.ws, self.loss = Guarded(self.nws, torch.float64), Guarded(3)
        self.dlocs, self.dscores = Guarded(N * P * 6), Guarded(N * P * self.ncls)
        self.var_ws = Guarded(self.var_bytes // 8, torch.float64)
        self.flag = Guarded(1, torch.int32)
        self.flag.v.zero_()
        return self

    def inputs(self):
        return [ptr(self.locs), ptr(self.scores), ptr(self.tc), ptr(self.tl)]

    def dims(self):
        return [self.N, self.P, self.ncls]

    def outputs(self):
        return self.ws, self.loss, self.dlocs, self.dscores, self.var_ws

    def mask(self):
        return self.var_ws.bytes[:self.N * self.P * 4].view(torch.float32).view(self.N, self.P)

    def sums(self):
        return self.var_ws.bytes[(self.N * self.P * 4 + 15) & ~15:].view(torch.float64)

    # the entry points
    def fwd(self):
        _lib.call("msl_multibox_loss_fwd", *self.inputs(), self.ws.p, self.loss.p, *self.dims(), st())

    def bwd(self, loss_out):
        _lib.call("msl_multibox_loss_bwd", *self.inputs(), ptr(loss_out), ptr(self.up), self.dlocs.p, self.dscores.p,
                  *self.dims(), st())

    def fwd_bwd(self, flag=True):
        _lib.call("msl_multibox_loss_fwd_bwd", *self.inputs(), self.ws.p, self.loss.p, ptr(self.up), self.dlocs.p,
                  self.dscores.p, self.flag.p if flag else None, *self.dims(), st())

    def var(self, flags, grads=True, flag=True):
        _lib.call("msl_multibox_loss_var", *self.inputs(), self.ws.p, self.var_ws.p, self.loss.p, ptr(self.up),
                  self.dlocs.p if grads else None, self.dscores.p if grads else None, self.flag.p if flag else None,
                  *self.dims(), flags, self.c["ratio"], st())


def check_losses(what, name, b, flags):
    """loss_out against the fp64 reference; returns the measured deviations."""
    r, (tol, dev32) = ref64(name, flags), bound(name)
    torch.cuda.synchronize()
    b.loss.written(what)
    b.ws.written(what)
    got = b.loss.v.cpu()
    assert float(got[2]) == float(r["n_pos"]), f"{what}: loss_out[2] = {float(got[2])}, {r['n_pos']} positives"
    devs = dict(conf=R.deviation(got[0], r["conf"]), loc=R.deviation(got[1], r["loc"]))
    for k, d in devs.items():
        print(f"{what} {k}: kernel deviation {d:.3e}, allowed {tol:.3e} (8 x fp32 torch {dev32:.3e}, cap 1e-4)")
        assert d <= tol, f"{what} {k}: deviation {d:.3e} from fp64 over {tol:.3e} (8 x fp32 torch {dev32:.3e}, cap 1e-4)"
    return got


def check_grads(what, name, b, flags):
    r, (tol, dev32), c = ref64(name, flags), bound(name), b.c
    torch.cuda.synchronize()
    b.dlocs.written(what)
    b.dscores.written(what)
    dl, ds = b.dlocs.v.view(b.N, b.P, 6).cpu(), b.dscores.v.view(b.N, b.P, b.ncls).cpu()
    for k, got in (("dlocs", dl), ("dscores", ds)):
        d = R.deviation(got, r[k])
        print(f"{what} {k}: kernel deviation {d:.3e}, allowed {tol:.3e} (8 x fp32 torch {dev32:.3e}, cap 1e-4)")
        assert d <= tol, f"{what} {k}: deviation {d:.3e} from fp64 over {tol:.3e} (8 x fp32 torch {dev32:.3e}, cap 1e-4)"
        zero = r[k] == 0
        assert float(got[zero].abs().max() if zero.any() else 0.0) == 0.0, f"{what} {k}: non-zero where the gradient is exactly 0"
    tc = c["true_classes"]
    assert float(ds[tc < 0].abs().max() if (tc < 0).any() else 0.0) == 0.0, f"{what}: ignored priors have a score gradient"
    assert float(dl[tc <= 0].abs().max() if (tc <= 0).any() else 0.0) == 0.0, f"{what}: non-positive priors have a box gradient"
    if not flags & R.SMOOTH:  # L1: +-(u_loc / (n_pos * 6)) evaluated in fp32, or 0 at a zero residual
        gl = torch.tensor(C.UPSTREAM[1], dtype=torch.float32) / (torch.tensor(float(r["n_pos"]), dtype=torch.float32) * 6.0)
        want = torch.sign(c["locs"] - c["true_locs"]) * gl * (tc > 0)[..., None]
        assert torch.equal(dl, want), f"{what}: {int((dl != want).sum())} L1 gradients are not exactly +-{float(gl)} or 0"
    if flags & R.HNM:
        b.var_ws.intact(what)
        got = b.mask().cpu()
        assert bool(((got == 0) | (got == 1)).all()), f"{what}: the mined mask holds something else than 0 and 1"
        diff = int(((got != 0) != r["mask"]).sum())
        assert diff == 0, f"{what}: the mined mask differs from the reference at {diff} priors"
        assert not bool(torch.isnan(b.sums().cpu()).any()), f"{what}: a per-image mined sum was not written"


@pytest.mark.parametrize("name", C.LOSS_NAMES)
def test_live_loss_entries_against_fp64(name):
    """msl_multibox_loss_fwd, _bwd (reading _fwd's loss_out) and _fwd_bwd."""
    b = LossBuffers(C.loss_case(name))
    b.fwd()
    fwd = check_losses(f"{name} loss_fwd", name, b, 0)
    for o in (b.dlocs, b.dscores):
        o.untouched("loss_fwd")
    loss_of_fwd = b.loss.v.clone()
    _KEEP.append(loss_of_fwd)
    b.bwd(loss_of_fwd)
    check_grads(f"{name} loss_bwd", name, b, 0)
    b.fresh().fwd_bwd()
    both = check_losses(f"{name} loss_fwd_bwd", name, b, 0)
    check_grads(f"{name} loss_fwd_bwd", name, b, 0)
    b.flag.intact("nan flag")
    assert int(b.flag.v) == 0
    assert float(both[2]) == float(fwd[2])


@pytest.mark.parametrize("name", C.LOSS_NAMES)
def test_loss_variants_against_fp64(name):
    """msl_multibox_loss_var with every flag set it accepts, with gradients; flags 0, 1, 4, 7 also forward-only."""
    c = C.loss_case(name)
    b = LossBuffers(c)
    for flags in R.valid_flags(c["ncls"]):
        b.fresh().var(flags)
        got = check_losses(f"{name} loss_var flags {flags}", name, b, flags)
        check_grads(f"{name} loss_var flags {flags}", name, b, flags)
        assert int(b.flag.v) == 0
        if flags in (0, 1, 4, 7):
            b.fresh().var(flags, grads=False)
            only = check_losses(f"{name} loss_var flags {flags} forward-only", name, b, flags)
            for o in (b.dlocs, b.dscores):
                o.untouched("forward-only loss_var")
            assert torch.equal(only.view(torch.int32), got.view(torch.int32)), "forward-only losses differ from the call with gradients"


@pytest.mark.parametrize("name", C.MINING_NAMES)
def test_hard_negative_mining_keeps_exactly_the_reference_set(name):
    c = C.mining_case(name)
    b = LossBuffers(c)
    for flags in (1, 5, 7):
        b.fresh().var(flags)
        check_losses(f"{name} loss_var flags {flags}", name, b, flags)
        check_grads(f"{name} loss_var flags {flags}", name, b, flags)
        b.fresh().var(flags, grads=False)
        check_losses(f"{name} loss_var flags {flags} forward-only", name, b, flags)
        diff = int(((b.mask().cpu() != 0) != ref64(name, flags)["mask"]).sum())
        assert diff == 0, f"{name} flags {flags} forward-only: mask differs at {diff} priors"


def test_loss_entries_refuse_bad_arguments():
    c3, c2 = C.loss_case("N1_P255_C3"), C.loss_case("N1_P255_C2")
    b = LossBuffers(c3)
    i, up = b.inputs(), ptr(b.up)
    N, P = b.N, b.P
    for ncls in (1, 17):
        assert fn("msl_multibox_loss_fwd")(*i, b.ws.p, b.loss.p, N, P, ncls, st()) == ERR_ARG
        assert fn("msl_multibox_loss_bwd")(*i, b.loss.p, up, b.dlocs.p, b.dscores.p, N, P, ncls, st()) == ERR_ARG
        assert fn("msl_multibox_loss_fwd_bwd")(*i, b.ws.p, b.loss.p, up, b.dlocs.p, b.dscores.p, b.flag.p, N, P, ncls, st()) == ERR_ARG
        assert fn("msl_multibox_loss_var")(*i, b.ws.p, b.var_ws.p, b.loss.p, up, b.dlocs.p, b.dscores.p, b.flag.p, N, P, ncls, 0, 3,
                                           st()) == ERR_ARG
    var = lambda dl, ds, flags, ratio: fn("msl_multibox_loss_var")(  # noqa: E731
        *i, b.ws.p, b.var_ws.p, b.loss.p, up, dl, ds, b.flag.p, N, P, 3, flags, ratio, st())
    assert var(b.dlocs.p, b.dscores.p, 4, 3) == ERR_UNSUPPORTED, "focal with three classes"
    assert var(b.dlocs.p, b.dscores.p, 5, 3) == ERR_UNSUPPORTED
    assert var(b.dlocs.p, b.dscores.p, 8, 3) == ERR_ARG
    assert var(b.dlocs.p, b.dscores.p, -1, 3) == ERR_ARG
    assert var(b.dlocs.p, None, 0, 3) == ERR_ARG, "one null gradient pointer"
    assert var(None, b.dscores.p, 0, 3) == ERR_ARG
    assert var(b.dlocs.p, b.dscores.p, 1, -1) == ERR_ARG, "a negative ratio"
    assert fn("msl_multibox_loss_var")(*i, b.ws.p, None, b.loss.p, up, b.dlocs.p, b.dscores.p, b.flag.p, N, P, 3, 0, 3, st()) == ERR_ARG
    assert fn("msl_multibox_loss_var")(*i, b.ws.p, b.var_ws.p, b.loss.p, None, b.dlocs.p, b.dscores.p, b.flag.p, N, P, 3, 0, 3,
                                       st()) == ERR_ARG, "gradients without upstream factors"
    torch.cuda.synchronize()
    for o in b.outputs():
        o.untouched("a refused loss call")
    assert int(b.flag.v) == 0
    b2 = LossBuffers(c2)  # focal with two classes is accepted
    b2.var(4)
    check_losses("N1_P255_C2 loss_var flags 4", "N1_P255_C2", b2, 4)


# ----------------------------------------------------------------------------------------------------------- pack
class PackRun:
    """msl_multibox_match_count + msl_multibox_loss_pack + a kind-4 msl_grad_reduce_batch on one pack case."""

    def __init__(self, c, locs=None, scores=None, flag=True):
        self.c = c
        N, P, ncls, dims = c["N"], c["P"], c["ncls"], c["dims"]
        L = _lib.load()
        self.npos = Guarded(1, torch.int32)
        self.npos.v.fill_(-5)
        self.m = MatchRun(c, self.npos.v)
        self.locs, self.scores = dev(c["locs"] if locs is None else locs), dev(c["scores"] if scores is None else scores)
        self.up = dev(torch.tensor(C.UPSTREAM, dtype=torch.float32))
        self.nparts = L.msl_multibox_loss_pack_num_partials(N, P)
        assert self.nparts == -(-N * P // 256)
        self.parts, self.loss = Guarded(2 * self.nparts, torch.float64), Guarded(3)
        self.flag = Guarded(1, torch.int32)
        self.flag.v.zero_()
        CO = R.head_co(ncls)
        self.imgs = []
        for d in dims:
            g = Guarded(N * CO * (d[0] + 2) * (d[1] + 2) * (d[2] + 2))
            g.v.fill_(SENT)
            self.imgs.append(g)
        n = len(dims)
        I = ctypes.c_int * n
        self.host = [(ctypes.c_void_p * n)(*[g.p for g in self.imgs])] + [I(*[d[a] for d in dims]) for a in range(3)] + [
            I(*c["prior_off"])]
        self.flag_ptr = self.flag.p if flag else None

    def pack_args(self, n=None, ncls=None):
        c = self.c
        return [ptr(self.locs), ptr(self.scores), self.m.tc.p, self.m.tl.p, self.npos.p, ptr(self.up), self.parts.p, self.flag_ptr,
                *[ctypes.addressof(x) for x in self.host], len(c["dims"]) if n is None else n, c["N"], c["P"],
                c["ncls"] if ncls is None else ncls, st()]

    def run(self, reduce=True):
        L = _lib.load()
        _lib.call("msl_multibox_loss_pack", *self.pack_args())
        if reduce:
            host = (ctypes.c_ubyte * L.msl_grad_reduce_entry_bytes())()
            assert L.msl_grad_reduce_table_set(ctypes.addressof(host), 0, 0, 4, self.parts.p, self.loss.p, self.npos.p, self.nparts, 1,
                                               0, 0, 0, 0) == 1
            table = dev(torch.frombuffer(bytearray(host), dtype=torch.uint8))
            _lib.call("msl_grad_reduce_batch", ptr(table), 1, 1, st())
        torch.cuda.synchronize()
        return self


@pytest.mark.parametrize("name", C.PACK_NAMES)
def test_loss_pack_against_fp64_and_the_documented_layout(name):
    c = C.pack_case(name)
    N, P, ncls = c["N"], c["P"], c["ncls"]
    p = PackRun(c).run()
    # the reference takes the targets the matcher left (they are checked against the oracle here and, at length, above)
    tc, tl = p.m.tc.v.view(N, P).cpu(), p.m.tl.v.view(N, P, 6).cpu()
    otc, otl, _ = OMB.match_batch(c["boxes"], c["labels"], c["priors"], c["threshold"])
    assert torch.equal(tc, otc), "targets of the matcher"
    torch.testing.assert_close(tl, otl, rtol=2e-6, atol=2e-6)
    r = R.losses_and_grads(c["locs"], c["scores"], tc, tl, 0, 3, *C.UPSTREAM)
    tol, dev32 = R.tolerance(c["locs"], c["scores"], tc, tl, ncls, 3, *C.UPSTREAM, flag_sets=[0])
    want_imgs = R.head_grad_images(r["dlocs"], r["dscores"], c["dims"], c["prior_off"], ncls, fill=SENT)
    assert int(p.npos.v) == r["n_pos"]
    p.parts.written(f"{name} pack partials")
    p.loss.written(f"{name} pack loss_out")
    got = p.loss.v.cpu()
    assert float(got[2]) == float(r["n_pos"])
    for k, i in (("conf", 0), ("loc", 1)):
        d = R.deviation(got[i], r[k])
        print(f"{name} loss_pack {k}: kernel deviation {d:.3e}, allowed {tol:.3e} (8 x fp32 torch {dev32:.3e}, cap 1e-4)")
        assert d <= tol, f"{name} loss_pack {k}: deviation {d:.3e} over {tol:.3e} (8 x fp32 torch {dev32:.3e}, cap 1e-4)"
    gl = torch.tensor(C.UPSTREAM[1], dtype=torch.float32) / (torch.tensor(float(r["n_pos"]), dtype=torch.float32) * 6.0)
    scale = {"loc": float(r["dlocs"].abs().max()), "cls": float(r["dscores"].abs().max())}
    for s, (g, want, d) in enumerate(zip(p.imgs, want_imgs, c["dims"])):
        what = f"{name} head-gradient image of scale {s} {d}"
        g.intact(what)
        img = g.v.view(want.shape).cpu()
        outside = want == SENT  # halo cells and rows >= 12 + 2*ncls
        assert torch.equal(img[outside], want[outside].float()), f"{what}: halo or padding rows were written"
        assert not bool((img[~outside] == SENT).any()), f"{what}: an interior cell was not written"
        for k, rows in (("loc", slice(0, 12)), ("cls", slice(12, 12 + 2 * ncls))):
            a, w = img[:, rows, 1:-1, 1:-1, 1:-1].double(), want[:, rows, 1:-1, 1:-1, 1:-1]
            dv = float((a - w).abs().max()) / scale[k]
            print(f"{what} {k} rows: kernel deviation {dv:.3e}, allowed {tol:.3e}")
            assert dv <= tol, f"{what} {k} rows: deviation {dv:.3e} over {tol:.3e} (8 x fp32 torch {dev32:.3e}, cap 1e-4)"
            assert float(a[w == 0].abs().max() if (w == 0).any() else 0.0) == 0.0, f"{what} {k} rows: non-zero where the gradient is 0"
        a, w = img[:, :12, 1:-1, 1:-1, 1:-1], want[:, :12, 1:-1, 1:-1, 1:-1]
        assert torch.equal(a, (torch.sign(w) * gl).float()), f"{what}: box gradients are not exactly 0 or +-{float(gl)}"
    assert int(p.flag.v) == 0


def test_loss_pack_refuses_bad_scale_and_class_counts():
    p = PackRun(C.pack_case("two_scales"))
    pack = fn("msl_multibox_loss_pack")
    for n in (0, 5):
        assert pack(*p.pack_args(n=n)) == ERR_ARG, f"{n} scales"
    for ncls in (1, 17):
        assert pack(*p.pack_args(ncls=ncls)) == ERR_ARG, f"{ncls} classes"
    torch.cuda.synchronize()
    p.parts.untouched("a refused pack call")
    for g in p.imgs:
        g.intact("a refused pack call")
        assert bool((g.v == SENT).all())


# ----------------------------------------------------------------------------------------------------- NaN guards
NAN_CASE = "N3_P7001_C3"  # N*P = 21003: indices >= 16384 are read by the second grid-stride trip only
NAN_SPOTS = ((True, False, 1), (False, True, 2), (True, True, 3))


def _poisoned(c, where, in_loc, in_score):
    """-> (locs, scores) with one NaN at prior index ``where`` of the flattened batch."""
    locs, scores = c["locs"].clone(), c["scores"].clone()
    if in_loc:
        locs.view(-1, 6)[where, where % 6] = float("nan")
    if in_score:
        scores.view(-1, c["ncls"])[where, where % c["ncls"]] = float("nan")
    return locs, scores


@pytest.mark.parametrize("entry", ["fwd_bwd", "var0", "var3"])
def test_nan_guard_of_the_loss_entries(entry):
    c = C.loss_case(NAN_CASE)
    total = c["N"] * c["P"]
    assert total > 16384 + 256
    run = {"fwd_bwd": lambda b, f: b.fwd_bwd(flag=f), "var0": lambda b, f: b.var(0, flag=f),
           "var3": lambda b, f: b.var(3, flag=f)}[entry]
    for where in (0, total - 1, 16384 + 77):
        for in_loc, in_score, want in NAN_SPOTS:
            locs, scores = _poisoned(c, where, in_loc, in_score)
            b = LossBuffers(dict(c, locs=locs, scores=scores))
            run(b, True)
            torch.cuda.synchronize()
            b.flag.intact("nan flag")
            assert int(b.flag.v) == want, f"{entry}: NaN at prior {where} (loc {in_loc}, score {in_score}) -> flag {int(b.flag.v)}"
    b = LossBuffers(c)
    run(b, True)
    torch.cuda.synchronize()
    assert int(b.flag.v) == 0, "clean input"
    clean = b.loss.v.clone()
    b.fresh()
    run(b, False)  # a null flag pointer is accepted and changes nothing else
    torch.cuda.synchronize()
    assert torch.equal(b.loss.v.view(torch.int32), clean.view(torch.int32)) and int(b.flag.v) == 0


def test_nan_guard_of_the_pack_entry():
    c = C.pack_case("two_large")
    total = c["N"] * c["P"]
    assert total > 16384 + 256
    for where in (0, total - 1, 16384 + 77):
        for in_loc, in_score, want in NAN_SPOTS:
            locs, scores = _poisoned(c, where, in_loc, in_score)
            p = PackRun(c, locs, scores).run(reduce=False)
            p.flag.intact("nan flag")
            assert int(p.flag.v) == want, f"pack: NaN at prior {where} (loc {in_loc}, score {in_score}) -> flag {int(p.flag.v)}"
    p = PackRun(c).run(reduce=False)
    assert int(p.flag.v) == 0, "clean input"
    q = PackRun(c, flag=False).run(reduce=False)
    assert int(q.flag.v) == 0
    assert torch.equal(q.parts.v.view(torch.int64), p.parts.v.view(torch.int64))
    for a, b in zip(p.imgs, q.imgs):
        assert torch.equal(a.v.view(torch.int32), b.v.view(torch.int32))
