"""Every instantiation of the per-channel backward link (csrc/chanlink.hip): 13 configurations x fp32 / bf16 storage x with /
without the depthwise weight gradient, against the two-stage float64 reference of tests/chanlink_ref.py (bounds derived there,
not tuned; each failure message prints the worst error / bound and its index).

The BatchNorm vectors are made on the host and ``stem_ref.mask32`` reproduces both ReLU masks bit for bit, so no element is
excluded and no margin around zero is used.  Every output - dL/dz (in place over g), dL/dy, dw and the four BatchNorm gradient
vectors - sits between NaN guard bands and, where it is not also an input, is pre-filled with NaN.  Each case id names the
instantiation it reaches (tests/chanlink_cases.py; asserted per case in tests/test_chanlink_ref_cpu.py); DESIGN.md, Appendix A.3,
lists every instantiation with its case.  With MSL_CHANLINK_RATIO_LOG=<file> every comparison appends
"<case id> <what> <error / bound>" to that file (for the error / bound table of DESIGN.md)."""
import functools
import os

import pytest
import torch

from mslesions3d_amd import _lib
from mslesions3d_amd._lib import ptr
from tests import bf16pw_ref as P
from tests import chanlink_cases as C
from tests import chanlink_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = 64  # guard elements on each side of every output (a multiple of 4: the views stay 16-byte aligned)
NAN = float("nan")
ENTRY = {False: "msl_block_bwd_channel_link", True: "msl_block_bwd_channel_link_bf16"}


def st():
    return torch.cuda.current_stream().cuda_stream


class Guarded:
    """An output buffer of n elements, NaN-filled (or holding ``init``), between two bands of G NaN guard elements."""

    def __init__(self, n, dtype=torch.float32, init=None):
        self.n = n
        self.full = torch.full((n + 2 * G,), NAN, dtype=dtype, device=DEV)
        self.v = self.full[G:G + n]
        if init is not None:
            self.v.copy_(init.reshape(-1).to(DEV))

    def intact(self, what):
        bands = torch.cat([self.full[:G], self.full[G + self.n:]])
        assert bool(torch.isnan(bands).all()), f"{what}: wrote outside its range"

    def untouched(self, what):
        assert bool(torch.isnan(self.full).all()), f"{what}: wrote to an output it must leave alone"

    def written(self, what):
        bad = int(torch.isnan(self.v).sum())
        assert bad == 0, f"{what}: {bad} elements were never written (or are NaN)"


def same_bits(a, b):
    it = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return a.dtype == b.dtype and bool(torch.equal(a.contiguous().view(it), b.contiguous().view(it)))


@functools.lru_cache(maxsize=None)
def inputs(cid, bf16):
    """Operands of one case (CPU, fp32 tensors; bf16 storage: holding bf16 values); computed once, never modified."""
    _, N, c, dims, stride, acc = C.BY_ID[cid]
    inp, _ = S.chain_case(N, c, dims, stride, acc, seed=1 + C.CASES.index(C.BY_ID[cid]))
    return S.as_bf16(inp) if bf16 else inp


class Launch:
    """The buffers of one call and the call itself (not synchronised)."""

    def __init__(self, inp, N, dims, stride, acc, bf16, with_dw):
        L = _lib.load()
        dt = torch.bfloat16 if bf16 else torch.float32
        c = inp["z"].shape[1]
        self.c, self.with_dw = c, with_dw
        self.src = {k: inp[k].to(DEV).to(dt if k in ("z", "y") else torch.float32).contiguous() for k in ("z", "y", "vz", "vy", "w")}
        self.ins = {k: v.clone() for k, v in self.src.items()}
        self.gz = Guarded(inp["G"].numel(), dt, init=inp["G"].to(dt))
        self.gy = Guarded(inp["y"].numel(), dt, init=inp["Hs"].to(dt) if acc else None)  # accumulate == 0: NaN must not leak
        self.dw = Guarded(c * 27)
        self.vec = [Guarded(c) for _ in range(4)]
        self.shapes = (inp["G"].shape, inp["y"].shape)
        i = self.ins
        self.rc = getattr(L, ENTRY[bf16])(ptr(self.gz.v), ptr(i["z"]), ptr(i["vz"]), ptr(i["w"]), ptr(i["y"]), ptr(i["vy"]), ptr(self.gy.v),
                                          ptr(self.vec[0].v), ptr(self.vec[1].v), ptr(self.vec[2].v), ptr(self.vec[3].v),
                                          ptr(self.dw.v) if with_dw else None, N, c, *dims, stride, acc, st())

    def outputs(self, what):
        """After a synchronise: bands intact, every slot written, inputs unchanged -> dict of chanlink_ref.KEYS."""
        assert self.rc == 0, f"{what}: returned {self.rc}"
        named = dict(gz=self.gz, gy=self.gy, dgam1=self.vec[0], dbet1=self.vec[1], dgam2=self.vec[2], dbet2=self.vec[3])
        for k, o in named.items():
            o.intact(f"{what} {k}")
            o.written(f"{what} {k}")
        if self.with_dw:
            self.dw.intact(f"{what} dw")
            self.dw.written(f"{what} dw")
        else:
            self.dw.untouched(f"{what} dw (dw == NULL)")
        for k in self.src:
            assert same_bits(self.ins[k], self.src[k]), f"{what}: input {k} changed"
        out = {k: o.v.clone() for k, o in named.items()}
        out["gz"], out["gy"] = out["gz"].view(self.shapes[0]), out["gy"].view(self.shapes[1])
        out["dw"] = self.dw.v.view(self.c, 27).clone() if self.with_dw else None
        return out


def check(cid, tag, got, inp, N, dims, stride, acc, bf16, with_dw):
    rep = S.judge(P.Report(f"{cid} {tag}"), got, inp, N, dims, stride, acc, bf16, with_dw)
    log = os.environ.get("MSL_CHANLINK_RATIO_LOG")
    if log:
        with open(log, "a") as f:
            for r in rep.rows:
                f.write(f"{cid} {tag}:{r['what']} {r['ratio']:.4f}\n")
    assert not rep.failures(), "\n".join(rep.failures())


def tag_of(bf16, with_dw):
    return ("bf16" if bf16 else "fp32") + ("+dw" if with_dw else "")


def run_case(cid, inp, N, dims, stride, acc, bf16):
    """Both forms (with the weight gradient, and dw == NULL) of one entry point at one case, each launched twice."""
    for with_dw in (True, False):
        tag = tag_of(bf16, with_dw)
        a = Launch(inp, N, dims, stride, acc, bf16, with_dw)
        b = Launch(inp, N, dims, stride, acc, bf16, with_dw)
        torch.cuda.synchronize()
        got, again = a.outputs(f"{cid} {tag}"), b.outputs(f"{cid} {tag}, second call")
        check(cid, tag, got, inp, N, dims, stride, acc, bf16, with_dw)
        # fixed summation order, no atomics: two calls on equal inputs agree bit for bit
        for k in S.KEYS:
            assert (got[k] is None and again[k] is None) or same_bits(got[k], again[k]), f"{cid} {tag}: {k} differs between two calls"


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("cid", [c[0] for c in C.CASES])
def test_channel_link(cid, bf16):
    """One configuration (named by the id), one storage type, BWW on and off."""
    _, N, c, dims, stride, acc = C.BY_ID[cid]
    p = S.plan(N, dims, stride)
    assert _lib.load().msl_block_bwd_channel_link_supported(N, *dims, stride) == p["nw"] == C.config_of_id(cid)[0]
    run_case(cid, inputs(cid, bf16), N, dims, stride, acc, bf16)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("acc", [0, 1])
def test_cancelled_channel(acc, bf16):
    """Seed 0 of 4 x 2 x 16^3: the BatchNorm2 scale gradient of one channel is what is left of terms 60 000 times its size.
    Its bound is relative to the sum of those terms' magnitudes, so the case passes for the right reason."""
    cid, N, c, dims, stride = C.CANCELLED
    inp, _ = S.chain_case(N, c, dims, stride, acc, seed=0)
    run_case(cid, S.as_bf16(inp) if bf16 else inp, N, dims, stride, acc, bf16)


@pytest.mark.parametrize("cid", C.STALE_LDS)
def test_no_stale_lds_between_launches(cid):
    """Two different inputs back to back on one stream, no synchronise in between: nothing of one launch's LDS image (or of
    its tap-gradient exchange, which reuses the image region) may show in the next."""
    _, N, c, dims, stride, acc = C.BY_ID[cid]
    first = inputs(cid, False)
    second, _ = S.chain_case(N, c, dims, stride, acc, seed=400)
    runs = [(inp, Launch(inp, N, dims, stride, acc, False, True)) for inp in (first, second, first)]
    torch.cuda.synchronize()
    for k, (inp, run) in enumerate(runs):
        check(cid, f"back-to-back-{k}", run.outputs(f"{cid} launch {k}"), inp, N, dims, stride, acc, False, True)


# ------------------------------------------------------------------------------------------------- refusals
def _refusal_buffers(N, c, dims):
    n = max(N, 1) * max(c, 1) * max(dims[0], 1) * max(dims[1], 1) * max(dims[2], 1)
    cc = max(c, 1)
    ins = dict(z=torch.ones(n, device=DEV), y=torch.ones(n, device=DEV), vz=torch.ones(4 * cc, device=DEV),
               vy=torch.ones(4 * cc, device=DEV), w=torch.ones(27 * cc, device=DEV))
    outs = dict(gz=Guarded(n), gy=Guarded(n), dw=Guarded(27 * cc), **{f"v{k}": Guarded(cc) for k in range(4)})
    return ins, outs


def _call(L, bf16, ins, outs, N, c, dims, stride, acc, null=None):
    a = [ptr(outs["gz"].v), ptr(ins["z"]), ptr(ins["vz"]), ptr(ins["w"]), ptr(ins["y"]), ptr(ins["vy"]), ptr(outs["gy"].v)]
    if null is not None:
        a[null] = None
    return getattr(L, ENTRY[bf16])(*a, ptr(outs["v0"].v), ptr(outs["v1"].v), ptr(outs["v2"].v), ptr(outs["v3"].v), ptr(outs["dw"].v),
                                   N, c, *dims, stride, acc, st())


@pytest.mark.parametrize("case", C.REFUSALS, ids=[c[0] for c in C.REFUSALS])
def test_refusals(case):
    """Both entry points return the code, launch nothing (msl_thread_launch_count) and leave every output NaN."""
    _, N, c, dims, stride, want = case
    L = _lib.load()
    ins, outs = _refusal_buffers(N, c, dims)
    if want == -2 or N <= 0:
        assert L.msl_block_bwd_channel_link_supported(N, *dims, stride) == 0
    n0 = L.msl_thread_launch_count()
    for bf16 in (False, True):
        for acc in (0, 1):
            assert _call(L, bf16, ins, outs, N, c, dims, stride, acc) == want, (bf16, acc)
    assert L.msl_thread_launch_count() == n0, "a refused call launched a kernel"
    torch.cuda.synchronize()
    for k, o in outs.items():
        o.untouched(k)


def test_null_pointer_refusals():
    """g_z, z, vec_z, w_dw, y_prev, vec_y, g_y: each one NULL is MSL_ERR_ARG at a shape that is otherwise served."""
    L = _lib.load()
    N, c, dims = 2, 2, (4, 4, 8)
    ins, outs = _refusal_buffers(N, c, dims)
    n0 = L.msl_thread_launch_count()
    for bf16 in (False, True):
        for stride in (1, 2):
            assert L.msl_block_bwd_channel_link_supported(N, *dims, stride) > 0
            for k in range(7):
                assert _call(L, bf16, ins, outs, N, c, dims, stride, 1, null=k) == -1, (bf16, stride, k)
    assert L.msl_thread_launch_count() == n0, "a refused call launched a kernel"
    torch.cuda.synchronize()
    for k, o in outs.items():
        o.untouched(k)
