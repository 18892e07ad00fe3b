"""Every depthwise-convolution FORWARD entry point - msl_dwconv_fwd, msl_dwconv_fwd_fold, msl_dwconv_fwd_bf16,
msl_dwconv_fwd_small_eval_bf16 and msl_dwconv_fwd_wave_bf16_fold - path by path against the float64 reference of
tests/dwfwd_ref.py (bounds derived there, not tuned; a failure prints the worst error / bound and its index).

The cases are the CPU data of tests/dwfwd_cases.py; tests/test_dwfwd_ref_cpu.py proves at the same cases that every check accepts
honest fp32 and rejects ten kinds of wrong kernel.  Every test first asserts the route its case id names, then runs with and
without the input affine.  fp32 outputs are held to their bound, bf16 outputs to their rounding interval; every statistics slot
is held to the float64 sum of the reference over exactly the outputs the kernel adds into it - on bf16 storage the sums of the
unrounded accumulators.  Outputs are pre-filled with NaN between guard bands; partial buffers are sized exactly by the count
query, NaN-filled, with a guard of 64 sentinel doubles inside the same allocation.  Every line printed is
"<case id> aff<0|1> route=<route> y=<error / bound> [sum=.. sumsq=..] [pinned=<share>]"; with MSL_DWFWD_RATIO_LOG=<file> the line
is appended to that file too."""
import os

import pytest
import torch

from mslesions3d_amd import _lib
from mslesions3d_amd._lib import ptr
from tests import dwfwd_cases as C
from tests import dwfwd_ref as D
from tests.test_dwfwd_ref_cpu import assert_route
from tests.test_gpu_dw_exact import GUARD, assert_guard_untouched, guarded
from tests.test_gpu_pw import Guarded, dev, same_bits, st
from tests.test_gpu_pw import _release_kept  # noqa: F401  (autouse fixture: frees what dev() and Guarded keep alive)

pytestmark = pytest.mark.gpu
NAN = float("nan")
ERR_ARG, ERR_UNSUPPORTED = -1, -2


def partial_buffer(C_, NP):
    """[2 C NP NaN doubles | guard] in one allocation -> (whole buffer, partial region)."""
    buf, part = guarded(2 * C_ * NP)
    part.fill_(NAN)
    assert buf.numel() == 2 * C_ * NP + GUARD
    return buf, part


def launch(case, d, affine, sc=None, sh=None, fold=False):
    """One launch of the case's entry point into fresh buffers -> (y Guarded, partials (2, C, NP) on the device or None, NP)."""
    id_, entry, bf16, N, Cc, dims, stride, o = case
    L = _lib.load()
    dt = torch.bfloat16 if bf16 else torch.float32
    OD, OH, OW = D.out_dims(dims, stride)
    xd, wd = dev(d["x"].to(dt)), dev(d["w"])
    scp, shp = (ptr(dev(sc)), ptr(dev(sh))) if affine and not fold else (None, None)
    y = Guarded(N * Cc * OD * OH * OW, dtype=dt)
    shape = (N, Cc, *dims, stride)
    buf = part = None
    NP = 0
    if entry in ("train", "fold"):
        if o.get("force_naive"):  # channel_stats_kernel's grid (dwconv.hip, the Naive branch of dwconv_fwd_impl): no query counts it
            NP = N * D.cdiv(OD * OH * OW, 4096)
        else:
            NP = (L.msl_dwconv_fwd_bf16_num_partials if bf16 else L.msl_dwconv_fwd_num_partials)(*shape)
        assert NP > 0
        buf, part = partial_buffer(Cc, NP)
    if fold:
        pin, ga, be = dev(d["part_in"]), dev(d["gamma"]), dev(d["beta"])
        fn = L.msl_dwconv_fwd_wave_bf16_fold if bf16 else L.msl_dwconv_fwd_fold
        rc = fn(ptr(xd), ptr(pin), o["in_np"], C.FOLD_COUNT, ptr(ga), ptr(be), C.EPS, ptr(wd), ptr(y.v), ptr(buf), *shape, st())
    elif entry == "small_bf16":
        rc = L.msl_dwconv_fwd_small_eval_bf16(ptr(xd), scp, shp, ptr(wd), ptr(y.v), *shape, st())
    elif bf16:
        rc = L.msl_dwconv_fwd_bf16(ptr(xd), scp, shp, ptr(wd), ptr(y.v), ptr(buf) if buf is not None else None, *shape, st())
    else:
        rc = L.msl_dwconv_fwd(ptr(xd), scp, shp, ptr(wd), ptr(y.v), ptr(buf) if buf is not None else None, *shape,
                              int(bool(o.get("force_naive"))), st())
    torch.cuda.synchronize()
    assert rc == 0, f"{id_}: returned {rc}"
    y.intact(f"{id_}: y")
    if buf is not None:
        assert_guard_untouched(buf, 2 * Cc * NP, f"{id_}: partials")
        part = part.view(2, Cc, NP)
    assert same_bits(xd.float(), d["x"].to(dt).float().to("cuda")) and same_bits(wd, d["w"].to("cuda")), f"{id_}: inputs changed"
    return y, part, NP


def judge(case, affine, e, y, part, route, plan):
    """Print the figures, then assert every check of dwfwd_ref.check."""
    id_, entry, bf16, N, Cc, dims, stride, o = case
    OD, OH, OW = D.out_dims(dims, stride)
    rep = D.check(id_, e, y.v.detach().cpu().float().view(N, Cc, OD, OH, OW), bf16, None if part is None else part.cpu(), route, plan,
                  dims, stride)
    line = f"{id_} aff{affine} route={route} " + " ".join(f"{r['what']}={r['ratio']:.4f}" for r in rep.rows)
    if bf16:
        line += f" pinned={rep.rows[0]['pinned']:.4f}"
    print(line)
    log = os.environ.get("MSL_DWFWD_RATIO_LOG")
    if log:
        with open(log, "a") as f:
            f.write(line + "\n")
    assert rep.failures() == [], "\n".join(rep.failures())


def run_case(case, affine):
    route, plan = assert_route(case)
    d = C.make_data(case)
    sc, sh = (d["sc"], d["sh"]) if affine else (None, None)
    y, part, _ = launch(case, d, affine, sc, sh)
    judge(case, affine, D.expect(d["x"], d["w"], case[6], sc, sh), y, part, route, plan)


@pytest.mark.parametrize("affine", [0, 1])
@pytest.mark.parametrize("case", C.TRAIN_CASES, ids=C.ids(C.TRAIN_CASES))
def test_dw_fwd_with_statistics(case, affine):
    """msl_dwconv_fwd / msl_dwconv_fwd_bf16 with partials: wave (both strides, shared and split planes), stream (both
    instantiations), resident, naive (by shape and forced) and the bf16 tiled kernel (both staging paths, several tiles)."""
    run_case(case, affine)


@pytest.mark.parametrize("affine", [0, 1])
@pytest.mark.parametrize("case", C.EVAL_CASES, ids=C.ids(C.EVAL_CASES))
def test_dw_fwd_without_statistics(case, affine):
    """The statistics-free forward on the rows and small-map kernels, fp32 and bf16, the latter through both of its entries."""
    run_case(case, affine)


@pytest.mark.parametrize("case", C.FOLD_CASES, ids=C.ids(C.FOLD_CASES))
def test_dw_fwd_fold(case):
    """msl_dwconv_fwd_fold / msl_dwconv_fwd_wave_bf16_fold: the (scale | shift) msl_bn_finalize writes for the same producer
    partials are the operands of the reference, and y and the partials equal the explicit path's bit for bit."""
    id_, entry, bf16, N, Cc, dims, stride, o = case
    L = _lib.load()
    route, plan = assert_route(case)
    d = C.make_data(case)
    vec = dev(torch.zeros(4 * Cc))  # scale | shift | mean | invstd
    rc = L.msl_bn_finalize(ptr(dev(d["part_in"])), o["in_np"], C.FOLD_COUNT, ptr(dev(d["gamma"])), ptr(dev(d["beta"])), None, None, None,
                           0.1, C.EPS, ptr(vec), ptr(vec[Cc:]), ptr(vec[2 * Cc:]), ptr(vec[3 * Cc:]), Cc, st())
    torch.cuda.synchronize()
    assert rc == 0
    sc, sh = vec[:Cc].cpu(), vec[Cc:2 * Cc].cpu()
    y, part, NP = launch(case, d, 1, fold=True)
    judge(case, 1, D.expect(d["x"], d["w"], stride, sc, sh), y, part, route, plan)
    explicit = (id_, "train", bf16, N, Cc, dims, stride, dict(route=o["route"]))
    y2, part2, NP2 = launch(explicit, d, 1, sc, sh)
    assert NP2 == NP
    assert torch.equal(y.v, y2.v) and same_bits(y.v.float(), y2.v.float()), f"{id_}: y differs from the explicit path's"
    assert torch.equal(part, part2) and same_bits(part, part2), f"{id_}: the partials differ from the explicit path's"


def test_dw_fwd_refusals():
    """Bad arguments -> ERR_ARG, a bf16 fold or small-map call on a shape without that kernel -> ERR_UNSUPPORTED; by return code
    only, and nothing is written."""
    L = _lib.load()
    x, w, v = dev(torch.ones(4096)), dev(torch.ones(64 * 27)), dev(torch.ones(64))
    xb = dev(torch.ones(4096).to(torch.bfloat16))
    pin = dev(torch.ones(2 * 64 * 6, dtype=torch.float64))
    y, yb, part = Guarded(4096), Guarded(4096, dtype=torch.bfloat16), Guarded(4096, dtype=torch.float64)
    for shape in ((0, 2, 4, 4, 4, 1), (1, 0, 4, 4, 4, 1), (1, 2, 4, 4, 0, 1), (1, 2, 4, 4, 4, 3), (1, 2, 4, 4, 4, 0)):
        assert L.msl_dwconv_fwd(ptr(x), None, None, ptr(w), ptr(y.v), ptr(part.v), *shape, 0, st()) == ERR_ARG
        assert L.msl_dwconv_fwd_bf16(ptr(xb), None, None, ptr(w), ptr(yb.v), ptr(part.v), *shape, st()) == ERR_ARG
        assert L.msl_dwconv_fwd_small_eval_bf16(ptr(xb), None, None, ptr(w), ptr(yb.v), *shape, st()) == ERR_ARG
        assert L.msl_dwconv_fwd_fold(ptr(x), ptr(pin), 6, 100.0, ptr(v), ptr(v), C.EPS, ptr(w), ptr(y.v), ptr(part.v), *shape, st()) == ERR_ARG
        assert L.msl_dwconv_fwd_wave_bf16_fold(ptr(xb), ptr(pin), 6, 100.0, ptr(v), ptr(v), C.EPS, ptr(w), ptr(yb.v), ptr(part.v), *shape,
                                               st()) == ERR_ARG
    ok = (1, 2, 4, 4, 4, 1)
    assert L.msl_dwconv_fwd_fold(ptr(x), None, 6, 100.0, ptr(v), ptr(v), C.EPS, ptr(w), ptr(y.v), ptr(part.v), *ok, st()) == ERR_ARG
    assert L.msl_dwconv_fwd_fold(ptr(x), ptr(pin), 0, 100.0, ptr(v), ptr(v), C.EPS, ptr(w), ptr(y.v), ptr(part.v), *ok, st()) == ERR_ARG
    # 6 x 6 planes: no wave kernel; 9 x 9 x 9: 729 voxels are more than the small-map kernel parks
    assert L.msl_dwconv_fwd_wave_bf16_fold(ptr(xb), ptr(pin), 6, 100.0, ptr(v), ptr(v), C.EPS, ptr(w), ptr(yb.v), ptr(part.v), 1, 2, 4, 6, 6, 1,
                                           st()) == ERR_UNSUPPORTED
    assert L.msl_dwconv_fwd_small_eval_bf16(ptr(xb), None, None, ptr(w), ptr(yb.v), 1, 2, 9, 9, 9, 1, st()) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    for b in (y, yb, part):
        b.untouched("a refused depthwise forward")
