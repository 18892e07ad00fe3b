"""msl_detect_objects (csrc/detect.hip) branch by branch against oracle/detect.py: every case of tests/detect_cases.py (the
branch each reaches is proved in tests/test_detect_cases_cpu.py), called through ``_lib.call`` with the test's own priors.

Every scratch and output buffer is overwritten with garbage before every launch (0xFF bytes in the integer buffers, NaN in
the float ones, 0xA5 bytes in the outputs): the header promises no initialisation, so the kernel may rely on none.  The
keep-lists are exact by construction (detect_cases' docstring), so everything but the decode test is asserted bit for bit:
outputs, probabilities (== torch.softmax) and the scratch the header documents - ncand, nkept, the ranked candidates, the keep
bits with zero words beyond the last block - plus the threshold bin, histogram and shortlist in ``select_ws``."""
import types

import numpy as np
import pytest
import torch

from mslesions3d_amd import _lib
from mslesions3d_amd._lib import ptr
from mslesions3d_amd.ssd3d import LSSD3D
from tests import detect_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OUT_BYTE, COUNT_FILL = 0xA5, -77
FLOAT_SCRATCH = ("probs", "boxes", "tmp_s")
INT_SCRATCH = ("sorted_idx", "ncand", "mask", "keep", "nkept", "tmp_r", "sel")


def st():
    return torch.cuda.current_stream().cuda_stream


def poison(w):
    for k in FLOAT_SCRATCH:
        w[k].fill_(float("nan"))
    for k in INT_SCRATCH:
        w[k].fill_(-1)  # 0xFF bytes: index -1, all-ones masks
    w["out_all"].fill_(OUT_BYTE)
    w["oc"].fill_(COUNT_FILL)


def launch(c, w, dev_in, top_k=None, N=None, P=None, ncls=None, sel="sel"):
    locs, scores, priors = dev_in
    _lib.call("msl_detect_objects", ptr(locs), ptr(scores), ptr(priors), c.N if N is None else N, c.P if P is None else P,
              c.ncls if ncls is None else ncls, float(c.min_score), float(c.max_overlap), int(c.top_k if top_k is None else top_k),
              ptr(w["probs"]), ptr(w["boxes"]), ptr(w["sorted_idx"]), ptr(w["ncand"]), ptr(w["mask"]), ptr(w["keep"]),
              ptr(w["nkept"]), ptr(w["tmp_s"]), ptr(w["tmp_r"]), ptr(w[sel]) if sel else None, ptr(w["ob"]), ptr(w["os"]),
              ptr(w["ol"]), ptr(w["op"]), ptr(w["oc"]), st())


def to_dev(c):
    return c.locs.to(DEV).contiguous(), c.scores.to(DEV).contiguous(), c.priors.to(DEV).contiguous()


def run(c, w=None, fresh_poison=True):
    """One launch on a poisoned workspace -> (detections as _detect_collect returns them, scratch on the host)."""
    if w is None:
        w = LSSD3D.new_detect_workspace(c.N, c.P, c.ncls, c.top_k, DEV)
    if fresh_poison:
        poison(w)
    dev_in = to_dev(c)
    launch(c, w, dev_in)
    det = LSSD3D._detect_collect(w, c.N, return_prior_index=True)
    torch.cuda.synchronize()
    scratch = {k: w[k].cpu() for k in FLOAT_SCRATCH + INT_SCRATCH if k != "mask"}
    return [[t.cpu() for t in lst] for lst in det], scratch


def same_bits(a, b):
    return a.dtype == b.dtype == torch.float32 and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def check_probs(c, r, scratch):
    """bit for bit torch.softmax where torch is not NaN; NaN where it is"""
    got = scratch["probs"]                       # (N, ncls-1, P)
    want = r.probs[:, :, 1:].permute(0, 2, 1)    # (N, P, ncls) -> (N, ncls-1, P)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), f"{c.id}: NaN probabilities differ from torch.softmax"
    assert same_bits(torch.where(nan, torch.zeros_like(got), got), torch.where(nan, torch.zeros_like(want), want).contiguous()), \
        f"{c.id}: probabilities are not torch.softmax bit for bit"


def check(c, det, scratch):
    r = C.reference(c.id)
    check_probs(c, r, scratch)
    boxes, labels, scores, prior = det
    cap, k1 = 10 * c.top_k, c.ncls - 1
    Wn = (cap + 63) // 64
    dec = torch.cat([c.priors[:, :3] - c.priors[:, 3:] / 2, c.priors[:, :3] + c.priors[:, 3:] / 2], dim=1)
    assert same_bits(scratch["boxes"], dec[None].expand(c.N, -1, -1).contiguous()), f"{c.id}: decoded boxes (locs = 0)"
    sel = scratch["sel"].numpy().reshape(c.N * k1, C.sel_stride(c.P))
    keep_words = scratch["keep"].numpy().view(np.uint64).reshape(c.N * k1, Wn)
    for n in range(c.N):
        for k in range(1, c.ncls):
            nc, what = n * k1 + (k - 1), f"{c.id} image {n} class {k}"
            ncand, ranked, keep = r.trace[(n, k)]
            ranked, keep = ranked.numpy(), keep.numpy()
            M = ranked.size
            assert int(scratch["ncand"][nc]) == ncand, (what, "ncand", int(scratch["ncand"][nc]), ncand)
            want = C.selection(r.probs[n, :, k].numpy(), c.min_score, cap)
            assert np.array_equal(sel[nc, :C.HB], want["hist"]), (what, "score histogram")
            assert int(sel[nc, C.HB]) == want["thr"], (what, "threshold bin", int(sel[nc, C.HB]), want["thr"])
            K = int(sel[nc, C.HB + 1])
            assert K == want["shortlist"].size, (what, "shortlist length", K, want["shortlist"].size)
            assert np.array_equal(np.sort(sel[nc, C.HB + 4:C.HB + 4 + K]), want["shortlist"]), (what, "shortlist")
            got_rank = scratch["sorted_idx"][n, k - 1, :M].numpy()
            assert np.array_equal(got_rank, ranked), (what, "ranked candidates", got_rank, ranked)
            bits = ((keep_words[nc][:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool).reshape(-1)
            nblk = (M + 63) // 64
            assert not keep_words[nc][nblk:].any(), (what, "keep words beyond the last block", keep_words[nc][nblk:])
            assert np.array_equal(bits[:M], keep), (what, "keep bits", np.nonzero(bits[:M] != keep)[0])
            assert not bits[M:].any(), (what, "keep bits beyond the last candidate")
            assert int(scratch["nkept"][nc]) == int(keep.sum()), (what, "nkept")
    for n in range(c.N):
        what = f"{c.id} image {n}"
        assert boxes[n].shape[0] == r.boxes[n].shape[0], (what, "count", boxes[n].shape[0], r.boxes[n].shape[0])
        assert torch.equal(prior[n], r.prior[n]), (what, "prior indices", prior[n], r.prior[n])
        assert torch.equal(labels[n], r.labels[n]), (what, "labels", labels[n], r.labels[n])
        assert same_bits(scores[n], r.scores[n]), (what, "scores")
        assert same_bits(boxes[n], r.boxes[n]), (what, "boxes")
        if r.prior[n][0] >= 0:  # scores are the softmax gathered at (prior, label)
            assert same_bits(scores[n], r.probs[n][r.prior[n], r.labels[n]]), (what, "scores vs softmax")


@pytest.mark.parametrize("cid", C.CASE_IDS)
def test_case_matches_the_oracle(cid):
    c = C.case(cid)
    check(c, *run(c))


def test_one_poisoned_workspace_three_inputs():
    """Many candidates, then few, then none through ONE workspace that was poisoned once: nothing of an earlier batch (its
    counters, shortlist, keep words, outputs) may leak into the next."""
    cs = [C.case(i) for i in C.REUSE_IDS]
    w = LSSD3D.new_detect_workspace(cs[0].N, cs[0].P, cs[0].ncls, cs[0].top_k, DEV)
    poison(w)
    for c in cs:
        check(c, *run(c, w, fresh_poison=False))


def test_decode_within_the_derived_bound():
    """The only tolerance of this file: the ``boxes`` scratch against the decode in float64 on the same fp32 inputs, bound
    derived per element in detect_cases.decode_reference (fp32 torch is proved to stay inside it on the CPU)."""
    c = C.decode_case()
    _, scratch = run(c)
    check_probs(c, types.SimpleNamespace(probs=torch.softmax(c.scores, dim=2)), scratch)
    ref, bound = C.decode_reference(c.locs[0], c.priors)
    err = np.abs(scratch["boxes"][0].double().numpy() - ref)
    worst = np.unravel_index(np.argmax(err / bound), err.shape)
    print(f"decode: worst error / bound = {(err / bound).max():.3f} at {worst}")
    assert (err <= bound).all(), (worst, err[worst], bound[worst])


REFUSALS = [
    ("top_k=410", dict(top_k=410), -2),
    ("ncls=3,P=1", dict(), -2),
    ("top_k=0", dict(top_k=0), -1),
    ("N=0", dict(N=0), -1),
    ("P=0", dict(P=0), -1),
    ("ncls=1", dict(ncls=1), -1),
    ("null-select_ws", dict(sel=None), -1),
]


@pytest.mark.parametrize("name,kw,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_return_before_any_launch(name, kw, code):
    """Each refusal comes back with its code and leaves every pre-filled output and scratch buffer as it was."""
    if name == "ncls=3,P=1":
        c = C._ns(name, C.lattice_boxes(1, 1), np.zeros((1, 1, 3), dtype=np.float32), 5, 0.25, 0.5, {})
    else:
        c = C.case("sel:below-cap-P257")
    # buffers sized for the arguments actually passed, so that a refusal that failed could not write out of bounds
    w = LSSD3D.new_detect_workspace(c.N, c.P, c.ncls, max(c.top_k, kw.get("top_k", 0)), DEV)
    poison(w)
    torch.cuda.synchronize()
    before = {k: w[k].clone() for k in FLOAT_SCRATCH + INT_SCRATCH + ("out_all", "oc")}
    with pytest.raises(_lib.HipKernelError, match=rf"code {code} "):
        launch(c, w, to_dev(c), **kw)
    torch.cuda.synchronize()
    for k, b in before.items():
        assert torch.equal(w[k].view(torch.uint8), b.view(torch.uint8)), (name, k, "changed by a refused call")
    assert (w["out_all"] == OUT_BYTE).all() and (w["oc"] == COUNT_FILL).all()
