"""Proves the reference (tests/multibox_ref.py) and the cases (tests/multibox_cases.py) of tests/test_gpu_multibox.py, without
a GPU: the reference against the oracle's MultiBox loss, and every condition the cases promise against the oracle's IoU."""
import numpy as np
import pytest
import torch

from oracle import boxes as OB
from oracle import multibox as OMB
from tests import multibox_cases as C
from tests import multibox_ref as R
from tests.golden import cases, detinit
from tests.util import oracle_model


# ------------------------------------------------------------------------------------------ reference against oracle
@pytest.fixture(scope="module")
def priors_c64():
    return oracle_model().priors_cxcycz


@pytest.mark.parametrize("name", list(cases.matching_cases().keys()))
def test_reference_equals_the_oracle_loss_and_its_autograd(name, priors_c64):
    """fp64 reference from the oracle's targets against oracle.multibox.multibox_loss (fp32) and autograd on it, for all eight
    flag sets: 2e-5 relative for the losses (sums of ~1.2 k fp32 terms), and for the gradients 2e-5 of their largest
    magnitude."""
    c = cases.matching_cases()[name]
    n = len(c["boxes"])
    locs, scores = detinit.make_head_outputs(c["head_seed"], n, cases.P_C64)
    locs = locs * 3.0
    tc, tl, _ = OMB.match_batch(c["boxes"], c["labels"], priors_c64, c["threshold"])
    for flags in range(8):
        ol, osc = locs.clone().requires_grad_(True), scores.clone().requires_grad_(True)
        oc, olc = OMB.multibox_loss(ol, osc, c["boxes"], c["labels"], priors_c64, c["threshold"],
                                    hard_negative_mining=bool(flags & 1), smooth_l1=bool(flags & 2), focal=bool(flags & 4),
                                    neg_pos_ratio=3)
        (0.7 * oc + 1.3 * olc).backward()
        r = R.losses_and_grads(locs, scores, tc, tl, flags, 3, 0.7, 1.3)
        assert r["n_pos"] == int((tc > 0).sum())
        np.testing.assert_allclose(float(r["conf"]), oc.item(), rtol=2e-5, err_msg=f"conf, flags {flags}")
        np.testing.assert_allclose(float(r["loc"]), olc.item(), rtol=2e-5, err_msg=f"loc, flags {flags}")
        assert R.deviation(ol.grad, r["dlocs"]) < 2e-5, f"dlocs, flags {flags}"
        assert R.deviation(osc.grad, r["dscores"]) < 2e-5, f"dscores, flags {flags}"
        assert float(r["dscores"][tc < 0].abs().max() if (tc < 0).any() else 0.0) == 0.0
        assert float(r["dlocs"][tc <= 0].abs().max()) == 0.0


# -------------------------------------------------------------------------------------------------- matching cases
def _iou(c, i):
    return OB.iou_matrix(c["boxes"][i], OB.cxcycz_to_xyz(c["priors"]))


def test_matching_cases_cover_every_prior_count_and_batch_size():
    got = {(C.matching_case(n)["priors"].shape[0], len(C.matching_case(n)["boxes"])) for n in C.MATCH_NAMES}
    assert {p for p, _ in got} == set(C.MATCH_P)
    for p in C.MATCH_P:
        assert {n for q, n in got if q == p} == {1, 3}, p
    kinds = {k for n in C.MATCH_NAMES for k in C.matching_case(n)["kinds"]}
    assert kinds == {"none", "one", "dozen", "many300", "special", "dozen_dup"}


@pytest.mark.parametrize("name", C.MATCH_NAMES)
def test_matching_cases_keep_their_promises(name):
    c = C.matching_case(name)
    pri = c["priors"]
    lo, hi, soft = C.thresholds(c["threshold"])
    # the dyadic grid: every coordinate a multiple of 2^-5, corners of the priors multiples of 2^-6
    for t in [pri] + c["boxes"]:
        assert torch.equal(t * 32, (t * 32).round())
        assert t.numel() == 0 or (float(t.min()) >= 0 and float(t.max()) <= 1)
    for i, (boxes, labels, prom) in enumerate(zip(c["boxes"], c["labels"], c["promises"])):
        if boxes.shape[0] == 0:
            continue
        assert bool(((boxes[:, 3:] - boxes[:, :3]) > 0).all()) and bool((labels > 0).all())
        iou = _iou(c, i)
        pxyz = OB.cxcycz_to_xyz(pri)
        union = OB.box_volume(boxes)[:, None] + OB.box_volume(pxyz)[None, :] - OB.intersection(boxes, pxyz)
        assert float(union.min()) > 0 and not bool(torch.isnan(iou).any()), "no union is 0"
        # exact in fp32: the same IoU from float64 arithmetic, rounded once
        i64 = OB.iou_matrix(boxes.double(), pxyz.double())
        assert torch.equal(iou, i64.float()), "the geometry is not exact in fp32"
        label, obj, overlap, _ = OMB.match_image(boxes, labels, pri, c["threshold"])
        best_prior = OMB._first_argmax(iou, 1)[1]
        for o, tied in prom.get("ties", []):
            at_max = (iou[o] == iou[o].max()).nonzero().flatten().tolist()
            assert tuple(at_max) == tuple(sorted(tied)) and len(tied) >= 2, (o, at_max, tied)
            assert len({iou[o, p].view(torch.int32).item() for p in tied}) == 1, "tied priors must have bit-equal IoU"
            assert int(best_prior[o]) == min(tied)
        for p, value, o in prom.get("thr", []):
            assert overlap[p].item() == value and int(obj[p]) == o, (p, overlap[p].item(), int(obj[p]))
            if value == lo:  # on thr_lo: not below it, so the label survives (hard) or is ignored (soft)
                assert int(label[p]) == (-1 if soft else int(labels[o]))
            elif soft and value == hi:  # on thr_hi: not inside the band
                assert int(label[p]) == int(labels[o])
        if prom.get("thr"):
            assert {v for _, v, _ in prom["thr"]} >= ({lo, hi} if soft else {lo}), "no IoU on this case's threshold"
        for o in prom.get("unmatched", []):
            assert float(iou[o].max()) < lo, "the box only the force-match assigns overlaps a prior"
            assert int(label[best_prior[o]]) == int(labels[o]) and overlap[best_prior[o]].item() == 1.0
        for o1, o2 in prom.get("dup", []):
            assert torch.equal(boxes[o1], boxes[o2]) and int(labels[o1]) != int(labels[o2]) and o1 < o2
            assert int(best_prior[o1]) == int(best_prior[o2]) and int(obj[best_prior[o1]]) == o2, "last claim wins"
            first = OMB._first_argmax(iou, 0)[1]
            shared = (first == o1) & (iou[o1] > 0)
            shared[best_prior[o1]] = False
            assert bool(shared.any()) and bool((obj[shared] == o1).all()), "first of two equal objects wins elsewhere"
        if prom.get("many"):
            assert boxes.shape[0] == 300
            assert best_prior.unique().numel() < 300, "300 objects without a duplicate claim"
            later = best_prior[256:]
            assert bool((later[:, None] == best_prior[None, :256]).any()), "no claim of objects >= 256 meets an earlier one"


# ------------------------------------------------------------------------------------------------- mining conditions
def _mining_inputs():
    for name in C.LOSS_NAMES:
        yield name, C.loss_case(name)
    for name in C.MINING_NAMES:
        yield name, C.mining_case(name)


@pytest.mark.parametrize("name,c", list(_mining_inputs()), ids=[n for n, _ in _mining_inputs()])
def test_mined_set_does_not_depend_on_rounding(name, c):
    """The condition that lets the GPU test demand an exact mask: distinct negative losses are at least 1e-3 (relative) apart
    in fp64, and the mask from fp32 torch equals the mask from fp64."""
    tc = c["true_classes"]
    for flags in ([R.HNM, R.HNM | R.FOCAL] if c["ncls"] == 2 else [R.HNM]):
        neg64 = R.conf_loss_neg(c["scores"], tc, flags, torch.float64)
        neg32 = R.conf_loss_neg(c["scores"], tc, flags, torch.float32)
        v = neg64[tc == 0].sort().values
        if v.numel() > 1:
            gap, mag = v[1:] - v[:-1], v[1:]
            distinct = gap > 1e-9 * mag  # bit-equal rows give equal fp64 losses up to nothing at all
            assert float(v.min()) > 0
            assert bool((gap[~distinct] == 0).all()), "near-equal losses that are not copies"
            if distinct.any():
                assert float((gap / mag)[distinct].min()) >= 1e-3, float((gap / mag)[distinct].min())
        n_pos = (tc > 0).sum(dim=1)
        m64, m32 = R.mined_mask(neg64, n_pos, c["ratio"]), R.mined_mask(neg32, n_pos, c["ratio"])
        assert torch.equal(m64, m32)
        for n in range(c["N"]):  # equal fp64 losses are equal in fp32 too (the stable order is then the same)
            assert torch.equal(neg32[n].sort(descending=True, stable=True).indices,
                               neg64[n].sort(descending=True, stable=True).indices)


@pytest.mark.parametrize("name", C.MINING_NAMES)
def test_mining_cases_put_the_cut_where_they_say(name):
    c = C.mining_case(name)
    tc, P = c["true_classes"], c["P"]
    for flags in (R.HNM, R.HNM | R.FOCAL):
        neg = R.conf_loss_neg(c["scores"], tc, flags)[0]
        k = min(c["ratio"] * int((tc[0] > 0).sum()), P)
        s = neg.sort(descending=True, stable=True).values
        mask = R.mined_mask(neg[None], (tc[:1] > 0).sum(dim=1), c["ratio"])[0]
        if c["kind"] == "run":
            assert 0 < k < P and s[k - 1] == s[k] and float(s[k]) > 0, "the cut is not inside a run of copied rows"
            idx = (neg == s[k]).nonzero().flatten()
            kept = int(mask[idx].sum())
            assert 0 < kept < idx.numel() and bool(mask[idx[:kept]].all()), "ties must be kept in index order"
        elif c["kind"] == "zeros":
            assert int((neg > 0).sum()) <= k < P, "the cut is not among the zeros of the positive and ignored priors"
            assert bool(mask[neg > 0].all()) and int(mask.sum()) == k
        elif c["kind"] == "k0":
            assert k == 0 and not bool(mask.any())
        else:
            assert c["ratio"] * int((tc[0] > 0).sum()) >= P and bool(mask.all())


def test_loss_cases_are_what_the_suite_needs():
    assert {(C.loss_case(n)["N"], C.loss_case(n)["P"]) for n in C.LOSS_NAMES} == set(C.LOSS_SHAPES)
    for name in C.LOSS_NAMES:
        c = C.loss_case(name)
        tc, d = c["true_classes"], (c["locs"] - c["true_locs"])
        assert int(tc.max()) == c["ncls"] - 1 or c["P"] == 1
        assert int(tc.min()) >= -1 and int(tc[0, 0]) > 0 and int(tc[0, -1]) > 0
        if c["N"] > 1:
            assert bool((tc[1] == 0).all()), "image 1 has neither positives nor ignored priors"
        if c["P"] >= 255:
            dp = d[tc > 0]
            assert bool((dp == 0).any()) and bool((dp.abs() > 1).any()) and bool(((dp.abs() < 1) & (dp != 0)).any())
            assert bool((tc == -1).any())


# --------------------------------------------------------------------------------------------------- image layout
def test_head_gradient_images_equal_a_direct_loop():
    """The vectorised layout of the reference against a loop over (n, scale, d, h, w, a), at the model's (8,8,8), (4,4,4),
    (2,2,2) geometry, three classes."""
    dims, ncls, N = [(8, 8, 8), (4, 4, 4), (2, 2, 2)], 3, 2
    offs, P = C.prior_offsets(dims)
    assert P == cases.P_C64
    g = torch.Generator().manual_seed(3)
    dl, ds = torch.randn((N, P, 6), generator=g), torch.randn((N, P, ncls), generator=g)
    imgs = R.head_grad_images(dl, ds, dims, offs, ncls, fill=-7.0)
    for (D, H, W), off, img in zip(dims, offs, imgs):
        want = torch.full((N, 32, D + 2, H + 2, W + 2), -7.0)
        for n in range(N):
            for d in range(D):
                for h in range(H):
                    for w in range(W):
                        for a in range(2):
                            p = off + 2 * ((d * H + h) * W + w) + a
                            want[n, a * 6:a * 6 + 6, d + 1, h + 1, w + 1] = dl[n, p]
                            want[n, 12 + a * ncls:12 + (a + 1) * ncls, d + 1, h + 1, w + 1] = ds[n, p]
        assert torch.equal(img, want)
    assert [R.head_co(c) for c in (2, 3, 10, 16)] == [16, 32, 32, 48]


@pytest.mark.parametrize("name", C.PACK_NAMES)
def test_pack_cases_have_positives_and_odd_sizes(name):
    c = C.pack_case(name)
    assert 1 <= len(c["dims"]) <= 4 and (c["N"] * c["P"]) % 256 != 0
    tc, _, _ = OMB.match_batch(c["boxes"], c["labels"], c["priors"], c["threshold"])
    assert int((tc > 0).sum()) > 0 and int(tc.max()) <= c["ncls"] - 1 and bool((tc[1] == 0).all())
