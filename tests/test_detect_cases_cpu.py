"""The cases of tests/detect_cases.py land where their ids say - proved from the oracle side alone (torch softmax, oracle/detect.py
and the restatements of csrc/detect.hip kept next to the cases), so that an edit cannot move a case off its branch silently.
No GPU.  Also: the construction rules that make the keep-lists exact hold for every case, and the decode bound of
detect_cases.decode_reference holds for honest fp32 torch."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import boxes as OB
from tests import detect_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_IDS = C.CASE_IDS + C.REUSE_IDS


def _per_class(cid):
    """-> list over (image, class) of (probs (P,) np, restated selection, oracle trace entry), in the kernel's nc order."""
    c, r = C.case(cid), C.reference(cid)
    out = []
    for n in range(c.N):
        for k in range(1, c.ncls):
            p = r.probs[n, :, k].numpy()
            out.append((p, C.selection(p, c.min_score, 10 * c.top_k), r.trace[(n, k)]))
    return out


def test_restated_constants_are_the_kernels():
    src = open(os.path.join(ROOT, "mslesions3d_amd", "csrc", "detect.hip")).read()
    assert f"constexpr int HB = {C.HB};" in src
    assert "constexpr int PER = HB / 64;" in src and C.PER == C.HB // 64
    assert f"constexpr int SCAN_LDS = {C.SCAN_LDS};" in src and "(size_t)M * Wn <= SCAN_LDS" in src
    assert f"constexpr int FIN_LDS = {C.FIN_LDS};" in src and "total <= FIN_LDS" in src
    assert f"if (cap > {C.CAP_MAX}) return MSL_ERR_UNSUPPORTED;" in src
    assert "return (size_t)HB + 4 + P;" in src and C.sel_stride(10) == C.HB + 14
    assert "min(HB - 1, max(0, (int)(sc * (float)HB)))" in src


def test_ids_are_unique():
    assert len(set(ALL_IDS)) == len(ALL_IDS)
    assert all(i.split(":")[0] in ("sel", "nms", "fin") for i in C.CASE_IDS)


@pytest.mark.parametrize("cid", ALL_IDS)
def test_case_lands_where_its_id_says(cid):
    c, r = C.case(cid), C.reference(cid)
    e = c.expect
    cap, Wn = 10 * c.top_k, (10 * c.top_k + 63) // 64
    assert cap <= C.CAP_MAX
    pcs = _per_class(cid)
    ncand = [s["ncand"] for _, s, _ in pcs]
    assert ncand == [t[0] for _, _, t in pcs], "restated candidate rule vs oracle"
    thr = [s["thr"] for _, s, _ in pcs]
    short = [int(s["shortlist"].size) for _, s, _ in pcs]
    M = [min(n, cap) for n in ncand]
    nkept = [int(t[2].sum()) for _, _, t in pcs]
    staged = [C.scan_staged(m, Wn) for m in M]
    for (_, s, t), m, k in zip(pcs, M, short):
        assert t[1].numel() == m and k >= m
        assert np.isin(t[1].numpy(), s["shortlist"]).all(), "every ranked candidate is on the shortlist"
    k1 = c.ncls - 1
    total = [sum(nkept[n * k1:(n + 1) * k1]) for n in range(c.N)]
    resort = [C.resort_path(t, c.top_k, c.ncls) for t in total]
    count = [int(b.shape[0]) for b in r.boxes]
    got = dict(ncand=ncand, thr=thr, short=short, nkept=nkept, staged=staged, total=total, resort=resort, count=count)
    assert set(e) <= set(got)
    for key, want in e.items():
        assert got[key] == want, (cid, key, got[key], want)
    # what the id itself states
    m = re.search(r"thr-bin(\d+)", cid)
    if m:
        assert thr == [int(m.group(1))]
        assert ncand[0] > cap, "a threshold bin needs more candidates than cap"
    m = re.search(r"-lane(\d+)", cid)
    if m:
        assert thr[0] // C.PER == int(m.group(1))
    if "lowest-bin" in cid:
        assert thr[0] % C.PER == 0
    if "highest-bin" in cid:
        assert thr[0] % C.PER == C.PER - 1
    if "exact-cap" in cid:
        assert short[0] == cap
    m = re.search(r"shortlist-(\d+)", cid)
    if m:
        assert short == [int(m.group(1))]
    m = re.search(r"random-M(\d+)-topk(\d+)", cid)
    if m:
        assert M == [int(m.group(1))] and c.top_k == int(m.group(2))
        assert Wn > (M[0] + 63) // 64, "keep words beyond the last block exist"
    if cid.endswith("-staged"):
        assert staged == [True] and not C.scan_staged(M[0] + 1, Wn), "the last staged M"
    if cid.endswith("-unstaged"):
        assert staged == [False] and C.scan_staged(M[0] - 1, Wn), "the first unstaged M"
    if "global-resort" in cid:
        assert total[0] > C.FIN_LDS
    if "lds-resort" in cid:
        assert c.top_k < total[0] <= C.FIN_LDS


@pytest.mark.parametrize("cid", ALL_IDS)
def test_construction_rules(cid):
    """locs = 0, lattice priors, dyadic thresholds; for the smaller suppression cases: intersection and union are exact in fp32."""
    c = C.case(cid)
    assert not c.locs.any()
    pr = c.priors.double().numpy() * 256
    assert (pr == np.round(pr)).all() and pr[:, :3].min() >= 0 and pr[:, :3].max() <= 256 and pr[:, 3:].max() < 128
    for v in (c.max_overlap, c.min_score):
        assert v * 4096 == round(v * 4096) and np.float32(v) == v
    if cid.startswith("nms:") and c.P <= 400:
        b32 = OB.cxcycz_to_xyz(c.priors)
        b64 = OB.cxcycz_to_xyz(c.priors.double())
        assert torch.equal(b32.double(), b64)
        i32, i64 = OB.intersection(b32, b32), OB.intersection(b64, b64)
        u32 = OB.box_volume(b32)[:, None] + OB.box_volume(b32)[None, :] - i32
        u64 = OB.box_volume(b64)[:, None] + OB.box_volume(b64)[None, :] - i64
        assert torch.equal(i32.double(), i64) and torch.equal(u32.double(), u64)


# ------------------------------------------------------------------------------------------ properties of single cases
def _ranked(cid, nc=0):
    t = _per_class(cid)[nc][2]
    return t[1].numpy(), t[2].numpy()


@pytest.mark.parametrize("cid", [i for i in C.CASE_IDS if i.startswith("nms:")])
def test_suppression_cases_sort_as_chosen(cid):
    c = C.case(cid)
    ranked, _ = _ranked(cid)
    assert np.array_equal(ranked, c.rank_to_prior[:ranked.size])
    p = C.reference(cid).probs[0, :, 1].numpy()[c.rank_to_prior]
    assert (np.diff(p) < 0).all(), "strictly descending scores"


def test_chain_keeps_the_even_ranks():
    _, keep = _ranked("nms:chain130-from-rank0")
    assert np.array_equal(keep, np.arange(130) % 2 == 0) and keep.sum() == 65
    _, keep = _ranked("nms:chain130-behind-40-isolated")
    assert keep[:40].all() and np.array_equal(keep[40:], np.arange(130) % 2 == 0) and keep[40:].sum() == 65
    # the chain is one run across the block boundaries at ranks 64 and 128
    c = C.case("nms:chain130-behind-40-isolated")
    b = OB.cxcycz_to_xyz(c.priors[c.rank_to_prior])
    iou = OB.iou_matrix(b, b).numpy()
    assert iou[63, 64] > 0.25 and iou[127, 128] > 0.25
    near = np.abs(np.subtract.outer(np.arange(170), np.arange(170))) == 1
    chain = np.zeros((170, 170), dtype=bool)
    chain[40:, 40:] = near[40:, 40:]
    assert np.array_equal(iou[chain], np.full(chain.sum(), np.float32(1) / np.float32(3)))
    off = ~chain & ~np.eye(170, dtype=bool)
    assert (iou[off] == 0).all()


def test_identical_zero_size_and_max_overlap_one():
    _, keep = _ranked("nms:all-identical-one-kept")
    assert keep[0] and not keep[1:].any()
    assert _ranked("nms:identical-max-overlap-1-all-kept")[1].all()
    c = C.case("nms:zero-size-nan-iou-none-suppressed")
    b = OB.cxcycz_to_xyz(c.priors)
    assert torch.isnan(OB.iou_matrix(b, b)).all()
    assert _ranked(c.id)[1].all()


def test_three_blocks():
    c = C.case("nms:three-blocks-A-kills-C-B-spares-D")
    _, keep = _ranked(c.id)
    r = c.ranks
    assert (r["A"] // 64, r["B"] // 64, r["C"] // 64, r["D"] // 64) == (0, 1, 2, 2)
    assert keep[r["A"]] and not keep[r["B"]] and not keep[r["C"]] and keep[r["D"]]
    assert keep.sum() == 148
    b = OB.cxcycz_to_xyz(c.priors[c.rank_to_prior])
    over = OB.iou_matrix(b, b).numpy() > c.max_overlap
    np.fill_diagonal(over, False)
    pairs = {tuple(sorted(p)) for p in zip(*np.nonzero(over))}
    assert pairs == {tuple(sorted((r[a], r[b_]))) for a, b_ in (("A", "C"), ("A", "B"), ("B", "D"))}


@pytest.mark.parametrize("cid", [i for i in C.CASE_IDS if i.startswith("nms:random-M")])
def test_random_sets_suppress_within_and_across_blocks(cid):
    c = C.case(cid)
    ranked, keep = _ranked(cid)
    M = ranked.size
    if M == 1:
        assert keep.all()
        return
    assert 1 < keep.sum() < M
    b = OB.cxcycz_to_xyz(c.priors[ranked])
    over = OB.iou_matrix(b, b).numpy() > c.max_overlap
    blk = np.arange(M) // 64
    kept_suppresses = over & keep[:, None] & (np.arange(M)[:, None] < np.arange(M)[None, :])
    assert (kept_suppresses & (blk[:, None] == blk[None, :])).any(), "a suppression inside one block"
    if M >= 128:
        assert (kept_suppresses & (blk[:, None] < blk[None, :])).any(), "a suppression from an earlier block"
        # and a suppressed candidate that overlaps a later kept one: dropping the 'kept' condition would change the result
        assert (over & ~keep[:, None] & keep[None, :] & (np.arange(M)[:, None] < np.arange(M)[None, :])).any()


def test_wn64_keeps_candidates_in_the_last_word():
    ranked, keep = _ranked("nms:wn64-kept-in-last-word")
    assert ranked.size == 4090 and keep[63 * 64:].any() and not keep[63 * 64:].all() and keep.sum() > 409


def test_selection_properties():
    # the lowest of cap + 1 distinct scores drops
    c = C.case("sel:cap+1-distinct")
    ranked, keep = _ranked(c.id)
    p = C.reference(c.id).probs[0, :, 1].numpy()
    cands = c.where
    assert np.unique(p[cands]).size == 51
    assert set(cands) - set(ranked) == {cands[np.argmin(p[cands])]} and keep.all()
    # of the two equal lowest scores the higher prior index drops
    c = C.case("sel:cap+1-last-two-equal")
    ranked, _ = _ranked(c.id)
    p = C.reference(c.id).probs[0, :, 1].numpy()
    a, b = c.where[-2:]
    assert p[a] == p[b] == p[c.where].min() and np.unique(p[c.where]).size == 50
    assert set(c.where) - set(ranked) == {max(a, b)} and ranked[-1] == min(a, b)
    # all equal: the first 50 prior indices, in order
    ranked, _ = _ranked("sel:all-equal-P1000")
    assert np.array_equal(ranked, np.arange(50))
    # the run of 300 equal scores: 30 better candidates, then the run's 20 lowest prior indices in ascending order
    c = C.case("sel:tie-run-300-straddles-cut-and-tiles")
    ranked, _ = _ranked(c.id)
    p = C.reference(c.id).probs[0, :, 1].numpy()
    run = np.sort(c.where[30:330])
    assert np.unique(p[run]).size == 1 and (p[ranked[:30]] > p[run[0]]).all()
    assert np.array_equal(ranked[30:], run[:20])
    # 60 probabilities of exactly 1.0f share the clamped last bin: the 50 lowest prior indices
    c = C.case("sel:thr-bin2047-one-bin-over-cap-60-ones")
    ranked, _ = _ranked(c.id)
    p = C.reference(c.id).probs[0, :, 1].numpy()
    ones = np.nonzero(p == 1.0)[0]
    assert ones.size == 60 and np.array_equal(ranked, ones[:50])
    assert (p * np.float32(C.HB))[ones[0]] == C.HB, "the clamp is what keeps 1.0f inside the histogram"
    p = C.reference("sel:thr-bin2020-lane63-with-ones").probs[0, :, 1].numpy()
    assert (p == 1.0).sum() == 13
    # probability == min_score is no candidate
    c = C.case("sel:score-equals-min-score")
    p = C.reference(c.id).probs[0, :, 1].numpy()
    assert (p == np.float32(c.min_score)).sum() == 40 and (p > np.float32(c.min_score)).sum() == 12


def test_special_logits():
    p = C.reference("sel:nan-logits").probs[0, :, 1].numpy()
    assert np.isnan(p).sum() == 20 and int(torch.isfinite(C.case("sel:nan-logits").scores).sum()) < 260
    p = C.reference("sel:inf-logits").probs[0, :, 1].numpy()
    assert np.isnan(p).sum() == 16 and (p == 1.0).sum() == 4 and (p == 0.0).sum() == 4
    p = C.reference("sel:logits-pm100").probs[0, :, 1].numpy()
    tiny = np.float32(np.finfo(np.float32).tiny)
    assert ((p > 0) & (p < tiny)).sum() == 8, "exp(-100) is a subnormal probability and a candidate at min_score = 0"
    assert (p == 1.0).sum() == 8 and (p == 0.5).sum() == 8 and (p == 0.0).sum() == 130 - 44


def test_finalize_properties():
    r = C.reference("fin:batch3-over-placeholder-under")
    assert r.boxes[1].tolist() == [[0, 0, 0, 1, 1, 1]] and r.scores[1].tolist() == [0] and r.labels[1].tolist() == [0]
    assert r.prior[1].tolist() == [-1]
    assert (np.diff(r.scores[0].numpy()) <= 0).all() and set(r.labels[0].tolist()) == {1, 2}
    for cid in ("fin:c3-total-below-topk-class-major", "fin:c3-total-equals-topk-class-major"):
        r = C.reference(cid)
        lab, sc = r.labels[0].numpy(), r.scores[0].numpy()
        assert np.array_equal(lab, np.sort(lab)) and set(lab) == {1, 2}
        assert sc[lab == 1].max() < sc[lab == 2].min(), "class-major is NOT the score order: a re-sort would show"
    r = C.reference("fin:c3-total-topk+1-resorted")
    lab, sc = r.labels[0].numpy(), r.scores[0].numpy()
    assert (np.diff(sc) < 0).all() and lab.tolist() == [2] * 5 + [1] * 3
    r = C.reference("fin:c3-equal-scores-class1-first")
    sc = r.scores[0].numpy()
    assert r.labels[0].tolist() == [1, 2] * 3 and (sc[0::2] == sc[1::2]).all() and np.array_equal(r.prior[0][0::2], r.prior[0][1::2])
    for cid in ("fin:c4-topk300-total9000-global-resort", "fin:c4-topk200-total6000-lds-resort"):
        r = C.reference(cid)
        sc, lab = r.scores[0].numpy(), r.labels[0].numpy()
        assert set(lab) == {1, 2, 3} and (np.diff(sc) <= 0).any() and (np.diff(sc) == 0).any(), "equal scores reach the top-k"
        tie = np.nonzero(np.diff(sc) == 0)[0]
        assert (lab[tie] != lab[tie + 1]).any(), "and some of them across classes"


def test_reuse_sequence():
    n = [C.case(i).expect["ncand"][0] for i in C.REUSE_IDS]
    assert n == [300, 7, 0] and n[0] > 10 * C.case(C.REUSE_IDS[0]).top_k
    assert len({(C.case(i).P, C.case(i).ncls, C.case(i).top_k, C.case(i).N) for i in C.REUSE_IDS}) == 1
    assert C.reference("reuse:none").prior[0].tolist() == [-1]


def test_decode_bound_holds_for_fp32_torch():
    c = C.decode_case()
    g = c.locs[0]
    assert g[:, 3:].abs().max() == 10 and (g[0, 3:] == 10).all() and (g[1, 3:] == -10).all() and (g != 0).sum() > 6 * 250
    ref, bound = C.decode_reference(g, c.priors)
    got = OB.cxcycz_to_xyz(OB.decode(g, c.priors))
    assert got.dtype == torch.float32
    err = np.abs(got.double().numpy() - ref)
    assert (err <= bound).all(), (err / bound).max()
    # "a small multiple of eps times |c| + size": never more than 4 U (|c*| + size*), and tight enough to see a wrong operation
    scale = np.abs((ref[:, :3] + ref[:, 3:]) / 2) + (ref[:, 3:] - ref[:, :3])
    assert (bound <= 4 * C.U * np.concatenate([scale, scale], axis=1)).all()
    wrong = OB.cxcycz_to_xyz(torch.cat([g[:, :3] * c.priors[:, 3:] / 10 + c.priors[:, :3],
                                        torch.exp(g[:, 3:] * 0.2) * c.priors[:, 3:] * (1 + 2e-6)], dim=1))
    assert (np.abs(wrong.double().numpy() - ref) > bound).any()
