"""Case tables of tests/test_gpu_detect.py (shared with tests/test_detect_cases_cpu.py, which proves from the oracle side alone
that every case lands on the branch of csrc/detect.hip its id names, so an edit cannot move a case silently).

Plain data plus builders.  ``case(id)`` -> namespace with N, P, ncls, top_k, min_score, max_overlap, priors (P, 6), locs
(N, P, 6), scores (N, P, ncls) (fp32 CPU tensors) and ``expect``: the machine-readable form of the id - per (image, class)
lists ``ncand``, ``thr`` (threshold bin), ``short`` (shortlist length), ``nkept``, ``staged``; per image ``total`` and
``resort`` (None / "lds" / "global").  Every key that is present is asserted on the CPU.

Keep-lists are exact by construction: ``locs = 0`` (the decoded box IS the prior's box), centres on multiples of 1/256 and
sizes of at most 7 significant bits, so that intersection, volumes and union are exact in fp32 and only the final division
rounds; ``max_overlap`` and ``min_score`` are dyadic.  Scores come from logits (0, x[, x2, ...]).

Restated from csrc/detect.hip, next to the cases: the score histogram (``score_bin``), the threshold-bin rule, the
``M * Wn`` staging predicate of the scan, the LDS limit of the cross-class re-sort and the layout of ``select_ws``."""
import functools
import types

import numpy as np
import torch

from oracle import detect as OD

F32 = np.float32
HB = 2048            # histogram bins over [0, 1]
PER = HB // 64       # bins per lane of the threshold search: lane l owns [l * PER, (l + 1) * PER)
SCAN_LDS = 6144      # the scan stages the mask rows in LDS when M * Wn <= SCAN_LDS
FIN_LDS = 8192       # finalize re-sorts from LDS when total <= FIN_LDS
CAP_MAX = 4096       # cap = 10 * top_k beyond this is refused


def sel_stride(P):
    """ints of select_ws per (image, foreground class): [hist HB | threshold bin | shortlist count | pad 2 | shortlist P]"""
    return HB + 4 + P


def score_bin(p):
    """min(HB - 1, max(0, (int)(p * HB))) in fp32 (the product with a power of two is exact)."""
    p = np.asarray(p, dtype=F32)
    return np.clip((p * F32(HB)).astype(np.int64), 0, HB - 1)


def threshold_bin(hist, cap):
    """The highest bin b with #(candidates in bins >= b) >= cap; bin 0 with fewer than cap candidates."""
    above = np.cumsum(hist[::-1])[::-1]
    hit = np.nonzero(above >= cap)[0]
    return int(hit.max()) if hit.size else 0


def selection(probs_c, min_score, cap):
    """What the histogram, threshold and compaction launches leave for one (image, class): probs_c (P,) fp32."""
    p = np.asarray(probs_c, dtype=F32)
    cand = p > F32(min_score)  # strict; NaN is never a candidate
    idx = np.nonzero(cand)[0]
    bins = score_bin(p[idx])
    hist = np.bincount(bins, minlength=HB)
    thr = threshold_bin(hist, cap)
    return dict(ncand=int(idx.size), hist=hist, thr=thr, shortlist=idx[bins >= thr])


def scan_staged(M, Wn):
    return M * Wn <= SCAN_LDS


def resort_path(total, top_k, ncls):
    if not (total > top_k and ncls > 2):
        return None
    return "lds" if total <= FIN_LDS else "global"


# ---------------------------------------------------------------------------------------------------------------- geometry
def lattice_boxes(n, seed, size_lo=24, size_hi=64, c_lo=64, c_hi=192):
    """n centre-size boxes: centres k/256, sizes k/256 with k < 128 (7 significant bits)."""
    rng = np.random.RandomState(seed)
    c = rng.randint(c_lo, c_hi + 1, size=(n, 3))
    s = rng.randint(size_lo, size_hi + 1, size=(n, 3))
    return (np.concatenate([c, s], axis=1) / 256.0).astype(F32)


def isolated_boxes(n, x=200):
    """n boxes of size 2/256 on a (y, z) grid of pitch 3/256 at one x: no two overlap."""
    j = np.arange(n)
    out = np.empty((n, 6))
    out[:, 0] = x
    out[:, 1] = 4 + 3 * (j % 81)
    out[:, 2] = 4 + 3 * (j // 81)
    out[:, 3:] = 2
    assert out[:, 2].max() <= 244
    return (out / 256.0).astype(F32)


def chain_boxes(n, x0=20):
    """n boxes of width 2/256 at pitch 1/256 along x (y = z = 250/256): neighbours have IoU 1/3, all other pairs 0."""
    out = np.empty((n, 6))
    out[:, 0] = x0 + np.arange(n)
    out[:, 1:3] = 250
    out[:, 3:] = 2
    return (out / 256.0).astype(F32)


# ------------------------------------------------------------------------------------------------------------------ scores
def logit(p):
    p = np.asarray(p, dtype=np.float64)
    return np.log(p / (1.0 - p)).astype(F32)


def in_bin(b, k, lo=0.1, hi=0.9):
    """k logits x whose softmax((0, x))[1] lie, distinct, inside histogram bin b (asserted on the CPU)."""
    return logit((b + np.linspace(lo, hi, k)) / HB)


def in_bins(b_lo, b_hi, k):
    """k logits spread evenly over the bins b_lo .. b_hi (inclusive), distinct."""
    return logit(np.linspace(b_lo + 0.25, b_hi + 0.75, k) / HB)


def descending(m, hi=2.0, lo=-2.0):
    """m strictly descending logits (probabilities about 0.88 .. 0.12)."""
    return np.linspace(hi, lo, m).astype(F32) if m > 1 else np.array([hi], dtype=F32)


def _ns(cid, priors, scores, top_k, min_score, max_overlap, expect, locs=None, note=""):
    priors = torch.from_numpy(np.ascontiguousarray(priors, dtype=F32))
    scores = torch.from_numpy(np.ascontiguousarray(scores, dtype=F32))
    if scores.dim() == 2:
        scores = scores[None]
    N, P, ncls = scores.shape
    assert priors.shape == (P, 6)
    locs = torch.zeros((N, P, 6), dtype=torch.float32) if locs is None else torch.from_numpy(np.ascontiguousarray(locs, dtype=F32))
    return types.SimpleNamespace(id=cid, N=N, P=P, ncls=ncls, top_k=top_k, min_score=float(min_score),
                                 max_overlap=float(max_overlap), priors=priors, locs=locs, scores=scores, expect=expect,
                                 note=note)


def two_class(x):
    """logits (0, x) per prior"""
    x = np.asarray(x, dtype=F32)
    return np.stack([np.zeros_like(x), x], axis=1)


# ------------------------------------------------------------------------------------- selection and rank (ncls 2, no NMS)
NOT_CAND = F32(-4.0)  # softmax((0, -4))[1] = 0.018: below the min_score of every case that uses it


def _sel(cid, P, x_cand, expect, top_k=5, min_score=0.0625, seed=0, x_rest=None, where=None):
    """P priors; the candidates' logits ``x_cand`` go to the prior indices ``where`` (default: a seeded choice that always
    holds the first and the last prior), every other prior gets ``x_rest`` (default: no candidate)."""
    rng = np.random.RandomState(1000 + seed)
    x_cand = np.asarray(x_cand, dtype=F32)
    k = x_cand.size
    if where is None:
        if k >= 2 and P >= 2:
            mid = rng.choice(np.arange(1, P - 1), size=k - 2, replace=False) if k > 2 else np.zeros(0, dtype=np.int64)
            where = np.concatenate([[0, P - 1], mid]).astype(np.int64)
            rng.shuffle(where)
        else:
            where = np.arange(k)
    x = np.full(P, NOT_CAND, dtype=F32) if x_rest is None else np.asarray(x_rest, dtype=F32).copy()
    x[where] = x_cand
    c = _ns(cid, lattice_boxes(P, 7 + seed), two_class(x), top_k, min_score, 1.0, expect)
    c.where = np.asarray(where)
    return c


def _sel_cases():
    out = {}
    cap = 50  # top_k = 5

    def add(cid, fn):
        out[cid] = fn

    for P in (1, 255, 256, 257):
        k = 1 if P == 1 else 30
        add(f"sel:below-cap-P{P}", lambda P=P, k=k: _sel(f"sel:below-cap-P{P}", P, descending(k), dict(ncand=[k], thr=[0], short=[k], nkept=[k]), seed=P))
    add("sel:exactly-cap", lambda: _sel("sel:exactly-cap", 300, descending(cap),
                                        dict(ncand=[cap], short=[cap], nkept=[cap]), seed=1))
    add("sel:cap+1-distinct", lambda: _sel("sel:cap+1-distinct", 300, descending(cap + 1),
                                           dict(ncand=[cap + 1], nkept=[cap]), seed=2))

    def last_two_equal():
        x = descending(cap + 1)
        x[-1] = x[-2]
        return _sel("sel:cap+1-last-two-equal", 300, x, dict(ncand=[cap + 1], nkept=[cap]), seed=3)
    add("sel:cap+1-last-two-equal", last_two_equal)

    def thr_case(cid, b, n_above, n_in, n_below, b_top, seed, min_score=0.0625, extra_top=(), b_floor=None):
        """n_above candidates in bins (b, b_top], n_in inside bin b (the cap-th best is one of them), n_below in lower bins"""
        def build():
            floor = max(1, int(min_score * HB) + 1) if b_floor is None else b_floor
            xs = [np.asarray(extra_top, dtype=F32), in_bins(b + 1, b_top, n_above - len(extra_top)), in_bin(b, n_in)]
            if n_below:
                xs.append(in_bins(floor, b - 1, n_below))
            x = np.concatenate(xs)
            n = x.size
            # at min_score = 0 the other priors get exp(-200) = 0: still no candidate
            return _sel(cid, 600, x, dict(ncand=[n], thr=[b], short=[n_above + n_in], nkept=[cap]), min_score=min_score, seed=seed,
                        x_rest=None if min_score > 0 else np.full(600, -200.0))
        add(cid, build)

    # lane 0 owns bins 0 .. 31: the cap-th probability is below 1/64, so min_score = 0
    thr_case("sel:thr-bin20-lane0", 20, 45, 12, 300, 2000, 4, min_score=0.0, b_floor=0)
    # lane 63 owns bins 2016 .. 2047; probabilities of exactly 1.0f (logits 100 and 30) are clamped into bin 2047
    thr_case("sel:thr-bin2020-lane63-with-ones", 2020, 44, 10, 400, 2046, 5, extra_top=[100.0] * 7 + [30.0] * 6)
    # lane boundary: bin 640 is the LAST bin lane 20 looks at, bin 639 the FIRST of lane 19.  The count reaches cap exactly in
    # the threshold bin at 640 (44 + 6) and overshoots it at 639 (44 + 9)
    thr_case("sel:thr-bin640-lane20-lowest-bin-exact-cap", 640, 44, 6, 300, 1900, 6)
    thr_case("sel:thr-bin639-lane19-highest-bin", 639, 44, 9, 300, 1900, 7)

    def ones60():
        x = np.concatenate([np.full(30, 100.0), np.full(30, 20.0), in_bins(200, 2040, 200)]).astype(F32)
        return _sel("sel:thr-bin2047-one-bin-over-cap-60-ones", 600, x, dict(ncand=[260], thr=[2047], short=[60], nkept=[cap]), seed=8)
    add("sel:thr-bin2047-one-bin-over-cap-60-ones", ones60)

    add("sel:all-equal-P1000", lambda: _sel("sel:all-equal-P1000", 1000, np.full(1000, 1.0),
                                            dict(ncand=[1000], short=[1000], nkept=[cap]), seed=9))

    def tie_run():
        b = int(score_bin(torch.softmax(torch.tensor([0.0, 0.5]), 0)[1].numpy()))
        x = np.concatenate([in_bins(b + 40, 1900, 30), np.full(300, 0.5), in_bins(200, b - 40, 250)]).astype(F32)
        return _sel("sel:tie-run-300-straddles-cut-and-tiles", 700, x, dict(ncand=[580], thr=[b], short=[330], nkept=[cap]), seed=10)
    add("sel:tie-run-300-straddles-cut-and-tiles", tie_run)

    for K in (256, 257):
        thr_case(f"sel:shortlist-{K}", 900, 49, K - 49, 200, 1900, 11 + K)

    def equals_min():
        # logits (0, 0) give exactly 0.5 = min_score: no candidate (strict >); 12 priors lie above
        x = np.concatenate([descending(12, 2.0, 0.25), np.zeros(40)]).astype(F32)
        return _sel("sel:score-equals-min-score", 200, x, dict(ncand=[12], thr=[0], short=[12], nkept=[12]), min_score=0.5, seed=12)
    add("sel:score-equals-min-score", equals_min)

    def nan_logits():
        c = _sel("sel:nan-logits", 130, descending(20), dict(ncand=[20], thr=[0], short=[20], nkept=[20]), seed=13)
        free = np.setdiff1d(np.arange(130), c.where)
        nan = float("nan")
        for k, pair in enumerate([(0.0, nan), (nan, 0.0), (nan, nan), (nan, 5.0), (5.0, nan)] * 4):
            c.scores[0, free[k * 3]] = torch.tensor(pair)
        return c
    add("sel:nan-logits", nan_logits)

    def inf_logits():
        # torch: (0, -inf) -> 0, (-inf, 0) -> 1; (0, inf), (inf, 0), (inf, inf), (-inf, -inf) -> NaN
        c = _sel("sel:inf-logits", 130, descending(20), dict(ncand=[24], thr=[0], short=[24], nkept=[24]), seed=14)
        free = np.setdiff1d(np.arange(130), c.where)
        inf = float("inf")
        for k, pair in enumerate([(0.0, -inf), (-inf, 0.0), (0.0, inf), (inf, 0.0), (inf, inf), (-inf, -inf)] * 4):
            c.scores[0, free[k * 3]] = torch.tensor(pair)
        return c
    add("sel:inf-logits", inf_logits)

    def pm100():
        # (0, 100) -> 1; (0, -100) -> 3.8e-44 (subnormal); (100, 0) likewise; (-100, 0) -> 1; (100, 100), (-100, -100) -> 0.5
        c = _sel("sel:logits-pm100", 130, descending(20), dict(ncand=[44], thr=[0], short=[44], nkept=[44]), min_score=0.0, seed=15,
                 x_rest=np.full(130, -200.0))  # exp(-200) underflows to 0: no candidate even at min_score = 0
        free = np.setdiff1d(np.arange(130), c.where)
        for k, pair in enumerate([(0.0, 100.0), (0.0, -100.0), (100.0, 0.0), (-100.0, 0.0), (100.0, 100.0), (-100.0, -100.0)] * 4):
            c.scores[0, free[k * 3]] = torch.tensor(pair)
        return c
    add("sel:logits-pm100", pm100)
    return out


# ------------------------------------------------------------------------------------------------------------- suppression
def _nms(cid, geom, expect, top_k=20, max_overlap=0.25, seed=0, min_score=0.0625):
    """``geom`` (M, 6) centre-size boxes in RANK order: rank r goes to prior perm[r] with the r-th of M strictly descending
    scores, so the sorted order is known and differs from the prior order."""
    M = geom.shape[0]
    perm = np.random.RandomState(2000 + seed).permutation(M)
    priors = np.empty((M, 6), dtype=F32)
    x = np.empty(M, dtype=F32)
    priors[perm] = geom
    x[perm] = descending(M)
    c = _ns(cid, priors, two_class(x), top_k, min_score, max_overlap, expect)
    c.rank_to_prior = perm
    return c


def three_block_geometry():
    """150 candidates in rank order.  D - B - A - C sit along x at pitch 1/256, width 2/256 (neighbours IoU 1/3): A (rank 5,
    block 0) overlaps B and C; B (rank 70, block 1) overlaps A and D; C (rank 130) and D (rank 140) are in block 2.  The
    rest is isolated.  Greedy result: A kept, B suppressed by A, C suppressed by A, D kept (B is not kept)."""
    geom = isolated_boxes(150)
    four = chain_boxes(4)  # positions 0..3 = D, B, A, C
    ranks = dict(D=140, B=70, A=5, C=130)
    for pos, name in enumerate("DBAC"):
        geom[ranks[name]] = four[pos]
    return geom, ranks


def _nms_cases():
    out = {}

    def add(cid, fn):
        out[cid] = fn

    add("nms:chain130-from-rank0", lambda: _nms("nms:chain130-from-rank0", chain_boxes(130),
                                                 dict(ncand=[130], nkept=[65], staged=[True]), seed=1))
    add("nms:chain130-behind-40-isolated", lambda: _nms("nms:chain130-behind-40-isolated",
                                                         np.concatenate([isolated_boxes(40), chain_boxes(130)]),
                                                         dict(ncand=[170], nkept=[105], staged=[True]), seed=2))
    ident = np.tile(np.array([[128, 128, 128, 32, 32, 32]], dtype=F32) / 256, (100, 1))
    add("nms:all-identical-one-kept", lambda: _nms("nms:all-identical-one-kept", ident, dict(ncand=[100], nkept=[1]), seed=3))
    add("nms:identical-max-overlap-1-all-kept", lambda: _nms("nms:identical-max-overlap-1-all-kept", ident,
                                                              dict(ncand=[100], nkept=[100]), max_overlap=1.0, seed=4))
    zero = lattice_boxes(100, 5)
    zero[:, 3:] = 0
    zero[:, :3] = zero[0, :3]  # the same point: intersection 0, union 0, IoU NaN
    add("nms:zero-size-nan-iou-none-suppressed", lambda: _nms("nms:zero-size-nan-iou-none-suppressed", zero,
                                                               dict(ncand=[100], nkept=[100]), seed=5))
    for M in (1, 63, 64, 65, 128, 129):  # cap 200, Wn = 4 > block count (<= 3)
        add(f"nms:random-M{M}-topk20", lambda M=M: _nms(f"nms:random-M{M}-topk20", lattice_boxes(M, 31), dict(ncand=[M], staged=[True]), seed=M))
    for M, top_k, st in ((384, 100, True), (385, 100, False), (96, 409, True), (97, 409, False)):
        cid = f"nms:random-M{M}-topk{top_k}-{'staged' if st else 'unstaged'}"
        add(cid, lambda M=M, top_k=top_k, st=st, cid=cid: _nms(cid, lattice_boxes(M, 32), dict(ncand=[M], staged=[st]), top_k=top_k, seed=M))

    def three():
        geom, ranks = three_block_geometry()
        c = _nms("nms:three-blocks-A-kills-C-B-spares-D", geom, dict(ncand=[150], nkept=[148], staged=[True]), seed=6)
        c.ranks = ranks
        return c
    add("nms:three-blocks-A-kills-C-B-spares-D", three)
    # Wn = 64 (top_k 409, cap 4090): 4090 candidates, small boxes, kept candidates in the last keep word
    add("nms:wn64-kept-in-last-word", lambda: _nms("nms:wn64-kept-in-last-word", lattice_boxes(4090, 33, size_lo=8, size_hi=24, c_lo=16, c_hi=240),
                                                   dict(ncand=[4090], staged=[False]), top_k=409, max_overlap=0.5, seed=7))
    return out


# ---------------------------------------------------------------------------------------------------------------- finalize
def _fin_cases():
    out = {}

    def add(cid, fn):
        out[cid] = fn

    def three_class(P, c1, c2, both=()):
        """logits (0, x1, x2): priors in ``c1`` {prior: x} are candidates of class 1 only, ``c2`` of class 2 only."""
        s = np.tile(np.array([0.0, -3.0, -3.0], dtype=F32), (P, 1))
        for p, x in c1.items():
            s[p, 1] = x
        for p, x in c2.items():
            s[p, 2] = x
        for p, x in both:
            s[p, 1] = s[p, 2] = x
        return s

    def batch3():
        P = 64
        img0 = three_class(P, {3: 0.5, 10: 0.75, 17: 1.0, 40: 1.25, 63: 1.5}, {0: 0.625, 9: 0.875, 30: 1.125, 50: 1.375})
        img1 = three_class(P, {}, {})
        img2 = three_class(P, {5: 0.5, 20: 1.5}, {41: 1.0})
        return _ns("fin:batch3-over-placeholder-under", lattice_boxes(P, 41), np.stack([img0, img1, img2]), 6, 0.25, 1.0,
                   dict(ncand=[5, 4, 0, 0, 2, 1], total=[9, 0, 3], resort=["lds", None, None], count=[6, 1, 3]))
    add("fin:batch3-over-placeholder-under", batch3)

    low = {2: 0.25, 11: 0.375, 23: 0.3125, 37: 0.4375}           # class 1: probabilities about 0.55
    high = {5: 2.0, 8: 2.5, 19: 2.25, 30: 1.75, 44: 3.0}         # class 2: about 0.85 .. 0.95

    def cmajor(cid, n2, top_k, resort):
        def build():
            c2 = dict(list(high.items())[:n2])
            total = len(low) + n2
            return _ns(cid, lattice_boxes(48, 42), three_class(48, low, c2), top_k, 0.25, 1.0,
                       dict(ncand=[len(low), n2], total=[total], resort=[resort], count=[min(total, top_k)]))
        add(cid, build)
    cmajor("fin:c3-total-below-topk-class-major", 3, 10, None)
    cmajor("fin:c3-total-equals-topk-class-major", 4, 8, None)
    cmajor("fin:c3-total-topk+1-resorted", 5, 8, "lds")

    def equal_scores():
        both = [(p, x) for p, x in zip((1, 4, 9, 16, 25, 36, 38, 39, 12, 20), np.linspace(1.0, 2.0, 10))]
        return _ns("fin:c3-equal-scores-class1-first", lattice_boxes(40, 43), three_class(40, {}, {}, both), 6, 0.25, 1.0,
                   dict(ncand=[10, 10], total=[20], resort=["lds"], count=[6]))
    add("fin:c3-equal-scores-class1-first", equal_scores)

    def big(cid, top_k, resort):
        def build():
            P = 3072
            rng = np.random.RandomState(44)
            s = np.zeros((P, 4), dtype=F32)
            s[:, 1:] = rng.randint(0, 65, size=(P, 3)) / 16.0  # a coarse grid: equal scores inside and across classes
            cap = 10 * top_k
            return _ns(cid, lattice_boxes(P, 45), s, top_k, 0.0, 1.0,
                       dict(ncand=[P] * 3, nkept=[cap] * 3, total=[3 * cap], resort=[resort], count=[top_k]))
        add(cid, build)
    big("fin:c4-topk300-total9000-global-resort", 300, "global")
    big("fin:c4-topk200-total6000-lds-resort", 200, "lds")
    return out


# ------------------------------------------------------------------------------------------------------------------ decode
def decode_case():
    """Random non-zero locs at P = 257: centre offsets within +-3, size logits within +-10 with both ends present."""
    P = 257
    rng = np.random.RandomState(51)
    g = np.empty((1, P, 6), dtype=F32)
    g[0, :, :3] = rng.uniform(-3, 3, size=(P, 3))
    g[0, :, 3:] = rng.uniform(-10, 10, size=(P, 3))
    g[0, 0, 3:] = 10.0
    g[0, 1, 3:] = -10.0
    g[0, 2] = 0.0
    x = rng.uniform(-2, 2, size=P).astype(F32)
    return _ns("dec:random-locs-P257", lattice_boxes(P, 52), two_class(x), 5, 0.0625, 0.5, {}, locs=g)


U = 2.0 ** -24  # unit roundoff of fp32


def decode_reference(locs, priors):
    """-> (corner boxes (P, 6) in float64 from the fp32 inputs, bound (P, 6)).

    The kernel (and the oracle's fp32 decode) computes, per axis, with every operation rounded once (relative error <= U):
      cx = fl(fl(fl(g * s) / 10) + c)        |cx - cx*| <= 2 U |g s / 10| + U |cx*|
      sz = fl(exp~(fl(g / 5)) * s)           fl(g / 5) moves the exponent by <= U |g / 5|, i.e. the exponential by that
                                             relative amount; exp~ is within 1 ulp (<= 2 U relative) in both the device's
                                             expf and torch's; the product adds U:  |sz - sz*| <= (|g| / 5 + 3) U sz*
      h = sz / 2 (exact),  corner = fl(cx -+ h)   |corner - corner*| <= |cx - cx*| + |sz - sz*| / 2 + U |corner*|
    so  bound = (1 + 2^-10) U (2 |g s / 10| + |cx*| + (|g| / 5 + 3) sz* / 2 + |corner*|); the factor in front covers the
    second-order terms.  With |g| <= 10 that is at most U (2.2 |c| + 3.1 sz*): a small multiple of U times |c| + size."""
    g = locs.double().numpy()
    pr = priors.double().numpy()
    gc, gs, c, s = g[:, :3], g[:, 3:], pr[:, :3], pr[:, 3:]
    cx = gc * s / 10.0 + c
    sz = np.exp(gs / 5.0) * s
    e_c = 2 * np.abs(gc * s / 10.0) + np.abs(cx)
    e_h = (np.abs(gs) / 5.0 + 3.0) * sz / 2.0
    lo, hi = cx - sz / 2, cx + sz / 2
    ref = np.concatenate([lo, hi], axis=1)
    bound = (1 + 2.0 ** -10) * U * np.concatenate([e_c + e_h + np.abs(lo), e_c + e_h + np.abs(hi)], axis=1)
    return ref, bound


# ------------------------------------------------------------------------------------------------------------------- tables
_BUILDERS = {}
_BUILDERS.update(_sel_cases())
_BUILDERS.update(_nms_cases())
_BUILDERS.update(_fin_cases())
CASE_IDS = list(_BUILDERS)
# the three inputs that share one poisoned workspace, in this order: many candidates, few, none (same N, P, ncls, top_k)
REUSE_IDS = ["reuse:many", "reuse:few", "reuse:none"]


def _reuse(cid):
    geom = lattice_boxes(300, 61)
    x = {"reuse:many": descending(300), "reuse:few": np.concatenate([descending(7), np.full(293, NOT_CAND)]),
         "reuse:none": np.full(300, NOT_CAND)}[cid].astype(F32)
    x = x[np.random.RandomState(62).permutation(300)]
    n = int((x > NOT_CAND).sum())
    return _ns(cid, geom, two_class(x), 20, 0.0625, 0.25, dict(ncand=[n]))


@functools.lru_cache(maxsize=None)
def case(cid):
    if cid in REUSE_IDS:
        return _reuse(cid)
    c = _BUILDERS[cid]()
    assert c.id == cid, (c.id, cid)
    return c


@functools.lru_cache(maxsize=None)
def reference(cid):
    """The oracle's answer for a case, computed once and shared: detections, per-(image, class) trace, probabilities."""
    c = case(cid)
    trace = {}
    b, l, s, pi = OD.detect_objects(c.locs, c.scores, c.priors, c.min_score, c.max_overlap, c.top_k,
                                    return_prior_index=True, trace=trace)
    return types.SimpleNamespace(boxes=b, labels=l, scores=s, prior=pi, trace=trace, probs=torch.softmax(c.scores, dim=2))
