"""Cases of tests/test_gpu_multibox.py, built from seeded generators (nothing stored, no network needed).  What each case
promises - real ties, IoUs exactly on a threshold, duplicate claims, a mining cut inside a run of equal losses - is asserted
by tests/test_multibox_ref_cpu.py on the oracle, not assumed.

Matching runs on synthetic priors on a dyadic grid: centres, sizes and ground-truth corners are multiples of 2^-5, so every
corner is a multiple of 2^-6 and every volume, intersection and union is a multiple of 2^-18 below 2: exact in fp32.  Equal
geometry then gives bit-equal IoU, and ties are ties for every implementation.  All lengths below are in units of 2^-5."""
import functools
import math

import torch

U = 2.0 ** -5
MATCH_P = (1, 255, 1024, 1025, 4096, 4097, 9223)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def dyadic_priors(P, seed):
    """(P, 6) centre-size priors: centres 0..32, sizes 4..16 (units of 2^-5), independent per axis."""
    g = _gen(seed)
    c = torch.randint(0, 33, (P, 3), generator=g)
    s = torch.randint(4, 17, (P, 3), generator=g)
    return (torch.cat([c, s], dim=1).float() * U).contiguous()


def random_boxes(n, seed, n_labels=3):
    """n corner boxes with dyadic corners inside [0, 1], sizes 2..8, labels 1..n_labels."""
    g = _gen(seed)
    s = torch.randint(2, 9, (n, 3), generator=g)
    lo = (torch.rand((n, 3), generator=g) * (33 - s).float()).floor().long()
    boxes = torch.cat([lo, lo + s], dim=1).float() * U
    return boxes, torch.randint(1, n_labels + 1, (n,), generator=g)


def _box(centre, size):
    c, s = torch.tensor(centre, dtype=torch.float32), torch.tensor(size, dtype=torch.float32)
    return torch.cat([c - s / 2, c + s / 2]) * U


def _prior(centre, size):
    return torch.tensor(list(centre) + list(size), dtype=torch.float32) * U


def _tie_slots(P):
    """Groups of prior indices that share one best IoU.  match_object_best_kernel: thread t visits t, t + 1024, ... in trips
    of 4 * 1024.  (900, 1024): different threads of one trip, the higher index in the lower thread (the LDS reduction's index
    rule decides).  (0, 4096) / (200, 4296): one thread, two trips (its strict > decides).  (3000, 5000, 7000): three-way."""
    if P < 255:
        return []
    slots = [(10, 200)] if P < 1025 else [(900, 1024)]
    if P >= 4097:
        slots.append((0, 4096) if P < 4297 else (200, 4296))
    if P >= 9223:
        slots.append((3000, 5000, 7000))
    return slots


# centre of the tied box of every slot and the shifts (of size-8 cubes) that give each tied prior IoU 7/9
_TIE_CENTRES = ((8, 24, 8), (24, 24, 8), (24, 24, 24))
_TIE_SHIFTS = ((-1, 0, 0), (1, 0, 0), (0, 0, 1))
# IoU exactly 1/2: extents 6 shifted by 2 (4 / 8).  IoU exactly 1/4: extents 10 shifted by 6 (4 / 16).
_THR = dict(half=dict(centre=(6, 6, 6), size=(6, 8, 8), shift=2, exact=20, hit=21, value=0.5),
            quarter=dict(centre=(8, 6, 22), size=(10, 8, 8), shift=6, exact=22, hit=23, value=0.25))


def special_image(priors):
    """Plants priors into ``priors`` (in place) and returns the image that goes with them:
    (boxes, labels, promises).  Objects: one tied box per slot of ``_tie_slots``; two boxes whose IoU with one planted prior
    is exactly 1/2 and 1/4 (each also has an identical prior, which the force-match takes); a 1^3 box that no prior overlaps
    by more than 1/64; two identical boxes with labels 1 and 2; four random boxes."""
    P = priors.shape[0]
    boxes, labels, prom = [], [], dict(ties=[], thr=[], unmatched=[], dup=[])
    for k, slot in enumerate(_tie_slots(P)):
        c = _TIE_CENTRES[k]
        for idx, sh in zip(slot, _TIE_SHIFTS):
            priors[idx] = _prior([c[a] + sh[a] for a in range(3)], (8, 8, 8))
        prom["ties"].append((len(boxes), tuple(slot)))
        boxes.append(_box(c, (8, 8, 8)))
        labels.append(1 + k % 3)
    for t in _THR.values():
        priors[t["exact"]] = _prior(t["centre"], t["size"])
        priors[t["hit"]] = _prior((t["centre"][0] + t["shift"],) + t["centre"][1:], t["size"])
        prom["thr"].append((t["hit"], t["value"], len(boxes)))
        boxes.append(_box(t["centre"], t["size"]))
        labels.append(2)
    prom["unmatched"].append(len(boxes))
    boxes.append(_box((15.5, 15.5, 15.5), (1, 1, 1)))
    labels.append(3)
    prom["dup"].append((len(boxes), len(boxes) + 1))
    boxes += [_box((20, 8, 20), (6, 6, 8))] * 2
    labels += [1, 2]
    rb, rl = random_boxes(4, 78)
    return torch.cat([torch.stack(boxes), rb]), torch.cat([torch.tensor(labels), rl]), prom


def _image(kind, priors, seed):
    empty = (torch.zeros((0, 6)), torch.zeros((0,), dtype=torch.long), {})
    if kind == "none":
        return empty
    if kind == "one":
        return random_boxes(1, seed) + ({},)
    if kind == "dozen":
        return random_boxes(12, seed) + ({},)
    if kind == "many300":  # the o += 256 loop of match_force_kernel runs twice
        return random_boxes(300, seed) + (dict(many=True),)
    if kind == "dozen_dup":  # two identical boxes with labels 1 and 2 among a dozen
        b, l = random_boxes(12, seed)
        b[7], l[3], l[7] = b[3], 1, 2
        return b, l, dict(dup=[(3, 7)])
    assert kind == "special"
    return special_image(priors)


SOFT, HARD_Q, HARD_H = [0.25, 0.5], 0.25, 0.5
# name -> (P, per-image object sets, threshold).  Every P with N = 1 or 3; "special" needs P >= 255.
_MATCH = {
    "P1_one_soft": (1, ["one"], SOFT),
    "P1_dozen_none_one_hardH": (1, ["dozen", "none", "one"], HARD_H),
    "P255_many300_soft": (255, ["many300"], SOFT),
    "P255_special_none_dozen_soft": (255, ["special", "none", "dozen"], SOFT),
    "P1024_special_hardQ": (1024, ["special"], HARD_Q),
    "P1024_all_empty_hardH": (1024, ["none", "none", "none"], HARD_H),
    "P1025_special_many300_one_soft": (1025, ["special", "many300", "one"], SOFT),
    "P1025_special_hardH": (1025, ["special"], HARD_H),
    "P4096_special_soft": (4096, ["special"], SOFT),
    "P4097_special_dozen_none_hardQ": (4097, ["special", "dozen", "none"], HARD_Q),
    "P4097_many300_hardH": (4097, ["many300"], HARD_H),
    "P9223_special_many300_dozendup_soft": (9223, ["special", "many300", "dozen_dup"], SOFT),
    "P9223_special_hardH": (9223, ["special"], HARD_H),
    "P9223_empty_soft": (9223, ["none"], SOFT),
    "P4096_dozen_one_none_hardH": (4096, ["dozen", "one", "none"], HARD_H),
}
MATCH_NAMES = list(_MATCH)


@functools.lru_cache(maxsize=None)
def matching_case(name):
    """-> dict(priors (P,6), boxes [N], labels [N], threshold, promises [N])."""
    P, kinds, thr = _MATCH[name]
    seed = 1000 + MATCH_NAMES.index(name) * 10
    priors = dyadic_priors(P, seed)
    imgs = [_image(k, priors, seed + 1 + i) for i, k in enumerate(kinds)]
    return dict(priors=priors, boxes=[i[0] for i in imgs], labels=[i[1] for i in imgs], threshold=thr,
                promises=[i[2] for i in imgs], kinds=kinds)


def thresholds(threshold):
    """-> (thr_lo, thr_hi, soft) as the C ABI takes them."""
    if isinstance(threshold, list):
        return float(threshold[0]), float(threshold[1]), 1
    return float(threshold), 0.0, 0


# ------------------------------------------------------------------------------------------------------------- loss
NPROTO = 80


def score_prototypes(ncls, seed):
    """NPROTO score rows whose negatives' losses are far apart, so that which negatives the mining keeps depends on nobody's
    rounding; ties come only from using a row more than once (bit-equal rows give bit-equal losses).
    ncls 2: the foreground logit x1 takes every multiple of 2^-4 in [-2.5, 2.5) once and the margin x1 - x0 every multiple of
    2^-3 in [-5, 5) once, in a seeded pairing - the cross entropy is monotone in the margin and the focal loss in x1.
    ncls > 2: random foreground logits (multiples of 2^-4) and x0 such that the cross entropy against class 0 is (j+1) / 16."""
    g = _gen(seed)
    j = torch.arange(NPROTO)
    if ncls == 2:
        x1 = (j - NPROTO // 2).double() / 16
        margin = (torch.randperm(NPROTO, generator=g) - NPROTO // 2).double() / 8
        return torch.stack([x1 - margin, x1], dim=1).float()
    fg = (torch.randn((NPROTO, ncls - 1), generator=g, dtype=torch.float64) * 1.5 * 16).round() / 16
    x0 = torch.logsumexp(fg, dim=1) - torch.log(torch.expm1((j + 1).double() / 16))
    return torch.cat([x0[:, None], fg], dim=1).float()


def make_targets(N, P, ncls, seed, f_pos=0.05, f_ign=0.05, plain_image=True):
    """true_classes (N,P) in {-1, 0, 1..ncls-1}, true_locs, locs.  Image 1 (if any, and ``plain_image``) has neither a positive
    nor an ignored prior; the first and the last prior of the batch's image 0 are positive.  Residuals locs - true_locs have
    standard deviation 1.5 (both sides of the smooth-L1 knee at 1); about 2 % are exactly 0, one of a positive prior always."""
    g = _gen(seed)
    u = torch.rand((N, P), generator=g)
    tc = torch.zeros((N, P), dtype=torch.long)
    fg = torch.randint(1, ncls, (N, P), generator=g)
    tc[u < f_pos] = fg[u < f_pos]
    tc[u > 1 - f_ign] = -1
    if N > 1 and plain_image:
        tc[1] = 0
    tc[0, 0] = 1
    tc[0, P - 1] = ncls - 1
    tl = torch.randn((N, P, 6), generator=g)
    resid = torch.randn((N, P, 6), generator=g) * 1.5
    resid[torch.rand((N, P, 6), generator=g) < 0.02] = 0.0
    resid[0, 0, 0] = 0.0  # a positive prior
    locs = tl + resid
    locs[resid == 0] = tl[resid == 0]
    return tc, tl, locs, g


LOSS_SHAPES = ((1, 1), (1, 255), (2, 8192), (1, 16385), (3, 7001))
LOSS_NCLS = (2, 3, 5, 16)
LOSS_NAMES = [f"N{n}_P{p}_C{c}" for n, p in LOSS_SHAPES for c in LOSS_NCLS]
UPSTREAM = (0.7, 1.3)  # (u_conf, u_loc)


@functools.lru_cache(maxsize=None)
def loss_case(name):
    """-> dict(N, P, ncls, locs, scores, true_classes, true_locs, ratio)."""
    N, P, ncls = (int(x[1:]) for x in name.split("_"))
    seed = 5000 + LOSS_NAMES.index(name)
    tc, tl, locs, g = make_targets(N, P, ncls, seed)
    proto = score_prototypes(ncls, seed)
    scores = proto[torch.randint(0, NPROTO, (N, P), generator=g)].contiguous()
    return dict(N=N, P=P, ncls=ncls, locs=locs, scores=scores, true_classes=tc, true_locs=tl, ratio=3)


# ----------------------------------------------------------------------------------------------------------- mining
MINING_P = (1023, 1024, 1025, 3000)
# kind -> (f_pos, f_ign, ratio).  Image 0 of the case keeps what the kind promises (asserted on the CPU):
#   run:   0 < k < P and the k-th and (k+1)-th largest negative losses are one non-zero value (a run of copied rows)
#   zeros: #negatives <= k < P, so the cut falls among the exact zeros of the positive and ignored priors
#   k0:    ratio 0 -> nothing kept;   all: ratio * n_pos >= P -> everything kept
MINING_KINDS = {"run": (0.05, 0.05, 3), "zeros": (0.4, 0.1, 2), "k0": (0.05, 0.05, 0), "all": (0.05, 0.05, 10000)}
MINING_NAMES = [f"P{p}_{k}" for p in MINING_P for k in MINING_KINDS]


@functools.lru_cache(maxsize=None)
def mining_case(name):
    """Two classes, two images; rows 100..399 of every image are one copied row, the others are drawn from the prototypes."""
    p, kind = name.split("_")
    P, (f_pos, f_ign, ratio) = int(p[1:]), MINING_KINDS[kind]
    seed = 7000 + MINING_NAMES.index(name)
    tc, tl, locs, g = make_targets(2, P, 2, seed, f_pos, f_ign, plain_image=False)
    proto = score_prototypes(2, seed)
    scores = proto[torch.randint(0, NPROTO, (2, P), generator=g)].contiguous()
    scores[:, 100:400] = proto[NPROTO - 9]
    return dict(N=2, P=P, ncls=2, locs=locs, scores=scores, true_classes=tc, true_locs=tl, ratio=ratio, kind=kind)


# ------------------------------------------------------------------------------------------------------------- pack
# name -> (N, feature-map sizes, ncls).  P = 2 * sum(D*H*W)
_PACK = {
    "one_scale_111": (2, [(1, 1, 1)], 2),
    "two_scales": (3, [(2, 3, 5), (1, 4, 4)], 3),
    "three_scales": (2, [(2, 3, 5), (3, 1, 2), (1, 1, 1)], 10),
    "four_scales": (3, [(2, 3, 5), (1, 4, 4), (3, 1, 2), (1, 1, 1)], 16),
    "model_64": (2, [(8, 8, 8), (4, 4, 4), (2, 2, 2)], 2),
    "two_large": (2, [(16, 16, 16), (7, 8, 9)], 3),  # N*P = 18400: prior indices past 16384
}
PACK_NAMES = list(_PACK)


def prior_offsets(dims):
    offs, o = [], 0
    for d in dims:
        offs.append(o)
        o += 2 * math.prod(d)
    return offs, o


@functools.lru_cache(maxsize=None)
def pack_case(name):
    """-> dict(N, P, ncls, dims, prior_off, priors, boxes, labels, threshold, locs, scores).  Targets come from the matcher
    (image 1 has no object); the head outputs are plain normal draws."""
    N, dims, ncls = _PACK[name]
    seed = 9000 + PACK_NAMES.index(name) * 10
    offs, P = prior_offsets(dims)
    imgs = [random_boxes(12, seed + i, n_labels=ncls - 1) for i in range(N)]
    imgs[1] = (torch.zeros((0, 6)), torch.zeros((0,), dtype=torch.long))
    g = _gen(seed + 5)
    return dict(N=N, P=P, ncls=ncls, dims=dims, prior_off=offs, priors=dyadic_priors(P, seed + 6),
                boxes=[i[0] for i in imgs], labels=[i[1] for i in imgs], threshold=SOFT,
                locs=torch.randn((N, P, 6), generator=g) * 1.5, scores=torch.randn((N, P, ncls), generator=g) * 2.0)
