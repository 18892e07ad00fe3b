"""Cases of tests/test_gpu_iouloss.py: named, seeded, nothing stored.  What they promise - every comparison of the loss at
least MARGIN away from its switch point, which geometries are planted - is asserted by tests/test_iouloss_ref_cpu.py.

Targets and scores come from tests/multibox_cases.py (``make_targets``, ``score_prototypes``); the offsets of the POSITIVE
priors are replaced by boxes placed relative to their prior: a box with centre ``p_c + d * p_s`` and size ``r * p_s`` has
offsets ``(10 d, 5 log r)`` whatever the prior.  Priors have their own size on every axis."""
import functools
import math

import torch

from tests import iouloss_ref as IR
from tests import multibox_cases as C

MARGIN = 1e-4  # image fractions (and units of g / 5 for the clamp), evaluated in float64
SHAPES = ((1, 1), (1, 255), (2, 8192), (3, 7001))
NCLS = (2, 3)
NAMES = [f"N{n}_P{p}_C{c}" for n, p in SHAPES for c in NCLS]
NO_POSITIVE = "N2_P255_C2_nopos"   # a batch without a single positive prior
IDENTICAL = "N1_P255_C3_same"      # locs == true_locs bit for bit
ALL_NAMES = NAMES + [NO_POSITIVE, IDENTICAL]
UPSTREAM = C.UPSTREAM

# planted positives: name -> (prediction (d, r), target (d, r)) per axis, in units of the prior's size; None: offset given below
PLANTED = {
    "disjoint_1": (((2.0, 0.1, -0.1), (1.0, 1.1, 0.9)), ((0.0, 0.0, 0.0), (0.8, 1.0, 1.2))),
    "disjoint_2": (((2.0, -1.8, 0.1), (1.0, 1.1, 0.9)), ((0.0, 0.0, 0.0), (0.8, 1.0, 1.2))),
    "disjoint_3": (((2.0, -1.8, 1.7), (1.0, 1.1, 0.9)), ((0.0, 0.0, 0.0), (0.8, 1.0, 1.2))),
    "pred_inside": (((0.1, -0.1, 0.05), (0.5, 0.6, 0.4)), ((0.0, 0.05, 0.0), (1.2, 1.3, 1.1))),
    "target_inside": (((0.05, 0.0, -0.05), (1.5, 1.4, 1.6)), ((0.1, -0.1, 0.0), (0.6, 0.5, 0.7))),
    "partial": (((0.4, -0.3, 0.2), (1.0, 1.0, 1.0)), ((0.0, 0.0, 0.0), (0.9, 1.1, 1.0))),
    "clamp_high": (((0.1, -0.1, 0.05), (1.0, 0.9, 1.15)), ((0.0, 0.0, 0.0), (0.9, 1.2, 1.0))),   # + size offset 21 on axis 0
    "clamp_low": (((0.1, -0.1, 0.05), (1.0, 0.9, 1.15)), ((0.0, 0.0, 0.0), (0.9, 1.2, 1.0))),    # + size offset -22 on axis 1
}
PLANTED_AT = {k: 3 + 7 * i for i, k in enumerate(PLANTED)}  # prior index in image 0 (P >= 255)
CLAMP_OFFSETS = {"clamp_high": (3, 21.0), "clamp_low": (4, -22.0)}


def offsets(d, r):
    return torch.tensor([10.0 * x for x in d] + [5.0 * math.log(x) for x in r], dtype=torch.float32)


def priors(P, seed):
    """(P, 6) centre-size: centres in [0.1, 0.9], sizes in [0.05, 0.25], independent per axis."""
    g = torch.Generator().manual_seed(seed)
    c = 0.1 + 0.8 * torch.rand((P, 3), generator=g)
    s = 0.05 + 0.2 * torch.rand((P, 3), generator=g)
    return torch.cat([c, s], dim=1).float().contiguous()


def _draw(n, g):
    """n random (prediction, target) offset rows: centres within 0.6 / 0.3 prior sizes, size ratios within e^+-0.7 / e^+-0.5."""
    u = lambda lo, hi: lo + (hi - lo) * torch.rand((n, 3), generator=g)  # noqa: E731
    return (torch.cat([10.0 * u(-0.6, 0.6), 5.0 * u(-0.7, 0.7)], dim=1).float(),
            torch.cat([10.0 * u(-0.3, 0.3), 5.0 * u(-0.5, 0.5)], dim=1).float())


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(N, P, ncls, locs, scores, true_classes, true_locs, priors, ratio, planted {name: flat prior index})."""
    N, P, ncls = (int(x[1:]) for x in name.split("_")[:3])
    seed = 11000 + ALL_NAMES.index(name)
    tc, tl, locs, g = C.make_targets(N, P, ncls, seed)
    proto = C.score_prototypes(ncls, seed)
    scores = proto[torch.randint(0, C.NPROTO, (N, P), generator=g)].contiguous()
    pri = priors(P, seed + 500)
    if N > 2:
        tc[2] = -1  # an all-ignored image (image 1 has neither a positive nor an ignored prior: make_targets)
    planted = {}
    if name == NO_POSITIVE:
        tc[tc > 0] = 0
    pos = (tc > 0).view(-1).nonzero().view(-1)
    fl, ft, fp = locs.view(-1, 6), tl.view(-1, 6), pri.repeat(N, 1)
    if pos.numel():
        fl[pos], ft[pos] = _draw(pos.numel(), g)
        for _ in range(64):  # re-draw the positives with a comparison closer than MARGIN to its switch point
            bad = pos[(IR.margins(fl[pos], ft[pos], fp[pos]).view(pos.numel(), -1).min(dim=1).values < 2 * MARGIN)]
            if not bad.numel():
                break
            fl[bad], ft[bad] = _draw(bad.numel(), g)
    if P >= 255 and name not in (NO_POSITIVE, IDENTICAL):
        for k, (pred, targ) in PLANTED.items():
            i = PLANTED_AT[k]
            tc[0, i] = 1
            fl[i], ft[i] = offsets(*pred), offsets(*targ)
            if k in CLAMP_OFFSETS:
                q, v = CLAMP_OFFSETS[k]
                fl[i, q] = v
            planted[k] = i
    if name == IDENTICAL:
        locs = tl.clone()
    return dict(N=N, P=P, ncls=ncls, locs=locs.contiguous(), scores=scores, true_classes=tc, true_locs=tl.contiguous(),
                priors=pri, ratio=3, planted=planted)


def positive_rows(c):
    """-> (locs, true_locs, priors) rows of the positive priors of a case."""
    pos = c["true_classes"] > 0
    pri = c["priors"][None].expand(c["N"], -1, -1)
    return c["locs"][pos], c["true_locs"][pos], pri[pos]
