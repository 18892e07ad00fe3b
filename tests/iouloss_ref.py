"""Plain-torch reference of msl_multibox_loss_iou (csrc/multibox.hip), on the CPU, for tests/test_gpu_iouloss.py and
tests/test_gpu_iouloss_model.py (checked against central differences and the oracle's box functions by
tests/test_iouloss_ref_cpu.py).

The confidence side is tests/multibox_ref.py's (cross entropy or focal, hard-negative mining).  The localisation term of a
positive prior with prior row p, predicted offsets g and target offsets t is, per axis a,

    c = g_a p_{3+a} / 10 + p_a,   s = exp(clamp(g_{3+a} / 5, -4, 4)) p_{3+a},   lo = c - s / 2,   hi = c + s / 2
    (target: the same decode of t without the clamp)
    inter = prod max(min(hi, thi) - max(lo, tlo), 0),   union = prod s + prod ts - inter,   e = max(hi, thi) - min(lo, tlo)
    iou: 1 - inter / union        giou: + (prod e - union) / prod e        diou: + sum (c - tc)^2 / sum e^2

and loc = sum over positives / number of positives.  Gradients come from autograd.  Everything runs in ``dtype``."""
import torch

from tests import multibox_ref as R

KINDS = {"iou": 1, "giou": 2, "diou": 3}
FLAG_SETS = (0, 1, 4, 5)  # the confidence bits: hard-negative mining, focal
CLAMP = 4.0


def valid_flags(ncls):
    return [f for f in FLAG_SETS if not (f & R.FOCAL) or ncls == 2]


def decode(g, priors, clamp):
    """(M, 6) offsets, (M, 6) centre-size priors -> centre (M, 3), size, lo, hi."""
    z = g[:, 3:] / 5
    if clamp:
        z = z.clamp(-CLAMP, CLAMP)
    c = g[:, :3] * priors[:, 3:] / 10 + priors[:, :3]
    s = torch.exp(z) * priors[:, 3:]
    return c, s, c - s / 2, c + s / 2


def per_prior(g, t, priors, kind):
    """(M,) loss of every row; ``kind`` a key of KINDS."""
    c, s, lo, hi = decode(g, priors, True)
    tc, ts, tlo, thi = decode(t, priors, False)
    inter = (torch.minimum(hi, thi) - torch.maximum(lo, tlo)).clamp(min=0).prod(dim=1)
    union = s.prod(dim=1) + ts.prod(dim=1) - inter
    e = torch.maximum(hi, thi) - torch.minimum(lo, tlo)
    l = 1 - inter / union
    if kind == "giou":
        enc = e.prod(dim=1)
        l = l + (enc - union) / enc
    elif kind == "diou":
        l = l + ((c - tc) ** 2).sum(dim=1) / (e ** 2).sum(dim=1)
    else:
        assert kind == "iou", kind
    return l


def margins(g, t, priors):
    """How far every comparison of ``per_prior`` is from its switch point, in float64: (M, 3, 5) =
    [|hi - thi|, |lo - tlo|, |min(hi, thi) - max(lo, tlo)|, |g/5 - 4|, |g/5 + 4|] per axis."""
    g, t, priors = g.double(), t.double(), priors.double()
    _, _, lo, hi = decode(g, priors, True)
    _, _, tlo, thi = decode(t, priors, False)
    w = torch.minimum(hi, thi) - torch.maximum(lo, tlo)
    z = g[:, 3:] / 5
    return torch.stack([(hi - thi).abs(), (lo - tlo).abs(), w.abs(), (z - CLAMP).abs(), (z + CLAMP).abs()], dim=2)


def losses(locs, scores, true_classes, true_locs, priors_c, kind, flags=0, neg_pos_ratio=3, dtype=torch.float64):
    """-> (conf, loc, n_positives, mined mask or None), as multibox_ref.losses."""
    assert not flags & R.SMOOTH
    locs, scores, true_locs, priors_c = locs.to(dtype), scores.to(dtype), true_locs.to(dtype), priors_c.to(dtype)
    pos = true_classes > 0
    n_pos = int(pos.sum())
    ce = R.conf_per_prior(scores, true_classes, bool(flags & R.FOCAL))
    neg = torch.where(pos, torch.zeros_like(ce), ce)
    pri = priors_c[None].expand(locs.shape[0], -1, -1)
    loc = per_prior(locs[pos], true_locs[pos], pri[pos], kind).sum() / n_pos  # no positive: 0 / 0 = NaN
    mask = None
    if flags & R.HNM:
        mask = R.mined_mask(neg.detach(), pos.sum(dim=1), neg_pos_ratio)
        conf = (neg[mask].sum() + ce[pos].sum()) / n_pos
    else:
        conf = (neg.sum() + ce[pos].sum()) / n_pos
    return conf, loc, n_pos, mask


def losses_and_grads(locs, scores, true_classes, true_locs, priors_c, kind, flags=0, neg_pos_ratio=3, u_conf=1.0, u_loc=1.0,
                     dtype=torch.float64):
    """-> dict(conf, loc, n_pos, mask, dlocs, dscores): gradients of u_conf * conf + u_loc * loc by autograd in ``dtype``."""
    gl = locs.detach().to(dtype).requires_grad_(True)
    gs = scores.detach().to(dtype).requires_grad_(True)
    conf, loc, n_pos, mask = losses(gl, gs, true_classes, true_locs, priors_c, kind, flags, neg_pos_ratio, dtype)
    (u_conf * conf + u_loc * loc).backward()
    return dict(conf=conf.detach(), loc=loc.detach(), n_pos=n_pos, mask=mask, dlocs=gl.grad, dscores=gs.grad)


def tolerance(locs, scores, true_classes, true_locs, priors_c, kind, ncls, neg_pos_ratio, u_conf, u_loc):
    """The project's rule (multibox_ref.tolerance) for one case and one kind, from the reference side only: ``dev32`` is the
    largest deviation of the float32 evaluation of these formulas from the float64 one, over conf / loc / dlocs / dscores and
    every flag set the class count allows; a kernel gets 8 x dev32, capped at 1e-4.  -> (bound, dev32)."""
    dev32 = 0.0
    for f in valid_flags(ncls):
        a = (locs, scores, true_classes, true_locs, priors_c, kind, f, neg_pos_ratio, u_conf, u_loc)
        r64, r32 = losses_and_grads(*a, torch.float64), losses_and_grads(*a, torch.float32)
        dev32 = max([dev32] + [R.deviation(r32[q], r64[q]) for q in R.QUANTITIES])
    return min(R.LOSS_RTOL_CAP, 8.0 * dev32), dev32
