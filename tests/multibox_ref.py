"""Plain-torch reference of the MultiBox loss of csrc/multibox.hip, on the CPU, for tests/test_gpu_multibox.py (proved against
the oracle by tests/test_multibox_ref_cpu.py).

The loss takes the TARGETS (true_classes, true_locs) as inputs, so it is tested without the matcher; the matcher's reference
is ``oracle.multibox.match_batch`` itself.  Formulas are those of oracle/multibox.py: ignored priors (-1) contribute nothing;
cross entropy (or ``focal_binary`` on the foreground logit) summed over every prior with class >= 0 and divided by the number
of positives; L1 (or smooth-L1, beta 1) mean over positives x 6; hard-negative mining by a stable descending sort per image.
Gradients come from autograd on these formulas.  Everything runs in ``dtype`` (float64 for the reference; float32 for the
deviation the kernels are judged against, see ``tolerance``)."""
import torch
import torch.nn.functional as F

from oracle import multibox as OMB

HNM, SMOOTH, FOCAL = 1, 2, 4
LOSS_RTOL_CAP = 1e-4  # BASELINE.json: losses within 1e-4 of the reference


def valid_flags(ncls):
    """The flag sets msl_multibox_loss_var accepts for this class count (focal: background + one class)."""
    return [f for f in range(8) if not (f & FOCAL) or ncls == 2]


def conf_per_prior(scores, true_classes, focal):
    """(N, P) confidence loss of every prior; ignored priors 0."""
    n, p, c = scores.shape
    if focal:
        ce = OMB.focal_binary(scores[..., 1], true_classes > 0)
    else:
        ce = F.cross_entropy(scores.reshape(-1, c), true_classes.clamp(min=0).reshape(-1), reduction="none").view(n, p)
    return torch.where(true_classes < 0, torch.zeros_like(ce), ce)


def mined_mask(conf_loss_neg, n_pos, ratio):
    """The 0/1 mask multibox_hnm_select_kernel documents: per image, with k = min(ratio * n_pos, P), nothing if k <= 0,
    everything if k >= P, otherwise the first k of a stable descending sort of conf_loss_neg.  -> bool (N, P)."""
    N, P = conf_loss_neg.shape
    mask = torch.zeros((N, P), dtype=torch.bool)
    for n in range(N):
        k = min(int(ratio) * int(n_pos[n]), P)
        if k <= 0:
            continue
        if k >= P:
            mask[n] = True
            continue
        order = conf_loss_neg[n].sort(descending=True, stable=True).indices
        mask[n, order[:k]] = True
    return mask


def conf_loss_neg(scores, true_classes, flags, dtype=torch.float64):
    """(N, P): the confidence loss of the negatives, 0 for positive and ignored priors (what the mining sorts)."""
    ce = conf_per_prior(scores.detach().to(dtype), true_classes, bool(flags & FOCAL))
    return torch.where(true_classes > 0, torch.zeros_like(ce), ce)


def losses(locs, scores, true_classes, true_locs, flags=0, neg_pos_ratio=3, dtype=torch.float64):
    """-> (conf, loc, n_positives, mined mask or None); conf / loc are 0-d tensors of ``dtype`` (autograd-capable)."""
    locs, scores, true_locs = locs.to(dtype), scores.to(dtype), true_locs.to(dtype)
    pos = true_classes > 0
    n_pos = int(pos.sum())
    ce = conf_per_prior(scores, true_classes, bool(flags & FOCAL))
    neg = torch.where(pos, torch.zeros_like(ce), ce)
    if flags & SMOOTH:
        loc_sum = F.smooth_l1_loss(locs[pos], true_locs[pos], reduction="sum", beta=1.0)
    else:
        loc_sum = (locs[pos] - true_locs[pos]).abs().sum()
    loc = loc_sum / (n_pos * 6)
    mask = None
    if flags & HNM:
        mask = mined_mask(neg.detach(), pos.sum(dim=1), neg_pos_ratio)
        conf = (neg[mask].sum() + ce[pos].sum()) / n_pos
    else:
        conf = (neg.sum() + ce[pos].sum()) / n_pos
    return conf, loc, n_pos, mask


def losses_and_grads(locs, scores, true_classes, true_locs, flags=0, neg_pos_ratio=3, u_conf=1.0, u_loc=1.0,
                     dtype=torch.float64):
    """-> dict(conf, loc, n_pos, mask, dlocs, dscores): gradients of u_conf * conf + u_loc * loc by autograd in ``dtype``."""
    gl = locs.detach().to(dtype).requires_grad_(True)
    gs = scores.detach().to(dtype).requires_grad_(True)
    conf, loc, n_pos, mask = losses(gl, gs, true_classes, true_locs, flags, neg_pos_ratio, dtype)
    (u_conf * conf + u_loc * loc).backward()
    return dict(conf=conf.detach(), loc=loc.detach(), n_pos=n_pos, mask=mask, dlocs=gl.grad, dscores=gs.grad)


def deviation(a, ref):
    """Largest absolute difference, relative to the largest magnitude of the reference."""
    a, ref = a.detach().double().reshape(-1), ref.detach().double().reshape(-1)
    return float((a - ref).abs().max() / ref.abs().max().clamp(min=1e-300))


QUANTITIES = ("conf", "loc", "dlocs", "dscores")


def tolerance(locs, scores, true_classes, true_locs, ncls, neg_pos_ratio, u_conf, u_loc, flag_sets=None):
    """The bound a kernel result of this case is held to, from the reference side only: the same formulas evaluated in
    float32 torch deviate from the float64 result by ``dev32`` (the largest ``deviation`` over the four quantities and over
    every flag set the case runs with, ``flag_sets``, by default all the class count allows); the kernels use other expf /
    logf implementations and another summation order, so they get 8 times that, capped at the 1e-4 BASELINE.json allows a
    loss.  -> (bound, dev32)."""
    dev32 = 0.0
    for f in (valid_flags(ncls) if flag_sets is None else flag_sets):
        r64 = losses_and_grads(locs, scores, true_classes, true_locs, f, neg_pos_ratio, u_conf, u_loc, torch.float64)
        r32 = losses_and_grads(locs, scores, true_classes, true_locs, f, neg_pos_ratio, u_conf, u_loc, torch.float32)
        dev32 = max([dev32] + [deviation(r32[q], r64[q]) for q in QUANTITIES])
    return min(LOSS_RTOL_CAP, 8.0 * dev32), dev32


def head_co(ncls):
    return 16 * ((12 + 2 * ncls + 15) // 16)


def head_grad_images(dlocs, dscores, dims, prior_off, ncls, fill):
    """The gradient images the head convolutions' backward reads, as the comments on LossPackDst and msl_head_grad_pack state
    the layout: per scale (D, H, W) an image (N, CO, D+2, H+2, W+2), CO = 16 * ceil((12 + 2*ncls) / 16); prior
    ``prior_off + 2*pos + a`` with pos = (d*H + h)*W + w sits at (d+1, h+1, w+1); its box gradients in rows a*6 + q, its class
    gradients in rows 12 + a*ncls + c.  The halo and the remaining rows hold ``fill``."""
    N = dlocs.shape[0]
    out = []
    for (D, H, W), off in zip(dims, prior_off):
        S = D * H * W
        img = torch.full((N, head_co(ncls), D + 2, H + 2, W + 2), fill, dtype=dlocs.dtype)
        gl = dlocs[:, off:off + 2 * S].reshape(N, D, H, W, 2, 6)
        gs = dscores[:, off:off + 2 * S].reshape(N, D, H, W, 2, ncls)
        img[:, :12, 1:-1, 1:-1, 1:-1] = gl.permute(0, 4, 5, 1, 2, 3).reshape(N, 12, D, H, W)
        img[:, 12:12 + 2 * ncls, 1:-1, 1:-1, 1:-1] = gs.permute(0, 4, 5, 1, 2, 3).reshape(N, 2 * ncls, D, H, W)
        out.append(img)
    return out
