"""Reference of the prior fit report (msl_prior_fit): a loop over images around
``oracle.multibox.match_image`` with every label 1 - the five per-box arrays the kernel writes, from the (P,) vectors the
oracle's matching returns.  CPU only."""
import numpy as np
import torch

from oracle import boxes as B
from oracle import multibox as MB


def reference(true_boxes, priors_c, thresholds, scale_off):
    """true_boxes: list of (n_i,6) arrays; priors_c (P,6) f32; thresholds (T,); scale_off (S+1,) ->
    dict(best_iou (G,) f32, best_prior (G,) i64, held (G,) i64, pos (G,T,S) i64, image (G,) i64)."""
    pri = torch.as_tensor(np.asarray(priors_c, np.float32))
    off = np.asarray(scale_off, np.int64)
    thr = [float(np.float32(t)) for t in thresholds]
    S, T = off.size - 1, len(thr)
    scale_of_prior = np.searchsorted(off, np.arange(pri.shape[0]), side="right") - 1
    best_iou, best_prior, held, pos, image = [], [], [], [], []
    for n, b in enumerate(true_boxes):
        b = torch.as_tensor(np.asarray(b, np.float32).reshape(-1, 6))
        k = b.shape[0]
        if k == 0:
            continue
        iou = B.iou_matrix(b, B.cxcycz_to_xyz(pri))
        mx, first = MB._first_argmax(iou, 1)  # iou.max(1) and prior_for_obj
        first = first.numpy()
        best_iou.append(mx.numpy().astype(np.float32))
        best_prior.append(first.astype(np.int64))
        held.append(np.array([int(not (first[g + 1:] == first[g]).any()) for g in range(k)], dtype=np.int64))
        p = np.zeros((k, T, S), dtype=np.int64)
        for t in range(T):
            label, obj, _, _ = MB.match_image(b, torch.ones(k, dtype=torch.int64), pri, [thr[t]])
            sel = (label > 0).numpy()
            np.add.at(p, (obj.numpy()[sel], t, scale_of_prior[sel]), 1)
        pos.append(p)
        image.append(np.full(k, n, dtype=np.int64))
    cat = lambda xs, shape, dt: np.concatenate(xs) if xs else np.zeros(shape, dt)
    return {"best_iou": cat(best_iou, (0,), np.float32), "best_prior": cat(best_prior, (0,), np.int64),
            "held": cat(held, (0,), np.int64), "pos": cat(pos, (0, T, S), np.int64), "image": cat(image, (0,), np.int64)}
