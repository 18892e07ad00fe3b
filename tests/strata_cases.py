"""Inputs and the brute-force restatement shared by tests/test_strata_cpu.py and tests/test_gpu_strata.py (DESIGN.md "Eval by
lesion size").  A case is the tuple (det_boxes, det_labels, det_scores, true_boxes, true_labels) of per-image lists."""
import numpy as np

from tests.golden import cases as golden_cases

NEVER = 0x7FFFFFFF
EDGES = [27.0, 125.0, 1000.0]


def boxes(rs, n, lo_max=0.8, ext=(0.02, 0.25)):
    lo = rs.uniform(0, lo_max, (n, 3)).astype(np.float32)
    return np.concatenate([lo, lo + rs.uniform(*ext, (n, 3)).astype(np.float32)], 1)


def map_case(name):
    c = golden_cases.map_cases()[name]
    return c["det_boxes"], c["det_labels"], c["det_scores"], c["true_boxes"], c["true_labels"]


def random_case(seed, n_img=12, max_det=30, max_gt=6, quant=8):
    """12 images x 0-30 detections, 0-6 boxes: hits with jitter, duplicates, misses, label 0 / 2 rows on both sides, scores
    quantised to 1/quant (ties), one image without ground truth and one without detections."""
    rs = np.random.RandomState(seed)
    tb, tl, db, dl, ds = [], [], [], [], []
    for i in range(n_img):
        ng = 0 if i == seed % n_img else int(rs.randint(0, max_gt + 1))
        nd = 0 if i == (seed + 5) % n_img else int(rs.randint(0, max_det + 1))
        t, d = boxes(rs, ng), boxes(rs, nd)
        if ng and nd:
            k = min(nd, 2 * ng)
            d[:k] = t[rs.randint(0, ng, k)] + rs.uniform(-0.02, 0.02, (k, 6)).astype(np.float32)
        lab = np.ones(ng, np.int64)
        lab[rs.rand(ng) < 0.15] = 2
        lab[rs.rand(ng) < 0.05] = 0
        lb = np.ones(nd, np.int64)
        lb[rs.rand(nd) < 0.1] = 2
        lb[rs.rand(nd) < 0.1] = 0
        sc = rs.uniform(0, 1, nd)
        sc = (np.round(sc * quant) / quant if quant else sc).astype(np.float32)
        tb.append(t), tl.append(lab), db.append(d), dl.append(lb), ds.append(sc)
    return db, dl, ds, tb, tl


def grid_case(seed, n_img, per, max_gt=6, quant=256, no_gt_every=13):
    """``n_img`` images x ``per`` detections (three jittered copies of every box first), 1 .. max_gt boxes."""
    rs = np.random.RandomState(seed)
    tb = [boxes(rs, 0 if i % no_gt_every == no_gt_every - 1 else int(rs.randint(1, max_gt + 1))) for i in range(n_img)]
    tl = [np.ones(len(t), np.int64) for t in tb]
    db, dl, ds = [], [], []
    for t in tb:
        d = boxes(rs, per)
        k = min(per, 3 * len(t))
        if k:
            d[:k] = np.repeat(t, 3, axis=0)[:k] + rs.uniform(-0.02, 0.02, (k, 6)).astype(np.float32)
        db.append(d), dl.append(np.ones(per, np.int64))
        ds.append((np.round(rs.uniform(0, 1, per) * quant) / quant).astype(np.float32))
    return db, dl, ds, tb, tl


def edge_case():
    """Three images in a frame of 1000 voxels, edges 27 / 125 / 1000.  Image 0: a box of exactly 125 voxels (0.5^3: on the
    edge, so in the bin above it), a zero-volume box (bin 0) and the whole frame (1000: the top bin); its detections are the
    same three boxes and a far miss of 1 voxel.  The flat detection's IoU with the flat box is 0 / 0: a false positive of
    volume 0.  Image 1: a box of 64 voxels and no detection.  Image 2: a box with a NaN corner and the same box as its
    only detection (IoU NaN: a false positive), both unbinned.
    Rank order: half 0.9 TP | flat 0.8 FP | nan 0.7 FP | whole 0.6 TP | miss 0.5 FP;  K = 5."""
    half = [0.0, 0.0, 0.0, 0.5, 0.5, 0.5]
    flat = [0.6, 0.6, 0.6, 0.6, 0.9, 0.9]
    nan = [0.7, 0.7, np.nan, 0.9, 0.9, 0.9]
    whole = [0.0, 0.0, 0.0, 1.0, 1.0, 1.0]
    miss = [0.5, 0.0, 0.0, 0.625, 0.125, 0.0625]
    tb = [np.array([half, flat, whole], np.float32), np.array([[0.0, 0.0, 0.0, 0.4, 0.4, 0.4]], np.float32),
          np.array([nan], np.float32)]
    tl = [np.ones(3, np.int64), np.ones(1, np.int64), np.ones(1, np.int64)]
    db = [np.array([half, flat, whole, miss], np.float32), np.zeros((0, 6), np.float32), np.array([nan], np.float32)]
    dl = [np.ones(4, np.int64), np.zeros(0, np.int64), np.ones(1, np.int64)]
    ds = [np.array([0.9, 0.8, 0.6, 0.5], np.float32), np.zeros(0, np.float32), np.array([0.7], np.float32)]
    return db, dl, ds, tb, tl


def volume_f32(b):
    b = np.asarray(b, np.float32)
    return (b[3] - b[0]) * (b[4] - b[1]) * (b[5] - b[2])  # three f32 subtractions, two f32 multiplications, left to right


def stratum(vol_f32, voxels, edges):
    v = float(np.float32(vol_f32)) * float(voxels)
    if v != v:
        return -1
    return sum(1 for e in edges if e <= v)


def matching(case, min_overlap):
    """Class 1 only, by the rule of oracle/metrics.py::class_metrics, keeping what it drops: -> ranked detections as
    (image, box, tp) and class-1 ground truth as (image, box, claim rank or NEVER)."""
    from oracle import metrics as OM
    db, dl, ds, tb, tl = case
    dets = [(n, np.asarray(b, np.float32), np.float32(s)) for n in range(len(dl))
            for b, l, s in zip(db[n], dl[n], ds[n]) if l == 1]
    sco = np.array([d[2] for d in dets], np.float32)
    order = np.lexsort((np.arange(len(dets)), -sco.astype(np.float64)))
    gts = [[n, np.asarray(b, np.float32), NEVER] for n in range(len(tl)) for b, l in zip(tb[n], tl[n]) if l == 1]
    ranked = []
    for rank, j in enumerate(order):
        n, box, _ = dets[j]
        same = [g for g, gt in enumerate(gts) if gt[0] == n]
        tp = 0
        if same:
            ov = OM._iou_1_to_many(box, np.stack([gts[g][1] for g in same]))
            mx = ov.max()
            pick = same[int(np.nonzero(ov == mx)[0][0])] if not np.isnan(mx) else same[int(np.argmax(ov))]
            if mx > min_overlap and gts[pick][2] == NEVER:
                gts[pick][2] = rank
                tp = 1
        ranked.append((n, box, tp))
    return ranked, gts


def brute_force(case, voxels, edges, min_overlaps, weights, cuts):
    """The definitions applied literally, one Python integer at a time."""
    w = np.asarray(weights, np.int64)
    N = w.shape[1]
    vox = np.broadcast_to(np.asarray(voxels, np.float64).reshape(-1), (N,)) if np.size(voxels) == 1 else np.asarray(voxels)
    R1, S1 = w.shape[0], len(edges) + 2
    cuts = np.asarray(cuts, np.int64)
    tp_out = np.zeros((R1, len(min_overlaps), cuts.shape[2], S1), np.int64)
    fp_out = np.zeros_like(tp_out)
    gw = np.zeros((R1, S1), np.int64)
    unb = np.zeros(R1, np.int64)
    K = 0
    for t, ov in enumerate(min_overlaps):
        ranked, gts = matching(case, ov)
        K = len(ranked)
        d_s = [stratum(volume_f32(b), vox[n], edges) for n, b, _ in ranked]
        g_s = [stratum(volume_f32(b), vox[n], edges) for n, b, _ in gts]
        for r in range(R1):
            if t == 0:
                for (n, _, _), s in zip(gts, g_s):
                    gw[r, s] += int(w[r, n])  # s = -1 lands in the last slot
                unb[r] = sum(int(w[r, n]) for (n, _, _), s in zip(ranked, d_s) if s < 0)
            for q in range(cuts.shape[2]):
                k = min(max(int(cuts[r, t, q]), 0), K)
                for (n, _, claim), s in zip(gts, g_s):
                    if claim < k:
                        tp_out[r, t, q, s] += int(w[r, n])
                for (n, _, tp), s in list(zip(ranked, d_s))[:k]:
                    fp_out[r, t, q, s] += int(w[r, n]) * (1 - tp)
    return {"tp": tp_out, "fp": fp_out, "gw": gw, "det_unbinned": unb, "nw": w.sum(1), "cuts": np.clip(cuts, 0, K)}


def same_ints(a, b, what=""):
    for k in ("tp", "fp", "gw", "det_unbinned", "nw", "cuts"):
        assert a[k].dtype == b[k].dtype == np.int64 and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), \
            (what, k, a[k], b[k])
