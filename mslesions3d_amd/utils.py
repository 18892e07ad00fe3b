"""Box utilities and detection metrics — host-side mirror of the reference's ``lesions3d/utils.py:25-396``.

* Box transforms / IoU (``utils.py:42-149``) run as HIP kernels (``csrc/multibox.hip``) on GPU tensors; there is
  no CPU path for them.
* ``calculate_mAP`` (``utils.py:157-396``) is host-side bookkeeping in the reference (a Python loop per
  detection) and stays host-side here: detections are tiny ragged lists, copied to the host once.
* ``calculate_mAP_device`` computes the same values with one HIP launch (``csrc/metrics.hip``), bit for bit; the fused
  trainer runs that kernel on the detections ``msl_detect_objects`` leaves in device memory (training metrics without a
  host synchronisation per step).
* ``evaluate_detections`` computes the (IoU x score threshold) grid of the reference's ``eval.py`` at dataset scale
  (``csrc/evaluate.hip``: no cap on detections or ground truth), each grid point bit-identical to ``calculate_mAP``.
* ``evaluate_froc`` and ``evaluate_strata`` read what that sweep leaves on the device: FROC with bootstrap intervals, and
  sensitivity / false positives per lesion-size bin (not in the reference; numpy twins ``froc_host``, ``strata_host``).
"""
import numpy as np
import torch

from . import _lib
from ._lib import ptr

device = torch.device("cuda" if torch.cuda.is_available() else "cpu")

# Label map (utils.py:25-30)
voc_labels = tuple(["lesion"])
label_map = {k: v + 1 for v, k in enumerate(voc_labels)}
label_map['background'] = 0
rev_label_map = {v: k for k, v in label_map.items()}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _gpu(t, what):
    if not t.is_cuda:
        raise _lib.HipKernelError(f"{what}: expected a tensor on the HIP device (no CPU fallback)")
    return t.contiguous().float()


def _transform(boxes, priors, op, what):
    boxes = _gpu(boxes, what)
    if priors is not None:
        priors = _gpu(priors, what)
        assert priors.shape == boxes.shape
    out = torch.empty_like(boxes)
    _lib.call("msl_box_transform", ptr(boxes), ptr(priors), ptr(out), boxes.shape[0], op, _stream())
    return out


def cxcycz_to_xyz(cxcycz):
    """utils.py:42-51."""
    return _transform(cxcycz, None, 0, "cxcycz_to_xyz")


def xyz_to_cxcycz(xy):
    """utils.py:92-102."""
    return _transform(xy, None, 1, "xyz_to_cxcycz")


def cxcycz_to_gcxgcygcz(cxcycz, priors_cxcycz):
    """utils.py:71-89."""
    return _transform(cxcycz, priors_cxcycz, 2, "cxcycz_to_gcxgcygcz")


def gcxgcygcz_to_cxcycz(gcxgcygcz, priors_cxcycz):
    """utils.py:54-68."""
    return _transform(gcxgcygcz, priors_cxcycz, 3, "gcxgcygcz_to_cxcycz")


def _pairwise(set_1, set_2, inter_only, what):
    a, b = _gpu(set_1, what), _gpu(set_2, what)
    out = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
    _lib.call("msl_iou_matrix", ptr(a), ptr(b), ptr(out), a.shape[0], b.shape[0], inter_only, _stream())
    return out


def find_intersection3d(set_1, set_2):
    """utils.py:105-122."""
    return _pairwise(set_1, set_2, 1, "find_intersection3d")


def find_jaccard_overlap3d(set_1, set_2):
    """utils.py:125-149."""
    return _pairwise(set_1, set_2, 0, "find_jaccard_overlap3d")


def volume(box):
    """utils.py:152-154."""
    return (box[3] - box[0]) * (box[4] - box[1]) * (box[5] - box[2])


# ----------------------------------------------------------------------------------------------------------
# metrics (host side)

def _np(t, dtype=None):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return a.astype(dtype) if dtype is not None else a


def _iou_one_to_many(box, others):
    """fp32, same operation order as utils.py:105-149."""
    lo = np.maximum(box[None, :3], others[:, :3])
    hi = np.minimum(box[None, 3:], others[:, 3:])
    ext = np.clip(hi - lo, 0, None).astype(np.float32)
    inter = ext[:, 0] * ext[:, 1] * ext[:, 2]
    va = (box[3] - box[0]) * (box[4] - box[1]) * (box[5] - box[2])
    vb = (others[:, 3] - others[:, 0]) * (others[:, 4] - others[:, 1]) * (others[:, 5] - others[:, 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / (va + vb - inter)


def compute_metrics_per_class(det_class_images, det_class_boxes, det_class_scores, true_class_images, true_class_boxes,
                              true_class_difficulties, min_overlap):
    """utils.py:157-239 (numpy arrays in, numpy arrays out).  Detections are visited in stable descending score
    order; a detection is a true positive iff its best-IoU (first max) ground truth in the same image has
    IoU > min_overlap, is not 'difficult' and is not claimed yet."""
    order = np.lexsort((np.arange(det_class_scores.shape[0]), -det_class_scores.astype(np.float64)))
    det_class_images, det_class_boxes, det_class_scores = det_class_images[order], det_class_boxes[order], det_class_scores[order]
    detected = np.zeros(true_class_boxes.shape[0], dtype=np.uint8)
    tp = np.zeros(det_class_boxes.shape[0], dtype=np.float32)
    fp = np.zeros(det_class_boxes.shape[0], dtype=np.float32)
    for d in range(det_class_boxes.shape[0]):
        same = np.nonzero(true_class_images == det_class_images[d])[0]
        if same.size == 0:
            fp[d] = 1
            continue
        ov = _iou_one_to_many(det_class_boxes[d], true_class_boxes[same])
        ind = int(np.argmax(ov))  # first maximum
        if ov[ind] > min_overlap:
            if not true_class_difficulties[same[ind]]:
                if detected[same[ind]] == 0:
                    tp[d] = 1
                    detected[same[ind]] = 1
                else:
                    fp[d] = 1
        else:
            fp[d] = 1
    vols = np.array([volume(b) for b, dif in zip(true_class_boxes, true_class_difficulties) if not dif], dtype=np.float32)
    return tp, fp, detected, det_class_scores, vols[detected == 1], vols[detected == 0]


def calculate_mAP(det_boxes, det_labels, det_scores, true_boxes, true_labels, true_difficulties, min_overlap=0.5,
                  return_detail=False):
    """utils.py:242-396.  Inputs: lists (one entry per image) of tensors (any device) or arrays.
    Returns ``(APs, mAP)`` or, with ``return_detail``, the reference's detail dict (torch CPU tensors / floats).

    This is the literal mirror of the reference, 'difficult' flags included, and the device paths do not reproduce those
    flags' semantics because the reference's are broken twice: utils.py:230-233 indexes a volume vector that has the
    difficult boxes removed with a mask that still has them (IndexError as soon as a flag is set - the mirror above keeps
    the mask consistent instead), and utils.py:323-324 still counts difficult boxes as false negatives in ``recall``.
    Ground truth that must not count is expressed with ``true_ignore`` of ``evaluate_detections`` / ``evaluate_froc`` /
    ``evaluate_strata``, whose semantics are defined there, not copied from the reference."""
    assert len(det_boxes) == len(det_labels) == len(det_scores) == len(true_boxes) == len(true_labels) == len(true_difficulties)
    n_classes = len(label_map)
    n_img = len(true_labels)
    t_img = np.concatenate([np.full(len(true_labels[i]), i, dtype=np.int64) for i in range(n_img)])
    t_box = np.concatenate([_np(b, np.float32).reshape(-1, 6) for b in true_boxes])
    t_lab = np.concatenate([_np(l, np.int64) for l in true_labels])
    t_dif = np.concatenate([_np(d).astype(bool) for d in true_difficulties])
    assert t_img.shape[0] == t_box.shape[0] == t_lab.shape[0]
    d_img = np.concatenate([np.full(len(det_labels[i]), i, dtype=np.int64) for i in range(n_img)])
    d_box = np.concatenate([_np(b, np.float32).reshape(-1, 6) for b in det_boxes])
    d_lab = np.concatenate([_np(l, np.int64) for l in det_labels])
    d_sco = np.concatenate([_np(s, np.float32) for s in det_scores])
    assert d_img.shape[0] == d_box.shape[0] == d_lab.shape[0] == d_sco.shape[0]

    average_precisions = np.zeros(n_classes - 1, dtype=np.float32)
    per = {}
    n_easy = 0
    for c in range(1, n_classes):
        ts, ds = t_lab == c, d_lab == c
        n_easy = int((~t_dif[ts]).sum())
        if ds.sum() == 0:
            continue
        tp, fp, detected, sorted_scores, found, not_found = compute_metrics_per_class(
            d_img[ds], d_box[ds], d_sco[ds], t_img[ts], t_box[ts], t_dif[ts], min_overlap)
        fn = np.float32((1 - detected.astype(np.float32)).sum())
        tps = np.float32(tp.sum())
        with np.errstate(invalid="ignore", divide="ignore"):
            recall = tps / (tps + fn)
            precision = tps / (tps + np.float32(fp.sum()))
            f1 = (2 * precision * recall) / (precision + recall)
            ctp, cfp = np.cumsum(tp, dtype=np.float32), np.cumsum(fp, dtype=np.float32)
            cprec = ctp / (ctp + cfp + np.float32(1e-10))
            crec = ctp / np.float32(n_easy)
        thresholds = torch.arange(start=0, end=1.1, step=.1).tolist()
        precs = np.zeros(len(thresholds), dtype=np.float32)
        for i, t in enumerate(thresholds):
            above = crec >= t
            precs[i] = cprec[above].max() if above.any() else 0.
        average_precisions[c - 1] = precs.mean(dtype=np.float32)
        per[c] = dict(tp=tp, fp=fp, detected=detected, scores=sorted_scores, found=found, not_found=not_found,
                      recall=float(recall), precision=float(precision), f1=float(f1))

    mean_average_precision = float(average_precisions.mean())
    aps = {rev_label_map[c + 1]: float(v) for c, v in enumerate(average_precisions.tolist())}
    if not return_detail:
        return aps, mean_average_precision
    T = torch.from_numpy
    if 1 in per:  # n_classes == 2 in the reference (utils.py:359-369)
        p = per[1]
        return {"APs": aps[rev_label_map[1]], "mAP": mean_average_precision, "precision": p["precision"],
                "recall": p["recall"], "f1_score": p["f1"], "sorted_det_scores": {1: T(p["scores"])},
                "TP": T(p["tp"]), "FP": T(p["fp"]), "n_true_boxes": int(p["detected"].shape[0]),
                "found_boxes_volumes_per_class": T(p["found"]), "not_found_boxes_volumes_per_class": T(p["not_found"])}
    vols = np.array([volume(b) for b in t_box], dtype=np.float32)  # utils.py:370-380: nothing detected
    return {"APs": 0., "mAP": mean_average_precision, "precision": 0., "recall": 0., "f1_score": 0.,
            "sorted_det_scores": {}, "TP": torch.zeros(0), "FP": torch.zeros(0), "n_true_boxes": n_easy,
            "found_boxes_volumes_per_class": torch.zeros(0), "not_found_boxes_volumes_per_class": T(vols)}


# ----------------------------------------------------------------------------------------------------------
# metrics (device side, csrc/metrics.hip)

METRIC_SUMMARY = 8  # per threshold: AP, mAP, precision, recall, f1, n_true_boxes, class-1 detections, TP count
_recall_tables = {}


def recall_thresholds(dev):
    """The 11 recall thresholds of utils.py:336 as f32 device table (the f32 values of ``torch.arange(0, 1.1, .1)``)."""
    t = _recall_tables.get(dev)
    if t is None:
        t = _recall_tables[dev] = torch.arange(start=0, end=1.1, step=.1).to(device=dev, dtype=torch.float32)
    return t


def metric_capacity_check(N, top_k, G, n_thr):
    """Host planning of ``msl_detection_metrics``: raise instead of truncating a batch the kernel cannot hold."""
    lib = _lib.load()
    if N * top_k > lib.msl_detection_metrics_max(0):
        raise _lib.HipKernelError(f"detection metrics: {N} images x {top_k} detection slots exceed the kernel's "
                                  f"{lib.msl_detection_metrics_max(0)} detections per batch")
    if G > lib.msl_detection_metrics_max(1):
        raise _lib.HipKernelError(f"detection metrics: {G} ground-truth boxes exceed the kernel's "
                                  f"{lib.msl_detection_metrics_max(1)} per batch")
    if not 0 < n_thr <= lib.msl_detection_metrics_max(2):
        raise _lib.HipKernelError(f"detection metrics: {n_thr} IoU thresholds")


def metric_out_size(n_thr, D, G):
    """f32 elements of one result buffer: [summary | sorted scores | TP | FP | GT status | GT volumes]."""
    return n_thr * METRIC_SUMMARY + D + 2 * n_thr * D + n_thr * G + G


def _metric_views(out, n_thr, D, G):
    sizes = [("summary", n_thr * METRIC_SUMMARY), ("scores", D), ("tp", n_thr * D), ("fp", n_thr * D),
             ("status", n_thr * G), ("vol", G)]
    v, o = {}, 0
    for name, n in sizes:
        v[name] = out[o:o + n]
        o += n
    v["summary"] = v["summary"].reshape(n_thr, METRIC_SUMMARY)
    for name in ("tp", "fp", "status"):
        v[name] = v[name].reshape(n_thr, -1)
    return v


def launch_detection_metrics(ob, os_, ol, oc, gt_boxes, gt_labels, obj_off, G, thresholds, out, accum=None, stream=None):
    """Enqueue ``msl_detection_metrics`` (no synchronisation): detections in msl_detect_objects' layout (ob (N,k,6),
    os_ (N,k), ol (N,k) i64, oc (>= N) i32), packed ground truth, f32 device table of IoU thresholds, ``out`` of
    ``metric_out_size`` f32 elements; ``accum`` (n_thr*4+1 f64) collects per-step sums."""
    N, top_k = ol.shape
    n_thr, D = thresholds.numel(), N * top_k
    metric_capacity_check(N, top_k, G, n_thr)
    v = _metric_views(out, n_thr, D, G)
    _lib.call("msl_detection_metrics", ptr(ob), ptr(os_), ptr(ol), ptr(oc), N, top_k, ptr(gt_boxes), ptr(gt_labels),
              ptr(obj_off), G, ptr(thresholds), n_thr, ptr(recall_thresholds(ob.device)), ptr(v["summary"]), ptr(v["tp"]),
              ptr(v["fp"]), ptr(v["scores"]), ptr(v["status"]), ptr(v["vol"]), ptr(accum),
              _stream() if stream is None else stream)


def _detail_dict(sm, scores, tp, fp, vol, status):
    """calculate_mAP's ``return_detail`` dict (same keys, same types) from host copies of one grid point's device results:
    ``sm`` its METRIC_SUMMARY values (sm[6] = K, the class-1 detections kept), ``scores`` / ``tp`` / ``fp`` in rank order
    (first K entries used), ``vol`` every ground-truth volume, ``status`` per ground-truth box (1 detected, 0 not, 2 not
    class 1)."""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    K = int(sm[6])
    if K == 0:  # utils.py:370-380: nothing detected (every ground-truth volume, whatever its label, is "not found")
        return {"APs": 0., "mAP": float(sm[1]), "precision": 0., "recall": 0., "f1_score": 0., "sorted_det_scores": {},
                "TP": torch.zeros(0), "FP": torch.zeros(0), "n_true_boxes": int(sm[5]),
                "found_boxes_volumes_per_class": torch.zeros(0), "not_found_boxes_volumes_per_class": T(vol)}
    return {"APs": float(sm[0]), "mAP": float(sm[1]), "precision": float(sm[2]), "recall": float(sm[3]),
            "f1_score": float(sm[4]), "sorted_det_scores": {1: T(scores[:K])}, "TP": T(tp[:K]),
            "FP": T(fp[:K]), "n_true_boxes": int(sm[5]), "found_boxes_volumes_per_class": T(vol[status == 1]),
            "not_found_boxes_volumes_per_class": T(vol[status == 0])}


def metric_details(host_out, n_thr, D, G, t):
    """Threshold ``t``'s detail dict (calculate_mAP's ``return_detail`` form: same keys, same types) from a host copy of a
    result buffer.  ``G``: the batch's number of ground-truth boxes."""
    v = _metric_views(np.asarray(host_out, dtype=np.float32), n_thr, D, G)
    return _detail_dict(v["summary"][t], v["scores"], v["tp"][t], v["fp"][t], v["vol"], v["status"][t])


def calculate_mAP_device(det_boxes, det_labels, det_scores, true_boxes, true_labels, true_difficulties, min_overlap=0.5,
                         return_detail=False):
    """``calculate_mAP`` (utils.py:242-396) on the HIP device: same parameters, same return values, bit for bit.
    Inputs: lists (one entry per image) of device tensors.  The ragged lists are packed into the padded layout of
    ``msl_detect_objects``; one launch, one device-to-host copy of the results.  'difficult' ground truth (never set in
    this repository) is not supported."""
    from .ssd3d import MultiBoxLoss
    assert len(det_boxes) == len(det_labels) == len(det_scores) == len(true_boxes) == len(true_labels) == len(true_difficulties)
    if any(bool(torch.as_tensor(d).bool().any()) for d in true_difficulties):
        raise NotImplementedError("calculate_mAP_device: 'difficult' ground-truth boxes are not supported (ground truth "
                                  "that must not be scored: true_ignore of evaluate_detections, DESIGN.md section 4.6d)")
    N = len(true_labels)
    dev = next((t.device for t in list(det_boxes) + list(true_boxes) if torch.is_tensor(t) and t.is_cuda), None)
    if dev is None:
        raise _lib.HipKernelError("calculate_mAP_device: expected tensors on the HIP device (no CPU fallback)")
    counts = [int(l.shape[0]) for l in det_labels]
    top_k = max([1] + counts)
    gb, gl, off, G = MultiBoxLoss.pack_targets([b.reshape(-1, 6) for b in true_boxes], [l.reshape(-1) for l in true_labels], dev)
    metric_capacity_check(N, top_k, G, 1)
    ob = torch.zeros((N, top_k, 6), dtype=torch.float32, device=dev)
    os_ = torch.zeros((N, top_k), dtype=torch.float32, device=dev)
    ol = torch.zeros((N, top_k), dtype=torch.int64, device=dev)
    for i, k in enumerate(counts):
        if k:
            ob[i, :k] = det_boxes[i].reshape(-1, 6).to(device=dev, dtype=torch.float32)
            os_[i, :k] = det_scores[i].reshape(-1).to(device=dev, dtype=torch.float32)
            ol[i, :k] = det_labels[i].reshape(-1).to(device=dev, dtype=torch.int64)
    oc = torch.tensor(counts, dtype=torch.int32).to(dev)
    thr = torch.tensor([min_overlap], dtype=torch.float32).to(dev)
    out = torch.empty(metric_out_size(1, N * top_k, G), dtype=torch.float32, device=dev)
    launch_detection_metrics(ob, os_, ol, oc, gb, gl, off, G, thr, out)
    d = metric_details(out.cpu().numpy(), 1, N * top_k, G, 0)  # the one device-to-host copy
    if not return_detail:
        return {rev_label_map[1]: d["APs"]}, d["mAP"]
    return d


# ----------------------------------------------------------------------------------------------------------
# dataset-scale evaluation (device side, csrc/evaluate.hip): the (IoU x score threshold) grid of the reference's eval.py

def _host(x, dtype):
    return torch.as_tensor(x).detach().to(device="cpu", dtype=dtype)


def evaluate_capacity_check(D, N, G, n_iou, n_sc, ignore=False):
    """Host planning of ``msl_evaluate_detections``: its workspace size in bytes, or HipKernelError for sizes it cannot
    index (the limits are int32 indexing and memory; there is no fixed cap).  ``ignore``: the size
    ``msl_evaluate_detections_ign`` takes with ignore flags."""
    if N <= 0 or n_iou <= 0 or n_sc <= 0:
        raise _lib.HipKernelError(f"evaluate_detections: {N} images, {n_iou} IoU thresholds, {n_sc} score thresholds")
    lib = _lib.load()
    ws = (lib.msl_evaluate_workspace_bytes_ign if ignore else lib.msl_evaluate_workspace_bytes)(D, N, G, n_iou, n_sc)
    if ws == 0:
        raise _lib.HipKernelError(f"evaluate_detections: {D} detections, {N} images, {G} ground-truth boxes x {n_iou} IoU "
                                  f"thresholds x {n_sc} score thresholds exceed int32 indexing")
    return ws


def ignore_flags(true_ignore, true_labels):
    """``true_ignore`` (None, or one bool tensor / array per image, aligned with ``true_boxes``) -> None, or a list of
    (n_i,) bool arrays.  A list of another length, or an entry whose length is not its image's number of boxes:
    ValueError (before anything is packed or launched)."""
    if true_ignore is None:
        return None
    if len(true_ignore) != len(true_labels):
        raise ValueError(f"true_ignore: {len(true_ignore)} entries for {len(true_labels)} images")
    out = []
    for i, (f, l) in enumerate(zip(true_ignore, true_labels)):
        f = _np(f).astype(bool).reshape(-1)
        n = int(_np(l).reshape(-1).shape[0])
        if f.shape[0] != n:
            raise ValueError(f"true_ignore: image {i} has {f.shape[0]} flags for {n} ground-truth boxes")
        out.append(f)
    return out


def ignore_below(true_boxes, voxels, min_size):
    """The flags ``eval.py --ignore_below`` sets: per image, ``size < min_size`` with the size ``evaluate_strata`` bins by
    (the f32 bounding-box volume times the image's voxel count, one f64 multiply).  A NaN size is not below anything."""
    vox = _strata_voxels(voxels, len(true_boxes))
    with np.errstate(invalid="ignore"):
        return [_volume_f32(_np(b, np.float32)).astype(np.float64) * vox[i] < float(min_size) for i, b in enumerate(true_boxes)]


def prepare_evaluation(det_boxes, det_labels, det_scores, true_boxes, true_labels, min_overlaps, min_scores,
                       true_ignore=None):
    """Pack one evaluation for ``msl_evaluate_detections``: the detections into one host buffer with one host-to-device
    copy, the ground truth with ``MultiBoxLoss.pack_targets``, the workspace and the result buffer allocated.  Returns a
    dict with ``launch()`` (enqueue the whole pipeline on the current stream, no synchronisation), ``out`` (the device
    result buffer) and the sizes.  With ``true_ignore`` (see ``ignore_flags``) the call is
    ``msl_evaluate_detections_ign`` on its larger workspace, and the dict also has ``absorbed`` (device int32: (n_iou, n_sc)
    absorbed counts | (n_iou, D) absorbed flags in rank order); ``None`` is the path without flags, unchanged."""
    from .ssd3d import MultiBoxLoss
    ious, scs = list(min_overlaps), list(min_scores)
    N, n_iou, n_sc = len(true_labels), len(ious), len(scs)
    ign = ignore_flags(true_ignore, true_labels)
    dev = next((t.device for t in [*det_boxes, *det_scores, *true_boxes] if torch.is_tensor(t) and t.is_cuda), None)
    if dev is None:
        if not torch.cuda.is_available():
            raise _lib.HipKernelError("evaluate_detections: needs the HIP device (no CPU fallback)")
        dev = torch.device("cuda", torch.cuda.current_device())
    boxes = [_host(b, torch.float32).reshape(-1, 6) for b in det_boxes]
    scores = [_host(s, torch.float32).reshape(-1, 1) for s in det_scores]
    labels = [_host(l, torch.int64).reshape(-1, 1) for l in det_labels]
    counts = [b.shape[0] for b in boxes]
    assert counts == [s.shape[0] for s in scores] == [l.shape[0] for l in labels]
    D = sum(counts)
    gb, gl, goff, G = MultiBoxLoss.pack_targets([_host(b, torch.float32).reshape(-1, 6) for b in true_boxes],
                                                [_host(l, torch.int64).reshape(-1) for l in true_labels], dev)
    ws_bytes = evaluate_capacity_check(D, N, G, n_iou, n_sc, ignore=ign is not None)
    # one host buffer, one copy: detection rows (D,8) [box, score, label as f32] | det_off (N+1) i32 | IoU thresholds f32 |
    # (8-byte aligned) score thresholds f64
    det_off = np.zeros(N + 1, dtype=np.int32)
    det_off[1:] = np.cumsum(counts)
    rows = torch.cat([torch.cat(boxes), torch.cat(scores), torch.cat(labels).to(torch.float32)], 1) if D else torch.zeros((0, 8))
    o_off = D * 8
    o_iou = o_off + N + 1
    o_sc = o_iou + n_iou + ((o_iou + n_iou) & 1)
    packed = torch.cat([rows.reshape(-1), torch.from_numpy(det_off).view(torch.float32),
                        torch.tensor(ious, dtype=torch.float32), torch.zeros(o_sc - o_iou - n_iou),
                        torch.tensor(scs, dtype=torch.float64).view(torch.float32)]).to(dev)
    base = packed.data_ptr()
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty(n_iou * n_sc * METRIC_SUMMARY + D + n_iou * D + n_iou * G + G, dtype=torch.float32, device=dev)
    recall = recall_thresholds(dev)
    args = (base, base + 4 * o_off, D, N, ptr(gb), ptr(gl), ptr(goff), G, base + 4 * o_iou, n_iou, base + 4 * o_sc, n_sc,
            ptr(recall), ptr(ws), ws_bytes, ptr(out))

    absorbed = gi = None
    if ign is not None:
        flat = np.concatenate(ign + [np.zeros(0, bool)]).astype(np.uint8)
        gi = torch.from_numpy(flat if G else np.zeros(1, np.uint8)).to(dev)
        absorbed = torch.empty(n_iou * n_sc + n_iou * D, dtype=torch.int32, device=dev)

    def launch():
        if ign is None:
            _lib.call("msl_evaluate_detections", *args, _stream())
        else:
            _lib.call("msl_evaluate_detections_ign", *args, ptr(gi), ptr(absorbed), _stream())

    # "ws" / "ws_bytes" / "sorted_scores": what msl_evaluate_froc consumes after launch() on the same stream;
    # msl_evaluate_strata also reads "det_rows" and "obj_off" (device addresses of this call's inputs)
    return {"launch": launch, "out": out, "D": D, "N": N, "G": G, "ious": ious, "scores": scs,
            "ws": ws, "ws_bytes": ws_bytes, "sorted_scores": out[n_iou * n_sc * METRIC_SUMMARY:n_iou * n_sc * METRIC_SUMMARY + D],
            "det_rows": base, "obj_off": ptr(goff), "absorbed": absorbed, "args": args, "gt_ignore": gi,
            "keep": (packed, ws, gb, gl, goff, recall, gi)}


def evaluate_detections(det_boxes, det_labels, det_scores, true_boxes, true_labels, true_difficulties,
                        min_overlaps=(0.5,), min_scores=(0.0,), return_detail=False, true_ignore=None):
    """The grid of the reference's eval.py on the HIP device: ``{(min_overlap, min_score): calculate_mAP(<the detections
    with score >= min_score>, ..., min_overlap=min_overlap, return_detail=return_detail)}``, bit for bit, NaNs included.
    A detection is kept iff ``float(score) >= float(min_score)`` (f64, as eval.py's retrieve_boxes compares).

    Inputs: lists (one entry per image) of tensors on any device, or arrays.  The detections are packed on the host and
    copied to the device once; the ground truth is packed by ``MultiBoxLoss.pack_targets``; every grid point comes from
    one enqueue of ``msl_evaluate_detections`` and one device-to-host copy.  No cap on detections or ground truth.
    'difficult' ground truth is not supported.

    ``true_ignore`` (one bool tensor / array per image, aligned with ``true_boxes``): a class-1 box
    with its flag set is neither hit nor miss.  A detection whose first-maximum-IoU box is ignored and has IoU >
    min_overlap is absorbed (neither TP nor FP, nothing claimed); ``n_true_boxes``, recall and the found / not-found volumes
    cover the other boxes only.  The detail dict then gains ``n_ignored_boxes`` and ``absorbed`` (per rank, beside ``TP``
    and ``FP``), at the price of a second device-to-host copy.  ``None``: the path above, unchanged."""
    assert len(det_boxes) == len(det_labels) == len(det_scores) == len(true_boxes) == len(true_labels) == len(true_difficulties)
    if any(bool(torch.as_tensor(d).bool().any()) for d in true_difficulties):
        raise NotImplementedError("evaluate_detections: 'difficult' ground-truth boxes are not supported (ground truth "
                                  "that must not be scored: the true_ignore keyword, DESIGN.md section 4.6d)")
    plan = prepare_evaluation(det_boxes, det_labels, det_scores, true_boxes, true_labels, min_overlaps, min_scores,
                              true_ignore=true_ignore)
    plan["launch"]()
    ious, scs, D, G = plan["ious"], plan["scores"], plan["D"], plan["G"]
    n_iou, n_sc = len(ious), len(scs)
    n_sum = n_iou * n_sc * METRIC_SUMMARY
    host = (plan["out"] if return_detail else plan["out"][:n_sum]).cpu().numpy()  # the one device-to-host copy
    summary = host[:n_sum].reshape(n_iou, n_sc, METRIC_SUMMARY)
    if not return_detail:
        return {(ious[t], scs[c]): ({rev_label_map[1]: float(summary[t, c, 0])}, float(summary[t, c, 1]))
                for t in range(n_iou) for c in range(n_sc)}
    sorted_scores = host[n_sum:n_sum + D]
    tp = host[n_sum + D:n_sum + D + n_iou * D].reshape(n_iou, D)
    claim = host[n_sum + D + n_iou * D:n_sum + D + n_iou * (D + G)].view(np.int32).reshape(n_iou, G)
    vol = host[n_sum + D + n_iou * (D + G):]
    ab = n_ign = None
    if plan["absorbed"] is not None:
        ab = plan["absorbed"].cpu().numpy()[n_iou * n_sc:].reshape(n_iou, D).astype(np.float32)
        n_ign = int((claim[0] == _IGNORED).sum()) if n_iou else 0
    res = {}
    for t in range(n_iou):
        fp = np.float32(1) - tp[t] if ab is None else np.float32(1) - tp[t] - ab[t]
        for c in range(n_sc):
            K = int(summary[t, c, 6])
            status = np.where(claim[t] < 0, 2, np.where(claim[t] < K, 1, 0))  # ignored boxes (-2) are in neither volume list
            d = _detail_dict(summary[t, c], sorted_scores, tp[t], fp, vol, status)
            if ab is not None:
                d["n_ignored_boxes"] = n_ign
                d["absorbed"] = torch.from_numpy(np.ascontiguousarray(ab[t, :K])) if K else torch.zeros(0)
                if K == 0:  # nothing detected: "not found" lists every volume but the ignored boxes'
                    d["not_found_boxes_volumes_per_class"] = torch.from_numpy(np.ascontiguousarray(vol[claim[t] != _IGNORED]))
            res[(ious[t], scs[c])] = d
    return res


# ----------------------------------------------------------------------------------------------------------
# FROC ("FROC"): sensitivity at fixed numbers of false positives per image, CPM, bootstrap intervals over
# cases.  Not in the reference; the matching rule is calculate_mAP's (rank order and TP flags of the existing pipeline).

FROC_TILE = 1024      # EV_FROC_TILE of csrc/evaluate.hip: ranks one workgroup of ev_froc_kernel takes per step
FROC_MAX_RATES = 16   # EV_FROC_MAX_RATES
FROC_RATE_MAX = 1 << 20
DEFAULT_FP_RATES = ((1, 8), (1, 4), (1, 2), (1, 1), (2, 1), (4, 1), (8, 1))  # false positives per image, as num / den


def froc_rates(fp_rates):
    """-> [(num, den)] of exact positive rationals, each part <= 2^20, at most 16.  An entry is a (num, den) pair or
    anything ``fractions.Fraction`` takes (a float stands for its exact binary value)."""
    from fractions import Fraction
    out = []
    for r in fp_rates:
        f = Fraction(int(r[0]), int(r[1])) if isinstance(r, (tuple, list)) else Fraction(r)
        if not (0 < f.numerator <= FROC_RATE_MAX and 0 < f.denominator <= FROC_RATE_MAX):
            raise ValueError(f"FROC rate {r!r}: a positive rational with numerator and denominator up to 2^20")
        out.append((f.numerator, f.denominator))
    if not 1 <= len(out) <= FROC_MAX_RATES:
        raise ValueError(f"1 .. {FROC_MAX_RATES} FROC rates, got {len(out)}")
    return out


def bootstrap_weights(n_images, n_boot, seed=0):
    """(n_boot + 1, N) int32: row 0 all ones (the plain curve), row r > 0 the multiplicities of the r-th resample of
    ``np.random.default_rng(seed).integers(0, N, size=(n_boot, N))``."""
    N, R = int(n_images), int(n_boot)
    if N <= 0 or R < 0:
        raise ValueError(f"bootstrap_weights: {N} images, {R} resamples")
    w = np.ones((R + 1, N), dtype=np.int32)
    if R:
        draws = np.random.default_rng(seed).integers(0, N, size=(R, N))
        w[1:] = np.stack([np.bincount(d, minlength=N) for d in draws]).astype(np.int32)
    return w


def _froc_weights(weights, N, n_boot, seed):
    if weights is None:
        return bootstrap_weights(N, n_boot, seed)
    w = np.asarray(weights)
    if w.ndim != 2 or w.shape[1] != N or w.shape[0] < 1 or not np.issubdtype(w.dtype, np.integer) or (w < 0).any() \
            or (w > 0x7FFFFFFF).any():
        raise ValueError(f"FROC weights: an integer array (rows, {N}) of values >= 0")
    return np.ascontiguousarray(w, dtype=np.int32)


def _froc_class1(det_boxes, det_labels, det_scores, true_boxes, true_labels, true_ignore=None):
    """The class-1 detections and ground truth as calculate_mAP concatenates them, the per-image ground-truth counts and
    the scores in rank order (compute_metrics_per_class's lexsort).  NaN scores: ValueError.  With ``true_ignore``:
    ``t_ign`` (the flag of every class-1 box) and ``g`` counting the boxes that are not ignored; else ``t_ign`` is None."""
    n_img = len(true_labels)
    ign = ignore_flags(true_ignore, true_labels)
    assert len(det_boxes) == len(det_labels) == len(det_scores) == len(true_boxes) == n_img > 0
    t_lab = [_np(l, np.int64).reshape(-1) for l in true_labels]
    d_lab = [_np(l, np.int64).reshape(-1) for l in det_labels]
    t_img = np.concatenate([np.full(len(l), i, dtype=np.int64) for i, l in enumerate(t_lab)])
    d_img = np.concatenate([np.full(len(l), i, dtype=np.int64) for i, l in enumerate(d_lab)])
    t_box = np.concatenate([_np(b, np.float32).reshape(-1, 6) for b in true_boxes])
    d_box = np.concatenate([_np(b, np.float32).reshape(-1, 6) for b in det_boxes])
    d_sco = np.concatenate([_np(s, np.float32).reshape(-1) for s in det_scores])
    ts, ds = np.concatenate(t_lab) == 1, np.concatenate(d_lab) == 1
    d_img, d_box, d_sco = d_img[ds], d_box[ds], d_sco[ds]
    if np.isnan(d_sco).any():
        raise ValueError("FROC: NaN detection scores")
    order = np.lexsort((np.arange(d_sco.shape[0]), -d_sco.astype(np.float64)))
    t_ign = None if ign is None else np.concatenate(ign + [np.zeros(0, bool)])[ts]
    counted = t_img[ts] if t_ign is None else t_img[ts][~t_ign]
    return {"d_img": d_img, "d_box": d_box, "d_sco": d_sco, "t_img": t_img[ts], "t_box": t_box[ts], "order": order,
            "g": np.bincount(counted, minlength=n_img).astype(np.int64), "N": n_img, "t_ign": t_ign}


def match_with_ignore(c, min_overlap):
    """The matching of DESIGN.md section 4.6d on the class-1 sets of ``_froc_class1`` (``t_ign`` given): detections in rank
    order; the candidate is the first-maximum-IoU box of the image over ALL its class-1 boxes; IoU > f32(min_overlap) and
    the candidate ignored: absorbed (nothing claimed); not ignored: TP if unclaimed (it claims the box), else FP; anything
    else FP.  -> (tp (K,), absorbed (K,), claim (class-1 boxes,): rank, _NEVER, or _IGNORED), int64."""
    order, t_img, t_box, t_ign = c["order"], c["t_img"], c["t_box"], c["t_ign"]
    img, box = c["d_img"][order], c["d_box"][order]
    K, thr = order.shape[0], np.float32(min_overlap)
    tp, ab = np.zeros(K, dtype=np.int64), np.zeros(K, dtype=np.int64)
    claim = np.where(t_ign, _IGNORED, _NEVER).astype(np.int64)
    for j in range(K):
        same = np.nonzero(t_img == img[j])[0]
        if same.size == 0:
            continue
        ov = _iou_one_to_many(box[j], t_box[same])
        ind = int(np.argmax(ov))  # first maximum; a NaN wins and then fails the compare
        if not ov[ind] > thr:
            continue
        g = same[ind]
        if t_ign[g]:
            ab[j] = 1
        elif claim[g] == _NEVER:
            claim[g] = j
            tp[j] = 1
    return tp, ab, claim


def froc_host(det_boxes, det_labels, det_scores, true_boxes, true_labels, min_overlaps, fp_rates, weights, true_ignore=None):
    """The numpy twin of ``msl_evaluate_froc``: rank order and TP flags from ``compute_metrics_per_class``, then the
    definitions of DESIGN.md "FROC" as written.  -> ``{"k", "tp": (rows, n_iou, n_rates) int64, "gw", "nw": (rows,)
    int64, "scores": the class-1 scores in rank order (K,) f32}``: the integers the kernel writes.  ``true_ignore``
    (DESIGN.md section 4.6d): FPw sums the detections that are neither TP nor absorbed, Gw the boxes that are not ignored;
    the dict gains ``"absorbed"`` (rows, n_iou, n_rates): the weighted absorbed detections among the first k*."""
    c = _froc_class1(det_boxes, det_labels, det_scores, true_boxes, true_labels, true_ignore)
    ious, rates, N = list(min_overlaps), froc_rates(fp_rates), c["N"]
    w = _froc_weights(weights, N, 0, 0).astype(np.int64)
    R1, K = w.shape[0], c["d_sco"].shape[0]
    gw, nw = (w * c["g"][None, :]).sum(1), w.sum(1)
    scores = c["d_sco"][c["order"]]
    img = c["d_img"][c["order"]]
    adm = np.ones(K + 1, dtype=bool)  # prefix lengths a score threshold can realise
    adm[1:K] = scores[:-1] != scores[1:]
    k_out = np.zeros((R1, len(ious), len(rates)), dtype=np.int64)
    tp_out = np.zeros_like(k_out)
    ab_out = np.zeros_like(k_out)
    # int64 holds every product while these stay below 2^63; Python integers otherwise
    big = int(w.max(initial=0)) * K * max(d for _, d in rates) >= 2 ** 63 or \
        int(nw.max(initial=0)) * max(n for n, _ in rates) >= 2 ** 63
    dt = object if big else np.int64
    for t, ov in enumerate(ious):
        tp = ab = np.zeros(K, dtype=np.int64)
        if K and c["t_ign"] is not None:
            tp, ab, _ = match_with_ignore(c, ov)
        elif K:
            tp = compute_metrics_per_class(c["d_img"], c["d_box"], c["d_sco"], c["t_img"], c["t_box"],
                                           np.zeros(c["t_box"].shape[0], dtype=bool), ov)[0].astype(np.int64)
        for r0 in range(0, R1, 128):
            wj = w[r0:r0 + 128][:, img].astype(dt)  # (rows, K): the weight of every ranked detection's image
            TP = np.zeros((wj.shape[0], K + 1), dtype=dt)
            FP = np.zeros((wj.shape[0], K + 1), dtype=dt)
            AB = np.zeros((wj.shape[0], K + 1), dtype=dt)
            TP[:, 1:] = np.cumsum(wj * tp[None, :], axis=1)
            FP[:, 1:] = np.cumsum(wj * (1 - tp - ab)[None, :], axis=1)
            AB[:, 1:] = np.cumsum(wj * ab[None, :], axis=1)
            for ci, (num, den) in enumerate(rates):
                ok = adm[None, :] & (FP * den <= (nw[r0:r0 + 128].astype(dt) * num)[:, None])
                ks = K - np.argmax(ok[:, ::-1], axis=1)  # the largest qualifying admissible k (k = 0 always qualifies)
                k_out[r0:r0 + 128, t, ci] = ks
                tp_out[r0:r0 + 128, t, ci] = TP[np.arange(wj.shape[0]), ks].astype(np.int64)
                ab_out[r0:r0 + 128, t, ci] = AB[np.arange(wj.shape[0]), ks].astype(np.int64)
    out = {"k": k_out, "tp": tp_out, "gw": gw, "nw": nw, "scores": scores}
    if c["t_ign"] is not None:
        out["absorbed"] = ab_out
    return out


def froc_summary(ints, min_overlaps, fp_rates):
    """``{min_overlap: {"rates", "sensitivity", "score_threshold", "cpm", "ci_low", "ci_high", "cpm_ci", "n_cases",
    "n_lesions", "n_boot", "dropped"}}`` from the integers of ``froc_host`` / ``msl_evaluate_froc``.  Row 0 is the plain
    curve (sensitivity NaN without any ground truth); rows 1.. are bootstrap resamples: the interval is
    ``np.percentile(sens[1:], [2.5, 97.5])`` over the rows with Gw > 0, ``dropped`` counts the others; without resamples
    (or with every one dropped) the interval entries are None."""
    rates = froc_rates(fp_rates)
    k, tp, gw, nw, scores = ints["k"], ints["tp"], ints["gw"], ints["nw"], ints["scores"]
    n_boot = int(k.shape[0]) - 1
    keep = np.nonzero(gw[1:] > 0)[0] + 1
    out = {}
    for t, ov in enumerate(min_overlaps):
        sens = [int(tp[0, t, c]) / int(gw[0]) if gw[0] > 0 else float("nan") for c in range(len(rates))]
        thr = [float(scores[int(k[0, t, c]) - 1]) if k[0, t, c] > 0 else float("inf") for c in range(len(rates))]
        d = {"rates": [n / m for n, m in rates], "sensitivity": sens, "score_threshold": thr,
             "cpm": sum(sens) / len(sens), "ci_low": None, "ci_high": None, "cpm_ci": None, "n_cases": int(nw[0]),
             "n_lesions": int(gw[0]), "n_boot": n_boot, "dropped": n_boot - int(keep.size)}
        if keep.size:
            boot = np.array([[int(tp[r, t, c]) / int(gw[r]) for c in range(len(rates))] for r in keep], dtype=np.float64)
            lo, hi = np.percentile(boot, [2.5, 97.5], axis=0)
            d["ci_low"], d["ci_high"] = [float(v) for v in lo], [float(v) for v in hi]
            d["cpm_ci"] = [float(v) for v in np.percentile(boot.mean(axis=1), [2.5, 97.5])]
        out[ov] = d
    return out


def prepare_froc(plan, gt_count, weights, rates):
    """Pack one ``msl_evaluate_froc`` call behind ``plan`` (``prepare_evaluation``): rates, weights and ground-truth counts
    in one host buffer with one host-to-device copy, the result buffer allocated.  Returns ``launch()`` (enqueue on the
    current stream after ``plan["launch"]()``, no synchronisation), ``out`` (device, int64) and the sizes."""
    dev = plan["out"].device
    w = np.ascontiguousarray(weights, dtype=np.int32)
    R1, N, n_iou, n_rates = w.shape[0], plan["N"], len(plan["ious"]), len(rates)
    assert w.shape == (R1, N) and len(gt_count) == N and 1 <= n_rates <= FROC_MAX_RATES
    host = np.concatenate([np.asarray(rates, dtype=np.int64).reshape(-1).view(np.int32), w.reshape(-1),
                           np.asarray(gt_count, dtype=np.int32)])
    packed = torch.from_numpy(host).to(dev)
    base = packed.data_ptr()
    o_w = 4 * n_rates
    out = torch.empty(R1 * n_iou * n_rates * 2 + R1 * 2, dtype=torch.int64, device=dev)
    args = (ptr(plan["ws"]), plan["ws_bytes"], ptr(plan["sorted_scores"]) if plan["D"] else None, plan["D"], N, plan["G"],
            n_iou, base + 4 * (o_w + R1 * N), base + 4 * o_w, R1, base, n_rates, ptr(out))

    def launch():
        _lib.call("msl_evaluate_froc", *args, _stream())

    return {"launch": launch, "out": out, "R1": R1, "n_iou": n_iou, "n_rates": n_rates, "keep": (packed, plan)}


def froc_ints(host_out, R1, n_iou, n_rates, scores):
    """The result buffer of ``msl_evaluate_froc`` (host copy) as the dict ``froc_host`` returns."""
    a = np.asarray(host_out, dtype=np.int64)
    n = R1 * n_iou * n_rates * 2
    kt, gn = a[:n].reshape(R1, n_iou, n_rates, 2), a[n:n + 2 * R1].reshape(R1, 2)
    return {"k": kt[..., 0].copy(), "tp": kt[..., 1].copy(), "gw": gn[:, 0].copy(), "nw": gn[:, 1].copy(), "scores": scores}


def _absorbed_upto(plan, img, k, w):
    """Weighted absorbed detections among the first ``k`` ranks (``k``: (rows, n_iou, n) host integers) from the absorbed
    flags a sweep with ignore flags left in ``plan["absorbed"]``; ``img``: the image of every rank (the host's lexsort is
    the device's rank order).  Reporting only: the flags are the device's, the prefix sums are taken on the host."""
    D, n_iou, n_sc = plan["D"], len(plan["ious"]), len(plan["scores"])
    ab = plan["absorbed"].cpu().numpy()[n_iou * n_sc:].reshape(n_iou, D).astype(np.int64)
    K = img.shape[0]
    out = np.zeros(k.shape, dtype=np.int64)
    for t in range(n_iou):
        for r in range(k.shape[0]):
            cum = np.concatenate([[0], np.cumsum(w[r, img].astype(np.int64) * ab[t, :K])])
            out[r, t] = cum[np.clip(k[r, t], 0, K)]
    return out


def evaluate_froc_ints(det_boxes, det_labels, det_scores, true_boxes, true_labels, min_overlaps, fp_rates, weights,
                       true_ignore=None):
    """``froc_host`` on the HIP device: the sweep of ``prepare_evaluation``, one upload of weights, rates and ground-truth
    counts, ``msl_evaluate_froc`` on the workspace the sweep left, one device-to-host copy.  ``true_ignore``: as
    ``froc_host`` (the sweep is ``msl_evaluate_detections_ign``; ``"absorbed"`` costs further copies)."""
    c = _froc_class1(det_boxes, det_labels, det_scores, true_boxes, true_labels, true_ignore)  # rejects NaN scores
    rates = froc_rates(fp_rates)
    w = _froc_weights(weights, c["N"], 0, 0)
    plan = prepare_evaluation(det_boxes, det_labels, det_scores, true_boxes, true_labels, min_overlaps, [0.0],
                              true_ignore=true_ignore)
    f = prepare_froc(plan, c["g"], w, rates)
    plan["launch"]()
    f["launch"]()
    host = f["out"].cpu().numpy()  # the one device-to-host copy
    ints = froc_ints(host, f["R1"], f["n_iou"], f["n_rates"], c["d_sco"][c["order"]])
    if true_ignore is not None:
        ints["absorbed"] = _absorbed_upto(plan, c["d_img"][c["order"]], ints["k"], w)
    return ints


def ignored_summary(ints, t):
    """The ``absorbed`` entry a summary gains with ``true_ignore``: row 0's absorbed detections per rate / cut at IoU ``t``."""
    return [int(v) for v in ints["absorbed"][0, t]]


def evaluate_froc(det_boxes, det_labels, det_scores, true_boxes, true_labels, min_overlaps=(0.5,),
                  fp_rates=DEFAULT_FP_RATES, n_boot=0, seed=0, weights=None, true_ignore=None):
    """FROC of a detection set on the HIP device -> ``froc_summary``'s dict per IoU threshold.  ``weights`` (rows, N)
    replaces the bootstrap matrix ``bootstrap_weights(N, n_boot, seed)``; its row 0 is reported as the plain curve.
    ``true_ignore``: ignored boxes are no lesions, absorbed detections no false positives; every
    IoU threshold's dict gains ``absorbed`` (the absorbed detections among the first k* of every rate).  ``None``: unchanged."""
    ious = list(min_overlaps)
    w = _froc_weights(weights, len(true_labels), n_boot, seed)
    ints = evaluate_froc_ints(det_boxes, det_labels, det_scores, true_boxes, true_labels, ious, fp_rates, w,
                              true_ignore=true_ignore)
    out = froc_summary(ints, ious, fp_rates)
    if true_ignore is not None:
        for t, ov in enumerate(ious):
            out[ov]["absorbed"] = ignored_summary(ints, t)
    return out


# ----------------------------------------------------------------------------------------------------------
# Eval by lesion size ("Eval by lesion size"): weighted TP / FP counts per size bin at cuts of the rank order.
# Not in the reference, which only lists the found / not-found volumes; the matching rule is calculate_mAP's.

STRATA_MAX_EDGES = 15  # EV_STRATA_MAX_EDGES of csrc/evaluate.hip
STRATA_MAX_CUTS = 32   # EV_STRATA_MAX_CUTS
_NEVER = 0x7FFFFFFF    # claim rank of a ground-truth box nobody claimed
_IGNORED = -2          # claim entry of an ignored class-1 box (IGNORED of csrc/evaluate.hip)


def strata_edges(size_edges):
    """-> (m,) f64: 1 .. 15 finite, strictly ascending bin edges (in voxels of the frame ``voxels`` counts)."""
    e = np.asarray(list(size_edges), dtype=np.float64).reshape(-1)
    if not 1 <= e.size <= STRATA_MAX_EDGES or not np.isfinite(e).all() or (np.diff(e) <= 0).any():
        raise ValueError(f"size edges: 1 .. {STRATA_MAX_EDGES} finite, strictly ascending values, got {size_edges!r}")
    return e


def _strata_voxels(voxels, N):
    v = np.asarray(voxels, dtype=np.float64).reshape(-1)
    v = np.full(N, v[0]) if v.size == 1 else v
    if v.shape != (N,) or not np.isfinite(v).all() or (v <= 0).any():
        raise ValueError(f"voxels: one finite value > 0 per image ({N}), or one for all")
    return np.ascontiguousarray(v)


def _volume_f32(boxes):
    """``volume`` of every row in f32, left to right."""
    b = np.asarray(boxes, np.float32).reshape(-1, 6)
    return (b[:, 3] - b[:, 0]) * (b[:, 4] - b[:, 1]) * (b[:, 5] - b[:, 2])


def size_stratum(vol_f32, voxels, edges):
    """Stratum of every box: the number of edges <= ``float64(vol_f32) * voxels``; -1 where that size is NaN."""
    with np.errstate(invalid="ignore"):
        v = np.asarray(vol_f32, np.float32).astype(np.float64) * np.asarray(voxels, np.float64)
    s = np.searchsorted(edges, v, side="right").astype(np.int64)
    s[np.isnan(v)] = -1
    return s


def _strata_cuts(cuts, R1, n_iou):
    c = np.asarray(cuts)
    if not np.issubdtype(c.dtype, np.integer) or c.ndim not in (1, 3):
        raise ValueError("cuts: integers, (n_cuts,) or (rows, n_iou, n_cuts)")
    c = np.broadcast_to(c if c.ndim == 3 else c[None, None, :], (R1, n_iou, c.shape[-1]))
    if not 1 <= c.shape[2] <= STRATA_MAX_CUTS:
        raise ValueError(f"1 .. {STRATA_MAX_CUTS} cuts, got {c.shape[2]}")
    return np.ascontiguousarray(c, dtype=np.int64)


def strata_cuts_host(det_boxes, det_labels, det_scores, true_boxes, true_labels, min_overlaps, min_scores, fp_rates, weights,
                     true_ignore=None):
    """The cuts ``evaluate_strata`` takes, on the host -> (rows, n_iou, n_sc + n_rates) int64: ``K_c`` of every score
    threshold (class-1 detections with ``float(score) >= float(threshold)``, the same for every row and IoU), then
    ``froc_host``'s ``k*`` of every rate (``fp_rates`` None: none)."""
    c = _froc_class1(det_boxes, det_labels, det_scores, true_boxes, true_labels)
    w = _froc_weights(weights, c["N"], 0, 0)
    ious = list(min_overlaps)
    kc = np.array([int((c["d_sco"].astype(np.float64) >= float(s)).sum()) for s in min_scores], dtype=np.int64)
    cuts = np.broadcast_to(kc[None, None, :], (w.shape[0], len(ious), kc.size))
    if fp_rates is not None:
        k = froc_host(det_boxes, det_labels, det_scores, true_boxes, true_labels, ious, fp_rates, w, true_ignore=true_ignore)["k"]
        cuts = np.concatenate([cuts, k], axis=2)
    return np.ascontiguousarray(cuts, dtype=np.int64)


def _cum_by_slot(values, slots, S1):
    """(n,) int64 values, (n,) slots -> (n + 1, S1): the sum of the first i values per slot."""
    m = np.zeros((values.shape[0] + 1, S1), dtype=np.int64)
    m[np.arange(1, values.shape[0] + 1), slots] = values
    return np.cumsum(m, axis=0)


def strata_host(det_boxes, det_labels, det_scores, true_boxes, true_labels, voxels, size_edges, min_overlaps, weights, cuts,
                true_ignore=None):
    """The numpy twin of ``msl_evaluate_strata``: rank order and TP flags from ``compute_metrics_per_class``, the claim rank
    of a ground-truth box = the rank of the true positive whose first-maximum IoU it is, then the definitions of DESIGN.md
    "Eval by lesion size" as written.  ``cuts``: prefix lengths, (n_cuts,) or (rows, n_iou, n_cuts), clamped to 0 .. K.
    With S strata and slot S the unbinned one -> ``{"tp", "fp": (rows, n_iou, n_cuts, S + 1), "gw": (rows, S + 1),
    "det_unbinned", "nw": (rows,), "cuts": the clamped cuts}``, all int64: the integers the kernel writes.  ``true_ignore``
    (DESIGN.md section 4.6d): an ignored box is in no bin (neither ``gw`` nor ``tp``), an absorbed detection in no ``fp``;
    the dict gains ``"absorbed"`` (rows, n_iou, n_cuts): the weighted absorbed detections below every cut."""
    c = _froc_class1(det_boxes, det_labels, det_scores, true_boxes, true_labels, true_ignore)
    ious, N, edges = list(min_overlaps), c["N"], strata_edges(size_edges)
    vox = _strata_voxels(voxels, N)
    w = _froc_weights(weights, N, 0, 0).astype(np.int64)
    R1, K, S1 = w.shape[0], c["d_sco"].shape[0], edges.size + 2
    cuts = np.clip(_strata_cuts(cuts, R1, len(ious)), 0, K)
    order = c["order"]
    img, box = c["d_img"][order], c["d_box"][order]
    t_img, t_box = c["t_img"], c["t_box"]
    d_slot = size_stratum(_volume_f32(box), vox[img], edges)
    g_slot = size_stratum(_volume_f32(t_box), vox[t_img], edges)
    d_slot[d_slot < 0] = S1 - 1
    g_slot[g_slot < 0] = S1 - 1
    t_ign = c["t_ign"]
    scored = np.ones(t_box.shape[0], dtype=bool) if t_ign is None else ~t_ign  # the boxes that belong to a bin at all
    gw = np.zeros((R1, S1), dtype=np.int64)
    for s in range(S1):
        gw[:, s] = w[:, t_img[scored & (g_slot == s)]].sum(1)
    tp_out = np.zeros((R1, len(ious), cuts.shape[2], S1), dtype=np.int64)
    fp_out = np.zeros_like(tp_out)
    ab_out = np.zeros((R1, len(ious), cuts.shape[2]), dtype=np.int64)
    for t, ov in enumerate(ious):
        tp = ab = np.zeros(K, dtype=np.int64)
        claim = np.full(t_box.shape[0], _NEVER, dtype=np.int64)
        if t_ign is not None:
            tp, ab, claim = match_with_ignore(c, ov)
        else:
            if K:
                tp = compute_metrics_per_class(c["d_img"], c["d_box"], c["d_sco"], t_img, t_box,
                                               np.zeros(t_box.shape[0], dtype=bool), ov)[0].astype(np.int64)
            for j in np.nonzero(tp)[0]:
                same = np.nonzero(t_img == img[j])[0]
                claim[same[int(np.argmax(_iou_one_to_many(box[j], t_box[same])))]] = j
        by_claim = np.argsort(claim, kind="stable")
        by_claim = by_claim[scored[by_claim]]
        for r in range(R1):
            TP = _cum_by_slot(w[r, t_img[by_claim]], g_slot[by_claim], S1)  # boxes in claim-rank order
            FP = _cum_by_slot(w[r, img] * (1 - tp - ab), d_slot, S1)
            k = cuts[r, t]
            tp_out[r, t] = TP[np.searchsorted(claim[by_claim], k, side="left")]  # boxes with claim rank < k
            fp_out[r, t] = FP[k]
            ab_out[r, t] = np.concatenate([[0], np.cumsum(w[r, img] * ab)])[k]
    unb = (w[:, img] * (d_slot == S1 - 1)[None, :]).sum(1) if K else np.zeros(R1, dtype=np.int64)
    out = {"tp": tp_out, "fp": fp_out, "gw": gw, "det_unbinned": unb.astype(np.int64), "nw": w.sum(1), "cuts": cuts}
    if t_ign is not None:
        out["absorbed"] = ab_out
    return out


def strata_ints(host_out, R1, n_iou, n_cuts, S1, cuts=None):
    """The result buffer of ``msl_evaluate_strata`` (host copy) as the dict ``strata_host`` returns."""
    a = np.asarray(host_out, dtype=np.int64)
    n = R1 * n_iou * n_cuts * S1 * 2
    cnt = a[:n].reshape(R1, n_iou, n_cuts, S1, 2)
    tail = a[n + R1 * S1:n + R1 * S1 + 2 * R1].reshape(R1, 2)
    return {"tp": cnt[..., 0].copy(), "fp": cnt[..., 1].copy(), "gw": a[n:n + R1 * S1].reshape(R1, S1).copy(),
            "det_unbinned": tail[:, 0].copy(), "nw": tail[:, 1].copy(), "cuts": cuts}


def prepare_strata(plan, voxels, size_edges, weights, cuts):
    """Pack one ``msl_evaluate_strata`` call behind ``plan`` (``prepare_evaluation``): voxels, edges and weights in one host
    buffer with one host-to-device copy; workspace and result buffer allocated.  ``cuts``: a device int64 tensor (rows,
    n_iou, n_cuts) - whatever wrote it on the current stream before ``launch()`` - or host integers, which ride in the same
    upload.  Returns ``launch()`` (enqueue after ``plan["launch"]()``, no synchronisation), ``out`` (device, int64), the
    device ``cuts`` and the sizes."""
    dev = plan["out"].device
    w = np.ascontiguousarray(weights, dtype=np.int32)
    R1, N, D, G, n_iou = w.shape[0], plan["N"], plan["D"], plan["G"], len(plan["ious"])
    edges, vox = strata_edges(size_edges), _strata_voxels(voxels, N)
    assert w.shape == (R1, N)
    parts = [vox.view(np.int32), edges.view(np.int32)]
    if not torch.is_tensor(cuts):
        parts.append(_strata_cuts(cuts, R1, n_iou).reshape(-1).view(np.int32))
    packed = torch.from_numpy(np.concatenate(parts + [w.reshape(-1)])).to(dev)
    base = packed.data_ptr()
    o_e = 2 * N
    o_c = o_e + 2 * edges.size
    if torch.is_tensor(cuts):
        assert cuts.dtype == torch.int64 and cuts.device == dev and cuts.is_contiguous() and cuts.shape[:2] == (R1, n_iou)
        n_cuts, cuts_ptr, o_w = int(cuts.shape[2]), cuts.data_ptr(), o_c
    else:
        n_cuts = (packed.numel() - o_c - R1 * N) // (2 * R1 * n_iou)
        cuts_ptr, o_w = base + 4 * o_c, o_c + 2 * R1 * n_iou * n_cuts
        cuts = packed[o_c:o_w].view(torch.int64).reshape(R1, n_iou, n_cuts)
    if not 1 <= n_cuts <= STRATA_MAX_CUTS:
        raise ValueError(f"1 .. {STRATA_MAX_CUTS} cuts, got {n_cuts}")
    S1 = edges.size + 2
    ws_bytes = 5 * (D + G)
    ws = torch.empty(max(ws_bytes, 4), dtype=torch.uint8, device=dev)
    out = torch.empty(R1 * n_iou * n_cuts * S1 * 2 + R1 * S1 + R1 * 2, dtype=torch.int64, device=dev)
    args = (ptr(plan["ws"]), plan["ws_bytes"], ptr(plan["out"]), D, N, G, n_iou, len(plan["scores"]),
            plan["det_rows"] if D else None, plan["obj_off"], base, base + 4 * o_e, int(edges.size), base + 4 * o_w, R1, cuts_ptr, n_cuts, ptr(ws), ws_bytes, ptr(out))

    def launch():
        _lib.call("msl_evaluate_strata", *args, _stream())

    return {"launch": launch, "out": out, "cuts": cuts, "R1": R1, "n_iou": n_iou, "n_cuts": n_cuts, "S1": S1, "ws": ws,
            "args": args, "keep": (packed, plan)}


def evaluate_strata_ints(det_boxes, det_labels, det_scores, true_boxes, true_labels, voxels, size_edges, min_overlaps,
                         min_scores, fp_rates, weights, true_ignore=None):
    """``strata_host`` at the cuts of ``strata_cuts_host``, on the HIP device: the sweep of ``prepare_evaluation``, FROC
    when ``fp_rates`` is given, one upload of voxels, edges and weights, ``msl_evaluate_strata`` at cuts that never leave
    the device (``K_c`` from the sweep's summary, ``k*`` from FROC's result), one device-to-host copy.  ``true_ignore``: as
    ``strata_host`` (``"absorbed"`` costs one further copy)."""
    c = _froc_class1(det_boxes, det_labels, det_scores, true_boxes, true_labels, true_ignore)  # rejects NaN scores
    w = _froc_weights(weights, c["N"], 0, 0)
    scs = list(min_scores)
    plan = prepare_evaluation(det_boxes, det_labels, det_scores, true_boxes, true_labels, min_overlaps, scs,
                              true_ignore=true_ignore)
    n_iou, n_sc, R1 = len(plan["ious"]), len(scs), w.shape[0]
    f = prepare_froc(plan, c["g"], w, froc_rates(fp_rates)) if fp_rates is not None else None
    plan["launch"]()
    kc = plan["out"][:n_iou * n_sc * METRIC_SUMMARY].reshape(n_iou, n_sc, METRIC_SUMMARY)[:, :, 6].to(torch.int64)
    cuts = kc[None].expand(R1, n_iou, n_sc)
    if f is not None:
        f["launch"]()
        k = f["out"][:R1 * n_iou * f["n_rates"] * 2].reshape(R1, n_iou, f["n_rates"], 2)[..., 0]
        cuts = torch.cat([cuts, k], dim=2)
    s = prepare_strata(plan, voxels, size_edges, w, cuts.contiguous())
    s["launch"]()
    host = torch.cat([s["out"], s["cuts"].reshape(-1)]).cpu().numpy()  # the one device-to-host copy
    n = s["out"].numel()
    ints = strata_ints(host[:n], R1, n_iou, s["n_cuts"], s["S1"], host[n:].reshape(R1, n_iou, s["n_cuts"]).copy())
    if true_ignore is not None:
        ints["absorbed"] = _absorbed_upto(plan, c["d_img"][c["order"]], ints["cuts"], w)
    return ints


def _ratio(a, b):
    return int(a) / int(b) if b > 0 else float("nan")


def strata_summary(ints, size_edges, min_overlaps, cut_labels):
    """``{min_overlap: {...}}`` from the integers of ``strata_host`` / ``msl_evaluate_strata``.  Per IoU threshold:
    ``edges``, ``n_lesions`` (Gw_s of row 0 per bin), ``cuts`` (one dict per cut: the entries of ``cut_labels`` plus ``k``,
    row 0's prefix length, ``sensitivity`` = TPw / Gw_s per bin, NaN for a bin without lesions, ``fp_per_case`` = FPw / Nw
    per bin and, with bootstrap rows, ``ci_low`` / ``ci_high`` / ``fp_ci_low`` / ``fp_ci_high``), ``dropped`` (per bin: the
    bootstrap rows with Gw_s = 0, left out of that bin's sensitivity interval), ``unbinned`` (row 0: lesions, detections,
    and per cut the true and false positives among them), ``n_cases``, ``n_boot``.  Sizes are bounding-box volumes.  The
    intervals are ``np.percentile(rows 1.., [2.5, 97.5])``; an interval without a row to take it over is None."""
    edges = strata_edges(size_edges)
    tp, fp, gw, nw = ints["tp"], ints["fp"], ints["gw"], ints["nw"]
    R1, n_iou, n_cuts, S1 = tp.shape
    S = S1 - 1
    assert S == edges.size + 1 and n_iou == len(min_overlaps) and n_cuts == len(cut_labels)
    keep = [np.nonzero(gw[1:, s] > 0)[0] + 1 for s in range(S)]
    rows_fp = np.nonzero(nw[1:] > 0)[0] + 1
    pct = lambda vals: [float(v) for v in np.percentile(np.asarray(vals, dtype=np.float64), [2.5, 97.5])]
    out = {}
    for t, ov in enumerate(min_overlaps):
        cut_dicts = []
        for q, label in enumerate(cut_labels):
            d = dict(label)
            d["k"] = int(ints["cuts"][0, t, q])
            d["sensitivity"] = [_ratio(tp[0, t, q, s], gw[0, s]) for s in range(S)]
            d["fp_per_case"] = [_ratio(fp[0, t, q, s], nw[0]) for s in range(S)]
            ci = [pct([_ratio(tp[r, t, q, s], gw[r, s]) for r in keep[s]]) if keep[s].size else None for s in range(S)]
            fci = [pct([_ratio(fp[r, t, q, s], nw[r]) for r in rows_fp]) if rows_fp.size else None for s in range(S)]
            d["ci_low"], d["ci_high"] = [c and c[0] for c in ci], [c and c[1] for c in ci]
            d["fp_ci_low"], d["fp_ci_high"] = [c and c[0] for c in fci], [c and c[1] for c in fci]
            d["unbinned_tp"], d["unbinned_fp"] = int(tp[0, t, q, S]), int(fp[0, t, q, S])
            cut_dicts.append(d)
        out[ov] = {"edges": [float(e) for e in edges], "n_lesions": [int(v) for v in gw[0, :S]], "cuts": cut_dicts,
                   "dropped": [R1 - 1 - int(k.size) for k in keep],
                   "unbinned": {"n_lesions": int(gw[0, S]), "detections": int(ints["det_unbinned"][0])},
                   "n_cases": int(nw[0]), "n_boot": R1 - 1}
    return out


def strata_cut_labels(min_scores, fp_rates):
    """One label per cut, in the order of ``strata_cuts_host``."""
    labels = [{"min_score": float(s)} for s in min_scores]
    if fp_rates is not None:
        labels += [{"fp_rate": n / d} for n, d in froc_rates(fp_rates)]
    return labels


def evaluate_strata(det_boxes, det_labels, det_scores, true_boxes, true_labels, voxels, size_edges, min_overlaps=(0.5,),
                    min_scores=(0.5,), fp_rates=None, n_boot=0, seed=0, weights=None, true_ignore=None):
    """Sensitivity and false positives per case by lesion size on the HIP device -> ``strata_summary``'s dict per IoU
    threshold, at every score threshold of ``min_scores`` and, with ``fp_rates``, at the FROC operating point of every rate.
    ``voxels``: the voxel count of the frame each image's boxes are fractions of (one value, or one per image);
    ``size_edges``: ascending bin edges in voxels.  ``weights`` replaces ``bootstrap_weights(N, n_boot, seed)``.  NaN
    scores: ValueError.  ``true_ignore``: an ignored box belongs to no bin, an absorbed detection
    is no false positive of any; every IoU threshold's dict gains ``absorbed`` (the absorbed detections below every cut).
    ``None``: unchanged."""
    ious, scs = list(min_overlaps), list(min_scores)
    w = _froc_weights(weights, len(true_labels), n_boot, seed)
    ints = evaluate_strata_ints(det_boxes, det_labels, det_scores, true_boxes, true_labels, voxels, size_edges, ious, scs,
                                fp_rates, w, true_ignore=true_ignore)
    out = strata_summary(ints, size_edges, ious, strata_cut_labels(scs, fp_rates))
    if true_ignore is not None:
        for t, ov in enumerate(ious):
            out[ov]["absorbed"] = ignored_summary(ints, t)
    return out


# ---- prior fit report (csrc/priorfit.hip): which lesions the prior boxes can match ---------------
PRIOR_FIT_QUANTILES = (0.0, 0.05, 0.25, 0.5)  # of best_iou: the low end is where lesions are lost


def _prior_fit_boxes(true_boxes):
    """list of per-image (n_i,6) boxes -> list of f32 arrays; a non-finite or inverted box is a ValueError."""
    boxes = [np.ascontiguousarray(_np(b, np.float32).reshape(-1, 6)) for b in true_boxes]
    for n, b in enumerate(boxes):
        if not np.isfinite(b).all():
            raise ValueError(f"prior_fit: image {n} has a non-finite ground-truth box")
        if (b[:, 3:] < b[:, :3]).any():
            raise ValueError(f"prior_fit: image {n} has a ground-truth box with max < min")
    return boxes


def prior_fit_ranges(scale_ranges, P):
    """``{feature map: (lo, hi)}`` (or a list of pairs) -> (S + 1,) int32 offsets: contiguous ascending ranges from 0 to P."""
    pairs = list(scale_ranges.values()) if isinstance(scale_ranges, dict) else list(scale_ranges)
    off = [0]
    for lo, hi in pairs:
        if int(lo) != off[-1] or int(hi) < int(lo):
            raise ValueError(f"scale ranges must be contiguous and ascending from 0, got {pairs}")
        off.append(int(hi))
    if not 1 <= len(pairs) <= _lib.PRIOR_FIT_MAX_SCALES or off[-1] != int(P):
        raise ValueError(f"1 .. {_lib.PRIOR_FIT_MAX_SCALES} scale ranges that end at the number of priors ({P}), got {pairs}")
    return np.asarray(off, dtype=np.int32)


def _prior_fit_thresholds(thresholds):
    thr = np.asarray(list(thresholds), dtype=np.float32).reshape(-1)
    if not 1 <= thr.size <= _lib.PRIOR_FIT_MAX_THRESHOLDS or np.isnan(thr).any():
        raise ValueError(f"1 .. {_lib.PRIOR_FIT_MAX_THRESHOLDS} thresholds (no NaN), got {thresholds!r}")
    return thr


def prepare_prior_fit(true_boxes, dev=None):
    """Validate and upload the ground truth of a data set once -> a plan ``run_prior_fit`` takes any number of times (one
    call per candidate prior set of a sweep).  Raises ValueError for a bad box before anything touches the device."""
    from .ssd3d import MultiBoxLoss
    boxes = _prior_fit_boxes(true_boxes)
    if dev is None:
        if not torch.cuda.is_available():
            raise _lib.HipKernelError("prior_fit: needs the HIP device (no CPU fallback)")
        dev = torch.device("cuda", torch.cuda.current_device())
    gb, _, off, G = MultiBoxLoss.pack_targets([torch.from_numpy(b) for b in boxes],
                                              [torch.zeros(b.shape[0], dtype=torch.int64) for b in boxes], dev)
    image = np.repeat(np.arange(len(boxes), dtype=np.int64), [b.shape[0] for b in boxes])
    return {"gb": gb, "off": off, "G": G, "N": len(boxes), "image": image, "dev": dev}


def run_prior_fit(plan, priors_cxcycz, thresholds, scale_ranges):
    """One ``msl_prior_fit`` call and one device-to-host copy -> dict of CPU tensors over the G ground-truth boxes:
    ``best_iou`` f32, ``best_prior`` / ``best_scale`` / ``held`` / ``image`` i64, ``pos`` (G, n_thr, S) i64."""
    priors = _gpu(priors_cxcycz, "prior_fit").reshape(-1, 6)
    P, G, N = int(priors.shape[0]), plan["G"], plan["N"]
    off, thr = prior_fit_ranges(scale_ranges, P), _prior_fit_thresholds(thresholds)
    if N < 1:
        raise ValueError("prior_fit: no image")
    S, T = off.size - 1, thr.size
    dev = plan["dev"]
    ws_bytes = _lib.load().msl_prior_fit_workspace_bytes(G)
    ws = torch.empty(max(ws_bytes // 8, 1), dtype=torch.int64, device=dev)
    out = torch.empty(max(G * (3 + T * S), 1), dtype=torch.int32, device=dev)  # best_iou bits | best_prior | held | pos
    base = out.data_ptr()
    _lib.call("msl_prior_fit", ptr(plan["gb"]), ptr(plan["off"]), N, G, ptr(priors), P, off.ctypes.data, S, thr.ctypes.data, T,
              ptr(ws), ws_bytes, base, base + 4 * G, base + 8 * G, base + 12 * G, _stream())
    host = out.cpu().numpy()[:G * (3 + T * S)]  # the one device-to-host copy
    best_prior = host[G:2 * G].astype(np.int64)
    return {"best_iou": torch.from_numpy(host[:G].view(np.float32).copy()),
            "best_prior": torch.from_numpy(best_prior),
            "best_scale": torch.from_numpy((np.searchsorted(off, best_prior, side="right") - 1).astype(np.int64)),
            "held": torch.from_numpy(host[2 * G:3 * G].astype(np.int64)),
            "pos": torch.from_numpy(host[3 * G:].astype(np.int64).reshape(G, T, S)),
            "image": torch.from_numpy(plan["image"].copy())}


def prior_fit(true_boxes, priors_cxcycz, thresholds, scale_ranges):
    """What the matching of ``MultiBoxLoss`` gives every ground-truth box, for every threshold at once, on the HIP device
    (``msl_prior_fit``: no (N,P) buffer).  ``true_boxes``: list of per-image (n_i,6) fractional corner boxes;
    ``priors_cxcycz`` (P,6) on the device; ``scale_ranges``: ``LSSD3D.prior_ranges()``.  Per box, in packed order:
    ``best_iou`` / ``best_prior`` (first maximum, before the force-match), ``best_scale`` (the range of that prior),
    ``held`` (1: the box keeps its force-matched prior), ``pos[g, t, s]`` (positive priors of range s at threshold t that
    train on box g; their sum over s is 0 for an orphaned box), ``image``."""
    return run_prior_fit(prepare_prior_fit(true_boxes, priors_cxcycz.device if torch.is_tensor(priors_cxcycz) else None),
                         priors_cxcycz, thresholds, scale_ranges)


def _quantiles(values, qs):
    v = np.asarray(values, dtype=np.float64)
    return [float(x) for x in np.quantile(v, qs)] if v.size else [None] * len(qs)


def prior_fit_summary(fit, true_boxes, voxels, size_edges, thresholds, shapes=None, scale_names=None):
    """Host-side summary of a ``prior_fit`` result (G is small: numpy).  Lesion size and ``size_edges`` mean what they mean
    in ``evaluate_strata``: bounding-box volume in f32 times ``voxels`` of the image (one value, or one per image), stratum
    = number of edges <= size; ``size_edges`` may be empty (the "all" row only).  Per threshold: one row per stratum plus
    "all", each with ``lesions``, ``matchable`` (best_iou >= thr), ``forced_only`` (best_iou < thr and held: positive only
    through the force-match), ``orphaned`` (no positive prior), ``positives`` per lesion (mean / median / max),
    ``positives_per_scale`` (sums), ``best_iou`` quantiles (min, 5 %, 25 %, 50 %); and ``positives_per_image`` (the mean
    over ALL images: the loss normaliser).  ``extent``: box extents per axis (min, quartiles, max), in voxels when
    ``shapes`` (one (D,H,W), or one per image) is given, else as fractions of the frame."""
    boxes = _prior_fit_boxes(true_boxes)
    N = len(boxes)
    flat = np.concatenate(boxes) if boxes else np.zeros((0, 6), np.float32)
    G = flat.shape[0]
    img = np.repeat(np.arange(N), [b.shape[0] for b in boxes])
    host = {k: _np(v) for k, v in fit.items()}
    thr = _prior_fit_thresholds(thresholds)
    pos = host["pos"].reshape(G, thr.size, -1).astype(np.int64)
    best, held = host["best_iou"].astype(np.float32), host["held"].astype(np.int64)
    S = pos.shape[2]
    names = [str(s) for s in (scale_names if scale_names is not None else range(S))]
    assert len(names) == S and best.shape == (G,) and np.array_equal(host["image"], img)
    edges = strata_edges(size_edges) if len(list(size_edges)) else np.zeros(0)
    stratum = size_stratum(_volume_f32(flat), _strata_voxels(voxels, N)[img], edges) if G else np.zeros(0, np.int64)
    groups = [("all", np.ones(G, dtype=bool))]
    if edges.size:
        bounds = [0.0] + [float(e) for e in edges] + [float("inf")]
        groups += [(f"[{bounds[s]:g}, {bounds[s + 1]:g})", stratum == s) for s in range(edges.size + 1)]
    out = {"n_images": N, "n_lesions": G, "edges": [float(e) for e in edges], "scales": names, "thresholds": []}
    for t in range(thr.size):
        total = pos[:, t, :].sum(1)
        rows = []
        for name, m in groups:
            n = int(m.sum())
            rows.append({"stratum": name, "lesions": n,
                         "matchable": int((best[m] >= thr[t]).sum()),
                         "forced_only": int(((best[m] < thr[t]) & (held[m] == 1)).sum()),
                         "orphaned": int((total[m] == 0).sum()),
                         "positives": {"mean": float(total[m].mean()) if n else None,
                                       "median": float(np.median(total[m])) if n else None,
                                       "max": int(total[m].max()) if n else None},
                         "positives_per_scale": {names[s]: int(pos[m, t, s].sum()) for s in range(S)},
                         "best_iou": dict(zip(("min", "q05", "q25", "q50"), _quantiles(best[m], PRIOR_FIT_QUANTILES)))})
        out["thresholds"].append({"threshold": float(thr[t]), "positives_per_image": int(total.sum()) / N if N else None,
                                  "strata": rows})
    ext = flat[:, 3:] - flat[:, :3]
    if shapes is not None:
        sh = np.asarray(shapes, dtype=np.float64).reshape(-1, 3)
        ext = ext.astype(np.float64) * (np.broadcast_to(sh, (N, 3)) if sh.shape[0] == 1 else sh)[img]
    out["extent"] = {"unit": "voxels" if shapes is not None else "fraction",
                     "axes": [dict(zip(("min", "q25", "q50", "q75", "max"), _quantiles(ext[:, a], (0, .25, .5, .75, 1))))
                              for a in range(3)]}
    return out


# ---- box overlays (utils.py:516-617, predict.py:186-220) ----------------------------------------------------------------
DRAW_STYLES = {"edges": 0, "preds": 1}  # msl_draw_boxes's style argument


def draw_boxes(boxes, labels, scores, shape, style, min_score=0.):
    """The box-overlay volumes of the reference on the host -> ``(instances, classes)``, two int16 arrays of ``shape``.

    ``style="edges"`` restates ``make_segmentation_from_bboxes`` (utils.py:559-598) for one image: label 0 is skipped
    (``scores`` and ``min_score`` are not looked at), the voxel box is the fp32 product ``clip(box, 0, 1) * shape``
    truncated to int with ``max = min(max, n - 1)``, and six half-open faces are assigned.  ``style="preds"`` restates
    ``save_predictions_example`` (predict.py:186-220): ``score < min_score`` (compared as ``save_predictions`` compares, in
    f64) and label 0 are skipped, ``max = min(max + 1, n - 1)``, and the six faces, three edge lines and the far corner are
    assigned.  Boxes are applied in ascending j and a later box overwrites an earlier one: a drawn voxel of ``instances``
    holds j + 1 of the last box whose assignments cover it, where j counts every detection, skipped ones included, and
    ``classes`` holds that box's label.  The reference has the class plane for "edges" only; for "preds" it is this
    project's extension.  An assignment on an index the reference would raise IndexError for (a min coordinate >= 1 gives
    index n) writes nothing.  ``msl_draw_boxes`` (csrc/overlay.hip) computes the same volumes on the device, bit for bit."""
    if style not in DRAW_STYLES:
        raise ValueError(f"style must be one of {sorted(DRAW_STYLES)}, got {style!r}")
    shape = tuple(int(n) for n in shape)
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError(f"shape must be three positive sizes, got {shape}")
    boxes = np.asarray(torch.as_tensor(boxes).cpu() if torch.is_tensor(boxes) else boxes, dtype=np.float32).reshape(-1, 6)
    labels = np.asarray(torch.as_tensor(labels).cpu() if torch.is_tensor(labels) else labels).reshape(-1)
    preds = style == "preds"
    if preds:
        scores = np.asarray(torch.as_tensor(scores).cpu() if torch.is_tensor(scores) else scores, dtype=np.float32).reshape(-1)
    if boxes.shape[0] > 32766:
        raise ValueError("draw_boxes: more than 32766 boxes do not fit the int16 ids")
    shape2 = np.asarray(shape * 2, dtype=np.float32)
    planes = np.zeros((2,) + shape, dtype=np.int16)
    for j in range(boxes.shape[0]):
        label = int(labels[j])
        if label == 0 or (preds and float(scores[j]) < min_score):
            continue
        vox = (np.clip(boxes[j], np.float32(0), np.float32(1)) * shape2).astype(int).tolist()
        x0, y0, z0 = vox[:3]
        x1, y1, z1 = (min(v + preds, n - 1) for v, n in zip(vox[3:], shape))
        value = np.array([j + 1, label], dtype=np.int16)[:, None, None]
        # (a fixed index equal to n - only a min can be - is out of range in the reference; nothing is written there)
        if x0 < shape[0]:
            planes[:, x0, y0:y1, z0:z1] = value
        planes[:, x1, y0:y1, z0:z1] = value
        if y0 < shape[1]:
            planes[:, x0:x1, y0, z0:z1] = value
        planes[:, x0:x1, y1, z0:z1] = value
        if z0 < shape[2]:
            planes[:, x0:x1, y0:y1, z0] = value
        planes[:, x0:x1, y0:y1, z1] = value
        if preds:
            planes[:, x0:x1, y1, z1] = value[:, :, 0]
            planes[:, x1, y0:y1, z1] = value[:, :, 0]
            planes[:, x1, y1, z0:z1] = value[:, :, 0]
            planes[:, x1, y1, z1] = value[:, 0, 0]
    return planes[0], planes[1]


def draw_boxes_device(boxes, labels, scores, shape, style, min_score=0., classes=True, out=None):
    """``draw_boxes`` for N images on the HIP device (msl_draw_boxes, one launch per image on the current stream, no
    synchronisation): ``boxes`` / ``labels`` / ``scores`` are lists of N device tensors (or one tensor for N = 1) ->
    ``(instances, classes)``, int16 (N,) + shape on the device; ``classes`` is None when not asked for.  ``out``: a pair
    of buffers to write into (every voxel is written: they need no clearing)."""
    if torch.is_tensor(boxes):
        boxes, labels, scores = [boxes], [labels], [scores]
    if style not in DRAW_STYLES:
        raise ValueError(f"style must be one of {sorted(DRAW_STYLES)}, got {style!r}")
    N, shape = len(boxes), tuple(int(n) for n in shape)
    dev = boxes[0].device
    b = torch.cat([_gpu(x, "draw_boxes_device").reshape(-1, 6) for x in boxes])
    l = torch.cat([x.reshape(-1).to(device=dev, dtype=torch.int64) for x in labels])
    s = torch.cat([_gpu(x, "draw_boxes_device").reshape(-1) for x in scores])
    off = np.concatenate([[0], np.cumsum([x.reshape(-1, 6).shape[0] for x in boxes])]).astype(np.int32)
    if out is None:
        inst = torch.empty((N,) + shape, dtype=torch.int16, device=dev)
        cls = torch.empty((N,) + shape, dtype=torch.int16, device=dev) if classes else None
    else:
        inst, cls = out
    _lib.call("msl_draw_boxes", ptr(b), ptr(l), ptr(s), off.ctypes.data, N, *shape, DRAW_STYLES[style], float(min_score),
              ptr(inst), ptr(cls) if cls is not None else None, _stream())
    return inst, cls


# ---- multi-view prediction: detections of V views of one case merged in the case frame --------
MERGE_MODES = {"nms": 0, "fuse": 1}  # msl_views_merge's mode argument
MERGE_MAX_VIEWS, MERGE_MAX_CANDIDATES = 64, 8192  # msl_views_merge's capacity: V and V * top_k


def _merge_geometry(views, tile, case_shape, margin):
    views = np.ascontiguousarray(np.asarray(views, dtype=np.int32))
    tile, case_shape, margin = (np.asarray(x, dtype=np.int64).reshape(-1) for x in (tile, case_shape, margin))
    if views.ndim != 2 or views.shape[1] != 6 or views.shape[0] < 1 or not np.isin(views[:, 3:], (0, 1)).all():
        raise ValueError("merge_views: views is (V, 6) rows o0, o1, o2, f0, f1, f2 with V >= 1 and 0 / 1 flip flags")
    if not (tile.shape == case_shape.shape == margin.shape == (3,)) or tile.min() < 1 or case_shape.min() < 1 or margin.min() < 0:
        raise ValueError("merge_views: tile, case_shape and margin are three ints each (sizes >= 1, margins >= 0)")
    return views, tile, case_shape, margin


def _owned(centre, origin, tile, case_shape, margin):
    """The ownership test of a centre (..., 3) f32 in case voxels by the view(s) at ``origin`` (..., 3) ints: per axis
    ``c >= o + m`` unless the tile starts at or before the case border, ``c < o + T - m`` unless it ends at or behind it."""
    lo, hi = origin + margin, origin + tile - margin
    return (((origin <= 0) | (centre >= lo.astype(np.float32))) &
            ((origin + tile >= case_shape) | (centre < hi.astype(np.float32)))).all(-1)


def _iou6_rows(a, b):
    """csrc/iou6.hpp on the host: IoU of box ``a`` (6,) with the rows of ``b`` (M, 6), f32, the same operation order."""
    e = np.maximum(np.minimum(a[3:], b[:, 3:]) - np.maximum(a[:3], b[:, :3]), np.float32(0))
    inter = e[:, 0] * e[:, 1] * e[:, 2]
    va = (a[3] - a[0]) * (a[4] - a[1]) * (a[5] - a[2])
    vb = (b[:, 3] - b[:, 0]) * (b[:, 4] - b[:, 1]) * (b[:, 5] - b[:, 2])
    return inter / (va + vb - inter)


def merge_views(boxes, scores, labels, counts, views, tile, case_shape, margin, max_overlap, mode="nms", out_top_k=None):
    """The detections of the V views of one case (``datasets.view_plan``) as ONE list in the case's own frame ->
    ``(boxes (n, 6) f32, labels (n,) i64, scores (n,) f32, support (n,) i32)``, n <= ``out_top_k`` and possibly 0.

    ``boxes`` (V, top_k, 6), ``scores`` (V, top_k), ``labels`` (V, top_k), ``counts`` (V,): what ``msl_detect_objects``
    leaves per view (corner boxes as fractions of the view).  All f32 steps are single rounded operations.

    Map: per axis k a corner pair (a, b) of a view flipped along k becomes (1 - b, 1 - a); voxel x = a * T_k + o_k; case
    fraction x / n_k; nothing is clamped.  Candidates: slots j < counts[v] with label >= 1 (0 is the empty image's
    placeholder) and a score that is not NaN whose centre (x_lo + x_hi) * 0.5 passes the view's ownership test
    (``_owned``): a tile owns its core, out to the case border where it touches it, so of the copies of one lesion in
    overlapping tiles only one is taken.  Per class, ascending: candidates ranked by descending score, ties by ascending
    (view, slot); greedy NMS with ``iou > max_overlap`` on the case-frame boxes; a suppressed candidate is assigned to the
    earliest-ranked kept one that overlaps it; ``support`` of a kept box = distinct views among it and its members.
    ``mode="nms"``: the kept candidate's own box and score.  ``mode="fuse"``: box = sum(s_i * B_i) / sum(s_i) over the
    cluster in rank order, accumulated in f64 and rounded to f32 once; score = the sum over views (ascending) of the view's
    best member score, in f64, over max(cover, support), where cover = the views whose ownership test the kept centre
    passes - a lesion one flip of eight sees is demoted, one all of them see keeps about its mean score.  Output: all
    classes, by descending final score, ties by (class, rank of the kept candidate), the first ``out_top_k``.
    ``msl_views_merge`` (csrc/views.hip) computes the same values on the device, bit for bit."""
    f32 = np.float32
    views, tile, case_shape, margin = _merge_geometry(views, tile, case_shape, margin)
    if mode not in MERGE_MODES:
        raise ValueError(f"merge must be one of {sorted(MERGE_MODES)}, got {mode!r}")
    V = views.shape[0]
    boxes = np.asarray(boxes, dtype=f32).reshape(V, -1, 6)
    K = boxes.shape[1]
    scores = np.asarray(scores, dtype=f32).reshape(V, K)
    labels = np.asarray(labels, dtype=np.int64).reshape(V, K)
    counts = np.asarray(counts, dtype=np.int64).reshape(V)
    out_top_k = V * K if out_top_k is None else int(out_top_k)
    origin, flip = views[:, None, :3].astype(np.int64), views[:, None, 3:] != 0
    lo, hi = boxes[..., :3], boxes[..., 3:]
    a, b = np.where(flip, f32(1) - hi, lo), np.where(flip, f32(1) - lo, hi)
    x_lo, x_hi = a * tile.astype(f32) + origin.astype(f32), b * tile.astype(f32) + origin.astype(f32)
    centre = (x_lo + x_hi) * f32(0.5)
    cand = (np.arange(K)[None, :] < counts[:, None]) & (labels >= 1) & (scores == scores)
    cand &= _owned(centre, origin, tile, case_shape, margin)
    idx = np.flatnonzero(cand.reshape(-1))
    frac = np.concatenate([x_lo / case_shape.astype(f32), x_hi / case_shape.astype(f32)], axis=-1).reshape(-1, 6)[idx]
    sc, lab, view, cen = scores.reshape(-1)[idx], labels.reshape(-1)[idx], idx // K, centre.reshape(-1, 3)[idx]
    order = np.lexsort((idx, -sc, lab))  # class ascending, score descending, (view, slot) ascending
    frac, sc, lab, view, cen = frac[order], sc[order], lab[order], view[order], cen[order]
    M = order.shape[0]
    assign = np.full(M, -1, dtype=np.int64)
    thr = f32(max_overlap)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for k in range(M):
            if assign[k] >= 0:
                continue
            assign[k] = k
            end = k + 1 + int(np.searchsorted(lab[k + 1:], lab[k], side="right"))  # the class ends here
            if end > k + 1:
                over = (_iou6_rows(frac[k], frac[k + 1:end]) > thr) & (assign[k + 1:end] < 0)
                assign[k + 1:end][over] = k
        kept = np.flatnonzero(assign == np.arange(M))
        ob, os_ = np.empty((kept.shape[0], 6), dtype=f32), np.empty(kept.shape[0], dtype=f32)
        support = np.empty(kept.shape[0], dtype=np.int32)
        members = {int(k): [] for k in kept}
        for i in range(M):
            members[int(assign[i])].append(i)  # rank order
        for r, k in enumerate(kept):
            mem = members[int(k)]
            seen = sorted(set(int(view[i]) for i in mem))
            support[r] = len(seen)
            if MERGE_MODES[mode] == 0:
                ob[r], os_[r] = frac[k], sc[k]
                continue
            acc, wsum = np.zeros(6, dtype=np.float64), np.float64(0)
            for i in mem:
                w = np.float64(sc[i])
                acc = acc + w * frac[i].astype(np.float64)
                wsum = wsum + w
            ob[r] = (acc / wsum).astype(f32)
            total = np.float64(0)
            for v in seen:
                total = total + np.float64(max(sc[i] for i in mem if view[i] == v))
            cover = int(_owned(cen[k][None, :], views[:, :3].astype(np.int64), tile, case_shape, margin).sum())
            os_[r] = f32(total / np.float64(max(cover, int(support[r]))))
    final = np.argsort(-os_, kind="stable")[:out_top_k]  # ties: (class, rank of the kept candidate) = position in kept
    return ob[final], lab[kept][final].astype(np.int64), os_[final], support[final]


def merge_views_workspace(V, top_k, dev):
    """Workspace and output buffers of one ``msl_views_merge`` shape (raises beyond its capacity)."""
    nbytes = int(_lib.load().msl_views_merge_workspace_bytes(int(V), int(top_k)))
    if nbytes == 0:
        raise ValueError(f"msl_views_merge takes at most {MERGE_MAX_VIEWS} views and {MERGE_MAX_CANDIDATES} detections "
                         f"(views x top_k), got {V} x {top_k}")
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


def merge_views_device(boxes, scores, labels, counts, views, tile, case_shape, margin, max_overlap, mode="nms",
                       out_top_k=None, workspace=None, out=None):
    """``merge_views`` on the HIP device (msl_views_merge on the current stream, no synchronisation): ``boxes`` (V, top_k,
    6) f32, ``scores`` (V, top_k) f32, ``labels`` (V, top_k) i64 and ``counts`` (V,) i32 are device tensors in
    ``msl_detect_objects``' output layout -> dict of device tensors ``boxes`` (out_top_k, 6), ``scores``, ``labels``,
    ``support`` and ``count`` (1,): rows past ``count`` are not written."""
    views, tile, case_shape, margin = _merge_geometry(views, tile, case_shape, margin)
    if mode not in MERGE_MODES:
        raise ValueError(f"merge must be one of {sorted(MERGE_MODES)}, got {mode!r}")
    V, K = views.shape[0], boxes.shape[1]
    if tuple(boxes.shape) != (V, K, 6) or tuple(scores.shape) != (V, K) or tuple(labels.shape) != (V, K) or counts.numel() != V:
        raise ValueError("merge_views_device: boxes (V, top_k, 6), scores / labels (V, top_k), counts (V,)")
    boxes, scores = _gpu(boxes, "merge_views_device"), _gpu(scores, "merge_views_device")
    dev = boxes.device
    labels, counts = labels.to(device=dev, dtype=torch.int64).contiguous(), counts.to(device=dev, dtype=torch.int32).contiguous()
    out_top_k = V * K if out_top_k is None else int(out_top_k)
    if workspace is None:
        workspace = merge_views_workspace(V, K, dev)
    if out is None:
        out = dict(boxes=torch.empty((out_top_k, 6), dtype=torch.float32, device=dev),
                   scores=torch.empty(out_top_k, dtype=torch.float32, device=dev),
                   labels=torch.empty(out_top_k, dtype=torch.int64, device=dev),
                   support=torch.empty(out_top_k, dtype=torch.int32, device=dev),
                   count=torch.empty(1, dtype=torch.int32, device=dev))
    geometry = np.asarray(list(tile) + list(case_shape) + list(margin) + [V, K, out_top_k], dtype=np.int32)
    _lib.call("msl_views_merge", ptr(boxes), ptr(scores), ptr(labels), ptr(counts), views.ctypes.data, geometry.ctypes.data,
              float(max_overlap), MERGE_MODES[mode], ptr(workspace), workspace.numel(), ptr(out["boxes"]), ptr(out["scores"]),
              ptr(out["labels"]), ptr(out["support"]), ptr(out["count"]), _stream())
    return out
