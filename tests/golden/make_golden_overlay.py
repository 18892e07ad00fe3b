"""Mint ``overlay.npz``: the box-overlay volumes of the REFERENCE's own drawing code (build container only).

    python -m tests.golden.make_golden_overlay

* ``utils.make_segmentation_from_bboxes`` (utils.py:516-617): the instance plane and the class plane ("edges" style);
* ``predict.save_predictions_example(..., save_images=True)`` (predict.py:155-232): the array it hands to ``nib.save``,
  captured by the inert ``nibabel`` of ``make_golden_data`` ("preds" style).

Per case the file holds the inputs (boxes, labels, scores, shape, min_score) and the three recorded volumes as int16 (the
script asserts that the reference returned integers that fit).  No case has a min coordinate >= 1: the reference indexes
voxel n there and raises IndexError.
"""
import os
import tempfile

import numpy as np
import torch

from .make_golden_data import SAVED, install

OUT = os.path.dirname(os.path.abspath(__file__))
SHAPE = (24, 28, 36)


def cases():
    """name -> (shape, boxes (K, 6) f32, labels (K), scores (K) f32, min_score)."""
    f = lambda rows: np.asarray(rows, dtype=np.float32).reshape(-1, 6)
    out = {}
    out["none"] = (SHAPE, f([]), [], [], 0.5)
    out["placeholder"] = (SHAPE, f([[0, 0, 0, 1, 1, 1]]), [0], [0.0], 0.5)
    out["interior"] = (SHAPE, f([[0.25, 0.30, 0.20, 0.60, 0.70, 0.55]]), [1], [0.9], 0.5)
    a, b = [0.20, 0.20, 0.20, 0.60, 0.60, 0.60], [0.40, 0.35, 0.30, 0.80, 0.75, 0.70]
    out["overlap_ab"] = (SHAPE, f([a, b]), [1, 2], [0.9, 0.8], 0.5)
    out["overlap_ba"] = (SHAPE, f([b, a]), [2, 1], [0.8, 0.9], 0.5)
    clipped = []
    for axis in range(3):  # a box through each of the six faces
        lo, hi = [0.3, 0.3, 0.3, 0.6, 0.6, 0.6], [0.3, 0.3, 0.3, 0.6, 0.6, 0.6]
        lo[axis], hi[axis + 3] = -0.2, 1.3
        clipped += [lo, hi]
    out["clipped"] = (SHAPE, f(clipped), [1, 2, 1, 2, 1, 2], [0.9] * 6, 0.5)
    # min and max truncate to the same voxel on one axis (x: 0.51 * 24 = 12.24, 0.53 * 24 = 12.72)
    out["flat_axis"] = (SHAPE, f([[0.51, 0.2, 0.2, 0.53, 0.7, 0.7], [0.1, 0.52, 0.1, 0.4, 0.53, 0.5],
                                  [0.5, 0.1, 0.501, 0.9, 0.4, 0.502]]), [1, 1, 2], [0.9, 0.9, 0.9], 0.5)
    # reaching the last voxel: "edges" keeps max = n - 1, "preds" clamps max + 1 to it
    out["last_voxel"] = (SHAPE, f([[0.5, 0.5, 0.5, 1.0, 1.0, 1.0], [0.1, 0.1, 0.1, 0.97, 0.97, 0.98]]), [1, 2], [0.9, 0.7], 0.5)
    # a label-0 box between two others: the third box is still number 3
    out["label0_between"] = (SHAPE, f([[0.1, 0.1, 0.1, 0.4, 0.4, 0.4], [0.2, 0.2, 0.2, 0.7, 0.7, 0.7],
                                       [0.5, 0.5, 0.5, 0.9, 0.9, 0.9]]), [1, 0, 2], [0.9, 0.9, 0.9], 0.5)
    below = np.nextafter(np.float32(0.5), np.float32(0))
    out["scores"] = (SHAPE, f([[0.1, 0.1, 0.1, 0.5, 0.5, 0.5], [0.3, 0.3, 0.3, 0.7, 0.7, 0.7], [0.5, 0.2, 0.4, 0.9, 0.6, 0.8],
                               [0.05, 0.5, 0.05, 0.3, 0.9, 0.4]]), [1, 1, 2, 1], [0.5, below, 0.75, 0.25], 0.5)
    rs = np.random.RandomState(20)
    lo = rs.uniform(-0.1, 0.9, (40, 3))
    boxes = np.concatenate([lo, lo + rs.uniform(0.02, 0.5, (40, 3))], 1).astype(np.float32)
    out["random40"] = (SHAPE, boxes, rs.randint(0, 3, 40), rs.uniform(0.2, 1.0, 40).astype(np.float32), 0.5)
    lo = rs.uniform(0.0, 0.8, (12, 3))
    boxes = np.concatenate([lo, lo + rs.uniform(0.05, 0.4, (12, 3))], 1).astype(np.float32)
    out["noncube_odd_w"] = ((9, 14, 21), boxes, rs.randint(0, 3, 12), rs.uniform(0.3, 1.0, 12).astype(np.float32), 0.6)
    for name, (shape, b, l, s, m) in out.items():
        assert b.shape[0] == len(l) == len(s) and (b.size == 0 or b[:, :3].max() < 1.0), name
    return out


def as_int16(a, what):
    a = np.asarray(a, dtype=np.float64)
    assert np.array_equal(a, np.rint(a)) and a.min() >= 0 and a.max() <= 32767, what
    return a.astype(np.int16)


def main():
    install()
    import sys
    old, sys.argv = sys.argv, ["predict.py"]
    try:
        import predict as ref_predict
    finally:
        sys.argv = old
    import utils as ref_utils
    arrays, names = {}, []
    for name, (shape, boxes, labels, scores, min_score) in cases().items():
        names.append(name)
        b, l, s = torch.from_numpy(boxes.copy()), torch.tensor(labels, dtype=torch.long), torch.tensor(scores, dtype=torch.float32)
        if boxes.shape[0]:
            inst, cls = ref_utils.make_segmentation_from_bboxes(b.clone(), l.clone(), shape, return_type="numpy")
            inst, cls = inst.reshape(shape), cls.reshape(shape)
        else:  # (the reference cannot concatenate an empty batch: nothing is drawn)
            inst = cls = np.zeros(shape)
        SAVED.clear()
        loader = [{"img_meta_dict": [{"affine": torch.eye(4)[None]}], "subject": ["0001"], "img": torch.zeros((1, 1) + shape),
                   "boxes": [torch.zeros((0, 6))]}]
        ref_predict.save_predictions_example(loader, [b.clone()], [l.clone()], [s.clone()], min_score=min_score,
                                             output_dir=tempfile.mkdtemp(), save_images=True)
        preds = SAVED["sub-0001_preds.nii.gz"]
        assert preds.shape == tuple(shape)
        arrays[f"{name}__shape"] = np.asarray(shape, dtype=np.int32)
        arrays[f"{name}__boxes"] = boxes.astype(np.float32).reshape(-1, 6)
        arrays[f"{name}__labels"] = np.asarray(labels, dtype=np.int64).reshape(-1)
        arrays[f"{name}__scores"] = np.asarray(scores, dtype=np.float32).reshape(-1)
        arrays[f"{name}__min_score"] = np.float64(min_score)
        arrays[f"{name}__edges_instances"] = as_int16(inst, name)
        arrays[f"{name}__edges_classes"] = as_int16(cls, name)
        arrays[f"{name}__preds_instances"] = as_int16(preds, name)
    arrays["names"] = np.asarray(names)
    path = os.path.join(OUT, "overlay.npz")
    np.savez_compressed(path, **arrays)
    print("wrote overlay.npz", len(names), "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
