"""Clinical trees on their NATIVE grid, on top of ``tests/lesion_tree``: every case is a lesion_tree case stored with a
sidecar affine (``PATH.affine.npy``: voxel -> world, RAS+ mm) that is a signed axis permutation times a spacing per
stored axis, plus a translation; and the same cases put on the LPI 1 mm grid by the host ``datasets.regrid`` and stored
as plain ``.npy`` (what an offline preprocessing step would have written)."""
import itertools
import os

import numpy as np

from tests import lesion_tree, lesion_tree_mc

SIGNED_PERMUTATIONS = [(w, s) for w in itertools.permutations(range(3)) for s in itertools.product((1, -1), repeat=3)]


def make_affine(world, sign, zoom, translation=(0.0, 0.0, 0.0)):
    """Stored axis j runs along world axis world[j] with direction sign[j] and spacing zoom[j] mm."""
    a = np.eye(4, dtype=np.float64)
    a[:3, :3] = 0.0
    for j in range(3):
        a[world[j], j] = sign[j] * zoom[j]
    a[:3, 3] = translation
    return a


# (stored shape, world axis of each stored axis, direction, spacing): every case differs in permutation or spacing; the
# first is already LPI at 1 mm (an identity plan), the second is LPI with a spacing to snap
SPECS = [((40, 44, 38), (0, 1, 2), (-1, -1, -1), (1.0, 1.0, 1.0)),
         ((42, 40, 44), (0, 1, 2), (-1, -1, -1), (1.00005, 0.8, 1.25)),
         ((38, 46, 40), (0, 1, 2), (1, 1, 1), (1.0, 1.0, 1.0)),
         ((44, 36, 42), (2, 0, 1), (1, -1, 1), (0.9, 1.0, 1.2)),
         ((36, 42, 46), (1, 0, 2), (-1, 1, -1), (1.3, 0.7, 1.0)),
         ((41, 39, 43), (0, 2, 1), (1, 1, -1), (0.75, 1.1, 0.95)),
         ((45, 37, 40), (2, 1, 0), (-1, -1, 1), (1.0, 1.0, 1.5))]


def _probe(data_dir, sequences):
    from mslesions3d_amd.datasets import LesionsDataModule
    probe = LesionsDataModule.__new__(LesionsDataModule)
    probe.data_dir, probe.registration, probe.skullstripped = data_dir, "T2star", True
    probe.input_images, probe.segmentation = tuple(sequences), "labeled_lesions"
    return probe


def _save(path, arr, affine=None):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.save(path + ".npy", arr)
    if affine is not None:
        np.save(path + ".affine.npy", affine)


def make_trees(root, specs=SPECS, sequences=("FLAIR",), two_classes=False, centers=lesion_tree.CENTERS, sidecars=True):
    """Tree A under ``root/native`` (stored grid + sidecars) and tree B under ``root/regridded`` (the host-regridded
    arrays, no sidecars) -> (data_dir_a, data_dir_b, plans).  ``sidecars=False`` writes tree A without them."""
    from mslesions3d_amd import datasets as DS
    dir_a, dir_b = os.path.join(str(root), "native", "raw"), os.path.join(str(root), "regridded", "raw")
    pa, pb = _probe(dir_a, sequences), _probe(dir_b, sequences)
    plans = []
    for k, (shape, world, sign, zoom) in enumerate(specs):
        c, s = centers[k % len(centers)], f"{100 - k:03d}"
        for p in (pa, pb):
            os.makedirs(os.path.join(p._get_data_dir(c), f"sub-{s}"), exist_ok=True)
        first, seg = lesion_tree.make_case(k, shape, two_classes=two_classes)
        imgs = [first] + [lesion_tree_mc.extra_channel(k, ch, first) for ch in range(1, len(sequences))]
        affine = make_affine(world, sign, zoom, translation=(-90.0 + k, 126.0 - 2 * k, -72.0 + 0.5 * k))
        plan = DS.regrid_plan(affine, shape)
        plans.append(plan)
        img_b, seg_b = DS.regrid(np.stack(imgs), seg, plan)
        for name, a, b in zip(sequences, imgs, img_b):
            _save(pa._get_sequence(c, s, name), a, affine if sidecars else None)
            _save(pb._get_sequence(c, s, name), np.ascontiguousarray(b))
        _save(pa._get_sequence(c, s, pa.segmentation), seg, affine if sidecars else None)
        _save(pb._get_sequence(c, s, pb.segmentation), np.ascontiguousarray(seg_b))
    return dir_a, dir_b, plans
