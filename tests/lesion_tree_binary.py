"""The clinical tree of ``lesion_tree`` with a binary mask beside every instance mask: ``lesions_binary`` (a segmentation
name without "labeled", which the data module reads in "binary" mode) holds ``seg != 0`` of ``labeled_lesions``.  Every
case carries two extra lesions that touch face to face: two instances, but one component of the binary mask, so the two
modes give different boxes and a test cannot pass through the wrong box stage."""
import os

import numpy as np

from tests import lesion_tree

CENTERS = lesion_tree.CENTERS
BINARY = "lesions_binary"
INSTANCES = "labeled_lesions"


def make_case(seed, shape):
    """-> (image f32, instance mask int16, binary mask int16)."""
    img, seg = lesion_tree.make_case(seed, shape)
    lo = np.argwhere(img > 0).min(0) + 1  # inside the brain box (at least 18 voxels wide for shapes of 40 and more)
    a = tuple(slice(int(v), int(v) + 3) for v in lo)
    seg[a] = 41  # lesion_tree's ids end at 39
    seg[a[0], a[1], slice(a[2].stop, a[2].stop + 3)] = 42  # shares a face with 41
    return img, seg, (seg != 0).astype(np.int16)


def make_tree(root, shapes, centers=CENTERS):
    """One case per entry of ``shapes`` with both masks.  -> data_dir."""
    from mslesions3d_amd.datasets import LesionsDataModule
    data_dir = os.path.join(str(root), "raw")
    probe = LesionsDataModule.__new__(LesionsDataModule)
    probe.data_dir, probe.registration, probe.skullstripped = data_dir, "T2star", True
    probe.input_images = ("FLAIR",)
    for k, shape in enumerate(shapes):
        c, s = centers[k % len(centers)], f"{100 - k:03d}"
        os.makedirs(os.path.join(probe._get_data_dir(c), f"sub-{s}"), exist_ok=True)
        img, inst, binary = make_case(k, shape)
        for name, mask in ((INSTANCES, inst), (BINARY, binary)):
            probe.segmentation = name
            lesion_tree.write_case(probe, c, s, img, mask)
    return data_dir
