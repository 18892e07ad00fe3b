"""A small synthetic clinical tree for the LesionsDataModule tests: ``.npy`` volumes of differing shapes in the
reference's BIDS layout, a positive 'brain' box inside a zero border, instance-labelled cubes inside the brain."""
import os

import numpy as np

CENTERS = ("B_CENTER", "A_CENTER")


def write_case(module, center, subject, img, seg):
    for name, arr in ((module.input_images[0], img), (module.segmentation, seg)):
        path = module._get_sequence(center, subject, name) + ".npy"
        os.makedirs(os.path.dirname(path), exist_ok=True)
        np.save(path, arr)


def make_case(seed, shape, n_lesions=(2, 6), two_classes=False, background=True):
    """-> (image f32, mask int16).  The brain box leaves a zero border of 7 .. 11 voxels (more than the crop margin)."""
    rs = np.random.RandomState(seed)
    img = np.zeros(shape, np.float32)
    lo = [int(rs.randint(7, 12)) for _ in shape]
    hi = [n - int(rs.randint(7, 12)) for n in shape]
    brain = tuple(slice(a, b) for a, b in zip(lo, hi))
    img[brain] = (rs.rand(*[b - a for a, b in zip(lo, hi)]) * 100 + 1).astype(np.float32)
    seg = np.zeros(shape, np.int16)
    ids = rs.permutation(np.arange(1, 40))[:rs.randint(*n_lesions)]
    for k, v in enumerate(ids):
        size = rs.randint(2, 7, 3)
        at = [int(rs.randint(a, b - s + 1)) for a, b, s in zip(lo, hi, size)]
        seg[tuple(slice(a, a + s) for a, s in zip(at, size))] = int(v) + (1000 * (1 + k % 2) if two_classes else 0)
    if not background:
        seg[seg == 0] = 1 if not two_classes else 1001
    return img, seg


def make_tree(root, shapes, two_classes=False, centers=CENTERS):
    """One case per entry of ``shapes``, dealt over the centers.  -> data_dir.  The sub-* directories the reference lists
    (datasets.py:181) are created under each center's registration directory."""
    from mslesions3d_amd.datasets import LesionsDataModule
    data_dir = os.path.join(str(root), "raw")
    probe = LesionsDataModule.__new__(LesionsDataModule)
    probe.data_dir, probe.registration, probe.skullstripped = data_dir, "T2star", True
    probe.input_images, probe.segmentation = ("FLAIR",), "labeled_lesions"
    for k, shape in enumerate(shapes):
        c, s = centers[k % len(centers)], f"{100 - k:03d}"
        os.makedirs(os.path.join(probe._get_data_dir(c), f"sub-{s}"), exist_ok=True)
        write_case(probe, c, s, *make_case(k, shape, two_classes=two_classes))
    return data_dir
