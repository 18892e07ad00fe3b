"""Several MR sequences per case on top of ``tests/lesion_tree``: the first sequence and the mask are lesion_tree's,
every further sequence is a 'brain' of its own content on a scale 100 times smaller, whose support is either inside the
first one's (odd cases: the union's crop box is the first sequence's) or shifted by three voxels along one axis (even
cases: the union's box is larger than either channel's)."""
import os

import numpy as np

from tests import lesion_tree

SEQUENCES = ("FLAIR", "acq-mag_T2star", "acq-phase_T2star")


def extra_channel(k, c, first):
    """Sequence c >= 1 of case k, from the case's first sequence."""
    rs = np.random.RandomState(7919 * c + k)
    fg = np.argwhere(first > 0)
    lo, hi = fg.min(0), fg.max(0) + 1
    if k % 2:
        lo, hi = lo + 2, hi - 2
    else:
        a = (k // 2 + c) % 3
        lo[a], hi[a] = lo[a] + 3, hi[a] + 3  # lesion_tree leaves a border of at least seven voxels
    out = np.zeros(first.shape, np.float32)
    out[tuple(slice(a, b) for a, b in zip(lo, hi))] = (rs.rand(*(hi - lo)) + 0.01).astype(np.float32)
    return out


def make_tree(root, shapes, sequences=SEQUENCES[:2], centers=lesion_tree.CENTERS):
    """lesion_tree.make_tree plus the further sequences of every case.  -> data_dir."""
    from mslesions3d_amd.datasets import LesionsDataModule
    data_dir = lesion_tree.make_tree(root, shapes, centers=centers)
    probe = LesionsDataModule.__new__(LesionsDataModule)
    probe.data_dir, probe.registration, probe.skullstripped = data_dir, "T2star", True
    assert sequences[0] == "FLAIR"
    for k, shape in enumerate(shapes):
        ctr, sub = centers[k % len(centers)], f"{100 - k:03d}"
        first = np.load(probe._get_sequence(ctr, sub, "FLAIR") + ".npy")
        for c, name in enumerate(sequences[1:], 1):
            path = probe._get_sequence(ctr, sub, name) + ".npy"
            os.makedirs(os.path.dirname(path), exist_ok=True)
            np.save(path, extra_channel(k, c, first))
    return data_dir
