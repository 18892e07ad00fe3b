"""Hand-built cases of the lesionpaste stage for ``datasets.paste_lesions`` and
msl_paste_lesions: three ragged donor cases, two targets, and a table of samples - each a list of paste rows with the
reports they must give and the number of voxels they must write.  Pure numpy; the CPU test checks the host function
against the table, the GPU test the kernel against the host function."""
import numpy as np

from mslesions3d_amd.datasets import PASTE_HEAD

DONOR_SHAPES = [(10, 9, 12), (14, 16, 8), (33, 6, 7)]
TARGET, TARGET_32 = (16, 12, 20), (34, 8, 40)
N_CAND = 3  # candidates per row of the table (a shorter list repeats its last entry)
K = 2       # rows per sample (a shorter list is padded with inactive rows)
LESION_ID = 5  # the target's own lesion, at LESION_BOX
LESION_BOX = ((8, 5, 8), (10, 7, 10))  # [lo, hi) per axis

# the donor lesions: (case, min, extents, voxels).  A and D are not whole boxes (voxels inside the box stay unwritten and
# become rim), B and C touch their case's border (rim coordinates fall outside the donor), E is 32 voxels long
A = (0, (3, 2, 4), (3, 4, 2), 22)
B = (0, (0, 0, 0), (2, 3, 2), 12)
C_ = (0, (8, 6, 9), (2, 3, 3), 17)
D = (1, (5, 6, 2), (4, 5, 3), 56)
E = (2, (1, 1, 1), (32, 3, 4), 380)


def donors(C):
    """-> [(image (C, n0, n1, n2) f32 without a zero, mask (n0, n1, n2) int16)] of the three donor cases."""
    out = []
    for k, shape in enumerate(DONOR_SHAPES):
        rs = np.random.RandomState(100 + k)
        img = (rs.randn(C, *shape) + 3.0 * np.sign(rs.randn(C, *shape))).astype(np.float32)
        seg = np.zeros(shape, np.int16)
        if k == 0:
            seg[3:6, 2:6, 4:6] = 11
            seg[3, 2, 4] = seg[5, 5, 5] = 0  # A: 24 - 2
            seg[0:2, 0:3, 0:2] = 12           # B: 12
            seg[8:10, 6:9, 9:12] = 13
            seg[8, 6, 9] = 0                  # C: 18 - 1
        elif k == 1:
            seg[5:9, 6:11, 2:5] = 21
            seg[5, 6:8, 2:4] = 0              # D: 60 - 4
        else:
            seg[1:33, 1:4, 1:5] = 31
            seg[1:5, 1, 1] = 0                # E: 384 - 4
        out.append((img, seg))
    return out


def target(C, shape=TARGET):
    """-> (image (C,) + shape f32, mask shape int16): channel 0 is background (exactly 0) from voxel 16 of the last axis
    on, channel 1 from voxel 18 on, so a centre at 16 or 17 is background in one channel only; one lesion of id 5."""
    rs = np.random.RandomState(7)
    img = (rs.randn(C, *shape) + 3.0 * np.sign(rs.randn(C, *shape))).astype(np.float32)
    for c in range(C):
        img[c, :, :, 16 + 2 * c:] = 0.0
    seg = np.zeros(shape, np.int16)
    (a0, a1, a2), (b0, b1, b2) = LESION_BOX
    seg[a0:b0, a1:b1, a2:b2] = LESION_ID
    return img, seg


def row(lesion, cands, flips=0, value=1, active=1, centre=None, case=None, mn=None, e=None):
    """One paste row (the layout of include/mslesions3d_hip.h); ``case`` / ``mn`` / ``e`` / ``centre`` override the lesion's."""
    case = lesion[0] if case is None else case
    mn = np.asarray(lesion[1] if mn is None else mn)
    e = np.asarray(lesion[2] if e is None else e)
    if centre is None:
        centre = (mn + mn + e - 1) // 2 - mn
        centre = np.where([(flips >> a) & 1 for a in range(3)], e - 1 - centre, centre)
    cands = list(cands) + [cands[-1]] * (N_CAND - len(cands))
    return np.asarray([active, case, *mn, *e, flips, value, *centre, *np.asarray(cands).reshape(-1)], dtype=np.int32)


def inactive():
    return np.zeros(PASTE_HEAD + 3 * N_CAND, dtype=np.int32)


ON_LESION = (7, 4, 7)   # A's box would overlap the target's lesion
FREE = (2, 2, 2)        # clear of it and of the background
FAR = (11, 6, 2)


def samples(value):
    """-> [(name, target shape, [rows], [reports], [voxels written per row])] for pastes that write ``value``."""
    v = dict(value=value)
    out = [
        ("first_candidate", TARGET, [row(A, [FREE], **v)], [0], [A[3]]),
        ("later_candidate_after_a_lesion", TARGET, [row(A, [ON_LESION, FREE], **v)], [1], [A[3]]),
        # A is 3 voxels long on axis 0: at 5 it ends at 7, its dilated box reaches the lesion's first plane at 8
        ("dilated_box_touches", TARGET, [row(A, [(5, 3, 8)], **v)], [-1], [0]),
        ("one_voxel_further_is_clear", TARGET, [row(A, [(5, 3, 8), (4, 3, 8)], **v)], [1], [A[3]]),
        # A's centre lands on voxel lo + 0 of the last axis: 17 is background in channel 0 alone
        ("background_centre", TARGET, [row(A, [(2, 2, 17), (2, 2, 16), FREE], **v)], [2], [A[3]]),
        ("all_rejected", TARGET, [row(A, [ON_LESION, (5, 3, 8), (2, 2, 17)], **v)], [-1], [0]),
        ("second_rejected_by_the_first", TARGET, [row(A, [FREE, FAR], **v), row(D, [(3, 3, 3)], **v)], [0, -1], [A[3], 0]),
        ("order_swapped", TARGET, [row(D, [(3, 3, 3)], **v), row(A, [FREE, FAR], **v)], [0, 1], [D[3], A[3]]),
        ("donor_at_the_low_border", TARGET, [row(B, [FREE], **v), row(B, [FAR], flips=7, **v)], [0, 0], [B[3], B[3]]),
        ("donor_at_the_high_border", TARGET, [row(C_, [FREE], **v), row(C_, [FAR], flips=5, **v)], [0, 0], [C_[3], C_[3]]),
        ("destination_at_the_borders", TARGET, [row(A, [(0, 0, 0)], **v), row(D, [(12, 7, 0)], **v)], [0, 0], [A[3], D[3]]),
        # (the last axis keeps both clear of the target's lesion at 8 .. 9 and of the background from 16 on)
        ("extent_32", TARGET_32, [row(E, [(2, 5, 11)], flips=1, **v), row(E, [(0, 0, 0)], **v)], [0, 0], [E[3], E[3]]),
        ("extent_exceeds_the_target", TARGET, [row(E, [(0, 0, 0)], **v), row(A, [FREE], **v)], [-2, 0], [0, A[3]]),
        ("inactive_rows", TARGET, [inactive(), row(A, [FREE], **v)], [-2, 0], [0, A[3]]),
    ]
    for f in (1, 2, 4, 7):
        out.append((f"flips_{f}", TARGET, [row(A, [FREE], flips=f, **v), row(D, [(10, 1, 11)], flips=f, **v)], [0, 0],
                    [A[3], D[3]]))
    refused = {"case_past_the_arena": row(A, [FREE], case=3, **v), "case_negative": row(A, [FREE], case=-1, **v),
               "box_outside_its_case": row(A, [FREE], mn=(8, 2, 4), **v), "box_before_its_case": row(A, [FREE], mn=(3, -1, 4), **v),
               "extent_33": row(E, [(0, 0, 0)], e=(33, 3, 4), mn=(0, 1, 1), **v), "extent_0": row(A, [FREE], e=(3, 0, 2), centre=(1, 0, 0), **v),
               "candidate_negative": row(A, [FREE, (2, -1, 2)], **v), "candidate_past_the_sample": row(A, [FREE, (14, 2, 2)], **v),
               "value_0": row(A, [FREE], value=0), "value_past_int16": row(A, [FREE], value=32768),
               "centre_outside_the_box": row(A, [FREE], centre=(1, 4, 0), **v)}
    for name, r in refused.items():  # the walk goes on behind a refused row
        out.append((f"refused_{name}", TARGET, [r, row(A, [FAR], **v)], [-2, 0], [0, A[3]]))
    return [(name, shape, rows + [inactive()] * (K - len(rows)), reports + [-2] * (K - len(reports)),
             counts + [0] * (K - len(counts))) for name, shape, rows, reports, counts in out]


def dilated_boxes(rows, reports, shape):
    """-> bool array of ``shape``: the union of the dilated destination boxes of the accepted rows."""
    inside = np.zeros(shape, bool)
    for r, rep in zip(rows, reports):
        if rep >= 0:
            lo = r[PASTE_HEAD + 3 * rep:PASTE_HEAD + 3 * rep + 3]
            inside[tuple(slice(max(int(a) - 1, 0), int(a) + int(e) + 1) for a, e in zip(lo, r[5:8]))] = True
    return inside


# ---- end to end: small clinical trees (tests/lesion_tree*.py), five cases each: four train, one validates -------------
TREE_SHAPES = [(30, 32, 34), (32, 30, 36), (34, 36, 30), (30, 34, 32), (33, 31, 35)]
FIT_TARGET, PATCH = (24, 28, 26), (16, 20, 18)
RECIPE = ["flip", "lesionpaste", "gaussiannoise"]


def recipe(prob=1.0):
    """flip, lesionpaste and an MR entry behind it, every probability 1 (``prob``: lesionpaste's own)."""
    from mslesions3d_amd.datasets import select_training_augmentations
    return [(n, dict(kw, prob=prob if n == "lesionpaste" else 1.0)) for n, kw in select_training_augmentations(RECIPE)]


def module(tmp_path, kind, patch=None, prob=1.0, batch_size=2):
    """A set-up LesionsDataModule over a fresh tree: ``kind`` "instances" (tests/lesion_tree), "binary"
    (tests/lesion_tree_binary) or "mc" (tests/lesion_tree_mc, two sequences)."""
    from mslesions3d_amd.datasets import LesionsDataModule
    from tests import lesion_tree, lesion_tree_binary, lesion_tree_mc
    kw = {}
    if kind == "binary":
        data_dir, kw = lesion_tree_binary.make_tree(tmp_path, TREE_SHAPES), {"segmentation": lesion_tree_binary.BINARY}
    elif kind == "mc":
        data_dir, kw = lesion_tree_mc.make_tree(tmp_path, TREE_SHAPES), {"input_images": lesion_tree_mc.SEQUENCES[:2]}
    else:
        data_dir = lesion_tree.make_tree(tmp_path, TREE_SHAPES)
    dm = LesionsDataModule(data_dir=data_dir, centers=lesion_tree.CENTERS, batch_size=batch_size, spatial_size=FIT_TARGET,
                           augmentations=recipe(prob), patch_size=patch, tile_margin=(2, 2, 2), **kw)
    dm.setup("fit")
    return dm
