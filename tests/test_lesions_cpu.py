"""datasets.LesionsDataModule on the host: instance boxes against the reference's own BoundingBoxesGeneratord
(tests/golden/instances.npz, minted by tests/golden/make_golden_instances.py), crop_foreground and
resize_with_pad_or_crop against their formulas, paths / subjects / split on a small tree, the pipeline order, and the
shape-changing permutations of the device path."""
import os

import numpy as np
import pytest
import torch

from mslesions3d_amd import datasets as DS
from mslesions3d_amd.devicedata import (AffineStage, IntensityOp, fit_rows, permute_numpy, sample_params,
                                        threshold_table)
from tests import lesion_tree

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "instances.npz"))
INF = np.iinfo(np.int32).max
NAMES = [str(n) for n in GOLD["names"]]


def _pairs(name):
    return [(int(lo), np.inf if hi == INF else int(hi)) for lo, hi in GOLD[f"{name}__thresholds"]]


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


# ---- instance boxes ------------------------------------------------------------------------------------------------
def test_the_fixture_covers_the_cases():
    need = {"one_class", "two_classes_with_outsiders", "flat", "empty", "no_background", "touching", "noncube", "binary"}
    assert need <= set(NAMES)
    assert GOLD["noncube__seg"].shape == (48, 64, 64)
    assert len(GOLD["flat__labels"]) < len(np.unique(GOLD["flat__seg"])) - 1           # flat lesions were removed
    assert 3 in GOLD["no_background__seg"] and 0 not in GOLD["no_background__seg"]
    assert set(GOLD["two_classes_with_outsiders__labels"].tolist()) == {1, 2}


@pytest.mark.parametrize("name", NAMES)
def test_boxes_from_instances_match_the_reference_bit_for_bit(name):
    mode = str(GOLD[f"{name}__mode"])
    boxes, labels = DS.boxes_from_instances(GOLD[f"{name}__seg"][None], _pairs(name), mode)
    assert boxes.dtype == torch.float32 and labels.dtype == torch.int64 and boxes.shape == (len(labels), 6)
    assert np.array_equal(_bits(boxes.numpy()), _bits(GOLD[f"{name}__boxes"])), name
    assert np.array_equal(labels.numpy(), GOLD[f"{name}__labels"]), name


def test_threshold_table():
    assert threshold_table([(1, np.inf)]).tolist() == [[1, INF]]
    assert threshold_table([(1000, 2000), (2000, np.inf)]).tolist() == [[1000, 2000], [2000, INF]]
    with pytest.raises(ValueError):
        threshold_table([(0.5, 2)])


# ---- crop_foreground / resize_with_pad_or_crop -----------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_crop_foreground_formula(seed):
    rs = np.random.RandomState(seed)
    shape = tuple(rs.randint(12, 30, 3))
    img = np.zeros(shape, np.float32)
    lo = [rs.randint(0, n // 2) for n in shape]
    hi = [rs.randint(n // 2 + 1, n + 1) for n in shape]
    img[tuple(slice(a, b) for a, b in zip(lo, hi))] = rs.rand(*[b - a for a, b in zip(lo, hi)]).astype(np.float32) - 0.3
    seg = rs.randint(0, 5, shape).astype(np.int16)
    F = np.argwhere(img > 0)
    want_lo = [max(int(F[:, a].min()) - 5, 0) for a in range(3)]
    want_hi = [min(int(F[:, a].max()) + 5 + 1, shape[a]) for a in range(3)]
    assert DS.foreground_box(img, 5) == (tuple(want_lo), tuple(want_hi))
    ci, cs = DS.crop_foreground(img, seg, 5)
    sl = tuple(slice(a, b) for a, b in zip(want_lo, want_hi))
    assert np.array_equal(ci, img[sl]) and np.array_equal(cs, seg[sl])


def test_crop_foreground_of_an_empty_image_keeps_it():
    img = -np.ones((5, 6, 7), np.float32)  # nothing > 0
    assert DS.foreground_box(img) == ((0, 0, 0), (5, 6, 7))


def _fit_by_hand(vol, target):
    """The issue's formula with np.pad(mode="edge") and a slice, axis by axis."""
    for a, t in enumerate(target):
        n = vol.shape[a]
        if n < t:
            before = (t - n) // 2
            pad = [(0, 0)] * vol.ndim
            pad[a] = (before, t - n - before)
            vol = np.pad(vol, pad, mode="edge")
        elif n > t:
            start = n // 2 - t // 2
            vol = np.take(vol, np.arange(start, start + t), axis=a)
    return vol


@pytest.mark.parametrize("shape,target", [((10, 21, 16), (15, 16, 16)), ((11, 20, 9), (16, 13, 12)),
                                          ((9, 9, 9), (12, 5, 9)), ((16, 15, 14), (9, 20, 19)), ((7, 8, 9), (7, 8, 9))])
def test_resize_with_pad_or_crop_formula(shape, target):
    """pads on one axis and crops on another, with odd and even differences"""
    rs = np.random.RandomState(sum(shape))
    for vol in (rs.randn(*shape).astype(np.float32), rs.randint(0, 3000, shape).astype(np.int16)):
        got = DS.resize_with_pad_or_crop(vol[None], target)
        assert got.shape == (1,) + target and got.dtype == vol.dtype
        assert np.array_equal(got[0], _fit_by_hand(vol, target))
        for a in range(3):  # the clamped-shift form the device kernel uses
            n, t = shape[a], target[a]
            idx = np.clip(np.arange(t) + DS.fit_shift(n, t), 0, n - 1)
            assert np.array_equal(np.take(vol, idx, axis=a), _fit_by_hand(vol, [t if k == a else shape[k] for k in range(3)]))


# ---- the data module -------------------------------------------------------------------------------------------------
SHAPES = [(40, 44, 50), (52, 48, 46), (44, 70, 52), (60, 50, 72), (48, 64, 64), (42, 42, 42), (50, 45, 58),
          (46, 66, 49), (41, 51, 61), (55, 47, 43)]


def _module(tmp_path, **kw):
    data_dir = lesion_tree.make_tree(tmp_path, SHAPES)
    args = dict(data_dir=data_dir, centers=lesion_tree.CENTERS, batch_size=2, spatial_size=(48, 64, 64))
    args.update(kw)
    return DS.LesionsDataModule(**args)


def test_paths_sorted_subjects_and_split(tmp_path):
    from sklearn.model_selection import train_test_split
    dm = _module(tmp_path)
    reg = os.path.join(dm.data_dir, "A_CENTER", "derivatives", "registrations", "registrations_to_T2star")
    assert dm._get_data_dir("A_CENTER") == reg
    assert dm._get_sequence("A_CENTER", "007", "FLAIR") == os.path.join(
        reg, "derivatives", "skullstripped", "sub-007", "ses-01", "sub-007_ses-01_FLAIR")
    assert dm._get_sequence("A_CENTER", "007", "labeled_lesions") == os.path.join(
        reg, "derivatives", "lesionmasks", "sub-007", "ses-01", "sub-007_ses-01_labeled_lesions")
    dm.skullstripped = False
    assert dm._get_sequence("A_CENTER", "007", "FLAIR") == os.path.join(reg, "sub-007", "ses-01", "anat",
                                                                        "sub-007_ses-01_FLAIR")
    dm.skullstripped = True
    want = sorted((lesion_tree.CENTERS[k % 2], f"{100 - k:03d}") for k in range(len(SHAPES)))
    assert dm.subjects_list == want and want[0][0] == "A_CENTER"
    dm.setup("fit")
    tr, te = train_test_split(want, train_size=0.8, test_size=0.2, random_state=970205)
    assert dm.train_dataset.subjects == tr and dm.test_dataset.subjects == te and len(te) == 2
    assert dm.thresholds == [(1, np.inf)] and dm.segmentation_mode == "instances" and dm.n_classes == 1
    two = DS.LesionsDataModule(data_dir=dm.data_dir, centers=lesion_tree.CENTERS, classes=("a", "b"))
    assert two.thresholds == [(1000, 2000), (2000, np.inf)]
    with pytest.raises(NotImplementedError):
        DS.LesionsDataModule(data_dir=dm.data_dir, centers=lesion_tree.CENTERS, input_images=("FLAIR", "T1"))
    half = DS.LesionsDataModule(data_dir=dm.data_dir, centers=lesion_tree.CENTERS, percentage=0.5)
    assert half.subjects_list == want[:5]


def test_loader_surface(tmp_path):
    dm = _module(tmp_path, augmentations=DS.select_augmentations(["flip", "rotate90"]))
    dm.setup("fit")
    dm.set_epoch(3)
    batches = list(dm.train_dataloader())
    assert [len(b["subject"]) for b in batches] == [2, 2, 2, 2]
    assert all(b["img"].shape == (2, 1, 48, 64, 64) and b["img"].dtype == torch.float32 for b in batches)
    assert sorted(s for b in batches for s in b["subject"]) == sorted(dm.train_dataset.subjects)
    val = list(dm.test_dataloader())
    assert len(val) == 1 and val[0]["img"].shape == (2, 1, 48, 64, 64)
    assert sum(len(l) for b in batches + val for l in b["labels"]) > 0
    assert len(list(dm.predict_dataloader())) == 2


def test_pipeline_order_one_augmented_sample_by_hand(tmp_path):
    """crop -> normalise -> augment at the cropped shape -> fit -> boxes"""
    augs = DS.select_augmentations(["flip", "rotate90", "affine", "shiftintensity", "scaleintensity"])
    augs = [(n, dict(kw, prob=1.0)) for n, kw in augs]  # everything drawn: the rot90s change the shape
    dm = _module(tmp_path, augmentations=augs)
    dm.setup("fit")
    dm.set_epoch(1)
    ds = dm.train_dataset
    changed = 0
    for i in range(3):
        img, seg = ds.load(i)
        lo, hi = DS.foreground_box(img, 5)
        assert any(a > 0 for a in lo) and any(b < n for b, n in zip(hi, img.shape))  # the crop does something
        sl = tuple(slice(a, b) for a, b in zip(lo, hi))
        x, m = DS.normalize_nonzero(img[sl])[None], seg[sl][None]
        cropped = x.shape
        rs = DS.sample_rng(dm.random_state, 1, ds.subjects[i])
        for name, kw in augs:
            x, m = DS.AUGMENTATIONS[name](x, m, rs, **kw)
        changed += x.shape != cropped
        x, m = _fit_by_hand(x[0], dm.spatial_size), _fit_by_hand(m[0], dm.spatial_size)
        boxes, labels = DS.boxes_from_instances(m, dm.thresholds)
        got = ds[i]
        assert got["subject"] == ds.subjects[i]
        assert np.array_equal(_bits(got["img"][0].numpy()), _bits(x))
        assert np.array_equal(_bits(got["boxes"].numpy()), _bits(boxes.numpy())) and torch.equal(got["labels"], labels)
    assert changed > 0


# ---- the device path's host side ---------------------------------------------------------------------------------------
def test_ragged_permutations_equal_numpy(tmp_path):
    augs = [(n, dict(kw, prob=0.8)) for n, kw in DS.select_augmentations(["flip", "rotate90"])]
    vol = np.arange(5 * 6 * 7).reshape(5, 6, 7)
    seen = set()
    for seed in range(60):
        draws = DS.draw_augmentations(augs, np.random.RandomState(seed))
        want, _ = vol[None], None
        rs = np.random.RandomState(seed)
        m = vol[None]
        for name, kw in augs:
            want, m = DS.AUGMENTATIONS[name](want, m, rs, **kw)
        perm, stages = sample_params(draws, vol.shape, augs, ragged=True)
        assert stages == [] and np.array_equal(permute_numpy(vol, perm), want[0])
        seen.add(want[0].shape)
        if want[0].shape != vol.shape:
            with pytest.raises(NotImplementedError):
                sample_params(draws, vol.shape, augs)
    assert len(seen) >= 4


def test_ragged_affine_is_computed_for_the_permuted_shape():
    augs = [("rotate90", {"spatial_axes": (0, 2), "prob": 1.0, "max_k": 1}),
            ("affine", {"rotate_range": (0.3, 0.3, 0.3), "padding_mode": "border", "prob": 1.0}),
            ("shiftintensity", {"offsets": 0.1, "prob": 1.0})]
    draws = DS.draw_augmentations(augs, np.random.RandomState(0))
    perm, stages = sample_params(draws, (10, 20, 30), augs, ragged=True)
    assert sorted(perm[0]) == [0, 1, 2] and perm[0][0] == 2 and perm[0][2] == 0
    assert isinstance(stages[0], AffineStage) and isinstance(stages[1], IntensityOp)
    m, off = DS.affine_matrix((30, 20, 10), *draws[1][1])
    assert np.array_equal(stages[0].matrix, m) and np.array_equal(stages[0].offset, off)
    rows = fit_rows([3], [(perm, stages)])
    assert rows.shape == (1, 32) and rows[0, 0] == 3 and rows[0, 7] == 1 and rows[0, 20] == 1 and rows[0, 21] == 1
    with pytest.raises(NotImplementedError):
        fit_rows([0], [(perm, [stages[0], stages[0]])])
