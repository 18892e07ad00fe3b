"""Multi-sequence clinical cases on the host (datasets.LesionsDataModule(input_images=(...)), 1 <= C <= 4): the union
foreground box, per-channel normalisation, the channel-first sample, and the -ii flag of the entry points.  The reference
refuses more than one sequence, so the contract is the one in the class docstring / DESIGN.md section 4.8."""
import numpy as np
import pytest
import torch

from mslesions3d_amd import datasets as DS
from tests import lesion_tree, lesion_tree_mc

SHAPES = [(40, 44, 50), (52, 48, 46), (44, 70, 52), (60, 50, 72), (48, 64, 64), (42, 42, 42), (50, 45, 58),
          (46, 66, 49), (41, 51, 61), (55, 47, 43)]
TARGET = (48, 64, 64)
TWO = lesion_tree_mc.SEQUENCES[:2]


def _bits(a):
    a = np.ascontiguousarray(a.numpy() if torch.is_tensor(a) else a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _module(data_dir, input_images=TWO, **kw):
    kw.setdefault("spatial_size", TARGET)
    return DS.LesionsDataModule(data_dir=data_dir, centers=lesion_tree.CENTERS, batch_size=2, input_images=input_images, **kw)


# ---- foreground --------------------------------------------------------------------------------------------------------
def test_union_foreground_box_is_larger_than_either_channel():
    v = np.zeros((2, 30, 34, 38), np.float32)
    v[0, 8:15, 10:20, 12:30] = 3.0
    v[1, 11:22, 12:18, 9:25] = 0.5
    v[0, 0, 0, 0] = -4.0  # negative voxels are background
    for margin in (0, 2, 5):
        lo, hi = DS.foreground_box(v, margin)
        assert len(lo) == len(hi) == 3
        boxes = [DS.foreground_box(v[c], margin) for c in range(2)]
        want_lo = tuple(min(b[0][a] for b in boxes) for a in range(3))
        want_hi = tuple(max(b[1][a] for b in boxes) for a in range(3))
        assert (lo, hi) == (want_lo, want_hi)
        for blo, bhi in boxes:  # strictly larger than either channel's own box along at least one axis
            assert any(h - l > bh - bl for l, h, bl, bh in zip(lo, hi, blo, bhi))
    img, seg = DS.crop_foreground(v, np.arange(30 * 34 * 38).reshape(30, 34, 38), 0)
    assert img.shape == (2, 14, 10, 21) and seg.shape == (14, 10, 21)
    assert np.array_equal(img, v[:, 8:22, 10:20, 9:30]) and seg[0, 0, 0] == (8 * 34 + 10) * 38 + 9


def test_union_foreground_box_edge_cases():
    one = np.zeros((12, 13, 14), np.float32)
    one[3:6, 4:9, 5:7] = 2.0
    # a channel that is all zero, and one with negative values only, add nothing
    for other in (np.zeros_like(one), -np.ones_like(one)):
        for order in ((one, other), (other, one)):
            assert DS.foreground_box(np.stack(order), 1) == DS.foreground_box(one, 1) == ((2, 3, 4), (7, 10, 8))
    # an empty union keeps the whole volume (three axes, not four)
    empty = np.stack([np.zeros_like(one), -np.ones_like(one)])
    assert DS.foreground_box(empty, 5) == ((0, 0, 0), (12, 13, 14))
    img, seg = DS.crop_foreground(empty, np.zeros(one.shape, np.int16), 5)
    assert img.shape == (2, 12, 13, 14) and seg.shape == (12, 13, 14)
    # three channels, and the one-channel form unchanged
    assert DS.foreground_box(np.stack([one, one * 0, one]), 0) == DS.foreground_box(one, 0)
    assert DS.foreground_box(one[None], 0) == DS.foreground_box(one, 0)


# ---- normalisation -----------------------------------------------------------------------------------------------------
def test_every_channel_is_normalised_over_its_own_nonzero_voxels(tmp_path):
    """Channels 100 times apart in scale: each one's non-zero voxels end at mean 0 / std 1 and zeros stay zero.  Bound:
    normalize_nonzero works in f32 on ~3e4 voxels; numpy's pairwise f32 sum carries a relative error of about
    log2(3e4) * 2^-24 ~ 1e-6 on a mean that is 1.7 deviations from zero, i.e. ~2e-6 deviations; 1e-5 leaves room for the
    f32 rounding of the division.  The pooled normalisation (the reference's transform on a stacked image) is far off."""
    data_dir = lesion_tree_mc.make_tree(tmp_path, SHAPES[:3])
    probe = _module(data_dir)
    probe.setup("fit")
    case = probe.subjects_list[0]
    ds = probe.train_dataset
    img, seg = ds.load(ds.subjects.index(case)) if case in ds.subjects else probe.test_dataset.load(
        probe.test_dataset.subjects.index(case))
    assert img.shape[0] == 2 and img[0].max() > 50 * img[1].max()  # scales apart
    crop, _ = DS.crop_foreground(img, seg, probe.margin)
    dm = _module(data_dir, subject=case, spatial_size=crop.shape[1:])  # the fit is the identity
    dm.setup("fit")
    x = dm.test_dataset[0]["img"].numpy()
    assert x.shape == crop.shape
    for c in range(2):
        nz = crop[c] != 0
        assert nz.sum() > 1000 and (~nz).sum() > 1000
        pop = x[c][nz].astype(np.float64)
        assert abs(pop.mean()) <= 1e-5 and abs(pop.std() - 1.0) <= 1e-5, (c, pop.mean(), pop.std())
        assert not x[c][~nz].any()
        assert np.array_equal(_bits(x[c]), _bits(DS.normalize_nonzero(crop[c])))
    pooled = DS.normalize_nonzero(crop)
    for c in range(2):
        pop = pooled[c][crop[c] != 0].astype(np.float64)
        assert abs(pop.mean()) > 0.1 and abs(pop.std() - 1.0) > 0.1  # what pooling the channels would have given
        assert np.abs(pooled[c] - x[c]).max() > 0.1


# ---- the module --------------------------------------------------------------------------------------------------------
def test_two_sequence_module_against_the_one_sequence_module(tmp_path):
    data_dir = lesion_tree_mc.make_tree(tmp_path, SHAPES)
    two, one = _module(data_dir), _module(data_dir, ("FLAIR",))
    two.setup("fit")
    one.setup("fit")
    assert two.input_images == TWO and two.train_dataset.subjects == one.train_dataset.subjects
    same_crop = other_crop = 0
    for ds2, ds1 in ((two.train_dataset, one.train_dataset), (two.test_dataset, one.test_dataset)):
        for i in range(len(ds2)):
            img, seg = ds2.load(i)
            img1, seg1 = ds1.load(i)
            assert img.shape == (2,) + seg.shape and img.dtype == np.float32 and img1.shape == seg.shape
            assert np.array_equal(img[0], img1) and np.array_equal(seg, seg1) and not np.array_equal(img[0], img[1])
            s2, s1 = ds2[i], ds1[i]
            assert s2["img"].shape == (2,) + TARGET and s2["img"].dtype == torch.float32 and s1["img"].shape == (1,) + TARGET
            assert s2["subject"] == s1["subject"]
            # by hand: one box for both channels and the mask, each channel normalised alone, then the fit
            lo, hi = DS.foreground_box(img, two.margin)
            sl = tuple(slice(a, b) for a, b in zip(lo, hi))
            for c in range(2):
                want = DS.resize_with_pad_or_crop(DS.normalize_nonzero(img[c][sl]), TARGET)
                assert np.array_equal(_bits(s2["img"][c]), _bits(want)), (i, c)
            boxes, labels = DS.boxes_from_instances(DS.resize_with_pad_or_crop(seg[sl], TARGET), two.thresholds)
            assert np.array_equal(_bits(s2["boxes"]), _bits(boxes)) and torch.equal(s2["labels"], labels)
            if (lo, hi) == DS.foreground_box(img1, one.margin):  # the same crop: the same masks, the same first channel
                same_crop += 1
                assert np.array_equal(_bits(s2["boxes"]), _bits(s1["boxes"])) and torch.equal(s2["labels"], s1["labels"])
                assert np.array_equal(_bits(s2["img"][0]), _bits(s1["img"][0]))
            else:
                other_crop += 1
    assert same_crop >= 3 and other_crop >= 3
    batches = list(two.train_dataloader())
    assert all(b["img"].shape == (2, 2) + TARGET for b in batches) and len(batches) == 4
    assert list(two.test_dataloader())[0]["img"].shape == (2, 2) + TARGET


def test_augmentations_move_all_channels_and_the_mask_together(tmp_path):
    augs = DS.select_augmentations(["flip", "rotate90", "affine", "shiftintensity", "scaleintensity"])
    augs = [(n, dict(kw, prob=1.0)) for n, kw in augs]
    data_dir = lesion_tree_mc.make_tree(tmp_path, SHAPES[:5], lesion_tree_mc.SEQUENCES)
    dm = _module(data_dir, lesion_tree_mc.SEQUENCES, augmentations=augs)
    dm.setup("fit")
    dm.set_epoch(2)
    ds = dm.train_dataset
    for i in range(2):
        img, seg = DS.crop_foreground(*ds.load(i), margin=dm.margin)
        got = ds[i]
        assert got["img"].shape == (3,) + TARGET
        for c in range(3):  # the same draws on one channel at a time: one-channel pipeline by hand
            x, m = DS.normalize_nonzero(img[c])[None], seg[None]
            rs = DS.sample_rng(dm.random_state, 2, ds.subjects[i])
            for name, kw in augs:
                x, m = DS.AUGMENTATIONS[name](x, m, rs, **kw)
            assert np.array_equal(_bits(got["img"][c]), _bits(DS.resize_with_pad_or_crop(x, TARGET)[0])), (i, c)
        boxes, labels = DS.boxes_from_instances(DS.resize_with_pad_or_crop(m, TARGET), dm.thresholds)
        assert np.array_equal(_bits(got["boxes"]), _bits(boxes)) and torch.equal(got["labels"], labels)


def test_what_the_module_refuses(tmp_path):
    data_dir = lesion_tree_mc.make_tree(tmp_path, SHAPES[:5])
    for names in ((), ("FLAIR", "FLAIR"), ("FLAIR", "acq-mag_T2star", "acq-phase_T2star", "a", "b")):
        with pytest.raises(ValueError):
            _module(data_dir, names)
    assert _module(data_dir, ("acq-mag_T2star",)).input_images == ("acq-mag_T2star",)
    dm = _module(data_dir)
    dm.setup("fit")
    c, s = dm.train_dataset.subjects[0]
    path = dm._get_sequence(c, s, TWO[1]) + ".npy"
    vol = np.load(path)
    np.save(path, vol[:, :-1])
    with pytest.raises(ValueError, match=f"{s}.*{TWO[1]}"):
        dm.train_dataset.load(0)
    np.save(path, vol)
    assert dm.train_dataset.load(0)[0].shape == (2,) + vol.shape
    one = _module(data_dir, ("FLAIR",))
    one.setup("fit")
    assert one.train_dataset.load(0)[0].ndim == 3  # one sequence: (D, H, W), as before


# ---- entry points ------------------------------------------------------------------------------------------------------
def test_both_parsers_take_several_input_images():
    from mslesions3d_amd import predict as P
    from mslesions3d_amd import train as T
    for mod in (T, P):
        p = mod.build_parser()
        assert p.parse_args([]).input_images == ["FLAIR"]
        assert p.parse_args(["-dm", "lesions", "-ii", "FLAIR", "acq-mag_T2star"]).input_images == ["FLAIR", "acq-mag_T2star"]
        assert p.parse_args(["--input_images", "A"]).input_images == ["A"]
    with pytest.raises(ValueError, match="one-channel"):
        T.example(T.build_parser().parse_args(["-dm", "example", "-ii", "A", "B"]))
    with pytest.raises(ValueError, match="one-channel"):
        P.predict_example(P.build_parser().parse_args(["-dm", "example", "-ii", "A", "B"]))


def test_checkpoint_channel_mismatch_names_both():
    from mslesions3d_amd.train import check_input_channels

    class M:
        input_channels = 2
    check_input_channels(M, ("FLAIR", "acq-mag_T2star"), "x.ckpt")
    with pytest.raises(ValueError, match=r"input_channels=2.*1 input image.*FLAIR"):
        check_input_channels(M, ("FLAIR",), "x.ckpt")
