"""Host side of the prediction overlays: utils.draw_boxes against volumes recorded from the
reference's own drawing code (tests/golden/overlay.npz), datasets.fit_to_case_frame against the boxes of the un-cropped
mask, the geometry keys of the LesionsDataModule samples, and predict.py's new flags.  CPU only."""
import os

import numpy as np
import pytest
import torch

from mslesions3d_amd import datasets as DS
from mslesions3d_amd.utils import draw_boxes
from tests import lesion_tree

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "overlay.npz"))
CASES = [str(n) for n in GOLD["names"]]
SHAPES = [(40, 44, 50), (52, 48, 46), (44, 70, 52), (60, 50, 72)]


def gold_case(name):
    return (GOLD[f"{name}__boxes"], GOLD[f"{name}__labels"], GOLD[f"{name}__scores"], tuple(int(v) for v in GOLD[f"{name}__shape"]),
            float(GOLD[f"{name}__min_score"]))


# ---- draw_boxes ---------------------------------------------------------------------------------------------------------
def test_the_fixture_holds_the_cases():
    assert {"none", "placeholder", "interior", "overlap_ab", "overlap_ba", "clipped", "flat_axis", "last_voxel",
            "label0_between", "scores", "random40", "noncube_odd_w"} <= set(CASES)
    for name in CASES:
        for plane in ("edges_instances", "edges_classes", "preds_instances"):
            a = GOLD[f"{name}__{plane}"]
            assert a.dtype == np.int16 and a.shape == gold_case(name)[3] and max(a.shape) <= 36
    assert GOLD["noncube_odd_w__shape"][2] % 2 == 1
    # the two styles' max rules differ where a box reaches the last voxel; a skipped box keeps its number
    assert not np.array_equal(GOLD["last_voxel__edges_instances"], GOLD["last_voxel__preds_instances"])
    assert set(np.unique(GOLD["label0_between__preds_instances"])) == {0, 1, 3}
    assert set(np.unique(GOLD["scores__preds_instances"])) == {0, 1, 3} and 2 in GOLD["scores__edges_instances"]


@pytest.mark.parametrize("name", CASES)
def test_draw_boxes_edges_equals_the_reference(name):
    boxes, labels, scores, shape, _ = gold_case(name)
    inst, cls = draw_boxes(boxes, labels, scores, shape, "edges")
    assert inst.dtype == cls.dtype == np.int16 and inst.shape == cls.shape == shape
    assert np.array_equal(inst, GOLD[f"{name}__edges_instances"])
    assert np.array_equal(cls, GOLD[f"{name}__edges_classes"])


@pytest.mark.parametrize("name", CASES)
def test_draw_boxes_preds_equals_the_reference(name):
    boxes, labels, scores, shape, min_score = gold_case(name)
    inst, cls = draw_boxes(torch.from_numpy(boxes), torch.from_numpy(labels), torch.from_numpy(scores), shape, "preds", min_score)
    assert inst.dtype == cls.dtype == np.int16
    assert np.array_equal(inst, GOLD[f"{name}__preds_instances"])
    # the class plane of "preds" is this project's extension: the label of the box each drawn voxel names
    drawn = inst > 0
    assert np.array_equal(cls[drawn], labels[inst[drawn] - 1]) and not cls[~drawn].any()


def test_draw_boxes_refuses_bad_arguments_and_skips_out_of_range_faces():
    with pytest.raises(ValueError):
        draw_boxes(np.zeros((0, 6)), [], [], (4, 4, 4), "faces")
    with pytest.raises(ValueError):
        draw_boxes(np.zeros((0, 6)), [], [], (4, 0, 4), "edges")
    # a box wholly above 1: every min is voxel n, which the reference cannot index; the max faces' slices [n, n - 1) are
    # empty, so "edges" draws nothing and "preds" its far corner alone
    for style in ("edges", "preds"):
        inst, cls = draw_boxes(np.asarray([[1.5, 1.5, 1.5, 2, 2, 2]], np.float32), [2], [0.9], (5, 6, 7), style)
        want = np.zeros((5, 6, 7), np.int16)
        want[4, 5, 6] = style == "preds"
        assert np.array_equal(inst, want) and np.array_equal(cls, 2 * want)


# ---- fit_to_case_frame --------------------------------------------------------------------------------------------------
def _one_case(tmp_path, k, target):
    data_dir = str(tmp_path / "raw")
    if not os.path.exists(data_dir):
        lesion_tree.make_tree(tmp_path, SHAPES)
    c, s = lesion_tree.CENTERS[k % 2], f"{100 - k:03d}"
    dm = DS.LesionsDataModule(data_dir=data_dir, centers=lesion_tree.CENTERS, batch_size=1, spatial_size=target, subject=(c, s))
    dm.setup("predict")
    return dm


def _crop_shape(tmp_path, k):
    dm = _one_case(tmp_path, k, (8, 8, 8))
    img, seg = dm.predict_dataset.load(0)
    lo, hi = DS.foreground_box(img, dm.margin)
    return tuple(b - a for a, b in zip(lo, hi)), lo, seg


@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_mapped_ground_truth_names_the_voxels_of_the_uncropped_mask(tmp_path, k):
    n, lo, seg = _crop_shape(tmp_path, k)
    assert n != seg.shape and min(lo) >= 1
    # axis 0 padded, axis 1 cropped to [2, n - 2) (every lesion lies inside the brain, five voxels or more from the crop's
    # faces), axis 2 equal
    target = (n[0] + 7, n[1] - 4, n[2])
    sample = _one_case(tmp_path, k, target).predict_dataset[0]
    assert sample["crop_shape"] == n and sample["crop_origin"] == lo and sample["full_shape"] == seg.shape
    full, full_labels = DS.boxes_from_instances(seg, [(1, np.inf)])
    mapped = DS.fit_to_case_frame(sample["boxes"].numpy(), target, sample["crop_shape"], sample["crop_origin"], sample["full_shape"])
    assert mapped.dtype == np.float32 and mapped.shape == tuple(full.shape) and len(full) >= 1
    s2 = np.asarray(seg.shape * 2, dtype=np.float32)
    assert np.array_equal(np.rint(mapped * s2).astype(int), np.rint(full.numpy() * s2).astype(int))
    assert torch.equal(sample["labels"], full_labels)


def test_a_lesion_across_the_crop_window_maps_back_as_its_part_inside(tmp_path):
    """The limit of the map: where the fit crops an axis the fitted mask holds a lesion's part inside the kept window only."""
    found = None
    for k in range(len(SHAPES)):
        n, lo, seg = _crop_shape(tmp_path, k)
        full, _ = DS.boxes_from_instances(seg, [(1, np.inf)])
        ext = np.rint(full.numpy() * np.asarray(seg.shape * 2, dtype=np.float32)).astype(int)  # inclusive voxel extents
        for e in ext:
            if e[4] - e[1] >= 2:  # three voxels or more along axis 1: cut after the first one, two or more stay
                start = e[1] - lo[1] + 1  # first kept voxel of the cropped axis
                for t1 in range(n[1] - 1, 1, -1):
                    if DS.fit_shift(n[1], t1) == start:
                        found = (k, n, lo, seg, ext, t1, start)
                        break
            if found:
                break
        if found:
            break
    assert found is not None
    k, n, lo, seg, ext, t1, start = found
    target = (n[0], t1, n[2])
    sample = _one_case(tmp_path, k, target).predict_dataset[0]
    mapped = DS.fit_to_case_frame(sample["boxes"].numpy(), target, n, lo, seg.shape)
    got = np.rint(mapped * np.asarray(seg.shape * 2, dtype=np.float32)).astype(int)
    w0, w1 = lo[1] + start, lo[1] + start + t1 - 1  # the kept window of axis 1 in the case's frame, inclusive
    want, cut = [], 0
    for e in ext:
        a, b = max(e[1], w0), min(e[4], w1)
        if b - a >= 1:  # (a part one voxel thick is a flat box: dropped, like a lesion outside the window)
            want.append([e[0], a, e[2], e[3], b, e[5]])
            cut += (a, b) != (e[1], e[4])
    assert cut >= 1 and np.array_equal(got, np.asarray(want).reshape(-1, 6))


def test_fit_to_case_frame_is_three_rounded_f32_operations():
    rs = np.random.RandomState(5)
    boxes = rs.uniform(-0.3, 1.3, (50, 6)).astype(np.float32)
    target, crop, lo, full = (48, 64, 30), (41, 80, 30), (3, 0, 9), (50, 91, 47)
    got = DS.fit_to_case_frame(boxes, target, crop, lo, full)
    for a in range(6):
        t, n, o, s = target[a % 3], crop[a % 3], lo[a % 3], full[a % 3]
        d = -((t - n) // 2) if n < t else n // 2 - t // 2
        for i in range(50):
            want = np.float32(np.float32(boxes[i, a] * np.float32(t)) + np.float32(d + o)) / np.float32(s)
            assert got[i, a].tobytes() == np.float32(want).tobytes()
    assert DS.fit_to_case_frame(np.zeros((0, 6), np.float32), target, crop, lo, full).shape == (0, 6)
    assert got.min() < 0 and got.max() > 1  # not clamped


# ---- samples and collate_fn ---------------------------------------------------------------------------------------------
def test_samples_and_batches_carry_the_geometry_and_keep_the_old_keys(tmp_path):
    target = (48, 64, 64)
    lesion_tree.make_tree(tmp_path, SHAPES)
    dm = DS.LesionsDataModule(data_dir=str(tmp_path / "raw"), centers=lesion_tree.CENTERS, batch_size=2, spatial_size=target)
    dm.setup("predict_train")
    ds = dm.predict_dataset
    samples = [ds[i] for i in range(len(ds))]
    assert len(samples) >= 2
    for i, s in enumerate(samples):
        img, seg = ds.load(i)
        lo, hi = DS.foreground_box(img, dm.margin)
        assert s["crop_origin"] == lo and s["crop_shape"] == tuple(b - a for a, b in zip(lo, hi)) and s["full_shape"] == seg.shape
        assert all(isinstance(v, int) for key in DS.GEOMETRY_KEYS for v in s[key])
        # the sample as it was before the keys were added, key by key
        ci, cs = DS.crop_foreground(img, seg, margin=dm.margin)
        x = np.ascontiguousarray(DS.resize_with_pad_or_crop(DS.normalize_nonzero(ci)[None], target))
        boxes, labels = DS.boxes_from_instances(DS.resize_with_pad_or_crop(cs[None], target), dm.thresholds, "instances")
        old = {"img": torch.from_numpy(x), "boxes": boxes, "labels": labels, "seg": [boxes, labels], "subject": ds.subjects[i],
               "img_meta_dict": {"affine": np.eye(4)}, "seg_meta_dict": {}, "img_transforms": [], "seg_transforms": []}
        assert set(s) == set(old) | set(DS.GEOMETRY_KEYS)
        assert torch.equal(s["img"], old["img"]) and torch.equal(s["boxes"], boxes) and torch.equal(s["labels"], labels)
        assert torch.equal(s["seg"][0], boxes) and torch.equal(s["seg"][1], labels) and s["subject"] == old["subject"]
        assert np.array_equal(s["img_meta_dict"]["affine"], np.eye(4)) and list(s["img_meta_dict"]) == ["affine"]
        assert s["seg_meta_dict"] == {} and s["img_transforms"] == [] and s["seg_transforms"] == []
    batch = DS.collate_fn(samples[:2])
    for key in DS.GEOMETRY_KEYS:
        assert batch[key] == [samples[0][key], samples[1][key]]
    assert batch["subject"] == [samples[0]["subject"], samples[1]["subject"]] and batch["img"].shape == (2, 1) + target
    assert set(batch) == {"img", "seg", "boxes", "labels", "subject", "img_meta_dict", "seg_meta_dict", "img_transforms",
                          "seg_transforms"} | set(DS.GEOMETRY_KEYS)
    # samples without the keys (the example data module) collate as before
    plain = [{k: v for k, v in s.items() if k not in DS.GEOMETRY_KEYS} for s in samples[:2]]
    assert not set(DS.collate_fn(plain)) & set(DS.GEOMETRY_KEYS)


# ---- predict.py's flags -------------------------------------------------------------------------------------------------
def test_parser_accepts_the_new_flags_and_keeps_the_old_defaults():
    from mslesions3d_amd.predict import build_parser
    old = {"dataset_path": r'../data/artificial_dataset', "dataset_name": None, "model_path": r'model_final.ckpt',
           "percentage": 1., "subject": None, "n_classes": 1, "num_workers": 0, "predict_subset": "train", "min_score": 0.5,
           "top_k": 100, "output_dir": r"../data/predictions/", "dtype": "f32", "data_module": "example",
           "centers": ['CHUV_RIM_OK', 'BASEL_INSIDER_OK'], "spatial_size": [250, 300, 300], "input_images": ["FLAIR"]}
    args = vars(build_parser().parse_args([]))
    assert {k: args[k] for k in old} == old
    assert args["save_images"] == 0 and args["cache"] == 0 and args["model_name"] is None
    assert set(args) == set(old) | {"save_images", "cache", "model_name"}
    # -c has been --n_classes since the first parser (the reference's own spelling), so the device feed is --cache
    args = build_parser().parse_args(["-c", "1", "--cache", "1", "-si", "1", "-mn", "NAME"])
    assert (args.n_classes, args.cache, args.save_images, args.model_name) == (1, 1, 1, "NAME")
    assert build_parser().parse_args(["-c", "2"]).n_classes == 2


def test_output_dir_takes_the_model_name_like_the_reference():
    from mslesions3d_amd.predict import build_parser, output_dir_of
    assert output_dir_of(build_parser().parse_args(["-o", "out"])) == "out"
    assert output_dir_of(build_parser().parse_args(["-o", "out", "-mn", "run7"])) == os.path.join("out", "run7")
