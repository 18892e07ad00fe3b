"""Host side of the device data pipeline (devicedata.py, train.py -c): the CLI flag, the per-sample random draws, the
signed axis permutation that replaces flip / rot90, and the batch order.  CPU only."""
import numpy as np
import pytest

from mslesions3d_amd import datasets
from mslesions3d_amd.datasets import (AUGMENTATIONS, REFERENCE_AUGMENTATIONS, ExampleDataset, draw_augmentations,
                                      generate_artificial_dataset, select_augmentations)
from mslesions3d_amd.devicedata import permute_numpy, sample_params, train_batch_order
from mslesions3d_amd.train import build_parser


def test_cache_flag():
    p = build_parser()
    assert p.parse_args([]).cache == 0
    assert p.parse_args(["-c", "1"]).cache == 1
    assert p.parse_args(["--cache", "1"]).cache == 1


@pytest.mark.parametrize("entry", range(len(REFERENCE_AUGMENTATIONS)))
def test_draws_consume_the_host_stream(entry):
    """The draw of each reference entry leaves the RandomState where the host transform leaves it (50 seeds)."""
    t = select_augmentations([REFERENCE_AUGMENTATIONS[entry][0]])
    t = [x for x in t if x[1] is REFERENCE_AUGMENTATIONS[entry][1]]
    assert len(t) == 1
    name, kw = t[0]
    img = np.random.RandomState(0).rand(1, 6, 6, 6).astype(np.float32)
    seg = (img > 0.5).astype(np.uint8)
    for seed in range(50):
        a, b = np.random.RandomState(seed), np.random.RandomState(seed)
        AUGMENTATIONS[name](img, seg, a, **kw)
        draw_augmentations(t, b)
        sa, sb = a.get_state(), b.get_state()
        assert sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:], (entry, seed)


def test_all_draws_in_call_order():
    augs = select_augmentations(["flip", "rotate90", "translate", "scale"])
    img = np.random.RandomState(1).rand(1, 8, 8, 8).astype(np.float32)
    seg = (img > 0.7).astype(np.uint8)
    for seed in range(50):
        a, b = np.random.RandomState(seed), np.random.RandomState(seed)
        x, s = img, seg
        for name, kw in augs:
            x, s = AUGMENTATIONS[name](x, s, a, **kw)
        draws = draw_augmentations(augs, b)
        assert len(draws) == len(augs)
        assert a.randint(1 << 30) == b.randint(1 << 30)


def test_permutation_equals_flip_rot90():
    """sample_params' signed permutation reproduces np.flip / np.rot90 exactly, for every drawn combination."""
    augs = select_augmentations(["flip", "rotate90"])
    vol = np.arange(7 ** 3, dtype=np.int32).reshape(7, 7, 7)
    seen = set()
    for seed in range(400):
        a, b = np.random.RandomState(seed), np.random.RandomState(seed)
        x, s = vol[None], vol[None]
        for name, kw in augs:
            x, s = AUGMENTATIONS[name](x, s, a, **kw)
        perm, stages = sample_params(draw_augmentations(augs, b), vol.shape)
        assert stages == []
        assert np.array_equal(permute_numpy(vol, perm), x[0]), seed
        seen.add((tuple(perm[0]), tuple(perm[1])))
    assert len(seen) > 20
    for k in (1, 2, 3):
        for ax in ((0, 1), (1, 2), (0, 2)):
            perm, _ = sample_params([("rotate90", (k, ax))], vol.shape)
            assert np.array_equal(permute_numpy(vol, perm), np.rot90(vol, k, ax))


def test_affine_stage_parameters():
    augs = select_augmentations(["translate", "scale"])
    shape = (9, 10, 11)
    for seed in range(20):
        d = draw_augmentations(augs, np.random.RandomState(seed))
        _, stages = sample_params(d, shape)
        assert len(stages) == 2
        for (name, dr), st in zip(d, stages):
            assert (dr is None) == (st is None)
            if st is not None:
                assert st[0] == list(dr[0])
                assert np.array_equal(np.array(st[1]), datasets.affine_offset(shape, *dr))


def test_shape_changing_rot90_is_refused():
    with pytest.raises(NotImplementedError):
        sample_params([("rotate90", (1, (0, 1)))], (8, 9, 9))
    with pytest.raises(NotImplementedError):
        sample_params([("affine", None), ("flip", (0,))], (8, 8, 8))


@pytest.mark.parametrize("rank,world,epoch", [(0, 1, 0), (0, 1, 3), (1, 2, 0), (2, 3, 5), (0, 4, 1)])
def test_batch_order_equals_host_loader(tmp_path, rank, world, epoch):
    generate_artificial_dataset(str(tmp_path), "toy", num_images=23, image_size=(8, 8, 8), object_size=(2, 4))
    ds = ExampleDataset(data_dir=str(tmp_path), dataset_name="toy", batch_size=3, rank=rank, world_size=world)
    ds.setup("fit")
    ds.set_epoch(epoch)
    host = [list(b["subject"]) for b in ds.train_dataloader()]
    dev = [[ds.train_dataset.subjects[i] for i in chunk] for chunk in train_batch_order(ds, epoch)]
    assert dev == host
