"""msl_augment_affine (csrc/datapipe.hip) and its routing through devicedata.DeviceCache against the host transforms of
datasets.py: the rotating affine bit for bit under the three boundaries, the intensity operations as single f32
roundings, untouched guard bands around the outputs, whole batches of the train_lesions() set, the trainer's replayed
program and the entry point."""
import json
import os

import numpy as np
import pytest
import torch

from mslesions3d_amd import _lib
from mslesions3d_amd import datasets as DS
from mslesions3d_amd.datasets import boxes_from_segmentation, draw_augmentations, sample_rng, select_augmentations
from mslesions3d_amd.devicedata import (AFFINE_STRIDE, BOUNDARY, OP_ADD, OP_MUL, AffineStage, DeviceCache, IntensityOp,
                                        affine_row, permute_numpy, sample_params)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NORM_RTOL, NORM_ATOL = 1e-5, 1e-5  # the normalisation bound of DESIGN.md §4.7 (tests/test_gpu_datapipe.py)
GUARD = 4096  # elements of guard band on either side of each output
IMG_PATTERN, SEG_PATTERN = 0x5A5AC3C3, 0xA5
LESIONS = ["flip", "rotate90", "affine", "shiftintensity", "scaleintensity"]
# (lo, hi) pairs that keep every draw away from the identity (tests/test_affine_cpu.py): >= 5 % of the output voxels
# sample outside the volume, asserted per case
ROT = {"rotate_range": ((0.2, 0.5), (-0.5, -0.2), (0.2, 0.5))}
VARIANTS = {"rotate": ROT, "rotate_scale": dict(ROT, scale_range=(0.2, 0.2, 0.2)),
            "rotate_scale_translate": dict(ROT, scale_range=(0.2, 0.2, 0.2), translate_range=((3, 8), (-8, -3), (3, 8)))}


def _volume(shape, seed):
    rs = np.random.RandomState(seed)
    img = rs.randn(*shape).astype(np.float32)
    seg = (rs.rand(*shape) < 0.3).astype(np.uint8) * rs.randint(1, 3, shape).astype(np.uint8)
    return img, seg


def _outside_share(shape, m, off):
    o = np.stack(np.meshgrid(*(np.arange(n) for n in shape), indexing="ij"), -1).astype(np.float64)
    c = o @ np.asarray(m).T + np.asarray(off)
    return float(((c < 0) | (c > np.array(shape) - 1)).any(-1).mean())


def _launch(img, seg, rows):
    """One msl_augment_affine launch: (n_src, D, H, W) device sources, rows (N, AFFINE_STRIDE) -> outputs on the host.
    The outputs sit between guard bands of a fixed bit pattern, which must come back intact."""
    rows = np.asarray(rows, dtype=np.float64)
    N, shape = rows.shape[0], tuple(img.shape[1:])
    assert rows.shape == (N, AFFINE_STRIDE)
    V = int(np.prod(shape))
    p = torch.from_numpy(rows).to(DEV)
    bi = torch.full((N * V + 2 * GUARD,), IMG_PATTERN, dtype=torch.int32, device=DEV)
    bs = torch.full((N * V + 2 * GUARD,), SEG_PATTERN, dtype=torch.uint8, device=DEV)
    oi, os_ = bi[GUARD:GUARD + N * V], bs[GUARD:GUARD + N * V]
    _lib.call("msl_augment_affine", img.data_ptr(), seg.data_ptr(), img.shape[0], p.data_ptr(), N, *shape,
              oi.data_ptr(), os_.data_ptr(), torch.cuda.current_stream().cuda_stream)
    hi, hs = bi.cpu(), bs.cpu()
    for band in (hi[:GUARD], hi[GUARD + N * V:]):
        assert bool((band == IMG_PATTERN).all()), "image guard band overwritten"
    for band in (hs[:GUARD], hs[GUARD + N * V:]):
        assert bool((band == SEG_PATTERN).all()), "mask guard band overwritten"
    return (hi[GUARD:GUARD + N * V].view(torch.float32).reshape((N,) + shape),
            hs[GUARD:GUARD + N * V].reshape((N,) + shape))


def _same(a, b):
    a, b = torch.as_tensor(np.ascontiguousarray(a)), torch.as_tensor(np.ascontiguousarray(b))
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return a.dtype == b.dtype and torch.equal(a, b)


# ---- 8 / 12. the rotating affine against the host transform, guard bands ---------------------------------------------
@pytest.mark.parametrize("shape,perm", [((32, 32, 32), ([2, 0, 1], [1, 0, 1])), ((64, 64, 64), ([1, 2, 0], [0, 1, 1])),
                                        ((48, 64, 64), ([0, 2, 1], [1, 1, 0]))])
@pytest.mark.parametrize("pad", ["reflection", "border", "zeros"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_affine_equals_the_host_transform(variant, pad, shape, perm):
    seeds = range(20)
    vols = [_volume(shape, s) for s in seeds]
    kw = dict(VARIANTS[variant], padding_mode=pad, prob=1.0)
    aug = [("affine", kw)]
    rows, want = [], []
    for s, (img, seg) in zip(seeds, vols):
        pi, ps = permute_numpy(img, perm), permute_numpy(seg, perm)
        want.append(DS._aug_affine(pi[None], ps[None], np.random.RandomState(s), **kw))
        _, (stage,) = sample_params(draw_augmentations(aug, np.random.RandomState(s)), shape, aug)
        assert isinstance(stage, AffineStage) and stage.boundary == BOUNDARY[pad]
        assert _outside_share(shape, stage.matrix, stage.offset) >= 0.05
        rows.append(affine_row(s, perm, stage))
    ti = torch.from_numpy(np.stack([v[0] for v in vols])).to(DEV)
    ts = torch.from_numpy(np.stack([v[1] for v in vols])).to(DEV)
    oi, os_ = _launch(ti, ts, rows)
    for s in seeds:
        assert torch.equal(os_[s], torch.from_numpy(want[s][1][0])), (variant, pad, shape, s)
        assert torch.equal(oi[s].view(torch.int32), torch.from_numpy(want[s][0][0]).view(torch.int32)), (variant, pad, shape, s)


def test_invalid_rows_write_zeros_and_read_nothing():
    img, seg = _volume((16, 16, 16), 0)
    ti, ts = torch.from_numpy(img[None]).to(DEV), torch.from_numpy(seg[None]).to(DEV)
    rows = [affine_row(1), affine_row(-1), affine_row(0, ([0, 0, 1], [0, 0, 0])), affine_row(0, ([0, 1, 5], [0, 0, 0])),
            affine_row(0)]
    oi, os_ = _launch(ti, ts, rows)
    assert not oi[:4].any() and not os_[:4].any()
    assert _same(oi[4], img) and _same(os_[4], seg)
    for bad in (dict(N=0), dict(D=0)):
        a = dict(N=1, D=16)
        a.update(bad)
        with pytest.raises(_lib.HipKernelError):
            _lib.call("msl_augment_affine", ti.data_ptr(), ts.data_ptr(), 1, ti.data_ptr(), a["N"], a["D"], 16, 16,
                      ti.data_ptr(), ts.data_ptr(), torch.cuda.current_stream().cuda_stream)


# ---- 9. intensity ---------------------------------------------------------------------------------------------------
def test_intensity_only_launch_is_a_permuted_copy_with_the_arithmetic():
    shape = (24, 24, 24)
    perm = ([1, 0, 2], [0, 1, 1])
    vols = [_volume(shape, s) for s in range(4)]
    add, mul = IntensityOp(OP_ADD, np.float32(0.0731)), IntensityOp(OP_MUL, np.float32(1.0 + 0.0457))
    lists = [[], [add], [mul, add], [add, mul, add, mul]]
    ti = torch.from_numpy(np.stack([v[0] for v in vols])).to(DEV)
    ts = torch.from_numpy(np.stack([v[1] for v in vols])).to(DEV)
    oi, os_ = _launch(ti, ts, [affine_row(n, perm, None, ops) for n, ops in enumerate(lists)])
    for n, ops in enumerate(lists):
        want = np.ascontiguousarray(permute_numpy(vols[n][0], perm))
        for op in ops:
            want = want + op.value if op.kind == OP_ADD else want * op.value
        assert want.dtype == np.float32 and _same(oi[n], want), n
        assert _same(os_[n], permute_numpy(vols[n][1], perm)), n


@pytest.mark.parametrize("pad", ["reflection", "border", "zeros"])
def test_affine_and_intensity_equal_the_host_chain(pad):
    shape = (32, 32, 32)
    augs = [("affine", dict(VARIANTS["rotate_scale_translate"], padding_mode=pad, prob=1.0)),
            ("shiftintensity", {"offsets": 0.1, "prob": 1.0}), ("scaleintensity", {"factors": 0.1, "prob": 1.0})]
    vols = [_volume(shape, s) for s in range(8)]
    rows, want = [], []
    for s, (img, seg) in enumerate(vols):
        rs = np.random.RandomState(s)
        x, m = img[None], seg[None]
        for name, kw in augs:
            x, m = DS.AUGMENTATIONS[name](x, m, rs, **kw)
        want.append((x[0], m[0]))
        perm, stages = sample_params(draw_augmentations(augs, np.random.RandomState(s)), shape, augs)
        rows.append(affine_row(s, perm, stages[0], stages[1:]))
    ti = torch.from_numpy(np.stack([v[0] for v in vols])).to(DEV)
    ts = torch.from_numpy(np.stack([v[1] for v in vols])).to(DEV)
    oi, os_ = _launch(ti, ts, rows)
    for s in range(len(vols)):
        assert _same(oi[s], want[s][0]) and _same(os_[s], want[s][1]), (pad, s)
    if pad == "zeros":  # outside the volume the image is cval 0 with the operations applied, not 0
        off, f = np.float32(rows[0][23]), np.float32(rows[0][25])
        assert off != 0 and (oi[0].numpy() == (np.float32(0) + off) * f).mean() >= 0.05


# ---- 10. whole batches ----------------------------------------------------------------------------------------------
def _dataset(tmp_path, augmentations, n=14, size=(32, 32, 32), batch=4):
    if not os.path.exists(tmp_path / "data"):
        DS.generate_artificial_dataset(str(tmp_path / "data"), "toy", num_images=n, image_size=size, object_size=(4, 10))
    ds = DS.ExampleDataset(data_dir=str(tmp_path / "data"), dataset_name="toy", batch_size=batch,
                           augmentations=augmentations)
    ds.setup("fit")
    return ds


def _snapshot(b):
    return {"img": b["img"].cpu(), "seg": b["seg"].cpu(), "gb": b["gb"].cpu(), "gl": b["gl"].cpu(),
            "obj_off": b["obj_off"].cpu(), "subject": list(b["subject"])}


def _check_against_host_functions(ds, cache, epochs=(0, 1)):
    """Every device batch against the host transforms applied to the CACHED volumes: everything bit-identical."""
    tr = ds.train_dataset
    drawn = {}
    for epoch in epochs:
        ds.set_epoch(epoch)
        host = list(ds.train_dataloader())
        dev = [_snapshot(b) for b in cache.train_batches(epoch)]
        assert [d["subject"] for d in dev] == [h["subject"] for h in host]
        for d, h in zip(dev, host):
            off = d["obj_off"].tolist()
            assert off[0] == 0 and len(off) == len(d["subject"]) + 1
            for n, s in enumerate(d["subject"]):
                slot = cache.slot[(tr.root, s)]
                x, m = cache.img[slot].cpu().numpy()[None], cache.seg[slot].cpu().numpy()[None]
                rs = sample_rng(tr.seed, epoch, s)
                for (name, kw), (_, dr) in zip(ds.augmentations, draw_augmentations(ds.augmentations,
                                                                                    sample_rng(tr.seed, epoch, s))):
                    x, m = DS.AUGMENTATIONS[name](x, m, rs, **kw)
                    drawn[name] = drawn.get(name, 0) + (dr is not None)
                assert _same(d["seg"][n], m[0]), (epoch, s)
                assert _same(d["img"][n, 0], x[0]), (epoch, s)
                boxes, labels = boxes_from_segmentation(m, ds.n_classes)
                assert _same(d["gb"][off[n]:off[n + 1]], boxes) and torch.equal(d["gl"][off[n]:off[n + 1]], labels)
                # and what the host LOADER makes of the same case: same mask-derived targets, image within the bound
                assert _same(boxes, h["boxes"][n]) and torch.equal(labels, h["labels"][n])
            np.testing.assert_allclose(d["img"].numpy(), h["img"].numpy(), rtol=NORM_RTOL, atol=NORM_ATOL)
    return drawn


def test_train_lesions_batches_equal_the_host_functions(tmp_path):
    ds = _dataset(tmp_path, select_augmentations(LESIONS))
    cache = DeviceCache(ds, DEV)
    drawn = _check_against_host_functions(ds, cache)
    assert drawn["shiftintensity"] == drawn["scaleintensity"] == 2 * len(ds.train_dataset) and drawn["flip"] > 0
    runs = [[_snapshot(b) for e in (0, 1) for b in cache.train_batches(e)] for _ in range(2)]
    for a, b in zip(*runs):
        assert all(_same(a[k], b[k]) for k in ("img", "seg", "gb", "gl", "obj_off"))


def test_batches_with_frequent_and_stacked_affines(tmp_path):
    """The named set draws its affine for one sample in ten; here every kind of stage is drawn often: a rotating affine
    with border padding, a translating one with zeros padding, an old diagonal stage, then the intensity pair."""
    les = dict(select_augmentations(["affine"])[0][1], prob=0.7)
    augs = select_augmentations(["flip", "rotate90", "scale"]) + [
        ("affine", les), ("affine", {"translate_range": (4, 4, 4), "padding_mode": "zeros", "prob": 0.5}),
        ("shiftintensity", {"offsets": 0.1, "prob": 0.5}), ("scaleintensity", {"factors": (0.0, 0.2), "prob": 0.5})]
    ds = _dataset(tmp_path, augs)
    drawn = _check_against_host_functions(ds, DeviceCache(ds, DEV))
    assert drawn["affine"] >= 10 and drawn["shiftintensity"] > 0 and drawn["scaleintensity"] > 0


def test_old_set_still_yields_the_host_loader_batches(tmp_path):
    ds = _dataset(tmp_path, select_augmentations(["flip", "rotate90", "translate", "scale"]))
    drawn = _check_against_host_functions(ds, DeviceCache(ds, DEV))
    assert drawn["affine"] > 0


def test_unsupported_orders_are_refused_at_construction(tmp_path):
    les = select_augmentations(LESIONS)
    for bad, msg in ((les[-2:] + les[:1], "a flip / rot90 after an intensity operation"),
                     (les[-1:] + les[-3:-2], "an affine stage after an intensity operation"),
                     (les[-3:-2] + les[:1], "a flip / rot90 after an affine stage")):
        with pytest.raises(NotImplementedError, match=msg):
            DeviceCache(_dataset(tmp_path, bad), DEV)


# ---- 11. trainer and entry point ------------------------------------------------------------------------------------
def _model(size, seed=1234):
    from mslesions3d_amd.ssd3d import LSSD3D
    from tests.golden import detinit
    m = LSSD3D(n_classes=2, input_channels=1, input_size=size, threshold=[0.1, 0.2], lr=1e-3)
    m.load_state_dict(detinit.fill_state_dict(m.state_dict(), seed))
    return m.to(DEV).train()


def test_trainer_replays_one_program(tmp_path):
    from mslesions3d_amd.trainer import FusedTrainer
    lib = _lib.load()
    assert lib.msl_program_fn_id(b"msl_augment_affine") >= 0  # recorded programs can carry the launch
    assert lib.msl_program_fn_id(b"msl_augment_affine") != lib.msl_program_fn_id(b"msl_augment_resample")
    ds = _dataset(tmp_path, select_augmentations(LESIONS), size=(64, 64, 64), n=10, batch=2)
    cache = DeviceCache(ds, DEV)
    tr = FusedTrainer(_model((64, 64, 64)))
    steps, mem, epoch = 0, [], 0
    while steps < 20:
        for b in cache.train_batches(epoch):
            out = cache.step(tr, b, metrics=steps % 3 == 0)
            assert np.isfinite(out["loss"])
            steps += 1
            if steps in (5, 20):
                torch.cuda.synchronize()
                mem.append(torch.cuda.memory_allocated(DEV))
            if steps == 20:
                break
        epoch += 1
    assert len(tr._programs) == 1  # 8 training cases, batch 2: one shape, one recorded program
    assert mem[0] == mem[1]


@pytest.mark.parametrize("cache", [1, 0])
def test_train_entry_point_with_the_lesions_set(tmp_path, cache):
    from mslesions3d_amd import train as T
    DS.generate_artificial_dataset(str(tmp_path / "data"), "toy64", num_images=10, image_size=(64, 64, 64))
    args = T.build_parser().parse_args(["-d", str(tmp_path / "data"), "-dn", "toy64", "-b", "2", "-me", "2",
                                        "-ld", str(tmp_path / "logs"), "-en", "run", "-c", str(cache), "-a", *LESIONS])
    T.example(args)
    recs = [json.loads(l) for l in open(tmp_path / "logs" / "run" / "metrics.jsonl")]
    train = [r["total_loss/training"] for r in recs if "total_loss/training" in r]
    val = [r["avg_val_loss"] for r in recs if "avg_val_loss" in r]
    assert len(train) >= 2 and len(val) == 2 and np.isfinite(train).all() and np.isfinite(val).all()
