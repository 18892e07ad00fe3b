"""Device data pipeline (csrc/datapipe.hip, devicedata.py, train.py -c 1) against the host pipeline of datasets.py:
connected-component boxes bit for bit, flip / rot90 exactly, translate / scale as scipy computes them, normalisation
within its bound, whole batches, determinism, the trainer's replayed program and the entry point."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from mslesions3d_amd import _lib
from mslesions3d_amd import datasets as DS
from mslesions3d_amd.datasets import boxes_from_segmentation, draw_augmentations, select_augmentations
from mslesions3d_amd.devicedata import (PARAM_STRIDE, DeviceCache, boxes_from_segmentation_device, permute_numpy,
                                        sample_params)
from mslesions3d_amd.synth import generate_volume

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
# NormalizeIntensity: the device reduces in f64, numpy in f32 pairwise; the mean / std it rounds to f32 may then differ
# by an ulp, which moves a normalised voxel by at most a few f32 ulps of its own magnitude plus ulp(mean) / std
NORM_RTOL, NORM_ATOL = 1e-5, 1e-5


def _check_boxes(masks, n_classes=1, capacity=None):
    seg = torch.from_numpy(np.ascontiguousarray(np.stack(masks)).astype(np.uint8)).to(DEV)
    boxes, labels, (gb, gl, off, cap) = boxes_from_segmentation_device(seg, n_classes, capacity=capacity)
    for n, m in enumerate(masks):
        hb, hl = boxes_from_segmentation(m[None], n_classes)
        db, dl = boxes[n].cpu(), labels[n].cpu()
        assert db.dtype == torch.float32 and dl.dtype == torch.int64
        assert torch.equal(db.view(torch.int32), hb.view(torch.int32)), (n, db, hb)
        assert torch.equal(dl, hl), n
    return sum(int(b.shape[0]) for b in boxes)


@pytest.mark.parametrize("size", [(32, 32, 32), (64, 64, 64), (128, 128, 128), (48, 64, 64)])
def test_boxes_generator_masks(size):
    masks = [generate_volume(i, size, (1, 8), (4, 14), 7)[1] for i in range(3)]
    assert _check_boxes(masks) > 0


def test_boxes_two_classes():
    rs = np.random.RandomState(3)
    masks = []
    for _ in range(3):
        m = np.zeros((40, 40, 40), np.uint8)
        for _ in range(12):
            e = rs.randint(2, 9)
            o = rs.randint(0, 40 - e, 3)
            m[o[0]:o[0] + e, o[1]:o[1] + e, o[2]:o[2] + e] = rs.randint(1, 3)
        masks.append(m)
    assert _check_boxes(masks, n_classes=2) > 0
    assert _check_boxes(masks, n_classes=1) > 0  # class 2 voxels are background for one class


def test_boxes_edge_and_corner_contacts_stay_separate():
    m = np.zeros((20, 20, 20), np.uint8)
    m[2:5, 2:5, 2:5] = 1
    m[5:8, 5:8, 2:5] = 1      # shares an edge with the first
    m[8:11, 8:11, 5:8] = 1    # shares a corner with the second
    m[12:15, 2:5, 2:5] = 1
    m[12:15, 5:8, 2:5] = 1    # shares a face: merged
    assert _check_boxes([m]) == 4


def test_boxes_u_shapes_and_spirals():
    u = np.zeros((32, 32, 32), np.uint8)
    for k in range(4):  # nested U shapes whose arms meet only at the bottom
        z = 2 + 7 * k
        u[z:z + 3, 2:28, 2:4] = 1
        u[z:z + 3, 2:28, 26:28] = 1
        u[z:z + 3, 26:28, 2:28] = 1
    s = np.zeros((33, 33, 33), np.uint8)
    y, x, dy, dx = 16, 16, 0, 1
    steps, length = 0, 1
    while 0 <= y < 33 and 0 <= x < 33:  # a square spiral in every third plane, the planes joined at one end
        for _ in range(2):
            for _ in range(length):
                if 0 <= y < 33 and 0 <= x < 33:
                    s[1::3, y, x] = 1
                y, x = y + dy, x + dx
            dy, dx = dx, -dy
        length += 2
        steps += 1
    s[:, 16, 16] = 1
    c = np.zeros((30, 30, 30), np.uint8)  # comb: teeth joined only by the last row
    c[2:28, 2:28:2, 5] = 1
    c[27, 2:28, 5] = 1
    assert _check_boxes([u[:30, :30, :30], s[:30, :30, :30], c]) > 0


def test_boxes_single_voxels_flat_and_faces():
    m = np.zeros((24, 24, 24), np.uint8)
    m[3, 3, 3] = 1                  # single voxel: dropped
    m[6, 2:9, 2:9] = 1              # flat: dropped
    m[10:13, 10, 4:9] = 1           # flat in y: dropped
    m[0:3, 10:14, 10:14] = 1        # every face of the volume
    m[21:24, 10:14, 10:14] = 1
    m[10:14, 0:3, 15:19] = 1
    m[10:14, 21:24, 15:19] = 1
    m[15:19, 15:19, 0:3] = 1
    m[15:19, 15:19, 21:24] = 1
    m[0:24, 0:2, 0:2] = 1           # an edge of the volume
    assert _check_boxes([m]) == 7  # six face cubes and the edge bar


def test_boxes_empty_full_and_noise():
    rs = np.random.RandomState(0)
    noise = (rs.rand(48, 48, 48) < 0.35).astype(np.uint8)  # percolating clusters: many merges
    assert _check_boxes([np.zeros((16, 16, 16), np.uint8), np.ones((16, 16, 16), np.uint8)]) == 1
    _check_boxes([noise, (rs.rand(48, 48, 48) < 0.2).astype(np.uint8)], capacity=65536)


def test_boxes_thousands_of_components():
    m = np.zeros((40, 40, 40), np.uint8)
    for z in range(0, 39, 3):
        for y in range(0, 39, 3):
            for x in range(0, 39, 3):
                m[z:z + 2, y:y + 2, x:x + 2] = 1
    assert _check_boxes([m, m[::-1].copy()], capacity=8192) == 2 * 13 ** 3


def test_boxes_overflow_raises():
    m = np.zeros((2, 20, 20, 20), np.uint8)
    for k in range(5):
        m[:, 3 * k:3 * k + 2, 2:5, 2:5] = 1
    seg = torch.from_numpy(m).to(DEV)
    assert len(boxes_from_segmentation_device(seg, 1, capacity=10)[0][1]) == 5
    with pytest.raises(_lib.HipKernelError, match="capacity of 9"):
        boxes_from_segmentation_device(seg, 1, capacity=9)


# ---- augmentation -------------------------------------------------------------------------------------------------
def _resample(img, seg, rows):
    """One msl_augment_resample launch of (N, D, H, W) tensors with parameter rows (N, PARAM_STRIDE)."""
    N = img.shape[0]
    p = torch.from_numpy(np.asarray(rows, dtype=np.float64).reshape(N, PARAM_STRIDE)).to(DEV)
    oi, os_ = torch.empty_like(img), torch.empty_like(seg)
    _lib.call("msl_augment_resample", img.data_ptr(), seg.data_ptr(), N, p.data_ptr(), N, *img.shape[1:],
              oi.data_ptr(), os_.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return oi.cpu().numpy(), os_.cpu().numpy()


def _row(n, perm=((0, 1, 2), (0, 0, 0)), affine=None):
    r = np.zeros(PARAM_STRIDE)
    r[0], r[1:4], r[4:7] = n, perm[0], perm[1]
    if affine is not None:
        r[7], r[8:11], r[11:14] = 1, affine[0], affine[1]
    return r


def _volume(shape, seed):
    rs = np.random.RandomState(seed)
    img = rs.randn(*shape).astype(np.float32)
    seg = (rs.rand(*shape) < 0.3).astype(np.uint8) * rs.randint(1, 3, shape).astype(np.uint8)
    return img, seg


def test_flip_and_rot90_exact():
    img, seg = _volume((12, 12, 12), 0)
    ti, ts = torch.from_numpy(img[None]).to(DEV), torch.from_numpy(seg[None]).to(DEV)
    draws = [[("flip", ax)] for ax in ((0,), (1,), (2,), (0, 1, 2), (1, 2))]
    draws += [[("rotate90", (k, ax))] for k in (1, 2, 3) for ax in ((0, 1), (1, 2), (0, 2))]
    for d in draws:
        perm, _ = sample_params(d, img.shape)
        oi, os_ = _resample(ti, ts, [_row(0, perm)])
        if d[0][0] == "flip":
            ri, rsg = np.flip(img, d[0][1]), np.flip(seg, d[0][1])
        else:
            ri, rsg = np.rot90(img, d[0][1][0], d[0][1][1]), np.rot90(seg, d[0][1][0], d[0][1][1])
        assert np.array_equal(oi[0], ri) and np.array_equal(os_[0], rsg), d
        assert np.array_equal(permute_numpy(img, perm), ri)


@pytest.mark.parametrize("which", ["translate", "scale", "both"])
def test_translate_scale_match_scipy(which):
    """_aug_affine (scipy.ndimage.affine_transform, reflect) over 20 seeds: mask exact, image bit for bit (bound: 0 ulp)."""
    names = ["translate", "scale"] if which == "both" else [which]
    augs = [(n, dict(kw, prob=1.0)) for n, kw in select_augmentations(names)]
    shape = (20, 24, 28)
    worst = 0
    for seed in range(20):
        img, seg = _volume(shape, seed)
        hi, hs = img[None], seg[None]
        rs = np.random.RandomState(seed)
        for name, kw in augs:
            hi, hs = DS.AUGMENTATIONS[name](hi, hs, rs, **kw)
        _, stages = sample_params(draw_augmentations(augs, np.random.RandomState(seed)), shape)
        di, ds_ = img[None], seg[None]
        for st in stages:
            di, ds_ = _resample(torch.from_numpy(np.ascontiguousarray(di)).to(DEV),
                                torch.from_numpy(np.ascontiguousarray(ds_)).to(DEV), [_row(0, affine=st)])
        assert np.array_equal(ds_, hs), seed
        ulp = np.abs(di.view(np.int32).astype(np.int64) - hi.astype(np.float32).view(np.int32).astype(np.int64)).max()
        worst = max(worst, int(ulp))
    assert worst == 0, worst


# ---- normalize ----------------------------------------------------------------------------------------------------
def _host_normalize(img):
    img = img.copy()
    nz = img != 0
    if nz.any():
        std = img[nz].std()
        img[nz] = (img[nz] - img[nz].mean()) / (std if std != 0 else 1.0)
    return img


def test_normalize_nonzero():
    rs = np.random.RandomState(5)
    shape = (64, 64, 16)
    vols = [generate_volume(i, shape, random_seed=2)[0].astype(np.float32) for i in range(2)]
    sparse = rs.randn(*shape).astype(np.float32) * 3 + 7
    sparse[rs.rand(*shape) < 0.6] = 0
    const = np.zeros(shape, np.float32)
    const[5:20, 5:20, 5:10] = 2.5
    vols += [sparse, const, np.zeros(shape, np.float32)]
    V = int(np.prod(shape))
    outs = []
    for _ in range(2):
        x = torch.from_numpy(np.stack(vols)).to(DEV)
        _lib.call("msl_normalize_nonzero", x.data_ptr(), len(vols), V, torch.cuda.current_stream().cuda_stream)
        outs.append(x.cpu().numpy())
    assert np.array_equal(outs[0].view(np.int32), outs[1].view(np.int32))  # run to run
    for v, o in zip(vols, outs[0]):
        assert np.array_equal(o[v == 0], v[v == 0])                     # zeros stay zero
        np.testing.assert_allclose(o, _host_normalize(v), rtol=NORM_RTOL, atol=NORM_ATOL)
    assert np.array_equal(outs[0][-1], vols[-1])                        # all zero: unchanged
    assert np.all(outs[0][-2][vols[-2] != 0] == 0)                      # constant: std 0 -> divide by 1


# ---- whole batches --------------------------------------------------------------------------------------------------
def _dataset(tmp_path, augment, n_classes=1, n=14, size=(32, 32, 32), batch=4, rank=0, world=1):
    if not os.path.exists(tmp_path / "data"):
        DS.generate_artificial_dataset(str(tmp_path / "data"), "toy", num_images=n, image_size=size, object_size=(4, 10))
    ds = DS.ExampleDataset(data_dir=str(tmp_path / "data"), dataset_name="toy", batch_size=batch, rank=rank,
                           world_size=world, augmentations=DS.select_augmentations(augment))
    ds.setup("fit")
    return ds


def _unpack(b):
    off = b["obj_off"].cpu().tolist()
    gb, gl = b["gb"].cpu(), b["gl"].cpu()
    return [gb[off[n]:off[n + 1]] for n in range(len(off) - 1)], [gl[off[n]:off[n + 1]] for n in range(len(off) - 1)]


@pytest.mark.parametrize("augment", [[], ["flip", "rotate90", "translate", "scale"]])
def test_batches_equal_the_host_loader(tmp_path, augment):
    ds = _dataset(tmp_path, augment)
    cache = DeviceCache(ds, DEV)
    assert cache.nbytes() >= 14 * 32 ** 3 * 5 and "MiB" in cache.footprint()
    for epoch in (0, 1):
        ds.set_epoch(epoch)
        host = list(ds.train_dataloader())
        dev = list(b for b in ({**b, "host": _unpack(b), "img_h": b["img"].cpu()} for b in cache.train_batches(epoch)))
        assert [b["subject"] for b in dev] == [h["subject"] for h in host]
        for d, h in zip(dev, host):
            boxes, labels = d["host"]
            for db, hb, dl, hl in zip(boxes, h["boxes"], labels, h["labels"]):
                assert torch.equal(db.view(torch.int32), hb.view(torch.int32)) and torch.equal(dl, hl)
            np.testing.assert_allclose(d["img_h"].numpy(), h["img"].numpy(), rtol=NORM_RTOL, atol=NORM_ATOL)
    val_h = list(ds.test_dataloader())
    val_d = list(cache.val_batches())
    assert [b["subject"] for b in val_d] == [b["subject"] for b in val_h]
    for d, h in zip(val_d, val_h):
        for db, hb in zip(d["boxes"], h["boxes"]):
            assert torch.equal(db.cpu(), hb)
        np.testing.assert_allclose(d["img"].cpu().numpy(), h["img"].numpy(), rtol=NORM_RTOL, atol=NORM_ATOL)


def test_batches_two_classes_non_cube(tmp_path):
    root = tmp_path / "data" / "multiple_objects" / "double_class" / "toy"
    os.makedirs(root / "images")
    os.makedirs(root / "labels")
    rs = np.random.RandomState(1)
    for i in range(6):
        img = rs.rand(24, 32, 32).astype(np.float32)
        seg = np.zeros(img.shape, np.uint8)
        for _ in range(6):
            e = rs.randint(3, 8)
            o = [rs.randint(0, s - e) for s in img.shape]
            seg[o[0]:o[0] + e, o[1]:o[1] + e, o[2]:o[2] + e] = rs.randint(1, 3)
        np.save(root / "images" / f"sub-{i:04d}_image.npy", img)
        np.save(root / "labels" / f"sub-{i:04d}_seg.npy", seg)
    ds = DS.ExampleDataset(n_classes=2, data_dir=str(tmp_path / "data"), dataset_name="toy", batch_size=2,
                           augmentations=DS.select_augmentations(["flip", "rotate90", "translate", "scale"]))
    ds.setup("fit")
    # rot90 over (0, 1) / (0, 2) would change a 24 x 32 x 32 volume's shape
    with pytest.raises(NotImplementedError):
        DeviceCache(ds, DEV)
    ds = DS.ExampleDataset(n_classes=2, data_dir=str(tmp_path / "data"), dataset_name="toy", batch_size=2,
                           augmentations=DS.select_augmentations(["flip", "translate", "scale"]))
    ds.setup("fit")
    cache = DeviceCache(ds, DEV)
    host = list(ds.train_dataloader())
    for d, h in zip(cache.train_batches(0), host):
        boxes, labels = _unpack(d)
        assert d["subject"] == h["subject"]
        for db, hb, dl, hl in zip(boxes, h["boxes"], labels, h["labels"]):
            assert torch.equal(db, hb) and torch.equal(dl, hl)


def test_pipeline_is_deterministic(tmp_path):
    ds = _dataset(tmp_path, ["flip", "rotate90", "translate", "scale"], size=(64, 64, 64), n=8)
    cache = DeviceCache(ds, DEV)
    runs = []
    for _ in range(2):
        runs.append([(b["img"].cpu(), b["seg"].cpu(), b["gb"].cpu(), b["gl"].cpu(), b["obj_off"].cpu())
                     for b in cache.train_batches(3)])
    for a, b in zip(*runs):
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.uint8) if x.dtype != torch.uint8 else x,
                               y.view(torch.uint8) if y.dtype != torch.uint8 else y)


# ---- trainer --------------------------------------------------------------------------------------------------------
def _model(size, seed=1234):
    from mslesions3d_amd.ssd3d import LSSD3D
    from tests.golden import detinit
    m = LSSD3D(n_classes=2, input_channels=1, input_size=size, threshold=[0.1, 0.2], lr=1e-3)
    m.load_state_dict(detinit.fill_state_dict(m.state_dict(), seed))
    return m.to(DEV).train()


def test_trainer_replays_one_program(tmp_path):
    from mslesions3d_amd.trainer import FusedTrainer
    ds = _dataset(tmp_path, ["flip", "rotate90", "translate", "scale"], size=(64, 64, 64), n=10, batch=2)
    cache = DeviceCache(ds, DEV)
    tr = FusedTrainer(_model((64, 64, 64)))
    steps, mem = 0, []
    epoch = 0
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


def test_first_step_matches_host_fed_step(tmp_path):
    from mslesions3d_amd.trainer import FusedTrainer
    ds = _dataset(tmp_path, [], size=(64, 64, 64), n=10, batch=2)
    cache = DeviceCache(ds, DEV)
    b = next(iter(cache.train_batches(0)))
    a = cache.step(FusedTrainer(_model((64, 64, 64))), b)
    ds.set_epoch(0)
    h = next(iter(ds.train_dataloader()))
    r = FusedTrainer(_model((64, 64, 64))).step(h["img"].to(DEV), h["boxes"], h["labels"])
    for k in ("conf", "loc"):
        assert abs(a[k] - r[k]) <= 1e-4 * abs(r[k]), (k, a[k], r[k])
    assert a["n_positives"] == r["n_positives"]


def test_bf16_step(tmp_path):
    from mslesions3d_amd.trainer import FusedTrainer
    ds = _dataset(tmp_path, ["flip", "translate"], size=(64, 64, 64), n=6, batch=2)
    cache = DeviceCache(ds, DEV)
    m = _model((64, 64, 64))
    m.compute_dtype = "bf16"
    out = cache.step(FusedTrainer(m), next(iter(cache.train_batches(0))))
    assert np.isfinite(out["loss"]) and out["n_positives"] > 0


def test_overflow_surfaces_at_the_step(tmp_path):
    from mslesions3d_amd.trainer import FusedTrainer
    ds = _dataset(tmp_path, [], size=(64, 64, 64), n=6, batch=2)
    cache = DeviceCache(ds, DEV, max_objects_per_image=1)  # the generator puts 2-5 cubes in every volume
    with pytest.raises(_lib.HipKernelError, match="capacity of 2"):
        cache.step(FusedTrainer(_model((64, 64, 64))), next(iter(cache.train_batches(0))))


# ---- entry point ----------------------------------------------------------------------------------------------------
def _run_train(tmp_path, cache, extra=()):
    from mslesions3d_amd import train as T
    args = T.build_parser().parse_args(["-d", str(tmp_path / "data"), "-dn", "toy64", "-b", "2", "-me", "2",
                                        "-ld", str(tmp_path / "logs"), "-en", f"c{cache}", "-c", str(cache), *extra])
    T.example(args)
    return [json.loads(l) for l in open(tmp_path / "logs" / f"c{cache}" / "metrics.jsonl")]


def test_train_entry_point_cache(tmp_path):
    DS.generate_artificial_dataset(str(tmp_path / "data"), "toy64", num_images=10, image_size=(64, 64, 64))
    host = _run_train(tmp_path, 0)
    dev = _run_train(tmp_path, 1)
    assert [sorted(r) for r in host] == [sorted(r) for r in dev]
    assert os.path.exists(tmp_path / "logs" / "c1" / "last.ckpt")
    # epoch 0 only differs by the normalisation bound of the inputs: the losses agree to 1e-3 relative
    for h, d in zip(host, dev):
        if h["epoch"] == 0 and "total_loss/training" in h:
            assert abs(h["total_loss/training"] - d["total_loss/training"]) <= 1e-3 * abs(h["total_loss/training"])
        if h["epoch"] == 0 and "avg_val_loss" in h:
            assert abs(h["avg_val_loss"] - d["avg_val_loss"]) <= 1e-3 * abs(h["avg_val_loss"])


def test_train_entry_point_cache_options(tmp_path):
    DS.generate_artificial_dataset(str(tmp_path / "data"), "toy64", num_images=6, image_size=(64, 64, 64))
    recs = _run_train(tmp_path, 1, ["--dtype", "bf16", "-a", "flip", "rotate90", "translate", "scale"])
    assert any("total_loss/training" in r for r in recs) and any("avg_val_loss" in r for r in recs)


def test_train_entry_point_cache_two_ranks(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    DS.generate_artificial_dataset(str(tmp_path / "data"), "toy64", num_images=10, image_size=(64, 64, 64))
    env = dict(os.environ, MSL_DP_BACKEND="gloo", MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2", PYTHONPATH=root)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), "-m", "mslesions3d_amd.train", "-d", str(tmp_path / "data"), "-dn", "toy64", "-b", "2",
           "-me", "1", "-ld", str(tmp_path / "logs"), "-en", "run", "-c", "1", "-a", "flip", "translate"]
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [json.loads(l) for l in open(tmp_path / "logs" / "run" / "metrics.jsonl")]
    assert sum("avg_val_loss" in l for l in lines) == 1
    assert [l["step"] for l in lines if "total_loss/training" in l] == [1, 2]
