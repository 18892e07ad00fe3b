"""msl_foreground_box, msl_augment_fit (the C = 1 forwards of the one foreground / fit kernel) and msl_instance_boxes
(csrc/datapipe.hip) through the C ABI, and the one-sequence route through devicedata.LesionCache (the _mc entry points
with C = 1) and the entry point, against the host pipeline of datasets.LesionsDataModule."""
import json
import os

import numpy as np
import pytest
import torch

from mslesions3d_amd import _lib
from mslesions3d_amd import datasets as DS
from mslesions3d_amd.devicedata import (AFFINE_STRIDE, LesionCache, LesionPredictFeed, _InstBoxOut,
                                        boxes_from_instances_device, fit_rows, sample_params)
from tests import lesion_tree

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NORM_RTOL, NORM_ATOL = 1e-5, 1e-5  # the normalisation bound of DESIGN.md §4.7 (tests/test_gpu_datapipe.py)
GUARD = 4096
IMG_PATTERN, SEG_PATTERN = 0x5A5AC3C3, 0x5AA5
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "instances.npz"))
INF = np.iinfo(np.int32).max
INSTANCE_CASES = [str(n) for n in GOLD["names"] if str(GOLD[f"{n}__mode"]) == "instances"]
LESIONS = ["flip", "rotate90", "affine", "shiftintensity", "scaleintensity"]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(a, b):
    a, b = _bits(a), _bits(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


# ---- msl_foreground_box ------------------------------------------------------------------------------------------------
def _fg_cases():
    rs = np.random.RandomState(0)
    out = []
    for shape, lo, hi in (((40, 50, 70), (9, 11, 13), (30, 41, 66)), ((33, 65, 129), (0, 2, 60), (33, 64, 70)),
                          ((20, 20, 20), (7, 7, 7), (8, 8, 8)), ((17, 31, 300), (3, 3, 290), (12, 20, 300))):
        v = np.zeros(shape, np.float32)
        sl = tuple(slice(a, b) for a, b in zip(lo, hi))
        v[sl] = (rs.rand(*[b - a for a, b in zip(lo, hi)]) < 0.4).astype(np.float32) * 3
        v[sl][tuple(0 for _ in lo)] = 1  # both corners of the box are foreground
        v[tuple(b - 1 for b in hi)] = 2
        v[tuple(0 for _ in shape)] = -5  # negative and zero voxels are background
        out.append(v)
    out.append(np.zeros((12, 13, 14), np.float32))          # empty: the whole volume
    out.append(-np.ones((12, 13, 14), np.float32))
    out.append(np.ones((9, 10, 11), np.float32))
    return out


@pytest.mark.parametrize("margin", [5, 0, 2])
def test_foreground_box_equals_the_host_box(margin):
    for v in _fg_cases():
        box = torch.full((8,), -77, dtype=torch.int32, device=DEV)
        _lib.call("msl_foreground_box", torch.from_numpy(v).to(DEV).data_ptr(), *v.shape, margin, box.data_ptr(), _stream())
        got = box.cpu().tolist()
        lo, hi = DS.foreground_box(v, margin)
        assert got[:6] == list(lo) + list(hi), (v.shape, margin)
        assert got[6:] == [-77, -77]
    with pytest.raises(_lib.HipKernelError):
        _lib.call("msl_foreground_box", box.data_ptr(), 0, 4, 4, 5, box.data_ptr(), _stream())


# ---- msl_instance_boxes ------------------------------------------------------------------------------------------------
def _device_boxes(segs, thr, capacity):
    """-> (gb, gl, obj_off, flag) on the host for a list of equal-shape int16 masks."""
    seg = torch.from_numpy(np.stack(segs).astype(np.int16)).to(DEV)
    out = _InstBoxOut(len(segs), seg.shape[1:], thr, capacity, DEV)
    out.gb.fill_(-1.0)
    out.launch(seg, _stream())
    torch.cuda.synchronize()
    return out.gb.cpu(), out.gl.cpu(), out.obj_off.cpu().tolist(), int(out.flag.item())


@pytest.mark.parametrize("name", INSTANCE_CASES)
def test_instance_boxes_match_the_reference_bit_for_bit(name):
    thr = [(int(a), int(b)) for a, b in GOLD[f"{name}__thresholds"]]
    gb, gl, off, flag = _device_boxes([GOLD[f"{name}__seg"]], thr, 64)
    want_b, want_l = GOLD[f"{name}__boxes"], GOLD[f"{name}__labels"]
    assert flag == 0 and off == [0, len(want_l)]
    assert _same(gb[:off[1]], want_b) and np.array_equal(gl[:off[1]].numpy(), want_l)
    assert bool((gb[off[1]:] == -1.0).all())  # rows past the end untouched


def test_instance_boxes_batch_order_and_determinism():
    from scipy.ndimage import label
    names = ["random_0", "one_class", "binary", "flat24"]
    segs = [GOLD["random_0__seg"], GOLD["one_class__seg"], label(GOLD["binary__seg"])[0].astype(np.int16),
            np.zeros((24, 24, 24), np.int16)]
    runs = [_device_boxes(segs, [(1, INF)], 64) for _ in range(2)]
    gb, gl, off, flag = runs[0]
    assert flag == 0 and off[0] == 0 and off[3] == off[4]  # the last image is empty
    for n, name in enumerate(names[:3]):
        assert _same(gb[off[n]:off[n + 1]], GOLD[f"{name}__boxes"]), name
        assert np.array_equal(gl[off[n]:off[n + 1]].numpy(), GOLD[f"{name}__labels"]), name
    assert _same(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]) and runs[0][2] == runs[1][2]
    boxes, labels, _ = boxes_from_instances_device(torch.from_numpy(np.stack(segs)).to(DEV), [(1, np.inf)])
    for n in range(4):
        hb, hl = DS.boxes_from_instances(segs[n], [(1, np.inf)])
        assert _same(boxes[n], hb.numpy()) and torch.equal(labels[n].cpu(), hl)


def test_instance_boxes_on_an_odd_volume_take_the_unaligned_path():
    rs = np.random.RandomState(3)
    seg = np.zeros((7, 9, 11), np.int16)  # 693 voxels: not a multiple of eight
    for v in (4, 9, 300, 32767):
        at = [rs.randint(0, n - 3) for n in seg.shape]
        seg[at[0]:at[0] + 3, at[1]:at[1] + 2, at[2]:at[2] + 3] = v
    seg[-1, -1, -3:] = 77  # in the tail chunk, flat
    seg[-2:, -2:, -2:] = 78
    gb, gl, off, flag = _device_boxes([seg, seg[::-1].copy()], [(1, 100), (100, INF)], 32)
    assert flag == 0
    for n, s in enumerate((seg, seg[::-1])):
        hb, hl = DS.boxes_from_instances(s, [(1, 100), (100, np.inf)])
        assert _same(gb[off[n]:off[n + 1]], hb.numpy()) and torch.equal(gl[off[n]:off[n + 1]], hl)


def test_instance_boxes_overflow_and_bad_values():
    seg = GOLD["random_0__seg"]
    n_boxes = len(GOLD["random_0__labels"])
    assert n_boxes >= 4
    gb, gl, off, flag = _device_boxes([seg, seg], [(1, INF)], n_boxes + 2)
    assert flag & 1 and off == [0, n_boxes, n_boxes + 2] and max(off) <= n_boxes + 2
    assert _same(gb[:n_boxes], GOLD["random_0__boxes"]) and _same(gb[n_boxes:], GOLD["random_0__boxes"][:2])
    gb, gl, off, flag = _device_boxes([seg, seg], [(1, INF)], 0)
    assert flag & 1 and off == [0, 0, 0]
    with pytest.raises(_lib.HipKernelError, match="msl_instance_boxes: a batch holds more ground-truth boxes than the "
                                                  "capacity of 2 rows"):
        boxes_from_instances_device(torch.from_numpy(seg[None]).to(DEV), [(1, np.inf)], capacity=2)
    bad = seg.copy()
    bad[0, 0, 0] = -3
    assert _device_boxes([bad], [(1, INF)], 64)[3] & 4
    with pytest.raises(_lib.HipKernelError, match="msl_instance_boxes: a mask holds a negative value"):
        boxes_from_instances_device(torch.from_numpy(bad[None]).to(DEV), [(1, np.inf)], capacity=64)
    out = _InstBoxOut(1, seg.shape, [(1, INF)], 8, DEV)
    t = torch.from_numpy(seg[None]).to(DEV)
    for args in ((0, *seg.shape, out.thr.ctypes.data, 1), (1, *seg.shape, out.thr.ctypes.data, 9),
                 (1, *seg.shape, out.thr.ctypes.data, 0)):
        with pytest.raises(_lib.HipKernelError):
            _lib.call("msl_instance_boxes", t.data_ptr(), *args, 8, out.ws.data_ptr(), out.ws.numel(), out.gb.data_ptr(),
                      out.gl.data_ptr(), out.obj_off.data_ptr(), out.flag.data_ptr(), _stream())
    with pytest.raises(_lib.HipKernelError):  # workspace too small
        _lib.call("msl_instance_boxes", t.data_ptr(), 1, *seg.shape, out.thr.ctypes.data, 1, 8, out.ws.data_ptr(), 1024,
                  out.gb.data_ptr(), out.gl.data_ptr(), out.obj_off.data_ptr(), out.flag.data_ptr(), _stream())


# ---- msl_augment_fit ---------------------------------------------------------------------------------------------------
CASE_SHAPES = [(30, 52, 41), (50, 40, 70), (44, 66, 60), (37, 37, 64)]
ROT = {"rotate_range": ((0.2, 0.5), (-0.5, -0.2), (0.2, 0.5)), "scale_range": (0.2, 0.2, 0.2)}


class _Arena:
    def __init__(self, shapes=CASE_SHAPES, seed=0):
        rs = np.random.RandomState(seed)
        self.shapes = list(shapes)
        self.img = [rs.randn(*s).astype(np.float32) for s in shapes]
        self.seg = [((rs.rand(*s) < 0.3) * rs.randint(1, 3000, s)).astype(np.int16) for s in shapes]
        off = np.concatenate([[0], np.cumsum([int(np.prod(s)) for s in shapes])])
        self.d_img = torch.from_numpy(np.concatenate([v.reshape(-1) for v in self.img])).to(DEV)
        self.d_seg = torch.from_numpy(np.concatenate([v.reshape(-1) for v in self.seg])).to(DEV)
        self.table = torch.tensor([[int(off[k]), *shapes[k]] for k in range(len(shapes))], dtype=torch.int64, device=DEV)

    def launch(self, rows, target, table=None):
        rows = np.asarray(rows, dtype=np.float64)
        N, V = rows.shape[0], int(np.prod(target))
        assert rows.shape == (N, AFFINE_STRIDE)
        p = torch.from_numpy(rows).to(DEV)
        bi = torch.full((N * V + 2 * GUARD,), IMG_PATTERN, dtype=torch.int32, device=DEV)
        bs = torch.full((N * V + 2 * GUARD,), SEG_PATTERN, dtype=torch.int16, device=DEV)
        oi, os_ = bi[GUARD:GUARD + N * V], bs[GUARD:GUARD + N * V]
        table = self.table if table is None else table
        _lib.call("msl_augment_fit", self.d_img.data_ptr(), self.d_seg.data_ptr(), self.d_img.numel(), table.data_ptr(),
                  table.shape[0], p.data_ptr(), N, *target, oi.data_ptr(), os_.data_ptr(), _stream())
        hi, hs = bi.cpu(), bs.cpu()
        for band in (hi[:GUARD], hi[GUARD + N * V:]):
            assert bool((band == IMG_PATTERN).all()), "image guard band overwritten"
        for band in (hs[:GUARD], hs[GUARD + N * V:]):
            assert bool((band == SEG_PATTERN).all()), "mask guard band overwritten"
        return (hi[GUARD:GUARD + N * V].view(torch.float32).reshape((N,) + tuple(target)).numpy(),
                hs[GUARD:GUARD + N * V].reshape((N,) + tuple(target)).numpy())


def _host_sample(arena, case, augs, seed, target):
    """Host steps 3-4 on a cached case -> (image, mask, share of padded output voxels, affine share outside)."""
    x, m = arena.img[case][None], arena.seg[case][None]
    rs = np.random.RandomState(seed)
    for name, kw in augs:
        x, m = DS.AUGMENTATIONS[name](x, m, rs, **kw)
    shape = x.shape[1:]
    inside = np.ones(target, bool)
    for a in range(3):
        o = np.arange(target[a]) + DS.fit_shift(shape[a], target[a])
        sel = [None] * 3
        sel[a] = slice(None)
        inside &= ((o >= 0) & (o < shape[a]))[tuple(sel)]
    perm, stages = sample_params(DS.draw_augmentations(augs, np.random.RandomState(seed)), arena.shapes[case], augs,
                                 ragged=True)
    outside = 0.0
    geo = [st for st in stages if hasattr(st, "matrix")]
    if geo:
        o = np.stack(np.meshgrid(*(np.arange(n) for n in shape), indexing="ij"), -1).astype(np.float64)
        c = o @ np.asarray(geo[0].matrix).T + np.asarray(geo[0].offset)
        outside = float(((c < 0) | (c > np.array(shape) - 1)).any(-1).mean())
    return (DS.resize_with_pad_or_crop(x, target)[0], DS.resize_with_pad_or_crop(m, target)[0], 1.0 - inside.mean(),
            outside, (perm, stages), shape)


def _variants():
    p1 = {"prob": 1.0}
    rot = [("rotate90", dict(spatial_axes=ax, **p1)) for ax in ((1, 2), (0, 1), (0, 2))]
    inten = [("shiftintensity", {"offsets": 0.1, "prob": 1.0}), ("scaleintensity", {"factors": 0.1, "prob": 1.0})]
    out = {"identity": [], "flip": [("flip", {"spatial_axis": (0, 2), "prob": 1.0})], "rot90": rot,
           "intensity": inten}
    for pad in ("reflection", "border", "zeros"):
        out[f"affine_{pad}"] = [("affine", dict(ROT, padding_mode=pad, **p1))]
    out["recipe"] = [("flip", {"spatial_axis": (0, 1, 2), "prob": 1.0})] + rot + \
        [("affine", dict(ROT, padding_mode="border", **p1))] + inten
    return out


@pytest.mark.parametrize("target", [(40, 48, 64), (33, 70, 45)])  # vector stores / a last axis that is not 4-aligned
@pytest.mark.parametrize("variant", list(_variants()))
def test_augment_fit_equals_the_host_steps(variant, target):
    arena = _Arena()
    augs = _variants()[variant]
    cases = [0, 1, 2, 3, 2, 0]  # four shapes in one batch
    host = [_host_sample(arena, c, augs, 10 + n, target) for n, c in enumerate(cases)]
    oi, os_ = arena.launch(fit_rows(cases, [h[4] for h in host]), target)
    for n, h in enumerate(host):
        assert _same(os_[n], h[1]), (variant, n)
        assert _same(oi[n], h[0]), (variant, n)
    # the draws exercise the fit: at least 10 % of the output voxels lie in the padded region, and under the affine at
    # least 5 % of the (cropped-shape) output voxels sample outside the source
    assert np.mean([h[2] for h in host]) >= 0.10, [h[2] for h in host]
    if "affine" in variant or variant == "recipe":
        assert min(h[3] for h in host) >= 0.05
    if variant in ("rot90", "recipe"):
        assert any(h[5] != arena.shapes[c] for h, c in zip(host, cases))  # a rot90 changed the shape


def test_augment_fit_refuses_what_it_cannot_read():
    arena = _Arena(CASE_SHAPES[:2])
    ident = (([0, 1, 2], [0, 0, 0]), [])
    rows = fit_rows([0, 2, -1, 1, 1], [ident] * 5)
    rows[3, 1:4] = (0, 0, 1)  # not a permutation
    oi, os_ = arena.launch(rows, (16, 16, 16))
    assert not oi[1:4].any() and not os_[1:4].any() and oi[0].any() and oi[4].any()
    bad = arena.table.clone()
    bad[1, 0] = arena.d_img.numel() - 5  # the case would end past the arena
    oi, os_ = arena.launch(rows[[0, 4]], (16, 16, 16), bad)
    assert oi[0].any() and not oi[1].any() and not os_[1].any()
    with pytest.raises(_lib.HipKernelError):
        _lib.call("msl_augment_fit", arena.d_img.data_ptr(), arena.d_seg.data_ptr(), arena.d_img.numel(),
                  arena.table.data_ptr(), 2, arena.table.data_ptr(), 0, 16, 16, 16, arena.d_img.data_ptr(),
                  arena.d_seg.data_ptr(), _stream())


# ---- end to end --------------------------------------------------------------------------------------------------------
SHAPES = [(40, 44, 50), (52, 48, 46), (44, 70, 52), (60, 50, 72), (48, 64, 64), (42, 42, 42), (50, 45, 58),
          (46, 66, 49), (41, 51, 61), (55, 47, 43)]
TARGET = (48, 64, 64)


def _module(tmp_path, augmentations, batch=2):
    data_dir = lesion_tree.make_tree(tmp_path, SHAPES) if not os.path.exists(tmp_path / "raw") else str(tmp_path / "raw")
    dm = DS.LesionsDataModule(data_dir=data_dir, centers=lesion_tree.CENTERS, batch_size=batch, spatial_size=TARGET,
                              augmentations=augmentations)
    dm.setup("fit")
    return dm


def test_cache_holds_the_cropped_normalised_cases(tmp_path):
    dm = _module(tmp_path, None)
    cache = LesionCache(dm, DEV)
    assert len(set(cache.shapes)) >= 3 and "MiB" in cache.footprint()
    assert cache.nbytes() >= 6 * sum(int(np.prod(s)) for s in cache.shapes)
    tr = dm.train_dataset
    for i in range(len(tr)):
        img, seg = tr.load(i)
        ci, cs = DS.crop_foreground(img, seg, 5)
        di, dseg = cache.case(cache.slot[tr.subjects[i]])
        assert tuple(di.shape) == ci.shape and ci.shape != img.shape
        assert np.array_equal(dseg.cpu().numpy(), cs)
        np.testing.assert_allclose(di.cpu().numpy(), DS.normalize_nonzero(ci), rtol=NORM_RTOL, atol=NORM_ATOL)


def test_cache_refuses_what_it_cannot_hold(tmp_path):
    dm = _module(tmp_path, None)
    c, s = dm.train_dataset.subjects[0]
    path = dm._get_sequence(c, s, dm.segmentation) + ".npy"
    seg = np.load(path)
    np.save(path, seg.astype(np.float32) + 0.5 * (seg > 0))
    with pytest.raises(ValueError, match="integer-valued"):
        LesionCache(dm, DEV)
    np.save(path, seg)
    two = DS.select_augmentations(["translate", "scale"])
    with pytest.raises(NotImplementedError, match="two affine stages"):
        LesionCache(_module(tmp_path, two), DEV)


def _snapshot(b):
    return {"img": b["img"].cpu(), "seg": b["seg"].cpu(), "gb": b["gb"].cpu(), "gl": b["gl"].cpu(),
            "obj_off": b["obj_off"].cpu(), "subject": list(b["subject"])}


def test_train_batches_equal_the_host_loader(tmp_path):
    augs = DS.select_augmentations(LESIONS)
    augs = [(n, dict(kw, prob=0.6) if n == "affine" else kw) for n, kw in augs]  # the affine drawn often
    dm = _module(tmp_path, augs)
    cache = LesionCache(dm, DEV)
    tr = dm.train_dataset
    drawn, boxes_seen = {}, 0
    for epoch in (0, 1):
        dm.set_epoch(epoch)
        host = list(dm.train_dataloader())
        dev = [_snapshot(b) for b in cache.train_batches(epoch)]
        assert [d["subject"] for d in dev] == [h["subject"] for h in host]
        for d, h in zip(dev, host):
            off = d["obj_off"].tolist()
            assert off[0] == 0 and len(off) == len(d["subject"]) + 1
            for n, s in enumerate(d["subject"]):
                ci, cs = cache.case(cache.slot[s])
                x, m = ci.cpu().numpy()[None], cs.cpu().numpy()[None]
                rs = DS.sample_rng(tr.seed, epoch, s)
                for (name, kw), (_, dr) in zip(augs, DS.draw_augmentations(augs, DS.sample_rng(tr.seed, epoch, s))):
                    x, m = DS.AUGMENTATIONS[name](x, m, rs, **kw)
                    drawn[name] = drawn.get(name, 0) + (dr is not None)
                x, m = DS.resize_with_pad_or_crop(x, TARGET)[0], DS.resize_with_pad_or_crop(m, TARGET)[0]
                assert _same(d["seg"][n], m), (epoch, s)
                assert _same(d["img"][n, 0], x), (epoch, s)
                # the host LOADER's targets for the same case, bit for bit; its image within the normalisation bound
                assert _same(d["gb"][off[n]:off[n + 1]], h["boxes"][n]), (epoch, s)
                assert torch.equal(d["gl"][off[n]:off[n + 1]], h["labels"][n])
                boxes_seen += off[n + 1] - off[n]
            np.testing.assert_allclose(d["img"].numpy(), h["img"].numpy(), rtol=NORM_RTOL, atol=NORM_ATOL)
    assert drawn["affine"] >= 4 and drawn["rotate90"] >= 4 and drawn["flip"] >= 2 and boxes_seen >= 16
    runs = [[_snapshot(b) for b in cache.train_batches(1)] for _ in range(2)]
    for a, b in zip(*runs):
        assert all(_same(a[k], b[k]) for k in ("img", "seg", "gb", "gl", "obj_off"))
    val_d, val_h = list(cache.val_batches()), list(dm.test_dataloader())
    assert [d["subject"] for d in val_d] == [h["subject"] for h in val_h]
    for d, h in zip(val_d, val_h):
        np.testing.assert_allclose(d["img"].cpu().numpy(), h["img"].numpy(), rtol=NORM_RTOL, atol=NORM_ATOL)
        for n in range(len(d["subject"])):
            assert _same(d["boxes"][n], h["boxes"][n]) and torch.equal(d["labels"][n].cpu(), h["labels"][n])


def _recorded(work):
    _lib.start_recording()
    try:
        work()
    finally:
        prog = _lib.stop_recording()
    return [fn.__name__ for fn, _, _ in prog if fn is not None]


def test_one_sequence_takes_the_entry_points_of_every_channel_count(tmp_path):
    """One sequence is C = 1 of the calls C > 1 makes: the build's foreground box and the batch's fit of a one-sequence
    ``LesionCache`` and ``LesionPredictFeed`` go through msl_foreground_box_mc / msl_augment_fit_mc (the values are
    test_train_batches_equal_the_host_loader's and test_predict_entry_point_on_lesion_cases' to prove)."""
    dm = _module(tmp_path, None)
    assert len(dm.input_images) == 1

    def train():
        next(iter(LesionCache(dm, DEV).train_batches(0)))

    def predict():
        next(iter(LesionPredictFeed(dm, DEV).batches([0])))

    for work in (train, predict):
        names = _recorded(work)
        torch.cuda.synchronize()
        assert "msl_foreground_box_mc" in names and "msl_augment_fit_mc" in names, names
        assert "msl_foreground_box" not in names and "msl_augment_fit" not in names, names


def _run_train(tmp_path, cache):
    from mslesions3d_amd import train as T
    args = T.build_parser().parse_args(["-dm", "lesions", "-d", str(tmp_path / "raw"), "--centers", *lesion_tree.CENTERS,
                                        "--spatial_size", *map(str, TARGET), "-b", "2", "-me", "2",
                                        "-ld", str(tmp_path / "logs"), "-en", f"c{cache}", "-c", str(cache), "-a", *LESIONS])
    T.example(args)
    return [json.loads(l) for l in open(tmp_path / "logs" / f"c{cache}" / "metrics.jsonl")]


def test_train_entry_point_on_lesion_cases(tmp_path):
    lesion_tree.make_tree(tmp_path, SHAPES)
    host = _run_train(tmp_path, 0)
    dev = _run_train(tmp_path, 1)
    assert [sorted(r) for r in host] == [sorted(r) for r in dev]
    train = [r["total_loss/training"] for r in dev if "total_loss/training" in r]
    val = [r["avg_val_loss"] for r in dev if "avg_val_loss" in r]
    assert len(train) == 8 and len(val) == 2 and np.isfinite(train).all() and np.isfinite(val).all()
    # epoch 0 only differs by the normalisation bound of the inputs: the losses agree to 1e-3 relative, the tolerance
    # tests/test_gpu_datapipe.py holds DeviceCache to
    for h, d in zip(host, dev):
        for key in ("total_loss/training", "avg_val_loss"):
            if h["epoch"] == 0 and key in h:
                print(key, h[key], d[key])
                assert abs(h[key] - d[key]) <= 1e-3 * abs(h[key])


def test_predict_entry_point_on_lesion_cases(tmp_path):
    from mslesions3d_amd import predict as P
    lesion_tree.make_tree(tmp_path, SHAPES)
    _run_train(tmp_path, 1)
    args = P.build_parser().parse_args(["-dm", "lesions", "-d", str(tmp_path / "raw"), "--centers", *lesion_tree.CENTERS,
                                        "--spatial_size", *map(str, TARGET), "-m", str(tmp_path / "logs" / "c1" / "last.ckpt"),
                                        "-ps", "test", "-o", str(tmp_path / "preds"), "-sc", "0.01"])
    metrics = P.predict_example(args)
    assert len(metrics["0.5"]) == 2
    for subj in metrics["0.5"]:
        assert os.path.exists(tmp_path / "preds" / f"sub-{subj}_preds.json") and "_CENTER_" in subj
