"""msl_binary_boxes (csrc/datapipe.hip) through the C ABI against scipy.ndimage.label plus the host walk
(datasets.boxes_from_instances in "binary" mode) and the reference's goldens, bit for bit; then its routing through
devicedata.LesionCache, LesionPredictFeed and the training entry point on a tree of binary masks."""
import json
import os

import numpy as np
import pytest
import torch

from mslesions3d_amd import _lib
from mslesions3d_amd import datasets as DS
from mslesions3d_amd.devicedata import (LesionCache, LesionPredictFeed, _BinBoxOut, _BoxOut, _InstBoxOut,
                                        boxes_from_binary_device)
from tests import lesion_tree_binary

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NORM_RTOL, NORM_ATOL = 1e-5, 1e-5  # the image bound of tests/test_gpu_lesions.py
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "instances.npz"))
BINARY_CASES = ["binary", "binary_full", "binary_random"]
ONE = [(1, np.inf)]
GUARD = 1024
FILL = {torch.int32: 0x5A5AC3C3, torch.float32: -1.0, torch.int64: -7}
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


def _host(seg):
    b, l = DS.boxes_from_instances(seg, ONE, "binary")
    return b.numpy().reshape(-1, 6), l.numpy()


def _n_runs(segs):
    """Runs of non-zero voxels along the last axis, all images together."""
    m = np.stack(segs) != 0
    return int(m[..., 0].sum() + (m[..., 1:] & ~m[..., :-1]).sum())


class _Guarded:
    """A device buffer between two guard bands of a known pattern."""

    def __init__(self, n, dtype):
        self.n, self.fill = n, FILL[dtype]
        self.buf = torch.full((n + 2 * GUARD,), self.fill, dtype=dtype, device=DEV)
        self.view = self.buf[GUARD:GUARD + n]

    def intact(self):
        h = self.buf.cpu()
        return bool((h[:GUARD] == self.fill).all()) and bool((h[GUARD + self.n:] == self.fill).all())


def _launch(segs, capacity, run_cap=None, misalign=False):
    """One call on a list of equal-shape masks, every output and the workspace between guard bands.
    -> (gb (capacity, 6), gl, obj_off list, flag) on the host.  ``misalign``: the mask starts two bytes off a 16-byte
    boundary (the scalar-load path)."""
    lib = _lib.load()
    stack = np.stack(segs).astype(np.int16)
    N, shape = stack.shape[0], stack.shape[1:]
    run_cap = max(_n_runs(segs), 1) if run_cap is None else run_cap
    nbytes = lib.msl_binary_boxes_workspace_bytes(N, *shape, run_cap)
    assert nbytes > 0 and nbytes % 4 == 0
    holder = torch.zeros(stack.size + 16, dtype=torch.int16, device=DEV)
    seg = holder[1:1 + stack.size] if misalign else holder[:stack.size]
    seg.copy_(torch.from_numpy(stack.reshape(-1)))
    assert (seg.data_ptr() % 16 != 0) == misalign
    ws, gb, gl = _Guarded(nbytes // 4, torch.int32), _Guarded(max(capacity, 1) * 6, torch.float32), \
        _Guarded(max(capacity, 1), torch.int64)
    off, flag = _Guarded(N + 1, torch.int32), _Guarded(1, torch.int32)
    _lib.call("msl_binary_boxes", seg.data_ptr(), N, *shape, capacity, run_cap, ws.view.data_ptr(), nbytes,
              gb.view.data_ptr(), gl.view.data_ptr(), off.view.data_ptr(), flag.view.data_ptr(), _stream())
    torch.cuda.synchronize()
    for g in (ws, gb, gl, off, flag):
        assert g.intact(), "a guard band was overwritten"
    return gb.view.cpu().reshape(-1, 6), gl.view.cpu(), off.view.cpu().tolist(), int(flag.view.item())


def _check(segs, capacity=64, **kw):
    """The call's rows equal the host's, image by image; rows past the end keep the fill."""
    gb, gl, off, flag = _launch(segs, capacity, **kw)
    assert flag == 0 and off[0] == 0 and len(off) == len(segs) + 1
    for n, seg in enumerate(segs):
        hb, hl = _host(seg)
        assert off[n + 1] - off[n] == len(hl), (n, off, len(hl))
        assert _same(gb[off[n]:off[n + 1]], hb) and np.array_equal(gl[off[n]:off[n + 1]].numpy(), hl), n
    assert bool((gb[off[-1]:] == FILL[torch.float32]).all()) and bool((gl[off[-1]:] == FILL[torch.int64]).all())
    return gb, gl, off


# ---- the goldens -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BINARY_CASES)
def test_binary_boxes_match_the_reference_bit_for_bit(name):
    assert str(GOLD[f"{name}__mode"]) == "binary"
    gb, gl, off = _check([GOLD[f"{name}__seg"]])
    want_b, want_l = GOLD[f"{name}__boxes"], GOLD[f"{name}__labels"]
    assert off == [0, len(want_l)]
    assert _same(gb[:off[1]], want_b.reshape(-1, 6)) and np.array_equal(gl[:off[1]].numpy(), want_l)


def test_batch_of_four_order_and_determinism():
    gold = GOLD["binary__seg"]
    neg = gold.copy()
    neg[gold != 0] = -3          # negative values are foreground
    neg[1:4, 1:4, 1:3] = -1
    neg[2, 2, 1] = 5
    segs = [gold, np.zeros_like(gold), np.ones_like(gold), neg]
    runs = [_launch(segs, 64) for _ in range(2)]
    gb, gl, off, flag = runs[0]
    n_gold = len(GOLD["binary__labels"])
    assert flag == 0 and off[:4] == [0, n_gold, n_gold, n_gold]  # the empty and the full image yield nothing
    assert _same(gb[:n_gold], GOLD["binary__boxes"].reshape(-1, 6))
    hb, hl = _host(neg)
    assert off[4] - off[3] == len(hl) >= n_gold and _same(gb[off[3]:off[4]], hb)
    assert bool((gl[:off[4]] == 1).all())
    for a, b in zip(runs[0][:2], runs[1][:2]):
        assert _same(a, b)
    assert runs[0][2:] == runs[1][2:]
    boxes, labels, _ = boxes_from_binary_device(torch.from_numpy(np.stack(segs)).to(DEV))
    for n in range(4):
        hb, hl = _host(segs[n])
        assert _same(boxes[n], hb) and np.array_equal(labels[n].cpu().numpy(), hl)


# ---- connectivity ------------------------------------------------------------------------------------------------------
def _serpentine():
    """One voxel thick, every second row of every second plane of a 16^3 volume, joined at alternating ends."""
    seg = np.zeros((16, 16, 16), np.int16)
    for zi, z in enumerate(range(0, 16, 2)):
        for yi, y in enumerate(range(0, 16, 2)):
            seg[z, y, :] = 1
            if y + 2 < 16:
                seg[z, y + 1, 15 if yi % 2 == 0 else 0] = 1
        if z + 2 < 16:
            seg[z + 1, 14 if zi % 2 == 0 else 0, 7] = 1
    return seg


def test_connectivity_is_six_neighbour():
    from scipy.ndimage import label
    snake = _serpentine()
    assert label(snake)[1] == 1
    gb, _, off = _check([snake])
    assert off == [0, 1] and _same(gb[0], np.array([0, 0, 0, 14 / 16, 14 / 16, 15 / 16], np.float32))
    edge, corner, zjoin, yjoin = (np.zeros((16, 16, 16), np.int16) for _ in range(4))
    edge[2:4, 2:4, 2:4] = edge[4:6, 4:6, 2:4] = 1        # the cubes share an edge
    corner[2:4, 2:4, 2:4] = corner[4:6, 4:6, 4:6] = 1    # ... a corner
    zjoin[2:4, 2:4, 2:4] = zjoin[4:6, 3:5, 3:5] = 1      # joined through the z-neighbour (3, 3, 3) - (4, 3, 3) alone
    yjoin[2:4, 2:4, 2:4] = yjoin[2:4, 4:6, 3:5] = 1      # ... the y-neighbours (z, 3, 3) - (z, 4, 3) alone
    _, _, off = _check([edge, corner, zjoin, yjoin])
    assert np.diff(off).tolist() == [2, 2, 1, 1]


# ---- tails -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("misalign", [False, True], ids=["aligned", "two_bytes_off"])
def test_odd_volume_and_rows_across_the_chunks(misalign):
    rs = np.random.RandomState(3)
    a = (rs.rand(7, 9, 11) < 0.35).astype(np.int16)  # 693 voxels: not a multiple of eight, rows begin inside chunks
    b = a[::-1, :, ::-1].copy()
    b[-2:, -2:, -3:] = 1  # a component in the tail chunk of the buffer
    gb, _, off = _check([a, b], misalign=misalign)
    assert off[2] >= 4


def test_rows_longer_than_a_wave_span():
    seg = np.zeros((3, 5, 700), np.int16)
    seg[0:2, 3:5, 100:651] = 1   # runs that cross chunks and the 512-voxel span of a wave
    seg[1:3, 0:2, 690:700] = 1   # runs ending at x = W - 1 ...
    seg[1:3, 2:4, 0:10] = 1      # ... and runs starting at x = 0 of the next row: another component
    seg[0, 0, 505:520] = 1       # flat, over the span boundary
    from scipy.ndimage import label
    assert label(seg)[1] == 4
    gb, _, off = _check([seg, seg[:, ::-1].copy()])
    assert off == [0, 3, 6]
    _check([seg], misalign=True)


def test_two_cubed():
    full, one, pair = np.ones((2, 2, 2), np.int16), np.zeros((2, 2, 2), np.int16), np.ones((2, 2, 2), np.int16)
    one[1, 1, 1] = 1
    pair[0, 0, 0] = 0
    _, _, off = _check([full, one, pair])
    assert off == [0, 0, 0, 1]  # no background; one voxel is flat; seven voxels span the volume


@pytest.mark.parametrize("p", [0.02, 0.08, 0.3, 0.6, 0.95])
def test_density_sweep(p):
    rs = np.random.RandomState(int(p * 100))
    segs = [(rs.rand(20, 28, 24) < p).astype(np.int16) for _ in range(2)]
    assert all((s == 0).any() for s in segs)
    _check(segs, capacity=1024)


# ---- overflow and arguments --------------------------------------------------------------------------------------------
def test_overflow_flags_and_bounds():
    seg = GOLD["binary_random__seg"]
    n_boxes, n_runs = len(GOLD["binary_random__labels"]), _n_runs([seg])
    assert n_boxes >= 4 and n_runs > n_boxes
    gb, gl, off, flag = _launch([seg, seg], 2 * n_boxes - 1)  # (the guard bands are checked in _launch)
    assert flag == 1 and off == [0, n_boxes, 2 * n_boxes - 1]
    assert _same(gb[:n_boxes], GOLD["binary_random__boxes"].reshape(-1, 6))
    gb, gl, off, flag = _launch([seg, seg], 0)
    assert flag == 1 and off == [0, 0, 0]
    gb, gl, off, flag = _launch([seg], 64, run_cap=n_runs - 1)
    assert flag & 8 and max(off) <= 64
    assert _launch([seg], 64, run_cap=n_runs)[3] == 0
    gb, gl, off, flag = _launch([seg, seg], 64, run_cap=n_runs + 3)  # the second image does not fit
    assert flag & 8 and max(off) <= 64
    t = torch.from_numpy(seg[None]).to(DEV)
    with pytest.raises(_lib.HipKernelError, match=f"msl_binary_boxes: a batch holds more ground-truth boxes than the "
                                                  f"capacity of {n_boxes - 1} rows: raise max_objects_per_image"):
        boxes_from_binary_device(t, capacity=n_boxes - 1)
    with pytest.raises(_lib.HipKernelError, match=f"msl_binary_boxes: a batch holds more runs of lesion voxels than "
                                                  f"max_runs_per_image = {n_runs - 1} per image allows: raise "
                                                  f"max_runs_per_image"):
        boxes_from_binary_device(t, max_runs_per_image=n_runs - 1)


def test_box_stage_messages_per_flag_bit():
    """The (flag bit, message) table of every box stage, read off a flag word handed in (no launch): each message in
    full, the order in which the bits are tested (binary: the run overflow, bit 8, before the row overflow, bit 1), and
    silence on a word without the stage's bits."""
    shape, thr = (8, 8, 8), [(1, np.inf)]
    seg_out = _BoxOut(2, shape, 1, 5, 70, DEV)
    inst_out = _InstBoxOut(2, shape, thr, 5, DEV)
    bin_out = _BinBoxOut(2, shape, 5, DEV, max_runs_per_image=7)
    assert bin_out.run_cap == 14 and seg_out.comp_cap == 70 and seg_out.n_classes == 1 and len(inst_out.thr) == 1
    rows = "a batch holds more ground-truth boxes than the capacity of 5 rows"
    cases = [(seg_out, 1, f"msl_seg_boxes: {rows}$"), (seg_out, 3, f"msl_seg_boxes: {rows}$"),
             (seg_out, 2, "msl_seg_boxes: a batch holds more connected components than comp_cap = 70$"),
             (inst_out, 1, f"msl_instance_boxes: {rows}$"), (inst_out, 5, f"msl_instance_boxes: {rows}$"),
             (inst_out, 4, "msl_instance_boxes: a mask holds a negative value$"),
             (bin_out, 1, f"msl_binary_boxes: {rows}: raise max_objects_per_image$"),
             (bin_out, 8, "msl_binary_boxes: a batch holds more runs of lesion voxels than max_runs_per_image = 7 per "
                          "image allows: raise max_runs_per_image$"),
             (bin_out, 9, "msl_binary_boxes: a batch holds more runs")]
    for out, flag, message in cases:
        with pytest.raises(_lib.HipKernelError, match="^" + message):
            out.raise_on_overflow(flag)
    for out, flag in ((seg_out, 0), (seg_out, 4), (inst_out, 2), (bin_out, 6)):
        out.raise_on_overflow(flag)
    for make, message in ((lambda: _InstBoxOut(0, shape, thr, 5, DEV), "msl_instance_boxes: unsupported batch size N=0$"),
                          (lambda: _BoxOut(1, shape, 0, 5, 70, DEV),
                           r"msl_seg_boxes: unsupported sizes N=1 shape=\(8, 8, 8\) n_classes=0$"),
                          (lambda: _BinBoxOut(1, shape, 5, DEV, max_runs_per_image=0),
                           r"msl_binary_boxes: unsupported sizes N=1 shape=\(8, 8, 8\) max_runs_per_image=0$")):
        with pytest.raises(_lib.HipKernelError, match="^" + message):
            make()


def test_argument_errors_launch_nothing():
    lib = _lib.load()
    seg = torch.from_numpy(GOLD["binary__seg"][None]).to(DEV)
    shape = tuple(seg.shape[1:])
    nbytes = lib.msl_binary_boxes_workspace_bytes(1, *shape, 4096)
    ws = torch.full((nbytes // 4,), 77, dtype=torch.int32, device=DEV)
    gb = torch.full((8, 6), -1.0, device=DEV)
    gl = torch.full((8,), -7, dtype=torch.int64, device=DEV)
    off = torch.full((2,), -9, dtype=torch.int32, device=DEV)
    flag = torch.full((1,), -9, dtype=torch.int32, device=DEV)

    def call(**kw):
        a = dict(seg=seg.data_ptr(), N=1, shape=shape, capacity=8, run_cap=4096, ws=ws.data_ptr(), nbytes=nbytes,
                 gb=gb.data_ptr(), gl=gl.data_ptr(), off=off.data_ptr(), flag=flag.data_ptr())
        a.update(kw)
        return lib.msl_binary_boxes(a["seg"], a["N"], *a["shape"], a["capacity"], a["run_cap"], a["ws"], a["nbytes"],
                                    a["gb"], a["gl"], a["off"], a["flag"], _stream())

    for key in ("seg", "ws", "gb", "gl", "off", "flag"):
        assert call(**{key: None}) == -1, key
    assert call(capacity=-1) == -1 and call(nbytes=nbytes - 1) == -1 and call(N=0) == -1 and call(run_cap=0) == -1
    assert call(shape=(24, 0, 24)) == -1
    assert call(N=65536) == -2 and lib.msl_binary_boxes_workspace_bytes(65536, *shape, 4096) == 0
    assert call(run_cap=2**30) == -2 and lib.msl_binary_boxes_workspace_bytes(1, *shape, 2**30) == 0
    torch.cuda.synchronize()
    assert bool((ws == 77).all()) and bool((gb == -1.0).all()) and bool((gl == -7).all())
    assert off.tolist() == [-9, -9] and flag.item() == -9
    assert call() == 0
    torch.cuda.synchronize()
    assert flag.item() == 0 and off.tolist() == [0, len(GOLD["binary__labels"])]


def test_workspace_is_far_below_a_link_per_voxel():
    nbytes = _lib.load().msl_binary_boxes_workspace_bytes(2, 250, 300, 300, 2 * 262144)
    assert 0 < nbytes < 2 * 250 * 300 * 300 * 4 // 8


# ---- end to end --------------------------------------------------------------------------------------------------------
SHAPES = [(40, 44, 50), (52, 48, 46), (44, 60, 52), (60, 50, 62), (48, 64, 64), (42, 42, 42), (50, 45, 58), (46, 56, 49)]
TARGET = (48, 64, 64)
PATCH = (32, 32, 32)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("binary_tree")
    lesion_tree_binary.make_tree(root, SHAPES)
    return root


def _module(tree, augmentations, segmentation=lesion_tree_binary.BINARY, stage="fit", **kw):
    dm = DS.LesionsDataModule(data_dir=str(tree / "raw"), centers=lesion_tree_binary.CENTERS, spatial_size=TARGET,
                              augmentations=augmentations, segmentation=segmentation, **kw)
    dm.setup(stage)
    return dm


def _augs():
    augs = DS.select_augmentations(LESIONS)
    return [(n, dict(kw, prob=0.6) if n == "affine" else kw) for n, kw in augs]  # the affine drawn often


def _snapshot(b):
    return {k: (b[k].cpu() if torch.is_tensor(b[k]) else list(b[k])) for k in ("img", "gb", "gl", "obj_off", "subject")}


def test_cache_batches_equal_the_host_loader_on_binary_masks(tree):
    dm = _module(tree, _augs(), batch_size=2)
    inst = _module(tree, _augs(), lesion_tree_binary.INSTANCES, batch_size=2)
    assert dm.segmentation_mode == "binary" and inst.segmentation_mode == "instances"
    cache = LesionCache(dm, DEV)
    boxes_seen, differs = 0, 0
    for epoch in (0, 1):
        dm.set_epoch(epoch)
        inst.set_epoch(epoch)
        host, host_inst = list(dm.train_dataloader()), list(inst.train_dataloader())
        dev = [_snapshot(b) for b in cache.train_batches(epoch)]
        assert [d["subject"] for d in dev] == [h["subject"] for h in host] == [h["subject"] for h in host_inst]
        for d, h, hi in zip(dev, host, host_inst):
            off = d["obj_off"].tolist()
            assert off[0] == 0 and len(off) == len(d["subject"]) + 1
            for n in range(len(d["subject"])):
                assert _same(d["gb"][off[n]:off[n + 1]], h["boxes"][n]), (epoch, d["subject"][n])
                assert torch.equal(d["gl"][off[n]:off[n + 1]], h["labels"][n])
                boxes_seen += off[n + 1] - off[n]
                differs += len(hi["labels"][n]) != off[n + 1] - off[n]  # the touching pair: one box here, two there
            np.testing.assert_allclose(d["img"].numpy(), h["img"].numpy(), rtol=NORM_RTOL, atol=NORM_ATOL)
    assert boxes_seen >= 12 and differs >= 1
    box = cache._bufs[2]["box"]  # the footprint counts the binary stage's workspace
    assert "MiB" in cache.footprint() and cache.nbytes() >= cache.cache_bytes + box.ws.numel() + box.gb.numel() * 4
    val_d, val_h = list(cache.val_batches()), list(dm.test_dataloader())
    assert [d["subject"] for d in val_d] == [h["subject"] for h in val_h] and len(val_d) >= 1
    for d, h in zip(val_d, val_h):
        np.testing.assert_allclose(d["img"].cpu().numpy(), h["img"].numpy(), rtol=NORM_RTOL, atol=NORM_ATOL)
        for n in range(len(d["subject"])):
            assert _same(d["boxes"][n], h["boxes"][n]) and torch.equal(d["labels"][n].cpu(), h["labels"][n])


def test_patch_batches_equal_the_host_loader_on_binary_masks(tree):
    dm = _module(tree, _augs(), batch_size=2, patch_size=PATCH, patch_foreground=0.7, tile_margin=(4, 4, 6))
    cache = LesionCache(dm, DEV)
    tr = dm.train_dataset
    for i in range(len(tr)):
        _, seg = DS.crop_foreground(*tr.load(i), 5)
        want = DS.lesion_centres(seg, dm.thresholds, "binary")
        assert len(want) >= 1 and np.array_equal(cache.centres[cache.slot[tr.subjects[i]]], want)
    boxes_seen = 0
    for epoch in (0, 1):
        dm.set_epoch(epoch)
        host = list(dm.train_dataloader())
        dev = [dict(_snapshot(b), patch_origin=list(b["patch_origin"])) for b in cache.train_batches(epoch)]
        assert [d["subject"] for d in dev] == [h["subject"] for h in host]
        for d, h in zip(dev, host):
            off = d["obj_off"].tolist()
            assert d["patch_origin"] == h["patch_origin"] and _same(d["img"], h["img"])
            for n in range(len(d["subject"])):
                assert _same(d["gb"][off[n]:off[n + 1]], h["boxes"][n]), (epoch, d["subject"][n])
                assert torch.equal(d["gl"][off[n]:off[n + 1]], h["labels"][n])
                boxes_seen += off[n + 1] - off[n]
    assert boxes_seen >= 6
    val_d, val_h = list(cache.val_batches()), list(dm.test_dataloader())
    assert len(val_d) == len(val_h) >= 1
    for d, h in zip(val_d, val_h):
        assert d["subject"] == h["subject"] and d["patch_origin"] == h["patch_origin"] and _same(d["img"], h["img"])
        for n in range(len(d["subject"])):
            assert _same(d["boxes"][n], h["boxes"][n]) and torch.equal(d["labels"][n].cpu(), h["labels"][n])


def test_predict_feed_equals_the_host_predict_dataset_on_binary_masks(tree):
    dm = _module(tree, None, stage="predict_train", batch_size=1)
    inst = _module(tree, None, lesion_tree_binary.INSTANCES, stage="predict_train", batch_size=1)
    ds = dm.predict_dataset
    feed = LesionPredictFeed(dm, DEV)
    assert len(feed) == len(ds) >= 4
    boxes_seen, differs = 0, 0
    for i, b in enumerate(feed):
        h = DS.collate_fn([ds[i]])
        assert b["subject"] == h["subject"]
        np.testing.assert_allclose(b["img"].cpu().numpy(), h["img"].numpy(), rtol=NORM_RTOL, atol=NORM_ATOL)
        assert _same(b["boxes"][0], h["boxes"][0]) and torch.equal(b["labels"][0].cpu(), h["labels"][0])
        boxes_seen += len(h["labels"][0])
        differs += len(DS.collate_fn([inst.predict_dataset[i]])["labels"][0]) != len(h["labels"][0])
    assert boxes_seen >= 4 and differs >= 1


def _run_train(tree, logs, cache):
    from mslesions3d_amd import train as T
    args = T.build_parser().parse_args(["-dm", "lesions", "-d", str(tree / "raw"), "--centers", *lesion_tree_binary.CENTERS,
                                        "--segmentation", lesion_tree_binary.BINARY, "--spatial_size", *map(str, TARGET),
                                        "-b", "2", "-me", "1", "-ld", str(logs), "-en", f"c{cache}", "-c", str(cache),
                                        "-a", *LESIONS])
    T.example(args)
    return [json.loads(l) for l in open(logs / f"c{cache}" / "metrics.jsonl")]


def test_train_entry_point_on_binary_masks(tree, tmp_path):
    host = _run_train(tree, tmp_path / "logs", 0)
    dev = _run_train(tree, tmp_path / "logs", 1)  # (raised NotImplementedError before msl_binary_boxes)
    assert [sorted(r) for r in host] == [sorted(r) for r in dev]
    train = [(h["total_loss/training"], d["total_loss/training"]) for h, d in zip(host, dev) if "total_loss/training" in h]
    assert len(train) >= 2 and np.isfinite(train).all()
    # the two routes differ by the normalisation bound of the inputs: 1e-3 relative, the tolerance of the lesion entry-point
    # test (tests/test_gpu_lesions.py)
    for h, d in train:
        print("total_loss/training", h, d)
        assert abs(h - d) <= 1e-3 * abs(h)
