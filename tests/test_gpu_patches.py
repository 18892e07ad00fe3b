"""Patch training on the device: msl_augment_window_mc (csrc/datapipe.hip) through the C ABI
against datasets.window on the host steps, its routing through devicedata.LesionCache in patch mode and the entry points.
The arena, the variants and the seeds are tests/test_gpu_lesions(_mc).py's.  Comparisons are bit for bit, images
included: in patch mode the host normalises with the kernel's arithmetic (datasets.normalize_nonzero_device)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from mslesions3d_amd import _lib
from mslesions3d_amd import datasets as DS
from mslesions3d_amd.devicedata import AFFINE_STRIDE, LesionCache, fit_rows, sample_params
from tests import lesion_tree, lesion_tree_mc
from tests.test_gpu_lesions import CASE_SHAPES, GUARD, IMG_PATTERN, SEG_PATTERN, SHAPES, _same, _snapshot, _variants
from tests.test_gpu_lesions_mc import CASES, TWO, _Arena, _data

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
PATCHES = [(24, 32, 32), (17, 30, 21)]  # vector stores / the scalar tail path
PATCH = (32, 32, 32)
LESIONS = ["flip", "rotate90", "affine", "shiftintensity", "scaleintensity"]


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- msl_augment_window_mc ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _augmented(variant):
    """Host step 3 on the three-channel cases of the batch -> per sample (image (3,) + n', mask (1,) + n', (perm,
    stages)).  Read-only; shared by every patch and channel count."""
    img, seg = _data()
    augs = _variants()[variant]
    out = []
    for n, case in enumerate(CASES):
        x, m = img[case], seg[case][None]
        rs = np.random.RandomState(10 + n)
        for name, kw in augs:
            x, m = DS.AUGMENTATIONS[name](x, m, rs, **kw)
        x, m = np.ascontiguousarray(x), np.ascontiguousarray(m)
        x.setflags(write=False)
        m.setflags(write=False)
        out.append((x, m, sample_params(DS.draw_augmentations(augs, np.random.RandomState(10 + n)), CASE_SHAPES[case],
                                        augs, ragged=True)))
    return out


def _origins(shapes, patch):
    """Per sample of the batch an origin in its augmented frame: interior at an odd offset (as far as the case is large
    enough), negative, overhanging, in turn."""
    out = []
    for n, shape in enumerate(shapes):
        if n % 3 == 0:
            out.append(tuple(max(0, min(2 * a + 1, shape[a] - patch[a])) for a in range(3)))
        elif n % 3 == 1:
            out.append((-5, -7, -9))
        else:
            out.append(tuple(shape[a] - patch[a] + 6 + a for a in range(3)))
    return out


def _shares(shapes, origins, patch):
    """-> (share of the batch's output voxels that read a replicated border voxel, share that lie inside the case)."""
    inside = []
    for shape, o in zip(shapes, origins):
        ok = np.ones(patch, bool)
        for a in range(3):
            q = np.arange(patch[a]) + o[a]
            sel = [None] * 3
            sel[a] = slice(None)
            ok &= ((q >= 0) & (q < shape[a]))[tuple(sel)]
        inside.append(ok.mean())
    return 1.0 - float(np.mean(inside)), float(np.mean(inside))


def _launch(arena, rows, windows, patch, fn="msl_augment_window_mc"):
    """One launch into pattern-filled buffers with guard bands -> (rc, image (N, C) + patch, mask (N,) + patch, raw
    image words, raw mask words)."""
    rows = np.asarray(rows, dtype=np.float64)
    C, N, V = arena.C, rows.shape[0], int(np.prod(patch))
    assert rows.shape == (N, AFFINE_STRIDE)
    p = torch.from_numpy(rows).to(DEV)
    w = None if windows is None else torch.from_numpy(np.asarray(windows, dtype=np.int32).reshape(N, 3)).to(DEV)
    bi = torch.full((N * C * V + 2 * GUARD,), IMG_PATTERN, dtype=torch.int32, device=DEV)
    bs = torch.full((N * V + 2 * GUARD,), SEG_PATTERN, dtype=torch.int16, device=DEV)
    oi, os_ = bi[GUARD:GUARD + N * C * V], bs[GUARD:GUARD + N * V]
    args = [arena.d_img.data_ptr(), arena.d_seg.data_ptr(), arena.d_seg.numel(), C, arena.table.data_ptr(),
            arena.table.shape[0], p.data_ptr()]
    if fn == "msl_augment_window_mc":
        args.append(None if w is None else w.data_ptr())
    rc = getattr(_lib.load(), fn)(*args, N, *patch, oi.data_ptr(), os_.data_ptr(), _stream())
    hi, hs = bi.cpu(), bs.cpu()
    for band in (hi[:GUARD], hi[GUARD + N * C * V:]):
        assert bool((band == IMG_PATTERN).all()), "image guard band overwritten"
    for band in (hs[:GUARD], hs[GUARD + N * V:]):
        assert bool((band == SEG_PATTERN).all()), "mask guard band overwritten"
    return (rc, hi[GUARD:GUARD + N * C * V].view(torch.float32).reshape((N, C) + tuple(patch)).numpy(),
            hs[GUARD:GUARD + N * V].reshape((N,) + tuple(patch)).numpy(), hi[GUARD:GUARD + N * C * V], hs[GUARD:GUARD + N * V])


@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("patch", PATCHES)
@pytest.mark.parametrize("variant", list(_variants()))
def test_augment_window_mc_equals_the_host_steps(variant, patch, C):
    host = _augmented(variant)
    shapes = [h[0].shape[1:] for h in host]
    origins = _origins(shapes, patch)
    replicated, interior = _shares(shapes, origins, patch)
    print(f"{variant} {patch}: replicated {replicated:.3f} interior {interior:.3f}")
    assert replicated >= 0.10 and interior >= 0.30, (replicated, interior)
    assert any(min(o) < 0 for o in origins) and any(o[2] % 2 == 1 and o[2] > 0 for o in origins)
    rc, oi, os_, _, _ = _launch(_Arena(C), fit_rows(CASES, [h[2] for h in host]), origins, patch)
    assert rc == 0
    for n, (x, m, _) in enumerate(host):
        assert _same(os_[n], DS.window(m, origins[n], patch)[0]), (variant, n)
        want = DS.window(x[:C], origins[n], patch)
        for c in range(C):
            assert _same(oi[n, c], want[c]), (variant, n, c)


@pytest.mark.parametrize("patch", PATCHES)
def test_window_at_the_fit_shifts_is_msl_augment_fit_mc(patch):
    host = _augmented("recipe")
    rows = fit_rows(CASES, [h[2] for h in host])
    shifts = [[DS.fit_shift(n, t) for n, t in zip(h[0].shape[1:], patch)] for h in host]
    arena = _Arena(2)
    rc, oi, os_, _, _ = _launch(arena, rows, shifts, patch)
    rc_fit, fi, fs, _, _ = _launch(arena, rows, None, patch, fn="msl_augment_fit_mc")
    assert rc == 0 and rc_fit == 0 and _same(oi, fi) and _same(os_, fs) and oi.any() and os_.any()
    ident = (([0, 1, 2], [0, 0, 0]), [])  # the interior load path against the fit's voxel-by-voxel walk
    rows = fit_rows(CASES, [ident] * len(CASES))
    shifts = [[DS.fit_shift(n, t) for n, t in zip(CASE_SHAPES[c], patch)] for c in CASES]
    rc, oi, os_, _, _ = _launch(arena, rows, shifts, patch)
    rc_fit, fi, fs, _, _ = _launch(arena, rows, None, patch, fn="msl_augment_fit_mc")
    assert rc == 0 and rc_fit == 0 and _same(oi, fi) and _same(os_, fs)


def test_window_refuses_null_windows_and_zeroes_invalid_rows():
    arena = _Arena(2)
    ident = (([0, 1, 2], [0, 0, 0]), [])
    rows = fit_rows([0, 9, -1, 1], [ident] * 4)
    rc, _, _, raw_i, raw_s = _launch(arena, rows, None, (16, 16, 16))
    assert rc == -1  # nothing launched: the outputs still hold their patterns (the guard bands are checked in _launch)
    assert bool((raw_i == IMG_PATTERN).all()) and bool((raw_s == SEG_PATTERN).all())
    far = [[0, 0, 0], [1, 1, 1], [2, 2, 2], [-2 ** 31, 2 ** 31 - 1, 7]]  # any int is an origin
    rc, oi, os_, _, _ = _launch(arena, rows, far, (16, 16, 16))
    assert rc == 0 and oi[0].any() and not oi[1:3].any() and not os_[1:3].any()
    img, seg = _data()
    assert _same(oi[3], DS.window(img[1][:2], far[3], (16, 16, 16))) and _same(os_[3], DS.window(seg[1], far[3], (16, 16, 16)))
    with pytest.raises(_lib.HipKernelError):
        w = torch.zeros(3, dtype=torch.int32, device=DEV)
        _lib.call("msl_augment_window_mc", arena.d_img.data_ptr(), arena.d_seg.data_ptr(), arena.d_seg.numel(), 5,
                  arena.table.data_ptr(), 4, arena.table.data_ptr(), w.data_ptr(), 1, 16, 16, 16, arena.d_img.data_ptr(),
                  arena.d_seg.data_ptr(), _stream())


# ---- the host twin of msl_normalize_nonzero ----------------------------------------------------------------------------
def test_normalize_nonzero_device_equals_the_kernel():
    rs = np.random.RandomState(4)
    for shape in ((13, 17, 19), (3, 5, 7), (40, 64, 64), (51, 63, 67)):
        vols = np.stack([(rs.rand(*shape) * s + 1).astype(np.float32) * (rs.rand(*shape) < 0.8) for s in (100.0, 1.0)])
        vols[0].flat[3] = -2.0
        d = torch.from_numpy(vols).to(DEV)
        _lib.call("msl_normalize_nonzero", d.data_ptr(), 2, int(np.prod(shape)), _stream())
        for c in range(2):
            assert _same(d[c], DS.normalize_nonzero_device(vols[c])), (shape, c)


# ---- LesionCache in patch mode -----------------------------------------------------------------------------------------
def _module(tmp_path, augmentations, input_images, batch=2):
    make = lesion_tree.make_tree if len(input_images) == 1 else lesion_tree_mc.make_tree
    data_dir = make(tmp_path, SHAPES) if not os.path.exists(tmp_path / "raw") else str(tmp_path / "raw")
    dm = DS.LesionsDataModule(data_dir=data_dir, centers=lesion_tree.CENTERS, batch_size=batch, augmentations=augmentations,
                              input_images=input_images, patch_size=PATCH, patch_foreground=0.7, tile_margin=(4, 4, 6))
    dm.setup("fit")
    return dm


@pytest.mark.parametrize("input_images", [("FLAIR",), TWO], ids=["C1", "C2"])
def test_patch_batches_equal_the_host_loader(tmp_path, input_images):
    C = len(input_images)
    augs = DS.select_augmentations(LESIONS)
    augs = [(n, dict(kw, prob=0.6) if n == "affine" else kw) for n, kw in augs]  # the affine drawn often
    dm = _module(tmp_path, augs, input_images)
    cache = LesionCache(dm, DEV)
    assert str(PATCH) in cache.footprint() and cache.target == PATCH
    tr = dm.train_dataset
    for i in range(len(tr)):  # the centres the device recovered are the host's, and so is the normalised case
        img, seg = DS.crop_foreground(*tr.load(i), 5)
        assert np.array_equal(cache.centres[cache.slot[tr.subjects[i]]], DS.lesion_centres(seg, dm.thresholds))
        want = np.stack([DS.normalize_nonzero_device(ch) for ch in img.reshape((C,) + seg.shape)])
        assert _same(cache.case(cache.slot[tr.subjects[i]])[0].reshape(want.shape), want)
    boxes_seen, negative = 0, 0
    for epoch in (0, 1, 2):
        dm.set_epoch(epoch)
        host = list(dm.train_dataloader())
        dev = [dict(_snapshot(b), patch_origin=list(b["patch_origin"])) for b in cache.train_batches(epoch)]
        assert [d["subject"] for d in dev] == [h["subject"] for h in host]
        for d, h in zip(dev, host):
            off = d["obj_off"].tolist()
            assert off[0] == 0 and len(off) == len(d["subject"]) + 1
            assert d["patch_origin"] == h["patch_origin"] and tuple(d["img"].shape[1:]) == (C,) + PATCH
            for n, s in enumerate(d["subject"]):
                ci, cs = cache.case(cache.slot[s])
                x, m = ci.cpu().numpy().reshape((C,) + tuple(cs.shape)), cs.cpu().numpy()[None]
                rs = DS.sample_rng(tr.seed, epoch, s)
                for name, kw in augs:
                    x, m = DS.AUGMENTATIONS[name](x, m, rs, **kw)
                origin = d["patch_origin"][n]
                negative += min(origin) < 0
                assert _same(d["seg"][n], DS.window(m, origin, PATCH)[0]), (epoch, s)
                assert _same(d["img"][n], DS.window(x, origin, PATCH)), (epoch, s)
                assert _same(d["gb"][off[n]:off[n + 1]], h["boxes"][n]), (epoch, s)
                assert torch.equal(d["gl"][off[n]:off[n + 1]], h["labels"][n])
                boxes_seen += off[n + 1] - off[n]
            assert _same(d["img"], h["img"])  # the host loader's batch, bit for bit
    assert boxes_seen >= 16
    val_d, val_h = list(cache.val_batches()), list(dm.test_dataloader())
    assert len(val_d) == len(val_h) > 2
    for d, h in zip(val_d, val_h):
        assert d["subject"] == h["subject"] and d["patch_origin"] == h["patch_origin"]
        assert d["crop_shape"] == h["crop_shape"] and list(d["crop_origin"]) == list(h["crop_origin"])
        assert _same(d["img"], h["img"])
        for n, s in enumerate(d["subject"]):
            ci, _ = cache.case(cache.slot[s])
            x = ci.cpu().numpy().reshape((C,) + tuple(ci.shape[-3:]))
            assert _same(d["img"][n], DS.window(x, d["patch_origin"][n], PATCH))
            assert _same(d["boxes"][n], h["boxes"][n]) and torch.equal(d["labels"][n].cpu(), h["labels"][n])


# ---- the entry points ----------------------------------------------------------------------------------------------------
def _run_train(root, cache):
    from mslesions3d_amd import train as T
    args = T.build_parser().parse_args(["-dm", "lesions", "-d", str(root / "raw"), "--centers", *lesion_tree.CENTERS,
                                        "--patch_size", *map(str, PATCH), "-b", "2", "-me", "2", "-ld", str(root / "logs"),
                                        "-en", f"c{cache}", "-c", str(cache), "-a", *LESIONS,
                                        # a 32^3 input has 146 priors on the default layers, and the training metrics
                                        # refuse fewer than 501 (trainer.step, as the reference): a fourth, finer scale
                                        "-pl", "1 3 5 7"])
    T.example(args)
    return [l.rstrip("\n") for l in open(root / "logs" / f"c{cache}" / "metrics.jsonl")]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    root = tmp_path_factory.mktemp("patch_runs")
    lesion_tree.make_tree(root, SHAPES)
    return root, _run_train(root, 0), _run_train(root, 1)


def test_train_entry_point_trains_on_patches_on_both_routes(runs):
    root, host, dev = runs
    host, dev = [json.loads(l) for l in host], [json.loads(l) for l in dev]
    assert [sorted(r) for r in host] == [sorted(r) for r in dev]
    train = [r["total_loss/training"] for r in dev if "total_loss/training" in r]
    val = [r["avg_val_loss"] for r in dev if "avg_val_loss" in r]
    assert len(train) == 8 and len(val) == 2 and np.isfinite(train).all() and np.isfinite(val).all()
    from mslesions3d_amd.ssd3d import LSSD3D
    for c in (0, 1):
        model = LSSD3D.load_from_checkpoint(str(root / "logs" / f"c{c}" / "last.ckpt"))
        assert tuple(model.input_size) == PATCH


def test_both_routes_log_the_same_metrics_line_for_line(runs):
    """Both routes train on the same bits (windows, masks, boxes: test_patch_batches_equal_the_host_loader) with the same
    kernels in the same order, so the two files are equal as text."""
    _, host, dev = runs
    for h, d in zip(host, dev):
        print(h)
        print(d)
    assert host == dev


def test_predict_tiles_runs_on_a_patch_checkpoint(runs):
    from mslesions3d_amd import predict as P
    root = runs[0]
    args = P.build_parser().parse_args(["-dm", "lesions", "-d", str(root / "raw"), "--centers", *lesion_tree.CENTERS,
                                        "--spatial_size", *map(str, PATCH), "-m", str(root / "logs" / "c1" / "last.ckpt"),
                                        "-ps", "test", "-o", str(root / "preds"), "-sc", "0.01", "--views", "tiles",
                                        "--tile_margin", "4", "4", "6"])
    P.predict_example(args)
    written = sorted(os.listdir(root / "preds"))
    assert len([f for f in written if f.endswith("_preds_views.json")]) == 2, written
