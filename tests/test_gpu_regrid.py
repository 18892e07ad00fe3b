"""msl_regrid (csrc/datapipe.hip) through the C ABI against datasets.regrid, bit for bit, and the routing of cases on
their native grid through devicedata.LesionCache, devicedata.LesionPredictFeed and the predict entry point."""
import itertools
import json
import os

import numpy as np
import pytest
import torch

from mslesions3d_amd import _lib
from mslesions3d_amd import datasets as DS
from mslesions3d_amd.devicedata import LesionCache, plan_row, regrid_device
from tests import lesion_tree, lesion_tree_native as LTN

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NORM_RTOL, NORM_ATOL = 1e-5, 1e-5  # the normalisation bound of DESIGN.md §4.7 (tests/test_gpu_lesions.py)
GUARD = 4096
LESIONS = ["flip", "rotate90", "affine", "shiftintensity", "scaleintensity"]
ALL = [(ax, rev) for ax in itertools.permutations(range(3)) for rev in itertools.product((0, 1), repeat=3)]
# identity, the three single flips, one cyclic permutation, one transposition with a flip
SIX = [((0, 1, 2), (0, 0, 0)), ((0, 1, 2), (1, 0, 0)), ((0, 1, 2), (0, 1, 0)), ((0, 1, 2), (0, 0, 1)),
       ((1, 2, 0), (0, 0, 0)), ((0, 2, 1), (0, 1, 0))]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _plan(ax, rev, step, shape, start=(0.0, 0.0, 0.0)):
    """A RegridPlan with the given map (never flagged identity: the resample always runs) and regrid_plan's shape rule."""
    nr = [shape[a] for a in ax]
    out = tuple(max(1, int(np.round((nr[k] - 1) / step[k] + 1.0))) for k in range(3))
    return DS.RegridPlan(tuple(ax), tuple(bool(r) for r in rev), tuple(float(s) for s in step), tuple(start),
                         tuple(shape), out, None, False)


def _volume(shape, seed):
    rs = np.random.RandomState(seed)
    img = rs.randn(4, *shape).astype(np.float32)
    seg = ((rs.rand(*shape) < 0.4) * rs.randint(1, 32768, shape)).astype(np.int16)
    seg.flat[rs.randint(seg.size)] = 32767
    return img, seg


def _raw(img, seg, C, n, row, m, image=True, mask=True):
    """One msl_regrid call into sentinel-filled buffers (NaN / -1) with guard bands -> (rc, image or None, mask or None);
    the bands must be intact."""
    V = int(np.prod(m))
    bi = torch.full((C * V + 2 * GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    bs = torch.full((V + 2 * GUARD,), -1, dtype=torch.int16, device=DEV)
    oi, os_ = bi[GUARD:GUARD + C * V], bs[GUARD:GUARD + V]
    di = torch.from_numpy(np.ascontiguousarray(img)).to(DEV) if image else None
    dseg = torch.from_numpy(np.ascontiguousarray(seg)).to(DEV) if mask else None
    row = np.ascontiguousarray(row, dtype=np.float64)
    rc = _lib.load().msl_regrid(_lib.ptr(di), _lib.ptr(dseg), C, *n, row.ctypes.data, *m, oi.data_ptr() if image else None,
                                os_.data_ptr() if mask else None, _stream())
    torch.cuda.synchronize()
    hi, hs = bi.cpu(), bs.cpu()
    assert bool(torch.isnan(hi[:GUARD]).all()) and bool(torch.isnan(hi[GUARD + C * V:]).all()), "image guard band overwritten"
    assert bool((hs[:GUARD] == -1).all()) and bool((hs[GUARD + V:] == -1).all()), "mask guard band overwritten"
    return rc, hi[GUARD:GUARD + C * V].reshape((C,) + tuple(m)).numpy(), hs[GUARD:GUARD + V].reshape(tuple(m)).numpy()


def _check(img, seg, plan):
    """Every launch form of one (volume, plan) against the host arrays, which are computed once."""
    want_i, want_s = DS.regrid(img, seg, plan)
    n, m, row = plan.src_shape, plan.out_shape, plan_row(plan)
    assert want_s.shape == m and (want_s != 0).any()
    for C in (1, 2, 3, 4):
        rc, oi, os_ = _raw(img[:C], seg, C, n, row, m)
        assert rc == 0
        assert not np.isnan(oi).any() and (os_ >= 0).all()  # no sentinel survives inside the destination
        assert oi.tobytes() == want_i[:C].tobytes(), (plan, C)
        assert np.array_equal(os_, want_s), (plan, C)
    for c in range(4):  # every plane against its own one-channel launch
        rc, oi, os_ = _raw(img[c:c + 1], seg, 1, n, row, m)
        assert rc == 0 and oi[0].tobytes() == want_i[c].tobytes() and np.array_equal(os_, want_s)
    rc, oi, os_ = _raw(img[:3], seg, 3, n, row, m, mask=False)  # image only: the mask buffer is not touched
    assert rc == 0 and oi.tobytes() == want_i[:3].tobytes() and (os_ == -1).all()
    rc, oi, os_ = _raw(img[:2], seg, 2, n, row, m, image=False)  # mask only
    assert rc == 0 and np.array_equal(os_, want_s) and np.isnan(oi).all()


# ---- bit equality ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(48))
def test_regrid_equals_the_host_for_every_signed_permutation(k):
    ax, rev = ALL[k]
    img, seg = _volume((5, 7, 9), k)
    _check(img, seg, _plan(ax, rev, (1.3, 0.7, 2.5), (5, 7, 9)))


# (13, 70, 67): rows of 67 / 70 / 13 outputs at step 1 (not divisible by 4: scalar stores), 134 / 75 / 8 ... at the second
# step set; (3, 4, 130) at 0.6 on the long axis: a row of 216 outputs or, permuted, rows of 3 and 4 (shorter than one
# lane's four); the last four are this file's own: 483 outputs (a lane's second pass) and 2999 (three column chunks of a
# workgroup's 1024-entry table), both with scalar stores, then rows of 484 and 1028 outputs at step 1 on the long axis:
# the 16-byte stores with a second pass and with a second column chunk
SHAPES = [((13, 70, 67), (1.0, 1.0, 1.0)), ((13, 70, 67), (0.5, 0.9375, 1.7)), ((3, 4, 130), None),
          ((3, 4, 290), None), ((2, 3, 1800), None), ((3, 4, 484), (1.0, 1.0, 1.0)), ((2, 3, 1028), (1.0, 1.0, 1.0))]


@pytest.mark.parametrize("which", range(len(SHAPES)))
@pytest.mark.parametrize("k", range(len(SIX)))
def test_regrid_equals_the_host_on_long_and_odd_rows(k, which):
    ax, rev = SIX[k]
    shape, step = SHAPES[which]
    if step is None:  # 0.6 on whichever reoriented axis the long stored axis becomes
        step = tuple(0.6 if ax[a] == 2 else 1.25 for a in range(3))
    img, seg = _volume(shape, 100 + k)
    _check(img, seg, _plan(ax, rev, step, shape))


def test_regrid_into_destinations_off_a_16_byte_boundary():
    """A row length that allows the vector stores, destinations two elements into their buffers: the scalar fallback."""
    img, seg = _volume((4, 5, 12), 11)
    plan = _plan((0, 1, 2), (0, 1, 1), (0.8, 1.3, 1.0), (4, 5, 12))
    assert plan.out_shape[2] % 4 == 0
    want_i, want_s = DS.regrid(img[:2], seg, plan)
    V = int(np.prod(plan.out_shape))
    bi = torch.full((2 * V + 64,), float("nan"), dtype=torch.float32, device=DEV)
    bs = torch.full((V + 64,), -1, dtype=torch.int16, device=DEV)
    oi, os_ = bi[2:2 + 2 * V], bs[2:2 + V]
    assert oi.data_ptr() % 16 == 8 and os_.data_ptr() % 8 == 4
    row = plan_row(plan)
    di, dseg = torch.from_numpy(img[:2].copy()).to(DEV), torch.from_numpy(seg).to(DEV)
    _lib.call("msl_regrid", di.data_ptr(), dseg.data_ptr(), 2, *plan.src_shape, row.ctypes.data, *plan.out_shape, oi.data_ptr(), os_.data_ptr(), _stream())
    hi, hs = bi.cpu(), bs.cpu()
    assert hi[2:2 + 2 * V].numpy().tobytes() == want_i.tobytes() and np.array_equal(hs[2:2 + V].numpy().reshape(want_s.shape), want_s)
    assert bool(torch.isnan(hi[:2]).all()) and bool(torch.isnan(hi[2 + 2 * V:]).all())
    assert bool((hs[:2] == -1).all()) and bool((hs[2 + V:] == -1).all())


def test_regrid_with_a_start_and_through_the_wrapper():
    img, seg = _volume((9, 10, 12), 7)
    plan = _plan((2, 0, 1), (1, 0, 1), (0.8, 1.1, 0.7), (9, 10, 12), start=(-1.5, 0.25, 2.0))  # samples past both ends
    _check(img, seg, plan)
    di, dseg = regrid_device(torch.from_numpy(img[:2]).to(DEV), torch.from_numpy(seg).to(DEV), plan)
    wi, ws = DS.regrid(img[:2], seg, plan)
    assert di.cpu().numpy().tobytes() == wi.tobytes() and np.array_equal(dseg.cpu().numpy(), ws)
    d3, _ = regrid_device(torch.from_numpy(img[0]).to(DEV), None, plan)
    assert tuple(d3.shape) == plan.out_shape and d3.cpu().numpy().tobytes() == wi[0].tobytes()
    ident = DS.regrid_plan(LTN.make_affine((0, 1, 2), (-1, -1, -1), (1.0, 1.0, 1.0)), (9, 10, 12))
    t = torch.from_numpy(img[0]).to(DEV)
    assert regrid_device(t, None, ident)[0] is t


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_regrid_refuses_bad_arguments_and_writes_nothing():
    n, m = (5, 7, 9), (6, 8, 10)
    img, seg = _volume(n, 3)
    good = np.array([0, 1, 2, 0, 0, 0, 1.0, 1.0, 1.0, 0, 0, 0], dtype=np.float64)
    assert _raw(img[:1], seg, 1, n, good, m)[0] == 0
    bad_rows = []
    for at, value in ((1, 0.0), (2, 3.0), (0, -1.0), (1, 0.5), (2, np.nan),        # ax not a permutation of 0..2
                      (3, 2.0), (4, 0.5), (5, -1.0), (3, np.nan),                   # rev not 0 / 1
                      (6, 0.0), (7, -1.0), (8, np.inf), (6, np.nan),                # step not finite or <= 0
                      (9, np.inf), (10, -np.inf), (11, np.nan)):                    # start not finite
        row = good.copy()
        row[at] = value
        bad_rows.append((1, n, row, m))
    for C in (0, 5, -1):
        bad_rows.append((C, n, good, m))
    for k in range(3):
        bad_rows.append((1, tuple(0 if a == k else v for a, v in enumerate(n)), good, m))
        bad_rows.append((1, n, good, tuple(0 if a == k else v for a, v in enumerate(m))))
    for C, nn, row, mm in bad_rows:
        rc, oi, os_ = _refused(img, seg, C, nn, row, mm)
        assert rc == -1, (C, nn, row, mm)
        assert np.isnan(oi).all() and (os_ == -1).all(), (C, nn, row, mm)
    # both pairs null, and a pair with one half null
    out_i = torch.full((480,), float("nan"), device=DEV)
    out_s = torch.full((480,), -1, dtype=torch.int16, device=DEV)
    di, dseg = torch.from_numpy(img[0]).to(DEV), torch.from_numpy(seg).to(DEV)
    lib = _lib.load()
    for args in ((None, None, None, None), (di.data_ptr(), None, None, None), (None, dseg.data_ptr(), None, None),
                 (di.data_ptr(), dseg.data_ptr(), out_i.data_ptr(), None), (None, None, out_i.data_ptr(), out_s.data_ptr())):
        assert lib.msl_regrid(args[0], args[1], 1, *n, good.ctypes.data, *m, args[2], args[3], _stream()) == -1
    assert lib.msl_regrid(di.data_ptr(), dseg.data_ptr(), 1, *n, None, *m, out_i.data_ptr(), out_s.data_ptr(), _stream()) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(out_i).all()) and bool((out_s == -1).all())
    with pytest.raises(_lib.HipKernelError):
        _lib.call("msl_regrid", di.data_ptr(), dseg.data_ptr(), 9, *n, good.ctypes.data, *m, out_i.data_ptr(),
                  out_s.data_ptr(), _stream())


def _refused(img, seg, C, n, row, m):
    """A call that must return before any launch, into sentinel buffers sized for four planes of (6, 8, 10)."""
    oi = torch.full((4 * 480 + GUARD,), float("nan"), device=DEV)
    os_ = torch.full((480 + GUARD,), -1, dtype=torch.int16, device=DEV)
    di, dseg = torch.from_numpy(img).to(DEV), torch.from_numpy(seg).to(DEV)
    rc = _lib.load().msl_regrid(di.data_ptr(), dseg.data_ptr(), C, *n, np.ascontiguousarray(row).ctypes.data, *m,
                                oi.data_ptr(), os_.data_ptr(), _stream())
    torch.cuda.synchronize()
    return rc, oi.cpu().numpy(), os_.cpu().numpy()


# ---- the cache ------------------------------------------------------------------------------------------------------------
TARGET = (40, 48, 48)
CACHE_SPECS = [LTN.SPECS[0], LTN.SPECS[3], LTN.SPECS[4], LTN.SPECS[6]]  # identity plan, two permutations, flips + 1.5 mm


def _module(data_dir, sequences, augmentations=None, batch=2):
    dm = DS.LesionsDataModule(data_dir=data_dir, centers=lesion_tree.CENTERS, batch_size=batch, spatial_size=TARGET,
                              input_images=sequences, augmentations=augmentations)
    dm.setup("fit")
    return dm


def _snapshot(b):
    return {k: b[k].cpu().numpy().copy() for k in ("img", "seg", "gb", "gl", "obj_off")}, list(b["subject"])


@pytest.mark.parametrize("sequences", [("FLAIR",), ("FLAIR", "acq-mag_T2star")])
def test_cache_on_a_native_tree_equals_the_cache_on_the_regridded_tree(tmp_path, sequences):
    dir_a, dir_b, plans = LTN.make_trees(tmp_path, CACHE_SPECS, sequences)
    augs = DS.select_augmentations(LESIONS)
    augs = [(n, dict(kw, prob=0.6) if n == "affine" else kw) for n, kw in augs]
    a, b = _module(dir_a, sequences, augs), _module(dir_b, sequences, augs)
    ca, cb = LesionCache(a, DEV), LesionCache(b, DEV)
    assert ca.full_shapes == cb.full_shapes and ca.shapes == cb.shapes and ca.origins == cb.origins
    assert all(p is None for p in cb.plans) and sorted(p.src_shape for p in ca.plans) == sorted(p.src_shape for p in plans)
    assert [p.out_shape for p in ca.plans] == ca.full_shapes and sum(not p.identity for p in ca.plans) == 3
    boxes = 0
    for epoch in (0, 1):
        for ba, bb in zip(ca.train_batches(epoch), cb.train_batches(epoch)):
            (ta, sa), (tb, sb) = _snapshot(ba), _snapshot(bb)
            assert sa == sb and ta["img"].shape[1:] == (len(sequences),) + TARGET
            for key in ta:
                assert ta[key].tobytes() == tb[key].tobytes(), (epoch, sa, key)
            boxes += int(ta["obj_off"][-1])
    assert boxes >= 6
    va, vb = list(ca.val_batches()), list(cb.val_batches())
    assert len(va) == len(vb) >= 1
    for ba, bb in zip(va, vb):
        assert ba["subject"] == bb["subject"] and torch.equal(ba["img"], bb["img"])
        assert all(torch.equal(x, y) for x, y in zip(ba["boxes"], bb["boxes"]))
        assert all(torch.equal(x, y) for x, y in zip(ba["labels"], bb["labels"]))
        assert ba["full_shape"] == bb["full_shape"] and ba["crop_origin"] == bb["crop_origin"]
    # the cached cases are the host pipeline's crop / normalise result on the host-regridded case
    for ds in (a.train_dataset, a.test_dataset):
        for i in range(len(ds)):
            img, seg = ds.load(i)
            ci, cs = DS.crop_foreground(img, seg, 5)
            di, dseg = ca.case(ca.slot[ds.subjects[i]])
            assert tuple(di.shape) == ci.shape and np.array_equal(dseg.cpu().numpy(), cs)
            want = DS.normalize_nonzero(ci) if ci.ndim == 3 else np.stack([DS.normalize_nonzero(ch) for ch in ci])
            np.testing.assert_allclose(di.cpu().numpy(), want, rtol=NORM_RTOL, atol=NORM_ATOL)


# ---- predict --------------------------------------------------------------------------------------------------------------
# two of the four are signed permutations at 1 mm (at least one of them is in the predicted split of three)
PRED_SPECS = [LTN.SPECS[2], ((40, 38, 44), (1, 2, 0), (1, -1, 1), (1.0, 1.0, 1.0)), LTN.SPECS[4], LTN.SPECS[6]]
PRED_TARGET = (48, 64, 64)  # the fitted size the other predict tests run the network at


def test_predict_writes_native_boxes_and_overlays_on_both_routes(tmp_path):
    """The host route and the --cache 1 route on a native tree: the same sub-*_preds_case.json ("native" block included)
    and the same sub-*_preds_native.npy, drawn at the stored shape."""
    from mslesions3d_amd import predict as P
    from mslesions3d_amd.ssd3d import LSSD3D
    dir_a, _, plans = LTN.make_trees(tmp_path, PRED_SPECS)
    torch.manual_seed(0)
    ckpt = str(tmp_path / "random.ckpt")
    LSSD3D(n_classes=2, input_channels=1, input_size=PRED_TARGET).save_checkpoint(ckpt)
    by_subject = {f"{lesion_tree.CENTERS[k % 2]}_{100 - k:03d}": p for k, p in enumerate(plans)}
    outs = {}
    for route, extra in (("host", []), ("dev", ["--cache", "1"])):
        args = P.build_parser().parse_args(["-dm", "lesions", "-d", dir_a, "--centers", *lesion_tree.CENTERS,
                                            "--spatial_size", *map(str, PRED_TARGET), "-m", ckpt, "-ps", "train",
                                            "-o", str(tmp_path / route), "-sc", "0.01", "-k", "20", "-si", "1"])
        P.predict_example(args)
        outs[route] = tmp_path / route
    files = sorted(os.listdir(outs["host"]))
    assert files == sorted(os.listdir(outs["dev"]))
    subjects = [f[len("sub-"):-len("_preds_case.json")] for f in files if f.endswith("_preds_case.json")]
    assert len(subjects) == 3 and all(f"sub-{s}_preds_native.npy" in files for s in subjects)
    one_mm = 0
    for s in subjects:
        plan = by_subject[s]
        texts = [open(outs[r] / f"sub-{s}_preds_case.json").read() for r in ("host", "dev")]
        case = json.loads(texts[0])
        native = case.pop("native")
        assert native["shape"] == list(plan.src_shape) and len(native["boxes"]) == len(case) >= 1
        frac = np.asarray([v[0] for v in case.values()], np.float32).reshape(-1, 6)
        got = np.asarray(native["boxes"], np.float32).reshape(-1, 6)
        assert np.array_equal(got, DS.regrid_to_native(frac, plan))
        if all(st == 1.0 for st in plan.step):  # a signed permutation at 1 mm, by hand: voxel r of the reoriented axis
            one_mm += 1                         # is stored voxel r, or n - 1 - r with min and max swapped
            n = np.asarray(plan.out_shape, np.float64)
            lo, hi = frac[:, :3].astype(np.float64) * n, frac[:, 3:].astype(np.float64) * n
            for k in range(3):
                a, b = (n[k] - 1 - hi[:, k], n[k] - 1 - lo[:, k]) if plan.rev[k] else (lo[:, k], hi[:, k])
                np.testing.assert_allclose(got[:, plan.ax[k]], a / n[k], rtol=0, atol=1e-6)
                np.testing.assert_allclose(got[:, 3 + plan.ax[k]], b / n[k], rtol=0, atol=1e-6)
        vols = [np.load(outs[r] / f"sub-{s}_preds_native.npy") for r in ("host", "dev")]
        assert vols[0].shape == tuple(plan.src_shape) and vols[0].dtype == np.int16 and vols[0].any()
        assert np.load(outs["host"] / f"sub-{s}_preds.npy").shape == tuple(plan.out_shape)
        assert texts[0] == texts[1], s
        assert np.array_equal(vols[0], vols[1]), s
    assert one_mm >= 1
