"""The free-form deformation on the device: msl_augment_deform_mc (csrc/datapipe.hip) through
the C ABI against devicedata.deform_numpy + datasets.window on the host, its routing through devicedata.LesionCache on
the fit and the patch route, and the training entry point on both routes.  Comparisons are bit for bit, images and
masks."""
import functools
import json

import numpy as np
import pytest
import torch

from mslesions3d_amd import _lib
from mslesions3d_amd import datasets as DS
from mslesions3d_amd import devicedata as DD
from mslesions3d_amd.devicedata import AFFINE_STRIDE, LesionCache, deform_rows, sample_params
from tests import lesion_tree
from tests.test_gpu_lesions import GUARD, IMG_PATTERN, SEG_PATTERN, SHAPES, _same, _snapshot, _variants

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CASE_SHAPES = [(9, 14, 11), (17, 30, 21), (24, 32, 32), (5, 7, 130)]  # the last one: a row longer than a wave
TARGETS = [(16, 20, 24), (24, 32, 32)]  # pads every case / crops the largest one
LONG = (5, 7, 130)
PADS = ("reflection", "border", "zeros")
INTENSITY = [("shiftintensity", {"offsets": 0.1, "prob": 1.0}), ("scaleintensity", {"factors": 0.1, "prob": 1.0})]
FN = "msl_augment_deform_mc"


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _perms():
    """The signed-permutation classes of the fit's tests (tests/test_gpu_lesions.py::_variants), without their affine."""
    v = _variants()
    return {"identity": [], "flip": v["flip"], "rot90": v["rot90"], "recipe": v["recipe"][:4]}


# (case, permutation class, L, drawn, intensity operations): every class with a drawn deformation, every L, every case
# shape, rows that drew nothing between rows that did.  max_displacement is large, so the cap sets the amplitude
BATCH = [(0, "identity", 4, True, True), (1, "flip", 5, True, False), (2, "rot90", 7, True, False),
         (1, "recipe", 16, True, True), (2, "identity", 7, False, True), (0, "rot90", 5, True, True),
         (2, "flip", 4, False, False), (0, "recipe", 7, True, False), (1, "rot90", 4, True, True),
         (2, "recipe", 16, True, False)]
# the long case keeps its shape under flips only
LONG_BATCH = [(3, "identity", 4, True, True), (3, "flip", 16, True, False), (3, "identity", 7, False, True),
              (3, "flip", 5, True, True)]


@functools.lru_cache(maxsize=None)
def _data():
    rs = np.random.RandomState(0)
    img = [(rs.randn(2, *s) * np.array([1.0, 2.0]).reshape(2, 1, 1, 1)).astype(np.float32) for s in CASE_SHAPES]
    seg = [((rs.rand(*s) < 0.3) * rs.randint(1, 3000, s)).astype(np.int16) for s in CASE_SHAPES]
    return img, seg


class _Arena:
    def __init__(self, C):
        img, seg = _data()
        self.C = C
        off = np.concatenate([[0], np.cumsum([int(np.prod(s)) for s in CASE_SHAPES])])
        self.d_img = torch.from_numpy(np.concatenate([v[:C].reshape(-1) for v in img])).to(DEV)
        self.d_seg = torch.from_numpy(np.concatenate([v.reshape(-1) for v in seg])).to(DEV)
        self.table = torch.tensor([[int(off[k]), *CASE_SHAPES[k]] for k in range(len(CASE_SHAPES))], dtype=torch.int64,
                                  device=DEV)


def _launch(arena, rows, lattices, windows, target, fn=FN, lattices_len=None):
    """One launch into pattern-filled buffers with guard bands -> (rc, image (N, C) + target, mask (N,) + target, raw
    image words, raw mask words).  The bands in front of and behind both outputs must come back untouched."""
    rows = np.asarray(rows, dtype=np.float64)
    C, N, V = arena.C, rows.shape[0], int(np.prod(target))
    assert rows.shape == (N, AFFINE_STRIDE)
    p = torch.from_numpy(rows).to(DEV)
    t = None if lattices is None else torch.from_numpy(np.asarray(lattices, dtype=np.float64)).to(DEV)
    w = None if windows is None else torch.from_numpy(np.asarray(windows, dtype=np.int32).reshape(N, 3)).to(DEV)
    bi = torch.full((N * C * V + 2 * GUARD,), IMG_PATTERN, dtype=torch.int32, device=DEV)
    bs = torch.full((N * V + 2 * GUARD,), SEG_PATTERN, dtype=torch.int16, device=DEV)
    oi, os_ = bi[GUARD:GUARD + N * C * V], bs[GUARD:GUARD + N * V]
    args = [arena.d_img.data_ptr(), arena.d_seg.data_ptr(), arena.d_seg.numel(), C, arena.table.data_ptr(),
            arena.table.shape[0], p.data_ptr()]
    if fn == FN:
        args += [None if t is None else t.data_ptr(), (0 if t is None else t.numel()) if lattices_len is None else lattices_len]
    if fn != "msl_augment_fit_mc":
        args.append(None if w is None else w.data_ptr())
    rc = getattr(_lib.load(), fn)(*args, N, *target, oi.data_ptr(), os_.data_ptr(), _stream())
    hi, hs = bi.cpu(), bs.cpu()
    for band in (hi[:GUARD], hi[GUARD + N * C * V:]):
        assert bool((band == IMG_PATTERN).all()), "image guard band overwritten"
    for band in (hs[:GUARD], hs[GUARD + N * V:]):
        assert bool((band == SEG_PATTERN).all()), "mask guard band overwritten"
    return (rc, hi[GUARD:GUARD + N * C * V].view(torch.float32).reshape((N, C) + tuple(target)).numpy(),
            hs[GUARD:GUARD + N * V].reshape((N,) + tuple(target)).numpy(), hi[GUARD:GUARD + N * C * V], hs[GUARD:GUARD + N * V])


def _augs(perm, L, drawn, ops, pad):
    kw = {"control_points": L, "max_displacement": 100.0, "padding_mode": pad, "prob": 1.0 if drawn else 0.0}
    return list(_perms()[perm]) + [("elastic3d", kw)] + (INTENSITY if ops else [])


@functools.lru_cache(maxsize=None)
def _host(pad, long=False):
    """Per sample of BATCH (LONG_BATCH) -> (image (2,) + n', mask n', (perm, stages)): the permuted case, deformed by
    ``deform_numpy`` where the row drew, then the intensity operations in f32.  Read-only; shared by every target, route
    and C."""
    img, seg = _data()
    out = []
    for n, (case, perm, L, drawn, ops) in enumerate(LONG_BATCH if long else BATCH):
        augs = _augs(perm, L, drawn, ops, pad)
        ps = sample_params(DS.draw_augmentations(augs, np.random.RandomState(10 + n)), CASE_SHAPES[case], augs, ragged=True)
        x = np.stack([DD.permute_numpy(ch, ps[0]) for ch in img[case]])
        m = DD.permute_numpy(seg[case], ps[0])
        for st in ps[1]:
            if isinstance(st, DD.DeformStage):
                assert st.lattice.shape == (3, L, L, L)
                x = np.stack([DD.deform_numpy(ch, st.lattice, 1, st.boundary) for ch in x])
                m = DD.deform_numpy(m, st.lattice, 0, st.boundary)
            elif isinstance(st, DD.IntensityOp):
                x = x + st.value if st.kind == DD.OP_ADD else x * st.value
        assert x.dtype == np.float32 and m.dtype == np.int16 and drawn == any(isinstance(s, DD.DeformStage) for s in ps[1])
        x, m = np.ascontiguousarray(x), np.ascontiguousarray(m)
        x.setflags(write=False)
        m.setflags(write=False)
        out.append((x, m, ps))
    return out


def _origins(shapes, target):
    """Per sample an origin in its augmented frame: interior at an odd offset (as far as the case is large enough),
    negative, overhanging, in turn."""
    out = []
    for n, shape in enumerate(shapes):
        if n % 3 == 0:
            out.append(tuple(max(0, min(2 * a + 1, shape[a] - target[a])) for a in range(3)))
        elif n % 3 == 1:
            out.append((-5, -7, -9))
        else:
            out.append(tuple(shape[a] - target[a] + 6 + a for a in range(3)))
    return out


def _check(host, batch, rows_lat, origins, target, C, route):
    rows, lat = rows_lat
    rc, oi, os_, _, _ = _launch(_Arena(C), rows, lat, None if route == "fit" else origins, target)
    assert rc == 0
    for n, (x, m, _) in enumerate(host):
        assert _same(os_[n], DS.window(m, origins[n], target)), n
        want = DS.window(x[:C], origins[n], target)
        for c in range(C):
            assert _same(oi[n, c], want[c]), (n, c)
        if route == "fit":
            assert _same(os_[n], DS.resize_with_pad_or_crop(m, target))


@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("route", ["fit", "window"])
@pytest.mark.parametrize("target", TARGETS)
@pytest.mark.parametrize("pad", PADS)
def test_augment_deform_mc_equals_the_host_steps(pad, target, route, C):
    host = _host(pad)
    shapes = [h[1].shape for h in host]
    assert any(s != CASE_SHAPES[b[0]] for s, b in zip(shapes, BATCH))  # a rot90 changed a shape
    rows, lat = deform_rows([b[0] for b in BATCH], [h[2] for h in host])
    assert sorted(set(rows[:, 7].tolist())) == [0.0, 3.0] and sorted(set(rows[:, 9].tolist())) == [0.0, 4.0, 5.0, 7.0, 16.0]
    assert lat.size == sum(3 * b[2] ** 3 for b in BATCH if b[3])
    if route == "fit":
        origins = [[DS.fit_shift(n, t) for n, t in zip(s, target)] for s in shapes]
    else:
        origins = _origins(shapes, target)
        assert any(min(o) < 0 for o in origins)
        if target == TARGETS[0]:  # (no case holds the larger target with room to spare)
            assert any(o[2] % 2 == 1 and 0 < o[2] < s[2] - target[2] for o, s in zip(origins, shapes))
        assert any(o[a] + target[a] > s[a] and o[a] > 0 for o, s in zip(origins, shapes) for a in range(3))
    _check(host, BATCH, (rows, lat), origins, target, C, route)


@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("pad", PADS)
def test_a_row_longer_than_a_wave(pad, C):
    """(5, 7, 130) fitted to (5, 7, 130): every lane takes the row loop two or three times."""
    host = _host(pad, True)
    assert all(h[1].shape == LONG for h in host)
    rows_lat = deform_rows([b[0] for b in LONG_BATCH], [h[2] for h in host])
    _check(host, LONG_BATCH, rows_lat, [(0, 0, 0)] * len(host), LONG, C, "fit")
    _check(host, LONG_BATCH, rows_lat, [(0, 0, -3), (1, -2, 5), (0, 0, 0), (-1, 2, 40)], LONG, C, "window")


def test_the_drawn_rows_move_the_case_and_sample_outside_it():
    """What the comparisons above exercise: on every drawn row a fair share of the coordinates leaves the case, and on
    the rows of few control points (the cap allows A = spacing / 4, a fraction of a voxel under a fine lattice on a small
    case) most voxels move by more than a quarter voxel."""
    strong = 0
    for long in (False, True):
        for x, m, (perm, stages) in _host("border", long):
            for st in stages:
                if isinstance(st, DD.DeformStage):
                    coords = DS.deform_coords(m.shape, st.lattice)
                    grid = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in m.shape), indexing="ij")
                    out = np.zeros(m.shape, bool)
                    for g, n in zip(coords, m.shape):
                        out |= (g < 0) | (g > n - 1)
                    moved = np.sqrt(sum((c - g) ** 2 for c, g in zip(coords, grid))) > 0.25
                    assert out.mean() >= 0.02, (m.shape, out.mean())
                    strong += moved.mean() >= 0.5
    assert strong >= 6


@pytest.mark.parametrize("target", TARGETS)
def test_rows_that_drew_nothing_are_the_fit_and_the_window(target):
    """[7] = 0: the permuted copy of msl_augment_fit_mc (windows null) and msl_augment_window_mc, intensity operations
    included - alone in a batch and between deformation rows."""
    arena = _Arena(2)
    host = _host("border")
    cases = [b[0] for b in BATCH]
    plain = [(h[2][0], [st for st in h[2][1] if isinstance(st, DD.IntensityOp)]) for h in host]  # nobody draws
    rows, lat = deform_rows(cases, plain)
    assert lat.size == 0 and not rows[:, 7].any() and rows[:, 21].any()
    origins = _origins([h[1].shape for h in host], target)
    rc, oi, os_, _, _ = _launch(arena, rows, np.zeros(1), None, target)
    rc_f, fi, fs, _, _ = _launch(arena, rows, None, None, target, fn="msl_augment_fit_mc")
    assert rc == 0 and rc_f == 0 and _same(oi, fi) and _same(os_, fs) and oi.any() and os_.any()
    rc, oi, os_, _, _ = _launch(arena, rows, np.zeros(1), origins, target)
    rc_w, wi, ws, _, _ = _launch(arena, rows, None, origins, target, fn="msl_augment_window_mc")
    assert rc == 0 and rc_w == 0 and _same(oi, wi) and _same(os_, ws)
    mixed, lat = deform_rows(cases, [h[2] for h in host])
    rc, oi, os_, _, _ = _launch(arena, mixed, lat, origins, target)
    assert rc == 0
    for n, b in enumerate(BATCH):
        if not b[3]:
            assert _same(oi[n], wi[n]) and _same(os_[n], ws[n])
    again = _launch(arena, mixed, lat, origins, target)  # the same inputs, the same outputs
    assert again[0] == 0 and _same(again[1], oi) and _same(again[2], os_)


def test_invalid_rows_write_zeros_and_nothing_else():
    arena = _Arena(2)
    target = (16, 20, 24)
    host = _host("border")
    keep = [0, 1, 3]  # three drawn rows
    rows, lat = deform_rows([BATCH[n][0] for n in keep], [host[n][2] for n in keep])
    good = _launch(arena, rows, lat, None, target)
    assert good[0] == 0 and all(good[1][n].any() and good[2][n].any() for n in range(3))

    def zero_rows(rows, which, lattices_len=None):
        rc, oi, os_, _, _ = _launch(arena, rows, lat, None, target, lattices_len=lattices_len)  # (the bands: in _launch)
        assert rc == 0
        for n in range(rows.shape[0]):
            if n in which:
                assert not oi[n].any() and not os_[n].any(), n
            else:
                assert _same(oi[n], good[1][n]) and _same(os_[n], good[2][n]), n

    bad = rows.copy()
    bad[0, 0], bad[2, 0] = len(CASE_SHAPES), -1  # a case past the table, a negative case
    zero_rows(bad, {0, 2})
    for kind in (1.0, 2.0, 4.0, float("nan")):  # an affine row and a warp row are not this entry point's
        bad = rows.copy()
        bad[1, 7] = kind
        zero_rows(bad, {1})
    bad = rows.copy()
    bad[0, 1:4] = (0, 0, 1)  # not a permutation
    zero_rows(bad, {0})
    for L in (3.0, 17.0, 4.5, -4.0, 1e300, float("nan")):  # (a 3^3 or 17^3 lattice at [8] = 0 would lie inside the table)
        bad = rows.copy()
        bad[0, 9] = L
        zero_rows(bad, {0})
    # the last row's lattice ends exactly at lattices_len: valid; one double fewer and it ends past it
    assert rows[2, 8] + 3 * BATCH[3][2] ** 3 == lat.size
    zero_rows(rows, set())
    zero_rows(rows, {2}, lattices_len=lat.size - 1)
    for off in (lat.size, -1.0, float(lat.size - 3), 1e300, float("nan")):
        bad = rows.copy()
        bad[1, 8] = off
        zero_rows(bad, {1})


def test_deform_refuses_bad_arguments():
    arena = _Arena(2)
    target = (16, 20, 24)
    rows, lat = deform_rows([0], [_host("border")[0][2]])
    rc, _, _, raw_i, raw_s = _launch(arena, rows, None, None, target)  # lattices null
    assert rc == -1 and bool((raw_i == IMG_PATTERN).all()) and bool((raw_s == SEG_PATTERN).all())  # nothing written
    rc, _, _, raw_i, raw_s = _launch(arena, rows, lat, None, target, lattices_len=0)
    assert rc == -1 and bool((raw_i == IMG_PATTERN).all()) and bool((raw_s == SEG_PATTERN).all())
    p, t = torch.from_numpy(rows).to(DEV), torch.from_numpy(lat).to(DEV)
    di = torch.zeros((2,) + target, dtype=torch.float32, device=DEV)
    ds = torch.zeros(target, dtype=torch.int16, device=DEV)
    ok = [arena.d_img.data_ptr(), arena.d_seg.data_ptr(), arena.d_seg.numel(), 2, arena.table.data_ptr(), len(CASE_SHAPES),
          p.data_ptr(), t.data_ptr(), t.numel(), None, 1, *target, di.data_ptr(), ds.data_ptr(), _stream()]
    lib = _lib.load()
    assert lib.msl_augment_deform_mc(*ok) == 0 and di.any()
    for pos, value in ((0, None), (1, None), (2, 0), (3, 0), (3, 5), (4, None), (5, 0), (6, None), (7, None), (8, -4),
                       (10, 0), (11, 0), (12, 0), (13, 0), (14, None), (15, None)):
        args = list(ok)
        args[pos] = value
        assert lib.msl_augment_deform_mc(*args) == -1, (pos, value)
    args = list(ok)
    args[10] = 65536  # N past the grid's second dimension: refused before anything is launched
    assert lib.msl_augment_deform_mc(*args) == -2
    with pytest.raises(_lib.HipKernelError):
        _lib.call("msl_augment_deform_mc", *ok[:3], 0, *ok[4:])


# ---- LesionCache ---------------------------------------------------------------------------------------------------------
PATCH = (32, 32, 32)
TARGET = (48, 64, 64)


def _module(tmp_path, augmentations, patch):
    data_dir = lesion_tree.make_tree(tmp_path, SHAPES)
    kw = {"spatial_size": TARGET} if patch is None else {"patch_size": patch, "patch_foreground": 0.7, "tile_margin": (4, 4, 6)}
    dm = DS.LesionsDataModule(data_dir=data_dir, centers=lesion_tree.CENTERS, batch_size=2, augmentations=augmentations, **kw)
    dm.setup("fit")
    return dm


def _recorded_batches(cache, epoch):
    """The batches of an epoch with the entry points each one launched."""
    it = cache.train_batches(epoch)
    while True:
        _lib.start_recording()
        try:
            b = next(it, None)
        finally:
            prog = _lib.stop_recording()
        if b is None:
            return
        snap = _snapshot(b)
        if "patch_origin" in b:
            snap["patch_origin"] = list(b["patch_origin"])
        yield snap, [fn.__name__ for fn, _, _ in prog if fn is not None]


def _recipe(prob):
    """The recipe of the issue at every probability 1, the deformation's own at ``prob``."""
    augs = DS.select_training_augmentations(["flip", "rotate90", "elastic3d", "shiftintensity", "scaleintensity"])
    assert [n for n, _ in augs] == ["flip"] + ["rotate90"] * 3 + ["elastic3d", "shiftintensity", "scaleintensity"]
    return [(n, dict(kw, prob=prob if n == "elastic3d" else 1.0)) for n, kw in augs]


@pytest.mark.parametrize("patch", [None, PATCH], ids=["fit", "patch"])
def test_train_batches_equal_the_host_loader_under_the_deformation(tmp_path, patch):
    drawn, plain_batches, deform_batches, boxes_seen = 0, 0, 0, 0
    # two epochs with every sample deformed, then one in which two batches draw nothing and keep their old launch and
    # two hold one drawn and one plain sample (worked out on the host: the draws are the host's)
    for prob, epochs in ((1.0, (0, 1)), (0.5, (3,))):
        augs = _recipe(prob)
        dm = _module(tmp_path / f"p{prob}", augs, patch)
        cache = LesionCache(dm, DEV)
        tr = dm.train_dataset
        for epoch in epochs:
            dm.set_epoch(epoch)
            host = list(dm.train_dataloader())
            dev = list(_recorded_batches(cache, epoch))
            assert [d["subject"] for d, _ in dev] == [h["subject"] for h in host]
            for (d, names), h in zip(dev, host):
                off = d["obj_off"].tolist()
                in_batch = 0
                for n, s in enumerate(d["subject"]):
                    ci, cs = cache.case(cache.slot[s])
                    x, m = ci.cpu().numpy()[None], cs.cpu().numpy()[None]
                    rs = DS.sample_rng(tr.seed, epoch, s)
                    for (name, kw), (_, dr) in zip(augs, DS.draw_augmentations(augs, DS.sample_rng(tr.seed, epoch, s))):
                        x, m = DS.AUGMENTATIONS[name](x, m, rs, **kw)  # the host transforms (scipy) on the cached volume
                        in_batch += name == "elastic3d" and dr is not None
                    if patch is None:
                        x, m = DS.resize_with_pad_or_crop(x, TARGET), DS.resize_with_pad_or_crop(m, TARGET)
                    else:
                        assert d["patch_origin"][n] == h["patch_origin"][n]
                        x, m = DS.window(x, d["patch_origin"][n], patch), DS.window(m, d["patch_origin"][n], patch)
                    assert _same(d["seg"][n], m[0]), (epoch, s)
                    assert _same(d["img"][n], x), (epoch, s)
                    assert _same(d["gb"][off[n]:off[n + 1]], h["boxes"][n]), (epoch, s)
                    assert torch.equal(d["gl"][off[n]:off[n + 1]], h["labels"][n])
                    boxes_seen += off[n + 1] - off[n]
                if patch is not None:  # the host normalises with the kernel's arithmetic there: the loader's batch, bit for bit
                    assert _same(d["img"], h["img"])
                old = "msl_augment_fit_mc" if patch is None else "msl_augment_window_mc"
                assert (FN in names) == (in_batch > 0) and (old in names) == (in_batch == 0), names
                assert "msl_augment_warp_mc" not in names
                assert prob < 1.0 or in_batch == len(d["subject"])
                drawn += in_batch
                deform_batches += in_batch > 0
                plain_batches += in_batch == 0
    print(f"elastic3d: {drawn} drawn, {deform_batches} deformation batches, {plain_batches} plain batches, {boxes_seen} boxes")
    assert drawn == 18 and deform_batches == 10 and plain_batches == 2 and boxes_seen >= 16


def test_the_cache_refuses_a_second_resampling_stage(tmp_path):
    dm = _module(tmp_path, DS.select_training_augmentations(["flip", "affine", "elastic3d"]), None)
    with pytest.raises(NotImplementedError, match="two affine stages on cases of unequal shape"):
        LesionCache(dm, DEV)
    dm.train_dataset.augmentations = DS.select_training_augmentations(["zoom", "elastic3d"])
    with pytest.raises(NotImplementedError, match="two affine stages on cases of unequal shape"):
        LesionCache(dm, DEV)


# ---- the entry point -----------------------------------------------------------------------------------------------------
def _run_train(root, cache):
    from mslesions3d_amd import train as T
    args = T.build_parser().parse_args(["-dm", "lesions", "-d", str(root / "raw"), "--centers", *lesion_tree.CENTERS,
                                        "--patch_size", *map(str, PATCH), "-b", "2", "-me", "2", "-ld", str(root / "logs"),
                                        "-en", f"c{cache}", "-c", str(cache), "-a", "flip", "rotate90", "elastic3d",
                                        "shiftintensity", "scaleintensity",
                                        "-pl", "1 3 5 7"])  # a fourth, finer scale: 501 priors or more on a 32^3 input
    T.example(args)
    return [l.rstrip("\n") for l in open(root / "logs" / f"c{cache}" / "metrics.jsonl")]


def test_both_routes_train_under_elastic3d_and_log_the_same_lines(tmp_path):
    """Patch mode: both routes normalise with the same arithmetic, cut the same windows out of the same deformed cases and
    run the same kernels in the same order, so the two files are equal as text."""
    lesion_tree.make_tree(tmp_path, SHAPES)  # (every validation tile batch of this tree holds a lesion)
    host, dev = _run_train(tmp_path, 0), _run_train(tmp_path, 1)
    for h, d in zip(host, dev):
        print(h)
        print(d)
    assert host == dev and len(host) >= 8
    rec = [json.loads(l) for l in dev]
    train = [r["total_loss/training"] for r in rec if "total_loss/training" in r]
    assert len(train) == 8 and np.isfinite(train).all()
