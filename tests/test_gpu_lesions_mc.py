"""msl_foreground_box_mc and msl_augment_fit_mc (csrc/datapipe.hip) through the C ABI, their routing through
devicedata.LesionCache and the entry points for cases of several MR sequences, and the 2-channel training step on a
non-cube input, against the host pipeline of datasets.LesionsDataModule(input_images=(...)) and the oracle.

The geometry (case shapes, seeds 10 + n, rotation ranges, variants, targets) is tests/test_gpu_lesions.py's; the host
reference of a (variant, target) pair is computed once for three channels and shared by the C = 2 and C = 3 cases."""
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
from tests.test_gpu_lesions import (CASE_SHAPES, GUARD, IMG_PATTERN, LESIONS, NORM_ATOL, NORM_RTOL, SEG_PATTERN, SHAPES,
                                    TARGET, _same, _snapshot, _variants)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TWO = lesion_tree_mc.SEQUENCES[:2]
CASES = [0, 1, 2, 3, 2, 0]  # four shapes in one batch
MAX_C = 3


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- msl_foreground_box_mc -----------------------------------------------------------------------------------------------
def _fg_volumes():
    """Channel-first volumes of up to three channels; rows longer than a wave, a last axis that is no multiple of 64."""
    rs = np.random.RandomState(1)
    shape = (17, 31, 130)
    a, b, c = (np.zeros(shape, np.float32) for _ in range(3))
    a[3:9, 5:20, 70:128] = (rs.rand(6, 15, 58) < 0.5) * 2.0
    a[3, 5, 70] = a[8, 19, 127] = 1.0
    b[6:14, 2:11, 40:90] = (rs.rand(8, 9, 50) < 0.5) * 0.25
    b[6, 2, 40] = b[13, 10, 89] = 1.0
    c[1:4, 25:30, 100:130] = 7.0
    a[0, 0, 0] = b[16, 30, 129] = -5.0  # negative voxels are background
    zero, neg = np.zeros(shape, np.float32), -np.ones(shape, np.float32)
    return [np.stack([a, b, c]), np.stack([a, zero, b]), np.stack([neg, b, neg]), np.stack([zero, neg, zero]),
            np.stack([c, zero, zero])]


@pytest.mark.parametrize("margin", [5, 0, 2])
def test_foreground_box_mc_equals_the_host_union_box(margin):
    larger = 0
    for vol in _fg_volumes():
        for C in (1, 2, 3):
            v = np.ascontiguousarray(vol[:C])
            d = torch.from_numpy(v).to(DEV)
            box = torch.full((8,), -77, dtype=torch.int32, device=DEV)
            _lib.call("msl_foreground_box_mc", d.data_ptr(), C, *v.shape[1:], margin, box.data_ptr(), _stream())
            got = box.cpu().tolist()
            lo, hi = DS.foreground_box(v, margin)
            assert got[:6] == list(lo) + list(hi), (C, margin)
            assert got[6:] == [-77, -77]
            if C == 1:  # msl_foreground_box is the forward to this launch with C = 1
                one = torch.full((8,), -77, dtype=torch.int32, device=DEV)
                _lib.call("msl_foreground_box", d.data_ptr(), *v.shape[1:], margin, one.data_ptr(), _stream())
                assert one.cpu().tolist() == got
            else:
                own = [DS.foreground_box(ch, margin) for ch in v if (ch > 0).any()]
                larger += len(own) > 1 and all(any(h - l > bh - bl for l, h, bl, bh in zip(lo, hi, *b)) for b in own)
    assert larger >= 2  # unions strictly larger than every channel's own box were among the cases
    assert DS.foreground_box(_fg_volumes()[3][:2], margin) == ((0, 0, 0), (17, 31, 130))  # the empty union
    for C in (0, 5):
        with pytest.raises(_lib.HipKernelError):
            _lib.call("msl_foreground_box_mc", d.data_ptr(), C, 4, 4, 4, margin, box.data_ptr(), _stream())


# ---- msl_augment_fit_mc --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _data(shapes=tuple(CASE_SHAPES)):
    """-> (per case (MAX_C, n0, n1, n2) f32 planes of differing content, per case int16 mask)."""
    rs = np.random.RandomState(0)
    img = [(rs.randn(MAX_C, *s) * (1.0 + np.arange(MAX_C)).reshape(-1, 1, 1, 1)).astype(np.float32) for s in shapes]
    seg = [((rs.rand(*s) < 0.3) * rs.randint(1, 3000, s)).astype(np.int16) for s in shapes]
    for v in img:
        assert all(not np.array_equal(v[a], v[b]) for a in range(MAX_C) for b in range(a))
    return img, seg


class _Arena:
    """The first C planes of every case, channel-planar at C * offset; the mask arena and the table as for one channel."""

    def __init__(self, C, shapes=tuple(CASE_SHAPES)):
        img, seg = _data(shapes)
        self.C, self.shapes = C, list(shapes)
        off = np.concatenate([[0], np.cumsum([int(np.prod(s)) for s in shapes])])
        self.d_img = torch.from_numpy(np.concatenate([v[:C].reshape(-1) for v in img])).to(DEV)
        self.d_seg = torch.from_numpy(np.concatenate([v.reshape(-1) for v in seg])).to(DEV)
        assert self.d_img.numel() == C * self.d_seg.numel()
        self.table = torch.tensor([[int(off[k]), *shapes[k]] for k in range(len(shapes))], dtype=torch.int64, device=DEV)

    def launch(self, rows, target, table=None, seg_elems=None, C=None):
        rows = np.asarray(rows, dtype=np.float64)
        C = self.C if C is None else C
        N, V = rows.shape[0], int(np.prod(target))
        assert rows.shape == (N, AFFINE_STRIDE)
        p = torch.from_numpy(rows).to(DEV)
        bi = torch.full((N * C * V + 2 * GUARD,), IMG_PATTERN, dtype=torch.int32, device=DEV)
        bs = torch.full((N * V + 2 * GUARD,), SEG_PATTERN, dtype=torch.int16, device=DEV)
        oi, os_ = bi[GUARD:GUARD + N * C * V], bs[GUARD:GUARD + N * V]
        table = self.table if table is None else table
        _lib.call("msl_augment_fit_mc", self.d_img.data_ptr(), self.d_seg.data_ptr(),
                  self.d_seg.numel() if seg_elems is None else seg_elems, C, table.data_ptr(), table.shape[0],
                  p.data_ptr(), N, *target, oi.data_ptr(), os_.data_ptr(), _stream())
        hi, hs = bi.cpu(), bs.cpu()
        for band in (hi[:GUARD], hi[GUARD + N * C * V:]):
            assert bool((band == IMG_PATTERN).all()), "image guard band overwritten"
        for band in (hs[:GUARD], hs[GUARD + N * V:]):
            assert bool((band == SEG_PATTERN).all()), "mask guard band overwritten"
        return (hi[GUARD:GUARD + N * C * V].view(torch.float32).reshape((N, C) + tuple(target)).numpy(),
                hs[GUARD:GUARD + N * V].reshape((N,) + tuple(target)).numpy())


@functools.lru_cache(maxsize=None)
def _host(variant, target):
    """Host steps 3-4 on the MAX_C-channel cases of the batch -> per sample (image (MAX_C,) + target, mask, share of
    padded output voxels, affine share outside the source, (perm, stages), augmented shape).  Read-only."""
    img, seg = _data()
    augs = _variants()[variant]
    out = []
    for n, case in enumerate(CASES):
        seed = 10 + n
        x, m = img[case], seg[case][None]
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
        perm, stages = sample_params(DS.draw_augmentations(augs, np.random.RandomState(seed)), CASE_SHAPES[case], augs,
                                     ragged=True)
        outside = 0.0
        geo = [st for st in stages if hasattr(st, "matrix")]
        if geo:
            o = np.stack(np.meshgrid(*(np.arange(k) for k in shape), indexing="ij"), -1).astype(np.float64)
            c = o @ np.asarray(geo[0].matrix).T + np.asarray(geo[0].offset)
            outside = float(((c < 0) | (c > np.array(shape) - 1)).any(-1).mean())
        xi = np.ascontiguousarray(DS.resize_with_pad_or_crop(x, target))
        xi.setflags(write=False)
        out.append((xi, DS.resize_with_pad_or_crop(m, target)[0], 1.0 - inside.mean(), outside, (perm, stages), shape))
    return out


@pytest.mark.parametrize("C", [2, 3])  # an odd count: nothing may be wired for two
@pytest.mark.parametrize("target", [(40, 48, 64), (33, 70, 45)])  # vector stores / a last axis that is not 4-aligned
@pytest.mark.parametrize("variant", list(_variants()))
def test_augment_fit_mc_equals_the_host_steps(variant, target, C):
    host = _host(variant, target)
    oi, os_ = _Arena(C).launch(fit_rows(CASES, [h[4] for h in host]), target)
    for n, h in enumerate(host):
        assert _same(os_[n], h[1]), (variant, n)
        for c in range(C):
            assert _same(oi[n, c], h[0][c]), (variant, n, c)
        assert all(not np.array_equal(oi[n, a], oi[n, b]) for a in range(C) for b in range(a))
    # the geometry is the one-channel test's, and so are its shares, re-asserted from the host computation
    assert np.mean([h[2] for h in host]) >= 0.10, [h[2] for h in host]
    if "affine" in variant or variant == "recipe":
        assert min(h[3] for h in host) >= 0.05
    if variant in ("rot90", "recipe"):
        assert any(h[5] != CASE_SHAPES[c] for h, c in zip(host, CASES))


@pytest.mark.parametrize("target", [(40, 48, 64), (33, 70, 45)])
def test_one_channel_launch_is_msl_augment_fit_bit_for_bit(target):
    """msl_augment_fit forwards to the C = 1 launch of the one fit kernel: this pins the forward (arena_elems as
    seg_elems, C = 1, no windows) against msl_augment_fit_mc at C = 1, on both store paths."""
    arena = _Arena(1)
    rows = fit_rows(CASES, [h[4] for h in _host("recipe", target)])
    oi, os_ = arena.launch(rows, target)
    N, V = len(CASES), int(np.prod(target))
    di = torch.empty((N,) + target, dtype=torch.float32, device=DEV)
    ds = torch.empty((N,) + target, dtype=torch.int16, device=DEV)
    _lib.call("msl_augment_fit", arena.d_img.data_ptr(), arena.d_seg.data_ptr(), arena.d_seg.numel(),
              arena.table.data_ptr(), len(CASE_SHAPES), torch.from_numpy(rows).to(DEV).data_ptr(), N, *target,
              di.data_ptr(), ds.data_ptr(), _stream())
    assert _same(oi[:, 0], di) and _same(os_, ds) and oi.any()


def test_augment_fit_mc_is_deterministic():
    target = (33, 70, 45)
    rows = fit_rows(CASES, [h[4] for h in _host("recipe", target)])
    arena = _Arena(3)
    a, b = arena.launch(rows, target), arena.launch(rows, target)
    assert _same(a[0], b[0]) and _same(a[1], b[1])


@pytest.mark.parametrize("C", [2, 3])
def test_augment_fit_mc_refuses_what_it_cannot_read(C):
    shapes = tuple(CASE_SHAPES[:2])
    arena = _Arena(C, shapes)
    total = arena.d_seg.numel()
    ident = (([0, 1, 2], [0, 0, 0]), [])
    rows = fit_rows([0, 2, -1, 1, 1], [ident] * 5)
    rows[3, 1:4] = (0, 0, 1)  # not a permutation
    oi, os_ = arena.launch(rows, (16, 16, 16))  # rows 1 .. 3: a case past the table, a negative case, a bad axis list
    assert not oi[1:4].any() and not os_[1:4].any()
    # the last case ends exactly at seg_elems: valid, and every plane of it is written
    assert all(oi[n, c].any() for n in (0, 4) for c in range(C))
    want = DS.resize_with_pad_or_crop(_data(shapes)[0][1][:C], (16, 16, 16))
    assert _same(oi[4], want)
    # one element fewer and it ends past the arena: zeros in all planes, nothing read
    oi, os_ = arena.launch(rows[[0, 4]], (16, 16, 16), seg_elems=total - 1)
    assert all(oi[0, c].any() for c in range(C)) and not oi[1].any() and not os_[1].any()
    bad = arena.table.clone()
    bad[1, 0] = total - 5  # the offset moved: the case would end past the arena
    oi, os_ = arena.launch(rows[[0, 4]], (16, 16, 16), bad)
    assert oi[0].any() and not oi[1].any() and not os_[1].any()
    for kw in ({"C": 0}, {"C": 5}):
        with pytest.raises(_lib.HipKernelError):
            arena.launch(rows[:1], (16, 16, 16), **kw)
    with pytest.raises(_lib.HipKernelError):  # N = 0
        _lib.call("msl_augment_fit_mc", arena.d_img.data_ptr(), arena.d_seg.data_ptr(), total, C, arena.table.data_ptr(), 2,
                  arena.table.data_ptr(), 0, 16, 16, 16, arena.d_img.data_ptr(), arena.d_seg.data_ptr(), _stream())


# ---- LesionCache on a two-sequence tree ------------------------------------------------------------------------------------
def _module(tmp_path, augmentations, batch=2, input_images=TWO):
    data_dir = lesion_tree_mc.make_tree(tmp_path, SHAPES) if not os.path.exists(tmp_path / "raw") else str(tmp_path / "raw")
    dm = DS.LesionsDataModule(data_dir=data_dir, centers=lesion_tree.CENTERS, batch_size=batch, spatial_size=TARGET,
                              augmentations=augmentations, input_images=input_images)
    dm.setup("fit")
    return dm


def test_cache_holds_the_cropped_cases_channel_planar(tmp_path):
    dm = _module(tmp_path, None)
    cache = LesionCache(dm, DEV)
    voxels = sum(int(np.prod(s)) for s in cache.shapes)
    assert cache.channels == 2 and cache.cache_bytes == 10 * voxels and cache.nbytes() >= 10 * voxels
    assert cache.img.numel() == 2 * voxels and cache.seg.numel() == voxels and "MiB" in cache.footprint()
    union_larger = 0
    for ds in (dm.train_dataset, dm.test_dataset):
        for i in range(len(ds)):
            img, seg = ds.load(i)
            ci, cs = DS.crop_foreground(img, seg, 5)
            di, dseg = cache.case(cache.slot[ds.subjects[i]])
            assert tuple(di.shape) == ci.shape and ci.shape[0] == 2 and ci.shape[1:] != seg.shape
            union_larger += ci.shape[1:] != DS.crop_foreground(img[0], seg, 5)[0].shape
            assert np.array_equal(dseg.cpu().numpy(), cs)
            want = np.stack([DS.normalize_nonzero(ch) for ch in ci])
            np.testing.assert_allclose(di.cpu().numpy(), want, rtol=NORM_RTOL, atol=NORM_ATOL)
    assert union_larger >= 3
    next(iter(cache.val_batches()))
    assert cache.nbytes() >= 10 * voxels + 2 * 10 * int(np.prod(TARGET))  # a batch buffer of two cases, 10 B per voxel


def test_train_batches_equal_the_host_loader_on_two_sequences(tmp_path):
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
            assert d["img"].shape == (len(d["subject"]), 2) + TARGET == h["img"].shape
            off = d["obj_off"].tolist()
            assert off[0] == 0 and len(off) == len(d["subject"]) + 1
            for n, s in enumerate(d["subject"]):
                ci, cs = cache.case(cache.slot[s])
                x, m = ci.cpu().numpy(), cs.cpu().numpy()[None]
                rs = DS.sample_rng(tr.seed, epoch, s)
                for (name, kw), (_, dr) in zip(augs, DS.draw_augmentations(augs, DS.sample_rng(tr.seed, epoch, s))):
                    x, m = DS.AUGMENTATIONS[name](x, m, rs, **kw)
                    drawn[name] = drawn.get(name, 0) + (dr is not None)
                x, m = DS.resize_with_pad_or_crop(x, TARGET), DS.resize_with_pad_or_crop(m, TARGET)[0]
                assert _same(d["seg"][n], m), (epoch, s)
                for c in range(2):
                    assert _same(d["img"][n, c], x[c]), (epoch, s, c)
                assert _same(d["gb"][off[n]:off[n + 1]], h["boxes"][n]), (epoch, s)
                assert torch.equal(d["gl"][off[n]:off[n + 1]], h["labels"][n])
                boxes_seen += off[n + 1] - off[n]
            np.testing.assert_allclose(d["img"].numpy(), h["img"].numpy(), rtol=NORM_RTOL, atol=NORM_ATOL)
    assert drawn["affine"] >= 4 and drawn["rotate90"] >= 4 and drawn["flip"] >= 2 and boxes_seen >= 16
    val_d, val_h = list(cache.val_batches()), list(dm.test_dataloader())
    assert [d["subject"] for d in val_d] == [h["subject"] for h in val_h]
    for d, h in zip(val_d, val_h):
        assert d["img"].shape == h["img"].shape and d["img"].shape[1] == 2
        np.testing.assert_allclose(d["img"].cpu().numpy(), h["img"].numpy(), rtol=NORM_RTOL, atol=NORM_ATOL)
        for n in range(len(d["subject"])):
            assert _same(d["boxes"][n], h["boxes"][n]) and torch.equal(d["labels"][n].cpu(), h["labels"][n])


# ---- the 2-channel step on a non-cube input ----------------------------------------------------------------------------------
def _hip_model(cin, size, **kw):
    from mslesions3d_amd.ssd3d import LSSD3D
    from tests.golden import detinit
    m = LSSD3D(n_classes=2, input_channels=cin, input_size=size, threshold=[0.1, 0.2], **kw)
    m.load_state_dict(detinit.fill_state_dict(m.state_dict(), 1234))
    return m.to(DEV)


def _relerr(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def test_two_channel_noncube_fused_step_against_the_oracle():
    """Stem stride (1, 2, 2) with Cin = 2 (fp32): one FusedTrainer step against the oracle on the same weights and inputs,
    at the bars tests/test_gpu_model.py::test_network_forward_backward_golden applies to the 2-channel goldens: losses
    1e-4 relative, the norm of every parameter gradient within 2e-3 relative (+ 1e-7).  The fused step hands its
    gradients straight to Adam, so they are read from the autograd route through the same kernels, and the fused step
    must leave exactly the parameters that route leaves.

    On top of that every gradient ELEMENT is held to 2e-3 of the largest reference element
    (test_full_gradients_against_oracle's bar), against the oracle run in fp64.  The fp32 oracle cannot serve for that
    on this input: its own element-wise distance from its fp64 run is 2.1e-2 (stem weight), 1.3e-2 / 7.6e-3 (stem
    BatchNorm), 1.2e-2 (block-1 bn1 bias) and 8.2e-3 (block-1 depthwise weight), 2e-4 and below elsewhere (CPU,
    measured; by norm it stays within 5.6e-4) - and the HIP gradients showed exactly those five figures against it,
    i.e. they sit on the fp64 side.  Both distances are printed."""
    from mslesions3d_amd.trainer import FusedTrainer
    from oracle import multibox as OMB
    from tests.golden import detinit
    from tests.util import oracle_model
    size, n = (48, 64, 64), 2
    x = detinit.make_volume_batch(5, n, 2, size)
    boxes, labels = detinit.make_gt(8, n, size)
    o = oracle_model(2, size).train()
    ol, osc = o(x)
    oc, olc = OMB.multibox_loss(ol, osc, boxes, labels, o.priors_cxcycz, [0.1, 0.2])
    (oc + olc).backward()
    o64 = oracle_model(2, size).double().train()
    l64, s64 = o64(x.double())
    c64, lc64 = OMB.multibox_loss(l64, s64, [b.double() for b in boxes], labels, o64.priors_cxcycz.double(), [0.1, 0.2])
    (c64 + lc64).backward()
    xd = x.to(DEV)
    a = _hip_model(2, size, lr=1e-3).train()
    [opt], [sch] = a.configure_optimizers()
    lo, sc = a(xd)
    assert _relerr(lo, ol) <= 1e-4 and _relerr(sc, osc) <= 1e-4
    cf, lc = a.loss_fn(lo, sc, [b.to(DEV) for b in boxes], [t.to(DEV) for t in labels])
    (cf + a.loss_fn.alpha * lc).backward()
    og, og64 = dict((k, p.grad) for k, p in o.named_parameters()), dict((k, p.grad) for k, p in o64.named_parameters())
    norms, elems, elems32 = [], [], []
    for k, p in a.named_parameters():
        if og[k] is None:
            assert p.grad is None
            continue
        got, ref = p.grad.double().norm().item(), og[k].double().norm().item()
        norms.append((abs(got - ref), 2e-3 * abs(ref) + 1e-7, k))
        elems.append((_relerr(p.grad, og64[k]), k))
        elems32.append((_relerr(p.grad, og[k]), k))
    print("gradient norms, largest |hip - oracle| / bound:", sorted(((d / t, k) for d, t, k in norms), reverse=True)[:3])
    print("gradient elements against the fp64 oracle:", sorted(elems, reverse=True)[:3])
    print("gradient elements against the fp32 oracle:", sorted(elems32, reverse=True)[:5])
    bad = [(k, d, t) for d, t, k in norms if d > t]
    assert len(norms) >= 10 and not bad, f"gradient norms off (name, |hip - oracle|, bound): {bad[:6]}"
    assert max(elems)[0] <= 2e-3, f"largest element-wise gradient errors against the fp64 oracle: {sorted(elems, reverse=True)[:5]}"
    sch.step()
    opt.step()
    b = _hip_model(2, size, lr=1e-3).train()
    out = FusedTrainer(b).step(xd, boxes, labels)
    print("conf", out["conf"], oc.item(), "loc", out["loc"], olc.item())
    assert abs(out["conf"] - oc.item()) <= 1e-4 * abs(oc.item())
    assert abs(out["loc"] - olc.item()) <= 1e-4 * abs(olc.item())
    assert abs(out["loss"] - (oc + olc).item()) <= 1e-4 * abs((oc + olc).item())
    for (k, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(pa, pb), f"{k} differs between the autograd and the fused step"


# ---- entry points ------------------------------------------------------------------------------------------------------------
def _run_train(tmp_path, cache):
    from mslesions3d_amd import train as T
    args = T.build_parser().parse_args(["-dm", "lesions", "-d", str(tmp_path / "raw"), "--centers", *lesion_tree.CENTERS,
                                        "--spatial_size", *map(str, TARGET), "-b", "2", "-me", "2", "-ii", *TWO,
                                        "-ld", str(tmp_path / "logs"), "-en", f"c{cache}", "-c", str(cache), "-a", *LESIONS])
    model = T.example(args)
    assert model.input_channels == 2
    return [json.loads(l) for l in open(tmp_path / "logs" / f"c{cache}" / "metrics.jsonl")]


def test_entry_points_on_two_sequences(tmp_path):
    from mslesions3d_amd import predict as P
    from mslesions3d_amd import train as T
    lesion_tree_mc.make_tree(tmp_path, SHAPES)
    host = _run_train(tmp_path, 0)
    dev = _run_train(tmp_path, 1)
    assert [sorted(r) for r in host] == [sorted(r) for r in dev]
    train = [r["total_loss/training"] for r in dev if "total_loss/training" in r]
    val = [r["avg_val_loss"] for r in dev if "avg_val_loss" in r]
    assert len(train) == 8 and len(val) == 2 and np.isfinite(train).all() and np.isfinite(val).all()
    for h, d in zip(host, dev):  # epoch 0 differs by the normalisation bound of the inputs only
        for key in ("total_loss/training", "avg_val_loss"):
            if h["epoch"] == 0 and key in h:
                print(key, h[key], d[key])
                assert abs(h[key] - d[key]) <= 1e-3 * abs(h[key])
    ckpt = str(tmp_path / "logs" / "c1" / "last.ckpt")
    common = ["-dm", "lesions", "-d", str(tmp_path / "raw"), "--centers", *lesion_tree.CENTERS, "--spatial_size",
              *map(str, TARGET), "-m", ckpt, "-ps", "test", "-o", str(tmp_path / "preds"), "-sc", "0.01"]
    metrics = P.predict_example(P.build_parser().parse_args(common + ["-ii", *TWO]))
    assert len(metrics["0.5"]) == 2
    for subj in metrics["0.5"]:
        assert os.path.exists(tmp_path / "preds" / f"sub-{subj}_preds.json") and "_CENTER_" in subj
    with pytest.raises(ValueError, match=r"input_channels=2.*1 input image"):
        P.predict_example(P.build_parser().parse_args(common + ["-ii", "FLAIR"]))
    resume = T.build_parser().parse_args(["-dm", "lesions", "-d", str(tmp_path / "raw"), "--centers", *lesion_tree.CENTERS,
                                          "--spatial_size", *map(str, TARGET), "-b", "2", "-me", "3", "-cp", ckpt,
                                          "-ld", str(tmp_path / "logs"), "-en", "resume"])
    with pytest.raises(ValueError, match=r"input_channels=2.*1 input image"):
        T.example(resume)
