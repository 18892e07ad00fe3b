"""msl_draw_boxes and msl_boxes_to_case (csrc/overlay.hip) through the C ABI against the reference's recorded volumes
and the host functions, devicedata.LesionPredictFeed against the host predict data set, and predict.py's overlay output
on both routes."""
import json
import os

import numpy as np
import pytest
import torch

from mslesions3d_amd import _lib
from mslesions3d_amd import datasets as DS
from mslesions3d_amd.devicedata import LesionCache, LesionPredictFeed, boxes_to_case_device
from mslesions3d_amd.utils import DRAW_STYLES, draw_boxes
from tests import lesion_tree, lesion_tree_mc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NORM_RTOL, NORM_ATOL = 1e-5, 1e-5  # the normalisation bound of DESIGN.md §4.7 (tests/test_gpu_lesions.py)
GUARD, SENTINEL = 4096, 0x5AA5
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "overlay.npz"))
CASES = [str(n) for n in GOLD["names"]]
CHUNK = _lib.DRAW_BOXES_CHUNK


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _draw(per_image, shape, style, min_score, classes=True, offsets=None, expect_rc=0, shift=0):
    """One msl_draw_boxes call on sentinel-filled planes between guard bands -> (instances, classes or None) on the host, or
    None after checking that nothing was written when a refusal is expected.  ``shift``: elements the instance plane starts
    past a 16-byte boundary."""
    N, V = len(per_image), int(np.prod(shape))
    b = np.concatenate([np.asarray(p[0], np.float32).reshape(-1, 6) for p in per_image])
    l = np.concatenate([np.asarray(p[1], np.int64).reshape(-1) for p in per_image])
    s = np.concatenate([np.asarray(p[2], np.float32).reshape(-1) for p in per_image])
    off = np.concatenate([[0], np.cumsum([np.asarray(p[1]).size for p in per_image])]).astype(np.int32) if offsets is None \
        else np.asarray(offsets, np.int32)
    db, dl, ds = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (b, l, s))
    bufs = [torch.full((N * V + 2 * GUARD + 8,), SENTINEL, dtype=torch.int16, device=DEV) for _ in range(2)]
    shifts = (shift, (3 * shift) % 8)  # 1 -> (1, 3) and 3 -> (3, 1): the class plane on another alignment; 4 -> (4, 4)
    planes = [buf[GUARD + sh:GUARD + sh + N * V] for buf, sh in zip(bufs, shifts)]
    fn = _lib.load().msl_draw_boxes
    rc = fn(db.data_ptr() if b.size else None, dl.data_ptr() if l.size else None, ds.data_ptr() if s.size else None,
            off.ctypes.data, N, *shape, style if isinstance(style, int) else DRAW_STYLES[style], float(min_score),
            planes[0].data_ptr(), planes[1].data_ptr() if classes else None, _stream())
    torch.cuda.synchronize()
    assert rc == expect_rc
    host = [buf.cpu().numpy() for buf in bufs]
    for h, sh in zip(host, shifts):
        assert (h[:GUARD + sh] == SENTINEL).all() and (h[GUARD + sh + N * V:] == SENTINEL).all(), "guard band overwritten"
    body = [h[GUARD + sh:GUARD + sh + N * V].reshape((N,) + tuple(shape)) for h, sh in zip(host, shifts)]
    if expect_rc != 0:
        assert (body[0] == SENTINEL).all() and (body[1] == SENTINEL).all()
        return None
    if not classes:
        assert (body[1] == SENTINEL).all()
    return body[0], (body[1] if classes else None)


def _gold(name):
    return (GOLD[f"{name}__boxes"], GOLD[f"{name}__labels"], GOLD[f"{name}__scores"]), \
        tuple(int(v) for v in GOLD[f"{name}__shape"]), float(GOLD[f"{name}__min_score"])


# ---- msl_draw_boxes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_draw_boxes_equals_the_reference_volumes(name):
    det, shape, min_score = _gold(name)
    runs = [_draw([det], shape, "edges", 0.0) for _ in range(2)]
    assert np.array_equal(runs[0][0][0], GOLD[f"{name}__edges_instances"])
    assert np.array_equal(runs[0][1][0], GOLD[f"{name}__edges_classes"])
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    runs = [_draw([det], shape, "preds", min_score) for _ in range(2)]
    assert np.array_equal(runs[0][0][0], GOLD[f"{name}__preds_instances"])
    assert np.array_equal(runs[0][1][0], draw_boxes(*det, shape, "preds", min_score)[1])
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])


def _random_detections(rs, k, min_score):
    lo = rs.uniform(-0.3, 1.0, (k, 3))
    boxes = np.concatenate([lo, lo + rs.uniform(0.0, 0.6, (k, 3))], 1).astype(np.float32)
    if k >= 2:
        boxes[0] = [1.2, 1.3, 1.1, 1.6, 1.7, 1.8]     # wholly above 1
        boxes[1] = [-0.9, -0.8, -0.7, -0.1, -0.2, -0.3]  # wholly below 0
    scores = rs.uniform(0.0, 1.0, k).astype(np.float32)
    scores[::3] = min_score  # equal to the threshold: the test is <, these are kept
    return boxes, rs.randint(0, 3, k).astype(np.int64), scores


# rows shorter than a store and odd W; W % 8 = 4; aligned rows; a row wider than 256; a row of more than 64 chunks (two
# trips of the kernel's chunk loop)
SHAPES = [(5, 7, 9), (12, 16, 20), (8, 8, 64), (3, 4, 264), (2, 3, 530)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("style", ["edges", "preds"])
def test_draw_boxes_equals_the_host_on_random_input(shape, style):
    rs = np.random.RandomState(sum(shape) + len(style))
    min_score = float(np.float32(0.4))
    for counts in ([0], [1], [2], [37], [CHUNK + 1], [37, 0, 2], [1, CHUNK + 1, 5]):
        per_image = [_random_detections(rs, k, min_score) for k in counts]
        want = [draw_boxes(*p, shape, style, min_score) for p in per_image]
        for classes in (True, False):
            runs = [_draw(per_image, shape, style, min_score, classes=classes) for _ in range(2)]
            for n in range(len(counts)):
                assert np.array_equal(runs[0][0][n], want[n][0]), (counts, n)
                if classes:
                    assert np.array_equal(runs[0][1][n], want[n][1]), (counts, n)
            assert np.array_equal(runs[0][0], runs[1][0])
    assert any(w[0].any() for w in want)


@pytest.mark.parametrize("shift", [1, 3, 4])
def test_draw_boxes_on_planes_off_a_16_byte_boundary(shift):
    rs = np.random.RandomState(shift)
    per_image = [_random_detections(rs, 20, 0.4), _random_detections(rs, 9, 0.4)]
    for shape in ((6, 5, 40), (4, 6, 13)):
        got = _draw(per_image, shape, "preds", 0.4, shift=shift)
        for n, p in enumerate(per_image):
            want = draw_boxes(*p, shape, "preds", 0.4)
            assert np.array_equal(got[0][n], want[0]) and np.array_equal(got[1][n], want[1])


def test_draw_boxes_refuses_bad_arguments_and_writes_nothing():
    rs = np.random.RandomState(1)
    det = _random_detections(rs, 5, 0.4)
    shape = (6, 7, 9)
    for style in (2, -1):
        _draw([det], shape, style, 0.4, expect_rc=-1)
    for bad in ((0, 7, 9), (6, 0, 9), (6, 7, 0), (6, 7, -3)):
        N, V = 1, 6 * 7 * 9
        bufs = torch.full((V + 2 * GUARD,), SENTINEL, dtype=torch.int16, device=DEV)
        off = np.asarray([0, 0], np.int32)
        rc = _lib.load().msl_draw_boxes(None, None, None, off.ctypes.data, N, *bad, 0, 0.0, bufs[GUARD:].data_ptr(), None, _stream())
        torch.cuda.synchronize()
        assert rc == -1 and bool((bufs == SENTINEL).all())
    _draw([det, det], shape, "edges", 0.4, offsets=[0, 7, 5], expect_rc=-1)   # decreasing
    _draw([det, det], shape, "edges", 0.4, offsets=[-1, 5, 10], expect_rc=-1)  # negative
    many = (np.zeros((32767, 6), np.float32), np.ones(32767, np.int64), np.ones(32767, np.float32))
    _draw([many], shape, "edges", 0.4, expect_rc=-1)                           # j + 1 would not fit int16
    with pytest.raises(_lib.HipKernelError):
        _lib.call("msl_draw_boxes", None, None, None, np.asarray([0, 0], np.int32).ctypes.data, 1, 4, 4, 4, 3, 0.0,
                  torch.zeros(64, dtype=torch.int16, device=DEV).data_ptr(), None, _stream())


# ---- msl_boxes_to_case --------------------------------------------------------------------------------------------------
GEOMETRY = [((48, 64, 30), (41, 80, 30), (3, 0, 9), (50, 91, 47)),     # pad, crop, equal
            ((250, 300, 300), (160, 190, 301), (11, 7, 0), (182, 218, 301)),
            ((33, 70, 45), (60, 50, 45), (0, 4, 2), (71, 60, 50)),
            ((16, 16, 16), (16, 17, 15), (1, 1, 1), (20, 20, 20))]


def test_boxes_to_case_equals_the_host_bit_for_bit():
    rs = np.random.RandomState(11)
    counts = [70, 0, 90, 40]
    boxes = [rs.uniform(-0.4, 1.4, (k, 6)).astype(np.float32) for k in counts]
    packed = np.concatenate(boxes)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    geo = np.asarray([sum(map(list, g), []) for g in GEOMETRY], np.int32)
    buf = torch.full((packed.size + 2 * GUARD,), -77.0, dtype=torch.float32, device=DEV)
    out = buf[GUARD:GUARD + packed.size]
    runs = []
    for _ in range(2):
        out.fill_(-77.0)
        _lib.call("msl_boxes_to_case", torch.from_numpy(packed).to(DEV).data_ptr(), off.ctypes.data, geo.ctypes.data, 4,
                  out.data_ptr(), _stream())
        host = buf.cpu().numpy()
        assert (host[:GUARD] == -77.0).all() and (host[GUARD + packed.size:] == -77.0).all()
        runs.append(host[GUARD:GUARD + packed.size].reshape(-1, 6).copy())
    assert np.array_equal(runs[0].view(np.int32), runs[1].view(np.int32))
    for n, g in enumerate(GEOMETRY):
        want = DS.fit_to_case_frame(boxes[n], *g)
        assert np.array_equal(runs[0][off[n]:off[n + 1]].view(np.int32), want.view(np.int32)), n
    assert packed.min() < 0 and packed.max() > 1
    got = boxes_to_case_device([torch.from_numpy(b).to(DEV) for b in boxes], *zip(*GEOMETRY))
    assert all(np.array_equal(g.cpu().numpy().view(np.int32), runs[0][off[n]:off[n + 1]].view(np.int32)) for n, g in enumerate(got))
    bad = geo.copy()
    bad[0, 9] = 0
    for o, g in ((np.asarray([0, 5, 3, 6, 7], np.int32), geo), (off, bad)):
        out.fill_(-77.0)
        rc = _lib.load().msl_boxes_to_case(torch.from_numpy(packed).to(DEV).data_ptr(), o.ctypes.data, g.ctypes.data, 4,
                                           out.data_ptr(), _stream())
        torch.cuda.synchronize()
        assert rc == -1 and bool((buf == -77.0).all())


# ---- LesionPredictFeed --------------------------------------------------------------------------------------------------
CASE_SHAPES = [(40, 44, 50), (52, 48, 46), (44, 70, 52), (60, 50, 72), (48, 64, 64), (42, 42, 42), (50, 45, 58),
               (46, 66, 49), (41, 51, 61), (55, 47, 43)]
TARGET = (48, 64, 64)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("channels", [1, 2])
def test_predict_feed_equals_the_host_predict_dataset(tmp_path, channels):
    if channels == 1:
        data_dir, names = lesion_tree.make_tree(tmp_path, CASE_SHAPES[:6]), ("FLAIR",)
    else:
        names = lesion_tree_mc.SEQUENCES[:2]
        data_dir = lesion_tree_mc.make_tree(tmp_path, CASE_SHAPES[:6], names)
    dm = DS.LesionsDataModule(data_dir=data_dir, centers=lesion_tree.CENTERS, batch_size=1, spatial_size=TARGET,
                              input_images=names)
    dm.setup("predict_train")
    ds = dm.predict_dataset
    feed = LesionPredictFeed(dm, DEV)
    assert len(feed) == len(ds) >= 4
    got = [dict(b, img=b["img"].cpu()) for b in feed]
    boxes_seen = 0
    for i, b in enumerate(got):
        h = DS.collate_fn([ds[i]])
        assert b["subject"] == h["subject"] and b["img"].shape == (1, channels) + TARGET
        np.testing.assert_allclose(b["img"].numpy(), h["img"].numpy(), rtol=NORM_RTOL, atol=NORM_ATOL)
        assert _same_bits(b["boxes"][0].cpu().numpy(), h["boxes"][0].numpy())
        assert torch.equal(b["labels"][0].cpu(), h["labels"][0])
        for key in DS.GEOMETRY_KEYS:
            assert [tuple(v) for v in b[key]] == [tuple(v) for v in h[key]], key
        boxes_seen += len(h["labels"][0])
    assert boxes_seen >= 6
    order = [3, 0, 2]
    assert [b["subject"][0] for b in feed.batches(order)] == [ds.subjects[i] for i in order]
    # LesionCache.val_batches carries the same geometry
    dm.setup("fit")
    for b in LesionCache(dm, DEV).val_batches():
        for n, subj in enumerate(b["subject"]):
            s = dm.test_dataset[dm.test_dataset.subjects.index(subj)]
            assert all(tuple(b[key][n]) == tuple(s[key]) for key in DS.GEOMETRY_KEYS)


# ---- end to end ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """(root of a lesion tree, checkpoint of a 2-epoch run on it), made once for the module."""
    from mslesions3d_amd import train as T
    tmp_path = tmp_path_factory.mktemp("overlay")
    lesion_tree.make_tree(tmp_path, CASE_SHAPES)
    args = T.build_parser().parse_args(["-dm", "lesions", "-d", str(tmp_path / "raw"), "--centers", *lesion_tree.CENTERS,
                                        "--spatial_size", *map(str, TARGET), "-b", "2", "-me", "2",
                                        "-ld", str(tmp_path / "logs"), "-en", "ck", "-c", "1"])
    T.example(args)
    return tmp_path, str(tmp_path / "logs" / "ck" / "last.ckpt")


def _predict(tmp_path, ckpt, out, *extra):
    from mslesions3d_amd import predict as P
    args = P.build_parser().parse_args(["-dm", "lesions", "-d", str(tmp_path / "raw"), "--centers", *lesion_tree.CENTERS,
                                        "--spatial_size", *map(str, TARGET), "-m", ckpt, "-ps", "test",
                                        "-o", str(tmp_path / out), "-sc", "0.01", *extra])
    return P.predict_example(args)


def _volume_from_json(infos, n_rows, shape, min_score):
    """utils.draw_boxes on a sub-*_preds*.json's own boxes: row j of the detections is key j + 1; absent rows are skipped
    ones (label 0 here)."""
    boxes, labels, scores = np.zeros((n_rows, 6), np.float32), np.zeros(n_rows, np.int64), np.zeros(n_rows, np.float32)
    for key, (frac, _, label, score) in infos.items():
        boxes[int(key) - 1], labels[int(key) - 1], scores[int(key) - 1] = np.asarray(frac, np.float32), label, np.float32(score)
    return draw_boxes(boxes, labels, scores, shape, "preds", min_score)[0]


def test_predict_writes_case_frame_overlays_on_both_routes(trained):
    tmp_path, ckpt = trained
    _predict(tmp_path, ckpt, "plain")
    plain = sorted(os.listdir(tmp_path / "plain"))
    subjects = [f[len("sub-"):-len("_preds.json")] for f in plain if f.endswith("_preds.json")]
    # without -si and --cache: the files of the parent commit, and nothing else
    assert plain == sorted([f"sub-{s}_preds.{e}" for s in subjects for e in ("json", "csv")] +
                           [f"aa_metrics_per_subject_(min_IoU={i}).json" for i in (0.5, 0.1)]) and len(subjects) == 2
    dm = DS.LesionsDataModule(data_dir=str(tmp_path / "raw"), centers=lesion_tree.CENTERS, batch_size=1, spatial_size=TARGET)
    dm.setup("predict")
    geometry = {"_".join(s): dm.predict_dataset[i] for i, s in enumerate(dm.predict_dataset.subjects)}
    volumes = {}
    for route, extra in (("dev", ["--cache", "1", "-si", "1", "-mn", "run"]), ("host", ["-si", "1", "-mn", "run"])):
        _predict(tmp_path, ckpt, route, *extra)
        out = tmp_path / route / "run"
        assert sorted(os.listdir(out)) == sorted(plain + [f"sub-{s}_preds{e}" for s in subjects for e in (".npy", "_case.json")])
        for s in subjects:
            g = geometry[s]
            vol = np.load(out / f"sub-{s}_preds.npy")
            assert vol.dtype == np.int16 and vol.shape == tuple(g["full_shape"]) != TARGET
            fitted = json.load(open(out / f"sub-{s}_preds.json"))
            case = json.load(open(out / f"sub-{s}_preds_case.json"))
            n_rows = len(open(out / f"sub-{s}_preds.csv").read().strip().splitlines()) - 1
            assert list(case) == list(fitted) and len(fitted) >= 1
            frac = np.asarray([v[0] for v in fitted.values()], np.float32).reshape(-1, 6)
            want = DS.fit_to_case_frame(frac, TARGET, g["crop_shape"], g["crop_origin"], g["full_shape"])
            assert _same_bits(np.asarray([v[0] for v in case.values()], np.float32).reshape(-1, 6), want)
            assert [v[2:] for v in case.values()] == [v[2:] for v in fitted.values()]
            assert np.array_equal(vol, _volume_from_json(case, n_rows, g["full_shape"], 0.01)) and vol.any()
            volumes[route, s] = (vol, fitted)
    # the keep-lists of the two routes may differ at the score threshold (not asserted): report them
    for s in subjects:
        print(s, "device route keeps", len(volumes["dev", s][1]), "host route keeps", len(volumes["host", s][1]))
    # the host route's fitted-frame files are the plain run's, byte for byte
    for f in plain:
        assert open(tmp_path / "host" / "run" / f).read() == open(tmp_path / "plain" / f).read(), f


def test_head_outputs_of_the_device_built_batch_agree_with_the_host_built_one(trained):
    from mslesions3d_amd.ssd3d import LSSD3D
    tmp_path, ckpt = trained
    dm = DS.LesionsDataModule(data_dir=str(tmp_path / "raw"), centers=lesion_tree.CENTERS, batch_size=1, spatial_size=TARGET)
    dm.setup("predict")
    model = LSSD3D.load_from_checkpoint(ckpt).to(DEV).eval()
    with torch.no_grad():
        for i, b in enumerate(LesionPredictFeed(dm, DEV)):
            dev_out = [t.clone() for t in model(b["img"].clone())]
            host_out = model(DS.collate_fn([dm.predict_dataset[i]])["img"].to(DEV))
            for d, h in zip(dev_out, host_out):
                err, scale = float((d - h).abs().max()), float(h.abs().max())
                print("head output: max abs difference", err, "of", scale)
                assert err <= 1e-3 * scale
