"""msl_prior_fit on the device (csrc/priorfit.hip): every case of tests/priorfit_cases.py bit for bit
against the loop around the oracle's ``match_image`` (tests/priorfit_ref.py), the same counts from the existing device matcher,
repeatability, ``LSSD3D.prior_fit`` and ``python -m mslesions3d_amd.insight`` as a child process."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import priorfit_cases as C
from tests.priorfit_ref import reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {c["name"]: c for c in C.cases()}
KEYS = ("best_iou", "best_prior", "held", "pos", "image")


@functools.lru_cache(maxsize=None)
def _device_priors(name):
    """The prior set from msl_make_priors, checked against the numpy restatement the reference uses."""
    from mslesions3d_amd import _lib
    s = C.PRIOR_SETS[name]
    want, off = C.prior_set(name)
    dims, scales = C.fmap_dims(s["input"], max(s["layers"])), C.default_scales(s["input"], s["layers"])
    out = torch.empty((s["P"], 6), dtype=torch.float32, device=DEV)
    for f, lo in zip(s["layers"], off[:-1]):
        _lib.call("msl_make_priors", out.data_ptr(), int(lo), *dims[f], float(scales[f]), 2, torch.cuda.current_stream().cuda_stream)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))
    return out, want, off


@functools.lru_cache(maxsize=None)
def _reference(name):
    c = CASES[name]
    _, pri, off = _device_priors(c["set"])
    return reference(c["images"], pri, c["thresholds"], C.case_split(c, off))


def _ranges(off):
    return [(int(a), int(b)) for a, b in zip(off[:-1], off[1:])]


def _fit(name):
    from mslesions3d_amd.utils import prior_fit
    c = CASES[name]
    dpri, _, off = _device_priors(c["set"])
    return prior_fit(c["images"], dpri, c["thresholds"], _ranges(C.case_split(c, off)))


def _assert_same(got, want, what):
    for k in KEYS:
        g, w = got[k].numpy() if torch.is_tensor(got[k]) else got[k], want[k]
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        if k == "best_iou":
            assert g.dtype == np.float32 and np.array_equal(g.view(np.uint32), w.view(np.uint32)), (what, k, g, w)
        else:
            assert np.array_equal(g, w), (what, k, g, w)


@pytest.mark.parametrize("name", list(CASES))
def test_prior_fit_matches_the_reference(name):
    got, want = _fit(name), _reference(name)
    _assert_same(got, want, name)
    off = C.case_split(CASES[name], _device_priors(CASES[name]["set"])[2])
    assert np.array_equal(got["best_scale"].numpy(), np.searchsorted(off, want["best_prior"], side="right") - 1)


@pytest.mark.parametrize("name", ["forced_prior_taken", "zero_volume", "random_65_a", "thr8_four_ranges_b", "random_131_b"])
def test_positive_counts_agree_with_the_device_matcher(name):
    """sum_s pos[g, t, s] from msl_multibox_match: true_classes > 0 grouped by matched, per image and threshold."""
    from mslesions3d_amd import _lib
    from mslesions3d_amd.ssd3d import MultiBoxLoss
    c = CASES[name]
    dpri, _, _ = _device_priors(c["set"])
    P, N = dpri.shape[0], len(c["images"])
    got = _fit(name)["pos"].numpy().sum(2)
    boxes = [torch.from_numpy(b) for b in c["images"]]
    gb, gl, off, G = MultiBoxLoss.pack_targets(boxes, [torch.ones(b.shape[0], dtype=torch.int64) for b in boxes], DEV)
    sizes = [b.shape[0] for b in boxes]
    first = np.concatenate([[0], np.cumsum(sizes)])
    overlap = torch.empty((N, P), dtype=torch.float32, device=DEV)
    obj = torch.empty((N, P), dtype=torch.int32, device=DEV)
    pfo = torch.empty(max(G, 1), dtype=torch.int32, device=DEV)
    tc = torch.empty((N, P), dtype=torch.int64, device=DEV)
    tl = torch.empty((N, P, 6), dtype=torch.float32, device=DEV)
    matched = torch.empty((N, P), dtype=torch.int64, device=DEV)
    for t, thr in enumerate(c["thresholds"]):
        _lib.call("msl_multibox_match", gb.data_ptr(), gl.data_ptr(), off.data_ptr(), G, dpri.data_ptr(), N, P, float(thr), 0.0, 0,
                  overlap.data_ptr(), obj.data_ptr(), pfo.data_ptr(), tc.data_ptr(), tl.data_ptr(), matched.data_ptr(),
                  torch.cuda.current_stream().cuda_stream)
        want = np.zeros(G, dtype=np.int64)
        for n in range(N):
            if sizes[n]:
                want[first[n]:first[n + 1]] = torch.bincount(matched[n][tc[n] > 0], minlength=sizes[n]).cpu().numpy()
        assert np.array_equal(got[:, t], want), (name, thr)


def _raw(c, stream=None, **over):
    """One raw msl_prior_fit call -> (return code, the output buffer's bytes)."""
    from mslesions3d_amd import _lib
    from mslesions3d_amd.utils import prepare_prior_fit
    dpri, _, off = _device_priors(c["set"])
    plan = prepare_prior_fit(c["images"], torch.device(DEV))
    off = np.ascontiguousarray(over.pop("off", C.case_split(c, off)), dtype=np.int32)
    thr = np.asarray(over.pop("thr", c["thresholds"]), dtype=np.float32)
    G, S, T = plan["G"], off.size - 1, thr.size
    ws = torch.zeros(max(G, 1), dtype=torch.int64, device=DEV)
    out = torch.full((max(G, 1) * (3 + 64),), -7, dtype=torch.int32, device=DEV)
    b = out.data_ptr()
    args = dict(gt=plan["gb"].data_ptr(), off=plan["off"].data_ptr(), N=plan["N"], G=G, pri=dpri.data_ptr(), P=int(dpri.shape[0]),
                so=off.ctypes.data, S=S, thr=thr.ctypes.data, T=T, ws=ws.data_ptr(), wsb=8 * G, o0=b, o1=b + 4 * G, o2=b + 8 * G,
                o3=b + 12 * G)
    args.update(over)
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream.cuda_stream
    rc = _lib.load().msl_prior_fit(*[ctypes.c_void_p(v) if k in ("gt", "off", "pri", "so", "thr", "ws", "o0", "o1", "o2", "o3") else v
                                     for k, v in args.items()], ctypes.c_void_p(st))
    torch.cuda.synchronize()
    return rc, out.cpu().numpy().tobytes()


def test_two_calls_and_a_side_stream_return_equal_bytes():
    c = CASES["thr8_four_ranges_b"]
    rc0, a = _raw(c)
    rc1, b = _raw(c)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    rc2, s = _raw(c, stream=side)
    assert rc0 == rc1 == rc2 == 0 and a == b == s
    G = sum(x.shape[0] for x in c["images"])
    got = np.frombuffer(a, dtype=np.int32)
    assert np.array_equal(got[G:2 * G], _reference(c["name"])["best_prior"])
    assert (got[G * (3 + 8 * 4):] == -7).all()  # nothing is written past pos


def test_capacity_and_argument_codes():
    c = CASES["thr1_one_range_a"]
    P = C.PRIOR_SETS["a"]["P"]
    assert _raw(c)[0] == 0
    nine = np.linspace(0, P, 10).astype(np.int32)
    assert nine[0] == 0 and nine[-1] == P
    assert _raw(c, off=nine)[0] == -2                                   # S = 9
    assert _raw(c, thr=np.linspace(0.1, 0.9, 9))[0] == -2               # n_thr = 9
    assert _raw(c, off=nine[:9].tolist()[:8] + [P])[0] == 0             # S = 8 is served
    assert _raw(c, pri=None)[0] == -1                                   # a null pointer
    assert _raw(c, o3=None)[0] == -1
    assert _raw(c, off=[0, P - 1])[0] == -1                             # the ranges do not end at P
    assert _raw(c, off=[0, 100, 50, P])[0] == -1                        # not ascending
    assert _raw(c, wsb=8)[0] == -1                                      # workspace too small
    rc, raw = _raw(CASES["no_objects_a"], gt=None, ws=None, o0=None, o1=None, o2=None, o3=None)
    assert rc == 0 and (np.frombuffer(raw, dtype=np.int32) == -7).all()  # G = 0 is legal and writes nothing


def test_model_prior_fit_32():
    from mslesions3d_amd.ssd3d import LSSD3D
    c = CASES["random_65_a"]
    model = LSSD3D(n_classes=2, input_channels=1, input_size=(32, 32, 32), threshold=[0.1, 0.2],
                   aspect_ratios={3: [1.], 5: [1.], 7: [1.]})
    assert model.prior_ranges() == {3: (0, 128), 5: (128, 144), 7: (144, 146)}
    assert np.array_equal(model.priors_cxcycz.cpu().numpy(), C.prior_set("a")[0])
    fit, summary = model.prior_fit(c["images"], size_edges=(27, 125))
    _assert_same(fit, _reference("random_65_a"), "model")
    rows = summary["thresholds"][1]["strata"]
    assert summary["scales"] == ["3", "5", "7"] and rows[0]["lesions"] == 65 == sum(r["lesions"] for r in rows[1:])
    want = _reference("random_65_a")
    assert rows[0]["orphaned"] == int((want["pos"][:, 1].sum(1) == 0).sum())
    assert rows[0]["matchable"] == int((want["best_iou"] >= np.float32(0.2)).sum())
    with pytest.raises(ValueError):
        model.prior_fit([np.full((1, 6), np.nan, np.float32)])


def test_insight_entry_point(tmp_path):
    from mslesions3d_amd import datasets as DS
    from mslesions3d_amd.utils import prior_fit_summary
    data = str(tmp_path / "data")
    DS.generate_artificial_dataset(data, "toy", num_images=12, image_size=(32, 32, 32), object_size=(4, 8))
    ds = DS.ExampleDataset(n_classes=1, percentage=1., num_workers=0, data_dir=data, dataset_name="toy")
    ds.setup(stage="predict_train")
    boxes = [b.numpy() for batch in ds._loader(ds.predict_dataset, False, 32) for b in batch["boxes"]]
    G = sum(b.shape[0] for b in boxes)
    out = tmp_path / "out"
    cmd = [sys.executable, "-m", "mslesions3d_amd.insight", "-d", data, "-dn", "toy", "-ps", "train", "-th", "0.1", "0.2",
           "--scale_factors", "0.5,1,2", "--size_bins", "27,125", "--draw_priors", "1", "-o", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    rep = json.loads((out / "prior_fit.json").read_text())
    pri, off = C.prior_set("a")
    assert rep["n_priors"] == 146 and rep["input_size"] == [32, 32, 32] and [b["factor"] for b in rep["sweep"]] == [0.5, 1.0, 2.0]
    ref = reference(boxes, pri, [0.1, 0.2], off)
    want = prior_fit_summary(ref, boxes, 32 ** 3, [27, 125], [0.1, 0.2], shapes=(32, 32, 32), scale_names=[3, 5, 7])
    assert rep["sweep"][1]["fit"] == json.loads(json.dumps(want)) == rep["fit"]
    for t in rep["fit"]["thresholds"]:
        assert t["strata"][0]["lesions"] == G == sum(s["lesions"] for s in t["strata"][1:])
    assert rep["suggested"] in (0.5, 1.0, 2.0)
    # the other factors against the reference on the scaled priors
    for blk in (rep["sweep"][0], rep["sweep"][2]):
        sc = {f: v * blk["factor"] for f, v in C.default_scales((32, 32, 32), (3, 5, 7)).items()}
        ref_f = reference(boxes, C.priors_numpy((32, 32, 32), (3, 5, 7), sc)[0], [0.1, 0.2], off)
        assert blk["fit"] == json.loads(json.dumps(prior_fit_summary(ref_f, boxes, 32 ** 3, [27, 125], [0.1, 0.2],
                                                                     shapes=(32, 32, 32), scale_names=[3, 5, 7])))
    drawn = sorted(p.name for p in out.glob("sub-*_prior-boxes_fmap-*.npy"))
    assert len(drawn) == 3 and np.load(out / drawn[0]).shape == (32, 32, 32)
