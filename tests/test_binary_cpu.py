"""Binary lesion masks without a GPU: the --segmentation flag of the four command lines, a numpy model of the run-based
labelling msl_binary_boxes performs (checked against scipy.ndimage.label plus the host walk), and the host arithmetic of
its workspace."""
import os

import numpy as np
import pytest
import torch

from mslesions3d_amd import _lib
from mslesions3d_amd import datasets as DS
from tests import lesion_tree_binary

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "instances.npz"))
BINARY_CASES = [str(n) for n in GOLD["names"] if str(GOLD[f"{n}__mode"]) == "binary"]
ONE = [(1, np.inf)]


# ---- command lines -----------------------------------------------------------------------------------------------------
def _parsers():
    from mslesions3d_amd import eval as E
    from mslesions3d_amd import insight as I
    from mslesions3d_amd import predict as P
    from mslesions3d_amd import train as T
    return {"train": T.build_parser(), "predict": P.build_parser(), "eval": E.build_parser(), "insight": I.build_parser()}


@pytest.mark.parametrize("tool", ["train", "predict", "eval", "insight"])
def test_parsers_take_the_segmentation_name(tool, tmp_path):
    from mslesions3d_amd import eval as E
    from mslesions3d_amd.train import segmentation_of
    data_dir = lesion_tree_binary.make_tree(tmp_path, [(40, 44, 50), (41, 40, 42)])
    parser = _parsers()[tool]
    args = parser.parse_args(["-dm", "lesions", "--segmentation", lesion_tree_binary.BINARY])
    opt = E.eval_options(args) if tool == "eval" else args
    assert segmentation_of(opt) == lesion_tree_binary.BINARY
    dm = DS.LesionsDataModule(data_dir=data_dir, centers=lesion_tree_binary.CENTERS, segmentation=segmentation_of(opt))
    assert dm.segmentation_mode == "binary" and dm.thresholds == ONE
    plain = parser.parse_args(["-dm", "lesions"])
    plain = E.eval_options(plain) if tool == "eval" else plain
    assert segmentation_of(plain) == "labeled_lesions"
    if tool == "eval":  # a flag that is not given leaves no attribute behind
        assert not hasattr(parser.parse_args([]), "segmentation")
    refused = parser.parse_args(["-dm", "example", "--segmentation", "x"])
    with pytest.raises(ValueError, match="segmentation"):
        segmentation_of(E.eval_options(refused) if tool == "eval" else refused)


def test_example_module_refuses_a_segmentation_before_any_gpu_call(monkeypatch):
    from mslesions3d_amd import eval as E
    from mslesions3d_amd import insight as I
    from mslesions3d_amd import predict as P
    from mslesions3d_amd import train as T

    def no_gpu(*a, **k):
        raise AssertionError("a GPU call before the command line was refused")
    monkeypatch.setattr(torch.cuda, "set_device", no_gpu)
    flags = ["-dm", "example", "--segmentation", "x"]
    with pytest.raises(ValueError, match="segmentation"):
        T.example(T.build_parser().parse_args(flags))
    with pytest.raises(ValueError, match="segmentation"):
        P.predict_example(P.build_parser().parse_args(flags))
    with pytest.raises(ValueError, match="segmentation"):
        E.main(flags)
    with pytest.raises(ValueError, match="segmentation"):
        I.check_options(I.build_parser().parse_args(flags))


def test_binary_tree_differs_from_its_instances(tmp_path):
    """The fixture's touching pair: two instance boxes, one binary box."""
    _, inst, binary = lesion_tree_binary.make_case(0, (40, 44, 50))
    bi, _ = DS.boxes_from_instances(inst, ONE, "instances")
    bb, _ = DS.boxes_from_instances(binary, ONE, "binary")
    assert len(bb) < len(bi)


# ---- the run-based labelling, in numpy ---------------------------------------------------------------------------------
def run_components(seg):
    """The algorithm of msl_binary_boxes: runs of non-zero voxels per row in raster order; every run is united with the
    runs of rows y-1 and z-1 that share a column, larger root under smaller; extents folded into the roots.
    -> (inclusive extents of the components in root order, first voxel of every root)."""
    D, H, W = seg.shape
    rows = (np.asarray(seg) != 0).reshape(D * H, W)
    runs, rowoff = [], [0]
    for r in range(D * H):
        d = np.diff(np.concatenate([[0], rows[r].astype(np.int8), [0]]))
        runs += [(r, int(a), int(b)) for a, b in zip(np.flatnonzero(d == 1), np.flatnonzero(d == -1) - 1)]
        rowoff.append(len(runs))
    link = list(range(len(runs)))

    def find(i):
        while link[i] != i:
            i = link[i]
        return i

    for i, (r, x0, x1) in enumerate(runs):
        y, z = r % H, r // H
        for q in ([r - 1] if y > 0 else []) + ([r - H] if z > 0 else []):
            for j in range(rowoff[q], rowoff[q + 1]):
                if runs[j][1] <= x1 and runs[j][2] >= x0:
                    a, b = find(i), find(j)
                    if a != b:
                        link[max(a, b)] = min(a, b)
    ext = {}
    for i, (r, x0, x1) in enumerate(runs):
        y, z = r % H, r // H
        e = ext.setdefault(find(i), [z, y, x0, z, y, x1])
        e[:] = [min(e[0], z), min(e[1], y), min(e[2], x0), max(e[3], z), max(e[4], y), max(e[5], x1)]
    roots = sorted(ext)
    return [ext[k] for k in roots], [(runs[k][0] // H, runs[k][0] % H, runs[k][1]) for k in roots]


def run_boxes(seg):
    extents, _ = run_components(seg)
    if not (np.asarray(seg) == 0).any():
        extents = extents[1:]  # np.unique(...)[1:] on a mask without background
    boxes, keep = DS._fractional_boxes(extents, seg.shape)
    return boxes[keep] if boxes.numel() else boxes


def _bits(t):
    return np.ascontiguousarray(t.numpy() if torch.is_tensor(t) else t).view(np.int32)


def _random_masks():
    rs = np.random.RandomState(11)
    shapes = [(9, 12, 40), (7, 9, 11), (2, 2, 2), (5, 8, 33), (3, 5, 17), (8, 8, 8), (2, 6, 20), (6, 2, 23), (6, 7, 2)]  # (the host walk squeezes axes of one voxel)
    out = []
    for k in range(21):
        shape, p = shapes[k % len(shapes)], (0.02, 0.08, 0.3, 0.6, 0.95, 1.0, 0.0)[k % 7]
        seg = (rs.rand(*shape) < p).astype(np.int16)
        if k % 4 == 0:
            seg = seg * rs.randint(-5, 6, shape).astype(np.int16)  # negative values are foreground, zeros background
        out.append(seg)
    return out


@pytest.mark.parametrize("name", BINARY_CASES)
def test_run_model_reproduces_the_goldens(name):
    assert len(BINARY_CASES) == 3
    got = run_boxes(GOLD[f"{name}__seg"])
    assert np.array_equal(_bits(got).reshape(-1, 6), _bits(GOLD[f"{name}__boxes"]).reshape(-1, 6))


def test_run_model_numbers_components_as_scipy_does():
    from scipy.ndimage import label
    seen = 0
    for seg in _random_masks() + [GOLD[f"{n}__seg"] for n in BINARY_CASES]:
        lab, n = label(seg)
        extents, firsts = run_components(seg)
        assert len(extents) == n
        assert [int(lab[f]) for f in firsts] == list(range(1, n + 1))  # root order = label order
        for k, e in enumerate(extents):
            idx = np.where(lab == k + 1)
            assert e == [i.min() for i in idx] + [i.max() for i in idx]
        want, _ = DS.boxes_from_instances(seg, ONE, "binary")
        assert np.array_equal(_bits(run_boxes(seg)).reshape(-1, 6), _bits(want).reshape(-1, 6))
        seen += n
    assert seen >= 200


# ---- host arithmetic of the entry point --------------------------------------------------------------------------------
def test_workspace_holds_no_per_voxel_array():
    lib = _lib.load()
    N, D, H, W, cap = 2, 250, 300, 300, 2 * 262144
    nbytes = lib.msl_binary_boxes_workspace_bytes(N, D, H, W, cap)
    up = lambda b: (b + 255) // 256 * 256  # noqa: E731
    assert nbytes == up(4 * (N * D * H + 1)) + 4 * up(4 * cap) + up(20 * cap) + up(4 * N) + 256
    assert 0 < nbytes < N * D * H * W * 4 // 8
    # the same mask with a last axis ten times as long costs no more: nothing scales with the voxel count
    assert lib.msl_binary_boxes_workspace_bytes(N, D, H, 10 * W, cap) == nbytes
    for bad in ((0, 4, 4, 4, 16), (1, 4, 4, 0, 16), (1, 4, 4, 4, 0), (65536, 4, 4, 4, 16), (2, 40000, 40000, 4, 16)):
        assert lib.msl_binary_boxes_workspace_bytes(*bad) == 0, bad
