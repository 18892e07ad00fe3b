"""lesionpaste on the host: ``datasets.paste_lesions`` on the hand-built cases of
tests/lesionpaste_cases.py against the outcomes its table states and against a voxel-by-voxel restatement of the rule,
the draws, the bank, the lowering, the order checks and the host loader.  No GPU."""
import numpy as np
import pytest
import torch

from mslesions3d_amd import datasets as DS
from mslesions3d_amd.devicedata import PasteStage, check_ragged_pipeline, sample_params
from tests import lesionpaste_cases as LC


def _by_voxel(img, seg, r, lo, donors):
    """The writing rule of one accepted paste, voxel by voxel, from the old sample -> the new (img, seg)."""
    dimg, dseg = donors[int(r[1])]
    mn, e, flips, value = r[2:5], r[5:8], [(int(r[8]) >> a) & 1 for a in range(3)], r[9]
    out_i, out_s = img.copy(), seg.copy()

    def donor(p):
        return tuple(int(mn[a] + (e[a] - 1 - p[a] if flips[a] else p[a])) for a in range(3))

    def written(p):
        return all(0 <= p[a] < e[a] for a in range(3)) and dseg[donor(p)] != 0

    for p0 in range(-1, e[0] + 1):
        for p1 in range(-1, e[1] + 1):
            for p2 in range(-1, e[2] + 1):
                p, q = (p0, p1, p2), (lo[0] + p0, lo[1] + p1, lo[2] + p2)
                if not all(0 <= q[a] < seg.shape[a] for a in range(3)):
                    continue
                d = donor(p)
                if written(p):
                    out_i[(slice(None),) + q] = dimg[(slice(None),) + d]
                    out_s[q] = value
                elif any(written(tuple(p[a] + s * (a == ax) for a in range(3))) for ax in range(3) for s in (-1, 1)) \
                        and all(0 <= d[a] < dseg.shape[a] for a in range(3)):
                    out_i[(slice(None),) + q] = np.float32(0.5) * img[(slice(None),) + q] + np.float32(0.5) * dimg[(slice(None),) + d]
    return out_i, out_s


@pytest.mark.parametrize("value", [1, 7])
@pytest.mark.parametrize("C", [1, 2])
def test_paste_lesions_on_the_case_table(C, value):
    donors = LC.donors(C)
    kept = [(i.copy(), s.copy()) for i, s in donors]
    names = []
    for name, shape, rows, reports, counts in LC.samples(value):
        img, seg = LC.target(C, shape)
        i0, s0 = img.copy(), seg.copy()
        got = DS.paste_lesions(img, seg, np.stack(rows), donors)
        assert got == reports, name
        assert int((seg == value).sum()) == sum(counts), name  # (the target's own lesion has another id)
        box = LC.dilated_boxes(rows, reports, shape)
        assert np.array_equal(seg[~box], s0[~box]) and np.array_equal(img[:, ~box].view(np.int32), i0[:, ~box].view(np.int32)), name
        assert np.array_equal(seg == LC.LESION_ID, s0 == LC.LESION_ID), name
        want_i, want_s = i0, s0
        for r, rep in zip(rows, reports):
            if rep >= 0:
                want_i, want_s = _by_voxel(want_i, want_s, r, r[DS.PASTE_HEAD + 3 * rep:DS.PASTE_HEAD + 3 * rep + 3], donors)
        assert np.array_equal(seg, want_s) and np.array_equal(img.view(np.int32), want_i.view(np.int32)), name
        if any(rep >= 0 for rep in reports):
            assert not np.array_equal(img, i0) and bool(((img != i0).any(0) & (seg == s0)).any()), name  # a rim was blended
        names.append(name)
    assert len(set(names)) == len(names) >= 29
    for (i, s), (ki, ks) in zip(donors, kept):
        assert np.array_equal(i, ki) and np.array_equal(s, ks)  # the donors are read only


def test_a_flip_mirrors_the_box():
    donors = LC.donors(1)
    case, mn, e, _ = LC.D
    box = tuple(slice(a, a + b) for a, b in zip(mn, e))
    for f in (0, 1, 2, 4, 7):
        img, seg = LC.target(1)
        lo = (10, 1, 11)
        assert DS.paste_lesions(img, seg, LC.row(LC.D, [lo], flips=f, value=9)[None], donors) == [0]
        axes = tuple(a for a in range(3) if (f >> a) & 1)
        want = np.flip(donors[case][1][box] != 0, axes)
        dst = tuple(slice(a, a + b) for a, b in zip(lo, e))
        assert np.array_equal(seg[dst] == 9, want)
        assert np.array_equal(img[0][dst][want], np.flip(donors[case][0][0][box], axes)[want])


class _Counting(np.random.RandomState):
    calls = None

    def random_sample(self, size=None):
        self.calls = (self.calls or []) + [size]
        return super().random_sample(size)


@pytest.mark.parametrize("kw", [{}, {"max_lesions": 2, "candidates": 3}, {"max_lesions": 8, "candidates": 16}])
def test_the_draw_count_is_fixed(kw):
    full = dict(DS.PASTE_AUGMENTATIONS[0][1], **kw)
    n = 2 + full["max_lesions"] * (4 + 3 * full["candidates"])
    assert DS.paste_draw_count(full["max_lesions"], full["candidates"]) == n
    for prob in (0.0, 0.5, 1.0):
        for seed in range(4):
            rs, ref = _Counting(seed), np.random.RandomState(seed)
            d = DS.DRAWS["lesionpaste"](rs, **dict(kw, prob=prob))
            assert rs.calls == [n]  # one call, whatever was drawn: the bank and the data are not asked
            u = ref.random_sample(n)
            assert rs.rand() == ref.rand()  # the generator stands where n uniforms leave it
            assert (d is None) == (u[0] >= prob)
            if d is not None:
                assert len(d) == min(1 + int(u[1] * full["max_lesions"]), full["max_lesions"])
                assert d[0][0] == u[2] and d[0][1] == tuple(int(v >= 0.5) for v in u[3:6])
                assert np.array_equal(d[0][2].reshape(-1), u[6:6 + 3 * full["candidates"]])
    for bad in ({"max_lesions": 9}, {"max_lesions": 0}, {"candidates": 17}, {"candidates": 0}, {"max_volume": 0}):
        with pytest.raises(ValueError):
            DS.DRAWS["lesionpaste"](np.random.RandomState(0), **bad)


def test_bank_admission():
    shape = (60, 60, 60)
    ext = [[2, 2, 2, 5, 6, 7],         # enters: 3 * 4 * 5 = 60 voxels of box volume
           [10, 10, 10, 41, 12, 12],   # 32 voxels long: enters
           [10, 20, 10, 42, 22, 12],   # 33 voxels long
           [30, 40, 40, 32, 42, 42],   # face to face with the next: each one's dilated box meets the other's box
           [33, 41, 41, 35, 43, 43],
           [50, 50, 50, 52, 52, 52],   # one voxel of air between it and the next: clear
           [54, 50, 50, 59, 52, 52]]   # at the case's border: the dilation is clamped
    per_case = [(ext, [1, 1, 1, 2, 2, 1, 2], shape, [9, 2004]), (np.zeros((0, 6)), [], (5, 5, 5), [0, 1999]),
                ([[0, 0, 0, 1, 1, 1]], [2], (8, 8, 8), [0, 2001])]
    bank = DS.bank_from_lesions(per_case)
    assert bank.rows.tolist() == [[0, 1, *ext[0]], [0, 1, *ext[1]], [0, 1, *ext[5]], [0, 2, *ext[6]], [2, 2, 0, 0, 0, 1, 1, 1]]
    assert bank.max_ids.tolist() == [[9, 2004], [0, 1999], [0, 2001]] and bank.shapes == [shape, (5, 5, 5), (8, 8, 8)]
    # max_volume: the measure of eval --size_bins, prod(max - min)
    assert [r[2:] for r in DS.bank_from_lesions(per_case, max_volume=60).rows.tolist()] == [ext[0], ext[5], ext[6], [0, 0, 0, 1, 1, 1]]
    assert [r[2:] for r in DS.bank_from_lesions(per_case, max_volume=59).rows.tolist()] == [ext[5], ext[6], [0, 0, 0, 1, 1, 1]]
    assert len(DS.bank_from_lesions(per_case, max_volume=0.5).rows) == 0
    seg = np.zeros((4, 4, 4), np.int16)
    seg[0, 0, :3] = [3, 1500, 2007]
    assert DS.class_max_ids(seg, [(1000, 2000), (2000, np.inf)], "instances") == [1500, 2007]
    assert DS.class_max_ids(seg, [(1, 3), (5000, np.inf)], "instances") == [0, 4999]  # a class without an id: lo - 1
    assert DS.class_max_ids(seg, [(1, np.inf)], "binary") == [0]


def _draw(donor_us, flips=(0, 0, 0), cand=8):
    return [(u, flips, np.full((cand, 3), 0.5)) for u in donor_us]


def test_lowering_and_id_assignment():
    thr = [(1000, 2000), (2000, np.inf)]
    rows = np.array([[0, 1, 2, 3, 4, 4, 6, 9], [1, 2, 0, 0, 0, 3, 3, 3], [1, 1, 1, 1, 1, 20, 2, 2]], dtype=np.int64)
    bank = DS.LesionBank(rows, np.array([[1500, 2003], [1997, 32765]], dtype=np.int64), [(20, 20, 20), (30, 8, 8)])
    low = DS.lower_pastes(_draw([0.0, 0.4, 0.1, 0.5], flips=(1, 0, 1)), bank, 0, (16, 12, 20), thr, "instances", 4, 8)
    assert low.shape == (4, DS.PASTE_HEAD + 24) and low.dtype == np.int32
    # donor floor(u * 3); e = (3, 4, 6); centre floor((min + max) / 2) - min = (1, 1, 2), mirrored on axes 0 and 2
    assert low[0, :13].tolist() == [1, 0, 2, 3, 4, 3, 4, 6, 5, 1501, 1, 1, 3]
    assert low[0, 13:16].tolist() == [7, 4, 7]  # floor(0.5 * (t - e + 1))
    assert low[1, :10].tolist() == [1, 1, 0, 0, 0, 4, 4, 4, 5, 2004] and low[2, 9] == 1502 and low[3, 9] == 2005
    # the third bank row is 20 voxels long on axis 0: it does not fit a target of 16
    assert not DS.lower_pastes(_draw([0.9]), bank, 0, (16, 12, 20), thr, "instances", 4, 8).any()
    assert DS.lower_pastes(_draw([0.9]), bank, 0, (20, 12, 20), thr, "instances", 4, 8)[0, 0] == 1
    # exhaustion: class 1 of case 1 ends at 1997, ids 1998 and 1999 are left; class 2 holds 32765, 32766 and 32767 are left
    low = DS.lower_pastes(_draw([0.0] * 3 + [0.4] * 3), bank, 1, (16, 12, 20), thr, "instances", 6, 8)
    assert low[:, 0].tolist() == [1, 1, 0, 1, 1, 0] and low[:, 9].tolist() == [1998, 1999, 0, 32766, 32767, 0]
    # binary mode writes 1, whatever the case holds; rows past the drawn count and a sample without a draw are inactive
    low = DS.lower_pastes(_draw([0.0, 0.4]), bank, 1, (16, 12, 20), [(1, np.inf)], "binary", 4, 8)
    assert low[:, 0].tolist() == [1, 1, 0, 0] and low[:2, 9].tolist() == [1, 1]
    assert not DS.lower_pastes(None, bank, 0, (16, 12, 20), thr, "instances", 4, 8).any()
    with pytest.raises(ValueError, match="empty"):
        DS.lower_pastes(_draw([0.0]), DS.LesionBank(rows[:0], bank.max_ids, bank.shapes), 0, (16, 12, 20), thr, "instances", 4, 8)


def test_its_place_in_the_list():
    names = ["gaussiannoise", "lesionpaste", "scaleintensity", "flip", "elastic3d", "biasfield"]
    got = [n for n, _ in DS.select_training_augmentations(names)]
    assert got == ["flip", "elastic3d", "scaleintensity", "lesionpaste", "biasfield", "gaussiannoise"]
    assert DS.select_training_augmentations(["lesionpaste"]) == [("lesionpaste", {"prob": 0.5, "max_lesions": 4, "candidates": 8,
                                                                                "max_volume": None})]
    assert set(DS.DRAWS) == set(DS.AUGMENTATIONS) and "lesionpaste" in DS.DRAWS
    DS.check_mr_last(got)
    check_ragged_pipeline(got)
    for bad in (["lesionpaste", "flip"], ["lesionpaste", "shiftintensity", "gaussiannoise"], ["gaussiannoise", "lesionpaste"],
                ["flip", "lesionpaste", "affine"], ["lesionpaste", "lesionpaste"]):
        with pytest.raises(NotImplementedError):
            DS.check_mr_last(bad)
        with pytest.raises(NotImplementedError):
            sample_params([(n, None) for n in bad], (8, 8, 8), bad, ragged=True)
    with pytest.raises(NotImplementedError, match="example cache"):
        sample_params([("lesionpaste", None)], (8, 8, 8), ["lesionpaste"])
    perm, stages = sample_params([("flip", (0,)), ("lesionpaste", None), ("gaussiannoise", None)], (8, 8, 8),
                                 ["flip", "lesionpaste", "gaussiannoise"], ragged=True)
    assert isinstance(stages[0], PasteStage) and stages[0].draw is None and stages[0].kw["candidates"] == 8


def test_refused_without_a_bank(tmp_path):
    root = DS.generate_artificial_dataset(str(tmp_path), "paste", num_images=5, image_size=(16, 16, 16))
    with pytest.raises(NotImplementedError, match="lesionpaste"):
        DS.ExampleDataset(batch_size=2, augmentations=LC.recipe(), data_dir=str(tmp_path), dataset_name="paste").setup("fit")
    assert root
    from mslesions3d_amd.train import build_parser, paste_options_of
    args = build_parser().parse_args(["-a", "flip", "lesionpaste"])
    with pytest.raises(ValueError, match="-dm lesions"):
        paste_options_of(args, DS.select_training_augmentations(args.augmentations))
    args = build_parser().parse_args(["-dm", "lesions", "-a", "flip", "lesionpaste", "--paste_max_volume", "125"])
    augs, pasting = paste_options_of(args, DS.select_training_augmentations(args.augmentations))
    assert pasting and dict(augs)["lesionpaste"]["max_volume"] == 125.0 and DS.PASTE_AUGMENTATIONS[0][1]["max_volume"] is None
    with pytest.raises(ValueError, match="paste_max_volume"):
        paste_options_of(build_parser().parse_args(["-dm", "lesions", "--paste_max_volume", "125"]), [])


def test_an_empty_bank_is_refused_at_setup(tmp_path):
    from tests import lesion_tree
    data_dir = lesion_tree.make_tree(tmp_path, LC.TREE_SHAPES)
    augs = [("lesionpaste", {"max_volume": 0.5})]  # no box is that small
    dm = DS.LesionsDataModule(data_dir=data_dir, centers=lesion_tree.CENTERS, batch_size=2, spatial_size=LC.FIT_TARGET,
                              augmentations=augs)
    with pytest.raises(ValueError, match="bank is empty"):
        dm.setup("fit")


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    """(kind, patch) -> the set-up module with prob = 1, built once."""
    held = {}

    def get(kind, patch):
        if (kind, patch) not in held:
            held[(kind, patch)] = LC.module(tmp_path_factory.mktemp(f"{kind}_{'patch' if patch else 'fit'}"), kind, patch)
        return held[(kind, patch)]
    return get


@pytest.mark.parametrize("patch", [None, LC.PATCH])
@pytest.mark.parametrize("kind", ["instances", "binary", "mc"])
def test_every_configuration_accepts_a_paste(trees, kind, patch):
    """What tests/test_gpu_lesionpaste.py relies on: with these trees and seeds the host reference alone accepts at least
    one paste in each of the two epochs of every configuration."""
    dm = trees(kind, patch)
    tr = dm.train_dataset
    assert len(tr) == 4 and len(tr.bank.rows) >= 1 and len(tr.bank.shapes) == 4
    for epoch in range(2):
        dm.set_epoch(epoch)
        reports = [r for b in dm.train_dataloader() for rep in b["paste_report"] for r in rep]
        assert len(reports) == 4 * 4 and sum(r >= 0 for r in reports) >= 1, (kind, patch, epoch, reports)


@pytest.mark.parametrize("patch", [None, LC.PATCH])
def test_host_loader_on_a_tree(trees, tmp_path, patch):
    dm = trees("instances", patch)
    tr = dm.train_dataset
    plain = DS.LesionsDataModule(data_dir=dm.data_dir, centers=dm.centers, batch_size=2, spatial_size=LC.FIT_TARGET,
                                 augmentations=LC.recipe(0.0), patch_size=patch, tile_margin=(2, 2, 2))
    plain.setup("fit")
    assert plain.train_dataset.subjects == tr.subjects
    accepted = 0
    for epoch in range(2):
        dm.set_epoch(epoch)
        plain.set_epoch(epoch)
        for i in range(len(tr)):
            a, b, p = tr[i], tr[i], plain.train_dataset[i]
            # deterministic per (seed, epoch, subject)
            assert torch.equal(a["img"], b["img"]) and torch.equal(a["boxes"], b["boxes"]) and a["paste_report"] == b["paste_report"]
            assert p["paste_report"] == [-2] * 4
            # the un-pasted sample's boxes, plus one per accepted paste, the new ones behind the case's own
            n = sum(r >= 0 for r in a["paste_report"])
            accepted += n
            assert len(a["boxes"]) == len(p["boxes"]) + n
            assert torch.equal(a["boxes"][:len(p["boxes"])], p["boxes"]) and torch.equal(a["labels"][:len(p["labels"])], p["labels"])
            assert a.get("patch_origin") == p.get("patch_origin")  # the window's draws follow the list's: unchanged
            # the draws behind lesionpaste do not depend on it
            da = DS.draw_augmentations(tr.augmentations, tr.sample_rng(i))
            dp = DS.draw_augmentations(plain.train_dataset.augmentations, plain.train_dataset.sample_rng(i))
            assert [n for n, _ in da] == LC.RECIPE and da[1][1] is not None and dp[1][1] is None
            assert da[0] == dp[0] and da[2] == dp[2] and da[2][1] is not None
            if n == 0:
                assert torch.equal(a["img"], p["img"])
            else:
                assert not torch.equal(a["img"], p["img"])
    assert accepted >= 2
    dm.set_epoch(0)
    first = tr[0]["img"]
    dm.set_epoch(1)
    assert not torch.equal(first, tr[0]["img"])
    # validation samples are not pasted
    assert "paste_report" not in dm.test_dataset[0]
