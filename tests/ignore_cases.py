"""Seeded inputs for the tests of evaluation with ignored ground truth, shared by
tests/test_ignore_ref_cpu.py and tests/test_gpu_ignore.py.  Every builder returns ``{"case": (det_boxes, det_labels,
det_scores, true_boxes, true_labels, true_ignore), "ious": [...], "scores": [...]}`` (plus what its test needs) and is the
smallest shape at which its path can go wrong.  ``checked`` holds the builders' own assertions."""
import numpy as np

from tests import ignore_ref as R

F = np.float32
EV_TILE = 4096            # csrc/evaluate.hip
EV_MATCH_LDS_G = 16384    # csrc/evaluate.hip: more boxes in one image -> claims in global memory


def box(lo, size):
    lo = np.asarray(lo, F)
    return np.concatenate([lo, lo + F(size)]).astype(F)


def grid_boxes(n, cells, fill=0.5):
    """``n`` disjoint cubes on a cells^3 grid (cell edge 1 / cells, cube edge ``fill`` of it)."""
    idx = np.arange(n)
    lo = np.stack([idx % cells, (idx // cells) % cells, idx // (cells * cells)], 1).astype(F) / F(cells)
    return np.concatenate([lo, lo + F(fill / cells)], 1).astype(F)


def pack(images):
    """images: list of (det rows [(box, label, score)], gt rows [(box, label, ignore)]) -> the six lists."""
    db, dl, ds, tb, tl, ig = [], [], [], [], [], []
    for dets, gts in images:
        db.append(np.array([d[0] for d in dets], F).reshape(-1, 6))
        dl.append(np.array([d[1] for d in dets], np.int64))
        ds.append(np.array([d[2] for d in dets], F))
        tb.append(np.array([g[0] for g in gts], F).reshape(-1, 6))
        tl.append(np.array([g[1] for g in gts], np.int64))
        ig.append(np.array([g[2] for g in gts], bool))
    return db, dl, ds, tb, tl, ig


_matches = {}


def match(case, thr):
    """``ignore_ref.match``, computed once per (case, threshold) and process; the result is shared and left unchanged."""
    key = (id(case), float(thr))
    if key not in _matches:
        _matches[key] = (case, R.match(case, thr))  # holding the case keeps its id unique
    return _matches[key][1]


def without_flags(case):
    return case[:5] + ([np.zeros(len(f), bool) for f in case[5]],)


def checked(case, ious, share=None):
    """The builders' assertions: at least one detection absorbed at every IoU threshold used and, for the random cases
    (``share``), at least one detection that is a false positive in exactly one of the runs with and without the flags and
    an ignored share of the class-1 boxes inside [0.1, 0.4]."""
    for thr in ious:
        a = match(case, thr)
        assert a["ab"].sum() >= 1, ("no absorbed detection", thr)
        if share:  # the random cases
            if thr == ious[0]:
                assert (a["fp"] != R.match(without_flags(case), thr)["fp"]).any(), ("no false positive changes", thr)
            s = a["n_ignored"] / max(a["n_ignored"] + a["n_easy"], 1)
            assert 0.1 <= s <= 0.4, s
    return case


A = box([0.0, 0.0, 0.0], 0.25)
B = box([0.5, 0.5, 0.5], 0.25)
C = box([0.0, 0.5, 0.0], 0.25)
FAR = box([0.75, 0.0, 0.75], 0.125)


def iou_ties():
    """An ignored and a non-ignored box that are identical, in both orders: the first maximum decides.  Image 0 (ignored
    first): both detections absorbed.  Image 1 (non-ignored first): TP, then FP on the claimed box."""
    im0 = ([(A, 1, 0.9), (A, 1, 0.7)], [(A, 1, True), (A, 1, False)])
    im1 = ([(A, 1, 0.8), (A, 1, 0.6)], [(A, 1, False), (A, 1, True)])
    case = checked(pack([im0, im1]), [0.5])
    m = match(case, 0.5)
    assert m["ab"].tolist() == [1, 0, 1, 0] and m["tp"].tolist() == [0, 1, 0, 0] and m["fp"].tolist() == [0, 0, 0, 1]
    return {"case": case, "ious": [0.5], "scores": [0.0, 0.65]}


def exact_threshold():
    """A detection whose IoU with an ignored box is exactly the threshold (half the box: 0.5) is a FP; the whole box is
    absorbed."""
    half = A.copy()
    half[5] = F(0.125)
    assert R.OM._iou_1_to_many(half, A[None])[0] == F(0.5)
    case = checked(pack([([(half, 1, 0.9), (A, 1, 0.8)], [(A, 1, True)])]), [0.5])
    m = match(case, 0.5)
    assert m["fp"].tolist() == [1, 0] and m["ab"].tolist() == [0, 1]
    return {"case": case, "ious": [0.5, 0.25], "scores": [0.0]}


def multiple_absorbed():
    """One ignored box absorbs three detections; a lower-ranked TP follows; then a FP.  Score cuts between two absorbed
    detections (0.85), directly after one (0.8, 0.7) and behind everything."""
    dets = [(A, 1, 0.9), (A, 1, 0.8), (A, 1, 0.7), (B, 1, 0.6), (FAR, 1, 0.5)]
    case = checked(pack([(dets, [(A, 1, True), (B, 1, False)])]), [0.5])
    m = match(case, 0.5)
    assert m["ab"].tolist() == [1, 1, 1, 0, 0] and m["tp"].tolist() == [0, 0, 0, 1, 0] and m["claim"].tolist() == [R.IGNORED, 3]
    return {"case": case, "ious": [0.5], "scores": [0.0, 0.55, 0.65, 0.7, 0.8, 0.85, 0.95]}


def ignore_only_image():
    """Image 0 has only ignored boxes (it counts as an image without lesions), image 1 is ordinary."""
    im0 = ([(A, 1, 0.9), (FAR, 1, 0.85)], [(A, 1, True), (B, 1, True)])
    im1 = ([(A, 1, 0.8), (C, 1, 0.7)], [(A, 1, False), (B, 1, False)])
    case = checked(pack([im0, im1]), [0.5])
    assert match(case, 0.5)["g"].tolist() == [0, 2]
    return {"case": case, "ious": [0.5], "scores": [0.0, 0.75]}


def all_ignored():
    """Every box ignored: n_easy = 0, crec is NaN everywhere."""
    im0 = ([(A, 1, 0.9), (FAR, 1, 0.8)], [(A, 1, True)])
    im1 = ([(B, 1, 0.7)], [(B, 1, True), (C, 1, True)])
    case = checked(pack([im0, im1]), [0.5])
    assert match(case, 0.5)["n_easy"] == 0
    return {"case": case, "ious": [0.5], "scores": [0.0, 0.75]}


def no_class1_boxes():
    """Image 0 has no class-1 box at all (one box of label 2, flagged): its detections are FPs."""
    im0 = ([(A, 1, 0.9)], [(A, 2, True)])
    im1 = ([(A, 1, 0.8), (B, 1, 0.7)], [(A, 1, True), (B, 1, False)])
    case = checked(pack([im0, im1]), [0.5])
    assert match(case, 0.5)["fp"].tolist() == [1, 0, 0]
    return {"case": case, "ious": [0.5], "scores": [0.0]}


def other_label():
    """A flag on a box of label 2 changes nothing: ``case`` and ``same`` (that flag cleared) give the same results."""
    gts = [(A, 2, True), (A, 1, False), (B, 1, True), (C, 0, True)]
    dets = [(A, 1, 0.9), (B, 1, 0.8), (C, 1, 0.7)]
    case = checked(pack([(dets, gts)]), [0.5])
    same = pack([(dets, [(A, 2, False), (A, 1, False), (B, 1, True), (C, 0, False)])])
    return {"case": case, "same": same, "ious": [0.5], "scores": [0.0]}


def _hits(rs, gt, n_det, targets, jitter=0.0):
    """``n_det`` detections: the first ones copies of gt[targets] (in that order), the rest far misses; random scores
    quantised to 1/64."""
    d = np.tile(FAR, (n_det, 1))
    d[:len(targets)] = gt[targets]
    if jitter:
        d[:len(targets)] += rs.uniform(-jitter, jitter, (len(targets), 6)).astype(F)
    return d, (np.round(rs.uniform(0, 1, n_det) * 64) / 64).astype(F)


def boxes_130():
    """One image with 130 boxes: ignored ones inside the first 64 (held in registers) and in the later chunks."""
    rs = np.random.RandomState(130)
    gt = grid_boxes(130, 6)
    ign = np.zeros(130, bool)
    ign[[3, 40, 63, 64, 65, 100, 127, 128, 129]] = True
    targets = [3, 63, 64, 129, 3, 5, 5, 70, 128, 100, 64, 0, 66, 66, 127]
    d, s = _hits(rs, gt, 24, targets)
    case = checked((([d]), [np.ones(24, np.int64)], [s], [gt], [np.ones(130, np.int64)], [ign]), [0.5])
    return {"case": case, "ious": [0.5], "scores": [0.0, 0.5]}


def global_claim_path():
    """One image with EV_MATCH_LDS_G + 1 boxes (claims in global memory) and 40 detections; a second, small image."""
    rs = np.random.RandomState(7)
    G = EV_MATCH_LDS_G + 1
    gt = grid_boxes(G, 26)
    ign = np.zeros(G, bool)
    ign[[0, 63, 64, 5000, 16383, 16384]] = True
    targets = [0, 64, 16384, 16384, 5000, 1, 1, 16383, 200, 200, 9000, 63, 16382, 16382, 12345]
    d, s = _hits(rs, gt, 40, targets)
    im1 = pack([([(A, 1, 0.5), (B, 1, 0.25)], [(A, 1, True), (B, 1, False)])])
    case = ([d] + im1[0], [np.ones(40, np.int64)] + im1[1], [s] + im1[2], [gt] + im1[3], [np.ones(G, np.int64)] + im1[4],
            [ign] + im1[5])
    return {"case": checked(case, [0.5]), "ious": [0.5], "scores": [0.0]}


def ranked(D, absorbed_ranks, n_img=5, seed=0, denom=32768):
    """``D`` class-1 detections whose rank is their index (score 1 - j / denom, exact in f32), dealt round-robin over
    ``n_img`` images of four boxes (box 1 ignored).  The detections at ``absorbed_ranks`` sit on the ignored box of their
    image; a quarter of the others on a non-ignored box (jittered: some clear IoU 0.5, nearly all clear 0.1), the rest miss."""
    rs = np.random.RandomState(seed)
    gt = np.stack([A, B, C, box([0.5, 0.0, 0.5], 0.25)])
    boxes = np.tile(FAR, (D, 1))
    kind = rs.randint(0, 4, D)
    easy = gt[[0, 2, 3]][rs.randint(0, 3, D)] + rs.uniform(-0.07, 0.07, (D, 6)).astype(F)
    boxes[kind == 0] = easy[kind == 0]
    boxes[np.asarray(sorted(absorbed_ranks))] = B
    score = (F(1) - np.arange(D).astype(F) / F(denom)).astype(F)
    assert D < denom and (np.diff(score) < 0).all()
    db, dl, ds, tb, tl, ig = [], [], [], [], [], []
    for n in range(n_img):
        sel = np.arange(n, D, n_img)
        db.append(boxes[sel]), dl.append(np.ones(len(sel), np.int64)), ds.append(score[sel])
        tb.append(gt.copy()), tl.append(np.ones(4, np.int64)), ig.append(np.array([False, True, False, False]))
    return db, dl, ds, tb, tl, ig


def tile_boundary():
    """D = 4 100: absorbed flags on both sides of the EV_TILE boundary."""
    ab = [0, 7, EV_TILE - 2, EV_TILE - 1, EV_TILE, EV_TILE + 1, 4099]
    case = checked(ranked(4100, ab, seed=1), [0.5], share=True)
    m = match(case, 0.5)
    assert m["K"] == 4100 and m["ab"][[EV_TILE - 1, EV_TILE]].tolist() == [1, 1] and m["ab"].sum() == len(ab)
    return {"case": case, "ious": [0.5], "scores": [0.0, float(m["score"][EV_TILE - 1]), float(m["score"][EV_TILE])]}


def multi_block():
    """D = 16 400 with two IoU thresholds: the flag scan runs over 32 800 entries (several workgroups) and spans the two
    threshold rows."""
    rs = np.random.RandomState(2)
    ab = sorted(set(rs.randint(0, 16400, 700).tolist()) | {0, 4095, 4096, 8191, 8192, 16383, 16384, 16399})
    case = checked(ranked(16400, ab, seed=2), [0.1, 0.5], share=True)
    return {"case": case, "ious": [0.1, 0.5], "scores": [0.0, 0.75]}


def odd_scores():
    """NaN, -0.0 / 0.0 and tied scores among absorbed detections."""
    s = [0.5, 0.5, np.nan, -0.0, 0.0, 0.5, np.nan, 0.25]
    b = [A, B, A, A, B, A, B, FAR]
    case = checked(pack([(list(zip(b, [1] * 8, s)), [(A, 1, True), (B, 1, False)])]), [0.5])
    m = match(case, 0.5)
    assert m["ab"].sum() == 4 and np.isnan(m["score"][-2:]).all()
    return {"case": case, "ious": [0.5], "scores": [-1.0, 0.0, 0.25, 0.5]}


def froc_case():
    """Two images.  Rank order: absorbed .9 | absorbed .8 | FP .7 | absorbed .6 | TP .5 | FP .4.  At 1/2 false positive per
    image (FPw <= 1) the curve reaches k* = 5 and its TP only because the absorbed detections are no false positives.
    Weight rows with zeros."""
    im0 = ([(A, 1, 0.9), (FAR, 1, 0.7), (A, 1, 0.6)], [(A, 1, True)])
    im1 = ([(A, 1, 0.8), (B, 1, 0.5), (FAR, 1, 0.4)], [(A, 1, True), (B, 1, False)])
    case = checked(pack([im0, im1]), [0.5])
    rates = [(1, 2), (1, 1), (1, 4)]
    w = np.array([[1, 1], [0, 2], [2, 0], [1, 3]], np.int32)
    f = R.froc(case, [0.5], rates, w, match=match)
    assert f["k"][0, 0].tolist() == [5, 6, 2] and f["tp"][0, 0].tolist() == [1, 1, 0] and f["absorbed"][0, 0].tolist() == [3, 3, 2]
    m = match(case, 0.5)
    assert np.cumsum(m["fp"] + m["ab"])[4] * 2 > 1 * 2  # with absorbed counted as false positives the rate is not reached
    return {"case": case, "ious": [0.5], "scores": [0.0], "rates": rates, "weights": w}


def strata_case():
    """A frame of 1000 voxels, edges 27 / 125 / 1000.  Ignored boxes exactly on an edge (0.5^3 = 125 voxels), just beside
    it (64 voxels) and far from it; a non-ignored box on the same edge."""
    on = box([0.0, 0.0, 0.0], 0.5)         # 125 voxels: the bin [125, 1000)
    on2 = box([0.5, 0.5, 0.5], 0.5)
    beside = box([0.0, 0.5, 0.5], 0.4)     # 64 voxels: the bin [27, 125)
    tiny = box([0.6, 0.0, 0.0], 0.125)     # under 2 voxels: the bin below 27
    im0 = ([(on, 1, 0.9), (on2, 1, 0.8), (beside, 1, 0.7), (tiny, 1, 0.6), (FAR, 1, 0.5)],
           [(on, 1, True), (on2, 1, False), (beside, 1, True), (tiny, 1, False)])
    im1 = ([(beside, 1, 0.85), (tiny, 1, 0.3)], [(beside, 1, False), (tiny, 1, True)])
    case = checked(pack([im0, im1]), [0.5])
    w = np.array([[1, 1], [2, 0], [0, 3]], np.int32)
    return {"case": case, "ious": [0.5], "scores": [0.0, 0.65], "edges": [27.0, 125.0, 1000.0], "voxels": 1000.0,
            "weights": w, "cuts": [0, 1, 3, 5, 7]}


def random_case(seed, n_img=10, share=0.25):
    """Random images: hits with jitter, duplicates, misses, other labels on both sides, tied scores; ``share`` of the
    class-1 boxes ignored (checked to lie in [0.1, 0.4]); one image without ground truth, one without detections."""
    rs = np.random.RandomState(seed)
    db, dl, ds, tb, tl, ig = [], [], [], [], [], []
    for i in range(n_img):
        ng = 0 if i == seed % n_img else int(rs.randint(2, 7))
        nd = 0 if i == (seed + 3) % n_img else int(rs.randint(4, 25))
        lo = rs.uniform(0, 0.8, (ng, 3)).astype(F)
        t = np.concatenate([lo, lo + rs.uniform(0.02, 0.2, (ng, 3)).astype(F)], 1)
        d, _ = _hits(rs, t, nd, rs.randint(0, ng, min(nd, 2 * ng)) if ng else [], jitter=0.01)
        lab = np.ones(ng, np.int64)
        lab[rs.rand(ng) < 0.1] = 2
        lb = np.ones(nd, np.int64)
        lb[rs.rand(nd) < 0.1] = 0
        f = np.zeros(ng, bool)
        c1 = np.nonzero(lab == 1)[0]
        f[c1[:int(round(share * len(c1)))]] = True
        f |= (lab != 1) & (rs.rand(ng) < 0.5)  # flags on other labels: no effect
        db.append(d), dl.append(lb), ds.append((np.round(rs.uniform(0, 1, nd) * 8) / 8).astype(F))
        tb.append(t), tl.append(lab), ig.append(f)
    return {"case": checked((db, dl, ds, tb, tl, ig), [0.1, 0.5], share=True), "ious": [0.1, 0.5], "scores": [0.0, 0.5],
            "rates": [(1, 8), (1, 2), (1, 1), (4, 1)], "edges": [27.0, 125.0, 1000.0], "voxels": 32768.0}


SMALL = {"iou_ties": iou_ties, "exact_threshold": exact_threshold, "multiple_absorbed": multiple_absorbed,
         "ignore_only_image": ignore_only_image, "all_ignored": all_ignored, "no_class1_boxes": no_class1_boxes,
         "other_label": other_label, "odd_scores": odd_scores, "froc": froc_case, "strata": strata_case,
         "random_3": lambda: random_case(3), "random_11": lambda: random_case(11)}
LARGE = {"boxes_130": boxes_130, "global_claim_path": global_claim_path, "tile_boundary": tile_boundary,
         "multi_block": multi_block}
_built = {}


def get(name):
    """Every case is built (and its reference computed by the tests) once per process."""
    if name not in _built:
        _built[name] = {**SMALL, **LARGE}[name]()
    return _built[name]
