"""Mint ``instances.npz`` by running the REFERENCE's own ``BoundingBoxesGeneratord`` (utils.py:438-513) in 'instances'
and 'binary' mode on hand-made and random instance masks (build container only):

    python -m tests.golden.make_golden_instances

Only the masks, the threshold pairs and the resulting boxes / labels are stored; ``inf`` is stored as INT32_MAX.
"""
import os

import numpy as np

from . import make_golden_data

OUT = os.path.dirname(os.path.abspath(__file__))
INF = np.iinfo(np.int32).max
ONE = [(1, INF)]
TWO = [(1000, 2000), (2000, INF)]


def _cube(seg, lo, size, value):
    seg[tuple(slice(a, a + s) for a, s in zip(lo, size))] = value


def cases():
    """name -> (mode, mask int16 (D, H, W), [(lo, hi), ...])."""
    out = {}
    m = np.zeros((24, 24, 24), np.int16)
    _cube(m, (2, 3, 4), (5, 6, 7), 1)
    _cube(m, (12, 12, 12), (4, 4, 4), 2)
    _cube(m, (18, 2, 10), (3, 9, 2), 7)
    out["one_class"] = ("instances", m, ONE)
    m = np.zeros((24, 24, 24), np.int16)
    _cube(m, (2, 3, 4), (5, 6, 7), 2003)
    _cube(m, (12, 12, 12), (4, 4, 4), 1001)
    _cube(m, (18, 2, 10), (3, 9, 2), 1002)
    _cube(m, (10, 2, 2), (3, 3, 3), 2001)
    _cube(m, (1, 15, 15), (4, 4, 4), 5)        # below every pair
    _cube(m, (8, 18, 2), (2, 2, 2), 999)       # below every pair, next to its lower bound
    out["two_classes_with_outsiders"] = ("instances", m, TWO)
    m = np.zeros((20, 20, 20), np.int16)
    _cube(m, (3, 3, 3), (1, 6, 6), 1)          # one voxel thick: flat, removed
    _cube(m, (8, 8, 8), (4, 1, 4), 2)          # flat on another axis
    _cube(m, (14, 2, 2), (3, 3, 3), 3)
    _cube(m, (1, 14, 14), (1, 1, 1), 4)        # a single voxel
    out["flat"] = ("instances", m, ONE)
    out["empty"] = ("instances", np.zeros((16, 16, 16), np.int16), ONE)
    out["empty_two_classes"] = ("instances", np.zeros((16, 16, 16), np.int16), TWO)
    m = np.full((12, 12, 12), 3, np.int16)     # no background: the smallest id (3) is discarded
    _cube(m, (2, 2, 2), (4, 4, 4), 5)
    _cube(m, (7, 7, 7), (3, 3, 3), 9)
    out["no_background"] = ("instances", m, ONE)
    m = np.full((12, 12, 12), 1500, np.int16)  # the same with two classes: 1500 is lost
    _cube(m, (2, 2, 2), (4, 4, 4), 1700)
    _cube(m, (7, 7, 7), (3, 3, 3), 2100)
    out["no_background_two_classes"] = ("instances", m, TWO)
    m = np.zeros((20, 20, 20), np.int16)
    _cube(m, (4, 4, 4), (4, 4, 4), 1)
    _cube(m, (8, 4, 4), (4, 4, 4), 2)          # face to face with 1
    _cube(m, (4, 8, 4), (4, 4, 4), 32767)      # the largest id, touching 1 as well
    out["touching"] = ("instances", m, ONE)
    m = np.zeros((48, 64, 64), np.int16)
    _cube(m, (40, 3, 50), (8, 20, 14), 11)     # reaches the far corner
    _cube(m, (0, 0, 0), (3, 3, 3), 12)         # and the origin
    _cube(m, (20, 30, 30), (6, 9, 11), 4)
    out["noncube"] = ("instances", m, ONE)
    m = np.zeros((17, 30, 23), np.int16)
    _cube(m, (1, 2, 3), (5, 9, 4), 1999)
    _cube(m, (9, 15, 10), (6, 7, 8), 2000)
    _cube(m, (9, 2, 15), (2, 2, 2), 1000)
    out["noncube_odd_two_classes"] = ("instances", m, TWO)
    for seed, shape, pairs in ((0, (24, 24, 24), ONE), (1, (16, 40, 28), ONE), (2, (32, 20, 26), TWO)):
        rs = np.random.RandomState(seed)
        m = np.zeros(shape, np.int16)
        ids = rs.permutation(np.arange(1, 60))[:12] if pairs is ONE else rs.randint(900, 3200, 14)
        for v in ids:
            size = rs.randint(1, 7, 3)
            lo = [rs.randint(0, n - s + 1) for n, s in zip(shape, size)]
            _cube(m, lo, size, v)               # later cubes overwrite earlier ones: non-box shapes, split ids
        out[f"random_{seed}"] = ("instances", m, pairs)
    m = np.zeros((24, 24, 24), np.int16)
    _cube(m, (2, 3, 4), (5, 6, 7), 1)
    _cube(m, (7, 3, 4), (3, 3, 3), 1)          # touches the first cube: one component
    _cube(m, (15, 15, 15), (4, 5, 6), 1)
    _cube(m, (20, 2, 2), (1, 4, 4), 1)         # flat
    out["binary"] = ("binary", m, ONE)
    out["binary_full"] = ("binary", np.ones((10, 10, 10), np.int16), ONE)  # one component and no background: lost
    rs = np.random.RandomState(5)
    out["binary_random"] = ("binary", (rs.rand(20, 28, 24) < 0.08).astype(np.int16), ONE)
    return out


def main():
    make_golden_data.install()
    import utils as ref_utils
    out, names = {}, []
    for name, (mode, seg, pairs) in cases().items():
        thr = [(lo, np.inf if hi == INF else hi) for lo, hi in pairs]
        conv = ref_utils.BoundingBoxesGeneratord(keys=["seg"], segmentation_mode=mode,
                                                 thresholds=thr if mode == "instances" else None)
        try:
            b, l = conv.converter(seg[None].copy())  # the data module adds the channel axis first
            b, l = b.numpy().reshape(-1, 6), l.numpy()
        except RuntimeError as e:
            # utils.py:472 divides a (0,) tensor by a (6,) one when there is no object at all: the reference cannot
            # return here; the fixture records "no boxes", the only reading of an image without objects
            assert "must match" in str(e), e
            b, l = np.zeros((0, 6), np.float32), np.zeros((0,), np.int64)
            out[f"{name}__reference_raised"] = np.array(1)
        assert b.dtype == np.float32 and l.dtype == np.int64
        names.append(name)
        out[f"{name}__mode"] = np.array(mode)
        out[f"{name}__seg"] = seg
        out[f"{name}__thresholds"] = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
        out[f"{name}__boxes"] = b
        out[f"{name}__labels"] = l
        print(name, mode, seg.shape, "->", len(l), "boxes", "(reference raised)" if f"{name}__reference_raised" in out else "")
    out["names"] = np.array(names)
    np.savez_compressed(os.path.join(OUT, "instances.npz"), **out)
    print("wrote instances.npz", os.path.getsize(os.path.join(OUT, "instances.npz")), "bytes")


if __name__ == "__main__":
    main()
