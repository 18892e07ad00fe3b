"""The case list of the prior fit report's tests (tests/test_priorfit_ref_cpu.py, tests/test_gpu_priorfit.py): two prior
sets, restated in numpy (the GPU test checks msl_make_priors against them), and object lists named by what they can break."""
import numpy as np

from mslesions3d_amd import _lib

TILE, CHUNK = _lib.PRIOR_FIT_TILE, _lib.PRIOR_FIT_CHUNK

# (a) 32^3 on layers 3 5 7: 4^3 + 2^3 + 1 locations x 2 = 146 priors, less than one tile
# (b) (24,32,32) on layers 1 3 5 7: 12x8x8 + 6x4x4 + 3x2x2 + 2x1x1 = 878 locations x 2 = 1756 priors: more than one tile of
#     1024 and not a multiple of it
PRIOR_SETS = {"a": {"input": (32, 32, 32), "layers": (3, 5, 7), "P": 146},
              "b": {"input": (24, 32, 32), "layers": (1, 3, 5, 7), "P": 1756}}
assert PRIOR_SETS["a"]["P"] < TILE < PRIOR_SETS["b"]["P"] and PRIOR_SETS["b"]["P"] % TILE != 0

_STRIDES = (None, 2, 2, 1, 2, 1, 2, 1, 1, 1, 1, 1, 1, 1)  # of feature 1.. (mobilenet: 64 | 128 x2 | 256 x2 | 512 x6 | 1024 x2)


def fmap_dims(input_size, upto=7):
    """{feature: (d0, d1, d2)}: a k3 p1 convolution of stride s maps d to (d - 1) // s + 1; the stem strides (2,2,2) on a
    cube and (1,2,2) otherwise (ssd3d.py:60)."""
    cube = input_size[0] == input_size[1] == input_size[2]
    cur = tuple((d - 1) // s + 1 for d, s in zip(input_size, (2, 2, 2) if cube else (1, 2, 2)))
    dims = {0: cur}
    for f in range(1, upto + 1):
        cur = tuple((d - 1) // _STRIDES[f] + 1 for d in cur)
        dims[f] = cur
    return dims


def default_scales(input_size, layers, min_os=6, max_os=14):
    return dict(zip(layers, np.linspace(min_os / input_size[0], max_os / input_size[0], len(layers))))  # ssd3d.py:228-234


def priors_numpy(input_size, layers, scales=None, bpl=2):
    """ssd3d.py:286-342 -> ((P,6) f32 centre-size priors, (S+1,) row offsets): fp64 arithmetic rounded once, clamped."""
    dims = fmap_dims(input_size, max(layers))
    scales = default_scales(input_size, layers) if scales is None else scales
    rows, off = [], [0]
    for f in layers:
        d0, d1, d2 = dims[f]
        i, j, k, b = np.meshgrid(np.arange(d0), np.arange(d1), np.arange(d2), np.arange(bpl), indexing="ij")
        s = float(scales[f])
        with np.errstate(divide="ignore"):
            sz = np.where(b == 0, s, s + s / np.where(b == 0, 1, b).astype(np.float64))
        r = np.stack([(j + 0.5) / d1, (i + 0.5) / d0, (k + 0.5) / d2, sz, sz, sz], axis=-1).reshape(-1, 6)
        rows.append(np.clip(r.astype(np.float32), 0, 1))
        off.append(off[-1] + r.shape[0])
    return np.concatenate(rows), np.asarray(off, dtype=np.int32)


def prior_set(name):
    s = PRIOR_SETS[name]
    pri, off = priors_numpy(s["input"], s["layers"])
    assert pri.shape[0] == s["P"]
    return pri, off


def _c2x(c):
    c = np.asarray(c, np.float32)
    return np.concatenate([c[:3] - c[3:] / 2, c[:3] + c[3:] / 2]).astype(np.float32)


def _random_boxes(rs, n, size, vox=(2, 10)):
    """n boxes of 2 .. 10 voxels per axis inside the frame, as fractions."""
    size = np.asarray(size, np.float64)
    ext = rs.randint(vox[0], vox[1] + 1, (n, 3))
    lo = (rs.uniform(0, 1, (n, 3)) * (size - ext)).round()
    return np.concatenate([lo / size, (lo + ext) / size], 1).astype(np.float32)


# prior set (a): feature 3 is a 4^3 grid, row ((i * 4 + j) * 4 + k) * 2 + b, centre ((j+.5)/4, (i+.5)/4, (k+.5)/4), sizes
# 0.1875 (b = 0) and 0.375 (b = 1); every coordinate below is a multiple of 1/32, exact in f32
ON_PRIOR_54 = _c2x([0.625, 0.375, 0.875, 0.1875, 0.1875, 0.1875])     # i, j, k = 1, 2, 3: rows 54 (b = 0), 55 (b = 1)
BETWEEN_50_52 = _c2x([0.625, 0.375, 0.5, 0.1875, 0.1875, 0.1875])     # half way between k = 1 (row 50) and k = 2 (row 52)
INSIDE_PRIOR_54 = _c2x([0.625, 0.375, 0.875, 0.0625, 0.0625, 0.0625])  # best prior 54 too, at IoU 1/27
POINTS = [np.array([v] * 6, np.float32) for v in (0.3, 0.5, 0.7)]      # zero volume: IoU 0 with every prior

HAND_CASES = {  # name -> (images, thresholds), on prior set (a) split by feature map; expected values in test_priorfit_ref_cpu
    "equal_to_prior": ([np.stack([ON_PRIOR_54])], [0.1, 0.125, 0.2, 1.0]),
    "tie_first_index": ([np.stack([BETWEEN_50_52])], [0.1, 0.15, 0.2, 0.25]),
    "identical_pair": ([np.stack([ON_PRIOR_54, ON_PRIOR_54])], [0.1, 0.2, 1.0]),
    "zero_volume": ([np.stack(POINTS)], [0.0, 0.5, 1.0]),
    "forced_prior_taken": ([np.stack([ON_PRIOR_54, INSIDE_PRIOR_54])], [0.1, 0.2]),
}

THR8 = [0.0, 0.05, 0.1, 0.2, 0.3, 0.5, 0.75, 1.0]


def cases():
    """-> list of dict(name, set, split ("maps": one range per feature map, "one": a single range), images, thresholds)."""
    out = []
    for name, (images, thr) in HAND_CASES.items():
        out.append(dict(name=name, set="a", split="maps", images=images, thresholds=thr))
    rs = np.random.RandomState(20240611)
    e = np.zeros((0, 6), np.float32)
    for s in ("a", "b"):
        size = PRIOR_SETS[s]["input"]
        out.append(dict(name=f"empty_between_{s}", set=s, split="maps", thresholds=[0.1, 0.2],
                        images=[_random_boxes(rs, 3, size), e, _random_boxes(rs, 5, size)]))
        out.append(dict(name=f"no_objects_{s}", set=s, split="maps", images=[e], thresholds=[0.5]))
        for n in (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3):  # one image: the chunk boundaries of the LDS staging
            out.append(dict(name=f"random_{n}_{s}", set=s, split="maps", images=[_random_boxes(rs, n, size)],
                            thresholds=[0.1, 0.2]))
    out.append(dict(name="thr1_one_range_a", set="a", split="one", thresholds=[0.1],
                    images=[_random_boxes(rs, 7, (32, 32, 32)), _random_boxes(rs, 2, (32, 32, 32))]))
    out.append(dict(name="thr8_four_ranges_b", set="b", split="maps", thresholds=THR8,
                    images=[_random_boxes(rs, 20, (24, 32, 32)), e, _random_boxes(rs, CHUNK + 5, (24, 32, 32))]))
    out.append(dict(name="thr8_one_range_b", set="b", split="one", thresholds=THR8,
                    images=[np.concatenate([_random_boxes(rs, 9, (24, 32, 32)), np.stack(POINTS[:2])])]))
    return out


def case_split(case, off):
    return off if case["split"] == "maps" else np.asarray([0, off[-1]], dtype=np.int32)
