"""Case table of the per-channel backward link (csrc/chanlink.hip): the smallest shapes that reach each of the 13 configurations
(NW waves, QO, QI quads per thread, stride) ``link_launch`` can dispatch.  Each id names the instantiation it reaches
(``s<stride>-w<NW>-q<QI>``; asserted against chanlink_ref.plan and the library in tests/test_chanlink_ref_cpu.py).  Every
configuration appears with accumulate 0 and 1, with all lanes live and with masked quads (odd batches, non-cubic extents).
tqi = N D H W / 4 input quads per channel decides the configuration: <= 128 one wave, <= 1024 four, <= 2048 eight, <= 4096 sixteen."""

# (id, N, C, (D, H, W), stride, accumulate)
CASES = [
    # ---- stride 1
    ("s1-w1-q1-one-quad", 1, 3, (1, 1, 4), 1, 0),        # D == H == 1: every depth / row neighbour is halo
    ("s1-w1-q1-smallest-cube", 1, 2, (2, 2, 4), 1, 1),
    ("s1-w1-q1-live", 1, 3, (4, 4, 16), 1, 0),           # tqi = 64: all 64 lanes
    ("s1-w1-q2-live", 2, 3, (4, 4, 16), 1, 1),           # tqi = 128
    ("s1-w1-q2-masked", 3, 2, (2, 4, 16), 1, 0),         # tqi = 96
    ("s1-w4-q1-live", 1, 3, (4, 8, 32), 1, 0),           # tqi = 256
    ("s1-w4-q1-masked", 5, 2, (2, 4, 16), 1, 1),         # tqi = 160
    ("s1-w4-q1-rows-lds110k", 256, 2, (1, 1, 4), 1, 1),  # 256 one-row images: 110 592 B of LDS, almost all halo
    ("s1-w4-q2-live", 4, 2, (4, 8, 16), 1, 0),           # tqi = 512
    ("s1-w4-q2-masked", 3, 3, (4, 8, 16), 1, 1),         # tqi = 384
    ("s1-w4-q2-masked-n5", 5, 3, (4, 8, 8), 1, 0),       # tqi = 320
    ("s1-w4-q4-live", 1, 3, (16, 16, 16), 1, 1),         # tqi = 1024
    ("s1-w4-q4-masked", 3, 2, (8, 8, 16), 1, 0),         # tqi = 768
    ("s1-w8-q4-live", 2, 2, (16, 16, 16), 1, 1),         # tqi = 2048
    ("s1-w8-q4-masked", 3, 2, (16, 8, 16), 1, 0),        # tqi = 1536
    ("s1-w16-q4-live", 4, 2, (16, 16, 16), 1, 0),        # tqi = 4096
    ("s1-w16-q4-masked", 3, 2, (16, 16, 16), 1, 1),      # tqi = 3072
    ("s1-w16-q4-lds153856", 24, 2, (8, 8, 8), 1, 1),     # the largest LDS image link_plan accepts
    # ---- stride 2
    ("s2-w1-q4-od1-oh1", 1, 3, (2, 2, 8), 2, 0),         # the class is q; OD = OH = 1
    ("s2-w1-q4-interior", 1, 4, (4, 4, 8), 2, 1),
    ("s2-w1-q4-live-h2", 2, 4, (8, 2, 16), 2, 1),        # tqi = 128, H == 2
    ("s2-w1-q4-masked", 3, 3, (2, 4, 8), 2, 0),          # 12 of 64 lanes per class
    ("s2-w4-q1-live", 1, 3, (8, 8, 16), 2, 1),           # a wave is one class
    ("s2-w4-q1-live-d2", 4, 3, (2, 8, 16), 2, 0),
    ("s2-w4-q1-masked", 5, 3, (4, 4, 8), 2, 1),          # 40 of 64 lanes per wave
    ("s2-w4-q2-live", 2, 3, (8, 8, 16), 2, 0),           # classes paired ee + oo / eo + oe
    ("s2-w4-q2-masked", 3, 3, (8, 4, 16), 2, 1),
    ("s2-w4-q4-live", 4, 2, (8, 8, 16), 2, 1),           # tqi = 1024: the class is q, each wave runs all four
    ("s2-w4-q4-masked", 3, 2, (8, 8, 16), 2, 0),         # tqi = 768
    ("s2-w8-q4-live", 2, 3, (16, 16, 16), 2, 1),
    ("s2-w8-q4-live-d2", 8, 2, (2, 16, 32), 2, 0),
    ("s2-w8-q4-masked", 5, 2, (8, 8, 16), 2, 1),         # 5 of 8 image slots
    ("s2-w16-q4-live", 2, 2, (16, 16, 32), 2, 0),
    ("s2-w16-q4-live-d2", 16, 2, (2, 16, 32), 2, 1),
    ("s2-w16-q4-masked", 3, 2, (16, 16, 16), 2, 0),      # tqi = 3072
]

BY_ID = {c[0]: c for c in CASES}


def config_of_id(cid):
    """'s1-w4-q2-...' -> (NW, QO, QI, stride)"""
    s, w, q = cid.split("-")[:3]
    stride, nw, qi = int(s[1:]), int(w[1:]), int(q[1:])
    return (nw, qi if stride == 1 else 1, qi, stride)


# bf16 storage runs the same table; the GPU test runs every case with and without the weight gradient (BWW) at both storages
BF16_CASES = CASES

# the cancelled channel: at seed 0 the BatchNorm2 scale gradient of one channel is 0.106, what is left of terms that sum to 6100
CANCELLED = ("s1-w16-q4-cancelled", 4, 2, (16, 16, 16), 1)

# two launches in a row on one stream with different inputs: the smallest and the largest stride-1 image, and a stride-2 case
# whose tap-gradient exchange reuses the image region
STALE_LDS = ["s1-w1-q1-smallest-cube", "s1-w16-q4-live", "s2-w8-q4-live"]

# (id, N, C, (D, H, W), stride, return code): MSL_ERR_ARG = -1 (N, C: checked first), MSL_ERR_UNSUPPORTED = -2 (link_plan)
REFUSALS = [
    ("D3", 2, 2, (3, 4, 8), 1, -2), ("H6", 2, 2, (4, 6, 8), 1, -2), ("W12", 2, 2, (4, 4, 12), 1, -2),
    ("D3-s2", 2, 2, (3, 4, 8), 2, -2), ("W2", 2, 2, (4, 4, 2), 1, -2),
    ("s2-W4", 2, 2, (4, 4, 4), 2, -2), ("s2-D1", 2, 2, (1, 4, 8), 2, -2), ("s2-H1", 2, 2, (4, 1, 8), 2, -2),
    ("stride0", 2, 2, (4, 4, 8), 0, -2), ("stride3", 2, 2, (4, 4, 8), 3, -2),
    ("tqi5120", 5, 2, (16, 16, 16), 1, -2), ("tqi5120-s2", 5, 2, (16, 16, 16), 2, -2),
    ("lds-cap-25x8x8x8", 25, 2, (8, 8, 8), 1, -2), ("lds-cap-512-rows", 512, 2, (1, 1, 4), 1, -2),
    ("N0", 0, 2, (4, 4, 8), 1, -1), ("N-1", -1, 2, (4, 4, 8), 1, -1), ("C0", 2, 0, (4, 4, 8), 1, -1), ("C-1", 2, -1, (4, 4, 8), 1, -1),
    ("D0", 2, 2, (0, 4, 8), 1, -2), ("H0", 2, 2, (4, 0, 8), 1, -2), ("W0", 2, 2, (4, 4, 0), 1, -2),
]
