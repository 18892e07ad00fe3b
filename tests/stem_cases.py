"""Case tables of tests/test_gpu_stem.py (shared with tests/test_stem_ref_cpu.py, which proves every bound at every shape
with honest fp32 on the CPU and asserts, per case, the dispatch predicate of stem_fwd_impl / stem_bww_impl restated in
tests/stem_ref.py).  Plain data: (id, N, Cin, (D, H, W), (sd, sh, sw)).  The id starts with the kernel the case reaches and
its Cin - ``mfma<c>`` / ``rows<c>`` forward, ``wave<c>`` / ``tile<c>`` gradient - and carries ``iters2`` exactly when a wave
(tile kernel: a workgroup) walks two chunks (tiles); both are asserted on the CPU, so an edit cannot move a case silently.
These are the smallest shapes at which each path can still go wrong; none allocates more than a few tens of MB."""

S222, S122 = (2, 2, 2), (1, 2, 2)

# ------------------------------------------------------------------------------------------------- forward (fp32 and bf16 entry)
FWD_CASES = []
for _c in (1, 2, 3, 4):
    FWD_CASES += [
        (f"mfma<{_c}>:9x11x13-one-partial-tile-all-odd", 2, _c, (9, 11, 13), S222),       # OW = 7
        (f"mfma<{_c}>:5x6x70-whole+ragged-tile-sd1", 2, _c, (5, 6, 70), S122),            # OW = 35
    ]
FWD_CASES += [
    ("mfma<1>:4x5x130-one-column-chunk-dead-half", 2, 1, (4, 5, 130), S222),   # OW = 65 (W % 4 != 0: not row-staged)
    ("mfma<2>:4x5x131-odd-W-high-border-live", 2, 2, (4, 5, 131), S222),       # OW = 66
    ("mfma<1>:1x1x40-single-row-every-border", 2, 1, (1, 1, 40), S222),        # OW = 20
    ("mfma<4>:2x1x6-single-row", 2, 4, (2, 1, 6), S222),
    ("mfma<2>:5x6x40-s111", 2, 2, (5, 6, 40), (1, 1, 1)),                      # OW = 40: sw = 1, a ragged second tile
    ("mfma<2>:5x6x40-s212", 2, 2, (5, 6, 40), (2, 1, 2)),                      # OW = 20: W % 4 == 0 but OW % 32 != 0
    ("mfma<3>:5x6x40-s121", 2, 3, (5, 6, 40), (1, 2, 1)),
    ("mfma<1>:5x6x40-s221", 2, 1, (5, 6, 40), (2, 2, 1)),
    ("mfma<3>:6x7x64-rows-by-shape-declined-by-Cin", 2, 3, (6, 7, 64), S222),  # OW = 32 exactly
    ("mfma<4>:6x7x64-rows-by-shape-declined-by-Cin", 2, 4, (6, 7, 64), S222),
    # 1 089 chunks per image on 256 workgroups: the walk crosses rows and planes and ends on dead tiles (1 024 waves x 2 > 1 089)
    ("mfma<1>:66x66x40-iters2", 2, 1, (66, 66, 40), S222),
]
for _dims in ((3, 3, 64), (1, 1, 64), (6, 10, 128), (5, 8, 192), (7, 9, 320)):   # half / one / one and a half / five chunks
    for _s in (S222, S122, (1, 1, 2), (2, 1, 2)):
        for _c in (1, 2):
            FWD_CASES.append((f"rows<{_c}>:{'x'.join(map(str, _dims))}-s{''.join(map(str, _s))}", 2, _c, _dims, _s))
FWD_CASES.append(("rows<2>:66x66x64-iters2", 2, 2, (66, 66, 64), S222))

# ------------------------------------------------------------------------------------------------- weight gradient
# every case runs msl_stem_conv_bwd_weight, _bnapply, _fused, _bnapply_bf16, _fused_bf16 (MODE 0, 1, 2, 1 bf16, 2 bf16)
BWW_CASES = []
for _c in (1, 2, 3, 4):
    # outputs (5, 6, 7) and (6, 5, 8): every axis once odd, once even.  60 chunks -> 15 workgroups: no multiple of 8, so
    # these are the cases with the XCD remap of MODE 2 OFF
    BWW_CASES += [(f"wave<{_c}>:9x11x13-remap-off", 2, _c, (9, 11, 13), S222), (f"wave<{_c}>:11x9x16-remap-off", 2, _c, (11, 9, 16), S222)]
BWW_CASES += [
    ("wave<2>:5x11x13-sd1", 2, 2, (5, 11, 13), S122),
    ("wave<1>:3x4x140-two-chunks-per-row", 2, 1, (3, 4, 140), S222),           # OW = 70
    ("wave<3>:3x4x140-two-chunks-per-row", 2, 3, (3, 4, 140), S222),
    ("wave<3>:3x4x128-OW64", 2, 3, (3, 4, 128), S222),                         # H % 16 != 0: not tile-eligible by shape either
    ("wave<3>:3x16x128-tile-by-shape-declined-by-Cin", 2, 3, (3, 16, 128), S222),
    ("wave<1>:3x4x130-one-position-chunk", 2, 1, (3, 4, 130), S222),           # OW = 65
    ("wave<3>:3x4x130-one-position-chunk", 2, 3, (3, 4, 130), S222),
    # 2 178 chunks on 512 workgroups (2 048 waves x 2): the walk crosses the image boundary, dead chunks, grid % 8 == 0
    ("wave<1>:66x66x8-iters2-remap-on", 2, 1, (66, 66, 8), S222),
    ("wave<4>:66x66x8-iters2-remap-on", 2, 4, (66, 66, 8), S222),
]

# tile-staged kernel: reached by msl_stem_conv_bwd_weight_fused[_bf16] only (MODE 2), so only those two run
TILE_CASES = [
    ("tile<1>:1x16x128", 2, 1, (1, 16, 128), S222),
    ("tile<1>:2x16x128", 2, 1, (2, 16, 128), S222),
    ("tile<1>:5x48x128-odd-D-kd2-outside", 2, 1, (5, 48, 128), S222),
    ("tile<2>:6x32x128", 2, 2, (6, 32, 128), S222),
    ("tile<1>:258x16x128-iters2-516-tiles-on-512", 2, 1, (258, 16, 128), S222),
]

# the deferred form (dw == NULL) at one shape per kernel family
DEFERRED = ("wave<3>:9x11x13-remap-off", "wave<1>:66x66x8-iters2-remap-on", "tile<1>:2x16x128", "tile<2>:6x32x128")

# refusals: a general, a rows-eligible and a tile-eligible shape
REFUSAL_SHAPES = [("general", (9, 11, 13)), ("rows-eligible", (3, 3, 64)), ("tile-eligible", (2, 16, 128))]
