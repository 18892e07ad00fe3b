"""Cost of the lesionpaste stage (msl_paste_lesions, csrc/lesionpaste.hip).

    python tools/bench_lesionpaste.py [--reps 10] [--window 10] [--out profiles/lesionpaste_bench.json]

One (1, 230, 280, 260) case with 60 small lesions in the arena -> a (4, 1, 128, 128, 128) patch batch.  Microseconds of
one batch build (median, smallest and largest of --reps windows of --window back-to-back builds between two HIP events),
the two alternating in the same process:

  build        : msl_augment_window_mc + msl_instance_boxes - the batch build as it was before the stage existed
  build_paste  : msl_augment_window_mc + msl_paste_lesions + msl_instance_boxes, every sample drawing a paste
                 (prob = 1, max_lesions = 4, candidates = 8; rows from datasets.lower_pastes on the case's own bank)

The stage works in place, so it is timed behind the build that rewrites the batch, never alone in a loop: a second run on
the same batch would find its destinations taken.  The pasted batch is checked against datasets.paste_lesions before
anything is timed.  Writes one JSON file and prints it as one line.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mslesions3d_amd import _lib  # noqa: E402
from mslesions3d_amd import datasets as DS  # noqa: E402
from mslesions3d_amd.devicedata import _InstBoxOut, fit_rows  # noqa: E402
from tools.bench_patches import Arena, IDENT  # noqa: E402
from tools.bench_views import windows  # noqa: E402

CASE, PATCH, N = (230, 280, 260), (128, 128, 128), 4
KW = {"prob": 1.0, "max_lesions": 4, "candidates": 8}
THRESHOLDS = [(1, np.inf)]


def make_case(seed=1, lesions=60):
    """-> (image f32 without a zero, instance mask int16): ``lesions`` boxes of 3 .. 12 voxels a side on a 6 x 5 x 2 lattice
    of cells, so no two touch."""
    rs = np.random.RandomState(seed)
    img = (rs.randn(*CASE) + 3.0).astype(np.float32)
    img[img == 0] = 1.0
    seg = np.zeros(CASE, np.int16)
    cells = [(a, b, c) for a in range(6) for b in range(5) for c in range(2)]
    for k, (a, b, c) in enumerate(cells[:lesions]):
        size = rs.randint(3, 13, 3)
        at = np.array([10 + 36 * a, 10 + 52 * b, 20 + 120 * c]) + rs.randint(0, 12, 3)
        box = tuple(slice(int(o), int(o + s)) for o, s in zip(at, size))
        seg[box] = (k + 1) * (rs.rand(*size) < 0.8)
        seg[tuple(int(o) for o in at)] = seg[tuple(int(o + s - 1) for o, s in zip(at, size))] = k + 1
    return img, seg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--window", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lesionpaste_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    img, seg = make_case()
    extents, labels, shape = DS._instance_extents(seg, THRESHOLDS, "instances")
    keep = DS._fractional_boxes(extents, shape)[1].numpy()
    bank = DS.bank_from_lesions([(np.asarray(extents)[keep], np.asarray(labels)[keep], shape,
                                  DS.class_max_ids(seg, THRESHOLDS, "instances"))])
    rows = np.stack([DS.lower_pastes(DS.DRAWS["lesionpaste"](np.random.RandomState(50 + n), **KW), bank, 0, PATCH,
                                     THRESHOLDS, "instances", KW["max_lesions"], KW["candidates"]) for n in range(N)])
    origins = [(10, 20, 64), (90, 30, 8), (40, 150, 128), (100, 100, 40)]
    arena = Arena(img, seg, dev)
    di = torch.empty((N, 1) + PATCH, device=dev)
    ds = torch.empty((N,) + PATCH, dtype=torch.int16, device=dev)
    report = torch.empty((N, KW["max_lesions"]), dtype=torch.int32, device=dev)
    d_rows = torch.from_numpy(rows).to(dev)
    box = _InstBoxOut(N, PATCH, THRESHOLDS, 64 * N, dev)
    window = arena.call("msl_augment_window_mc", fit_rows([0] * N, [IDENT] * N), origins, PATCH, di, ds)

    def paste():
        _lib.call("msl_paste_lesions", arena.img.data_ptr(), arena.seg.data_ptr(), arena.seg.numel(), 1, arena.table.data_ptr(),
                  1, d_rows.data_ptr(), N, KW["max_lesions"], KW["candidates"], *PATCH, di.data_ptr(), ds.data_ptr(),
                  report.data_ptr(), stream)

    def build():
        window()
        box.launch(ds, stream)

    def build_paste():
        window()
        paste()
        box.launch(ds, stream)

    # the stage against its host mirror, on this very batch
    window()
    want_i, want_s = di.cpu().numpy(), ds.cpu().numpy()
    want_r = [DS.paste_lesions(want_i[n], want_s[n], rows[n], [(img[None], seg)]) for n in range(N)]
    paste()
    assert report.cpu().tolist() == want_r, "msl_paste_lesions != datasets.paste_lesions (report)"
    assert np.array_equal(ds.cpu().numpy(), want_s) and np.array_equal(di.cpu().numpy().view(np.int32), want_i.view(np.int32))
    a, b = [], []
    for _ in range(2):  # alternate the two in one process
        a.append(windows(build, args.reps, args.window))
        b.append(windows(build_paste, args.reps, args.window))
    best = lambda rs_: min(rs_, key=lambda r: r["us"])  # noqa: E731
    a, b = best(a), best(b)
    flat = [v for r in want_r for v in r]
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "window": args.window, "case": [1, *CASE],
           "batch": [N, 1, *PATCH], "max_lesions": KW["max_lesions"], "candidates": KW["candidates"], "bank_rows": len(bank.rows),
           "pastes_tested": sum(v > -2 for v in flat), "pastes_accepted": sum(v >= 0 for v in flat),
           "candidates_tried": sum((v + 1 if v >= 0 else KW["candidates"]) for v in flat if v > -2),
           "build": a, "build_paste": b, "stage_us": round(b["us"] - a["us"], 2), "paste_over_build": round(b["us"] / a["us"], 3)}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
