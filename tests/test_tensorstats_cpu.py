"""Host side of the gradient / weight histograms (mslesions3d_amd/diagnostics.py, train.py --grad_histograms): the bit-pattern
binning against the logarithm-spelled reference of tests/tensorstats_ref.py, the record format and the table.  CPU only."""
import json
import math

import numpy as np
import pytest

from mslesions3d_amd import diagnostics as D
from tests import tensorstats_ref as R


def test_bin_of_matches_the_reference_at_every_edge():
    v = R.edge_values()
    got, ref = D.bin_of(v), R.ref_bins(v)
    assert got.tolist() == ref.tolist(), [(float(x), int(a), int(b)) for x, a, b in zip(v, got, ref) if a != b]
    # the layout itself, spelled out once
    f = np.float32
    assert D.bin_of([f(np.nan), f(np.inf), -f(np.inf)]).tolist() == [0, 0, 0]
    assert D.bin_of([f(0.0), -f(0.0)]).tolist() == [1, 1]
    assert D.bin_of([f(1.0), -f(1.0)]).tolist() == [65 + 42, 2 + 42]
    assert D.bin_of([f(2.0 ** -43), f(1e-40), f(R.TINY), f(2.0 ** -42)]).tolist() == [65, 65, 65, 65]
    assert D.bin_of([np.nextafter(f(2.0 ** -41), f(0)), f(2.0 ** -41)]).tolist() == [65, 66]
    assert D.bin_of([np.nextafter(f(2.0 ** 20), f(0)), f(2.0 ** 20), f(2.0 ** 21), f(R.FLT_MAX)]).tolist() == [126, 127, 127, 127]
    assert D.bin_of([-f(R.FLT_MAX)]).tolist() == [64]


def test_bin_of_matches_the_reference_on_random_bit_patterns():
    v = R.random_bits(np.random.default_rng(20240607), 100_000)
    got, ref = D.bin_of(v), R.ref_bins(v)
    assert np.array_equal(got, ref), int((got != ref).sum())
    # the draw reaches every bin but +-0 (two patterns out of 2^32: the edge test has them), so every bin was compared
    assert sorted(set(range(D.N_BINS)) - set(np.unique(got).tolist())) == [1]


def test_bin_edges_and_labels():
    e = D.bin_edges()
    assert e.shape == (64,) and e[0] == 2.0 ** -42 and e[-1] == 2.0 ** 21
    for c in range(1, 62):  # interior classes: the lower edge is in, the upper edge is the next class
        assert D.bin_of([np.float32(e[c])])[0] == 65 + c and D.bin_of([np.nextafter(np.float32(e[c + 1]), np.float32(0))])[0] == 65 + c
    assert D.bin_label(0) == "nonfinite" and D.bin_label(1) == "zero"
    assert D.bin_label(65 + 42) == "+[2^0, 2^1)" and D.bin_label(2 + 42) == "-[2^0, 2^1)"
    assert D.bin_label(65) == "+(0, 2^-41)" and D.bin_label(127) == "+[2^20, max]" and D.bin_label(64) == "-[2^20, max]"
    with pytest.raises(ValueError):
        D.bin_label(128)


def test_block_table_helpers_are_host_arithmetic():
    """msl_tensor_stats_block_table / _workspace_bytes: pure host code of the library (no device is touched)."""
    from mslesions3d_amd import _lib
    L = _lib.load()
    C = int(L.msl_tensor_stats_chunk())
    assert C >= 256 and C % 4 == 0
    lens = np.array([4, C, C + 1, 3 * C + 5, 1], dtype=np.int32)
    chunks = [1, 1, 2, 4, 1]
    assert L.msl_tensor_stats_block_table(lens.ctypes.data, len(lens), None, 0) == sum(chunks)
    table = np.full(len(lens) + 1 + 2 * sum(chunks) + 3, -7, dtype=np.int32)  # three spare ints behind the table
    assert L.msl_tensor_stats_block_table(lens.ctypes.data, len(lens), table.ctypes.data, table.size - 3) == sum(chunks)
    assert table[:len(lens) + 1].tolist() == [0, 1, 2, 4, 8, 9] and table[-3:].tolist() == [-7, -7, -7]
    pairs = table[len(lens) + 1:-3].reshape(-1, 2).tolist()
    assert pairs == [[s, c] for s, n in enumerate(chunks) for c in range(n)]
    assert L.msl_tensor_stats_block_table(lens.ctypes.data, len(lens), table.ctypes.data, len(lens) + 2 * sum(chunks)) == 0  # one int short
    empty = np.array([3, 0], dtype=np.int32)
    assert L.msl_tensor_stats_block_table(empty.ctypes.data, 2, None, 0) == 0  # an empty segment
    assert L.msl_tensor_stats_workspace_bytes(2, 9) == 2 * 9 * 5 * 8
    assert L.msl_tensor_stats_workspace_bytes(0, 9) == 0 and L.msl_tensor_stats_workspace_bytes(5, 9) == 0 and L.msl_tensor_stats_workspace_bytes(1, 0) == 0


def test_summarize_moments():
    v = np.array([1.0, -2.0, 0.0, np.nan, 4.0], dtype=np.float32)
    r = R.ref_stats(v)
    s = D.summarize(v.size, r["hist"], (r["sum"], r["sum_sq"], r["sum_abs"], r["min"], r["max"]))
    assert (s["count"], s["nonfinite"], s["zeros"], s["min"], s["max"], s["l1"]) == (5, 1, 1, -2.0, 4.0, 7.0)
    assert s["mean"] == 3.0 / 4 and s["rms"] == math.sqrt(21.0 / 4)
    nothing = D.summarize(2, np.bincount([0, 0], minlength=128), (0.0, 0.0, 0.0, math.inf, -math.inf))
    assert nothing["nonfinite"] == 2 and math.isnan(nothing["mean"]) and math.isnan(nothing["rms"])


def _hand_made_record():
    def entry(values):
        v = np.asarray(values, dtype=np.float32)
        r = R.ref_stats(v)
        return D.summarize(v.size, r["hist"], (r["sum"], r["sum_sq"], r["sum_abs"], r["min"], r["max"]))
    stats = {"step": 50, "grad_scale": 0.5, "tensors": {
        "base.features.0.0.weight": {"grad": entry([0.5, -0.5, 0.5, -0.5]), "param": entry([2.0, 2.0, -2.0, 2.0])},
        "pred_convs.cl_conv3.bias": {"grad": entry([np.nan, 3e-5, 0.0]), "param": entry([1.0, np.inf, 1.0])}}}
    return D.to_record(stats, stats["step"], 3)


def test_cli_prints_the_table_of_a_record(tmp_path, capsys):
    rec = _hand_made_record()
    g = rec["tensors"]["base.features.0.0.weight"]["grad"]
    assert g["hist"] == {str(2 + 41): 2, str(65 + 41): 2}  # sparse: +-0.5 = class floor(log2 0.5) + 42 = 41
    other = dict(rec, step=25)
    path = tmp_path / "grad_hist.jsonl"
    path.write_text(json.dumps(other) + "\n" + json.dumps(rec) + "\n")
    assert [r["step"] for r in D.load_records(str(path))] == [25, 50]
    D.main([str(path)])  # default: the last record
    out = capsys.readouterr().out
    lines = out.splitlines()
    assert lines[0] == "step 50  epoch 3  grad_scale 0.5"
    assert lines[1].split() == ["tensor", "grad", "rms", "param", "rms", "grad/param", "nonfinite", "g/p", "grad", "range"]
    # gradient rms 0.5 scaled by grad_scale 0.5; parameter rms 2; ratio 0.125; nothing non-finite; one occupied binade
    assert lines[2].split() == ["base.features.0.0.weight", "2.500e-01", "2.000e+00", "1.250e-01", "0/0", "2^-1..2^0"]
    row = lines[3].split()
    assert row[0] == "pred_convs.cl_conv3.bias" and row[4] == "1/1" and row[5] == "2^-16..2^-15"
    D.main([str(path), "--step", "25"])
    assert capsys.readouterr().out.splitlines()[0].startswith("step 25 ")
    with pytest.raises(SystemExit):
        D.main([str(path), "--step", "26"])


def test_grad_histograms_flag_and_logging_points(tmp_path):
    from mslesions3d_amd.train import GradHistogramLog, build_parser
    assert build_parser().parse_args([]).grad_histograms == 0
    assert build_parser().parse_args(["--grad_histograms", "25"]).grad_histograms == 25

    class Trainer:  # last_stats() of a trainer whose latest stats step started from global_step `step`
        step = None

        def last_stats(self):
            return {"step": self.step, "grad_scale": 1.0, "tensors": {}}

    path, tr = tmp_path / "grad_hist.jsonl", Trainer()
    log = GradHistogramLog(25, str(path))
    asked = []
    for gs in range(60):
        if log.before_step(tr, gs, gs // 30):
            asked.append(gs)
            # a record is never read right after its own step: what is on disk now is from the logging points before this one
            assert [r["step"] for r in D.load_records(str(path))] == asked[:-1] if path.exists() else asked == [0]
            tr.step = gs
    assert asked == [0, 25, 50]
    log.close(tr)
    assert [(r["step"], r["epoch"]) for r in D.load_records(str(path))] == [(0, 0), (25, 0), (50, 1)]
    assert not GradHistogramLog(0, None).wanted(0)
