"""msl_tensor_stats (csrc/tensorstats.hip) through the C ABI, and its users ``diagnostics.TensorStats`` /
``FusedTrainer.step(..., stats=True)``, against the float64 / logarithm reference of tests/tensorstats_ref.py.

Histograms, min and max are compared exactly; the three sums against ``R.sum_bound`` (n * 2^-52 * sum of the absolute
terms: the bound of any summation order of exactly representable terms).  Every output and the workspace sit between
canary words."""
import functools
import math

import numpy as np
import pytest
import torch

from mslesions3d_amd import _lib
from mslesions3d_amd._lib import ptr
from tests import tensorstats_ref as R
from tests.golden import detinit

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = 64  # canary words on each side
CANARY_I, CANARY_D = 0x5A5A5A5A, -12345.678


def st():
    return torch.cuda.current_stream().cuda_stream


def chunk():
    return int(_lib.load().msl_tensor_stats_chunk())


def segment_lengths():
    C = chunk()
    return [1, 3, 4, 5, 63, 64, 65, C - 1, C, C + 1, 3 * C + 5]


@functools.lru_cache(maxsize=None)
def arena_case():
    """Four flat sources over one back-to-back segment table (most starts misaligned), and their reference, made once.
    Values: random bit patterns with the edge values of the binning sprinkled in; per source k one segment of zeros
    ((4 + k) % 11), one of NaN ((5 + k) % 11) and one of finite values with a single -Inf ((6 + k) % 11), so that the special
    segments also fall on the multi-chunk ones."""
    lens = segment_lengths()
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    total, edges = int(sum(lens)), R.edge_values()
    srcs = []
    for k in range(4):
        rng = np.random.default_rng(1000 + k)
        v = R.random_bits(rng, total).copy()
        where = rng.choice(total, size=total // 16, replace=False)
        v[where] = edges[rng.integers(0, len(edges), size=where.size)]
        for s, (o, n) in enumerate(zip(offs, lens)):
            if s == (4 + k) % 11:
                v[o:o + n] = np.float32(0) if k % 2 == 0 else -np.float32(0)
            elif s == (5 + k) % 11:
                v[o:o + n] = np.float32(np.nan)
            elif s == (6 + k) % 11:
                seg = v[o:o + n]
                seg[~np.isfinite(seg)] = np.float32(1.5)
                seg[n // 2] = -np.float32(np.inf)
        srcs.append(v)
    ref = [[R.ref_stats(v[o:o + n]) for o, n in zip(offs, lens)] for v in srcs]
    return lens, offs, srcs, ref


class Guarded:
    def __init__(self, n, dtype, canary, fill):
        self.n, self.canary = n, canary
        self.full = torch.full((n + 2 * G,), canary, dtype=dtype, device=DEV)
        self.v = self.full[G:G + n]
        self.v.fill_(fill)  # garbage the kernels must overwrite: nothing here is cleared by the caller

    def intact(self, what):
        band = torch.cat([self.full[:G], self.full[G + self.n:]]).cpu()
        assert bool((band == self.canary).all()), f"{what}: wrote outside its range"


class Launch:
    """Device tables + guarded outputs for the first n_src sources of ``arena_case``; ``run()`` -> (hist, moments) on the host."""

    def __init__(self, n_src, misalign=1):
        L = _lib.load()
        lens, offs, srcs, _ = arena_case()
        self.n_src, self.n_seg = n_src, len(lens)
        lens32 = np.asarray(lens, dtype=np.int32)
        self.n_blocks = int(L.msl_tensor_stats_block_table(lens32.ctypes.data, self.n_seg, None, 0))
        assert self.n_blocks == sum(-(-n // chunk()) for n in lens)
        table = np.full(self.n_seg + 1 + 2 * self.n_blocks, -1, dtype=np.int32)
        assert int(L.msl_tensor_stats_block_table(lens32.ctypes.data, self.n_seg, table.ctypes.data, table.size)) == self.n_blocks
        assert table[0] == 0 and table[self.n_seg] == self.n_blocks and (table >= 0).all()
        # source k starts k + misalign elements into its allocation: the 16-byte phase differs per source
        self.src = []
        for k in range(n_src):
            buf = torch.zeros(srcs[k].size + 8, dtype=torch.float32, device=DEV)
            view = buf[k + misalign:k + misalign + srcs[k].size]
            view.copy_(torch.from_numpy(srcs[k].view(np.int32)).to(DEV).view(torch.float32))
            self.src.append(view)
        self.seg_off = torch.from_numpy(offs).to(DEV)
        self.seg_len = torch.from_numpy(lens32).to(DEV)
        self.table = torch.from_numpy(table).to(DEV)
        ws = int(L.msl_tensor_stats_workspace_bytes(n_src, self.n_blocks))
        assert ws == n_src * self.n_blocks * 5 * 8
        self.ws = Guarded(ws // 8, torch.float64, CANARY_D, float("nan"))
        self.hist = Guarded(n_src * self.n_seg * 128, torch.int32, CANARY_I, 7777)
        self.mom = Guarded(n_src * self.n_seg * 5, torch.float64, CANARY_D, float("nan"))

    def run(self):
        p = [ptr(s) for s in self.src] + [None] * (4 - self.n_src)
        _lib.call("msl_tensor_stats", *p, self.n_src, ptr(self.seg_off), ptr(self.seg_len), self.n_seg, ptr(self.table),
                  self.n_blocks, ptr(self.ws.v), ptr(self.hist.v), ptr(self.mom.v), st())
        torch.cuda.synchronize()
        for g, what in ((self.ws, "workspace"), (self.hist, "hist"), (self.mom, "moments")):
            g.intact(what)
        return (self.hist.v.cpu().numpy().reshape(self.n_src, self.n_seg, 128).copy(),
                self.mom.v.cpu().numpy().reshape(self.n_src, self.n_seg, 5).copy())


def check_against_reference(hist, mom, ref, lens, what):
    """hist (128,), mom (5,) of one (source, segment) against its ``R.ref_stats``."""
    assert hist.sum() == lens, f"{what}: the bins hold {hist.sum()} of {lens} elements"
    assert np.array_equal(hist.astype(np.int64), ref["hist"]), \
        f"{what}: bins differ at {np.flatnonzero(hist != ref['hist']).tolist()}"
    assert mom[3] == ref["min"] and mom[4] == ref["max"], f"{what}: min / max {mom[3]!r} {mom[4]!r} vs {ref['min']!r} {ref['max']!r}"
    n = ref["n_finite"]
    for k, key, terms in ((0, "sum", ref["sum_abs"]), (1, "sum_sq", ref["sum_sq"]), (2, "sum_abs", ref["sum_abs"])):
        err, bound = abs(float(mom[k]) - ref[key]), R.sum_bound(n, terms)
        print(f"{what} {key}: error {err:.3e} bound {bound:.3e}")
        assert err <= bound, f"{what} {key}: {mom[k]!r} vs {ref[key]!r}: error {err:.3e} over the bound {bound:.3e}"


@pytest.mark.parametrize("n_src", [1, 2, 4])
def test_synthetic_arena_matches_the_reference(n_src):
    lens, _, _, ref = arena_case()
    hist, mom = Launch(n_src).run()
    for k in range(n_src):
        for s, n in enumerate(lens):
            check_against_reference(hist[k, s], mom[k, s], ref[k][s], n, f"source {k} segment {s} (length {n})")
    # the special segments of source 0, spelled out
    assert hist[0, 4, 1] == lens[4] and tuple(mom[0, 4]) == (0.0, 0.0, 0.0, 0.0, 0.0)
    assert hist[0, 5, 0] == lens[5] and tuple(mom[0, 5]) == (0.0, 0.0, 0.0, math.inf, -math.inf)
    assert hist[0, 6, 0] == 1 and math.isfinite(mom[0, 6, 3])


def test_runs_are_bit_identical_and_need_no_caller_side_clearing():
    a = Launch(4)
    h1, m1 = a.run()
    h2, m2 = a.run()  # the same buffers again, nothing cleared in between: hist would double if the zeroing were the caller's
    h3, m3 = Launch(4).run()  # fresh buffers at the same 16-byte phases: the same bits again
    for h, m in ((h2, m2), (h3, m3)):
        assert np.array_equal(h1, h)
        assert np.array_equal(m1.view(np.int64), m.view(np.int64))
    # another 16-byte phase moves elements between the peel, the 16-byte loads and the tail: another summation order, so
    # only what does not depend on the order is identical - and everything still meets the reference
    lens, _, _, ref = arena_case()
    h4, m4 = Launch(4, misalign=3).run()
    assert np.array_equal(h1, h4) and np.array_equal(m1[..., 3:], m4[..., 3:])
    for k in range(4):
        for s, n in enumerate(lens):
            check_against_reference(h4[k, s], m4[k, s], ref[k][s], n, f"phase 3: source {k} segment {s}")


def test_bad_arguments_launch_nothing():
    L = _lib.load()
    a = Launch(1)
    p = ptr(a.src[0])
    args = lambda **kw: [kw.get("src0", p), None, None, None, kw.get("n_src", 1), ptr(a.seg_off), ptr(a.seg_len), kw.get("n_seg", a.n_seg),
                         ptr(a.table), kw.get("n_blocks", a.n_blocks), ptr(a.ws.v), kw.get("hist", ptr(a.hist.v)), ptr(a.mom.v), st()]
    for bad in (dict(n_src=0), dict(n_src=5), dict(n_src=2), dict(src0=None), dict(n_seg=0), dict(n_blocks=a.n_seg - 1), dict(hist=None)):
        assert L.msl_tensor_stats(*args(**bad)) == -1, bad
    lens = np.array([4, 0], dtype=np.int32)
    assert L.msl_tensor_stats_block_table(lens.ctypes.data, 2, None, 0) == 0      # an empty segment
    assert L.msl_tensor_stats_block_table(None, 2, None, 0) == 0
    lens = np.array([4, 5], dtype=np.int32)
    small = np.zeros(6, dtype=np.int32)
    assert L.msl_tensor_stats_block_table(lens.ctypes.data, 2, small.ctypes.data, small.size) == 0  # needs 2 + 1 + 2 * 2 ints
    assert L.msl_tensor_stats_workspace_bytes(0, 4) == 0 and L.msl_tensor_stats_workspace_bytes(5, 4) == 0
    torch.cuda.synchronize()
    assert bool((a.hist.v == 7777).all())  # nothing was launched


# ---- through the trainer ---------------------------------------------------------------------------------------------------
SIZE, N = (64, 64, 64), 2  # config C64


def hip_model():
    from mslesions3d_amd.ssd3d import LSSD3D
    m = LSSD3D(n_classes=2, input_channels=1, input_size=SIZE, threshold=[0.1, 0.2], lr=1e-3)
    m.load_state_dict(detinit.fill_state_dict(m.state_dict(), 1234))
    return m.to(DEV).train()


def check_entry(entry, values, what):
    """One {count, nonfinite, zeros, min, max, mean, rms, l1, hist} dict of ``read()`` against the fp32 tensor it describes."""
    ref = R.ref_stats(values)
    n = ref["n_finite"]
    assert entry["count"] == values.size and entry["hist"].dtype == np.int64 and entry["hist"].shape == (128,), what
    assert np.array_equal(entry["hist"], ref["hist"]), f"{what}: bins differ at {np.flatnonzero(entry['hist'] != ref['hist']).tolist()}"
    assert entry["nonfinite"] == ref["hist"][0] and entry["zeros"] == ref["hist"][1], what
    assert entry["min"] == ref["min"] and entry["max"] == ref["max"], what
    u = 2.0 ** -53
    assert abs(entry["l1"] - ref["sum_abs"]) <= R.sum_bound(n, ref["sum_abs"]), what
    # mean = sum / n: the sum's bound over n, plus the rounding of the division
    mean = ref["sum"] / n
    assert abs(entry["mean"] - mean) <= R.sum_bound(n, ref["sum_abs"]) / n + 2 * u * abs(mean), what
    # rms = sqrt(sum_sq / n): half the relative error of sum_sq (n * 2^-52), plus the roundings of the division and the root
    rms = math.sqrt(ref["sum_sq"] / n)
    assert abs(entry["rms"] - rms) <= rms * (n * 2.0 ** -53 + 4 * u), what


def test_trainer_stats_are_a_snapshot_of_their_step_and_change_nothing():
    from mslesions3d_amd.diagnostics import TensorStats
    from mslesions3d_amd.trainer import FusedTrainer
    data = [(detinit.make_volume_batch(5 + s, N, 1, SIZE).to(DEV),) + detinit.make_gt(8 + s, N, SIZE) for s in range(2)]
    m, twin = hip_model(), hip_model()
    tr, tr_twin = FusedTrainer(m), FusedTrainer(twin)
    assert tr.last_stats() is None
    tr.step(*data[0], stats=True)
    arena = m._engine.arena
    grad, flat = arena.grad.clone(), arena.flat.clone()  # (the step was synchronous: these are its gradient and its update)
    tr.step(*data[1], stats=False)
    stats = tr.last_stats()
    assert stats["step"] == 0 and stats["grad_scale"] == 1.0
    params = dict(m.named_parameters())
    trainable = [k for k in m.state_dict() if k in params and k not in arena.no_grad_names]
    assert sorted(stats["tensors"]) == sorted(trainable) and len(trainable) == len(params) - len(arena.no_grad_names)
    grad, flat = grad.cpu().numpy(), flat.cpu().numpy()
    for name in trainable:
        off, n = arena.offsets[name]
        assert n == params[name].numel()
        rec = stats["tensors"][name]
        assert sorted(rec) == ["grad", "param"]
        check_entry(rec["grad"], grad[off:off + n], f"{name} grad")
        check_entry(rec["param"], flat[off:off + n], f"{name} param")
    # the pass reads: two steps with it leave the bits two steps without it leave
    for d in data:
        tr_twin.step(*d)
    assert torch.equal(arena.flat, twin._engine.arena.flat)
    assert tr.last_stats()["step"] == 0  # still the first step's snapshot
    # the optimiser's first moment as a source
    ts = TensorStats(arena, ("exp_avg",), optimizer=tr.opt)
    ts.enqueue()
    got, exp_avg = ts.read(), tr.opt.exp_avg.cpu().numpy()
    for name in trainable[:4] + trainable[-4:]:
        off, n = arena.offsets[name]
        check_entry(got[name]["exp_avg"], exp_avg[off:off + n], f"{name} exp_avg")


@pytest.mark.parametrize("cache", [1, 0])
def test_train_entry_point_writes_records_the_cli_prints(tmp_path, capsys, cache):
    """train.py --grad_histograms 3 on a toy set (8 training cases, batch 2, 2 epochs = global steps 0 .. 7): one record per
    logging point, the last one flushed at the end of the run, printable by the diagnostics CLI."""
    import json

    from mslesions3d_amd import datasets as DS
    from mslesions3d_amd import diagnostics as D
    from mslesions3d_amd import train as T
    DS.generate_artificial_dataset(str(tmp_path / "data"), "toy64", num_images=10, image_size=(64, 64, 64))
    args = T.build_parser().parse_args(["-d", str(tmp_path / "data"), "-dn", "toy64", "-b", "2", "-me", "2", "-ld", str(tmp_path / "logs"),
                                        "-en", "run", "-c", str(cache), "--grad_histograms", "3"])
    model = T.example(args)
    path = str(tmp_path / "logs" / "run" / "grad_hist.jsonl")
    recs = D.load_records(path)
    assert recs == [json.loads(l) for l in open(path)]  # plain JSON lines
    assert [r["step"] for r in recs] == list(range(0, model.global_step, 3)) and model.global_step == 8
    params = dict(model.named_parameters())
    trainable = sorted(k for k in model.state_dict() if k in params and k != "rescale_factors")
    for r in recs:
        assert r["grad_scale"] == 1.0 and r["epoch"] == r["step"] // 4 and sorted(r["tensors"]) == trainable
        for name, t in r["tensors"].items():
            assert sorted(t) == ["grad", "param"]
            for e in t.values():
                assert e["count"] == params[name].numel() == sum(e["hist"].values()) and all(n > 0 for n in e["hist"].values())
                assert e["nonfinite"] == 0 and math.isfinite(e["rms"])
    capsys.readouterr()
    D.main([path, "--step", "3"])
    out = capsys.readouterr().out.splitlines()
    assert out[0].startswith("step 3 ") and len(out) == 2 + len(trainable) and {l.split()[0] for l in out[2:]} == set(trainable)


def test_injected_nan_is_attributed_to_its_tensor():
    from mslesions3d_amd.diagnostics import TensorStats
    m = hip_model()
    dev = torch.device(DEV, torch.cuda.current_device())
    m._ensure_device_state(dev)
    arena = m._engine.ensure_arena(dev)
    ts = TensorStats(arena, ("param",))
    victim = ts.names[len(ts.names) // 2]
    off, n = arena.offsets[victim]
    with torch.no_grad():
        arena.flat[off + n // 2] = float("nan")
    ts.enqueue()
    got = ts.read()
    assert {name: rec["param"]["nonfinite"] for name, rec in got.items() if rec["param"]["nonfinite"]} == {victim: 1}
    assert got[victim]["param"]["hist"][0] == 1 and got[victim]["param"]["count"] == n
