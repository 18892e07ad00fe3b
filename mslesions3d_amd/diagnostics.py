"""Per-parameter gradient / weight histograms and moments, computed on the device (reference ``lesions3d/ssd3d.py:729-738``:
``on_after_backward`` -> ``add_histogram("epoch/" + name, grads)`` every 25 steps).

``TensorStats`` runs ``msl_tensor_stats`` (csrc/tensorstats.hip) over the flat parameter arena and its twins - one pass, no
copy of the arena to the host: per tensor a 128-bin histogram keyed on the fp32 bit pattern and five fp64 moments.

Bins (``bin_of``): 0 non-finite, 1 +-0, ``2 + c`` negative and ``65 + c`` positive finite non-zero values of magnitude class
``c = clamp(floor(log2|x|), -42, 20) + 42`` (subnormals: class 0).  One bin per binade: a vanishing gradient walks down the
bins, an exploding one up, a NaN lands in bin 0 - on a fixed axis that is the same for every tensor and every step.

    python -m mslesions3d_amd.diagnostics LOGDIR/EXPERIMENT/grad_hist.jsonl [--step K]

prints one record of ``train.py --grad_histograms N`` as a table.
"""
import argparse
import json
import math

import numpy as np

N_BINS = 128
BIN_NONFINITE, BIN_ZERO, BIN_NEG0, BIN_POS0 = 0, 1, 2, 65
N_CLASSES = 63            # magnitude classes per sign
EXP_LO, EXP_HI = -42, 20  # floor(log2|x|) of the first / last class
SOURCES = ("grad", "param", "exp_avg")


def bin_of(values):
    """Bin index (int64 array) of every fp32 value, from its bit pattern alone (no logarithm: exact at every edge)."""
    u = np.ascontiguousarray(values, dtype=np.float32).view(np.uint32).astype(np.int64)
    mag = u & 0x7FFFFFFF
    e = mag >> 23  # biased exponent field; 0: subnormal (or zero)
    c = np.where(e == 0, 0, np.clip(e - 127, EXP_LO, EXP_HI) - EXP_LO)
    b = np.where((u >> 31) != 0, BIN_NEG0, BIN_POS0) + c
    b = np.where(mag == 0, BIN_ZERO, b)
    return np.where(mag >= 0x7F800000, BIN_NONFINITE, b)


def bin_edges():
    """float64 array of 64 magnitudes 2^-42 .. 2^21: class c holds edges[c] <= |x| < edges[c + 1], except that class 0 also
    holds everything below 2^-42 (down to the smallest subnormal) and class 62 everything from 2^20 up to FLT_MAX."""
    return np.ldexp(1.0, np.arange(EXP_LO, EXP_HI + 2))


def _class_of(b):
    return b - (BIN_NEG0 if b < BIN_POS0 else BIN_POS0)


def bin_label(b):
    b = int(b)
    if not 0 <= b < N_BINS:
        raise ValueError(f"bin {b} outside 0 .. {N_BINS - 1}")
    if b == BIN_NONFINITE:
        return "nonfinite"
    if b == BIN_ZERO:
        return "zero"
    sign, c = ("-" if b < BIN_POS0 else "+"), _class_of(b)
    if c == 0:
        return f"{sign}(0, 2^{EXP_LO + 1})"
    if c == N_CLASSES - 1:
        return f"{sign}[2^{EXP_HI}, max]"
    return f"{sign}[2^{EXP_LO + c}, 2^{EXP_LO + c + 1})"


def summarize(count, hist, moments):
    """The per-tensor dict of ``TensorStats.read``: ``hist`` 128 counts, ``moments`` = (sum, sum_sq, sum_abs, min, max) over
    the finite values.  ``mean`` / ``rms`` are over the finite values too (NaN when there is none)."""
    hist = np.asarray(hist, dtype=np.int64)
    s, q, a, lo, hi = (float(v) for v in moments)
    finite = int(count) - int(hist[BIN_NONFINITE])
    return {"count": int(count), "nonfinite": int(hist[BIN_NONFINITE]), "zeros": int(hist[BIN_ZERO]), "min": lo, "max": hi,
            "mean": s / finite if finite else float("nan"), "rms": math.sqrt(q / finite) if finite else float("nan"),
            "l1": a, "hist": hist}


class TensorStats:
    """Histograms + moments of the trainable tensors of a ``ParamArena``, for ``sources`` out of ("grad", "param", "exp_avg"):
    ``arena.grad``, ``arena.flat[:n_trainable]``, the optimiser's first moment (``optimizer=`` a ``FusedAdam``).  The segment
    and block tables are built once; ``enqueue`` is three launches on the given stream and no host synchronisation; the
    outputs are a snapshot that only the next ``enqueue`` rewrites."""

    def __init__(self, arena, sources=("grad", "param"), optimizer=None):
        import torch

        from . import _lib
        sources = tuple(sources)
        if not sources or len(set(sources)) != len(sources) or any(s not in SOURCES for s in sources):
            raise ValueError(f"sources must be a non-empty subset of {SOURCES}, got {sources}")
        if "exp_avg" in sources and optimizer is None:
            raise ValueError('the "exp_avg" source needs optimizer=')
        self.arena, self.sources, self.optimizer = arena, sources, optimizer
        self.names = [n for n in arena.names if n not in arena.no_grad_names]
        offs = [arena.offsets[n][0] for n in self.names]
        self.counts = [arena.offsets[n][1] for n in self.names]
        if any(o + n > arena.n_trainable for o, n in zip(offs, self.counts)):
            raise _lib.HipKernelError("a trainable tensor lies outside the gradient arena")
        L, dev = _lib.load(), arena.flat.device
        n_seg, n_src = len(self.names), len(sources)
        lens = np.asarray(self.counts, dtype=np.int32)
        self.n_blocks = int(L.msl_tensor_stats_block_table(lens.ctypes.data, n_seg, None, 0))
        if self.n_blocks < 1:
            raise _lib.HipKernelError("msl_tensor_stats_block_table refused the segment lengths")
        table = np.zeros(n_seg + 1 + 2 * self.n_blocks, dtype=np.int32)
        if int(L.msl_tensor_stats_block_table(lens.ctypes.data, n_seg, table.ctypes.data, table.size)) != self.n_blocks:
            raise _lib.HipKernelError("msl_tensor_stats_block_table failed")
        self.seg_off = torch.tensor(offs, dtype=torch.int64).to(dev)
        self.seg_len = torch.from_numpy(lens).to(dev)
        self.table = torch.from_numpy(table).to(dev)
        self.partials = torch.empty(int(L.msl_tensor_stats_workspace_bytes(n_src, self.n_blocks)) // 8, dtype=torch.float64,
                                    device=dev)
        # one buffer, one copy back: [n_src][n_seg][5] f64 moments, then [n_src][n_seg][128] i32 counts
        self._n_mom = n_src * n_seg * 5
        self.out = torch.zeros(self._n_mom * 8 + n_src * n_seg * N_BINS * 4, dtype=torch.uint8, device=dev)
        self.moments = self.out[:self._n_mom * 8].view(torch.float64)
        self.hist = self.out[self._n_mom * 8:].view(torch.int32)
        self.enqueued = False

    def _source(self, name):
        a = self.arena
        if name == "grad":
            return a.grad
        if name == "param":
            return a.flat[:a.n_trainable]
        m = self.optimizer.exp_avg
        if m is None or m.numel() != a.n_trainable or m.device != a.flat.device:
            from . import _lib
            raise _lib.HipKernelError("the optimiser has no first moment for this arena yet (no step taken)")
        return m

    def enqueue(self, stream=None):
        """Launch the pass on ``stream`` (a raw handle; default: the current torch stream)."""
        import torch

        from . import _lib
        if stream is None:
            stream = torch.cuda.current_stream(self.out.device).cuda_stream
        src = [_lib.ptr(self._source(s)) for s in self.sources] + [None] * (4 - len(self.sources))
        _lib.call("msl_tensor_stats", *src, len(self.sources), _lib.ptr(self.seg_off), _lib.ptr(self.seg_len), len(self.names),
                  _lib.ptr(self.table), self.n_blocks, _lib.ptr(self.partials), _lib.ptr(self.hist), _lib.ptr(self.moments),
                  stream)
        self.enqueued = True

    def read(self):
        """{tensor name: {source: {count, nonfinite, zeros, min, max, mean, rms, l1, hist}}} of the latest ``enqueue``: one
        device-to-host copy on the current stream (which must be ordered behind the stream of the enqueue)."""
        if not self.enqueued:
            return None
        host = self.out.cpu().numpy()
        n_seg, n_src = len(self.names), len(self.sources)
        mom = host[:self._n_mom * 8].view(np.float64).reshape(n_src, n_seg, 5)
        hist = host[self._n_mom * 8:].view(np.int32).reshape(n_src, n_seg, N_BINS)
        return {name: {s: summarize(self.counts[i], hist[k, i], mom[k, i]) for k, s in enumerate(self.sources)}
                for i, name in enumerate(self.names)}


# ---- the JSONL record of train.py --grad_histograms and its table ---------------------------------------------------------
def to_record(stats, step, epoch):
    """``FusedTrainer.last_stats()`` -> one JSON-serialisable record; histograms sparse ({bin: count}, non-zero bins only)."""
    tensors = {}
    for name, per_source in stats["tensors"].items():
        tensors[name] = {}
        for s, d in per_source.items():
            e = {k: d[k] for k in ("count", "nonfinite", "zeros", "min", "max", "mean", "rms", "l1")}
            e["hist"] = {str(int(b)): int(d["hist"][b]) for b in np.flatnonzero(d["hist"])}
            tensors[name][s] = e
    return {"step": int(step), "epoch": int(epoch), "grad_scale": float(stats["grad_scale"]), "tensors": tensors}


def load_records(path):
    with open(path) as f:
        return [json.loads(line) for line in f if line.strip()]


def _bin_range(entry):
    """Occupied magnitude range of a sparse histogram: labels of the lowest and highest non-empty magnitude class."""
    classes = sorted(_class_of(int(b)) for b, n in entry["hist"].items() if int(b) >= BIN_NEG0 and n)
    if not classes:
        return "-"
    lo, hi = classes[0], classes[-1]
    return f"2^{EXP_LO + lo}..2^{EXP_LO + hi + 1}"


def format_record(rec):
    """The table of one record: per tensor the gradient rms (scaled by grad_scale: the mean gradient under data parallelism),
    the parameter rms, their ratio, the non-finite counts and the occupied magnitude range of the gradient."""
    scale = float(rec.get("grad_scale", 1.0))
    rows = [("tensor", "grad rms", "param rms", "grad/param", "nonfinite g/p", "grad range")]
    for name, t in rec["tensors"].items():
        g, p = t.get("grad"), t.get("param")
        g_rms = g["rms"] * scale if g else float("nan")
        p_rms = p["rms"] if p else float("nan")
        ratio = g_rms / p_rms if p_rms and p_rms == p_rms else float("nan")
        rows.append((name, f"{g_rms:.3e}", f"{p_rms:.3e}", f"{ratio:.3e}",
                     f"{g['nonfinite'] if g else '-'}/{p['nonfinite'] if p else '-'}", _bin_range(g) if g else "-"))
    w = [max(len(r[k]) for r in rows) for k in range(len(rows[0]))]
    lines = [f"step {rec['step']}  epoch {rec['epoch']}  grad_scale {scale:g}"]
    lines += ["  ".join(c.ljust(w[k]) if k == 0 else c.rjust(w[k]) for k, c in enumerate(r)) for r in rows]
    return "\n".join(lines)


def main(argv=None):
    p = argparse.ArgumentParser(description="print one record of a grad_hist.jsonl written by train.py --grad_histograms")
    p.add_argument("file")
    p.add_argument("--step", type=int, default=None, help="the record of this step (default: the last record)")
    args = p.parse_args(argv)
    recs = load_records(args.file)
    if args.step is not None:
        recs = [r for r in recs if r["step"] == args.step]
    if not recs:
        raise SystemExit(f"{args.file}: no record" + (f" of step {args.step}" if args.step is not None else ""))
    print(format_record(recs[-1]))


if __name__ == "__main__":
    main()
