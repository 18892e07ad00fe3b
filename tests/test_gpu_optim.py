"""Every entry point of csrc/optim.hip that computes - msl_adam_step, msl_grad_reduce_table_set / _batch / _batch_indexed,
msl_nan_flag, msl_nan_flag2, msl_fill_u32 - path by path against the float64 reference of tests/optim_ref.py (bounds derived
there, not tuned; each failure message prints the worst error / bound and its index).

The cases are CPU data of tests/optim_cases.py; tests/test_optim_ref_cpu.py proves at the same cases that every bound accepts a
plain fp32 evaluation and rejects a copy off by 2**-18 or short of one slab.  Every output sits between guard bands that must
come back bit for bit; fold destinations are pre-filled with NaN and must be written completely; source columns that no entry
owns hold NaN.  Each fold table runs in the search form and in the indexed form the engine launches (block_entry built from the
counts msl_grad_reduce_table_set returns, like Engine._grad_reduce), twice each, into fresh outputs: all four bit-identical.
With MSL_OPTIM_RATIO_LOG=<file> every comparison appends "<group> <case> <error / bound>" to that file."""
import ctypes
import os

import numpy as np
import pytest
import torch

from mslesions3d_amd import _lib
from mslesions3d_amd._lib import ptr
from tests import optim_cases as C
from tests import optim_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = 64  # guard elements on each side of every output (a multiple of 4: an unshifted view stays 16-byte aligned)
NAN = float("nan")
ERR_ARG = -1


def st():
    return torch.cuda.current_stream().cuda_stream


_KEEP = []


def dev(t):
    """Move to the GPU and keep the tensor alive until the end of the test."""
    d = t.detach().to(DEV).contiguous()
    _KEEP.append(d)
    return d


@pytest.fixture(autouse=True)
def _release_kept():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


def same_bits(a, b):
    """Bit identity of two device tensors of one dtype (NaN payloads and zero signs included)."""
    it = {1: torch.uint8, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return a.dtype == b.dtype and bool(torch.equal(a.contiguous().view(it), b.contiguous().view(it)))


class Guarded:
    """A buffer of n elements, ``off`` elements past a 16-byte boundary, between two guard bands; everything holds ``fill``
    (NaN, or a sentinel for integers) until ``load``.  ``intact`` / ``untouched`` compare bits with the state after the last
    load."""

    def __init__(self, n, dtype=torch.float32, off=0, fill=NAN):
        self.n, self.lo = n, G + off
        self.full = torch.full((n + 2 * G + 4,), fill, dtype=dtype, device=DEV)
        self.v = self.full[self.lo:self.lo + n]
        self.before = self.full.clone()
        assert (self.v.data_ptr() - 4 * off) % 16 == 0 or dtype not in (torch.float32, torch.int32)
        _KEEP.append(self)

    def load(self, data):
        self.v.copy_(data)
        self.before = self.full.clone()
        return self

    def intact(self, what):
        lo, hi = self.lo, self.lo + self.n
        ok = same_bits(self.full[:lo], self.before[:lo]) and same_bits(self.full[hi:], self.before[hi:])
        assert ok, f"{what}: wrote outside its range"

    def untouched(self, what):
        assert same_bits(self.full, self.before), f"{what}: a refused call wrote to its output"

    def written(self, what):
        bad = int(torch.isnan(self.v).sum())
        assert bad == 0, f"{what}: {bad} elements were never written (or are NaN)"


def log_ratio(group, what, ratio):
    log = os.environ.get("MSL_OPTIM_RATIO_LOG")
    if log:
        with open(log, "a") as f:
            f.write(f"{group} {what.replace(' ', '_')} {ratio:.4f}\n")


def check(group, what, actual, ref, bound):
    ratio, idx, bad = R.worst(actual, ref, bound)
    log_ratio(group, what, ratio)
    a, r = actual.detach().cpu().double().reshape(-1), ref.double().reshape(-1)
    assert bad == 0, (f"{group} {what}: {bad}/{r.numel()} elements over their bound; worst error / bound {ratio:.3f} at idx {idx} "
                      f"(got {a[idx].item():.9e}, ref {r[idx].item():.9e})")


def launches():
    return _lib.load().msl_thread_launch_count()


# ------------------------------------------------------------------------------------------------- Adam
class AdamRun:
    """p, exp_avg, exp_avg_sq guarded and loaded, g / hp / mask on the device; ``step`` launches msl_adam_step."""

    def __init__(self, x, mask, n):
        self.n = n
        self.P, self.M, self.V = (Guarded(n).load(x[k]) for k in "pmv")
        self.mask = dev(mask)
        self.mask0 = self.mask.clone()

    def step(self, g, hp, n=None):
        gd, hpd = dev(g), dev(torch.from_numpy(np.asarray(hp, dtype=np.float32)))
        rc = _lib.load().msl_adam_step(ptr(self.P.v), ptr(gd), ptr(self.M.v), ptr(self.V.v), ptr(hpd), ptr(self.mask),
                                       self.n if n is None else n, st())
        torch.cuda.synchronize()
        assert same_bits(gd, g.to(DEV)) and same_bits(self.mask, self.mask0), "an input was written"
        assert same_bits(hpd, torch.from_numpy(np.asarray(hp, dtype=np.float32)).to(DEV)), "hp was written"
        return rc

    def outputs(self):
        return (("p", self.P), ("m", self.M), ("v", self.V))


@pytest.mark.parametrize("case", C.ADAM_CASES, ids=[C.adam_id(c) for c in C.ADAM_CASES])
def test_adam_single_step(case):
    """One step from arbitrary state: p, exp_avg and exp_avg_sq each inside its own bound at every element; the all-zero
    block stays exactly 0; above one grid pass the last 300 elements are checked by themselves and must have moved."""
    n, mk, gs, wd, bt = case
    x, mask, hp = C.adam_inputs(n), C.adam_mask(n, mk), C.adam_hp(gs, wd, bt)
    ref = R.adam_step(x["p"], x["g"], x["m"], x["v"], hp, mask)
    run = AdamRun(x, mask, n)
    assert run.step(x["g"], hp) == 0
    zb = C.zero_block(n)
    for i, (name, out) in enumerate(run.outputs()):
        out.intact(f"adam {name}")
        got = out.v.cpu()
        assert bool(torch.isfinite(got).all()), f"adam {name}: not finite"
        check(f"adam-{name}", C.adam_id(case), got, ref[i], ref[3 + i])
        assert bool((got[zb] == 0).all()), f"adam {name}: the all-zero block moved"
        if n > C.ADAM_PASS:
            check(f"adam-{name}", C.adam_id(case) + "-tail", got[-300:], ref[i][-300:], ref[3 + i][-300:])
            if name != "p":  # (a parameter may legitimately keep its bits: an update below half an ulp)
                assert bool((got[-300:] != x[name][-300:]).all()), f"adam {name}: elements of the tail still hold their input"
    if n > C.ADAM_PASS:
        assert bool((run.P.v.cpu()[-300:] != x["p"][-300:]).any()), "adam p: the tail still holds its input"


def test_adam_three_steps():
    """3 steps on n = 10007 with the state carried on the device: p, exp_avg, exp_avg_sq inside the bounds the reference
    accumulates (every step takes the previous step's bounds as the uncertainty of its inputs)."""
    n = 10007
    x, mask = C.adam_inputs(n), C.adam_mask(n, "every7")
    run = AdamRun(x, mask, n)
    rp, rm, rv, bp, bm, bv = x["p"].double(), x["m"].double(), x["v"].double(), None, None, None
    for step in (1, 2, 3):
        g = C.adam_inputs(n, seed=step)["g"]
        hp = C.adam_hp(1.0 / 3.0, 5e-4, (0.9, 0.999), step)
        rp, rm, rv, bp, bm, bv = R.adam_step(rp, g, rm, rv, hp, mask, bp, bm, bv)
        assert run.step(g, hp) == 0
        for (name, out), r, b in zip(run.outputs(), (rp, rm, rv), (bp, bm, bv)):
            out.intact(f"adam {name}, step {step}")
            check(f"adam3-{name}", f"step{step}", out.v.cpu(), r, b)


@pytest.mark.parametrize("n", (0, -5))
def test_adam_refuses_empty(n):
    x, mask = C.adam_inputs(256), C.adam_mask(256, "every7")
    run = AdamRun(x, mask, 256)
    n0 = launches()
    assert run.step(x["g"], C.adam_hp(1.0, 5e-4, (0.9, 0.999)), n=n) == ERR_ARG
    assert launches() == n0, "a refused call launched a kernel"
    for name, out in run.outputs():
        out.untouched(f"adam {name}")


# ------------------------------------------------------------------------------------------------- gradient fold
def table_set(host, k, first, kind, src, dst, dst2, ns, count, stride, p=(0, 0, 0)):
    return _lib.load().msl_grad_reduce_table_set(ctypes.addressof(host) if host is not None else None, k, first, kind, src, dst,
                                                 dst2, ns, count, stride, *p)


def host_table(n):
    return (ctypes.c_ubyte * (_lib.load().msl_grad_reduce_entry_bytes() * n))()


def run_table(tab, bufs, form):
    """Fresh guarded NaN destinations for every row, the table, one launch in ``form`` ('search' | 'indexed').
    -> (destinations per row, workgroups per row)."""
    L = _lib.load()
    rows = tab["rows"]
    host = host_table(len(rows))
    outs, nbs, owner, first = [], [], [], 0
    for k, row in enumerate(rows):
        buf = bufs[row["buf"]]
        src = buf.data_ptr() + row["off"] * buf.element_size()
        dsts = [Guarded(n, off=o) for n, o in zip(C.dst_sizes(row), row["dst_off"])]
        dst2 = ptr(dsts[1].v) if row["kind"] == 3 else None
        if row["kind"] == 4:
            dst2 = ptr(dev(torch.tensor([row["npos"]], dtype=torch.int32)))
        nb = table_set(host, k, first, row["kind"], src, ptr(dsts[0].v), dst2, row["ns"], row["count"], row["stride"], row["p"])
        want = C.blocks(row["kind"], row["ns"], row["count"], row["stride"], src % 16 == 0, dsts[0].v.data_ptr() % 16 == 0)
        assert nb == want, f"{row['what']}: msl_grad_reduce_table_set returned {nb} workgroups, its documentation says {want}"
        outs.append(dsts)
        nbs.append(nb)
        owner += [k] * nb  # Engine._grad_reduce
        first += nb
    table = dev(torch.frombuffer(bytearray(host), dtype=torch.uint8))
    if form == "indexed":
        rc = L.msl_grad_reduce_batch_indexed(ptr(table), len(rows), ptr(dev(torch.tensor(owner, dtype=torch.int32))), first, st())
    else:
        rc = L.msl_grad_reduce_batch(ptr(table), len(rows), first, st())
    torch.cuda.synchronize()
    assert rc == 0
    return outs, nbs


def check_table(tab, name):
    """The table in both forms, twice each: the first run against the reference, all four bit-identical, guards intact."""
    bufs = [dev(b) for b in tab["buffers"]]
    runs = [run_table(tab, bufs, form) for form in ("search", "indexed", "search", "indexed")]
    for k, row in enumerate(tab["rows"]):
        what = f"{name}: {row['what']}"
        refs, bounds = C.reference(tab, row)
        for j, out in enumerate(runs[0][0][k]):
            out.intact(what)
            out.written(what)
            if row["kind"] == 4:
                got = out.v.cpu().numpy()
                assert C.in_loss_range(got, refs[j], bounds[j]), f"{what}: got {got}, expected {refs[j]} .. {bounds[j]}"
                assert got[2] == row["npos"]
                exact = R.loss_fold(C.src_matrix(tab, row).numpy(), row["npos"])
                log_ratio("kind4", what, float(np.any(got.view(np.uint32) != exact.view(np.uint32))))  # 0: loss_fold's bits
            else:
                check(f"kind{row['kind']}", what, out.v, refs[j], bounds[j])
            for r, form in zip(runs[1:], ("indexed", "search again", "indexed again")):
                assert same_bits(r[0][k][j].full, out.full), f"{what}: the {form} run differs from the first search run"
    for b, b0 in zip(bufs, tab["buffers"]):
        assert same_bits(b, b0.to(DEV)), f"{name}: a source was written"
    return runs[0][1]


@pytest.mark.parametrize("ns", C.SLAB_COUNTS)
def test_fold_slabs_and_stem(ns):
    """Kinds 0 and 2 at one slab count: counts below 4, multiples and non-multiples of 4 and 32, just above 1024 and 2048, each
    at stride == count, at a larger multiple of 4 and at a non-multiple; the stem image for Cin = 1, 2, 4.  Around GR_FEW
    (16 / 17), the 4-way unroll and its remainder, and k + 56 < nslabs (56 / 57, 64 / 65, 121, 130)."""
    tab = C.slab_table(ns)
    nbs = check_table(tab, f"ns{ns}")
    forms = {C.few_form(r["kind"], r["ns"], r["count"], r["stride"]) for r in tab["rows"]}
    assert forms == ({True, False} if ns <= C.GR_FEW else {False})
    assert len(nbs) == 3 * len(C.COUNTS) + 3


def test_fold_unaligned_pointers():
    """Few-slab cases whose source or destination is 1 to 3 floats off a 16-byte boundary: the entry takes the 32-outputs form
    (cdiv(count, 32) workgroups) and is right all the same; an unaligned destination of a kind that stores float by float changes nothing."""
    nbs = check_table(C.unaligned_table(), "unaligned")
    assert nbs == [C.cdiv(1028, 32)] * 3 + [C.cdiv(2048, 32), C.cdiv(6912, 32), C.cdiv(2048, 1024)]


@pytest.mark.parametrize("ns", C.HEAD_NS)
@pytest.mark.parametrize("ncls", C.HEAD_NCLS)
def test_fold_head_scales(ncls, ns):
    """Kind 3 for C = 16 and 48 (MT = 1 and 2; 12 + 2 ncls below, at and above a 16-row tile edge and 32) with the two head-bias
    rows of Engine._grad_reduce (count 12 from ``bias``, count 2 ncls from ``bias[12:]``, stride 16 MT).  check_table demands
    every element of dloc_w and dcl_w written and the guards around them NaN."""
    check_table(C.head_table(ncls, ns), f"head ncls{ncls} ns{ns}")


@pytest.mark.parametrize("NP", C.ELEM_NP)
def test_fold_f64_partials(NP):
    """Kind 1: NP around the lane count (31, 32, 33), the 8-deep unroll (p + 224 < NP: 224, 225, 256, 257) and beyond; counts
    that end 1 and 7 elements into a workgroup's 8-element pass, on the pass boundary and on the workgroup boundary."""
    check_table(C.elem_table(NP), f"NP{NP}")


@pytest.mark.parametrize("ns,npos", C.LOSS_CASES)
def test_fold_loss(ns, npos):
    """Kind 4: bit for bit optim_ref.loss_fold of the sums (a double sum's order error allowed before the cast); 0 positives
    yields what the float32 expression yields."""
    check_table(C.loss_table(ns, npos), f"loss ns{ns} npos{npos}")


def test_fold_mixed_table_at_the_limit():
    """64 entries of all kinds, a kind-4 entry in the middle, in both forms; 65 entries are refused."""
    L = _lib.load()
    tab = C.mixed_table()
    assert len(tab["rows"]) == 64
    check_table(tab, "mixed")
    out, table, owner = Guarded(64), dev(torch.zeros(65 * L.msl_grad_reduce_entry_bytes(), dtype=torch.uint8)), dev(torch.zeros(65, dtype=torch.int32))
    n0 = launches()
    assert L.msl_grad_reduce_batch(ptr(table), 65, 65, st()) == ERR_ARG
    assert L.msl_grad_reduce_batch_indexed(ptr(table), 65, ptr(owner), 65, st()) == ERR_ARG
    torch.cuda.synchronize()
    assert launches() == n0
    out.untouched("65 entries")


def test_fold_refusals():
    """Bad arguments return an error before any launch and leave the outputs as they were."""
    L = _lib.load()
    src, out, out2 = dev(torch.randn(4 * 64)), Guarded(64), Guarded(64)
    npos = dev(torch.tensor([3], dtype=torch.int32))
    parts = dev(torch.rand(8, dtype=torch.float64))
    host = host_table(2)
    s, d = ptr(src), ptr(out.v)
    n0 = launches()
    assert table_set(host, 0, 0, 0, s, d, None, 4, 64, 64) == 1  # (the good call these are variations of)
    for what, args in (("kind -1", (host, 0, 0, -1, s, d, None, 4, 64, 64)), ("kind 5", (host, 0, 0, 5, s, d, None, 4, 64, 64)),
                       ("null src", (host, 0, 0, 0, None, d, None, 4, 64, 64)), ("null dst", (host, 0, 0, 0, s, None, None, 4, 64, 64)),
                       ("nslabs 0", (host, 0, 0, 0, s, d, None, 0, 64, 64)), ("count 0", (host, 0, 0, 0, s, d, None, 4, 0, 64)),
                       ("kind 4 without dst2", (host, 0, 0, 4, ptr(parts), d, None, 4, 1, 0)), ("kind 3 as kind 9", (host, 0, 0, 9, s, d, ptr(out2.v), 4, 64, 64)),
                       ("null table", (None, 0, 0, 0, s, d, None, 4, 64, 64)), ("index -1", (host, -1, 0, 0, s, d, None, 4, 64, 64))):
        assert table_set(*args) < 0, what
    assert table_set(host, 0, 0, 4, ptr(parts), d, ptr(npos), 4, 1, 0) == 1
    assert table_set(host, 0, 0, 0, s, d, None, 4, 64, 64) == 1
    table, owner = dev(torch.frombuffer(bytearray(host), dtype=torch.uint8)), dev(torch.zeros(1, dtype=torch.int32))
    t, o = ptr(table), ptr(owner)
    for what, rc in (("null table", L.msl_grad_reduce_batch(None, 1, 1, st())), ("no entries", L.msl_grad_reduce_batch(t, 0, 1, st())),
                     ("total_blocks 0", L.msl_grad_reduce_batch(t, 1, 0, st())),
                     ("indexed: null table", L.msl_grad_reduce_batch_indexed(None, 1, o, 1, st())),
                     ("indexed: null block_entry", L.msl_grad_reduce_batch_indexed(t, 1, None, 1, st())),
                     ("indexed: no entries", L.msl_grad_reduce_batch_indexed(t, 0, o, 1, st())),
                     ("indexed: total_blocks 0", L.msl_grad_reduce_batch_indexed(t, 1, o, 0, st()))):
        assert rc == ERR_ARG, what
    torch.cuda.synchronize()
    assert launches() == n0, "a refused call launched a kernel"
    out.untouched("refusals")
    out2.untouched("refusals")
    assert L.msl_grad_reduce_batch_indexed(t, 1, o, 1, st()) == 0  # and the table they refused is a good one
    torch.cuda.synchronize()
    assert launches() == n0 + 1
    check("kind0", "after refusals", out.v, src.cpu().view(4, 64).double().sum(0), 3 * R.U * src.cpu().view(4, 64).double().abs().sum(0))


# ------------------------------------------------------------------------------------------------- NaN flags, fill
SENTINEL = 0x5A5A5A5A
NANS = (("nan", 0x7FC00000), ("-nan", 0xFFC00000 - (1 << 32)), ("payload", 0x7FA12345), ("-payload", 0xFF800001 - (1 << 32)))


def clean_values(n, seed):
    """Finite and infinite values that are no NaN: +-inf, +-0, the largest finite value, the smallest subnormal, normals."""
    special = torch.tensor([float("inf"), -float("inf"), 0.0, -0.0, 3.4028234663852886e38, -3.4028234663852886e38, 1e-45, -1e-45])
    x = torch.randn(n, generator=C.gen(seed))
    k = torch.arange(n)
    return torch.where(k % 5 == 0, special[(k // 5) % 8], x)


class Flag:
    def __init__(self, value):
        self.g = Guarded(1, dtype=torch.int32, fill=SENTINEL).load(torch.tensor([value], dtype=torch.int32))

    def set(self, value):
        self.g.load(torch.tensor([value], dtype=torch.int32))

    def read(self, what):
        torch.cuda.synchronize()
        self.g.intact(what)
        return int(self.g.v.item())


@pytest.mark.parametrize("n", (1, 63, 64, 65, 100000, C.NAN_PASS, C.NAN_PASS + 1, 2 * C.NAN_PASS + 5))
def test_nan_flag(n):
    """One NaN (positive, negative, with payloads) at the first element, the last, and just past the first grid pass sets the
    bit on top of the bits already there; +-inf, +-0, the largest finite value and a subnormal do not."""
    L = _lib.load()
    x = dev(clean_values(n, n))
    xi = x.view(torch.int32)
    flag = Flag(4)
    assert L.msl_nan_flag(ptr(x), n, ptr(flag.g.v), 2, st()) == 0
    assert flag.read("clean") == 4, "a tensor without NaN set the flag"
    for k, pos in enumerate(sorted({0, n - 1, n // 2} | ({C.NAN_PASS, C.NAN_PASS + 3} if n > C.NAN_PASS + 3 else set()))):
        if pos >= n:
            continue
        name, bits = NANS[k % 4]
        keep = int(xi[pos].item())
        xi[pos] = bits
        flag.set(4)
        assert L.msl_nan_flag(ptr(x), n, ptr(flag.g.v), 2, st()) == 0
        assert flag.read(f"{name} at {pos}") == 6, f"{name} at {pos} of {n} was not seen"
        flag.set(0)
        assert L.msl_nan_flag(ptr(x), n, ptr(flag.g.v), 1 << 30, st()) == 0
        assert flag.read(f"{name} at {pos}") == 1 << 30
        xi[pos] = keep
    flag.set(4)
    assert L.msl_nan_flag(ptr(x), n, ptr(flag.g.v), 2, st()) == 0
    assert flag.read("clean again") == 4


def test_nan_flag_every_nan_pattern_and_empty():
    L = _lib.load()
    x = dev(clean_values(1000, 3))
    flag = Flag(4)
    for name, bits in NANS:
        xi = x.view(torch.int32)
        xi[999] = bits
        flag.set(4)
        assert L.msl_nan_flag(ptr(x), 1000, ptr(flag.g.v), 1, st()) == 0
        assert flag.read(name) == 5, name
    n0 = launches()
    flag.set(4)
    assert L.msl_nan_flag(ptr(x), 0, ptr(flag.g.v), 1, st()) == 0  # n == 0: OK, nothing launched, the NaN at 999 not seen
    assert flag.read("n == 0") == 4 and launches() == n0


BIG = C.NAN_PASS + 300


@pytest.mark.parametrize("na,nb", ((BIG, 1000), (1000, BIG), (70, 64), (64, 257), (0, 500), (500, 0), (0, 0)))
def test_nan_flag2(na, nb):
    """Two tensors in one launch sized by the larger: a NaN only in a, only in b (past na where b is the longer one; past the
    first grid pass where it is the big one), in both, in neither -> exactly the expected bits on top of the ones there."""
    L = _lib.load()
    a, b = dev(clean_values(max(na, 1), 11)), dev(clean_values(max(nb, 1), 12))
    flag = Flag(8)
    n0 = launches()
    for in_a in (False, True):
        for in_b in (False, True):
            a2, b2 = a.clone(), b.clone()
            _KEEP.extend([a2, b2])
            if in_a:
                a2.view(torch.int32)[max(na, 1) - 1] = NANS[1][1]  # the last element (past one pass if a is the big one)
            if in_b:
                b2.view(torch.int32)[max(nb, 1) - 1] = NANS[2][1]  # likewise; past na whenever nb > na
            flag.set(8)
            assert L.msl_nan_flag2(ptr(a2), na, 1, ptr(b2), nb, 2, ptr(flag.g.v), st()) == 0
            want = 8 | (1 if in_a and na else 0) | (2 if in_b and nb else 0)
            assert flag.read(f"a {in_a} b {in_b}") == want, f"NaN in a: {in_a}, in b: {in_b}, na {na}, nb {nb}"
    assert launches() == n0 + (4 if na or nb else 0)


@pytest.mark.parametrize("side", (False, True), ids=("current", "side"))
@pytest.mark.parametrize("count", (0, 1, 1000003))
def test_fill_u32(count, side):
    L = _lib.load()
    pattern = 0xA1B2C3D4
    buf = Guarded(max(count, 1), dtype=torch.int32, fill=SENTINEL)
    torch.cuda.synchronize()
    s = torch.cuda.Stream() if side else torch.cuda.current_stream()
    assert L.msl_fill_u32(ptr(buf.v), pattern, count, s.cuda_stream) == 0
    s.synchronize()
    torch.cuda.synchronize()
    buf.intact(f"fill {count}")
    if count == 0:
        buf.untouched("fill 0")
    else:
        assert bool((buf.v == pattern - (1 << 32)).all()), "a word does not hold the pattern"
        assert buf.v.cpu().numpy().view(np.uint8)[:4].tolist() == [0xD4, 0xC3, 0xB2, 0xA1]
