"""msl_stem_dw_fwd_eval and msl_stem_dw_fwd_eval_bf16 (stem_dw_eval_kernel of csrc/stemdw.hip) at every reachable instantiation
and every SD, against the float64 reference of tests/stemdw_ref.py (bounds derived there, not tuned; a failure prints the worst
error / bound and its index).

The cases are tests/stemdw_cases.py; tests/test_stemdw_ref_cpu.py proves at the same cases that both checks accept an honest fp32
evaluation in the kernel's order and reject thirteen kinds of wrong kernel.  Every run: the output is NaN-filled between guard
bands, the call returns 0, the guards are intact and every element is written; the end-to-end check against ``ref`` (from x);
the second-stage check against ``ref_from_y`` on the raw stem output msl_stem_conv_fwd[_bf16] stores (bound gamma(n) absdot
alone; on bf16 storage an interval test whose intervals are almost all one value); bit identity with the two launches
(msl_stem_conv_fwd + msl_dwconv_fwd) wherever msl_dwconv_fwd_eval_rows_ok answers 1 - it does at every case of the table, the
rows kernel's order being the one the fused kernel copies; and a second call on equal inputs agrees bit for bit.
With MSL_STEMDW_RATIO_LOG=<file> every comparison appends "<case id> <what> <error / bound>" to that file (for the table of
DESIGN.md, Appendix F)."""
import functools
import os

import pytest
import torch

from mslesions3d_amd import _lib
from mslesions3d_amd._lib import ptr
from tests import stemdw_cases as C
from tests import stemdw_ref as R
from tests.test_gpu_stem import DEV, Guarded, dev, same_bits, st
from tests.test_gpu_stem import _release_kept  # noqa: F401  (autouse fixture: frees what dev() and Guarded keep alive)

pytestmark = pytest.mark.gpu
CASE_IDS = C.ids(C.CASES)


@functools.lru_cache(maxsize=None)
def _data(idx, variant=0):
    return C.make_data(C.CASES[idx], variant)


@functools.lru_cache(maxsize=None)
def _stem64(idx, variant=0):
    d = _data(idx, variant)
    return R.stem64(d["x"], d["w"])


@functools.lru_cache(maxsize=None)
def _expect(idx, bf16, variant=0):
    """The end-to-end reference of a case: computed once, shared by every test, never written to."""
    d = _data(idx, variant)
    return R.ref(d["x"], d["w"], d["sc"], d["sh"], d["wd"], bf16, stem=_stem64(idx, variant))


def judge(id_, what, e, z, bf16):
    """Log and print the figure, then assert the check."""
    rep = R.check(id_, what, e, z, bf16)
    row = rep.rows[0]
    line = f"{id_} {what} {row['ratio']:.4f}"
    print(line + (f" pinned={row['pinned']:.4f}" if bf16 else ""))
    log = os.environ.get("MSL_STEMDW_RATIO_LOG")
    if log:
        with open(log, "a") as f:
            f.write(line + "\n")
    assert rep.failures() == [], "\n".join(rep.failures())


def entry(L, bf16):
    return L.msl_stem_dw_fwd_eval_bf16 if bf16 else L.msl_stem_dw_fwd_eval


def operands(d):
    return tuple(dev(d[k]) for k in ("x", "w", "sc", "sh", "wd"))


def output(N, dims, bf16):
    zd, zh, zw = R.z_dims(dims)
    return Guarded(N * 32 * zd * zh * zw, dtype=torch.bfloat16 if bf16 else torch.float32)


def fused(L, ops, N, cin, dims, bf16, z=None, stream=None):
    """One launch into a guarded, NaN-filled output (a fresh one unless given) -> (Guarded, return code)."""
    z = output(N, dims, bf16) if z is None else z
    rc = entry(L, bf16)(*(ptr(t) for t in ops), ptr(z.v), N, cin, *dims, st() if stream is None else stream)
    return z, rc


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("idx", range(len(C.CASES)), ids=CASE_IDS)
def test_stem_dw_eval(idx, bf16):
    id_, N, cin, dims = C.CASES[idx]
    L = _lib.load()
    p = R.plan(N, cin, dims)
    assert p is not None and C.id_parts(id_) == (cin, p["th"], p["aw"], p["sd"])
    assert L.msl_stem_dw_fwd_eval_supported(N, cin, *dims) == 1
    d = _data(idx)
    ops = operands(d)
    sfx = "-bf16" if bf16 else "-fp32"
    dt = torch.bfloat16 if bf16 else torch.float32
    zs = (N, 32) + R.z_dims(dims)
    z, rc = fused(L, ops, N, cin, dims, bf16)
    torch.cuda.synchronize()
    assert rc == 0, f"{id_}: returned {rc}"
    z.intact(f"{id_}: z")
    z.written(f"{id_}: z")
    zh = z.v.cpu().float().view(zs)
    judge(id_, "end-to-end" + sfx, _expect(idx, bf16), zh, bf16)
    # the raw stem output as its own kernel stores it -> the second stage alone
    ad, ah, aw = R.act_dims(dims)
    y = Guarded(N * 32 * ad * ah * aw, dtype=dt)
    stem = L.msl_stem_conv_fwd_bf16 if bf16 else L.msl_stem_conv_fwd
    assert stem(ptr(ops[0]), ptr(ops[1]), ptr(y.v), None, N, cin, *dims, 2, 2, 2, st()) == 0
    torch.cuda.synchronize()
    y.intact(f"{id_}: y")
    y.written(f"{id_}: y")
    e2 = R.ref_from_y(y.v.cpu().float().view((N, 32, ad, ah, aw)), d["sc"], d["sh"], d["wd"])
    judge(id_, "from-y" + sfx, e2, zh, bf16)
    # the two launches, bit for bit
    if L.msl_dwconv_fwd_eval_rows_ok(N, 32, ad, ah, aw, 2) == 1:
        z2 = Guarded(z.n, dtype=dt)
        if bf16:
            rc2 = L.msl_dwconv_fwd_bf16(ptr(y.v), ptr(ops[2]), ptr(ops[3]), ptr(ops[4]), ptr(z2.v), None, N, 32, ad, ah, aw, 2, st())
        else:
            rc2 = L.msl_dwconv_fwd(ptr(y.v), ptr(ops[2]), ptr(ops[3]), ptr(ops[4]), ptr(z2.v), None, N, 32, ad, ah, aw, 2, 0, st())
        torch.cuda.synchronize()
        assert rc2 == 0
        z2.intact(f"{id_}: z of the two launches")
        assert same_bits(z.v, z2.v), (f"{id_}: differs from msl_stem_conv_fwd + msl_dwconv_fwd in "
                                      f"{int((z.v.float() != z2.v.float()).sum())} elements")
    # again on equal inputs
    z3, rc3 = fused(L, ops, N, cin, dims, bf16)
    torch.cuda.synchronize()
    assert rc3 == 0
    z3.intact(f"{id_}: z, second call")
    assert same_bits(z3.v, z.v), f"{id_}: two calls on equal inputs differ"
    for t, k in zip(ops, ("x", "w", "sc", "sh", "wd")):
        assert same_bits(t, d[k].to(DEV)), f"{id_}: {k} changed"


def test_rows_kernel_takes_the_activation_map_of_every_case():
    """The bit-identity assertion of test_stem_dw_eval is skipped for no case."""
    L = _lib.load()
    for _, N, cin, dims in C.CASES:
        assert L.msl_dwconv_fwd_eval_rows_ok(N, 32, *R.act_dims(dims), 2) == 1


def test_back_to_back_launches_of_different_instantiations():
    """On a stream of its own and with no synchronisation in between: the instantiation with the largest LDS request (above
    64 KiB: the function attribute is set), a small one, the first again on other data and in the other storage type, and the
    first once more.  Every result is correct, so nothing of an earlier launch's LDS image or attribute shows."""
    L = _lib.load()
    big, small = CASE_IDS.index("c1-th4-aw96-sd1:1x12x16x192"), CASE_IDS.index("c1-th2-aw32-sd1:3x12x8x64")
    assert R.plan(*C.CASES[big][1:])["lds"] > 64 * 1024 > R.plan(*C.CASES[small][1:])["lds"]
    seq = [(big, 0, False), (small, 0, True), (big, 1, True), (small, 0, False), (big, 0, False)]
    ops = {(i, v): operands(_data(i, v)) for i, v, _ in seq}
    zs = [output(C.CASES[i][1], C.CASES[i][3], b) for i, _, b in seq]
    torch.cuda.synchronize()  # the copies and the NaN fills ran on the current stream
    s = torch.cuda.Stream()
    out = []
    for (i, v, b), z in zip(seq, zs):
        _, N, cin, dims = C.CASES[i]
        out.append(fused(L, ops[(i, v)], N, cin, dims, b, z=z, stream=s.cuda_stream))
    s.synchronize()
    torch.cuda.synchronize()
    for k, ((i, v, b), (z, rc)) in enumerate(zip(seq, out)):
        id_, N, cin, dims = C.CASES[i]
        assert rc == 0
        z.intact(f"launch {k} ({id_})")
        z.written(f"launch {k} ({id_})")
        judge(id_, f"back-to-back-{k}-{'bf16' if b else 'fp32'}", _expect(i, b, v), z.v.cpu().float().view((N, 32) + R.z_dims(dims)), b)
    assert same_bits(out[0][0].v, out[4][0].v), "the same launch before and after the others differs"


_LAUNCHED = [r for r in C.REFUSED if r[4]]


@pytest.mark.parametrize("case", _LAUNCHED, ids=C.ids(_LAUNCHED))
def test_refused_shapes_write_nothing(case):
    """MSL_ERR_UNSUPPORTED from both entry points through the raw call, no kernel launched, the output untouched."""
    id_, N, cin, dims, _ = case
    L = _lib.load()
    assert L.msl_stem_dw_fwd_eval_supported(N, cin, *dims) == 0
    vol = max(N, 1) * max(cin, 1) * dims[0] * dims[1] * dims[2]
    x, w, v, wd = dev(torch.ones(vol)), dev(torch.ones(32 * 27 * max(cin, 1))), dev(torch.ones(32)), dev(torch.ones(32 * 27))
    n0 = L.msl_thread_launch_count()
    for bf16 in (False, True):
        z = Guarded(max(N, 1) * 32 * R.cdiv(dims[0], 4) * R.cdiv(dims[1], 4) * R.cdiv(dims[2], 4), dtype=torch.bfloat16 if bf16 else torch.float32)
        rc = entry(L, bf16)(ptr(x), ptr(w), ptr(v), ptr(v), ptr(wd), ptr(z.v), N, cin, *dims, st())
        torch.cuda.synchronize()
        assert rc == R.ERR_UNSUPPORTED, f"{id_}: returned {rc}"
        z.untouched(id_)
    assert L.msl_thread_launch_count() == n0, "a refused call launched a kernel"
