"""Every detection-head entry point of csrc/heads.hip - msl_head_conv_fwd, msl_head_conv_fwd_bf16, msl_head_grad_pack,
msl_head_pack_weights[_batch | _bf16], msl_head_conv_bwd_data[_bf16], msl_head_conv_bwd_weight[_bf16] (direct, and deferred through
msl_grad_reduce_batch) - route by route against the float64 reference of tests/heads_ref.py (bounds measured there on the CPU,
never on the GPU; a failure prints the worst error / bound and its index).

The cases are the CPU data of tests/heads_cases.py; tests/test_heads_ref_cpu.py proves at the same cases that every check accepts
honest fp32 and rejects thirteen kinds of wrong kernel.  Every test first asserts the route its case id names - against the plan
mirror and, through the three host-only queries, against the library - and then runs.  Workspaces are allocated at exactly the
queried size between two bands of sentinels, poisoned (NaN, then 3e38) before every call, and every entry runs twice: the two
results must agree bit for bit.  Outputs are NaN-filled between sentinel bands.  Every line printed is
"<case id> <entry> route=<route> <what>=<error / bound> ..."; with MSL_HEADS_RATIO_LOG=<file> the line is appended to that file.

Largest error / bound per entry on the MI355X (first run of this file):
    fwd             locs 0.1373   scores 0.1358
    fwd_bf16        locs 0.1522   scores 0.1838
    bwd_data        ga 0.3037
    bwd_data_bf16   ga 0.9991 (of B + half a bf16 ulp: the rounding itself; the assertion is the rounding interval)
    bww             dloc_w 0.1137   dcl_w 0.1453   dloc_b 0.2418   dcl_b 0.2570
    bww_bf16        dloc_w 0.1186   dcl_w 0.1110   dloc_b 0.2418   dcl_b 0.2570
(direct and deferred form alike: they are the same bits)
"""
import ctypes
import functools
import os

import pytest
import torch

from mslesions3d_amd import _lib
from mslesions3d_amd._lib import ptr
from tests import heads_cases as C
from tests import heads_ref as R
from tests.test_gpu_pw import Guarded, dev, same_bits, st
from tests.test_gpu_pw import _release_kept  # noqa: F401  (autouse fixture: frees what dev() and Guarded keep alive)
from tests.test_heads_ref_cpu import assert_route

pytestmark = pytest.mark.gpu
NAN = float("nan")
SENT = -7.5  # sentinel of guard bands, halos and the rows of other scales
POISONS = (NAN, 3.0e38)
ERR_ARG, ERR_UNSUPPORTED = -1, -2


@functools.lru_cache(maxsize=None)
def data(case):
    return C.make_data(case)


@functools.lru_cache(maxsize=None)
def reference(case, bf16):
    """Computed once per case and shared by the tests; nothing writes to it."""
    return R.reference(data(case), bf16)


def route_of(case, p):
    return R.bf16_route_name(case[2]) if case[0].startswith("bf16.") else R.route_name(p)


def judge(case, entry, p, rep, tag=""):
    """Print (and log) the figures, then assert every check."""
    line = f"{case[0]} {entry}{tag} route={route_of(case, p)} " + " ".join(f"{r['what']}={r['ratio']:.4f}" for r in rep.rows)
    print(line)
    log = os.environ.get("MSL_HEADS_RATIO_LOG")
    if log:
        with open(log, "a") as f:
            f.write(line + "\n")
    assert rep.failures() == [], "\n".join(rep.failures())


def sentinel_buffer(n, dtype=torch.float32):
    """n NaN elements between two bands of sentinels."""
    return Guarded(n, dtype=dtype, guard=SENT)


def workspace(nbytes, poison):
    assert nbytes % 4 == 0
    ws = sentinel_buffer(nbytes // 4)
    ws.v.fill_(poison)
    return ws


def padded_fp32(a):
    """(N, C, D + 2, H + 2, W + 2) with a zero halo: what the fp32 kernels read."""
    return dev(torch.nn.functional.pad(a, (1, 1, 1, 1, 1, 1)))


def padded_cl_bf16(a):
    """(N, D + 2, H + 2, W + 2, C) bf16 channels-last with a zero halo: what the bf16 kernels read."""
    return dev(torch.nn.functional.pad(a, (1, 1, 1, 1, 1, 1)).permute(0, 2, 3, 4, 1).contiguous().to(torch.bfloat16))


def packed_weights(d, Cc, ncls):
    """msl_head_pack_weights into NaN-filled guarded buffers -> (Wf, Wb) Guarded."""
    L = _lib.load()
    ne = L.msl_head_packed_weight_elems(Cc, ncls)
    Wf, Wb = sentinel_buffer(ne), sentinel_buffer(ne)
    rc = L.msl_head_pack_weights(ptr(dev(d["lw"])), ptr(dev(d["cw"])), ptr(Wf.v), ptr(Wb.v), Cc, ncls, st())
    torch.cuda.synchronize()
    assert rc == 0
    Wf.intact("Wf")
    Wb.intact("Wb")
    return Wf, Wb


def row_buffers(N, S, Ptot, off, ncls):
    """locs (N, Ptot, 6) and scores (N, Ptot, ncls): NaN in the scale's rows, sentinels in every other row and around the buffer."""
    out = []
    for width in (6, ncls):
        b = sentinel_buffer(N * Ptot * width)
        v = b.v.view(N, Ptot, width)
        v.fill_(SENT)
        v[:, off:off + 2 * S] = NAN
        out.append((b, v))
    return out


def rows_of_scale(case, bufs, S, off, what):
    """The sentinel rows before and after the scale's rows, of locs AND scores; -> the scale's rows on the host."""
    res = []
    for (b, v), name in zip(bufs, ("locs", "scores")):
        b.intact(f"{case[0]} {what}: {name}")
        assert bool((v[:, :off] == SENT).all()) and bool((v[:, off + 2 * S:] == SENT).all()), f"{case[0]} {what}: {name} rows of another scale"
        res.append(v[:, off:off + 2 * S].cpu())
    return tuple(res)


def assert_same(a, b, what):
    for x, y in zip(a, b):
        assert same_bits(x.float(), y.float()), f"{what}: two runs differ"


# ------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("case", C.CASES, ids=C.ids(C.CASES))
def test_head_fwd(case):
    """msl_head_conv_fwd: register-fed and LDS-staged (cubic and tiled) kernels, every K split with its finalize, one and two output
    tiles; once at prior_off = 10 inside a longer prior list and once as an exact fit (prior_off = 0, Ptot = 2 S)."""
    id_, N, Cc, dims, ncls = case
    L = _lib.load()
    p = assert_route(case)
    d, e, S = data(case), reference(case, False), dims[0] * dims[1] * dims[2]
    pad, (Wf, Wb) = padded_fp32(d["a"]), packed_weights(d, Cc, ncls)
    lb, cb = dev(d["lb"]), dev(d["cb"])
    nbytes = L.msl_head_fwd_workspace_bytes(N, Cc, *dims, ncls)
    assert (nbytes > 0) == (p["fwd"]["ksg"] > 1)
    outs = []
    for (off, Ptot), poison in zip(((10, 2 * S + 14), (0, 2 * S)), POISONS):
        ws = workspace(nbytes, poison)
        bufs = row_buffers(N, S, Ptot, off, ncls)
        rc = L.msl_head_conv_fwd(ptr(pad), ptr(Wf.v), ptr(lb), ptr(cb), ptr(bufs[0][1]), ptr(bufs[1][1]), ptr(ws.v), N, Cc, *dims, Ptot, off,
                                 ncls, st())
        torch.cuda.synchronize()
        assert rc == 0, f"{id_}: returned {rc}"
        ws.intact(f"{id_}: forward workspace")
        outs.append(rows_of_scale(case, bufs, S, off, f"fwd off{off}"))
        judge(case, "fwd", p, R.check(case, "fwd", e, outs[-1]), tag=f"@{off}")
    assert_same(outs[0], outs[1], f"{id_}: forward")


@pytest.mark.parametrize("case", C.BF16_CASES, ids=C.ids(C.BF16_CASES))
def test_head_fwd_bf16(case):
    """msl_head_conv_fwd_bf16 on the bf16 channels-last copy: every length of the tail loop, ragged last tile, ncls 1 and 2."""
    id_, N, Cc, dims, ncls = case
    L = _lib.load()
    p = assert_route(case)
    d, e, S = data(case), reference(case, True), dims[0] * dims[1] * dims[2]
    a_cl = padded_cl_bf16(d["a"])
    Wp = sentinel_buffer(L.msl_head_packed_weight_bf16_elems(Cc), dtype=torch.bfloat16)
    assert L.msl_head_pack_weights_bf16(ptr(dev(d["lw"])), ptr(dev(d["cw"])), ptr(Wp.v), Cc, ncls, st()) == 0
    lb, cb = dev(d["lb"]), dev(d["cb"])
    outs = []
    for off, Ptot in ((10, 2 * S + 14), (0, 2 * S)):
        bufs = row_buffers(N, S, Ptot, off, ncls)
        rc = L.msl_head_conv_fwd_bf16(ptr(a_cl), ptr(Wp.v), ptr(lb), ptr(cb), ptr(bufs[0][1]), ptr(bufs[1][1]), N, Cc, *dims, Ptot, off, ncls,
                                      st())
        torch.cuda.synchronize()
        assert rc == 0, f"{id_}: returned {rc}"
        outs.append(rows_of_scale(case, bufs, S, off, f"fwd_bf16 off{off}"))
        judge(case, "fwd_bf16", p, R.check(case, "fwd_bf16", e, outs[-1]), tag=f"@{off}")
    Wp.intact(f"{id_}: Wp")
    assert_same(outs[0], outs[1], f"{id_}: bf16 forward")


# ------------------------------------------------------------------------------------------------- packing
@pytest.mark.parametrize("case", C.CASES, ids=C.ids(C.CASES))
def test_head_grad_pack(case):
    """msl_head_grad_pack: the interior (pre-filled with NaN) is the scale's rows exactly, rows at and above 12 + 2 ncls are exactly
    zero, the halo (pre-filled with a sentinel) is left alone."""
    id_, N, Cc, dims, ncls = case
    L = _lib.load()
    assert_route(case)
    d, S, co = data(case), dims[0] * dims[1] * dims[2], 12 + 2 * ncls
    off, Ptot = 10, 2 * S + 14
    g = torch.Generator().manual_seed(1)
    dl, dc = torch.randn((N, Ptot, 6), generator=g), torch.randn((N, Ptot, ncls), generator=g)  # other scales' rows: noise
    dl[:, off:off + 2 * S], dc[:, off:off + 2 * S] = R.to_rows(d["dO"], ncls)
    CO = 16 * R.head_mt(ncls)
    shape = (N, CO) + tuple(s + 2 for s in dims)
    outs = []
    for _ in range(2):
        buf = sentinel_buffer(N * CO * (dims[0] + 2) * (dims[1] + 2) * (dims[2] + 2))
        v = buf.v.view(shape)
        v.fill_(SENT)
        v[:, :, 1:-1, 1:-1, 1:-1] = NAN
        rc = L.msl_head_grad_pack(ptr(dev(dl)), ptr(dev(dc)), ptr(v), N, *dims, Ptot, off, ncls, st())
        torch.cuda.synchronize()
        assert rc == 0
        buf.intact(f"{id_}: dO_pad")
        got = v.cpu()
        inner = got[:, :, 1:-1, 1:-1, 1:-1]
        assert same_bits(inner[:, :co].contiguous(), d["dO"]), f"{id_}: interior differs from the rows"
        assert same_bits(inner[:, co:].contiguous(), torch.zeros_like(inner[:, co:])), f"{id_}: padded channels are not zero"
        halo = got.clone()
        halo[:, :, 1:-1, 1:-1, 1:-1] = SENT
        assert bool((halo == SENT).all()), f"{id_}: the halo was written"
        outs.append(got)
    assert same_bits(outs[0], outs[1])


PACK_SHAPES = [(16, 1), (16, 2), (48, 2), (32, 3), (80, 10), (256, 2)]


@pytest.mark.parametrize("Cc,ncls", PACK_SHAPES)
def test_head_pack_weights(Cc, ncls):
    """msl_head_pack_weights against the two layout formulas; rows at and above 12 + 2 ncls are zero."""
    case = (f"pack:{Cc}-ncls{ncls}", 1, Cc, (1, 1, 1), ncls)
    d = C.make_data(case)
    Wf, Wb = packed_weights(d, Cc, ncls)
    rep = R.check(case, "pack", None, (Wf.v.cpu(), Wb.v.cpu()), d)
    assert rep.failures() == [], "\n".join(rep.failures())


@pytest.mark.parametrize("Cc,ncls", [(32, 1), (32, 2), (64, 2), (96, 2), (128, 1)])
def test_head_pack_weights_bf16(Cc, ncls):
    """msl_head_pack_weights_bf16 against the layout formula in its comment: [tap][C / 32][lane][8], co = lane & 15,
    ci = 32 cg + 8 (lane >> 4) + j; rows at and above 12 + 2 ncls are zero."""
    L = _lib.load()
    d = C.make_data((f"pack16:{Cc}-ncls{ncls}", 1, Cc, (1, 1, 1), ncls))
    want = R.pack_bf16_expect(d["lw"], d["cw"], ncls)
    assert L.msl_head_packed_weight_bf16_elems(Cc) == want.numel()
    Wp = sentinel_buffer(want.numel(), dtype=torch.bfloat16)
    assert L.msl_head_pack_weights_bf16(ptr(dev(d["lw"])), ptr(dev(d["cw"])), ptr(Wp.v), Cc, ncls, st()) == 0
    torch.cuda.synchronize()
    Wp.intact("Wp")
    got = Wp.v.cpu().float()
    assert same_bits(got, want), f"{int((got != want).sum())} of {want.numel()} packed bf16 weights differ"
    rows = got.view(27, Cc // 32, 4, 16, 8)[:, :, :, 12 + 2 * ncls:]
    assert rows.numel() > 0 or ncls == 2
    assert same_bits(rows.contiguous(), torch.zeros_like(rows)), "rows at and above 12 + 2 ncls are not zero"


@pytest.mark.parametrize("ncls", [2, 3])
@pytest.mark.parametrize("chans", [(128, 256, 512, 16), (16, 512), (48,), (32, 16, 80)])
def test_head_pack_weights_batch_is_the_single_launches_bit_for_bit(chans, ncls):
    """msl_head_pack_weights_batch (what the engine calls every step) == one msl_head_pack_weights per scale; the widest scale,
    which sizes the launch, is not the first entry."""
    L = _lib.load()
    n = len(chans)
    ds = [C.make_data((f"batch:{k}:{c}", 1, c, (1, 1, 1), ncls)) for k, c in enumerate(chans)]
    single = [packed_weights(d, c, ncls) for d, c in zip(ds, chans)]
    lws, cws = [dev(d["lw"]) for d in ds], [dev(d["cw"]) for d in ds]
    out = [(sentinel_buffer(s[0].n), sentinel_buffer(s[1].n)) for s in single]
    P = ctypes.c_void_p * n
    arrs = [P(*[ptr(t) for t in lws]), P(*[ptr(t) for t in cws]), P(*[ptr(o[0].v) for o in out]), P(*[ptr(o[1].v) for o in out]),
            (ctypes.c_int * n)(*chans)]
    rc = L.msl_head_pack_weights_batch(*[ctypes.addressof(a) for a in arrs], n, ncls, st())
    torch.cuda.synchronize()
    assert rc == 0
    for k in range(n):
        for j, name in ((0, "Wf"), (1, "Wb")):
            out[k][j].intact(f"scale {k} {name}")
            assert same_bits(out[k][j].v, single[k][j].v), f"scale {k} of {chans}: {name} differs from the single launch"


def test_head_pack_weights_refusals():
    """n = 0, n = 5, a C that is no multiple of 16, ncls < 1 and ncls >= 11: refused, nothing written."""
    L = _lib.load()
    lw, cw = dev(torch.ones(12 * 512 * 27)), dev(torch.ones(22 * 512 * 27))
    Wf, Wb = Guarded(512 // 4 * 27 * 3 * 64), Guarded(512 // 4 * 27 * 3 * 64)
    P5, I5 = ctypes.c_void_p * 5, ctypes.c_int * 5
    arrs = [P5(*[ptr(lw)] * 5), P5(*[ptr(cw)] * 5), P5(*[ptr(Wf.v)] * 5), P5(*[ptr(Wb.v)] * 5)]
    addr = [ctypes.addressof(a) for a in arrs]
    chans_ok, chans_bad = I5(16, 16, 16, 16, 16), I5(16, 24, 16, 16, 16)
    ok = ctypes.addressof(chans_ok)
    for n in (0, 5, -1):
        assert L.msl_head_pack_weights_batch(*addr, ok, n, 2, st()) == ERR_ARG
    assert L.msl_head_pack_weights_batch(*addr, ctypes.addressof(chans_bad), 2, 2, st()) == ERR_ARG
    for ncls in (0, -3, 11):
        assert L.msl_head_pack_weights_batch(*addr, ok, 2, ncls, st()) == ERR_ARG
        assert L.msl_head_pack_weights(ptr(lw), ptr(cw), ptr(Wf.v), ptr(Wb.v), 16, ncls, st()) == ERR_ARG
    assert L.msl_head_pack_weights(ptr(lw), ptr(cw), ptr(Wf.v), ptr(Wb.v), 24, 2, st()) == ERR_ARG
    assert L.msl_head_pack_weights_bf16(ptr(lw), ptr(cw), ptr(Wf.v), 48, 2, st()) == ERR_UNSUPPORTED
    assert L.msl_head_pack_weights_bf16(ptr(lw), ptr(cw), ptr(Wf.v), 32, 3, st()) == ERR_UNSUPPORTED
    assert L.msl_head_pack_weights_bf16(ptr(lw), ptr(cw), ptr(Wf.v), 32, 0, st()) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    Wf.untouched("a refused weight packing")
    Wb.untouched("a refused weight packing")


# ------------------------------------------------------------------------------------------------- bwd-data
@pytest.mark.parametrize("bf16_out", [0, 1], ids=["fp32", "bf16out"])
@pytest.mark.parametrize("case", C.CASES, ids=C.ids(C.CASES))
def test_head_bwd_data(case, bf16_out):
    """msl_head_conv_bwd_data[_bf16]: register-fed (C % 64 != 0, waves that exit) and LDS-staged kernels (ragged last channel
    group, 1 to 4 tiles per workgroup), one and two output tiles."""
    id_, N, Cc, dims, ncls = case
    L = _lib.load()
    p = assert_route(case)
    d, e = data(case), reference(case, False)
    entry = "bwd_data_bf16" if bf16_out else "bwd_data"
    dO = dev(R.dO_padded(d["dO"], ncls))
    _, Wb = packed_weights(d, Cc, ncls)
    fn = L.msl_head_conv_bwd_data_bf16 if bf16_out else L.msl_head_conv_bwd_data
    outs = []
    for poison in POISONS:
        ga = sentinel_buffer(d["a"].numel(), dtype=torch.bfloat16 if bf16_out else torch.float32)
        ga.v.fill_(poison)
        rc = fn(ptr(dO), ptr(Wb.v), ptr(ga.v), N, Cc, *dims, ncls, st())
        torch.cuda.synchronize()
        assert rc == 0, f"{id_}: returned {rc}"
        ga.intact(f"{id_}: g_a")
        outs.append((ga.v.cpu().float().view(d["a"].shape),))
    judge(case, entry, p, R.check(case, entry, e, outs[0]))
    assert_same(outs[0], outs[1], f"{id_}: {entry}")


# ------------------------------------------------------------------------------------------------- weight and bias gradients
@pytest.mark.parametrize("bf16_cl", [0, 1], ids=["fp32", "bf16cl"])
@pytest.mark.parametrize("case", C.CASES, ids=C.ids(C.CASES))
def test_head_bwd_weight(case, bf16_cl):
    """msl_head_conv_bwd_weight[_bf16], direct and deferred (slabs left in the workspace, then msl_grad_reduce_batch kind 3 on
    the weight slabs and kind 0 on the bias slabs, as the training step does): both inside the bound, and equal bit for bit."""
    from tests.test_gpu_kernels import grad_reduce
    id_, N, Cc, dims, ncls = case
    L = _lib.load()
    p = assert_route(case)
    d, e = data(case), reference(case, bool(bf16_cl))
    entry = "bww_bf16" if bf16_cl else "bww"
    MT, co = p["MT"], 12 + 2 * ncls
    dO = dev(R.dO_padded(d["dO"], ncls))
    feat = padded_cl_bf16(d["a"]) if bf16_cl else padded_fp32(d["a"])
    fn = L.msl_head_conv_bwd_weight_bf16 if bf16_cl else L.msl_head_conv_bwd_weight
    nbytes = L.msl_head_bwd_weight_workspace_bytes(N, Cc, *dims, ncls)
    ns = L.msl_head_conv_bwd_weight_nslabs(N, Cc, *dims, ncls)
    slab = (Cc // 16) * 27 * MT * 256
    assert ns == p["bww"]["nblocks"] and nbytes == (ns * slab + ns * 16 * MT) * 4

    def outputs():
        return [sentinel_buffer(n) for n in (12 * Cc * 27, 2 * ncls * Cc * 27, 12, 2 * ncls)]

    def read(bufs, what):
        for b in bufs:
            b.intact(f"{id_}: {what}")
        return (bufs[0].v.cpu().view(12, Cc, 3, 3, 3), bufs[1].v.cpu().view(2 * ncls, Cc, 3, 3, 3), bufs[2].v.cpu(), bufs[3].v.cpu())

    direct = []
    for poison in POISONS:
        ws, o = workspace(nbytes, poison), outputs()
        rc = fn(ptr(dO), ptr(feat), ptr(o[0].v), ptr(o[1].v), ptr(o[2].v), ptr(o[3].v), ptr(ws.v), N, Cc, *dims, ncls, st())
        torch.cuda.synchronize()
        assert rc == 0, f"{id_}: returned {rc}"
        ws.intact(f"{id_}: weight-gradient workspace")
        direct.append(read(o, "direct"))
    judge(case, entry, p, R.check(case, entry, e, direct[0]), tag=":direct")
    assert_same(direct[0], direct[1], f"{id_}: {entry} direct")

    ws, o = workspace(nbytes, NAN), outputs()
    rc = fn(ptr(dO), ptr(feat), None, None, None, None, ptr(ws.v), N, Cc, *dims, ncls, st())
    torch.cuda.synchronize()
    assert rc == 0
    bias = ws.v[ns * slab:]
    assert bias.numel() == ns * 16 * MT
    grad_reduce([(3, ws.v, o[0].v, o[1].v, ns, slab, slab, Cc, MT, co),
                 (0, bias, o[2].v, None, ns, 12, 16 * MT, 0, 0, 0),
                 (0, bias[12:], o[3].v, None, ns, 2 * ncls, 16 * MT, 0, 0, 0)])
    ws.intact(f"{id_}: weight-gradient workspace (deferred)")
    deferred = read(o, "deferred")
    judge(case, entry, p, R.check(case, entry, e, deferred), tag=":deferred")
    for x, y, name in zip(direct[0], deferred, ("dloc_w", "dcl_w", "dloc_b", "dcl_b")):
        assert same_bits(x, y), f"{id_}: {name} of the direct and the deferred form differ in {int((x != y).sum())} elements"


# ------------------------------------------------------------------------------------------------- refusals
BAD_SHAPES = [  # (N, C, D, H, W, ncls)
    (1, 16, 2, 2, 2, 11), (1, 16, 2, 2, 2, 12), (1, 16, 2, 2, 2, 0), (1, 16, 2, 2, 2, -1), (0, 16, 2, 2, 2, 2), (-1, 16, 2, 2, 2, 2),
    (1, 16, 0, 2, 2, 2), (1, 16, 2, 0, 2, 2), (1, 16, 2, 2, -2, 2), (1, 24, 2, 2, 2, 2), (1, 8, 2, 2, 2, 2)]


def test_head_refusals():
    """Bad arguments -> ERR_ARG (the bf16 forward: ERR_UNSUPPORTED for what its one kernel cannot take) before any launch: by
    return code, and nothing is written.  Every buffer is sized for ncls = 11 (three output tiles of a 2 x 2 x 2 map, 32
    channels), so that a build without the checks would still stay inside them."""
    L = _lib.load()
    nvol, rows = 4 * 4 * 4, 2 * 8 + 14
    src = dev(torch.ones(32 * 48 * nvol))                      # feature map / dO_pad / rows, whichever the call reads
    srcb = dev(torch.ones(32 * 48 * nvol).to(torch.bfloat16))
    w = dev(torch.ones(L.msl_head_packed_weight_elems(32, 10) * 2))
    outs = [Guarded(32 * 48 * nvol) for _ in range(4)]
    outb = Guarded(32 * 48 * nvol, dtype=torch.bfloat16)
    ws = Guarded(64 * 2 * 27 * 3 * 256 + 64 * 48)
    for N, Cc, D, H, W, ncls in BAD_SHAPES:
        shape = (N, Cc, D, H, W)
        assert L.msl_head_conv_fwd(ptr(src), ptr(w), ptr(src), ptr(src), ptr(outs[0].v), ptr(outs[1].v), ptr(ws.v), *shape, rows, 0, ncls,
                                   st()) == ERR_ARG, shape
        assert L.msl_head_conv_fwd_bf16(ptr(srcb), ptr(w), ptr(src), ptr(src), ptr(outs[0].v), ptr(outs[1].v), *shape, rows, 0, ncls,
                                        st()) in (ERR_ARG, ERR_UNSUPPORTED), shape
        assert L.msl_head_conv_bwd_data(ptr(src), ptr(w), ptr(outs[0].v), *shape, ncls, st()) == ERR_ARG, shape
        assert L.msl_head_conv_bwd_data_bf16(ptr(src), ptr(w), ptr(outb.v), *shape, ncls, st()) == ERR_ARG, shape
        for fn, feat in ((L.msl_head_conv_bwd_weight, src), (L.msl_head_conv_bwd_weight_bf16, srcb)):
            assert fn(ptr(src), ptr(feat), ptr(outs[0].v), ptr(outs[1].v), ptr(outs[2].v), ptr(outs[3].v), ptr(ws.v), *shape, ncls,
                      st()) == ERR_ARG, shape
            assert fn(ptr(src), ptr(feat), None, None, None, None, ptr(ws.v), *shape, ncls, st()) == ERR_ARG, shape
        if Cc % 16 == 0:  # msl_head_grad_pack takes no channel count
            assert L.msl_head_grad_pack(ptr(src), ptr(src), ptr(outs[0].v), N, D, H, W, rows, 0, ncls, st()) == ERR_ARG, shape
            I1 = ctypes.c_int * 1
            arrs = [(ctypes.c_void_p * 1)(ptr(outs[0].v)), I1(D), I1(H), I1(W), I1(0)]
            assert L.msl_head_grad_pack_batch(ptr(src), ptr(src), *[ctypes.addressof(a) for a in arrs], 1, N, rows, ncls, st()) == ERR_ARG, shape
        if ncls >= 1 and not (N > 0 and D > 0 and H > 0 and W > 0 and Cc % 16 == 0):
            assert L.msl_head_conv_bwd_weight_nslabs(*shape, ncls) == ERR_ARG, shape
    # the bf16 forward has one output tile and 32-channel k-steps
    assert L.msl_head_conv_fwd_bf16(ptr(srcb), ptr(w), ptr(src), ptr(src), ptr(outs[0].v), ptr(outs[1].v), 1, 32, 2, 2, 2, rows, 0, 3,
                                    st()) == ERR_UNSUPPORTED
    assert L.msl_head_conv_fwd_bf16(ptr(srcb), ptr(w), ptr(src), ptr(src), ptr(outs[0].v), ptr(outs[1].v), 1, 48, 2, 2, 2, rows, 0, 2,
                                    st()) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    for b in outs + [outb, ws]:
        b.untouched("a refused head call")
