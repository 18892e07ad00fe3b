"""The cases of tests/test_gpu_optim.py, as plain CPU data: tests/test_optim_ref_cpu.py walks the same list to prove that every
bound of tests/optim_ref.py accepts a plain fp32 evaluation of the case and rejects a perturbed one.  Nothing here imports the
package; the dispatch of msl_grad_reduce_table_set (few-slab / many-slab form, workgroups per entry) is restated from its
documentation so that the GPU suite can assert which form an entry took.

A fold table is ``dict(buffers=[flat CPU tensors], rows=[row, ...])``; a row is a dict of
    kind, buf (index into buffers), off (elements from the start of the buffer to the entry's source), ns, count, stride,
    p = (p0, p1, p2), dst_off = elements by which each destination is shifted off a 16-byte boundary, npos (kind 4), what.
Source columns that no entry owns (stride > count, the shift in front of an unaligned source, and a stretch behind the last slab
or partial of every buffer) hold NaN: a read of them poisons the sum.  (The head workspace keeps the engine's layout - slabs, then
the row sums - so only the row sums are followed by NaN.)"""
import functools

import numpy as np
import torch

from tests import optim_ref as R

NAN = float("nan")
GR_FEW = 16
ADAM_PASS = 2048 * 256   # elements of one grid pass of adam_kernel
NAN_PASS = 1024 * 256    # of nan_flag_kernel / nan_flag2_kernel


def cdiv(a, b):
    return (a + b - 1) // b


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------- Adam
ADAM_SIZES = (1, 255, 256, 257, 10007, ADAM_PASS, ADAM_PASS + 1, 2 * ADAM_PASS + 77)
MASKS = ("zeros", "ones", "every7")
SCALES = (1.0, 0.25, 1.0 / 3.0)
DECAYS = (0.0, 5e-4)
BETAS = ((0.9, 0.999), (0.5, 0.9))


def _adam_cases():
    """Every (mask, scale, decay, betas) at n = 10007; every size twice, the options rotating so that each value of each
    option meets a size above one grid pass."""
    cases = [(10007, mk, gs, wd, bt) for mk in MASKS for gs in SCALES for wd in DECAYS for bt in BETAS]
    for i, n in enumerate(ADAM_SIZES):
        for j in (0, 1):
            k = 2 * i + j
            c = (n, MASKS[k % 3], SCALES[(k + j) % 3], DECAYS[(i + j) % 2], BETAS[j])
            if c not in cases:
                cases.append(c)
    return cases


ADAM_CASES = _adam_cases()


def adam_id(c):
    n, mk, gs, wd, bt = c
    return f"n{n}-{mk}-gs{gs:.3g}-wd{wd:g}-b{bt[0]:g}"


def adam_mask(n, kind):
    m = torch.zeros(n, dtype=torch.uint8)
    if kind == "ones":
        m[:] = 1
    elif kind == "every7":
        m[::7] = 1
    return m


def zero_block(n):
    """The elements whose p = g = m = v = 0 (in the middle: the tail stays live)."""
    return slice(n // 2, n // 2 + min(40, n // 4))


def _magnitudes(n, g):
    """|x| in [1e-12, 1e3]: every third element log-uniform over the whole range, the rest |normal| (no fp32 denormals)."""
    wide = 10.0 ** (torch.rand(n, generator=g, dtype=torch.float64) * 15.0 - 12.0)
    norm = torch.randn(n, generator=g, dtype=torch.float64).abs().clamp(1e-12, 1e3)
    return torch.where(torch.arange(n) % 3 == 0, wide, norm).float().clamp(1e-12, 1e3)


def adam_inputs(n, seed=0):
    """-> dict of fp32 p, g, m (signed), v (>= 0) with the zero block."""
    g = gen(7919 * seed + n)
    out = {}
    for k in ("p", "g", "m", "v"):
        x = _magnitudes(n, g)
        if k != "v":
            x = x * (torch.randint(0, 2, (n,), generator=g) * 2 - 1).float()
        x[zero_block(n)] = 0.0
        out[k] = x
    return out


def adam_hp(gs, wd, betas, step=3):
    return R.make_hp(1e-3, betas, 1e-8, wd, step, gs)


# ------------------------------------------------------------------------------------------------- fold tables
def few_form(kind, ns, count, stride, src_aligned=True, dst_aligned=True):
    """msl_grad_reduce_table_set: the 4-outputs-per-thread form, else 32 outputs per workgroup."""
    few = kind not in (1, 4) and ns <= GR_FEW and count % 4 == 0 and stride % 4 == 0
    return few and src_aligned and (kind != 0 or dst_aligned)


def blocks(kind, ns, count, stride, src_aligned=True, dst_aligned=True):
    if kind == 4:
        return 1
    return cdiv(count, 1024) if few_form(kind, ns, count, stride, src_aligned, dst_aligned) else cdiv(count, 32)


OVER = 8  # slabs of NaN behind the last one: a loop that runs past nslabs reads them (and stays inside the allocation)


def _slab_buffer(g, ns, count, stride, off=0):
    buf = torch.full((off + (ns - 1) * stride + count + OVER * max(stride, count),), NAN)
    torch.as_strided(buf, (ns, count), (stride, 1), off).copy_(torch.randn((ns, count), generator=g))
    return buf


def _row(kind, buf, ns, count, stride, p=(0, 0, 0), off=0, dst_off=(0, 0), npos=None, what=""):
    return dict(kind=kind, buf=buf, off=off, ns=ns, count=count, stride=stride, p=p, dst_off=dst_off, npos=npos, what=what)


def _add_slab(tab, g, ns, count, stride, off=0, dst_off=0, what=""):
    tab["buffers"].append(_slab_buffer(g, ns, count, stride, off))
    tab["rows"].append(_row(0, len(tab["buffers"]) - 1, ns, count, stride, off=off, dst_off=(dst_off, 0),
                            what=what or f"kind0 ns{ns} count{count} stride{stride}"))


def _add_stem(tab, g, ns, cin, off=0, dst_off=0):
    K, NT = 27 * cin, cdiv(27 * cin, 32)
    tab["buffers"].append(_slab_buffer(g, ns, 1024 * NT, 1024 * NT, off))
    tab["rows"].append(_row(2, len(tab["buffers"]) - 1, ns, 1024 * NT, 1024 * NT, (K, NT, 0), off, (dst_off, 0),
                            what=f"kind2 ns{ns} cin{cin}"))


def head_shape(C, ncls):
    mt = (12 + 2 * ncls + 15) // 16
    return mt, (C // 16) * 27 * mt * 256


def _add_head(tab, g, ns, C, ncls, off=0, dst_off=(0, 0), bias_rows=False):
    """One scale of Engine._grad_reduce: the head workspace [ns][slab] followed by [ns][16 mt] row sums; kind 3 over the
    slabs and, with ``bias_rows``, the two kind-0 rows over ``bias`` and ``bias[12:]``."""
    mt, slab = head_shape(C, ncls)
    ws = torch.cat([torch.full((off,), NAN), torch.randn(ns * slab + ns * 16 * mt, generator=g), torch.full((OVER * 16 * mt,), NAN)])
    tab["buffers"].append(ws)
    b = len(tab["buffers"]) - 1
    tab["rows"].append(_row(3, b, ns, slab, slab, (C, mt, 12 + 2 * ncls), off, dst_off, what=f"kind3 ns{ns} C{C} ncls{ncls}"))
    if bias_rows:
        bias = off + ns * slab
        tab["rows"].append(_row(0, b, ns, 12, 16 * mt, off=bias, dst_off=(dst_off[0], 0), what=f"loc bias ns{ns} C{C} ncls{ncls}"))
        tab["rows"].append(_row(0, b, ns, 2 * ncls, 16 * mt, off=bias + 12, dst_off=(dst_off[1], 0),
                                what=f"cls bias ns{ns} C{C} ncls{ncls}"))


def _add_elem(tab, g, NP, count):
    tab["buffers"].append(torch.cat([torch.randn(count * NP, generator=g, dtype=torch.float64),
                                     torch.full((OVER * 32,), NAN, dtype=torch.float64)]))
    tab["rows"].append(_row(1, len(tab["buffers"]) - 1, NP, count, 0, what=f"kind1 NP{NP} count{count}"))


def _add_loss(tab, g, ns, npos):
    """Non-negative partial sums like the loss kernel's, over six decades."""
    x = torch.rand(2 * ns, generator=g, dtype=torch.float64) * 10.0 ** torch.randint(-3, 3, (2 * ns,), generator=g).double()
    tab["buffers"].append(torch.cat([x, torch.full((2 * 64,), NAN, dtype=torch.float64)]))
    tab["rows"].append(_row(4, len(tab["buffers"]) - 1, ns, 1, 0, npos=npos, what=f"kind4 ns{ns} npos{npos}"))


SLAB_COUNTS = (1, 3, 4, 5, 15, 16, 17, 40, 56, 57, 63, 64, 65, 121, 130)  # 40: the many-slab form the issue asks of kind 2
COUNTS = (3, 4, 33, 64, 1028, 1029, 1056, 2050, 2052)


def strides_of(count):
    """stride == count; the next larger multiple of 4; a larger one that is no multiple of 4."""
    up4 = (count // 4 + 1) * 4
    return (count, up4, up4 + 3)


@functools.lru_cache(maxsize=None)
def slab_table(ns):
    tab, g = dict(buffers=[], rows=[]), gen(100 + ns)
    for count in COUNTS:
        for stride in strides_of(count):
            _add_slab(tab, g, ns, count, stride)
    for cin in (1, 2, 4):
        _add_stem(tab, g, ns, cin)
    return tab


@functools.lru_cache(maxsize=None)
def unaligned_table():
    """Few-slab cases but for a pointer 1 to 3 floats off a 16-byte boundary.  The last row's destination is unaligned under a
    kind that stores float by float: it keeps the few-slab form."""
    tab, g = dict(buffers=[], rows=[]), gen(200)
    _add_slab(tab, g, 5, 1028, 1032, off=1, what="kind0 src+1")
    _add_slab(tab, g, 5, 1028, 1032, dst_off=2, what="kind0 dst+2")
    _add_slab(tab, g, 16, 1028, 1028, off=3, dst_off=1, what="kind0 src+3 dst+1")
    _add_stem(tab, g, 9, 2, off=1)
    _add_head(tab, g, 5, 16, 2, off=2)
    _add_stem(tab, g, 9, 2, dst_off=1)
    return tab


HEAD_NCLS = (1, 2, 3, 10)
HEAD_NS = (5, 16, 17, 40)


@functools.lru_cache(maxsize=None)
def head_table(ncls, ns):
    """Two scales (C = 16, 48) as Engine._grad_reduce lays them out: kind 3, then ``bias`` and ``bias[12:]``.  The second
    scale's destinations sit where a packed arena puts them behind 2 ncls class biases: off a 16-byte boundary for odd ncls."""
    tab, g = dict(buffers=[], rows=[]), gen(300 + 50 * ncls + ns)
    for s, C in enumerate((16, 48)):
        o = (s * 2 * ncls) % 4
        _add_head(tab, g, ns, C, ncls, dst_off=(o, o), bias_rows=True)
    return tab


ELEM_NP = (1, 31, 32, 33, 224, 225, 256, 257, 600)
ELEM_COUNTS = (1, 7, 8, 9, 27, 32, 33, 864)


@functools.lru_cache(maxsize=None)
def elem_table(NP):
    tab, g = dict(buffers=[], rows=[]), gen(400 + NP)
    for count in ELEM_COUNTS:
        _add_elem(tab, g, NP, count)
    return tab


LOSS_CASES = [(ns, npos) for ns in (1, 63, 64, 65, 1000) for npos in (1, 37)] + [(64, 0)]


@functools.lru_cache(maxsize=None)
def loss_table(ns, npos):
    tab = dict(buffers=[], rows=[])
    _add_loss(tab, gen(500 + 40 * ns + npos), ns, npos)
    return tab


@functools.lru_cache(maxsize=None)
def mixed_table(n=64):
    """``n`` entries of every kind in turn (both forms, ragged sizes), a kind-4 entry in the middle."""
    tab, g = dict(buffers=[], rows=[]), gen(600)
    for i in range(n):
        if i == n // 2 - 1:
            _add_loss(tab, g, 65, 37)
        elif i % 4 == 0:
            count = 30 + 5 * i
            _add_slab(tab, g, i % 20 + 1, count, count + i % 3)
        elif i % 4 == 1:
            _add_elem(tab, g, 10 + 7 * i, i + 1)
        elif i % 4 == 2:
            _add_stem(tab, g, i % 18 + 1, (1, 2, 4)[i % 3])
        else:
            _add_head(tab, g, i % 19 + 1, 16, (1, 2, 3)[i % 3])
    assert len(tab["rows"]) == n
    return tab


def all_tables():
    """(id, table) of every fold table of the GPU suite."""
    out = [(f"slabs-ns{ns}", slab_table(ns)) for ns in SLAB_COUNTS]
    out.append(("unaligned", unaligned_table()))
    out += [(f"head-ncls{c}-ns{ns}", head_table(c, ns)) for c in HEAD_NCLS for ns in HEAD_NS]
    out += [(f"elem-NP{NP}", elem_table(NP)) for NP in ELEM_NP]
    out += [(f"loss-ns{ns}-npos{p}", loss_table(ns, p)) for ns, p in LOSS_CASES]
    out.append(("mixed", mixed_table()))
    return out


# ------------------------------------------------------------------------------------------------- rows -> reference
def src_matrix(tab, row):
    """The entry's source as the reference functions take it: [ns][count] slabs, [count][NP] partials or [ns][2] loss sums."""
    buf = tab["buffers"][row["buf"]]
    if row["kind"] == 1:
        return buf[row["off"]:row["off"] + row["count"] * row["ns"]].view(row["count"], row["ns"])
    if row["kind"] == 4:
        return buf[row["off"]:row["off"] + 2 * row["ns"]].view(row["ns"], 2)
    return torch.as_strided(buf, (row["ns"], row["count"]), (row["stride"], 1), row["off"])


def dst_sizes(row):
    kind, (p0, p1, p2) = row["kind"], row["p"]
    if kind == 2:
        return (32 * p0,)
    if kind == 3:
        return (12 * p0 * 27, (p2 - 12) * p0 * 27)
    if kind == 4:
        return (3,)
    return (row["count"],)


def fold_kwargs(row):
    kind, (p0, p1, p2) = row["kind"], row["p"]
    return {2: dict(K=p0, NT=p1), 3: dict(C=p0, MT=p1, ncls=(p2 - 12) // 2)}.get(kind, {})


def reference(tab, row):
    """kinds 0-3 -> (exact sums per destination, bounds per destination); kind 4 -> ((lo,), (hi,)) float32 value ranges."""
    x = src_matrix(tab, row)
    if row["kind"] == 1:
        r, b = R.fold_partials_f64(x)
        return [r], [b]
    if row["kind"] == 4:
        lo, hi = R.loss_fold_range(x.numpy(), row["npos"])
        return [lo], [hi]
    return R.fold_slabs(x, row["kind"], **fold_kwargs(row))


def in_loss_range(got, lo, hi):
    """``got`` (float32 [3]) is a value the kernel may produce: the one bit pattern where lo == hi, else between them."""
    got, lo, hi = (np.asarray(a, dtype=np.float32) for a in (got, lo, hi))
    same = lo.view(np.uint32) == hi.view(np.uint32)
    with np.errstate(invalid="ignore"):
        return bool(np.all(np.where(same, got.view(np.uint32) == lo.view(np.uint32), (lo <= got) & (got <= hi))))
