"""tests/optim_ref.py proved on the CPU, without the library: the Adam reference against torch.optim.Adam in float64, the layout
maps of the stem image and the head slabs against an independent permute / reshape, and every bound against (a) a plain
numpy-fp32 evaluation of the same operation, which must lie inside it, and (b) a perturbed copy - scaled by 1 + 2**-18, or with
one slab dropped - which must lie outside it, at every case of tests/test_gpu_optim.py (tests/optim_cases.py)."""
import numpy as np
import pytest
import torch

from tests import optim_cases as C
from tests import optim_ref as R

OFF = 1.0 + 2.0 ** -18


def t64(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float64))


def inside(what, actual, ref, bound):
    ratio, idx, bad = R.worst(t64(actual), ref, bound)
    assert bad == 0, f"{what}: {bad} elements of a plain fp32 evaluation over their bound (worst {ratio:.3f} at {idx})"
    return ratio


def outside(what, actual, ref, bound, live):
    """More than half of the ``live`` elements (those the perturbation moves) must be over their bound."""
    a, r, b = t64(actual).reshape(-1), ref.reshape(-1), bound.reshape(-1)
    over = ((a - r).abs() > b) & live.reshape(-1)
    n = int(live.sum())
    assert n > 0 and int(over.sum()) * 2 > n, f"{what}: the bound accepts {n - int(over.sum())} of {n} perturbed elements"


# ------------------------------------------------------------------------------------------------- Adam
def adam_np32(p, g, m, v, hp, is_bias):
    """adam_kernel line by line in numpy float32 (numpy rounds every operation: no contraction)."""
    p, g, m, v = (np.asarray(x, dtype=np.float32) for x in (p, g, m, v))
    ss_b, ss_o, bc2s, b1, b2, eps, wd, gs = (np.float32(x) for x in hp)
    one = np.float32(1.0)
    gi = g * gs
    gi = gi + wd * p
    mi = m + (gi - m) * (one - b1)
    vi = v * b2 + (one - b2) * gi * gi
    denom = np.sqrt(vi) / bc2s + eps
    pn = p - np.where(np.asarray(is_bias) != 0, ss_b, ss_o) * (mi / denom)
    assert pn.dtype == mi.dtype == vi.dtype == np.float32
    return pn, mi, vi


def test_adam_ref_is_torch_adam_float64():
    """3 steps, two parameter groups (biases at 2 lr), weight_decay 5e-4: adam_step iterated == torch.optim.Adam, to 1e-12.
    The betas are the fp32 values the kernel gets (1 - beta in fp32 is then exact); everything else stays a double."""
    g = C.gen(1)
    betas = (float(np.float32(0.9)), float(np.float32(0.999)))
    lr, eps, wd = 1e-3, 1e-8, 5e-4
    w0, b0 = torch.randn(300, generator=g, dtype=torch.float64), torch.randn(45, generator=g, dtype=torch.float64)
    w, b = w0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
    opt = torch.optim.Adam([dict(params=[b], lr=2 * lr), dict(params=[w])], lr=lr, betas=betas, eps=eps, weight_decay=wd,
                           foreach=False)
    p = torch.cat([w0, b0])
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    mask = torch.cat([torch.zeros(300), torch.ones(45)]).to(torch.uint8)
    for step in (1, 2, 3):
        grad = torch.randn(345, generator=g, dtype=torch.float64) * 0.3
        w.grad, b.grad = grad[:300].clone(), grad[300:].clone()
        opt.step()
        hp = R.make_hp(lr, betas, eps, wd, step, dtype=np.float64)
        p, m, v = R.adam_step(p, grad, m, v, hp, mask)[:3]
        want = torch.cat([w.detach(), b.detach()])
        assert float((p - want).abs().max()) <= 1e-12, f"step {step}: {float((p - want).abs().max()):.3e}"
    st_w, st_b = opt.state[w], opt.state[b]
    assert float((m - torch.cat([st_w["exp_avg"], st_b["exp_avg"]])).abs().max()) <= 1e-12
    assert float((v - torch.cat([st_w["exp_avg_sq"], st_b["exp_avg_sq"]])).abs().max()) <= 1e-12


def test_adam_hp_follows_the_optimizer():
    hp = R.make_hp(1e-3, (0.9, 0.999), 1e-8, 5e-4, 3, 0.25)
    assert hp.dtype == np.float32 and hp[0] == np.float32(2e-3 / (1 - 0.9 ** 3)) and hp[1] == np.float32(1e-3 / (1 - 0.9 ** 3))
    assert hp[2] == np.float32((1 - 0.999 ** 3) ** 0.5) and list(hp[3:]) == [np.float32(x) for x in (0.9, 0.999, 1e-8, 5e-4, 0.25)]


@pytest.mark.parametrize("case", C.ADAM_CASES, ids=[C.adam_id(c) for c in C.ADAM_CASES])
def test_adam_bound_accepts_fp32_rejects_perturbed(case):
    n, mk, gs, wd, bt = case
    x, mask, hp = C.adam_inputs(n), C.adam_mask(n, mk), C.adam_hp(gs, wd, bt)
    for k in ("p", "g", "m"):
        a = x[k].abs()
        assert bool(((a == 0) | ((a >= 1e-12) & (a <= 1e3))).all())
    assert bool((x["v"] >= 0).all()) and float(x["v"].max()) <= 1e3
    ref = R.adam_step(x["p"], x["g"], x["m"], x["v"], hp, mask)
    got = adam_np32(x["p"].numpy(), x["g"].numpy(), x["m"].numpy(), x["v"].numpy(), hp, mask.numpy())
    zb = C.zero_block(n)
    for i, name in enumerate("pmv"):
        r, b = ref[i], ref[3 + i]
        assert bool(torch.isfinite(r).all()) and bool(torch.isfinite(b).all())
        assert bool((b[zb] == 0).all()) and bool((r[zb] == 0).all()), "the zero block must demand exact zeros"
        assert bool((got[i][zb] == 0).all())
        inside(f"adam {name}", got[i], r, b)
        outside(f"adam {name} * (1 + 2^-18)", got[i].astype(np.float64) * OFF, r, b, r != 0)
    # the tail check of the GPU suite (sizes above one grid pass) is sound: exp_avg and exp_avg_sq move at each of the last 300
    for name, new in (("m", got[1]), ("v", got[2])) if n > C.ADAM_PASS else ():
        assert bool((new[-300:] != x[name].numpy()[-300:]).all()), f"{name}: an element of the tail does not move"


def test_adam_v_stored_before_the_decay_is_rejected():
    """A kernel that stores ``v`` before the multiply by beta2 (v + (1 - b2) g g) is outside the bound of exp_avg_sq."""
    n = 10007
    x, mask, hp = C.adam_inputs(n), C.adam_mask(n, "every7"), C.adam_hp(1.0, 5e-4, (0.9, 0.999))
    ref = R.adam_step(x["p"], x["g"], x["m"], x["v"], hp, mask)
    gi = x["g"].double() + float(hp[6]) * x["p"].double()
    wrong = x["v"].double() + (1.0 - float(hp[4])) * gi * gi
    outside("v without the decay", wrong.float().numpy(), ref[2], ref[5], x["v"] != 0)


def test_adam_three_steps_accumulated_bound():
    """3 steps in fp32 stay inside the bounds the reference accumulates (each step's input bounds are the last step's)."""
    n = 10007
    x, mask = C.adam_inputs(n), C.adam_mask(n, "every7")
    p, m, v = (x[k].numpy() for k in "pmv")
    rp, rm, rv, bp, bm, bv = x["p"].double(), x["m"].double(), x["v"].double(), None, None, None
    for step in (1, 2, 3):
        g = C.adam_inputs(n, seed=step)["g"]
        hp = C.adam_hp(1.0 / 3.0, 5e-4, (0.9, 0.999), step)
        rp, rm, rv, bp, bm, bv = R.adam_step(rp, g, rm, rv, hp, mask, bp, bm, bv)
        p, m, v = adam_np32(p, g.numpy(), m, v, hp, mask.numpy())
        for name, a, r, b in (("p", p, rp, bp), ("m", m, rm, bm), ("v", v, rv, bv)):
            inside(f"step {step} {name}", a, r, b)
    for name, a, r, b in (("p", p, rp, bp), ("m", m, rm, bm), ("v", v, rv, bv)):  # and still reject a copy off by 2^-18
        outside(f"3 steps {name} * (1 + 2^-18)", a.astype(np.float64) * OFF, r, b, r != 0)


# ------------------------------------------------------------------------------------------------- layout maps
@pytest.mark.parametrize("cin", (1, 2, 4))
def test_stem_map_is_the_cropped_image(cin):
    K, NT = 27 * cin, C.cdiv(27 * cin, 32)
    assert NT == cin
    img = torch.arange(1024 * NT)
    idx = R.stem_map(K, NT)
    assert torch.equal(img[idx], img.view(32, 32 * NT)[:, :K].reshape(-1))
    assert idx.unique().numel() == 32 * K


@pytest.mark.parametrize("ncls", (1, 2, 3, 10))
@pytest.mark.parametrize("C_", (16, 48))
def test_head_map_is_the_permuted_slab(C_, ncls):
    mt, slab = C.head_shape(C_, ncls)
    assert mt == (1 if ncls <= 2 else 2)
    s = torch.arange(slab)
    loc, cl = R.head_map(C_, mt, ncls)
    w = s.view(C_ // 16, 27, mt, 16, 16).permute(2, 3, 0, 4, 1).reshape(16 * mt, C_, 27)  # [co][ci][tap]
    assert torch.equal(s[loc], w[:12].reshape(-1)) and torch.equal(s[cl], w[12:12 + 2 * ncls].reshape(-1))
    both = torch.cat([loc, cl])
    assert int(both.min()) >= 0 and both.unique().numel() == both.numel() == (12 + 2 * ncls) * C_ * 27


# ------------------------------------------------------------------------------------------------- folds
def serial32(x):
    """Slab 0 + slab 1 + ... in fp32."""
    s = x[0].copy()
    for k in range(1, x.shape[0]):
        s = s + x[k]
    return s


def grouped32(x):
    """Every 8th slab added serially, then the 8 group sums added serially, in fp32 (the many-slab order)."""
    groups = [serial32(x[j::8]) if j < x.shape[0] else np.zeros_like(x[0]) for j in range(8)]
    return serial32(np.stack(groups))


def place(row, flat):
    """A folded slab [count] -> its destinations, by the reference's own maps."""
    kw = C.fold_kwargs(row)
    if row["kind"] == 2:
        return [flat[R.stem_map(kw["K"], kw["NT"]).numpy()]]
    if row["kind"] == 3:
        return [flat[i.numpy()] for i in R.head_map(kw["C"], kw["MT"], kw["ncls"])]
    return [flat]


TABLES = C.all_tables()


@pytest.mark.parametrize("tab", [t for _, t in TABLES], ids=[i for i, _ in TABLES])
def test_fold_bounds_accept_fp32_reject_perturbed(tab):
    for row in tab["rows"]:
        x = C.src_matrix(tab, row)
        assert bool(torch.isfinite(x).all()), "an entry owns a NaN column"
        refs, bounds = C.reference(tab, row)
        assert [len(r) for r in refs] == list(C.dst_sizes(row))
        what = row["what"]
        if row["kind"] == 4:
            xs = x.numpy()
            ce, l1 = 0.0, 0.0
            for k in range(row["ns"]):  # a plain serial double sum
                ce, l1 = ce + xs[k, 0], l1 + xs[k, 1]
            got = R._loss_values(ce, l1, row["npos"])
            assert C.in_loss_range(got, refs[0], bounds[0]), what
            assert C.in_loss_range(R.loss_fold(xs, row["npos"]), refs[0], bounds[0]), what
            assert got[2] == row["npos"]
            if row["npos"] > 0:
                assert not C.in_loss_range(got * np.float32(OFF), refs[0], bounds[0]), f"{what}: accepts a scaled copy"
                assert not C.in_loss_range(R._loss_values(ce - xs[-1, 0], l1 - xs[-1, 1], row["npos"]), refs[0], bounds[0]), what
            else:
                assert np.isinf(got[0]) and np.isinf(got[1]) and got[2] == 0
            continue
        if row["kind"] == 1:
            got = x.numpy().sum(axis=1).astype(np.float32)
            inside(what, got, refs[0], bounds[0])
            outside(f"{what} * (1 + 2^-18)", got.astype(np.float64) * OFF, refs[0], bounds[0], refs[0] != 0)
            dropped = (x.numpy().sum(axis=1) - x.numpy()[:, -1]).astype(np.float32)
            outside(f"{what} without a partial", dropped, refs[0], bounds[0], x[:, -1] != 0)
            continue
        xs = x.numpy()
        for order in (serial32, grouped32):
            for got, r, b in zip(place(row, order(xs)), refs, bounds):
                inside(f"{what} {order.__name__}", got, r, b)
        last = torch.as_tensor(xs[-1]) != 0
        lives = place(row, last.numpy())
        for got, r, b, live in zip(place(row, serial32(xs[:-1]) if row["ns"] > 1 else np.zeros_like(xs[0])), refs, bounds, lives):
            outside(f"{what} without a slab", got, r, b, torch.as_tensor(live))
        if row["ns"] == 1:
            assert all(bool((b == 0).all()) for b in bounds), "one slab is a copy: the bound must demand equality"


def test_dispatch_restated():
    """few_form / blocks: the few-slab form needs <= 16 slabs, count and stride multiples of 4 and aligned pointers."""
    assert C.blocks(0, 16, 1028, 1028) == 2 and C.blocks(0, 17, 1028, 1028) == 33
    assert C.blocks(0, 5, 1028, 1031) == 33 and C.blocks(0, 5, 1029, 1032) == 33
    assert C.blocks(0, 5, 1028, 1028, src_aligned=False) == 33 and C.blocks(0, 5, 1028, 1028, dst_aligned=False) == 33
    assert C.blocks(2, 9, 2048, 2048, dst_aligned=False) == 2 and C.blocks(3, 5, 6912, 6912, src_aligned=False) == 216
    assert C.blocks(1, 3, 864, 0) == 27 and C.blocks(4, 1000, 1, 0) == 1
    tabs = dict(TABLES)
    assert len(tabs["mixed"]["rows"]) == 64 and tabs["mixed"]["rows"][31]["kind"] == 4
    assert {r["kind"] for r in tabs["mixed"]["rows"]} == {0, 1, 2, 3, 4}
