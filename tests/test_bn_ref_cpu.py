"""tests/bn_ref.py (the stage-wise float64 reference of the BatchNorm kernels) against torch's own float64
batch_norm + relu and its autograd: shows that the reference the GPU tests rely on is itself right.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

from tests import bn_ref as R

SHAPES = [(3, 8, (4, 6, 8)), (2, 4, (5, 7, 9)), (1, 1, (1, 1, 2)), (4, 2, (16, 8, 8)), (2, 5, (3, 5, 7))]
EPS, MOM = 1e-5, 0.1


def _case(N, C, dims, seed, mean=1.0, std=2.0):
    g = torch.Generator().manual_seed(seed)
    y = (torch.randn((N, C) + dims, generator=g) * std + mean).double()
    gamma = (torch.randn(C, generator=g).abs() + 0.5).double()
    beta = (torch.randn(C, generator=g) * 0.2).double()
    rm, rv = (torch.randn(C, generator=g) * 0.1).double(), (torch.randn(C, generator=g).abs() + 0.5).double()
    go = torch.randn((N, C) + dims, generator=g).double()
    return y, gamma, beta, rm, rv, go


def _sums(y):
    d = (0,) + tuple(range(2, y.dim()))
    return y.sum(d), (y * y).sum(d), y.numel() // y.shape[1]


def _close(a, b, what, tol=1e-11):
    err = float((a - b).abs().max())
    assert err <= tol * (1.0 + float(b.abs().max())), f"{what}: max abs err {err:.3e}"


@pytest.mark.parametrize("N,C,dims", SHAPES)
def test_stages_match_float64_autograd(N, C, dims):
    y, gamma, beta, rm, rv, go = _case(N, C, dims, seed=N * 100 + C)
    yt, gt, bt = y.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rm_t, rv_t = rm.clone(), rv.clone()
    a = torch.relu(F.batch_norm(yt, rm_t, rv_t, gt, bt, True, MOM, EPS))
    a.backward(go)
    s, q, n = _sums(y)
    r = R.finalize_ref(s, q, n, gamma, beta, EPS, MOM, rm, rv)
    # eps and momentum enter as the fp32 values a C float carries: 1e-5 and 0.1 differ from those by 2**-25 relative
    _close(r["running_mean"], rm_t, "running_mean", 1e-8)
    _close(r["running_var"], rv_t, "running_var", 1e-8)
    vec = torch.stack([r["scale"], r["shift"], r["mean"], r["invstd"]])  # float64 vectors: no rounding in the way
    _close(R.act_ref(y, vec[0], vec[1]), a.detach(), "act", 1e-9)
    dbeta, dgamma = R.bwd_sums_ref(go, y, vec)
    _close(dbeta, bt.grad, "dbeta", 1e-9)
    _close(dgamma, gt.grad, "dgamma", 1e-9)
    dy = R.bwd_apply_ref(go, y, vec, dbeta / n, dgamma / n)
    _close(dy, yt.grad, "dy", 1e-9)
    # the folded form of the same gradient
    cC, cE = R.coef_ref(dbeta, dgamma, n, vec)
    v = lambda t: t.view((1, -1) + (1,) * len(dims))
    gm = torch.where(a.detach() > 0, go, torch.zeros_like(go))
    _close(v(vec[0]) * gm + (v(cC) * y + v(cE)), yt.grad, "coef form", 1e-9)
    # eval form
    es, eh = R.eval_affine_ref(gamma, beta, rm_t, rv_t, EPS)
    _close(y * v(es) + v(eh), F.batch_norm(y, rm_t, rv_t, gamma, beta, False, MOM, EPS), "eval affine", 1e-9)
    # the host-made fp32 vectors are the float64 ones rounded once
    hv = R.host_vectors(y.float(), gamma.float(), beta.float(), EPS)
    assert hv.dtype == torch.float32 and hv.shape == (4, C)
    y32 = y.float().double()
    s32, q32, _ = _sums(y32)
    r32 = R.finalize_ref(s32, q32, n, gamma.float(), beta.float(), EPS, MOM)
    for k, key in enumerate(("scale", "shift", "mean", "invstd")):
        assert torch.equal(hv[k], r32[key].float()), key


def test_finalize_edges():
    one = torch.ones(2, dtype=torch.float64)
    # count == 1: the running variance takes the biased value (0 here)
    r = R.finalize_ref(torch.tensor([3.0, -2.0]), torch.tensor([9.0, 4.0]), 1, one, 0 * one, EPS, 0.5, 0 * one, one)
    assert torch.equal(r["var"], 0 * one)
    _close(r["running_var"], 0.5 * one, "running_var at count 1")
    _close(r["running_mean"], torch.tensor([1.5, -1.0]).double(), "running_mean at count 1")
    # inconsistent partials, q / count < mean**2: clamped, invstd = 1 / sqrt(eps)
    r = R.finalize_ref(torch.tensor([10.0, 10.0]), torch.tensor([1.0, 60.0]), 2, one, one, EPS, 0.1)
    assert float(r["var"][0]) == 0.0 and abs(float(r["invstd"][0]) - float(torch.tensor(EPS).float().double()) ** -0.5) < 1e-9
    assert abs(float(r["var"][1]) - 5.0) < 1e-12
    assert r["running_mean"] is None and r["running_var"] is None


def test_nan_survives_act_and_bounds_are_positive():
    y = torch.tensor([[[1.0, float("nan"), -3.0, 0.0]]])
    sc, sh = torch.tensor([2.0]), torch.tensor([0.5])
    a = R.act_ref(y, sc, sh)
    assert torch.isnan(a[0, 0, 1]) and a[0, 0, 0] == 2.5 and a[0, 0, 2] == 0.0 and a[0, 0, 3] == 0.5
    b = R.act_bound(y, sc, sh)
    assert float(b[0, 0, 0]) == 3 * R.U * 2.5 and float(b[0, 0, 2]) == 3 * R.U * 6.5


def test_separate_preactivation_leaves_no_element_near_zero():
    for (N, C, dims), (mean, std) in zip(SHAPES, [(1, 2), (300, 0.05), (1, 2), (0, 1), (300, 0.05)]):
        y, gamma, beta, *_ = _case(N, C, dims, seed=7, mean=mean, std=std)
        y2, amin = R.separate_preactivation(y.float(), gamma.float(), beta.float(), EPS, 1e-3)
        assert amin >= 1e-3
        hv = R.host_vectors(y2, gamma.float(), beta.float(), EPS).double()
        v = lambda t: t.view((1, -1) + (1,) * len(dims))
        assert float((y2.double() * v(hv[0]) + v(hv[1])).abs().min()) >= 0.9e-3


def test_worst_reports_ratio_index_and_nan_rules():
    ref = torch.tensor([1.0, 2.0, 0.0, float("nan")], dtype=torch.float64)
    bound = torch.tensor([0.1, 0.1, 0.0, 0.1], dtype=torch.float64)
    ok = torch.tensor([1.05, 2.0, 0.0, float("nan")])
    ratio, idx, bad = R.worst(ok, ref, bound)
    assert bad == 0 and idx == 0 and abs(ratio - 0.5) < 1e-6
    assert R.worst(torch.tensor([1.0, 2.3, 0.0, float("nan")]), ref, bound)[1:] == (1, 1)
    assert R.worst(torch.tensor([1.0, 2.0, 1e-30, float("nan")]), ref, bound)[0] == float("inf")   # zero bound: equality
    assert R.worst(torch.tensor([1.0, 2.0, 0.0, 0.0]), ref, bound)[0] == float("inf")              # NaN must stay NaN
    assert R.worst(torch.tensor([float("nan"), 2.0, 0.0, float("nan")]), ref, bound)[0] == float("inf")


def test_exact_sum_has_no_order():
    p = torch.tensor([[1e16, 1.0, -1e16, 1.0], [1.0, 1e16, 1.0, -1e16]], dtype=torch.float64)
    assert R.exact_sum(p).tolist() == [2.0, 2.0]
