"""The reference of the IoU-family localisation losses (tests/iouloss_ref.py) and what tests/iouloss_cases.py promises, on the
CPU: gradients against central differences, kind 1 against the oracle's own IoU of the decoded boxes, the ranges of the three
losses, the confidence side against tests/multibox_ref.py, and the distance of every comparison from its switch point.  Also
the Python surface that needs no device: ``set_loc_loss`` on MultiBoxLoss / LSSD3D and ``--loc_loss`` of train.py."""
import pytest
import torch

from oracle import boxes as OB
from tests import iouloss_cases as IC
from tests import iouloss_ref as IR
from tests import multibox_ref as R

GRAD_CASES = [n for n in IC.ALL_NAMES if n not in (IC.NO_POSITIVE, IC.IDENTICAL)]


def test_every_comparison_of_every_gradient_case_keeps_its_margin():
    for name in GRAD_CASES:
        c = IC.case(name)
        g, t, p = IC.positive_rows(c)
        assert g.shape[0] > 0, name
        m = IR.margins(g, t, p)
        assert m.dtype == torch.float64
        assert float(m.min()) >= IC.MARGIN, f"{name}: a comparison is {float(m.min()):.3e} from its switch point"


def test_planted_positives_are_what_their_names_say():
    seen = set()
    for name in GRAD_CASES:
        c = IC.case(name)
        if c["P"] < 255:
            assert not c["planted"]
            continue
        assert set(c["planted"]) == set(IC.PLANTED)
        pri = c["priors"].double()
        for k, i in c["planted"].items():
            assert int(c["true_classes"][0, i]) > 0
            g, t = c["locs"][0, i][None].double(), c["true_locs"][0, i][None].double()
            _, s, lo, hi = IR.decode(g, pri[i][None], True)
            _, ts, tlo, thi = IR.decode(t, pri[i][None], False)
            w = (torch.minimum(hi, thi) - torch.maximum(lo, tlo))[0]
            z = g[0, 3:] / 5
            if k.startswith("disjoint"):
                assert int((w < 0).sum()) == int(k[-1]), (name, k, w)
            elif k == "pred_inside":
                assert bool((lo > tlo).all() and (hi < thi).all())
            elif k == "target_inside":
                assert bool((lo < tlo).all() and (hi > thi).all())
            elif k == "partial":
                assert bool((w > 0).all()) and not bool(((lo > tlo) & (hi < thi)).all()) and not bool(((lo < tlo) & (hi > thi)).all())
            elif k == "clamp_high":
                assert float(c["locs"][0, i, 3]) > 20 and float(z.max()) > IR.CLAMP
                assert torch.allclose(s[0, 0], torch.exp(torch.tensor(4.0, dtype=torch.float64)) * pri[i, 3])
            elif k == "clamp_low":
                assert float(c["locs"][0, i, 4]) < -20 and float(z.min()) < -IR.CLAMP
                assert torch.allclose(s[0, 1], torch.exp(torch.tensor(-4.0, dtype=torch.float64)) * pri[i, 4])
            seen.add(k)
    assert seen == set(IC.PLANTED)


def test_cases_hold_the_promised_images():
    c = IC.case("N3_P7001_C2")
    tc = c["true_classes"]
    assert int((tc[0] > 0).sum()) > 0
    assert int((tc[1] > 0).sum()) == 0 and int((tc[1] < 0).sum()) == 0, "image 1: no positive, nothing ignored"
    assert bool((tc[2] == -1).all()), "image 2: all ignored"
    assert int((IC.case("N2_P8192_C3")["true_classes"][1] > 0).sum()) == 0
    n = IC.case(IC.NO_POSITIVE)
    assert int((n["true_classes"] > 0).sum()) == 0 and int((n["true_classes"] == 0).sum()) > 0
    s = IC.case(IC.IDENTICAL)
    assert torch.equal(s["locs"].view(torch.int32), s["true_locs"].view(torch.int32)) and int((s["true_classes"] > 0).sum()) > 0
    one = IC.case("N1_P1_C2")
    assert one["locs"].shape == (1, 1, 6) and int(one["true_classes"][0, 0]) > 0
    for name in IC.ALL_NAMES:  # priors: another size on every axis
        p = IC.case(name)["priors"]
        assert bool((p[:, 3] != p[:, 4]).all() and (p[:, 4] != p[:, 5]).all() and (p[:, 3:] > 0).all())


@pytest.mark.parametrize("kind", list(IR.KINDS))
def test_reference_gradients_against_central_differences(kind):
    """fp64 autograd of ``per_prior`` against central differences, on the planted geometries and 40 random positives."""
    c = IC.case("N1_P255_C2")
    g, t, p = (x.double() for x in IC.positive_rows(c))
    assert g.shape[0] >= len(IC.PLANTED)
    g, t, p = g[:48], t[:48], p[:48]
    x = g.clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda v: IR.per_prior(v, t, p, kind), (x,), eps=1e-6, atol=1e-6, rtol=1e-5)
    planted = [c["planted"][k] for k in ("clamp_high", "clamp_low")]
    x = c["locs"][0, planted].double().requires_grad_(True)
    IR.per_prior(x, c["true_locs"][0, planted].double(), c["priors"][planted].double(), kind).sum().backward()
    assert float(x.grad[0, 3]) == 0.0 and float(x.grad[1, 4]) == 0.0, "the clamp's derivative outside [-4, 4] is 0"
    assert float(x.grad[0, 4]) != 0.0 and float(x.grad[1, 3]) != 0.0


def test_kind_iou_is_one_minus_the_oracles_iou_of_the_decoded_boxes():
    for name in ("N1_P255_C3", "N3_P7001_C2"):
        g, t, p = (x.double() for x in IC.positive_rows(IC.case(name)))
        # the oracle decodes without a clamp: take the clamp first
        gc = torch.cat([g[:, :3], (g[:, 3:] / 5).clamp(-IR.CLAMP, IR.CLAMP) * 5], dim=1)
        a, b = OB.cxcycz_to_xyz(OB.decode(gc, p)), OB.cxcycz_to_xyz(OB.decode(t, p))
        iou = OB.iou_matrix(a, b).diagonal()
        torch.testing.assert_close(IR.per_prior(g, t, p, "iou"), 1 - iou, rtol=1e-12, atol=1e-12)
        assert float(iou.min()) == 0.0 and float(iou.max()) > 0.25


def test_identical_boxes_give_zero_and_the_ranges_hold():
    s = IC.case(IC.IDENTICAL)
    g, t, p = (x.double() for x in IC.positive_rows(s))
    for kind in IR.KINDS:
        assert float(IR.per_prior(g, t, p, kind).abs().max()) <= 1e-13  # (hi - lo is s up to a rounding)
    for name in IC.NAMES:
        g, t, p = (x.double() for x in IC.positive_rows(IC.case(name)))
        for kind in IR.KINDS:  # IoU in [0, 1] (1 for disjoint boxes), GIoU and DIoU in [0, 2)
            l = IR.per_prior(g, t, p, kind)
            assert float(l.min()) >= 0.0 and (float(l.max()) <= 1.0 if kind == "iou" else float(l.max()) < 2.0), (name, kind)
    # disjoint boxes: IoU saturates at exactly 1 (no gradient), GIoU and DIoU do not
    c = IC.case("N1_P255_C2")
    i = c["planted"]["disjoint_3"]
    a = (c["locs"][0, i][None].double(), c["true_locs"][0, i][None].double(), c["priors"][i][None].double())
    assert float(IR.per_prior(*a, "iou")) == 1.0
    assert 1.0 < float(IR.per_prior(*a, "giou")) < 2.0 and 1.0 < float(IR.per_prior(*a, "diou")) < 2.0


def test_confidence_side_is_multibox_refs():
    """Whatever the kind: conf, the mined mask and dscores are those of multibox_ref (the L1 loss) with the same flags."""
    for name in ("N1_P255_C2", "N3_P7001_C3"):
        c = IC.case(name)
        a = (c["locs"], c["scores"], c["true_classes"], c["true_locs"])
        for f in IR.valid_flags(c["ncls"]):
            want = R.losses_and_grads(*a, f, c["ratio"], *IC.UPSTREAM)
            for kind in IR.KINDS:
                got = IR.losses_and_grads(*a, c["priors"], kind, f, c["ratio"], *IC.UPSTREAM)
                assert got["n_pos"] == want["n_pos"] and torch.equal(got["conf"], want["conf"])
                assert torch.equal(got["dscores"], want["dscores"])
                assert (got["mask"] is None) == (want["mask"] is None) and (got["mask"] is None or torch.equal(got["mask"], want["mask"]))
                assert float(got["dlocs"][c["true_classes"] <= 0].abs().max()) == 0.0
    n = IC.case(IC.NO_POSITIVE)
    r = IR.losses_and_grads(n["locs"], n["scores"], n["true_classes"], n["true_locs"], n["priors"], "giou")
    assert torch.isnan(r["loc"]) and r["n_pos"] == 0 and float(r["dlocs"].abs().max()) == 0.0


def test_tolerance_follows_the_projects_rule():
    c = IC.case("N1_P255_C3")
    tol, dev32 = IR.tolerance(c["locs"], c["scores"], c["true_classes"], c["true_locs"], c["priors"], "diou", c["ncls"], c["ratio"],
                              *IC.UPSTREAM)
    assert 0.0 < dev32 and tol == min(1e-4, 8.0 * dev32)


# ---------------------------------------------------------------------------------------------------- Python surface
def test_set_loc_loss_on_the_loss_module():
    from mslesions3d_amd.ssd3d import LOC_LOSS_KINDS, MultiBoxLoss
    assert LOC_LOSS_KINDS == {"l1": 0, "iou": 1, "giou": 2, "diou": 3}
    lf = MultiBoxLoss(None, threshold=0.5)
    assert lf.loc_loss == "l1" and lf.can_pack(3)
    for kind in ("iou", "giou", "diou"):
        lf.set_loc_loss(kind)
        assert lf.loc_loss == kind and not lf.can_pack(3)
    lf.set_loc_loss("l1")
    assert lf.can_pack(3)
    for bad in ("ciou", "L1", None, 2):
        with pytest.raises(ValueError):
            lf.set_loc_loss(bad)
    assert lf.loc_loss == "l1"
    sm = MultiBoxLoss(None, threshold=0.5, smooth_l1=True, hard_negative_mining=True)
    sm.set_loc_loss("l1")
    with pytest.raises(ValueError, match="smooth_l1"):
        sm.set_loc_loss("giou")
    assert sm.loc_loss == "l1"
    MultiBoxLoss(None, threshold=0.5, hard_negative_mining=True, focal=True).set_loc_loss("diou")


def test_set_loc_loss_on_the_model_and_its_checkpoint(tmp_path):
    from mslesions3d_amd.ssd3d import LSSD3D
    kw = dict(n_classes=2, input_channels=1, input_size=(64, 64, 64), threshold=[0.1, 0.2])
    m = LSSD3D(**kw)
    keys = set(m.hparams)
    assert m.loss_fn.loc_loss == "l1" and "loc_loss" not in keys
    assert m.set_loc_loss("giou") is m
    assert m.loss_fn.loc_loss == "giou" and m.hparams["loc_loss"] == "giou" and set(m.hparams) == keys | {"loc_loss"}
    m.save_checkpoint(str(tmp_path / "giou.ckpt"))
    assert LSSD3D.read_checkpoint(str(tmp_path / "giou.ckpt"))["hyper_parameters"]["loc_loss"] == "giou"
    back = LSSD3D.load_from_checkpoint(str(tmp_path / "giou.ckpt"))
    assert back.loss_fn.loc_loss == "giou" and back.hparams["loc_loss"] == "giou"
    assert LSSD3D.load_from_checkpoint(str(tmp_path / "giou.ckpt"), loc_loss="diou").loss_fn.loc_loss == "diou"
    m.set_loc_loss("l1")
    assert set(m.hparams) == keys
    m.save_checkpoint(str(tmp_path / "l1.ckpt"))
    assert "loc_loss" not in LSSD3D.read_checkpoint(str(tmp_path / "l1.ckpt"))["hyper_parameters"]
    assert LSSD3D.load_from_checkpoint(str(tmp_path / "l1.ckpt")).loss_fn.loc_loss == "l1"
    with pytest.raises(ValueError):
        LSSD3D(smooth_l1=True, **kw).set_loc_loss("iou")


def test_train_flag(capsys):
    from mslesions3d_amd.train import build_parser, loc_loss_of, parse_args
    # not given: None (a new model trains with l1, a resumed one keeps its checkpoint's kind); given: that kind, l1 included
    assert parse_args([]).loc_loss is None and loc_loss_of(parse_args(["--smooth_l1"])) is None
    for kind in ("l1", "iou", "giou", "diou"):
        assert loc_loss_of(parse_args(["--loc_loss", kind, "--focal_loss"])) == kind
    assert parse_args(["--loc_loss", "l1", "--smooth_l1"]).smooth_l1
    for bad in (["--loc_loss", "ciou"], ["--loc_loss", "giou", "--smooth_l1"], ["--smooth_l1", "--loc_loss", "iou"]):
        with pytest.raises(SystemExit) as e:
            parse_args(bad)
        assert e.value.code == 2
    assert "--smooth_l1" in capsys.readouterr().err
    # a caller that parses with build_parser() alone is refused by example() before the first GPU call
    with pytest.raises(ValueError, match="smooth_l1"):
        loc_loss_of(build_parser().parse_args(["--loc_loss", "diou", "--smooth_l1"]))
