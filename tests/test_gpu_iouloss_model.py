"""The IoU-family localisation losses through the model: ``set_loc_loss`` on a 64^3 network (batch 2, the synthetic case of
tests/test_gpu_model.py) against tests/iouloss_ref.py on the model's own head outputs and targets, the fused training step
against the module's autograd path, a replayed launch program against the Python-driven steps, checkpoints and train.py."""
import functools
import glob
import json

import numpy as np
import pytest
import torch

from tests import iouloss_ref as IR
from tests import multibox_ref as R
from tests.golden import detinit

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZE, N = (64, 64, 64), 2


def hip_model(kind, seed=1234, **kw):
    from mslesions3d_amd.ssd3d import LSSD3D
    m = LSSD3D(n_classes=2, input_channels=1, input_size=SIZE, threshold=[0.1, 0.2], **kw)
    m.load_state_dict(detinit.fill_state_dict(m.state_dict(), seed))
    return m.to(DEV).set_loc_loss(kind).train()


@functools.lru_cache(maxsize=None)
def batch():
    x = detinit.make_volume_batch(5, N, 1, SIZE).to(DEV)
    boxes, labels = detinit.make_gt(8, N, SIZE)
    return x, [b.to(DEV) for b in boxes], [l.to(DEV) for l in labels]


@pytest.mark.parametrize("kind", ["giou", "diou"])
def test_module_loss_and_gradients_equal_the_reference(kind):
    alpha = 0.5
    m = hip_model(kind, alpha=alpha)
    x, boxes, labels = batch()
    assert m.loss_fn.loc_loss == kind and not m.loss_fn.can_pack(3)
    with torch.no_grad():
        locs, scores = m(x)
    gl, gs = locs.detach().clone().requires_grad_(True), scores.detach().clone().requires_grad_(True)
    conf, loc = m.loss_fn(gl, gs, boxes, labels)
    (conf + m.loss_fn.alpha * loc).backward()
    tc, tl, _ = m.loss_fn.match(boxes, labels)
    a = (gl.detach().cpu(), gs.detach().cpu(), tc.cpu(), tl.cpu(), m.priors_cxcycz.cpu())
    assert int((tc > 0).sum()) > 0
    r = IR.losses_and_grads(*a, kind, 0, 3, 1.0, alpha)
    tol, dev32 = IR.tolerance(*a, kind, 2, 3, 1.0, alpha)
    for k, got in (("conf", conf), ("loc", loc), ("dlocs", gl.grad), ("dscores", gs.grad)):
        d = R.deviation(got.detach().cpu(), r[k])
        print(f"{kind} {k}: deviation {d:.3e}, allowed {tol:.3e} (8 x fp32 torch {dev32:.3e}, cap 1e-4)")
        assert d <= tol, f"{kind} {k}: deviation {d:.3e} from fp64 over {tol:.3e} (8 x fp32 torch {dev32:.3e}, cap 1e-4)"
    assert 0.0 <= loc.item() < 2.0
    with torch.no_grad():  # the forward-only call publishes the same losses
        c2, l2 = m.loss_fn(locs, scores, boxes, labels)
    assert c2.item() == conf.item() and l2.item() == loc.item()
    # with the reference's loss the same model gives another localisation loss: the switch is live
    c1, l1 = m.set_loc_loss("l1").loss_fn(locs, scores, boxes, labels)
    assert c1.item() == conf.item() and l1.item() != loc.item()


def test_fused_step_equals_the_autograd_step():
    """One FusedTrainer.step with giou against forward + loss + backward + Adam through the module: same losses (the bound of
    the loss-variant test there, 1e-6) and the same parameters after the update, bit for bit (same kernels, same gradients)."""
    from mslesions3d_amd.trainer import FusedTrainer
    x, boxes, labels = batch()
    a = hip_model("giou", lr=1e-3)
    [opt], [sch] = a.configure_optimizers()
    lo, sc = a(x)
    cf, lc = a.loss_fn(lo, sc, boxes, labels)
    (cf + a.loss_fn.alpha * lc).backward()
    sch.step()
    opt.step()
    b = hip_model("giou", lr=1e-3)
    out = FusedTrainer(b).step(x, boxes, labels)
    np.testing.assert_allclose(out["conf"], cf.item(), rtol=1e-6)
    np.testing.assert_allclose(out["loc"], lc.item(), rtol=1e-6)
    assert 0.0 <= out["loc"] < 2.0
    for (k, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(pa, pb), f"{k} differs between the autograd and the fused step"
    c = hip_model("l1", lr=1e-3)  # and the reference's loss moves the parameters elsewhere
    FusedTrainer(c).step(x, boxes, labels)
    assert any(not torch.equal(pb, pc) for pb, pc in zip(b.parameters(), c.parameters()))


def test_replayed_program_equals_python_driven_steps():
    from mslesions3d_amd.ssd3d import MultiBoxLoss
    from mslesions3d_amd.trainer import FusedTrainer
    batches = []
    for k in range(2):
        xs = detinit.make_volume_batch(50 + k, N, 1, SIZE).to(DEV)
        bs, ls = detinit.make_gt(60 + k, N, SIZE)
        batches.append((xs,) + MultiBoxLoss.pack_targets(bs, ls, torch.device(DEV)))
    results = []
    for use_programs in (True, False):
        m = hip_model("giou", lr=1e-3)
        tr = FusedTrainer(m)
        tr.use_programs = use_programs
        outs = [tr.step_packed(*batches[s % 2]) for s in range(4)]
        if use_programs:
            assert len(tr._programs) == 1, "steps 2..4 replay the program of step 1"
        results.append(([(o["conf"], o["loc"]) for o in outs], torch.cat([p.detach().reshape(-1) for p in m.parameters()]).clone()))
    assert results[0][0] == results[1][0]
    assert torch.equal(results[0][1], results[1][1])
    assert all(0.0 <= loc < 2.0 for _, loc in results[0][0])


def test_switching_the_loss_records_a_new_program():
    from mslesions3d_amd.ssd3d import MultiBoxLoss
    from mslesions3d_amd.trainer import FusedTrainer
    xs = detinit.make_volume_batch(50, N, 1, SIZE).to(DEV)
    bs, ls = detinit.make_gt(60, N, SIZE)
    packed = (xs,) + MultiBoxLoss.pack_targets(bs, ls, torch.device(DEV))
    m = hip_model("l1", lr=0.0)
    tr = FusedTrainer(m)
    l1 = [tr.step_packed(*packed)["loc"] for _ in range(2)]
    m.set_loc_loss("giou")
    giou = [tr.step_packed(*packed)["loc"] for _ in range(2)]
    assert len(tr._programs) == 2 and l1[0] != giou[0] and 0.0 <= giou[1] < 2.0


def test_checkpoint_round_trip(tmp_path):
    from mslesions3d_amd.ssd3d import LSSD3D
    from mslesions3d_amd.trainer import FusedTrainer
    x, boxes, labels = batch()
    m = hip_model("diou", lr=1e-3)
    tr = FusedTrainer(m)
    tr.step(x, boxes, labels)
    m.save_checkpoint(str(tmp_path / "diou.ckpt"), tr)
    assert LSSD3D.read_checkpoint(str(tmp_path / "diou.ckpt"))["hyper_parameters"]["loc_loss"] == "diou"
    back = LSSD3D.load_from_checkpoint(str(tmp_path / "diou.ckpt")).to(DEV).train()
    assert back.loss_fn.loc_loss == "diou" and not back.loss_fn.can_pack(3)
    with torch.no_grad():
        la, lb = m.loss_fn(*m(x), boxes, labels), back.loss_fn(*back(x), boxes, labels)
    assert la[1].item() == lb[1].item()
    plain = hip_model("l1")
    plain.save_checkpoint(str(tmp_path / "l1.ckpt"))
    assert "loc_loss" not in LSSD3D.read_checkpoint(str(tmp_path / "l1.ckpt"))["hyper_parameters"]


def test_train_entry_point_with_loc_loss(tmp_path):
    """``train --loc_loss giou``: two epochs at 64^3, a localisation loss in [0, 2) in every logged line, the kind in the
    checkpoints."""
    from mslesions3d_amd import datasets as DS
    from mslesions3d_amd import train as T
    from mslesions3d_amd.ssd3d import LSSD3D
    DS.generate_artificial_dataset(str(tmp_path / "data"), "toy64", num_images=10, image_size=SIZE)
    args = T.parse_args(["-d", str(tmp_path / "data"), "-dn", "toy64", "-b", "2", "-me", "2", "-ld",
                         str(tmp_path / "logs"), "-en", "run", "--loc_loss", "giou"])
    model = T.example(args)
    assert model.loss_fn.loc_loss == "giou" and model.global_step == 8
    lines = [json.loads(l) for l in open(tmp_path / "logs" / "run" / "metrics.jsonl")]
    seen = [v for l in lines for k, v in l.items() if k.startswith("localization_loss")]
    assert seen and all(0.0 <= v < 2.0 for v in seen), seen
    ckpts = sorted(glob.glob(str(tmp_path / "logs" / "run" / "*.ckpt")))
    assert ckpts and LSSD3D.load_from_checkpoint(ckpts[0]).loss_fn.loc_loss == "giou"
