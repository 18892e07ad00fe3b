"""Mint ``step_programs.json``: the launch program one ``FusedTrainer`` step records per input shape, storage type and
engine options, and the one a bare eval-mode forward pass records (``EVAL``).  The first twelve step cases were taken at the
commit BEFORE the backward passes read their kernel routes from ``Plan.routes``; the cases with fold options and the eval
cases at the commit BEFORE the forward passes read their BatchNorm folds from ``Plan.folds``; the one-stream, ``-unbatched``,
``-tailpw`` and 136 x 128 x 128 cases at the commit BEFORE the passes issued their launches through the emitters of
``Engine`` (so the file pins which entry point the inline code of the four passes chose, on which stream, in which order
and with which arguments):

    python -m tests.golden.make_step_programs            # writes the file (needs the GPU)
    python -m tests.golden.make_step_programs --dump     # prints every normalised program instead (to diff two commits)

Per case, the first step of a fresh trainer is recorded and taken through ``_lib._fuse_stop_events`` (what the native replay
compiles).  Every entry becomes ``[role, entry point, tag, arguments]``: ``role`` is the stream it is issued on (chain /
heads / wgrad / other), an integer argument below 2^31 in magnitude and a float are kept by value, ``None`` stays ``None``
and every larger integer - device pointers, host-array addresses, event and stream handles - is replaced by ``"#k"``, k the
ordinal of its first appearance in the program.  A Python hook becomes ``["hook", tag]``.  The file keeps, per case, the
``[role, entry point, tag]`` list and a SHA-256 over the fully normalised entries.
``tests/test_gpu_model.py::test_step_program_is_the_recorded_one`` and ``test_eval_program_is_the_recorded_one`` rebuild
the same cases and compare.

When minting, every backward route the engine can take must show among the cases of each storage type that has it
(``ROUTES``), and so must both forms of every forward launch that can fold a BatchNorm (fp32: the folding form and the one
that reads the vectors of an ``msl_bn_finalize`` on the chain).  Two fp32 routes, ``msl_pwconv_bwd_fused`` and
``msl_dwconv_s2_bwd_data_bnreduce_bww``, need a block i >= 2 whose input has more than 65536 positions per channel over the
batch; at 128^3 x 2 block 2's input has exactly 65536, so one fp32-only case (``F32_ONLY``) has one axis of 136: 69632.

The cases with ``multi_stream=False`` pin the one-stream branches of the four passes and, as the trainer's one-launch loss
needs the side streams, the per-scale ``msl_head_grad_pack``.  The ``-unbatched`` ones set ``batch_tail_pw`` and
``batch_head_gpack`` off: that is the default program (the tail is unbatched by default, and on three streams the loss
kernel writes the head-gradient images itself, so no pack runs either way), pinned under its own name so that a change of
either default shows.  The fp32 ``-tailpw`` case pins the other side, the tail's pointwise weight gradients in one launch.
"""
import argparse
import hashlib
import json
import os

from tests.golden import detinit

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "step_programs.json")
TINY = 16  # edge of the tiny cube (see tiny_cube)
FUSE, NOFUSE = {"fuse_stem": True}, {"fuse_stem": False}
# name -> (batch, input size, input channels, options: Engine attributes set before the first step); each with fp32 and bf16
# storage, 2 classes
SHAPES = {"64x2": (2, (64, 64, 64), 1, FUSE),
          "48x64x64x2-2ch": (2, (48, 64, 64), 2, FUSE),  # smallest shape of the suite on the big-producer paths
          "64x2-nofuse": (2, (64, 64, 64), 1, NOFUSE),
          # block 1 itself takes a channel link, which leaves the stem its BatchNorm backward done (fp32; the fused stem pass
          # goes first wherever it is enabled, so this route only exists with Engine.fuse_stem off)
          "tiny-nofuse": (2, (TINY,) * 3, 1, NOFUSE),
          "128x2": (2, (128, 128, 128), 1, FUSE),          # bf16: a stride-2 patch pass feeding block 1's BatchNorm backward
          "128x2-nofuse": (2, (128, 128, 128), 1, NOFUSE),  # fp32: msl_dwconv_bwd_data_bnreduce, the stem's bn-apply weight gradient
          # the forward pass away from the default fold options: fp32 folds no BatchNorm, bf16 falls to its floor of 64 partials
          "64x2-nofold": (2, (64, 64, 64), 1, dict(FUSE, fold_np_max=0)),
          "64x2-foldall": (2, (64, 64, 64), 1, dict(FUSE, fold_bn=True)),  # fp32 folds every BatchNorm, bf16 does not consult it
          # fold_np_max does not reach the BatchNorm of a depthwise output (FOLD_NP_MAX_PW = 64 partials, never more at batch
          # 2): 33 tiny volumes leave block 1's with 66, so its pointwise layer reads the vectors of a finalize on the chain
          "tiny-x33": (33, (TINY,) * 3, 1, FUSE),
          "64x2-1stream": (2, (64, 64, 64), 1, dict(FUSE, multi_stream=False)),
          "64x2-unbatched": (2, (64, 64, 64), 1, dict(FUSE, batch_tail_pw=False, batch_head_gpack=False))}
# the same for fp32 storage only
F32_ONLY = {"136x128x128x2": (2, (136, 128, 128), 1, FUSE),  # block 2: msl_pwconv_bwd_fused, msl_dwconv_s2_bwd_data_bnreduce_bww
            "64x2-tailpw": (2, (64, 64, 64), 1, dict(FUSE, batch_tail_pw=True))}  # (the bf16 pass does not consult it)
# a bare eval-mode forward pass (record_eval): name -> (batch, input size, input channels, options, storage type)
EVAL = {"eval-64x2-f32": (2, (64, 64, 64), 1, {}, "f32"),
        "eval-64x2-bf16": (2, (64, 64, 64), 1, {"bf16_heads": "f32"}, "bf16"),
        "eval-64x2-bf16-bf16heads": (2, (64, 64, 64), 1, {"bf16_heads": "bf16"}, "bf16"),
        # msl_stem_dw_fwd_eval_supported says yes at 64^3 and at 128^3 alike; this shape is one it refuses
        "eval-32x32x96x2-f32": (2, (32, 32, 96), 1, {}, "f32")}


def _entry(name):
    return lambda p, sfx: any(e == name for e, _ in p)


def _link(with_dw_bww):
    return lambda p, sfx: any((f"msl_block_bwd_channel_link{sfx}", f"link{i}") in p
                              and any(t == f"dw_bww{i}" for _, t in p) == with_dw_bww for i in range(1, 16))


# route -> (storage types in which some case must take it, predicate over the program's (entry point, tag) pairs and the
# entry points' storage suffix)
ROUTES = {
    "link": (("f32", "bf16"), _link(True)),
    "link without a following dw_bww": (("f32", "bf16"), _link(False)),
    "msl_dwconv_bwd_data_bnreduce": (("f32",), _entry("msl_dwconv_bwd_data_bnreduce")),
    "s2_patch": (("bf16",), _entry("msl_dwconv_bwd_data_s2_patch_bf16")),
    "dw_bwd1 fused": (("f32", "bf16"), lambda p, sfx: (f"msl_dwconv_s2_bwd_bnreduce_bww{sfx}", "dw_bwd1") in p),
    "plain": (("f32", "bf16"), lambda p, sfx: any(e == f"msl_dwconv_bwd_data{sfx}" for e, _ in p)),
    "pw_bwd_fused": (("f32",), _entry("msl_pwconv_bwd_fused")),
    "msl_dwconv_s2_bwd_data_bnreduce_bww": (("f32",), _entry("msl_dwconv_s2_bwd_data_bnreduce_bww")),
    "pw_bww_tail": (("f32",), _entry("msl_pwconv_bwd_weight_slabs_batch")),
    "msl_head_grad_pack": (("f32", "bf16"), _entry("msl_head_grad_pack")),
}
# the forward pass: a BatchNorm folded into its consumer from the partials, or finalized on the chain and read as vectors
ROUTES.update({name: (("f32",), _entry(name)) for name in (
    "msl_dwconv_fwd", "msl_dwconv_fwd_fold", "msl_pwconv_fwd", "msl_pwconv_fwd_fold", "msl_bn_relu_materialize",
    "msl_bn_relu_materialize_fold", "msl_bn_finalize")})


def cases():
    """name -> (batch, input size, input channels, options, dtype)."""
    both = {f"{tag}-{dtype}": shape + (dtype,) for tag, shape in SHAPES.items() for dtype in ("f32", "bf16")}
    return dict(both, **{f"{tag}-f32": shape + ("f32",) for tag, shape in F32_ONLY.items()})


def eval_cases():
    return dict(EVAL)


def tiny_cube(batch=2):
    """Edge of the smallest cube (a multiple of 8) at which block 1 itself can take a channel link: the link serves its
    producer, the stem activation.  A host query; TINY must be its answer."""
    from mslesions3d_amd import _lib
    for edge in range(8, 129, 8):
        half = (edge - 1) // 2 + 1
        if _lib.load().msl_block_bwd_channel_link_supported(batch, half, half, half, 2) > 0:
            return edge
    return None


def _model(case, device):
    """A fresh model for ``case`` with its options set, and the case's input batch."""
    from mslesions3d_amd.ssd3d import LSSD3D
    n, size, cin, options, dtype = case
    m = LSSD3D(n_classes=2, input_channels=cin, input_size=size, threshold=[0.1, 0.2], lr=1e-3, batch_size=n)
    m.load_state_dict(detinit.fill_state_dict(m.state_dict(), 1234))
    m = m.to(device)
    m.compute_dtype = dtype
    for name, value in options.items():
        assert hasattr(m._engine, name), name
        setattr(m._engine, name, value)
    return m, detinit.make_volume_batch(5, n, cin, size).to(device)


def record(case, device="cuda"):
    """One step of a fresh trainer on ``case`` -> (normalised program, the step's plan)."""
    from mslesions3d_amd.trainer import FusedTrainer
    m, x = _model(case, device)
    n, size = case[:2]
    tr = FusedTrainer(m.train())
    boxes, labels = detinit.make_gt(8, n, size)
    tr.step(x, [b.to(device) for b in boxes], [t.to(device) for t in labels])
    entry = list(tr._programs.values())[-1]
    return _normalise(entry["prog"], m._engine, tr._stream.cuda_stream, x.device), entry["plan"]


def record_eval(case, device="cuda"):
    """A bare eval-mode forward pass of a fresh model on ``case`` -> (normalised program, the pass's plan)."""
    import torch
    from mslesions3d_amd import _lib
    m, x = _model(case, device)
    eng = m.eval()._engine
    _lib.start_recording()
    try:
        eng.forward(x, training=False, need_grad=False)
    finally:
        prog = _lib.stop_recording()
    return _normalise(prog, eng, torch.cuda.current_stream().cuda_stream, x.device), eng.plan_for(x, False)


def _normalise(recorded, engine, chain, device):
    from mslesions3d_amd import _lib
    heads, wgrad = (s.cuda_stream for s in engine.side_streams(device))
    roles = {chain: "chain", heads: "heads", wgrad: "wgrad"}
    seen = {}

    def norm(a):
        if a is None or isinstance(a, float):
            return a
        a = int(a)
        return a if abs(a) < (1 << 31) else "#%d" % seen.setdefault(a, len(seen))
    prog = []
    for fn, args, tag, stream in _lib._fuse_stop_events(recorded, ()):
        if fn is None:
            prog.append(["hook", tag])
        else:
            prog.append([roles.get(stream, "other"), fn.__name__, tag, [norm(a) for a in args]])
    return prog


def summary(prog):
    """What the file keeps of a normalised program."""
    return {"sha256": hashlib.sha256(json.dumps(prog).encode()).hexdigest(), "entries": [e[:3] for e in prog]}


def write(progs, out):
    with open(out, "w") as f:  # one entry per line
        body = []
        for name, prog in progs.items():
            s = summary(prog)
            body.append(f' "{name}": {{"sha256": "{s["sha256"]}", "entries": [\n  '
                        + ",\n  ".join(json.dumps(e) for e in s["entries"]) + "]}")
        f.write("{\n" + ",\n".join(body) + "\n}\n")
    print(f"{out}: {len(progs)} cases, {sum(len(p) for p in progs.values())} entries")


def check_routes(progs):
    """Every route of ROUTES shows in a case of each storage type listed for it."""
    pairs = {name: {(e[1], e[2]) for e in prog if e[0] != "hook"} for name, prog in progs.items()}
    for route, (dtypes, found) in ROUTES.items():
        for dtype in dtypes:
            hit = [name for name, p in pairs.items() if name.endswith("-" + dtype) and found(p, "_bf16" if dtype == "bf16" else "")]
            print(f"route {route!r} ({dtype}): {hit}")
            assert hit, f"no {dtype} case takes the route {route!r}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--dump", action="store_true", help="print the full normalised programs instead of writing the file")
    args = ap.parse_args()
    assert tiny_cube() == TINY, f"the tiny case must be the {tiny_cube()}^3 cube"
    steps = {name: record(c, args.device)[0] for name, c in cases().items()}
    progs = dict(steps, **{name: record_eval(c, args.device)[0] for name, c in eval_cases().items()})
    if args.dump:
        for name, prog in progs.items():
            print(f"== {name}")
            for k, e in enumerate(prog):
                print(f"{k:4d} " + " ".join(json.dumps(v) for v in e))
        return
    write(progs, args.out)
    check_routes(steps)


if __name__ == "__main__":
    main()
