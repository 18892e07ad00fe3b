"""Mint ``plan_inventory.json``: what ``Engine.plan_for`` lays out per input shape, storage type and mode, taken at the
commit BEFORE the fp32 and bf16 plan builders became one class (so the file pins what the two builders allocated):

    python -m tests.golden.make_plan_inventory [--device cuda]

Per case, every attribute of the fresh plan that holds tensors or integers: a tensor as {"dtype", "shape"}, an int / bool
by value, ``None`` as null, lists / tuples / dicts walked.  Attributes without a tensor or an integer in them (empty
containers, ``None``, events) are left out.  ``tests/test_gpu_model.py::test_plan_buffer_inventory`` builds the same
cases and compares.
"""
import argparse
import json
import os

import torch

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "plan_inventory.json")
SHAPES = {"64x2": (2, (64, 64, 64)), "48x64x64x1": (1, (48, 64, 64))}  # name -> (batch, input size); 1 channel


def cases():
    """name -> (batch, input size, dtype, need_grad, Engine.bf16_heads)."""
    out = {}
    for tag, (n, size) in SHAPES.items():
        for dtype in ("f32", "bf16"):
            for need_grad in (False, True):
                out[f"{tag}-{dtype}-{'train' if need_grad else 'infer'}"] = (n, size, dtype, need_grad, "f32")
        out[f"{tag}-bf16-infer-bf16heads"] = (n, size, "bf16", False, "bf16")
    return out


def build_plan(case, device):
    """A fresh model and the plan of ``case`` (nothing has run on it) -> (engine, plan)."""
    from mslesions3d_amd.ssd3d import LSSD3D
    n, size, dtype, need_grad, heads = case
    m = LSSD3D(n_classes=2, input_channels=1, input_size=size, threshold=[0.1, 0.2]).to(device)
    m.compute_dtype = dtype
    m._engine.bf16_heads = heads
    x = torch.zeros((n, 1) + tuple(size), dtype=torch.float32, device=device)
    return m._engine, m._engine.plan_for(x, need_grad)


class _Skip(Exception):
    pass


def _enc(v, leaves):
    if torch.is_tensor(v):
        leaves.append(v)
        return {"dtype": str(v.dtype).replace("torch.", ""), "shape": list(v.shape)}
    if isinstance(v, (bool, int)):
        leaves.append(v)
        return v
    if v is None:
        return None
    if isinstance(v, (list, tuple)):
        return [_enc(e, leaves) for e in v]
    if isinstance(v, (set, frozenset)):
        return [_enc(e, leaves) for e in sorted(v)]
    if isinstance(v, dict):
        return {str(k): _enc(e, leaves) for k, e in v.items()}
    raise _Skip


def inventory(plan):
    """attribute name -> JSON-able description (see the module docstring)."""
    out = {}
    for name, v in sorted(vars(plan).items()):
        leaves = []
        try:
            enc = _enc(v, leaves)
        except _Skip:
            continue
        if leaves:
            out[name] = enc
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    inv = {name: inventory(build_plan(c, args.device)[1]) for name, c in cases().items()}
    with open(args.out, "w") as f:  # one attribute per line
        body = [f' "{name}": {{\n' + ",\n".join(f'  "{k}": {json.dumps(v)}' for k, v in attrs.items()) + "\n }"
                for name, attrs in inv.items()]
        f.write("{\n" + ",\n".join(body) + "\n}\n")
    print(f"{args.out}: {len(inv)} cases, {sum(len(v) for v in inv.values())} attributes")


if __name__ == "__main__":
    main()
