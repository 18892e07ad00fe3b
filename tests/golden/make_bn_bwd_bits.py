"""Mint ``bn_bwd_bits.json``: a SHA-256 of every output buffer of the eight BatchNorm+ReLU-backward entry points
(``msl_bn_relu_bwd_reduce``, ``_apply``, ``_fused``, ``_finalize_apply``, ``msl_bn_relu_bwd_reduce_bf16``, ``_apply_bf16``,
``_fused_bf16`` and ``msl_bn_bwd_finalize`` fed from the reduce partials) at the shapes at which the tests pin their paths.  The
file was taken at the commit BEFORE the fp32 and the bf16 kernels became one family templated on the storage type, so it pins
the bits of the two separate families; it is never minted again from later code:

    python -m tests.golden.make_bn_bwd_bits            # writes the file (needs the GPU)

The kernels use no atomics and add in a fixed order, so the digests are a property of the code and of gfx950.  Inputs are
made on the host from ``numpy.random.RandomState.random_sample`` (integers of the Mersenne twister scaled by a power of two)
and elementwise IEEE arithmetic only - no library function whose last bit could differ from one host to the next: y and g
uniform in [-4, 4), scale > 0 and shift = 4/3 scale, so a third of the pre-activations fma(y, scale, shift) is negative.
The bf16 cases round y and g to bf16 (nearest even) before the upload.  C is 1 and 5.
``tests/test_gpu_bn.py::test_bn_relu_bwd_bits_are_the_recorded_ones`` recomputes every digest and compares.

Shapes: fp32 fused - ``FUSED_CASES`` of tests/test_gpu_bn.py; fp32 reduce / finalize / apply / finalize_apply - its ``BWD_S``
with N in {1, 4}; bf16 - the reduce, apply and fused tables of tests/bf16pw_cases.py."""
import argparse
import hashlib
import json
import os

import numpy as np
import torch

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bn_bwd_bits.json")
CHANNELS = (1, 5)


def sha(t):
    torch.cuda.synchronize()
    t = t.contiguous()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def inputs(seed, N, C, S, bf16, device):
    """-> g, y (N, C, S) in the storage type, vec (8, C) fp32 rows [scale, shift, mean, invstd, 0, 0, 0, 0]."""
    rs = np.random.RandomState(seed)
    y = torch.from_numpy((rs.random_sample((N, C, S)) * 8.0 - 4.0).astype(np.float32))
    g = torch.from_numpy((rs.random_sample((N, C, S)) * 8.0 - 4.0).astype(np.float32))
    scale = (rs.random_sample(C) + 0.5).astype(np.float32)
    shift = scale * np.float32(4.0 / 3.0)
    mean = (rs.random_sample(C) - 0.5).astype(np.float32)
    invstd = (rs.random_sample(C) * 0.5 + 0.25).astype(np.float32)
    vec = torch.zeros((8, C))
    vec[:4] = torch.from_numpy(np.stack([scale, shift, mean, invstd]))
    if bf16:
        g, y = g.to(torch.bfloat16), y.to(torch.bfloat16)
    return g.to(device), y.to(device), vec.to(device)


def digests(device="cuda"):
    """{"<entry point> <case> <buffer>": sha256} of every case."""
    from mslesions3d_amd import _lib
    from mslesions3d_amd._lib import ptr
    from tests import bf16pw_cases as B
    from tests.test_gpu_bn import BWD_S, FUSED_CASES
    L = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    f32 = lambda *shape: torch.full(shape, float("nan"), device=device)
    out = {}

    def put(entry, case, **buffers):
        for name, t in buffers.items():
            out[f"{entry} {case} {name}"] = sha(t)

    def finalize(case, part, NP, count, C):
        dgamma, dbeta, c1, c2 = f32(C), f32(C), f32(C), f32(C)
        _lib.call("msl_bn_bwd_finalize", ptr(part), NP, count, ptr(dgamma), ptr(dbeta), ptr(c1), ptr(c2), C, st)
        put("msl_bn_bwd_finalize", case, dgamma=dgamma, dbeta=dbeta, c1=c1, c2=c2)
        return c1, c2

    for C in CHANNELS:
        for N, S in FUSED_CASES:
            case = f"N{N}-C{C}-S{S}"
            g, y, vec = inputs(100 + N * 7 + S + C, N, C, S, False, device)
            dgamma, dbeta, dy = f32(C), f32(C), f32(N, C, S)
            _lib.call("msl_bn_relu_bwd_fused", ptr(g), ptr(y), ptr(vec[0]), ptr(vec[1]), ptr(vec[2]), ptr(vec[3]), ptr(dgamma),
                      ptr(dbeta), ptr(dy), N, C, S, st)
            put("msl_bn_relu_bwd_fused", case, dgamma=dgamma, dbeta=dbeta, dy=dy)
        for N in (1, 4):
            for S in BWD_S:
                case = f"N{N}-C{C}-S{S}"
                g, y, vec = inputs(200 + N * 3 + S + C, N, C, S, False, device)
                NP, count = L.msl_bn_relu_bwd_num_partials(N, S), float(N * S)
                part = torch.full((2, C, NP), float("nan"), dtype=torch.float64, device=device)
                _lib.call("msl_bn_relu_bwd_reduce", ptr(g), ptr(y), ptr(vec[0]), ptr(vec[1]), ptr(vec[2]), ptr(vec[3]), ptr(part),
                          N, C, S, st)
                put("msl_bn_relu_bwd_reduce", case, partials=part)
                c1, c2 = finalize(case, part, NP, count, C)
                dy = f32(N, C, S)
                _lib.call("msl_bn_relu_bwd_apply", ptr(g), ptr(y), ptr(vec[0]), ptr(vec[1]), ptr(vec[2]), ptr(vec[3]), ptr(c1),
                          ptr(c2), ptr(dy), N, C, S, st)
                put("msl_bn_relu_bwd_apply", case, dy=dy)
                assert NP <= 256
                dgamma, dbeta, dy = f32(C), f32(C), f32(N, C, S)
                _lib.call("msl_bn_relu_bwd_finalize_apply", ptr(part), NP, count, ptr(g), ptr(y), ptr(vec), ptr(dgamma), ptr(dbeta),
                          ptr(dy), N, C, S, st)
                put("msl_bn_relu_bwd_finalize_apply", case, dgamma=dgamma, dbeta=dbeta, c1=vec[4], c2=vec[5], dy=dy)
        for id_, N, S in B.REDUCE_CASES:
            case = f"{id_}-C{C}"
            g, y, vec = inputs(300 + N * 3 + S + C, N, C, S, True, device)
            NP = L.msl_bn_relu_bwd_bf16_num_partials(N, S)
            part = torch.full((2, C, NP), float("nan"), dtype=torch.float64, device=device)
            _lib.call("msl_bn_relu_bwd_reduce_bf16", ptr(g), ptr(y), ptr(vec[0]), ptr(vec[1]), ptr(vec[2]), ptr(vec[3]), ptr(part),
                      N, C, S, st)
            put("msl_bn_relu_bwd_reduce_bf16", case, partials=part)
            finalize(case, part, NP, float(N * S), C)
        for id_, N, S, _ in B.APPLY_CASES:
            g, y, vec = inputs(400 + N * 3 + S + C, N, C, S, True, device)
            rs = np.random.RandomState(450 + S + C)  # c1, c2: any fp32 values
            vec[4:6] = torch.from_numpy((rs.random_sample((2, C)) - 0.5).astype(np.float32)).to(device)
            dy = torch.full((N, C, S), float("nan"), dtype=torch.bfloat16, device=device)
            _lib.call("msl_bn_relu_bwd_apply_bf16", ptr(g), ptr(y), ptr(vec), ptr(dy), N, C, S, st)
            put("msl_bn_relu_bwd_apply_bf16", f"{id_}-C{C}", dy=dy)
        for id_, N, S, _ in B.FUSED_CASES:
            g, y, vec = inputs(500 + N * 3 + S + C, N, C, S, True, device)
            dgamma, dbeta = f32(C), f32(C)
            dy = torch.full((N, C, S), float("nan"), dtype=torch.bfloat16, device=device)
            _lib.call("msl_bn_relu_bwd_fused_bf16", ptr(g), ptr(y), ptr(vec), ptr(dgamma), ptr(dbeta), ptr(dy), N, C, S, st)
            put("msl_bn_relu_bwd_fused_bf16", f"{id_}-C{C}", dgamma=dgamma, dbeta=dbeta, dy=dy)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    d = digests(args.device)
    with open(args.out, "w") as f:  # one digest per line
        f.write("{\n" + ",\n".join(f' {json.dumps(k)}: "{v}"' for k, v in d.items()) + "\n}\n")
    entries = sorted({k.split()[0] for k in d})
    print(f"{args.out}: {len(d)} digests of {len(entries)} entry points: {', '.join(entries)}")


if __name__ == "__main__":
    main()
