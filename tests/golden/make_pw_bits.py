"""Mint ``pw_bits.json``: a SHA-256 of every output buffer of the pointwise-convolution entry points, fp32 (csrc/pwconv.hip,
csrc/pwfused.hip) and bf16 (csrc/bf16.hip), at every case of tests/pw_cases.py and at the GEMM, fold, bwd-data and weight-gradient
tables of tests/bf16pw_cases.py.  The file was taken at the commit BEFORE the host code of these files got its single route
(csrc/pwroute.hpp), so it pins the bits of the launches the old free functions and macro cascades made; it is never minted again
from later code:

    python -m tests.golden.make_pw_bits            # writes the file (needs the GPU)

The kernels use no atomics and add in a fixed order, so the digests are a property of the code and of gfx950.  The inputs are
each case's own seeded inputs, exactly as tests/test_gpu_pw.py and tests/test_gpu_bf16pw.py make them (their input helpers are
called here).  Every output buffer has exactly the size its count query gives and is NaN-filled before the launch.
``test_pw_bits_are_the_recorded_ones`` (tests/test_gpu_pw.py) and ``test_pw_bf16_bits_are_the_recorded_ones``
(tests/test_gpu_bf16pw.py) recompute the digests of their half and compare."""
import argparse
import ctypes
import hashlib
import json
import os

import torch

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pw_bits.json")
FOLD_NP = (7, 65)  # the serial fold (NP <= 64) and the wave tree
EPS = 1e-5
NAN = float("nan")


def sha(t):
    torch.cuda.synchronize()
    t = t.contiguous()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def _tools(device):
    from mslesions3d_amd import _lib
    st = torch.cuda.current_stream().cuda_stream
    out, keep = {}, []

    def put(entry, case, **buffers):
        for name, t in buffers.items():
            key = f"{entry} {case.replace(' ', '_')} {name}"
            assert key not in out, key
            out[key] = sha(t)
        keep.clear()  # the case's uploads: alive until its launches have been waited for

    def nan(n, dtype=torch.float32):
        return torch.full((n,), NAN, dtype=dtype, device=device)

    def up(t, dtype=None):
        keep.append((t if dtype is None else t.to(dtype)).to(device).contiguous())
        return keep[-1]

    return _lib, _lib.load(), st, out, put, nan, up


def digests_fp32(device="cuda"):
    """{"<entry point> <case> <buffer>": sha256} of every case of tests/pw_cases.py."""
    from mslesions3d_amd._lib import ptr
    from tests import pw_cases as C
    from tests import pw_ref as P
    from tests import test_gpu_pw as T
    _lib, L, st, out, put, nan, up = _tools(device)
    f64 = torch.float64

    for path, N, Cin, Cout, S, _ in C.FWD_CASES:
        d = T.fwd_inputs(N, Cin, Cout, S)
        NP = L.msl_pwconv_fwd_num_partials(N, Cin, Cout, S)
        w, sc, sh = up(d["w"]), up(d["sc"]), up(d["sh"])
        forms = dict(plain=(up(P.act32(d["z"], d["sc"], d["sh"])), None, None))
        if Cin <= 512:
            forms["affine"] = (up(d["z"]), sc, sh)
        for form, (x, a, b) in forms.items():
            y, part, y2 = nan(N * Cout * S), nan(2 * Cout * NP, f64), nan(N * Cout * S)
            _lib.call("msl_pwconv_fwd", ptr(x), ptr(a), ptr(b), ptr(w), ptr(y), ptr(part), N, Cin, Cout, S, st)
            _lib.call("msl_pwconv_fwd", ptr(x), ptr(a), ptr(b), ptr(w), ptr(y2), None, N, Cin, Cout, S, st)
            put("msl_pwconv_fwd", f"{path}:{form}", y=y, partials=part, y_nostats=y2)
    for path, N, Cin, Cout, S in C.FOLD_CASES:
        NP = L.msl_pwconv_fwd_num_partials(N, Cin, Cout, S)
        for in_np in FOLD_NP:
            z, w, gamma, beta, parts = T.fold_inputs(N, Cin, Cout, S, in_np, float(N * S))
            y, part = nan(N * Cout * S), nan(2 * Cout * NP, f64)
            _lib.call("msl_pwconv_fwd_fold", ptr(up(z)), ptr(up(parts)), in_np, float(N * S), ptr(up(gamma)), ptr(up(beta)), EPS,
                      ptr(up(w)), ptr(y), ptr(part), N, Cin, Cout, S, st)
            put("msl_pwconv_fwd_fold", f"{path}:np{in_np}", y=y, partials=part)
    for path, N, Cin, Cout, S, _ in C.BWD_DATA_CASES:
        dy, w = T.bwd_data_inputs(N, Cin, Cout, S)
        g = nan(N * Cin * S)
        _lib.call("msl_pwconv_bwd_data", ptr(up(dy)), ptr(up(w)), ptr(g), N, Cin, Cout, S, st)
        put("msl_pwconv_bwd_data", path, g_in=g)
    for path, N, Cin, Cout, S in C.BWW_CASES:
        dy, z, sc, sh = (up(t) for t in T.bww_data(N, Cin, Cout, S))
        ns = L.msl_pwconv_bwd_weight_nslabs(N, Cin, Cout, S)
        for form, (a, b) in dict(affine=(sc, sh), plain=(None, None)).items():
            slabs, dw, ws = nan(ns * Cout * Cin), nan(Cout * Cin), nan(ns * Cout * Cin)
            _lib.call("msl_pwconv_bwd_weight_slabs", ptr(dy), ptr(z), ptr(a), ptr(b), ptr(slabs), N, Cin, Cout, S, st)
            _lib.call("msl_pwconv_bwd_weight", ptr(dy), ptr(z), ptr(a), ptr(b), ptr(dw), ptr(ws), N, Cin, Cout, S, st)
            put("msl_pwconv_bwd_weight", f"{path}:{form}", slabs=slabs, dw=dw)
    for id_, shapes in (("batch1", [(32, 64, 1312)]), ("batch3-unequal-S", [(32, 64, 224), (128, 128, 96), (64, 64, 1312)])):
        N, n, rows = 3, len(shapes), []
        for q, (Cin, Cout, S) in enumerate(shapes):
            dy, z, sc, sh = (up(t) for t in T.bww_data(N, Cin, Cout, S, seed=q))
            rows.append((dy, z, sc, sh, nan(L.msl_pwconv_bwd_weight_nslabs(N, Cin, Cout, S) * Cout * Cin), Cin, Cout, S))
        Pp, I = ctypes.c_void_p * n, ctypes.c_int * n
        arrs = [Pp(*[ptr(r[c]) for r in rows]) for c in range(5)] + [I(*[r[c] for r in rows]) for c in range(5, 8)]
        _lib.call("msl_pwconv_bwd_weight_slabs_batch", *[ctypes.addressof(a) for a in arrs], n, N, st)
        put("msl_pwconv_bwd_weight_slabs_batch", id_, **{f"slabs{q}": r[4] for q, r in enumerate(rows)})
    N, Cin, Cout, S = C.FUSED_CASE
    gy, y, z, w, vy, vz, parts, ynp, count = T.fused_inputs()
    NPW = L.msl_pwconv_bwd_fused_num_partials(N, Cin, Cout, S)
    gz, zpart, slabs, dgam, dbet = nan(N * Cin * S), nan(2 * Cin * NPW, f64), nan(NPW * Cout * Cin), nan(Cout), nan(Cout)
    _lib.call("msl_pwconv_bwd_fused", ptr(up(gy)), ptr(up(y)), ptr(up(vy)), ptr(up(parts)), ynp, count, ptr(dgam), ptr(dbet),
              ptr(up(w)), ptr(up(z)), ptr(up(vz)), ptr(gz), ptr(zpart), ptr(slabs), N, Cin, Cout, S, st)
    put("msl_pwconv_bwd_fused", "fused", g_z=gz, z_partials=zpart, slabs=slabs, dgamma_y=dgam, dbeta_y=dbet)
    return out


def digests_bf16(device="cuda"):
    """{"<entry point> <case> <buffer>": sha256} of the GEMM, fold, bwd-data and weight-gradient tables of tests/bf16pw_cases.py."""
    from mslesions3d_amd._lib import ptr
    from tests import bf16pw_cases as C
    _lib, L, st, out, put, nan, up = _tools(device)
    BF, f64 = torch.bfloat16, torch.float64

    for id_, N, Cin, Cout, S, _ in C.FWD_CASES:
        d = C.gemm_data(N, Cin, Cout, S)
        NP = L.msl_pwconv_fwd_bf16_num_partials(N, S)
        z, w = up(d["z"], BF), up(d["w"])
        for form, (a, b) in dict(affine=(up(d["sc"]), up(d["sh"])), plain=(None, None)).items():
            y, part, y2 = nan(N * Cout * S, BF), nan(2 * Cout * NP, f64), nan(N * Cout * S, BF)
            _lib.call("msl_pwconv_fwd_bf16", ptr(z), ptr(a), ptr(b), ptr(w), ptr(y), ptr(part), N, Cin, Cout, S, st)
            _lib.call("msl_pwconv_fwd_bf16", ptr(z), ptr(a), ptr(b), ptr(w), ptr(y2), None, N, Cin, Cout, S, st)
            put("msl_pwconv_fwd_bf16", f"{id_}:{form}", y=y, partials=part, y_nostats=y2)
    for id_, N, Cin, Cout, S, _ in C.FOLD_CASES:
        NP = L.msl_pwconv_fwd_bf16_num_partials(N, S)
        for in_np in C.FOLD_NP:
            g = C.gen(7100 + in_np + S)
            d = C.gemm_data(N, Cin, Cout, S)
            gamma, beta = torch.randn(Cin, generator=g).abs() + 0.5, torch.randn(Cin, generator=g) * 0.3
            parts = C.fold_partials(Cin, in_np, float(N * S), g)
            y, part = nan(N * Cout * S, BF), nan(2 * Cout * NP, f64)
            _lib.call("msl_pwconv_fwd_bf16_fold", ptr(up(d["z"], BF)), ptr(up(parts)), in_np, float(N * S), ptr(up(gamma)),
                      ptr(up(beta)), EPS, ptr(up(d["w"])), ptr(y), ptr(part), N, Cin, Cout, S, st)
            put("msl_pwconv_fwd_bf16_fold", f"{id_}:np{in_np}", y=y, partials=part)
    for id_, N, Cin, Cout, S, _ in C.BWD_DATA_CASES:
        d = C.gemm_data(N, Cin, Cout, S)
        g = nan(N * Cin * S, BF)
        _lib.call("msl_pwconv_bwd_data_bf16", ptr(up(d["dy"], BF)), ptr(up(d["w"])), ptr(g), N, Cin, Cout, S, st)
        put("msl_pwconv_bwd_data_bf16", id_, g_in=g)
    for id_, N, Cin, Cout, S, _ in C.BWW_CASES:
        d = C.gemm_data(N, Cin, Cout, S)
        ns = L.msl_pwconv_bwd_weight_bf16_nslabs(N, Cin, Cout, S)
        dy, z = up(d["dy"], BF), up(d["z"], BF)
        for form, (a, b) in dict(affine=(up(d["sc"]), up(d["sh"])), plain=(None, None)).items():
            slabs = nan(ns * Cout * Cin)
            _lib.call("msl_pwconv_bwd_weight_slabs_bf16", ptr(dy), ptr(z), ptr(a), ptr(b), ptr(slabs), N, Cin, Cout, S, st)
            put("msl_pwconv_bwd_weight_slabs_bf16", f"{id_}:{form}", slabs=slabs)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    d = dict(fp32=digests_fp32(args.device), bf16=digests_bf16(args.device))
    with open(args.out, "w") as f:  # one digest per line
        f.write("{\n" + ",\n".join(
            f' {json.dumps(half)}: {{\n' + ",\n".join(f'  {json.dumps(k)}: "{v}"' for k, v in d[half].items()) + "\n }"
            for half in d) + "\n}\n")
    print(f"{args.out}: {len(d['fp32'])} fp32 and {len(d['bf16'])} bf16 digests")


if __name__ == "__main__":
    main()
