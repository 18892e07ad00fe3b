"""Static executor for the 3D-SSD network on one MI355X.

The network of ``lesions3d/ssd3d.py:248-263`` (MobileNet-3D backbone ``ssd3d.py:47-100`` /
``mobilenet.py:26-49`` + prediction heads ``ssd3d.py:113-169``) is a fixed chain, so instead of a tracing
compiler the executor lays the whole step out once per input shape ("plan"): every activation, gradient,
BatchNorm vector and workspace is a resident HBM buffer (the 128^3 x 4 plan is ~0.8 GB of 288 GB), and
forward / backward are fixed sequences of C-ABI kernel launches on the current HIP stream (capturable into a
HIP graph: no host synchronisation, no allocation inside).

Data convention: conv kernels write RAW outputs + fp64 statistic partials; ``msl_bn_finalize`` turns them into
a per-channel (scale, shift); the next kernel applies relu(x*scale+shift) while loading.  Only the three
feature maps the heads read are materialised (in a zero-haloed layout).
"""
import ctypes
import os
import typing

import torch

from . import _lib
from ._lib import ptr

BN_ROWS = 8  # scale, shift, mean, invstd, c1, c2, cC, cE (the last two: msl_bn_bwd_finalize_coef)
# a depthwise output's only consumer is the pointwise GEMM of its block (one fold per wave, 32-64 channels wide): the
# BatchNorm of a depthwise output is folded into it up to this many partials per channel (block 1's depthwise emits 64)
FOLD_NP_MAX_PW = 64
# the bf16 step (plan_folds): the floor of its threshold for y, and what its pointwise GEMM folds (partials, input channels)
BF16_FOLD_NP_FLOOR, BF16_FOLD_NP_MAX_PW, BF16_FOLD_CIN_MAX_PW = 64, 64, 1024
# a channel link (csrc/chanlink.hip) also produces the depthwise weight gradient while it has at most this many waves per
# channel (with more it is bound by instruction issue; the stride-2 forms above 4 waves also spill)
LINK_BWW_MAX_WAVES = 4


def conv_out(d, s):
    return (d - 1) // s + 1


def bn_bwd_one_launch(bf16, N, S):
    """Is the BatchNorm backward of N x S values per channel one launch (reduce + finalize + apply; bf16: the channel's data
    held in registers)?  If not, a stride-2 depthwise backward emits the reduce sums of such a producer along the way."""
    return ((N * S <= 32768 and S % 8 == 0) or N * S <= 4096) if bf16 else N * S <= 65536


class Route(typing.NamedTuple):
    """How the backward pass runs block i >= 1: ``Plan.routes[i]``, chosen by ``plan_routes``."""
    bn2: str         # who turns g_y[i] into dL/dy_i: "link" (block i+1's channel link), "pw_fused" (msl_pwconv_bwd_fused) or "bn"
    y_np: object     # "pw_fused" / "bn" (_bn_bwd): reduce sums per channel that block i+1's depthwise form left in pl.partials
    dw: str          # depthwise backward: "link" | "link_bww" (writes dW too) | "fused_stem" | "s2_bww" | "bnreduce" | "s2_patch" | "plain"
    pw_part: object  # (slabs, count) Engine._grad_reduce folds into the pointwise dW; None: the kernel wrote the arena itself
    dw_part: object  # (fp64 partials, count) it folds into the depthwise dW; None: the channel link wrote the arena


class StemRoute(typing.NamedTuple):
    """The same for the stem: ``Plan.routes[0]``."""
    bn: str       # "link": block 1's channel link left dL/dy_0 (tiny inputs); "bn": the stem does its own BatchNorm backward
    y_np: object  # "bn": reduce sums per channel that block 1's depthwise form left in pl.partials (None: none)
    wgrad: str    # weight gradient from dL/dy_0 ("plain"), with the BatchNorm backward applied on load ("bnapply"), or rebuilt
    #               from dL/dz_1 ("fused": after the fused stem pass, on the coefficients of msl_bn_bwd_finalize_coef)


DW_BWW = ("link", "bnreduce", "s2_patch", "plain")  # Route.dw forms that leave the depthwise weight gradient to its own launch


def plan_routes(pl, engine):
    """-> ``Plan.routes`` of a training plan: which kernel form carries each piece of the backward pass, from the tail (a
    block's depthwise form decides what is left to do for its producer).  All of it follows from the plan's shapes, its
    scratch size and ``Engine.fuse_stem``; both backward passes and ``Engine._grad_reduce`` read the result, so they cannot
    disagree about where a gradient was summed."""
    L = _lib.load()
    specs, N, bf16 = engine.layer_specs, pl.N, pl.bf16
    fuse_stem = engine.fuse_stem and pl.fused_stem_np > 0
    routes = [None] * len(specs)
    y_np, linked = None, False  # what the depthwise form of block i+1 did for y_i
    for i in range(len(specs) - 1, 0, -1):
        cin, cout, s = specs[i]["cin"], specs[i]["cout"], specs[i]["stride"][0]
        pd, ph, pw = pl.dims[i - 1]
        # big early block whose producer left the BatchNorm2-backward sums: one pass (csrc/pwfused.hip; fp32 plans only)
        pw_fused = not linked and y_np is not None and i in pl.pw_fused and 2 * cout * y_np <= pl.partials.numel()
        # big stride-2 producer layer: emit the BatchNorm-backward sums of y_{i-1} while its gradient is in registers
        big = s == 2 and not bn_bwd_one_launch(bf16, N, pd * ph * pw) and (not bf16 or pw % 4 == 0)
        np_red = L.msl_dwconv_bwd_data_bnreduce_num_partials(N, cin, pd, ph, pw) if big else -1
        fused_stem = i == 1 and fuse_stem
        # tail of the network: BatchNorm1 backward of z_i, depthwise bwd-data (+ the heads' share) and BatchNorm2 backward of
        # y_{i-1} are all per channel and a channel's population fits one workgroup: ONE launch (csrc/chanlink.hip)
        link_nw = L.msl_block_bwd_channel_link_supported(N, pd, ph, pw, s)
        link = link_nw > 0 and not fused_stem and not pw_fused and (i >= 2 and not big if bf16 else np_red <= 0)
        left, dw_part = None, (pl.dw_part[i], pl.dw_np[i])
        if link and link_nw <= LINK_BWW_MAX_WAVES:  # (with few waves per channel the link takes the weight gradient along)
            dw, dw_part = "link_bww", None
        elif link:
            dw = "link"
        elif fused_stem:
            dw, left, dw_part = "fused_stem", pl.fused_stem_np, (pl.partials_wf, pl.fused_stem_np)
        elif bf16 and big:
            dw, left = "s2_patch", np_red
        elif np_red > 0 and i in pl.dw_fused_part:
            dw, left, dw_part = "s2_bww", pl.dw_fused_part[i][1], pl.dw_fused_part[i]
        elif np_red > 0 and 2 * cin * np_red <= pl.partials.numel():
            dw, left = "bnreduce", np_red
        else:
            dw = "plain"
        pw_part = (pl.pw_slabs[i], pl.pw_nslabs[i]) if pl.pw_nslabs[i] > 1 else None
        if pw_fused:
            pw_part = (pl.pw_fused[i][0], pl.pw_fused[i][2])
        routes[i] = Route("link" if linked else "pw_fused" if pw_fused else "bn", y_np, dw, pw_part, dw_part)
        y_np, linked = left, link
    # (fp32: the apply-on-load kernel is built for the 32-channel stem and needs the sums of block 1's depthwise form)
    bnapply = bf16 or (y_np is not None and specs[0]["cout"] == 32)
    routes[0] = StemRoute("link" if linked else "bn", y_np, "fused" if fuse_stem else "bnapply" if bnapply else "plain")
    return routes


class Fold(typing.NamedTuple):
    """What a train-mode forward pass does with the BatchNorms of feature index i: ``Plan.folds.at[i]``."""
    dw: bool       # block i+1's depthwise layer rebuilds (scale, shift) of y[i] from the statistics partials
    copy: bool     # y[i] is a feature map and the copy its head reads does the same
    chain: object  # msl_bn_finalize of y[i] on the chain: "producer" (right behind the launch that wrote y[i]) or "consumer"
    #                (right in front of block i+1's depthwise layer); None: in the batched finalize
    pw: bool       # block i's pointwise layer folds the BatchNorm of z[i]; else it is finalized on the chain in front of it


class Folds(typing.NamedTuple):
    at: list     # Fold per feature index
    batch: list  # ("y" | "z", i) of the BatchNorms left to the one msl_bn_finalize_batch, in the order of its table


NO_FOLD = Fold(False, False, None, False)  # every layer of an eval-mode pass: nothing folds, nothing is finalized

# Every layer kernel the passes launch: logical op -> (fp32 entry point, bf16 entry point).  A plan takes its column when it
# is built (``Plan.ops``), a form its storage type lacks (None) is not in it, and the emitters of ``Engine`` (one per layer
# launch, for both storage types) look the name up there.
OPS = {
    "stem_fwd": ("msl_stem_conv_fwd", "msl_stem_conv_fwd_bf16"),
    "stem_dw_eval": ("msl_stem_dw_fwd_eval", "msl_stem_dw_fwd_eval_bf16"),
    "dw_fwd": ("msl_dwconv_fwd", "msl_dwconv_fwd_bf16"),
    "dw_fwd_fold": ("msl_dwconv_fwd_fold", "msl_dwconv_fwd_wave_bf16_fold"),
    "pw_fwd": ("msl_pwconv_fwd", "msl_pwconv_fwd_bf16"),
    "pw_fwd_fold": ("msl_pwconv_fwd_fold", "msl_pwconv_fwd_bf16_fold"),
    "copy": ("msl_bn_relu_materialize", "msl_bn_relu_materialize_bf16_pad32"),
    "copy_fold": ("msl_bn_relu_materialize_fold", "msl_bn_relu_materialize_bf16_pad32_fold"),
    "pw_bwd": ("msl_pwconv_bwd_data", "msl_pwconv_bwd_data_bf16"),
    "pw_bwd_fused": ("msl_pwconv_bwd_fused", None),
    "link": ("msl_block_bwd_channel_link", "msl_block_bwd_channel_link_bf16"),
    # "dw_bwd:" + Route.dw (the two link forms are "link" above)
    "dw_bwd:fused_stem": ("msl_dwconv_s2_bwd_bnreduce_bww", "msl_dwconv_s2_bwd_bnreduce_bww_bf16"),
    "dw_bwd:s2_bww": ("msl_dwconv_s2_bwd_data_bnreduce_bww", None),
    "dw_bwd:bnreduce": ("msl_dwconv_bwd_data_bnreduce", None),
    "dw_bwd:s2_patch": (None, "msl_dwconv_bwd_data_s2_patch_bf16"),
    "dw_bwd:plain": ("msl_dwconv_bwd_data", "msl_dwconv_bwd_data_bf16"),
    "pw_bww": ("msl_pwconv_bwd_weight_slabs", "msl_pwconv_bwd_weight_slabs_bf16"),
    "dw_bww": ("msl_dwconv_bwd_weight", "msl_dwconv_bwd_weight_bf16"),
    # "stem_bww:" + StemRoute.wgrad (plan_routes never sends a bf16 plan to "plain")
    "stem_bww:plain": ("msl_stem_conv_bwd_weight", None),
    "stem_bww:bnapply": ("msl_stem_conv_bwd_weight_bnapply", "msl_stem_conv_bwd_weight_bnapply_bf16"),
    "stem_bww:fused": ("msl_stem_conv_bwd_weight_fused", "msl_stem_conv_bwd_weight_fused_bf16"),
    "head_bwd": ("msl_head_conv_bwd_data", "msl_head_conv_bwd_data_bf16"),
}
# The two columns take the same argument list, except that the fp32 entry point of these ops takes this many more: an unused
# slot (the depthwise forward's ``0``, the ``None`` of the feature copy and of the depthwise weight gradient), or the four
# BatchNorm vectors one by one where the bf16 one takes the (BN_ROWS, C) buffer.  The emitter holds that piece per type.
F32_EXTRA_ARGS = {"dw_fwd": 1, "copy": 1, "copy_fold": 1, "dw_bww": 1, "dw_bwd:fused_stem": 3}


def plan_folds(pl, engine):
    """-> ``Plan.folds``: which BatchNorms a train-mode forward pass folds into their consumers from the statistics partials
    (no launch between producer and consumer; running statistics and backward vectors come from one batched launch at the
    end) and where the others are finalized.  All of it follows from the plan's partial counts, ``Engine.fold_bn`` and
    ``Engine.fold_np_max``; both forward passes launch what it says."""
    L = _lib.load()
    specs, last = engine.layer_specs, len(engine.layer_specs) - 1
    at = []
    for i, sp in enumerate(specs):
        feat = i in pl.feat_ids
        if pl.bf16:  # (Engine.fold_bn is not consulted)
            y_max = max(BF16_FOLD_NP_FLOOR, engine.fold_np_max)
            copy = feat and pl.f32_heads and pl.np_y[i] <= y_max
            # (a feature map that is finalized for its copy has its vectors: the depthwise layer reads them)
            dw = (i < last and pl.np_y[i] <= y_max and (copy or not feat)
                  and L.msl_dwconv_wave_num_partials(pl.N, specs[i + 1]["cin"], *pl.dims[i], specs[i + 1]["stride"][0]) > 0)
            if feat:  # "consumer": the copy folded, the depthwise layer cannot
                chain = "producer" if not copy else None if dw or i == last else "consumer"
            else:
                chain = None if dw else "consumer"
            pw = i > 0 and pl.np_z[i] <= BF16_FOLD_NP_MAX_PW and sp["cin"] <= BF16_FOLD_CIN_MAX_PW
        else:
            fold = engine.fold_bn or pl.np_y[i] <= engine.fold_np_max
            dw, copy, chain = fold and i < last, fold and feat, None if fold else "producer"
            pw = i > 0 and (engine.fold_bn or pl.np_z[i] <= FOLD_NP_MAX_PW)
        at.append(Fold(dw, copy, chain, pw))
    batch = [(k, i) for i, f in enumerate(at) for k in ("z", "y") if (f.pw if k == "z" else f.chain is None)]
    return Folds(at, batch)


class ParamArena:
    """All parameters of the model in one flat fp32 HBM buffer, ordered by backward completion (heads first,
    stem last, gradient-less parameters at the end), with flat grad / Adam-moment twins.  ``nn.Parameter``s
    become views of the arena, so ``state_dict`` / ``load_state_dict`` keep working with the reference's keys."""

    def __init__(self, model, device):
        named = list(model.named_parameters())
        self.no_grad_names = {"rescale_factors"}  # unused in forward (ssd3d.py:251-254): grad stays None

        def order_key(item):
            name = item[0]
            if name in self.no_grad_names:
                return (2, 0, name)
            if name.startswith("pred_convs"):
                return (0, 0, name)
            idx = int(name.split(".")[2])  # base.features.<idx>....
            return (1, -idx, name)

        ordered = sorted(named, key=order_key)
        self.names = [n for n, _ in ordered]
        total = sum(p.numel() for _, p in ordered)
        self.n_trainable = sum(p.numel() for n, p in ordered if n not in self.no_grad_names)
        self.flat = torch.empty(total, dtype=torch.float32, device=device)
        self.grad = torch.zeros(self.n_trainable, dtype=torch.float32, device=device)
        self.is_bias = torch.zeros(self.n_trainable, dtype=torch.uint8, device=device)
        self.offsets = {}
        self.views = {}
        self.grad_views = {}
        off = 0
        with torch.no_grad():
            for name, p in ordered:
                n = p.numel()
                view = self.flat[off:off + n].view(p.shape)
                view.copy_(p.detach().to(device=device, dtype=torch.float32))
                p.data = view
                self.offsets[name] = (off, n)
                self.views[name] = view
                if name not in self.no_grad_names:
                    self.grad_views[name] = self.grad[off:off + n].view(p.shape)
                    if name.endswith(".bias"):  # ssd3d.py:709 (BN betas match the rule too)
                        self.is_bias[off:off + n] = 1
                off += n
        self.params = {name: p for name, p in ordered}
        # ownership fingerprint (see owns): every parameter slot and every sub-module slot of the model at build time
        self._model = model
        self._slots = []
        for prefix, mod in model.named_modules():
            for key, q in mod._parameters.items():
                if q is not None:
                    name = f"{prefix}.{key}" if prefix else key
                    self._slots.append((mod._parameters, key, q, self.views[name].data_ptr()))
        self._mods = [(parent._modules, name, child) for parent in model.modules()
                      for name, child in parent._modules.items() if child is not None]

    def owns(self, model):
        """Are the model's parameters still the views of this arena?  Called on every step / batch, so it must not walk
        ``named_parameters()`` (~100 us of Python): it re-checks the slots recorded at build time - a parameter object
        replaced in its module, a parameter whose storage moved (``.to()``, ``p.data = ...``), a sub-module swapped."""
        if model is not self._model:
            return False
        for d, k, q, ptr in self._slots:
            cur = d.get(k)
            if cur is not q or cur.data_ptr() != ptr:
                return False
        for d, k, child in self._mods:
            if d.get(k) is not child:
                return False
        return True

    def bucket_ranges(self, n_buckets):
        """Contiguous [lo, hi) ranges of the flat gradient that complete in this order during backward."""
        bounds = [0]
        # Split on parameter boundaries.  The LAST bucket completes with the last backward kernel, so its all-reduce is
        # the only one whose latency is exposed in front of the optimiser: keep it tiny (the final ~2 % of the
        # gradient: the first blocks and the stem, a latency-only exchange); the buckets before it share the rest
        # equally and overlap the remaining backward kernels.
        tail = 0.98 if n_buckets > 1 else 1.0
        targets = [self.n_trainable * tail * k / max(n_buckets - 1, 1) for k in range(1, n_buckets)]
        acc = 0
        for name in self.names:
            if name in self.no_grad_names:
                continue
            acc = self.offsets[name][0] + self.offsets[name][1]
            if len(bounds) <= len(targets) and acc >= targets[len(bounds) - 1] and acc < self.n_trainable:
                bounds.append(acc)
        bounds.append(self.n_trainable)
        return [(bounds[i], bounds[i + 1]) for i in range(len(bounds) - 1) if bounds[i + 1] > bounds[i]]


class Plan:
    """Buffers + static shape data for one (batch, input size, mode, storage type).  ``dtype`` ("f32" / "bf16",
    ``LSSD3D.compute_dtype``) is how raw convolution outputs and activation gradients are stored in HBM; weights, BatchNorm
    vectors / statistics, head inputs and outputs and weight-gradient sums are fp32 / fp64 either way.  What the bf16 step
    lays out differently is in the branches on ``bf16`` below; every other line serves both.  A plan also holds the BatchNorm
    folds of its forward pass (``folds``: see ``plan_folds``) and a training plan the kernel routes of its backward pass
    (``routes``: see ``plan_routes``), fixed like its buffers when it is built."""

    def __init__(self, engine, N, in_dims, device, need_grad, dtype="f32"):
        L = _lib.load()
        m, specs = engine.model, engine.layer_specs
        ncls = m.n_classes
        bf16 = dtype == "bf16"
        self.N, self.in_dims, self.need_grad, self.bf16 = N, tuple(in_dims), need_grad, bf16
        self.ops = {op: names[bf16] for op, names in OPS.items() if names[bf16] is not None}  # this storage type's kernels
        act = dict(dtype=torch.bfloat16 if bf16 else torch.float32, device=device)  # y, z, g_y, g_z
        f32 = dict(dtype=torch.float32, device=device)
        f64 = dict(dtype=torch.float64, device=device)
        self.dims = []  # output dims per feature index
        cur = tuple(in_dims)
        for sp in specs:
            cur = tuple(conv_out(d, s) for d, s in zip(cur, sp["stride"]))
            self.dims.append(cur)
        self.y = []   # raw conv output of feature i (stem conv / block pointwise)
        self.z = [None]  # raw depthwise output of block i
        self.bn_y = []   # (BN_ROWS, C) BatchNorm vectors for y[i]
        self.bn_z = [None]
        # one statistics buffer per BatchNorm (np_* partials per channel: the counts of the kernels of this storage type): the
        # consumer folds them in its prologue while the finalize kernel (running stats + vectors for backward) reads them on
        # a side stream
        self.np_y, self.np_z, self.part_y, self.part_z = [], [None], [], [None]
        for i, sp in enumerate(specs):
            D, H, W = self.dims[i]
            if i == 0:
                self.np_y.append(L.msl_stem_conv_fwd_num_partials(N, D, H, W))
            else:
                pd, ph, pw = self.dims[i - 1]
                self.z.append(torch.empty((N, sp["cin"], D, H, W), **act))
                self.bn_z.append(torch.zeros((BN_ROWS, sp["cin"]), **f32))
                if bf16:
                    self.np_z.append(L.msl_dwconv_fwd_bf16_num_partials(N, sp["cin"], pd, ph, pw, sp["stride"][0]))
                    self.np_y.append(L.msl_pwconv_fwd_bf16_num_partials(N, D * H * W))
                else:
                    self.np_z.append(L.msl_dwconv_fwd_num_partials(N, sp["cin"], pd, ph, pw, sp["stride"][0]))
                    self.np_y.append(L.msl_pwconv_fwd_num_partials(N, sp["cin"], sp["cout"], D * H * W))
                self.part_z.append(torch.empty(2 * sp["cin"] * self.np_z[i], **f64))
            self.y.append(torch.empty((N, sp["cout"], D, H, W), **act))
            self.bn_y.append(torch.zeros((BN_ROWS, sp["cout"]), **f32))
            self.part_y.append(torch.empty(2 * sp["cout"] * self.np_y[i], **f64))

        # heads: on the fp32 kernels from a zero-haloed fp32 copy of the feature map (the fp32 step; the bf16 training step
        # always, bf16 inference unless Engine.bf16_heads says "bf16"), else on the bf16 MFMA kernel from a channels-last copy
        self.feat_ids = list(m.aspect_ratios.keys())
        self.prior_off, off = {}, 0
        for f in self.feat_ids:
            self.prior_off[f] = off
            D, H, W = self.dims[f]
            off += D * H * W * m.boxes_per_location
        self.P = off
        self.f32_heads = not bf16 or need_grad or engine.bf16_heads != "bf16"
        if self.f32_heads:
            self.fpad, self.Wf, self.Wb, self.head_ws = {}, {}, {}, {}
            for f in self.feat_ids:
                C = specs[f]["cout"]
                D, H, W = self.dims[f]
                self.fpad[f] = torch.zeros((N, C, D + 2, H + 2, W + 2), **f32)
                ne = L.msl_head_packed_weight_elems(C, ncls)
                self.Wf[f] = torch.empty(ne, **f32)
                self.Wb[f] = torch.empty(ne, **f32)
                ws = max(L.msl_head_fwd_workspace_bytes(N, C, D, H, W, ncls),
                         L.msl_head_bwd_weight_workspace_bytes(N, C, D, H, W, ncls) if need_grad else 0)
                self.head_ws[f] = torch.empty(max(ws // 4, 1), **f32)
        else:
            bf = dict(dtype=torch.bfloat16, device=device)
            self.fpad_cl = {f: torch.zeros((N,) + tuple(d + 2 for d in self.dims[f]) + (specs[f]["cout"],), **bf) for f in self.feat_ids}
            self.Wp = {f: torch.empty(L.msl_head_packed_weight_bf16_elems(specs[f]["cout"]), **bf) for f in self.feat_ids}
        self.locs = torch.empty((N, self.P, 6), **f32)
        self.scores = torch.empty((N, self.P, ncls), **f32)
        self.nan_flag = torch.zeros(1, dtype=torch.int32, device=device)

        # fp64 scratch for per-channel sums that one kernel leaves for the next (Engine._bn_bwd and the producers of its
        # ``pre_np``): the largest count over the layers.  The fp32 step sizes it from its forward counts too.
        bwd_np = L.msl_bn_relu_bwd_bf16_num_partials if bf16 else L.msl_bn_relu_bwd_num_partials
        part_elems = 0
        for i, sp in enumerate(specs):
            D, H, W = self.dims[i]
            if not bf16:
                part_elems = max(part_elems, 2 * sp["cout"] * self.np_y[i], 2 * sp["cin"] * self.np_z[i] if i else 0)
            if need_grad:
                part_elems = max(part_elems, 2 * sp["cout"] * bwd_np(N, D * H * W))
                if i:
                    part_elems = max(part_elems, 2 * sp["cin"] * bwd_np(N, D * H * W), 2 * sp["cin"] * max(
                        L.msl_dwconv_bwd_data_bnreduce_num_partials(N, sp["cin"], *self.dims[i - 1]), 0))

        # fp32-only one-pass backward kernels (filled below; a bf16 plan has none)
        self.pw_fused = {}       # block -> (slabs [NP][Cout][Cin], fp64 statistics partials [2][Cin][NP], NP): csrc/pwfused.hip
        self.dw_fused_part = {}  # big stride-2 block -> (fp64 partials [Cin*27][NP], NP): weight gradient with the bwd-data pass
        if need_grad:
            self.g_y = [torch.empty_like(t) for t in self.y]
            self.g_z = [None] + [torch.empty_like(t) for t in self.z[1:]]
            mt16 = 16 * ((12 + 2 * ncls + 15) // 16)
            self.dO = {f: torch.zeros((N, mt16) + tuple(d + 2 for d in self.dims[f]), **f32) for f in self.feat_ids}
            self.ws_stem = torch.empty(max(L.msl_stem_conv_bwd_weight_workspace_bytes(specs[0]["cin"]) // 4, 1), **f32)
            # Deferred gradient reduction (Engine._grad_reduce): every weight-gradient kernel leaves its partial sums in a
            # buffer of ITS OWN (they all stay live until the one batched reduction in front of the optimiser):
            #   pw_slabs[i]  fp32 [nslabs][Cout][Cin] (None: the kernel covers the whole position range and writes dW itself)
            #   dw_part[i]   fp64 [Cin*27][NP]  (bf16: the depthwise weight-gradient kernel has the forward's partition)
            self.pw_nslabs, self.pw_slabs, self.dw_np, self.dw_part = [0], [None], [0], [None]
            for i in range(1, len(specs)):
                cin, cout = specs[i]["cin"], specs[i]["cout"]
                D, H, W = self.dims[i]
                pd, ph, pw = self.dims[i - 1]
                if bf16:
                    ns = L.msl_pwconv_bwd_weight_bf16_nslabs(N, cin, cout, D * H * W)
                    if ns < 1:
                        raise _lib.HipKernelError(f"msl_pwconv_bwd_weight_bf16_nslabs failed for block {i}")
                    npd = self.np_z[i]
                else:
                    ns = L.msl_pwconv_bwd_weight_nslabs(N, cin, cout, D * H * W)
                    npd = L.msl_dwconv_bwd_weight_num_partials(N, cin, pd, ph, pw, specs[i]["stride"][0])
                    part_elems = max(part_elems, cin * 27 * npd)
                self.pw_nslabs.append(ns)
                self.pw_slabs.append(torch.empty(ns * cin * cout, **f32) if ns > 1 else None)
                self.dw_np.append(npd)
                self.dw_part.append(torch.empty(cin * 27 * npd, **f64))
            for i in () if bf16 else range(1, len(specs)):  # fp32 only (part_elems is final for fp32 here)
                cin, cout = specs[i]["cin"], specs[i]["cout"]
                D, H, W = self.dims[i]
                pd, ph, pw = self.dims[i - 1]
                nf = L.msl_pwconv_bwd_fused_num_partials(N, cin, cout, D * H * W)
                if nf > 0:
                    self.pw_fused[i] = (torch.empty(nf * cin * cout, **f32), torch.empty(2 * cin * nf, **f64), nf)
                if i >= 2 and specs[i]["stride"][0] == 2 and N * pd * ph * pw > 65536:
                    npw = L.msl_dwconv_s2_bwd_bnreduce_bww_num_partials(N, cin, pd, ph, pw)
                    if npw > 0 and 2 * cin * npw <= part_elems:
                        self.dw_fused_part[i] = (torch.empty(cin * 27 * npw, **f64), npw)
            self.head_nslabs = {f: L.msl_head_conv_bwd_weight_nslabs(N, specs[f]["cout"], *self.dims[f], ncls) for f in self.feat_ids}
            self.stem_nslabs = L.msl_stem_conv_bwd_weight_nslabs(N, *self.in_dims, *specs[0]["stride"])
            # fused stem backward (block 1 is a stride-2 depthwise layer fed by a 32-channel stem that is not a head
            # feature): its dL/d(stem activation) is never materialised (plan_routes: "fused_stem").  fp32: where the sums
            # fit the scratch, laid out whatever Engine.fuse_stem says; bf16: only with Engine.fuse_stem, the scratch grows
            self.fused_stem_np = -1
            fusable = (len(specs) > 1 and specs[0]["cout"] == 32 and specs[1]["cin"] == 32
                       and tuple(specs[1]["stride"]) == (2, 2, 2) and 0 not in self.feat_ids)
            if fusable and (engine.fuse_stem or not bf16):
                np_f = L.msl_dwconv_s2_bwd_bnreduce_bww_num_partials(N, 32, *self.dims[0])
                small = self.y[0].numel() * self.y[0].element_size() < (1 << 32)  # the fused kernel uses 32-bit byte offsets
                if np_f > 0 and small and (bf16 or 2 * 32 * np_f <= part_elems):
                    self.fused_stem_np = np_f
                    self.partials_wf = torch.empty(32 * 27 * np_f, **f64)
                    self.w1_taps_t = torch.empty((27, 32), **f32)
                    if bf16:
                        part_elems = max(part_elems, 2 * 32 * np_f)
                        self.g_y[0] = None  # never materialised
        if need_grad or not bf16:  # (a bf16 inference plan has none)
            self.partials = torch.empty(max(part_elems, 1), **f64)

        # ---- what the passes write later (declared here so that no reader has to probe for it) -----------------------------
        self.events = {}           # Engine._event
        self.saved_input = None    # Engine.forward / _forward_bf16, FusedTrainer (replayed steps)
        self.generation = 0        # the same: +1 per forward pass
        self.trained_mode = False  # the same: was the latest forward pass a train-mode one?
        self.stem_dw_eval = False  # Engine.forward / _forward_bf16: stem + block-1 depthwise ran as one launch
        self.loss_fold = None      # FusedTrainer._eager_step: (parts, nparts, loss_out, npos) of the one-launch loss
        self.bn_table = {False: (None, None), True: (None, None)}  # Engine._finalize_all: eval_mode -> (key, (table, n, channels))
        self.pwb_key = self.pwb_args = None      # Engine._pw_bww_batch
        self.pack_key = self.pack_args = None    # Engine._pack_head_weights
        self.gpack_key = self.gpack_args = None  # Engine._head_gpack_batch
        self.grad_tables = {}       # Engine._grad_reduce
        # the backward pass, decided once: what Engine.backward / _backward_bf16 launch and Engine._grad_reduce folds
        self.routes = plan_routes(self, engine) if need_grad else None  # [StemRoute, Route of block 1, ...]
        # and the BatchNorm folds of a train-mode forward pass (an eval-mode pass folds nothing and finalizes nothing)
        self.folds = plan_folds(self, engine)


class Engine:
    """Schedule: the main stream carries the dependency chain (backbone forward; activation-gradient chain in
    backward).  Two side streams take what is off that chain and too small to fill 256 CUs on its own:
    * ``heads``  — forward: the head convolutions of scales 3 and 5 run beside backbone blocks 4-7; backward: their
      weight / data gradients run beside the backward of blocks 7..4;
    * ``wgrad``  — every pointwise / depthwise weight gradient runs beside the next layer's data-gradient chain.
    Forks and joins are hipEvents recorded through the C ABI, so the schedule survives launch-program replay.
    Which kernel form carries each piece of the backward pass is fixed per plan (``Plan.routes``), and so is which
    BatchNorms the forward pass folds into their consumers (``Plan.folds``); the four passes only decide per call what the
    caller can change between calls (train / eval mode, streams, reducer stages, batching)."""

    def __init__(self, model):
        self.model = model
        # ---- schedule options: plain attributes (defaults = what the measurements of rounds 1-3 chose; probes and
        #      `bench.py --opt name=value` set them; the library reads no environment variable for any of them) ------------
        self.multi_stream = True
        # (fold_bn, fold_np_max, bf16_heads and fuse_stem are baked into a plan when it is built: see plan_for)
        self.fold_bn = False      # fold EVERY BatchNorm into its consumers (slower: big layers have thousands of partials)
        # fold only the BatchNorms with at most this many statistics partials per channel into their depthwise / pointwise
        # consumers (one finalize launch less on the chain each; a folded stem BatchNorm - 1024 partials - costs block 1's
        # depthwise what the launch saves)
        self.fold_np_max = 512     # (65536 - the stem's 1024 partials too - gains another 2 us per step but costs the roofline
        #                             kernel, block 1's depthwise forward, 4.5 us: the launch stays)
        # bf16 path: head convolutions on the fp32 kernels from an fp32 feature copy ("f32": measured faster at every size
        # tried, and no second rounding of the head operands) or on the bf16 MFMA kernel from a channels-last bf16 copy
        # ("bf16", inference only)
        self.bf16_heads = "f32"
        # set by a caller (FusedTrainer) while it records a step whose heads stream it orders itself, every step, behind the
        # previous step's optimiser: the forward pass then has no "fwd_start" record at the head of the chain
        self.prologue_presynced = False
        # pointwise weight gradients of the tail blocks in ONE launch (single process only).  Paid while a fork cost the chain
        # 5-7 us; with stop-event forks (~1 us) four separate launches that start as their dL/dy arrive are 1.5 % faster
        self.batch_tail_pw = False
        self.batch_head_gpack = True  # head-gradient images of all scales in one launch
        self.fuse_stem = True     # block-1 / stem backward without materialising dL/d(stem activation)
        self.side = {}
        self.arena = None
        self.plans = {}
        self.prof, self.prof_tags = None, None
        feats = model.base.features
        specs = []
        for i, f in enumerate(feats):
            if i == 0:
                conv = f[0]
                specs.append(dict(kind="stem", cin=conv.in_channels, cout=conv.out_channels, stride=tuple(conv.stride)))
            else:
                specs.append(dict(kind="block", cin=f.conv1.in_channels, cout=f.conv2.out_channels,
                                  stride=tuple(f.conv1.stride)))
        self.layer_specs = specs

    # ------------------------------------------------------------------------------------------------
    def ensure_arena(self, device):
        if self.arena is None or self.arena.flat.device != device or not self.arena.owns(self.model):
            self.arena = ParamArena(self.model, device)
            self.plans = {}
        return self.arena

    def plan_for(self, x, need_grad):
        """The plan for this input shape, mode and the model's storage type (built once).  The key holds the options a plan
        bakes in when it is built: setting one afterwards builds a new plan."""
        dtype = getattr(self.model, "compute_dtype", "f32")
        bf16 = dtype == "bf16"
        key = (dtype, x.shape[0], tuple(x.shape[2:]), x.device, need_grad, self.bf16_heads if bf16 else None,
               self.fuse_stem if need_grad else None, self.fold_bn, self.fold_np_max)
        p = self.plans.get(key)
        if p is None:
            p = self.plans[key] = Plan(self, x.shape[0], x.shape[2:], x.device, need_grad, dtype)
        return p

    @staticmethod
    def _stream():
        return torch.cuda.current_stream().cuda_stream

    def side_streams(self, device):
        """(heads, wgrad) torch streams for ``device`` (created once)."""
        key = (device.type, device.index)
        if key not in self.side:
            # (restricting the side streams to a CU subset with hipExtStreamCreateWithCUMask was measured 8-9 % slower for
            # every mask - half, quarter, three quarters of the chip - so they are ordinary streams)
            self.side[key] = (torch.cuda.Stream(device=device), torch.cuda.Stream(device=device))
        return self.side[key]

    @staticmethod
    def _event(pl, name):
        """The plan's event ``name``.  Events that only order this GPU's own streams are created without the
        system-scope fence when ``_lib.DEVICE_SCOPE_EVENTS`` is set; the ``bucket_*`` events, which a communication
        stream (RCCL: peer-to-peer traffic) waits for, always keep it."""
        ev = pl.events.get(name)
        if ev is None:
            ev = pl.events[name] = _lib.new_event(device_only=not name.startswith("bucket_"))
        return ev

    @classmethod
    def _record(cls, pl, name, stream):
        ev = cls._event(pl, name)
        _lib.call("msl_event_record", ev, stream, tag="event")
        return ev

    @staticmethod
    def _wait(stream, ev):
        _lib.call("msl_stream_wait_event", stream, ev, tag="event")

    @classmethod
    def _fork(cls, pl, name, src, dst):
        """dst stream waits for everything enqueued on src so far."""
        ev = cls._event(pl, name)
        _lib.call("msl_event_record", ev, src, tag="event")
        _lib.call("msl_stream_wait_event", dst, ev, tag="event")

    # -- optional per-launch HIP-event timing (bench.py's roofline leg) -------------------------------------
    def start_profile(self, tags=None):
        """Record a HIP event pair (on the launch stream) around every tagged launch; tags=None -> all."""
        self.prof, self.prof_tags = {}, (None if tags is None else set(tags))

    def prof_all(self):
        """True while every launch is being timed (the trainer then uses the eager path, which tags every launch)."""
        return self.prof is not None and self.prof_tags is None

    def stop_profile(self):
        """-> {tag: [ms, ...]} (synchronises)."""
        torch.cuda.synchronize()
        out = {}
        for t, evs in (self.prof or {}).items():
            out[t] = [(_lib.elapsed_ms(e[1], e[2]) if e[0] == "c" else e[0].elapsed_time(e[1])) for e in evs]
            for e in evs:  # the native replay creates a fresh timed pair per tagged launch and replay: release them
                if e[0] == "c":
                    _lib.destroy_event(e[1])
                    _lib.destroy_event(e[2])
        self.prof = None
        return out

    def _k(self, tag, name, *args):
        if self.prof is None or (self.prof_tags is not None and tag not in self.prof_tags):
            _lib.call(name, *args, tag=tag)
            return
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.call(name, *args, tag=tag)
        e1.record()
        self.prof.setdefault(tag, []).append((e0, e1))

    @staticmethod
    def _hook(cb, tag):
        if cb is not None:
            cb(tag)
            _lib.record_hook(lambda: cb(tag), tag=f"hook:{tag}")

    def _bn_entry(self, pl, kind, i):
        """(bn module, vector buffer, statistics partials, NP, element count) of the BatchNorm of y[i] ("y") or z[i] ("z")."""
        feats = self.model.base.features
        D, H, W = pl.dims[i]
        if kind == "z":
            return feats[i].bn1, pl.bn_z[i], pl.part_z[i], pl.np_z[i], pl.N * D * H * W
        return (feats[i].bn2 if i else feats[0][1]), pl.bn_y[i], pl.part_y[i], pl.np_y[i], pl.N * D * H * W

    def _bn_finalize(self, pl, kind, i, st):
        """One BatchNorm of a train-mode pass finalized by a launch of its own (``Fold.chain`` / not ``Fold.pw``)."""
        bn, vec, partials, NP, count = self._bn_entry(pl, kind, i)
        mom = 0.1 if bn.momentum is None else bn.momentum
        _lib.call("msl_bn_finalize", ptr(partials), NP, float(count), ptr(bn.weight), ptr(bn.bias), ptr(bn.running_mean),
                  ptr(bn.running_var), ptr(bn.num_batches_tracked), mom, bn.eps, ptr(vec[0]), ptr(vec[1]), ptr(vec[2]),
                  ptr(vec[3]), vec.shape[1], st)

    def _forward_open(self, x, training, need_grad):
        """What both forward passes do before their first launch -> (plan, chain stream, heads stream).  The heads stream is
        the chain itself for a one-stream pass and for bf16 inference on the bf16 head kernel (that pass used to be one stream
        on either head route: 86 us of feature copies and head convolutions on the chain at 192^3 x 2)."""
        x = x.contiguous().float()
        self.ensure_arena(x.device)
        pl = self.plan_for(x, need_grad)
        pl.generation += 1
        pl.saved_input, pl.trained_mode = x, training
        st = self._stream()
        return pl, st, self.side_streams(x.device)[0].cuda_stream if self.multi_stream and pl.f32_heads else st

    def _forward_prologue(self, pl, training, st, stH):
        """What a forward pass starts with -> the event behind the packed head weights (None: they are on the chain).
        ``stH`` is the heads stream, or ``st`` for a pass without one."""
        ones = [1] * len(pl.y)
        eval_np = (ones, ones) if pl.bf16 else (pl.np_y, pl.np_z)  # partial counts (of y[i], of z[i]) of the eval-mode table
        if not training:
            # eval mode: (scale, shift) of all BatchNorms depend on parameters and running statistics only - one launch.  It
            # is the FIRST launch of the pass, in front of the prologue's fork: the fork's record then rides on it as a stop
            # event instead of being a packet of its own at the head of the chain (the heads stream still starts behind
            # everything the chain held before this pass)
            every = []
            for kind, i in [("y", 0)] + [(k, i) for i in range(1, len(pl.y)) for k in ("z", "y")]:
                every.append(self._bn_entry(pl, kind, i)[:3] + (eval_np[1 if kind == "z" else 0][i], 1.0))
            self._finalize_all(pl, every, st, eval_mode=True)
        # the NaN-flag reset and the MFMA-fragment copies of the head weights (all scales, once per pass) are needed 200 us
        # into the pass (first head convolution) and at its end (loss / NaN checks): on the heads stream they cost the
        # dependency chain nothing (in front of the stem they were a memset + a launch + two dispatch gaps, ~20 us).  The
        # heads stream first waits for everything the chain has done so far (the previous step's optimiser wrote the weights).
        if stH != st and not self.prologue_presynced:  # (a caller that orders the heads stream itself: FusedTrainer)
            self._fork(pl, "fwd_start", st, stH)
        _lib.call("msl_fill_u32", ptr(pl.nan_flag), 0, 1, stH)
        if pl.f32_heads:  # (the bf16 head kernel packs its weights scale by scale)
            self._pack_head_weights(pl, stH)
        return self._record(pl, "head_pack_done", stH) if stH != st else None

    def _forward_epilogue(self, pl, nan_check, st, stH):
        if stH != st:
            self._fork(pl, "fwd_heads_done", stH, st)
        if nan_check:  # the fused training step lets the loss kernel set the flag instead (it reads both tensors anyway)
            _lib.call("msl_nan_flag2", ptr(pl.locs), pl.locs.numel(), 1, ptr(pl.scores), pl.scores.numel(), 2, ptr(pl.nan_flag), st)
        return pl.locs, pl.scores

    # -- forward emitters: one layer launch each, for both storage types (entry points: ``pl.ops``, folds: ``pl.folds``) -----
    def _stem_forward(self, pl, training, st):
        """features[0]'s convolution -> raw y[0]; eval mode, where the kernel takes the shape: with block 1's depthwise
        layer, -> z[1] (``pl.stem_dw_eval``)."""
        feats, sp, N = self.model.base.features, self.layer_specs[0], pl.N
        D, H, W = pl.in_dims
        x, w = ptr(pl.saved_input), ptr(feats[0][0].weight)
        pl.stem_dw_eval = self._stem_dw_eval(self.layer_specs, training, N, D, H, W)
        if pl.stem_dw_eval:
            self._k("stem_fwd", pl.ops["stem_dw_eval"], x, w, ptr(pl.bn_y[0][0]), ptr(pl.bn_y[0][1]), ptr(feats[1].conv1.weight),
                    ptr(pl.z[1]), N, sp["cin"], D, H, W, st)
        else:
            self._k("stem_fwd", pl.ops["stem_fwd"], x, w, ptr(pl.y[0]), ptr(pl.part_y[0]) if training else None, N, sp["cin"],
                    D, H, W, *sp["stride"], st)

    def _dw_forward(self, pl, i, training, st):
        """Block i's depthwise layer: y[i-1] -> raw z[i], folding the BatchNorm of y[i-1] from its partials (``Fold.dw``) or
        reading its vectors."""
        if i == 1 and pl.stem_dw_eval:
            return  # z1 came with the stem
        feats, sp, N = self.model.base.features, self.layer_specs[i], pl.N
        pd, ph, pw = pl.dims[i - 1]
        w, shape = ptr(feats[i].conv1.weight), (N, sp["cin"], pd, ph, pw, sp["stride"][0])
        if training and pl.folds.at[i - 1].dw:
            bn = feats[0][1] if i == 1 else feats[i - 1].bn2
            self._k(f"dw_fwd{i}", pl.ops["dw_fwd_fold"], ptr(pl.y[i - 1]), ptr(pl.part_y[i - 1]), pl.np_y[i - 1],
                    float(N * pd * ph * pw), ptr(bn.weight), ptr(bn.bias), bn.eps, w, ptr(pl.z[i]), ptr(pl.part_z[i]), *shape, st)
        else:
            unused = () if pl.bf16 else (0,)
            self._k(f"dw_fwd{i}", pl.ops["dw_fwd"], ptr(pl.y[i - 1]), ptr(pl.bn_y[i - 1][0]), ptr(pl.bn_y[i - 1][1]), w,
                    ptr(pl.z[i]), ptr(pl.part_z[i]) if training else None, *shape, *unused, st)

    def _pw_forward(self, pl, i, training, st):
        """Block i's pointwise layer: z[i] -> raw y[i], folding the BatchNorm of z[i] (``Fold.pw``) or reading its vectors,
        which a train-mode pass finalizes right in front."""
        blk, sp, N = self.model.base.features[i], self.layer_specs[i], pl.N
        D, H, W = pl.dims[i]
        w, shape = ptr(blk.conv2.weight), (N, sp["cin"], sp["cout"], D * H * W)
        if training and pl.folds.at[i].pw:
            self._k(f"pw_fwd{i}", pl.ops["pw_fwd_fold"], ptr(pl.z[i]), ptr(pl.part_z[i]), pl.np_z[i], float(N * D * H * W),
                    ptr(blk.bn1.weight), ptr(blk.bn1.bias), blk.bn1.eps, w, ptr(pl.y[i]), ptr(pl.part_y[i]), *shape, st)
        else:
            if training:
                self._bn_finalize(pl, "z", i, st)
            self._k(f"pw_fwd{i}", pl.ops["pw_fwd"], ptr(pl.z[i]), ptr(pl.bn_z[i][0]), ptr(pl.bn_z[i][1]), w, ptr(pl.y[i]),
                    ptr(pl.part_y[i]) if training else None, *shape, st)

    def _feature_copy(self, pl, i, training, st):
        """The zero-haloed fp32 copy of feature map i that its fp32 head convolution reads, with BatchNorm and ReLU applied
        (``Fold.copy``: from the partials)."""
        bn, sp, N = self.model.base.features[i].bn2, self.layer_specs[i], pl.N
        D, H, W = pl.dims[i]
        dst = (ptr(pl.fpad[i]),) if pl.bf16 else (None, ptr(pl.fpad[i]))  # (fp32: an unused slot in front)
        if training and pl.folds.at[i].copy:
            self._k(f"materialize{i}", pl.ops["copy_fold"], ptr(pl.y[i]), ptr(pl.part_y[i]), pl.np_y[i], float(N * D * H * W),
                    ptr(bn.weight), ptr(bn.bias), bn.eps, *dst, N, sp["cout"], D, H, W, st)
        else:
            self._k(f"materialize{i}", pl.ops["copy"], ptr(pl.y[i]), ptr(pl.bn_y[i][0]), ptr(pl.bn_y[i][1]), *dst, N,
                    sp["cout"], D, H, W, st)

    # ------------------------------------------------------------------------------------------------
    def forward(self, x, training, need_grad, nan_check=True, after_block=None):
        """x (N,Cin,D,H,W) fp32 on the GPU -> (locs (N,P,6), scores (N,P,n_classes)).
        ``after_block``: {block index: callable} - side work (the trainer's target matching) to enqueue once that block's
        launches have been issued."""
        if not x.is_cuda:
            raise _lib.HipKernelError("mslesions3d_amd runs on the HIP device only (no CPU fallback): move the "
                                      "model and the input to 'cuda'")
        m = self.model
        if getattr(m, "compute_dtype", "f32") == "bf16":
            return self._forward_bf16(x, training=training, need_grad=need_grad, nan_check=nan_check, after_block=after_block)
        pl, st, stH = self._forward_open(x, training, need_grad)
        specs = self.layer_specs
        ev_pack = self._forward_prologue(pl, training, st, stH)
        # which BatchNorms the consumers fold from the partials, and which a launch on the chain finalizes right behind its
        # producer: fixed per plan.  The folded ones (bn module, vector buffer, partials, NP, element count) get their running
        # statistics and backward vectors from ONE launch after the last block: nothing in the forward pass reads them
        fo = pl.folds.at if training else [NO_FOLD] * len(specs)
        bn_layers = [self._bn_entry(pl, k, i) for k, i in pl.folds.batch] if training else []
        deferred = []
        ev_bn_done = None

        def flush():
            nonlocal deferred
            for fn in deferred:
                fn()
            deferred = []

        self._stem_forward(pl, training, st)  # (features[0] = Conv3d + BN + ReLU)
        if fo[0].chain:
            self._bn_finalize(pl, "y", 0, st)
        for i in range(1, len(specs)):
            self._dw_forward(pl, i, training, st)
            flush()
            self._pw_forward(pl, i, training, st)
            flush()
            if fo[i].chain:
                self._bn_finalize(pl, "y", i, st)
            ev_feat = None  # the event a side stream waits for at this block, shared by everything forked here
            if i in pl.fpad:
                # this scale's head convolution only needs the feature map: run it beside the remaining blocks - and with it
                # the zero-haloed activation copy it reads (nothing on the chain reads that copy: the next depthwise layer
                # re-creates the activation from the raw output itself), when the BatchNorm is folded from the partials
                # (an unfolded one is finalised on the chain first, so its vectors are ready on either stream)
                last = i == len(specs) - 1
                if self.multi_stream and not last:
                    ev = ev_feat = self._record(pl, f"fwd_feat{i}", st)
                    deferred.append(lambda ev=ev, i=i: (self._wait(stH, ev), self._feature_copy(pl, i, training, stH),
                                                        self._head_forward(pl, i, stH)))
                else:
                    if last and bn_layers and self.multi_stream:
                        ev_bn_done = self._finalize_all_beside(pl, bn_layers, st)
                    self._feature_copy(pl, i, training, st)
                    if ev_pack is not None:  # this scale's convolution runs on the chain: the packed weights come from stH
                        self._wait(st, ev_pack)
                        ev_pack = None
                    self._head_forward(pl, i, st)
            if after_block and i in after_block:
                after_block[i](ev_feat)  # (side work forked after this block waits for the same event: one record, not two)
        flush()
        if ev_bn_done is not None:
            self._wait(st, ev_bn_done)
        elif bn_layers:
            self._finalize_all(pl, bn_layers, st)
        return self._forward_epilogue(pl, nan_check, st, stH)

    # ------------------------------------------------------------------------------------------------
    def _forward_bf16(self, x, training=False, need_grad=False, nan_check=True, after_block=None):
        """Forward with bf16 activations in HBM (csrc/bf16.hip + the bf16 head kernel): fp32 input volume, fp32 weights and
        BatchNorm vectors / statistics, bf16 everything in between, fp32 locs / scores out.  A BatchNorm that is not folded is
        finalized in front of the first launch that reads its vectors (``Fold.chain``)."""
        # The schedule of the fp32 pass, except: nothing is issued a layer late (a feature copy and its head convolution are
        # forked and issued in place), ``after_block`` fires in front of a "producer" finalize, a "consumer" finalize sits in
        # front of the depthwise layer, the batched finalize stays on the chain, and inference may take the bf16 head route
        pl, st, stH = self._forward_open(x, training, need_grad)
        specs, last = self.layer_specs, len(self.layer_specs) - 1
        ev_pack = self._forward_prologue(pl, training, st, stH)
        fo = pl.folds.at if training else [NO_FOLD] * len(specs)
        self._stem_forward(pl, training, st)
        for i in range(1, len(specs)):
            if fo[i - 1].chain == "consumer":
                self._bn_finalize(pl, "y", i - 1, st)
            self._dw_forward(pl, i, training, st)
            self._pw_forward(pl, i, training, st)
            if after_block and i in after_block:
                after_block[i](None)
            # a feature map's BatchNorm: folded into the fp32 copy (and into the next depthwise layer) from the partials when
            # they are few - no finalize launch on the chain; else finalised here (the copy below reads the vectors)
            if fo[i].chain == "producer":
                self._bn_finalize(pl, "y", i, st)
            if i in pl.feat_ids and pl.f32_heads:
                # the fp32 zero-haloed copy only feeds this scale's head convolution: it goes to the heads stream with it
                # (as in the fp32 pass; 6-8 us per scale off the chain)
                sF = stH if i != last else st
                if sF != st:
                    self._fork(pl, f"fwd_feat{i}", st, stH)
                self._feature_copy(pl, i, training, sF)
                if sF == st and ev_pack is not None:  # the packed weights come from the heads stream
                    self._wait(st, ev_pack)
                    ev_pack = None
                self._head_forward(pl, i, sF)
            elif i in pl.feat_ids:
                self._head_forward_bf16(pl, i, st)
        if training and pl.folds.batch:  # running statistics and backward vectors of the folded BatchNorms: one launch
            self._finalize_all(pl, [self._bn_entry(pl, k, i) for k, i in pl.folds.batch], st)
        return self._forward_epilogue(pl, nan_check, st, stH)

    def _bn_bwd_bf16(self, g, y, vec, bn_name, N, C, S, pl, st, pre_np=None):
        """In place: g (bf16, = dL/d relu(bn(y))) becomes dL/dy; dgamma / dbeta into the gradient arena.
        ``pre_np``: the producer of g already left that many reduce partials per channel in pl.partials."""
        gv = self.arena.grad_views
        if pre_np is None:
            if bn_bwd_one_launch(True, N, S):
                self._k("bn_bwd_fused:" + bn_name, "msl_bn_relu_bwd_fused_bf16", ptr(g), ptr(y), ptr(vec), ptr(gv[bn_name + ".weight"]),
                        ptr(gv[bn_name + ".bias"]), ptr(g), N, C, S, st)
                return
            pre_np = _lib.load().msl_bn_relu_bwd_bf16_num_partials(N, S)
            self._k("bn_bwd_reduce:" + bn_name, "msl_bn_relu_bwd_reduce_bf16", ptr(g), ptr(y), ptr(vec[0]), ptr(vec[1]), ptr(vec[2]),
                    ptr(vec[3]), ptr(pl.partials), N, C, S, st)
        _lib.call("msl_bn_bwd_finalize", ptr(pl.partials), pre_np, float(N * S), ptr(gv[bn_name + ".weight"]),
                  ptr(gv[bn_name + ".bias"]), ptr(vec[4]), ptr(vec[5]), C, st)
        self._k("bn_bwd_apply:" + bn_name, "msl_bn_relu_bwd_apply_bf16", ptr(g), ptr(y), ptr(vec), ptr(g), N, C, S, st)

    def _backward_bf16(self, pl, dlocs, dscores, on_bucket_ready=None):
        """Backward of the bf16 training step: activation gradients are bf16 tensors, weight gradients fp32 partial sums
        folded by the batched reduction.  Same three-stream schedule as the fp32 step (dependency chain on the main stream,
        head gradients of the earlier scales on the heads stream, weight gradients alternating over the two side streams);
        a data-parallel reducer gets each bucket as soon as the launches producing it are enqueued (as in the fp32 step)."""
        # The schedule of the fp32 pass, except: every side-stream launch is forked and issued in place, not one layer late
        # (both weight gradients of block i wait for one "dz" record made behind the channel link, in front of any other
        # depthwise form; odd blocks go to the wgrad stream, even ones to the heads stream), the chain's own scale goes first
        # on one stream too, and the tail's pointwise weight gradients are never batched
        st, stH, stW, dlocs, dscores, _, groups, report, last, side_feats, packed = self._backward_open(
            pl, dlocs, dscores, on_bucket_ready)
        ms = self.multi_stream
        self._head_backward(pl, last, dlocs, dscores, st, weight=False, packed=packed)  # its data gradient starts the chain
        if stW != st:
            self._wait(stW, self._record(pl, f"head_dO{last}", st))
        self._head_backward(pl, last, dlocs, dscores, stW, data=False)
        for f in reversed(side_feats) if ms else [f for f in pl.feat_ids if f != last]:
            self._head_backward(pl, f, dlocs, dscores, stH, self._event(pl, f"head_done{f}") if ms else None, packed=packed)
        report("heads")
        for i in range(last, 0, -1):
            link = pl.routes[i].dw in ("link", "link_bww")  # the per-channel link of the tail blocks, as in the fp32 step
            self._pw_backward(pl, i, st)
            accumulate = 1 if (i - 1) in pl.feat_ids else 0  # the heads already wrote their share
            if not link:
                self._bn_backward(pl, "z", i, st)
            if accumulate and (i - 1) in side_feats:
                self._wait(st, pl.events[f"head_done{i - 1}"])
            if link:
                self._channel_link(pl, i, accumulate, st)
            sX = st
            if ms:  # both weight gradients of the block on a side stream, once dL/dy_i and dL/dz_i are final
                sX = stW if i % 2 else stH
                self._wait(sX, self._record(pl, f"dz{i}", st))
            if not link:
                self._dw_backward(pl, i, accumulate, st)
            self._pw_wgrad(pl, i, sX)
            self._dw_wgrad(pl, i, sX)
            report(i)
        self._stem_backward(pl, st)
        self._backward_close(pl, groups, report, st, stH, stW)

    def _stem_dw_eval(self, specs, training, N, D, H, W):
        """Eval mode: may the stem and block 1's depthwise convolution run as one launch (csrc/stemdw.hip: the stem
        activation never goes to HBM)?"""
        if training or len(specs) < 2:
            return False
        if tuple(specs[0]["stride"]) != (2, 2, 2) or tuple(specs[1]["stride"]) != (2, 2, 2) or specs[0]["cout"] != 32:
            return False
        return bool(_lib.load().msl_stem_dw_fwd_eval_supported(N, specs[0]["cin"], D, H, W))

    def _finalize_all_beside(self, pl, bn_layers, st):
        """_finalize_all on the weight-gradient stream, ordered behind what ``st`` holds so far (the last pointwise
        convolution: every layer's partial sums exist) -> the event the chain waits for at the end of the pass.
        Nothing in the forward pass reads its outputs, so in the fp32 pass it runs beside the last head convolution
        instead of 9 us on the chain (-0.4 %).  The bf16 pass keeps it on the chain: its list is short (+0.4 % beside)."""
        stW = self.side_streams(pl.locs.device)[1].cuda_stream
        self._fork(pl, "fwd_bn_parts", st, stW)
        self._finalize_all(pl, bn_layers, stW)
        return self._record(pl, "fwd_bn_done", stW)

    @staticmethod
    def _bn_table(bn_layers):
        """Device table of the listed BatchNorms (bn module, vector buffer, partials, NP, element count) for
        msl_bn_finalize_batch / msl_bn_eval_affine_batch -> (table, entries, channels)."""
        L = _lib.load()
        esz = L.msl_bn_finalize_entry_bytes()
        host = (ctypes.c_ubyte * (esz * len(bn_layers)))()
        first = 0
        for k, (bn, vec, part, NP, count) in enumerate(bn_layers):
            C = vec.shape[1]
            mom = 0.1 if bn.momentum is None else bn.momentum
            _lib.check(L.msl_bn_finalize_table_set(ctypes.addressof(host), k, first, ptr(part), NP, float(count),
                                                   ptr(bn.weight), ptr(bn.bias), ptr(bn.running_mean),
                                                   ptr(bn.running_var), ptr(bn.num_batches_tracked), mom, bn.eps,
                                                   ptr(vec[0]), ptr(vec[1]), ptr(vec[2]), ptr(vec[3]), C),
                       "msl_bn_finalize_table_set")
            first += C
        return torch.frombuffer(bytearray(host), dtype=torch.uint8).to(vec.device), len(bn_layers), first

    def _finalize_all(self, pl, bn_layers, st, eval_mode=False):
        """One launch for the running statistics and backward vectors of the listed BatchNorms (table built once per
        plan and mode); ``eval_mode``: one launch for their eval-mode (scale, shift) instead."""
        key = tuple((ptr(bn.weight), ptr(bn.running_mean)) for bn, *_ in bn_layers)
        if pl.bn_table[eval_mode][0] != key:
            pl.bn_table[eval_mode] = (key, self._bn_table(bn_layers))
        table, n, channels = pl.bn_table[eval_mode][1]
        if eval_mode:
            _lib.call("msl_bn_eval_affine_batch", ptr(table), n, channels, st, tag="bn_eval_all")
        else:
            _lib.call("msl_bn_finalize_batch", ptr(table), n, channels, st, tag="bn_finalize_all")

    def _pw_bww_batch(self, pl, rows, N, st):
        """msl_pwconv_bwd_weight_slabs for several tail blocks in one launch; rows = (dy, z, scale, shift, out, cin, cout, S)."""
        key = tuple(rows)
        if pl.pwb_key != key:
            n = len(rows)
            P, I = ctypes.c_void_p * n, ctypes.c_int * n
            pl.pwb_args = tuple(P(*[r[c] for r in rows]) for c in range(5)) + tuple(I(*[r[c] for r in rows]) for c in range(5, 8))
            pl.pwb_key = key
        a = pl.pwb_args  # host arrays: kept alive by the plan (a recorded launch program points at them)
        self._k("pw_bww_tail", "msl_pwconv_bwd_weight_slabs_batch", *[ctypes.addressof(x) for x in a], len(rows), N, st)

    def _pack_head_weights(self, pl, st):
        m = self.model
        key = tuple(ptr(c.weight) for c in m.pred_convs.loc_convs) + tuple(ptr(c.weight) for c in m.pred_convs.cl_convs)
        if pl.pack_key != key:
            n = len(pl.feat_ids)
            P = ctypes.c_void_p * n
            pl.pack_args = (P(*[ptr(c.weight) for c in m.pred_convs.loc_convs]), P(*[ptr(c.weight) for c in m.pred_convs.cl_convs]),
                            P(*[ptr(pl.Wf[f]) for f in pl.feat_ids]), P(*[ptr(pl.Wb[f]) for f in pl.feat_ids]),
                            (ctypes.c_int * n)(*[self.layer_specs[f]["cout"] for f in pl.feat_ids]))
            pl.pack_key = key
        a = pl.pack_args  # host arrays: kept alive by the plan (a recorded launch program points at them)
        n = len(pl.feat_ids)
        for g0 in range(0, n, 4):  # the batch entry holds four scales (`--prediction_layers "1 2 3 5 7"`: two launches)
            self._k("head_pack", "msl_head_pack_weights_batch", *[ctypes.addressof(a[c]) + 8 * g0 for c in range(4)],
                    ctypes.addressof(a[4]) + 4 * g0, min(4, n - g0), m.n_classes, st)

    def _head_forward(self, pl, f, st):
        m = self.model
        ncls = m.n_classes
        k = pl.feat_ids.index(f)
        lc, cc = m.pred_convs.loc_convs[k], m.pred_convs.cl_convs[k]
        C = self.layer_specs[f]["cout"]
        D, H, W = pl.dims[f]
        self._k(f"head_fwd{f}", "msl_head_conv_fwd", ptr(pl.fpad[f]), ptr(pl.Wf[f]), ptr(lc.bias), ptr(cc.bias), ptr(pl.locs),
                ptr(pl.scores), ptr(pl.head_ws[f]), pl.N, C, D, H, W, pl.P, pl.prior_off[f], ncls, st)

    def _head_forward_bf16(self, pl, f, st):
        """bf16 inference with ``bf16_heads = "bf16"``: the channels-last bf16 copy of feature map f, this scale's packed
        weights and its head convolution on the bf16 MFMA kernel."""
        m = self.model
        ncls = m.n_classes
        k = pl.feat_ids.index(f)
        lc, cc = m.pred_convs.loc_convs[k], m.pred_convs.cl_convs[k]
        C = self.layer_specs[f]["cout"]
        D, H, W = pl.dims[f]
        self._k(f"materialize{f}", "msl_bn_relu_materialize_bf16", ptr(pl.y[f]), ptr(pl.bn_y[f][0]), ptr(pl.bn_y[f][1]), None,
                ptr(pl.fpad_cl[f]), pl.N, C, D, H, W, st)
        self._k(f"head_pack{f}", "msl_head_pack_weights_bf16", ptr(lc.weight), ptr(cc.weight), ptr(pl.Wp[f]), C, ncls, st)
        self._k(f"head_fwd{f}", "msl_head_conv_fwd_bf16", ptr(pl.fpad_cl[f]), ptr(pl.Wp[f]), ptr(lc.bias), ptr(cc.bias),
                ptr(pl.locs), ptr(pl.scores), pl.N, C, D, H, W, pl.P, pl.prior_off[f], ncls, st)

    # ------------------------------------------------------------------------------------------------
    def _bn_bwd(self, g, y, vec, bn_name, count, N, C, S, pl, st, pre_np=None, apply=True, coef=False, partials=None):
        """In place: g (= dL/d relu(bn(y))) becomes dL/dy; writes dgamma/dbeta into the gradient arena.
        ``pre_np``: the producer of g already emitted the reduce partials (pl.partials, that many per channel);
        ``apply=False``: the consumer applies the BatchNorm backward itself while loading (only c1/c2 are produced)."""
        gv = self.arena.grad_views
        part = pl.partials if partials is None else partials  # (``partials``: where the producer left its pre_np sums)
        if pre_np is not None and coef:
            _lib.call("msl_bn_bwd_finalize_coef", ptr(part), pre_np, float(count), ptr(gv[bn_name + ".weight"]),
                      ptr(gv[bn_name + ".bias"]), ptr(vec), C, st)
            return
        if pre_np is None:  # nobody left the sums
            if bn_bwd_one_launch(False, N, S):  # small per-channel data: reduce + finalize + apply
                self._k("bn_bwd_fused:" + bn_name, "msl_bn_relu_bwd_fused", ptr(g), ptr(y), ptr(vec[0]), ptr(vec[1]),
                        ptr(vec[2]), ptr(vec[3]), ptr(gv[bn_name + ".weight"]), ptr(gv[bn_name + ".bias"]), ptr(g), N, C, S, st)
                return
            pre_np, part, apply = _lib.load().msl_bn_relu_bwd_num_partials(N, S), pl.partials, True
            self._k("bn_bwd_reduce:" + bn_name, "msl_bn_relu_bwd_reduce", ptr(g), ptr(y), ptr(vec[0]), ptr(vec[1]), ptr(vec[2]),
                    ptr(vec[3]), ptr(pl.partials), N, C, S, st)
        if apply and pre_np <= 256:
            self._k("bn_bwd_apply:" + bn_name, "msl_bn_relu_bwd_finalize_apply", ptr(part), pre_np, float(count), ptr(g),
                    ptr(y), ptr(vec), ptr(gv[bn_name + ".weight"]), ptr(gv[bn_name + ".bias"]), ptr(g), N, C, S, st)
            return
        _lib.call("msl_bn_bwd_finalize", ptr(pl.partials), pre_np, float(count), ptr(gv[bn_name + ".weight"]),
                  ptr(gv[bn_name + ".bias"]), ptr(vec[4]), ptr(vec[5]), C, st)
        if apply:
            self._k("bn_bwd_apply:" + bn_name, "msl_bn_relu_bwd_apply", ptr(g), ptr(y), ptr(vec[0]), ptr(vec[1]), ptr(vec[2]),
                    ptr(vec[3]), ptr(vec[4]), ptr(vec[5]), ptr(g), N, C, S, st)

    def _head_gpack_batch(self, pl, dlocs, dscores, st):
        """msl_head_grad_pack of every scale in one launch."""
        key = (ptr(dlocs), ptr(dscores)) + tuple(ptr(pl.dO[f]) for f in pl.feat_ids)
        if pl.gpack_key != key:
            n = len(pl.feat_ids)
            I = ctypes.c_int * n
            pl.gpack_args = ((ctypes.c_void_p * n)(*[ptr(pl.dO[f]) for f in pl.feat_ids]),) + tuple(
                I(*[pl.dims[f][a] for f in pl.feat_ids]) for a in range(3)) + (I(*[pl.prior_off[f] for f in pl.feat_ids]),)
            pl.gpack_key = key
        a = pl.gpack_args  # host arrays: kept alive by the plan (a recorded launch program points at them)
        n = len(pl.feat_ids)
        for g0 in range(0, n, 4):  # four scales per launch (msl_head_grad_pack_batch)
            self._k("head_gpack_all", "msl_head_grad_pack_batch", ptr(dlocs), ptr(dscores), ctypes.addressof(a[0]) + 8 * g0,
                    *[ctypes.addressof(x) + 4 * g0 for x in a[1:]], min(4, n - g0), pl.N, pl.P, self.model.n_classes, st)

    def _head_backward(self, pl, f, dlocs, dscores, st, data_done_event=None, data=True, weight=True, packed=False):
        ncls = self.model.n_classes
        C = self.layer_specs[f]["cout"]
        D, H, W = pl.dims[f]
        if data:
            if not packed:
                self._k(f"head_gpack{f}", "msl_head_grad_pack", ptr(dlocs), ptr(dscores), ptr(pl.dO[f]), pl.N, D, H, W, pl.P,
                        pl.prior_off[f], ncls, st)
            self._k(f"head_bwd{f}", pl.ops["head_bwd"], ptr(pl.dO[f]), ptr(pl.Wb[f]), ptr(pl.g_y[f]), pl.N, C, D, H, W, ncls, st)
            if data_done_event is not None:  # the activation-gradient chain only waits for the data gradient
                _lib.call("msl_event_record", data_done_event, st, tag="event")
        if not weight:
            return
        # weight and bias slabs stay in head_ws[f] (folded by the batched gradient reduction)
        self._k(f"head_bww{f}", "msl_head_conv_bwd_weight", ptr(pl.dO[f]), ptr(pl.fpad[f]), None, None, None, None,
                ptr(pl.head_ws[f]), pl.N, C, D, H, W, ncls, st)

    def _reporter(self, pl, on_bucket_ready, groups, st, stH, stW, ms):
        """-> report(stage, join_heads=True): tell the data-parallel reducer that every launch producing the gradients of
        ``stage`` ('heads', 7, ..., 0) has been enqueued - after making the stream the exchange will run on wait for the
        streams that produced them (the heads stream too, which carries the head gradients and the odd blocks' weight
        gradients) and folding the stage's partial sums there."""
        wanted = getattr(on_bucket_ready, "stages", None)

        def report(stage, join_heads=True):
            if on_bucket_ready is None or (wanted is not None and stage not in wanted):
                return
            comm = getattr(on_bucket_ready, "comm_stream", None)
            if comm is not None and stage == 0 and getattr(on_bucket_ready, "final_on_main", False):
                # every stream has just been joined into the chain: the last bucket is exchanged right here.  Collectives
                # of one communicator must not overlap each other, so the chain first waits for the communication stream
                # (whose buckets were issued ~0.3 ms ago: the wait is normally satisfied on arrival)
                self._fork(pl, "bucket_tail", comm.cuda_stream, st)
            elif comm is not None:
                # the exchange has a stream of its own: IT waits for the streams that produced the bucket, the
                # dependency chain never does (joining the weight-gradient stream into the chain three times per step
                # cost 0.19 ms of a 1.0 ms step: tools/probes/dp_host_cost.py)
                dst = comm.cuda_stream
                self._fork(pl, f"bucket_m{stage}", st, dst)
                if ms:
                    if dst != stW:
                        self._fork(pl, f"bucket_w{stage}", stW, dst)
                    if join_heads and dst != stH:
                        self._fork(pl, f"bucket_h{stage}", stH, dst)
            elif ms:  # the exchange follows the main stream: bring the side streams' work in first
                self._fork(pl, f"bucket_w{stage}", stW, st)
                if join_heads:
                    self._fork(pl, f"bucket_h{stage}", stH, st)
            if stage in groups:  # fold the partial sums of this stage's buckets where their exchange will run
                comm2 = getattr(on_bucket_ready, "comm_stream", None)
                on_main = comm2 is None or (stage == 0 and getattr(on_bucket_ready, "final_on_main", False))
                self._grad_reduce(pl, stage, groups[stage], st if on_main else comm2.cuda_stream)
            # the waits above are part of the launch program; the reducer must not repeat them at the torch level - told per
            # call (eager and replayed alike), never through state that outlives the call (a flag left set
            # by an fp32 step made a later bf16 step on the same reducer skip its wait)
            presync = comm is not None and hasattr(on_bucket_ready, "presynced")

            def fire(tag, presync=presync):
                if presync:
                    on_bucket_ready.presynced = True
                try:
                    on_bucket_ready(tag)
                finally:
                    if presync:
                        on_bucket_ready.presynced = False
            if getattr(on_bucket_ready, "native", False):
                on_bucket_ready(stage)  # issues C-ABI calls itself (recorded like any other launch): no Python hook
            else:
                self._hook(fire, stage)
        return report

    def _backward_open(self, pl, dlocs, dscores, on_bucket_ready):
        """What both backward passes do before the first head gradient -> (chain, heads and wgrad stream - the chain three
        times for a one-stream pass -, contiguous dlocs / dscores, the reducer's stages, groups, report, index of the last
        block, the scales whose gradients run on the heads stream, whether the head-gradient images are already packed)."""
        st = self._stream()
        ms = self.multi_stream
        stH, stW = (s.cuda_stream for s in self.side_streams(pl.locs.device)) if ms else (st, st)
        prepacked = dlocs is None  # the loss kernel wrote the head-gradient images itself (MultiBoxLoss._run_loss_pack)
        if not prepacked:
            dlocs, dscores = dlocs.contiguous(), dscores.contiguous()
        last = len(self.layer_specs) - 1
        if last not in pl.feat_ids:
            raise RuntimeError("the last backbone feature must feed a head")
        wanted = getattr(on_bucket_ready, "stages", None)
        # data parallel: the partial sums of a gradient bucket are folded when the bucket's last stage has been enqueued
        # (stage -> parameter names); single process: one reduction at the very end
        groups = self._bucket_groups(on_bucket_ready) if wanted else {}
        report = self._reporter(pl, on_bucket_ready, groups, st, stH, stW, ms)
        side_feats = [f for f in pl.feat_ids if f != last] if ms else []
        packed = prepacked or (bool(side_feats) and self.batch_head_gpack)
        if packed and not prepacked:
            self._head_gpack_batch(pl, dlocs, dscores, st)
        if side_feats:
            # the earlier scales' gradients (heads stream) need the head-gradient images - written by the launch in front
            # of this point (the loss kernel, or the batched pack), whose stop event this record becomes: no packet on the
            # chain, and the heads stream starts one launch earlier than behind the chain's own head bwd-data (which was
            # measured 1-2 % slower: the heads stream's gradients are as critical as the chain here)
            self._fork(pl, "bwd_loss_ready", st, stH)
        return st, stH, stW, dlocs, dscores, wanted, groups, report, last, side_feats, packed

    def _backward_close(self, pl, groups, report, st, stH, stW):
        if self.multi_stream:  # every gradient is complete once the side streams have been joined
            self._fork(pl, "bwd_join_w", stW, st)
            self._fork(pl, "bwd_join_h", stH, st)
        if not groups:  # single process: ONE reduction launch for every layer's partial sums, right in front of the optimiser
            self._grad_reduce(pl, "all", None, st)
        report(0, join_heads=False)

    # -- backward emitters: one layer launch each, for both storage types (entry points: ``pl.ops``, forms: ``pl.routes``) ---
    def _bn_backward(self, pl, kind, i, st):
        """BatchNorm backward of y[i] ("y") or z[i] ("z") of block i, in place, by the driver of the plan's storage type -
        from the reduce sums another launch left, where the route says so."""
        sp, r, N = self.layer_specs[i], pl.routes[i], pl.N
        D, H, W = pl.dims[i]
        S = D * H * W
        if kind == "y":
            g, t, vec, C, name, pre_np, part = pl.g_y[i], pl.y[i], pl.bn_y[i], sp["cout"], f"base.features.{i}.bn2", r.y_np, None
        else:  # ("pw_fused", fp32: the one-pass pointwise backward left the sums of z[i] in its own buffer)
            _, part, pre_np = pl.pw_fused[i] if r.bn2 == "pw_fused" else (None, None, None)
            g, t, vec, C, name = pl.g_z[i], pl.z[i], pl.bn_z[i], sp["cin"], f"base.features.{i}.bn1"
        if pl.bf16:
            self._bn_bwd_bf16(g, t, vec, name, N, C, S, pl, st, pre_np=pre_np)
        else:
            self._bn_bwd(g, t, vec, name, N * S, N, C, S, pl, st, pre_np=pre_np, partials=part)

    def _pw_backward(self, pl, i, st):
        """dL/dy_i -> dL/d relu(bn1(z_i)) in g_z[i]: BatchNorm2 backward where it is still to do (``Route.bn2``), then the
        pointwise bwd-data GEMM."""
        blk, sp, r, N = self.model.base.features[i], self.layer_specs[i], pl.routes[i], pl.N
        D, H, W = pl.dims[i]
        S = D * H * W
        if r.bn2 == "pw_fused":
            # BatchNorm backward of y_i (applied on load), bwd-data GEMM, BatchNorm1-backward sums of z_i and the pointwise
            # weight gradient in ONE pass (csrc/pwfused.hip)
            gv, name = self.arena.grad_views, f"base.features.{i}.bn2"
            slabs_f, part_f, _ = pl.pw_fused[i]
            self._k(f"pw_bwd_fused{i}", pl.ops["pw_bwd_fused"], ptr(pl.g_y[i]), ptr(pl.y[i]), ptr(pl.bn_y[i]), ptr(pl.partials),
                    r.y_np, float(N * S), ptr(gv[name + ".weight"]), ptr(gv[name + ".bias"]), ptr(blk.conv2.weight),
                    ptr(pl.z[i]), ptr(pl.bn_z[i]), ptr(pl.g_z[i]), ptr(part_f), ptr(slabs_f), N, sp["cin"], sp["cout"], S, st)
            return
        if r.bn2 == "bn":  # ("link": the channel link of block i+1 has already turned g_y[i] into dL/dy_i)
            self._bn_backward(pl, "y", i, st)
        self._k(f"pw_bwd{i}", pl.ops["pw_bwd"], ptr(pl.g_y[i]), ptr(blk.conv2.weight), ptr(pl.g_z[i]), N, sp["cin"], sp["cout"],
                S, st)

    def _channel_link(self, pl, i, accumulate, st):
        """Tail block: BatchNorm1 backward of z_i, depthwise bwd-data (+ the heads' share of g_y[i-1]: ``accumulate``) and
        BatchNorm2 backward of y_{i-1} in one launch; "link_bww": the depthwise weight gradient too."""
        sp, gv = self.layer_specs[i], self.arena.grad_views
        name, prev = f"base.features.{i}", "base.features.0.1" if i == 1 else f"base.features.{i - 1}.bn2"
        self._k(f"link{i}", pl.ops["link"], ptr(pl.g_z[i]), ptr(pl.z[i]), ptr(pl.bn_z[i]),
                ptr(self.model.base.features[i].conv1.weight), ptr(pl.y[i - 1]), ptr(pl.bn_y[i - 1]), ptr(pl.g_y[i - 1]),
                ptr(gv[name + ".bn1.weight"]), ptr(gv[name + ".bn1.bias"]), ptr(gv[prev + ".weight"]), ptr(gv[prev + ".bias"]),
                ptr(gv[name + ".conv1.weight"]) if pl.routes[i].dw == "link_bww" else None, pl.N, sp["cin"], *pl.dims[i - 1],
                sp["stride"][0], accumulate, st)

    def _dw_backward(self, pl, i, accumulate, st):
        """Depthwise bwd-data of block i in the form of ``Route.dw`` (a block without a channel link): dL/dz_i -> g_y[i-1]."""
        sp, dw, N = self.layer_specs[i], pl.routes[i].dw, pl.N
        g, w, y = ptr(pl.g_z[i]), ptr(self.model.base.features[i].conv1.weight), ptr(pl.y[i - 1])
        dims, s = pl.dims[i - 1], sp["stride"][0]
        # the BatchNorm of y_{i-1}, for the forms that need it: the vectors one by one (fp32) or their buffer (bf16)
        vec = () if dw == "plain" else (ptr(pl.bn_y[i - 1]),) if pl.bf16 else tuple(ptr(pl.bn_y[i - 1][k]) for k in range(4))
        if dw == "fused_stem":
            # one pass over (dL/dz_1, y_0): BatchNorm-backward sums of the stem + the depthwise weight gradient; the stem
            # weight gradient rebuilds dL/d(stem activation) from dL/dz_1 on the fly
            args = (g, w, y, *vec, ptr(pl.partials), ptr(pl.partials_wf), ptr(pl.w1_taps_t), N, 32, *dims)
        elif dw == "s2_bww":
            # big stride-2 producer layer: bwd-data, the BatchNorm-backward sums of y_{i-1} AND this block's depthwise
            # weight gradient in one pass over (dL/dz_i, y_{i-1}) - the weight-gradient launch on the side stream (the same
            # 38 MB read again, 35 us beside the chain at block 2) disappears
            args = (g, w, ptr(pl.g_y[i - 1]), y, *vec, ptr(pl.partials), ptr(pl.routes[i].dw_part[0]), N, sp["cin"], *dims,
                    accumulate)
        elif dw == "bnreduce":
            # big producer layer: emit the BatchNorm-backward partials of y_{i-1} while its gradient is in registers
            args = (g, w, ptr(pl.g_y[i - 1]), y, *vec, ptr(pl.partials), N, sp["cin"], *dims, s, accumulate)
        elif dw == "s2_patch":  # (the same, stride 2)
            args = (g, w, ptr(pl.g_y[i - 1]), y, *vec, ptr(pl.partials), N, sp["cin"], *dims, accumulate)
        else:
            assert dw == "plain", dw
            args = (g, w, ptr(pl.g_y[i - 1]), N, sp["cin"], *dims, s, accumulate)
        self._k(f"dw_bwd{i}", pl.ops["dw_bwd:" + dw], *args, st)

    def _pw_wgrad_row(self, pl, i):
        """(dL/dy_i, z_i, scale and shift of its BatchNorm, destination, Cin, Cout, S) of block i's pointwise weight gradient:
        partial sums only - slabs stay in this layer's own buffer until Engine._grad_reduce."""
        sp, r = self.layer_specs[i], pl.routes[i]
        D, H, W = pl.dims[i]
        out = r.pw_part[0] if r.pw_part is not None else self.arena.grad_views[f"base.features.{i}.conv2.weight"]
        return ptr(pl.g_y[i]), ptr(pl.z[i]), ptr(pl.bn_z[i][0]), ptr(pl.bn_z[i][1]), ptr(out), sp["cin"], sp["cout"], D * H * W

    def _pw_wgrad(self, pl, i, st):
        row = self._pw_wgrad_row(pl, i)
        self._k(f"pw_bww{i}", pl.ops["pw_bww"], *row[:5], pl.N, *row[5:], st)

    def _dw_wgrad(self, pl, i, st):
        """Block i's depthwise weight gradient (fp64 partials for Engine._grad_reduce), where no other pass sums it: else its
        partials came with the depthwise backward pass (``Route.dw_part``) or the link wrote dW."""
        if pl.routes[i].dw not in DW_BWW:
            return
        sp = self.layer_specs[i]
        dst = (ptr(pl.dw_part[i]),) if pl.bf16 else (None, ptr(pl.dw_part[i]))  # (fp32: an unused slot in front)
        self._k(f"dw_bww{i}", pl.ops["dw_bww"], ptr(pl.g_z[i]), ptr(pl.y[i - 1]), ptr(pl.bn_y[i - 1][0]), ptr(pl.bn_y[i - 1][1]),
                *dst, pl.N, sp["cin"], *pl.dims[i - 1], sp["stride"][0], st)

    def _stem_backward(self, pl, st):
        """The stem's tail of the backward pass: its BatchNorm backward as far as ``StemRoute`` leaves it to do, then the
        weight gradient in the form of ``StemRoute.wgrad``."""
        sp, r, N, gv = self.layer_specs[0], pl.routes[0], pl.N, self.arena.grad_views
        od, oh, ow = pl.dims[0]
        S0, vec = od * oh * ow, pl.bn_y[0]
        if pl.bf16:  # BatchNorm-backward sums (unless block 1's depthwise form left them), then the coefficients
            NP = r.y_np
            if NP is None:
                NP = _lib.load().msl_bn_relu_bwd_bf16_num_partials(N, S0)
                self._k("bn_bwd_reduce:stem", "msl_bn_relu_bwd_reduce_bf16", ptr(pl.g_y[0]), ptr(pl.y[0]), ptr(vec[0]), ptr(vec[1]),
                        ptr(vec[2]), ptr(vec[3]), ptr(pl.partials), N, sp["cout"], S0, st)
            bn = ("base.features.0.1.weight", "base.features.0.1.bias")
            if r.wgrad == "fused":
                _lib.call("msl_bn_bwd_finalize_coef", ptr(pl.partials), NP, float(N * S0), ptr(gv[bn[0]]), ptr(gv[bn[1]]),
                          ptr(vec), sp["cout"], st)
            else:
                _lib.call("msl_bn_bwd_finalize", ptr(pl.partials), NP, float(N * S0), ptr(gv[bn[0]]), ptr(gv[bn[1]]),
                          ptr(vec[4]), ptr(vec[5]), sp["cout"], st)
        elif r.bn == "bn":  # ("link", tiny inputs: block 1's channel link has already applied the stem's BatchNorm backward)
            # "bnapply" / "fused": the reduce came with the depthwise bwd-data, the apply is part of the weight gradient
            self._bn_bwd(pl.g_y[0], pl.y[0], vec, "base.features.0.1", N * S0, N, sp["cout"], S0, pl, st, pre_np=r.y_np,
                         apply=r.wgrad == "plain", coef=r.wgrad == "fused")
        if r.wgrad == "fused":  # rebuilt from dL/dz_1, on the coefficients of msl_bn_bwd_finalize_coef
            src = (ptr(pl.g_z[1]), ptr(pl.w1_taps_t), ptr(pl.y[0]), ptr(vec))
        elif r.wgrad == "bnapply":  # the BatchNorm backward applied on load
            src = (ptr(pl.g_y[0]), ptr(pl.y[0]), ptr(vec))
        else:
            src = (ptr(pl.g_y[0]),)
        self._k("stem_bww", pl.ops["stem_bww:" + r.wgrad], *src, ptr(pl.saved_input), None, ptr(pl.ws_stem), N, sp["cin"],
                *pl.in_dims, *sp["stride"], st)

    def backward(self, pl, dlocs, dscores, on_bucket_ready=None):
        """Given dL/dlocs, dL/dscores, fill the flat gradient arena.  ``on_bucket_ready(stage)`` is called right
        after the launches that complete a gradient stage ('heads', 7, ..., 0) have been enqueued; if it has a
        ``stages`` attribute only those stages are reported (and the side streams are joined first)."""
        if not pl.need_grad or not pl.trained_mode:
            raise RuntimeError("backward needs a train-mode forward made with gradients enabled")
        if pl.bf16:
            return self._backward_bf16(pl, dlocs, dscores, on_bucket_ready)
        # (the bf16 step: _backward_bf16, which says how its schedule differs from this one)
        specs, N, ms = self.layer_specs, pl.N, self.multi_stream
        st, stH, stW, dlocs, dscores, wanted, groups, report, last, side_feats, packed = self._backward_open(
            pl, dlocs, dscores, on_bucket_ready)
        L = _lib.load()
        pending = []  # side-stream launches, issued one layer late so that the chain's launches always go first
        sinks = []    # (closure, event) of the weight-gradient launches still to be issued
        tail = []     # blocks whose pointwise weight gradients share one launch (deepest first), and their arguments
        if ms and not groups and self.batch_tail_pw:
            for i in range(last, 0, -1):
                D_, H_, W_ = pl.dims[i]
                if N * D_ * H_ * W_ <= 4096 and L.msl_pwconv_bwd_weight_batchable(N, specs[i]["cin"], specs[i]["cout"], D_ * H_ * W_) == 1:
                    tail.append(i)
            tail = tail[:4] if len(tail) >= 2 else []
        tail_args = []
        # heads: the last scale feeds the chain immediately (main stream); the earlier scales are only needed when
        # the chain reaches their feature map, so they run on the heads stream beside blocks 7..4
        for f in pl.feat_ids:  # the chain's own scale first: its data gradient starts the backward chain
            if f not in side_feats:
                if ms:
                    self._head_backward(pl, f, dlocs, dscores, st, weight=False, packed=packed)
                    ev = self._record(pl, f"head_dO{f}", st)
                    pending.append(lambda f=f, ev=ev: (self._wait(stW, ev),
                                                       self._head_backward(pl, f, dlocs, dscores, stW, data=False)))
                else:
                    self._head_backward(pl, f, dlocs, dscores, st, packed=packed)
        for f in reversed(side_feats):  # the deeper scale is needed first
            pending.append(lambda f=f: self._head_backward(pl, f, dlocs, dscores, stH, self._event(pl, f"head_done{f}"), packed=packed))
        if wanted is not None and "heads" in wanted:
            for fn in pending:
                fn()
            pending = []
        report("heads")
        for i in range(last, 0, -1):
            # y_i = pw(relu(bn1(z_i))): BN2 backward, then the two GEMMs; z_i = dw(relu(bn(y_{i-1}))): BN1 backward,
            # then the depthwise gradients.  The host enqueues the dependency chain (main stream) FIRST and the two
            # weight gradients (wgrad stream, waiting on events recorded in the chain) afterwards: the chain is made of
            # ~10 us kernels, so any launch queued in front of its next link shows up as idle time.
            r = pl.routes[i]
            pw_fused, link = r.bn2 == "pw_fused", r.dw in ("link", "link_bww")
            self._pw_backward(pl, i, st)
            accumulate = 1 if (i - 1) in pl.fpad else 0  # the heads already wrote their share
            # a block whose pointwise weight gradient rides in the tail's batched launch (issued with the shallowest of them) and
            # whose depthwise weight gradient the link produces has nothing waiting for dL/dz_i: no event record on the chain
            idle_sink = (r.dw == "link_bww" and i in tail and i != tail[-1]) or (pw_fused and r.dw == "fused_stem")
            rec_here = ms and not idle_sink
            if not link:
                self._bn_backward(pl, "z", i, st)
                ev_dz = self._record(pl, f"dz{i}", st) if rec_here else None
            if accumulate and (i - 1) in side_feats:
                self._wait(st, pl.events[f"head_done{i - 1}"])
            if link:
                self._channel_link(pl, i, accumulate, st)
                ev_dz = self._record(pl, f"dz{i}", st) if rec_here else None
            else:
                self._dw_backward(pl, i, accumulate, st)

            def wgrads(ev_dz, i=i, idle_sink=idle_sink, pw_fused=pw_fused):
                # the heads stream is idle once the head gradients are done: odd blocks go there, even ones to the wgrad stream
                sX = (stH if i % 2 else stW) if ms else st
                if ms and not idle_sink:  # the pointwise gradient needs dL/dy_i, the depthwise one dL/dz_i (final later)
                    self._wait(sX, ev_dz)
                if i in tail and not pw_fused:  # (pw_fused: its slabs came with the fused pointwise backward)
                    tail_args.append(self._pw_wgrad_row(pl, i))
                    if i == tail[-1]:  # the shallowest: every dL/dy of the group is final (same chain, earlier)
                        self._pw_bww_batch(pl, tail_args, N, sX)
                elif not pw_fused:
                    self._pw_wgrad(pl, i, sX)
                self._dw_wgrad(pl, i, sX)

            # issue what earlier layers left for the side streams (the head gradients the chain waits for and the weight
            # gradients, which nothing in the step waits for: one layer late), then queue this layer's
            for fn in pending:
                fn()
            pending = []
            if ms:
                for fn, e in sinks:
                    fn(e)
                sinks = [(wgrads, ev_dz)]
            else:
                wgrads(None)
            if wanted is not None and i in wanted:
                for fn, e in sinks:
                    fn(e)
                sinks = []
            report(i)
        self._stem_backward(pl, st)
        for fn in pending:
            fn()
        for fn, e in sinks:
            fn(e)
        self._backward_close(pl, groups, report, st, stH, stW)

    def _bucket_groups(self, reducer):
        """stage -> set of parameter names whose gradient bucket completes at that stage (GradBucketReducer layout)."""
        groups = {}
        for stage, buckets in reducer.trigger.items():
            names = set()
            for k in buckets:
                lo, hi = reducer.ranges[k]
                names |= {n for n, (off, cnt) in self.arena.offsets.items() if n not in self.arena.no_grad_names and lo <= off < hi}
            groups[stage] = names
        return groups

    def _grad_reduce(self, pl, key, names, st):
        """One launch that folds the partial weight-gradient sums (pointwise slabs, depthwise fp64 partials, head and stem
        slabs) of the parameters in ``names`` (None: all) into the gradient arena (table built once per plan and key)."""
        L = _lib.load()
        fold = pl.loss_fold
        tkey = (key, None if fold is None else ptr(fold[0]))
        ent = pl.grad_tables.get(tkey)
        if ent is None:
            gv = self.arena.grad_views
            specs, m = self.layer_specs, self.model
            ncls = m.n_classes
            rows = []  # (kind, src, dst, dst2, nslabs, count, stride, p0, p1, p2)
            want = lambda n: names is None or n in names
            for k, f in enumerate(pl.feat_ids):
                lw, cw = f"pred_convs.loc_convs.{k}.weight", f"pred_convs.cl_convs.{k}.weight"
                if want(lw) or want(cw):
                    if not (want(lw) and want(cw)):
                        raise RuntimeError("a gradient bucket boundary separates the two head convolutions of one scale")
                    C = specs[f]["cout"]
                    mt = (12 + 2 * ncls + 15) // 16
                    slab = (C // 16) * 27 * mt * 256
                    ns = pl.head_nslabs[f]
                    rows.append((3, pl.head_ws[f], gv[lw], gv[cw], ns, slab, slab, C, mt, 12 + 2 * ncls))
                    bias = pl.head_ws[f][ns * slab:]  # [ns][16*mt] row sums of dO: rows 0-11 loc, 12.. cls
                    rows.append((0, bias, gv[lw[:-6] + "bias"], None, ns, 12, 16 * mt, 0, 0, 0))
                    rows.append((0, bias[12:], gv[cw[:-6] + "bias"], None, ns, 2 * ncls, 16 * mt, 0, 0, 0))
            for i in range(len(specs) - 1, 0, -1):  # (a gradient without partials was written to the arena by its kernel)
                name, r = f"base.features.{i}", pl.routes[i]
                cnt = specs[i]["cin"] * specs[i]["cout"]
                if want(name + ".conv2.weight") and r.pw_part is not None:
                    rows.append((0, r.pw_part[0], gv[name + ".conv2.weight"], None, r.pw_part[1], cnt, cnt, 0, 0, 0))
                if want(name + ".conv1.weight") and r.dw_part is not None:
                    rows.append((1, r.dw_part[0], gv[name + ".conv1.weight"], None, r.dw_part[1], specs[i]["cin"] * 27, 0, 0, 0, 0))
            if want("base.features.0.0.weight"):
                K = specs[0]["cin"] * 27
                nt = (K + 31) // 32
                rows.append((2, pl.ws_stem, gv["base.features.0.0.weight"], None, pl.stem_nslabs, 1024 * nt, 1024 * nt, K, nt, 0))
            if fold is not None and key in ("all", 0):  # the loss values of MultiBoxLoss._run_loss_pack ride along (kind 4)
                parts, nparts, loss_out, npos = fold
                rows.append((4, parts, loss_out, npos, nparts, 1, 0, 0, 0, 0))
            esz = L.msl_grad_reduce_entry_bytes()
            host = (ctypes.c_ubyte * (esz * max(len(rows), 1)))()
            first = 0
            owner = []  # table entry of every workgroup
            for k, (kind, src, dst, dst2, ns, cnt, stride, p0, p1, p2) in enumerate(rows):
                nb = L.msl_grad_reduce_table_set(ctypes.addressof(host), k, first, kind, ptr(src), ptr(dst), ptr(dst2), ns, cnt,
                                                 stride, p0, p1, p2)
                if nb < 0:
                    raise _lib.HipKernelError(f"msl_grad_reduce_table_set failed for entry {k} (kind {kind})")
                first += nb
                owner += [k] * nb
            dev = self.arena.grad.device
            table = torch.frombuffer(bytearray(host), dtype=torch.uint8).to(dev) if rows else None
            ent = pl.grad_tables[tkey] = (table, len(rows), first, torch.tensor(owner, dtype=torch.int32, device=dev))
        table, n, blocks, owner = ent
        if n:
            self._k(f"grad_reduce:{key}", "msl_grad_reduce_batch_indexed", ptr(table), n, ptr(owner), blocks, st)

    def check_nan(self, pl):
        """One host sync: raise like ssd3d.py:258-261 if the forward produced NaN."""
        self.raise_on_nan_flag(int(pl.nan_flag.item()))

    @staticmethod
    def raise_on_nan_flag(flag):
        if flag & 2:
            raise Exception("Oh no not this NaN error again... (forward SSD), CLASSES_SCORES is nan!")
        if flag & 1:
            raise Exception("Oh no not this NaN error again... (forward SSD), LOCS is nan!")
