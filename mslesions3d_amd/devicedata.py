"""Device-resident training data (``train.py -c 1``; the reference's ``-c/--cache``, MONAI ``CacheDataset``): the cases
are loaded and normalised ONCE into HBM, and every batch is gathered, augmented, labelled into boxes and packed into
``FusedTrainer.step_packed``'s target layout on the device (csrc/datapipe.hip).  Host mirror: ``datasets._Cases`` and
``datasets.boxes_from_segmentation``; the per-sample random draws are the host's own (``datasets.draw_augmentations``
on ``datasets.sample_rng``), so a batch holds the same subjects, the same masks and bit-identical boxes as the host
loader's, and images within the normalisation bound of DESIGN.md §4.7.

Limits: rot90 on an axis pair of unequal sizes (a shape-changing rotation) raises NotImplementedError, and so does a
flip / rot90 placed after an affine stage (the reference's order puts them first).
"""
import numpy as np
import torch
from os.path import join as pjoin

from . import _lib
from ._lib import ptr
from .datasets import ShardSampler, _load, affine_offset, draw_augmentations, sample_rng

PARAM_STRIDE = 16  # f64 per sample of msl_augment_resample


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


class _BoxOut:
    """Packed targets + workspace of msl_seg_boxes for one (N, D, H, W, n_classes, capacity)."""

    def __init__(self, N, shape, n_classes, capacity, comp_cap, dev):
        lib = _lib.load()
        self.N, self.shape, self.n_classes, self.capacity, self.comp_cap = N, tuple(shape), n_classes, capacity, comp_cap
        nbytes = lib.msl_seg_boxes_workspace_bytes(N, *self.shape, n_classes, comp_cap)
        if nbytes == 0:
            raise _lib.HipKernelError(f"msl_seg_boxes: unsupported sizes N={N} shape={self.shape} n_classes={n_classes}")
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.gb = torch.zeros((max(capacity, 1), 6), dtype=torch.float32, device=dev)
        self.gl = torch.ones(max(capacity, 1), dtype=torch.int64, device=dev)
        self.obj_off = torch.zeros(N + 1, dtype=torch.int32, device=dev)
        self.flag = torch.zeros(1, dtype=torch.int32, device=dev)
        self.flag_host = torch.zeros(1, dtype=torch.int32, pin_memory=True)

    def launch(self, seg, stream):
        _lib.call("msl_seg_boxes", ptr(seg), self.N, *self.shape, self.n_classes, self.capacity, self.comp_cap,
                  ptr(self.ws), self.ws.numel(), ptr(self.gb), ptr(self.gl), ptr(self.obj_off), ptr(self.flag), stream)
        self.flag_host.copy_(self.flag, non_blocking=True)  # read after the next synchronising read: no sync of its own

    def raise_on_overflow(self, flag=None):
        f = int(self.flag_host.item() if flag is None else flag)
        if f & 1:
            raise _lib.HipKernelError(f"msl_seg_boxes: a batch holds more ground-truth boxes than the capacity of "
                                      f"{self.capacity} rows")
        if f & 2:
            raise _lib.HipKernelError(f"msl_seg_boxes: a batch holds more connected components than comp_cap = "
                                      f"{self.comp_cap}")


def _default_comp_cap(capacity):
    return max(65536, 4 * capacity)


def boxes_from_segmentation_device(seg, n_classes=1, capacity=None, comp_cap=None):
    """``datasets.boxes_from_segmentation`` for every image of a device uint8 (N, 1, D, H, W) or (N, D, H, W) mask.

    -> (boxes list[(n_i, 6) f32], labels list[(n_i,) i64], (gb, gl, obj_off, capacity)): the per-image lists the host
    function returns (device views) and the packed form ``msl_multibox_match`` reads.  Default capacity: 1024 rows per
    image.  More boxes than the capacity raise HipKernelError.  One host synchronisation (obj_off)."""
    if not seg.is_cuda or seg.dtype != torch.uint8:
        raise _lib.HipKernelError("boxes_from_segmentation_device takes a uint8 tensor on the HIP device")
    if seg.dim() == 5:
        if seg.shape[1] != 1:
            raise ValueError(f"one mask channel expected, got {seg.shape[1]}")
        seg = seg[:, 0]
    if seg.dim() != 4:
        raise ValueError(f"(N, 1, D, H, W) or (N, D, H, W) expected, got {tuple(seg.shape)}")
    seg = seg.contiguous()
    N = seg.shape[0]
    capacity = 1024 * N if capacity is None else int(capacity)
    out = _BoxOut(N, seg.shape[1:], int(n_classes), capacity, comp_cap or _default_comp_cap(capacity), seg.device)
    out.launch(seg, _stream(seg.device))
    off = out.obj_off.cpu().tolist()
    out.raise_on_overflow(out.flag.item())
    boxes = [out.gb[off[n]:off[n + 1]] for n in range(N)]
    labels = [out.gl[off[n]:off[n + 1]] for n in range(N)]
    return boxes, labels, (out.gb, out.gl, out.obj_off, capacity)


def sample_params(draws, shape):
    """One sample's draws (``datasets.draw_augmentations``) -> (signed axis permutation, [affine stages]).

    The permutation is (axis, rev): output axis a reads source axis axis[a], reversed iff rev[a]; it composes the flips
    and rot90s exactly as np.flip / np.rot90 index.  Each affine stage is None (not drawn) or (zoom, offset) in f64."""
    axis, rev = [0, 1, 2], [0, 0, 0]
    stages = []

    def swap(a, b):
        axis[a], axis[b] = axis[b], axis[a]
        rev[a], rev[b] = rev[b], rev[a]

    for name, d in draws:
        if name == "affine":
            stages.append(None if d is None else (list(d[0]), list(affine_offset(shape, *d))))
            continue
        if stages:
            raise NotImplementedError("device pipeline: a flip / rot90 after an affine stage")
        if d is None:
            continue
        if name == "flip":
            for a in d:
                rev[a] ^= 1
        else:  # np.rot90(m, k, (a, b)): k=1 transpose(flip(m, b)), k=2 flip both, k=3 flip(transpose(m), b)
            k, (a, b) = d[0] % 4, d[1]
            if shape[a] != shape[b]:
                raise NotImplementedError(f"device pipeline: rot90 over axes {(a, b)} of sizes {shape[a]} != {shape[b]}")
            if k == 1:
                rev[b] ^= 1
                swap(a, b)
            elif k == 2:
                rev[a] ^= 1
                rev[b] ^= 1
            elif k == 3:
                swap(a, b)
                rev[b] ^= 1
    return (axis, rev), stages


def train_batch_order(dataset, epoch):
    """The index chunks of ``dataset.train_dataloader()`` in ``epoch``: ShardSampler order of this rank, batch_size
    chunks, the last one short (drop_last=False)."""
    sampler = ShardSampler(len(dataset.train_dataset), dataset.rank, dataset.world_size, True, dataset.random_state)
    sampler.set_epoch(epoch)
    order = sampler.indices().tolist()
    return [order[i:i + dataset.batch_size] for i in range(0, len(order), dataset.batch_size)]


def permute_numpy(vol, perm):
    """Host form of the kernel's gather: out[q] = vol[s] with s[axis[a]] = rev[a] ? n - 1 - q[a] : q[a]."""
    axis, rev = perm
    out = np.transpose(vol, axis)  # out axis a <- source axis axis[a]
    flip = tuple(a for a in range(3) if rev[a])
    return np.flip(out, flip) if flip else out


class DeviceCache:
    """The cases of a ``setup()`` ``ExampleDataset`` in HBM (image f32 normalised, mask u8), and the device pipeline that
    turns them into training / validation batches.

    ``train_batches(epoch)`` yields the batches of ``dataset.train_dataloader()`` for that epoch (same ShardSampler order,
    same chunks, same per-sample draws) as dicts {"img", "seg", "gb", "gl", "obj_off", "capacity", "subject"}: the
    tensors are FIXED buffers, one set per batch shape, rewritten by the next batch.  Feed them to ``step(trainer, batch)``
    (``FusedTrainer.step_packed(..., resident=True)`` with total_objects = capacity: one recorded launch program per
    shape).  ``val_batches()`` yields ``validation_step`` batches of this rank's validation shard, without augmentation."""

    def __init__(self, dataset, device, max_objects_per_image=64, comp_cap=None):
        if dataset.train_dataset is None:
            raise ValueError("DeviceCache needs a dataset after setup()")
        self.dataset, self.device = dataset, torch.device(device)
        self.n_classes, self.batch_size = int(dataset.n_classes), int(dataset.batch_size)
        self.augmentations = list(dataset.train_dataset.augmentations)
        tr, te = dataset.train_dataset, dataset.test_dataset
        if dataset.world_size > 1:
            val_idx = ShardSampler(len(te), dataset.rank, dataset.world_size, False, dataset.random_state).indices()
        else:
            val_idx = np.arange(len(te))
        # every rank may draw any training case in a later epoch; validation shards are fixed
        keys = [(tr.root, s) for s in tr.subjects] + [(te.root, te.subjects[i]) for i in val_idx]
        self.slot = {}
        for k in keys:
            self.slot.setdefault(k, len(self.slot))
        self.train_slots = [self.slot[(tr.root, s)] for s in tr.subjects]
        self.val_order = [(te.subjects[i], self.slot[(te.root, te.subjects[i])]) for i in val_idx]
        cases = list(self.slot)
        first = _load(pjoin(cases[0][0], "images", f"sub-{cases[0][1]}_image"))
        self.shape = tuple(first.shape)
        if len(self.shape) != 3:
            raise ValueError(f"DeviceCache: 3-D volumes expected, got shape {self.shape}")
        V = int(np.prod(self.shape))
        self.cache_bytes = len(cases) * V * 5
        free, _ = torch.cuda.mem_get_info(self.device)
        if self.cache_bytes > 0.8 * free:
            raise MemoryError(f"DeviceCache: {len(cases)} cases of {self.shape} need {self.cache_bytes / 2**30:.2f} GiB, "
                              f"{free / 2**30:.2f} GiB free on {self.device}")
        self.img = torch.empty((len(cases),) + self.shape, dtype=torch.float32, device=self.device)
        self.seg = torch.empty((len(cases),) + self.shape, dtype=torch.uint8, device=self.device)
        for k, (root, s) in enumerate(cases):
            img = _load(pjoin(root, "images", f"sub-{s}_image")).astype(np.float32)
            seg = np.asarray(_load(pjoin(root, "labels", f"sub-{s}_seg")))
            if img.shape != self.shape or seg.shape != self.shape:
                raise ValueError(f"DeviceCache: case {s} has shape {img.shape} / {seg.shape}, the first case "
                                 f"{self.shape}: every cached case must have the same shape")
            seg8 = seg.astype(np.uint8)
            if not np.array_equal(seg8, seg):
                raise ValueError(f"DeviceCache: mask of case {s} is not integer-valued in [0, 255]")
            self.img[k].copy_(torch.from_numpy(img))
            self.seg[k].copy_(torch.from_numpy(seg8))
        _lib.call("msl_normalize_nonzero", ptr(self.img), len(cases), V, _stream(self.device))
        self.capacity = int(max_objects_per_image) * self.batch_size
        self.comp_cap = comp_cap or _default_comp_cap(self.capacity)
        self._bufs = {}
        for name, kw in ((t, {}) if isinstance(t, str) else t for t in self.augmentations):
            if name == "rotate90":
                a, b = kw.get("spatial_axes", (0, 1))
                if self.shape[a] != self.shape[b]:
                    raise NotImplementedError(f"device pipeline: rot90 over axes {(a, b)} of sizes "
                                              f"{self.shape[a]} != {self.shape[b]} changes the volume's shape")
        self.n_affine = sum(1 for t in self.augmentations if (t if isinstance(t, str) else t[0]) == "affine")

    # ---- footprint ----------------------------------------------------------------------------------------------------
    def nbytes(self):
        """Device bytes held: the cached cases plus every batch buffer set allocated so far."""
        n = self.cache_bytes
        for b in self._bufs.values():
            n += sum(t.numel() * t.element_size() for t in (b["img"], b["seg"], *b["tmp"], b["box"].ws, b["box"].gb,
                                                             b["box"].gl))
        return n

    def footprint(self):
        return (f"DeviceCache: {self.img.shape[0]} cases of {self.shape} on {self.device}: "
                f"{self.cache_bytes / 2**20:.1f} MiB cached, {self.nbytes() / 2**20:.1f} MiB with batch buffers")

    # ---- the pipeline -------------------------------------------------------------------------------------------------
    def _buffers(self, N):
        b = self._bufs.get(N)
        if b is None:
            dev = self.device
            tmp = [(torch.empty((N,) + self.shape, dtype=torch.float32, device=dev),
                    torch.empty((N,) + self.shape, dtype=torch.uint8, device=dev)) for _ in range(min(self.n_affine, 2))]
            b = self._bufs[N] = {"img": torch.empty((N, 1) + self.shape, dtype=torch.float32, device=dev),
                                 "seg": torch.empty((N,) + self.shape, dtype=torch.uint8, device=dev),
                                 "tmp": [t for pair in tmp for t in pair],
                                 "box": _BoxOut(N, self.shape, self.n_classes, self.capacity, self.comp_cap, dev)}
        return b

    def _params(self, slots, per_sample):
        """-> (n_stages, N, PARAM_STRIDE) f64 and which stages any sample uses (stage 0 always runs: the gather)."""
        N, n_st = len(slots), max(1, self.n_affine)
        p = np.zeros((n_st, N, PARAM_STRIDE), dtype=np.float64)
        used = [True] + [False] * (n_st - 1)
        for n, (slot, ((axis, rev), stages)) in enumerate(zip(slots, per_sample)):
            for j in range(n_st):
                row = p[j, n]
                row[0] = slot if j == 0 else n
                row[1:4] = axis if j == 0 else (0, 1, 2)
                row[4:7] = rev if j == 0 else (0, 0, 0)
                st = stages[j] if j < len(stages) else None
                if st is not None:
                    row[7], row[8:11], row[11:14] = 1.0, st[0], st[1]
                    used[j] = True
        return p, used

    def _run(self, slots, per_sample, b):
        dev = self.device
        stream = _stream(dev)
        p, used = self._params(slots, per_sample)
        pd = torch.from_numpy(p).pin_memory().to(dev, non_blocking=True)
        N = len(slots)
        stages = [j for j in range(len(used)) if used[j]]
        src_img, src_seg, n_src = self.img, self.seg, self.img.shape[0]
        for k, j in enumerate(stages):
            last = k == len(stages) - 1
            dst_img, dst_seg = (b["img"], b["seg"]) if last else (b["tmp"][2 * (k % 2)], b["tmp"][2 * (k % 2) + 1])
            _lib.call("msl_augment_resample", ptr(src_img), ptr(src_seg), n_src, ptr(pd[j]), N, *self.shape,
                      ptr(dst_img), ptr(dst_seg), stream)
            src_img, src_seg, n_src = dst_img, dst_seg, N
        b["box"].launch(b["seg"], stream)

    def train_batches(self, epoch):
        tr = self.dataset.train_dataset
        for idx in train_batch_order(self.dataset, epoch):
            per_sample = []
            for i in idx:
                draws = draw_augmentations(self.augmentations, sample_rng(tr.seed, epoch, tr.subjects[i])) \
                    if self.augmentations else []
                per_sample.append(sample_params(draws, self.shape))
            b = self._buffers(len(idx))
            self._run([self.train_slots[i] for i in idx], per_sample, b)
            yield {"img": b["img"], "seg": b["seg"], "gb": b["box"].gb, "gl": b["box"].gl, "obj_off": b["box"].obj_off,
                   "capacity": self.capacity, "subject": [tr.subjects[i] for i in idx], "_box": b["box"]}

    def step(self, trainer, batch, metrics=False):
        """One ``FusedTrainer.step_packed`` on a ``train_batches`` batch; raises HipKernelError if the batch overflowed
        the capacity (checked after the step's own loss read: no extra synchronisation)."""
        out = trainer.step_packed(batch["img"], batch["gb"], batch["gl"], batch["obj_off"], batch["capacity"],
                                  resident=True, metrics=metrics)
        batch["_box"].raise_on_overflow()
        return out

    def val_batches(self):
        """``validation_step`` batches (device tensors, per-image box lists) of this rank's validation shard."""
        ident = (([0, 1, 2], [0, 0, 0]), [])
        for i0 in range(0, len(self.val_order), self.batch_size):
            chunk = self.val_order[i0:i0 + self.batch_size]
            b = self._buffers(len(chunk))
            self._run([slot for _, slot in chunk], [ident] * len(chunk), b)
            box = b["box"]
            off = box.obj_off.cpu().tolist()
            box.raise_on_overflow(box.flag.item())
            boxes = [box.gb[off[n]:off[n + 1]].clone() for n in range(len(chunk))]
            labels = [box.gl[off[n]:off[n + 1]].clone() for n in range(len(chunk))]
            yield {"img": b["img"].clone(), "seg": [boxes, labels], "boxes": boxes, "labels": labels,
                   "subject": [s for s, _ in chunk]}
