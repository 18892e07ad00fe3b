"""msl_paste_lesions (csrc/lesionpaste.hip) through the C ABI against its host mirror
``datasets.paste_lesions`` bit for bit on the cases of tests/lesionpaste_cases.py, and the lesionpaste stage of
``devicedata.LesionCache`` (fit and patch-window routes; instance, binary and two-sequence trees) against the host loader."""
import numpy as np
import pytest
import torch

from mslesions3d_amd import _lib
from mslesions3d_amd import datasets as DS
from mslesions3d_amd.devicedata import LesionCache
from tests import lesionpaste_cases as LC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GUARD = 4096
PATTERN, PATTERN16 = 0x5A5AC3C3, 0x5A5A


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _arena(donors):
    """The donor cases as msl_augment_fit_mc's arenas: (image arena, mask arena, table (n, 4) i64), on the device."""
    C = donors[0][0].shape[0]
    sizes = [int(np.prod(s.shape)) for _, s in donors]
    offs = [0] + np.cumsum(sizes).tolist()
    img = np.concatenate([i.reshape(-1) for i, _ in donors])  # case k: C planes from element C * off_k on
    seg = np.concatenate([s.reshape(-1) for _, s in donors])
    table = np.array([[offs[k], *donors[k][1].shape] for k in range(len(donors))], dtype=np.int64)
    assert img.size == C * offs[-1]
    return torch.from_numpy(img).to(DEV), torch.from_numpy(seg).to(DEV), torch.from_numpy(table).to(DEV)


def _guarded(host, pattern, as_int):
    """A device copy of ``host`` between two poisoned guard zones -> (whole buffer, view of the payload)."""
    n = host.numel()
    buf = torch.full((n + 2 * GUARD,), pattern, dtype=as_int, device=DEV)
    view = buf[GUARD:GUARD + n].view(host.dtype).view(host.shape)
    view.copy_(host)
    return buf, view


def _guards_intact(buf, n, pattern):
    host = buf.cpu()
    return bool((host[:GUARD] == pattern).all()) and bool((host[GUARD + n:] == pattern).all())


@pytest.mark.parametrize("value", [1, 7])
@pytest.mark.parametrize("C", [1, 2])
def test_kernel_equals_the_host_function_on_every_case(C, value):
    donors = LC.donors(C)
    arena_img, arena_seg, table = _arena(donors)
    samples = LC.samples(value)
    for shape in (LC.TARGET, LC.TARGET_32):
        group = [s for s in samples if s[1] == shape]
        N = len(group)
        img0, seg0 = LC.target(C, shape)
        rows = np.stack([np.stack(s[2]) for s in group])  # (N, K, stride)
        assert rows.shape == (N, LC.K, DS.PASTE_HEAD + 3 * LC.N_CAND)
        want_img, want_seg, want_rep = [], [], []
        for s in group:
            i, m = img0.copy(), seg0.copy()
            want_rep.append(DS.paste_lesions(i, m, np.stack(s[2]), donors))
            assert want_rep[-1] == s[3], s[0]
            want_img.append(i)
            want_seg.append(m)
        bi, img = _guarded(torch.from_numpy(np.stack([img0] * N)), PATTERN, torch.int32)
        bs, seg = _guarded(torch.from_numpy(np.stack([seg0] * N)), PATTERN16, torch.int16)
        br, rep = _guarded(torch.full((N, LC.K), 77, dtype=torch.int32), PATTERN, torch.int32)
        d_rows = torch.from_numpy(rows).to(DEV)
        _lib.call("msl_paste_lesions", arena_img.data_ptr(), arena_seg.data_ptr(), arena_seg.numel(), C, table.data_ptr(),
                  len(donors), d_rows.data_ptr(), N, LC.K, LC.N_CAND, *shape, img.data_ptr(), seg.data_ptr(), rep.data_ptr(),
                  _stream())
        torch.cuda.synchronize()
        assert _guards_intact(bi, img.numel(), PATTERN) and _guards_intact(bs, seg.numel(), PATTERN16)
        assert _guards_intact(br, rep.numel(), PATTERN)
        assert torch.equal(rep.cpu(), torch.tensor(want_rep, dtype=torch.int32))
        assert torch.equal(seg.cpu(), torch.from_numpy(np.stack(want_seg)))
        assert torch.equal(img.cpu().view(torch.int32), torch.from_numpy(np.stack(want_img)).view(torch.int32))  # the bits
        # the arenas are read only
        assert torch.equal(arena_seg.cpu(), torch.from_numpy(np.concatenate([s.reshape(-1) for _, s in donors])))
        assert torch.equal(arena_img.cpu(), torch.from_numpy(np.concatenate([i.reshape(-1) for i, _ in donors])))


def test_error_returns_write_nothing():
    lib = _lib.load()
    donors = LC.donors(1)
    arena_img, arena_seg, table = _arena(donors)
    img0, seg0 = LC.target(1)
    img, seg = torch.from_numpy(img0[None]).to(DEV), torch.from_numpy(seg0[None]).to(DEV)
    rep = torch.full((1, 16), 77, dtype=torch.int32, device=DEV)
    rows = torch.from_numpy(np.stack([LC.row(LC.A, [LC.FREE])] * 16)).to(DEV)  # enough ints for every K and n_cand below

    def call(C=1, n_cases=3, N=1, K=1, n_cand=LC.N_CAND, T=LC.TARGET, seg_elems=None, **null):
        p = {"arena_img": arena_img, "arena_seg": arena_seg, "table": table, "rows": rows, "img": img, "seg": seg, "report": rep}
        p.update(null)
        return lib.msl_paste_lesions(_lib.ptr(p["arena_img"]), _lib.ptr(p["arena_seg"]),
                                     arena_seg.numel() if seg_elems is None else seg_elems, C, _lib.ptr(p["table"]), n_cases,
                                     _lib.ptr(p["rows"]), N, K, n_cand, *T, _lib.ptr(p["img"]), _lib.ptr(p["seg"]),
                                     _lib.ptr(p["report"]), _stream())

    for name in ("arena_img", "arena_seg", "table", "rows", "img", "seg", "report"):
        assert call(**{name: None}) == -1, name
    for bad in (dict(C=0), dict(n_cases=0), dict(N=0), dict(K=0), dict(n_cand=0), dict(T=(16, 0, 20)), dict(seg_elems=0)):
        assert call(**bad) == -1, bad
    for bad in (dict(C=5), dict(K=9), dict(n_cand=17)):
        assert call(**bad) == -2, bad
    torch.cuda.synchronize()
    assert torch.equal(img.cpu(), torch.from_numpy(img0[None])) and torch.equal(seg.cpu(), torch.from_numpy(seg0[None]))
    assert bool((rep == 77).all())
    # an arena shorter than the table says: the row is refused, not read
    assert call(seg_elems=int(np.prod(LC.DONOR_SHAPES[0])) - 1) == 0
    torch.cuda.synchronize()
    assert rep[0, 0].item() == -2 and torch.equal(seg.cpu(), torch.from_numpy(seg0[None]))
    assert call() == 0
    torch.cuda.synchronize()
    assert rep[0, 0].item() == 0 and int((seg == 1).sum()) == LC.A[3]


# ---- end to end ----------------------------------------------------------------------------------------------------------
def _snapshot(b):
    return {k: (b[k].cpu() if torch.is_tensor(b[k]) else list(b[k])) for k in
            ("img", "seg", "gb", "gl", "obj_off", "subject", "paste_report")}


@pytest.mark.parametrize("patch", [None, LC.PATCH])
@pytest.mark.parametrize("kind", ["instances", "binary", "mc"])
def test_lesion_cache_batches_equal_the_host_loader(tmp_path, monkeypatch, kind, patch):
    """Two epochs, prob = 1, the MR stage behind the paste.  On the patch route the host loader normalises with the
    device's arithmetic, so its batches are the cache's, bit for bit.  On the fit route it normalises with numpy's sums
    (the bound of DESIGN.md section 4.7): boxes, labels and reports are compared with that loader as it is, and images with
    the same loader reading the cached volumes (target and donors), which is what the stage is: the same bits from the
    same input."""
    dm = LC.module(tmp_path, kind, patch)
    tr = dm.train_dataset
    cache = LesionCache(dm, DEV)
    assert np.array_equal(cache.bank.rows, tr.bank.rows) and np.array_equal(cache.bank.max_ids, tr.bank.max_ids)
    assert cache.bank.shapes == tr.bank.shapes and cache.train_slots == list(range(len(tr)))
    plain = []
    for epoch in range(2):
        dm.set_epoch(epoch)
        plain.append(list(dm.train_dataloader()))
    if patch is None:  # the host loader on the cached volumes
        tr.donors._held.clear()
        cropped = tr.__class__.cropped

        def cached(i):
            ci, cs = cache.case(cache.slot[tr.subjects[i]])
            ci = ci.cpu().numpy()
            return (ci[None] if ci.ndim == 3 else ci, cs.cpu().numpy()[None]) + cropped(tr, i)[2:]
        monkeypatch.setattr(tr, "cropped", cached)
    asked = accepted = 0
    for epoch in range(2):
        dm.set_epoch(epoch)
        host = list(dm.train_dataloader())
        dev = [_snapshot(b) for b in cache.train_batches(epoch)]
        assert [d["subject"] for d in dev] == [h["subject"] for h in host] == [h["subject"] for h in plain[epoch]]
        seen = 0
        for d, h, p in zip(dev, host, plain[epoch]):
            off = d["obj_off"].tolist()
            assert d["paste_report"].tolist() == h["paste_report"] == p["paste_report"]
            assert torch.equal(d["img"].view(torch.int32), h["img"].view(torch.int32))
            for n in range(len(d["subject"])):
                for ref in (h, p):
                    assert torch.equal(d["gb"][off[n]:off[n + 1]], ref["boxes"][n])
                    assert torch.equal(d["gl"][off[n]:off[n + 1]], ref["labels"][n])
            seen += int((d["paste_report"] >= 0).sum())
            asked += int((d["paste_report"] > -2).sum())
        assert seen >= 1, (kind, patch, epoch)  # (tests/test_lesionpaste_cpu.py shows it of the host reference alone)
        accepted += seen
    assert cache.paste_counts() == (asked, accepted) and cache.paste_counts() == (0, 0)
    # validation batches are not pasted
    assert "paste_report" not in next(iter(cache.val_batches()))
