"""GPU tests (-m gpu) of csrc/dataload.hip through dinounet_amd.dataloading, against the numpy restatement that CPU tensors run
(tests/test_cpu_dataloading.py checks that restatement against brute force).  Every comparison is exact: the results are integers or copies
of fp32 values.

The volumes give n = 1, exactly one chunk of 1024 voxels, one voxel more, a non-multiple and many chunks (512 for (8, 256, 256)); the ranks
asked for are a permutation of ALL ranks of a class, so the first and the last member of every chunk are selected.  The reference of a
volume is computed once."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from dinounet_amd import _lib
from dinounet_amd import dataloading as DL
from test_cpu_dataloading import FINAL, IGNORE, LABELS, PATCH, make_case, make_dataset
from test_gpu_ops import dev

pytestmark = pytest.mark.gpu

VOLUMES = [(1, 1, 1), (1, 32, 32), (1, 25, 41), (2, 9, 67), (5, 37, 131), (8, 256, 256)]
MIXED = [5, 1, 6, 7, (2, 3), (0, 1, 63)]          # absent; a plain class; first and last voxel only; whole chunks without it; regions


def mixed_volume(shape):
    """labels -1, 0, 1, 2, 3, 70 at random; 6 in the first and the last voxel only; 7 in every fifth chunk of 1024 voxels only"""
    rng = np.random.RandomState(sum(shape))
    n = int(np.prod(shape))
    seg = rng.choice(np.array([-1, 0, 1, 2, 3, 70], np.int16), size=n)
    chunk = np.arange(n) // 1024
    seven = (chunk % 5 == 2) & (rng.random_sample(n) < 0.3)
    seg[seven] = 7
    seg[0], seg[-1] = 6, 6
    return seg.reshape(shape)


@functools.lru_cache(maxsize=None)
def volume_reference(shape, kind):
    seg = np.full(shape, 4, np.int16) if kind == "full" else mixed_volume(shape)
    entries = [4, 5] if kind == "full" else MIXED
    t = torch.from_numpy(seg)
    counts = DL.ClassCounts(t, entries)
    totals = counts.totals.tolist()
    ranks = [torch.from_numpy(np.random.RandomState(g).permutation(n)) for g, n in enumerate(totals)]
    rows = [counts.select(g, r) if len(r) else None for g, r in enumerate(ranks)]
    return t, entries, totals, ranks, rows


@pytest.mark.parametrize("kind", ["full", "mixed"])
@pytest.mark.parametrize("shape", VOLUMES, ids=str)
def test_counts_and_select(shape, kind):
    t, entries, totals, ranks, rows = volume_reference(shape, kind)
    seg = t.to(dev())
    counts = DL.ClassCounts(seg, entries)
    got = counts.totals.cpu().tolist()
    print(f"{shape} {kind}: totals {got} (restatement {totals})")
    assert got == totals
    if kind == "full":
        assert totals == [int(np.prod(shape)), 0]
    else:
        assert totals[0] == 0 and totals[2] == (1 if shape == (1, 1, 1) else 2)
    for g, r in enumerate(ranks):
        if len(r) == 0:
            continue
        out = counts.select(g, r.to(dev()))
        assert out.dtype == torch.int32 and tuple(out.shape) == (len(r), 4)
        assert torch.equal(out.cpu(), rows[g]), f"class {entries[g]}"
    assert torch.equal(seg.cpu(), t), "the input was modified"


def test_select_rank_outside_total():
    """a rank outside [0, total) names no voxel: {0, -1, -1, -1}, nothing else is touched"""
    t, entries, totals, _, rows = volume_reference((2, 9, 67), "mixed")
    counts = DL.ClassCounts(t.to(dev()), entries)
    r = torch.tensor([0, totals[1], -1, totals[1] - 1, 1 << 40], dtype=torch.int64, device=dev())
    out = counts.select(1, r).cpu()
    first_last = DL.ClassCounts(t, entries).select(1, torch.tensor([0, totals[1] - 1]))
    assert torch.equal(out[[0, 3]], first_last)
    assert out[[1, 2, 4]].tolist() == [[0, -1, -1, -1]] * 3


def check_locations(seg, entries):
    t_tables, t_mirror = DL.sample_foreground_locations(seg, entries)
    g_tables, g_mirror = DL.sample_foreground_locations(seg.to(dev()), entries)
    assert list(g_tables) == list(t_tables) == list(g_mirror)
    for k in t_tables:
        assert g_tables[k].is_cuda and g_tables[k].dtype == torch.int32
        assert torch.equal(g_tables[k].cpu(), t_tables[k]), k
        if len(t_mirror[k]) == 0:
            assert g_mirror[k] == [] and tuple(g_tables[k].shape) == (0, 4)
        else:
            assert isinstance(g_mirror[k], np.ndarray) and np.array_equal(g_mirror[k], t_mirror[k])
    return t_mirror


@pytest.mark.parametrize("shape", VOLUMES[:5], ids=str)
def test_sample_foreground_locations_small(shape):
    check_locations(torch.from_numpy(mixed_volume(shape))[None], MIXED)


def test_sample_foreground_locations_one_percent_rule():
    """one class with more than 1 000 000 voxels: the 1 % rule decides the size of its table"""
    rng = np.random.RandomState(0)
    seg = (rng.random_sample((1, 5, 512, 512)) < 0.85).astype(np.int16)
    seg[0, 2, 100:140, 200:260] = 2
    mirror = check_locations(torch.from_numpy(seg), [1, 2, (1, 2)])
    n = int((seg == 1).sum())
    assert n > 1000000 and len(mirror[1]) == int(np.ceil(n * 0.01)) > 10000
    assert len(mirror[2]) == 2400


# ------------------------------------------------------------------------------------------------ gather
GATHER_SHAPES = [(2, 40, 50), (1, 33, 47), (3, 10, 13), (2, 64, 64), (1, 70, 31)]
#           inside      top edge    bottom edge  left edge   right edge
WINDOWS_A = [(1, 5, 7), (0, -9, 3), (2, 3, 5), (1, 11, -17), (0, 20, 9)]
#           corner        entirely outside  patch > image  odd x0     past the high corner
WINDOWS_B = [(0, -5, -11), (0, 500, -300), (1, -7, -9), (0, 13, 21), (0, 60, 25)]


@functools.lru_cache(maxsize=None)
def gather_datasets(channels):
    cpu, gpu = DL.DeviceDataset(), DL.DeviceDataset()
    for i, shape in enumerate(GATHER_SHAPES):
        data, seg = make_case(shape, channels, 40 + i, False)
        d, s = torch.from_numpy(data), torch.from_numpy(seg)
        cpu.add(i, d, s, {"class_locations": {}})
        gpu.add(i, d.to(dev()), s.to(dev()), {"class_locations": {}})
    return cpu, gpu


@pytest.mark.parametrize("seg_float", [False, True], ids=["int16", "fp32"])
@pytest.mark.parametrize("windows", [WINDOWS_A, WINDOWS_B], ids=["edges", "corners"])
@pytest.mark.parametrize("patch", [(24, 30), (16, 32)], ids=str)
@pytest.mark.parametrize("channels", [1, 3])
def test_gather(channels, patch, windows, seg_float):
    cpu, gpu = gather_datasets(channels)
    d = dict(keys=list(range(5)), slices=np.array([min(w[0], GATHER_SHAPES[i][0] - 1) for i, w in enumerate(windows)]),
             bbox_lbs=np.array([w[1:] for w in windows]))
    want_data, want_seg = DL.DataLoader2D(cpu, 5, patch, patch, LABELS, False).assemble(d, seg_float=seg_float)
    before = [(gpu[i][0].clone(), gpu[i][1].clone()) for i in range(5)]
    data, seg = DL.DataLoader2D(gpu, 5, patch, patch, LABELS, False).assemble(d, seg_float=seg_float)
    assert data.is_cuda and data.dtype == torch.float32 and seg.dtype == (torch.float32 if seg_float else torch.int16)
    assert tuple(data.shape) == (5, channels, *patch) and tuple(seg.shape) == (5, 1, *patch)
    assert torch.equal(data.cpu(), want_data)
    assert torch.equal(seg.cpu(), want_seg)
    if windows is WINDOWS_B:
        assert not want_data[1].any() and (want_seg[1] == -1).all()                   # entirely outside: all padding
        assert (want_seg[2] == -1).any() and (want_seg[2, 0, 7:17, 9:22] >= 0).all()  # the whole (10, 13) image inside the larger patch
    for i in range(5):
        assert torch.equal(gpu[i][0], before[i][0]) and torch.equal(gpu[i][1], before[i][1]), "the input was modified"


# ------------------------------------------------------------------------------------------------ the loader
@functools.lru_cache(maxsize=None)
def datasets(with_ignore):
    return make_dataset("cpu", with_ignore=with_ignore), make_dataset(dev(), with_ignore=with_ignore)


@pytest.mark.parametrize("with_ignore", [False, True], ids=["plain", "ignore"])
def test_loader_batch(with_ignore):
    cpu, gpu = datasets(with_ignore)
    for k in cpu:                                                                     # the tables the two loaders draw from are the same
        for c, rows in cpu[k][2]["class_locations"].items():
            assert np.array_equal(np.asarray(gpu[k][2]["class_locations"][c]), np.asarray(rows))
    a = DL.DataLoader2D(gpu, 7, PATCH, FINAL, LABELS, with_ignore, seed=21)
    b = DL.DataLoader2D(cpu, 7, PATCH, FINAL, LABELS, with_ignore, seed=21)
    for _ in range(2):
        batch = next(a)
        d = a.last_draw
        d_cpu = b.draw()
        assert d["keys"] == d_cpu["keys"] and np.array_equal(d["slices"], d_cpu["slices"]) and np.array_equal(d["bbox_lbs"], d_cpu["bbox_lbs"])
        want_data, want_seg = b.assemble(d)
        assert batch["data"].is_cuda and batch["seg"].dtype == torch.int16
        assert torch.equal(batch["data"].cpu(), want_data) and torch.equal(batch["seg"].cpu(), want_seg)
        assert batch["keys"] == d["keys"] and batch["properties"][0] is gpu[d["keys"][0]][2]
        assert (want_seg == -1).any()                                                 # some case is smaller than the patch


@pytest.mark.parametrize("regions", [None, [(1, 2), 2]], ids=["labels", "regions"])
@pytest.mark.parametrize("with_ignore", [False, True], ids=["plain", "ignore"])
def test_train_batches(with_ignore, regions):
    from dinounet_amd.augment import GPUAugment2D
    from dinounet_amd.training import labels_to_regions
    _, gpu = datasets(with_ignore)
    patch, B = (32, 40), 4
    kw = dict(all_labels=LABELS, ignore_label=IGNORE) if with_ignore else {}
    tb = DL.TrainBatches(gpu, patch, B, regions=regions, seed=3, **kw)
    assert tb.loader.patch_size == DL.initial_patch_size(patch) and tb.loader.final_patch_size == patch
    for _ in range(2):
        x, t = next(tb)
        d, a = tb.last_draw
        data, seg = tb.loader.assemble(d)
        assert seg.dtype == torch.float32 and tuple(data.shape) == (B, 2, *tb.loader.patch_size)
        want_x, want_t = GPUAugment2D(patch).apply(data, seg, a)
        want_t = want_t.long()
        assert not (want_t < 0).any()
        if regions is not None:
            want_t = labels_to_regions(want_t, regions, IGNORE if with_ignore else None)
        assert torch.equal(x, want_x) and torch.equal(t, want_t)
        assert x.dtype == torch.float32 and tuple(x.shape) == (B, 2, *patch)
        if regions is None:                                                           # what TrainStep's static buffers are: fp32 x, int64 labels
            assert t.dtype == torch.int64 and tuple(t.shape) == (B, 1, *patch)
            x_buf, t_buf = torch.zeros(x.shape, device=dev()), torch.zeros(t.shape, dtype=torch.long, device=dev())
            assert torch.equal(x_buf.copy_(x), x) and torch.equal(t_buf.copy_(t), t)
        else:
            assert t.dtype == torch.uint8 and tuple(t.shape) == (B, 2 + int(with_ignore), *patch)


def test_val_batches():
    cpu, gpu = datasets(True)
    a = DL.TrainBatches(gpu, (64, 72), 5, all_labels=LABELS, ignore_label=IGNORE, seed=2, val=True)
    b = DL.TrainBatches(cpu, (64, 72), 5, all_labels=LABELS, ignore_label=IGNORE, seed=2, val=True)
    x, t = next(a)
    want_x, want_t = next(b)
    assert a.loader.patch_size == (64, 72) and a.last_draw[1] is None
    assert torch.equal(x.cpu(), want_x) and torch.equal(t.cpu(), want_t)
    assert t.dtype == torch.int64 and not (t < 0).any()
    assert (a.loader.assemble(a.last_draw[0])[1] == -1).any()                         # the loader's batch had padding


# ------------------------------------------------------------------------------------------------ error returns
def test_error_returns():
    """every error comes back before anything is launched, as a RuntimeError naming the code"""
    L = _lib.lib()
    d = dev()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    seg = torch.zeros((2, 8, 8), dtype=torch.int16, device=d)
    masks = torch.tensor([2], dtype=torch.int64, device=d)
    totals = torch.full((1,), -7, dtype=torch.int64, device=d)
    ws = torch.full((8,), -7, dtype=torch.int32, device=d)
    ranks = torch.zeros(1, dtype=torch.int64, device=d)
    out = torch.full((1, 4), -7, dtype=torch.int32, device=d)
    p = lambda t: C.c_void_p(t.data_ptr())
    need = DL.workspace_elems(2, 8, 8, 1)
    assert need == 4

    def bad(rc, code):
        with pytest.raises(RuntimeError, match=code):
            _lib.check(rc, "du_dl")

    bad(L.du_dl_class_counts(None, p(masks), 1, 2, 8, 8, p(ws), need, p(totals), st), "DU_ERR_BAD_ARG")
    bad(L.du_dl_class_counts(p(seg), p(masks), 1, 2, 8, 8, None, need, p(totals), st), "DU_ERR_BAD_ARG")
    bad(L.du_dl_class_counts(p(seg), p(masks), 1, 2, 0, 8, p(ws), need, p(totals), st), "DU_ERR_BAD_ARG")
    bad(L.du_dl_class_counts(p(seg), p(masks), 0, 2, 8, 8, p(ws), need, p(totals), st), "DU_ERR_BAD_ARG")
    bad(L.du_dl_class_counts(p(seg), p(masks), 1, 2, 8, 8, p(ws), need - 1, p(totals), st), "DU_ERR_BAD_ARG")
    bad(L.du_dl_class_counts(p(seg), p(masks), 1, 2, 8, 8, C.c_void_p(ws.data_ptr() + 4), need, p(totals), st), "DU_ERR_BAD_ARG")
    bad(L.du_dl_class_counts(p(seg), p(masks), 1, 2048, 1024, 1024, p(ws), need, p(totals), st), "DU_ERR_UNSUPPORTED")
    bad(L.du_dl_select(p(seg), p(masks), 1, 0, 2, 8, 8, p(ws), need, None, 1, p(out), st), "DU_ERR_BAD_ARG")
    bad(L.du_dl_select(p(seg), p(masks), 1, 0, 2, 8, 8, p(ws), need, p(ranks), 0, p(out), st), "DU_ERR_BAD_ARG")
    bad(L.du_dl_select(p(seg), p(masks), 1, 1, 2, 8, 8, p(ws), need, p(ranks), 1, p(out), st), "DU_ERR_BAD_ARG")
    bad(L.du_dl_select(p(seg), p(masks), 1, 0, 2, 8, 8, p(ws), need - 1, p(ranks), 1, p(out), st), "DU_ERR_BAD_ARG")
    jobs = torch.zeros((1, 8), dtype=torch.int64, device=d)
    img = torch.full((1, 1, 4, 4), -7.0, device=d)
    lab = torch.full((1, 1, 4, 4), -7, dtype=torch.int16, device=d)
    bad(L.du_dl_gather(None, 1, 1, 4, 4, p(img), p(lab), 0, st), "DU_ERR_BAD_ARG")
    bad(L.du_dl_gather(p(jobs), 1, 1, 4, 4, None, p(lab), 0, st), "DU_ERR_BAD_ARG")
    bad(L.du_dl_gather(p(jobs), 1, 1, 0, 4, p(img), p(lab), 0, st), "DU_ERR_BAD_ARG")
    bad(L.du_dl_gather(p(jobs), 0, 1, 4, 4, p(img), p(lab), 0, st), "DU_ERR_BAD_ARG")
    # through the size function: nothing is allocated for a shape that is refused
    with pytest.raises(RuntimeError, match="DU_ERR_UNSUPPORTED"):
        DL.workspace_elems(2048, 1024, 1024, 1)
    with pytest.raises(RuntimeError, match="DU_ERR_UNSUPPORTED"):
        DL.workspace_elems(1 << 16, 1 << 15, 1, 1)
    with pytest.raises(RuntimeError, match="DU_ERR_BAD_ARG"):
        DL.workspace_elems(0, 8, 8, 1)
    assert DL.workspace_elems(2047, 1024, 1024, 2) == 2 * 2047 * 1024
    torch.cuda.synchronize()
    for t in (totals, ws, out, lab):                                                  # no kernel ran: nothing was written
        assert (t == -7).all()
    assert (img == -7).all()
