"""CPU tests of dinounet_amd.dataloading: the numpy restatement that CPU tensors run (and that tests/test_gpu_dataloading.py compares the
kernels of csrc/dataload.hip against) is checked here against brute force written in this file.  Every comparison is exact: everything is
integers or copies of fp32 values.

The draw sequence is checked against a straight-line transcription of the order in which nnUNetDataLoader2D.generate_train_batch and
nnUNetDataLoaderBase.get_bbox draw from numpy's GLOBAL stream after np.random.seed(s); RandomState(s) and the seeded global stream agree
draw for draw.  The helpers that build synthetic cases are shared with the GPU tests."""
import numpy as np
import pytest
import torch

from dinounet_amd import dataloading as DL

CASE_SHAPES = [(1, 40, 50), (3, 33, 47), (2, 64, 64), (4, 20, 90), (1, 70, 30), (2, 45, 45)]     # (D, H, W); some smaller than the patch
PATCH, FINAL = (48, 56), (40, 48)
LABELS, IGNORE = (0, 1, 2), 3


# ------------------------------------------------------------------------------------------------ synthetic cases
def make_case(shape, channels, seed, with_ignore, foreground=True):
    """(data (C, D, H, W) fp32, seg (1, D, H, W) int16): blocks of labels 1 and 2 on background 0, with_ignore: a band of label 3"""
    rng = np.random.RandomState(seed)
    D, H, W = shape
    data = rng.randn(channels, D, H, W).astype(np.float32)
    seg = np.zeros((1, D, H, W), np.int16)
    if foreground:
        for lab in (1, 2, 1):
            z, y, x = rng.randint(0, D), rng.randint(0, H - 4), rng.randint(0, W - 4)
            seg[0, z:z + 2, y:y + rng.randint(3, 12), x:x + rng.randint(3, 12)] = lab
    if with_ignore:
        seg[0, :, :, W // 2:W // 2 + 5] = IGNORE
    return data, seg


def make_dataset(device, channels=2, with_ignore=False, seed=0):
    """six cases of different shapes on `device`, the fourth without foreground; class locations of labels 1, 2 (and the annotated key)"""
    ds = DL.DeviceDataset()
    for i, shape in enumerate(CASE_SHAPES):
        data, seg = make_case(shape, channels, seed * 100 + i, with_ignore, foreground=i != 3)
        d, s = torch.from_numpy(data).to(device), torch.from_numpy(seg).to(device)
        props = DL.add_class_locations(s, {"name": f"case{i}"}, [1, 2], all_labels=LABELS if with_ignore else None)
        ds.add(f"case{i}", d, s, props)
    return ds


def brute_locations(seg, entries, seed=1234):
    """the reference's recipe on the (1, D, H, W) array: np.argwhere and one shared RandomState"""
    rs = np.random.RandomState(seed)
    out = {}
    for c in entries:
        labels = list(c) if isinstance(c, (tuple, list)) else [c]
        mask = np.isin(seg, labels)
        locs = np.argwhere(mask)
        key = tuple(c) if isinstance(c, (tuple, list)) else c
        if len(locs) == 0:
            out[key] = []
            continue
        m = max(min(10000, len(locs)), int(np.ceil(len(locs) * 0.01)))
        out[key] = locs[rs.choice(len(locs), m, replace=False)]
    return out


def same_tables(got, want):
    assert list(got.keys()) == list(want.keys())
    for k in want:
        if len(want[k]) == 0:
            assert len(got[k]) == 0
        else:
            assert np.array_equal(np.asarray(got[k]), want[k]), k


# ------------------------------------------------------------------------------------------------ class locations
def test_class_locations_restatement():
    rng = np.random.RandomState(3)
    seg = rng.choice(np.array([-1, 0, 1, 2, 3, 70], np.int16), size=(1, 3, 17, 23))
    entries = [1, 2, (1, 3), 5, [2, 3], 0]
    tables, mirror = DL.sample_foreground_locations(torch.from_numpy(seg), entries)
    want = brute_locations(seg, entries)
    assert list(mirror.keys()) == [1, 2, (1, 3), 5, (2, 3), 0]
    same_tables(mirror, want)
    assert mirror[5] == [] and tuple(tables[5].shape) == (0, 4)
    for k in want:
        assert tables[k].dtype == torch.int32
        same_tables({k: tables[k].numpy()}, {k: want[k]})
    counts = DL.ClassCounts(torch.from_numpy(seg), entries)
    assert counts.totals.tolist() == [int(np.isin(seg, [c] if isinstance(c, int) else list(c)).sum()) for c in entries]
    # labels -1 and 70 are in no mask, not even one with every bit set
    every = DL.ClassCounts(torch.from_numpy(seg), [tuple(range(64))])
    assert every.totals.tolist() == [int(((seg >= 0) & (seg <= 63)).sum())]
    with pytest.raises(ValueError):
        DL.sample_foreground_locations(torch.from_numpy(seg), [70])
    # the (D, H, W) form gives the same rows
    t3, m3 = DL.sample_foreground_locations(torch.from_numpy(seg[0]), entries)
    same_tables(m3, want)


@pytest.mark.parametrize("n, m", [(1, 1), (9999, 9999), (10000, 10000), (10001, 10000), (1000001, 10001)])
def test_class_locations_size_rule(n, m):
    assert DL.target_num_samples(n) == m
    shape = (1, 1, 1001, 1000) if n > 20000 else (1, 2, 80, 70)
    seg = np.zeros(int(np.prod(shape)), np.int16)
    seg[np.random.RandomState(n).permutation(seg.size)[:n]] = 1
    seg = seg.reshape(shape)
    _, mirror = DL.sample_foreground_locations(torch.from_numpy(seg), [1])
    want = brute_locations(seg, [1])
    assert len(want[1]) == m
    same_tables(mirror, want)


def test_add_class_locations_keys():
    _, seg = make_case((2, 30, 40), 1, 5, True)
    props = DL.add_class_locations(torch.from_numpy(seg), {}, [1, 2], all_labels=LABELS)
    assert list(props["class_locations"].keys()) == [1, 2, LABELS]
    same_tables(props["class_locations"], brute_locations(seg, [1, 2, list(LABELS)]))
    props = DL.add_class_locations(torch.from_numpy(seg), {}, [(1, 2), 2])
    assert list(props["class_locations"].keys()) == [(1, 2), 2]
    same_tables(props["class_locations"], brute_locations(seg, [(1, 2), 2]))


# ------------------------------------------------------------------------------------------------ the draw sequence
def transcribed_draws(ds, B, patch, final, all_labels, has_ignore, p, probs, probabilistic):
    """the reference's draws in the reference's order, from numpy's global stream"""
    annotated = tuple(all_labels)
    keys = list(ds.keys())
    selected_keys = np.random.choice(keys, B, True, probs)
    out_keys, slices, lbs_out, classes = [], [], [], []
    for j, key in enumerate(selected_keys):
        force_fg = (np.random.uniform() < p) if probabilistic else (not j < round(B * (1 - p)))
        data, seg, properties = ds[str(key)]
        locs = properties["class_locations"]
        if not force_fg:
            sel = annotated if has_ignore else None
        else:
            eligible = [i for i in locs.keys() if len(locs[i]) > 0]
            tmp = [i == annotated if isinstance(i, tuple) else False for i in eligible]
            if any(tmp) and len(eligible) > 1:
                eligible.pop(np.where(tmp)[0][0])
            sel = eligible[np.random.choice(len(eligible))] if len(eligible) > 0 else None
        if sel is not None:
            z = np.random.choice(locs[sel][:, 1])
        else:
            z = np.random.choice(len(data[0]))
        shape = tuple(data.shape[2:])
        need = [patch[i] - final[i] for i in range(2)]
        for d in range(2):
            if need[d] + shape[d] < patch[d]:
                need[d] = patch[d] - shape[d]
        lbs = [-need[i] // 2 for i in range(2)]
        ubs = [shape[i] + need[i] // 2 + need[i] % 2 - patch[i] for i in range(2)]
        if sel is None:
            bbox = [np.random.randint(lbs[i], ubs[i] + 1) for i in range(2)]
        else:
            rows = locs[sel][locs[sel][:, 1] == z][:, (0, 2, 3)]
            voxel = rows[np.random.choice(len(rows))]
            bbox = [max(lbs[i], voxel[i + 1] - patch[i] // 2) for i in range(2)]
        out_keys.append(str(key))
        slices.append(int(z))
        lbs_out.append([int(v) for v in bbox])
        classes.append(sel)
    return out_keys, slices, lbs_out, classes


DRAW_CONFIGS = {
    "plain": dict(with_ignore=False, probabilistic=False, probs=None, p=0.33),
    "ignore": dict(with_ignore=True, probabilistic=False, probs=None, p=0.33),
    "probabilistic": dict(with_ignore=False, probabilistic=True, probs=None, p=0.5),
    "ignore_probabilistic": dict(with_ignore=True, probabilistic=True, probs=None, p=0.5),
    "sampling_probabilities": dict(with_ignore=False, probabilistic=False, probs=[0.05, 0.1, 0.15, 0.4, 0.2, 0.1], p=0.66),
}
_DATASETS = {}


def cpu_dataset(with_ignore):
    if with_ignore not in _DATASETS:
        _DATASETS[with_ignore] = make_dataset("cpu", with_ignore=with_ignore)
    return _DATASETS[with_ignore]


@pytest.mark.parametrize("seed", [0, 1, 7, 1234])
@pytest.mark.parametrize("config", list(DRAW_CONFIGS))
def test_draw_sequence(config, seed):
    cfg = DRAW_CONFIGS[config]
    ds = cpu_dataset(cfg["with_ignore"])
    assert len(ds["case3"][2]["class_locations"][1]) == 0 and len(ds["case3"][2]["class_locations"][2]) == 0     # the case without foreground
    B = 7
    loader = DL.DataLoader2D(ds, B, PATCH, FINAL, LABELS, cfg["with_ignore"], cfg["p"], cfg["probs"], cfg["probabilistic"], seed=seed)
    np.random.seed(seed)
    for _ in range(3):                                                                # three batches: the streams stay in step
        d = loader.draw()
        keys, slices, lbs, classes = transcribed_draws(ds, B, PATCH, FINAL, LABELS, cfg["with_ignore"], cfg["p"], cfg["probs"],
                                                       cfg["probabilistic"])
        assert d["keys"] == keys
        assert d["slices"].tolist() == slices
        assert d["bbox_lbs"].tolist() == lbs
        assert d["classes"] == classes
    assert np.random.uniform() == loader.rs.uniform()                                 # not one draw more or less


def test_draw_covers_every_path():
    """over some batches the configurations above take the random-position path, the class path and the no-foreground fallback"""
    ds = cpu_dataset(False)
    loader = DL.DataLoader2D(ds, 7, PATCH, FINAL, LABELS, False, 0.33, seed=5)
    seen = set()
    for _ in range(20):
        d = loader.draw()
        for k, f, c in zip(d["keys"], d["force_fg"], d["classes"]):
            seen.add((k == "case3", f, c is None))
    assert {(False, False, True), (False, True, False), (True, True, True)} <= seen


def test_ignore_without_annotated_voxel_raises():
    data, seg = make_case((1, 30, 30), 1, 0, False)
    seg[:] = IGNORE
    props = DL.add_class_locations(torch.from_numpy(seg), {}, [1, 2], all_labels=LABELS)
    ds = DL.DeviceDataset({"a": (torch.from_numpy(data), torch.from_numpy(seg), props)})
    with pytest.raises(ValueError, match="no annotated voxel"):
        DL.DataLoader2D(ds, 2, PATCH, FINAL, LABELS, True, seed=0).draw()
    with pytest.raises(ValueError, match="annotated-classes key"):
        DL.DataLoader2D(DL.DeviceDataset({"a": (torch.from_numpy(data), torch.from_numpy(seg), {"class_locations": {1: []}})}), 2, PATCH,
                        FINAL, LABELS, True)


# ------------------------------------------------------------------------------------------------ bounding boxes
def bbox_loader():
    data, seg = make_case((1, 30, 30), 1, 0, False)
    ds = DL.DeviceDataset({"a": (torch.from_numpy(data), torch.from_numpy(seg), {"class_locations": {1: []}})})
    return DL.DataLoader2D(ds, 2, PATCH, FINAL, LABELS, False, seed=0)


@pytest.mark.parametrize("shape", [(20, 100), (100, 21), (20, 21), (48, 56), (47, 55), (41, 49)])
def test_bbox_image_smaller_than_patch(shape):
    """a random box: every draw lies in [lbs, ubs], the image is inside the box wherever it is smaller than the patch, and the padding
    on the two sides differs by at most one"""
    loader = bbox_loader()
    seen = [set(), set()]
    for _ in range(200):
        lbs, ubs = loader.get_bbox(list(shape), None)
        for i in range(2):
            assert ubs[i] == lbs[i] + PATCH[i]
            seen[i].add(lbs[i])
            if shape[i] + (PATCH[i] - FINAL[i]) <= PATCH[i]:                          # the whole image fits: the box covers it, centred
                assert lbs[i] <= 0 and ubs[i] >= shape[i]
                assert abs(-lbs[i] - (ubs[i] - shape[i])) <= 1
    for i in range(2):
        need = max(PATCH[i] - FINAL[i], PATCH[i] - shape[i])
        allowed = set(range(-(need // 2) - need % 2, shape[i] + need // 2 + need % 2 - PATCH[i] + 1))
        assert seen[i] <= allowed and (len(allowed) > 2 or seen[i] == allowed)        # 200 draws miss one of two values with probability 2^-199


def test_bbox_voxel_at_corner_and_high_edge():
    loader = bbox_loader()
    H, W = 100, 120                                                                   # need_to_pad (8, 8): lbs (-4, -4), ubs (56, 68)
    lbs, ubs = loader.get_bbox([H, W], np.array([[0, 0, 0]]))
    assert lbs == [-4, -4] and ubs == [44, 52]                                        # voxel - patch // 2 = (-24, -28): held at lbs
    lbs, ubs = loader.get_bbox([H, W], np.array([[0, H - 1, W - 1]]))
    assert lbs == [99 - 24, 119 - 28] and lbs[0] > 56 and lbs[1] > 68                 # past ubs: NOT clamped
    assert ubs == [75 + 48, 91 + 56] and ubs[0] - H == 23 and ubs[1] - W == 27        # the box runs past the image
    lbs, _ = loader.get_bbox([H, W], np.array([[0, 50, 3]]))
    assert lbs == [26, -4]


# ------------------------------------------------------------------------------------------------ trainer arithmetic
def test_split_batch_for_rank():
    assert DL.split_batch_for_rank(8, 0.33, 0, 3) == (3, 0.0)
    assert DL.split_batch_for_rank(8, 0.33, 1, 3) == (3, 1 / 3)
    assert DL.split_batch_for_rank(8, 0.33, 2, 3) == (2, 1.0)
    for b, p in ((8, 0.33), (2, 0.0), (5, 1.0)):
        assert DL.split_batch_for_rank(b, p, 0, 1) == (b, p)
    with pytest.raises(ValueError):
        DL.split_batch_for_rank(2, 0.33, 0, 3)
    for world in (2, 3, 4, 8):                                                        # the ranks share out the batch and its oversampled tail
        parts = [DL.split_batch_for_rank(12, 0.33, r, world) for r in range(world)]
        assert sum(b for b, _ in parts) == 12
        assert round(sum(b * p for b, p in parts)) == 12 - round(12 * 0.67)


def test_initial_patch_size():
    assert DL.initial_patch_size((512, 512)) == (602, 602)
    assert DL.initial_patch_size((256, 256)) == (301, 301)
    a, b = DL.initial_patch_size((256, 512))                                          # aspect 2: the 15 degree limit
    c, s = np.cos(np.pi / 12), np.sin(np.pi / 12)
    assert (a, b) == (int(max(256 * c + 512 * s, 256) / 0.85), int(max(abs(512 * c - 256 * s), 512) / 0.85))


# ------------------------------------------------------------------------------------------------ batch assembly
def padded_window(img, pad_value, z, y0, x0, ph, pw):
    """img (C, D, H, W): the slice padded far enough on every side with np.pad, then the window"""
    m = max(ph, pw) + abs(y0) + abs(x0) + max(img.shape[2:])
    big = np.pad(img[:, z], ((0, 0), (m, m), (m, m)), "constant", constant_values=pad_value)
    return big[:, y0 + m:y0 + m + ph, x0 + m:x0 + m + pw]


def check_assembly(loader, ds, d, seg_float):
    data, seg = loader.assemble(d, seg_float=seg_float)
    ph, pw = loader.patch_size
    assert data.dtype == torch.float32 and seg.dtype == (torch.float32 if seg_float else torch.int16)
    assert tuple(seg.shape) == (len(d["keys"]), 1, ph, pw)
    for j, k in enumerate(d["keys"]):
        img, lab, _ = ds[k]
        z, (y0, x0) = int(d["slices"][j]), (int(v) for v in d["bbox_lbs"][j])
        assert np.array_equal(data[j].numpy(), padded_window(img.numpy(), 0, z, y0, x0, ph, pw))
        assert np.array_equal(seg[j].numpy(), padded_window(lab.numpy(), -1, z, y0, x0, ph, pw).astype(seg[j].numpy().dtype))


@pytest.mark.parametrize("seg_float", [False, True], ids=["int16", "fp32"])
def test_assembly_restatement(seg_float):
    ds = cpu_dataset(False)
    loader = DL.DataLoader2D(ds, 7, PATCH, FINAL, LABELS, False, seed=11)
    for _ in range(3):
        check_assembly(loader, ds, loader.draw(), seg_float)
    # windows the draws above may not reach: over every edge, a corner, entirely outside, an odd offset
    d = dict(keys=["case2"] * 7, slices=np.array([0, 1, 0, 1, 0, 1, 0]),
             bbox_lbs=np.array([[-10, 5], [30, 3], [5, -13], [7, 31], [-9, -11], [200, 300], [-48, 0]]))
    check_assembly(loader, ds, d, seg_float)
    batch = next(loader)
    assert sorted(batch) == ["data", "keys", "properties", "seg"] and batch["properties"][0] is ds[batch["keys"][0]][2]
    with pytest.raises(ValueError):
        loader.assemble(dict(keys=["case0"], slices=np.array([1]), bbox_lbs=np.array([[0, 0]])))


def test_val_batches_on_cpu():
    """the validation variant needs no kernel: patch == final patch, no augmentation, -1 -> 0"""
    ds = cpu_dataset(True)
    tb = DL.TrainBatches(ds, (64, 72), 5, all_labels=LABELS, ignore_label=IGNORE, seed=2, val=True)
    x, t = next(tb)
    d, a = tb.last_draw
    assert a is None and tb.loader.patch_size == (64, 72) and tb.augment is None
    data, seg = tb.loader.assemble(d)
    assert torch.equal(x, data) and t.dtype == torch.int64 and tuple(t.shape) == (5, 1, 64, 72)
    assert (seg == -1).any() and not (t < 0).any() and torch.equal(t, seg.long().clamp(min=0))
    tb = DL.TrainBatches(ds, (64, 72), 5, all_labels=LABELS, ignore_label=IGNORE, regions=[(1, 2), 2], seed=2, val=True)
    _, r = next(tb)
    assert r.dtype == torch.uint8 and tuple(r.shape) == (5, 3, 64, 72)
    assert torch.equal(r[:, 0], ((t[:, 0] == 1) | (t[:, 0] == 2)).to(torch.uint8)) and torch.equal(r[:, 2], (t[:, 0] == IGNORE).to(torch.uint8))
