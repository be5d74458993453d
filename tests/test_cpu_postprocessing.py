"""CPU tests of dinounet_amd.postprocessing: the scipy restatement of "keep only the largest 26-connected component" against a brute-force
flood fill, remove_all_but_largest_component_from_segmentation, apply_postprocessing and the search determine_postprocessing on hand-built
cases.  Everything is integer: every comparison is equality.  The GPU tests (tests/test_gpu_postprocessing.py) compare csrc/cc.hip against
the path checked here and reuse the patterns and hand cases of this file."""
import itertools
import math

import numpy as np
import pytest
import torch

from dinounet_amd import postprocessing as PP

REMOVE = PP.remove_all_but_largest_component_from_segmentation


# ------------------------------------------------------------------------------------------------ brute force
def flood_fill(mask):
    """ids int32 (id = smallest linear index of the component, -1 outside), {id: size}: an explicit 26-neighbour stack"""
    D, H, W = mask.shape
    ids = np.full(mask.shape, -1, dtype=np.int32)
    sizes = {}
    offs = [o for o in itertools.product((-1, 0, 1), repeat=3) if o != (0, 0, 0)]
    for z, y, x in itertools.product(range(D), range(H), range(W)):          # raster order: the first voxel met has the smallest index
        if not mask[z, y, x] or ids[z, y, x] >= 0:
            continue
        cid = (z * H + y) * W + x
        ids[z, y, x] = cid
        stack, n = [(z, y, x)], 0
        while stack:
            cz, cy, cx = stack.pop()
            n += 1
            for dz, dy, dx in offs:
                nz, ny, nx = cz + dz, cy + dy, cx + dx
                if 0 <= nz < D and 0 <= ny < H and 0 <= nx < W and mask[nz, ny, nx] and ids[nz, ny, nx] < 0:
                    ids[nz, ny, nx] = cid
                    stack.append((nz, ny, nx))
        sizes[cid] = n
    return ids, sizes


def largest_of(sizes):
    """explicit tie rule: most voxels, then the smallest id"""
    best = -1
    for cid in sorted(sizes):
        if best < 0 or sizes[cid] > sizes[best]:
            best = cid
    return best


@pytest.mark.parametrize("density", [0.1, 0.3, 0.6])
@pytest.mark.parametrize("shape", [(12, 12, 12), (1, 9, 11), (5, 7, 12), (3, 1, 10), (1, 1, 12), (2, 2, 2), (1, 1, 1)])
def test_restatement_against_flood_fill(shape, density):
    rng = np.random.default_rng(7 + shape[0] * 100 + shape[2] + int(density * 10))
    for _ in range(3):
        mask = rng.random(shape) < density
        seg = torch.from_numpy(mask.astype(np.uint8))
        ids, stats = PP.component_ids(seg, 1)
        want_ids, sizes = flood_fill(mask)
        assert ids.dtype == torch.int32 and np.array_equal(ids.numpy(), want_ids)
        best = largest_of(sizes)
        assert stats == {"n_components": len(sizes), "largest_size": sizes.get(best, 0), "largest_id": best}
        got_sizes = dict(zip(*np.unique(ids.numpy()[ids.numpy() >= 0], return_counts=True)))
        assert got_sizes == sizes
        kept = REMOVE(seg, 1).numpy()
        assert np.array_equal(kept, (mask & (want_ids == best)).astype(np.uint8) if sizes else seg.numpy())


def test_tie_keeps_first_in_raster_order():
    seg = torch.zeros((3, 6, 9), dtype=torch.uint8)
    seg[2, 4:6, 0:2] = 1                                   # 4 voxels, later in raster order
    seg[0, 1:3, 6:8] = 1                                   # 4 voxels, first
    seg[1, 5, 4] = 1                                       # 1 voxel, not adjacent to either (dy = 2 / dx = 2 away)
    ids, stats = PP.component_ids(seg, 1)
    assert stats == {"n_components": 3, "largest_size": 4, "largest_id": (0 * 6 + 1) * 9 + 6}
    out = REMOVE(seg, 1)
    want = torch.zeros_like(seg)
    want[0, 1:3, 6:8] = 1
    assert torch.equal(out, want)
    _, sizes = flood_fill(seg.numpy() == 1)
    assert largest_of(sizes) == stats["largest_id"]


# ------------------------------------------------------------------------------------------------ patterns shared with the GPU tests
def serpentine_slice(H, W):
    """even rows full, odd rows one voxel at alternating ends: one 8-connected component through every row"""
    m = np.zeros((H, W), dtype=bool)
    m[0::2] = True
    for y in range(1, H, 2):
        m[y, W - 1 if (y // 2) % 2 == 0 else 0] = True
    return m


def triangle(t, D):
    return 0 if D == 1 else (D - 1) - abs(t % (2 * D - 2) - (D - 1))


def make_mask(pattern, shape, seed=0):
    """bool (D, H, W) test masks"""
    D, H, W = shape
    rng = np.random.default_rng(1000 + seed + D * 7 + H * 3 + W)
    m = np.zeros(shape, dtype=bool)
    if pattern.startswith("random"):
        m = rng.random(shape) < float(pattern[6:])
    elif pattern == "serpentine":                          # even slices snake, odd slices hold one connecting voxel
        m[0::2] = serpentine_slice(H, W)
        m[1::2, 0, 0] = True
    elif pattern == "two_serpentines":                     # equal sizes in slices 0 and 2, slice 1 empty
        m[0] = serpentine_slice(H, W)
        m[2] = serpentine_slice(H, W)
    elif pattern in ("diagonal", "antidiagonal", "diagonals"):
        for t in range(min(H, W)):
            if pattern != "antidiagonal":
                m[triangle(t, D), t, t] = True
            if pattern != "diagonal":
                m[triangle(t, D), t, W - 1 - t] = True
    elif pattern == "full":
        m[:] = True
    elif pattern == "empty":
        pass
    elif pattern == "far_blob":                            # isolated single voxels on a stride-3 lattice, one 3^3 blob at the far corner
        m[0::3, 0::3, 0::3] = True
        m[max(D - 5, 0):, max(H - 5, 0):, max(W - 5, 0):] = False
        m[max(D - 3, 0):, max(H - 3, 0):, max(W - 3, 0):] = True
    else:
        raise KeyError(pattern)
    return m


PATTERNS = ["random0.05", "random0.25", "random0.6", "serpentine", "diagonal", "antidiagonal", "diagonals", "full", "empty", "far_blob"]


@pytest.mark.parametrize("pattern", PATTERNS)
def test_patterns_against_flood_fill(pattern):
    mask = make_mask(pattern, (5, 11, 12))
    ids, stats = PP.component_ids(torch.from_numpy(mask.astype(np.uint8)), 1)
    want_ids, sizes = flood_fill(mask)
    assert np.array_equal(ids.numpy(), want_ids)
    assert stats["n_components"] == len(sizes) and stats["largest_id"] == largest_of(sizes)
    if pattern == "serpentine":
        assert stats["n_components"] == 1


def test_two_serpentines_tie():
    mask = make_mask("two_serpentines", (3, 40, 130))
    seg = torch.from_numpy(mask.astype(np.uint8))
    _, stats = PP.component_ids(seg, 1)
    assert stats == {"n_components": 2, "largest_size": 2620, "largest_id": 0}
    out = REMOVE(seg, 1)
    assert torch.equal(out[0], seg[0]) and int(out[1:].sum()) == 0


# ------------------------------------------------------------------------------------------------ the remove function
def label_map(shape, seed=3):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.choice(np.array([0, 1, 2, 3, 5, 200], dtype=np.uint8), size=shape, p=[0.75, 0.06, 0.06, 0.05, 0.04, 0.04]))


def expected_remove(seg, labels, background_label=0):
    """from the flood fill: labels = the plain labels whose union is the mask"""
    s = seg.numpy()
    mask = np.isin(s, [l for l in labels if l < 64])
    ids, sizes = flood_fill(mask)
    out = s.copy()
    if sizes:
        out[mask & (ids != largest_of(sizes))] = background_label
    return out


@pytest.mark.parametrize("lor,labels", [(1, [1]), ((2, 3), [2, 3]), ([1, (2, 3)], [1, 2, 3]), ([5, 1], [1, 5]), ([1, 200], [1]), ([(1, 200), 3], [1, 3])])
def test_remove_unions_and_leaves_other_labels(lor, labels):
    seg = label_map((4, 10, 12))
    before = seg.clone()
    out = REMOVE(seg, lor)
    assert torch.equal(seg, before), "the input was modified"
    assert out.data_ptr() != seg.data_ptr() and out.dtype == torch.uint8 and out.shape == seg.shape
    assert np.array_equal(out.numpy(), expected_remove(seg, labels))
    outside = ~np.isin(seg.numpy(), labels)
    assert np.array_equal(out.numpy()[outside], seg.numpy()[outside])
    assert (out.numpy() != seg.numpy()).any()


def test_remove_background_label():
    seg = label_map((3, 9, 14), seed=5)
    out = REMOVE(seg, [1, 2], background_label=7)
    assert np.array_equal(out.numpy(), expected_remove(seg, [1, 2], 7))
    assert (out == 7).any() and not (seg == 7).any()


def test_label_above_63_is_in_no_mask_and_empty_mask_copies():
    seg = label_map((3, 9, 14), seed=6)
    assert (seg == 200).any()
    for lor in (200, [200, 64], (64, 255), 4):             # 4: a label that is not in the map
        out = REMOVE(seg, lor, background_label=9)
        assert torch.equal(out, seg) and out.data_ptr() != seg.data_ptr()
        ids, stats = PP.component_ids(seg, lor)
        assert int((ids != -1).sum()) == 0 and stats == {"n_components": 0, "largest_size": 0, "largest_id": -1}


def test_remove_2d_case_is_8_connected():
    seg = torch.zeros((1, 5, 5), dtype=torch.uint8)
    seg[0, 0, 0] = seg[0, 1, 1] = seg[0, 2, 2] = 1         # one diagonal component of 3
    seg[0, 4, 0] = seg[0, 4, 1] = 1                        # 2 voxels, two rows from the diagonal
    out = REMOVE(seg, 1)
    assert int(out.sum()) == 3 and int(out[0, 4].sum()) == 0


def test_validation():
    seg = torch.zeros((2, 3, 4), dtype=torch.uint8)
    for bad in (seg.float(), seg[0], seg[:0], seg.numpy()):
        with pytest.raises(ValueError):
            REMOVE(bad, 1)
        with pytest.raises(ValueError):
            PP.component_ids(bad, 1)
    for lor in ([], ()):
        with pytest.raises(ValueError):
            REMOVE(seg, lor)
    for bg in (-1, 256):
        with pytest.raises(ValueError):
            REMOVE(seg, 1, background_label=bg)
    big = torch.zeros(1, dtype=torch.uint8).expand(2048, 1024, 1024)          # 2^31 voxels, one byte of memory
    with pytest.raises(ValueError):
        REMOVE(big, 1)
    with pytest.raises(ValueError):
        PP.component_ids(big, 1)


def test_apply_postprocessing_chains_in_order():
    seg = label_map((3, 9, 14), seed=8)
    fns, kw = [REMOVE, REMOVE], [{"labels_or_regions": [1, 2]}, {"labels_or_regions": 3, "background_label": 2}]
    assert torch.equal(PP.apply_postprocessing(seg, fns, kw), REMOVE(REMOVE(seg, [1, 2]), 3, background_label=2))
    assert PP.apply_postprocessing(seg, [], []) is seg


# ------------------------------------------------------------------------------------------------ determine_postprocessing, hand-built
HAND_SHAPE = (2, 12, 20)


def _blank():
    return torch.zeros(HAND_SHAPE, dtype=torch.uint8)


def hand_case(name):
    """-> dict(preds, refs, labels, foreground, kwargs = the expected pp_fn_kwargs, final = the expected searched maps)"""
    if name == "i":        # two adjacent blobs (one foreground component) plus isolated false positives of both labels: step 1 is adopted
        r0, r1 = _blank(), _blank()
        r0[:, 2:6, 2:6], r0[:, 2:6, 6:10] = 1, 2
        r1[:, 5:9, 8:12], r1[:, 5:9, 12:16] = 1, 2
        p0, p1 = r0.clone(), r1.clone()
        p0[0, 10, 15], p0[1, 9, 18] = 1, 2
        p1[0, 0, 0], p1[1, 11, 1] = 2, 1
        return dict(preds=[p0, p1], refs=[r0, r1], labels=[1, 2], foreground=[1, 2], kwargs=[{"labels_or_regions": [1, 2]}], final=[r0, r1])
    if name == "ii":       # the reference has two true blobs of label 1: removing the smaller hurts label 1, nothing is adopted
        r = _blank()
        r[:, 1:5, 1:5], r[:, 1:5, 5:8], r[:, 8:11, 12:15] = 1, 2, 1
        p = r.clone()
        return dict(preds=[p], refs=[r], labels=[1, 2], foreground=[1, 2], kwargs=[], final=[p])
    if name == "iii":      # separate blobs: step 1 would delete whole labels; labels 1 and 2 lose a false positive each, label 3 has two blobs
        r = _blank()
        r[:, 0:3, 0:3], r[:, 0:3, 8:12], r[:, 6:9, 0:3], r[:, 8:12, 10:14] = 1, 2, 3, 3
        p = r.clone()
        p[0, 11, 19], p[1, 5, 17] = 1, 2
        return dict(preds=[p], refs=[r], labels=[1, 2, 3], foreground=[1, 2, 3],
                    kwargs=[{"labels_or_regions": 1}, {"labels_or_regions": 2}], final=[r])
    if name == "iv":       # label 3 is in no case: its mean and the foreground mean are nan, every comparison with them is false
        r = _blank()
        r[:, 0:3, 0:3], r[:, 6:9, 8:12] = 1, 2
        p = r.clone()
        p[1, 11, 19] = 1
        return dict(preds=[p], refs=[r], labels=[1, 2, 3], foreground=[1, 2, 3], kwargs=[{"labels_or_regions": 1}], final=[r])
    if name == "v":        # one label: step 1 only
        r = _blank()
        r[:, 3:8, 4:9] = 1
        p = r.clone()
        p[0, 11, 0] = 1
        return dict(preds=[p], refs=[r], labels=[1], foreground=[1], kwargs=[{"labels_or_regions": [1]}], final=[r])
    raise KeyError(name)


def same_number(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))


def same_report(a, b):
    if list(a) != list(b) or a["postprocessing_fns"] != b["postprocessing_fns"] or a["postprocessing_kwargs"] != b["postprocessing_kwargs"]:
        return False
    for part in ("input_folder", "postprocessed"):
        if list(a[part]["mean"]) != list(b[part]["mean"]):
            return False
        if not same_number(a[part]["foreground_mean"]["Dice"], b[part]["foreground_mean"]["Dice"]):
            return False
        if not all(same_number(a[part]["mean"][k]["Dice"], b[part]["mean"][k]["Dice"]) for k in a[part]["mean"]):
            return False
    return True


def run_search(case, device=None):
    preds = [p if device is None else p.to(device) for p in case["preds"]]
    refs = [r if device is None else r.to(device) for r in case["refs"]]
    fns, kwargs, report = PP.determine_postprocessing(preds, refs, case["labels"], case["foreground"])
    final = [PP.apply_postprocessing(p, fns, kwargs) for p in preds]
    return fns, kwargs, report, final


@pytest.mark.parametrize("name", ["i", "ii", "iii", "iv", "v"])
def test_determine_postprocessing_hand_cases(name):
    case = hand_case(name)
    before = [p.clone() for p in case["preds"]]
    fns, kwargs, report, final = run_search(case)
    assert kwargs == case["kwargs"]
    assert fns == [REMOVE] * len(kwargs)
    assert all(torch.equal(f, w) for f, w in zip(final, case["final"]))
    assert all(torch.equal(p, b) for p, b in zip(case["preds"], before)), "the predictions were modified"
    assert list(report) == ["input_folder", "postprocessed", "postprocessing_fns", "postprocessing_kwargs"]
    assert report["postprocessing_fns"] == ["remove_all_but_largest_component_from_segmentation"] * len(kwargs)
    assert report["postprocessing_kwargs"] == kwargs
    for part in ("input_folder", "postprocessed"):
        assert list(report[part]) == ["foreground_mean", "mean"]
        assert list(report[part]["mean"]) == [str(l) for l in case["labels"]]
        assert list(report[part]["foreground_mean"]) == ["Dice"]
    post, base = report["postprocessed"], report["input_folder"]
    if name == "iv":
        assert math.isnan(base["mean"]["3"]["Dice"]) and math.isnan(post["mean"]["3"]["Dice"])
        assert math.isnan(base["foreground_mean"]["Dice"]) and math.isnan(post["foreground_mean"]["Dice"])
        assert post["mean"]["1"]["Dice"] == 1.0 and base["mean"]["1"]["Dice"] == 2 * 18 / (2 * 18 + 1)
    elif name == "ii":
        assert post == base and base["foreground_mean"]["Dice"] == 1.0
    else:
        assert post["foreground_mean"]["Dice"] == 1.0 > base["foreground_mean"]["Dice"]
        assert all(post["mean"][k]["Dice"] >= base["mean"][k]["Dice"] for k in post["mean"])
    if name == "i":        # nanmean over the two cases of 2 tp / (2 tp + fp + fn): label 1 has 32 voxels and one false positive in each
        assert base["mean"]["1"]["Dice"] == np.mean([64 / 65, 64 / 65])
        assert base["foreground_mean"]["Dice"] == np.mean([base["mean"]["1"]["Dice"], base["mean"]["2"]["Dice"]])


def test_single_label_skips_step_2(monkeypatch):
    case = hand_case("v")
    calls = []

    def counting(seg, **kw):
        calls.append(kw)
        return REMOVE(seg, **kw)

    monkeypatch.setattr(PP, "remove_all_but_largest_component_from_segmentation", counting)
    PP.determine_postprocessing(case["preds"], case["refs"], case["labels"], case["foreground"])
    assert calls == [{"labels_or_regions": [1]}] * len(case["preds"])


def test_later_labels_see_the_updated_maps(monkeypatch):
    case = hand_case("iii")
    seen = []

    def recording(seg, **kw):
        seen.append((kw["labels_or_regions"], seg.clone()))
        return REMOVE(seg, **kw)

    monkeypatch.setattr(PP, "remove_all_but_largest_component_from_segmentation", recording)
    PP.determine_postprocessing(case["preds"], case["refs"], case["labels"], case["foreground"])
    assert [s[0] for s in seen] == [[1, 2, 3], 1, 2, 3]
    p, r = case["preds"][0], case["refs"][0]
    only_2 = r.clone()
    only_2[1, 5, 17] = 2                                   # the false positive of label 1 is gone, that of label 2 is still there
    assert torch.equal(seen[1][1], p) and torch.equal(seen[2][1], only_2) and torch.equal(seen[3][1], r)


def test_determine_postprocessing_regions_and_ignore_label():
    case = hand_case("i")
    fns, kwargs, report = PP.determine_postprocessing(case["preds"], case["refs"], [(1, 2), (2,)], [1, 2], ignore_label=None)
    assert kwargs[0] == {"labels_or_regions": [1, 2]} and list(report["postprocessed"]["mean"]) == ["(1, 2)", "(2,)"]
    assert report["postprocessed"]["foreground_mean"]["Dice"] == 1.0
    refs = [r.clone() for r in case["refs"]]
    for p, r in zip(case["preds"], refs):
        r[(p != 0) & (r == 0)] = 9                         # every false positive sits on an ignored voxel: nothing to gain
    assert PP.determine_postprocessing(case["preds"], refs, [1, 2], [1, 2], ignore_label=9)[1] == []
    with pytest.raises(ValueError):
        PP.determine_postprocessing(case["preds"], case["refs"][:1], [1, 2], [1, 2])
    with pytest.raises(ValueError):
        PP.determine_postprocessing([], [], [1, 2], [1, 2])
