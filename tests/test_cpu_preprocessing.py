"""The restatements of dinounet_amd.preprocessing (what CPU tensors run, and what tests/test_gpu_preprocessing.py compares the kernels
against) checked against independent code: a brute-force flood fill and scipy.ndimage.binary_fill_holes, scipy.ndimage.zoom for both
resampling orders, and the reference's normalisation recipes typed out in numpy.  No GPU.

The reference's own preprocessing cannot be imported (skimage, acvl_utils and batchgenerators are not vendored); what those packages
compute is restated in the module docstring of dinounet_amd.preprocessing."""
import collections

import numpy as np
import pytest
import torch
from scipy import ndimage

from dinounet_amd import export as EX
from dinounet_amd import preprocessing as P

PATTERNS = ["shells", "serpentine_open", "serpentine_closed", "tile_face_hole", "diagonal_leak", "faces", "noise"]


def make_mask(pattern, shape, seed=0):
    """bool (D, H, W): the NON-ZERO voxels of a test case.  Never empty."""
    D, H, W = shape
    rng = np.random.RandomState(seed + 17 * D + H + 3 * W)
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    zm = D // 2
    if pattern == "shells":                       # nested box shells, two voxels apart: every second gap is a hole inside a hole
        dist = np.full(shape, 1 << 20)
        for idx, n in ((z, D), (y, H), (x, W)):
            if n > 2:                             # an axis of extent <= 2 has no interior: the shells are drawn in the other axes
                dist = np.minimum(dist, np.minimum(idx, n - 1 - idx))
        m = dist % 4 == 1 if (dist < (1 << 20)).any() and (dist % 4 == 1).any() else np.ones(shape, dtype=bool)
    elif pattern in ("serpentine_open", "serpentine_closed"):
        # a solid block with one snake of zero voxels in the middle slice; "open": its far end alone reaches the face x = W - 1
        m = np.ones(shape, dtype=bool)
        rows = list(range(1, H - 1, 2))
        for i, r in enumerate(rows):
            m[zm, r, 1:W - 1] = False
            if i + 1 < len(rows) and r + 1 < H - 1:
                m[zm, r + 1, W - 2 if i % 2 == 0 else 1] = False
        if pattern == "serpentine_open" and rows:
            m[zm, rows[-1], W - 1] = False
    elif pattern == "tile_face_hole":             # one box of zeros across the tile faces x = 64, y = 8, z = 4, closed on every side
        m = np.ones(shape, dtype=bool)
        m[max(1, min(2, D - 2)):max(1, min(6, D - 1)), 6:min(10, H - 1), 60:min(70, W - 1)] = False
    elif pattern == "diagonal_leak":              # a zero voxel that meets the zero corner voxel only across an edge: it is a hole
        m = np.ones(shape, dtype=bool)
        m[zm, 0, 0] = False
        if H > 1 and W > 1:
            m[zm, 1, 1] = False
        if H > 2 and W > 1:                       # and one that does leak, through a face neighbour
            m[zm, H - 1, W - 1] = False
            m[zm, H - 2, W - 1] = False
    elif pattern == "faces":                      # a mask that touches every face, random inside
        m = rng.random_sample(shape) < 0.55
        m[0], m[-1], m[:, 0], m[:, -1], m[:, :, 0], m[:, :, -1] = True, True, True, True, True, True
    elif pattern == "noise":
        m = rng.random_sample(shape) < 0.62       # above the site-percolation threshold of the complement: many enclosed pockets
    else:
        raise KeyError(pattern)
    if not m.any():
        m = np.ones(shape, dtype=bool)
    return m


def make_data(pattern, shape, channels, dtype=np.float32, seed=0):
    """(C, D, H, W): non-zero exactly on make_mask, every voxel of it in one random channel or in all"""
    m = make_mask(pattern, shape, seed)
    rng = np.random.RandomState(seed + 5)
    owner = rng.randint(0, channels + 1, size=shape)          # `channels` = every channel
    vals = rng.randint(1, 120, size=(channels, *shape)) * rng.choice([-1, 1], size=(channels, *shape))
    if np.dtype(dtype) == np.uint8:
        vals = np.abs(vals)
    data = np.zeros((channels, *shape), dtype=dtype)
    for c in range(channels):
        on = m & ((owner == c) | (owner == channels))
        data[c][on] = vals[c][on].astype(dtype)
    return data


def make_seg(shape, seed=0):
    rng = np.random.RandomState(seed + 9)
    return rng.choice(np.array([0, 0, 1, 2, 126], dtype=np.int16), size=(1, *shape))


def flood_fill_holes(mask):
    """brute force: the zero voxels reached from the faces through 6 neighbours stay zero, every other voxel is in the result"""
    D, H, W = mask.shape
    reach = np.zeros(mask.shape, dtype=bool)
    todo = collections.deque()
    for z in range(D):
        for y in range(H):
            for x in range(W):
                if (z in (0, D - 1) or y in (0, H - 1) or x in (0, W - 1)) and not mask[z, y, x]:
                    reach[z, y, x] = True
                    todo.append((z, y, x))
    while todo:
        z, y, x = todo.popleft()
        for dz, dy, dx in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
            a, b, c = z + dz, y + dy, x + dx
            if 0 <= a < D and 0 <= b < H and 0 <= c < W and not mask[a, b, c] and not reach[a, b, c]:
                reach[a, b, c] = True
                todo.append((a, b, c))
    return ~reach


# ------------------------------------------------------------------------------------------------ fill holes
@pytest.mark.parametrize("shape", [(1, 20, 70), (2, 9, 67), (3, 16, 70), (5, 37, 131), (1, 1, 1), (2, 2, 2)], ids=str)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_fill_holes_matches_flood_fill_and_scipy(pattern, shape):
    m = make_mask(pattern, shape)
    got = P._fill_holes_numpy(m)
    assert np.array_equal(got, flood_fill_holes(m))
    assert np.array_equal(got, ndimage.binary_fill_holes(m))
    data = torch.from_numpy(make_data(pattern, shape, 3))
    assert np.array_equal(P.create_nonzero_mask(data).numpy(), got)
    if shape[0] <= 2:
        assert np.array_equal(got, m), "with D <= 2 every voxel lies on a z face: nothing may be filled"


def test_fill_holes_depth_1_2_3():
    for D in (1, 2, 3):
        m = np.ones((D, 9, 9), dtype=bool)
        m[D // 2, 4, 4] = False
        got = P._fill_holes_numpy(m)
        assert np.array_equal(got, ndimage.binary_fill_holes(m))
        assert bool(got[D // 2, 4, 4]) == (D == 3)


def test_fill_holes_patterns_do_what_they_say():
    shape = (5, 37, 131)
    filled = {p: int((P._fill_holes_numpy(make_mask(p, shape)) != make_mask(p, shape)).sum()) for p in PATTERNS}
    zeros = {p: int((~make_mask(p, shape)).sum()) for p in PATTERNS}
    print(filled, zeros)
    assert filled["serpentine_open"] == 0 and zeros["serpentine_open"] > 2000
    assert filled["serpentine_closed"] == zeros["serpentine_closed"] == zeros["serpentine_open"] - 1
    assert filled["tile_face_hole"] == zeros["tile_face_hole"] == 2 * 4 * 10        # z 2..3, y 6..9, x 60..69: across x = 64 and y = 8
    assert filled["diagonal_leak"] == 1 and zeros["diagonal_leak"] == 4
    assert filled["faces"] == zeros["faces"] > 0
    assert 0 < filled["noise"] < zeros["noise"]
    assert 0 < filled["shells"] < zeros["shells"]


# ------------------------------------------------------------------------------------------------ order 3
CUBIC_SIZES = [((9, 11), (13, 7)), ((64, 64), (64, 100)), ((1, 5), (3, 5)), ((2, 300), (5, 130)), ((130, 70), (65, 35)), ((3, 17), (8, 17)),
               ((20, 3), (11, 7))]


def spiky(shape, seed=0, offset=0.0):
    """nearly flat planes with one isolated spike each: a cubic spline rings next to it, below the minimum for a positive spike (even
    indices of the first axis) and above the maximum for a negative one (odd indices), so the clip acts, per plane and per volume.
    Every plane has its own amplitude, so the two scopes clip differently."""
    rng = np.random.RandomState(seed)
    planes = int(np.prod(shape[:-2]))
    amp = 1.0 + np.arange(planes).reshape(*shape[:-2], 1, 1)
    sign = np.where((np.arange(planes) // (planes // shape[0])) % 2 == 0, 1.0, -1.0).reshape(*shape[:-2])
    x = (0.05 * rng.randn(*shape) + offset) * amp
    H, W = shape[-2:]
    x[..., H // 2, W // 2] += 40.0 * sign * amp[..., 0, 0]
    return x


@pytest.mark.parametrize("hw,out", CUBIC_SIZES, ids=str)
def test_cubic_matches_scipy_zoom(hw, out):
    """the hand-written prefilter and taps against scipy.ndimage.zoom(order=3, mode='nearest', grid_mode=True) in fp64: 1e-12 max|x|"""
    x = spiky((2, *hw), seed=1, offset=3.0)
    got = P._resize_cubic_float64(x, out)
    want = np.stack([ndimage.zoom(p, (out[0] / hw[0], out[1] / hw[1]), order=3, mode="nearest", grid_mode=True) for p in x])
    err = float(np.abs(got - want).max() / np.abs(x).max())
    print(f"{hw} -> {out}: max |restatement - scipy| / max |x| = {err:.2e}")
    assert got.shape == want.shape == (2, *out)
    assert err <= 1e-12


@pytest.mark.parametrize("hw,out", [((9, 11), (13, 7)), ((64, 64), (64, 100)), ((130, 70), (65, 35)), ((2, 300), (5, 130))], ids=str)
def test_cubic_clip_scopes(hw, out):
    """resample_data_or_seg_to_shape against scipy: per slice (2-D zoom, clipped per slice) with an anisotropic axis 0, on the volume
    (3-D zoom with z unchanged, clipped per channel volume) otherwise.  Both sides round fp64 values that differ by at most
    1e-12 max|x| to fp32: they may land on neighbouring floats, one ulp of max|x| apart at the most."""
    x = spiky((2, 3, *hw), seed=2).astype(np.float32)
    t = torch.from_numpy(x)
    new_shape = (3, *out)
    zf = (out[0] / hw[0], out[1] / hw[1])
    x64 = x.astype(np.float64)
    tol = (1e-12 + 2.0 ** -23) * float(np.abs(x).max())
    per_slice = P.resample_data_or_seg_to_shape(t, new_shape, (5.0, 1.0, 1.0), (5.0, 0.7, 0.7)).numpy()
    want = np.stack([np.stack([np.clip(ndimage.zoom(s, zf, order=3, mode="nearest", grid_mode=True), s.min(), s.max()) for s in c])
                     for c in x64])
    assert per_slice.dtype == np.float32 and np.abs(per_slice - want).max() <= tol
    volume = P.resample_data_or_seg_to_shape(t, new_shape, (1.0, 1.0, 1.0), (1.0, 0.7, 0.7)).numpy()
    want_v = np.stack([np.clip(ndimage.zoom(c, (1.0, *zf), order=3, mode="nearest", grid_mode=True), c.min(), c.max()) for c in x64])
    assert np.abs(volume - want_v).max() <= tol
    raw = P._resize_cubic_float64(x64, out)
    assert (raw > x64.max(axis=(2, 3), keepdims=True)).any() or (raw < x64.min(axis=(2, 3), keepdims=True)).any(), "the clip never acted"
    assert not np.array_equal(per_slice, volume), "the two clip scopes must differ on slices of different range"
    # two anisotropic axes, or none: the volume rule (default_resampling.py:107-116)
    assert np.array_equal(P.resample_data_or_seg_to_shape(t, new_shape, (5.0, 5.0, 1.0), (5.0, 5.0, 0.7)).numpy(), volume)
    assert np.array_equal(P.resample_data_or_seg_to_shape(t, new_shape, (5.0, 1.0, 1.0), (5.0, 0.7, 0.7), force_separate_z=False).numpy(), volume)


def test_unchanged_shape_returns_the_input():
    t = torch.from_numpy(spiky((2, 3, 9, 11)).astype(np.float32))
    assert P.resample_data_or_seg_to_shape(t, (3, 9, 11), (1, 1, 1), (1, 1, 1)) is t
    s = torch.zeros((1, 3, 9, 11), dtype=torch.int16)
    assert P.resample_data_or_seg_to_shape(s, (3, 9, 11), (1, 1, 1), (1, 1, 1), is_seg=True, order=1) is s


# ------------------------------------------------------------------------------------------------ order 1, segmentation
SEG_SIZES = [((9, 11), (13, 7)), ((64, 64), (64, 100)), ((1, 5), (3, 5)), ((2, 300), (5, 130)), ((130, 70), (65, 35)), ((64, 64), (32, 32))]
SEG_LABELS = np.array([-1, 0, 1, 2, 126], dtype=np.int16)


def blocky_seg(shape, seed=0):
    """(D, H, W) int16 labels in patches of a few pixels plus single-pixel noise"""
    rng = np.random.RandomState(seed)
    D, H, W = shape
    coarse = rng.randint(0, len(SEG_LABELS), size=(D, (H + 3) // 4, (W + 4) // 5))
    seg = np.repeat(np.repeat(coarse, 4, axis=1), 5, axis=2)[:, :H, :W]
    noise = rng.random_sample(shape) < 0.1
    seg = np.where(noise, rng.randint(0, len(SEG_LABELS), size=shape), seg)
    return SEG_LABELS[seg]


def float_vote(seg, out):
    """resize_segmentation(order 1) as published: per label in ascending order, zoom of the one-hot map, painted where >= 0.5"""
    H, W = seg.shape[1:]
    res = np.zeros((seg.shape[0], *out), dtype=np.int16)
    for lab in np.unique(seg):
        r = np.stack([ndimage.zoom((s == lab).astype(np.float64), (out[0] / H, out[1] / W), order=1, mode="nearest", grid_mode=True)
                      for s in seg])
        res[r >= 0.5] = lab
    return res


def tie_pixels(seg, out):
    """bool (D, Ho, Wo): some label's exact weight equals 1/2, from the integers"""
    labels, weights = P._label_weights(seg, out)
    den = 4 * out[0] * out[1]
    tie = np.zeros(labels[0].shape, dtype=bool)
    for q in range(4):
        tot = sum(np.where(labels[r] == labels[q], weights[r][None], 0) for r in range(4))
        tie |= 2 * tot == den
    return tie


# sizes for the comparison with the float recipe.  The upper tap weight along an axis is ((2 o + 1) n_in - n_out) mod 2 n_out over 2 n_out:
# it is exactly 1/2 only if (2 o + 1) n_in is a multiple of 2 n_out, which an ODD n_in rules out; what is left are products that happen
# to add up to 1/2.  The pairs of SEG_SIZES with an even n_in (64 -> 100, 300 -> 130, 130 -> 65) tie at 4 % to 17 % of their pixels and
# are left to the integer comparison on the device.
FLOAT_VOTE_SIZES = [((9, 11), (13, 7)), ((1, 5), (3, 5)), ((65, 63), (51, 77)), ((3, 301), (5, 131)), ((131, 71), (67, 37)), ((31, 47), (45, 29))]


@pytest.mark.parametrize("hw,out", FLOAT_VOTE_SIZES, ids=str)
def test_integer_vote_matches_float_recipe(hw, out):
    """away from exact ties the two cannot differ: the nearest value to 1/2 that is not a tie is 1 / (4 Ho Wo) away, far above the
    rounding of four products in fp64.  Ties are counted from the integers and excluded; they must be rare."""
    seg = blocky_seg((3, *hw), seed=3)
    got = P._resize_seg_numpy(seg, out)
    want = float_vote(seg, out)
    tie = tie_pixels(seg, out)
    share = float(tie.mean())
    print(f"{hw} -> {out}: {int(tie.sum())} tie pixels of {tie.size}, {int((got != want).sum())} differing pixels")
    assert share <= 1e-3
    assert got.dtype == np.int16 and np.array_equal(got[~tie], want[~tie])
    t = P.resample_data_or_seg_to_shape(torch.from_numpy(seg[None]), (3, *out), (1, 1, 1), (1, 1, 1), is_seg=True, order=1)
    assert t.dtype == torch.int16 and np.array_equal(t.numpy()[0], got)


def test_integer_vote_at_dyadic_ties():
    """downsampling by 2: every output pixel is the mean of a 2 x 2 block, so two labels with two pixels each tie at exactly 1/2: both
    are painted (>=), the larger label last; -1 with two pixels of four is painted like any label.  One pixel of four never reaches 1/2: 0."""
    seg = np.array([[[1, 1, 2, 2, -1, -1, 126, 0], [2, 2, 1, 2, 2, 126, 1, 2]]], dtype=np.int16)
    got = P._resize_seg_numpy(seg, (1, 4))
    assert got.tolist() == [[[2, 2, -1, 0]]]
    assert np.array_equal(got, float_vote(seg, (1, 4)))                              # 1/2 and 1/4 are exact in floating point
    seg = blocky_seg((2, 64, 64), seed=4)
    assert tie_pixels(seg, (32, 32)).sum() > 50
    assert np.array_equal(P._resize_seg_numpy(seg, (32, 32)), float_vote(seg, (32, 32)))


def test_int_taps_are_source_taps():
    for n_in, n_out in [(9, 13), (11, 7), (1, 3), (300, 130), (64, 64)]:
        lo, hi, wa, wb = P._int_taps(n_in, n_out)
        a, b, w = EX.source_taps(n_in, n_out)
        assert np.array_equal(lo, a.numpy()) and np.array_equal(hi, b.numpy())
        assert np.array_equal(wb / (2.0 * n_out), w.numpy()) and np.array_equal(wa + wb, np.full(n_out, 2 * n_out))


# ------------------------------------------------------------------------------------------------ normalisation
INTENSITY = {"0": {"mean": 99.2, "std": 37.7, "percentile_00_5": -3.4, "percentile_99_5": 210.7}}


def ct_like(shape, seed=0):
    rng = np.random.RandomState(seed)
    return (rng.randn(*shape) * 80 + 60).astype(np.float32)


def reference_recipe(scheme, image, seg=None, use_mask=False, ip=None):
    """default_normalization_schemes.py, typed out: `image` float32, changed in place and returned"""
    if scheme == "NoNormalization":
        return image.astype(np.float32, copy=False)
    if scheme == "RGBTo01Normalization":
        assert image.min() >= 0 and image.max() <= 255
        image /= 255.
        return image
    if scheme == "CTNormalization":
        np.clip(image, ip["percentile_00_5"], ip["percentile_99_5"], out=image)
        image -= ip["mean"]
        image /= max(ip["std"], 1e-8)
        return image
    if scheme == "RescaleTo01Normalization":
        image -= image.min()
        image /= np.clip(image.max(), a_min=1e-8, a_max=None)
        return image
    if scheme == "ZScoreNormalization":
        if use_mask:
            mask = seg >= 0
            mean = image[mask].mean()
            std = image[mask].std()
            image[mask] = (image[mask] - mean) / (max(std, 1e-8))
        else:
            mean = image.mean()
            std = image.std()
            image -= mean
            image /= (max(std, 1e-8))
        return image
    raise KeyError(scheme)


@pytest.mark.parametrize("scheme", ["NoNormalization", "RGBTo01Normalization", "CTNormalization", "RescaleTo01Normalization"])
def test_fp32_schemes_equal_the_reference_recipe(scheme):
    shape = (1, 3, 37, 53)
    x = ct_like(shape, 5)
    if scheme == "RGBTo01Normalization":
        x = np.random.RandomState(6).randint(0, 256, size=shape).astype(np.float32)
    want = reference_recipe(scheme, x[0].copy(), ip=INTENSITY["0"])
    t = torch.from_numpy(x.copy())
    got = P.normalize(t, None, [scheme], [False], INTENSITY)
    assert got is t and got.dtype == torch.float32
    assert np.array_equal(got.numpy()[0].view(np.uint32), want.view(np.uint32))
    if scheme != "NoNormalization":
        assert not np.array_equal(got.numpy(), x)


def test_rescale_of_a_constant_channel_and_rgb_range():
    t = torch.full((1, 1, 4, 5), 3.5)
    assert np.array_equal(P.normalize(t, None, ["RescaleTo01Normalization"], [False], None).numpy(), np.zeros((1, 1, 4, 5), np.float32))
    for bad in (-1.0, 256.0):
        t = torch.zeros((1, 1, 4, 5))
        t[0, 0, 1, 1] = bad
        with pytest.raises(ValueError):
            P.normalize(t, None, ["RGBTo01Normalization"], [False], None)


@pytest.mark.parametrize("use_mask", [False, True])
def test_zscore_fp64_against_numpy_float32(use_mask):
    """the distance is numpy's own float32 summation error (pairwise sums of 1000-offset data): printed, recorded in DESIGN 3e, not
    asserted beyond a sanity bound.  The fp64 restatement itself is checked against a two-pass formula written with math.fsum."""
    import math
    shape = (1, 5, 37, 131)
    x = (np.random.RandomState(7).randn(*shape) + 1000.0).astype(np.float32)
    seg = np.where(np.random.RandomState(8).random_sample(shape) < 0.3, -1, 0).astype(np.int16)
    want32 = reference_recipe("ZScoreNormalization", x[0].copy(), seg[0], use_mask)
    t = torch.from_numpy(x.copy())
    got = P.normalize(t, torch.from_numpy(seg), ["ZScoreNormalization"], [use_mask], None).numpy()[0]
    sel = x[0][seg[0] >= 0] if use_mask else x[0].ravel()
    mean = math.fsum(sel.astype(np.float64)) / sel.size
    std = math.sqrt(math.fsum((sel.astype(np.float64) - mean) ** 2) / sel.size)
    exact = ((x[0].astype(np.float64) - mean) / max(std, 1e-8)).astype(np.float32)
    if use_mask:
        exact[seg[0] < 0] = x[0][seg[0] < 0]
        assert np.array_equal(got[seg[0] < 0], x[0][seg[0] < 0]), "voxels outside the mask must keep their bits"
    err = np.abs(got.astype(np.float64) - exact).max()
    dist = float(np.abs(got.astype(np.float64) - want32).max())
    print(f"ZScore (mask {use_mask}): max |fp64 restatement - numpy float32 recipe| = {dist:.3e}; against fsum = {err:.3e}")
    assert err <= 2.0 ** -23 * np.abs(exact).max()
    assert dist < 1e-2


def test_zscore_single_voxel_and_constant():
    x = ct_like((1, 2, 5, 7), 9)
    seg = np.full((1, 2, 5, 7), -1, dtype=np.int16)
    seg[0, 1, 2, 3] = 0
    got = P.normalize(torch.from_numpy(x.copy()), torch.from_numpy(seg), ["ZScoreNormalization"], [True], None).numpy()
    want = x.copy()
    want[0, 1, 2, 3] = 0.0
    assert np.array_equal(got, want)
    got = P.normalize(torch.full((1, 2, 5, 7), 7.0), None, ["ZScoreNormalization"], [False], None).numpy()
    assert np.array_equal(got, np.zeros((1, 2, 5, 7), np.float32))


# ------------------------------------------------------------------------------------------------ run_case
def raw_case(shape, frame, channels=1, seed=0):
    """(C, *shape) float32 image that is zero on a frame of `frame` voxels per axis (where the axis is longer than 2 frames) and has a
    few zero pockets inside; seg (1, *shape) int16, labels 0..2, zero wherever the image is zero"""
    rng = np.random.RandomState(seed)
    img = (rng.randint(1, 200, size=(channels, *shape))).astype(np.float32)
    inner = tuple(slice(f, n - f) if n > 2 * f else slice(None) for n, f in zip(shape, frame))
    keep = np.zeros(shape, dtype=bool)
    keep[inner] = True
    pockets = rng.random_sample(shape) < 0.02
    img[:, ~keep | pockets] = 0
    seg = rng.randint(0, 3, size=(1, *shape)).astype(np.int16)
    seg[:, ~keep] = 0
    return img, seg


def test_run_case_properties_and_round_trip():
    """no resampling: the one-hot logits of the preprocessed segmentation, exported with the properties run_case filled, are the raw
    segmentation again (transpose, crop and their inverses fit each other and export.py)"""
    img, seg = raw_case((6, 40, 50), (1, 5, 7), channels=2, seed=1)
    props = {"spacing": (1.0, 2.5, 1.0)}
    tf = (1, 0, 2)
    data, s = P.run_case(torch.from_numpy(img), torch.from_numpy(seg), props, transpose_forward=tf, spacing=[2.5, 1.0, 1.0],
                         normalization_schemes=["ZScoreNormalization", "NoNormalization"], use_mask_for_norm=[True, False],
                         foreground_intensity_properties_per_channel=None)
    assert props["shape_before_cropping"] == (40, 6, 50)
    assert props["bbox_used_for_cropping"] == [[5, 35], [1, 5], [7, 43]]
    assert props["shape_after_cropping_and_before_resampling"] == (30, 4, 36)
    assert data.dtype == torch.float32 and tuple(data.shape) == (2, 30, 4, 36)
    assert s.dtype == torch.int16 and tuple(s.shape) == (1, 30, 4, 36)
    assert int(s.min()) >= -1
    assert np.array_equal(data[1].numpy(), img[1].transpose(1, 0, 2)[5:35, 1:5, 7:43])   # NoNormalization: the cropped bits
    lab = s[0].clamp(min=0).long()
    logits = torch.nn.functional.one_hot(lab, 3).permute(3, 0, 1, 2).float().contiguous()
    back = EX.logits_to_segmentation(logits, properties=props, transpose_backward=[tf.index(i) for i in range(3)])
    assert back.dtype == torch.uint8 and tuple(back.shape) == (6, 40, 50)
    assert np.array_equal(back.numpy(), seg[0].astype(np.uint8))


def test_run_case_without_seg_and_2d_spacing():
    img, _ = raw_case((1, 70, 150), (0, 6, 9), channels=3, seed=2)
    raw = img.copy()
    props = {"spacing": (999.0, 1.0, 1.0)}
    data, s = P.run_case(torch.from_numpy(img), None, props, transpose_forward=(0, 1, 2), spacing=[1.25, 0.8],
                         normalization_schemes=["ZScoreNormalization"] * 3, use_mask_for_norm=[False] * 3,
                         foreground_intensity_properties_per_channel=None)
    assert np.array_equal(img, raw), "the input was modified"
    assert props["bbox_used_for_cropping"] == [[0, 1], [6, 64], [9, 141]]
    new = P.compute_new_shape((1, 58, 132), (999.0, 1.0, 1.0), (999.0, 1.25, 0.8))
    assert new == [1, 46, 165] and tuple(data.shape) == (3, *new) and tuple(s.shape) == (1, *new)
    assert set(np.unique(s.numpy())) <= {-1, 0} and (s.numpy() == 0).mean() > 0.9
    plans = {"transpose_forward": [0, 1, 2], "foreground_intensity_properties_per_channel": {},
             "configurations": {"base": {"spacing": [1.25, 0.8], "normalization_schemes": ["ZScoreNormalization"] * 3,
                                         "use_mask_for_norm": [False] * 3,
                                         "resampling_fn_data_kwargs": {"is_seg": False, "order": 3, "order_z": 0, "force_separate_z": None}},
                                "2d": {"inherits_from": "base"}}}
    props2 = {"spacing": (999.0, 1.0, 1.0)}
    data2, s2 = P.run_case_from_plans(torch.from_numpy(img), None, props2, plans, "2d")
    assert torch.equal(data, data2) and torch.equal(s, s2) and props == props2


def test_compute_new_shape_rounds_like_python():
    assert P.compute_new_shape((10, 5, 7), (1.0, 1.0, 1.0), (1.0, 2.0, 2.0)) == [10, 2, 4]      # round(2.5) = 2, round(3.5) = 4


def test_value_errors():
    img, seg = raw_case((4, 20, 24), (1, 2, 2), seed=3)
    kw = dict(transpose_forward=(0, 1, 2), spacing=[1.0, 1.0, 1.0], normalization_schemes=["NoNormalization"], use_mask_for_norm=[False],
              foreground_intensity_properties_per_channel=None)
    t = torch.from_numpy(img)
    with pytest.raises(ValueError):                                                  # an all-zero case
        P.run_case(torch.zeros_like(t), None, {"spacing": (1, 1, 1)}, **kw)
    with pytest.raises(ValueError):
        P.crop_to_nonzero(torch.zeros_like(t))
    with pytest.raises(ValueError):                                                  # the number of slices would change
        P.run_case(t, None, {"spacing": (2.0, 1.0, 1.0)}, **kw)
    with pytest.raises(ValueError):                                                  # separate z along axis 2
        P.resample_data_or_seg_to_shape(t, (4, 20, 30), (1.0, 1.0, 5.0), (1.0, 1.0, 4.0))
    with pytest.raises(ValueError):
        P.resample_data_or_seg_to_shape(t, (5, 20, 24), (1.0, 1.0, 1.0), (1.0, 1.0, 1.0))
    for is_seg, order in ((False, 1), (True, 3), (False, 0), (True, 0)):
        with pytest.raises(ValueError):
            P.resample_data_or_seg_to_shape(t, (4, 20, 30), (1, 1, 1), (1, 1, 1), is_seg=is_seg, order=order)
    with pytest.raises(ValueError):
        P.run_case(t, None, {"spacing": (1, 1, 1)}, **{**kw, "normalization_schemes": ["NoSuchNormalization"]})
    with pytest.raises(ValueError):
        P.run_case(t, None, {"spacing": (1, 1, 1)}, **{**kw, "normalization_schemes": ["CTNormalization"]})
    with pytest.raises(ValueError):
        P.run_case(t, None, {"spacing": (1, 1, 1)}, **{**kw, "transpose_forward": (0, 1, 1)})
    with pytest.raises(ValueError):
        P.run_case(t, torch.from_numpy(seg[:, :3]), {"spacing": (1, 1, 1)}, **kw)
    with pytest.raises(ValueError):
        P.crop_to_nonzero(t.to(torch.int64))


def test_predict_from_raw_is_part_of_inference():
    from dinounet_amd import inference
    assert inference.predict_from_raw is P.predict_from_raw
