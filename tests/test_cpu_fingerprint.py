"""dinounet_amd.fingerprint on CPU tensors: the numpy restatement of the device semantics against independent numpy -- np.percentile,
np.median, np.min, np.max and RandomState.choice themselves, which is what DatasetFingerprintExtractor calls
(dinounet/experiment_planning/dataset_fingerprint/fingerprint_extractor.py:42-80, :156-177).  Order statistics and samples are compared
to the bit (==, so -0.0 equals +0.0; the samples as int32 views); mean and std against math.fsum with derived bounds."""
import math

import numpy as np
import pytest
import torch

from dinounet_amd import fingerprint as FP
from dinounet_amd import preprocessing as PRE

SHAPE = (3, 10, 17)                                                                   # 510 voxels
N_FG = [0, 1, 2, 3, 199, 200, 201]
KEYS = {"mean", "median", "min", "max", "percentile_99_5", "percentile_00_5"}


def values(model, shape, seed):
    rng = np.random.RandomState(seed)
    if model == "ct":                                                                 # integer-valued: heavy with ties
        return rng.randint(-1024, 3072, shape).astype(np.float32)
    return (1000.0 + rng.randn(*shape)).astype(np.float32)                            # neighbouring floats


def labels(n_fg, seed, shape=SHAPE):
    """(1, *shape) int16 with exactly n_fg voxels from {1, 2, 70}, the rest from {-1, 0}"""
    rng = np.random.RandomState(seed)
    n = int(np.prod(shape))
    seg = rng.choice(np.array([-1, 0], np.int16), n)
    where = rng.permutation(n)[:n_fg]
    seg[where] = rng.choice(np.array([1, 2, 70], np.int16), n_fg)
    if n_fg >= 3:
        seg[where[:3]] = (1, 2, 70)
    return seg.reshape(1, *shape)


def fsum_mean_std(x):
    x = np.asarray(x, np.float64)
    mean = math.fsum(x.tolist()) / x.size                                             # lists: fsum over Python floats is several times faster
    return mean, math.sqrt(math.fsum(((x - mean) ** 2).tolist()) / x.size)


@pytest.mark.parametrize("n_fg", N_FG)
@pytest.mark.parametrize("model", ["ct", "gauss"])
def test_case_statistics_equal_numpy(model, n_fg):
    C = 2
    img = values(model, (C, *SHAPE), 10 + n_fg)
    seg = labels(n_fg, 20 + n_fg)
    assert int((seg > 0).sum()) == n_fg
    inten, stats = FP.collect_foreground_intensities(torch.from_numpy(seg), torch.from_numpy(img), num_samples=37)
    assert len(stats) == C and all(set(s) == KEYS for s in stats)
    if n_fg == 0:
        assert tuple(inten.shape) == (C, 0) and inten.dtype == torch.float32
        assert all(math.isnan(v) for s in stats for v in s.values())
        return
    assert tuple(inten.shape) == (C, 37)
    for c in range(C):
        fg = img[c][seg[0] > 0]
        s = stats[c]
        assert all(isinstance(v, float) for v in s.values())
        assert s["min"] == float(np.min(fg)) and s["max"] == float(np.max(fg))
        assert s["median"] == float(np.median(fg))
        assert s["percentile_00_5"] == float(np.percentile(fg, 0.5))
        assert s["percentile_99_5"] == float(np.percentile(fg, 99.5))
        mean, _ = fsum_mean_std(fg)
        if model == "ct":
            assert s["mean"] == mean                                                  # the sums are exact below 2^53
        else:
            assert abs(s["mean"] - mean) <= n_fg * 2.0 ** -52 * abs(mean)
        print(f"{model} n_fg={n_fg} c={c}: mean - np.mean(float32) = {s['mean'] - float(np.mean(fg)):.3e}")


@pytest.mark.parametrize("m", [50, 500])
def test_samples_equal_randomstate_choice(m):
    C, n_fg = 3, 201
    img = values("gauss", (C, *SHAPE), 3)
    seg = labels(n_fg, 4)
    inten, _ = FP.collect_foreground_intensities(torch.from_numpy(seg), torch.from_numpy(img), seed=1234, num_samples=m)
    rs = np.random.RandomState(1234)
    for c in range(C):
        want = rs.choice(img[c][seg[0] > 0], m, replace=True)
        assert np.array_equal(inten[c].numpy().view(np.int32), want.view(np.int32))
    other, _ = FP.collect_foreground_intensities(torch.from_numpy(seg), torch.from_numpy(img), seed=99, num_samples=m)
    assert not torch.equal(other, inten)


def test_virtual_index_is_a_rounded_float32_above_2_24():
    n = 2 ** 24 + 3
    x = (np.random.RandomState(5).standard_normal(n) * 1000).astype(np.float32)
    lo, hi, g = FP.virtual_index(10 ** 8, 99.5)
    assert (lo, hi, float(g)) == (99_500_000, 99_500_001, 0.0)                        # not 99 499 999.005
    _, stats = FP.collect_foreground_intensities(torch.ones((1, 1, 1, n), dtype=torch.int16), torch.from_numpy(x).reshape(1, 1, 1, n),
                                                 num_samples=4)
    s = np.sort(x)
    for name, q in (("percentile_00_5", 0.5), ("percentile_99_5", 99.5)):
        assert stats[0][name] == float(np.percentile(x, q))
        lo, hi, g = FP.virtual_index(n, q)
        exact = (n - 1) * q / 100
        print(f"q={q}: float32 virtual index {lo} + {float(g)} against the exact {exact}")
        assert float(FP.lerp(s[lo], s[hi], g)) == stats[0][name]
    assert stats[0]["median"] == float(np.median(x))


@pytest.mark.parametrize("model", ["ct", "gauss"])
def test_moments_against_fsum(model):
    n = 5003
    x = values(model, (2, n), 8)
    seg = np.where(np.random.RandomState(9).rand(n) < 0.6, 3, 0).astype(np.int16)
    rows = FP.foreground_moments(torch.from_numpy(x), torch.from_numpy(seg), with_std=True).numpy()
    for c in range(2):
        fg = x[c][seg > 0]
        k = fg.size
        mean, std = fsum_mean_std(fg)
        assert rows[c, 0] == k and rows[c, 1] == fg.min() and rows[c, 2] == fg.max() and rows[c, 4] == 0
        if model == "ct":
            assert rows[c, 3] / k == mean
        ours = math.sqrt(rows[c, 5] / k)
        assert abs(ours - std) <= k * 2.0 ** -52 * std                                # every one of the k additions rounds once
        print(f"{model} c={c}: mean - np.mean = {rows[c, 3] / k - float(np.mean(fg)):.3e}, std - np.std = {ours - float(np.std(fg)):.3e}")
    with_nan = x.copy()
    with_nan[1, np.flatnonzero(seg > 0)[7]] = np.nan
    rows = FP.foreground_moments(torch.from_numpy(with_nan), torch.from_numpy(seg)).numpy()
    assert rows[0, 4] == 0 and rows[1, 4] == 1 and rows[1, 0] == rows[0, 0]


def synthetic_case(shape, seed, foreground=True, C=2):
    """an integer-valued CT-like case with a zero border (so the crop takes something away) and labels {-1 .. 70} inside"""
    rng = np.random.RandomState(seed)
    D, H, W = shape
    img = np.zeros((C, D, H, W), np.float32)
    img[:, :, 2:H - 1, 1:W - 3] = rng.randint(-1024, 3072, (C, D, H - 3, W - 4)).astype(np.float32)
    seg = np.zeros((1, D, H, W), np.int16)
    if foreground:
        seg[0, :, 2:H - 1, 1:W - 3] = rng.choice(np.array([0, 0, 1, 2, 70], np.int16), (D, H - 3, W - 4))
    return torch.from_numpy(img), torch.from_numpy(seg), (1.0 + seed, 0.5, 0.75)


def test_extract_fingerprint():
    cases = [synthetic_case((2, 12, 19), 1), synthetic_case((1, 30, 11), 2, foreground=False), synthetic_case((3, 9, 25), 3)]
    fp = FP.extract_fingerprint(cases, num_foreground_voxels=900)
    assert set(fp) == {"spacings", "shapes_after_crop", "foreground_intensity_properties_per_channel", "median_relative_size_after_cropping"}
    assert fp["spacings"] == [c[2] for c in cases]
    crops = [PRE.crop_to_nonzero(c[0], c[1]) for c in cases]
    assert fp["shapes_after_crop"] == [tuple(d.shape[1:]) for d, _, _ in crops]
    assert all(a != tuple(c[0].shape[1:]) for a, c in zip(fp["shapes_after_crop"], cases))
    rel = [np.prod(d.shape[1:]) / np.prod(c[0].shape[1:]) for (d, _, _), c in zip(crops, cases)]
    assert fp["median_relative_size_after_cropping"] == float(np.median(rel, 0))
    per_case = [FP.analyze_case(*c, num_samples=300) for c in cases]
    assert [tuple(r[2].shape) for r in per_case] == [(2, 300), (2, 0), (2, 300)]
    assert per_case[1][0] == fp["shapes_after_crop"][1] and per_case[1][4] == rel[1]
    props = fp["foreground_intensity_properties_per_channel"]
    assert sorted(props) == [0, 1]
    for c in range(2):
        x = np.concatenate([r[2][c].numpy() for r in per_case])
        assert x.size == 600
        p = props[c]
        assert set(p) == {"mean", "median", "std", "min", "max", "percentile_99_5", "percentile_00_5"}
        assert all(isinstance(v, float) for v in p.values())
        assert p["median"] == float(np.median(x)) and p["min"] == float(np.min(x)) and p["max"] == float(np.max(x))
        assert p["percentile_00_5"] == float(np.percentile(x, 0.5)) and p["percentile_99_5"] == float(np.percentile(x, 99.5))
        mean, std = fsum_mean_std(x)
        assert p["mean"] == mean
        assert abs(p["std"] - std) <= x.size * 2.0 ** -52 * std
        print(f"c={c}: mean - np.mean = {p['mean'] - float(np.mean(x)):.3e}, std - np.std = {p['std'] - float(np.std(x)):.3e}")
    # what CTNormalization is given
    data, seg, _ = crops[0]
    want = data.numpy().copy()
    out = PRE.normalize(data.clone(), seg, ["CTNormalization"] * 2, None, props)
    for c in range(2):
        p = props[c]
        ref = np.clip(want[c], np.float32(p["percentile_00_5"]), np.float32(p["percentile_99_5"]))
        ref = (ref - np.float32(p["mean"])) / np.float32(max(p["std"], 1e-8))
        assert np.array_equal(out[c].numpy(), ref)


def test_extract_fingerprint_refusals():
    with pytest.raises(ValueError):
        FP.extract_fingerprint([synthetic_case((1, 30, 11), 2, foreground=False), synthetic_case((2, 8, 9), 4, foreground=False)], 100)
    img, seg, spacing = synthetic_case((2, 12, 19), 1)
    z, y, x = (int(v[0]) for v in np.nonzero(seg[0].numpy() > 0))
    img[1, z, y, x] = float("nan")
    with pytest.raises(ValueError):
        FP.extract_fingerprint([(img, seg, spacing)], 100)
    with pytest.raises(ValueError):
        FP.extract_fingerprint([])
