"""GPU tests (-m gpu) of csrc/fingerprint.hip through dinounet_amd.fingerprint, against the numpy restatement that CPU tensors run
(tests/test_cpu_fingerprint.py checks that restatement against np.percentile, np.median and RandomState.choice).  Order statistics and
samples are copies of fp32 values and are compared exactly (==, the samples as int32 views); count, min and max exactly; the fp64 sum
exactly where the values are integers; std within n 2^-52 relative of the math.fsum formula (every one of the n additions rounds once).

The case shapes give n = 1, exactly one chunk of 1024 voxels, one voxel more, a non-multiple and many chunks, as
test_gpu_dataloading.VOLUMES do; every value set aims at one way a radix select fails.  Small shapes are asked for EVERY rank (a
permutation of 0..n-1 in groups of 8), large ones for {0, n-1, lo / hi of the percentiles 0.5, 50, 99.5}."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from dinounet_amd import _lib
from dinounet_amd import fingerprint as FP
from dinounet_amd import preprocessing as PRE
from test_cpu_fingerprint import fsum_mean_std, synthetic_case
from test_gpu_ops import dev

pytestmark = pytest.mark.gpu

CASES = [(1, 1, 1, 1), (2, 1, 32, 32), (1, 1, 25, 41), (3, 2, 9, 67), (2, 5, 37, 131), (1, 8, 256, 256)]
PATTERNS = ["all", "first_last", "fifth_chunk", "random30", "none"]
FLAT = [1, 2, 1023, 1025, 30000, 2 ** 20 + 1]
VALUE_SETS = ["equal", "low_bit", "signs", "ct", "gauss", "exponents"]
INTEGER_SETS = ("equal", "ct")                                                        # fp64 sums of these are exact in any order
EVERY_RANK_BELOW = 1300


def make_values(kind, C_, n, seed):
    rng = np.random.RandomState(seed)
    if kind == "equal":                                                               # one bin through every digit
        return np.full((C_, n), 3.25, np.float32)
    if kind == "low_bit":                                                             # two values that differ in the lowest bit only
        a = np.float32(1000.0)
        return rng.choice(np.array([a, np.nextafter(a, np.float32(2000))], np.float32), (C_, n))
    if kind == "signs":                                                               # the key map and its sign flip
        pool = np.array([-0.0, 0.0, -1.5, 1.5, -1e-30, 1e-30, -1e-45, 1e-45, -3e38, 3e38, 2.0, -2.0], np.float32)
        return rng.choice(pool, (C_, n))
    if kind == "ct":                                                                  # ties: the rank falls inside a run of equal keys
        return rng.randint(-1024, 3072, (C_, n)).astype(np.float32)
    if kind == "gauss":
        return (1000.0 + rng.randn(C_, n)).astype(np.float32)
    k = rng.randint(-20, 21, (C_, n))                                                 # every digit position is used
    return (rng.choice(np.array([-1.0, 1.0]), (C_, n)) * 2.0 ** k).astype(np.float32)


def make_seg(pattern, n, seed):
    rng = np.random.RandomState(seed)
    seg = rng.choice(np.array([-1, 0], np.int16), n)
    if pattern == "all":
        seg = rng.choice(np.array([1, 2, 70], np.int16), n)
    elif pattern == "first_last":
        seg[0], seg[-1] = 70, 1
    elif pattern == "fifth_chunk":
        seg[(np.arange(n) // 1024) % 5 == 0] = 2                                      # chunk 0 too: no shape is left without members
    elif pattern == "random30":
        hit = rng.random_sample(n) < 0.3
        seg[hit] = rng.choice(np.array([1, 2, 70], np.int16), int(hit.sum()))
    return seg


def rank_groups(k, seed):
    """(groups, 8) int64: every rank of 0..k-1 once when k is small, else the ranks the statistics ask for"""
    if k < EVERY_RANK_BELOW:
        r = np.random.RandomState(seed).permutation(k)
        r = np.resize(r, k + (-k) % 8)                                                # the last group is filled up with repeats
    else:
        plan, _ = FP._rank_plan(k)
        r = np.array([0, k - 1] + plan)
    return r.reshape(-1, 8).astype(np.int64)


def check_operations(x, seg, tag):
    """moments, order statistics and samples of x (C, n) / seg (n) or None on the device against the CPU restatement"""
    d = dev()
    C_, n = x.shape
    xt, st = torch.from_numpy(x), None if seg is None else torch.from_numpy(seg)
    xd, sd = xt.to(d), None if seg is None else st.to(d)
    ref = FP.foreground_moments(xt, st, with_std=True).numpy()
    got_t = FP.foreground_moments(xd, sd, with_std=True)
    again = FP.foreground_moments(xd, sd, with_std=True)
    assert torch.equal(got_t.view(torch.int64), again.view(torch.int64)), f"{tag}: a repeated call differs"
    got = got_t.cpu().numpy()
    k = int(ref[0, 0])
    assert np.array_equal(got[:, [0, 1, 2, 4]], ref[:, [0, 1, 2, 4]]), f"{tag}: count / min / max / NaN count"
    members = x if seg is None else x[:, seg > 0]
    for c in range(C_ if k else 0):
        if tag.split("/")[0] in INTEGER_SETS:
            assert got[c, 3] == ref[c, 3] == float(members[c].astype(np.float64).sum()), f"{tag}: the sum of integers is exact"
        else:
            x64 = members[c].astype(np.float64)                                       # k - 1 additions, each within 2^-53 of sum|x|
            assert abs(got[c, 3] - math.fsum(x64.tolist())) <= k * 2.0 ** -53 * math.fsum(np.abs(x64).tolist())
        ours = math.sqrt(got[c, 5] / k)
        std = fsum_mean_std(members[c])[1]
        print(f"{tag} c={c}: k={k} std {ours!r} against fsum {std!r}")
        assert abs(ours - std) <= k * 2.0 ** -52 * std
    if k == 0:
        assert np.all(got[:, 3] == 0) and np.all(got[:, 5] == 0)
        return
    srt = np.sort(members, axis=1)
    for g, row in enumerate(rank_groups(k, n)):
        ranks = torch.from_numpy(np.stack([np.roll(row, c) for c in range(C_)]))      # every channel its own order
        out = FP.foreground_order_stats(xd, sd, ranks.to(d)).cpu().numpy()
        want = np.take_along_axis(srt, ranks.numpy(), axis=1)
        assert np.all(out == want), f"{tag}: order statistics, group {g}: {out} against {want}"
    rng = np.random.RandomState(n + 1)
    ranks = np.stack([np.concatenate([rng.permutation(k), rng.randint(0, k, min(k, 100))]) for _ in range(C_)]).astype(np.int64)
    out = FP.foreground_sample(xd, sd, torch.from_numpy(ranks).to(d)).cpu().numpy()
    want = np.take_along_axis(members, ranks, axis=1)
    assert np.array_equal(out.view(np.int32), want.view(np.int32)), f"{tag}: samples"
    assert np.array_equal(FP.foreground_sample(xt, st, torch.from_numpy(ranks)).numpy().view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", CASES, ids=str)
def test_case_shapes(shape, pattern):
    C_, n = shape[0], int(np.prod(shape[1:]))
    seg = make_seg(pattern, n, n)
    for i, kind in enumerate(VALUE_SETS):
        check_operations(make_values(kind, C_, n, 7 * n + i), seg, f"{kind}/{shape}/{pattern}")


@pytest.mark.parametrize("C_", [1, 3])
@pytest.mark.parametrize("n", FLAT)
def test_flat_shapes(n, C_):
    for i, kind in enumerate(VALUE_SETS):
        check_operations(make_values(kind, C_, n, 11 * n + i), None, f"{kind}/({C_}, {n})/flat")


def assert_stats_agree(got, want, members, integer):
    """got: the statistics from CUDA tensors, want: from CPU tensors, members: per channel the n values they describe (None: no foreground).
    Order statistics, min and max are equal.  mean and std are held against math.fsum over the members with the real n: the mean of
    integers exactly; any other mean within n 2^-52 mean|x| (n - 1 additions of the sequential sum, each at most 2^-53 of sum|x|, and the
    division); std within n 2^-52 relative."""
    assert len(got) == len(want) == len(members)
    for g, w, x in zip(got, want, members):
        assert set(g) == set(w)
        if x is None:
            assert all(math.isnan(g[key]) and math.isnan(w[key]) for key in w)
            continue
        n = x.size
        mean, std = fsum_mean_std(x)
        for key in w:
            if key == "std":
                print(f"n={n}: std {g[key]!r} against fsum {std!r}")
                assert abs(g[key] - std) <= n * 2.0 ** -52 * std
            elif key == "mean" and integer:
                assert g[key] == w[key] == mean
            elif key == "mean":
                print(f"n={n}: mean {g[key]!r} against fsum {mean!r}")
                assert abs(g[key] - mean) <= n * 2.0 ** -52 * math.fsum(np.abs(x.astype(np.float64)).tolist()) / n
            else:
                assert g[key] == w[key], (key, g[key], w[key])


@pytest.mark.parametrize("kind", ["ct", "gauss"])
@pytest.mark.parametrize("shape,pattern", [((3, 2, 9, 67), "random30"), ((2, 5, 37, 131), "fifth_chunk"), ((1, 8, 256, 256), "random30"),
                                           ((2, 1, 32, 32), "none")], ids=str)
def test_collect_foreground_intensities(shape, pattern, kind):
    d = dev()
    C_, n = shape[0], int(np.prod(shape[1:]))
    img = torch.from_numpy(make_values(kind, C_, n, n).reshape(shape))
    seg = torch.from_numpy(make_seg(pattern, n, n).reshape(1, *shape[1:]))
    want_i, want_s = FP.collect_foreground_intensities(seg, img, num_samples=1500)
    got_i, got_s = FP.collect_foreground_intensities(seg.to(d), img.to(d), num_samples=1500)
    assert got_i.device.type == "cuda" and got_i.dtype == torch.float32 and tuple(got_i.shape) == tuple(want_i.shape)
    assert torch.equal(got_i.cpu().view(torch.int32), want_i.view(torch.int32))
    fg = seg.numpy()[0] > 0
    assert_stats_agree(got_s, want_s, [img.numpy()[c][fg] if fg.any() else None for c in range(C_)], kind == "ct")
    if pattern != "none":
        bad = img.clone()
        bad[C_ - 1].view(-1)[int(np.flatnonzero(seg.numpy().ravel() > 0)[-1])] = float("nan")
        with pytest.raises(ValueError):
            FP.collect_foreground_intensities(seg.to(d), bad.to(d), num_samples=10)
        ok = img.clone()                                                              # a NaN outside the foreground is nobody's business
        ok[0].view(-1)[int(np.flatnonzero(seg.numpy().ravel() <= 0)[0])] = float("nan")
        again, _ = FP.collect_foreground_intensities(seg.to(d), ok.to(d), num_samples=1500)
        assert torch.equal(again, got_i)


def test_analyze_case_and_extract_fingerprint():
    d = dev()
    cases = [synthetic_case((2, 12, 19), 1), synthetic_case((1, 30, 11), 2, foreground=False), synthetic_case((3, 40, 45), 3)]
    on_dev = [(i.to(d), s.to(d), sp) for i, s, sp in cases]
    per_case = []
    for host, device in zip(cases, on_dev):
        w = FP.analyze_case(*host, num_samples=1000)                                  # what extract_fingerprint(cases, 3000) keeps of a case
        g = FP.analyze_case(*device, num_samples=1000)
        assert g[0] == w[0] and g[1] == w[1] and g[4] == w[4]
        assert torch.equal(g[2].cpu().view(torch.int32), w[2].view(torch.int32))
        data, cseg, _ = PRE.crop_to_nonzero(host[0], host[1])
        fg = cseg.numpy()[0] > 0
        assert_stats_agree(g[3], w[3], [data.numpy()[c][fg] if fg.any() else None for c in range(2)], True)
        per_case.append(w[2].numpy())
    want = FP.extract_fingerprint(cases, 3000)
    got = FP.extract_fingerprint(on_dev, 3000)
    assert set(got) == set(want)
    for key in ("spacings", "shapes_after_crop", "median_relative_size_after_cropping"):
        assert got[key] == want[key]
    key = "foreground_intensity_properties_per_channel"
    assert sorted(got[key]) == sorted(want[key]) == [0, 1]
    samples = np.concatenate(per_case, axis=1)                                        # (2, 2000): one case has no foreground
    assert samples.shape == (2, 2000)
    assert_stats_agree([got[key][c] for c in (0, 1)], [want[key][c] for c in (0, 1)], [samples[0], samples[1]], True)
    with pytest.raises(ValueError):
        FP.extract_fingerprint([on_dev[1]], 100)                                      # no foreground anywhere
    img = cases[0][0].clone()
    z, y, x = (int(v[0]) for v in np.nonzero(cases[0][1][0].numpy() > 0))
    img[0, z, y, x] = float("nan")
    with pytest.raises(ValueError):
        FP.extract_fingerprint([(img.to(d), on_dev[0][1], cases[0][2])], 100)


def test_c_abi_refusals():
    """return codes only: every refusal comes back before a launch.  The ranks live on the device, so a rank >= count is the one thing the
    call cannot refuse: it is answered with NaN in that place and leaves its neighbours alone."""
    d = dev()
    L = _lib.lib()
    BAD, UNSUPPORTED = -1, -2
    n, Cn, R = 3000, 2, 4
    img = torch.arange(Cn * n, dtype=torch.float32, device=d).reshape(Cn, n)
    seg = torch.ones(n, dtype=torch.int16, device=d)
    ranks = torch.zeros((Cn, R), dtype=torch.int64, device=d)
    out = torch.zeros((Cn, R), dtype=torch.float32, device=d)
    stats = torch.zeros((Cn, 6), dtype=torch.float64, device=d)
    w = FP.workspace_elems(Cn, n)
    ws = torch.zeros(w + 4, dtype=torch.int32, device=d)
    i, s, r, o, t, k = (x.data_ptr() for x in (img, seg, ranks, out, stats, ws))
    big = 2 ** 31

    def moments(img=i, seg=s, n=n, mode=0, stats=t, ws=k, w=w):
        return L.du_fp_moments(img, seg, Cn, n, mode, stats, ws, w, None)

    def order(img=i, seg=s, n=n, ranks=r, R=R, out=o, ws=k, w=w):
        return L.du_fp_order_stats(img, seg, Cn, n, ranks, R, out, ws, w, None)

    def sample(img=i, seg=s, n=n, ranks=r, m=R, out=o, ws=k, w=w):
        return L.du_fp_sample(img, seg, Cn, n, ranks, m, out, ws, w, None)

    for fn in (moments, order, sample):
        assert fn(img=None) == BAD and fn(ws=None) == BAD
        assert fn(img=i + 2) == BAD and fn(seg=s + 1) == BAD and fn(ws=k + 4) == BAD
        assert fn(w=w - 4) == BAD
        assert fn(n=0) == BAD
        assert fn(n=big) == UNSUPPORTED
    assert moments(stats=None) == BAD and moments(stats=t + 4) == BAD and moments(mode=2) == BAD
    for fn in (order, sample):
        assert fn(ranks=None) == BAD and fn(out=None) == BAD and fn(ranks=r + 4) == BAD and fn(out=o + 2) == BAD
    assert order(R=0) == BAD and order(R=9) == BAD and sample(m=0) == BAD
    assert L.du_fp_ws_elems(Cn, big) == UNSUPPORTED and L.du_fp_ws_elems(0, n) == BAD and L.du_fp_ws_elems(Cn, 0) == BAD
    assert L.du_fp_ws_elems(70000, n) == UNSUPPORTED
    with pytest.raises(RuntimeError, match="DU_ERR_UNSUPPORTED"):
        FP.workspace_elems(1, big)
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0                                              # nothing ran
    half = torch.from_numpy(np.where(np.arange(n) % 2 == 0, 1, 0).astype(np.int16)).to(d)                      # count = 1500
    rk = torch.tensor([[0, 1500, 1499, -1], [3000, 7, 2 ** 40, 1]], dtype=torch.int64, device=d)
    want = np.array([[0, np.nan, 2998, np.nan], [np.nan, n + 14, np.nan, n + 2]], np.float32)
    for got in (FP.foreground_order_stats(img, half, rk), FP.foreground_sample(img, half, rk)):
        assert np.array_equal(got.cpu().numpy(), want, equal_nan=True)
