"""CPU tests of the cases path of inference (a list of cases, windows batched across cases): the batch plan, the host restatements of
du_window_gather / du_window_accumulate_cases against the plain construction (pad_to_patch + slicing + the reference's sequential `+=`
loop in float32, predict_from_raw_data.py:607-610) bit for bit, the memoised importance map against scipy's construction bit for bit, and
the ValueErrors that precede any launch."""
import numpy as np
import pytest
import torch

from dinounet_amd import inference as INF
from _window_ref import plain_accumulate

# list A of the issue: patch (64, 64), step 0.5, batch 8 -> 1, 1, 6, 4, 3, 4 windows = 19 windows in 3 chunks (the per-case loop: 6)
LIST_A = [(1, 40, 50), (1, 64, 64), (1, 70, 100), (1, 96, 96), (3, 64, 64), (1, 130, 64)]
WINDOWS_A = [1, 1, 6, 4, 3, 4]
PATCHES = [(64, 64), (48, 80), (17, 33), (5, 7), (512, 512)]


def padded(shape, patch):
    return (shape[0], max(shape[1], patch[0]), max(shape[2], patch[1]))


# ------------------------------------------------------------------------------------------------ plan_case_batches
def test_plan_list_a():
    plan = INF.plan_case_batches(LIST_A, (64, 64), 0.5, 8)
    assert len(plan) == 1
    members, chunks = plan[0]
    assert members == list(range(6)) and [len(c) for c in chunks] == [8, 8, 3]
    flat = [w for c in chunks for w in c]
    assert [sum(1 for w in flat if w[0] == i) for i in range(6)] == WINDOWS_A
    assert [w[0] for w in flat] == sorted(w[0] for w in flat)                     # cases in list order
    for i, s in enumerate(LIST_A):                                                 # every case's windows in sliding_window_origins order
        assert [w[1:] for w in flat if w[0] == i] == INF.sliding_window_origins(padded(s, (64, 64)), (64, 64), 0.5)
    assert INF.count_case_forwards(plan) == 3
    assert INF.count_case_forwards(plan, mirror_axes=(0, 1)) == 12
    per_case = sum(INF.count_case_forwards(INF.plan_case_batches([s], (64, 64), 0.5, 8)) for s in LIST_A)
    assert per_case == 6


def test_plan_budget_splits_the_list():
    vox = [int(np.prod(padded(s, (64, 64)))) for s in LIST_A]
    assert vox == [4096, 4096, 7000, 9216, 12288, 8320]
    # a budget that the first three cases fill: the list is cut after the third case -- and, the rule being the same for every group,
    # again wherever the next case would not fit (cases 3, 4 and 5 are each above half of it)
    plan = INF.plan_case_batches(LIST_A, (64, 64), 0.5, 8, max_voxels_in_flight=sum(vox[:3]))
    assert [m for m, _ in plan] == [[0, 1, 2], [3], [4], [5]]
    assert [[len(c) for c in chunks] for _, chunks in plan] == [[8], [4], [3], [4]]
    assert INF.count_case_forwards(plan) == 4
    plan = INF.plan_case_batches(LIST_A, (64, 64), 0.5, 8, max_voxels_in_flight=22000)
    assert [m for m, _ in plan] == [[0, 1, 2], [3, 4], [5]]
    assert [[len(c) for c in chunks] for _, chunks in plan] == [[8], [7], [4]]
    # two groups of three cases, 8 windows each, batch 6: 2 + 2 chunks, a window batch never spans two groups and only a group's last chunk
    # is ragged (one group of the six cases: 16 windows in 3 chunks)
    twice = LIST_A[:3] + LIST_A[:3]
    plan = INF.plan_case_batches(twice, (64, 64), 0.5, 6, max_voxels_in_flight=sum(vox[:3]))
    assert [m for m, _ in plan] == [[0, 1, 2], [3, 4, 5]]
    assert [[len(c) for c in chunks] for _, chunks in plan] == [[6, 2], [6, 2]]
    assert {w[0] for c in plan[1][1] for w in c} == {3, 4, 5}                      # `case` indexes the whole list
    assert INF.count_case_forwards(INF.plan_case_batches(twice, (64, 64), 0.5, 6)) == 3


def test_plan_case_larger_than_the_budget_is_its_own_group():
    plan = INF.plan_case_batches(LIST_A, (64, 64), 0.5, 8, max_voxels_in_flight=64 * 64)
    assert [m for m, _ in plan] == [[0], [1], [2], [3], [4], [5]]                  # cases 2..5 alone exceed it and still run
    assert [sum(len(c) for c in chunks) for _, chunks in plan] == WINDOWS_A
    plan = INF.plan_case_batches(LIST_A, (64, 64), 0.5, 8, max_voxels_in_flight=2 * 64 * 64)
    assert [m for m, _ in plan] == [[0, 1], [2], [3], [4], [5]]


# ------------------------------------------------------------------------------------------------ the host restatements
CASES = [(1, 5, 7), (2, 8, 12), (1, 13, 12), (3, 9, 31)]


def test_plan_chunks_above_the_accumulate_launch_limit():
    """the chunks tests/test_gpu_predict_cases.py accumulates in two launches (MAX_WINDOW_BATCH slots, then the rest)"""
    assert INF.MAX_WINDOW_BATCH == 64
    assert [[len(c) for c in chunks] for _, chunks in INF.plan_case_batches([CASES[3]], (6, 10), 0.3, 128)] == [[72]]
    assert [[len(c) for c in chunks] for _, chunks in INF.plan_case_batches(CASES, (6, 10), 0.3, 100)] == [[95]]


def make_cases(C, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((C, *s)).astype(np.float32) for s in CASES]


def plain_gather(cases, desc, patch, slots):
    out = torch.zeros((slots, cases[0].shape[0], *patch))
    for s, (i, d, y0, x0) in enumerate(desc):
        p, _ = INF.pad_to_patch(torch.from_numpy(cases[i]), patch)
        out[s] = p[:, d, y0:y0 + patch[0], x0:x0 + patch[1]]
    return out.numpy()


@pytest.mark.parametrize("patch", [(8, 12), (6, 10)])
@pytest.mark.parametrize("C", [1, 3])
def test_gather_numpy_matches_pad_and_slice(patch, C):
    cases = make_cases(C)
    (_, chunks), = INF.plan_case_batches(CASES, patch, 0.5, 64)
    desc = chunks[0]
    assert len({w[0] for w in desc}) == 4
    got = INF._gather_cases_numpy(cases, desc, patch, slots=len(desc) + 2)
    want = plain_gather(cases, desc, patch, len(desc) + 2)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32))
    assert not got[len(desc):].any()


@pytest.mark.parametrize("patch", [(8, 12), (6, 10)])
@pytest.mark.parametrize("step", [0.5, 0.3])
@pytest.mark.parametrize("chunk", [1, 5, 16])
def test_accumulate_numpy_matches_the_sequential_loop(patch, step, chunk):
    K = 3
    rng = np.random.default_rng(1)
    gauss = INF.compute_gaussian(patch, sigma_scale=1.0 / 8, value_scaling_factor=10).numpy()
    shapes = [padded(s, patch) for s in CASES]
    got = [np.zeros((K, *s), np.float32) for s in shapes], [np.zeros(s, np.float32) for s in shapes]
    want = [np.zeros((K, *s), np.float32) for s in shapes], [np.zeros(s, np.float32) for s in shapes]
    (_, chunks), = INF.plan_case_batches(CASES, patch, step, chunk)
    for desc in chunks:
        logits = rng.standard_normal((len(desc), K, *patch)).astype(np.float32)
        INF._accumulate_cases_numpy(logits, gauss, desc, *got)
        plain_accumulate(logits, gauss, desc, *want)
    for a, b in zip(got[0] + got[1], want[0] + want[1]):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    if step == 0.3:                                                                # more than 4 windows meet somewhere
        cover = np.zeros(shapes[3][1:], int)
        for _, d, y0, x0 in [w for c in chunks for w in c if w[0] == 3 and w[1] == 0]:
            cover[y0:y0 + patch[0], x0:x0 + patch[1]] += 1
        assert cover.max() > 4


# ------------------------------------------------------------------------------------------------ the importance map
def scipy_gaussian(tile_size, sigma_scale=1.0 / 8, value_scaling_factor=1.0, dtype=torch.float32):
    """sliding_window_prediction.py:10-31 as this package computed it before the map was memoised"""
    from scipy.ndimage import gaussian_filter
    tmp = np.zeros(tile_size)
    tmp[tuple(i // 2 for i in tile_size)] = 1
    g = torch.from_numpy(gaussian_filter(tmp, [i * sigma_scale for i in tile_size], 0, mode="constant", cval=0))
    g = (g / torch.max(g) * value_scaling_factor).type(dtype)
    g[g == 0] = torch.min(g[g != 0])
    return g


@pytest.mark.parametrize("patch", PATCHES)
def test_compute_gaussian_equals_scipy_to_the_bit(patch):
    for scale, dtype in ((10, torch.float32), (1.0, torch.float64)):
        got = INF.compute_gaussian(patch, sigma_scale=1.0 / 8, value_scaling_factor=scale, dtype=dtype)
        want = scipy_gaussian(patch, 1.0 / 8, scale, dtype)
        assert got.dtype == dtype and got.shape == want.shape
        assert torch.equal(got.view(torch.int32 if dtype == torch.float32 else torch.int64),
                           want.view(torch.int32 if dtype == torch.float32 else torch.int64))


def test_compute_gaussian_is_memoised_and_private(monkeypatch):
    import scipy.ndimage
    real, calls = scipy.ndimage.gaussian_filter, []

    def counting(arr, *a, **k):
        calls.append(np.ndim(arr))
        return real(arr, *a, **k)

    monkeypatch.setattr(scipy.ndimage, "gaussian_filter", counting)
    first = INF.compute_gaussian((40, 56), value_scaling_factor=10)                # a size no other test uses: the cache is cold
    assert calls and all(nd == 1 for nd in calls), calls                           # lines only, never the tile
    n = len(calls)
    keep = first.clone()
    first.zero_()                                                                  # a caller ruins its copy
    second = INF.compute_gaussian((40, 56), value_scaling_factor=10)
    assert len(calls) == n                                                         # no filtering at all on the second call
    assert torch.equal(second, keep) and second.data_ptr() != first.data_ptr()
    second.mul_(3.0)
    assert torch.equal(INF.compute_gaussian((40, 56), value_scaling_factor=10), keep)
    assert torch.equal(INF.compute_gaussian((40, 56), sigma_scale=1.0 / 4, value_scaling_factor=10), scipy_gaussian((40, 56), 1.0 / 4, 10))


# ------------------------------------------------------------------------------------------------ errors before any launch
class NoLaunch(torch.nn.Module):
    """a network that must never be reached"""

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))

    def forward(self, x):
        raise AssertionError("the network was called")


@pytest.mark.parametrize("fn", ["predict_cases_logits", "predict_cases_segmentation"])
def test_value_errors(fn, monkeypatch):
    monkeypatch.setattr(INF._lib, "lib", lambda: pytest.fail("a launch was attempted"))
    f, net = getattr(INF, fn), NoLaunch()
    ok = torch.zeros((3, 1, 10, 10))
    with pytest.raises(ValueError):
        f(net, [], (8, 8))
    with pytest.raises(ValueError):
        f(net, [ok, torch.zeros((3, 10, 10))], (8, 8))                             # not (C, D, H, W)
    with pytest.raises(ValueError):
        f(net, ok, (8, 8))                                                         # a single array is not a list
    with pytest.raises(ValueError):
        f(net, [ok, torch.zeros((2, 1, 10, 10))], (8, 8))                          # differing channel counts
    with pytest.raises(ValueError):
        f(net, [ok, ok], (8, 8), batch_size=65)
    with pytest.raises(ValueError):
        f(net, [ok], (8, 8), batch_size=0)
    if fn == "predict_cases_segmentation":
        with pytest.raises(ValueError):
            f(net, [ok, ok], (8, 8), properties=[{}])                              # a properties list of another length
        with pytest.raises(ValueError):
            f(net, [ok, ok], (8, 8), properties={})


def test_value_errors_raw(monkeypatch):
    monkeypatch.setattr(INF._lib, "lib", lambda: pytest.fail("a launch was attempted"))
    kw = dict(transpose_forward=(0, 1, 2), spacing=[1.0, 1.0], normalization_schemes=["ZScoreNormalization"], use_mask_for_norm=[False],
              foreground_intensity_properties_per_channel=None)
    img = np.zeros((1, 1, 10, 10), np.float32)
    net = NoLaunch()
    with pytest.raises(ValueError):
        INF.predict_from_list_of_npy_arrays(net, [], [], (8, 8), **kw)
    with pytest.raises(ValueError):
        INF.predict_from_list_of_npy_arrays(net, [img, img], [{"spacing": (1.0, 1.0, 1.0)}], (8, 8), **kw)
    with pytest.raises(ValueError):
        INF.predict_from_list_of_npy_arrays(net, img, [{"spacing": (1.0, 1.0, 1.0)}], (8, 8), **kw)
    with pytest.raises(ValueError):
        INF.predict_from_list_of_npy_arrays(net, [img], [{"spacing": (1.0, 1.0, 1.0)}], (8, 8), batch_size=65, **kw)
    with pytest.raises(ValueError):
        INF.predict_from_list_of_npy_arrays(net, [img], [{"spacing": (1.0, 1.0, 1.0)}], (8, 8), properties=[None], **kw)
    ok = {"spacing": (1.0, 1.0, 1.0)}
    with pytest.raises(ValueError):                                                # a bad case behind a good one: still before any launch
        INF.predict_from_list_of_npy_arrays(net, [img, np.zeros((2, 1, 10, 10), np.float32)], [dict(ok), dict(ok)], (8, 8), **kw)
    with pytest.raises(ValueError):
        INF.predict_from_list_of_npy_arrays(net, [img, np.zeros((1, 10, 10), np.float32)], [dict(ok), dict(ok)], (8, 8), **kw)
    with pytest.raises(ValueError):
        INF.predict_from_list_of_npy_arrays(net, [img, img], [dict(ok), {"spacing": (1.0, 1.0)}], (8, 8), **kw)
