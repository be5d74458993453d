"""GPU tests (-m gpu) of csrc/preprocess.hip through dinounet_amd.preprocessing, against the numpy / scipy restatement that CPU tensors run
(tests/test_cpu_preprocessing.py checks that restatement against scipy and brute force).

Integer results (mask, bounding box, segmentation, properties) and the four fp32 normalisation schemes must be equal.  The float bounds:
  ZScore   |gpu - cpu| <= 2^-23 |cpu| + 1e-10 max|x - mean| / max(std, 1e-8): one fp32 rounding of two fp64 values that differ only by
           the order of the fp64 sums, and that order acting on the mean.  Integer-valued inputs with a power-of-two count have exact
           sums: equal to the bit.
  order 3  |gpu - cpu| <= 2^-22 max|x|: both sides are fp64 rounded once to fp32, the clip bounds the outputs by max|x|; the kernel's
           truncation of the prefilter's impulse response at 32 samples contributes less than 1e-18.
The shapes cross the 4 x 8 x 64 tile of the fill kernels in every axis, hit exact multiples of it, and degenerate; (8, 256, 256) has 256
tiles, so many workgroups merge at once.  The reference of a case is computed once."""
import functools

import numpy as np
import pytest
import torch

from dinounet_amd import preprocessing as P
from test_cpu_preprocessing import (INTENSITY, PATTERNS, SEG_LABELS, SEG_SIZES, blocky_seg, ct_like, make_data, make_mask, make_seg, raw_case,
                                    spiky, tie_pixels)
from test_gpu_ops import dev

pytestmark = pytest.mark.gpu

FILL_SHAPES = [(1, 70, 150), (2, 9, 67), (3, 64, 128), (5, 37, 131), (1, 1, 1), (2, 2, 2), (8, 256, 256)]


# ------------------------------------------------------------------------------------------------ mask, fill, bbox, outside label
@functools.lru_cache(maxsize=None)
def crop_reference(pattern, shape, channels, with_seg, dtype="float32"):
    data = torch.from_numpy(make_data(pattern, shape, channels, dtype=np.dtype(dtype)))
    seg = torch.from_numpy(make_seg(shape)) if with_seg else None
    return data, seg, P.create_nonzero_mask(data), P.crop_to_nonzero(data, seg)


def check_crop(data, seg, want_mask, want):
    d = data.to(dev())
    s = None if seg is None else seg.to(dev())
    mask = P.create_nonzero_mask(d)
    img, sg, bbox = P.crop_to_nonzero(d, s)
    w_img, w_sg, w_bbox = want
    print(f"{tuple(data.shape)}: bbox {bbox} (restatement {w_bbox}); mask differs at {int((mask.cpu() != want_mask).sum())} voxels, "
          f"filled {int(want_mask.sum()) - int((data != 0).any(0).sum())}")
    assert mask.dtype == torch.bool and mask.is_cuda and img.is_cuda and sg.is_cuda
    assert torch.equal(mask.cpu(), want_mask)
    assert bbox == w_bbox
    assert img.dtype == torch.float32 and sg.dtype == torch.int16 and tuple(sg.shape) == (1, *img.shape[1:])
    assert torch.equal(img.cpu(), w_img)
    assert torch.equal(sg.cpu(), w_sg)
    assert torch.equal(d.cpu(), data) and (s is None or torch.equal(s.cpu(), seg)), "the input was modified"


@pytest.mark.parametrize("with_seg", [False, True], ids=["noseg", "seg"])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("shape", FILL_SHAPES, ids=str)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_crop_patterns(pattern, shape, channels, with_seg):
    check_crop(*crop_reference(pattern, shape, channels, with_seg))


@pytest.mark.parametrize("dtype", ["float64", "uint8", "int16", "int32"])
def test_crop_dtypes(dtype):
    check_crop(*crop_reference("noise", (5, 37, 131), 2, True, dtype))


def test_fill_depth_and_diagonal():
    """D <= 2: nothing is ever filled; D = 3: the middle slice's hole is; a hole that meets the outside only across an edge is filled"""
    for D in (1, 2, 3):
        x = torch.ones((1, D, 9, 9))
        x[0, D // 2, 4, 4] = 0
        assert bool(P.create_nonzero_mask(x.to(dev()))[D // 2, 4, 4]) == (D == 3)
    m = make_mask("diagonal_leak", (5, 37, 131))
    got = P.create_nonzero_mask(torch.from_numpy(m.astype(np.float32))[None].to(dev())).cpu().numpy()
    assert int((got != m).sum()) == 1 and got[2, 1, 1] and not got[2, 0, 0]


def test_all_zero_raises():
    with pytest.raises(ValueError):
        P.crop_to_nonzero(torch.zeros((2, 3, 9, 70), device=dev()))


# ------------------------------------------------------------------------------------------------ normalisation
def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("shape", [(1, 3, 37, 53), (1, 1, 1, 1), (1, 2, 128, 130)], ids=str)
@pytest.mark.parametrize("scheme", ["NoNormalization", "RGBTo01Normalization", "CTNormalization", "RescaleTo01Normalization"])
def test_fp32_schemes_equal_to_the_bit(scheme, shape):
    x = ct_like(shape, 5)
    if scheme == "RGBTo01Normalization":
        x = np.random.RandomState(6).randint(0, 256, size=shape).astype(np.float32)
    want = P.normalize(torch.from_numpy(x.copy()), None, [scheme], [False], INTENSITY)
    d = torch.from_numpy(x.copy()).to(dev())
    got = P.normalize(d, None, [scheme], [False], INTENSITY)
    assert got is d
    assert torch.equal(bits(got), bits(want))


def test_mixed_schemes_and_rgb_range():
    x = np.random.RandomState(3).randint(0, 256, size=(4, 2, 20, 70)).astype(np.float32)
    schemes = ["RGBTo01Normalization", "RescaleTo01Normalization", "NoNormalization", "CTNormalization"]
    ip = {"3": INTENSITY["0"]}
    want = P.normalize(torch.from_numpy(x.copy()), None, schemes, [False] * 4, ip)
    got = P.normalize(torch.from_numpy(x.copy()).to(dev()), None, schemes, [False] * 4, ip)
    assert torch.equal(bits(got), bits(want))
    for bad in (-1.0, 256.0):
        d = torch.from_numpy(x.copy()).to(dev())
        d[0, 1, 3, 5] = bad
        with pytest.raises(ValueError):
            P.normalize(d, None, schemes, [False] * 4, ip)


def zscore_pair(x, seg, use_mask):
    C = x.shape[0]
    s = None if seg is None else torch.from_numpy(seg)
    want = P.normalize(torch.from_numpy(x.copy()), s, ["ZScoreNormalization"] * C, [use_mask] * C, None)
    got = P.normalize(torch.from_numpy(x.copy()).to(dev()), None if s is None else s.to(dev()), ["ZScoreNormalization"] * C, [use_mask] * C, None)
    return got.cpu(), want


@pytest.mark.parametrize("use_mask", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("shape", [(2, 3, 37, 131), (1, 1, 200, 300)], ids=str)
def test_zscore_offset_data(shape, use_mask):
    """mean 1000, std 1: a one-pass variance in fp32 or a mean in fp32 would fail this"""
    x = (np.random.RandomState(7).randn(*shape) + 1000.0).astype(np.float32)
    seg = np.where(np.random.RandomState(8).random_sample((1, *shape[1:])) < 0.3, -1, 0).astype(np.int16)
    got, want = zscore_pair(x, seg, use_mask)
    g, w = got.numpy().astype(np.float64), want.numpy().astype(np.float64)
    for c in range(shape[0]):
        sel = x[c][seg[0] >= 0] if use_mask else x[c].ravel()
        mean, std = sel.astype(np.float64).mean(), sel.astype(np.float64).std()
        bound = 2.0 ** -23 * np.abs(w[c]) + 1e-10 * np.abs(sel - mean).max() / max(std, 1e-8)
        err = np.abs(g[c] - w[c])
        print(f"{shape} channel {c} mask {use_mask}: max |gpu - cpu| = {err.max():.3e}, {int((err > 0).sum())} voxels differ; std of the output "
              f"{w[c][seg[0] >= 0].std() if use_mask else w[c].std():.6f}")
        assert (err <= bound).all()
        if use_mask:
            assert np.array_equal(got.numpy()[c][seg[0] < 0], x[c][seg[0] < 0]), "voxels outside the mask must keep their bits"


def test_zscore_single_voxel_mask_and_constant():
    x = ct_like((1, 2, 5, 70), 9)
    seg = np.full((1, 2, 5, 70), -1, dtype=np.int16)
    seg[0, 1, 2, 3] = 0
    got, want = zscore_pair(x, seg, True)
    assert torch.equal(bits(got), bits(want)) and float(got[0, 1, 2, 3]) == 0.0 and int((got.numpy() != x).sum()) == 1
    # std == 0.  An integer constant: its sums are exact, so x - mean is exactly 0 on both sides (for any other constant the result is the
    # rounding of the mean times 1e8 on either side, which no bound describes)
    got, want = zscore_pair(np.full((2, 3, 9, 70), 7.0, dtype=np.float32), None, False)
    assert torch.equal(bits(got), bits(want)) and not got.any()


@pytest.mark.parametrize("use_mask", [False, True], ids=["plain", "masked"])
def test_zscore_exact_inputs_equal_to_the_bit(use_mask):
    """integers around 1000 over a power-of-two count: the sum, the mean, every deviation, its square and their sum are exact in fp64
    whatever the order, so both sides do the same arithmetic on the same numbers"""
    shape = (2, 2, 32, 64)
    x = (np.random.RandomState(11).randint(-50, 51, size=shape) + 1000).astype(np.float32)
    seg = np.full((1, *shape[1:]), -1, dtype=np.int16)
    seg.reshape(-1)[np.random.RandomState(12).permutation(seg.size)[:2048]] = 0
    got, want = zscore_pair(x, seg, use_mask)
    assert torch.equal(bits(got), bits(want))
    assert abs(float(want[0][torch.from_numpy(seg[0] >= 0)].mean() if use_mask else want[0].mean())) < 1e-6


# ------------------------------------------------------------------------------------------------ order 3
CUBIC_SIZES = [((9, 11), (13, 7)), ((64, 64), (64, 100)), ((1, 5), (3, 5)), ((2, 300), (5, 130)), ((130, 70), (65, 35))]
SCOPES = {"slice": ((5.0, 1.0, 1.0), (5.0, 0.7, 0.7)), "volume": ((1.0, 1.0, 1.0), (1.0, 0.7, 0.7))}


@functools.lru_cache(maxsize=None)
def cubic_reference(hw, out, C, D, scope):
    x = torch.from_numpy(spiky((C, D, *hw), seed=2, offset=0.5).astype(np.float32))
    return x, P.resample_data_or_seg_to_shape(x, (D, *out), *SCOPES[scope])


@pytest.mark.parametrize("scope", ["slice", "volume"])
@pytest.mark.parametrize("C,D", [(1, 1), (3, 3), (1, 3), (3, 1)])
@pytest.mark.parametrize("hw,out", CUBIC_SIZES, ids=str)
def test_cubic_resampling(hw, out, C, D, scope):
    x, want = cubic_reference(hw, out, C, D, scope)
    d = x.to(dev())
    got = P.resample_data_or_seg_to_shape(d, (D, *out), *SCOPES[scope])
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (C, D, *out)
    err = float((got.cpu().double() - want.double()).abs().max())
    bound = 2.0 ** -22 * float(x.abs().max())
    print(f"{hw} -> {out}, C {C}, D {D}, {scope}: max |gpu - cpu| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert torch.equal(d.cpu(), x), "the input was modified"
    if hw[0] > 1:
        raw = P._resize_cubic_float64(x.numpy(), out)
        axes = (2, 3) if scope == "slice" else (1, 2, 3)
        lo, hi = x.numpy().min(axis=axes, keepdims=True), x.numpy().max(axis=axes, keepdims=True)
        assert ((raw < lo) | (raw > hi)).any(), "the clip never acted"
        assert float(got.min()) >= float(x.min()) and float(got.max()) <= float(x.max())
    if D == 3 and hw[0] > 1:                          # (a single row upsampled along y is constant along y: nothing overshoots)
        assert not torch.equal(cubic_reference(hw, out, C, D, "slice")[1], cubic_reference(hw, out, C, D, "volume")[1])


def test_cubic_unchanged_shape_returns_the_input():
    d = torch.from_numpy(spiky((2, 3, 9, 70)).astype(np.float32)).to(dev())
    keep = d.clone()
    assert P.resample_data_or_seg_to_shape(d, (3, 9, 70), (5.0, 1.0, 1.0), (5.0, 1.0, 1.0)) is d
    assert torch.equal(bits(d), bits(keep))


# ------------------------------------------------------------------------------------------------ order 1, segmentation
@functools.lru_cache(maxsize=None)
def seg_reference(hw, out, D):
    seg = torch.from_numpy(blocky_seg((D, *hw), seed=3)[None])
    return seg, P.resample_data_or_seg_to_shape(seg, (D, *out), (1, 1, 1), (1, 1, 1), is_seg=True, order=1)


@pytest.mark.parametrize("D", [1, 3])
@pytest.mark.parametrize("hw,out", SEG_SIZES, ids=str)
def test_seg_resampling(hw, out, D):
    seg, want = seg_reference(hw, out, D)
    assert set(np.unique(seg.numpy())) <= set(SEG_LABELS.tolist())
    got = P.resample_data_or_seg_to_shape(seg.to(dev()), (D, *out), (1, 1, 1), (1, 1, 1), is_seg=True, order=1)
    ties = int(tie_pixels(seg.numpy()[0], out).sum())
    print(f"{hw} -> {out}, D {D}: {int((got.cpu() != want).sum())} of {want.numel()} pixels differ; {ties} exact ties")
    assert got.dtype == torch.int16 and got.is_cuda and tuple(got.shape) == (1, D, *out)
    assert torch.equal(got.cpu(), want)
    if (hw, out) == ((64, 64), (32, 32)):
        assert ties > 20, "the dyadic case must pin the >= and the overwrite order"


def test_seg_dyadic_ties_by_hand():
    seg = torch.tensor([[[[1, 1, 2, 2, -1, -1, 126, 0], [2, 2, 1, 2, 2, 126, 1, 2]]]], dtype=torch.int16)
    got = P.resample_data_or_seg_to_shape(seg.to(dev()), (1, 1, 4), (1, 1, 1), (1, 1, 1), is_seg=True, order=1)
    assert got.cpu().tolist() == [[[[2, 2, -1, 0]]]]


# ------------------------------------------------------------------------------------------------ run_case
def run_both(img, seg, spacing_raw, **kw):
    pc, pg = {"spacing": spacing_raw}, {"spacing": spacing_raw}
    s = None if seg is None else torch.from_numpy(seg)
    want = P.run_case(torch.from_numpy(img), s, pc, **kw)
    got = P.run_case(torch.from_numpy(img).to(dev()), None if s is None else s.to(dev()), pg, **kw)
    assert pc == pg and all(type(pc[k]) is type(pg[k]) for k in pc), (pc, pg)
    assert got[0].is_cuda and got[1].is_cuda and got[0].dtype == torch.float32 and got[1].dtype == torch.int16
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape
    assert torch.equal(got[1].cpu(), want[1])
    return got[0].cpu(), want[0], pc


def test_run_case_natural_image():
    img, _ = raw_case((1, 70, 150), (0, 6, 9), channels=3, seed=2)
    got, want, props = run_both(img, None, (999.0, 1.0, 1.0), transpose_forward=(0, 1, 2), spacing=[1.25, 0.8],
                                normalization_schemes=["ZScoreNormalization", "RescaleTo01Normalization", "RGBTo01Normalization"],
                                use_mask_for_norm=[False] * 3, foreground_intensity_properties_per_channel=None)
    assert props["bbox_used_for_cropping"] == [[0, 1], [6, 64], [9, 141]] and tuple(want.shape) == (3, 1, 46, 165)
    for c in range(3):
        err, bound = float((got[c].double() - want[c].double()).abs().max()), 2.0 ** -22 * float(want[c].abs().max())
        print(f"channel {c}: max |gpu - cpu| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound


def test_run_case_volume_masked_zscore():
    img, seg = raw_case((5, 37, 131), (0, 3, 10), channels=1, seed=4)
    got, want, props = run_both(img, seg, (4.0, 1.0, 1.0), transpose_forward=(0, 2, 1), spacing=[4.0, 0.8, 1.3],
                                normalization_schemes=["ZScoreNormalization"], use_mask_for_norm=[True],
                                foreground_intensity_properties_per_channel=None)
    assert props["shape_before_cropping"] == (5, 131, 37) and props["shape_after_cropping_and_before_resampling"] == (5, 111, 31)
    assert tuple(want.shape) == (1, 5, 139, 24)
    err, bound = float((got.double() - want.double()).abs().max()), 2.0 ** -22 * float(want.abs().max())
    print(f"max |gpu - cpu| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound


# ------------------------------------------------------------------------------------------------ predict_from_raw
def test_predict_from_raw():
    """the smallest network of the end-to-end tests at 64 x 64 windows, one window per launch (windows of one launch meet in fp32 atomics,
    whose order is free; launches are ordered), a zero frame around the raw image and a resampling step"""
    from dinounet_amd import inference as INF
    from test_gpu_export import e2e_net
    net = e2e_net()
    img, _ = raw_case((1, 76, 110), (0, 8, 10), channels=3, seed=5)
    kw = dict(transpose_forward=(0, 1, 2), spacing=[0.9375, 0.9375], normalization_schemes=["ZScoreNormalization"] * 3,
              use_mask_for_norm=[False] * 3, foreground_intensity_properties_per_channel=None)
    pk = dict(tile_step_size=0.5, use_gaussian=True, batch_size=1)
    raw = torch.from_numpy(img).to(dev())
    props = {"spacing": (999.0, 1.0, 1.0)}
    seg = INF.predict_from_raw(net, raw, props, (64, 64), **kw, **pk)
    assert seg.dtype == torch.uint8 and tuple(seg.shape) == (1, 76, 110) and seg.is_cuda
    assert props["bbox_used_for_cropping"] == [[0, 1], [8, 68], [10, 100]]
    props2 = {"spacing": (999.0, 1.0, 1.0)}
    pre, _ = P.run_case(raw, None, props2, **kw)
    assert tuple(pre.shape) == (3, 1, 64, 96) and props2 == props
    want = INF.predict_segmentation(net, pre, (64, 64), properties=props2, transpose_backward=[0, 1, 2], **pk)
    assert torch.equal(seg, want)
    outside = torch.ones((1, 76, 110), dtype=torch.bool)
    outside[:, 8:68, 10:100] = False
    print(f"labels predicted: {torch.bincount(seg.flatten().long()).tolist()}")
    assert not seg.cpu()[outside].any()
    assert torch.equal(raw.cpu(), torch.from_numpy(img)), "the input was modified"
