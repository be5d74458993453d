"""GPU tests (-m gpu) of the export tail: du_export_seg and du_seg_counts (csrc/export.hip) through dinounet_amd.export against the
reference's fixture (tests/golden/export_reference.npz), against torch.argmax where no arithmetic is involved, against the float64
restatement where all arithmetic is exact, and predict_segmentation against predict_sliding_window_logits on a real network.

Bounds.  Labels: equal outside the tie band (1e-5 * max|logit|, a voxel is inside if its float64 top-two gap / any |logit| in region mode
is below it -- ten times the ~1e-6 * max|logit| fp32 error of normalisation plus four taps), at most 0.1 % of the voxels inside; exact
cases and every no-resample case: equal everywhere.  Probabilities: test_gpu_ops.rel < 2e-5, the fp32 gate of that file (measured maximum
over the fixture: see DESIGN).  End to end: every voxel on which two runs differ lies in the band of the logits and their share is below
1e-4, the bound test_sliding_window_inference_matches_oracle applies to two runs whose float-atomic order differs."""
import numpy as np
import pytest
import torch

from dinounet_amd import export as EX
from test_cpu_export import CASES, METRIC_CASES, Z, check_case_labels, check_metrics, lors_of
from test_gpu_ops import dev, gen, rel

pytestmark = pytest.mark.gpu

BAND_REL = 1e-5


def pow2(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.pow(2.0, torch.randint(-2, 4, shape, generator=g).float())


def region_labels(x, order):
    lab = torch.zeros(x.shape[1:], dtype=torch.uint8)
    for i, c in enumerate(order):
        lab[x[i] > 0] = c
    return lab


def in_band(z64, regions=False):
    """the tie band of float64 logits (K, ...): top-two gap (softmax) / any |logit| (regions) below 1e-5 * max|logit|"""
    band = BAND_REL * float(z64.abs().max())
    if regions:
        return (z64.abs() < band).any(0)
    top = z64.topk(2, dim=0).values
    return (top[0] - top[1]) < band


# ------------------------------------------------------------------------------------------------ the reference's fixture
@pytest.mark.parametrize("name", list(CASES))
def test_fixture_cases(name):
    c = CASES[name]
    d = dev()
    logits = torch.from_numpy(Z[f"{name}/logits"]).to(d)
    seg, probs = EX.logits_to_segmentation(logits, regions_class_order=c["regions_class_order"], properties=c["properties"],
                                           transpose_backward=c["transpose_backward"], return_probabilities=True)
    assert seg.is_cuda and probs.is_cuda and probs.dtype == torch.float32
    check_case_labels(name, seg)
    fig = rel(probs, torch.from_numpy(Z[f"{name}/probs"]))
    print(f"{name}: probabilities rel {fig:.3e}")
    assert fig < 2e-5
    # the same logits as window sums: n_predictions from powers of two, so sums / n_predictions gives the logits back exactly
    npred = pow2(tuple(logits.shape[1:]), 11).to(d)
    seg2, probs2 = EX.logits_to_segmentation(logits * npred, npred, regions_class_order=c["regions_class_order"], properties=c["properties"],
                                             transpose_backward=c["transpose_backward"], return_probabilities=True)
    assert torch.equal(seg2, seg) and torch.equal(probs2, probs)
    assert torch.equal(EX.logits_to_segmentation(logits, regions_class_order=c["regions_class_order"], properties=c["properties"],
                                                 transpose_backward=c["transpose_backward"]), seg)


# ------------------------------------------------------------------------------------------------ no resampling: no arithmetic
@pytest.mark.parametrize("shape", [(2, 1, 4, 4), (3, 2, 17, 23), (8, 1, 32, 32), (4, 3, 48, 40)])
def test_no_resample_equals_argmax(shape):
    d = dev()
    K, D, H, W = shape
    logits = (gen(*shape, seed=K * 100 + W) * 2.0).float()
    logits[:, :, ::3, ::2] = logits[:, :, ::3, ::2].round()                       # some exact ties among the maxima
    want = logits.argmax(0).to(torch.uint8)
    npred = pow2((D, H, W), 5)
    assert torch.equal(EX.logits_to_segmentation(logits.to(d)).cpu(), want)
    assert torch.equal(EX.logits_to_segmentation((logits * npred).to(d), npred.to(d)).cpu(), want)
    orders = {1: [5], 8: [3, 7, 1, 8, 2, 6, 4, 5]}
    # un-padding windows: odd and even x0, accumulator rows that are / are not a multiple of 4 wide (vector and guarded loads)
    for y0, x0, Wp in [(0, 0, W), (1, 1, W + 3), (2, 2, W + 8), (0, 3, W + 4), (3, 4, W + 4), (1, 6, W + 9)]:
        Hp = H + y0 + 2
        sums = torch.full((K, D, Hp, Wp), float("nan"))                           # the padding is never read
        nacc = torch.full((D, Hp, Wp), float("nan"))
        sums[:, :, y0:y0 + H, x0:x0 + W], nacc[:, y0:y0 + H, x0:x0 + W] = logits * npred, npred
        got = EX._export(sums.to(d), nacc.to(d), (y0, x0, H, W), None, None, None, False)
        assert torch.equal(got.cpu(), want), (y0, x0, Wp)
        for R, order in orders.items():
            if R <= K:
                got = EX._export(sums[:R].contiguous().to(d), nacc.to(d), (y0, x0, H, W), order, None, None, False)
                assert torch.equal(got.cpu(), region_labels(logits[:R], order)), (R, y0, x0, Wp)
    # pasted at an odd column of a larger volume, probabilities too: the kernel against the restatement's labels, bit for bit
    props = {"shape_before_cropping": [D + 1, H + 5, W + 6], "bbox_used_for_cropping": [[1, D + 1], [2, H + 2], [3, W + 3]],
             "shape_after_cropping_and_before_resampling": [D, H, W]}
    seg, probs = EX.logits_to_segmentation((logits * npred).to(d), npred.to(d), properties=props, return_probabilities=True)
    seg_c, probs_c = EX.logits_to_segmentation(logits * npred, npred, properties=props, return_probabilities=True)
    assert torch.equal(seg.cpu(), seg_c) and rel(probs, probs_c) < 2e-5


# ------------------------------------------------------------------------------------------------ exact resize
@pytest.mark.parametrize("factor", [2, 4])
def test_exact_resize_matches_float64(factor):
    """integer logits (|x| <= 8), 2x / 4x upsampling: every weight is dyadic, so fp32 equals float64 and labels are equal, ties included"""
    d = dev()
    K, D, H, W = 4, 2, 13, 18
    g = torch.Generator().manual_seed(factor)
    logits = torch.randint(-8, 9, (K, D, H, W), generator=g).float()
    npred = pow2((D, H, W), 9)
    props = {"shape_before_cropping": [D, H * factor + 3, W * factor + 1], "bbox_used_for_cropping": [[0, D], [3, H * factor + 3], [0, W * factor]],
             "shape_after_cropping_and_before_resampling": [D, H * factor, W * factor]}
    z = EX.resize_inplane_float64(logits, (H * factor, W * factor))
    top = z.topk(2, dim=0).values
    assert int((top[0] == top[1]).sum()) >= 20                                     # the ties are there
    for order in (None, [3, 1, 4, 2]):
        want = EX.logits_to_segmentation(logits, regions_class_order=order, properties=props)
        got = EX.logits_to_segmentation(logits.to(d), regions_class_order=order, properties=props)
        assert torch.equal(got.cpu(), want), order
        got = EX.logits_to_segmentation((logits * npred).to(d), npred.to(d), regions_class_order=order, properties=props)
        assert torch.equal(got.cpu(), want), order
    # one perturbed input must change the result
    want = EX.logits_to_segmentation(logits, properties=props)
    moved = logits.clone()
    k_new = (int(logits[:, 1, 5, 7].argmax()) + 1) % K
    moved[k_new, 1, 5, 7] = 100.0
    got = EX.logits_to_segmentation(moved.to(d), properties=props).cpu()
    assert not torch.equal(got, want) and torch.equal(got, EX.logits_to_segmentation(moved, properties=props))
    assert int(got[1, 3 + 5 * factor + factor // 2, 7 * factor + factor // 2]) == k_new
    assert torch.equal(got[0], want[0])                                            # slices are independent


# ------------------------------------------------------------------------------------------------ geometry
def raw_export(sums, npred, seg_ptr, probs_ptr, window, out_hw, before, corner, mode=0, order=0):
    from dinounet_amd import _lib
    K, D, Hp, Wp = sums.shape
    flag = torch.zeros(1, dtype=torch.int32, device=sums.device)
    rc = _lib.lib().du_export_seg(sums.data_ptr(), None if npred is None else npred.data_ptr(), seg_ptr, probs_ptr, flag.data_ptr(), K, D,
                                  Hp, Wp, *window, *out_hw, *before, *corner, mode, order, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, int(flag.item())


@pytest.mark.parametrize("out_hw", [(9, 14), (13, 21)])
def test_geometry_every_corner_and_guard_band(out_hw):
    """the bbox at every corner of a larger shape_before_cropping; seg and probs pre-filled: the kernel writes all of the volume and
    nothing around it (aligned and unaligned output pointers: word and byte stores)"""
    d = dev()
    K, D, H, W = 3, 2, 9, 14
    logits = (gen(K, D, H, W, seed=21) * 2.0).float()
    before = (D + 2, out_hw[0] + 3, out_hw[1] + 6)                                  # W0 = 20 (words) / 27 (bytes)
    n = before[0] * before[1] * before[2]
    for corner in [(a, b, c) for a in (0, 2) for b in (0, 3) for c in (0, 6)]:
        props = {"shape_before_cropping": list(before), "bbox_used_for_cropping": [[corner[0], corner[0] + D], [corner[1], corner[1] + out_hw[0]],
                                                                                    [corner[2], corner[2] + out_hw[1]]],
                 "shape_after_cropping_and_before_resampling": [D, *out_hw]}
        want_seg, want_probs = EX.logits_to_segmentation(logits, properties=props, return_probabilities=True)
        for guard in (64, 67):
            seg_buf = torch.full((n + 2 * guard,), 255, dtype=torch.uint8, device=d)
            probs_buf = torch.full((K * n + 2 * guard,), -7.0, dtype=torch.float32, device=d)
            rc, flag = raw_export(logits.to(d), None, seg_buf.data_ptr() + guard, probs_buf.data_ptr() + 4 * guard, (0, 0, H, W), out_hw, before,
                                  corner)
            assert rc == 0 and flag == 0
            seg = seg_buf[guard:guard + n].view(before).cpu()
            assert bool((seg_buf[:guard] == 255).all()) and bool((seg_buf[guard + n:] == 255).all()), (corner, guard)
            assert bool((probs_buf[:guard] == -7.0).all()) and bool((probs_buf[guard + K * n:] == -7.0).all()), (corner, guard)
            diff = seg != want_seg
            if out_hw == (H, W):
                assert not diff.any(), (corner, guard)
            else:
                z = EX.resize_inplane_float64(logits, out_hw)
                band = torch.zeros(before, dtype=torch.bool)
                band[corner[0]:corner[0] + D, corner[1]:corner[1] + out_hw[0], corner[2]:corner[2] + out_hw[1]] = in_band(z)
                assert not (diff & ~band).any(), (corner, guard)
            assert rel(probs_buf[guard:guard + K * n].view(K, *before), want_probs) < 2e-5, (corner, guard)


def test_error_codes():
    from dinounet_amd import _lib
    d = dev()
    x = torch.zeros((3, 2, 8, 8), device=d)
    seg = torch.zeros((2, 10, 10), dtype=torch.uint8, device=d)
    args = dict(window=(0, 0, 8, 8), out_hw=(8, 8), before=(2, 10, 10), corner=(0, 1, 2))
    assert raw_export(x, None, seg.data_ptr(), None, **args)[0] == 0
    assert raw_export(x, None, seg.data_ptr(), None, **dict(args, corner=(0, 1, 3)))[0] == -1            # bbox does not fit
    assert raw_export(x, None, seg.data_ptr(), None, **dict(args, corner=(1, 0, 0)))[0] == -1
    assert raw_export(x, None, seg.data_ptr(), None, **dict(args, window=(1, 0, 8, 8)))[0] == -1          # window outside the accumulators
    assert raw_export(torch.zeros((9, 2, 8, 8), device=d), None, seg.data_ptr(), None, **args)[0] == -2  # K out of range
    assert raw_export(torch.zeros((1, 2, 8, 8), device=d), None, seg.data_ptr(), None, **args)[0] == -2
    assert raw_export(torch.zeros((1, 2, 8, 8), device=d), None, seg.data_ptr(), None, mode=1, order=3, **args)[0] == 0
    with pytest.raises(ValueError, match="does not fit"):
        EX.logits_to_segmentation(x, properties={"shape_before_cropping": [2, 10, 10], "bbox_used_for_cropping": [[0, 2], [1, 9], [3, 11]],
                                                 "shape_after_cropping_and_before_resampling": [2, 8, 8]})
    # n >= 2^31 is refused before any launch
    L = _lib.lib()
    ws = torch.zeros(64, dtype=torch.int32, device=d)
    table, counts = torch.ones(1, dtype=torch.int64, device=d), torch.zeros((4, 1), dtype=torch.int64, device=d)
    assert L.du_seg_counts(seg.data_ptr(), seg.data_ptr(), table.data_ptr(), counts.data_ptr(), 2 ** 31, 1, 0, 0, ws.data_ptr(), 1 << 30, None) == -2
    assert L.du_seg_counts(seg.data_ptr(), seg.data_ptr(), table.data_ptr(), counts.data_ptr(), 200, 9, 0, 0, ws.data_ptr(), 64, None) == -2
    assert L.du_seg_counts_ws_elems(2 ** 31 - 1, 8) == 1024 * 25


# ------------------------------------------------------------------------------------------------ the flag
@pytest.mark.parametrize("out_hw", [(10, 12), (15, 18)])
def test_flag_reads_the_window_only(out_hw):
    d = dev()
    K, D, H, W = 3, 1, 10, 12
    logits = (gen(K, D, H, W, seed=2) * 2.0).float()
    sums, npred = torch.zeros((K, D, 14, 20)), torch.ones((D, 14, 20))
    sums[:, :, 2:12, 5:17] = logits
    props = {"shape_before_cropping": [D, *out_hw], "bbox_used_for_cropping": [[0, D], [0, out_hw[0]], [0, out_hw[1]]],
             "shape_after_cropping_and_before_resampling": [D, *out_hw]}
    window = (2, 5, H, W)
    clean = EX._export(sums.to(d), npred.to(d), window, None, props, None, False)
    outside = sums.clone()
    outside[:, :, :2], outside[:, :, 12:], outside[:, :, :, :5], outside[:, :, :, 17:] = float("inf"), float("inf"), float("nan"), float("inf")
    n_out = npred.clone()
    n_out[:, :2], n_out[:, :, 17:] = float("inf"), float("nan")
    assert torch.equal(EX._export(outside.to(d), n_out.to(d), window, None, props, None, False), clean)       # padding only: no error
    for k, y, x in [(0, 2, 5), (2, 11, 16), (1, 6, 9)]:
        bad = sums.clone()
        bad[k, 0, y, x] = float("inf")
        with pytest.raises(RuntimeError, match="Encountered inf in predicted array"):
            EX._export(bad.to(d), npred.to(d), window, None, props, None, False)
    if out_hw != (H, W):                                  # the normalised logits are needed: n_predictions is read
        bad_n = npred.clone()
        bad_n[0, 7, 7] = float("nan")
        with pytest.raises(RuntimeError, match="Encountered inf in predicted array"):
            EX._export(sums.to(d), bad_n.to(d), window, None, props, None, False)


# ------------------------------------------------------------------------------------------------ counts
@pytest.mark.parametrize("n", [1, 17 * 23, 64 * 64, 5 * 1024 * 1024])
def test_seg_counts_match_cpu(n):
    d = dev()
    g = torch.Generator().manual_seed(n % 1000)
    ref = torch.randint(0, 7, (n + 1,), generator=g, dtype=torch.uint8)
    pred = torch.where(torch.rand(n + 1, generator=g) < 0.6, ref, torch.randint(0, 6, (n + 1,), generator=g, dtype=torch.uint8))
    ref[n // 2], pred[n // 3] = 200, 77                                             # labels outside 0..63 are in no region
    ref_d, pred_d = ref.to(d), pred.to(d)
    regions = {1: [3], 8: [1, (1, 2, 3), (2, 3), 3, 0, (4, 5), 63, (0, 1, 2, 3, 4, 5, 6)]}
    for off in (0, 1):                                   # 16-byte vector loads / byte loads from an odd address
        for R, lors in regions.items():
            for ig in (None, 6):
                want = EX.segmentation_counts(pred[off:off + n], ref[off:off + n], lors, ig)
                got = EX.segmentation_counts(pred_d[off:off + n], ref_d[off:off + n], lors, ig)
                assert got.dtype == torch.int64 and got.shape == (4, R) and torch.equal(got, want), (off, R, ig)
                valid = n if ig is None else int((ref[off:off + n] != ig).sum())
                assert bool((got.sum(0) == valid).all()), (off, R, ig)


@pytest.mark.parametrize("name", list(METRIC_CASES))
def test_case_metrics_on_the_gpu(name):
    c = METRIC_CASES[name]
    d = dev()
    pred, ref = torch.from_numpy(Z[f"metrics_{name}/pred"]).to(d), torch.from_numpy(Z[f"metrics_{name}/ref"]).to(d)
    check_metrics(name, EX.case_metrics(pred, ref, lors_of(c), c["ignore_label"]))
    many = list(range(12))                                # more than 8 labels: several launches
    assert torch.equal(EX.segmentation_counts(pred, ref, many, c["ignore_label"]), EX.segmentation_counts(pred.cpu(), ref.cpu(), many, c["ignore_label"]))


# ------------------------------------------------------------------------------------------------ end to end
_E2E = {}


def e2e_net():
    if "net" not in _E2E:
        from oracle import weights
        from dinounet_amd.network_architecture import DinoUNet
        from dinounet_amd.plans import PLANS_2D
        net = DinoUNet.from_config(PLANS_2D, 3, 3, dinov3_pretrained_path=None, dinov3_model_name="dinounet_s", precision="fp32")
        ks = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
        net.load_state_dict(weights.make_state_dict(ks, seed=0), strict=True)
        _E2E["net"] = net.to(dev()).eval()
    return _E2E["net"]


def e2e_logits(shape, bs, mirror):
    """predict_sliding_window_logits of the shared network, once per (shape, mirroring)"""
    key = (shape, mirror)
    if key not in _E2E:
        from dinounet_amd import inference as INF
        _E2E[key] = INF.predict_sliding_window_logits(e2e_net(), gen(*shape, seed=7), (128, 128), tile_step_size=0.5, use_gaussian=True,
                                                      batch_size=bs, mirror_axes=mirror)
    return _E2E[key]


def assert_same_up_to_band(got, want, band):
    diff = got.cpu() != want.cpu()
    share = float(diff.float().mean())
    print(f"differing voxels {int(diff.sum())} of {diff.numel()}, in band {int(band.sum())}")
    assert not (diff & ~band).any() and share < 1e-4, (int(diff.sum()), int((diff & ~band).sum()), share)


@pytest.mark.parametrize("variant", ["eager", "graph", "mirror", "resample"])
@pytest.mark.parametrize("shape,bs", [((3, 2, 160, 200), 5), ((3, 1, 100, 128), 8)])
def test_predict_segmentation_end_to_end(shape, bs, variant):
    from dinounet_amd import inference as INF
    net = e2e_net()
    data = gen(*shape, seed=7)
    mirror = (0, 1) if variant == "mirror" else None
    logits = e2e_logits(shape, bs, mirror)
    D, H, W = shape[1:]
    assert logits.shape == (3, D, H, W)
    kw = dict(tile_step_size=0.5, use_gaussian=True, batch_size=bs, graph=variant == "graph", mirror_axes=mirror)
    if variant != "resample":
        seg = INF.predict_segmentation(net, data, (128, 128), **kw)
        assert seg.dtype == torch.uint8 and seg.shape == (D, H, W) and seg.is_cuda
        assert_same_up_to_band(seg, logits.argmax(0).to(torch.uint8), in_band(logits.double().cpu()))
    else:
        Ho, Wo = (3 * H) // 2, (3 * W) // 2
        props = {"shape_before_cropping": [D + 1, Ho + 7, Wo + 5], "bbox_used_for_cropping": [[1, D + 1], [4, Ho + 4], [5, Wo + 5]],
                 "shape_after_cropping_and_before_resampling": [D, Ho, Wo]}
        seg, probs = INF.predict_segmentation(net, data, (128, 128), properties=props, transpose_backward=(0, 2, 1), return_probabilities=True,
                                              **kw)
        want, want_probs = INF.logits_to_segmentation(logits, properties=props, transpose_backward=(0, 2, 1), return_probabilities=True)
        assert seg.shape == (D + 1, Wo + 5, Ho + 7) and probs.shape == (3, D + 1, Wo + 5, Ho + 7)
        band = torch.zeros((D + 1, Ho + 7, Wo + 5), dtype=torch.bool)
        band[1:, 4:Ho + 4, 5:Wo + 5] = in_band(EX.resize_inplane_float64(logits.cpu(), (Ho, Wo)))
        assert_same_up_to_band(seg, want, band.permute(0, 2, 1))
        assert rel(probs, want_probs) < 2e-5
    assert net.training is False
