"""CPU tests of the export tail (dinounet_amd/export.py): the float64 torch restatement of du_export_seg and the torch path of the
per-case counts against the reference's own results (tests/golden/export_reference.npz, tools/make_golden_export.py), the interpolation
against scipy.ndimage.zoom, every error the interface raises.  The GPU tests (tests/test_gpu_export.py) compare the kernels with this path.

Bounds.  Labels: equal to the reference outside the case's tie band (stored per case; 0 for the exact cases), at most 0.1 % of the voxels
inside it.  Probabilities: the restatement evaluates softmax / sigmoid in float64 and rounds once, the reference rounds the resampled logits
to fp32 and evaluates in fp32: 2e-6 relative to the largest probability (a few fp32 ulps of the logits, which are < 16 here).  Interpolation
against zoom: 1e-12 absolute on N(0, 2) logits (float64 round-off of two 2-tap sums)."""
import inspect
import json
import math
import os

import numpy as np
import pytest
import torch

from dinounet_amd import export as EX

GOLD = os.path.join(os.path.dirname(__file__), "golden", "export_reference.npz")


def load_fixture():
    z = np.load(GOLD)
    return z, json.loads(str(z["meta"]))


Z, META = load_fixture()
CASES = {c["name"]: c for c in META["cases"]}
METRIC_CASES = {c["name"]: c for c in META["metric_cases"]}
RESIZES = [((17, 23), (40, 31)), ((64, 64), (37, 129)), ((33, 20), (33, 47)), ((20, 30), (7, 9)), ((12, 10), (24, 40))]


def check_case_labels(name, seg):
    """labels equal the reference outside the band; the band holds at most the capped share of the voxels"""
    c = CASES[name]
    want, band = Z[f"{name}/seg"], Z[f"{name}/band"].astype(bool)
    got = seg.cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    n_bbox = int(np.prod(c["properties"]["shape_after_cropping_and_before_resampling"]))
    assert int(band.sum()) == c["n_inband"] and band.sum() <= META["band_cap"] * n_bbox, name
    if c["exact"]:
        assert not band.any()
    diff = got != want
    assert not (diff & ~band).any(), (name, int(diff.sum()), int((diff & ~band).sum()))


def lors_of(c):
    return [tuple(r) if isinstance(r, list) else r for r in c["labels_or_regions"]]


def check_metrics(name, metrics):
    c = METRIC_CASES[name]
    table = Z[f"metrics_{name}/table"]
    for i, r in enumerate(lors_of(c)):
        for j, k in enumerate(META["metric_keys"]):
            got, want = metrics[r][k], table[i, j]
            if math.isnan(want):
                assert math.isnan(got), (name, r, k, got)
            elif j < 5:
                assert isinstance(got, float) and got == want, (name, r, k, got, want)      # same int64 counts, same float64 division
            else:
                assert isinstance(got, int) and got == int(want), (name, r, k, got, want)
        assert set(metrics[r]) == set(META["metric_keys"])


@pytest.mark.parametrize("name", list(CASES))
def test_torch_path_matches_reference(name):
    c = CASES[name]
    logits = torch.from_numpy(Z[f"{name}/logits"])
    seg, probs = EX.logits_to_segmentation(logits, regions_class_order=c["regions_class_order"], properties=c["properties"],
                                           transpose_backward=c["transpose_backward"], return_probabilities=True)
    check_case_labels(name, seg)
    want = Z[f"{name}/probs"]
    assert probs.dtype == torch.float32 and tuple(probs.shape) == want.shape
    err = float(np.abs(probs.numpy() - want).max() / np.abs(want).max())
    print(f"{name}: probabilities max rel err {err:.3e}")
    assert err < 2e-6
    only = EX.logits_to_segmentation(logits, regions_class_order=c["regions_class_order"], properties=c["properties"],
                                     transpose_backward=c["transpose_backward"])
    assert torch.equal(only, seg)


def test_fixture_covers_the_listed_cases():
    kinds = {(c["kind"], c["C"]) for c in CASES.values()}
    assert {("softmax", 2), ("softmax", 3), ("softmax", 8), ("regions", 1), ("regions", 3), ("regions", 4)} <= kinds
    assert any(c["regions_class_order"] and c["regions_class_order"] != sorted(c["regions_class_order"]) for c in CASES.values())
    assert any(c["exact"] for c in CASES.values()) and any(c["transpose_backward"] != [0, 1, 2] for c in CASES.values())
    sides = set()
    for c in CASES.values():
        p = c["properties"]
        sides.add(sum(int(lo == 0) + int(hi == n) for (lo, hi), n in zip(p["bbox_used_for_cropping"], p["shape_before_cropping"])))
    assert {0, 1, 6} <= sides
    assert os.path.getsize(GOLD) < 400 * 1024


@pytest.mark.parametrize("src,dst", RESIZES)
def test_float64_restatement_matches_scipy_zoom(src, dst):
    from scipy.ndimage import zoom
    g = torch.Generator().manual_seed(src[0] * 1000 + dst[1])
    x = (torch.randn((2, *src), generator=g) * 2.0).float()
    got = EX.resize_inplane_float64(x, dst).numpy()
    assert got.dtype == np.float64 and got.shape == (2, *dst)
    for i in range(2):
        want = zoom(x[i].numpy().astype(np.float64), (dst[0] / src[0], dst[1] / src[1]), order=1, mode="nearest", grid_mode=True)
        assert np.abs(got[i] - want).max() < 1e-12
    lo, hi, w = EX.source_taps(src[0], dst[0])
    pos = (np.arange(dst[0]) + 0.5) * src[0] / dst[0] - 0.5                                   # the half-pixel map
    assert np.abs(np.clip(pos, 0, src[0] - 1) - np.clip(lo.numpy() + w.numpy() * (hi.numpy() - lo.numpy()), 0, src[0] - 1)).max() < 1e-12


def test_sums_with_npred_equal_finished_logits():
    """un-normalised sums with n_predictions drawn from powers of two (exact products) give the labels of the logits, with and without
    resampling; a padded window is cut out first"""
    g = torch.Generator().manual_seed(3)
    logits = (torch.randn((3, 2, 17, 23), generator=g) * 2.0).float()
    npred = torch.pow(2.0, torch.randint(-2, 4, (2, 17, 23), generator=g).float())
    for props in (None, {"shape_before_cropping": [3, 50, 40], "bbox_used_for_cropping": [[1, 3], [5, 45], [2, 33]],
                         "shape_after_cropping_and_before_resampling": [2, 40, 31]}):
        a = EX.logits_to_segmentation(logits, properties=props)
        b = EX.logits_to_segmentation(logits * npred, npred, properties=props)
        assert torch.equal(a, b)
    big, bign = torch.full((3, 2, 20, 30), float("inf")), torch.ones((2, 20, 30))
    big[:, :, 1:18, 4:27], bign[:, 1:18, 4:27] = logits * npred, npred
    seg = EX._export(big, bign, (1, 4, 17, 23), None, None, None, False)                     # an inf in the padding is never read
    assert torch.equal(seg, logits.argmax(0).to(torch.uint8))


@pytest.mark.parametrize("name", list(METRIC_CASES))
def test_case_metrics_match_reference(name):
    c = METRIC_CASES[name]
    pred, ref = torch.from_numpy(Z[f"metrics_{name}/pred"]), torch.from_numpy(Z[f"metrics_{name}/ref"])
    metrics = EX.case_metrics(pred, ref, lors_of(c), c["ignore_label"])
    check_metrics(name, metrics)
    counts = EX.segmentation_counts(pred, ref, lors_of(c), c["ignore_label"])
    valid = int((ref != c["ignore_label"]).sum()) if c["ignore_label"] is not None else ref.numel()
    assert counts.dtype == torch.int64 and bool((counts.sum(0) == valid).all())


def test_metrics_nan_for_absent_label():
    m = EX.case_metrics(torch.zeros((1, 4, 4), dtype=torch.uint8), torch.zeros((1, 4, 4), dtype=torch.uint8), [0, 1])
    assert m[0]["Dice"] == 1.0 and math.isnan(m[0]["Specificity"])
    assert all(math.isnan(m[1][k]) for k in ("Dice", "IoU", "Sensitivity", "Precision")) and m[1]["Specificity"] == 1.0 and m[1]["TN"] == 16


def test_value_errors():
    x = torch.zeros((3, 2, 8, 8))
    with pytest.raises(ValueError, match="classes"):
        EX.logits_to_segmentation(torch.zeros((1, 2, 8, 8)))
    with pytest.raises(ValueError, match="classes"):
        EX.logits_to_segmentation(torch.zeros((9, 2, 8, 8)))
    with pytest.raises(ValueError, match="regions"):
        EX.logits_to_segmentation(torch.zeros((9, 2, 8, 8)), regions_class_order=list(range(1, 10)))
    with pytest.raises(ValueError, match="entries"):
        EX.logits_to_segmentation(x, regions_class_order=[1, 2])
    with pytest.raises(ValueError, match="254"):
        EX.logits_to_segmentation(x, regions_class_order=[1, 2, 255])
    ok = {"shape_before_cropping": [2, 10, 10], "bbox_used_for_cropping": [[0, 2], [1, 9], [2, 10]],
          "shape_after_cropping_and_before_resampling": [2, 8, 8]}
    assert EX.logits_to_segmentation(x, properties=ok).shape == (2, 10, 10)
    for bad_bbox in ([[0, 2], [1, 9], [3, 11]], [[0, 2], [-1, 7], [2, 10]], [[0, 2], [1, 8], [2, 10]]):
        with pytest.raises(ValueError, match="does not fit"):
            EX.logits_to_segmentation(x, properties=dict(ok, bbox_used_for_cropping=bad_bbox))
    with pytest.raises(ValueError, match="out-of-plane resampling is not supported"):
        EX.logits_to_segmentation(x, properties=dict(ok, shape_after_cropping_and_before_resampling=[4, 8, 8],
                                                     bbox_used_for_cropping=[[0, 4], [1, 9], [2, 10]], shape_before_cropping=[4, 10, 10]))
    with pytest.raises(ValueError, match="permutation"):
        EX.logits_to_segmentation(x, transpose_backward=(0, 1, 1))
    with pytest.raises(ValueError, match="uint8"):
        EX.case_metrics(torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.uint8), [1])


def test_non_finite_logits_raise():
    x = torch.zeros((2, 1, 8, 8))
    x[1, 0, 3, 4] = float("inf")
    with pytest.raises(RuntimeError, match="Encountered inf in predicted array"):
        EX.logits_to_segmentation(x)
    n = torch.ones((1, 8, 8))
    n[0, 0, 0] = float("nan")
    with pytest.raises(RuntimeError, match="Encountered inf in predicted array"):
        EX.logits_to_segmentation(torch.zeros((2, 1, 8, 8)), n)


def test_inference_interface_unchanged():
    from dinounet_amd import inference as INF
    sig = inspect.signature(INF.predict_sliding_window_logits)
    assert list(sig.parameters) == ["net", "data", "patch_size", "tile_step_size", "use_gaussian", "batch_size", "graph", "mirror_axes"]
    assert [p.default for p in sig.parameters.values()][3:] == [0.5, True, 8, False, None]
    assert INF.logits_to_segmentation is EX.logits_to_segmentation and INF.predict_segmentation is EX.predict_segmentation
    assert INF.case_metrics is EX.case_metrics
    win = list(inspect.signature(EX.predict_segmentation).parameters)
    assert win[:8] == list(sig.parameters) and win[8:] == ["regions_class_order", "properties", "transpose_backward", "return_probabilities"]
