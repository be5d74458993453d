"""GPU tests (-m gpu) of the surface metrics: the border, distance-transform and gather kernels of csrc/surface.hip through
dinounet_amd.export (border_distance_sq, surface_metrics, case_metrics(spacing=...)) against the scipy / numpy restatement the CPU path
runs (tests/test_cpu_surface.py checks that restatement against brute force).

Bounds, all properties of fp64 arithmetic and none of the data (no tie band, no case left out).  Border bits and surface counts: equal.
Squared distance field: bit for bit (inf included) for the spacings whose products are exact, against the squared offsets to scipy's own
nearest border voxel added in axis order; 8 * 2^-53 relative for the inexact spacing (three products and two sums per candidate, and
candidates at equal distance whose offsets differ).  HD95: 4 * 2^-53 (exact spacings: identical order statistics, the rounding of the
interpolation formula) / 16 * 2^-53 (inexact).  ASD: n * 2^-52 with n the prediction's surface count (a sum of n non-negative doubles in
any order plus one rounding per square root)."""
import functools
import math

import numpy as np
import pytest
import torch

from dinounet_amd import export as EX
from test_cpu_surface import EXACT_SPACINGS, HAND_REGIONS, INEXACT_SPACING, U, blob_maps, close, fields_close, hand_maps
from test_gpu_ops import dev

pytestmark = pytest.mark.gpu

VOLUMES = [(1, 5, 7), (1, 32, 32), (3, 17, 23), (2, 64, 130), (9, 33, 65), (5, 40, 48), (4, 256, 256)]
SPACINGS = EXACT_SPACINGS + [INEXACT_SPACING]
REGIONS = [1, 2, 3, (1, 2), (3, 1, 2)]
HAND_VOLUME = (9, 33, 65)


@functools.lru_cache(maxsize=None)
def maps(shape):
    return blob_maps(shape, seed=100 + shape[1]) if shape != "hand" else hand_maps(HAND_VOLUME)


@functools.lru_cache(maxsize=None)
def want_field(shape, region, spacing):
    """(border, dist_sq) of the reference map from the restatement, computed once"""
    b, d = EX.border_distance_sq(maps(shape)[1], list(region) if isinstance(region, tuple) else region, spacing)
    return b.numpy(), d.numpy()


@functools.lru_cache(maxsize=None)
def want_metrics(shape, regions, spacing):
    pred, ref = maps(shape)
    return EX.surface_metrics(pred, ref, list(regions), spacing)


def check_metrics(got, want, spacing):
    assert list(got) == list(want)
    hd_bound = (4 if spacing in EXACT_SPACINGS else 16) * U
    for r in want:
        g, w = got[r], want[r]
        print(f"{r}: HD95 {g['HD95']!r} vs {w['HD95']!r}, ASD {g['ASD']!r} vs {w['ASD']!r}, surface {g['n_surface_pred']} / {g['n_surface_ref']}")
        assert list(g) == ["HD95", "ASD", "n_surface_pred", "n_surface_ref"]
        assert g["n_surface_pred"] == w["n_surface_pred"] and g["n_surface_ref"] == w["n_surface_ref"], r
        assert close(g["HD95"], w["HD95"], hd_bound), (r, spacing, g["HD95"], w["HD95"])
        assert close(g["ASD"], w["ASD"], max(1, w["n_surface_pred"]) * 2 * U), (r, spacing, g["ASD"], w["ASD"])


def check_field(shape, region, spacing):
    d = dev()
    ref = maps(shape)[1].to(d)
    border, d2 = EX.border_distance_sq(ref, list(region) if isinstance(region, tuple) else region, spacing)
    assert border.is_cuda and d2.is_cuda and border.dtype == torch.bool and d2.dtype == torch.float64
    wb, wd = want_field(shape, region, spacing)
    assert np.array_equal(border.cpu().numpy(), wb), (shape, region)
    got = d2.cpu().numpy()
    if spacing in EXACT_SPACINGS:
        assert np.array_equal(got, wd), (shape, region, spacing, int((got != wd).sum()))
    else:
        fin = np.isfinite(wd)
        worst = float(np.max(np.abs(got[fin] - wd[fin]) / np.maximum(wd[fin], 1e-300))) if fin.any() else 0.0
        print(f"{shape} {region} {spacing}: largest relative difference {worst / U:.2f} * 2^-53")
        assert fields_close(got, wd, 8 * U), (shape, region, spacing)


# ------------------------------------------------------------------------------------------------ border, counts, distance field
@pytest.mark.parametrize("shape", VOLUMES)
def test_border_and_surface_counts(shape):
    d = dev()
    pred, ref = maps(shape)
    want = want_metrics(shape, tuple(REGIONS), SPACINGS[0])
    got = EX.surface_metrics(pred.to(d), ref.to(d), REGIONS, SPACINGS[0])
    for r in REGIONS:
        border, _ = EX.border_distance_sq(ref.to(d), r, SPACINGS[0])
        wb = want_field(shape, r, SPACINGS[0])[0]
        assert np.array_equal(border.cpu().numpy(), wb)
        assert got[r]["n_surface_ref"] == int(wb.sum()) == want[r]["n_surface_ref"]
        assert got[r]["n_surface_pred"] == want[r]["n_surface_pred"]
    if shape[0] == 1:                                                                 # D == 1: the border is the mask
        assert torch.equal(EX.border_distance_sq(ref.to(d), 1, SPACINGS[0])[0].cpu(), ref == 1)


@pytest.mark.parametrize("spacing", SPACINGS)
@pytest.mark.parametrize("shape", VOLUMES)
def test_distance_field(shape, spacing):
    for region in [1, (1, 2, 3)]:
        check_field(shape, region, spacing)


def test_distance_field_without_border_is_inf():
    d = dev()
    _, d2 = EX.border_distance_sq(maps((3, 17, 23))[1].to(d), 9, (1.0, 1.0, 1.0))
    assert bool(torch.isinf(d2).all()) and bool((d2 > 0).all())


@pytest.mark.parametrize("spacing", [SPACINGS[2], SPACINGS[4]])
def test_hand_map_fields(spacing):
    """rows and whole slices without a border voxel, a region that fills the volume, a single voxel, a region absent from this side"""
    for region in HAND_REGIONS:
        check_field("hand", region, spacing)


# ------------------------------------------------------------------------------------------------ HD95 / ASD
@pytest.mark.parametrize("spacing", SPACINGS)
@pytest.mark.parametrize("shape", VOLUMES)
def test_hd95_asd(shape, spacing):
    d = dev()
    pred, ref = maps(shape)
    check_metrics(EX.surface_metrics(pred.to(d), ref.to(d), REGIONS, spacing), want_metrics(shape, tuple(REGIONS), spacing), spacing)


@pytest.mark.parametrize("spacing", SPACINGS)
def test_hand_map_metrics(spacing):
    d = dev()
    pred, ref = maps("hand")
    got = EX.surface_metrics(pred.to(d), ref.to(d), HAND_REGIONS, spacing)
    check_metrics(got, want_metrics("hand", tuple(HAND_REGIONS), spacing), spacing)
    assert math.isnan(got[3]["HD95"]) and math.isnan(got[4]["ASD"]) and got[3]["n_surface_ref"] > 0 and got[4]["n_surface_pred"] == 1


def test_two_runs_same_bits():
    d = dev()
    pred, ref = (t.to(d) for t in maps((4, 256, 256)))
    a = EX.surface_metrics(pred, ref, REGIONS, INEXACT_SPACING)
    b = EX.surface_metrics(pred, ref, REGIONS, INEXACT_SPACING)
    for r in REGIONS:
        for k in a[r]:
            assert np.float64(a[r][k]).tobytes() == np.float64(b[r][k]).tobytes(), (r, k)


def test_eleven_regions_cross_the_chunk():
    d = dev()
    shape, sp = (5, 40, 48), SPACINGS[2]
    pred, ref = maps(shape)
    lors = [1, 2, 3, (1, 2), (1, 3), (2, 3), (1, 2, 3), (0,), (0, 1), 7, (3, 2)]
    assert len(lors) == 11
    got = EX.surface_metrics(pred.to(d), ref.to(d), lors, sp)
    check_metrics(got, want_metrics(shape, tuple(lors), sp), sp)
    assert math.isnan(got[7]["HD95"])
    alone = EX.surface_metrics(pred.to(d), ref.to(d), [(3, 2)], sp)                   # position in a chunk changes nothing
    assert alone[(3, 2)] == got[(3, 2)]


def test_empty_region_inside_a_chunk():
    d = dev()
    shape, sp = (9, 33, 65), INEXACT_SPACING
    pred, ref = (t.to(d) for t in maps(shape))
    without = EX.surface_metrics(pred, ref, [1, 2, (1, 3)], sp)
    mixed = EX.surface_metrics(pred, ref, [1, 9, 2, (40, 41), (1, 3)], sp)
    for r in (9, (40, 41)):
        assert math.isnan(mixed[r]["HD95"]) and math.isnan(mixed[r]["ASD"]) and mixed[r]["n_surface_pred"] == mixed[r]["n_surface_ref"] == 0
    for r in without:
        assert mixed[r] == without[r], r
    # a label on one side only: its own result is nan, its border field still exists and the other regions do not move
    pred2 = pred.clone()
    pred2[pred2 == 2] = 0
    one_side = EX.surface_metrics(pred2, ref, [1, 2, (1, 3)], sp)
    assert math.isnan(one_side[2]["HD95"]) and one_side[2]["n_surface_ref"] == without[2]["n_surface_ref"] and one_side[2]["n_surface_pred"] == 0
    check_metrics(one_side, EX.surface_metrics(pred2.cpu(), ref.cpu(), [1, 2, (1, 3)], sp), sp)


def test_case_metrics_on_the_device_equals_the_cpu_path():
    d = dev()
    shape, sp = (5, 40, 48), SPACINGS[3]
    pred, ref = maps(shape)
    lors = [1, 2, [1, 2], 3, 9]
    want = EX.case_metrics(pred, ref, lors, ignore_label=3, spacing=sp)
    got = EX.case_metrics(pred.to(d), ref.to(d), lors, ignore_label=3, spacing=sp)
    plain = EX.case_metrics(pred.to(d), ref.to(d), lors, ignore_label=3)
    assert list(got) == list(want)
    for r in want:
        assert list(got[r]) == list(want[r])
        n = EX.surface_metrics(pred, ref, [r], sp)[tuple(r) if isinstance(r, list) else r]["n_surface_pred"]
        for k in want[r]:
            g, w = got[r][k], want[r][k]
            if k == "HD95":
                assert close(g, w, 4 * U), (r, k, g, w)
            elif k == "ASD":
                assert close(g, w, max(1, n) * 2 * U), (r, k, g, w)
            else:
                assert g == w or (math.isnan(g) and math.isnan(w)), (r, k, g, w)
                assert g == plain[r][k] or math.isnan(g)


def test_supported_extents():
    d = dev()
    ok = (1.0, 1.0, 1.0)
    for shape in [(1025, 1, 1), (1, 1025, 2), (1, 1, 1025)]:
        big = torch.zeros(shape, dtype=torch.uint8, device=d)
        with pytest.raises(ValueError):
            EX.surface_metrics(big, big, [1], ok)
        with pytest.raises(ValueError):
            EX.border_distance_sq(big, 1, ok)
    with pytest.raises(ValueError):
        EX.surface_metrics(torch.zeros((2, 4, 4), dtype=torch.uint8, device=d), torch.zeros((2, 4, 4), dtype=torch.uint8), [1], ok)
    with pytest.raises(ValueError):
        EX.surface_metrics(torch.zeros((4, 4), dtype=torch.uint8, device=d), torch.zeros((4, 4), dtype=torch.uint8, device=d), [1], ok)
    # the longest supported axis, one line of voxels: every scan at its largest extent
    line = torch.zeros((1, 1, 1024), dtype=torch.uint8, device=d)
    line[0, 0, 3] = 1
    line[0, 0, 1000] = 1
    for perm in [(0, 1, 2), (2, 0, 1), (0, 2, 1)]:
        seg = line.permute(*perm).contiguous()
        border, d2 = EX.border_distance_sq(seg, 1, ok)
        assert int(border.sum()) == 2
        idx = torch.arange(1024, dtype=torch.float64)
        want = torch.minimum((idx - 3) ** 2, (idx - 1000) ** 2)
        assert torch.equal(d2.flatten().cpu(), want)
