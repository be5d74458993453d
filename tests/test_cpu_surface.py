"""CPU tests of the surface metrics (dinounet_amd/export.py: surface_metrics, border_distance_sq, case_metrics(spacing=...)): the scipy /
numpy restatement of medpy.metric.hd95 / asd against brute force (border by explicit neighbour loops, distances as the float64 minimum
over all border voxels, the percentile by sorting) on volumes of at most 12^3 voxels, the fixed cases, the key order of case_metrics.
The GPU tests (tests/test_gpu_surface.py) compare the kernels with this restatement and take their volumes from here.

Bounds.  Border and counts: equal.  Squared distances: equal for spacings whose products are exact in fp64 (every candidate cost is exact
and the minimum is unique as a value), 8 * 2^-53 relative otherwise.  HD95 / ASD against brute force: 4 * 2^-53 (exact spacings: the same
order statistics, one rounding each in the root and the interpolation) and n * 2^-52 (a sum of n non-negative doubles in any order)."""
import math

import numpy as np
import pytest
import torch

from dinounet_amd import export as EX

U = 2.0 ** -53
EXACT_SPACINGS = [(1.0, 1.0, 1.0), (3.0, 1.0, 1.0), (2.5, 0.75, 0.75), (1.0, 0.5, 2.0)]
INEXACT_SPACING = (3.0, 0.7, 0.7)


# ------------------------------------------------------------------------------------------------ label maps (shared with the GPU tests)
def blob_maps(shape, seed, n_labels=3):
    """seeded blobs of labels 1 .. n_labels that touch every face of the volume, and a perturbed copy as the prediction"""
    D, H, W = shape
    rng = np.random.RandomState(seed)
    zz, yy, xx = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    ref = np.zeros(shape, dtype=np.uint8)
    corners = [(0, 0, 0), (D - 1, H - 1, W - 1), (0, H - 1, 0), (D - 1, 0, W - 1)]
    for i in range(3 * n_labels + 4):
        c = corners[i] if i < 4 else (rng.randint(D), rng.randint(H), rng.randint(W))
        r = (max(1.0, D * rng.uniform(0.15, 0.5)), max(1.5, H * rng.uniform(0.1, 0.35)), max(1.5, W * rng.uniform(0.1, 0.35)))
        inside = ((zz - c[0]) / r[0]) ** 2 + ((yy - c[1]) / r[1]) ** 2 + ((xx - c[2]) / r[2]) ** 2 <= 1.0
        ref[inside] = 1 + i % n_labels
    pred = np.roll(ref, (D > 2, 1, -2), axis=(0, 1, 2)).copy()
    flip = rng.rand(*shape) < 0.02
    pred[flip] = rng.randint(0, n_labels + 1, size=int(flip.sum())).astype(np.uint8)
    return torch.from_numpy(pred), torch.from_numpy(ref)


def hand_maps(shape):
    """label 1: a block in a corner region (rows and whole slices of the volume hold no border voxel of it); label 2: one voxel; label 3:
    in the reference only; label 4: in the prediction only; region (0, 1, 2, 3, 4) fills the volume"""
    D, H, W = shape
    ref = np.zeros(shape, dtype=np.uint8)
    ref[: max(1, D // 3), 1: max(2, H // 3), 2: max(3, W // 2)] = 1
    ref[D - 1, H - 1, W - 1] = 2
    ref[D // 2, H // 2:, : W // 3] = 3
    pred = ref.copy()
    pred[pred == 3] = 0
    pred[: max(1, D // 3), 1: max(2, H // 3) + 1, 2: max(3, W // 2) - 1] = 1
    pred[pred == 2] = 0
    pred[D - 1, H - 2, W - 1] = 2
    pred[D // 2, 0, W - 1] = 4
    return torch.from_numpy(pred), torch.from_numpy(ref)


HAND_REGIONS = [1, 2, 3, 4, (0, 1, 2, 3, 4), (1, 3)]


# ------------------------------------------------------------------------------------------------ brute force
def brute_mask(seg, r):
    labels = r if isinstance(r, tuple) else (r,)
    m = np.zeros(seg.shape, dtype=bool)
    for l in labels:
        m |= seg == l
    return m


def brute_border(mask):
    D, H, W = mask.shape
    out = np.zeros_like(mask)
    for z in range(D):
        for y in range(H):
            for x in range(W):
                if not mask[z, y, x]:
                    continue
                for dz, dy, dx in ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)):
                    a, b, c = z + dz, y + dy, x + dx
                    if not (0 <= a < D and 0 <= b < H and 0 <= c < W) or not mask[a, b, c]:
                        out[z, y, x] = True
    return out


def brute_dist_sq(border, spacing):
    """float64 minimum over all border voxels of (dz sz)^2 + (dy sy)^2 + (dx sx)^2, the squares added in that order"""
    pts = np.argwhere(border).astype(np.float64)
    if len(pts) == 0:
        return np.full(border.shape, np.inf)
    grid = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in border.shape], indexing="ij"), -1).reshape(-1, 1, 3)
    off = (grid - pts[None]) * np.asarray(spacing, dtype=np.float64)
    sq = off * off
    return ((sq[..., 0] + sq[..., 1]) + sq[..., 2]).min(1).reshape(border.shape)


def brute_percentile95(values):
    s = sorted(values)
    vi = (len(s) - 1) * 0.95
    lo = math.floor(vi)
    a, b, t = s[lo], s[min(lo + 1, len(s) - 1)], vi - lo
    return a + (b - a) * t


def brute_surface(pred, ref, r, spacing):
    mp, mr = brute_mask(pred, r), brute_mask(ref, r)
    bp, br = brute_border(mp), brute_border(mr)
    out = {"HD95": math.nan, "ASD": math.nan, "n_surface_pred": int(bp.sum()), "n_surface_ref": int(br.sum())}
    if mp.any() and mr.any():
        d_pr = np.sqrt(brute_dist_sq(br, spacing)[bp])
        d_rp = np.sqrt(brute_dist_sq(bp, spacing)[br])
        out["HD95"] = brute_percentile95(list(d_pr) + list(d_rp))
        out["ASD"] = math.fsum(d_pr) / len(d_pr)
    return out


def close(got, want, bound):
    if math.isnan(want):
        return math.isnan(got)
    if want == 0.0:
        return got == 0.0
    return abs(got - want) <= bound * abs(want)


def fields_close(got, want, bound):
    """equal where either is not finite (inf means no border voxel at all), |got - want| <= bound * want elsewhere"""
    fin = np.isfinite(want) & np.isfinite(got)
    return np.array_equal(got[~fin], want[~fin]) and bool(np.all(np.abs(got[fin] - want[fin]) <= bound * want[fin]))


SMALL = [((4, 7, 9), 3), ((1, 11, 12), 4), ((12, 12, 12), 5), ((3, 5, 6), 6)]


# ------------------------------------------------------------------------------------------------ the restatement against brute force
@pytest.mark.parametrize("shape,seed", SMALL)
def test_border_and_distance_match_brute_force(shape, seed):
    pred, ref = blob_maps(shape, seed)
    for r in [1, 2, (1, 3), 7]:
        want_b = brute_border(brute_mask(ref.numpy(), r))
        for sp in EXACT_SPACINGS + [INEXACT_SPACING]:
            border, d2 = EX.border_distance_sq(ref, list(r) if isinstance(r, tuple) else r, sp)
            assert border.dtype == torch.bool and d2.dtype == torch.float64 and tuple(d2.shape) == shape
            assert np.array_equal(border.numpy(), want_b)
            want = brute_dist_sq(want_b, sp)
            if sp in EXACT_SPACINGS:
                assert np.array_equal(d2.numpy(), want), (r, sp)
            else:
                assert fields_close(d2.numpy(), want, 8 * U), (r, sp)
    assert np.isinf(EX.border_distance_sq(ref, 7, (1, 1, 1))[1].numpy()).all()


@pytest.mark.parametrize("shape,seed", SMALL)
def test_surface_metrics_match_brute_force(shape, seed):
    pred, ref = blob_maps(shape, seed)
    lors = [1, 2, 3, (1, 2), (2, 3, 1), 9]
    for sp in EXACT_SPACINGS + [INEXACT_SPACING]:
        got = EX.surface_metrics(pred, ref, lors, sp)
        assert list(got) == lors
        for r in lors:
            want = brute_surface(pred.numpy(), ref.numpy(), r, sp)
            g = got[r]
            assert list(g) == ["HD95", "ASD", "n_surface_pred", "n_surface_ref"]
            assert g["n_surface_pred"] == want["n_surface_pred"] and g["n_surface_ref"] == want["n_surface_ref"]
            hd_bound = 4 * U if sp in EXACT_SPACINGS else 16 * U
            assert close(g["HD95"], want["HD95"], hd_bound), (r, sp, g["HD95"], want["HD95"])
            assert close(g["ASD"], want["ASD"], max(1, want["n_surface_pred"]) * 2 * U), (r, sp, g["ASD"], want["ASD"])


def test_hand_map_matches_brute_force():
    pred, ref = hand_maps((5, 9, 10))
    got = EX.surface_metrics(pred, ref, HAND_REGIONS, (2.5, 0.75, 0.75))
    for r in HAND_REGIONS:
        want = brute_surface(pred.numpy(), ref.numpy(), r, (2.5, 0.75, 0.75))
        assert got[r]["n_surface_pred"] == want["n_surface_pred"] and got[r]["n_surface_ref"] == want["n_surface_ref"]
        assert close(got[r]["HD95"], want["HD95"], 4 * U) and close(got[r]["ASD"], want["ASD"], max(1, want["n_surface_pred"]) * 2 * U)
    assert math.isnan(got[3]["HD95"]) and math.isnan(got[4]["ASD"])               # on one side only
    assert got[3]["n_surface_ref"] > 0 and got[3]["n_surface_pred"] == 0


# ------------------------------------------------------------------------------------------------ fixed cases
def test_single_slice_border_is_the_mask():
    pred, ref = blob_maps((1, 9, 11), 8)
    border, d2 = EX.border_distance_sq(ref, 1, (5.0, 1.0, 1.0))
    assert torch.equal(border, ref == 1) and bool((d2[border] == 0).all())
    m = EX.surface_metrics(pred, ref, [1], (5.0, 1.0, 1.0))[1]
    assert m["n_surface_pred"] == int((pred == 1).sum()) and m["n_surface_ref"] == int((ref == 1).sum())


def test_empty_side_is_nan():
    pred, ref = blob_maps((3, 8, 8), 9)
    none = torch.zeros_like(ref)
    for a, b in [(none, ref), (pred, none), (none, none)]:
        m = EX.surface_metrics(a, b, [1, (1, 2)], (1, 1, 1))
        for r in [1, (1, 2)]:
            assert math.isnan(m[r]["HD95"]) and math.isnan(m[r]["ASD"])


def test_identical_maps_are_zero():
    _, ref = blob_maps((4, 9, 9), 10)
    m = EX.surface_metrics(ref, ref.clone(), [1, 2, (1, 2, 3)], (2.5, 0.75, 0.75))
    for r in m:
        assert m[r]["HD95"] == 0.0 and m[r]["ASD"] == 0.0 and m[r]["n_surface_pred"] == m[r]["n_surface_ref"] > 0


def test_single_voxels_hand_value():
    pred = torch.zeros((4, 6, 7), dtype=torch.uint8)
    ref = torch.zeros_like(pred)
    pred[0, 1, 2] = 1
    ref[3, 5, 4] = 1
    sp = (2.0, 0.5, 1.5)
    want = math.sqrt((3 * 2.0) ** 2 + (4 * 0.5) ** 2 + (2 * 1.5) ** 2)                 # 36 + 4 + 9 = 49
    m = EX.surface_metrics(pred, ref, [1], sp)[1]
    assert want == 7.0 and m == {"HD95": 7.0, "ASD": 7.0, "n_surface_pred": 1, "n_surface_ref": 1}


# ------------------------------------------------------------------------------------------------ case_metrics
def test_case_metrics_without_spacing_is_unchanged():
    pred, ref = blob_maps((3, 10, 9), 11)
    lors = [1, 2, [1, 2], (3,)]
    a, b = EX.case_metrics(pred, ref, lors, ignore_label=3), EX.case_metrics(pred, ref, lors, ignore_label=3, spacing=None)
    assert list(a) == list(b)
    for r in a:
        assert list(a[r]) == list(b[r]) == ["Dice", "IoU", "Sensitivity", "Specificity", "Precision", "FP", "TP", "FN", "TN", "n_pred", "n_ref"]
        for k in a[r]:
            assert a[r][k] == b[r][k] or (math.isnan(a[r][k]) and math.isnan(b[r][k]))


def test_case_metrics_with_spacing_key_order_and_values():
    pred, ref = blob_maps((3, 10, 9), 11)
    lors = [1, 2, [1, 2], 9]
    sp = (3.0, 1.0, 1.0)
    m = EX.case_metrics(pred, ref, lors, ignore_label=3, spacing=sp)
    plain = EX.case_metrics(pred, ref, lors, ignore_label=3)
    surf = EX.surface_metrics(pred, ref, lors, sp)
    assert list(m) == [1, 2, (1, 2), 9]
    for r in m:
        # the order in which compute_metrics fills its dict (evaluate_predictions.py:189-234)
        assert list(m[r]) == ["Dice", "IoU", "Sensitivity", "Specificity", "Precision", "HD95", "ASD", "FP", "TP", "FN", "TN", "n_pred", "n_ref"]
        for k in plain[r]:
            assert m[r][k] == plain[r][k] or (math.isnan(m[r][k]) and math.isnan(plain[r][k]))
        for k in ("HD95", "ASD"):
            assert m[r][k] == surf[r][k] or (math.isnan(m[r][k]) and math.isnan(surf[r][k]))
    assert math.isnan(m[9]["HD95"]) and m[1]["HD95"] > 0


# ------------------------------------------------------------------------------------------------ errors
def test_errors():
    pred, ref = blob_maps((2, 6, 6), 12)
    ok = (1.0, 1.0, 1.0)
    with pytest.raises(ValueError):
        EX.surface_metrics(pred.int(), ref, [1], ok)
    with pytest.raises(ValueError):
        EX.surface_metrics(pred[:1], ref, [1], ok)
    with pytest.raises(ValueError):
        EX.surface_metrics(pred, ref, [], ok)
    with pytest.raises(ValueError):
        EX.surface_metrics(pred[0], ref[0], [1], ok)                                  # 2-D maps: pass D == 1
    for bad in [(1.0, 1.0), (1.0, 1.0, 0.0), (1.0, -1.0, 1.0), (1.0, 1.0, float("inf")), (1.0, 1.0, float("nan")), None, 1.0]:
        with pytest.raises(ValueError):
            EX.surface_metrics(pred, ref, [1], bad)
    with pytest.raises(ValueError):
        EX.border_distance_sq(pred.float(), 1, ok)
    with pytest.raises(ValueError):
        EX.case_metrics(pred, ref, [1], spacing=(1.0, 1.0))
