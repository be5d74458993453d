"""Keeps the instruments of tests/_augment_ref.py honest without a GPU.  The fp64 references agree with scipy, numpy and the oracle's
restatements; the launch predicates reproduce the clamps of csrc/augment.hip and every listed shape lands in the form it is named for; an
fp32 emulation of each kernel passes its gate on every listed shape; each deliberately broken emulation is rejected by the gate meant for
it; the two exclusion caps (labels near a tie, gamma arguments below 1e-3 in apply()) hold for the reference alone."""
import numpy as np
import pytest
from scipy import ndimage

import _augment_ref as R
from oracle import augment_oracle as AO

f32, f64 = np.float32, np.float64


def inside(out, ref, bound):
    return R.within(out, ref, bound)[0]


# ---------------------------------------------------------------------------------------------------- launch predicates
def test_launch_predicates_reproduce_the_clamps():
    assert R.stats_passes(4) == (1, 0, 1) and R.stats_passes(1320) == (1, 0, 330) and R.stats_passes(4092) == (1, 0, 1023)
    assert R.stats_passes(4096) == (1, 1, 1024) and R.stats_passes(4100) == (2, 1, 1024) and R.stats_passes(262148) == (65, 64, 1024)
    for n, form in R.STATS_N.items():
        assert n % 4 == 0 and R.stats_form(n) == form
    assert R.plane_grid(4) == 1 and R.plane_grid(262144) == 1024 and R.plane_grid(262145) == 1024
    assert R.plane_sweeps(262144) == 1 and R.plane_sweeps(512 * 512) == 1 and R.plane_sweeps(262145) == 2
    for n, sweeps in R.POINT_N.items():
        assert R.plane_sweeps(n) == sweeps
    assert R.spatial_grid(16 * 512 * 512) == 16384 and R.spatial_sweeps(16 * 512 * 512) == 1
    B, _, H, W = R.CLAMP_CASE
    assert R.spatial_sweeps(B * H * W) == 2
    assert tuple(R.blur_radius(s) for s in R.BLUR_SIGMAS) == R.BLUR_RADII
    assert R.lowres_grid(0.5125, 40, 33) == (20, 17) and R.lowres_grid(0.5, 7, 5) == (4, 2)          # 20.5, 3.5, 2.5: ties to even
    for H, W in R.LOWRES_SHAPES:
        assert R.lowres_grid(0.01, H, W) == (1, 1) and R.lowres_grid(0.995, H, W) == (H, W)
        assert all(R.lowres_grid(z, H, W) is None for z in (0.0, 1.0, 1.3))


# ---------------------------------------------------------------------------------------------------- 1. statistics
@pytest.mark.parametrize("n", list(R.STATS_N))
def test_stats_emulation_passes_and_the_mutants_fail(n):
    x, want = R.two_value_planes(3, n, seed=n)
    assert np.array_equal(R.stats64(x), want)                            # numpy's own mean / std / min / max
    for p in range(3):
        assert np.array_equal(R.emu_stats(x[p]).astype(f64), want[p])
        if R.STATS_N[n] in ("ragged", "many"):
            assert not np.array_equal(R.emu_stats(x[p], drop_ragged=True).astype(f64)[:2], want[p, :2])
    xo = R.offset_planes(n, seed=100 + n)
    ref = R.stats64(xo)
    bm, bs = R.stats_bounds(xo)
    got = np.stack([R.emu_stats(row) for row in xo])
    old = np.stack([R.emu_stats(row, one_pass=True) for row in xo])
    assert np.array_equal(got[:, 2:].astype(f64), ref[:, 2:])
    assert inside(got[:, 0], ref[:, 0], bm) and inside(got[:, 1], ref[:, 1], bs), (n, got, ref, bm, bs)
    assert got[-1, 1] == 0 and got[-1, 0] == 33
    for p in (2, 3):                                                     # |m| / s = 600: the one-pass variance misses the bound
        assert abs(old[p, 1] - ref[p, 1]) > 10 * bs[p], (n, p, old[p, 1], ref[p, 1], bs[p])
    assert not inside(old[:, 1], ref[:, 1], bs)


def test_one_pass_bound_is_not_the_gate():
    """the gate is the two-pass bound: at |m| / s = 600 the one-pass formula's own bound is five orders of magnitude wider"""
    x = R.offset_planes(4096, seed=1)
    st = R.stats64(x)
    _, bs = R.stats_bounds(x)
    one_pass = (R.stats_depth(4096) + 4) * R.U * ((x.astype(f64) ** 2).mean(1) + st[:, 0] ** 2) / (2 * np.maximum(st[:, 1], 1e-30))
    assert one_pass[2] > 1e4 * bs[2]


# ---------------------------------------------------------------------------------------------------- 2. pointwise
@pytest.mark.parametrize("n", list(R.POINT_N))
def test_pointwise_emulations_pass_and_the_mutants_fail(n):
    x = R.point_planes(n, seed=n)
    st = R.stats_in(x)
    m = np.array([1.2, 0.8, 1.0, 0.75, 1.25, 1.0, 0.9, 1.1], f32)
    a, b = np.array([1.0, -1.0, 0.5, 1.0, 1.37, -2.1, 1.0, 0.3], f32), np.array([0.0, 0.0, 1.0, 0.25, -0.7, 3.0, 0.0, 0.0], f32)
    f = np.array([0.8, 1.0, 1.2, 0.77, 1.24, 1.0, 1.1, 1.25], f32)
    g = np.array([0.7, 1.0, 1.5, 0.0, 0.7, 1.5, -1.0, 1.0], f32)
    runs = [("mult", R.emu_mult(x, m), R.mult64(x, m)), ("affine", R.emu_affine(x, a, b), R.affine64(x, a, b)),
            ("contrast", R.emu_contrast(x, f, st), R.contrast64(x, f, st))]
    for inv in (0.0, 1.0):
        runs.append((f"gamma inv {inv}", R.emu_gamma(x, g, np.full(8, inv), st), R.gamma64(x, g, np.full(8, inv), st)[:2]))
    for what, out, (ref, bound) in runs:
        assert inside(out, ref, bound), R.within(out, ref, bound, what)[1]
        if R.POINT_N[n] > 1:                                             # a loop that stops after one sweep
            assert not inside(R.one_sweep(out, x), ref, bound), what
    # the clip omitted: the result leaves [min, max] and the gate
    raw = R.emu_contrast(x, f, st, clip=False)
    if n > 4:
        assert (raw.min(1) < st[:, 2]).any() and not inside(raw, *R.contrast64(x, f, st))
    out = R.emu_contrast(x, f, st)
    assert (out.min(1) >= st[:, 2]).all() and (out.max(1) <= st[:, 3]).all()
    # the oracle's restatements (statistics in fp64) agree with the references (statistics rounded to fp32) up to that rounding
    x64 = x.astype(f64)[None]
    assert np.abs(AO.contrast(x64, f[None])[0] - R.contrast64(x, f, st)[0]).max() < 1e-5
    for inv in (False, True):
        og = AO.gamma(x64, g[None], inv, retain_stats=False)[0]
        rg = R.gamma64(x, g, np.full(8, float(inv)), st)[0]
        assert np.abs(np.where((g > 0)[:, None], og - (-rg if inv else rg), 0.0)).max() < 1e-5


# ---------------------------------------------------------------------------------------------------- 3. blur
@pytest.mark.parametrize("H,W", R.BLUR_SHAPES)
def test_blur_reference_is_scipy_and_the_gate_sees_radius_and_reflection(H, W):
    sigma = np.array(R.BLUR_SIGMAS + (0.0,), f32)
    x = (np.random.RandomState(H * W).standard_normal((len(sigma), H, W)) + 0.5).astype(f32)
    for axis in (0, 1):
        ref = R.blur_axis(x, sigma, axis)
        for p, s in enumerate(sigma):
            want = ndimage.gaussian_filter1d(x[p].astype(f64), float(s), axis=axis, mode="reflect", truncate=4.0) if s > 0 else x[p]
            assert np.abs(ref[p] - want).max() < 1e-14, (axis, s)
        bound = R.blur_bound(x, sigma, axis)
        assert inside(R.blur_axis(x, sigma, axis, f32), ref, bound), R.within(R.blur_axis(x, sigma, axis, f32), ref, bound)[1]
        for shift in (-1, 1):
            assert not inside(R.blur_axis(x, sigma, axis, f32, r_shift=shift), ref, bound)
        if x.shape[1 + axis] == 3:                                       # the radius of 4 exceeds the axis: one reflection is not enough
            assert not inside(R.blur_axis(x, sigma, axis, f32, single=True), ref, bound)
    ref2, bound2 = R.blur2_64(x, sigma)
    for p, s in enumerate(sigma):
        want = ndimage.gaussian_filter(x[p].astype(f64), float(s), mode="reflect", truncate=4.0) if s > 0 else x[p]
        assert np.abs(ref2[p] - want).max() < 1e-14
    assert np.abs(ref2 - AO.blur(x.astype(f64)[None], sigma[None])[0]).max() < 1e-14
    assert inside(R.blur_axis(R.blur_axis(x, sigma, 0, f32), sigma, 1, f32), ref2, bound2)


# ---------------------------------------------------------------------------------------------------- 4. low resolution
@pytest.mark.parametrize("H,W", R.LOWRES_SHAPES)
def test_lowres_reference_is_the_oracle_and_the_emulation_passes(H, W):
    zoom = np.array(R.LOWRES_ZOOMS + R.LOWRES_COPIES, f32)
    x = (np.random.RandomState(H + W).standard_normal((len(zoom), H, W)) + 0.5).astype(f32)
    ref, bound = R.lowres64(x, zoom)
    k = len(R.LOWRES_ZOOMS)
    on = [p for p in range(len(zoom)) if R.lowres_grid(zoom[p], H, W) not in (None, (H, W))]
    assert on == list(range(k))
    assert np.abs(ref[:k] - AO.lowres(x.astype(f64)[None], zoom[None].astype(f64))[0][:k]).max() < 1e-12
    assert np.abs(ref[k:] - x[k:]).max() < 1e-12                         # 0.995 goes through the resampler at the full size: the same plane
    out = R.emu_lowres(x, zoom)
    assert inside(out, ref, bound), R.within(out, ref, bound, "lowres")[1]
    assert np.array_equal(out[k:], x[k:])                               # ... and bit for bit in fp32
    assert np.ptp(ref[3]) < 1e-12                                       # a 1 x 1 low grid: one value
    if (H, W) == (40, 33):
        # the gate sees the tie 20.5 rounded away from zero (roundf instead of rintf): a low grid of 21 rows, here through a zoom that gives 21
        z21 = f32(20.9 / 40)
        assert R.lowres_grid(z21, H, W) == (21, 17)
        assert not inside(R.lowres_plane(x[2], z21, f32)[None], ref[2:3], bound[2:3])


# ---------------------------------------------------------------------------------------------------- 5. noise
def test_noise_gates_pass_on_the_restated_generator_and_see_shared_fields():
    n, seed = R.NOISE_HW[0] * R.NOISE_HW[1], 1234

    def fields(**mutant):
        return np.stack([[[R.emu_normal(s, b * R.NOISE_C + c, n, **mutant) for c in range(R.NOISE_C)] for b in range(R.NOISE_B)]
                         for s in (seed, seed + 1)])
    assert R.noise_violations(fields()) == []
    bad = R.noise_violations(fields(same_plane=True))
    assert any("channels" in v for v in bad) and any("samples" in v for v in bad)
    bad = R.noise_violations(fields(same_seed=True))
    assert any("seeds" in v for v in bad)
    z = fields()
    assert R.noise_violations(np.clip(z, -2.9, 2.9)) != []              # no tails
    smooth = z.copy()
    smooth[..., 1:] = 0.8 * z[..., 1:] + 0.6 * z[..., :-1]
    assert any("lag 1" in v for v in R.noise_violations(smooth))
    assert float(np.sqrt(-2 * np.log(2.0 ** -24))) < R.Z_MAX


# ---------------------------------------------------------------------------------------------------- 6. spatial
SAMPLES = R.SAMPLES


@pytest.mark.parametrize("geo", list(R.SPATIAL_GEOS))
def test_spatial_reference_is_the_oracle_and_the_gate_sees_a_swapped_mirror(geo):
    Hi, Wi, Ho, Wo = R.SPATIAL_GEOS[geo]
    prm = np.stack([R.spatial_params(*s) for s in SAMPLES])
    data = R.spatial_image(len(SAMPLES), 2, Hi, Wi, seed=Hi)
    ref, bound = R.spatial64(data, prm, (Ho, Wo))
    assert np.abs(ref - AO.spatial(data, None, prm, (Ho, Wo))[0]).max() < 1e-12
    out, _ = R.emu_spatial(data, None, prm, (Ho, Wo))
    assert inside(out, ref, bound), R.within(out, ref, bound, geo)[1]
    if geo == "half-pixel":                                              # far taps alone inside the image: the Horner weights' absolute error shows
        assert not inside(R.emu_spatial(data, None, prm, (Ho, Wo), keys=R.keys_horner)[0], ref, bound)
    bad, _ = R.emu_spatial(data, None, prm, (Ho, Wo), mirror_swap=True)
    for b, s in enumerate(SAMPLES):
        assert inside(bad[b], ref[b], bound[b]) == (not (s[2] or s[3])), (geo, b)
    if (Hi - Ho) % 2 == 0:
        ident = np.stack([R.spatial_params(0.0, 1.0, fy, fx) for fy, fx in ((0, 0), (1, 0), (0, 1), (1, 1))])
        out, _ = R.emu_spatial(data[:4], None, ident, (Ho, Wo))
        for b in range(4):
            assert np.array_equal(out[b], R.centre_crop(data[b], ident[b], (Ho, Wo)))


def test_spatial_gate_sees_a_loop_that_stops_after_one_sweep():
    """the clamp case: one sweep of 16384 workgroups covers exactly 16 of the 17 samples; the emulation returns the input, the mutant
    leaves the last sample unwritten"""
    B, Cc, H, W = R.CLAMP_CASE
    assert R.spatial_grid(B * H * W) * 256 == (B - 1) * H * W
    data = np.random.RandomState(0).standard_normal((B, Cc, H, W)).astype(f32)
    prm = np.tile(R.IDENT, (B, 1))
    prm[-1, 4:] = 1
    out, _ = R.emu_spatial(data, None, prm, (H, W))
    want = data.copy()
    want[-1] = data[-1, :, ::-1, ::-1]
    assert np.array_equal(out, want)
    cut = R.spatial_one_sweep(out)
    assert np.array_equal(cut[:-1], want[:-1]) and not np.array_equal(cut[-1], want[-1])


@pytest.mark.parametrize("labels", R.LABEL_SETS)
@pytest.mark.parametrize("geo", ["crop", "pad"])
def test_label_reference_is_the_oracle_and_the_exclusion_cap_holds(geo, labels):
    Hi, Wi, Ho, Wo = R.SPATIAL_GEOS[geo]
    prm = np.stack([R.spatial_params(*s) for s in SAMPLES])
    B = len(SAMPLES)
    seg = np.tile(R.label_image(labels, Hi, Wi), (B, 1, 1))
    assert set(np.unique(seg)) == set(labels)
    assert all(len(np.unique(edge)) > 1 for edge in (seg[0, 0], seg[0, -1], seg[0, :, 0], seg[0, :, -1]))       # regions touch every border
    want, und = R.labels64(seg, prm, (Ho, Wo))
    data = np.zeros((B, 1, Hi, Wi), f32)
    assert np.array_equal(want, AO.spatial(data, seg[:, None], prm, (Ho, Wo))[1][:, 0])
    print(f"undecided share {geo} {labels}: {und.mean():.5f}")
    assert und.mean() <= 0.01
    _, got = R.emu_spatial(data, seg, prm, (Ho, Wo))
    assert not ((got != want) & ~und).any()
    _, bad = R.emu_spatial(data, seg, prm, (Ho, Wo), mirror_swap=True)
    assert ((bad != want) & ~und).any()
    _, bad = R.emu_spatial(data, seg, prm, (Ho, Wo), edge_interp=True)      # a label claimed up to half a pixel outside the image
    assert ((bad != want) & ~und).any()


# ---------------------------------------------------------------------------------------------------- 7. the whole apply()
def test_apply_reference_is_the_oracle_chain_and_its_exclusion_cap_holds():
    """apply64 is the oracle's functions chained in the reference's order; pixels whose normalised gamma argument is below 1e-3 are 1 % at
    the most for the reference alone; the tolerance is finite, positive and far below the data's spread"""
    data, draw, ref, tol, excl = R.apply_case()
    H, W = R.APPLY_GEO[2:]
    x = AO.spatial(data, None, draw["spatial"], (H, W))[0]
    x = AO.blur(x, draw["blur_sigma"])
    x = x * draw["mult"].astype(f64)[:, :, None, None]
    x = AO.lowres(AO.contrast(x, draw["contrast"]), draw["zoom"])
    x = AO.gamma(AO.gamma(x, draw["gamma_inv"], True), draw["gamma"], False)
    assert np.abs(x - ref).max() < 1e-12
    print(f"apply(): excluded share {excl.mean():.5f}, tolerance median {np.median(tol):.3e}, max {tol.max():.3e}")
    assert 0 < excl.mean() <= 0.01
    assert np.isfinite(tol).all() and (tol > 0).all() and tol[~excl].max() < 1e-3 * ref.std()
    for k in ("blur_sigma", "mult", "contrast", "zoom", "gamma_inv", "gamma"):            # plane 0 has every transform active
        off = {"mult": 1, "contrast": 1}.get(k, 0)
        assert draw[k][0, 0] != off
    # the |J| t written down for the linear stages is what the finite differences give
    t = np.abs(np.random.RandomState(0).standard_normal((H, W))) * 1e-6
    r = ref[0, 0]
    assert np.abs(R._carry(lambda v: R._st_blur(v, 0.7), r, t) - R._st_blur(t[None], 0.7)[0]).max() < 1e-12
    assert np.abs(R._st_lowres(r[None], 0.6)[0] - R.lowres_plane(r, 0.6)).max() < 1e-12


def test_apply_emulation_passes_and_the_mutants_fail():
    """the fp32 emulation of apply() lies inside the carried tolerance; the gammas applied in the wrong order, the inverted gamma's offset
    restored without its sign and the retain_stats rescale inverted do not; neither does the reference of the draw with the gammas swapped"""
    data, draw, ref, tol, excl = R.apply_case()
    H, W = R.APPLY_GEO[2:]

    def outside(out):
        return float(((np.abs(out - ref) > tol) & ~excl).mean())
    assert outside(R.emu_apply(data, draw, (H, W))) == 0
    wrong = tuple(R.STAGES[:4]) + ("gamma", "gamma_inv")
    assert outside(R.emu_apply(data, draw, (H, W), order=wrong)) > 0.1
    assert outside(R.emu_apply(data, draw, (H, W), forget_sign=True)) > 0.1
    assert outside(R.emu_apply(data, draw, (H, W), inverse_rescale=True)) > 0.1
    assert outside(R.apply_case(True)[2]) > 0.1
