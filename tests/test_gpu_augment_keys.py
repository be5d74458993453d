"""The Keys augmentation kernels of csrc/augment.hip (GPUAugment2D(interpolation="keys"), the default training augmentation), each called
through the C ABI with parameters and statistics supplied by the test, per element against fp64 (tests/_augment_ref.py, kept honest by
tests/test_cpu_augment_keys.py), in every launch form: idle threads, one, a ragged second and many passes of the statistics kernel; the
grid-stride loops of the plane kernels past the 1024-workgroup clamp; du_aug_spatial past its 16384 workgroups; non-square outputs.

Instruments.  Exact inputs where the arithmetic allows (integer planes with exact mean and std, identity resampling, copies): bit for
bit.  Elsewhere a per-element bound derived in _augment_ref.py; the worst share of each bound is printed.  Buffers a kernel writes are
pre-filled with the sentinel and followed by a guard band.

GPUAugment2D.apply() as a whole: against the oracle's functions chained in fp64 with the stage bounds carried through the later stages, and
to the bit against the same kernels called one by one in the reference's order."""
import numpy as np
import pytest
import torch

import _augment_ref as R
from test_gpu_ops import dev
from test_gpu_small_ops import assert_flat_guard, call, flat_guarded, ok, untouched
from test_gpu_small_ops import P as ptr

pytestmark = pytest.mark.gpu

f32 = torch.float32


def up(a, d):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(d)


def down(t):
    return t.detach().cpu().numpy()


def guarded_copy(a, d):
    """(whole, view): the array a in a sentinel-guarded device buffer (for kernels that work in place)"""
    a = np.ascontiguousarray(a, np.float32)
    whole, view = flat_guarded(a.size, f32, d)
    view.copy_(torch.from_numpy(a).reshape(-1))
    return whole, view


def gate(out, ref64, bound, what):
    good, msg, _ = R.within(out, ref64, bound, what)
    print("[share] " + msg)
    assert good, msg


# ---------------------------------------------------------------------------------------------------- 1. du_aug_plane_stats
def run_stats(x, d):
    P_, n = x.shape
    xg = up(x, d)
    whole, st = flat_guarded(P_ * 4, f32, d)
    ok("du_aug_plane_stats", ptr(xg), ptr(st), P_, n)
    assert_flat_guard(whole, P_ * 4, what=f"plane_stats n {n}")
    return down(st).reshape(P_, 4)


@pytest.mark.parametrize("n", list(R.STATS_N))
def test_plane_stats_integer_planes_to_the_bit(n):
    """planes m +- s with integer m and s: every sum of the kernel is an exact integer, so mean (mean n is the integer sum), std, min and max
    equal the fp64 values bit for bit -- with idle threads, in one pass, with a ragged second pass and over 65 passes"""
    d = dev()
    assert R.stats_form(n) == R.STATS_N[n], (n, R.stats_passes(n))
    x, want = R.two_value_planes(5, n, seed=n)
    got = run_stats(x, d).astype(np.float64)
    assert np.array_equal(got, want), f"n {n}: got {got.tolist()}, want {want.tolist()}"


@pytest.mark.parametrize("n", list(R.STATS_N))
def test_plane_stats_offset_planes_within_the_two_pass_bound(n):
    """planes m + s z at |m| / s up to 600 and a constant plane: mean and std within the bound of a two-pass fp32 algorithm (relative to
    the plane's spread, R.stats_bounds), min and max exact, the constant plane's std exactly 0.  The one-pass E[x^2] - mean^2 this kernel
    used to compute misses the bound of the offset rows by orders of magnitude (tests/test_cpu_augment_keys.py keeps it as a mutant)."""
    d = dev()
    x = R.offset_planes(n, seed=100 + n)
    got, want = run_stats(x, d), R.stats64(x)
    bm, bs = R.stats_bounds(x)
    for p in range(x.shape[0]):
        print(f"n {n} plane {p}: mean {got[p, 0]!r} (fp64 {want[p, 0]!r}, bound {bm[p]:.3e}), std {got[p, 1]!r} (fp64 {want[p, 1]!r}, bound {bs[p]:.3e})")
    assert np.array_equal(got[:, 2:].astype(np.float64), want[:, 2:])
    gate(got[:, 0], want[:, 0], bm, f"stats mean n {n}")
    gate(got[:, 1], want[:, 1], bs, f"stats std n {n}")
    assert got[-1, 1] == 0.0 and got[-1, 0] == 33.0


def test_plane_stats_declines_a_ragged_plane_without_a_launch():
    d = dev()
    xg = up(np.ones((2, 6)), d)
    whole, st = flat_guarded(8, f32, d)
    assert call("du_aug_plane_stats", ptr(xg), ptr(st), 2, 6) == -1
    torch.cuda.synchronize()
    assert untouched(whole)


# ---------------------------------------------------------------------------------------------------- 2. contrast, gamma, affine, multiplier
def in_place(name, x, d, *params):
    """an in-place plane kernel on x (P, n) with per-plane parameter arrays -> result (P, n) as numpy"""
    P_, n = x.shape
    whole, v = guarded_copy(x, d)
    dv = [up(a, d) for a in params]
    ok(name, ptr(v), *[ptr(t) for t in dv], P_, n)
    assert_flat_guard(whole, P_ * n, what=name, written=False)
    return down(v).reshape(P_, n)


def noise_mult(x, sigma, mult, seed, d):
    P_, n = x.shape
    whole, v = guarded_copy(x, d)
    sg, m = up(sigma, d), up(mult, d)
    ok("du_aug_noise_mult", ptr(v), ptr(sg), ptr(m), P_, n, seed)
    assert_flat_guard(whole, P_ * n, what="noise_mult", written=False)
    return down(v).reshape(P_, n)


@pytest.mark.parametrize("n", list(R.POINT_N))
def test_multiplier_and_affine(n):
    d = dev()
    assert R.plane_sweeps(n) == R.POINT_N[n]
    x = R.point_planes(n, seed=n)
    m = np.array([1.2, 0.8, 1.0, 0.75, 1.25, 1.0, 0.9, 1.1], np.float32)
    out = noise_mult(x, np.zeros(8), m, 0, d)
    gate(out, *R.mult64(x, m), f"multiplier n {n}")
    assert np.array_equal(out[m == 1], x[m == 1])
    a = np.array([1.0, -1.0, 0.5, 1.0, 1.37, -2.1, 1.0, 0.3], np.float32)
    b = np.array([0.0, 0.0, 1.0, 0.25, -0.7, 3.0, 0.0, 0.0], np.float32)
    out = in_place("du_aug_affine", x, d, a, b)
    gate(out, *R.affine64(x, a, b), f"affine n {n}")
    off = (a == 1) & (b == 0)
    assert off.sum() == 2 and np.array_equal(out[off], x[off])


@pytest.mark.parametrize("n", list(R.POINT_N))
def test_contrast(n):
    """per element against fp64; no output outside [min, max]; for factors above 1 the elements at min and at max stay put (below 1 the
    transform itself pulls them towards the mean); factor 1 leaves the plane untouched"""
    d = dev()
    x = R.point_planes(n, seed=10 + n)
    f = np.array([0.8, 1.0, 1.2, 0.77, 1.24, 1.0, 1.1, 1.25], np.float32)
    st = R.stats_in(x)
    P_ = x.shape[0]
    whole, v = guarded_copy(x, d)
    fg, sg = up(f, d), up(st, d)
    ok("du_aug_contrast", ptr(v), ptr(fg), ptr(sg), P_, n)
    assert_flat_guard(whole, P_ * n, what="contrast", written=False)
    out = down(v).reshape(P_, n)
    ref, bound = R.contrast64(x, f, st)
    gate(out, ref, bound, f"contrast n {n}")
    assert np.array_equal(out[f == 1], x[f == 1])
    assert (out.min(1) >= st[:, 2]).all() and (out.max(1) <= st[:, 3]).all()
    for p in np.nonzero(f > 1)[0]:
        assert out[p, x[p].argmin()] == st[p, 2] and out[p, x[p].argmax()] == st[p, 3]


@pytest.mark.parametrize("inverted", [False, True], ids=["plain", "inverted"])
@pytest.mark.parametrize("n", list(R.POINT_N))
def test_gamma(n, inverted):
    """the body of GammaTransform on x or on -x with g in {0.7, 1.0, 1.5}; g <= 0 leaves the plane untouched; a constant plane (range 0)
    comes back as the constant"""
    d = dev()
    x = R.point_planes(n, seed=20 + n)
    g = np.array([0.7, 1.0, 1.5, 0.0, 0.7, 1.5, -1.0, 1.0], np.float32)
    inv = np.full(8, float(inverted), np.float32)
    st = R.stats_in(x)
    out = in_place("du_aug_gamma", x, d, g, inv, st)
    ref, bound, _ = R.gamma64(x, g, inv, st)
    gate(out, ref, bound, f"gamma n {n} {'inverted' if inverted else 'plain'}")
    assert np.array_equal(out[g <= 0], x[g <= 0])
    assert (out[-1] == (-x[-1] if inverted else x[-1])).all()
    # range 0 with every g: 0^g 0 + min, finite and the constant itself
    const = np.stack([np.full(n, v, np.float32) for v in (1.75, -0.3, 2.5)])
    gc = np.array([0.7, 1.0, 1.5], np.float32)
    out = in_place("du_aug_gamma", const, d, gc, inv[:3], R.stats_in(const))
    assert np.isfinite(out).all() and np.array_equal(out, -const if inverted else const)


# ---------------------------------------------------------------------------------------------------- 3. du_aug_blur
def run_blur(x, sigma, axis, d):
    P_, H, W = x.shape
    xg, sg = up(x, d), up(sigma, d)
    whole, y = flat_guarded(x.size, f32, d)
    ok("du_aug_blur", ptr(xg), ptr(y), ptr(sg), P_, H, W, axis)
    assert_flat_guard(whole, x.size, what=f"blur {H} x {W} axis {axis}")
    return down(y).reshape(P_, H, W)


@pytest.mark.parametrize("H,W", R.BLUR_SHAPES, ids=[f"{h}x{w}" for h, w in R.BLUR_SHAPES])
def test_blur_each_axis_and_both(H, W):
    """one launch with sigma 0.1 (radius 0), 0.374, 0.375, 0.625, 1.0 and 0 mixed over its planes: each axis on its own and the two passes
    against the fp64 filter (scipy's gaussian_filter1d / gaussian_filter, tests/test_cpu_augment_keys.py); radius-0 planes bit-identical.
    On the 3-pixel axes the radius exceeds the axis and the reflection repeats"""
    d = dev()
    sigma = np.array(R.BLUR_SIGMAS + (0.0,), np.float32)
    assert tuple(R.blur_radius(s) for s in R.BLUR_SIGMAS) == R.BLUR_RADII
    x = (np.random.RandomState(H * W).standard_normal((len(sigma), H, W)) + 0.5).astype(np.float32)
    copies = np.array([R.blur_radius(s) == 0 for s in sigma])
    y1 = None
    for axis in (0, 1):
        out = run_blur(x, sigma, axis, d)
        gate(out, R.blur_axis(x, sigma, axis), R.blur_bound(x, sigma, axis), f"blur {H} x {W} axis {axis}")
        assert np.array_equal(out[copies], x[copies])
        y1 = out if axis == 0 else y1
    out2 = run_blur(y1, sigma, 1, d)
    gate(out2, *R.blur2_64(x, sigma), f"blur {H} x {W} both passes")


# ---------------------------------------------------------------------------------------------------- 4. du_aug_lowres
@pytest.mark.parametrize("H,W", R.LOWRES_SHAPES, ids=[f"{h}x{w}" for h, w in R.LOWRES_SHAPES])
def test_lowres(H, W):
    """zooms 0.5, 0.77, 0.5125 (40 x 0.5125 = 20.5 in fp32: ties to even) and 0.01 (a 1 x 1 low grid: one value) against fp64; zooms 0, 1, 1.3
    and 0.995 (rint gives the full size) are bit-identical copies"""
    d = dev()
    zoom = np.array(R.LOWRES_ZOOMS + R.LOWRES_COPIES, np.float32)
    if (H, W) == (40, 33):
        assert R.lowres_grid(0.5125, H, W)[0] == 20 and float(np.float32(40) * np.float32(0.5125)) == 20.5
    assert R.lowres_grid(0.01, H, W) == (1, 1) and R.lowres_grid(0.995, H, W) == (H, W)
    x = (np.random.RandomState(H + W).standard_normal((len(zoom), H, W)) + 0.5).astype(np.float32)
    xg, zg = up(x, d), up(zoom, d)
    whole, y = flat_guarded(x.size, f32, d)
    ok("du_aug_lowres", ptr(xg), ptr(y), ptr(zg), len(zoom), H, W)
    assert_flat_guard(whole, x.size, what=f"lowres {H} x {W}")
    out = down(y).reshape(x.shape)
    gate(out, *R.lowres64(x, zoom), f"lowres {H} x {W}")
    k = len(R.LOWRES_ZOOMS)
    assert np.array_equal(out[k:], x[k:])


# ---------------------------------------------------------------------------------------------------- 5. noise
def noise_field(sigma, seed, n, d):
    """the field of du_aug_noise_mult on zeros with multiplier 1: (B C, n)"""
    P_ = R.NOISE_B * R.NOISE_C
    return noise_mult(np.zeros((P_, n), np.float32), np.full(P_, sigma, np.float32), np.ones(P_, np.float32), seed, d)


def test_noise_field():
    """deterministic; counter-based (element i does not depend on n); sigma scales the field to one rounding; independent between channels,
    samples, seeds s and s + 1 and neighbouring elements; normal deciles and tails; finite and inside the Box-Muller ceiling"""
    d = dev()
    n, seed = R.NOISE_HW[0] * R.NOISE_HW[1], 1234
    z0, z1 = noise_field(1.0, seed, n, d), noise_field(1.0, seed + 1, n, d)
    assert np.array_equal(z0, noise_field(1.0, seed, n, d))
    assert np.array_equal(noise_field(1.0, seed, 4096, d), z0[:, :4096])
    assert np.array_equal(noise_field(0.3, seed, n, d), np.float32(0.3) * z0)
    z = np.stack([z0, z1]).reshape(2, R.NOISE_B, R.NOISE_C, n)
    bad = R.noise_violations(z)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------- 6. du_aug_spatial
SAMPLES = R.SAMPLES


def run_spatial(data, seg, prm, patch, d):
    B, Cc, Hi, Wi = data.shape
    Ho, Wo = patch
    dg, pg = up(data, d), up(prm, d)
    sg = None if seg is None else up(seg, d)
    whole, out = flat_guarded(B * Cc * Ho * Wo, f32, d)
    swhole, sout = flat_guarded(B * Ho * Wo, f32, d)
    ok("du_aug_spatial", ptr(dg), None if seg is None else ptr(sg), ptr(pg), ptr(out), None if seg is None else ptr(sout), B, Cc, Hi, Wi, Ho, Wo)
    assert_flat_guard(whole, out.numel(), what="spatial image")
    assert_flat_guard(swhole, sout.numel(), what="spatial labels", written=seg is not None)
    return out.view(B, Cc, Ho, Wo), (None if seg is None else sout.view(B, Ho, Wo))


@pytest.mark.parametrize("geo", list(R.SPATIAL_GEOS))
def test_spatial_image_within_the_bound(geo):
    """rotations 0, pi / 2 and 0.6, scales 0.8 and 1.3, flips of y, of x and of both on a 48 x 40 output with content that is asymmetric on
    both axes, from an input larger than the patch, smaller on one axis (zero padding) and with odd size differences (half-pixel identity):
    per element against the fp64 Keys resampler.  A flipped sample is bit for bit its unflipped twin, flipped"""
    d = dev()
    Hi, Wi, Ho, Wo = R.SPATIAL_GEOS[geo]
    prm = np.stack([R.spatial_params(*s) for s in SAMPLES])
    data = R.spatial_image(len(SAMPLES), 2, Hi, Wi, seed=Hi)
    out, _ = run_spatial(data, None, prm, (Ho, Wo), d)
    gate(down(out), *R.spatial64(data, prm, (Ho, Wo)), f"spatial image {geo}")
    same = run_spatial(data[[4, 3]], None, prm[[5, 6]], (Ho, Wo), d)[0]      # the twins' data under the flipped parameters
    plain = run_spatial(data[[4, 3]], None, prm[[4, 3]], (Ho, Wo), d)[0]
    assert torch.equal(same[0], plain[0].flip(-2)) and torch.equal(same[1], plain[1].flip(-1))


@pytest.mark.parametrize("geo", ["crop", "pad"])
def test_spatial_identity_is_the_centre_crop(geo):
    """no rotation, no scale, even size differences: image and labels are torch.equal to the centre crop (zeros where the patch is larger than
    the input), unflipped and under each flip"""
    d = dev()
    Hi, Wi, Ho, Wo = R.SPATIAL_GEOS[geo]
    prm = np.stack([R.spatial_params(0.0, 1.0, fy, fx) for fy, fx in ((0, 0), (1, 0), (0, 1), (1, 1))])
    data = R.spatial_image(4, 2, Hi, Wi, seed=3)
    seg = np.stack([R.label_image(R.LABEL_SETS[b % 2], Hi, Wi) for b in range(4)])
    out, sout = run_spatial(data, seg, prm, (Ho, Wo), d)
    for b in range(4):
        assert np.array_equal(down(out[b]), R.centre_crop(data[b], prm[b], (Ho, Wo))), (geo, b)
        assert np.array_equal(down(sout[b]), R.centre_crop(seg[b], prm[b], (Ho, Wo))), (geo, b)


def test_spatial_past_the_workgroup_clamp():
    """17 x 512 x 512 outputs are more than the 16384 workgroups of 256 cover in one sweep (the production batch of 16 is exactly one):
    identity, the last sample flipped on both axes, torch.equal to the input"""
    d = dev()
    B, Cc, H, W = R.CLAMP_CASE
    assert R.spatial_sweeps(B * H * W) == 2 and R.spatial_sweeps((B - 1) * H * W) == 1 and R.spatial_grid(B * H * W) == 16384
    g = torch.Generator().manual_seed(5)
    data = torch.randn(B, Cc, H, W, generator=g).to(d)
    prm = np.tile(R.IDENT, (B, 1))
    prm[-1, 4:] = 1
    pg = up(prm, d)
    whole, out = flat_guarded(data.numel(), f32, d)
    ok("du_aug_spatial", ptr(data), None, ptr(pg), ptr(out), None, B, Cc, H, W, H, W)
    assert_flat_guard(whole, data.numel(), what="spatial past the clamp")
    out = out.view(B, Cc, H, W)
    assert torch.equal(out[:-1], data[:-1]) and torch.equal(out[-1], data[-1].flip(-1, -2))


@pytest.mark.parametrize("labels", R.LABEL_SETS, ids=["0123", "027"])
@pytest.mark.parametrize("geo", ["crop", "pad"])
def test_spatial_labels_follow_the_order1_rule(geo, labels):
    """labels equal the fp64 rule exactly, except where the reference's deciding score lies within twice the coordinate error of 0.5; those
    pixels are excluded and may be 1 % at the most (the reference alone: tests/test_cpu_augment_keys.py)"""
    d = dev()
    Hi, Wi, Ho, Wo = R.SPATIAL_GEOS[geo]
    prm = np.stack([R.spatial_params(*s) for s in SAMPLES])
    B = len(SAMPLES)
    seg = np.tile(R.label_image(labels, Hi, Wi), (B, 1, 1))
    data = R.spatial_image(B, 1, Hi, Wi, seed=1)
    _, sout = run_spatial(data, seg, prm, (Ho, Wo), d)
    want, und = R.labels64(seg, prm, (Ho, Wo))
    got = down(sout)
    assert und.mean() <= 0.01, und.mean()
    wrong = (got != want) & ~und
    print(f"labels {geo} {labels}: {int((got != want).sum())} differ, {int(und.sum())} of {und.size} undecided")
    assert not wrong.any(), f"{int(wrong.sum())} decided pixels differ, first {np.argwhere(wrong)[:5].tolist()}"
    assert set(np.unique(got).tolist()) <= set(float(v) for v in labels)


# ---------------------------------------------------------------------------------------------------- 7. the order inside apply()
REF_ORDER = ("blur", "mult", "contrast", "lowres", "gamma_inv", "gamma")      # after the spatial pass and the noise (off here)


def kernel_chain(data, draw, patch, order, d):
    """the kernels of one GPUAugment2D.apply() called one by one through the C ABI in `order`, each stage as apply() drives it (the
    retain_stats rescale of a gamma stage: statistics before and after, x a + b with a = std / (std' + 1e-8)).  The same kernels on the
    same inputs in the same order give the same bits: apply() must equal this chain for the reference's order and for no other"""
    B, Cc, Hi, Wi = data.shape
    H, W = patch
    P_, n = B * Cc, H * W
    out = run_spatial(data, None, draw["spatial"], patch, d)[0].contiguous()
    tmp, stats = torch.empty_like(out), torch.empty((P_, 4), dtype=f32, device=d)
    one, zero = up(np.ones(P_), d), up(np.zeros(P_), d)
    for stage in order:
        if stage == "blur":
            sg = up(draw["blur_sigma"], d)
            ok("du_aug_blur", ptr(out), ptr(tmp), ptr(sg), P_, H, W, 0)
            ok("du_aug_blur", ptr(tmp), ptr(out), ptr(sg), P_, H, W, 1)
        elif stage == "mult":
            m = up(draw["mult"], d)
            ok("du_aug_noise_mult", ptr(out), ptr(zero), ptr(m), P_, n, 0)
        elif stage == "contrast":
            f = up(draw["contrast"], d)
            ok("du_aug_plane_stats", ptr(out), ptr(stats), P_, n)
            ok("du_aug_contrast", ptr(out), ptr(f), ptr(stats), P_, n)
        elif stage == "lowres":
            z = up(draw["zoom"], d)
            ok("du_aug_lowres", ptr(out), ptr(tmp), ptr(z), P_, H, W)
            out, tmp = tmp, out
        else:
            g = draw[stage]
            on = (g > 0).astype(np.float32)
            t_g, t_inv, onv = up(g, d), up(on * float(stage == "gamma_inv"), d), up(on, d).view(-1)
            ok("du_aug_plane_stats", ptr(out), ptr(stats), P_, n)
            before = stats.clone()
            ok("du_aug_gamma", ptr(out), ptr(t_g), ptr(t_inv), ptr(stats), P_, n)
            ok("du_aug_plane_stats", ptr(out), ptr(stats), P_, n)
            sgn = 1.0 - 2.0 * t_inv.view(-1)
            a = before[:, 1] / (stats[:, 1] + 1e-8)
            bb = before[:, 0] * sgn - stats[:, 0] * a
            a, bb = ((a * sgn) * onv + (1 - onv)).contiguous(), ((bb * sgn) * onv).contiguous()
            ok("du_aug_affine", ptr(out), ptr(a), ptr(bb), P_, n)
        torch.cuda.synchronize()
    return out


def test_apply_runs_the_kernels_in_the_reference_order():
    """one draw with blur, multiplier, contrast, low resolution, inverted gamma and gamma all active, on plane (0, 0) all six and on the other
    planes some, noise off, a 56 x 60 input and a 40 x 48 patch: apply() is bit for bit the chain of the kernels in the order blur,
    multiplier, contrast, low resolution, inverted gamma, gamma (each kernel is held against fp64 above), and differs from the chain
    with any two neighbouring stages from the multiplier on exchanged (blur and multiplier commute up to rounding and are not tried).
    This checks the order alone, to the bit, with apply()'s own glue restated; the values are held against fp64 by
    test_apply_against_the_oracle_chained_in_fp64"""
    from dinounet_amd.augment import GPUAugment2D
    d = dev()
    B, Cc, Hi, Wi, H, W = 2, 2, 56, 60, 40, 48
    data = R.spatial_image(B, Cc, Hi, Wi, seed=7)
    a = lambda *v: np.array(v, np.float32).reshape(B, Cc)
    draw = dict(spatial=np.stack([R.spatial_params(0.6, 1.3, 1, 0), R.spatial_params(0.0, 1.0, 0, 1)]), noise_sigma=a(0, 0, 0, 0),
                blur_sigma=a(0.7, 0, 0.9, 0.6), mult=a(1.2, 1.0, 0.8, 1.1), contrast=a(0.8, 1.2, 1.0, 1.1), zoom=a(0.6, 0, 0, 0.8),
                gamma_inv=a(0.8, 0, 1.4, 0), gamma=a(1.3, 0.7, 0, 0), seed=3)
    got, _ = GPUAugment2D((H, W), seed=0).apply(up(data, d), None, draw)
    assert torch.isfinite(got).all()
    assert torch.equal(got, kernel_chain(data, draw, (H, W), REF_ORDER, d))
    for i in (1, 2, 3, 4):
        order = list(REF_ORDER)
        order[i], order[i + 1] = order[i + 1], order[i]
        other = kernel_chain(data, draw, (H, W), order, d)
        assert not torch.equal(got[0, 0], other[0, 0]), order


def test_apply_against_the_oracle_chained_in_fp64():
    """one draw with blur, multiplier, contrast, low resolution, inverted gamma and gamma all active on plane 0 and three of them on plane
    1, noise off, 56 x 60 -> 40 x 48: apply() per element against the oracle's functions chained in fp64 in the reference's order
    (R.apply64).  Tolerance: the stage bounds, each carried through the later stages by the reference's own sensitivity; pixels whose
    normalised gamma argument is below 1e-3 are excluded, 1 % at the most.  The draw with the two gammas swapped must differ"""
    from dinounet_amd.augment import GPUAugment2D
    d = dev()
    H, W = R.APPLY_GEO[2:]
    data, draw, ref, tol, excl = R.apply_case()
    assert excl.mean() <= 0.01
    aug = GPUAugment2D((H, W), seed=0)
    got = down(aug.apply(up(data, d), None, draw)[0])
    gate(got, ref, np.where(excl, np.inf, tol), "apply()")
    swapped = down(aug.apply(up(data, d), None, R.apply_draw(swap_gammas=True))[0])
    differs = (np.abs(swapped - ref) > tol) & ~excl
    assert differs[0, 0].mean() > 0.5, differs.mean()
    gate(swapped, R.apply_case(True)[2], np.where(R.apply_case(True)[4], np.inf, R.apply_case(True)[3]), "apply(), gammas swapped")
