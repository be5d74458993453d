"""fp64 references, shape lists, launch predicates, bounds and fp32 emulations for the Keys augmentation kernels of csrc/augment.hip
(tests/test_gpu_augment_keys.py, kept honest by tests/test_cpu_augment_keys.py).  Plain numpy / scipy on the CPU, no library load.

Every comparison is per element against fp64.  Each bound is a formula over the inputs whose constant is counted from the kernel's
operations (U = 2^-24, one fp32 rounding); the two terms that cannot be counted from outside, the device's pow and exp, are measured
against fp64 and carried with a factor 4 (E_POW, E_EXP below).  The emulations restate each kernel in fp32 numpy, in the kernel's order
of operations; their mutants exist so that the CPU module can show that each gate sees its bug.

The whole GPUAugment2D.apply() is compared with the oracle's functions chained in fp64 (apply64): the stage bounds are carried through
the later stages by the reference's own sensitivity, the error of the statistics kernel that feeds contrast and retain_stats included."""
import numpy as np
from scipy import ndimage, special

from oracle import augment_oracle as AO

U = 2.0 ** -24
f32, f64 = np.float32, np.float64


def cdiv(a, b):
    return -(-a // b)


def within(out, ref64, bound, what=""):
    """(ok, message) of the per-element gate |out - ref| <= bound, and the worst share of the bound that is used"""
    out, ref64 = np.asarray(out, f64), np.asarray(ref64, f64)
    bound = np.broadcast_to(np.asarray(bound, f64), ref64.shape)
    if out.shape != ref64.shape:
        return False, f"{what}: shape {out.shape}, want {ref64.shape}", np.inf
    if not np.isfinite(out).all():
        return False, f"{what}: non-finite values", np.inf
    err = np.abs(out - ref64)
    bad = err > bound
    share = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    if bad.any():
        i = np.unravel_index(int(np.argmax(err - bound)), err.shape)
        return False, (f"{what}: {int(bad.sum())} of {bad.size} elements outside the bound; worst at {tuple(int(v) for v in i)}: got {out[i]!r}, "
                       f"want {ref64[i]!r}, |diff| {err[i]:.3e}, bound {bound[i]:.3e}"), share
    return True, f"{what}: worst share of the bound {share:.3f}", share


# ---------------------------------------------------------------------------------------------------- launch arithmetic of augment.hip
def stats_passes(n):
    """aug_plane_stats_kernel, 1024 threads, thread t loads the float4 at 4 t + 4096 k < n: (most passes of a thread, fewest, threads
    that load anything)"""
    return cdiv(n, 4096), cdiv(max(n - 4092, 0), 4096), min(n // 4, 1024)


def stats_form(n):
    most, least, active = stats_passes(n)
    if active < 1024:
        return "idle"
    if most == least:
        return "one-pass" if most == 1 else "full"
    return "ragged" if most == 2 else "many"


def stats_depth(n):
    """additions on the longest path of one block sum: four per pass of a thread, six levels in the wave, sixteen wave totals in sequence"""
    return 4 * cdiv(n, 4096) + 6 + 16


def plane_grid(n):
    """workgroups per plane of noise, contrast, gamma, affine, blur and lowres (256 threads each)"""
    return min(cdiv(n, 256), 1024)


def plane_sweeps(n):
    return cdiv(n, plane_grid(n) * 256)


def spatial_grid(total):
    return min(cdiv(total, 256), 16384)


def spatial_sweeps(total):
    return cdiv(total, spatial_grid(total) * 256)


# ---------------------------------------------------------------------------------------------------- shape lists
STATS_N = {4: "idle", 1320: "idle", 4092: "idle", 4096: "one-pass", 4100: "ragged", 262148: "many"}
OFFSETS = ((0.0, 1.0), (3.0, 0.05), (30.0, 0.05), (-30.0, 0.05))
POINT_N = {4: 1, 1320: 1, 262144 + 256: 2}                     # plane size -> sweeps of the grid-stride loop
BLUR_SHAPES = ((40, 33), (3, 40), (40, 3), (64, 64))
BLUR_SIGMAS = (0.1, 0.374, 0.375, 0.625, 1.0)
BLUR_RADII = (0, 1, 2, 3, 4)                                   # int(4 sigma + 0.5) of the sigmas above
LOWRES_SHAPES = ((40, 33), (64, 64), (7, 5))
LOWRES_ZOOMS = (0.5, 0.77, 0.5125, 0.01)
LOWRES_COPIES = (0.0, 1.0, 1.3, 0.995)                          # 0.995: inside (0, 1) but rint(size * z) is the full size on every shape
NOISE_HW, NOISE_B, NOISE_C = (256, 256), 2, 2
SPATIAL_GEOS = {"crop": (80, 72, 48, 40), "pad": (30, 50, 48, 40), "half-pixel": (49, 45, 48, 40)}
LABEL_SETS = ((0, 1, 2, 3), (0, 2, 7))
CLAMP_CASE = (17, 1, 512, 512)                                 # B, C, H, W: one sweep of 16384 workgroups is 16 of the 17 samples


# ---------------------------------------------------------------------------------------------------- 1. plane statistics
def two_value_planes(P, n, seed):
    """integer planes with the mean m in [-3, 3] and the std s in {1, 2, 3, 4} exactly: m + s on a random half of the elements, m - s on the
    other.  Sums of x, of x - x[0], of x - m and of their squares (each term at most 49) are integers below 2^24 for n <= 262148: exact in
    fp32 in any order, so mean, std, min and max come back bit for bit (mean n is the integer sum)"""
    assert n % 2 == 0 and 49 * n < 2 ** 24
    rs = np.random.RandomState(seed)
    m, s = rs.randint(-3, 4, (P, 1)).astype(f32), rs.randint(1, 5, (P, 1)).astype(f32)
    half = np.argsort(rs.rand(P, n), 1) < n // 2
    x = m + np.where(half, s, -s).astype(f32)
    return x.astype(f32), np.concatenate([m, s, m - s, m + s], 1).astype(f64)


def offset_planes(n, seed):
    """one plane m + s z per entry of OFFSETS (z standard normal), and a constant plane 33"""
    rs = np.random.RandomState(seed)
    rows = [(f32(m) + f32(s) * rs.standard_normal(n).astype(f32)).astype(f32) for m, s in OFFSETS]
    return np.stack(rows + [np.full(n, 33.0, f32)])


def stats64(x):
    x = np.asarray(x, f64)
    return np.stack([x.mean(1), x.std(1), x.min(1), x.max(1)], 1)


def stats_bounds(x):
    """(|d mean|, |d std|) per plane for a two-pass (or shifted) fp32 algorithm, D = stats_depth(n).
    mean = m1 + c, c = sum(fl(x - m1)) / n: the true mean is m1 + E[x - m1] whatever m1 is, so the error is that of c -- one rounding per
    difference, D per sum, one for the division: (D + 2) U E|x - m1| -- plus the final add, U |mean|.  E|x - m1| is E|x - mean| up to m1's
    own error, which is of second order: one more U covers it.  |d mean| <= (D + 3) U E|x - mean| + U |mean|.
    var = E[d^2] - c^2, d = fl(x - m1): two roundings in d^2 from d, one from the square, D from the sum, one from the division, one
    from the subtraction (c^2 is of second order): (D + 5) U var; the square root halves it and adds one: |d std| <= (D / 2 + 4) U std.
    A constant plane has both deviations 0: std must come back as 0 and the mean to one rounding.
    The one-pass formula E[x^2] - mean^2 would need (D + 4) U (E[x^2] + mean^2) / (2 std^2) U std instead: (mean / std)^2 times as much."""
    x = np.asarray(x, f64)
    D = stats_depth(x.shape[1])
    st = stats64(x)
    mad = np.abs(x - st[:, :1]).mean(1)
    return (D + 3) * U * mad + U * np.abs(st[:, 0]), (D / 2 + 4) * U * st[:, 1]


def _block_sum(v, m, term):
    """one block sum as the kernel forms it, in fp32: v (passes, 1024, 4), m (passes, 1024) which float4s exist; a thread adds the four
    terms of a float4 left to right and the result to its running sum; xor butterfly in the wave; the 16 wave totals in sequence"""
    acc = np.zeros(1024, f32)
    for k in range(v.shape[0]):
        t = term(v[k])
        acc = np.where(m[k], acc + (((t[:, 0] + t[:, 1]) + t[:, 2]) + t[:, 3]), acc)
    w = acc.reshape(16, 64)
    for o in (1, 2, 4, 8, 16, 32):
        w = w + w[:, np.arange(64) ^ o]
    tot = f32(0)
    for k in range(16):
        tot = f32(tot + w[k, 0])
    return tot


def emu_stats(x, one_pass=False, drop_ragged=False):
    """aug_plane_stats_kernel on one plane x (n,) in fp32 -> (mean, std, min, max).  Mutants: the one-pass variance E[x^2] - mean^2 (the
    kernel before the two-pass rewrite); a loop that runs only the full passes (n // 4096 of them once n >= 4096)"""
    x = np.asarray(x, f32)
    n = x.size
    passes = cdiv(n, 4096)
    if drop_ragged and n >= 4096:
        passes = n // 4096
    keep = min(n, passes * 4096)
    xp = np.zeros(passes * 4096, f32)
    xp[:keep] = x[:keep]
    m = (np.arange(passes * 4096) < keep).reshape(passes, 1024, 4)[:, :, 0]
    v = xp.reshape(passes, 1024, 4)
    nf = f32(n)
    mn, mx = x[:keep].min(), x[:keep].max()
    if one_pass:
        a, b = _block_sum(v, m, lambda t: t), _block_sum(v, m, lambda t: t * t)
        mean = f32(a / nf)
        var = f32(f32(b / nf) - f32(mean * mean))
        return np.array([mean, np.sqrt(max(var, f32(0))), mn, mx], f32)
    K = x[0]
    m1 = f32(K + f32(_block_sum(v, m, lambda t: t - K) / nf))
    c = f32(_block_sum(v, m, lambda t: t - m1) / nf)
    b = _block_sum(v, m, lambda t: (t - m1) * (t - m1))
    var = f32(f32(b / nf) - f32(c * c))
    return np.array([f32(m1 + c), np.sqrt(max(var, f32(0))), mn, mx], f32)


# ---------------------------------------------------------------------------------------------------- 2. pointwise kernels
# pow and exp of the device cannot be counted from outside.  The HIP documentation that lists their ULP figures is not part of the ROCm
# installation this was written against, so both were measured on the MI355X against fp64 (2026-10-21) and carry a factor 4, since the
# error depends on the argument and the sample is finite.
# Both figures are printed by tools/measure_aug_intrinsics.py.
# E_POW_MEASURED: worst |pow(a, g) / a^g - 1| of du_aug_gamma with min 0 and max 1 over 2^20 arguments in (0, 1], uniform and log-uniform
# down to 1e-6, for each g in {0.7, 0.85, 1.0, 1.2, 1.5}.  With these statistics the range is 1 and the products and sums around the pow are
# exact; range + 1e-7 rounds to 1 + 2^-23 and the quotient by it rounds once: a is taken as that fp32 quotient (numpy's, correctly
# rounded), so a division on the device that rounded differently would be part of the figure.
E_POW_MEASURED = 1.3783e-7
E_POW = 4 * E_POW_MEASURED
# E_EXP_MEASURED: worst |w / exp(a) - 1| / (1 + |a|), a = -k^2 / (2 sigma^2), of the blur weights read back as the response to a unit pulse
# (out[c + k] / out[c]; the two divisions by the weight sum are part of the figure) for the sigmas of BLUR_SIGMAS and 64 more in [0.5, 1].
# The form (1 + |a|) is that of __expf = exp2(a log2 e): the rounded product errs by U |a| log2 e in the exponent.
E_EXP_MEASURED = 1.1567e-7
E_EXP = 4 * E_EXP_MEASURED


def point_planes(n, seed, P=8):
    """P planes of n elements: smooth-free random data at different offsets and spreads; the last one is constant"""
    rs = np.random.RandomState(seed)
    x = (rs.standard_normal((P, n)) * rs.uniform(0.2, 2.0, (P, 1)) + rs.uniform(-3, 3, (P, 1))).astype(f32)
    x[-1] = f32(1.75)
    return x


def stats_in(x):
    """the statistics a kernel is handed: fp64, rounded to fp32"""
    return stats64(x).astype(f32)


def mult64(x, m):
    """x m; one rounding"""
    ref = np.asarray(x, f64) * np.asarray(m, f64)[:, None]
    return ref, U * np.abs(ref)


def affine64(x, a, b):
    """x a + b: the product and the sum round (or neither, fused)"""
    xa = np.asarray(x, f64) * np.asarray(a, f64)[:, None]
    ref = xa + np.asarray(b, f64)[:, None]
    return ref, U * (np.abs(xa) + np.abs(ref))


def contrast64(x, f, st, clip=True):
    """clip((x - mean) f + mean, min, max) with the fp32 statistics st; planes with f == 1 untouched.  Bound: the difference rounds
    (U |x - mean|, scaled by |f|), the product rounds, the sum rounds: U (2 |f (x - mean)| + |y|); the clip is 1-Lipschitz"""
    x, f, st = np.asarray(x, f64), np.asarray(f, f64)[:, None], np.asarray(st, f64)
    t = (x - st[:, :1]) * f
    y = t + st[:, :1]
    out = np.clip(y, st[:, 2:3], st[:, 3:4]) if clip else y
    on = f != 1
    return np.where(on, out, x), np.where(on, U * (2 * np.abs(t) + np.abs(y)), 0.0)


def gamma64(x, g, inv, st):
    """((v - min) / (range + 1e-7))^g range + min on v = x or -x (statistics of v: min' = -max, max' = -min; the result is NOT negated
    back, du_aug_affine does that); g <= 0 untouched.  Bound on p = a^g range: the argument a carries five roundings (the difference,
    the range, the add of 1e-7, the quotient at up to 2 U), which pow turns into 5 g; pow itself E_POW; the product with the range and the
    range's own rounding 2, one to spare; the final add U |ref|.  |d| <= |p| (5 g U + E_POW + 3 U) + U |ref|.
    A constant plane has range 0: 0^g 0 + min = the constant, exactly."""
    x, g, st = np.asarray(x, f64), np.asarray(g, f64)[:, None], np.asarray(st, f64)
    inv = np.asarray(inv)[:, None] != 0
    v = np.where(inv, -x, x)
    lo, hi = np.where(inv, -st[:, 3:4], st[:, 2:3]), np.where(inv, -st[:, 2:3], st[:, 3:4])
    rng = hi - lo
    a = np.maximum((v - lo) / (rng + f64(f32(1e-7))), 0.0)
    p = np.power(a, np.where(g > 0, g, 1.0)) * rng
    ref = p + lo
    on = g > 0
    return np.where(on, ref, x), np.where(on, np.abs(p) * (5 * g * U + E_POW + 3 * U) + U * np.abs(ref), 0.0), a


def one_sweep(out, x):
    """mutant of any grid-stride kernel: the loop stops after one sweep, elements past plane_grid(n) 256 keep what they held"""
    out = np.array(out)
    done = plane_grid(x.shape[1]) * 256
    out[:, done:] = x[:, done:]
    return out


def emu_mult(x, m):
    return (np.asarray(x, f32) * np.asarray(m, f32)[:, None]).astype(f32)


def emu_affine(x, a, b):
    return (np.asarray(x, f32) * np.asarray(a, f32)[:, None] + np.asarray(b, f32)[:, None]).astype(f32)


def emu_contrast(x, f, st, clip=True):
    x, f, st = np.asarray(x, f32), np.asarray(f, f32)[:, None], np.asarray(st, f32)
    y = (x - st[:, :1]) * f + st[:, :1]
    if clip:
        y = np.minimum(np.maximum(y, st[:, 2:3]), st[:, 3:4])
    return np.where(f != 1, y, x).astype(f32)


def emu_gamma(x, g, inv, st):
    x, g, st = np.asarray(x, f32), np.asarray(g, f32)[:, None], np.asarray(st, f32)
    inv = np.asarray(inv)[:, None] != 0
    v = np.where(inv, -x, x)
    lo, hi = np.where(inv, -st[:, 3:4], st[:, 2:3]), np.where(inv, -st[:, 2:3], st[:, 3:4])
    rng = (hi - lo).astype(f32)
    a = np.maximum((v - lo) / (rng + f32(1e-7)), f32(0)).astype(f32)
    y = np.power(a, np.where(g > 0, g, f32(1)).astype(f32)).astype(f32) * rng + lo
    return np.where(g > 0, y, x).astype(f32)


# ---------------------------------------------------------------------------------------------------- 3. blur
def reflect_idx(i, n, single=False):
    """scipy's "reflect" (d c b a | a b c d | d c b a) at any distance; single = True is the mutant that reflects once (an `if` where the
    kernel has a `while`): at a radius above the axis length the index stays outside 0 .. n - 1"""
    i = np.asarray(i)
    if single:
        return np.where(i < 0, -i - 1, np.where(i >= n, 2 * n - 1 - i, i))
    i = np.mod(i, 2 * n)
    return np.where(i >= n, 2 * n - 1 - i, i)


def blur_radius(sg):
    """int(4 sigma + 0.5) in fp32, 0 for sigma <= 0"""
    sg = f32(sg)
    return int(f32(4.0) * sg + f32(0.5)) if sg > 0 else 0


def blur_axis(x, sigma, axis, dt=f64, r_shift=0, single=False):
    """one pass of du_aug_blur along axis 0 (y) / 1 (x) of x (P, H, W): weights exp(-k^2 / (2 sigma^2)), |k| <= r, summed from -r upwards and
    divided by the weight sum; r = 0 copies.  dt = float64 is the reference (sigma is the fp32 value), float32 the emulation.  Mutants: the
    radius off by r_shift; a single reflection"""
    x = np.asarray(x, dt)
    out = x.copy()
    n = x.shape[1 + axis]
    for p in range(x.shape[0]):
        r = blur_radius(sigma[p])
        if r == 0:
            continue
        r = max(r + r_shift, 0)
        sg = dt(f32(sigma[p]))
        acc, wsum = np.zeros(x.shape[1:], dt), dt(0)
        for k in range(-r, r + 1):
            wk = np.exp(dt(-0.5) * dt(k * k) / (sg * sg)).astype(dt)
            idx = reflect_idx(np.arange(n) + k, n, single)
            if single:                                                   # an index outside the axis reads whatever lies there in the plane
                H, W = x.shape[1:]
                flat = idx[:, None] * W + np.arange(W)[None, :] if axis == 0 else np.arange(H)[:, None] * W + idx[None, :]
                tap = np.take(x[p].reshape(-1), flat, mode="wrap")
            else:
                tap = np.take(x[p], idx, axis)
            acc = (acc + wk * tap).astype(dt)
            wsum = dt(wsum + wk)
        out[p] = acc / wsum
    return out


def blur_bound(x, sigma, axis):
    """(2 r + 2) U sum w |x| / sum w for the 2 r + 1 products, the 2 r additions and the division, plus the weights' own error: a weight
    w_k (1 + e_k) changes the normalised weight by at most (|e_k| + max |e|), |e_k| <= E_EXP (1 + k^2 / (2 sigma^2)): 2 E_EXP (1 + r^2 /
    (2 sigma^2)) sum w |x| / sum w.  (The fp32 quotient -k^2 / 2 / fl(sigma^2) that feeds the exponential is part of the measured figure.)
    Planes with r = 0 are copies: bound 0"""
    g = blur_axis(np.abs(np.asarray(x, f64)), sigma, axis)
    k = np.zeros(len(sigma))
    for p in range(len(sigma)):
        r = blur_radius(sigma[p])
        if r:
            k[p] = (2 * r + 2) * U + 2 * E_EXP * (1 + r * r / (2 * f64(f32(sigma[p])) ** 2))
    return k[:, None, None] * g


def blur2_64(x, sigma):
    """both passes as GPUAugment2D runs them (axis 0, then axis 1) and the bound of the result: the second pass's own bound on the first's
    reference, plus the first pass's bound blurred by the second (non-negative normalised weights)"""
    y1 = blur_axis(x, sigma, 0)
    return blur_axis(y1, sigma, 1), blur_bound(y1, sigma, 1) + blur_axis(blur_bound(x, sigma, 0), sigma, 1)


# ---------------------------------------------------------------------------------------------------- Keys sampling (lowres, spatial)
def keys_factored(t):
    """the Keys kernel (a = -0.5) as augment.hip evaluates it, in t's own precision: (1 - t) (1 + t - 1.5 t^2) on [0, 1] and
    -0.5 (t - 1) (2 - t)^2 on (1, 2).  The factors that vanish at t = 1 and t = 2 are exact differences, so a weight errs relative to itself"""
    t = np.abs(t)
    dt = t.dtype.type
    inner = (dt(1) - t) * ((dt(1) + t) - dt(1.5) * t * t)
    outer = dt(-0.5) * (t - dt(1)) * (dt(2) - t) * (dt(2) - t)
    return np.where(t <= 1, inner, np.where(t < 2, outer, dt(0))).astype(dt)


def keys_horner(t):
    """the same polynomials in Horner form (what the kernel evaluated before): near t = 2 and t = 1 the value is the small difference of
    terms of size 2 to 4, so a weight errs by about 2^-22 ABSOLUTE: more than K_TAPS U |w| |v| allows where a far tap is the only one inside
    the image.  Kept as a mutant"""
    t = np.abs(t)
    dt = t.dtype.type
    inner = (dt(1.5) * t - dt(2.5)) * t * t + dt(1)
    outer = ((dt(-0.5) * t + dt(2.5)) * t - dt(4)) * t + dt(2)
    return np.where(t <= 1, inner, np.where(t < 2, outer, dt(0))).astype(dt)


def keys_sample(img, y, x, edge, dt=f64, keys=keys_factored):
    """sum over the 4 x 4 taps around (y, x) of keys(y - yy) keys(x - xx) img[yy, xx], taps outside the image clamped to the edge (edge =
    True) or 0; -> (value, sum |w| |v|).  dt = float32 adds the taps in the kernel's order (rows, then columns, one running sum)"""
    img = np.asarray(img, dt)
    H, W = img.shape
    y, x = np.broadcast_arrays(np.asarray(y, dt), np.asarray(x, dt))
    y0, x0 = np.floor(y).astype(np.int64), np.floor(x).astype(np.int64)
    acc, mag = np.zeros(y.shape, dt), np.zeros(y.shape, f64)
    for j in range(-1, 3):
        yy = y0 + j
        wy = keys((y - yy.astype(dt)).astype(dt))
        for i in range(-1, 3):
            xx = x0 + i
            v = img[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
            if not edge:
                v = np.where((yy >= 0) & (yy < H) & (xx >= 0) & (xx < W), v, dt(0))
            w = (wy * keys((x - xx.astype(dt)).astype(dt))).astype(dt)
            acc = (acc + w * v).astype(dt)
            mag += np.abs(w.astype(f64) * v.astype(f64))
    return acc, mag


def keys_gradient(img, y, x, edge, h=2.0 ** -8):
    """(|d/dy|, |d/dx|) of the fp64 resampler by central differences (the Keys interpolant is C^1, also across the clamped / zero border)"""
    gy = (keys_sample(img, y + h, x, edge)[0] - keys_sample(img, y - h, x, edge)[0]) / (2 * h)
    gx = (keys_sample(img, y, x + h, edge)[0] - keys_sample(img, y, x - h, edge)[0]) / (2 * h)
    return np.abs(gy), np.abs(gx)


K_TAPS = 18      # 16 taps: 15 additions, the two products w_y w_x v, one to spare for the polynomial's own roundings


# ---------------------------------------------------------------------------------------------------- 4. low resolution
def lowres_grid(z, H, W):
    """(Hl, Wl) = max(rint(size * zoom), 1) in fp32, ties to even, as du_aug_lowres; None where the plane is copied"""
    z = f32(z)
    if not (z > 0 and z < 1):
        return None
    return max(int(np.rint(f32(H) * z)), 1), max(int(np.rint(f32(W) * z)), 1)


def lowres_src(nl, n):
    """source pixel of each low-grid sample: min(int((i + 0.5) n / nl), n - 1), the quotient in fp32"""
    q = (np.arange(nl).astype(f32) + f32(0.5)) * f32(n) / f32(nl)
    return np.minimum(q.astype(np.int64), n - 1)


def lowres_plane(x, z, dt=f64, want_bound=False):
    """du_aug_lowres on one plane: nearest-neighbour down to the low grid, Keys cubic back up at (y + 0.5) Hl / H - 0.5 with replicated
    edges.  Integer decisions in fp32 as the kernel takes them; coordinates, weights and sums in dt.
    Bound: K_TAPS U sum |w| |v| for the tap sum, plus the coordinate: ((y + 0.5) Hl) / H - 0.5 is an exact product, a rounded quotient and
    a rounded difference, |d fy| <= 2 U (Hl + 1), times the reference's own gradient along that axis"""
    H, W = x.shape
    g = lowres_grid(z, H, W)
    if g is None:
        return (np.asarray(x, dt), np.zeros(x.shape)) if want_bound else np.asarray(x, dt)
    Hl, Wl = g
    low = np.asarray(x, dt)[np.ix_(lowres_src(Hl, H), lowres_src(Wl, W))]
    fy = ((np.arange(H).astype(dt) + dt(0.5)) * dt(Hl) / dt(H) - dt(0.5)).astype(dt)[:, None]
    fx = ((np.arange(W).astype(dt) + dt(0.5)) * dt(Wl) / dt(W) - dt(0.5)).astype(dt)[None, :]
    out, mag = keys_sample(low, fy, fx, True, dt)
    if not want_bound:
        return out
    gy, gx = keys_gradient(low, fy, fx, True)
    return out, K_TAPS * U * mag + 2 * U * ((Hl + 1) * gy + (Wl + 1) * gx)


def lowres64(x, zoom):
    """x (P, H, W), zoom (P) -> (reference, bound)"""
    pairs = [lowres_plane(x[p], zoom[p], f64, True) for p in range(x.shape[0])]
    return np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs])


def emu_lowres(x, zoom):
    return np.stack([lowres_plane(x[p], zoom[p], f32) for p in range(x.shape[0])]).astype(f32)


# ---------------------------------------------------------------------------------------------------- 5. noise
def _hash32(x):
    x = x.astype(np.uint64)
    m = np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & m
    x ^= x >> np.uint64(16)
    return x


def emu_normal(seed, plane, n, same_plane=False, same_seed=False):
    """normal_at(seed, plane, 0 .. n - 1): the counter hash restated, Box-Muller in fp64.  Mutants: the plane left out of the counter; the
    lowest bit of the seed left out (seeds s and s + 1 draw the same field for even s)"""
    m = np.uint64(0xFFFFFFFF)
    if same_plane:
        plane = 0
    if same_seed:
        seed = seed & ~1
    inner = _hash32(np.array([(plane + 0x9e3779b9 * seed) & 0xFFFFFFFF], np.uint64))[0]
    idx = np.arange(n, dtype=np.uint64)
    h1 = _hash32(((idx * np.uint64(2654435761)) & m) ^ inner)
    h2 = _hash32(h1 ^ np.uint64(0x85ebca6b))
    u1 = ((h1 >> np.uint64(8)).astype(f64) + 1.0) / 16777216.0
    u2 = (h2 >> np.uint64(8)).astype(f64) / 16777216.0
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(f64(f32(6.28318530718)) * u2)


Z_MAX = 5.8      # sqrt(-2 ln 2^-24) = 5.768: the largest radius Box-Muller can draw from a 24-bit uniform


def _corr(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).mean() / np.sqrt((a * a).mean() * (b * b).mean()))


def noise_violations(z):
    """z (2, B, C, N): the standard-normal fields of seeds s and s + 1 on the B x C planes.  -> list of violated gates (empty = pass).
    Independent N(0, 1) fields have sample correlations of standard deviation 1 / sqrt(N) and bin counts of binomial standard deviation
    sqrt(N p (1 - p)); every gate is five of those"""
    z = np.asarray(z, f64)
    _, B, Cc, N = z.shape
    lim = 5.0 / np.sqrt(N)
    bad = []
    if not np.isfinite(z).all():
        return ["non-finite values"]
    if np.abs(z).max() > Z_MAX:
        bad.append(f"max |z| {np.abs(z).max():.3f} > {Z_MAX}")
    pairs = [(f"channels of sample {b}", z[0, b, 0], z[0, b, 1]) for b in range(B)]
    pairs += [(f"samples 0 and {b}, channel {c}", z[0, 0, c], z[0, b, c]) for b in range(1, B) for c in range(Cc)]
    pairs += [(f"seeds s and s + 1, plane ({b}, {c})", z[0, b, c], z[1, b, c]) for b in range(B) for c in range(Cc)]
    for b in range(B):
        for c in range(Cc):
            pairs += [(f"lag {k}, plane ({b}, {c})", z[0, b, c, :-k], z[0, b, c, k:]) for k in (1, 2, 3, 4)]
    for what, a, b_ in pairs:
        r = _corr(a, b_)
        if abs(r) >= lim:
            bad.append(f"correlation {r:.4f} ({what}) >= 5 / sqrt(N) = {lim:.4f}")
    edges = special.ndtri(np.arange(1, 10) / 10.0)
    for b in range(B):
        for c in range(Cc):
            v = z[0, b, c]
            counts = np.bincount(np.searchsorted(edges, v), minlength=10)
            sd = np.sqrt(N * 0.1 * 0.9)
            for k in range(10):
                if abs(counts[k] - 0.1 * N) > 5 * sd:
                    bad.append(f"decile {k} of plane ({b}, {c}): {counts[k]} of {N}, expected {0.1 * N:.0f} +- {sd:.0f}")
            pt = 2 * special.ndtr(-3.0)
            nt = int((np.abs(v) > 3).sum())
            if abs(nt - pt * N) > 5 * np.sqrt(N * pt * (1 - pt)):
                bad.append(f"tails |z| > 3 of plane ({b}, {c}): {nt} of {N}, expected {pt * N:.0f} +- {np.sqrt(N * pt * (1 - pt)):.0f}")
    return bad


# ---------------------------------------------------------------------------------------------------- 6. spatial
def spatial_params(angle, scale, flip_y=0, flip_x=0):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([c * scale, -s * scale, s * scale, c * scale, flip_y, flip_x], f32)


IDENT = np.array([1, 0, 0, 1, 0, 0], f32)


def spatial_image(B, Cc, Hi, Wi, seed):
    """smooth content, asymmetric on both axes (a ramp along each plus waves of different periods), with a little noise"""
    rs = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.arange(Hi, dtype=f64), np.arange(Wi, dtype=f64), indexing="ij")
    planes = [np.sin(yy * (0.11 + 0.03 * k)) * np.cos(xx * (0.07 + 0.02 * k)) + 0.01 * yy - 0.02 * xx + 0.3 for k in range(B * Cc)]
    return (np.stack(planes).reshape(B, Cc, Hi, Wi) + 0.05 * rs.standard_normal((B, Cc, Hi, Wi))).astype(f32)


def label_image(labels, Hi, Wi):
    """blocks of 9 x 11 pixels cycling through the label set; the regions touch every border"""
    yy, xx = np.meshgrid(np.arange(Hi), np.arange(Wi), indexing="ij")
    return np.asarray(labels, f32)[(yy // 9 + 2 * (xx // 11)) % len(labels)]


def coord_err(Hi, Wi):
    """fp32 coordinate m0 cy + m1 cx + centre: two rounded products, two rounded sums, each below U max(Hi, Wi) for the scales used"""
    return 4 * U * max(Hi, Wi)


def spatial64(data, prm, patch):
    """data (B, C, Hi, Wi) -> (reference (B, C, Ho, Wo), bound): K_TAPS U sum |w| |v| + coord_err (|d/dy| + |d/dx|) of the fp64 resampler"""
    B, Cc, Hi, Wi = data.shape
    ref, bound = np.zeros((B, Cc) + tuple(patch)), np.zeros((B, Cc) + tuple(patch))
    for b in range(B):
        y, x = AO._coords(prm[b], Hi, Wi, *patch)
        for c in range(Cc):
            ref[b, c], mag = keys_sample(data[b, c], y, x, False)
            gy, gx = keys_gradient(data[b, c], y, x, False)
            bound[b, c] = K_TAPS * U * mag + coord_err(Hi, Wi) * (gy + gx)
    return ref, bound


def labels64(seg, prm, patch):
    """seg (B, Hi, Wi) -> (labels, undecided): batchgenerators' order-1 rule in fp64 (per label in ascending order: bilinear interpolation of
    its one-hot map with cval -1, >= 0.5 overwrites; nothing claimed = 0).  undecided: some label's score lies within 2 coord_err of 0.5, or
    jumps within the coordinate error (the image's edge; this goes beyond a score near 0.5 and is needed because mode="constant" makes
    every score discontinuous there; not for integer matrices such as the identity, whose fp32 coordinates are exact)"""
    B, Hi, Wi = seg.shape
    out, und = np.zeros((B,) + tuple(patch)), np.zeros((B,) + tuple(patch), bool)
    for b in range(B):
        y, x = AO._coords(prm[b], Hi, Wi, *patch)
        for lab in np.sort(np.unique(seg[b])):
            m = ndimage.map_coordinates((seg[b] == lab).astype(f64), [y, x], order=1, mode="constant", cval=-1.0)
            out[b][m >= 0.5] = lab
            und[b] |= np.abs(m - 0.5) <= 2 * coord_err(Hi, Wi)
        # mode="constant" does not interpolate towards cval: every score jumps to -1 where a coordinate leaves [0, n - 1]; within the
        # coordinate error of that edge the fp32 coordinate may lie on the other side
        e = coord_err(Hi, Wi)
        if all(float(v).is_integer() for v in prm[b][:4]):               # an integer matrix: fp32 forms the same (half-)integers exactly
            continue
        und[b] |= (np.abs(y) <= e) | (np.abs(y - (Hi - 1)) <= e) | (np.abs(x) <= e) | (np.abs(x - (Wi - 1)) <= e)
    return out, und


def centre_crop(x, prm, patch):
    """the identity transform with even size differences: rows / columns (n_in - n_out) / 2 onwards (zeros where the patch is larger),
    flipped"""
    Hi, Wi = x.shape[-2:]
    Ho, Wo = patch
    assert (Hi - Ho) % 2 == 0 and (Wi - Wo) % 2 == 0
    out = np.zeros(x.shape[:-2] + (Ho, Wo), x.dtype)
    oy, ox = (Hi - Ho) // 2, (Wi - Wo) // 2
    y0, y1, x0, x1 = max(oy, 0), min(oy + Ho, Hi), max(ox, 0), min(ox + Wo, Wi)
    out[..., y0 - oy:y1 - oy, x0 - ox:x1 - ox] = x[..., y0:y1, x0:x1]
    if prm[4]:
        out = out[..., ::-1, :]
    if prm[5]:
        out = out[..., :, ::-1]
    return np.ascontiguousarray(out)


def emu_spatial(data, seg, prm, patch, mirror_swap=False, keys=keys_factored, edge_interp=False):
    """aug_spatial_kernel in fp32: image and labels.  Mutants: Ho and Wo swapped in the mirror; the Keys weights in Horner form; labels
    interpolated towards cval in the half-pixel strip outside the image (what the kernel did before: scipy returns cval there)"""
    B, Cc, Hi, Wi = data.shape
    Ho, Wo = patch
    out = np.zeros((B, Cc, Ho, Wo), f32)
    sout = None if seg is None else np.zeros((B, Ho, Wo), f32)
    yo, xo = np.meshgrid(np.arange(Ho), np.arange(Wo), indexing="ij")
    for b in range(B):
        q = np.asarray(prm[b], f32)
        ys = ((Wo if mirror_swap else Ho) - 1 - yo) if q[4] else yo
        xs = ((Ho if mirror_swap else Wo) - 1 - xo) if q[5] else xo
        cy, cx = ys.astype(f32) - f32(0.5) * f32(Ho - 1), xs.astype(f32) - f32(0.5) * f32(Wo - 1)
        y = (q[0] * cy + q[1] * cx + (f32(0.5) * f32(Hi) - f32(0.5))).astype(f32)
        x = (q[2] * cy + q[3] * cx + (f32(0.5) * f32(Wi) - f32(0.5))).astype(f32)
        for c in range(Cc):
            out[b, c] = keys_sample(data[b, c], y, x, False, f32, keys)[0]
        if seg is not None:
            y0, x0 = np.floor(y).astype(np.int64), np.floor(x).astype(np.int64)
            fy, fx = y - y0.astype(f32), x - x0.astype(f32)
            w = [(1 - fy) * (1 - fx), (1 - fy) * fx, fy * (1 - fx), fy * fx]
            lab = []
            for k in range(4):
                yy, xx = y0 + (k >> 1), x0 + (k & 1)
                ok = (yy >= 0) & (yy < Hi) & (xx >= 0) & (xx < Wi)
                lab.append(np.where(ok, seg[b][np.clip(yy, 0, Hi - 1), np.clip(xx, 0, Wi - 1)], f32(-1)))
            wout = sum(np.where(lab[j] < 0, w[j], f32(0)) for j in range(4)).astype(f32)
            best = np.zeros((Ho, Wo), f32)
            for k in range(4):
                s = -wout
                for j in range(4):
                    s = (s + np.where(lab[j] == lab[k], w[j], f32(0))).astype(f32)
                take = (lab[k] >= 0) & (s >= f32(0.5)) & (lab[k] > best)
                best = np.where(take, lab[k], best)
            inside = (y >= 0) & (y <= f32(Hi - 1)) & (x >= 0) & (x <= f32(Wi - 1))
            sout[b] = best if edge_interp else np.where(inside, best, f32(0))
    return out, sout


def spatial_one_sweep(out):
    """mutant: the loop of aug_spatial_kernel stops after one sweep of the clamped grid; the outputs behind it keep the buffer's 0"""
    B, Cc, Ho, Wo = out.shape
    flat = out.transpose(0, 2, 3, 1).reshape(B * Ho * Wo, Cc).copy()
    flat[spatial_grid(B * Ho * Wo) * 256:] = 0
    return flat.reshape(B, Ho, Wo, Cc).transpose(0, 3, 1, 2).copy()


# ---------------------------------------------------------------------------------------------------- 7. the whole apply()
# (angle, scale, flip y, flip x) of the spatial cases.  Scale 0.8 comes with the arbitrary angle only: at rotations 0 and pi / 2 its coordinates
# 0.8 (k + 0.5) + c hit the fraction 0.5 exactly, and 4 % of such a sample's labels sit on a tie of the order-1 rule (the cap is 1 %)
SAMPLES = [(0.0, 1.0, 0, 0), (0.0, 1.3, 0, 0), (np.pi / 2, 1.3, 0, 0), (0.6, 0.8, 0, 0), (0.6, 1.3, 0, 0), (0.6, 1.3, 1, 0), (0.6, 0.8, 0, 1),
           (np.pi / 2, 1.3, 1, 1)]
APPLY_GEO = (56, 60, 40, 48)
STAGES = ("blur", "mult", "contrast", "lowres", "gamma_inv", "gamma")      # the reference's order after the spatial pass (noise off)
GAMMA_ARG_MIN = 1e-3


def apply_draw(swap_gammas=False):
    """one draw for B = 1, C = 2: plane 0 has all six intensity transforms active, plane 1 blur, contrast and the plain gamma.  The patch
    stays inside the image (scale 0.8) and the contrast factors are below 1: a zero-padded corner or clipped pixels would be hundreds of
    tied minima, each of which moves the gamma's range, and all of them would sit at argument 0 and be excluded"""
    a = lambda *v: np.array(v, f32).reshape(1, 2)
    d = dict(spatial=np.stack([spatial_params(0.6, 0.8, 1, 0)]), noise_sigma=a(0, 0), blur_sigma=a(0.7, 0.9), mult=a(1.2, 1.0),
             contrast=a(0.8, 0.9), zoom=a(0.6, 0), gamma_inv=a(0.8, 0), gamma=a(1.3, 0.7), seed=3)
    if swap_gammas:
        d["gamma_inv"], d["gamma"] = d["gamma"], d["gamma_inv"]
    return d


def _keys_matrix(n, nl):
    """(n, nl): the Keys up-sampling of a line of nl samples to n, edge samples replicated (the weights of lowres_plane as a matrix)"""
    f = (np.arange(n) + 0.5) * nl / n - 0.5
    y0 = np.floor(f).astype(np.int64)
    m = np.zeros((n, nl))
    for j in range(-1, 3):
        np.add.at(m, (np.arange(n), np.clip(y0 + j, 0, nl - 1)), keys_factored(f - (y0 + j)))
    return m


def _st_blur(x, sg):
    r = blur_radius(sg)
    for ax in (1, 2):
        x = ndimage.gaussian_filter1d(x, float(f32(sg)), axis=ax, mode="reflect", radius=r)
    return x


def _st_contrast(x, f):
    mean = x.mean((1, 2), keepdims=True)
    return np.clip((x - mean) * f64(f) + mean, x.min((1, 2), keepdims=True), x.max((1, 2), keepdims=True))


def _st_lowres(x, z):
    H, W = x.shape[1:]
    Hl, Wl = lowres_grid(z, H, W)
    low = x[:, lowres_src(Hl, H)][:, :, lowres_src(Wl, W)]
    return np.einsum("yh,nhw,xw->nyx", _keys_matrix(H, Hl), low, _keys_matrix(W, Wl))


def _gamma_body(v, g):
    lo = v.min((1, 2), keepdims=True)
    rng = v.max((1, 2), keepdims=True) - lo
    a = np.maximum((v - lo) / (rng + f64(f32(1e-7))), 0.0)
    return np.power(a, f64(g)) * rng + lo, a, lo


def _retain(p, mb, sb):
    return (p - p.mean((1, 2), keepdims=True)) / (p.std((1, 2), keepdims=True) + 1e-8) * sb + mb


def _st_gamma(v, g):
    """augment_gamma with retain_stats on v (N, H, W) (the caller negates for the inverted transform)"""
    return _retain(_gamma_body(v, g)[0], v.mean((1, 2), keepdims=True), v.std((1, 2), keepdims=True))


def _carry(fn, r, t, h=2.0 ** -20):
    """|J| t: the tolerance t (H, W) on the input r of a stage, carried through it by the reference's own sensitivity -- the Jacobian of
    fn at r by forward differences, one input pixel at a time, absolute values, times t.  First order in t (t is of order 1e-6).  The linear
    stages need no differences: their |J| t is written down in apply64"""
    if not t.any():
        return np.zeros_like(t)
    H, W = r.shape
    E = np.eye(H * W).reshape(H * W, H, W) * h
    D = (fn(r[None] + E) - fn(r[None])) / h
    return np.tensordot(t.ravel(), np.abs(D), 1)


def apply64(data, draw, patch, order=STAGES):
    """GPUAugment2D.apply() in fp64: the Keys resampling, then the oracle's transforms in `order`, per plane.  -> (reference, tolerance,
    excluded).  Tolerance: after every stage t <- |J_stage| t + b_stage, b_stage the stage's own bound (the bounds above, evaluated on the
    reference's input of that stage) and |J_stage| by _carry; |J_k| ... |J_1| b is no smaller than |J_k ... J_1| b.  The statistics a
    stage reads come from du_aug_plane_stats on the device's own data: their dependence on the data is part of J, the kernel's own error
    (stats_bounds) part of b: contrast (1 - f) d mean; the retain_stats rescale x a + bb, a = std / (std' + 1e-8), bb = mean - mean' a:
    d a = a (d std / std + d std' / std' + 3 U), d bb = d mean + a d mean' + |mean'| d a + 3 U (|mean| + |mean' a|), and the
    affine kernel's U (|p a| + |out|).  Excluded: pixels whose normalised gamma argument is below GAMMA_ARG_MIN in either gamma stage
    (the slope of a^g is unbounded there for g < 1)"""
    ref, tol = spatial64(data, draw["spatial"], patch)
    ref, tol = ref.copy(), tol.copy()
    excl = np.zeros(ref.shape, bool)
    B, Cc = ref.shape[:2]
    for b in range(B):
        for c in range(Cc):
            r, t = ref[b, c], tol[b, c]
            for stage in order:
                if stage == "blur" and blur_radius(draw["blur_sigma"][b, c]) > 0:
                    sg = draw["blur_sigma"][b, c]
                    fn, own = (lambda x, sg=sg: _st_blur(x, sg)), blur2_64(r[None], [sg])[1][0]
                    carried = fn(t[None])[0]                             # non-negative weights: |J| t is the blur of t
                elif stage == "mult" and draw["mult"][b, c] != 1:
                    m = f64(draw["mult"][b, c])
                    fn, own = (lambda x, m=m: x * m), U * np.abs(r * m)
                    carried = abs(m) * t
                elif stage == "contrast" and draw["contrast"][b, c] != 1:
                    f = draw["contrast"][b, c]
                    st = stats64(r.reshape(1, -1))
                    fn = lambda x, f=f: _st_contrast(x, f)
                    own = contrast64(r.reshape(1, -1), [f], st)[1].reshape(r.shape) + abs(1 - f64(f)) * stats_bounds(r.reshape(1, -1))[0][0]
                    carried = _carry(fn, r, t)
                elif stage == "lowres" and lowres_grid(draw["zoom"][b, c], *r.shape) is not None:
                    z = draw["zoom"][b, c]
                    fn, own = (lambda x, z=z: _st_lowres(x, z)), lowres_plane(r, z, f64, True)[1]
                    Hl, Wl = lowres_grid(z, *r.shape)                    # separable: |J| = |Wy Sy| (x) |Wx Sx|, S the nearest-source selection
                    ay, ax = (np.abs(_keys_matrix(n_, l_)) @ np.eye(n_)[lowres_src(l_, n_)] for n_, l_ in ((r.shape[0], Hl), (r.shape[1], Wl)))
                    carried = ay @ t @ ax.T
                elif stage in ("gamma_inv", "gamma") and draw[stage][b, c] > 0:
                    g = f64(draw[stage][b, c])
                    sgn = -1.0 if stage == "gamma_inv" else 1.0
                    v = sgn * r
                    p, a, lo = _gamma_body(v[None], g)
                    p, a = p[0], a[0]
                    excl[b, c] |= a < GAMMA_ARG_MIN
                    mb, sb, ma, sa = v.mean(), v.std(), p.mean(), p.std()
                    body = np.abs(p - lo[0]) * (5 * g * U + E_POW + 3 * U) + U * np.abs(p)
                    (bmb,), (bsb,) = stats_bounds(v.reshape(1, -1))
                    (bma,), (bsa,) = stats_bounds(p.reshape(1, -1))
                    aa = sb / (sa + 1e-8)
                    da = aa * (bsb / sb + bsa / sa + 3 * U)
                    dbb = bmb + aa * bma + abs(ma) * da + 3 * U * (abs(mb) + abs(ma * aa))
                    out = _retain(p[None], mb, sb)[0]
                    own = _carry(lambda q: _retain(q, mb, sb), p, body) + np.abs(p) * da + dbb + U * (np.abs(p * aa) + np.abs(out))
                    fn = lambda x, g=g, sgn=sgn: sgn * _st_gamma(sgn * x, g)
                    carried = _carry(fn, r, t)
                else:
                    continue
                t = carried + own
                r = fn(r[None])[0]
            ref[b, c], tol[b, c] = r, t
    return ref, tol, excl


_APPLY_CASES = {}


def apply_case(swap_gammas=False):
    """(data, draw, reference, tolerance, excluded) of the apply() case, computed once per process"""
    if swap_gammas not in _APPLY_CASES:
        Hi, Wi, H, W = APPLY_GEO
        data, draw = spatial_image(1, 2, Hi, Wi, seed=7), apply_draw(swap_gammas)
        _APPLY_CASES[swap_gammas] = (data, draw) + apply64(data, draw, (H, W))
    return _APPLY_CASES[swap_gammas]


def emu_apply(data, draw, patch, order=STAGES, forget_sign=False, inverse_rescale=False):
    """GPUAugment2D.apply() in fp32 from the emulated kernels, the retain_stats glue as apply() computes it.  Mutants: another order of
    the stages; the inverted gamma's offset put back without its sign; the rescale std' / std instead of std / std'"""
    x = emu_spatial(data, None, draw["spatial"], patch)[0]
    B, Cc, H, W = x.shape
    x = x.reshape(B * Cc, H, W)
    flat = lambda k: np.asarray(draw[k], f32).reshape(-1)
    stats = lambda v: np.stack([emu_stats(p.reshape(-1)) for p in v])
    for stage in order:
        if stage == "blur":
            x = blur_axis(blur_axis(x, flat("blur_sigma"), 0, f32), flat("blur_sigma"), 1, f32)
        elif stage == "mult":
            x = emu_mult(x.reshape(B * Cc, -1), flat("mult")).reshape(x.shape)
        elif stage == "contrast":
            x = emu_contrast(x.reshape(B * Cc, -1), flat("contrast"), stats(x)).reshape(x.shape)
        elif stage == "lowres":
            x = emu_lowres(x, flat("zoom"))
        else:
            g = flat(stage)
            on = (g > 0).astype(f32)
            inv = on * f32(stage == "gamma_inv")
            before = stats(x)
            y = emu_gamma(x.reshape(B * Cc, -1), g, inv, before)
            after = stats(y)
            sgn = f32(1) - f32(2) * inv
            a = (after[:, 1] / (before[:, 1] + f32(1e-8)) if inverse_rescale else before[:, 1] / (after[:, 1] + f32(1e-8))).astype(f32)
            bb = (before[:, 0] * sgn - after[:, 0] * a).astype(f32)
            a, bb = (a * sgn * on + (1 - on)).astype(f32), (bb * (f32(1) if forget_sign else sgn) * on).astype(f32)
            x = emu_affine(y, a, bb).reshape(x.shape)
    return x.reshape(B, Cc, H, W)
