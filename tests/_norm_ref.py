"""fp64 references, draws, shape lists, regime predicates and bounds for the kernels of csrc/norm.hip (tests/test_gpu_norms.py, kept
honest by tests/test_cpu_norms.py).  Plain torch on the CPU, no library load.  NHWC tensors are held flat as (G, P, C): G groups
(samples of an InstanceNorm, 1 for BatchNorm) of P pixels; LayerNorm tensors as (rows, D).

Two instruments, as in tests/_exact.py.  Exact inputs: every reduction of norm.hip is an fp32 sum of per-element terms followed by strip
partials, an LDS / shuffle combine and a finalize kernel; integer or dyadic terms below 2^24 granules make it exact in any order and the
fp64 value must come back bit for bit.  Derived per-element bounds where a result passes through rsqrtf, a division by a count that is no
power of two or a rounding into bf16: each bound below is a formula over the inputs, its constant counted from the operations (never
fitted to a kernel).  The emulations and their mutants at the end exist so that the CPU module can show that each gate sees its bug."""
import torch
import torch.nn.functional as F

import _exact as X
from _small_ref import DTS, LEAKY, U, VEC, bf, f32, quant, within  # noqa: F401  (re-exported for the two test modules)

ACT_NONE, ACT_GELU, ACT_RELU, ACT_LEAKY = 0, 1, 2, 3                   # dinounet_amd._lib
ACTS = {"none": ACT_NONE, "relu": ACT_RELU, "leaky": ACT_LEAKY}      # what the call sites of ops.norm_act pass (no GELU)
EPS_LN, EPS_N = 1e-6, 1e-5
UF = X.U_F32


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------- regimes (the formulas of norm.hip)
def lanes(C, dt):
    """(cvb, np): channel vectors per pass and pixel lanes of a 256-thread workgroup (strip_reduce and the elementwise kernels)"""
    cvb = min(C // VEC[dt], 256)
    return cvb, 256 // cvb


def pick_strip(G, P, C, dt):
    """pixels per workgroup of the strip reductions (pick_strip with its default target of 512 workgroups)"""
    _, np_ = lanes(C, dt)
    target = min(65536 * 8 // C, 512)
    target = max(target, 256)
    per_group = max(target // G, 1)
    return min(max(cdiv(P, per_group), 4 * np_), P)


def strips(G, P, C, dt):
    return cdiv(P, pick_strip(G, P, C, dt))


def ws_elems(G, P, C, dt):
    """du_reduce_ws_elems"""
    return G * strips(G, P, C, dt) * C * 2


def reduce_path(C, dt):
    """lane_reduce: xor shuffles when cvb is a power of two below 64, LDS otherwise"""
    cvb, _ = lanes(C, dt)
    return "shuffle" if (cvb & (cvb - 1)) == 0 and cvb < 64 else "lds"


def passes(C, dt):
    return cdiv(C // VEC[dt], 256)


def idle_lanes(C, dt):
    cvb, np_ = lanes(C, dt)
    return 256 - cvb * np_


def sum_depth(G, P, C, dt):
    """an upper bound of the additions on the longest path of a two-stage reduction: a lane's own pixels, the combine over the pixel
    lanes (np in sequence through LDS; 6 + 4 on the shuffle path), a finalize lane's strips (LANES >= 8) and its LANES <= 64"""
    _, np_ = lanes(C, dt)
    return cdiv(pick_strip(G, P, C, dt), np_) + np_ + cdiv(strips(G, P, C, dt), 8) + 64 + 8


def norm_slots(G, P, C, dt, bwd=False):
    """pixel-lane slots per group of norm_act_fwd_kernel (cap 4096 / G) and norm_act_bwd_dx_kernel (cap 512 / G)"""
    _, np_ = lanes(C, dt)
    cap = max((512 if bwd else 4096) // G, 1)
    return max(min(cdiv(P, 4 * np_), cap), 1)


def elementwise_loops(G, P, C, dt, bwd=False):
    """(which of the unrolled pixel loops run in one launch, whether the slot cap binds): a thread walks n = ceil or floor of
    P / (slots np) pixels; the forward takes them four at a time and then one at a time, the backward four, two, one"""
    _, np_ = lanes(C, dt)
    slots = norm_slots(G, P, C, dt, bwd)
    step = slots * np_
    out = set()
    for n in {cdiv(P, step), P // step}:
        if n >= 4:
            out.add(4)
        r = n % 4
        if bwd:
            if r >= 2:
                out.add(2)
            if r % 2:
                out.add(1)
        elif r:
            out.add(1)
    return out, cdiv(P, 4 * np_) > slots


def finalize_cols(n2, threshold):
    """COLS of a finalize kernel: 32 (8 strip lanes) from `threshold` columns on, else 4 (64 strip lanes); finalize_kernel and
    finalize_stats_kernel switch at G C 2 >= 4096, finalize_grads_kernel at C 2 >= 512"""
    return 32 if n2 >= threshold else 4


def ln_maxv(D, dt):
    return cdiv(D // VEC[dt], 64)


def ln_route(D, dt):
    """du_layernorm_bwd with scratch: one fused kernel while a lane's columns fit (maxv <= 4; its LDS, 24 D bytes, is then <= 48 KB),
    the dx + column-reduction pair above, nothing above 16 vectors per lane"""
    m = ln_maxv(D, dt)
    return "unsupported" if m > 16 else ("fused" if m <= 4 and 24 * D <= 65536 else "pair")


def ln_rows_per_wave(rows, D, dt):
    """most rows one wave of the fused backward visits (rows r0 + wave, + 4, + 8 ...): more than 2 means a second trip of its loop"""
    return cdiv(pick_strip(1, rows, D, dt), 4)


# ---------------------------------------------------------------------------------------------------- shape lists
# channel reductions (stats, dot, bwd_stats, colsum): C by regime
CHAN_C = {f32: {"shuffle": (4, 32, 128), "idle": (12, 96, 1000), "lds": (256, 1024), "passes": (1028, 2048)},
          bf: {"shuffle": (8, 64, 256), "idle": (24, 192), "lds": (512, 2048), "passes": (2056, 4096)}}
CHAN_CASES = [(dt, C, name) for dt in DTS for name, cs in CHAN_C[dt].items() for C in cs]


def chan_id(c):
    return f"{'f32' if c[0] == f32 else 'bf16'}-C{c[1]}-{c[2]}"


def chan_regime_ok(dt, C, name):
    cvb, np_ = lanes(C, dt)
    if name == "shuffle":
        return reduce_path(C, dt) == "shuffle" and passes(C, dt) == 1
    if name == "idle":
        return reduce_path(C, dt) == "lds" and (cvb & (cvb - 1)) != 0 and idle_lanes(C, dt) > 0 and passes(C, dt) == 1
    if name == "lds":
        return reduce_path(C, dt) == "lds" and cvb >= 64 and passes(C, dt) == 1
    return passes(C, dt) > 1 and reduce_path(C, dt) == "lds"


def chan_gp(dt, C):
    """(G, P, what) per channel count: one pixel; fewer pixels than lanes; one strip shorter than the minimum; a second strip of one
    pixel; several strips with a ragged last one in three groups; so many groups that per_group clamps to 1"""
    _, np_ = lanes(C, dt)
    out = [(1, 1, "P=1"), (3, 4 * np_ - 1, "short-strip"), (1, 4 * np_ + 1, "strip+1"), (3, 3 * 4 * np_ + 2, "multi")]
    if np_ > 2:
        out.append((1, np_ - 1, "P<np"))
    if C <= 32:
        out.append((600, 5, "per_group=1"))
    return out


def gp_regime_ok(dt, C, G, P, what):
    S, n, (_, np_) = pick_strip(G, P, C, dt), strips(G, P, C, dt), lanes(C, dt)
    return {"P=1": P == 1 and n == 1, "P<np": P < np_ and n == 1, "short-strip": n == 1 and S == P < 4 * np_,
            "strip+1": n == 2 and P - S == 1, "multi": n >= 3 and P % S != 0, "per_group=1": G > 512 and n == 1}[what]


# bwd_stats: strip lengths of every residue mod U np (U = 4 for bf16, 2 for fp32) at np = 4
UNROLL = {f32: (256, 2), bf: (512, 4)}                      # (C, U)
# finalize kernels on synthetic partials: (COLS, G, C, strips)
FIN_STRIPS = {4: (1, 63, 64, 65, 255, 256, 257, 513), 32: (1, 7, 8, 9, 31, 32, 33, 100)}
FIN_CASES = ([(4, 1, 6, s) for s in FIN_STRIPS[4]] + [(4, 3, 5, 65), (4, 1, 2047, 3)] +
             [(32, 3, 700, s) for s in FIN_STRIPS[32]] + [(32, 1, 2048, 9)])
# finalize_grads_kernel through du_norm_act_bwd_stats_grads: (dt, G, P, C, COLS): both sides of C 2 = 512, more than one trip of the
# 2x-unrolled strip loop (strips > 2 LANES), G > 1
# 2x-unrolled strip loop (strips > 2 LANES), G > 1; the last entry: the least number of strips the case must have
GRADS_CASES = [(f32, 1, 16 * 129 + 1, 248, 4, 129), (f32, 3, 70, 252, 4, 2), (f32, 3, 16 * 17 + 1, 256, 32, 17), (bf, 2, 32 * 4 + 16, 248, 4, 2),
               (bf, 2, 32 * 17 + 3, 256, 32, 17)]

# LayerNorm
LN_D = {f32: (4, 8, 252, 256, 260, 1020, 1024, 1028, 2048, 4096), bf: (8, 16, 504, 512, 520, 2040, 2048, 2056, 4096, 8192)}
LN_D_REFUSED = {f32: 4100, bf: 8200}
LN_FIRST_PAIR = {f32: 1028, bf: 2056}                      # the first D the fused backward does not take
LN_FWD_ROWS = (1, 2, 3, 4, 5, 7, 8, 9)
LN_BWD_ROWS = (1, 3, 5, 9, 16, 17, 21, 37)                 # at D = 256 fp32 / 512 bf16 strips are 16 rows
LN_BWD_D = {f32: 256, bf: 512}
LN_TWO_TRIPS = {f32: (4097, 1024), bf: (4097, 2048)}       # (rows, D): np = 1, strips of 9 rows: wave 0 visits rows 0, 4 and 8
LN_PAIRS = [(f32, f32), (f32, bf), (bf, bf), (bf, f32)]


# ---------------------------------------------------------------------------------------------------- exact draws and their sums
def chan_inputs(G, P, C, seed):
    """two integer tensors in [-4, 4] (bf16 holds them): x / a and b"""
    return X.integers(G, P, C, seed=seed, lo=-4, hi=4), X.integers(G, P, C, seed=seed + 1, lo=-4, hi=4)


def sums64(a, b):
    """(G, P, C) terms -> (G, C, 2) fp64 sums over the pixels"""
    return torch.stack((a.double().sum(1), b.double().sum(1)), -1)


def stats64(x):
    return sums64(x, x.double() ** 2)


def dot64(a, b):
    return sums64(a.double() * b.double(), a)


def require_sums_exact(P, amax, granule=1.0):
    X.require_exact(P * amax, granule)


def act_grad64(z, act):
    if act == ACT_RELU:
        return (z > 0).double()
    if act == ACT_LEAKY:
        return torch.where(z > 0, torch.ones_like(z), torch.full_like(z, LEAKY))
    return torch.ones_like(z)


def act64(z, act):
    if act == ACT_RELU:
        return z.clamp_min(0.0)
    if act == ACT_LEAKY:
        return torch.where(z > 0, z, LEAKY * z)
    return z


def bwd_exact_inputs(G, P, C, seed):
    """x, dy integers in [-4, 4]; chosen statistics: integer mean in [-2, 2], rstd in {0.5, 1, 2}; w in {+-0.5, +-1, +-2}; b an odd
    multiple of 1/8.  xhat is a multiple of 1/2 with |xhat| <= 12, z = xhat w + b an odd multiple of 1/8 (never 0), dz xhat a multiple of
    1/2 with magnitude <= 48"""
    x, dy = chan_inputs(G, P, C, seed)
    mean = X.integers(G, C, seed=seed + 2, lo=-2, hi=2)
    rstd = X.choice([0.5, 1.0, 2.0], G, C, seed=seed + 3)
    w = X.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], C, seed=seed + 4)
    b = (2 * X.integers(C, seed=seed + 5, lo=-4, hi=3) + 1) / 8
    return x, dy, mean, rstd, w, b


def norm_terms64(x, dy, mean, rstd, w, b, act):
    """xhat, z, dz = dy act'(z) in fp64 (x, dy (G, P, C); mean, rstd (G, C); w, b (C))"""
    xh = (x.double() - mean.double()[:, None]) * rstd.double()[:, None]
    z = xh * w.double() + b.double()
    return xh, z, dy.double() * act_grad64(z, act)


def bwd_stats64(x, dy, mean, rstd, w, b, act):
    """bsums (G, C, 2) = (sum dz, sum dz xhat), dw (C) = sum_g bsums[g, :, 1], db (C) = sum_g bsums[g, :, 0]"""
    xh, z, dz = norm_terms64(x, dy, mean, rstd, w, b, act)
    bs = sums64(dz, dz * xh)
    return bs, bs[..., 1].sum(0), bs[..., 0].sum(0)


def fin_inputs(G, n, C, seed):
    """synthetic partials (G n, C, 2): first components integers in [-2, 2], second in [4, 12]: with a count of 8 n or more the variance
    second / count - (first / count)^2 is at least 1/4 - 1/16, and 513 strips stay below half the sentinel"""
    p = torch.stack((X.integers(G * n, C, seed=seed, lo=-2, hi=2), X.integers(G * n, C, seed=seed + 1, lo=4, hi=12)), -1)
    return p.contiguous()


def fin64(part, G):
    return part.double().view(G, -1, part.shape[1], 2).sum(1)


# ---------------------------------------------------------------------------------------------------- statistics: references and bounds
def stats_finalize64(sums, count, eps, rm=None, rv=None, momentum=0.1, biased=False):
    """mean, biased variance (clamped at 0), rstd and the BatchNorm running statistics (unbiased variance: count / (count - 1)) from
    (G, C, 2) sums.  biased = True is the mutant."""
    m = sums[..., 0].double() / count
    ex2 = sums[..., 1].double() / count
    var = (ex2 - m * m).clamp_min(0.0)
    out = [m, var, 1.0 / torch.sqrt(var + eps), ex2]
    if rm is not None:
        unb = 1.0 if (biased or count <= 1) else count / (count - 1.0)
        out += [(1 - momentum) * rm.double() + momentum * m[0], (1 - momentum) * rv.double() + momentum * var[0] * unb]
    return out


K_VAR = 4


def mean_bound(absmean, exact, depth=0):
    """|d mean|: 0 where the sum is exact and the count a power of two; else (2 + depth) U_F32 E|x|: the rounded 1 / count and the product
    with it, and one rounding per addition on the longest path of the sum (depth = 0 where the sum itself is exact, else sum_depth: a
    chain of n additions can err by n U_F32 of the total, and the finalize kernels do add up to 64 strip totals in sequence)"""
    return 0.0 * absmean if exact else (2 + depth) * UF * absmean


def var_bound(ex2, mean, depth=0):
    """|d var| <= K U_F32 (E[x^2] + mean^2), K = 4, for var = E[x^2] - mean^2 in fp32: E[x^2] carries three roundings (the square of an
    fp32 value, 1 / count, the product with it), mean^2 five (twice the mean's two and the product), the subtraction one of
    |var| = E[x^2] - mean^2: 3 E + 5 m^2 + (E - m^2) = 4 (E + m^2).  That is the formula's own error on sums that are exact or nearly so
    (integers, bf16-held values).  Where the sums themselves round (fp32-held random data) each of the `depth` additions on their
    longest path adds U_F32 to E[x^2] and, through the mean, 2 U_F32 to mean^2: K + 2 depth."""
    return (K_VAR + 2 * depth) * UF * (ex2 + mean * mean)


def rstd_bound(rstd, var, ex2, mean, eps, exact, depth=0):
    """|d rstd| <= rstd (1/2 |d var| / (var + eps) + 4 U_F32): the add of eps (1/2 after the square root), rsqrtf at 1 ulp = 2 U_F32, and
    one to spare"""
    dv = 0.0 if exact else var_bound(ex2, mean, depth)
    return rstd * (0.5 * dv / (var + eps) + 4 * UF)


def run_bound(old, new_term):
    """running statistics (1 - m) old + m new [unbias]: four products and one add"""
    return 6 * UF * (old.abs() + new_term.abs())


K_Y = 12


def y_bound(ref, x, mean, rstd, w, b, u_out, d_mean=0.0, d_rstd_rel=4 * UF):
    """|y - ref| <= u_out |ref| + K U_F32 ((|x| + |mean|) |rstd w| + |b|), K = 12, for y = act(x sc + sh), sc = rstd w,
    sh = b - mean sc.  Counted: rstd 4, sc 1, x sc 1, mean sc 1 (+ 2 in the mean), the subtraction in sh 1, the final add 1, the leaky
    product 1 -- 10 on the mean's term, 8 on x's, 3 on |b|.  A statistic that is off by more than its rounding (offset data) enters with
    its own bound: |x - mean| |w rstd| d_rstd_rel + |w rstd| d_mean.  LayerNorm ((x - mean) rstd w + b: 8) fits the same form."""
    sc = (rstd * w).abs()
    return u_out * ref.abs() + K_Y * UF * ((x.abs() + mean.abs()) * sc + b.abs()) + (x - mean).abs() * sc * (d_rstd_rel - 4 * UF) + sc * d_mean


K_DX = 24


def dx_bound(ref, w, rstd, dz, k1, k2, xh, u_out, depth, mdz, mdzxh):
    """|dx - ref| <= u_out |ref| + U_F32 |w rstd| (K (|dz| + |k1| + |xhat k2|) + depth (E|dz| + |xhat| E|dz xhat|)), K = 24, for
    dx = w rstd (dz - k1 - xhat k2), k = sums / count.  Counted: the prefactor 6 (rstd 4, w rstd 1, the last product 1); dz 1 (leaky);
    k1 2 (1 / count rounded, the product); xhat 5 (rstd 4, its product 1); k2's terms 8 (xhat 5, dz 1, product 1, 1 / count 1) and the
    product xhat k2 1: 14; two subtractions 2 -- 22 on the largest term.  depth: the additions on the longest path of the two sums
    (sum_depth), each at most U_F32 of the running magnitude <= count E|term|."""
    return u_out * ref.abs() + UF * (w * rstd).abs() * (K_DX * (dz.abs() + k1.abs() + (xh * k2).abs()) + depth * (mdz + xh.abs() * mdzxh))


def norm_formulas64(x, dy, w, b, act, eps, mean=None, var=None, use_batch=True):
    """the kernels' formulas in fp64 on (G, P, C): statistics over P (or the given mean / var), y, and the gradients
    dx = w rstd (dz - k1 - xhat k2) (k = 0 without batch statistics), dw, db.  -> dict"""
    x, dy, w, b = x.double(), dy.double(), w.double(), b.double()
    ex2 = (x * x).mean(1)
    if mean is None:
        mean = x.mean(1)
        var = ((x - mean[:, None]) ** 2).mean(1)                      # two-pass: the true value
    rstd = 1.0 / torch.sqrt(var + eps)
    xh, z, dz = norm_terms64(x, dy, mean, rstd, w, b, act)
    k1, k2 = (dz.mean(1), (dz * xh).mean(1)) if use_batch else (torch.zeros_like(mean), torch.zeros_like(mean))
    dx = (w * rstd)[:, None] * (dz - k1[:, None] - xh * k2[:, None])
    return dict(mean=mean, var=var, rstd=rstd, ex2=ex2, xh=xh, z=z, dz=dz, k1=k1, k2=k2, y=act64(z, act), dx=dx,
                dw=(dz * xh).sum((0, 1)), db=dz.sum((0, 1)), mdz=dz.abs().mean(1), mdzxh=(dz * xh).abs().mean(1))


def torch_norm_act64(x, dy, w, b, kind, act, eps, training=True, rm=None, rv=None, momentum=0.1):
    """the reference: F.instance_norm / F.batch_norm + activation in fp64 and torch's autograd on (G, P, C) (G = B for 'in', 1 for 'bn')
    -> y, dx, dw, db, running mean, running variance"""
    G, P, C = x.shape
    xr = x.double().permute(0, 2, 1).reshape(G, C, P, 1).contiguous().clone().requires_grad_(True)    # (plain NCHW strides, grad_output too)
    wr, br = w.double().clone().requires_grad_(True), b.double().clone().requires_grad_(True)
    rm, rv = (None, None) if rm is None else (rm.double().clone(), rv.double().clone())
    if kind == "in":
        z = F.instance_norm(xr, None, None, wr, br, True, 0.0, eps)
    else:
        z = F.batch_norm(xr, rm, rv, wr, br, training, momentum, eps)
    y = {ACT_NONE: lambda t: t, ACT_RELU: F.relu, ACT_LEAKY: lambda t: F.leaky_relu(t, LEAKY)}[act](z)
    dx, dw, db = torch.autograd.grad(y, (xr, wr, br), dy.double().permute(0, 2, 1).reshape(G, C, P, 1).contiguous())
    back = lambda t: t.reshape(G, C, P).permute(0, 2, 1)
    return back(y.detach()), back(dx), dw, db, rm, rv


def two_value_draw(G, P, C, seed, dt=f32):
    """each (group, channel) takes m + s on a random half of its pixels and m - s on the other (P even): sum = P m, sum of squares =
    P (m^2 + s^2): mean m and variance s^2 exactly.  m in [-3, 3] and s in {1, 2, 3, 4} differ per group and channel; bf16 holds m +- s"""
    assert P % 2 == 0
    g = torch.Generator().manual_seed(seed)
    m = torch.randint(-3, 4, (G, 1, C), generator=g).float()
    s = torch.randint(1, 5, (G, 1, C), generator=g).float()
    half = torch.rand(G, P, C, generator=g).argsort(1) < P // 2
    return m + torch.where(half, s, -s), m[:, 0], s[:, 0]


def affine_for(C, seed):
    """w, b per channel with |z| >= 0.25 on the two-value draw whatever rstd's last bits: xhat = +-s rstd is within 1e-5 of +-1 (eps
    against s^2 >= 1), so z = +-w + b up to 1e-5 |w|; |w| in [0.5, 2] in steps of 1/16 and b = +-(|w| + 0.3 + k / 8) keeps
    |z| >= 0.3 - 1e-4"""
    g = torch.Generator().manual_seed(seed)
    w = (8 + torch.randint(0, 25, (C,), generator=g)).float() / 16 * (torch.randint(0, 2, (C,), generator=g).float() * 2 - 1)
    b = (w.abs() + 0.3 + torch.randint(0, 8, (C,), generator=g).float() / 8) * (torch.randint(0, 2, (C,), generator=g).float() * 2 - 1)
    return w, b


def bias_for_eval(m, rm, rv, w, eps):
    """BatchNorm in eval normalises with the running statistics, which are not the data's: b = -(m - rm) rstd w centres z on the two
    values +-s rstd w, and with running variances in [1, 3] |z| >= 1 / sqrt(3 + eps) / 2 > 0.28"""
    return (-(m.double() - rm.double()) / torch.sqrt(rv.double() + eps) * w.double()).float()


# norm_act through ops.norm_act and autograd: (dt, G, P, C)
NORM_ACT_SHAPES = [(f32, 3, 2, 4), (f32, 1, 130, 12), (f32, 3, 64, 32), (f32, 2, 46, 1028), (bf, 3, 6, 8), (bf, 2, 258, 24), (bf, 1, 1024, 64),
                   (bf, 2, 34, 2056)]
NORM_ACT_MODES = ("in", "bn-train", "bn-eval")


# ---------------------------------------------------------------------------------------------------- LayerNorm: references and bounds
def ln_draw(rows, D, seed):
    """each row takes m_r + a_r on a random half of its columns and m_r - a_r on the other: mean m_r and variance a_r^2 exactly;
    w in [0.5, 2] in steps of 1/8 and b in quarters differ per column"""
    x, m, a = two_value_draw(1, D, rows, seed)
    col = torch.arange(D)
    return x[0].t().contiguous(), m[0], a[0], 0.5 + (col * 7 % 13).float() / 8, ((col * 5 % 9) - 4).float() / 4


def ln_fwd64(x, w, b, eps):
    x = x.double()
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / torch.sqrt(var + eps)
    return (x - mean[:, None]) * rstd[:, None] * w.double() + b.double(), mean, rstd


def ln_bwd_inputs(rows, D, seed):
    """x, dy, dres integers in [-4, 4]; integer mean in [-2, 2] and rstd in {0.5, 1, 2} per row; w in {+-0.5, +-1, +-2}: g = dy w, xhat
    and every term of c1, c2, dw, db are multiples of 1/4 below 2^7"""
    x, dy = (t[0] for t in chan_inputs(1, rows, D, seed))
    return (x, dy, X.integers(rows, seed=seed + 2, lo=-2, hi=2), X.choice([0.5, 1.0, 2.0], rows, seed=seed + 3),
            X.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], D, seed=seed + 4), X.integers(rows, D, seed=seed + 5, lo=-4, hi=4))


def ln_bwd64(x, dy, w, mean, rstd, dres=None, c1_short=0):
    """dx = rstd (g - c1 - xhat c2) [+ dres], g = dy w, c1 = mean_D g, c2 = mean_D g xhat; dw = sum_rows dy xhat, db = sum_rows dy.
    c1_short > 0 is the mutant that forms c1 over D - c1_short columns.  -> dx, dwdb (2, D) planar, and the bound's terms"""
    x, dy, w, mean, rstd = (t.double() for t in (x, dy, w, mean, rstd))
    D = x.shape[1]
    xh = (x - mean[:, None]) * rstd[:, None]
    g = dy * w
    c1 = g[:, :D - c1_short].sum(1) / D
    c2 = (g * xh).mean(1)
    dx = rstd[:, None] * (g - c1[:, None] - xh * c2[:, None])
    if dres is not None:
        dx = dx + dres.double()
    return dx, torch.stack(((dy * xh).sum(0), dy.sum(0))), (g, c1, c2, xh)


K_LN_DX = 8


def ln_dx_bound(ref, rstd, g, c1, c2, xh, dres, u_out):
    """|dx - ref| <= u_out |ref| + K U_F32 (rstd (|g| + |c1| + |xhat c2|) + |dres|), K = 8.  Counted on the exact draws (sums exact):
    c1 and c2 one division each, xhat c2 1, two subtractions 2, the product with rstd 1, the add of dres 1 -- 7, and one for g = dy w
    where w is not dyadic"""
    terms = rstd[:, None] * (g.abs() + c1.abs()[:, None] + (xh * c2[:, None]).abs())
    return u_out * ref.abs() + K_LN_DX * UF * (terms + (0.0 if dres is None else dres.double().abs()))


# ---------------------------------------------------------------------------------------------------- offset statistics
OFFSETS = (0.0, 8.0, 64.0)


def offset_draw(P, C, m, seed, full=False):
    """(1, P, C): N(+-m, 1) held in bf16 (the data the bound K = 4 was characterised on; the fp32 kernels read the same values);
    the last channel is the constant m + 3 (sigma = 0).  full = True keeps fp32's whole mantissa (measured and printed, never gated:
    there the sums round too)"""
    g = torch.Generator().manual_seed(seed)
    sign = (torch.arange(C) % 2).float() * 2 - 1
    x = torch.randn(1, P, C, generator=g) + m * sign
    x[..., -1] = m + 3.0
    return x if full else quant(x, bf)


def offset_bounds(x, w, b, eps, u_out, depth):
    """fp64 statistics of x (1, P, C) (two-pass, what torch computes) and the bounds of mean, rstd and y for a kernel that forms the
    variance as E[x^2] - mean^2 in fp32"""
    f = norm_formulas64(x, torch.zeros_like(x), w, b, ACT_NONE, eps)
    dm = mean_bound(x.double().abs().mean(1), False, depth)
    dr = rstd_bound(f["rstd"], f["var"], f["ex2"], f["mean"], eps, exact=False)
    yb = y_bound(f["y"], x.double(), f["mean"][:, None], f["rstd"][:, None], w.double(), b.double(), u_out, d_mean=dm[:, None],
                 d_rstd_rel=(dr / f["rstd"])[:, None])
    return f, dm, dr, yb


# ---------------------------------------------------------------------------------------------------- emulated kernels (CPU, fp32) and mutants
def emu_strip_sums(a, b, STRIP, np_, seed=0, drop_last_pixel=False, group_shift=0, skip_strip=None, slot_shift=0):
    """a two-stage reduction as norm.hip runs it, in fp32: (G, P, C) terms -> per strip and pixel lane a running sum, lanes combined in a
    scrambled order, strips combined in a scrambled order.  Mutants: the last pixel of every strip dropped; the group boundary off by
    `group_shift` pixels (the flat tensor is cut at g P + shift); one strip left out of the finalize; the last channel vector (4 channels)
    written `slot_shift` slots further.  -> (G, C, 2) fp32"""
    G, P, C = a.shape
    gen = torch.Generator().manual_seed(seed)
    fa, fb = a.float().reshape(G * P, C), b.float().reshape(G * P, C)
    out = torch.zeros(G, C, 2)
    for g in range(G):
        parts = []
        for p0 in range(0, P, STRIP):
            p1 = min(P, p0 + STRIP) - (1 if drop_last_pixel else 0)
            lo = min(max(g * P + group_shift + p0, 0), G * P)
            hi = min(max(g * P + group_shift + p1, 0), G * P)
            lane = []
            for tp in range(np_):
                sa, sb = torch.zeros(C), torch.zeros(C)
                for p in range(lo + tp, hi, np_):
                    sa, sb = sa + fa[p], sb + fb[p]
                lane.append(torch.stack((sa, sb), -1))
            acc = torch.zeros(C, 2)
            for i in torch.randperm(np_, generator=gen).tolist():
                acc = acc + lane[i]
            parts.append(acc)
        tot = torch.zeros(C, 2)
        for i in torch.randperm(len(parts), generator=gen).tolist():
            if i != skip_strip:
                tot = tot + parts[i]
        out[g] = tot
    if slot_shift:
        moved = out.clone()
        moved[:, C - 4:] = 0
        dst = (C - 4 + 4 * slot_shift) % C
        moved[:, dst:dst + 4] = out[:, C - 4:]
        out = moved
    return out


def emu_stats_finalize(sums, count, eps, rm=None, rv=None, momentum=0.1, mean_bf16=False):
    """finalize_stats_kernel / norm_stats_finalize_kernel in fp32: the one-pass variance.  Mutant: the mean taken through bf16"""
    inv = torch.tensor(1.0 / count, dtype=f32)
    m = sums[..., 0] * inv
    if mean_bf16:
        m = m.to(bf).float()
    var = (sums[..., 1] * inv - m * m).clamp_min(0.0)
    rstd = torch.rsqrt(var + torch.tensor(eps, dtype=f32))
    if rm is None:
        return m, rstd
    mo, unb = torch.tensor(momentum, dtype=f32), torch.tensor(count / (count - 1.0) if count > 1 else 1.0, dtype=f32)
    return m, rstd, (1 - mo) * rm.float() + mo * m[0], (1 - mo) * rv.float() + mo * var[0] * unb


def emu_norm_fwd(x, mean, rstd, w, b, act, dt):
    """norm_act_fwd_kernel in fp32: y = act(x sc + sh), rounded into dt"""
    sc = rstd.float() * w.float()
    sh = b.float() - mean.float() * sc
    z = x.float() * sc[:, None] + sh[:, None]
    y = z if act == ACT_NONE else (z.clamp_min(0) if act == ACT_RELU else torch.where(z > 0, z, torch.tensor(0.01, dtype=f32) * z))
    return y.to(dt)


def emu_norm_bwd(x, dy, mean, rstd, w, b, act, count, dt, STRIP, np_, use_batch=True, leaky_at_zero_only=False, **mutant):
    """norm_act_bwd_stats_kernel + finalize + norm_act_bwd_dx_kernel in fp32.  Mutant: the leaky slope applied at z = 0 only (z < 0
    takes slope 0).  -> dx (dt), bsums (G, C, 2), dw, db"""
    xh = (x.float() - mean.float()[:, None]) * rstd.float()[:, None]
    z = xh * w.float() + b.float()
    slope = torch.tensor(0.01, dtype=f32)
    if act == ACT_LEAKY:
        gr = torch.where(z > 0, torch.ones_like(z), torch.where(z == 0, slope, torch.zeros_like(z)) if leaky_at_zero_only else slope.expand_as(z))
    else:
        gr = (z > 0).float() if act == ACT_RELU else torch.ones_like(z)
    dz = dy.float() * gr
    bs = emu_strip_sums(dz, dz * xh, STRIP, np_, **mutant)
    inv = torch.tensor(1.0 / count, dtype=f32)
    k1, k2 = (bs[..., 0] * inv, bs[..., 1] * inv) if use_batch else (torch.zeros_like(mean), torch.zeros_like(mean))
    dx = (w.float() * rstd.float())[:, None] * (dz - k1[:, None] - xh * k2[:, None])
    return dx.to(dt), bs, bs[..., 1].sum(0), bs[..., 0].sum(0)


def emu_ln_fwd(x, w, b, eps, dt):
    """layernorm_fwd_kernel in fp32: two-pass statistics over the row, y rounded into dt"""
    x = x.float()
    D = x.shape[1]
    mean = x.sum(1) / D
    d = x - mean[:, None]
    rstd = torch.rsqrt((d * d).sum(1) / D + torch.tensor(eps, dtype=f32))
    return (d * rstd[:, None] * w.float() + b.float()).to(dt), mean, rstd


def emu_ln_bwd(x, dy, w, mean, rstd, dres, dt, STRIP, seed=0, tail_row_missing=False, swapped=False, c1_short=0, unwritten_row=None):
    """the fused LayerNorm backward in fp32: dx per row, (dw, db) as strip partials combined in a scrambled order, planar (2, D).
    Mutants: the last row of every strip missing from dw / db (present in dx); dw and db swapped; c1 over D - c1_short columns; a row of
    dx never written (it keeps the sentinel)"""
    x, dy, w, mean, rstd = (t.float() for t in (x, dy, w, mean, rstd))
    rows, D = x.shape
    xh = (x - mean[:, None]) * rstd[:, None]
    g = dy * w
    c1 = g[:, :D - c1_short].sum(1) / D
    c2 = (g * xh).sum(1) / D
    dx = rstd[:, None] * (g - c1[:, None] - xh * c2[:, None])
    if dres is not None:
        dx = dx + dres.float()
    dx = dx.to(dt)
    if unwritten_row is not None:
        dx[unwritten_row] = X.SENTINEL
    gen = torch.Generator().manual_seed(seed)
    parts = []
    for r0 in range(0, rows, STRIP):
        r1 = min(rows, r0 + STRIP) - (1 if tail_row_missing else 0)
        parts.append(torch.stack(((dy[r0:r1] * xh[r0:r1]).sum(0), dy[r0:r1].sum(0))))
    tot = torch.zeros(2, D)
    for i in torch.randperm(len(parts), generator=gen).tolist():
        tot = tot + parts[i]
    return dx, (tot.flip(0) if swapped else tot)
