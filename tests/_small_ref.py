"""fp64 references, draws, shape lists and gates for the small NHWC kernels of csrc/elementwise.hip (tests/test_gpu_small_ops.py, kept
honest by tests/test_cpu_small_ops.py).  Plain torch on the CPU, no library load.  Tensors are NHWC throughout, like the kernels'.

Two instruments, as in tests/_exact.py: exact inputs (small integers, dyadic weights) compared bit for bit, and derived per-element bounds
where exactness is impossible (general resize ratios, sigmoid / erf).  The deliberately broken restatements (`pad`, `last`,
`align_corners`, `overwrite`, `wrong_scale`, `order`, `round_each`) exist so that the CPU module can show that each gate sees the bug."""
import math

import torch
import torch.nn.functional as F

import _exact as X

bf, f32 = torch.bfloat16, torch.float32
DTS = [f32, bf]
VEC = {f32: 4, bf: 8}                        # elements of a 16-byte vector (csrc/common.h: Elem<T>::VEC)
U = {f32: X.U_F32, bf: X.U_BF16}


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def quant(t, dt):
    """a CPU fp32 tensor through dt: the reference sees what the kernel sees"""
    return t.to(dt).float()


def within(out, ref64, bound, what=""):
    """(ok, message) of the per-element gate |out - ref| <= bound"""
    o = out.detach().cpu().double()
    assert o.shape == ref64.shape, (what, o.shape, ref64.shape)
    if not bool(torch.isfinite(o).all()):
        return False, f"{what}: non-finite values"
    ex = (o - ref64).abs() - bound
    i = int(ex.argmax())
    share = float(((o - ref64).abs() / torch.as_tensor(bound, dtype=torch.float64).expand_as(ex).clamp_min(1e-300)).max())
    return not bool((ex > 0).any()), (f"{what}: {int((ex > 0).sum())} of {ex.numel()} elements outside the bound; worst at flat index {i}: got "
                                      f"{float(o.flatten()[i])}, want {float(ref64.flatten()[i])}; worst share of the bound {share:.3f}")


# ---------------------------------------------------------------------------------------------------- max-pool 3 x 3 / stride 2 / pad 1
POOL_HW = [(1, 1), (1, 7), (2, 2), (3, 3), (4, 5), (5, 4), (8, 8), (17, 22)]
POOL_B = (1, 3)
POOL_C = {f32: (4, 12, 8, 24, 64), bf: (8, 24, 64)}
POOL_DRAWS = {"ties": [0.0, 1.0, 2.0], "negative": [-3.0, -2.0, -1.0]}


def pool_out(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def pool_inputs(B, H, W, Cc, draw, seed):
    """x from three values (ties in every window), dy integers in [-8, 8] (a pixel receives at most 4: exact in fp32 and in bf16)"""
    Ho, Wo = pool_out(H, W)
    return X.choice(POOL_DRAWS[draw], B, H, W, Cc, seed=seed), X.integers(B, Ho, Wo, Cc, seed=seed + 1, lo=-8, hi=8)


def pool_ref(x, dy, dtype=torch.float64):
    """torch's max_pool2d and its backward (tie rule: the first maximum in scan order) -> y, dx"""
    xr = nchw(x).to(dtype).clone().requires_grad_(True)
    y = F.max_pool2d(xr, 3, 2, 1)
    dx, = torch.autograd.grad(y, xr, nchw(dy).to(dtype))
    return nhwc(y.detach()), nhwc(dx)


def pool_brute(x, dy, pad=-math.inf, last=False):
    """a loop over the windows: the maximum of the taps inside the image starting from `pad`, the FIRST maximum taking the gradient.
    Mutants: pad = 0 (what a zero-padded window gives), last = True (the last maximum wins)."""
    x, dy = x.double(), dy.double()
    B, H, W, Cc = x.shape
    Ho, Wo = pool_out(H, W)
    y = torch.empty(B, Ho, Wo, Cc, dtype=torch.float64)
    dx = torch.zeros_like(x)
    for yo in range(Ho):
        for xo in range(Wo):
            best = torch.full((B, Cc), pad, dtype=torch.float64)
            tap = torch.full((B, Cc), -1, dtype=torch.long)
            taps = [(yo * 2 - 1 + i, xo * 2 - 1 + j) for i in range(3) for j in range(3)]
            for k, (yi, xi) in enumerate(taps):
                if 0 <= yi < H and 0 <= xi < W:
                    v = x[:, yi, xi]
                    upd = (v >= best) if last else (v > best)
                    best = torch.where(upd, v, best)
                    tap = torch.where(upd, torch.full_like(tap, k), tap)
            y[:, yo, xo] = best
            for k, (yi, xi) in enumerate(taps):
                if 0 <= yi < H and 0 <= xi < W:
                    dx[:, yi, xi] += torch.where(tap == k, dy[:, yo, xo], torch.zeros_like(best))
    return y, dx


# ---------------------------------------------------------------------------------------------------- bilinear add / resize
# exact arm: dyadic weights (1x, 2x, 4x, 0.5x) on integers -- every product and sum is a multiple of 1/64 below 2^5: exact in fp32
BL_EXACT = [((4, 4), (8, 8)), ((3, 5), (12, 20)), ((8, 8), (4, 4)), ((6, 6), (6, 6))]
BL_GENERAL = [((4, 4), (16, 16)), ((16, 24), (31, 40)), ((12, 10), (12, 17)), ((16, 16), (13, 11)), ((10, 10), (4, 4)), ((1, 7), (5, 7)),
              ((7, 1), (7, 5)), ((32, 32), (11, 3)), ((3, 5), (32, 29)), ((9, 9), (27, 27)), ((5, 6), (1, 1))]


def bl_id(g):
    return f"{g[0][0]}x{g[0][1]}to{g[1][0]}x{g[1][1]}"


def bl_exact_inputs(geo, Cc, dt, seed=1, B=2):
    """src, base, dy: integers in [-8, 8].  At 4x the weights are multiples of 1/64, and only ~0.93 of such results fit bf16's 8 bits: for
    bf16 the 4x sources are multiples of 4 (granule 1/16), which brings the share of exactly representable results to 1.0"""
    (hs, ws), size = geo
    step = 4 if (dt == bf and size[0] == 4 * hs) else 1
    src = X.integers(B, hs, ws, Cc, seed=seed, lo=-8 // step, hi=8 // step) * step
    return src, X.integers(B, *size, Cc, seed=seed + 1, lo=-8, hi=8), X.integers(B, *size, Cc, seed=seed + 2, lo=-8, hi=8)


def bilinear_ref64(src, size, base=None, align_corners=False):
    """F.interpolate(bilinear) in fp64 (+ base); align_corners = True is the mutant"""
    r = nhwc(F.interpolate(nchw(src).double(), size=tuple(size), mode="bilinear", align_corners=align_corners))
    return r if base is None else r + base.double()


def bilinear_bwd_ref64(src_shape, dy, size, dtype=torch.float64):
    """the data gradient of F.interpolate(bilinear, align_corners=False) by torch's autograd"""
    B, Hs, Ws, Cc = src_shape
    x = torch.zeros(B, Cc, Hs, Ws, dtype=dtype, requires_grad=True)
    y = F.interpolate(x, size=tuple(size), mode="bilinear", align_corners=False)
    return nhwc(torch.autograd.grad(y, x, nchw(dy).to(dtype))[0])


def bilinear_bound(ref64, Hs, Ws, amax, dt):
    """|out - ref| <= u_out |ref| + 2^-23 (Hs + Ws + 4) max|src|: the output rounding, and the source coordinate formed in fp32 from a
    rounded scale (with or without an FMA), off by at most a few 2^-24 Hs, which moves the result by that times the tap difference"""
    return U[dt] * ref64.abs() + 2.0 ** -23 * (Hs + Ws + 4) * float(amax)


# ---------------------------------------------------------------------------------------------------- squeeze-excitation
SE_LDS_FLOATS = 8000                          # csrc/elementwise.hip, du_se_gate_bwd: Bc = 8000 / (C + R) samples resident at once
# (B, H, W, C, R, sliced, chunks the gate backward must take)
SE_SHAPES = [(20, 2, 2, 512, 32, False, (14, 6)), (70, 1, 1, 128, 8, False, (58, 12)), (15, 2, 3, 1024, 64, False, (7, 7, 1)),
             (2, 3, 3, 8, 1, False, (2,)), (3, 4, 4, 16, 2, True, (3,))]


def se_id(s):
    return "x".join(map(str, s[:5])) + ("-sliced" if s[5] else "") + f"-{len(s[6])}chunk" + ("s" if len(s[6]) > 1 else "")


def se_chunks(B, Cc, R):
    Bc = min(SE_LDS_FLOATS // (Cc + R), B)
    return tuple(min(Bc, B - b0) for b0 in range(0, B, Bc))


def se_inputs(B, H, W, Cc, R, dt, seed=1):
    g = lambda *s, seed, scale=1.0: torch.randn(*s, generator=torch.Generator().manual_seed(seed)) * scale
    x, sc, go = (quant(g(B, H, W, Cc, seed=seed + i), dt) for i in (0, 1, 6))
    w1, b1 = g(R, Cc, 1, 1, seed=seed + 2, scale=Cc ** -0.5), g(R, seed=seed + 3, scale=0.3)
    w2, b2 = g(Cc, R, 1, 1, seed=seed + 4, scale=R ** -0.5), g(Cc, seed=seed + 5, scale=0.3)
    return x, w1, b1, w2, b2, sc, go


def se_ref(x, w1, b1, w2, b2, sc, go, dtype=torch.float64):
    """y = x * sigmoid(W2 relu(W1 mean_hw(x) + b1) + b2) + shortcut and the six gradients (x, w1, b1, w2, b2, shortcut)"""
    ins = [t.to(dtype).clone().requires_grad_(True) for t in (x, w1, b1, w2, b2, sc)]
    xr, w1r, b1r, w2r, b2r, scr = ins
    s = xr.mean((1, 2))
    gate = torch.sigmoid(F.linear(F.relu(F.linear(s, w1r.flatten(1), b1r)), w2r.flatten(1), b2r))
    y = xr * gate[:, None, None, :] + scr
    return y.detach(), list(torch.autograd.grad(y, ins, go.to(dtype)))


def se_gate_bwd_chunked(x, w1, b1, w2, b2, go, Bc, overwrite=False):
    """the gate backward as the kernel walks it, in fp32: chunks of Bc samples, parameter gradients accumulated across chunks.
    overwrite = True is the mutant that stores the last chunk's sums instead of adding them.  -> dW1 (R, C), db1, dW2 (C, R), db2"""
    B, H, W, Cc = x.shape
    W1, W2 = w1.flatten(1).float(), w2.flatten(1).float()
    pooled = x.float().mean((1, 2))
    hidden = F.relu(pooled @ W1.t() + b1.float())
    gate = torch.sigmoid(hidden @ W2.t() + b2.float())
    dsum = (go.float() * x.float()).sum((1, 2))
    out = None
    for b0 in range(0, B, Bc):
        sl = slice(b0, min(b0 + Bc, B))
        dgp = dsum[sl] * gate[sl] * (1 - gate[sl])
        dhp = (dgp @ W2) * (hidden[sl] > 0)
        part = [dhp.t() @ pooled[sl], dhp.sum(0), dgp.t() @ hidden[sl], dgp.sum(0)]
        out = part if (out is None or overwrite) else [a + p for a, p in zip(out, part)]
    return out


def se_param_gate(got, want, dt, tol):
    """the gate of the four parameter gradients: rel() < 2 tol, and for fp32 element-wise |a - b| <= 1e-4 max|b| + 1e-3 |b|"""
    from test_gpu_ops import close, rel
    msgs = []
    for name, a, b in zip(("dw1", "db1", "dw2", "db2"), got, want):
        a = a.reshape(b.shape)
        r = rel(a, b)
        if not r < 2 * tol:
            msgs.append(f"{name}: rel {r:.3e}")
        if dt == f32:
            ok, m = close(a, b, 1e-3, 1e-4 * float(b.abs().max()))
            if not ok:
                msgs.append(f"{name}: {m}")
    return msgs


# ---------------------------------------------------------------------------------------------------- FiLM / FAPM projection
FILM_ROWS = (1, 3, 257)
FILM_R = {f32: (4, 12, 8, 24, 64), bf: (8, 24, 64)}
# (B, H, W, D, R): 2R = 64 (the packed-transpose data gradients once the pack is registered), 2R = 16 (mm_dgrad)
FAPM_SHAPES = [(2, 3, 5, 64, 32), (1, 2, 2, 48, 8)]


def film_inputs(rows, R, seed):
    return (X.integers(rows, 2 * R, seed=seed, lo=-8, hi=8), X.integers(rows, 2 * R, seed=seed + 1, lo=-8, hi=8),
            X.integers(rows, R, seed=seed + 2, lo=-8, hi=8))


def film_ref64(gb, z2, dz, wrong_scale=False):
    """z = gamma * z_specific + beta; dgb = [dz * z_specific | dz]; d z_specific = dz * gamma  (wrong_scale: * beta, the mutant)"""
    gb, z2, dz = gb.double(), z2.double(), dz.double()
    R = dz.shape[1]
    gamma, beta, zs = gb[:, :R], gb[:, R:], z2[:, R:]
    return gamma * zs + beta, torch.cat([dz * zs, dz], 1), dz * (beta if wrong_scale else gamma)


def fapm_inputs(B, H, W, D, R, dt, biases, seed=1):
    """x, ws, wp, bs, bp, wf, bf, go: weights already representable in dt (the op casts its fp32 masters to the activation dtype)"""
    g = lambda *s, seed, scale=1.0: quant(torch.randn(*s, generator=torch.Generator().manual_seed(seed)) * scale, dt)
    x, go = g(B, H, W, D, seed=seed), g(B, H, W, R, seed=seed + 1)
    ws, wp, wf = g(R, D, 1, 1, seed=seed + 2, scale=D ** -0.5), g(R, D, 1, 1, seed=seed + 3, scale=D ** -0.5), g(2 * R, R, 1, 1, seed=seed + 4, scale=R ** -0.5)
    bs, bp, bfm = (g(R, seed=seed + 5, scale=0.3), g(R, seed=seed + 6, scale=0.3), g(2 * R, seed=seed + 7, scale=0.3)) if biases else (None, None, None)
    return x, ws, wp, bs, bp, wf, bfm, go


def fapm_ref64(x, ws, wp, bs, bp, wf, bfm, go):
    """ops.fapm_project's docstring in fp64: z2 = x [Ws; Wp]^T + b, gb = z2[:, :R] Wf^T + bf, z = gamma * z2[:, R:] + beta.
    -> z (B, H, W, R), gradients in the order (x, ws, wp, bs, bp, wf, bf) (None for an absent bias)"""
    ins = [None if t is None else t.double().clone().requires_grad_(True) for t in (x, ws, wp, bs, bp, wf, bfm)]
    xr, wsr, wpr, bsr, bpr, wfr, bfr = ins
    R = ws.shape[0]
    z2 = xr.flatten(0, 2) @ torch.cat([wsr.flatten(1), wpr.flatten(1)], 0).t()
    if bsr is not None:
        z2 = z2 + torch.cat([bsr, bpr], 0)
    gb = z2[:, :R] @ wfr.flatten(1).t()
    if bfr is not None:
        gb = gb + bfr
    z = (gb[:, :R] * z2[:, R:] + gb[:, R:]).view(*x.shape[:3], R)
    have = [t for t in ins if t is not None]
    gr = iter(torch.autograd.grad(z, have, go.double()))
    return z.detach(), [None if t is None else next(gr) for t in ins]


# ---------------------------------------------------------------------------------------------------- streaming helpers
SWIGLU_SHAPES = {bf: [(1, 4), (3, 20)], f32: [(1, 2), (3, 10)]}
SWIGLU_BIG, SWIGLU_BLOCKS = (2049, 4096), 8192               # (rows, h); the launcher's grid clamp
SWIGLU_GATES = [30.0, -30.0, 90.0, -90.0, 120.0, -120.0]
SAMPLE_N, SAMPLE_BLOCKS = (4, 524292), 512
SPLITK_SPLITS, SPLITK_N = (1, 2, 7), (4, 1028, 65540)
CAST_N = (1, 7, 1025)
ACT_N_BIG, ACT_BLOCKS = 4194312, 2048
LEAKY = float(torch.tensor(0.01, dtype=f32).double())        # the slope as the kernel holds it (0.01f)


def swiglu_inputs(rows, h, seed):
    """u (rows, 2h), columns (2j, 2j + 1) = (gate, value): exact pre-activations in 1/32 steps, |.| <= 3.875, and in the first pairs (as
    many as fit) the large gates whose exp overflows or underflows fp32"""
    g, v = X.integers(rows, h, seed=seed, lo=-124, hi=124) / 32, X.integers(rows, h, seed=seed + 1, lo=-124, hi=124) / 32
    k = min(len(SWIGLU_GATES), rows * h)
    g.view(-1)[:k] = torch.tensor(SWIGLU_GATES[:k])
    return torch.stack((g, v), -1).reshape(rows, 2 * h).contiguous(), g, v


def sample_copy_ref(x, idx, src=None):
    """gather x[idx]; with src the scatter x[idx] = src on a copy"""
    if src is None:
        return x[idx]
    y = x.clone()
    y[idx] = src
    return y


def splitk_ref(slabs, reverse=False, round_each=False):
    """what du_splitk_reduce_bf16 does: slabs (splits, n) added in index order in fp32, rounded to bf16 once.  Mutants: reversed order;
    a rounding to bf16 after every slab"""
    order = range(slabs.shape[0] - 1, -1, -1) if reverse else range(slabs.shape[0])
    acc = None
    for s in order:
        acc = slabs[s].float().clone() if acc is None else acc + slabs[s].float()
        if round_each:
            acc = acc.to(bf).float()
    return acc.to(bf)


def splitk_midpoints():
    """two slabs whose sums are bf16 midpoints of both parities, and what ties-to-even makes of them"""
    a = torch.tensor([1.0, 1.0, -1.0, -1.0])
    b = torch.tensor([2.0 ** -8, 3 * 2.0 ** -8, -2.0 ** -8, -3 * 2.0 ** -8])
    want = torch.tensor([1.0, 1.0 + 2.0 ** -6, -1.0, -1.0 - 2.0 ** -6])
    return torch.stack((a, b)), want


def cast_specials():
    """fp32 inputs: bf16 midpoints of both parities (down to even / up to even), just off a midpoint, subnormals (fp32's and bf16's),
    +-inf, above bf16's largest finite (rounds to inf), bf16's largest finite, signed zeros, a NaN"""
    big = float(torch.finfo(bf).max)
    return torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -1.0 - 2.0 ** -8, -1.0 - 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, 1.0 + 2.0 ** -8 - 2.0 ** -20,
                         2.0 ** -149, 2.0 ** -130, -2.0 ** -133, 3 * 2.0 ** -135, math.inf, -math.inf, 3.4e38, -3.4e38, big, 0.0, -0.0, math.nan], dtype=f32)


def cast_inputs(n, dt, seed=0):
    s = cast_specials()
    r = torch.randn(max(n, 1), generator=torch.Generator().manual_seed(seed)) * 3
    t = torch.cat([s, r])
    t = torch.roll(t, -(n % 5)) if n < s.numel() else t             # short inputs start at different specials
    return t[:n].to(dt)


def same_bits(a, b):
    """equal bit for bit outside NaNs (signed zeros included), NaN exactly where b has one"""
    a, b = a.detach().cpu(), b.detach().cpu()
    if a.shape != b.shape or a.dtype != b.dtype or not torch.equal(a.isnan(), b.isnan()):
        return False
    it = torch.int16 if a.dtype == bf else torch.int32
    keep = ~b.isnan()
    return torch.equal(a.view(it)[keep], b.view(it)[keep])


def gelu_grad64(z):
    z = z.double()
    return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def gelu_tanh_grad64(z):
    """the derivative of the tanh form (the approximation that must stay outside the gate)"""
    z = z.double().clone().requires_grad_(True)
    return torch.autograd.grad(X.gelu_tanh64(z).sum(), z)[0]


def act_inputs(n, dt, seed):
    """z with +0, -0 and values on both sides; dy random; both representable in dt"""
    g = torch.Generator().manual_seed(seed)
    z, dy = quant(torch.randn(n, generator=g) * 2, dt), quant(torch.randn(n, generator=g), dt)
    z[::7] = 0.0
    z[3::7] = -0.0
    return z, dy


def act_bwd_ref64(z, dy, kind, slope=LEAKY):
    """dz = dy * act'(z): kind 'relu' / 'leaky' (exact: one fp32 product) / 'gelu' / 'gelu_tanh' (the mutant)"""
    z, dy = z.double(), dy.double()
    if kind == "relu":
        return dy * (z > 0)
    if kind == "leaky":
        return dy * torch.where(z > 0, torch.ones_like(z), torch.full_like(z, slope))
    return dy * (gelu_grad64(z) if kind == "gelu" else gelu_tanh_grad64(z))


def act_gelu_bound(ref64, dy, dt):
    """|dz - dy gelu'64(z)| <= u_out |ref| + E_ACT_CAP |dy|"""
    return U[dt] * ref64.abs() + X.E_ACT_CAP * dy.double().abs()


def act_gelu_excess(out, ref64, dy, dt):
    """the figure that is printed, never gated on: worst (|dz - ref| - u_out |ref|) / |dy|"""
    e = ((out.detach().cpu().double() - ref64).abs() - U[dt] * ref64.abs()) / dy.double().abs().clamp_min(1e-30)
    return float(e[dy != 0].max().clamp_min(0.0))
