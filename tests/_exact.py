"""Exact-input instruments for the sum-of-products kernels (tests/test_gpu_exact.py, kept honest by tests/test_cpu_exact.py).

Exact inputs: operands are small integers (or dyadic fractions), so every product and every partial sum is an integer multiple of a
granule with magnitude below 2^24 granules.  fp32 accumulation is then exact IN ANY ORDER (tile order, split-K, slab / ticket reduce,
pair exchange, atomics), the fp64 reference is the true value, and the kernel must equal it bit for bit: one missing, doubled or misplaced
term changes the integer.  There is no tolerance here.

Where exactness is impossible (erf / sigmoid / softmax) the pre-activation is still exact and the gate is a derived bound per element."""
import math

import torch

LIMIT = float(2 ** 24)       # integers of magnitude <= 2^24 are exact in fp32
SENTINEL = 12345.0           # pre-fill of every output buffer (bf16 rounds it to 12352); the conditions keep |reference| far below it
GUARD_ROWS = 64
U_BF16, U_F32 = 2.0 ** -8, 2.0 ** -24      # unit roundoff of the two result formats (round to nearest even)

# e_act: the allowance for the kernel's own evaluation of erf / exp / sigmoid in  |out - act64(s)| <= u_out |act64(s)| + e_act max(1, |s|).
# It cannot be derived from outside; it is MEASURED against the fp64 formula and doubled, and may never exceed the cap (a sixteenth of bf16's
# unit roundoff: the allowance must not become the gate; tanh-GELU differs from erf-GELU by ~2^-11 and has to stay outside).
E_ACT_CAP = 2.0 ** -12
# GELU: measured 7.909e-08 = worst |out - gelu64(s)| / max(1, |s|) over the fp32-result launches of the bias + erf-GELU epilogue on exact
# pre-activations in 1/32 steps (|s| <= 3.9): the 128 x 128 tile kernel (route 2) and the 256 x 256 / 256 x 128 multi-phase kernels (routes
# 3 / 4) at 8232 x 4096 x 1024, 33000 x 1000 x 896 / 640 and 70000 x 264 x 256 -- the same figure on every one of them (one erf routine);
# printed by test_gelu_epilogue_per_element_bound.  Factor 2.
E_ACT_GELU = 2 * 7.909e-08
# SwiGLU: the gate epilogue has no fp32-result launch (bf16 only), so it was measured on bf16 results (1029 x 16384 x 4096, routes 3 and 4),
# both ways the result format allows: on the 153307 elements whose fp64 value bf16 holds exactly, worst |out - ref| / max(1, |g v|) = 0.0;
# on the rest, the excess over the output rounding max(0, |out - ref| - 2^-8 |ref|) / max(1, |g v|) = 0.0 (printed by
# test_swiglu_epilogue_per_element_bound).  Twice zero is no allowance at all, and the gate's own arithmetic needs one: sigmoid is an
# exponential, an add and a divide in fp32 and two products follow, five roundings of 2^-24 relative to |silu(g) v| <= |g v|.  The constant is
# that figure, doubled like a measured one: 10 x 2^-24 = 6.0e-7, 1/400 of the cap.
E_ACT_SWIGLU = 2 * 5 * U_F32
assert E_ACT_GELU <= E_ACT_CAP and E_ACT_SWIGLU <= E_ACT_CAP


# ---------------------------------------------------------------------------------------------------- draws
def ternary(*shape, seed, density=2.0 / 3.0):
    """fp32 tensor drawn uniformly from {-1, 0, 1} (density = share of non-zeros; lower it where a long sum would leave bf16's integers)"""
    g = torch.Generator().manual_seed(seed)
    sign = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
    return sign * (torch.rand(shape, generator=g) < density).float()


def integers(*shape, seed, lo, hi):
    """fp32 tensor of integers drawn uniformly from [lo, hi]"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def choice(values, *shape, seed):
    """fp32 tensor drawn uniformly from the list `values`"""
    g = torch.Generator().manual_seed(seed)
    return torch.tensor(values, dtype=torch.float32)[torch.randint(0, len(values), shape, generator=g)]


# ---------------------------------------------------------------------------------------------------- conditions
def sum_bound(a, b=None):
    """upper bound of max_(m,n) sum_k |a[m,k]| |b[n,k]| (a, b: (rows, K)):  max_m sum_k |a| . max |b|, or the same with the roles swapped"""
    a = a.abs().double()
    if b is None:
        return float(a.flatten(1).sum(1).max())
    b = b.abs().double()
    return float(min(a.flatten(1).sum(1).max() * b.max(), b.flatten(1).sum(1).max() * a.max()))


def require_exact(bound, granule=1.0):
    """the condition that makes fp32 accumulation exact in any order: every partial sum is a multiple of `granule` below 2^24 granules"""
    assert bound / granule < LIMIT, f"partial sums up to {bound} in steps of {granule} are not guaranteed exact in fp32"


def bf16_share(ref):
    """share of the reference values that bf16 holds exactly"""
    r = ref.double()
    return float((r.float().to(torch.bfloat16).double() == r).double().mean())


def require_bf16_share(ref, least=0.95):
    s = bf16_share(ref)
    assert s >= least, f"only {s:.3f} of the reference values are exact in bf16: the output rounding could swallow a one-term error"


def require_random(*ts):
    """operands are random, not constant or symmetric, and pairwise different draws"""
    for t in ts:
        f = t.flatten().double()
        assert f.numel() < 2 or float(f.std()) > 0, "constant operand"
        if t.dim() == 2 and t.shape[0] == t.shape[1]:
            assert not torch.equal(t, t.t()), "symmetric operand"
    for i in range(len(ts)):
        for j in range(i + 1, len(ts)):
            if ts[i].shape == ts[j].shape:
                assert not torch.equal(ts[i], ts[j]), "two operands are the same draw"


# ---------------------------------------------------------------------------------------------------- the exact gate
def expected(ref64, dtype):
    """what the kernel must return for the exact fp64 reference: a plain cast, round to nearest even (csrc/common.h: f2bf)"""
    r = ref64.double().float()
    return r if dtype == torch.float32 else r.to(dtype)


def mismatch_report(out, want, tile=(256, 128), limit=6):
    """where two (rows, cols) results differ: count, row / column ranges, tile coordinates and lanes, the distinct differences (a difference
    equal to one product or one K slice names the culprit)"""
    o, w = out.double(), want.double()
    bad = (o != w) | (o.isnan() != w.isnan())
    if o.dim() != 2:
        return f"{int(bad.sum())} of {bad.numel()} elements differ; worst |diff| {float((o - w).abs().max())}"
    idx = bad.nonzero()
    rows, cols = idx[:, 0], idx[:, 1]
    diffs = (o - w)[bad]
    uniq = torch.unique(diffs)
    tiles = torch.unique(torch.stack((rows // tile[0], cols // tile[1]), 1), dim=0)
    return (f"{idx.shape[0]} of {bad.numel()} elements differ: rows {int(rows.min())}..{int(rows.max())} ({torch.unique(rows).numel()} distinct), "
            f"cols {int(cols.min())}..{int(cols.max())} ({torch.unique(cols).numel()} distinct); {tiles.shape[0]} tiles of {tile[0]} x {tile[1]}, first "
            f"{tiles[:limit].tolist()}; row % 16 in {torch.unique(rows % 16)[:16].tolist()}, col % 16 in {torch.unique(cols % 16)[:16].tolist()}; "
            f"first (row, col, got, want) {[(int(r), int(c), float(o[r, c]), float(w[r, c])) for r, c in idx[:limit].tolist()]}; "
            f"{uniq.numel()} distinct differences, first {uniq[:limit].tolist()}")


def is_exact(out, ref64):
    return torch.equal(out.detach().cpu(), expected(ref64, out.dtype))


def assert_exact(out, ref64, what="", sentinel=True):
    """bit-for-bit: torch.equal(out, cast(ref)).  No tolerance.  sentinel: the reference must stay far below the value output buffers are
    pre-filled with (a condition on the reference; switch it off for results that live in no sentinel-filled buffer and may be large)"""
    out = out.detach().cpu()
    want = expected(ref64, out.dtype)
    assert out.shape == want.shape, (what, out.shape, want.shape)
    assert not sentinel or float(ref64.abs().max()) < SENTINEL / 2, f"{what}: reference values come too close to the sentinel {SENTINEL}"
    if not torch.equal(out, want):
        o2, w2 = (out.reshape(-1, out.shape[-1]), want.reshape(-1, want.shape[-1])) if out.dim() >= 2 else (out, want)
        raise AssertionError(f"{what}: not bit-equal to the exact reference -- " + mismatch_report(o2, w2))


# ---------------------------------------------------------------------------------------------------- guarded output buffers
def guarded(M, N, dtype, device, fill=None):
    """(whole, view): a (M + GUARD_ROWS, N) buffer filled with the sentinel and its first M rows; fill (M, N): initial content of the
    view (an in-place residual).  An unwritten element keeps the sentinel, a write behind row M disturbs the guard band."""
    whole = torch.full((M + GUARD_ROWS, N), SENTINEL, dtype=dtype, device=device)
    view = whole[:M]
    if fill is not None:
        view.copy_(fill)
    return whole, view


def assert_guard(whole, M, what="", written=True):
    """the whole buffer: guard band untouched, and (written) no element of the result still holds the sentinel"""
    s = torch.tensor(SENTINEL).to(whole.dtype)
    g = whole[M:]
    assert bool((g == s.to(g.device)).all()), f"{what}: {int((g != s.to(g.device)).sum())} elements of the guard band behind row {M} were overwritten"
    if written:
        left = (whole[:M] == s.to(g.device))
        assert not bool(left.any()), f"{what}: {int(left.sum())} elements were never written (rows {torch.unique(left.nonzero()[:, 0])[:8].tolist()} ...)"


def check_rows(M):
    """rows compared against the fp64 reference.  All of them below 33000 rows; from there on (CPU cost of the fp64 product) every row of the
    first, one middle and the last 256-row block, the ragged rows behind the last full block, and every 97th row of the rest -- whole rows,
    all columns.  Sentinel / guard checks always cover the whole buffer."""
    if M < 33000:
        return None
    full = M // 256
    mid = (full // 2) * 256
    keep = torch.zeros(M, dtype=torch.bool)
    keep[:256] = True
    keep[mid:mid + 256] = True
    keep[(full - 1) * 256:] = True          # the last full block and the ragged rows behind it
    keep[::97] = True
    return keep.nonzero().flatten()


# ---------------------------------------------------------------------------------------------------- derived per-element bounds
def gelu64(s):
    s = s.double()
    return 0.5 * s * (1.0 + torch.erf(s / math.sqrt(2.0)))


def gelu_tanh64(s):
    s = s.double()
    return 0.5 * s * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (s + 0.044715 * s ** 3)))


def swiglu64(g, v):
    g, v = g.double(), v.double()
    return g * torch.sigmoid(g) * v


def act_excess(out, ref64, s64, u_out, e_act):
    """|out - act64(s)| - (u_out |act64(s)| + e_act max(1, |s|)) per element: <= 0 inside the bound"""
    return (out.double() - ref64).abs() - (u_out * ref64.abs() + e_act * s64.abs().clamp_min(1.0))


def assert_act(out, ref64, s64, e_act, what=""):
    out = out.detach().cpu()
    assert torch.isfinite(out.float()).all(), what
    u = U_BF16 if out.dtype == torch.bfloat16 else U_F32
    ex = act_excess(out, ref64, s64, u, e_act)
    bad = ex > 0
    if bool(bad.any()):
        i = int(ex.argmax())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the per-element bound; worst at flat index {i}: got "
                             f"{float(out.flatten()[i])}, want {float(ref64.flatten()[i])}, pre-activation {float(s64.flatten()[i])}, excess {float(ex.flatten()[i]):.3e}")


def measured_e_act(out, ref64, s64):
    """the figure E_ACT_* is derived from: worst |out - act64(s)| / max(1, |s|) (meaningful on fp32 results, where the output rounding is
    far below it, or on elements whose fp64 value the result format holds exactly)"""
    return float(((out.detach().cpu().double() - ref64).abs() / s64.abs().clamp_min(1.0)).max())


def attention_ref64(q, k, v, N):
    """fp64 softmax(q k^T) v for ONE head (q carries Dh^-0.5 log2 e: base-2 softmax), rows / keys 0..N-1, and the terms of the bound
        |out - ref| <= 2^-8 |ref| + (2^-8 + N 2^-24 + c_s) sum_k p_k |v_k|
    (output rounding; P rounded to bf16 before the PV product; fp32 accumulation of N terms; c_s: the rounding of the fp32 scores, which are
    in log2 units: a score error d changes a probability by the factor 2^d, d <= Dh 2^-24 max_k sum_d |q_d| |k_d| per query, and
    c_s = 2 ln 2 . d counts numerator and normaliser).  Returns (ref (N, Dh), bound (N, Dh))."""
    q, k, v = q[:N].double(), k[:N].double(), v[:N].double()
    Dh = q.shape[1]
    s = q @ k.t()
    p = torch.softmax(s * math.log(2.0), -1)
    ref = p @ v
    d = Dh * U_F32 * (q.abs() @ k.abs().t()).amax(1, keepdim=True)
    c_s = 2 * math.log(2.0) * d
    bound = U_BF16 * ref.abs() + (U_BF16 + N * U_F32 + c_s) * (p @ v.abs())
    return ref, bound


def conv3x3_ref64(x, w, bias, go=None):
    """fp64 3 x 3 / stride 1 / pad 1 convolution of an NHWC tensor as nine shifted matrix products (torch's fp64 conv2d takes minutes at
    8 x 512 x 512; a product per tap takes seconds): x (B, H, W, Cin), w (Cout, Cin, 3, 3), bias (Cout) or None -> y (B, H, W, Cout); with
    go (B, H, W, Cout) also the data gradient (B, H, W, Cin), the weight gradient (Cout, Cin, 3, 3) and the bias gradient (Cout).
    tests/test_cpu_exact.py holds it against conv2d's own autograd."""
    x, w = x.double(), w.double()
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
    y = torch.zeros(B, H, W, Cout, dtype=torch.float64) if bias is None else bias.double().expand(B, H, W, Cout).clone()
    for ky in range(3):
        for kx in range(3):
            y += xp[:, ky:ky + H, kx:kx + W] @ w[:, :, ky, kx].t()
    if go is None:
        return y
    go = go.double()
    gp = torch.nn.functional.pad(go, (0, 0, 1, 1, 1, 1))
    g2 = go.reshape(-1, Cout)
    gx = torch.zeros(B, H, W, Cin, dtype=torch.float64)
    gw = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            gx += gp[:, 2 - ky:2 - ky + H, 2 - kx:2 - kx + W] @ w[:, :, ky, kx]
            gw[:, :, ky, kx] = g2.t() @ xp[:, ky:ky + H, kx:kx + W].reshape(-1, Cin)
    return y, gx, gw, go.sum((0, 1, 2))


# ---------------------------------------------------------------------------------------------------- emulated kernels (CPU, plain torch)
def blocked_mm(a, b, bk=64, order=None):
    """a (M, K) @ b (N, K)^T with fp32 accumulation over K blocks of bk in `order` (a permutation of the blocks): what a tile kernel does"""
    a, b = a.float(), b.float()
    nb = (a.shape[1] + bk - 1) // bk
    acc = torch.zeros(a.shape[0], b.shape[0], dtype=torch.float32)
    for i in (order if order is not None else range(nb)):
        acc += a[:, i * bk:(i + 1) * bk] @ b[:, i * bk:(i + 1) * bk].t()
    return acc


def flash_attention_emulated(q, k, v, N, tile=32, drop_last_key=False, drop_last_tile=False):
    """ONE head of a flash-style kernel in plain torch: fp32 scores, running maximum over `tile`-key tiles, P rounded to bf16 before the
    PV product, fp32 accumulators, bf16 result.  The two mutants lose the last key / the last tile."""
    q, k, v = q[:N].float(), k[:N].float(), v[:N].float()
    nk = N - 1 if drop_last_key else N
    m = torch.full((N, 1), -float("inf"))
    l = torch.zeros(N, 1)
    acc = torch.zeros(N, q.shape[1])
    starts = list(range(0, nk, tile))
    if drop_last_tile:
        starts = starts[:-1]
    for t0 in starts:
        t1 = min(t0 + tile, nk)
        s = q @ k[t0:t1].t()
        mn = torch.maximum(m, s.amax(1, keepdim=True))
        p = torch.exp2(s - mn)
        c = torch.exp2(m - mn)
        l = l * c + p.sum(1, keepdim=True)
        acc = acc * c + p.to(torch.bfloat16).float() @ v[t0:t1]
        m = mn
    return (acc / l).to(torch.bfloat16)
