"""Keeps the references of tests/_small_ref.py honest without a GPU.  Every fp64 reference is either compared with torch's own op in fp32
on the CPU (max-pool, interpolate, squeeze-excitation, FiLM / FAPM, sample copy, cast), or a deliberately broken restatement of the kernel
is shown to FAIL the gate the GPU test uses (a pad value of 0 and the last maximum in max-pool, align_corners=True, an overwritten
squeeze-excitation chunk, d z_specific scaled by beta, a reversed or per-slab-rounded slab sum, a tanh-form GELU derivative).  Also asserts
the conditions the GPU tests rely on: bf16 shares, B > Bc, the bilinear bound for torch's own fp32, the over-the-clamp element counts."""
import math

import pytest
import torch
import torch.nn.functional as F

import _exact as X
import _small_ref as S

bf, f32 = S.bf, S.f32


def exact(out, ref64):
    try:
        X.assert_exact(out, ref64)
    except AssertionError:
        return False
    return True


# ---------------------------------------------------------------------------------------------------- max-pool
@pytest.mark.parametrize("draw", list(S.POOL_DRAWS))
@pytest.mark.parametrize("H,W", S.POOL_HW, ids=[f"{h}x{w}" for h, w in S.POOL_HW])
def test_maxpool_reference_is_the_first_maximum_in_scan_order(H, W, draw):
    """torch's fp64 forward / backward (the GPU test's reference) equal the brute-force loop with the kernel's documented tie rule, and
    torch's own fp32 and bf16 results are the same numbers"""
    x, dy = S.pool_inputs(3, H, W, 8, draw, seed=H * 31 + W)
    y, dx = S.pool_ref(x, dy)
    yb, dxb = S.pool_brute(x, dy)
    assert torch.equal(y, yb) and torch.equal(dx, dxb)
    for dt in (f32, bf):
        yt, dxt = S.pool_ref(x, dy, dt)
        assert torch.equal(yt.double(), y) and torch.equal(dxt.double(), dx), dt
    assert float(dx.abs().max()) <= 32 and X.bf16_share(dx) == 1.0
    if draw == "negative":
        assert bool((y < 0).all())


def test_maxpool_mutants_fail_the_gate():
    """a pad value of 0 shows on the negative draw (and not on the non-negative one: the gap the draw closes); the last maximum shows in
    the backward on ties"""
    x, dy = S.pool_inputs(3, 5, 4, 8, "negative", seed=3)
    y, dx = S.pool_ref(x, dy)
    y0, dx0 = S.pool_brute(x, dy, pad=0.0)
    assert not torch.equal(y0, y) and not bool((y0 < 0).all()) and not torch.equal(dx0, dx)
    x, dy = S.pool_inputs(3, 5, 4, 8, "ties", seed=4)
    y, dx = S.pool_ref(x, dy)
    y0, _ = S.pool_brute(x, dy, pad=0.0)
    assert torch.equal(y0, y)                                # invisible to non-negative inputs
    yl, dxl = S.pool_brute(x, dy, last=True)
    assert torch.equal(yl, y) and not torch.equal(dxl, dx)


# ---------------------------------------------------------------------------------------------------- bilinear
@pytest.mark.parametrize("geo", S.BL_EXACT, ids=S.bl_id)
def test_bilinear_exact_arm_conditions(geo):
    """dyadic ratios on integers: torch's own fp32 equals the fp64 reference bit for bit, >= 95 % of the reference is exact in bf16, and
    align_corners=True fails the exact gate (except at 1x, where the two conventions agree)"""
    (hs, ws), size = geo
    for dt in S.DTS:
        for Cc in (8, 12, 16, 40):
            src, base, dy = S.bl_exact_inputs(geo, Cc, dt)
            assert float(src.abs().max()) <= 8 and torch.equal(src, src.round()) and src.unique().numel() >= 5
            for b in (None, base):
                ref = S.bilinear_ref64(src, size, b)
                own = S.nhwc(F.interpolate(S.nchw(src), size=size, mode="bilinear", align_corners=False))
                assert exact(own if b is None else own + b, ref)
                if dt == bf:
                    X.require_bf16_share(ref, 0.95)
                assert exact(S.bilinear_ref64(src, size, b, align_corners=True).float().to(dt), ref) == ((hs, ws) == tuple(size))
            # the fp32 backward is exact too (16 dyadic terms at most); bf16 holds too few of these sums, so its backward is gated by the bound
            assert exact(S.bilinear_bwd_ref64(src.shape, dy, size, f32), S.bilinear_bwd_ref64(src.shape, dy, size))


@pytest.mark.parametrize("geo", S.BL_GENERAL, ids=S.bl_id)
def test_bilinear_bound_holds_for_torchs_own_fp32(geo):
    """the derived bound, for the reference alone: torch's fp32 forward and backward stay inside it (well inside: the worst share is
    printed), and align_corners=True is far outside wherever the two conventions differ"""
    (hs, ws), size = geo
    src = S.quant(torch.randn(2, hs, ws, 8, generator=torch.Generator().manual_seed(5)), f32)
    ref = S.bilinear_ref64(src, size)
    own = S.nhwc(F.interpolate(S.nchw(src), size=size, mode="bilinear", align_corners=False))
    ok, msg = S.within(own, ref, S.bilinear_bound(ref, hs, ws, src.abs().max(), f32), "forward")
    print(msg)
    assert ok, msg
    if (hs > 1 and hs != size[0]) or (ws > 1 and ws != size[1]):
        bad = S.bilinear_ref64(src, size, align_corners=True)
        for dt in (f32, bf):
            assert not S.within(bad.float().to(dt), ref, S.bilinear_bound(ref, hs, ws, src.abs().max(), dt))[0], dt
    dy = S.quant(torch.randn(2, *size, 8, generator=torch.Generator().manual_seed(6)), f32)
    gref = S.bilinear_bwd_ref64(src.shape, dy, size)
    ok, msg = S.within(S.bilinear_bwd_ref64(src.shape, dy, size, f32), gref, S.bilinear_bound(gref, hs, ws, dy.abs().max(), f32), "backward")
    print(msg)
    # the backward of a pixel sums (Ho / Hs)(Wo / Ws) weighted terms in fp32.  Up to 3x per axis torch's own fp32 stays inside the bound;
    # at (3, 5) -> (32, 29) (62 terms per pixel) it reaches 1.59 of it: printed, and not asserted for the reference
    assert ok or (size[0] > 3 * hs and size[1] > 3 * ws), msg


# ---------------------------------------------------------------------------------------------------- squeeze-excitation
@pytest.mark.parametrize("shape", S.SE_SHAPES, ids=S.se_id)
def test_se_reference_and_chunking(shape):
    """the fp64 reference against torch's own fp32 formula; the chunk list each shape is there for (B > Bc where it says so); the fp32
    restatement of the chunked gate backward passes the parameter-gradient gate and its overwrite mutant fails it"""
    from test_gpu_ops import TOL, rel
    B, H, W, Cc, R, _, chunks = shape
    assert S.se_chunks(B, Cc, R) == chunks
    if len(chunks) > 1:
        assert B > S.SE_LDS_FLOATS // (Cc + R)
    ins = S.se_inputs(B, H, W, Cc, R, f32)
    y, gr = S.se_ref(*ins)
    y32, gr32 = S.se_ref(*ins, dtype=f32)
    assert rel(y32, y) < TOL[f32]
    for a, b in zip(gr32, gr):
        assert rel(a, b) < 2 * TOL[f32]
    x, w1, b1, w2, b2, sc, go = ins
    Bc = S.SE_LDS_FLOATS // (Cc + R)
    good = S.se_gate_bwd_chunked(x, w1, b1, w2, b2, go, Bc)
    assert S.se_param_gate(good, gr[1:5], f32, TOL[f32]) == []
    if len(chunks) > 1:
        lost = S.se_gate_bwd_chunked(x, w1, b1, w2, b2, go, Bc, overwrite=True)
        for dt in (f32, bf):
            assert S.se_param_gate(lost, gr[1:5], dt, TOL[dt]) != [], dt


# ---------------------------------------------------------------------------------------------------- FiLM / FAPM
@pytest.mark.parametrize("dt", S.DTS, ids=["f32", "bf16"])
def test_film_reference_and_mutant(dt):
    """the closed-form FiLM reference against torch's autograd of gamma * z_specific + beta in fp32 (exact on these integers); every result
    is exact in bf16 too; d z_specific scaled by beta instead of gamma fails the exact gate"""
    for rows in S.FILM_ROWS:
        for R in S.FILM_R[dt]:
            gb, z2, dz = S.film_inputs(rows, R, seed=rows + R)
            z, dgb, dzs = S.film_ref64(gb, z2, dz)
            g, s = gb.clone().requires_grad_(True), z2.clone().requires_grad_(True)
            zt = g[:, :R] * s[:, R:] + g[:, R:]
            dg, ds = torch.autograd.grad(zt, (g, s), dz)
            assert exact(zt.detach(), z) and exact(dg, dgb) and exact(ds[:, R:], dzs) and not bool(ds[:, :R].any())
            for r in (z, dgb, dzs):
                X.require_bf16_share(r, 1.0)
                assert float(r.abs().max()) < X.SENTINEL / 2
            if rows * R >= 24:
                assert not exact(S.film_ref64(gb, z2, dz, wrong_scale=True)[2].to(dt), dzs)


@pytest.mark.parametrize("biases", [True, False], ids=["biases", "nobias"])
@pytest.mark.parametrize("shape", S.FAPM_SHAPES, ids=["x".join(map(str, s)) for s in S.FAPM_SHAPES])
def test_fapm_reference_matches_the_torch_module_form(shape, biases):
    """the fp64 matrix form against two 1 x 1 convolutions, a film generator and a chunk in fp32 (dinounet_training.py:423-429)"""
    from test_gpu_ops import TOL, rel
    B, H, W, D, R = shape
    x, ws, wp, bs, bp, wf, bfm, go = S.fapm_inputs(B, H, W, D, R, f32, biases)
    z, gr = S.fapm_ref64(x, ws, wp, bs, bp, wf, bfm, go)
    ins = [None if t is None else t.clone().requires_grad_(True) for t in (x, ws, wp, bs, bp, wf, bfm)]
    xr = S.nchw(ins[0])
    zsh, zsp = F.conv2d(xr, ins[1], ins[3]), F.conv2d(xr, ins[2], ins[4])
    gamma, beta = F.conv2d(zsh, ins[5], ins[6]).chunk(2, 1)
    zt = (gamma * zsp + beta).permute(0, 2, 3, 1)
    gt = iter(torch.autograd.grad(zt, [t for t in ins if t is not None], go))
    assert rel(zt, z) < TOL[f32]
    for t, want in zip(ins, gr):
        assert (t is None) == (want is None)
        if t is not None:
            assert rel(next(gt), want) < TOL[f32]


# ---------------------------------------------------------------------------------------------------- streaming helpers
def test_swiglu_inputs_are_exact_and_hold_the_large_gates():
    for dt in S.DTS:
        for rows, h in S.SWIGLU_SHAPES[dt]:
            u, g, v = S.swiglu_inputs(rows, h, seed=1)
            assert (2 * h) % S.VEC[dt] == 0 and torch.equal(u.to(dt).float(), u)
            assert torch.equal(u[:, 0::2], g) and torch.equal(u[:, 1::2], v)
            ref = X.swiglu64(g, v)
            assert bool(torch.isfinite(ref).all())
    u, g, v = S.swiglu_inputs(3, 20, seed=1)
    assert g.flatten()[:6].tolist() == S.SWIGLU_GATES
    # a gate that overflows to NaN (inf * 0, inf / inf) fails assert_act's finiteness check; the honest fp32 formula passes
    out = (g / (1 + torch.exp(-g)) * v)
    X.assert_act(out, X.swiglu64(g, v), g * v, X.E_ACT_SWIGLU)
    nan = (g * (1 / (1 + torch.exp(-g))) * torch.exp(g) / torch.exp(g) * v)
    with pytest.raises(AssertionError):
        X.assert_act(nan, X.swiglu64(g, v), g * v, X.E_ACT_SWIGLU)


def test_grid_clamps_are_exceeded_by_the_large_shapes():
    """the element counts quoted by the GPU tests, from the launchers' constants"""
    rows, h = S.SWIGLU_BIG
    for dt in S.DTS:
        assert rows * 2 * h // S.VEC[dt] > S.SWIGLU_BLOCKS * 256
        assert S.ACT_N_BIG % S.VEC[dt] == 0 and S.ACT_N_BIG // S.VEC[dt] > S.ACT_BLOCKS * 256
    assert rows * 2 * h // 8 == 2098176 and S.SWIGLU_BLOCKS * 256 == 2097152
    assert S.SAMPLE_N[1] % 4 == 0 and S.SAMPLE_N[1] // 4 == S.SAMPLE_BLOCKS * 256 + 1 == 131073
    assert S.ACT_N_BIG // 8 == S.ACT_BLOCKS * 256 + 1


def test_sample_copy_reference():
    x = torch.randn(5, 12, generator=torch.Generator().manual_seed(1))
    for idx in ([4, 0, 2], [3]):
        i = torch.tensor(idx)
        got = S.sample_copy_ref(x, i)
        assert torch.equal(got, torch.index_select(x, 0, i)) and all(torch.equal(got[j], x[k]) for j, k in enumerate(idx))
        src = torch.randn(len(idx), 12, generator=torch.Generator().manual_seed(2))
        y = S.sample_copy_ref(torch.full_like(x, X.SENTINEL), i, src)
        assert torch.equal(y, torch.full_like(x, X.SENTINEL).index_copy(0, i, src))
        assert all(bool((y[r] == X.SENTINEL).all()) for r in range(5) if r not in idx)


def test_splitk_reference_order_and_single_rounding_matter():
    """on the random draw the GPU test uses, a reversed slab order and a rounding per slab both differ from the reference; on the
    midpoint slabs ties go to even"""
    slabs = torch.randn(7, 65540, generator=torch.Generator().manual_seed(7))
    ref = S.splitk_ref(slabs)
    assert not torch.equal(S.splitk_ref(slabs, reverse=True), ref)
    assert not torch.equal(S.splitk_ref(slabs, round_each=True), ref)
    mid, want = S.splitk_midpoints()
    assert torch.equal(S.splitk_ref(mid).float(), want)
    assert torch.equal(S.splitk_ref(mid[:1]).float(), mid[0])


def test_cast_specials_are_what_they_claim():
    s = S.cast_specials()
    b = s.to(bf).float()
    assert b[:4].tolist() == [1.0, 1.0 + 2.0 ** -6, -1.0, -1.0 - 2.0 ** -6]                  # ties to even, both parities
    assert b[4] == 1.0 + 2.0 ** -7 and b[5] == 1.0                                          # just off the midpoint
    assert b[6] == 0 and b[7] == 2.0 ** -130 and b[8] == -2.0 ** -133 and b[9] in (2.0 ** -133, 2.0 ** -134)
    assert b[10] == math.inf and b[11] == -math.inf and b[12] == math.inf and b[13] == -math.inf
    assert b[14] == float(torch.finfo(bf).max) and math.copysign(1.0, float(b[16])) == -1.0 and bool(b[17].isnan())
    for n in S.CAST_N:
        for dt in S.DTS:
            t = S.cast_inputs(n, dt)
            assert t.numel() == n and t.dtype == dt and S.same_bits(t, t.clone())
    t = S.cast_inputs(1025, f32)
    assert bool(t.isnan().any()) and bool(t.isinf().any())
    assert not S.same_bits(torch.tensor([0.0]), torch.tensor([-0.0])) and not S.same_bits(torch.tensor([1.0]), torch.tensor([math.nan]))


def test_act_bwd_references_and_the_tanh_mutant():
    """gelu'64 against autograd of the fp64 erf form; ReLU / leaky against torch's own fp32 (to the bit); the tanh-form derivative is outside
    the GELU gate, an honest fp32 evaluation inside"""
    z, dy = S.act_inputs(2403, f32, seed=1)
    assert bool((z == 0).any()) and bool((torch.signbit(z) & (z == 0)).any())
    zz = z.double().clone().requires_grad_(True)
    auto = torch.autograd.grad(X.gelu64(zz).sum(), zz)[0]
    assert float((S.gelu_grad64(z) - auto).abs().max()) < 1e-14
    for kind, fn in (("relu", F.relu), ("leaky", lambda t: F.leaky_relu(t, 0.01))):
        zr = z.clone().requires_grad_(True)
        own = torch.autograd.grad(fn(zr), zr, dy)[0]
        assert exact(own, S.act_bwd_ref64(z, dy, kind))
    ref = S.act_bwd_ref64(z, dy, "gelu")
    zr = z.clone().requires_grad_(True)
    own = torch.autograd.grad(F.gelu(zr), zr, dy)[0]
    for dt in S.DTS:
        b = S.act_gelu_bound(ref, dy, dt)
        assert S.within(own.to(dt), ref, b)[0]
        assert not S.within(S.act_bwd_ref64(z, dy, "gelu_tanh").float().to(dt), ref, b)[0], dt
    assert S.act_gelu_excess(own, ref, dy, f32) < X.E_ACT_CAP
