"""The small NHWC kernels of csrc/elementwise.hip against exact and fp64 references (tests/_small_ref.py, kept honest by
tests/test_cpu_small_ops.py) at the edges where vector kernels go wrong: sizes that are no multiple of the 16-byte vector, pitches and
pointers that force the narrower launch form, more than one block, one element past a clamped grid, a batch that needs more than one
LDS chunk.

Instruments.  Exact inputs (small integers, dyadic weights): the result must equal the fp64 value bit for bit (tests/_exact.py).  Where
that is impossible a derived per-element bound (bilinear at general ratios, sigmoid / erf), or the gates of tests/test_gpu_ops.py (rel at
TOL) against fp64 for the ops built on GEMMs.  Every buffer a kernel writes directly through the C ABI is pre-filled with the sentinel and
followed by a guard band: every element must have been written and nothing behind the buffer touched.

Recorded for information, never a gate: the GELU-gradient excess printed by test_act_bwd_gelu_gate, worst (|dz - dy gelu'64(z)| -
u_out |ref|) / |dy|: fp32 7.3e-8 (vector and offset forms, 2400 elements), 8.4e-8 (2403 elements), 1.21e-7 (4 194 312 elements);
bf16 1.1e-8, 9.5e-9, 1.39e-8 -- three orders of magnitude inside the gate E_ACT_CAP = 2^-12 = 2.4e-4, which stays what it is."""
import pytest
import torch

import _exact as X
import _small_ref as S
from test_gpu_ops import TOL, dev, rel

pytestmark = pytest.mark.gpu

bf, f32 = S.bf, S.f32
DT_IDS = ["f32", "bf16"]


def L():
    from dinounet_amd import _lib
    return _lib.lib()


def call(name, *args):
    """a kernel through the C ABI on the current stream -> return code"""
    from dinounet_amd import ops
    return getattr(L(), name)(*args, ops._st())


def ok(name, *args):
    from dinounet_amd import _lib
    _lib.check(call(name, *args), name)


def P(t):
    from dinounet_amd import ops
    return ops._p(t)


def code(dt):
    from dinounet_amd import ops
    return ops._code(dt)


def flat_guarded(n, dt, d, lead=0):
    """(whole, view): a sentinel-filled flat buffer of lead + n + GUARD elements and its n elements behind the lead"""
    whole = torch.full((lead + n + X.GUARD_ROWS,), X.SENTINEL, dtype=dt, device=d)
    return whole, whole[lead:lead + n]


def assert_flat_guard(whole, n, lead=0, what="", written=True):
    s = torch.tensor(X.SENTINEL).to(whole.dtype).to(whole.device)
    assert bool((whole[:lead] == s).all()) and bool((whole[lead + n:] == s).all()), f"{what}: elements outside the buffer were overwritten"
    if written:
        left = whole[lead:lead + n] == s
        assert not bool(left.any()), f"{what}: {int(left.sum())} elements were never written (first {left.nonzero().flatten()[:8].tolist()})"


def untouched(whole):
    return bool((whole == torch.tensor(X.SENTINEL).to(whole.dtype).to(whole.device)).all())


# ---------------------------------------------------------------------------------------------------- 1. max-pool 3 x 3 / s2 / p1
@pytest.mark.parametrize("draw", list(S.POOL_DRAWS))
@pytest.mark.parametrize("dt", S.DTS, ids=DT_IDS)
@pytest.mark.parametrize("H,W", S.POOL_HW, ids=[f"{h}x{w}" for h, w in S.POOL_HW])
def test_maxpool_to_the_bit(H, W, dt, draw):
    """forward torch.equal to F.max_pool2d, backward torch.equal to torch's fp64 backward (first maximum in scan order), through
    ops.maxpool3x3s2 and through the C ABI into guarded buffers; on the negative draw every output is negative (the pad is -inf)"""
    from dinounet_amd import ops
    d = dev()
    Ho, Wo = S.pool_out(H, W)
    for B in S.POOL_B:
        for Cc in S.POOL_C[dt]:
            what = f"B {B} C {Cc}"
            x, dy = S.pool_inputs(B, H, W, Cc, draw, seed=H * 100 + W + B + Cc)
            yr, dxr = S.pool_ref(x, dy)
            xg, dyg = x.to(d, dt).requires_grad_(True), dy.to(d, dt)
            y = ops.maxpool3x3s2(xg)
            dx, = torch.autograd.grad(y, xg, dyg)
            assert torch.equal(y.detach().cpu().double(), yr), what
            assert torch.equal(dx.cpu().double(), dxr), what
            if draw == "negative":
                assert bool((y < 0).all()), what
            yw, yv = X.guarded(B * Ho * Wo, Cc, dt, d)
            dxw, dxv = X.guarded(B * H * W, Cc, dt, d)
            idx = torch.empty(B * Ho * Wo * Cc, dtype=torch.uint8, device=d)
            ok("du_maxpool3x3s2_fwd", code(dt), P(xg), P(yv), P(idx), B, H, W, Cc)
            ok("du_maxpool3x3s2_bwd", code(dt), P(idx), P(dyg), P(dxv), B, H, W, Cc)
            X.assert_guard(yw, B * Ho * Wo, what + " y")
            X.assert_guard(dxw, B * H * W, what + " dx")
            X.assert_exact(yv.view(B, Ho, Wo, Cc), yr, what + " y")
            X.assert_exact(dxv.view(B, H, W, Cc), dxr, what + " dx")


@pytest.mark.parametrize("dt", S.DTS, ids=DT_IDS)
def test_maxpool_refuses_a_ragged_channel_count(dt):
    d = dev()
    Cc = S.VEC[dt] + S.VEC[dt] // 2
    x = torch.zeros(1, 3, 3, Cc, dtype=dt, device=d)
    yw, yv = X.guarded(4, Cc, dt, d)
    dxw, dxv = X.guarded(9, Cc, dt, d)
    idx = torch.zeros(4 * Cc, dtype=torch.uint8, device=d)
    assert call("du_maxpool3x3s2_fwd", code(dt), P(x), P(yv), P(idx), 1, 3, 3, Cc) != 0
    assert call("du_maxpool3x3s2_bwd", code(dt), P(idx), P(yv), P(dxv), 1, 3, 3, Cc) != 0
    torch.cuda.synchronize()
    assert untouched(yw) and untouched(dxw)


# ---------------------------------------------------------------------------------------------------- 2. bilinear add / resize
def bl_direct(src, base, size, out_dt, Cc=None):
    """du_bilinear_add_fwd as ops calls it, into a guarded buffer -> (B, Ho, Wo, C) view"""
    from dinounet_amd import ops
    B, Hs, Ws, Cs, lds = ops._nhwc(src)
    Cc = Cc or Cs
    ldb = 0 if base is None else ops._nhwc(base)[4]
    n = B * size[0] * size[1]
    whole, view = X.guarded(n, Cc, out_dt, src.device)
    ok("du_bilinear_add_fwd", code(src.dtype), code(out_dt), P(src), lds, P(base), ldb, P(view), Cc, B, Hs, Ws, size[0], size[1], Cc)
    X.assert_guard(whole, n, "bilinear out")
    return view.view(B, size[0], size[1], Cc)


def sliced(t, lo, wide=40):
    """t as the channel slice [lo : lo + C] of a `wide`-channel tensor (pitch != C)"""
    w = torch.full(t.shape[:-1] + (wide,), 99.0, dtype=t.dtype, device=t.device)
    v = w[..., lo:lo + t.shape[-1]]
    v.copy_(t)
    return v


# (id, src dtype, out dtype, C, src slice offset, base slice offset): the launch form each one takes is in the id
BL_FORMS = [("bf16-C8-vec8", bf, bf, 8, None, None), ("bf16-C40-vec8", bf, bf, 40, None, None), ("bf16-C12-vec4-scalar-loads", bf, bf, 12, None, None),
            ("f32-C4-float4", f32, f32, 4, None, None), ("f32-C12-float4", f32, f32, 12, None, None),
            ("bf16-C16-src-slice8-vec8", bf, bf, 16, 8, None), ("bf16-C16-src-slice4-misaligned-vec4", bf, bf, 16, 4, None),
            ("f32-C16-src-slice8", f32, f32, 16, 8, None), ("f32-C16-src-slice4", f32, f32, 16, 4, None),
            ("bf16-C16-base-slice8-vec8", bf, bf, 16, None, 8), ("bf16-C16-base-slice4-vec4", bf, bf, 16, None, 4), ("f32-C16-base-slice4", f32, f32, 16, None, 4),
            ("f32src-bf16out-C8-vec8", f32, bf, 8, None, None), ("f32src-bf16out-C12-vec4", f32, bf, 12, None, None)]


@pytest.mark.parametrize("geo", S.BL_EXACT, ids=S.bl_id)
@pytest.mark.parametrize("form", BL_FORMS, ids=[f[0] for f in BL_FORMS])
def test_bilinear_exact_through_every_launch_form(form, geo):
    """dyadic ratios on integers: ops.bilinear_add and ops.bilinear_resize (where the form has no base) equal fp64 F.interpolate bit for
    bit on the 8-wide, 4-wide and scalar-load paths, with pitches != C, a source 8 bytes off 16-byte alignment, fp32 sources into bf16"""
    from dinounet_amd import ops
    _, sdt, odt, Cc, s_off, b_off = form
    d = dev()
    (hs, ws), size = geo
    src, base, dy = S.bl_exact_inputs(geo, Cc, odt)
    ref_add, ref = S.bilinear_ref64(src, size, base), S.bilinear_ref64(src, size)
    if odt == bf:
        X.require_bf16_share(ref_add, 0.95)
        X.require_bf16_share(ref, 0.95)
    sg, bg = src.to(d, sdt), base.to(d, odt)
    if s_off is not None:
        sg = sliced(sg, s_off)
        assert sg.stride(2) == 40 and (sg.data_ptr() % 16 == 0) == (s_off * sg.element_size() % 16 == 0)
    if b_off is not None:
        bg = sliced(bg, b_off)
    out = ops.bilinear_add(sg, bg)
    X.assert_exact(out, ref_add, "bilinear_add", sentinel=False)
    X.assert_exact(bl_direct(sg, bg, size, odt), ref_add, "du_bilinear_add_fwd")
    if b_off is None:
        X.assert_exact(bl_direct(sg, None, size, odt), ref, "du_bilinear_add_fwd without base")
        if sdt == odt:
            xg = sg.detach().requires_grad_(True)
            y = ops.bilinear_resize(xg, size)
            X.assert_exact(y, ref, "bilinear_resize", sentinel=False)
            if odt == f32:                  # at most 16 dyadic terms per pixel: the fp32 data gradient is exact too
                dx, = torch.autograd.grad(y, xg, dy.to(d, odt))
                X.assert_exact(dx, S.bilinear_bwd_ref64(src.shape, dy, size), "bilinear_resize backward", sentinel=False)


@pytest.mark.parametrize("dt", S.DTS, ids=DT_IDS)
@pytest.mark.parametrize("geo", S.BL_GENERAL, ids=S.bl_id)
def test_bilinear_general_ratios_within_the_derived_bound(geo, dt):
    """forward (add and resize), backward and the adjoint identity against fp64 F.interpolate on the quantised inputs:
    |out - ref| <= u_out |ref| + 2^-23 (Hs + Ws + 4) max|src| per element (max|dy| for the backward), at ratios from 1/11 to 11x"""
    from dinounet_amd import ops
    d = dev()
    (hs, ws), size = geo
    B, Cc = 2, 8
    g = lambda *s, seed: S.quant(torch.randn(*s, generator=torch.Generator().manual_seed(seed)), dt)
    src, base, dy = g(B, hs, ws, Cc, seed=5), g(B, *size, Cc, seed=6), g(B, *size, Cc, seed=7)
    ref, ref_add = S.bilinear_ref64(src, size), S.bilinear_ref64(src, size, base)
    amax = src.abs().max()
    xg = src.to(d, dt).requires_grad_(True)
    y = ops.bilinear_resize(xg, size)
    dx, = torch.autograd.grad(y, xg, dy.to(d, dt))
    fails = []
    for name, out, r in (("resize", y, ref), ("add", ops.bilinear_add(src.to(d, dt), base.to(d, dt)), ref_add), ("direct", bl_direct(src.to(d, dt), None, size, dt), ref)):
        good, msg = S.within(out, r, S.bilinear_bound(r, hs, ws, amax, dt), name)
        print(msg)
        if not good:
            fails.append(msg)
    gref = S.bilinear_bwd_ref64(src.shape, dy, size)
    gbound = S.bilinear_bound(gref, hs, ws, dy.abs().max(), dt)
    good, msg = S.within(dx, gref, gbound, "backward")
    print(msg)
    if not good:
        fails.append(msg)
    # <resize(x), g> = <x, resize_bwd(g)> in fp64 from the kernel's two outputs; tolerance: the two bounds summed over the elements
    lhs = float((y.detach().cpu().double() * dy.double()).sum())
    rhs = float((src.double() * dx.cpu().double()).sum())
    tol = float((S.bilinear_bound(ref, hs, ws, amax, dt) * dy.double().abs()).sum() + (gbound * src.double().abs()).sum())
    print(f"adjoint: {lhs:.9g} vs {rhs:.9g}, |diff| {abs(lhs - rhs):.3e}, tolerance {tol:.3e}")
    if not abs(lhs - rhs) <= tol:
        fails.append(f"adjoint identity: {lhs} vs {rhs}, tolerance {tol}")
    assert not fails, fails


def test_bilinear_add_asserts_that_source_and_base_agree():
    from dinounet_amd import ops
    d = dev()
    src, base = torch.zeros(2, 4, 4, 8, device=d), torch.zeros(2, 8, 8, 16, device=d)
    with pytest.raises(AssertionError):
        ops.bilinear_add(src, base)
    with pytest.raises(AssertionError):
        ops.bilinear_add(src, base[:1, ..., :8].contiguous())


# ---------------------------------------------------------------------------------------------------- 3. squeeze-excitation
@pytest.mark.parametrize("dt", S.DTS, ids=DT_IDS)
@pytest.mark.parametrize("shape", S.SE_SHAPES, ids=S.se_id)
def test_squeeze_excite_chunked_batches_vs_fp64(shape, dt):
    """forward and all six gradients against the torch formula in fp64, at batches the gate backward walks in two and three LDS chunks
    (the accumulate branch, the ragged last chunk), C > 256 (the strided loops of the gate forward), P = 1, R = 1, channel slices"""
    from dinounet_amd import ops
    d = dev()
    B, H, W, Cc, R, slc, chunks = shape
    assert S.se_chunks(B, Cc, R) == chunks
    if len(chunks) > 1:
        assert B > S.SE_LDS_FLOATS // (Cc + R)
    x, w1, b1, w2, b2, sc, go = S.se_inputs(B, H, W, Cc, R, dt)
    yr, gr = S.se_ref(x, w1, b1, w2, b2, sc, go)
    xg, scg = x.to(d, dt), sc.to(d, dt)
    if slc:
        xg, scg = sliced(xg, 8), sliced(scg, 16)
    ins = [t.detach().requires_grad_(True) for t in (xg, w1.to(d), b1.to(d), w2.to(d), b2.to(d), scg)]
    y = ops.squeeze_excite(*ins)
    got = torch.autograd.grad(y, ins, go.to(d, dt))
    tol = TOL[dt]
    fails = []
    e = rel(y, yr)
    print(f"y {e:.3e}")
    if not e < tol:
        fails.append(f"y: rel {e:.3e}")
    for name, a, b in zip(("dx", "dw1", "db1", "dw2", "db2", "dshortcut"), got, gr):
        e = rel(a.reshape(b.shape), b)
        print(f"{name} {e:.3e}")
        if not e < 2 * tol:
            fails.append(f"{name}: rel {e:.3e}")
    fails += S.se_param_gate([t.cpu() for t in got[1:5]], gr[1:5], dt, tol)
    assert not fails, fails


# ---------------------------------------------------------------------------------------------------- 4. FiLM and the FAPM projection
@pytest.mark.parametrize("dt", S.DTS, ids=DT_IDS)
@pytest.mark.parametrize("rows", S.FILM_ROWS)
def test_film_kernels_to_the_bit_and_left_half_untouched(rows, dt):
    """du_film_fwd / du_film_bwd on integers: z, dgamma, dbeta = dz and d z_specific equal fp64 bit for bit; the left half of dz2
    (columns [:R], filled by another kernel in the caller) still holds the sentinel after du_film_bwd"""
    d = dev()
    for R in S.FILM_R[dt]:
        what = f"rows {rows} R {R}"
        gb, z2, dz = S.film_inputs(rows, R, seed=rows + R)
        zr, dgbr, dzsr = S.film_ref64(gb, z2, dz)
        if dt == bf:
            for r in (zr, dgbr, dzsr):
                X.require_bf16_share(r)
        gbg, z2g, dzg = gb.to(d, dt), z2.to(d, dt), dz.to(d, dt)
        zw, zv = X.guarded(rows, R, dt, d)
        ok("du_film_fwd", code(dt), P(gbg), P(z2g), P(zv), rows, R)
        X.assert_guard(zw, rows, what + " z")
        X.assert_exact(zv, zr, what + " z")
        dgbw, dgbv = X.guarded(rows, 2 * R, dt, d)
        dz2w, dz2v = X.guarded(rows, 2 * R, dt, d)
        ok("du_film_bwd", code(dt), P(dzg), P(gbg), P(z2g), P(dgbv), P(dz2v), rows, R)
        X.assert_guard(dgbw, rows, what + " dgb")
        X.assert_guard(dz2w, rows, what + " dz2", written=False)
        X.assert_exact(dgbv, dgbr, what + " dgb")
        assert untouched(dz2v[:, :R]), f"{what}: du_film_bwd wrote into the z_shared half of dz2"
        assert not bool((dz2v[:, R:] == torch.tensor(X.SENTINEL).to(dt)).any()), f"{what}: elements of the z_specific half were never written"
        X.assert_exact(dz2v[:, R:], dzsr, what + " d z_specific")


@pytest.mark.parametrize("dt", S.DTS, ids=DT_IDS)
def test_film_refuses_a_ragged_width(dt):
    d = dev()
    R, rows = S.VEC[dt] // 2, 3
    gb, z2, dz = (t.to(d, dt) for t in S.film_inputs(rows, R, seed=1))
    zw, zv = X.guarded(rows, R, dt, d)
    dgbw, dgbv = X.guarded(rows, 2 * R, dt, d)
    dz2w, dz2v = X.guarded(rows, 2 * R, dt, d)
    assert call("du_film_fwd", code(dt), P(gb), P(z2), P(zv), rows, R) != 0
    assert call("du_film_bwd", code(dt), P(dz), P(gb), P(z2), P(dgbv), P(dz2v), rows, R) != 0
    torch.cuda.synchronize()
    assert untouched(zw) and untouched(dgbw) and untouched(dz2w)


@pytest.mark.parametrize("slc", [False, True], ids=["dense", "x-sliced"])
@pytest.mark.parametrize("biases", [True, False], ids=["biases", "nobias"])
@pytest.mark.parametrize("dt", S.DTS, ids=DT_IDS)
@pytest.mark.parametrize("shape", S.FAPM_SHAPES, ids=["x".join(map(str, s)) for s in S.FAPM_SHAPES])
def test_fapm_project_vs_fp64(shape, dt, biases, slc):
    """ops.fapm_project, forward and all seven gradients, against the fp64 formula of its docstring, on the immediate weight-gradient
    path: two steps around PACK.refresh() (the second reads the packed transposes where 2R % 64 == 0 in bf16), both compared"""
    from dinounet_amd import ops
    d = dev()
    B, H, W, D, R = shape
    x, ws, wp, bs, bp, wf, bfm, go = S.fapm_inputs(B, H, W, D, R, dt, biases)
    zr, gr = S.fapm_ref64(x, ws, wp, bs, bp, wf, bfm, go)
    par = [None if t is None else torch.nn.Parameter(t.to(d)) for t in (ws, wp, bs, bp, wf, bfm)]
    xg = sliced(x.to(d, dt), 8, wide=D + 16) if slc else x.to(d, dt)
    names = ("z", "dx", "dws", "dwp", "dbs", "dbp", "dwf", "dbf")

    def step():
        xi = xg.detach().requires_grad_(True)
        ops.TRACK_ROUTE, ops.ROUTES[:] = True, []
        try:
            z = ops.fapm_project(xi, *par)
            have = [xi] + [p for p in par if p is not None]
            g = iter(torch.autograd.grad(z, have, go.to(d, dt)))
        finally:
            ops.TRACK_ROUTE = False
        return [z.detach()] + [next(g)] + [None if p is None else next(g) for p in par], [(am, bm) for am, bm, _ in ops.ROUTES]

    enabled = ops.WGRAD.enabled
    ops.WGRAD.enabled = False                     # the immediate weight-gradient path
    try:
        ops.PACK.refresh()
        r0, routes0 = step()
        ops.PACK.refresh()
        r1, routes1 = step()
    finally:
        ops.WGRAD.enabled = enabled
    assert (ops.PLAIN_ROW, ops.PLAIN_COL) in routes0, routes0
    if dt == bf and (2 * R) % 64 == 0 and ops.PACK.enabled:
        assert (ops.PLAIN_ROW, ops.PLAIN_COL) not in routes1, routes1              # the packed-transpose route
    else:
        assert (ops.PLAIN_ROW, ops.PLAIN_COL) in routes1, routes1                  # mm_dgrad
    fails = []
    for k, res in enumerate((r0, r1)):
        for name, a, b in zip(names, res, [zr] + gr):
            assert (a is None) == (b is None), name
            if a is not None:
                e = rel(a.reshape(b.shape), b)
                print(f"step {k} {name} {e:.3e}")
                if not e < TOL[dt]:
                    fails.append(f"step {k} {name}: rel {e:.3e}")
    assert not fails, fails


# ---------------------------------------------------------------------------------------------------- 5. streaming helpers
def swiglu_run(u, rows, h, dt, d):
    whole, view = X.guarded(rows, h, dt, d)
    ok("du_swiglu_pairs", code(dt), P(u), P(view), rows, h)
    X.assert_guard(whole, rows, "swiglu out")
    return view


@pytest.mark.parametrize("dt", S.DTS, ids=DT_IDS)
def test_swiglu_pairs_small_shapes_and_overflowing_gates(dt):
    """exact pre-activations in 1/32 steps plus gates of +-30, +-90, +-120 (exp overflows fp32 from 88.7): finite, inside the derived bound"""
    d = dev()
    for rows, h in S.SWIGLU_SHAPES[dt]:
        u, g, v = S.swiglu_inputs(rows, h, seed=rows + h)
        out = swiglu_run(u.to(d, dt), rows, h, dt, d)
        X.assert_act(out, X.swiglu64(g, v), g * v, X.E_ACT_SWIGLU, f"({rows}, {h})")


@pytest.mark.parametrize("dt", S.DTS, ids=DT_IDS)
def test_swiglu_pairs_past_the_8192_block_clamp(dt):
    """(2049, 4096): 2 098 176 bf16 vectors against 8192 x 256 threads -- the grid-stride loop's second trip"""
    d = dev()
    rows, h = S.SWIGLU_BIG
    assert rows * 2 * h // S.VEC[dt] > S.SWIGLU_BLOCKS * 256
    u, g, v = S.swiglu_inputs(rows, h, seed=3)
    out = swiglu_run(u.to(d, dt), rows, h, dt, d)
    X.assert_act(out, X.swiglu64(g, v), g * v, X.E_ACT_SWIGLU, "past the clamp")


@pytest.mark.parametrize("dt", S.DTS, ids=DT_IDS)
def test_swiglu_pairs_refuses_a_ragged_width(dt):
    d = dev()
    h = S.VEC[dt] // 4
    u = torch.zeros(3, 2 * h, dtype=dt, device=d)
    whole, view = X.guarded(3, h, dt, d)
    assert call("du_swiglu_pairs", code(dt), P(u), P(view), 3, h) != 0
    torch.cuda.synchronize()
    assert untouched(whole)


def test_mm_swiglu_fp32_takes_the_pairs_kernel():
    """ops.mm_swiglu in fp32 (always product + du_swiglu_pairs) on exact pre-activations against fp64"""
    from dinounet_amd import ops
    d = dev()
    M, h, K = 5, 6, 16
    x = X.integers(M, K, seed=1, lo=-2, hi=2)
    w1, w2 = X.integers(h, K, seed=2, lo=-4, hi=4) / 32, X.integers(h, K, seed=3, lo=-4, hi=4) / 32
    b1, b2 = X.integers(h, seed=4, lo=-8, hi=8) / 32, X.integers(h, seed=5, lo=-8, hi=8) / 32
    g, v = x.double() @ w1.double().t() + b1.double(), x.double() @ w2.double().t() + b2.double()
    out = ops.mm_swiglu(x.to(d), ops.interleave_pairs(w1, w2).to(d), ops.interleave_pairs(b1, b2).to(d))
    X.assert_act(out, X.swiglu64(g, v), g * v, X.E_ACT_SWIGLU, "mm_swiglu fp32")


@pytest.mark.parametrize("n", S.SAMPLE_N, ids=["n4", "n524292-past-the-512-block-clamp"])
@pytest.mark.parametrize("idx", [[4, 0, 2], [3]], ids=["idx402", "idx3"])
def test_sample_gather_and_scatter(idx, n):
    """torch.equal with x[idx] and x[idx] = src; n = 524 292 is one float4 more than 512 blocks x 256; rows a scatter does not name keep
    their sentinel bit for bit"""
    from dinounet_amd import ops
    d = dev()
    B, k = 5, len(idx)
    assert n % 4 == 0 and (n == 4 or n // 4 > S.SAMPLE_BLOCKS * 256)
    x = torch.randn(B, n, generator=torch.Generator().manual_seed(1))
    src = torch.randn(k, n, generator=torch.Generator().manual_seed(2))
    ig = torch.tensor(idx, dtype=torch.int64, device=d)
    xg = x.to(d)
    assert torch.equal(ops.sample_gather(xg, ig).cpu(), S.sample_copy_ref(x, torch.tensor(idx)))
    whole, view = X.guarded(k, n, f32, d)
    ok("du_sample_copy", P(xg), P(view), P(ig), k, n, 0)
    X.assert_guard(whole, k, "gather")
    assert torch.equal(view.cpu(), x[idx])
    whole, view = X.guarded(B, n, f32, d)
    ops.sample_scatter_(view, src.to(d), ig)
    X.assert_guard(whole, B, "scatter", written=False)
    assert torch.equal(view.cpu(), S.sample_copy_ref(torch.full((B, n), X.SENTINEL), torch.tensor(idx), src))
    for r in range(B):
        assert (r in idx) or untouched(view[r]), r


def test_sample_copy_refuses_a_ragged_row():
    d = dev()
    x = torch.zeros(5, 6, device=d)
    whole, view = X.guarded(1, 6, f32, d)
    ig = torch.tensor([3], dtype=torch.int64, device=d)
    assert call("du_sample_copy", P(x), P(view), P(ig), 1, 6, 0) != 0
    assert call("du_sample_copy", P(x), P(view), P(ig), 1, 6, 1) != 0
    torch.cuda.synchronize()
    assert untouched(whole)


@pytest.mark.parametrize("n", S.SPLITK_N)
@pytest.mark.parametrize("splits", S.SPLITK_SPLITS)
def test_splitk_reduce_bf16_is_the_ordered_fp32_sum_rounded_once(splits, n):
    d = dev()
    slabs = torch.randn(splits, n, generator=torch.Generator().manual_seed(7))
    whole, view = flat_guarded(n, bf, d)
    sg = slabs.to(d)
    ok("du_splitk_reduce_bf16", P(sg), P(view), splits, n)
    assert_flat_guard(whole, n, what="splitk")
    assert torch.equal(view.cpu(), S.splitk_ref(slabs))


def test_splitk_reduce_bf16_ties_to_even():
    d = dev()
    mid, want = S.splitk_midpoints()
    whole, view = flat_guarded(4, bf, d)
    mg = mid.to(d)
    ok("du_splitk_reduce_bf16", P(mg), P(view), 2, 4)
    assert_flat_guard(whole, 4, what="splitk midpoints")
    assert torch.equal(view.cpu().float(), want) and torch.equal(view.cpu(), S.splitk_ref(mid))


@pytest.mark.parametrize("n", S.CAST_N)
@pytest.mark.parametrize("sdt,ddt", [(f32, bf), (bf, f32), (f32, f32), (bf, bf)], ids=["f32-bf16", "bf16-f32", "f32-f32", "bf16-bf16"])
def test_cast_equals_torch_to(sdt, ddt, n):
    """midpoints of both parities, subnormals, +-inf, overflow to inf, signed zeros bit for bit; a NaN stays a NaN"""
    from dinounet_amd import ops
    d = dev()
    x = S.cast_inputs(n, sdt)
    want = x.to(ddt)
    whole, view = flat_guarded(n, ddt, d)
    xg = x.to(d)
    ok("du_cast", code(sdt), code(ddt), P(xg), P(view), n)
    assert_flat_guard(whole, n, what="cast")
    assert S.same_bits(view, want), (view.cpu()[:18], want[:18])
    if sdt != ddt:
        assert S.same_bits(ops.cast(xg, ddt), want)


def act_run(z, dy, n, dt, d, act, lead=0):
    """du_act_bwd on tensors `lead` elements behind a 16-byte aligned base, into a guarded buffer"""
    zb, dyb = torch.zeros(lead + n, dtype=dt, device=d), torch.zeros(lead + n, dtype=dt, device=d)
    zb[lead:].copy_(z)
    dyb[lead:].copy_(dy)
    whole, view = flat_guarded(n, dt, d, lead)
    assert zb.data_ptr() % 16 == 0 and whole.data_ptr() % 16 == 0
    ok("du_act_bwd", code(dt), P(zb[lead:]), P(dyb[lead:]), P(view), n, act)
    assert_flat_guard(whole, n, lead, "act_bwd")
    return view


# (id, n, lead): the vector path, the scalar path by n, the scalar path by alignment, one vector past the 2048-block clamp
ACT_FORMS = [("vector", 2400, 0), ("scalar-n", 2403, 0), ("scalar-offset", 2400, 1), ("past-the-clamp", S.ACT_N_BIG, 0)]


@pytest.mark.parametrize("dt", S.DTS, ids=DT_IDS)
@pytest.mark.parametrize("form", ACT_FORMS, ids=[f[0] for f in ACT_FORMS])
def test_act_bwd_relu_and_leaky_to_the_bit(form, dt):
    from dinounet_amd._lib import ACT_LEAKY, ACT_RELU
    d = dev()
    _, n, lead = form
    z, dy = S.act_inputs(n, dt, seed=n)
    for kind, act in (("relu", ACT_RELU), ("leaky", ACT_LEAKY)):
        out = act_run(z, dy, n, dt, d, act, lead)
        X.assert_exact(out, S.act_bwd_ref64(z, dy, kind), f"{kind} {form[0]}")


@pytest.mark.parametrize("dt", S.DTS, ids=DT_IDS)
@pytest.mark.parametrize("form", ACT_FORMS, ids=[f[0] for f in ACT_FORMS])
def test_act_bwd_gelu_gate(form, dt):
    """|dz - dy gelu'64(z)| <= u_out |ref| + E_ACT_CAP |dy|; the measured excess is printed and is not the gate"""
    from dinounet_amd._lib import ACT_GELU
    d = dev()
    _, n, lead = form
    z, dy = S.act_inputs(n, dt, seed=n + 1)
    out = act_run(z, dy, n, dt, d, ACT_GELU, lead)
    ref = S.act_bwd_ref64(z, dy, "gelu")
    print(f"GELU-gradient excess ({form[0]}, {dt}): {S.act_gelu_excess(out, ref, dy, dt):.3e} (gate {X.E_ACT_CAP:.3e})")
    good, msg = S.within(out, ref, S.act_gelu_bound(ref, dy, dt), "gelu backward")
    assert good, msg
