"""Band-tiled depthwise 3 x 3 kernels (csrc/dwconv.hip) against the kernels they replace (csrc/elementwise.hip, du_set_option(19, 0)),
against fp64 and on exact inputs.  Shapes are the smallest at which a band kernel can go wrong: two bands that share a halo row, a grid
exactly one band high, a grid shorter than a band, level-to-level and image-to-image borders of the token pyramid, two channel slabs, a
channel count that is no whole number of slabs, a height that is no multiple of the band, a grid wider than one workgroup's 64 columns
(rows cut by a workgroup boundary: the edge threads of the fused GELU backward form the neighbour column themselves).

Bounds: y, z, dx bit-equal to the old kernels (same fma order and rounding points); dw / db of random inputs within 2e-5 of an fp64 sum
over the same x and the same bf16 dz (rel64 of tests/test_gpu_ops.py); everything bit-equal to fp64 on exact integer inputs; autograd
at test_dwconv_tokens_and_nhwc's tolerance."""
import pytest
import torch
import torch.nn.functional as F

import _exact as X
from test_gpu_ops import TOL, dev, gen, rel, rel64

pytestmark = pytest.mark.gpu

bf = torch.bfloat16
KEY = 19
# (B, H, W, C): H, W of ops.dwconv_tokens (grids 2H x 2W, H x W, H/2 x W/2)
PYRAMID = [(3, 8, 8, 64), (2, 8, 16, 128), (1, 16, 8, 72), (1, 2, 40, 8)]
NHWC = [(2, 12, 20, 32), (1, 3, 8, 8)]


class option:
    """du_set_option(19, value) for the body; the default (1) restored on exit"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        from dinounet_amd import _lib
        _lib.lib().du_set_option(KEY, self.value)

    def __exit__(self, *exc):
        from dinounet_amd import _lib
        _lib.lib().du_set_option(KEY, 1)
        return False


ROW, ROW4, BAND = 1, 2, 3                    # du_dwconv3x3_plan_describe, out[1]


def describe(dtype, B, H, W, Cc, pyramid, act, ld=None):
    """du_dwconv3x3_plan_describe of a call on dense tensors (or an NHWC tensor of pixel stride ld)"""
    import ctypes
    from dinounet_amd import _lib, ops
    ld = ld or Cc
    pix = 21 * (H * W // 4) if pyramid else H * W
    d = (ctypes.c_int64 * 7)()
    assert _lib.lib().du_dwconv3x3_plan_describe(ops._code(dtype), ld, pix * ld, B, H, W, Cc, pyramid, act, d, 7) == 7
    return list(d)


def band_ok(B, H, W, Cc, pyramid, dtype=bf):
    """1: the band family serves the call as this file makes it (the pyramid with GELU or without, one NHWC segment without activation)"""
    from dinounet_amd._lib import ACT_GELU, ACT_NONE
    ds = [describe(dtype, B, H, W, Cc, pyramid, act) for act in ((ACT_GELU, ACT_NONE) if pyramid else (ACT_NONE,))]
    assert len({(d[0], d[1] == BAND) for d in ds}) == 1, ds
    return int(ds[0][0] == 0 and ds[0][1] == BAND)


def grids(H, W):
    n = H * W // 4
    return ((0, 16 * n, 2 * H, 2 * W), (16 * n, 20 * n, H, W), (20 * n, 21 * n, H // 2, W // 2))


def to_images(t, pyramid, H, W):
    """(B, N, C) tokens or (B, H, W, C) -> list of (B, C, h, w) fp64 images on the CPU"""
    t = t.detach().double().cpu()
    if not pyramid:
        return [t.permute(0, 3, 1, 2)]
    B, N, Cc = t.shape
    return [t[:, lo:hi].transpose(1, 2).reshape(B, Cc, h, w) for (lo, hi, h, w) in grids(H, W)]


def from_images(imgs, pyramid):
    if not pyramid:
        return imgs[0].permute(0, 2, 3, 1).contiguous()
    return torch.cat([i.flatten(2).transpose(1, 2) for i in imgs], 1).contiguous()


def ref64(x, w, b, g, pyramid, H, W):
    """fp64 y (pre-activation), dx, dw, db of the depthwise convolution for the upstream gradient g of the PRE-activation"""
    Cc = w.shape[0]
    w64 = w.detach().double().cpu()
    b64 = None if b is None else b.detach().double().cpu()
    ys, dxs = [], []
    dw, db = torch.zeros(Cc, 3, 3, dtype=torch.float64), torch.zeros(Cc, dtype=torch.float64)
    for xi, gi in zip(to_images(x, pyramid, H, W), to_images(g, pyramid, H, W)):
        ys.append(F.conv2d(xi, w64, b64, 1, 1, groups=Cc))
        dxs.append(F.conv2d(gi, w64.flip(2, 3), None, 1, 1, groups=Cc))
        xp = F.pad(xi, (1, 1, 1, 1))
        h, ww = xi.shape[2:]
        for ky in range(3):
            for kx in range(3):
                dw[:, ky, kx] += (xp[:, :, ky:ky + h, kx:kx + ww] * gi).sum((0, 2, 3))
        db += gi.sum((0, 2, 3))
    return from_images(ys, pyramid), from_images(dxs, pyramid), dw.view(Cc, 1, 3, 3), db


def run(x, w, b, go, pyramid, H, W, act):
    """y, dx, dw, db through ops.dwconv_tokens / ops.dwconv3x3 on the path the option selects"""
    from dinounet_amd import ops
    xg, wg, bg = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = ops.dwconv_tokens(xg, wg, bg, H, W, act) if pyramid else ops.dwconv3x3(xg, wg, bg, act)
    dx, dw, db = torch.autograd.grad(y, (xg, wg, bg), go)
    return y.detach(), dx, dw, db


def forward_z(x, w, b, H, W, act, band):
    """the pre-activation copy of the pyramid forward, straight from the entry point (autograd keeps it to itself), under option(band):
    0 = the row kernels, 1 = the band kernels, >= 2 = bands of that many rows; the option is back at its default afterwards"""
    from dinounet_amd import _lib, ops
    B, N, Cc = x.shape
    y, z = torch.empty_like(x), torch.empty_like(x)
    with option(int(band)):
        assert band_ok(B, H, W, Cc, 1) == int(band != 0)
        _lib.check(_lib.lib().du_dwconv3x3_fwd(ops._code(x.dtype), ops._p(x), ops._p(w.float().view(Cc, 9).contiguous()), ops._p(b.float()), ops._p(y),
                                               ops._p(z), Cc, N * Cc, B, H, W, Cc, 1, act, ops._st()), "du_dwconv3x3_fwd")
    return y, z


def inputs(B, H, W, Cc, pyramid, seed):
    d = dev()
    shape = (B, 21 * (H * W // 4), Cc) if pyramid else (B, H, W, Cc)
    x = gen(*shape, seed=seed).to(d, bf)
    w = gen(Cc, 1, 3, 3, seed=seed + 1, scale=1 / 3).to(d)
    b = gen(Cc, seed=seed + 2).to(d)
    go = gen(*shape, seed=seed + 3).to(d, bf)
    return x, w, b, go


CASES = [(1, c) for c in PYRAMID] + [(0, c) for c in NHWC]
IDS = [("pyr" if p else "nhwc") + "-".join(map(str, c)) for p, c in CASES]


@pytest.mark.parametrize("pyramid,cfg", CASES, ids=IDS)
def test_band_equals_old_kernels_bitwise(pyramid, cfg):
    """(a) y, z, dx: the band path's bits are the old path's, with GELU (pyramid) and with no activation"""
    from dinounet_amd._lib import ACT_GELU, ACT_NONE
    B, H, W, Cc = cfg
    assert band_ok(B, H, W, Cc, pyramid) == 1
    x, w, b, go = inputs(B, H, W, Cc, pyramid, seed=10)
    for act in ((ACT_GELU, ACT_NONE) if pyramid else (ACT_NONE,)):
        with option(0):
            assert band_ok(B, H, W, Cc, pyramid) == 0
            y0, dx0, dw0, db0 = run(x, w, b, go, pyramid, H, W, act)
        z0 = forward_z(x, w, b, H, W, act, band=False)[1] if pyramid else None
        for rows in (1, 8):                     # the library's band height (4 rows at these sizes), and bands of 8 rows
            with option(rows):
                assert band_ok(B, H, W, Cc, pyramid) == 1
                y1, dx1, dw1, db1 = run(x, w, b, go, pyramid, H, W, act)
            yb, z1 = forward_z(x, w, b, H, W, act, band=rows) if pyramid else (y1, None)
            assert torch.equal(y0, y1), f"y differs (act {act}): {X.mismatch_report(y1.flatten(0, -2).cpu(), y0.flatten(0, -2).cpu())}"
            assert torch.equal(dx0, dx1), f"dx differs (act {act}): {X.mismatch_report(dx1.flatten(0, -2).cpu(), dx0.flatten(0, -2).cpu())}"
            if pyramid:
                assert torch.equal(yb, y1) and torch.equal(z0, z1), f"z differs (act {act})"
            # the two partitions of the same fp32 sums
            assert rel64(dw1, dw0.double()) < 2e-5 and rel64(db1, db0.double()) < 2e-5


@pytest.mark.parametrize("pyramid,cfg", CASES, ids=IDS)
def test_band_weight_gradient_vs_fp64(pyramid, cfg):
    """(b) dw, db of random inputs against an fp64 sum over the same x and the same bf16 dz (du_act_bwd's)"""
    from dinounet_amd import _lib, ops
    from dinounet_amd._lib import ACT_GELU, ACT_NONE
    B, H, W, Cc = cfg
    assert band_ok(B, H, W, Cc, pyramid) == 1
    x, w, b, go = inputs(B, H, W, Cc, pyramid, seed=20)
    act = ACT_GELU if pyramid else ACT_NONE
    _, dx, dw, db = run(x, w, b, go, pyramid, H, W, act)
    dz = go
    if act != ACT_NONE:
        z = forward_z(x, w, b, H, W, act, band=True)[1]
        dz = torch.empty_like(go)
        _lib.check(_lib.lib().du_act_bwd(ops._code(bf), ops._p(z), ops._p(go), ops._p(dz), go.numel(), act, ops._st()), "du_act_bwd")
    _, dxr, dwr, dbr = ref64(x, w, None, dz, pyramid, H, W)
    e_dw, e_db = rel64(dw, dwr.to(dw.device)), rel64(db, dbr.to(db.device))
    print(f"dw {e_dw:.3e} db {e_db:.3e}")
    assert e_dw < 2e-5 and e_db < 2e-5
    assert rel(dx, dxr) < TOL[bf]


@pytest.mark.parametrize("pyramid,cfg", CASES, ids=IDS)
def test_band_exact_inputs(pyramid, cfg):
    """(c) small integers, no activation: every fp32 sum is exact in any order, so y, dx, dw and db equal the fp64 reference bit for bit"""
    from dinounet_amd._lib import ACT_NONE
    B, H, W, Cc = cfg
    d = dev()
    assert band_ok(B, H, W, Cc, pyramid) == 1
    shape = (B, 21 * (H * W // 4), Cc) if pyramid else (B, H, W, Cc)
    x = X.integers(*shape, seed=30, lo=-3, hi=3)
    w = X.integers(Cc, 1, 3, 3, seed=31, lo=-2, hi=2)
    b = X.integers(Cc, seed=32, lo=-4, hi=4)
    go = X.integers(*shape, seed=33, lo=-3, hi=3)
    X.require_random(x, go)
    npix = x.numel() // Cc
    X.require_exact(9.0 * npix)                   # |x go| <= 9 per pixel: dw / db partial sums; y, dx stay below 9 * 6 + 4
    yr, dxr, dwr, dbr = ref64(x, w, b, go, pyramid, H, W)
    X.require_bf16_share(yr, least=1.0)
    X.require_bf16_share(dxr, least=1.0)
    y, dx, dw, db = run(x.to(d, bf), w.to(d), b.to(d), go.to(d, bf), pyramid, H, W, ACT_NONE)
    X.assert_exact(y, yr, "y")
    X.assert_exact(dx, dxr, "dx")
    X.assert_exact(dw, dwr, "dw", sentinel=False)
    X.assert_exact(db, dbr, "db", sentinel=False)


@pytest.mark.parametrize("pyramid,cfg", CASES, ids=IDS)
def test_band_autograd(pyramid, cfg):
    """(d) ops.dwconv_tokens (+ GELU) / ops.dwconv3x3 with gradients for x, w and b against F.conv2d(groups = C) (+ F.gelu)"""
    from dinounet_amd._lib import ACT_GELU, ACT_NONE
    B, H, W, Cc = cfg
    assert band_ok(B, H, W, Cc, pyramid) == 1
    x, w, b, go = inputs(B, H, W, Cc, pyramid, seed=40)
    xr = x.float().cpu().requires_grad_(True)
    wr, br = w.cpu().clone().requires_grad_(True), b.cpu().clone().requires_grad_(True)
    if pyramid:
        outs = [F.conv2d(xr[:, lo:hi].transpose(1, 2).reshape(B, Cc, h, ww), wr, br, 1, 1, groups=Cc).flatten(2).transpose(1, 2)
                for (lo, hi, h, ww) in grids(H, W)]
        yr = F.gelu(torch.cat(outs, 1))
    else:
        yr = F.conv2d(xr.permute(0, 3, 1, 2), wr, br, 1, 1, groups=Cc).permute(0, 2, 3, 1)
    gr = torch.autograd.grad(yr, (xr, wr, br), go.float().cpu())
    y, dx, dw, db = run(x, w, b, go, pyramid, H, W, ACT_GELU if pyramid else ACT_NONE)
    assert rel(y, yr) < TOL[bf]
    for a, r_ in zip((dx, dw, db), gr):
        assert rel(a, r_) < TOL[bf]


def test_band_declined_shapes():
    """(e) W = 6 (a 3-wide grid in the pyramid), an odd NHWC width, fp32: the query says 0 and the result is the old kernels'"""
    from dinounet_amd._lib import ACT_GELU, ACT_NONE
    B, H, W, Cc = 2, 8, 6, 64
    assert band_ok(B, H, W, Cc, 1) == 0 and band_ok(2, 9, 7, 32, 0) == 0
    assert band_ok(3, 8, 8, 64, 1, dtype=torch.float32) == 0
    assert band_ok(3, 8, 8, 60, 1) == 0
    x, w, b, go = inputs(B, H, W, Cc, 1, seed=50)
    res = run(x, w, b, go, 1, H, W, ACT_GELU)
    with option(0):
        old = run(x, w, b, go, 1, H, W, ACT_GELU)
    for a, o in zip(res, old):
        assert torch.equal(a, o)
    x, w, b, go = inputs(2, 9, 7, 32, 0, seed=51)
    res = run(x, w, b, go, 0, 9, 7, ACT_NONE)
    with option(0):
        old = run(x, w, b, go, 0, 9, 7, ACT_NONE)
    for a, o in zip(res[:2], old[:2]):
        assert torch.equal(a, o)
    yr, dxr, dwr, dbr = ref64(x, w, b, go, 0, 9, 7)
    assert rel(res[0], yr) < TOL[bf] and rel64(res[2], dwr.to(dev())) < 2e-5


@pytest.mark.parametrize("cfg", NHWC, ids=["-".join(map(str, c)) for c in NHWC])
def test_nhwc_with_gelu_stays_on_the_row_kernels(cfg):
    """(f) the one combination the band family declines for a band-shaped tensor: the plan says row kernels with a separate activation
    pass under either option, y and dx have the same bits under both, and the result is F.conv2d + F.gelu's"""
    from dinounet_amd._lib import ACT_GELU
    B, H, W, Cc = cfg
    assert band_ok(B, H, W, Cc, 0) == 1
    x, w, b, go = inputs(B, H, W, Cc, 0, seed=60)
    res = []
    for opt in (0, 1):
        with option(opt):
            assert describe(bf, B, H, W, Cc, 0, ACT_GELU)[:5] == [0, ROW, 0, 1, 1]
            res.append(run(x, w, b, go, 0, H, W, ACT_GELU))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    xr = x.float().cpu().requires_grad_(True)
    wr, br = w.cpu().clone().requires_grad_(True), b.cpu().clone().requires_grad_(True)
    yr = F.gelu(F.conv2d(xr.permute(0, 3, 1, 2), wr, br, 1, 1, groups=Cc).permute(0, 2, 3, 1))
    gr = torch.autograd.grad(yr, (xr, wr, br), go.float().cpu())
    y, dx, dw, db = res[1]
    assert rel(y, yr) < TOL[bf]
    for a, r_ in zip((dx, dw, db), gr):
        assert rel(a, r_) < TOL[bf]


# (dtype, B, H, W, C, pyramid, act, ld or None) -> what describe must say: {rc, forward kernel}
DECLINED = [
    ((bf, 2, 8, 6, 64, 1, 1, None), [0, ROW]),                   # a 3-wide grid in the pyramid
    ((bf, 2, 9, 7, 32, 0, 0, None), [0, ROW]),                   # an odd NHWC width
    ((torch.float32, 3, 8, 8, 64, 1, 1, None), [0, ROW]),        # fp32 (W % 8 == 0: the 4-pixel kernel is bf16 only)
    ((bf, 3, 8, 8, 60, 1, 1, None), [-1, 0]),                    # C % 8: neither family
    ((bf, 2, 12, 20, 32, 0, 0, 36), [-1, ROW]),                  # band-shaped, but pixels 72 bytes apart: the row family's DU_ERR_BAD_ARG
]


@pytest.mark.parametrize("call,want", DECLINED, ids=[f"{'pyr' if c[5] else 'nhwc'}-{'-'.join(map(str, c[1:5]))}-{str(c[0])[6:]}-ld{c[7]}" for c, _ in DECLINED])
def test_declined_calls_return_what_describe_says(call, want):
    """(g) describe reports the row family's decision, or its DU_ERR_BAD_ARG, and du_dwconv3x3_fwd / _bwd return that code; a refused call
    writes nothing"""
    from dinounet_amd import _lib, ops
    dt, B, H, W, Cc, pyramid, act, ld = call
    L, d = _lib.lib(), dev()
    desc = describe(dt, B, H, W, Cc, pyramid, act, ld)
    assert desc[:2] == want
    ld = ld or Cc
    pix = 21 * (H * W // 4) if pyramid else H * W
    bs = pix * ld
    x, go = gen(B, pix, ld, seed=70).to(d, dt), gen(B, pix, ld, seed=71).to(d, dt)
    w, b = gen(Cc, 9, seed=72, scale=1 / 3).to(d), gen(Cc, seed=73).to(d)
    y, z, dx, dz = (torch.full_like(x, 7.0) for _ in range(4))
    dw, db = torch.full((Cc, 9), 7.0, device=d), torch.full((Cc,), 7.0, device=d)
    geom = (ld, bs, B, H, W, Cc, pyramid, act)
    assert L.du_dwconv3x3_fwd(ops._code(dt), ops._p(x), ops._p(w), ops._p(b), ops._p(y), ops._p(z), *geom, ops._st()) == want[0]
    n = int(L.du_dwconv3x3_bwd_ws_elems(ops._code(dt), *geom))
    assert n == desc[6]
    ws = torch.empty(max(n, 1), dtype=torch.float32, device=d)
    assert L.du_dwconv3x3_bwd(ops._code(dt), ops._p(z), ops._p(go), ops._p(x), ops._p(w), ops._p(dx), ops._p(dw), ops._p(db), ops._p(dz), *geom,
                              ops._p(ws), n, ops._st()) == want[0]
    torch.cuda.synchronize()
    if want[0] != 0:
        assert all(bool((t == 7.0).all()) for t in (y, z, dx, dz, dw, db))
    else:
        assert not bool((y == 7.0).all()) and not bool((dx == 7.0).all()) and not bool((dw == 7.0).any())
