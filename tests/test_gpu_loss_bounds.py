"""The fused segmentation losses of csrc/loss.hip (plain Dice + CE, Dice + CE with an ignore label, Dice + BCE for regions, deep
supervision, the COUNTS twin of the validation step) and the per-voxel values of csrc/loss_topk.hip against the fp64 restatements of
tests/_loss_ref.py (kept honest by tests/test_cpu_loss_ref.py), through the C ABI: du_*_ws_elems, _sums, _finish and _bwd.

Instruments.  Exact draws (uniform and one-hot pixels): G, n_valid, I and P must come back bit for bit, CE / BCE to the bit where every
pixel is one-hot.  Derived bounds otherwise: per sum, per coefficient and per gradient element; the per-voxel NLL against 4 x the fp32
error of torch's own cross_entropy on the same draw.  Each stage is held against fp64 on its own inputs: the sums against the logits,
the finish kernel against the sums it was given, the backward pass against the closed form with the coefficients it was given.  ws, sums,
loss, coef and dlogits are pre-filled with the sentinel and followed by a guard band: every element a kernel owns must have been written
and nothing behind it touched.

Found by this module on the commit before it (one run on an MI355X against a library built from that commit's loss sources):
  * the plain kernel and its COUNTS twin (the same text) computed -log(max(p_t, 1e-38)).  On extreme_softmax_draw (targets 20 .. 200
    below the maximum) the CE sum came back 540.1255493164062 from both where fp64 gives 707.3856636282687: a target 88, 100, 128 or 200
    below the maximum contributed a saturated value near 87 instead of its gap.  Finite and deterministic, not inf.
  * every other softmax body computed (mx + log se) - xt, which rounds at the size of mx.  On offset_draw (2, 3, 100 x 100) seed 5 the
    per-voxel values of the top-k loss missed fp64 by 3.93e-6 / 3.86e-6 at c = +-64 and 6.11e-5 at c = +-1024 (2008, 263, 18703 and
    17896 of 20000 voxels outside the bound 3.39e-6), torch's fp32 cross_entropy by 8.48e-7 at every offset.
  * du_dice_ce_ws_elems accepted 9..16 classes, so ops.dice_ce_loss failed with a bare return code instead of its message.
Every softmax body now goes through softmax_nll of csrc/loss_common.h, (mx - xt) + log se: the CE sum of the extremes is
707.3856811523438, and the per-voxel values are 8.48e-7 from fp64 at every offset, the reference's own figure.

The premises of the exact draws (exp2(0) = 1, exp2 below -150 = 0, log2(1) = 0, exact reciprocals of powers of two) hold on gfx950:
every exact gate passes to the bit, up to 8 409 999 pixels.

Recorded for information, never a gate: the worst share of a bound taken on an MI355X, per family as (sums, gradient) over all tests of
a kind (seeds and shapes as in the tests; printed by every test with -s).  plain: instantiations (0.06, 0.40), quad edges (0.06, 0.41),
exact (0.06, 0.10), past the clamps (0.001, 0.05), gradients (0.04, 0.52), extremes (0.03, 0.38), offsets (0.02, 0.42).  masked: (0.05,
0.55), (0.07, 0.40), (0.06, 0.12), (0.01, 0.04), (0.04, 0.58), (0.03, 0.38), (0.06, 0.42).  regions without / with the ignore channel:
instantiations (0.10, 0.26) / (0.06, 0.30), quad edges (0.05, 0.24) / (0.05, 0.24), exact (0.04, 0.08) / (0.04, 0.06), past the clamps
- / (0.02, 0.05), gradients (0.07, 0.43) / (0.05, 0.39), extremes (0.02, 0.52) / (0.02, 0.52).  Per-voxel NLL: 8.48e-7 of the bound
3.39e-6 (0.25).  The 73 tests take 21 s."""
import ctypes as C

import pytest
import torch

import _exact as X
import _loss_ref as R
from test_gpu_ops import dev
from test_gpu_small_ops import L, P, assert_flat_guard, call, flat_guarded, ok, untouched

pytestmark = pytest.mark.gpu

f32 = torch.float32
BAD_ARG, UNSUPPORTED = -1, -2


def scalar(go, d):
    return None if go is None else torch.tensor([go], dtype=f32, device=d)


class Bufs:
    """sentinel-filled, guarded output buffers of one loss call"""

    def __init__(self, d, **sizes):
        self.n = sizes
        self.whole, self.view = {}, {}
        for k, (n, lead) in sizes.items():
            self.whole[k], self.view[k] = flat_guarded(n, f32, d, lead)

    def check(self, what, skip=()):
        for k, (n, lead) in self.n.items():
            if k not in skip:
                assert_flat_guard(self.whole[k], n, lead, f"{what} {k}")

    def untouched(self):
        return all(untouched(w) for w in self.whole.values())


def run_softmax(x, t, family, smooth=1e-5, gm=1.0, go=1.0, ignore=R.IGNORE, lead=0, val=False):
    """plain or masked Dice + CE through the C ABI on device tensors x (B, K, HW) and t (B, HW); lead: dlogits starts `lead` elements
    into its buffer (a misaligned pointer).  val: the sums from the COUNTS twin du_val_dice_ce[_masked]"""
    d = x.device
    B, K, HW = x.shape
    assert x.is_contiguous() and t.is_contiguous()
    pre = "du_dice_ce" if family == "plain" else "du_dice_ce_masked"
    n = int(getattr(L(), ("du_val_dice_ce" if family == "plain" else "du_val_dice_ce_masked") + "_ws_elems" if val else pre + "_ws_elems")(B, K, HW))
    NS = R.ns_of(family, K)
    if not val:
        assert n == R.ws_elems(family, B, K, HW)
    b = Bufs(d, ws=(n, 0), sums=(NS, 0), loss=(1, 0), coef=(2 * (K - 1) + (family != "plain"), 0), dl=(x.numel(), lead))
    v = b.view
    ig = () if family == "plain" else (ignore,)
    if val:
        counts = torch.zeros(3 * K, dtype=torch.int64, device=d)
        ok("du_val_dice_ce" if family == "plain" else "du_val_dice_ce_masked", P(x), P(t), P(v["sums"]), P(counts), None, B, K, HW, *ig, P(v["ws"]), n)
    else:
        ok(pre + "_sums", P(x), P(t), P(v["sums"]), B, K, HW, *ig, P(v["ws"]), n)
    if family == "plain":
        ok(pre + "_finish", P(v["sums"]), P(v["loss"]), P(v["coef"]), K, B * HW, smooth, gm)
    else:
        ok(pre + "_finish", P(v["sums"]), P(v["loss"]), P(v["coef"]), K, smooth, gm)
    ok(pre + "_bwd", P(x), P(t), P(v["coef"]), P(scalar(go, d)), P(v["dl"]), B, K, HW, *ig)
    torch.cuda.synchronize()
    b.check(f"{family} {tuple(x.shape)}")
    return R.SimpleNamespace(sums=v["sums"].cpu(), loss=v["loss"].cpu(), coef=v["coef"].cpu(), grad=v["dl"].cpu().view(B, K, HW))


def run_regions(x, tgt, u, smooth=1e-5, gm=1.0, go=1.0, lead=0):
    """Dice + BCE through the C ABI: x (B, R, HW), tgt (B, R + u, HW) uint8"""
    d = x.device
    B, Rn, HW = x.shape
    assert x.is_contiguous() and tgt.is_contiguous()
    n = int(L().du_dice_bce_ws_elems(B, Rn, HW))
    assert n == R.ws_elems("regions", B, Rn, HW)
    b = Bufs(d, ws=(n, 0), sums=(2 + 3 * Rn, 0), loss=(1, 0), coef=(2 * Rn + 1, 0), dl=(x.numel(), lead))
    v = b.view
    ok("du_dice_bce_sums", P(x), P(tgt), P(v["sums"]), B, Rn, HW, u, P(v["ws"]), n)
    ok("du_dice_bce_finish", P(v["sums"]), P(v["loss"]), P(v["coef"]), Rn, u, smooth, gm)
    ok("du_dice_bce_bwd", P(x), P(tgt), P(v["coef"]), P(scalar(go, d)), P(v["dl"]), B, Rn, HW, u)
    torch.cuda.synchronize()
    b.check(f"regions {tuple(x.shape)} u {u}")
    return R.SimpleNamespace(sums=v["sums"].cpu(), loss=v["loss"].cpu(), coef=v["coef"].cpu(), grad=v["dl"].cpu().view(B, Rn, HW))


def run_ds(mode, outs, t, H, W, weights, table=None, ignore=None, smooth=1e-5, gm=1.0, go=1.0):
    """deep supervision through the C ABI: outs = device (B, N, h, w) per scale (None where inactive), t (B, H W)"""
    d = t.device
    S = len(weights)
    first = next(o for o in outs if o is not None)
    assert t.is_contiguous() and all(o is None or o.is_contiguous() for o in outs)
    B, N = first.shape[:2]
    m = 1 if mode == "regions" else 0
    CD = N if m else N - 1
    shapes = [tuple(o.shape[-2:]) if o is not None else (1, 1) for o in outs]
    hs, wd = (C.c_int * S)(*[s[0] for s in shapes]), (C.c_int * S)(*[s[1] for s in shapes])
    wt = (C.c_float * S)(*weights)
    u, ig = (0, 0) if ignore is None else (1, int(ignore))
    n = int(L().du_ds_loss_ws_elems(m, B, N, H, W, S, hs, wd, wt))
    assert n == R.ds_table(B, shapes, weights, False)[1] * (2 + 3 * CD)
    sizes = dict(ws=(n, 0), sums=(S * (2 + 3 * CD), 0), loss=(1 + S, 0), coef=(S * (2 * CD + 1), 0))
    for s, o in enumerate(outs):
        if o is not None:
            sizes[f"dl{s}"] = (o.numel(), 0)
    b = Bufs(d, **sizes)
    v = b.view
    ptrs = (C.c_void_p * S)(*[None if o is None else o.data_ptr() for o in outs])
    dptrs = (C.c_void_p * S)(*[None if o is None else v[f"dl{s}"].data_ptr() for s, o in enumerate(outs)])
    tb = None if table is None else torch.tensor(table, dtype=torch.int64, device=d)
    ok("du_ds_loss_sums", m, ptrs, P(t), P(tb), P(v["sums"]), B, N, H, W, S, hs, wd, wt, u, ig, P(v["ws"]), n)
    ok("du_ds_loss_finish", m, P(v["sums"]), P(v["loss"]), P(v["coef"]), N, S, wt, u, smooth, gm)
    ok("du_ds_loss_bwd", m, ptrs, P(t), P(tb), P(v["coef"]), P(scalar(go, d)), dptrs, B, N, H, W, S, hs, wd, wt, u, ig)
    torch.cuda.synchronize()
    b.check(f"ds {mode} {shapes}")
    grads = [None if o is None else v[f"dl{s}"].cpu().view(B, N, -1) for s, o in enumerate(outs)]
    return R.SimpleNamespace(sums=v["sums"].cpu(), loss=v["loss"].cpu(), coef=v["coef"].cpu().view(S, -1), grads=grads)


def gate(run, ref_of, B, HW, N, family, smooth, gm, what, exact=None, npix=None, trip=None):
    """the three stages against fp64.  ref_of(coef) -> the restatement (coef None: its own coefficients).  exact: None (bounds) or
    whether CE is exact too.  trip: (lo, hi) pixel range of image B - 1 served by the backward pass's second trip, compared on its own"""
    ref = ref_of(None)
    sb = R.sums_bound(ref, B, HW)
    if exact is None:
        R.assert_within(run.sums, ref.sums, sb, what + " sums")
    else:
        R.exactness(ref.sums, N, family)
        X.assert_exact(run.sums[1:], ref.sums[1:], what + " n_valid / I / P / G", sentinel=False)
        if exact:
            X.assert_exact(run.sums[:1], ref.sums[:1], what + " CE", sentinel=False)
        else:
            R.assert_within(run.sums[:1], ref.sums[:1], sb[:1], what + " CE")
    l64, c64, lb, cb = R.finish_bound(run.sums, family, N, smooth, gm, npix=npix)
    R.assert_within(run.loss, l64.reshape(1), lb, what + " loss of the kernel's sums")
    R.assert_within(run.coef, c64, cb, what + " coef of the kernel's sums")
    rg = R.regrad(ref, run.coef)
    gb = R.grad_bound(rg)
    live = (rg.stats.m if family.startswith("regions") else rg.stats.valid)[:, None].expand(run.grad.shape)
    assert bool((run.grad[~live] == 0).all()), what + ": an ignored pixel has a non-zero gradient"
    if trip is not None:
        lo, hi = trip
        R.assert_within(run.grad[-1, :, lo:hi], rg.grad[-1, :, lo:hi], gb[-1, :, lo:hi], what + f" gradient of the second trip (image {B - 1}, pixels {lo}..{hi - 1})")
        R.assert_within(run.grad[-1, :, :lo], rg.grad[-1, :, :lo], gb[-1, :, :lo], what + " gradient before the second trip")
    R.assert_within(run.grad, rg.grad, gb, what + " gradient")
    shares = (R.share(run.sums, ref.sums, sb), R.share(run.grad, rg.grad, gb))
    print(f"[share] {what}: sums {shares[0]:.3f} grad {shares[1]:.3f}")
    return ref


def soft_gate(x, t, family, smooth=1e-5, gm=1.0, go=1.0, what="", **kw):
    d = dev()
    run = run_softmax(x.to(d), t.to(d), family, smooth, gm, go)
    B, K, HW = x.shape
    gof = 1.0 if go is None else go
    return gate(run, lambda cf: R.softmax_ref(x, t, family, R.IGNORE, smooth, gm, gof, coef=cf), B, HW, K, family, smooth, gm,
                f"{family} {what} {tuple(x.shape)}", npix=B * HW, **kw)


def region_gate(x, y, m, u, smooth=1e-5, gm=1.0, go=1.0, what="", **kw):
    d = dev()
    tgt = torch.cat((y, (~m)[:, None].to(torch.uint8)), 1).contiguous() if u else y.contiguous()
    run = run_regions(x.to(d), tgt.to(d), u, smooth, gm, go)
    B, Rn, HW = x.shape
    gof = 1.0 if go is None else go
    fam = "regions_ign" if u else "regions"
    return gate(run, lambda cf: R.sigmoid_ref(x, y, m, bool(u), smooth, gm, gof, coef=cf), B, HW, Rn, fam, smooth, gm,
                f"{fam} {what} {tuple(x.shape)}", **kw)


def ds_gate(mode, outs, t, H, W, weights, table=None, ignore=None, smooth=1e-5, gm=1.0, go=1.0, exact=None, what="", trip=None):
    d = dev()
    run = run_ds(mode, [None if o is None else o.to(d) for o in outs], t.to(d), H, W, weights, table, ignore, smooth, gm, go)
    S, B = len(weights), t.shape[0]
    N = next(o for o in outs if o is not None).shape[1]
    wf = tuple(C.c_float(w).value for w in weights)
    ref = R.ds_ref(outs, t, H, W, mode, wf, table, ignore, smooth, gm, go)
    CD = N if mode == "regions" else N - 1
    fam = ("regions_ign" if ignore is not None else "regions") if mode == "regions" else "masked"
    for s in range(S):
        if weights[s] == 0.0:
            continue
        got = torch.cat((run.sums[2 * s:2 * s + 2], run.sums[2 * S + 3 * CD * s:2 * S + 3 * CD * (s + 1)]))
        r = ref.refs[s]
        HW = outs[s].shape[-2] * outs[s].shape[-1]
        sb = R.sums_bound(r, B, HW)
        w_ = f"ds {mode} {what} scale {s}"
        if exact is None:
            R.assert_within(got, r.sums, sb, w_ + " sums")
        else:
            R.exactness(r.sums, N, fam)
            X.assert_exact(got[1:], r.sums[1:], w_ + " n_valid / I / P / G", sentinel=False)
            R.assert_within(got[:1], r.sums[:1], sb[:1], w_ + " CE / BCE")
    inactive = [s for s in range(S) if weights[s] == 0.0]
    for s in inactive:
        assert float(run.sums[2 * s:2 * s + 2].abs().sum()) == 0 and float(run.loss[1 + s]) == 0 and float(run.coef[s].abs().sum()) == 0
    l64, c64 = R.ds_finish64(run.sums, mode, N, S, wf, ignore is not None, smooth, gm)
    R.assert_within(run.coef, c64, 12 * R.U * c64.abs(), f"ds {mode} {what} coef")
    # per scale the bound of finish_bound; the total adds S products and S - 1 sums
    lb = sum(R.finish_bound(torch.cat((run.sums[2 * s:2 * s + 2], run.sums[2 * S + 3 * CD * s:2 * S + 3 * CD * (s + 1)])), fam, N, smooth, gm, wf[s])[2]
             for s in range(S) if weights[s] != 0.0)
    R.assert_within(run.loss[1:], l64[1:], lb, f"ds {mode} {what} scale losses")
    R.assert_within(run.loss[:1], l64[:1], lb + 2 * S * R.U * sum(abs(wf[s] * float(l64[1 + s])) for s in range(S)), f"ds {mode} {what} total")
    for s in range(S):
        if weights[s] == 0.0:
            continue
        r = R.regrad(ref.refs[s], run.coef[s])
        gb = R.grad_bound(r)
        w_ = f"ds {mode} {what} scale {s} gradient"
        if trip is not None and s == 0:
            lo, hi = trip
            R.assert_within(run.grads[0][-1, :, lo:hi], r.grad[-1, :, lo:hi], gb[-1, :, lo:hi], w_ + f" of the second trip (pixels {lo}..{hi - 1})")
        R.assert_within(run.grads[s], r.grad, gb, w_)
        live = (r.stats.m if mode == "regions" else r.stats.valid)[:, None].expand(run.grads[s].shape)
        assert bool((run.grads[s][~live] == 0).all()), w_ + ": an ignored pixel has a non-zero gradient"
    return ref


# ---------------------------------------------------------------------------------------------------- 1. every instantiation
@pytest.mark.parametrize("K", R.K_ALL)
def test_every_softmax_instantiation(K):
    """K = 2..8 of the plain, masked and deep-supervision softmax kernels at (2, K, 5, 7): HW = 35, quads straddle the image boundary"""
    B, H, W = R.INST_SHAPE
    x = R.general_draw(B, K, H * W, 100 + K)
    soft_gate(x, R.labels_draw(B, K, H * W, 200 + K), "plain", go=1.7, what="inst")
    t = R.labels_draw(B, K, H * W, 300 + K, ignore_frac=0.3)
    soft_gate(x, t, "masked", go=1.7, what="inst")
    outs = [x.view(B, K, H, W), R.general_draw(B, K, 6, 400 + K).view(B, K, 3, 2)]
    ds_gate("softmax", outs, t, H, W, (0.75, 0.25), ignore=R.IGNORE, go=1.7, what=f"inst K {K}")


@pytest.mark.parametrize("u", [0, 1])
@pytest.mark.parametrize("Rn", R.R_ALL)
def test_every_sigmoid_instantiation(Rn, u):
    B, H, W = R.INST_SHAPE
    x = R.general_draw(B, Rn, H * W, 500 + Rn)
    _, y = R.exact_sigmoid_draw(B, Rn, H * W, 600 + Rn)
    m = R.mask_draw(B, H * W, 700 + Rn, 0.3 if u else 0.0)
    region_gate(x, y, m, u, go=-0.5, what="inst")
    table = [(0b10 << r) | 0b1000000000 for r in range(Rn)]          # region r = labels {r + 1, 9}
    t = R.labels_draw(B, 10, H * W, 800 + Rn, ignore_frac=0.3 if u else 0.0)
    outs = [x.view(B, Rn, H, W), R.general_draw(B, Rn, 6, 900 + Rn).view(B, Rn, 3, 2)]
    ds_gate("regions", outs, t, H, W, (0.75, 0.25), table=table, ignore=R.IGNORE if u else None, go=-0.5, what=f"inst R {Rn} u {u}")


# ---------------------------------------------------------------------------------------------------- 2. quad edges
@pytest.mark.parametrize("HW", R.QUAD_HW)
def test_quad_edges(HW):
    """B = 3 images of 1..8 pixels: the last quad of an image is partial unless HW % 4 == 0"""
    B, K = 3, 3
    x = R.general_draw(B, K, HW, 1000 + HW)
    soft_gate(x, R.labels_draw(B, K, HW, 1100 + HW), "plain", what="edge")
    soft_gate(x, R.labels_draw(B, K, HW, 1200 + HW, ignore_frac=0.3), "masked", what="edge")
    _, y = R.exact_sigmoid_draw(B, K, HW, 1300 + HW)
    for u in (0, 1):
        region_gate(x, y, R.mask_draw(B, HW, 1400 + HW, 0.3 * u), u, what="edge")


def offset_copy(t, lead):
    """t as a contiguous view `lead` elements into a larger flat buffer: the same values behind a misaligned pointer"""
    flat = torch.zeros(t.numel() + 16, dtype=t.dtype, device=t.device)
    v = flat[lead:lead + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def test_misaligned_pointers_take_the_scalar_path_with_the_same_bits():
    """HW % 4 == 0 and one pointer off its boundary: vec is false for pointer reasons alone, and every result equals the aligned call's"""
    d = dev()
    B, K, HW = 3, 4, 8 * 12
    x = R.general_draw(B, K, HW, 1500).to(d)
    t = R.labels_draw(B, K, HW, 1501, ignore_frac=0.3).to(d)
    a = run_softmax(x, t, "masked", go=1.7)
    for name, r in (("logits + 1 element", run_softmax(offset_copy(x, 1), t, "masked", go=1.7)),
                    ("target + 1 element", run_softmax(x, offset_copy(t, 1), "masked", go=1.7)),
                    ("dlogits + 1 element", run_softmax(x, t, "masked", go=1.7, lead=1))):
        assert torch.equal(a.sums, r.sums) and torch.equal(a.loss, r.loss) and torch.equal(a.coef, r.coef) and torch.equal(a.grad, r.grad), name
    _, y = R.exact_sigmoid_draw(B, K, HW, 1502)
    m = R.mask_draw(B, HW, 1503, 0.3)
    tgt = torch.cat((y, (~m)[:, None].to(torch.uint8)), 1).contiguous().to(d)
    a = run_regions(x, tgt, 1, go=1.7)
    for name, r in (("logits + 1 element", run_regions(offset_copy(x, 1), tgt, 1, go=1.7)),
                    ("target + 1 byte", run_regions(x, offset_copy(tgt, 1), 1, go=1.7)),
                    ("dlogits + 1 element", run_regions(x, tgt, 1, go=1.7, lead=1))):
        assert torch.equal(a.sums, r.sums) and torch.equal(a.loss, r.loss) and torch.equal(a.coef, r.coef) and torch.equal(a.grad, r.grad), name
    # deep supervision: the full-resolution scale misaligned, the lower one aligned
    H, W = 8, 12
    outs = [x.view(B, K, H, W), R.general_draw(B, K, 24, 1504).view(B, K, 4, 6).to(d)]
    a = run_ds("softmax", outs, t, H, W, (0.75, 0.25), ignore=R.IGNORE)
    r = run_ds("softmax", [offset_copy(outs[0], 1), outs[1]], t, H, W, (0.75, 0.25), ignore=R.IGNORE)
    assert torch.equal(a.sums, r.sums) and torch.equal(a.loss, r.loss) and all(torch.equal(p, q) for p, q in zip(a.grads, r.grads))


# ---------------------------------------------------------------------------------------------------- 3. exact sums
@pytest.mark.parametrize("K", R.EXACT_K)
def test_exact_sums_softmax(K):
    """G, n_valid, I and P to the bit (a class with no pixel included), CE to the bit on one-hot draws, at ignore fractions 0, 0.3, 1"""
    B, H, W = R.EXACT_SHAPE
    HW = H * W
    empty = K - 1 if K > 2 else None
    for onehot in (False, True):
        x = R.exact_softmax_draw(B, K, HW, 2000 + K, onehot)
        soft_gate(x, R.labels_draw(B, K, HW, 2100 + K, empty=empty), "plain", exact=onehot, what=f"exact onehot {onehot}")
        for frac in R.IGNORE_FRACS:
            t = R.labels_draw(B, K, HW, 2200 + K, empty=empty, ignore_frac=frac)
            soft_gate(x, t, "masked", exact=onehot, what=f"exact onehot {onehot} ignore {frac}")


@pytest.mark.parametrize("Rn", R.EXACT_R)
def test_exact_sums_regions(Rn):
    B, H, W = R.EXACT_SHAPE
    HW = H * W
    for onehot in (False, True):
        x, y = R.exact_sigmoid_draw(B, Rn, HW, 2300 + Rn, onehot)
        y[:, Rn - 1] = 0                                   # a region with no pixel
        region_gate(x, y, R.mask_draw(B, HW, 0, 0.0), 0, exact=onehot, what=f"exact onehot {onehot}")
        for frac in R.IGNORE_FRACS:
            region_gate(x, y, R.mask_draw(B, HW, 2400 + Rn, frac), 1, exact=onehot, what=f"exact onehot {onehot} ignore {frac}")


@pytest.mark.parametrize("mode", ["softmax", "regions"])
def test_exact_sums_deep_supervision(mode):
    """three scales with a non-dyadic zoom, 18 x 10 -> 9 x 5 -> 5 x 3, and a fourth, inactive one"""
    B, (H, W) = 2, R.DS_EXACT[0]
    N = 4 if mode == "softmax" else 2
    shapes = list(R.DS_EXACT) + [(2, 2)]
    weights = (4 / 7, 2 / 7, 1 / 7, 0.0)
    for frac in R.IGNORE_FRACS:
        t = R.labels_draw(B, 4, H * W, 2500, ignore_frac=frac)
        if mode == "softmax":
            outs = [R.exact_softmax_draw(B, N, h * w, 2501 + i).view(B, N, h, w) for i, (h, w) in enumerate(shapes)]
        else:
            outs = [R.exact_sigmoid_draw(B, N, h * w, 2501 + i)[0].view(B, N, h, w) for i, (h, w) in enumerate(shapes)]
        outs[3] = None
        ds_gate(mode, outs, t, H, W, weights, table=[0b0110, 0b0100], ignore=R.IGNORE, exact=False, what=f"exact ignore {frac}")


# ---------------------------------------------------------------------------------------------------- 4. past the launch clamps
def second_trip_pixels(family, B, HW):
    """pixel range of the LAST image that the backward pass serves in its second grid-stride trip"""
    lo, hi = R.second_trip_range(family, B, HW)
    assert hi > lo
    if family == "plain":
        return lo - (B - 1) * HW, HW
    nq = R.cdiv(HW, 4)
    assert lo >= (B - 1) * nq
    return 4 * (lo - (B - 1) * nq), HW


def test_past_the_clamps_plain():
    B, H, W = R.PLAIN_BIG
    HW = H * W
    assert R.past_clamp("plain", B, HW, False) and R.past_clamp("plain", B, HW, True)
    x = R.exact_softmax_draw(B, 2, HW, 3000)
    soft_gate(x, R.labels_draw(B, 2, HW, 3001), "plain", exact=False, what="big", trip=second_trip_pixels("plain", B, HW))


@pytest.mark.parametrize("shape", [R.QUAD_BIG_VEC, R.QUAD_BIG_ODD], ids=["vec", "odd"])
@pytest.mark.parametrize("family", ["masked", "regions"])
def test_past_the_clamps_quads(family, shape):
    B, H, W = shape
    HW = H * W
    assert R.past_clamp(family, B, HW, False) and R.trips(family, B, HW, True) == 2
    trip = second_trip_pixels(family, B, HW)
    if family == "masked":
        x = R.exact_softmax_draw(B, 2, HW, 3100)
        soft_gate(x, R.labels_draw(B, 2, HW, 3101, ignore_frac=0.3), "masked", exact=False, what="big", trip=trip)
    else:
        x, y = R.exact_sigmoid_draw(B, 1, HW, 3200)
        region_gate(x, y, R.mask_draw(B, HW, 3201, 0.3), 1, exact=False, what="big", trip=trip)


@pytest.mark.parametrize("mode,shape", [("softmax", R.QUAD_BIG_VEC), ("regions", R.QUAD_BIG_ODD)], ids=["softmax-vec", "regions-odd"])
def test_past_the_clamps_deep_supervision(mode, shape):
    """one full-resolution scale past the cap plus one small scale whose blocks sit behind 8192 (backward) / 2048 (sums) blocks"""
    B, H, W = shape
    h, w = R.DS_BIG_SMALL
    tab, _ = R.ds_table(B, [(H, W), (h, w)], (0.5, 0.5), True)
    assert tab[1][0] == 8192
    t = R.labels_draw(B, 2, H * W, 3300, ignore_frac=0.3)
    if mode == "softmax":
        outs = [R.exact_softmax_draw(B, 2, H * W, 3301).view(B, 2, H, W), R.exact_softmax_draw(B, 2, h * w, 3302).view(B, 2, h, w)]
    else:
        outs = [R.exact_sigmoid_draw(B, 1, H * W, 3301)[0].view(B, 1, H, W), R.exact_sigmoid_draw(B, 1, h * w, 3302)[0].view(B, 1, h, w)]
    ds_gate(mode, outs, t, H, W, (0.5, 0.5), table=[0b10], ignore=R.IGNORE, exact=False, what="big", trip=second_trip_pixels("masked", B, H * W))


# ---------------------------------------------------------------------------------------------------- 5. per-element gradients
@pytest.mark.parametrize("go,smooth,gm", R.GO_SMOOTH_MULT, ids=["go1.7", "go-0.5-s1-m2", "go0-s0", "goNULL-m2"])
@pytest.mark.parametrize("shape", R.GRAD_SHAPES, ids=[str(s) for s in R.GRAD_SHAPES])
def test_per_element_gradients(shape, go, smooth, gm):
    B, N, H, W = shape
    HW = H * W
    x = R.general_draw(B, N, HW, 4000 + N)
    soft_gate(x, R.labels_draw(B, N, HW, 4100 + N), "plain", smooth, gm, go, what="grad")
    t = R.labels_draw(B, N, HW, 4200 + N, ignore_frac=0.3)
    soft_gate(x, t, "masked", smooth, gm, go, what="grad")
    _, y = R.exact_sigmoid_draw(B, N, HW, 4300 + N)
    for u in (0, 1):
        region_gate(x, y, R.mask_draw(B, HW, 4400 + N, 0.3 * u), u, smooth, gm, go, what="grad")
    outs = [x.view(B, N, H, W), R.general_draw(B, N, (H // 2) * (W // 3), 4500 + N).view(B, N, H // 2, W // 3)]
    ds_gate("softmax", outs, t, H, W, (2 / 3, 1 / 3), ignore=R.IGNORE, smooth=smooth, gm=gm, go=1.0 if go is None else go, what="grad")


# ---------------------------------------------------------------------------------------------------- 6. finish kernels on synthetic sums
def finish_call(family, sums, N, smooth, gm, npix=64):
    d = dev()
    C_ = N if family.startswith("regions") else N - 1
    b = Bufs(d, loss=(1, 0), coef=(2 * C_ + (family != "plain"), 0))
    s = sums.float().to(d)
    if family == "plain":
        ok("du_dice_ce_finish", P(s), P(b.view["loss"]), P(b.view["coef"]), N, npix, smooth, gm)
    elif family == "masked":
        ok("du_dice_ce_masked_finish", P(s), P(b.view["loss"]), P(b.view["coef"]), N, smooth, gm)
    else:
        ok("du_dice_bce_finish", P(s), P(b.view["loss"]), P(b.view["coef"]), N, int(family == "regions_ign"), smooth, gm)
    torch.cuda.synchronize()
    b.check("finish " + family)
    return b.view["loss"].cpu(), b.view["coef"].cpu()


@pytest.mark.parametrize("family", ["plain", "masked", "regions", "regions_ign"])
def test_finish_on_synthetic_sums(family):
    N = 3
    C_ = N if family.startswith("regions") else N - 1
    head = [96.5] if family == "plain" else [96.5, 48.0]
    ipg = [[12.25, 20.5, 16.0], [0.0, 3.75, 0.0], [7.5, 9.0, 8.0]][:C_]
    sums = torch.tensor(head + [v for row in ipg for v in row], dtype=torch.float64)
    for smooth, gm in ((1e-5, 1.0), (1.0, 2.0), (0.0, 1.0)):
        loss, coef = finish_call(family, sums, N, smooth, gm)
        l64, c64, lb, cb = R.finish_bound(sums, family, N, smooth, gm, npix=64)
        R.assert_within(loss, l64.reshape(1), lb, f"{family} loss smooth {smooth} mult {gm}")
        R.assert_within(coef, c64, cb, f"{family} coef smooth {smooth} mult {gm}")
    # the Dice slice all-reduced over two ranks (doubled), CE / BCE and n_valid local
    off = 1 if family == "plain" else 2
    s2 = sums.clone()
    s2[off:] *= 2
    loss, coef = finish_call(family, s2, N, 1e-5, 2.0)
    l64, c64, lb, cb = R.finish_bound(s2, family, N, 1e-5, 2.0, npix=64)
    R.assert_within(loss, l64.reshape(1), lb, family + " all-reduced loss")
    R.assert_within(coef, c64, cb, family + " all-reduced coef")
    if family != "plain":
        # everything ignored, smooth = 0: raw <= 1e-8, so cb == 0, the Dice term is 0, the scale 0 and the loss exactly 0
        z = torch.zeros_like(sums)
        loss, coef = finish_call(family, z, N, 0.0, 1.0)
        assert float(loss[0]) == 0.0 and float(coef[-1]) == 0.0 and bool((coef[1::2][:C_] == 0).all()), (loss, coef)
        assert bool(torch.isfinite(coef).all())


@pytest.mark.parametrize("mode", ["softmax", "regions"])
def test_ds_finish_on_synthetic_sums(mode):
    d = dev()
    N, S = 3, 3
    CD = N if mode == "regions" else N - 1
    weights = (0.5, 0.0, 0.25)
    wt = (C.c_float * S)(*weights)
    head = [96.5, 48.0, 0.0, 0.0, 20.25, 12.0]
    tail = ([12.25, 20.5, 16.0, 0.0, 3.75, 0.0, 7.5, 9.0, 8.0][:3 * CD] + [0.0] * (3 * CD) + [3.5, 6.25, 4.0, 1.0, 2.5, 3.0, 0.5, 0.75, 1.0][:3 * CD])
    sums = torch.tensor(head + tail, dtype=torch.float64)
    for smooth, gm in ((1e-5, 1.0), (1.0, 2.0)):
        b = Bufs(d, loss=(1 + S, 0), coef=(S * (2 * CD + 1), 0))
        ok("du_ds_loss_finish", int(mode == "regions"), P(sums.float().to(d)), P(b.view["loss"]), P(b.view["coef"]), N, S, wt, 1, smooth, gm)
        torch.cuda.synchronize()
        b.check("ds finish")
        loss, coef = b.view["loss"].cpu(), b.view["coef"].cpu().view(S, -1)
        l64, c64 = R.ds_finish64(sums, mode, N, S, weights, True, smooth, gm)
        R.assert_within(coef, c64, 12 * R.U * c64.abs(), "ds coef")
        R.assert_within(loss, l64, 32 * R.U * (l64.abs() + 1), "ds loss")
        assert float(loss[2]) == 0.0 and float(coef[1].abs().sum()) == 0.0            # the inactive scale
        # the total is the sum of w_s loss_s in scale order, formed from the kernel's own per-scale losses
        want = torch.tensor(0.0, dtype=f32)
        for s in range(S):
            if weights[s] != 0.0:
                want = want + torch.tensor(weights[s], dtype=f32) * loss[1 + s]
        assert abs(float(loss[0]) - float(want)) <= 2 * R.U * abs(float(want))


# ---------------------------------------------------------------------------------------------------- 7. extremes
@pytest.mark.parametrize("val", [False, True], ids=["train", "counts-twin"])
def test_extremes_plain(val):
    """targets 20 .. 200 below the maximum, and maxima as far above a wrong class: finite, within the per-sum and per-element bounds.
    The COUNTS twin (du_val_dice_ce) is the same text and must give the same bits"""
    d = dev()
    x, t = R.extreme_softmax_draw()
    run = run_softmax(x.to(d), t.to(d), "plain", val=val)
    print(f"[extremes] plain val {val}: CE sum {float(run.sums[0])!r} (fp64 {float(R.softmax_ref(x, t).sums[0])!r})")
    gate(run, lambda cf: R.softmax_ref(x, t, "plain", coef=cf), 1, x.shape[2], 3, "plain", 1e-5, 1.0, f"plain extremes val {val}", npix=x.shape[2])
    if val:
        assert torch.equal(run.sums, run_softmax(x.to(d), t.to(d), "plain").sums)


def test_extremes_masked_regions_and_deep_supervision():
    x, t = R.extreme_softmax_draw()
    soft_gate(x, t, "masked", what="extremes")
    HW = x.shape[2]
    ds_gate("softmax", [x.view(1, 3, 2, HW // 2)], t, 2, HW // 2, (1.0,), what="extremes")
    xs, ys = R.extreme_sigmoid_draw()
    m = torch.ones(1, xs.shape[2], dtype=torch.bool)
    for u in (0, 1):
        region_gate(xs, ys, m, u, what="extremes")


# ---------------------------------------------------------------------------------------------------- 8. offsets
@pytest.mark.parametrize("c", R.OFFSETS[1:])
def test_offsets(c):
    """logits + c against the offset-free fp64 reference: sums and gradients of the softmax families, and the per-voxel values and the
    selection map of the top-k loss"""
    from dinounet_amd import ops, training
    d = dev()
    B, K, H, W = R.OFFSET_SHAPE
    HW = H * W
    xc, x = R.offset_draw(B, K, HW, 5, c)
    t = R.labels_draw(B, K, HW, 6)
    for family in ("plain", "masked"):
        tt = t if family == "plain" else R.labels_draw(B, K, HW, 7, ignore_frac=0.3)
        run = run_softmax(xc.to(d), tt.to(d), family)
        gate(run, lambda cf: R.softmax_ref(x, tt, family, R.IGNORE, coef=cf), B, HW, K, family, 1e-5, 1.0, f"{family} offset {c}", npix=B * HW)
    ref = R.softmax_ref(x, t)
    bound = R.nll_bound(xc, t)
    _, values, sel, _ = ops.topk_ce_loss(xc.view(B, K, H, W).to(d), t.view(B, 1, H, W).to(d), 10, return_aux=True)
    values, sel = values.cpu(), sel.cpu().bool().reshape(-1)
    print(f"[offset {c}] per-voxel NLL: worst |values - fp64| {float((values.double() - ref.nll).abs().max()):.3e}, bound {bound:.3e}")
    R.assert_within(values, ref.nll, bound, f"top-k values at offset {c}")
    k_vox = training.topk_voxels(B * HW, 10)
    want, decided = R.topk_separated(ref.nll, k_vox, bound)
    assert int(sel.sum()) == k_vox
    assert 1 - float(decided.double().mean()) < 0.01
    assert torch.equal(sel[decided], want[decided]), f"offset {c}: {int((sel[decided] != want[decided]).sum())} decided voxels selected differently"


# ---------------------------------------------------------------------------------------------------- 9. refusals
def test_refusals_touch_nothing():
    d = dev()
    B, HW = 2, 35
    x = torch.zeros(B, 9, HW, device=d)
    t = torch.zeros(B, HW, dtype=torch.int64, device=d)
    tg = torch.zeros(B, 10, HW, dtype=torch.uint8, device=d)
    b = Bufs(d, ws=(4096, 0), sums=(64, 0), loss=(1, 0), coef=(32, 0), dl=(x.numel(), 0))
    v = b.view
    # one element short
    n = int(L().du_dice_ce_ws_elems(B, 3, HW))
    assert call("du_dice_ce_sums", P(x), P(t), P(v["sums"]), B, 3, HW, P(v["ws"]), n - 1) == BAD_ARG
    n = int(L().du_dice_ce_masked_ws_elems(B, 3, HW))
    assert call("du_dice_ce_masked_sums", P(x), P(t), P(v["sums"]), B, 3, HW, R.IGNORE, P(v["ws"]), n - 1) == BAD_ARG
    n = int(L().du_dice_bce_ws_elems(B, 3, HW))
    assert call("du_dice_bce_sums", P(x), P(tg), P(v["sums"]), B, 3, HW, 1, P(v["ws"]), n - 1) == BAD_ARG
    hs, wd, wt = (C.c_int * 1)(5), (C.c_int * 1)(7), (C.c_float * 1)(1.0)
    ptrs = (C.c_void_p * 1)(x.data_ptr())
    n = int(L().du_ds_loss_ws_elems(0, B, 3, 5, 7, 1, hs, wd, wt))
    assert n > 0 and call("du_ds_loss_sums", 0, ptrs, P(t), None, P(v["sums"]), B, 3, 5, 7, 1, hs, wd, wt, 0, 0, P(v["ws"]), n - 1) == BAD_ARG
    # class / region counts outside the instantiated range: the documented codes, scratch size 0
    for K, rc in ((1, BAD_ARG), (9, UNSUPPORTED)):
        assert int(L().du_dice_ce_ws_elems(B, K, HW)) == 0
        assert call("du_dice_ce_sums", P(x), P(t), P(v["sums"]), B, K, HW, P(v["ws"]), 4096) == rc
        assert call("du_dice_ce_bwd", P(x), P(t), P(v["coef"]), None, P(v["dl"]), B, K, HW) == rc
    for K in (1, 9):
        assert int(L().du_dice_ce_masked_ws_elems(B, K, HW)) == 0 and int(L().du_val_dice_ce_ws_elems(B, K, HW)) == 0
        assert call("du_dice_ce_masked_sums", P(x), P(t), P(v["sums"]), B, K, HW, R.IGNORE, P(v["ws"]), 4096) == UNSUPPORTED
        assert call("du_dice_ce_masked_finish", P(v["sums"]), P(v["loss"]), P(v["coef"]), K, 1e-5, 1.0) == UNSUPPORTED
        assert call("du_dice_ce_masked_bwd", P(x), P(t), P(v["coef"]), None, P(v["dl"]), B, K, HW, R.IGNORE) == UNSUPPORTED
        assert int(L().du_ds_loss_ws_elems(0, B, K, 5, 7, 1, hs, wd, wt)) == 0
        assert call("du_ds_loss_sums", 0, ptrs, P(t), None, P(v["sums"]), B, K, 5, 7, 1, hs, wd, wt, 0, 0, P(v["ws"]), 4096) == UNSUPPORTED
    for Rn in (0, 9):
        assert int(L().du_dice_bce_ws_elems(B, Rn, HW)) == 0
        assert call("du_dice_bce_sums", P(x), P(tg), P(v["sums"]), B, Rn, HW, 1, P(v["ws"]), 4096) == UNSUPPORTED
        assert call("du_dice_bce_finish", P(v["sums"]), P(v["loss"]), P(v["coef"]), Rn, 1, 1e-5, 1.0) == UNSUPPORTED
        assert call("du_dice_bce_bwd", P(x), P(tg), P(v["coef"]), None, P(v["dl"]), B, Rn, HW, 1) == UNSUPPORTED
        assert int(L().du_ds_loss_ws_elems(1, B, Rn, 5, 7, 1, hs, wd, wt)) == 0
    torch.cuda.synchronize()
    assert b.untouched()


def test_nine_classes_raise_the_wrappers_message():
    from dinounet_amd import ops
    d = dev()
    with pytest.raises(RuntimeError, match=r"supports 2\.\.8 classes, got 9"):
        ops.dice_ce_loss(torch.zeros(1, 9, 4, 4, device=d), torch.zeros(1, 1, 4, 4, dtype=torch.int64, device=d))
