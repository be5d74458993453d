"""GPU suite of the fused option losses (csrc/loss_opt.hip; training.build_loss weight_ce, weight_dice, batch_dice, do_bg,
ce_class_weights) against the fp64 oracle of tests/_loss_opt_ref.py, stage by stage through the C ABI into guarded buffers (sums, finish,
backward) and through the public modules.

Bounds: _loss_opt_ref.sums_bound / finish_bound / grad_bound = the error model of tests/_loss_ref.py (unit roundoff times the reduction
depth of the shape, the per-term errors of the native exp / log / rcp) with the factors the options add; every element is held to its own
bound, there is no share-of-elements allowance and no fitted constant.  Exact cases (integer logits, one-hot probabilities, power-of-two
class weights) are held to the bit.

Shapes: B = 3 with HW in (1, 2, 3, 4, 5, 7, 8) (partial quads, unaligned rows), (2, 5, 7), (3, 19, 21), and _loss_opt_ref.BIG =
(2048, 65, 65): with 2048 images the launch caps leave one sums block (5 grid-stride trips over the image's 1057 quads) and four backward
blocks (2 trips) per image."""
import ctypes as C

import pytest
import torch

import _exact as X
import _loss_opt_ref as O
import _loss_ref as R
from test_gpu_ops import dev
from test_gpu_small_ops import L, P, assert_flat_guard, flat_guarded, ok

pytestmark = pytest.mark.gpu
f32 = torch.float32
IGN = R.IGNORE


def scalar(go, d):
    return None if go is None else torch.tensor([go], dtype=f32, device=d)


def run_opt(x, t, *, regions=False, ignore=None, has_ignore=False, weight_ce=1.0, weight_dice=1.0, batch_dice=True, do_bg=None, class_w=None,
            smooth=1e-5, grad_mult=1.0, go=1.0):
    """the three stages through the C ABI on device tensors x (B, N, HW), t (B, HW) int64 or (B, R + u, HW) uint8, guarded buffers"""
    from dinounet_amd import _lib
    d = x.device
    B, N, HW = x.shape
    assert x.is_contiguous() and t.is_contiguous()
    if do_bg is None:
        do_bg = regions
    CD = O.cd_of(N, regions, do_bg)
    rows = 1 if batch_dice else B
    cw = None if class_w is None else torch.tensor(class_w, dtype=f32, device=d)
    u = int(has_ignore) if regions else int(ignore is not None)
    o = _lib.LossOpt(N, int(regions), u, 0 if ignore is None else ignore, int(do_bg), int(batch_dice), weight_ce, weight_dice,
                     None if cw is None else cw.data_ptr())
    ref = C.byref(o)
    n = int(L().du_loss_opt_ws_elems(ref, B, HW))
    assert n == O.ws_elems(B, N, HW, regions, do_bg)
    sizes = dict(ws=n, sums=rows * (2 + 3 * CD), loss=1, coef=rows * 2 * CD + 1, dl=x.numel())
    whole, v = {}, {}
    for k, sz in sizes.items():
        whole[k], v[k] = flat_guarded(sz, f32, d)
    ok("du_loss_opt_sums", ref, P(x), P(t), P(v["sums"]), B, HW, P(v["ws"]), n)
    ok("du_loss_opt_finish", ref, P(v["sums"]), P(v["loss"]), P(v["coef"]), B, smooth, grad_mult)
    ok("du_loss_opt_bwd", ref, P(x), P(t), P(v["coef"]), P(scalar(go, d)), P(v["dl"]), B, HW)
    torch.cuda.synchronize()
    for k, sz in sizes.items():
        assert_flat_guard(whole[k], sz, 0, f"opt {tuple(x.shape)} {k}")
    return R.SimpleNamespace(sums=v["sums"].cpu().view(rows, -1), loss=v["loss"].cpu(), coef=v["coef"].cpu(), grad=v["dl"].cpu().view(B, N, HW))


def gate(x, t, what="", exact=None, **kw):
    """sums, finish and backward of one call against fp64; x, t on the CPU.  exact: None (bounds), False (CE column inside its bound, every
    other column to the bit) or True (every column to the bit)"""
    d = dev()
    run = run_opt(x.to(d), t.to(d), **kw)
    okw = dict(kw)
    okw["go"] = 1.0 if kw.get("go", 1.0) is None else kw.get("go", 1.0)
    ref = O.opt_ref(x, t, **okw)
    sb = O.sums_bound(ref)
    what = f"{what} {tuple(x.shape)} {kw}"
    if exact is None:
        R.assert_within(run.sums, ref.sums, sb, what + " sums")
    else:
        X.assert_exact(run.sums[:, 1:], ref.sums[:, 1:], what + " sum w_t / n_valid, I, P, G", sentinel=False)
        if exact:
            X.assert_exact(run.sums[:, :1], ref.sums[:, :1], what + " CE", sentinel=False)
        else:
            R.assert_within(run.sums[:, :1], ref.sums[:, :1], sb[:, :1], what + " CE")
    regions = kw.get("regions", False)
    per_elem = regions and not kw.get("has_ignore", False)
    l64, c64, lb, cb = O.finish_bound(run.sums, ref.CD, per_elem, kw.get("weight_ce", 1.0), kw.get("weight_dice", 1.0), kw.get("smooth", 1e-5),
                                      kw.get("grad_mult", 1.0))
    R.assert_within(run.loss, l64.reshape(1), lb, what + " loss of the kernel's sums")
    R.assert_within(run.coef, c64, cb, what + " coef of the kernel's sums")
    if kw.get("weight_ce", 1.0) == 0:
        assert float(run.coef[-1]) == 0.0, what + ": weight_ce = 0 must give a CE scale of exactly 0"
    if kw.get("weight_dice", 1.0) == 0:
        assert bool((run.coef[:-1] == 0).all()), what + ": weight_dice = 0 must give Dice coefficients of exactly 0"
    rg = O.regrad(ref, x, t, run.coef)
    gb = O.grad_bound(rg)
    live = (rg.stats.m if regions else rg.stats.valid)[:, None].expand(run.grad.shape)
    assert bool((run.grad[~live] == 0).all()), what + ": an ignored pixel has a non-zero gradient"
    R.assert_within(run.grad, rg.grad, gb, what + " gradient")
    # ... and the whole chain against the oracle's own loss (the kernel's sums inside their bounds move the loss by at most lb_chain)
    l_ref, _, lb_ref, _ = O.finish_bound(ref.sums, ref.CD, per_elem, kw.get("weight_ce", 1.0), kw.get("weight_dice", 1.0),
                                         kw.get("smooth", 1e-5), kw.get("grad_mult", 1.0))
    print(f"[share] {what}: sums {R.share(run.sums, ref.sums, sb):.3f} grad {R.share(run.grad, rg.grad, gb):.3f} "
          f"loss {float(run.loss):.9g} fp64 {float(l_ref):.9g}")
    return run, ref


def soft_inputs(B, K, HW, seed, ign, empty=None):
    return R.general_draw(B, K, HW, seed), R.labels_draw(B, K, HW, seed + 100, empty=empty, ignore_frac=0.3 if ign else 0.0)


def region_inputs(B, Rn, HW, seed, u):
    x = R.general_draw(B, Rn, HW, seed)
    y = torch.randint(0, 2, (B, Rn, HW), generator=torch.Generator().manual_seed(seed + 100)).to(torch.uint8)
    if u:
        y = torch.cat((y, (~R.mask_draw(B, HW, seed + 200, 0.3))[:, None].to(torch.uint8)), 1)
    return x, y.contiguous()


def soft_kw(name, K, ign):
    kw = dict(O.OPTION_SETS[name])
    if kw.get("class_w") == "pow2":
        kw["class_w"] = O.class_weights(K, "pow2")
    kw["ignore"] = IGN if ign else None
    return kw


# ---------------------------------------------------------------------------------------------------- 1. shapes and options against fp64
@pytest.mark.parametrize("HW", O.QUAD_HW)
def test_quad_edges(HW):
    """B = 3: partial quads and rows that are not 16-byte aligned, every kind of kernel"""
    x, t = soft_inputs(3, 3, HW, 900 + HW, True)
    gate(x, t, "quad softmax", ignore=IGN, do_bg=True, batch_dice=False, class_w=O.class_weights(3, "general"), weight_ce=0.5, weight_dice=2.0)
    gate(x, R.labels_draw(3, 3, HW, 930 + HW), "quad softmax batch", weight_ce=0.5)
    for u in (0, 1):
        x, y = region_inputs(3, 3, HW, 950 + HW, u)
        gate(x, y, "quad regions", regions=True, has_ignore=bool(u), batch_dice=False, weight_dice=2.0)
        gate(x, y, "quad regions batch", regions=True, has_ignore=bool(u), weight_ce=0.5)


@pytest.mark.parametrize("name", list(O.OPTION_SETS))
@pytest.mark.parametrize("ign", [False, True], ids=["plain", "ignore"])
@pytest.mark.parametrize("K", O.K_SET)
def test_softmax_options(K, ign, name):
    for i, (B, H, W) in enumerate(O.SHAPES):
        x, t = soft_inputs(B, K, H * W, 1000 + 10 * K + i, ign)
        gate(x, t, name, **soft_kw(name, K, ign))


@pytest.mark.parametrize("K", O.K_SET)
def test_softmax_class_weights_ignore_weights_and_per_sample_together(K):
    B, H, W = O.SHAPES[1]
    x, t = soft_inputs(B, K, H * W, 1100 + K, True)
    gate(x, t, "all", ignore=IGN, class_w=O.class_weights(K, "general"), weight_ce=0.5, weight_dice=2.0, batch_dice=False, do_bg=True)


@pytest.mark.parametrize("name", O.REGION_SETS)
@pytest.mark.parametrize("u", [0, 1], ids=["plain", "ignore"])
@pytest.mark.parametrize("Rn", O.R_SET)
def test_region_options(Rn, u, name):
    for i, (B, H, W) in enumerate(O.SHAPES):
        x, y = region_inputs(B, Rn, H * W, 1200 + 10 * Rn + i, u)
        gate(x, y, name, regions=True, has_ignore=bool(u), **O.OPTION_SETS[name])


@pytest.mark.parametrize("go,smooth,gm", R.GO_SMOOTH_MULT, ids=["go1.7", "go-0.5-s1-m2", "go0-s0", "goNULL-m2"])
def test_grad_out_smooth_and_grad_mult(go, smooth, gm):
    B, H, W = O.SHAPES[1]
    x, t = soft_inputs(B, 5, H * W, 1300, True)
    gate(x, t, "go softmax", ignore=IGN, class_w=O.class_weights(5, "general"), weight_ce=0.5, weight_dice=2.0, do_bg=True, go=go, smooth=smooth,
         grad_mult=gm)
    gate(x, t, "go softmax per-sample", ignore=IGN, batch_dice=False, go=go, smooth=smooth)
    x, y = region_inputs(B, 3, H * W, 1310, 1)
    gate(x, y, "go regions", regions=True, has_ignore=True, weight_ce=0.5, weight_dice=2.0, go=go, smooth=smooth, grad_mult=gm)
    gate(x, y, "go regions per-sample", regions=True, has_ignore=True, batch_dice=False, go=go, smooth=smooth)


@pytest.mark.parametrize("kind", ["softmax", "regions"])
def test_past_one_pass_of_an_image_s_blocks(kind):
    """BIG: 1057 quads per image against 512 (sums, 1 block x 2 quads per lane) and 1024 (backward, 4 blocks): 5 and 2 grid-stride trips"""
    B, H, W = O.BIG
    HW = H * W
    assert O.trips(B, HW, False) > 2 and O.trips(B, HW, True) > 1
    if kind == "softmax":
        x, t = soft_inputs(B, 2, HW, 1400, True)
        run, _ = gate(x, t, "big", ignore=IGN, batch_dice=False, do_bg=True, class_w=[0.5, 2.0], weight_ce=0.5)
    else:
        x, y = region_inputs(B, 1, HW, 1410, 1)
        run, _ = gate(x, y, "big", regions=True, has_ignore=True, batch_dice=False, weight_dice=2.0)
    assert not bool((run.grad == X.SENTINEL).any())


# ---------------------------------------------------------------------------------------------------- 2. exact cases
@pytest.mark.parametrize("onehot_only", [True, False], ids=["onehot", "mixed"])
@pytest.mark.parametrize("K", R.EXACT_K)
def test_exact_sums_softmax(K, onehot_only):
    """integer logits, power-of-two class weights: sum w_t, G, I, P are sums of exactly representable terms (multiples of 1 / (4 K) far
    below 2^24 granules) and must equal fp64 to the bit; with one-hot probabilities alone so is the CE column (terms 0 or 128 w_t)"""
    B, H, W = R.EXACT_SHAPE
    x = R.exact_softmax_draw(B, K, H * W, 1500 + K, onehot_only=onehot_only)
    for ign in (False, True):
        t = R.labels_draw(B, K, H * W, 1510 + K, ignore_frac=0.3 if ign else 0.0)
        for bd in (True, False):
            _, ref = gate(x, t, "exact", exact=onehot_only, ignore=IGN if ign else None, class_w=O.class_weights(K, "pow2"), batch_dice=bd,
                          do_bg=True, weight_ce=0.5, weight_dice=2.0)
            X.require_exact(float(ref.sums[:, 1:].abs().max()), 1.0 / (2 * K))          # sum w_t in halves, I and P in 1 / K
            if onehot_only:
                X.require_exact(float(ref.sums[:, 0].abs().max()), 64.0)                # CE terms: 128 w_t


@pytest.mark.parametrize("onehot_only", [True, False], ids=["onehot", "mixed"])
@pytest.mark.parametrize("Rn", R.EXACT_R)
def test_exact_sums_regions(Rn, onehot_only):
    B, H, W = R.EXACT_SHAPE
    x, y = R.exact_sigmoid_draw(B, Rn, H * W, 1600 + Rn, onehot_only=onehot_only)
    for u in (0, 1):
        tg = torch.cat((y, (~R.mask_draw(B, H * W, 1610 + Rn, 0.3))[:, None].to(torch.uint8)), 1).contiguous() if u else y
        for bd in (True, False):
            gate(x, tg, "exact regions", exact=onehot_only, regions=True, has_ignore=bool(u), batch_dice=bd, weight_ce=0.5, weight_dice=2.0)


# ---------------------------------------------------------------------------------------------------- 3. degenerate rows and extremes
def test_an_image_without_a_class_and_an_ignored_image():
    B, K, HW = 3, 3, 35
    x = R.general_draw(B, K, HW, 1700)
    t = R.labels_draw(B, K, HW, 1701, ignore_frac=0.2)
    t[1] = torch.where(t[1] == 2, torch.zeros_like(t[1]), t[1])          # image 1 has no voxel of class 2
    t[2] = IGN                                                            # image 2 is ignored entirely
    run, ref = gate(x, t, "degenerate", ignore=IGN, batch_dice=False, do_bg=True, class_w=[1.0, 2.0, 4.0])
    assert bool((run.sums[2] == 0).all()) and bool((run.grad[2] == 0).all())
    assert float(run.sums[1, 2 + 3 * 2 + 2]) == 0.0                       # G of class 2 in image 1
    # the Dice of the ignored image is exactly 1 per class: with Dice alone and every image ignored the loss is exactly -weight_dice
    t[:] = IGN
    for bd in (True, False):
        run, _ = gate(x, t, "all ignored", ignore=IGN, batch_dice=bd, class_w=[1.0, 2.0, 4.0], weight_ce=0.5, weight_dice=2.0)
        assert float(run.loss) == -2.0 and float(run.coef[-1]) == 0.0 and bool((run.grad == 0).all())   # CE exactly 0, Dice exactly 1
        run, _ = gate(x, t, "all ignored, CE alone", ignore=IGN, batch_dice=bd, class_w=[1.0, 2.0, 4.0], weight_dice=0.0)
        assert float(run.loss) == 0.0 and bool((run.grad == 0).all())
    xr, y = region_inputs(B, 3, HW, 1710, 1)
    y[:, -1] = 1
    run, _ = gate(xr, y, "regions all ignored", regions=True, has_ignore=True, batch_dice=False, weight_ce=0.5, weight_dice=2.0)
    assert float(run.loss) == -2.0 and bool((run.grad == 0).all())


def test_weighted_ce_does_not_saturate_at_large_gaps():
    """GAPS: a target 20 .. 200 below the maximum gives w_t gap, not a saturated -log of an underflowed probability"""
    x, t = R.extreme_softmax_draw(3)
    w = [2.0, 0.5, 1.0]
    run, ref = gate(x, t, "gaps", class_w=w, weight_dice=0.0)
    wt = torch.tensor(w, dtype=torch.float64)[t[0]]
    want = float((wt * torch.tensor([g if below else 0.0 for g in R.GAPS for below in (True, False)], dtype=torch.float64)).sum() / wt.sum())
    assert abs(float(run.loss) - want) <= 1e-6 * want + float((wt * 1.4).sum() / wt.sum())      # (log se <= log 3 per pixel)
    assert float(run.loss) > 0.9 * want
    gate(x, t, "gaps + Dice", class_w=w, do_bg=True, batch_dice=False)


@pytest.mark.parametrize("c", R.OFFSETS[1:])
def test_weighted_ce_keeps_its_accuracy_under_a_common_offset(c):
    """x + c against the fp64 reference of x (the offset adds exactly): the bounds do not know c"""
    B, K, H, W = R.OFFSET_SHAPE
    xc, x = R.offset_draw(B, K, H * W, 5, c)
    t = R.labels_draw(B, K, H * W, 6, ignore_frac=0.2)
    d = dev()
    kw = dict(ignore=IGN, class_w=O.class_weights(K, "general"), batch_dice=False, weight_ce=0.5)
    run = run_opt(xc.to(d), t.to(d), **kw)
    ref = O.opt_ref(x, t, **kw)
    R.assert_within(run.sums, ref.sums, O.sums_bound(ref), f"offset {c} sums")
    rg = O.regrad(ref, x, t, run.coef)
    R.assert_within(run.grad, rg.grad, O.grad_bound(rg), f"offset {c} gradient")
    l64, _, lb, _ = O.finish_bound(run.sums, ref.CD, False, 0.5, 1.0, 1e-5, 1.0)
    R.assert_within(run.loss, l64.reshape(1), lb, f"offset {c} loss")


# ---------------------------------------------------------------------------------------------------- 4. a weight of 0 leaves no trace
def test_zero_weights_leave_no_trace_of_the_dropped_term():
    B, H, W = O.SHAPES[1]
    d = dev()
    x, t = soft_inputs(B, 5, H * W, 1800, True)
    base = dict(ignore=IGN, batch_dice=False, do_bg=True)
    # weight_ce = 0: the class weights cannot matter, to the bit; the gradient is the Dice term's alone (gate: against the oracle)
    a, _ = gate(x, t, "no CE", weight_ce=0.0, class_w=O.class_weights(5, "pow2"), **base)
    b = run_opt(x.to(d), t.to(d), weight_ce=0.0, class_w=[7.0, 0.125, 3.0, 11.0, 0.7], **base)
    c = run_opt(x.to(d), t.to(d), weight_ce=0.0, **base)
    assert torch.equal(a.grad, b.grad) and torch.equal(a.loss, b.loss) and torch.equal(a.grad, c.grad) and torch.equal(a.loss, c.loss)
    _, g_dice = O.ref_loss(x, t, weight_ce=0.0, **base)
    assert float((a.grad.double() - g_dice).abs().max()) <= 1e-5 * float(g_dice.abs().max())
    # weight_dice = 0: smooth, do_bg and batch_dice cannot matter, to the bit; the gradient is the CE term's alone
    kw = dict(ignore=IGN, class_w=O.class_weights(5, "general"), weight_dice=0.0)
    a, _ = gate(x, t, "no Dice", **kw)
    b = run_opt(x.to(d), t.to(d), smooth=3.0, do_bg=True, **kw)
    c = run_opt(x.to(d), t.to(d), batch_dice=False, **kw)
    assert torch.equal(a.grad, b.grad) and torch.equal(a.loss, b.loss) and torch.equal(a.grad, c.grad) and torch.equal(a.loss, c.loss)
    xr, y = region_inputs(B, 3, H * W, 1810, 1)
    a, _ = gate(xr, y, "regions no Dice", regions=True, has_ignore=True, weight_dice=0.0)
    b = run_opt(xr.to(d), y.to(d), regions=True, has_ignore=True, weight_dice=0.0, smooth=3.0, batch_dice=False)
    assert torch.equal(a.grad, b.grad) and torch.equal(a.loss, b.loss)


# ---------------------------------------------------------------------------------------------------- 5. the public modules
def _module_case(K=3, B=3, H=19, W=21, seed=1900):
    x, t = soft_inputs(B, K, H * W, seed, True)
    return x.view(B, K, H, W), t.view(B, 1, H, W)


OPTS = dict(weight_ce=0.5, weight_dice=2.0, batch_dice=False, do_bg=True, ce_class_weights=[1.0, 2.0, 0.5])


def _oracle(x, t, regions=False, **kw):
    B, N = x.shape[:2]
    kw = dict(kw)
    if "ce_class_weights" in kw:
        kw["class_w"] = kw.pop("ce_class_weights")
    return O.ref_loss(x.reshape(B, N, -1), t.reshape(B, -1) if not regions else t.reshape(B, t.shape[1], -1), regions=regions, **kw)


def test_module_matches_the_oracle_and_is_deterministic():
    from dinounet_amd.training import build_loss
    d = dev()
    x, t = _module_case()
    l = build_loss(3, ignore_label=IGN, **OPTS)
    assert not l.options_default and l.class_w.is_cuda
    res = []
    for _ in range(2):
        xd = x.to(d).requires_grad_(True)
        loss = l(xd, t.to(d))
        (g,) = torch.autograd.grad(loss, xd)
        res.append((loss.detach().cpu(), g.cpu()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])          # two calls, identical bits
    want, wg = _oracle(x, t, ignore=IGN, **OPTS)
    run, ref = gate(x.reshape(3, 3, -1), t.reshape(3, -1), "module", ignore=IGN, weight_ce=0.5, weight_dice=2.0, batch_dice=False, do_bg=True,
                    class_w=OPTS["ce_class_weights"])
    assert torch.equal(res[0][0].reshape(1), run.loss) and torch.equal(res[0][1].reshape(run.grad.shape), run.grad)   # the module is the C ABI's chain
    # regions through the module: labels -> planes on the device -> the option loss
    regs = [(1, 2), (2,)]
    lr = build_loss(2, regions=regs, ignore_label=3, weight_ce=0.5, weight_dice=2.0, batch_dice=False)
    lab = torch.randint(0, 4, (3, 1, 19, 21), generator=torch.Generator().manual_seed(5))
    xr = R.general_draw(3, 2, 399, 1910).view(3, 2, 19, 21)
    xd = xr.to(d).requires_grad_(True)
    loss = lr(xd, lab.to(d))
    (g,) = torch.autograd.grad(loss, xd)
    from dinounet_amd.training import labels_to_regions
    planes = labels_to_regions(lab, regs, 3)
    run, _ = gate(xr.reshape(3, 2, -1), planes.reshape(3, 3, -1).contiguous(), "module regions", regions=True, has_ignore=True, weight_ce=0.5,
                  weight_dice=2.0, batch_dice=False)
    assert torch.equal(loss.detach().cpu().reshape(1), run.loss) and torch.equal(g.cpu().reshape(run.grad.shape), run.grad)


def test_defaults_are_untouched():
    """with every option at its default the modules launch what they always launched: bit-identical to the ops they wrap"""
    from dinounet_amd import ops
    from dinounet_amd.training import build_loss, labels_to_regions
    d = dev()
    x, t = _module_case()
    xd, td = x.to(d), t.to(d)
    t0 = torch.where(t == IGN, torch.zeros_like(t), t).to(d)

    def both(f, xin):
        xin = xin.clone().requires_grad_(True)
        l = f(xin)
        (g,) = torch.autograd.grad(l, xin)
        return l.detach(), g

    for kw in (dict(), dict(weight_ce=1.0, weight_dice=1.0, batch_dice=True, do_bg=False, ce_class_weights=None)):
        a, b = both(lambda v: build_loss(3, **kw)(v, t0), xd), both(lambda v: ops.dice_ce_loss(v, t0), xd)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        a, b = both(lambda v: build_loss(3, ignore_label=IGN, **kw)(v, td), xd), both(lambda v: ops.dice_ce_masked_loss(v, td, IGN), xd)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    regs = [1, 2, (1, 2)]
    lab = torch.randint(0, 4, (3, 1, 19, 21), generator=torch.Generator().manual_seed(6)).to(d)
    for ig in (None, 3):
        planes = labels_to_regions(lab, regs, ig)
        a = both(lambda v: build_loss(3, regions=regs, ignore_label=ig, do_bg=True)(v, lab), xd)
        b = both(lambda v: ops.dice_bce_loss(v, planes, ig is not None), xd)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_unsupported_class_counts_raise_the_wrappers_message():
    from dinounet_amd import ops
    d = dev()
    x = torch.zeros(1, 9, 4, 4, device=d)
    with pytest.raises(RuntimeError, match="supports 2..8 classes, got 9"):
        ops.dice_ce_opt_loss(x, torch.zeros(1, 1, 4, 4, dtype=torch.long, device=d), weight_ce=0.5)
    with pytest.raises(RuntimeError, match="supports 1..8 regions, got 9"):
        ops.dice_bce_opt_loss(x, torch.zeros(1, 9, 4, 4, dtype=torch.uint8, device=d), False, weight_ce=0.5)


def test_deep_supervision_with_options_equals_the_composed_oracle():
    from dinounet_amd.training import build_loss
    d = dev()
    w = [4 / 7, 2 / 7, 1 / 7]
    l = build_loss(3, ignore_label=IGN, deep_supervision_weights=w, **OPTS)
    B = 2
    outs = [R.general_draw(B, 3, h * wd, 2000 + i).view(B, 3, h, wd) for i, (h, wd) in enumerate(R.DS_EXACT)]
    H, W = R.DS_EXACT[0]
    t = R.labels_draw(B, 3, H * W, 2003, ignore_frac=0.2)
    od = [o.to(d).requires_grad_(True) for o in outs]
    assert not l.fused(od)
    loss = l(od, t.view(B, 1, H, W).to(d))
    grads = torch.autograd.grad(loss, od)
    want, bound = 0.0, 0.0
    kw = dict(ignore=IGN, weight_ce=0.5, weight_dice=2.0, batch_dice=False, do_bg=True, class_w=OPTS["ce_class_weights"])
    for ws, o, g in zip(w, outs, grads):
        h, wd = o.shape[-2:]
        ts = R.ds_target(t, H, W, h, wd)
        xs = o.reshape(B, 3, -1)
        run = run_opt(xs.to(d), ts.contiguous().to(d), go=ws, **kw)
        ref = O.opt_ref(xs, ts, go=ws, **kw)
        rg = O.regrad(ref, xs, ts, run.coef)
        R.assert_within(g.cpu().reshape(rg.grad.shape), rg.grad, O.grad_bound(rg), f"scale {h} x {wd} gradient")
        R.assert_within(run.sums, ref.sums, O.sums_bound(ref), f"scale {h} x {wd} sums")
        l64, _, lb, _ = O.finish_bound(run.sums, ref.CD, False, 0.5, 2.0, 1e-5, 1.0)
        want, bound = want + ws * l64, bound + ws * lb + 4 * R.U * abs(ws * float(l64))       # the product and the sum of three terms
    R.assert_within(loss.detach().cpu().reshape(1), want.reshape(1), bound, "deep supervision total of the kernels' sums")
    total64 = sum(ws * O.ref_loss(o.reshape(B, 3, -1), R.ds_target(t, H, W, *o.shape[-2:]), **kw)[0] for ws, o in zip(w, outs))
    assert abs(float(loss) - float(total64)) <= 1e-5 * max(1.0, abs(float(total64)))


class _PixelNet(torch.nn.Module):
    """three logits per pixel from one input channel: elementwise, so a captured step holds the loss kernels and little else"""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor([0.5, -1.0, 1.5]).view(1, 3, 1, 1))
        self.b = torch.nn.Parameter(torch.tensor([0.1, 0.0, -0.2]).view(1, 3, 1, 1))

    def forward(self, x):
        return x * self.w + self.b


def test_val_step_with_options_counts_and_loss():
    from dinounet_amd.training import ValStep, build_loss
    d = dev()
    net = _PixelNet().to(d)
    x = torch.randn(3, 1, 19, 21, generator=torch.Generator().manual_seed(7)).to(d)
    t = R.labels_draw(3, 3, 399, 2100, ignore_frac=0.2).view(3, 1, 19, 21).to(d)
    l = build_loss(3, ignore_label=IGN, **OPTS)
    v0 = ValStep(net, x.shape, t.shape, d, loss=build_loss(3, ignore_label=IGN), graph=False)
    v = ValStep(net, x.shape, t.shape, d, loss=l, graph=False)
    v0(x, t)
    got = v(x, t)
    with torch.no_grad():
        want = l(net(x), t)
    assert torch.equal(v.counts, v0.counts) and int(v.counts.sum()) > 0 and torch.equal(got, want)
    assert not torch.equal(got, v0.loss)


def test_train_step_captured_with_options_equals_eager_bit_for_bit():
    from dinounet_amd.optim import FusedClipSGD
    from dinounet_amd.training import TrainStep, build_loss
    d = dev()
    x = torch.randn(2, 1, 16, 16, generator=torch.Generator().manual_seed(8)).to(d)
    t = R.labels_draw(2, 3, 256, 2200, ignore_frac=0.2).view(2, 1, 16, 16).to(d)
    out = {}
    for mode in (False, True):
        net = _PixelNet().to(d)
        params = list(net.parameters())
        opt = FusedClipSGD(params, 1e-2, momentum=0.99, nesterov=True, weight_decay=3e-5)
        ts = TrainStep(net, opt, params, x.shape, t.shape, d, graph=mode, warmup=2, loss=build_loss(3, ignore_label=IGN, **OPTS))
        ls = [ts(x, t).clone()] + [ts().clone() for _ in range(5)]
        torch.cuda.synchronize()
        if mode:
            assert ts.capture_mode == "whole_step", ts.capture_mode
        out[mode] = (torch.stack([v.detach().reshape(()) for v in ls]).cpu(), [p.detach().cpu().clone() for p in params])
    assert bool(torch.isfinite(out[True][0]).all())
    assert torch.equal(out[False][0], out[True][0]), (out[False][0], out[True][0])
    assert all(torch.equal(a, b) for a, b in zip(out[False][1], out[True][1]))
