"""fp64 oracle, regime formulas and bounds for the fused option losses of csrc/loss_opt.hip (tests/test_gpu_loss_options.py, kept honest by
tests/test_cpu_loss_options.py).  Plain torch on the CPU, no library load.  An extension of tests/_loss_ref.py, which is imported and
left alone: the draws, the per-term error model (softmax_term_err, sigmoid_term_err, eps_exp) and U are its.

Oracle.  `ref_loss` is the reference's formulas with stock torch in fp64: F.cross_entropy(x, t, weight=w, ignore_index=...) for the CE,
MemoryEfficientSoftDiceLoss.forward (dice.py:72-119) restated line for line for the Dice, binary_cross_entropy_with_logits for the
regions; the gradient is autograd's.  tests/golden/loss_options.json holds what the reference's own classes return for the same option
sets (tools/make_golden_loss_options.py); the CPU module compares the two.

`opt_ref` is the closed form of the same loss in the kernels' terms (sums rows, coefficients, d loss / d logits per element), which the
per-element bounds need; the CPU module holds it against `ref_loss`.

Bounds: those of _loss_ref.py with the factors the options add.
  sums:   the terms' own errors + depth u |sum|; the depth is that of the layout of loss_opt.hip (opt_sum_depth: a lane's trips x 4, wave
          tree 6, block 3, a second-stage thread's rows, tree 9; per-sample rows are shallower: G rows instead of B G).  The CE term w_t nll
          carries one more rounding (u w_t nll) and w_t times the error of nll; sum w_t has exact terms.
  finish: finish_bound's counts with the weights as factors (|wce| on the CE part, |wd| on the Dice part) and `rows` more additions where
          rows of CE heads / Dice quotients are added.
  grad:   grad_bound's formula per element with scale -> scale w_t (one more product: + u |A|) and the coefficient row of the pixel's image."""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

import _loss_ref as R

U = R.U
OPT_SUMS_CAP, OPT_BWD_CAP = 2048, 8192


# ---------------------------------------------------------------------------------------------------- regimes
def img_blocks(B, HW, per_block, cap):
    """opt_img_blocks of csrc/loss_opt.hip: blocks per image"""
    return int(min(max(R.cdiv(R.cdiv(HW, 4), per_block), 1), max(cap // B, 1)))


def sums_blocks(B, HW):
    return img_blocks(B, HW, 512, OPT_SUMS_CAP)


def bwd_blocks(B, HW):
    return img_blocks(B, HW, 256, OPT_BWD_CAP)


def trips(B, HW, bwd):
    """grid-stride trips of the longest-running thread: an image's quads over the 256 G lanes of its blocks"""
    g = bwd_blocks(B, HW) if bwd else sums_blocks(B, HW)
    return R.cdiv(R.cdiv(HW, 4), g * 256)


def cd_of(N, regions, do_bg):
    return N if (regions or do_bg) else N - 1


def ws_elems(B, N, HW, regions, do_bg):
    return B * sums_blocks(B, HW) * (2 + 3 * cd_of(N, regions, do_bg))


def opt_sum_depth(B, HW, batch_dice):
    G = sums_blocks(B, HW)
    return trips(B, HW, False) * 4 + 9 + R.cdiv(B * G if batch_dice else G, 256) + 9


# ---------------------------------------------------------------------------------------------------- the oracle (stock torch, fp64)
def ref_loss(x, t, *, regions=False, ignore=None, has_ignore=False, weight_ce=1.0, weight_dice=1.0, batch_dice=True, do_bg=None,
             class_w=None, smooth=1e-5):
    """x (B, N, HW) any dtype (made fp64, requires_grad) -> (loss, grad).  softmax: t (B, HW) int64; regions: t (B, R + u, HW) {0, 1}.
    DC_and_CE_loss.forward / DC_and_BCE_loss.forward (compound_losses.py:31-56, :83-99) and MemoryEfficientSoftDiceLoss.forward."""
    x = x.detach().double().requires_grad_(True)
    if do_bg is None:
        do_bg = regions
    if regions:
        Rn = x.shape[1]
        mask = (1 - t[:, -1:]).bool() if has_ignore else None
        y = t[:, :Rn].double()
        p = torch.sigmoid(x)
        if weight_ce != 0:
            if mask is not None:
                ce = (F.binary_cross_entropy_with_logits(x, y, reduction="none") * mask).sum() / torch.clip(mask.sum(), min=1e-8)
            else:
                ce = F.binary_cross_entropy_with_logits(x, y)
        y_onehot = y
    else:
        mask = (t != ignore)[:, None] if ignore is not None else None
        td = torch.where(mask[:, 0], t, torch.zeros_like(t)) if mask is not None else t
        p = torch.softmax(x, 1)
        if weight_ce != 0:
            w = None if class_w is None else torch.as_tensor(class_w, dtype=torch.float64)
            if mask is not None and not bool(mask.any()):
                ce = 0.0                                                   # compound_losses.py:53: num_fg > 0
            else:
                ce = F.cross_entropy(x, t, weight=w, ignore_index=ignore if ignore is not None else -100)
        y_onehot = torch.zeros(x.shape, dtype=torch.bool)
        y_onehot.scatter_(1, td[:, None], 1)
    total = 0.0
    if weight_ce != 0:
        total = weight_ce * ce
    if weight_dice != 0:
        # dice.py:72-119
        axes = (2,)
        with torch.no_grad():
            if not do_bg:
                y_onehot = y_onehot[:, 1:]
            sum_gt = y_onehot.sum(axes) if mask is None else (y_onehot * mask).sum(axes)
        if not do_bg:
            p = p[:, 1:]
        if mask is None:
            intersect = (p * y_onehot).sum(axes)
            sum_pred = p.sum(axes)
        else:
            intersect = (p * y_onehot * mask).sum(axes)
            sum_pred = (p * mask).sum(axes)
        if batch_dice:
            intersect, sum_pred, sum_gt = intersect.sum(0), sum_pred.sum(0), sum_gt.sum(0)
        dc = (2 * intersect + smooth) / (torch.clip(sum_gt + sum_pred + smooth, 1e-8))
        total = total + weight_dice * (-dc.mean())
    total.backward()
    return total.detach(), x.grad


# ---------------------------------------------------------------------------------------------------- closed form in the kernels' terms
def opt_ref(x, t, *, regions=False, ignore=None, has_ignore=False, weight_ce=1.0, weight_dice=1.0, batch_dice=True, do_bg=None,
            class_w=None, smooth=1e-5, grad_mult=1.0, go=1.0, coef=None):
    """-> sums (rows, NS), loss, coef (rows 2 CD + 1), grad (B, N, HW), and what the bounds need.  coef: take these (the kernel's own fp32
    coefficients) for the gradient instead of the fp64 ones."""
    B, N, HW = x.shape
    if do_bg is None:
        do_bg = regions
    CD = cd_of(N, regions, do_bg)
    rows = 1 if batch_dice else B
    if regions:
        m = (t[:, -1] == 0) if has_ignore else torch.ones(B, HW, dtype=torch.bool)
        s = R.sigmoid_stats(x, t[:, :N], m)
        mf = m[:, None].double()
        head = torch.stack(((s.bce * mf).sum((1, 2)), m.double().sum(1)), 1)                        # (B, 2)
        ipg = torch.stack(((s.s * s.y * mf).sum(2), (s.s * mf).sum(2), (s.y * mf).sum(2)), 2)       # (B, CD, 3)
        wt = None
    else:
        s = R.softmax_stats(x, t, ignore)
        vf = s.valid[:, None].double()
        w = torch.ones(N, dtype=torch.float64) if class_w is None else torch.as_tensor(class_w, dtype=torch.float64)
        tt = torch.where(s.valid, t, torch.zeros_like(t)).clamp(0, N - 1)
        wt = w[tt] * s.valid
        head = torch.stack(((wt * s.nll).sum(1), wt.sum(1)), 1)
        c0 = N - CD
        ipg = torch.stack(((s.p * s.oh).sum(2)[:, c0:], (s.p * vf).sum(2)[:, c0:], s.oh.double().sum(2)[:, c0:]), 2)
    per_img = torch.cat((head, ipg.reshape(B, -1)), 1)                                              # (B, NS)
    sums = per_img.sum(0, keepdim=True) if batch_dice else per_img
    loss, coef64 = finish64(sums, CD, regions and not has_ignore, weight_ce, weight_dice, smooth, grad_mult)
    cf = coef64 if coef is None else coef.double()
    scale = float(cf[-1])
    pairs = cf[:-1].view(rows, CD, 2)
    ca = pairs[:, :, 0].expand(B, CD)
    cb = pairs[:, :, 1].expand(B, CD)
    if regions:
        A = (s.s - s.y) * scale
        c = ca[:, :, None] * s.y + cb[:, :, None]
        Bt = c * s.s * (1 - s.s)
        grad = go * (A + Bt) * mf
        parts = SimpleNamespace(A=A, B=Bt, cabs=ca.abs()[:, :, None] * s.y + cb.abs()[:, :, None])
    else:
        z = torch.zeros(B, N - CD, dtype=torch.float64)
        ca, cb = torch.cat((z, ca), 1), torch.cat((z, cb), 1)
        oh = s.oh.double()
        g = ca[:, :, None] * oh + cb[:, :, None]
        dot = (g * s.p).sum(1, keepdim=True)
        A = (s.p - oh) * (scale * wt)[:, None]
        Bt = s.p * (g - dot)
        grad = go * (A + Bt) * s.valid[:, None].double()
        parts = SimpleNamespace(A=A, B=Bt, g=g, dot=dot, gabs=ca.abs()[:, :, None] * oh + cb.abs()[:, :, None])
    return SimpleNamespace(sums=sums, loss=loss, coef=coef64, scale=scale, wt=wt, grad=grad, stats=s, parts=parts, regions=regions, go=go,
                           rows=rows, CD=CD, B=B, HW=HW, batch_dice=batch_dice,
                           kw=dict(regions=regions, ignore=ignore, has_ignore=has_ignore, weight_ce=weight_ce, weight_dice=weight_dice,
                                   batch_dice=batch_dice, do_bg=do_bg, class_w=class_w, smooth=smooth, grad_mult=grad_mult, go=go))


def finish64(sums, CD, per_elem, weight_ce, weight_dice, smooth, grad_mult):
    """opt_finish_kernel in fp64 on any sums (rows, NS) -> (loss, coef (rows 2 CD + 1))"""
    sums = sums.double()
    rows = sums.shape[0]
    ipg = sums[:, 2:].view(rows, CD, 3)
    I, P, G = ipg[..., 0], ipg[..., 1], ipg[..., 2]
    num, raw = 2 * I + smooth, G + P + smooth
    den = raw.clamp_min(R.CLIP)
    cnt = CD * rows
    ca = -2.0 * (weight_dice / cnt) / den * grad_mult
    cb = torch.where(raw > R.CLIP, num / (den * den) * (weight_dice / cnt), torch.zeros_like(num)) * grad_mult
    if weight_dice == 0:
        ca, cb = torch.zeros_like(ca), torch.zeros_like(cb)
    nv = float(sums[:, 1].sum())
    scale = 0.0 if nv <= 0 else 1.0 / (nv * CD if per_elem else nv)
    loss = torch.zeros((), dtype=torch.float64)
    if weight_ce != 0:
        loss = loss + weight_ce * (sums[:, 0].sum() * scale)
    if weight_dice != 0:
        loss = loss - weight_dice * ((num / den).sum() / cnt)
    coef = torch.cat((torch.stack((ca, cb), 2).reshape(-1), torch.tensor([scale * weight_ce], dtype=torch.float64)))
    return loss, coef


def regrad(ref, x, t, coef):
    return opt_ref(x, t, coef=coef, **ref.kw)


# ---------------------------------------------------------------------------------------------------- bounds
def sums_bound(ref):
    """(rows, NS): the terms' own errors + depth u |sum|.  CE column: the term is w_t nll, one product more than _loss_ref's"""
    s = ref.stats
    B = ref.B
    d = opt_sum_depth(B, ref.HW, ref.batch_dice) * U
    if ref.regions:
        Es, Eb = R.sigmoid_term_err(s)
        mf = s.m[:, None].double()
        head = torch.stack(((Eb * mf).sum((1, 2)), torch.zeros(B, dtype=torch.float64)), 1)
        terr = torch.stack(((Es * s.y * mf).sum(2), (Es * mf).sum(2), torch.zeros(B, ref.CD, dtype=torch.float64)), 2)
    else:
        Ep, En = R.softmax_term_err(s)
        vf = s.valid[:, None].double()
        c0 = s.K - ref.CD
        head = torch.stack(((ref.wt * (En + U * s.nll)).sum(1), torch.zeros(B, dtype=torch.float64)), 1)
        terr = torch.stack(((Ep * s.oh).sum(2)[:, c0:], (Ep * vf).sum(2)[:, c0:], torch.zeros(B, ref.CD, dtype=torch.float64)), 2)
    per_img = torch.cat((head, terr.reshape(B, -1)), 1)
    e = per_img.sum(0, keepdim=True) if ref.batch_dice else per_img
    return e + d * ref.sums.abs()


def finish_bound(sums, CD, per_elem, weight_ce, weight_dice, smooth, grad_mult):
    """for any sums (rows, NS) -> (loss64, coef64, loss bound, coef bound).  _loss_ref.finish_bound's counts with the options' factors: a
    coefficient is at most 13 roundings from the sums (one more product: the weight over the count); the CE part: rows additions of
    the heads (twice: CE and weight), the scale (2), two products and the difference, (5 + 2 rows) u wce |CE scale|; the Dice part:
    CD rows quotients of 5 roundings, their sum, the division and the product, (9 + CD rows) u wd mean |dc|; the difference, u |loss|."""
    loss, coef = finish64(sums, CD, per_elem, weight_ce, weight_dice, smooth, grad_mult)
    s = sums.double()
    rows = s.shape[0]
    ipg = s[:, 2:].view(rows, CD, 3)
    dcs = ((2 * ipg[..., 0] + smooth) / (ipg[..., 1] + ipg[..., 2] + smooth).clamp_min(R.CLIP)).abs().sum() / (CD * rows)
    nv = float(s[:, 1].sum())
    scale = 0.0 if nv <= 0 else 1.0 / (nv * CD if per_elem else nv)
    ce = (s[:, 0].abs().sum() * scale)
    lb = U * ((5 + 2 * rows) * weight_ce * ce + (9 + CD * rows) * weight_dice * dcs + loss.abs())
    return loss, coef, lb, 13 * U * coef.abs()


def grad_bound(ref):
    """per element, for the coefficients the reference was given (the kernel's own): _loss_ref.grad_bound with scale -> scale w_t (A
    carries one more rounding) and the coefficient row of the pixel's image (already in ref.parts)"""
    s, pt, go = ref.stats, ref.parts, abs(ref.go)
    if ref.regions:
        Es, _ = R.sigmoid_term_err(s)
        EA = Es * abs(ref.scale) + 3 * U * pt.A.abs()
        EB = pt.cabs * Es + 5 * U * pt.cabs * s.s * (1 - s.s)
        return go * (EA + EB + 2 * U * (pt.A.abs() + pt.B.abs())) * s.m[:, None].double()
    Ep, _ = R.softmax_term_err(s)
    EA = Ep * (abs(ref.scale) * ref.wt)[:, None] + 4 * U * pt.A.abs()
    Edot = (pt.gabs * (Ep + (s.K + 2) * U * s.p)).sum(1, keepdim=True)
    EB = Ep * (pt.g - pt.dot).abs() + s.p * (2 * U * pt.gabs + U * pt.dot.abs() + Edot) + U * pt.B.abs()
    return go * (EA + EB + 2 * U * (pt.A.abs() + pt.B.abs())) * s.valid[:, None].double()


# ---------------------------------------------------------------------------------------------------- option sets and shapes of the GPU module
OPTION_SETS = {
    "weights": dict(weight_ce=0.5, weight_dice=2.0),
    "per_sample": dict(batch_dice=False),
    "do_bg": dict(do_bg=True),
    "class_w": dict(class_w="pow2"),
    "do_bg_per_sample": dict(do_bg=True, batch_dice=False),
    "no_ce": dict(weight_ce=0.0),
    "no_dice": dict(weight_dice=0.0),
}
REGION_SETS = ("weights", "per_sample", "no_ce", "no_dice")
K_SET, R_SET = (2, 3, 5, 8), (1, 3, 8)
QUAD_HW = R.QUAD_HW
SHAPES = ((2, 5, 7), (3, 19, 21))
# An image's quads exceed one pass of its blocks: with B = 2048 images the caps leave 1 sums block (512 quads in two trips) and 4
# backward blocks (1024 quads in one trip) per image; 65 x 65 = 4225 pixels are 1057 quads: 5 sums trips, 2 backward trips, HW odd
BIG = (2048, 65, 65)


def class_weights(K, kind="pow2"):
    """powers of two (exact products) or general positive weights (dyadic fractions: fp32 holds them, so the kernel and the fp64 oracle
    are given the same numbers)"""
    if kind == "pow2":
        return [2.0 ** ((k % 4) - 1) for k in range(K)]
    return [0.375 + 0.4375 * k for k in range(K)]


# ---------------------------------------------------------------------------------------------------- the golden's inputs
def golden_inputs(case):
    """the inputs of one case of tests/golden/loss_options.json from its seed: fp32 logits (B, N, H, W) and the target the reference's
    class takes: labels (B, 1, H, W) int64 (softmax) or one-hot planes (B, R + u, H, W) (regions, the ignore channel last)"""
    B, N, H, W = case["shape"]
    g = torch.Generator().manual_seed(case["seed"])
    x = (torch.randn(B, N, H, W, generator=g) * 2).float()
    ign = torch.rand(B, 1, H, W, generator=g) < case["ignore_frac"]
    if case["regions"]:
        y = torch.randint(0, 2, (B, N, H, W), generator=g)
        t = torch.cat((y, ign.long()), 1) if case["has_ignore"] else y
    else:
        t = torch.randint(0, N, (B, 1, H, W), generator=g)
        if case["has_ignore"]:
            t = torch.where(ign, torch.full_like(t, R.IGNORE), t)
    return x, t
