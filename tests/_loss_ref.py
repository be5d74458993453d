"""fp64 restatements, regime formulas, draws, bounds and fp32 emulations for the fused segmentation losses of csrc/loss.hip and the
per-voxel values of csrc/loss_topk.hip (tests/test_gpu_loss_bounds.py, kept honest by tests/test_cpu_loss_ref.py).  Plain torch on the
CPU, no library load.  Logits are held as (B, N, HW), label maps as (B, HW), region planes as (B, R + u, HW).

Four families: "plain" (Dice + CE), "masked" (Dice + CE with an ignore label), "regions" (Dice + BCE on sigmoid outputs) and deep
supervision over either per-pixel body.  A restatement returns everything the C ABI exposes: the sums vector in the kernel's
layout, the loss, the coefficient vector, d loss / d logits per element in closed form and the per-voxel NLL.

Two instruments, as in tests/_exact.py.  Exact draws: a pixel is either uniform (all K logits one small integer: exp2(0) = 1, se = K,
p = 1 / K for K in {2, 4, 8}) or one-hot (one class at a, the rest at a - 128: exp2 of -184.7 is 0, se = 1, p in {0, 1}, CE = 0 or 128);
regions take x in {0, +-128} (s in {1/2, 1, 0}).  G and n_valid are integers, I and P multiples of 1 / K below 2^24 granules, so the fp32
sums are exact in any order and must equal the fp64 value bit for bit.  Premise (instruction definitions; every exact gate of the GPU module passes to the bit on gfx950, so it holds there): exp2(0) is
1, exp2 below -150 is 0, log2(1) is 0 and the reciprocal of a power of two is exact.  Derived bounds otherwise: every bound is a formula
over the inputs whose constants are counted from the operations of the kernels (never fitted to an output); U carries the second-order
terms of the first-order counts.

The per-voxel NLL bound is measured, not derived: 4 x the worst error of torch's fp32 cross_entropy against fp64 on the same draw (the
factor for the native exp / log against libm).  Reference figures (torch fp32 against fp64, worst per voxel): offset_draw
(2, 3, 100 x 100) seed 5 with labels_draw seed 6: 8.48e-7 at every offset c in {0, +-64, +-1024}; general_draw with labels_draw at
(2, 3, 17 x 23) seeds 4003 / 4103: 9.26e-7, (3, 4, 48 x 40) seeds 4004 / 4104: 8.46e-7, (1, 8, 32 x 32) seeds 4008 / 4108: 7.30e-7.  The
bound does not grow with the offset because the reference's error does not.

The emulations at the end walk the kernels' own arithmetic in fp32 (per-lane quads, grid-stride trips, wave / block trees, partial rows,
the one-block row sum, dice_coefs, the backward line) with the launch caps as parameters, so that a second grid-stride trip exists at
small shapes; partial rows are indexed by block, so the order in which blocks run cannot matter and is not emulated.  One mutant per
gate: the CPU module shows each rejected by the gate meant for it."""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

import _exact as X

U = X.U_F32 * (1 + 2.0 ** -10)       # unit roundoff of fp32 with room for the second-order terms of the first-order counts below
TINY = 2.0 ** -126                   # a flushed subnormal: exp of an argument below -87.3
CLIP = float(torch.tensor(1e-8, dtype=torch.float32))      # the kernels' 1e-8f
IGNORE = 255                         # the ignore label of the draws (any value no class takes)
DS_MAX = 4
OFFSETS = (0.0, 64.0, -64.0, 1024.0, -1024.0)
GAPS = (20.0, 80.0, 87.0, 88.0, 100.0, 128.0, 200.0)
SIG_X = (0.0, 1e-7, -1e-7, 16.0, -16.0, 17.0, -17.0, 88.0, -88.0, 104.0, -104.0, 1e4, -1e4)


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------- regimes (the formulas of the kernels)
def loss_grid(npix, cap=2048):
    """blocks of the plain sums pass: four pixels per thread until the cap binds"""
    return int(min(max(cdiv(npix, 256) // 4, 1), cap))


def plain_bwd_grid(npix, cap=8192):
    return int(min(cdiv(npix, 256), cap))


def quad_items(B, HW):
    return B * cdiv(HW, 4)


def masked_grid(items, cap=2048):
    return int(min(max(cdiv(items, 512), 1), cap))


def elem_grid(items, cap=8192):
    return int(min(max(cdiv(items, 256), 1), cap))


def vec(HW, *aligned):
    """the 4-pixel vector path: HW % 4 == 0 and every pointer on its boundary (16 B fp32 / int64, 4 B uint8)"""
    return HW % 4 == 0 and all(aligned)


def ns_of(family, N):
    return 1 + 3 * (N - 1) if family == "plain" else (2 + 3 * (N - 1) if family == "masked" else 2 + 3 * N)


def ws_elems(family, B, N, HW):
    """du_dice_ce_ws_elems / du_dice_ce_masked_ws_elems / du_dice_bce_ws_elems"""
    g = loss_grid(B * HW) if family == "plain" else masked_grid(quad_items(B, HW))
    return g * ns_of(family, N)


def trips(family, B, HW, bwd):
    """grid-stride trips of the longest-running thread in the sums (bwd False) or backward pass of a family"""
    if family == "plain":
        n = B * HW
        g = plain_bwd_grid(n) if bwd else loss_grid(n)
    else:
        n = quad_items(B, HW)
        g = elem_grid(n) if bwd else masked_grid(n)
    return cdiv(n, g * 256)


def past_clamp(family, B, HW, bwd):
    """the launch cap binds: the pass runs more trips than it would with an unbounded grid (1 backward, 4 plain sums, 2 quad sums)"""
    return trips(family, B, HW, bwd) > (1 if bwd else (4 if family == "plain" else 2))


def second_trip_range(family, B, HW):
    """flat pixel index range [lo, hi) per image list that the backward pass serves in its second trip: the items from grid * 256 on"""
    if family == "plain":
        return plain_bwd_grid(B * HW) * 256, B * HW          # flat pixel indices
    return elem_grid(quad_items(B, HW)) * 256, quad_items(B, HW)      # quad items (b, q): item = b nq + q


def ds_table(B, shapes, weights, bwd):
    """(first, nblk) per scale and the total: active scales get consecutive block ranges, an inactive one (w == 0) none"""
    out, total = [], 0
    for (h, w), wt in zip(shapes, weights):
        if wt == 0.0:
            out.append((0, 0))
            continue
        items = quad_items(B, h * w)
        n = elem_grid(items) if bwd else masked_grid(items)
        out.append((total, n))
        total += n
    return out, total


def ds_src_index(n_out, n_in):
    """scipy.ndimage.zoom(order=0, mode="nearest", grid_mode=True) along one axis, NI_ZoomShift's fp64 steps"""
    z = float(n_in) / float(n_out)
    cc = (torch.arange(n_out, dtype=torch.float64) + 0.5) * z
    cc = (cc - 0.5).clamp(0.0, float(n_in - 1))
    return torch.floor(cc + 0.5).long()


def ds_target(t, H, W, h, w, mutant=None):
    """t (B, H W) -> (B, h w): the label map a scale sees"""
    if (h, w) == (H, W):
        return t
    if mutant == "ds_floor_index":
        # floor(i z), the "nearest" of torch's interpolate.  (floor((i + 0.5) z) is no mutant: it is the formula above with the -0.5 and
        # +0.5 cancelled, and picks the same index for every pair of sizes below 400: tests/test_cpu_loss_ref.py)
        iy = torch.floor(torch.arange(h, dtype=torch.float64) * (H / h)).long().clamp(max=H - 1)
        ix = torch.floor(torch.arange(w, dtype=torch.float64) * (W / w)).long().clamp(max=W - 1)
    else:
        iy, ix = ds_src_index(h, H), ds_src_index(w, W)
    return t.view(-1, H, W)[:, iy][:, :, ix].reshape(t.shape[0], h * w)


def region_planes(t, table, ignore=None):
    """labels (B, HW), table = R int bit masks -> (y (B, R, HW) in {0, 1}, m (B, HW) bool); du_labels_to_regions' convention"""
    ok = (t >= 0) & (t < 64)
    sh = t.clamp(0, 63)
    y = torch.stack([ok & (((int(m) >> sh) & 1) == 1) for m in table], 1)
    return y, (t != ignore if ignore is not None else torch.ones_like(t, dtype=torch.bool))


# ---------------------------------------------------------------------------------------------------- fp64 restatements
def dice_coefs64(ipg, smooth, mult):
    """ipg (C, 3) -> (mean dice, ca (C), cb (C)): dice_coefs of csrc/loss_common.h in fp64"""
    I, P, G = ipg[:, 0], ipg[:, 1], ipg[:, 2]
    C = ipg.shape[0]
    num, raw = 2 * I + smooth, G + P + smooth
    den = raw.clamp_min(CLIP)
    ca = -2.0 / C / den * mult
    cb = torch.where(raw > CLIP, num / (den * den) / C, torch.zeros_like(num)) * mult
    return (num / den).sum() / C, ca, cb


def softmax_stats(x, t, ignore):
    x = x.double()
    K = x.shape[1]
    valid = (t != ignore) if ignore is not None else torch.ones_like(t, dtype=torch.bool)
    tt = torch.where(valid, t, torch.zeros_like(t)).clamp(0, K - 1)
    mx = x.amax(1, keepdim=True)
    e = torch.exp(x - mx)
    se = e.sum(1, keepdim=True)
    p = e / se
    oh = F.one_hot(tt, K).permute(0, 2, 1).bool() & valid[:, None]
    nll = ((mx - x.gather(1, tt[:, None])) + torch.log(se))[:, 0] * valid
    return SimpleNamespace(x=x, p=p, oh=oh, valid=valid, nll=nll, a=(x - mx).abs(), se=se[:, 0], K=K)


def softmax_ref(x, t, family="plain", ignore=None, smooth=1e-5, grad_mult=1.0, go=1.0, weight=1.0, coef=None):
    """Dice + CE of one scale in fp64.  coef: take these (the kernel's own fp32 coefficients) for the gradient instead of the fp64 ones"""
    s = softmax_stats(x, t, ignore if family != "plain" else None)
    vf = s.valid[:, None].double()
    I = (s.p * s.oh).sum((0, 2))[1:]
    P = (s.p * vf).sum((0, 2))[1:]
    G = s.oh.double().sum((0, 2))[1:]
    ce, nv = s.nll.sum(), s.valid.double().sum()
    ipg = torch.stack((I, P, G), 1)
    head = [ce] if family == "plain" else [ce, nv]
    sums = torch.cat((torch.stack(head), ipg.reshape(-1)))
    return finish_and_grad(s, sums, family, smooth, grad_mult, go, weight, coef, npix=t.numel())


def sigmoid_stats(x, y, m):
    x, y = x.double(), y.double()
    e = torch.exp(-x.abs())
    sg = torch.where(x >= 0, 1 / (1 + e), e / (1 + e))
    bce = x.clamp_min(0) - x * y + torch.log1p(e)
    return SimpleNamespace(x=x, y=y, m=m, s=sg, bce=bce, e=e, K=x.shape[1])


def sigmoid_ref(x, y, m, has_ignore, smooth=1e-5, grad_mult=1.0, go=1.0, weight=1.0, coef=None):
    """Dice + BCE of one scale in fp64: x (B, R, HW), y (B, R, HW) in {0, 1}, m (B, HW) bool (all True without an ignore channel)"""
    s = sigmoid_stats(x, y, m)
    mf = m[:, None].double()
    ipg = torch.stack(((s.s * s.y * mf).sum((0, 2)), (s.s * mf).sum((0, 2)), (s.y * mf).sum((0, 2))), 1)
    sums = torch.cat((torch.stack(((s.bce * mf).sum(), m.double().sum())), ipg.reshape(-1)))
    return finish_and_grad(s, sums, "regions_ign" if has_ignore else "regions", smooth, grad_mult, go, weight, coef, npix=m.numel())


def finish64(sums, family, N, smooth, grad_mult, weight=1.0, npix=None):
    """the finish kernels in fp64 on any sums vector -> (loss, coef [(ca, cb) c < C, scale] (plain: no scale entry), scale)"""
    sums = sums.double()
    off = 1 if family == "plain" else 2
    dc, ca, cb = dice_coefs64(sums[off:].view(-1, 3), smooth, grad_mult * weight)
    if family == "plain":
        scale = 1.0 / npix
    else:
        nv = float(sums[1])
        scale = 0.0 if nv <= 0 else 1.0 / (nv * N if family == "regions" else nv)
    loss = sums[0] * scale - dc
    pairs = torch.stack((ca, cb), 1).reshape(-1)
    coef = pairs if family == "plain" else torch.cat((pairs, torch.tensor([scale * weight], dtype=torch.float64)))
    return loss, coef, scale * weight


def finish_and_grad(s, sums, family, smooth, grad_mult, go, weight, coef, npix):
    N = s.K
    loss, coef64, scale = finish64(sums, family, N, smooth, grad_mult, weight, npix)
    cf = coef64 if coef is None else coef.double()
    if family != "plain" and coef is not None:
        scale = float(cf[-1])
    C = N if family.startswith("regions") else N - 1
    ca, cb = cf[0:2 * C:2], cf[1:2 * C:2]
    if family.startswith("regions"):
        mf = s.m[:, None].double()
        A = (s.s - s.y) * scale
        c = ca[None, :, None] * s.y + cb[None, :, None]
        Bt = c * s.s * (1 - s.s)
        grad = go * (A + Bt) * mf
        parts = SimpleNamespace(A=A, B=Bt, cabs=ca.abs()[None, :, None] * s.y + cb.abs()[None, :, None])
        nll = None
    else:
        z = torch.zeros(1, dtype=torch.float64)
        ca, cb = torch.cat((z, ca)), torch.cat((z, cb))
        oh = s.oh.double()
        g = ca[None, :, None] * oh + cb[None, :, None]
        dot = (g * s.p).sum(1, keepdim=True)
        A = (s.p - oh) * scale
        Bt = s.p * (g - dot)
        grad = go * (A + Bt) * s.valid[:, None].double()
        parts = SimpleNamespace(A=A, B=Bt, g=g, dot=dot, gabs=ca.abs()[None, :, None] * oh + cb.abs()[None, :, None])
        nll = s.nll
    return SimpleNamespace(sums=sums, loss=loss, coef=coef64, ca=ca, cb=cb, scale=scale, grad=grad, nll=nll, stats=s, parts=parts,
                           family=family, go=go, args=(smooth, grad_mult, go, weight, npix))


def regrad(ref, coef):
    """the closed-form gradient of a restatement again, for other coefficients (the kernel's own fp32 ones): same statistics"""
    smooth, grad_mult, go, weight, npix = ref.args
    return finish_and_grad(ref.stats, ref.sums, ref.family, smooth, grad_mult, go, weight, coef, npix)


def ds_ref(outs, t, H, W, mode, weights, table=None, ignore=None, smooth=1e-5, grad_mult=1.0, go=1.0, coefs=None, mutant=None):
    """deep supervision in fp64.  outs: list of (B, N, h, w) (None where w_s == 0); mode "softmax" | "regions".  -> sums in the layout
    [(CE or BCE, n_valid) s < S | (I, P, G) c < C, s < S], loss [total, loss_s], coef (S, 2 C + 1) with w_s folded in, grads per scale"""
    S = len(weights)
    N = next(o for o in outs if o is not None).shape[1]
    C = N if mode == "regions" else N - 1
    head, tail, loss, coef, grads, refs = [], [], [], [], [], []
    total = torch.zeros((), dtype=torch.float64)
    for si, (o, w) in enumerate(zip(outs, weights)):
        if w == 0.0:
            head.append(torch.zeros(2, dtype=torch.float64)); tail.append(torch.zeros(3 * C, dtype=torch.float64))
            loss.append(torch.zeros((), dtype=torch.float64)); coef.append(torch.zeros(2 * C + 1, dtype=torch.float64))
            grads.append(None); refs.append(None)
            continue
        h, wd = o.shape[-2:]
        ts = ds_target(t, H, W, h, wd, mutant)
        x = o.reshape(o.shape[0], N, h * wd)
        cf = None if coefs is None else coefs[si]
        if mode == "regions":
            y, m = region_planes(ts, table, ignore)
            r = sigmoid_ref(x, y, m, ignore is not None, smooth, grad_mult, go, w, cf)
        else:
            r = softmax_ref(x, ts, "masked", ignore, smooth, grad_mult, go, w, cf)
        head.append(r.sums[:2]); tail.append(r.sums[2:]); loss.append(r.loss); coef.append(r.coef); grads.append(r.grad); refs.append(r)
        total = total + w * r.loss
    return SimpleNamespace(sums=torch.cat(head + tail), loss=torch.stack([total] + loss), coef=torch.stack(coef), grads=grads, refs=refs)


def ds_finish64(sums, mode, N, S, weights, has_ignore, smooth, grad_mult):
    """du_ds_loss_finish in fp64 on any sums vector -> (loss [total, loss_s], coef (S, 2 C + 1))"""
    C = N if mode == "regions" else N - 1
    fam = ("regions_ign" if has_ignore else "regions") if mode == "regions" else "masked"
    loss, coef, total = [], [], 0.0
    for s in range(S):
        if weights[s] == 0.0:
            loss.append(torch.zeros((), dtype=torch.float64)); coef.append(torch.zeros(2 * C + 1, dtype=torch.float64))
            continue
        v = torch.cat((sums[2 * s:2 * s + 2], sums[2 * S + 3 * C * s:2 * S + 3 * C * (s + 1)])).double()
        l, cf, _ = finish64(v, fam, N, smooth, grad_mult, weights[s])
        loss.append(l); coef.append(cf)
        total = total + weights[s] * l
    return torch.stack([torch.as_tensor(total, dtype=torch.float64)] + loss), torch.stack(coef)


# ---------------------------------------------------------------------------------------------------- draws
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def labels_draw(B, K, HW, seed, empty=None, ignore_frac=0.0):
    """(B, HW) int64 labels over the classes but `empty`; ignore_frac of the pixels carry IGNORE (0 and 1 included)"""
    g = _gen(seed)
    classes = torch.tensor([k for k in range(K) if k != empty])
    t = classes[torch.randint(0, len(classes), (B, HW), generator=g)]
    if ignore_frac > 0:
        t = torch.where(torch.rand(B, HW, generator=g) < ignore_frac, torch.full_like(t, IGNORE), t)
    return t


def exact_softmax_draw(B, K, HW, seed, onehot_only=False):
    """fp32 (B, K, HW): uniform pixels (all K logits one integer in -3..3) and one-hot pixels (one class at a in -2..2, the rest a - 128)"""
    assert K in (2, 4, 8)
    g = _gen(seed)
    base = torch.randint(-3, 4, (B, 1, HW), generator=g).float()
    hot = F.one_hot(torch.randint(0, K, (B, HW), generator=g), K).permute(0, 2, 1).float()
    kind = torch.ones(B, 1, HW) if onehot_only else (torch.rand(B, 1, HW, generator=g) < 0.5).float()
    return (base - 128.0 * (1 - hot) * kind).contiguous()        # (the permuted one-hot would hand its strides to the result)


def exact_sigmoid_draw(B, R, HW, seed, onehot_only=False):
    """fp32 (B, R, HW) in {0, +-128} (onehot_only: +-128, every BCE term 0 or 128) and uint8 planes (B, R, HW)"""
    g = _gen(seed)
    vals = torch.tensor([128.0, -128.0] if onehot_only else [0.0, 128.0, -128.0])
    x = vals[torch.randint(0, len(vals), (B, R, HW), generator=g)]
    y = torch.randint(0, 2, (B, R, HW), generator=g).to(torch.uint8)
    return x, y


def mask_draw(B, HW, seed, ignore_frac):
    return torch.rand(B, HW, generator=_gen(seed)) >= ignore_frac


def general_draw(B, N, HW, seed):
    """N(0, 2^2) logits: the draw of the existing loss tests"""
    return torch.randn(B, N, HW, generator=_gen(seed)) * 2.0


def offset_draw(B, N, HW, seed, c):
    """(x + c, x): multiples of 2^-10 in [-8, 8) plus a constant that adds exactly, so the fp64 reference of x serves x + c"""
    x = torch.randint(-8192, 8192, (B, N, HW), generator=_gen(seed)).float() / 1024.0
    xc = x + c
    assert torch.equal(xc.double(), x.double() + c), "the offset does not add exactly"
    return xc, x


def extreme_softmax_draw(K=3):
    """(1, K, HW) logits and labels: for each gap one pixel whose target sits `gap` below the maximum and one whose target is the maximum
    `gap` above a wrong class; the remaining class is 1 below the maximum"""
    cols, labs = [], []
    for gap in GAPS:
        for below in (True, False):
            v = torch.full((K,), -1.0)
            v[0] = 0.0
            v[1] = -gap
            cols.append(v); labs.append(1 if below else 0)
    return torch.stack(cols, 1)[None].contiguous(), torch.tensor(labs)[None]


def extreme_sigmoid_draw():
    """(1, 1, HW) logits over SIG_X, each against both label values"""
    x = torch.tensor([v for v in SIG_X for _ in (0, 1)], dtype=torch.float32)
    y = torch.tensor([l for _ in SIG_X for l in (0, 1)], dtype=torch.uint8)
    return x[None, None].contiguous(), y[None, None].contiguous()


def exactness(sums_ref, K, family):
    """the conditions of the exact gate: the Dice sums are multiples of 1 / K below 2^24 granules, the counts below 2^24"""
    off = 1 if family == "plain" else 2
    ipg = sums_ref[off:].view(-1, 3)
    gran = 1.0 / (2 if family.startswith("regions") else K)
    for v in ipg[:, :2].reshape(-1).tolist():
        assert v / gran == round(v / gran), f"{v} is no multiple of {gran}"
        X.require_exact(v, gran)
    for v in ipg[:, 2].tolist() + ([float(sums_ref[1])] if off == 2 else []):
        assert v == round(v)
        X.require_exact(v, 1.0)


# ---------------------------------------------------------------------------------------------------- bounds
def eps_exp(a):
    """relative error of __expf(-a) = exp2(-a log2 e): the subtraction that made a rounds (u a in the exponent), so does the scaling by
    log2 e (u a), and v_exp_f32 is good to 1 ulp (2 u)"""
    return (2 * a + 2) * U


def sum_depth(family, B, HW, bwd=False):
    """additions on the longest path of a two-stage sum: a lane's trips (x 4 pixels of a quad), the wave tree (6), the block's 4 waves
    (3), a second-stage thread's rows, its tree (6 + 3; 8 for the plain one)"""
    t = trips(family, B, HW, False) * (1 if family == "plain" else 4)
    g = loss_grid(B * HW) if family == "plain" else masked_grid(quad_items(B, HW))
    return t + 9 + cdiv(g, 256) + 9


def softmax_term_err(s):
    """per pixel: E_p (B, K, HW) of p_k and E_nll (B, HW).  e_k carries eps_exp(|x_k - mx|); se = sum e_k adds K - 1 roundings, so
    d_se = sum_j p_j eps_j + (K - 1) u relative; p_k = e_k * (1 / se): division (1 ulp = 2 u) and product (u).  nll = (mx - xt) + log se:
    the difference rounds once (u |mx - xt|), log se = v_log_f32 (2 u) times ln 2 (u) of an argument off by d_se (absolute d_se in the
    logarithm), and the sum rounds (u nll)."""
    eps = eps_exp(s.a)
    dse = (s.p * eps).sum(1) + (s.K - 1) * U
    Ep = s.p * (eps + dse[:, None] + 3 * U) + TINY
    Enll = U * (s.nll - torch.log(s.se)).abs() + dse + 3 * U * torch.log(s.se) + U * s.nll
    return Ep, Enll * s.valid


def sigmoid_term_err(s):
    """E_s and E_bce per element.  e = __expf(-|x|) carries eps_exp(|x|); 1 + e rounds (u), v_rcp_f32 is 1 ulp (2 u), x < 0 multiplies by e
    (its error and u): E_s = s (eps_e ([x < 0] + e / (1 + e)) + 4 u).  bce = (max(x, 0) - x y) + log(1 + e): the first part is exact
    (y in {0, 1}); 1 + e rounds by u relative to >= 1 (absolute u in the logarithm, which also covers e < u), e's error enters as
    eps_e e, the native log is 3 u relative, the sum rounds (u bce)."""
    eps = eps_exp(s.x.abs())
    Es = s.s * (eps * ((s.x < 0).double() + s.e / (1 + s.e)) + 4 * U) + TINY
    Ebce = U * (1 + s.bce + 3 * torch.log1p(s.e)) + eps * s.e + TINY
    return Es, Ebce


def sums_bound(ref, B, HW):
    """per sum: |got - ref| <= sum of the terms' own errors + depth u sum |term| (every term is >= 0, so sum |term| is the sum itself)"""
    s, fam = ref.stats, ref.family
    base = "regions" if fam.startswith("regions") else fam
    d = sum_depth(base, B, HW) * U
    if base == "regions":
        Es, Eb = sigmoid_term_err(s)
        mf = s.m[:, None].double()
        terr = torch.stack(((Es * s.y * mf).sum((0, 2)), (Es * mf).sum((0, 2)), torch.zeros(s.K, dtype=torch.float64)), 1).reshape(-1)
        head = torch.stack(((Eb * mf).sum(), torch.zeros((), dtype=torch.float64)))
    else:
        Ep, En = softmax_term_err(s)
        vf = s.valid[:, None].double()
        terr = torch.stack(((Ep * s.oh).sum((0, 2))[1:], (Ep * vf).sum((0, 2))[1:], torch.zeros(s.K - 1, dtype=torch.float64)), 1).reshape(-1)
        head = torch.stack([En.sum()] if fam == "plain" else [En.sum(), torch.zeros((), dtype=torch.float64)])
    return torch.cat((head, terr)) + d * ref.sums.abs()


def grad_bound(ref):
    """per element, for the coefficients the reference was given (the kernel's own).  Softmax, dx = go ((p - 1[t]) scale + p (g - dot)):
      A = (p - 1[t]) scale: E_p scale + 3 u |A| (difference, product, and the plain kernel's own rounding of 1 / npix);
      g = ca 1[t] + cb: u gabs, gabs = |ca| 1[t] + |cb|;  dot = sum_j g_j p_j: E_dot = sum_j gabs_j (E_p_j + (K + 2) u p_j);
      B = p (g - dot): E_p |g - dot| + p (2 u gabs + u |dot| + E_dot) + u |B|;  the sum and the product with go: 2 u (|A| + |B|).
    Sigmoid, dx = go ((s - y) scale + (ca y + cb) s (1 - s)): A as above with E_s; c = ca y + cb (u cabs); 1 - s inherits E_s, so
      B: cabs E_s (1 - s + s) + 5 u cabs s (1 - s)."""
    s, pt, go = ref.stats, ref.parts, abs(ref.go)
    if ref.family.startswith("regions"):
        Es, _ = sigmoid_term_err(s)
        EA = Es * abs(ref.scale) + 3 * U * pt.A.abs()
        EB = pt.cabs * Es + 5 * U * pt.cabs * s.s * (1 - s.s)
        return go * (EA + EB + 2 * U * (pt.A.abs() + pt.B.abs())) * s.m[:, None].double()
    Ep, _ = softmax_term_err(s)
    EA = Ep * abs(ref.scale) + 3 * U * pt.A.abs()
    Edot = (pt.gabs * (Ep + (s.K + 2) * U * s.p)).sum(1, keepdim=True)
    EB = Ep * (pt.g - pt.dot).abs() + s.p * (2 * U * pt.gabs + U * pt.dot.abs() + Edot) + U * pt.B.abs()
    return go * (EA + EB + 2 * U * (pt.A.abs() + pt.B.abs())) * s.valid[:, None].double()


def finish_bound(sums, family, N, smooth, grad_mult, weight=1.0, npix=None):
    """few ulp, for any sums vector -> (loss64, coef64, loss bound, coef bound).  A coefficient is at most 11 roundings from the sums
    (num 2, den 2, den^2 3, the quotient, 1 / C and two products; the scale entry 3): 12 u relative.  The loss: the scale (2) and its
    product with the CE sum (1) and the final difference (1), 4 u |CE scale|; C quotients of 5 roundings each, their sum (C) and the
    division by C, (8 + C) u mean |dc|; the difference, u |loss|."""
    loss, coef, _ = finish64(sums, family, N, smooth, grad_mult, weight, npix)
    off = 1 if family == "plain" else 2
    ipg = sums.double()[off:].view(-1, 3)
    C = ipg.shape[0]
    dcs = ((2 * ipg[:, 0] + smooth) / (ipg[:, 1] + ipg[:, 2] + smooth).clamp_min(CLIP)).abs().sum() / C
    ce = (loss + dice_coefs64(ipg, smooth, 1.0)[0]).abs()
    return loss, coef, U * (4 * ce + (8 + C) * dcs + loss.abs()), 12 * U * coef.abs()


def torch_nll_error(x, t, ignore=None):
    """the figure the per-voxel bound comes from: worst |torch fp32 cross_entropy - fp64| on this draw"""
    ii = -100 if ignore is None else ignore
    v32 = F.cross_entropy(x.float().unsqueeze(-1), t.unsqueeze(-1), reduction="none", ignore_index=ii)
    v64 = F.cross_entropy(x.double().unsqueeze(-1), t.unsqueeze(-1), reduction="none", ignore_index=ii)
    return float((v32.double() - v64).abs().max())


def nll_bound(x, t, ignore=None):
    """per-voxel NLL: 4 x the reference's own fp32 error on the same draw (measured, see the module docstring)"""
    return 4 * torch_nll_error(x, t, ignore)


def topk_separated(nll64, k_vox, bound):
    """(selection (flat bool), decided (flat bool)) of the fp64 top-k: a voxel is decided when its value is more than 2 x bound away from
    the k-th largest; the others may fall either way"""
    v = nll64.reshape(-1)
    thr = torch.topk(v, k_vox).values[-1]
    return v > thr, (v - thr).abs() > 2 * bound


# ---------------------------------------------------------------------------------------------------- gates
def within(got, ref, bound):
    got = got.detach().cpu().double()
    return bool(torch.isfinite(got).all()) and bool(((got - ref).abs() <= bound).all())


def assert_within(got, ref, bound, what=""):
    got = got.detach().cpu().double().reshape(ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite values {got[~torch.isfinite(got)][:4].tolist()}"
    ex = (got - ref).abs() - bound
    if bool((ex > 0).any()):
        i = int(ex.argmax())
        raise AssertionError(f"{what}: {int((ex > 0).sum())} of {ex.numel()} outside the bound; worst at flat index {i}: got "
                             f"{float(got.flatten()[i])!r}, want {float(ref.flatten()[i])!r}, bound {float(torch.as_tensor(bound).expand(ref.shape).flatten()[i]):.3e}")


def share(got, ref, bound):
    """worst |got - ref| / bound over the elements with a non-zero bound (recorded for information, never a gate)"""
    got = got.detach().cpu().double().reshape(ref.shape)
    b = torch.as_tensor(bound, dtype=torch.float64).expand(ref.shape)
    k = b > 0
    return float(((got - ref).abs()[k] / b[k]).max()) if bool(k.any()) else 0.0


def exact_sums_ok(got, ref, family, ce_exact, ce_bound=None):
    """G, n_valid, I and P to the bit; CE / BCE to the bit where every pixel is one-hot, else inside ce_bound"""
    got = got.detach().cpu()
    want = ref.sums.float()
    if not torch.equal(got[1:], want[1:]):
        return False
    return torch.equal(got[:1], want[:1]) if ce_exact else within(got[:1], ref.sums[:1], ce_bound)


def grad_ok(got, ref, bound=None):
    """every element inside its bound (exact draws: pass bound=None for bit equality is NOT meant; the closed form is compared), ignored
    pixels exactly 0, nothing left at the sentinel"""
    got = got.detach().cpu()
    if bool((got == X.SENTINEL).any()):
        return False
    s = ref.stats
    live = (s.m if ref.family.startswith("regions") else s.valid)[:, None].expand(got.shape)
    if bool((got[~live] != 0).any()):
        return False
    return within(got, ref.grad, grad_bound(ref) if bound is None else bound)


# ---------------------------------------------------------------------------------------------------- emulations (fp32, the kernels' own order)
def _wave_tree(v):
    """v (..., 64, NS) -> lane 0 of the xor butterfly 32, 16, .. 1"""
    idx = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., idx ^ o, :]
    return v[..., 0, :]


def _block_rows(lane_acc, grid):
    """lane_acc (grid * 256, NS) -> partial rows (grid, NS): wave trees, then waves 0..3 in sequence"""
    w = _wave_tree(lane_acc.view(grid, 4, 64, -1))
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def _rows_sum(part, tree256):
    """ONE block adds the rows: thread t takes rows t, t + 256, ..; then the 256-entry LDS tree (plain) or wave tree + 4 waves"""
    g, ns = part.shape
    pad = torch.zeros(cdiv(g, 256) * 256, ns)
    pad[:g] = part
    acc = torch.zeros(256, ns)
    for r in pad.view(-1, 256, ns):
        acc = acc + r
    if tree256:
        o = 128
        while o > 0:
            acc = torch.cat((acc[:o] + acc[o:2 * o], acc[o:]))
            o >>= 1
        return acc[0]
    return _block_rows(acc, 1)[0]


def emu_reduce(terms, HW, family, cap, mutant=None):
    """terms (B, HW, NS) fp32 -> sums (NS) as the two-stage reduction of the family forms them"""
    B, _, ns = terms.shape
    if family == "plain":
        n = B * HW
        grid = loss_grid(n, cap)
        L = grid * 256
        T = cdiv(n, L)
        it = torch.zeros(T * L, 1, ns)
        it[:n, 0] = terms.reshape(n, ns)
    else:
        nq = cdiv(HW, 4)
        t4 = torch.zeros(B, nq * 4, ns)
        t4[:, :HW] = terms
        if mutant == "drop_partial_quad" and HW % 4:
            t4[:, (nq - 1) * 4:] = 0
        n = B * nq
        grid = masked_grid(n, cap)
        L = grid * 256
        T = cdiv(n, L)
        it = torch.zeros(T * L, 4, ns)
        it[:n] = t4.view(n, 4, ns)
    it = it.view(T, L, -1, ns)
    acc = torch.zeros(L, ns)
    for tr in range(T):
        reps = 0 if (mutant == "drop_trip" and tr == 1) else (2 if (mutant == "dup_trip" and tr == 1) else 1)
        for _ in range(reps):
            for j in range(it.shape[2]):
                acc = acc + it[tr, :, j]
    return _rows_sum(_block_rows(acc, grid), family == "plain"), T


def _f32(v):
    return torch.tensor(v, dtype=torch.float32)


def emu_dice_coefs(ipg, smooth, mult, mutant=None):
    """dice_coefs in fp32, operation by operation -> (dc mean, coef pairs)"""
    C = ipg.shape[0]
    invc = _f32(1.0) / _f32(float(C))
    sm, gm = _f32(smooth), _f32(mult)
    dc, coef = _f32(0.0), []
    for c in range(C):
        I, P, G = ipg[c]
        num, raw = _f32(2.0) * I + sm, G + P + sm
        den = torch.maximum(raw, _f32(1e-8))
        dc = dc + num / den
        coef.append(_f32(-2.0) * invc / den * gm)
        d2 = den if mutant == "cb_den" else den * den
        coef.append((num / d2 * invc if bool(raw > _f32(1e-8)) else _f32(0.0)) * gm)
    return dc / _f32(float(C)), torch.stack(coef)


def emu_softmax(x, t, family="plain", ignore=None, smooth=1e-5, grad_mult=1.0, go=1.0, weight=1.0, caps=(2048, 8192), mutant=None,
                form="good"):
    """one scale of Dice + CE in fp32.  form: "good" (mx - xt) + log se | "lse" (mx + log se) - xt | "sat" -log(max(p_t, 1e-38)).
    -> sums, loss, coef, grad (sentinel where a mutant writes nothing), nll"""
    x = x.float()
    B, K, HW = x.shape
    valid = (t != ignore) if (ignore is not None and family != "plain") else torch.ones_like(t, dtype=torch.bool)
    tt = torch.where(valid, t, torch.zeros_like(t))
    mx = x.amax(1)
    e = torch.exp(x - mx[:, None])
    se = torch.zeros_like(mx)
    for k in range(K):
        se = se + e[:, k]
    p = e * (1.0 / se)[:, None]
    xt = x.gather(1, tt[:, None])[:, 0]
    if form == "good":
        nll = (mx - xt) + torch.log(se)
    elif form == "lse":
        nll = (mx + torch.log(se)) - xt
    else:
        nll = -torch.log(p.gather(1, tt[:, None])[:, 0].clamp_min(1e-38))
    vf = valid.float()
    nll = nll * vf
    oh = F.one_hot(tt, K).permute(0, 2, 1).float() * vf[:, None]
    pv = p if mutant == "ignored_in_P" else p * vf[:, None]
    cols = [nll] if family == "plain" else [nll, vf]
    for k in range(1, K):
        cols += [p[:, k] * oh[:, k], pv[:, k], oh[:, k]]
    sums, T = emu_reduce(torch.stack(cols, 2), HW, family, caps[0], mutant)
    off = 1 if family == "plain" else 2
    dc, pairs = emu_dice_coefs(sums[off:].view(-1, 3), smooth, grad_mult * (1.0 if mutant == "ds_weight_dropped" else weight), mutant)
    if family == "plain" or mutant == "ce_all_pixels":
        scale = _f32(1.0) / _f32(float(B * HW))
    else:
        scale = _f32(1.0) / sums[1] if bool(sums[1] > 0) else _f32(0.0)
    loss = sums[0] * scale - dc
    sw = scale * _f32(weight)
    coef = pairs if family == "plain" else torch.cat((pairs, sw[None]))
    ca = torch.cat((torch.zeros(1), pairs[0::2] * (1.0 if mutant != "grad_mult_dropped" else 1.0 / grad_mult)))
    cb = torch.cat((torch.zeros(1), pairs[1::2] * (1.0 if mutant != "grad_mult_dropped" else 1.0 / grad_mult)))
    ohf = F.one_hot(tt, K).permute(0, 2, 1).float()
    g = ca[None, :, None] * ohf + cb[None, :, None]
    dot = torch.zeros_like(mx)
    for k in range(K):
        dot = dot + g[:, k] * p[:, k]
    if mutant == "no_dot":
        dot = torch.zeros_like(dot)
    grad = _f32(go) * ((p - ohf) * sw + p * (g - dot[:, None])) * vf[:, None]
    grad = _bwd_trips(grad, HW, family, caps[1], mutant)
    return SimpleNamespace(sums=sums, loss=loss, coef=coef, grad=grad, nll=nll, trips=T)


def _bwd_trips(grad, HW, family, cap, mutant):
    """bwd_drop_trip: the pixels of the second grid-stride trip of the backward pass keep the sentinel"""
    if mutant != "bwd_drop_trip":
        return grad
    B, N, _ = grad.shape
    grad = grad.clone()
    if family == "plain":
        lo = plain_bwd_grid(B * HW, cap) * 256
        flat = grad.permute(0, 2, 1).reshape(B * HW, N)
        flat[lo:2 * lo] = X.SENTINEL
        return flat.view(B, HW, N).permute(0, 2, 1).contiguous()
    nq = cdiv(HW, 4)
    lo = elem_grid(B * nq, cap) * 256
    for item in range(lo, min(2 * lo, B * nq)):
        b, q = divmod(item, nq)
        grad[b, :, 4 * q:4 * q + 4] = X.SENTINEL
    return grad


def emu_sigmoid(x, y, m, has_ignore, smooth=1e-5, grad_mult=1.0, go=1.0, weight=1.0, caps=(2048, 8192), mutant=None):
    """one scale of Dice + BCE in fp32 (sigmoid_bce's one exponential, the quad reduction, dice_coefs, the backward line)"""
    x, yf, mf = x.float(), y.float(), m.float()[:, None]
    B, R, HW = x.shape
    e = torch.exp(-x.abs())
    inv = 1.0 / (1.0 + e)
    s = torch.where(x >= 0, inv, e * inv)
    bce = x.clamp_min(0) - x * yf + torch.log(1.0 + e)
    bsum = torch.zeros(B, HW)
    for r in range(R):
        bsum = bsum + bce[:, r] * mf[:, 0]          # (the kernel adds region by region into the same lane accumulator)
    cols = [bsum, mf[:, 0]]
    for r in range(R):
        cols += [s[:, r] * yf[:, r] * mf[:, 0], s[:, r] * mf[:, 0], yf[:, r] * mf[:, 0]]
    sums, T = emu_reduce(torch.stack(cols, 2), HW, "regions", caps[0], mutant)
    dc, pairs = emu_dice_coefs(sums[2:].view(-1, 3), smooth, grad_mult * (1.0 if mutant == "ds_weight_dropped" else weight), mutant)
    per_elem = (not has_ignore) or mutant == "bce_nvalid_R"
    scale = (_f32(1.0) / (sums[1] * _f32(float(R)) if per_elem else sums[1])) if bool(sums[1] > 0) else _f32(0.0)
    loss = sums[0] * scale - dc
    sw = scale * _f32(weight)
    ca, cb = pairs[0::2][None, :, None], pairs[1::2][None, :, None]
    grad = _f32(go) * ((s - yf) * sw + (ca * yf + cb) * s * (1.0 - s)) * mf
    grad = _bwd_trips(grad, HW, "regions", caps[1], mutant)
    return SimpleNamespace(sums=sums, loss=loss, coef=torch.cat((pairs, sw[None])), grad=grad, nll=None, trips=T)


def emu_ds(outs, t, H, W, mode, weights, table=None, ignore=None, smooth=1e-5, grad_mult=1.0, go=1.0, mutant=None):
    """deep supervision in fp32: every active scale through its body on the gathered target, the sums layout, total in scale order"""
    S = len(weights)
    N = next(o for o in outs if o is not None).shape[1]
    C = N if mode == "regions" else N - 1
    head, tail, loss, coef, grads = [], [], [], [], []
    total = _f32(0.0)
    for si, (o, w) in enumerate(zip(outs, weights)):
        if w == 0.0:
            head.append(torch.zeros(2)); tail.append(torch.zeros(3 * C)); loss.append(_f32(0.0)); coef.append(torch.zeros(2 * C + 1))
            grads.append(None)
            continue
        h, wd = o.shape[-2:]
        ts = ds_target(t, H, W, h, wd, "ds_floor_index" if mutant == "ds_floor_index" else None)
        xx = o.reshape(o.shape[0], N, h * wd)
        mu = mutant if (mutant != "ds_weight_dropped" or si == 1) else None
        if mode == "regions":
            y, m = region_planes(ts, table, ignore)
            r = emu_sigmoid(xx, y, m, ignore is not None, smooth, grad_mult, go, w, mutant=mu)
        else:
            r = emu_softmax(xx, ts, "masked", ignore, smooth, grad_mult, go, w, mutant=mu)
        head.append(r.sums[:2]); tail.append(r.sums[2:]); loss.append(r.loss); coef.append(r.coef); grads.append(r.grad)
        total = total + _f32(w) * r.loss
    return SimpleNamespace(sums=torch.cat(head + tail), loss=torch.stack([total] + loss), coef=torch.stack(coef), grads=grads)


# ---------------------------------------------------------------------------------------------------- shape lists of the GPU module
K_ALL, R_ALL = (2, 3, 4, 5, 6, 7, 8), (1, 2, 3, 4, 5, 6, 7, 8)
INST_SHAPE = (2, 5, 7)                                  # (B, H, W): HW = 35, quads straddle the image boundary
QUAD_HW = (1, 2, 3, 4, 5, 7, 8)                         # with B = 3
GRAD_SHAPES = ((2, 3, 17, 23), (3, 4, 48, 40), (1, 8, 32, 32))
GO_SMOOTH_MULT = ((1.7, 1e-5, 1.0), (-0.5, 1.0, 2.0), (0.0, 0.0, 1.0), (None, 1e-5, 2.0))
EXACT_K, EXACT_R = (2, 4, 8), (1, 2, 8)
EXACT_SHAPE = (3, 19, 21)                               # (B, H, W): HW = 399, odd
IGNORE_FRACS = (0.0, 0.3, 1.0)
DS_EXACT = ((18, 10), (9, 5), (5, 3))                   # three scales, non-dyadic zoom 9 -> 5, 5 -> 3
PLAIN_BIG = (1, 1449, 1449)                             # 2 099 601 pixels > 2 097 152
QUAD_BIG_VEC = (2, 2048, 2052)                          # 2 101 248 quads > 2 097 152
QUAD_BIG_ODD = (1, 2899, 2901)                          # HW odd, 2 102 500 quads
DS_BIG_SMALL = (5, 7)                                   # the second scale behind 8192 blocks
OFFSET_SHAPE = (2, 3, 100, 100)
