"""Keeps tests/_loss_ref.py honest without a GPU: the fp64 restatements against the package's torch formulas, their autograd and the
committed fixtures; the exactness conditions and regime predicates for every entry of the GPU module's shape lists; the honest fp32
emulation of each family inside every gate, and each mutant rejected by the gate meant for it."""
import os

import numpy as np
import pytest
import torch

import _exact as X
import _loss_ref as R
from dinounet_amd import training as T

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REGIONS3 = [(1, 2, 3), (2, 3), 3]
CAPS = (1, 1)                 # launch caps of the emulations: one block, so 3 x 1203 pixels take 4 quad trips in either pass


def close(a, b, tol=1e-12):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def autograd_of(fn, x4):
    x = x4.double().requires_grad_(True)
    l = fn(x)
    g, = torch.autograd.grad(l, x)
    return l.detach(), g


# ---------------------------------------------------------------------------------------------------- restatements
@pytest.mark.parametrize("K,smooth", [(2, 1e-5), (3, 1.0), (8, 0.0)])
def test_plain_and_masked_restatements_equal_training(K, smooth):
    B, H, W = 2, 9, 7
    x = R.general_draw(B, K, H * W, 3 + K)
    for frac in (None, 0.0, 0.3, 1.0):
        t = R.labels_draw(B, K, H * W, 5 + K, ignore_frac=frac or 0.0)
        ign = None if frac is None else R.IGNORE
        l, g = autograd_of(lambda v: T.dc_and_ce_loss(v, t.view(B, 1, H, W), smooth, ddp=False, ignore_label=ign), x.view(B, K, H, W))
        r = R.softmax_ref(x, t, "plain" if ign is None else "masked", ign, smooth)
        assert close(r.loss, l) and close(r.grad, g.view(B, K, -1)), (K, frac)
        # the coefficient vector is the derivative the closed form uses: grad_mult and go scale the gradient linearly
        r2 = R.softmax_ref(x, t, "plain" if ign is None else "masked", ign, smooth, grad_mult=1.0, go=-0.5)
        assert close(r2.grad, -0.5 * g.view(B, K, -1))


@pytest.mark.parametrize("Rn,ign", [(1, False), (3, True), (8, False), (5, True)])
def test_region_restatement_equals_training(Rn, ign):
    B, H, W = 2, 6, 5
    x = R.general_draw(B, Rn, H * W, 20 + Rn)
    _, y = R.exact_sigmoid_draw(B, Rn, H * W, 21 + Rn)
    for frac in ((0.0, 0.3, 1.0) if ign else (0.0,)):
        m = R.mask_draw(B, H * W, 22, frac)
        tgt = torch.cat((y, (~m)[:, None].to(torch.uint8)), 1) if ign else y
        l, g = autograd_of(lambda v: T.dc_and_bce_loss(v, tgt.view(B, -1, H, W), ign, 1e-5, ddp=False), x.view(B, Rn, H, W))
        r = R.sigmoid_ref(x, y, m, ign)
        assert close(r.loss, l) and close(r.grad, g.view(B, Rn, -1)), (Rn, frac)


@pytest.mark.parametrize("mode", ["softmax", "softmax_ignore", "regions"])
def test_deep_supervision_restatement_equals_wrapper(mode):
    B, (H, W) = 2, R.DS_EXACT[0]
    N = 3
    weights = (4 / 7, 2 / 7, 1 / 7, 0.0)
    shapes = list(R.DS_EXACT) + [(2, 2)]
    outs = [R.general_draw(B, N, h * w, 30 + i).view(B, N, h, w) for i, (h, w) in enumerate(shapes)]
    ign = None if mode == "softmax" else 4
    t = R.labels_draw(B, N + 1 if mode == "regions" else N, H * W, 31)
    if ign is not None:
        t = torch.where(R.mask_draw(B, H * W, 32, 0.3), t, torch.full_like(t, ign))
    base = T.SegLoss(N, regions=REGIONS3 if mode == "regions" else None, ignore_label=ign, ddp=False)
    ds = T.DeepSupervisionLoss(base, weights)
    xs = [o.double().requires_grad_(True) for o in outs]
    l = ds.composed(xs, t.view(B, 1, H, W))
    gs = torch.autograd.grad(l, xs[:3])
    r = R.ds_ref([o if w else None for o, w in zip(outs, weights)], t, H, W, "regions" if mode == "regions" else "softmax", weights,
                 table=T._region_masks(REGIONS3), ignore=ign)
    assert close(r.loss[0], l.detach())
    for s in range(3):
        assert close(r.grads[s], gs[s].reshape(B, N, -1)), s
    assert r.grads[3] is None and float(r.loss[4]) == 0.0
    assert torch.equal(R.ds_src_index(18, 148), T.ds_target_index(18, 148))


def test_floor_of_the_shifted_coordinate_is_the_same_index():
    """floor((i + 0.5) z) is the index formula with its -0.5 and +0.5 cancelled: it picks the same source index for every pair of sizes
    below 200, so it is no mutant a gate could reject; the emulations' wrong index is floor(i z)"""
    for n in range(2, 200):
        for m in range(1, n):
            alt = torch.floor((torch.arange(m, dtype=torch.float64) + 0.5) * (n / m)).long().clamp(max=n - 1)
            assert torch.equal(R.ds_src_index(m, n), alt), (n, m)


def test_per_voxel_nll_equals_topk_formula():
    B, K, HW = 2, 4, 60
    x = R.general_draw(B, K, HW, 40)
    t = R.labels_draw(B, K, HW, 41, ignore_frac=0.2)
    r = R.softmax_ref(x, t, "masked", R.IGNORE)
    v = torch.nn.functional.cross_entropy(x.double().unsqueeze(-1), t.unsqueeze(-1), reduction="none", ignore_index=R.IGNORE)[..., 0]
    assert close(r.nll, v)
    l = T.topk_ce_loss(x.double().view(B, K, 6, 10), t.view(B, 1, 6, 10), 10, ignore_label=R.IGNORE)
    assert close(torch.topk(r.nll.reshape(-1), T.topk_voxels(B * HW, 10)).values.mean(), l)


def test_restatements_equal_the_committed_fixtures():
    z = np.load(os.path.join(GOLD, "seg_loss_reference.npz"))
    for case, K in (("ce_ignore", 4), ("ce_all_ignored", 3)):
        x = torch.from_numpy(z[case + "/logits"])
        B, _, H, W = x.shape
        t = torch.from_numpy(z[case + "/labels"].astype(np.int64)).view(B, -1)
        ign = int(t.max())
        r = R.softmax_ref(x.view(B, K, -1), t, "masked", ign)
        assert close(r.loss, float(z[case + "/loss"]), 1e-9) and close(r.grad, torch.from_numpy(z[case + "/grad"]).view(B, K, -1), 1e-9), case
    for case, ign in (("regions_ignore", True), ("regions_tail", False)):
        x = torch.from_numpy(z[case + "/logits"])
        B, Rn, H, W = x.shape
        oh = torch.from_numpy(z[case + "/onehot"]).view(B, -1, H * W)
        m = oh[:, Rn] == 0 if ign else torch.ones(B, H * W, dtype=torch.bool)
        r = R.sigmoid_ref(x.view(B, Rn, -1), oh[:, :Rn], m, ign)
        assert close(r.loss, float(z[case + "/loss"]), 1e-9) and close(r.grad, torch.from_numpy(z[case + "/grad"]).view(B, Rn, -1), 1e-9), case
    z = np.load(os.path.join(GOLD, "deep_supervision_reference.npz"))
    x0 = torch.from_numpy(z["ds_plain/logits0"])
    B, K, H, W = x0.shape
    outs = [x0, torch.from_numpy(z["ds_plain/logits1"]), None]
    t = torch.from_numpy(z["ds_plain/labels"].astype(np.int64)).view(B, -1)
    r = R.ds_ref(outs, t, H, W, "softmax", T.deep_supervision_weights(3))
    assert close(r.loss[0], float(z["ds_plain/loss"]), 1e-9)
    assert close(r.grads[0], torch.from_numpy(z["ds_plain/grad0"]).view(B, K, -1), 1e-9)
    assert close(r.grads[1], torch.from_numpy(z["ds_plain/grad1"]).view(B, K, -1), 1e-9)


# ---------------------------------------------------------------------------------------------------- conditions and regimes
def test_regimes_of_every_gpu_shape():
    B, H, W = R.PLAIN_BIG
    assert B * H * W == 2_099_601 and R.past_clamp("plain", B, H * W, False) and R.past_clamp("plain", B, H * W, True)
    assert R.trips("plain", B, H * W, True) == 2 and R.trips("plain", B, H * W, False) == 5
    for fam in ("masked", "regions"):
        B, H, W = R.QUAD_BIG_VEC
        assert R.vec(H * W, True) and R.quad_items(B, H * W) == 2_101_248
        assert R.trips(fam, B, H * W, True) == 2 and R.past_clamp(fam, B, H * W, False)
        B, H, W = R.QUAD_BIG_ODD
        assert not R.vec(H * W, True) and (H * W) % 2 == 1 and R.quad_items(B, H * W) == 2_102_500
        assert R.trips(fam, B, H * W, True) == 2 and R.past_clamp(fam, B, H * W, False)
    # the shape the existing tests stop at sits exactly at the plain caps and under the quad ones
    assert not R.past_clamp("plain", 8, 512 * 512, False) and not R.past_clamp("plain", 8, 512 * 512, True)
    assert not R.past_clamp("masked", 8, 512 * 512, False) and not R.past_clamp("masked", 8, 512 * 512, True)
    # deep supervision: the small scale's blocks sit behind the 8192 (backward) / 2048 (sums) of the full-resolution scale
    B, H, W = R.QUAD_BIG_VEC
    tab, total = R.ds_table(B, [(H, W), R.DS_BIG_SMALL], (0.5, 0.5), True)
    assert tab[0] == (0, 8192) and tab[1] == (8192, 1) and total == 8193
    tab, _ = R.ds_table(B, [(H, W), R.DS_BIG_SMALL, (2, 2)], (0.5, 0.0, 0.5), False)
    assert tab == [(0, 2048), (0, 0), (2048, 1)]
    # quad edges: a partial last quad exists exactly where HW % 4 != 0; misaligned pointers alone switch the vector path off
    for hw in R.QUAD_HW:
        assert R.vec(hw, True) == (hw % 4 == 0) and not R.vec(hw, True, False)
    b, h, w = R.INST_SHAPE
    assert (h * w) % 4 == 3 and R.quad_items(b, h * w) == 18
    b, h, w = R.EXACT_SHAPE
    assert (h * w) % 4 != 0 and R.masked_grid(R.quad_items(b, h * w)) == 1
    for B, N, H, W in R.GRAD_SHAPES:
        assert R.trips("masked", B, H * W, True) == 1
    assert R.ws_elems("plain", 2, 3, 35) == 7 and R.ws_elems("masked", 2, 3, 35) == 8 and R.ws_elems("regions", 2, 3, 35) == 11


@pytest.mark.parametrize("big", [False, True])
def test_exactness_conditions_of_every_exact_shape(big):
    """the draws of the exact-sums and past-the-clamp tests satisfy the conditions that make fp32 sums exact in any order; every class
    has hits and misses, the empty class none"""
    if big:
        cases = [("plain", R.PLAIN_BIG, 2), ("masked", R.QUAD_BIG_VEC, 2), ("masked", R.QUAD_BIG_ODD, 2)]
    else:
        cases = [(f, R.EXACT_SHAPE, K) for f in ("plain", "masked") for K in R.EXACT_K]
    for fam, (B, H, W), K in cases:
        x = R.exact_softmax_draw(B, K, H * W, 7)
        t = R.labels_draw(B, K, H * W, 8, empty=(K - 1 if K > 2 else None), ignore_frac=0.3 if fam == "masked" else 0.0)
        r = R.softmax_ref(x, t, fam, R.IGNORE)
        R.exactness(r.sums, K, fam)
        ipg = r.sums[(1 if fam == "plain" else 2):].view(-1, 3)
        if K > 2:
            assert float(ipg[-1, 2]) == 0 and float(ipg[-1, 0]) == 0
        assert bool((ipg[:K - 2 if K > 2 else 1, 0] > 0).all()) and bool((ipg[:, 1] > ipg[:, 0]).all())
    for (B, H, W), Rn in ([(R.QUAD_BIG_VEC, 1), (R.QUAD_BIG_ODD, 1)] if big else [(R.EXACT_SHAPE, r) for r in R.EXACT_R]):
        x, y = R.exact_sigmoid_draw(B, Rn, H * W, 9)
        r = R.sigmoid_ref(x, y, R.mask_draw(B, H * W, 10, 0.3), True)
        R.exactness(r.sums, 2, "regions")
    # one-hot draws: every CE / BCE term is 0 or 128
    r = R.softmax_ref(R.exact_softmax_draw(2, 4, 99, 1, onehot_only=True), R.labels_draw(2, 4, 99, 2), "plain")
    assert set(r.nll.float().reshape(-1).tolist()) == {0.0, 128.0}
    x, y = R.exact_sigmoid_draw(2, 2, 99, 3, onehot_only=True)
    assert set(R.sigmoid_stats(x, y, None).bce.float().reshape(-1).tolist()) == {0.0, 128.0}


def test_offsets_add_exactly_and_the_reference_error_does_not_grow():
    B, K, H, W = R.OFFSET_SHAPE
    t = R.labels_draw(B, K, H * W, 6)
    figs = []
    for c in R.OFFSETS:
        xc, x = R.offset_draw(B, K, H * W, 5, c)
        figs.append(R.torch_nll_error(xc, t))
        assert close(R.softmax_ref(xc, t).nll, R.softmax_ref(x, t).nll, 1e-13)
    print("torch fp32 cross_entropy against fp64, worst per voxel, per offset:", figs)
    assert max(figs) <= 1.5 * min(figs) and max(figs) < 2e-6
    # with k = 10 % the voxels the selection gate has to leave open stay far below 1 %
    xc, x = R.offset_draw(B, K, H * W, 5, 1024.0)
    r = R.softmax_ref(x, t)
    _, decided = R.topk_separated(r.nll, T.topk_voxels(B * H * W, 10), R.nll_bound(xc, t))
    assert 1 - float(decided.double().mean()) < 0.01


# ---------------------------------------------------------------------------------------------------- emulations and mutants
def soft_case(family, K=4, HW=1203, B=3, exact=False, seed=50, frac=0.3, onehot=False):
    x = R.exact_softmax_draw(B, K, HW, seed, onehot) if exact else R.general_draw(B, K, HW, seed)
    t = R.labels_draw(B, K, HW, seed + 1, ignore_frac=frac if family == "masked" else 0.0)
    return x, t


def soft_gates(em, x, t, family, **kw):
    """(sums inside their bounds, gradient gate) of an emulated run against the fp64 restatement; the gradient reference takes the run's
    own coefficients, as the GPU module does"""
    B, _, HW = x.shape
    r = R.softmax_ref(x, t, family, R.IGNORE, **kw)
    rg = R.softmax_ref(x, t, family, R.IGNORE, coef=em.coef, **kw)
    _, cf, lb, cb = R.finish_bound(em.sums, family, x.shape[1], kw.get("smooth", 1e-5), kw.get("grad_mult", 1.0), npix=t.numel())
    return SimpleGates(sums=R.within(em.sums, r.sums, R.sums_bound(r, B, HW)), grad=R.grad_ok(em.grad, rg),
                       coef=R.within(em.coef, cf, cb), ref=r)


class SimpleGates:
    def __init__(self, **kw):
        self.__dict__.update(kw)


@pytest.mark.parametrize("family", ["plain", "masked"])
def test_honest_softmax_emulation_passes_every_gate(family):
    x, t = soft_case(family)
    em = R.emu_softmax(x, t, family, R.IGNORE, caps=CAPS, go=1.7, grad_mult=2.0)
    assert em.trips >= 3
    g = soft_gates(em, x, t, family, go=1.7, grad_mult=2.0)
    assert g.sums and g.grad and g.coef
    assert R.within(em.nll, g.ref.nll, R.nll_bound(x, t, R.IGNORE if family == "masked" else None))
    xe, te = soft_case(family, exact=True)
    ee = R.emu_softmax(xe, te, family, R.IGNORE, caps=CAPS)
    re = R.softmax_ref(xe, te, family, R.IGNORE)
    R.exactness(re.sums, 4, family)
    assert R.exact_sums_ok(ee.sums, re, family, False, R.sums_bound(re, 3, 1203)[:1])
    xo, to = soft_case(family, exact=True, onehot=True)
    assert R.exact_sums_ok(R.emu_softmax(xo, to, family, R.IGNORE, caps=CAPS).sums, R.softmax_ref(xo, to, family, R.IGNORE), family, True)


@pytest.mark.parametrize("mutant", ["drop_partial_quad", "drop_trip", "dup_trip", "ignored_in_P"])
def test_exact_sums_gate_rejects(mutant):
    x, t = soft_case("masked", exact=True)
    em = R.emu_softmax(x, t, "masked", R.IGNORE, caps=CAPS, mutant=mutant)
    r = R.softmax_ref(x, t, "masked", R.IGNORE)
    assert not R.exact_sums_ok(em.sums, r, "masked", False, R.sums_bound(r, 3, 1203)[:1])
    if mutant in ("drop_trip", "dup_trip"):
        xp, tp = soft_case("plain", exact=True)
        rp = R.softmax_ref(xp, tp, "plain")
        assert not R.exact_sums_ok(R.emu_softmax(xp, tp, "plain", caps=CAPS, mutant=mutant).sums, rp, "plain", False, R.sums_bound(rp, 3, 1203)[:1])


def test_finish_gate_rejects_ce_over_all_pixels_and_cb_with_den():
    x, t = soft_case("masked")
    for mutant in ("ce_all_pixels", "cb_den"):
        em = R.emu_softmax(x, t, "masked", R.IGNORE, mutant=mutant)
        l64, cf, lb, cb = R.finish_bound(em.sums, "masked", 4, 1e-5, 1.0)
        assert not (R.within(em.loss, l64, lb) and R.within(em.coef, cf, cb)), mutant
    em = R.emu_softmax(x, t, "masked", R.IGNORE)
    l64, cf, lb, cb = R.finish_bound(em.sums, "masked", 4, 1e-5, 1.0)
    assert R.within(em.loss, l64, lb) and R.within(em.coef, cf, cb)


def test_extremes_gate_rejects_the_saturating_form():
    x, t = R.extreme_softmax_draw()
    r = R.softmax_ref(x, t)
    b = R.sums_bound(r, 1, x.shape[2])
    good, sat = R.emu_softmax(x, t), R.emu_softmax(x, t, form="sat")
    assert R.within(good.sums, r.sums, b)
    assert not R.within(sat.sums, r.sums, b)
    assert abs(float(sat.nll.max()) - 87.498) < 0.3          # what the clamp at 1e-38 makes of every gap above ~87.3


def test_per_voxel_gate_rejects_the_offset_losing_form():
    B, K, H, W = R.OFFSET_SHAPE
    t = R.labels_draw(B, K, H * W, 6)
    xc, x = R.offset_draw(B, K, H * W, 5, 1024.0)
    r = R.softmax_ref(x, t)
    bound = R.nll_bound(xc, t)
    assert R.within(R.emu_softmax(xc, t).nll, r.nll, bound)
    assert not R.within(R.emu_softmax(xc, t, form="lse").nll, r.nll, bound)


@pytest.mark.parametrize("mutant", ["no_dot", "grad_mult_dropped", "bwd_drop_trip"])
def test_gradient_gate_rejects(mutant):
    for family in ("plain", "masked"):
        x, t = soft_case(family)
        em = R.emu_softmax(x, t, family, R.IGNORE, caps=CAPS, grad_mult=2.0, mutant=mutant)
        if mutant == "grad_mult_dropped":      # the coefficients are right, the backward line forgot the factor: compare with the fp64 ones
            r = R.softmax_ref(x, t, family, R.IGNORE, grad_mult=2.0)
            assert not R.grad_ok(em.grad, r, 2 * R.grad_bound(r) + 12 * R.U * r.grad.abs())
        else:
            assert not soft_gates(em, x, t, family, grad_mult=2.0).grad


@pytest.mark.parametrize("ign", [False, True])
def test_sigmoid_emulation_and_its_mutants(ign):
    B, Rn, HW = 3, 3, 1203
    x = R.general_draw(B, Rn, HW, 60)
    _, y = R.exact_sigmoid_draw(B, Rn, HW, 61)
    m = R.mask_draw(B, HW, 62, 0.3 if ign else 0.0)
    em = R.emu_sigmoid(x, y, m, ign, caps=CAPS, go=-0.5)
    r = R.sigmoid_ref(x, y, m, ign, go=-0.5)
    assert R.within(em.sums, r.sums, R.sums_bound(r, B, HW))
    assert R.grad_ok(em.grad, R.sigmoid_ref(x, y, m, ign, go=-0.5, coef=em.coef))
    fam = "regions_ign" if ign else "regions"
    l64, cf, lb, cb = R.finish_bound(em.sums, fam, Rn, 1e-5, 1.0)
    assert R.within(em.loss, l64, lb) and R.within(em.coef, cf, cb)
    if ign:
        bad = R.emu_sigmoid(x, y, m, ign, mutant="bce_nvalid_R")
        assert not R.within(bad.coef, R.finish_bound(bad.sums, fam, Rn, 1e-5, 1.0)[1], cb)
    xe, ye = R.exact_sigmoid_draw(B, Rn, HW, 63)
    re = R.sigmoid_ref(xe, ye, m, ign)
    assert R.exact_sums_ok(R.emu_sigmoid(xe, ye, m, ign, caps=CAPS).sums, re, fam, False, R.sums_bound(re, B, HW)[:1])
    for mutant in ("drop_partial_quad", "drop_trip", "dup_trip"):
        assert not R.exact_sums_ok(R.emu_sigmoid(xe, ye, m, ign, caps=CAPS, mutant=mutant).sums, re, fam, False, R.sums_bound(re, B, HW)[:1])
    xs, ys = R.extreme_sigmoid_draw()
    ms = torch.ones(1, xs.shape[2], dtype=torch.bool)
    rs = R.sigmoid_ref(xs, ys, ms, False)
    es = R.emu_sigmoid(xs, ys, ms, False)
    assert R.within(es.sums, rs.sums, R.sums_bound(rs, 1, xs.shape[2])) and R.grad_ok(es.grad, R.sigmoid_ref(xs, ys, ms, False, coef=es.coef))


@pytest.mark.parametrize("mode", ["softmax", "regions"])
def test_deep_supervision_emulation_and_its_mutants(mode):
    B, (H, W) = 2, R.DS_EXACT[0]
    N = 4 if mode == "softmax" else 2
    weights = (4 / 7, 2 / 7, 1 / 7)
    table = [0b0110, 0b0100]
    t = R.labels_draw(B, 4, H * W, 70, ignore_frac=0.3)
    if mode == "softmax":
        outs = [R.exact_softmax_draw(B, N, h * w, 71 + i).view(B, N, h, w) for i, (h, w) in enumerate(R.DS_EXACT)]
    else:
        outs = [R.exact_sigmoid_draw(B, N, h * w, 71 + i)[0].view(B, N, h, w) for i, (h, w) in enumerate(R.DS_EXACT)]
    kw = dict(table=table, ignore=R.IGNORE)
    r = R.ds_ref(outs, t, H, W, mode, weights, **kw)
    S, C = 3, (N if mode == "regions" else N - 1)

    def exact_part(em):       # n_valid and the Dice slices to the bit
        return torch.equal(em.sums[1:2 * S:2], r.sums[1:2 * S:2].float()) and torch.equal(em.sums[2 * S:], r.sums[2 * S:].float())

    def finish_ok(em):
        l64, c64 = R.ds_finish64(em.sums, mode, N, S, weights, True, 1e-5, 1.0)
        return R.within(em.coef, c64, 12 * R.U * c64.abs()) and R.within(em.loss, l64, 64 * R.U * (l64.abs() + 1))

    em = R.emu_ds(outs, t, H, W, mode, weights, **kw)
    assert exact_part(em) and finish_ok(em)
    assert not exact_part(R.emu_ds(outs, t, H, W, mode, weights, mutant="ds_floor_index", **kw))
    assert not finish_ok(R.emu_ds(outs, t, H, W, mode, weights, mutant="ds_weight_dropped", **kw))
