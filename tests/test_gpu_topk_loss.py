"""GPU suite (-m gpu) of the fused top-k losses (ops.topk_ce_loss / ops.dice_topk_loss, csrc/loss_topk.hip; training.dc_and_topk_loss,
build_loss(topk_percent=...)): the reference fixture (tests/golden/topk_loss_reference.npz, every threshold isolated by >= 1e-3 so
the kernel's selection is the reference's), a sweep over the shape edges against the fp64 formula in four chained checks (values,
integer-exact selection, loss, gradient), ties, an all-ignored batch, bit-reproducibility across calls and graph replays, TrainStep
captured against eager, ValStep, deep supervision and two ranks over gloo.

LOSS_TOL / GRAD_TOL are the family's bounds (tests/test_gpu_seg_loss.py).  VAL_TOL is the per-element bound on the values buffer,
|v - v64| <= 2e-5 max(1, v64): the fp32 logsumexp of <= 8 terms of magnitude <= ~10 rounds at ~1e-6, the fast exp / log add a few ulp."""
import functools
import json
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from test_gpu_ops import dev, rel

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "topk_loss_reference.npz")
LOSS_TOL, GRAD_TOL, VAL_TOL = 2e-5, 2e-4, 2e-5


def _fixture():
    g = np.load(GOLD)
    return g, json.loads(str(g["meta"]))


def hip_loss(kind, logits, labels, ignore_label, k, go=1.0, group=None):
    """fused HIP loss, d (go * loss) / d logits and the aux outputs (values, selection, threshold)"""
    from dinounet_amd import ops
    d = dev()
    x = logits.to(d).float().requires_grad_(True)
    lab = labels.to(d)
    if kind == "topk":
        loss, values, sel, thr = ops.topk_ce_loss(x, lab, k, ignore_label, return_aux=True)
    else:
        loss, values, sel, thr = ops.dice_topk_loss(x, lab, k, ignore_label, 1e-5, group, return_aux=True)
    (loss * go).backward()
    torch.cuda.synchronize()
    return loss.detach(), x.grad, (values, sel, thr)


def _assert_close(loss, grad, ref_loss, ref_grad, what):
    dl = abs(float(loss) - ref_loss)
    rg = rel(grad, torch.as_tensor(ref_grad))
    print(f"{what}: |dloss| {dl:.3e} (ref {ref_loss:.6f})  grad rel {rg:.3e}")
    assert dl <= LOSS_TOL * max(1.0, abs(ref_loss)), (what, float(loss), ref_loss)
    assert rg <= GRAD_TOL, (what, rg)


# ---- (a) every fixture case (world 1)
@pytest.mark.parametrize("name", ["plain", "ignore", "tail", "k8", "half_ignore", "all_ignored", "topk_only"])
def test_hip_matches_reference_fixture(name):
    g, meta = _fixture()
    c = [c for c in meta["cases"] if c["name"] == name][0]
    logits = torch.from_numpy(g[f"{name}/logits"])
    labels = torch.from_numpy(g[f"{name}/labels"].astype(np.int64))
    loss, grad, (values, sel, thr) = hip_loss(c["kind"], logits, labels, c["ignore_label"], c["k"])
    assert int(sel.sum()) == int(g[f"{name}/k_vox"])
    assert abs(float(thr) - float(g[f"{name}/threshold"])) <= VAL_TOL * max(1.0, float(g[f"{name}/threshold"]))
    _assert_close(loss, grad.cpu(), float(g[f"{name}/loss"]), g[f"{name}/grad"], name)


# ---- (b) sweep: values, selection, loss, gradient
SHAPES = [(1, 2, 4, 4), (2, 3, 17, 23), (3, 4, 48, 40), (1, 8, 32, 32), (2, 2, 64, 64), (8, 3, 512, 512)]
FRACS = [0.0, 0.3, 1.0]
KSEL = ["one", "tenth", "all"]
GO = 1.7


def _k_percent(N, which):
    from dinounet_amd.training import topk_voxels
    k = {"one": 150.0 / N, "tenth": 10 if N >= 20 else 150.0 / N, "all": 100}[which]
    want = {"one": 1, "tenth": max(1, int(0.1 * N)), "all": N}[which]
    assert topk_voxels(N, k) == want
    return k, want


@functools.lru_cache(maxsize=4)
def _reference(shape, frac, seed=0):
    """inputs and everything of the fp64 formula that does not depend on k (computed once per shape and ignored fraction, read-only):
    logits, labels, ignore label, v64 (N), p - onehot masked (B,K,H,W), the Dice term and its gradient"""
    from dinounet_amd import training as T
    B, K, H, W = shape
    g = torch.Generator().manual_seed(seed + 1000 * K + H)
    logits = (torch.randn(shape, generator=g) * 2).float()
    lab = torch.randint(0, K, (B, 1, H, W), generator=g)
    ign = None
    if frac > 0:
        ign = K
        lab = torch.where(torch.rand((B, 1, H, W), generator=g) < frac, torch.full_like(lab, ign), lab)
    x = logits.double().requires_grad_(True)
    v64 = torch.nn.functional.cross_entropy(x, lab[:, 0], reduction="none", ignore_index=-100 if ign is None else ign)
    (ce_grad,) = torch.autograd.grad(v64.sum(), x)                 # (p - onehot) on valid voxels, 0 on ignored ones
    dice = T._soft_dice_torch(x, lab, ign, 1e-5, False, None)
    (dice_grad,) = torch.autograd.grad(dice, x)
    return logits, lab, ign, v64.detach().reshape(-1), ce_grad, float(dice.detach()), dice_grad


def _check_selection(values, sel, thr, k_vox):
    """(2): the selection is exactly the top-k of the kernel's own values, ties to the lowest flat index.  Integer-exact."""
    v = values.reshape(-1).cpu()
    s = sel.reshape(-1).cpu().bool()
    T = float(thr)
    assert int(s.sum()) == k_vox, (int(s.sum()), k_vox)
    assert float(torch.sort(v, descending=True)[0][k_vox - 1]) == T                    # T is the k-th largest of the own values
    assert bool(s[v > T].all()) and not bool(s[v < T].any())
    ties = torch.nonzero(v == T).reshape(-1)
    need = k_vox - int((v > T).sum())
    assert 1 <= need <= ties.numel()
    assert torch.equal(torch.nonzero(s & (v == T)).reshape(-1), ties[:need])           # nonzero is ascending: the lowest indices
    assert bool((v >= 0).all()) and not bool(torch.signbit(v).any())                    # +0, never -0: the bits order as integers
    return v, s


@pytest.mark.parametrize("which", KSEL)
@pytest.mark.parametrize("frac", FRACS)
@pytest.mark.parametrize("shape", SHAPES)
def test_sweep_values_selection_loss_gradient(shape, frac, which):
    logits, lab, ign, v64, ce_grad, dice64, dice_grad = _reference(shape, frac)
    N = v64.numel()
    k, k_vox = _k_percent(N, which)
    loss, grad, (values, sel, thr) = hip_loss("dc_topk", logits, lab, ign, k, go=GO)
    assert values.shape == (shape[0], shape[2] * shape[3]) and values.dtype == torch.float32
    assert sel.shape == values.shape and sel.dtype == torch.uint8
    # (1) the values buffer against the fp64 CE per element
    worst = float(((values.reshape(-1).cpu().double() - v64).abs() / v64.clamp_min(1.0)).max())
    print(f"{shape} frac {frac} k_vox {k_vox}: worst |v - v64| / max(1, v64) = {worst:.3e}")
    assert worst <= VAL_TOL
    # (2)
    v, s = _check_selection(values, sel, thr, k_vox)
    # (3) the loss: the fp64 mean of the selected own values (1e-6 relative) minus the fp64 Dice term (LOSS_TOL)
    ce_own = float(v[s].double().sum() / k_vox)
    assert abs(float(loss) - (ce_own - dice64)) <= 1e-6 * abs(ce_own) + LOSS_TOL * max(1.0, abs(dice64)), (float(loss), ce_own, dice64)
    # (4) the gradient of the fp64 formula evaluated with the kernel's selection
    want = GO * (ce_grad * s.reshape(shape[0], 1, shape[2], shape[3]).double() / k_vox - dice_grad)
    rg = rel(grad, want)
    print(f"   loss {float(loss):.6f}  grad rel {rg:.3e}")
    assert rg <= GRAD_TOL


BEYOND_CAP = (8, 2, 1024, 1024)      # 8.4 M voxels: past the 4096 sweep waves a wave owns 2048 values, 8 steps with a running tie offset


def test_beyond_the_sweep_grid_cap_values_selection_loss_gradient(frac=0.3):
    logits, lab, ign, v64, ce_grad, dice64, dice_grad = _reference(BEYOND_CAP, frac)
    B, K, H, W = BEYOND_CAP
    k_vox = int(0.1 * v64.numel())
    loss, grad, (values, sel, thr) = hip_loss("dc_topk", logits, lab, ign, 10, go=GO)
    worst = float(((values.reshape(-1).cpu().double() - v64).abs() / v64.clamp_min(1.0)).max())
    print(f"{BEYOND_CAP} frac {frac} k_vox {k_vox}: worst |v - v64| / max(1, v64) = {worst:.3e}")
    assert worst <= VAL_TOL
    v, s = _check_selection(values, sel, thr, k_vox)
    ce_own = float(v[s].double().sum() / k_vox)
    assert abs(float(loss) - (ce_own - dice64)) <= 1e-6 * abs(ce_own) + LOSS_TOL * max(1.0, abs(dice64))
    assert rel(grad, GO * (ce_grad * s.reshape(B, 1, H, W).double() / k_vox - dice_grad)) <= GRAD_TOL


def test_beyond_the_sweep_grid_cap_ties_run_across_the_steps_of_a_wave():
    """all-equal logits: every voxel ties, the first k_vox are selected, so the running offset inside a wave's 8 steps and the offsets
    between the waves are all in play; k = 33 % ends the selection in the middle of a wave's range"""
    from dinounet_amd.training import topk_voxels
    B, K, H, W = BEYOND_CAP
    lab = torch.randint(0, K, (B, 1, H, W), generator=torch.Generator().manual_seed(46))
    k_vox = topk_voxels(B * H * W, 33)
    assert k_vox % 2048 != 0
    loss, _, (values, sel, thr) = hip_loss("topk", torch.full(BEYOND_CAP, -0.5), lab, None, 33)
    s = sel.reshape(-1)
    assert int(s.sum()) == k_vox and bool(s[:k_vox].all()) and float(values.min()) == float(values.max()) == float(thr)
    assert abs(float(loss) - math.log(K)) <= LOSS_TOL


def test_torch_formula_refuses_a_capture():
    """more than 8 classes take the torch formula, whose torch.topk must not be captured: the call raises before any kernel, inside the
    capture, and works outside it"""
    from dinounet_amd import training as T
    d = dev()
    g = torch.Generator().manual_seed(47)
    x = torch.randn(2, 9, 16, 16, generator=g).to(d)
    lab = torch.randint(0, 9, (2, 1, 16, 16), generator=g).to(d)
    assert not T._topk_fused(x)
    eager = T.dc_and_topk_loss(x, lab, 10)
    ref = T.dc_and_topk_loss(x.cpu().double(), lab.cpu(), 10)
    assert abs(float(eager) - float(ref)) <= LOSS_TOL * max(1.0, abs(float(ref)))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="cannot be captured"):
        with torch.cuda.graph(graph):
            T.dc_and_topk_loss(x, lab, 10)
    torch.cuda.synchronize()
    assert not torch.cuda.is_current_stream_capturing()
    assert float(T.dc_and_topk_loss(x, lab, 10)) == float(eager)          # the device is usable after the refused capture


def test_topk_only_mode_goes_through_the_same_kernels():
    logits, lab, ign, v64, ce_grad, _, _ = _reference((2, 3, 17, 23), 0.3)
    k_vox = int(0.1 * v64.numel())
    loss, grad, (values, sel, thr) = hip_loss("topk", logits, lab, ign, 10, go=GO)
    v, s = _check_selection(values, sel, thr, k_vox)
    ce_own = float(v[s].double().sum() / k_vox)
    assert abs(float(loss) - ce_own) <= 1e-6 * abs(ce_own)
    assert rel(grad, GO * ce_grad * s.reshape(2, 1, 17, 23).double() / k_vox) <= GRAD_TOL
    from dinounet_amd.training import topk_ce_loss
    assert float(topk_ce_loss(logits.to(dev()), lab.to(dev()), 10, ignore_label=ign)) == float(loss)      # the public route


# ---- (c) ties
@pytest.mark.parametrize("shape,k", [((2, 3, 17, 23), 10), ((3, 4, 48, 40), 25), ((1, 2, 64, 64), 50)])
def test_ties_at_the_threshold_go_to_the_lowest_flat_index(shape, k):
    """logits from {-1, 0, 1}: a few distinct CE values, hundreds of voxels equal to the threshold"""
    from dinounet_amd.training import topk_voxels
    B, K, H, W = shape
    g = torch.Generator().manual_seed(41)
    logits = torch.randint(-1, 2, shape, generator=g).float()
    lab = torch.randint(0, K, (B, 1, H, W), generator=g)
    k_vox = topk_voxels(B * H * W, k)
    loss, _, (values, sel, thr) = hip_loss("topk", logits, lab, None, k)
    v, s = _check_selection(values, sel, thr, k_vox)
    assert int((v == float(thr)).sum()) > 1
    ce_own = float(v[s].double().sum() / k_vox)
    assert abs(float(loss) - ce_own) <= 1e-6 * abs(ce_own)


@pytest.mark.parametrize("shape", [(2, 3, 17, 23), (1, 8, 32, 32), (4, 2, 128, 128)])
def test_all_equal_logits_give_log_k_and_select_the_first_voxels(shape):
    from dinounet_amd.training import topk_voxels
    B, K, H, W = shape
    g = torch.Generator().manual_seed(42)
    logits = torch.full(shape, 0.75)
    lab = torch.randint(0, K, (B, 1, H, W), generator=g)
    k_vox = topk_voxels(B * H * W, 10)
    loss, _, (values, sel, thr) = hip_loss("topk", logits, lab, None, 10)
    v, s = _check_selection(values, sel, thr, k_vox)
    assert bool((v == v[0]).all())
    assert bool(s[:k_vox].all()) and int(s.sum()) == k_vox                # the first k_vox voxels in (b, y, x) order
    assert abs(float(loss) - math.log(K)) <= LOSS_TOL
    ce_own = float(v[s].double().sum() / k_vox)
    assert abs(float(loss) - ce_own) <= 1e-6 * abs(ce_own)


# ---- (d) ignored voxels
def test_all_ignored_batch_has_zero_ce_part_and_ignored_voxels_zero_gradient():
    g = torch.Generator().manual_seed(43)
    logits = (torch.randn(2, 3, 17, 23, generator=g) * 2).float()
    lab = torch.full((2, 1, 17, 23), 3)
    loss, grad, (values, sel, thr) = hip_loss("topk", logits, lab, 3, 10)
    assert float(loss) == 0.0 and float(thr) == 0.0 and float(values.abs().max()) == 0.0
    assert float(grad.abs().max()) == 0.0 and int(sel.sum()) == 78
    loss, grad, _ = hip_loss("dc_topk", logits, lab, 3, 10)
    assert float(loss) == -1.0 and float(grad.abs().max()) == 0.0         # s / s per class, as the masked Dice + CE loss
    # a part ignored: dlogits exactly 0 in every channel of an ignored voxel, selected or not
    lab = torch.randint(0, 3, (2, 1, 17, 23), generator=g)
    lab = torch.where(torch.rand(lab.shape, generator=g) < 0.5, torch.full_like(lab, 3), lab)
    _, grad, (values, sel, _) = hip_loss("dc_topk", logits, lab, 3, 100, go=GO)
    ignored = (lab == 3).expand(2, 3, 17, 23)
    assert bool(sel.reshape(2, 1, 17, 23).cpu()[lab == 3].all())           # k = 100 %: they are selected
    assert float(grad.cpu()[ignored].abs().max()) == 0.0 and float(grad.cpu()[~ignored].abs().min()) > 0.0
    assert float(values.reshape(2, 1, 17, 23).cpu()[lab == 3].abs().max()) == 0.0


# ---- (e) bit-reproducibility: two calls, two graph replays
@pytest.mark.parametrize("shape,ign", [((8, 3, 512, 512), None), ((2, 4, 17, 23), 4)])
def test_two_calls_and_two_graph_replays_are_bit_identical(shape, ign):
    from dinounet_amd import ops
    d = dev()
    B, K, H, W = shape
    g = torch.Generator().manual_seed(44)
    x = (torch.randn(shape, generator=g) * 2).float().to(d).requires_grad_(True)
    lab = torch.randint(0, K + (1 if ign is not None else 0), (B, 1, H, W), generator=g).to(d)

    def run():
        loss = ops.dice_topk_loss(x, lab, 10, ign)
        (gx,) = torch.autograd.grad(loss * GO, x)
        return loss.detach(), gx

    outs = []
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            l, gx = run()
            outs.append((l.clone(), gx.clone()))
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        l, gx = run()
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        outs.append((l.clone(), gx.clone()))
    assert torch.isfinite(outs[0][0]) and float(outs[0][1].abs().max()) > 0
    for l2, g2 in outs[1:]:
        assert torch.equal(l2, outs[0][0]) and torch.equal(g2, outs[0][1])


# ---- (f) TrainStep / ValStep
def _net(num_classes, d, deep_supervision=False):
    from oracle import weights
    from oracle.refshim import PLANS_2D
    from dinounet_amd.dinov3.adapter import DropPath
    from dinounet_amd.network_architecture import DinoUNet
    plans = dict(PLANS_2D, architecture=dict(PLANS_2D["architecture"], deep_supervision=True)) if deep_supervision else PLANS_2D
    net = DinoUNet.from_config(plans, 3, num_classes, dinov3_pretrained_path=None, dinov3_model_name="dinounet_s", precision="bf16")
    ks = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    net.load_state_dict(weights.make_state_dict(ks, seed=0), strict=True)
    net = net.to(d).train()
    for m in net.modules():
        if isinstance(m, DropPath):
            m.drop_prob = 0.0
    net.encoder.dinov3_adapter.backbone.rope_embed.rescale_coords = None
    return net


def test_train_step_with_topk_loss_captured_equals_eager():
    """build_loss(3, topk_percent=10) on a dinounet_s 64 x 64 net, FusedClipSGD on both sides.  The two warm-up steps run with lr = 0, so
    the parameters stay the initial ones bit for bit (asserted); the third step, lr = 1e-3, is the captured one (one graph: nothing in
    the loss reads back) against the third eager step.
    Loss: bit for bit, all three steps (the same parameters and inputs through the forward pass and the loss kernels).
    Parameter update: the network's backward adds with fp32 atomics (MSDA grad_value, norm statistics), so two runs of the same step
    may differ in the last bits of a gradient, and elementwise equality would test the atomics' order.  Bound: the step moves an element by lr (g + mu buf) <= lr 4 |g| after three steps at mu = 0.99
    (nesterov), |g| <= 12 after the clip, a reordered fp32 sum differs by <= 1e-5 relative: 1e-3 * 4 * 12 * 1e-5 = 4.8e-7.  A wrong or
    missing loss gradient in the captured step moves the segmentation head by lr |g| ~ 1e-5 .. 1e-3."""
    from oracle import weights
    from dinounet_amd.optim import FusedClipSGD
    from dinounet_amd.training import TrainStep, build_loss
    d = dev()
    x = weights.make_input(2, 3, 64, 64, seed=5).to(d)
    lab = weights.make_target(2, 64, 64, 3, seed=5).to(d)
    res = {}
    for mode in (False, True):
        net = _net(3, d)
        params = [p for p in net.parameters() if p.requires_grad]
        init = [p.detach().clone() for p in params]
        opt = FusedClipSGD(params, 0.0, momentum=0.99, nesterov=True, weight_decay=3e-5)
        ts = TrainStep(net, opt, params, x.shape, lab.shape, d, graph=mode, warmup=2, loss=build_loss(3, topk_percent=10))
        ls = [ts(x, lab).clone(), ts().clone()]
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(init, params))        # lr = 0: nothing moved
        opt.param_groups[0]["lr"] = 1e-3
        ls.append(ts().clone())
        torch.cuda.synchronize()
        if mode:
            assert ts.capture_mode == "whole_step" and ts.graph is not None, ts.capture_mode
        assert all(bool(torch.isfinite(l)) for l in ls)
        res[mode] = (ls, [p.detach().clone() for p in params], init)
    print("eager", [float(l) for l in res[False][0]], "graph", [float(l) for l in res[True][0]])
    diff = max(float((a - b).abs().max()) for a, b in zip(res[False][1], res[True][1]))
    moved = max(float((a - b).abs().max()) for a, b in zip(res[False][1], res[False][2]))
    print(f"largest parameter difference after the captured step {diff:.3e}; largest move of the step {moved:.3e}")
    assert all(torch.equal(a, b) for a, b in zip(res[False][0], res[True][0]))
    assert moved > 10 * 4.8e-7 and diff <= 4.8e-7          # the step is well above the bound, the difference within it


@pytest.mark.parametrize("ign", [None, 3])
def test_val_step_with_topk_loss_counts_and_loss(ign):
    """counts: those of the plain softmax(-ignore) ValStep; loss: the top-k module's forward value on the same logits"""
    from oracle import weights
    from dinounet_amd.training import ValStep, build_loss
    d = dev()
    x = weights.make_input(2, 3, 64, 64, seed=6).to(d)
    lab = weights.make_target(2, 64, 64, 3, seed=6)
    if ign is not None:
        g = torch.Generator().manual_seed(12)
        lab = torch.where(torch.rand(lab.shape, generator=g) < 0.3, torch.full_like(lab, ign), lab)
    lab = lab.to(d)
    net = _net(3, d)
    loss_fn = build_loss(3, ignore_label=ign, topk_percent=10)
    vs = ValStep(net, x.shape, lab.shape, d, loss=loss_fn, graph=False)
    got = vs(x, lab).clone()
    plain = ValStep(net, x.shape, lab.shape, d, loss=build_loss(3, ignore_label=ign), graph=False)
    plain(x, lab)
    torch.cuda.synchronize()
    assert torch.equal(vs.step_counts, plain.step_counts) and torch.equal(vs.counts, plain.counts) and int(vs.counts.sum()) > 0
    net.eval()
    with torch.no_grad():
        want = loss_fn(net(x), lab)
    net.train()
    assert torch.equal(got, want) and float(vs.loss_sum) == float(want.double())
    assert float(got) != float(plain.loss)                                 # not the Dice + CE value


# ---- (g) deep supervision: the wrapper composes the fused per-scale top-k losses
def test_deep_supervision_three_scales_match_the_fp64_composition():
    from dinounet_amd import training as T
    d = dev()
    g = torch.Generator().manual_seed(53)
    sizes = [(48, 40), (24, 20), (12, 10)]
    outs = [(torch.randn(2, 3, h, w, generator=g) * 2).float() for h, w in sizes]
    lab = torch.randint(0, 3, (2, 1, 48, 40), generator=g)
    lab = torch.where(torch.rand(lab.shape, generator=g) < 0.3, torch.full_like(lab, 3), lab)
    for o in outs:      # whole gradients are comparable because every scale's threshold is isolated (the fixture's rule: gap >= 1e-3)
        v = torch.nn.functional.cross_entropy(o.double(), T.downsample_target(lab, o.shape[-2:])[:, 0], reduction="none", ignore_index=3)
        s = torch.sort(v.reshape(-1), descending=True)[0]
        k_vox = T.topk_voxels(s.numel(), 10)
        assert float(s[k_vox - 1] - s[k_vox]) >= 1e-3
    w = (0.5, 0.3, 0.2)
    m = T.build_loss(3, ignore_label=3, deep_supervision_weights=w, topk_percent=10)
    xs = [o.to(d).requires_grad_(True) for o in outs]
    assert not m.fused(xs)
    loss = m(xs, lab.to(d))
    (loss * GO).backward()
    x64 = [o.double().requires_grad_(True) for o in outs]
    ref = m(x64, lab)                                                      # CPU fp64: the torch formula per scale
    (ref * GO).backward()
    torch.cuda.synchronize()
    assert abs(float(loss.detach()) - float(ref.detach())) <= LOSS_TOL * max(1.0, abs(float(ref.detach())))
    for a, b in zip(xs, x64):
        assert rel(a.grad, b.grad) <= GRAD_TOL


# ---- (h) two ranks on one GPU over gloo against the reference's world-2 run
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _ddp_worker(rank, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        import torch.distributed as dist
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=2)
        g, meta = _fixture()
        out = {}
        for c in [c for c in meta["cases"] if c["world"] == 2]:
            n = c["name"]
            logits = torch.from_numpy(g[f"{n}/logits"])[rank:rank + 1]
            labels = torch.from_numpy(g[f"{n}/labels"].astype(np.int64))[rank:rank + 1]
            loss, grad, (_, sel, _) = hip_loss(c["kind"], logits, labels, c["ignore_label"], c["k"], group=dist.group.WORLD)
            out[n] = (float(loss), grad.cpu().numpy().copy(), int(sel.sum()))
        q.put((rank, out))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc()))


def test_two_ranks_on_one_gpu_match_reference_ddp_fixture():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_ddp_worker, args=(r, port, q)) for r in range(2)]
    [p.start() for p in procs]
    res = dict(q.get(timeout=300) for _ in range(2))
    [p.join(timeout=120) for p in procs]
    for r in range(2):
        assert not isinstance(res[r], str), res[r]
    assert all(p.exitcode == 0 for p in procs)
    g, meta = _fixture()
    for c in [c for c in meta["cases"] if c["world"] == 2]:
        n = c["name"]
        for r in range(2):
            loss, grad, nsel = res[r][n]
            assert nsel == int(g[f"{n}/k_vox"][r])                         # the top-k is the rank's own
            _assert_close(loss, torch.from_numpy(grad), float(g[f"{n}/loss"][r]), g[f"{n}/grad"][r:r + 1], f"{n} rank {r}")
