"""GPU tests (-m gpu) of the validation step: the HIP validation pass (csrc/loss.hip du_val_dice_ce / du_val_dice_ce_masked /
du_val_dice_bce through training.validation_counts and ops.val_dice_*) and training.ValStep.

Everything here is an equality.  Counts are integers: == the reference's own get_tp_fp_fn_tn (tests/golden/val_counts_reference.npz)
and == the CPU restatement over a sweep of the three label configurations.  The validation loss shares the per-pixel float code, the
reduction and the finish kernel with the training loss: bit-equal to SegLoss / dc_and_ce_loss forward.  The sweep's random logits are
N(0, 2) in fp32; a region logit inside (0, 1e-6) is moved to 1e-6, out of the only band where `x > 0` and torch's `sigmoid(x) > 0.5`
differ (0 < x < ~1.2e-7)."""
import json
import os

import numpy as np
import pytest
import torch

from test_gpu_ops import dev

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "val_counts_reference.npz")
CASES = ["softmax", "softmax_ignore", "softmax_all_ignored", "regions_ignore", "regions_tail", "softmax_ties", "regions_ties"]
REGION_SETS = {2: [1, (1, 2)], 3: [(1, 2, 3), (2, 3), (3,)], 4: [1, 2, 3, (1, 2, 3)],
               8: [1, 2, 3, 4, (1, 2), (3, 4), (5, 6), (1, 2, 3, 4, 5, 6)]}
# one partial block | HW % 4 != 0: guarded path, partial last quad | | several blocks | K = R = 8 | above the 2048-block cap: grid-stride loop
SHAPES = [(1, 2, 4, 4), (2, 3, 17, 23), (3, 4, 48, 40), (2, 3, 64, 64), (1, 8, 32, 32), (5, 2, 1024, 1024)]
MODES = ["softmax", "softmax_ignore", "regions", "regions_ignore"]


def _inputs(shape, mode, frac, seed):
    """logits N(0, 2), labels over the classes / the region labels, a fraction `frac` of them the ignore label"""
    B, C, H, W = shape
    regions = REGION_SETS[C] if mode.startswith("regions") else None
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(shape, generator=g) * 2.0
    top = C if regions is None else max(max((r,) if isinstance(r, int) else r) for r in regions) + 1
    ignore = max(top, C) if mode.endswith("ignore") else None       # build_loss: not a class index, not inside a region
    lab = torch.randint(0, top, (B, 1, H, W), generator=g)
    if ignore is not None:
        lab = torch.where(torch.rand((B, 1, H, W), generator=g) < frac, torch.full_like(lab, ignore), lab)
    if regions is not None:         # keep the inputs out of the band where x > 0 and torch's fp32 sigmoid(x) > 0.5 differ (0 < x < ~1.2e-7)
        logits = torch.where((logits > 0) & (logits < 1e-6), torch.full_like(logits, 1e-6), logits)
        assert not bool(((logits > 0) & (logits < 1e-6)).any())
    return logits, lab, regions, ignore


def _cpu_counts(logits, lab, regions, ignore):
    from dinounet_amd.training import validation_counts
    return torch.stack(validation_counts(logits.cpu(), lab.cpu(), regions=regions, ignore_label=ignore))


def _hip(logits, lab, regions, ignore, accum=None):
    """(loss, (3, C) counts) of the HIP validation pass through the public operators"""
    from dinounet_amd import ops
    from dinounet_amd.training import labels_to_regions
    if regions is not None:
        return ops.val_dice_bce(logits, labels_to_regions(lab, regions, ignore), ignore is not None, accum=accum)
    return ops.val_dice_ce(logits, lab, ignore, accum=accum)


def _train_loss(logits, lab, regions, ignore):
    """forward of the training loss on the same tensors"""
    from dinounet_amd.training import build_loss, dc_and_ce_loss
    if regions is None and ignore is None:
        return dc_and_ce_loss(logits, lab, ddp=False)
    return build_loss(logits.shape[1], regions=regions, ignore_label=ignore, ddp=False).to(logits.device)(logits, lab)


# ---- (a) the reference's own counts
@pytest.mark.parametrize("name", CASES)
def test_hip_counts_equal_reference_fixture(name):
    from dinounet_amd.training import validation_counts
    d = dev()
    g = np.load(GOLD)
    c = [c for c in json.loads(str(g["meta"]))["cases"] if c["name"] == name][0]
    regions = None if c["regions"] is None else [r if isinstance(r, int) else tuple(r) for r in c["regions"]]
    logits = torch.from_numpy(g[f"{name}/logits"]).to(d)
    labels = torch.from_numpy(g[f"{name}/labels"].astype(np.int64)).to(d)
    got = validation_counts(logits, labels, regions=regions, ignore_label=c["ignore_label"])
    for t, key in zip(got, ("tp", "fp", "fn")):
        assert t.dtype == torch.int64 and t.is_cuda
        assert np.array_equal(t.cpu().numpy(), g[f"{name}/{key}"].astype(np.int64)), (name, key, t, g[f"{name}/{key}"])


# ---- (b) sweep: counts == the CPU restatement, loss bit-equal to the training forward, two calls bit-identical
SWEEP = [(m, f) for m in MODES for f in ((0.0, 0.3, 1.0) if m.endswith("ignore") else (0.0,))]


@pytest.mark.parametrize("mode,frac", SWEEP)
@pytest.mark.parametrize("shape", SHAPES)
def test_sweep_counts_equal_cpu_and_loss_bits_equal_training_loss(shape, mode, frac):
    d = dev()
    logits, lab, regions, ignore = _inputs(shape, mode, frac, seed=11)
    want = _cpu_counts(logits, lab, regions, ignore)
    xl, xt = logits.to(d), lab.to(d)
    loss, counts = _hip(xl, xt, regions, ignore)
    loss2, counts2 = _hip(xl, xt, regions, ignore)
    ref = _train_loss(xl, xt, regions, ignore)
    torch.cuda.synchronize()
    what = (shape, mode, frac)
    assert counts.dtype == torch.int64 and torch.equal(counts.cpu(), want), (what, counts.cpu(), want)
    assert torch.equal(counts, counts2) and torch.equal(loss, loss2), what
    assert loss.dtype == torch.float32 and torch.equal(loss, ref.detach()), (what, float(loss), float(ref))
    if frac == 1.0:
        assert int(counts.abs().sum()) == 0, what


# ---- (c) ties
def test_ties_all_equal_logits_predict_class_0_and_zero_region_logits_predict_nothing():
    d = dev()
    g = torch.Generator().manual_seed(3)
    lab = torch.randint(0, 4, (2, 1, 17, 23), generator=g)
    n = torch.bincount(lab.flatten(), minlength=4)
    for value in (0.0, -2.5):
        _, c = _hip(torch.full((2, 4, 17, 23), value, device=d), lab.to(d), None, None)
        assert c[0].tolist() == [int(n[0]), 0, 0, 0]                      # tp: class 0 wherever it is labelled
        assert c[1].tolist() == [int(n[1] + n[2] + n[3]), 0, 0, 0]        # fp: class 0 everywhere else
        assert c[2].tolist() == [0, int(n[1]), int(n[2]), int(n[3])]      # fn
    # a tie among the later classes only: the lowest of them
    x = torch.zeros(2, 4, 17, 23)
    x[:, 2:] = 1.0
    _, c = _hip(x.to(d), lab.to(d), None, None)
    assert c[0].tolist() == [0, 0, int(n[2]), 0] and c[1].tolist() == [0, 0, int(n[0] + n[1] + n[3]), 0]
    regions = REGION_SETS[4]
    _, c = _hip(torch.zeros(2, 4, 17, 23, device=d), lab.to(d), regions, None)
    want = _cpu_counts(torch.zeros(2, 4, 17, 23), lab, regions, None)
    assert int(c[0].sum()) == 0 and int(c[1].sum()) == 0 and torch.equal(c.cpu(), want) and int(c[2].sum()) > 0


# ---- (d) an unaligned logits view takes the guarded scalar path: same counts, and the loss of the training forward on the same view
@pytest.mark.parametrize("mode", ["softmax_ignore", "regions_ignore"])
def test_unaligned_logits_view_gives_the_same_counts(mode):
    d = dev()
    shape = (2, 3, 64, 64)
    logits, lab, regions, ignore = _inputs(shape, mode, 0.3, seed=12)
    buf = torch.empty(logits.numel() + 1, device=d)
    view = buf[1:].view(shape)
    view.copy_(logits)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    xt = lab.to(d)
    loss_a, c_a = _hip(logits.to(d), xt, regions, ignore)
    loss_u, c_u = _hip(view, xt, regions, ignore)
    assert torch.equal(c_a, c_u) and torch.equal(c_u.cpu(), _cpu_counts(logits, lab, regions, ignore))
    assert torch.equal(loss_u, _train_loss(view, xt, regions, ignore).detach())


# ---- (e) the persistent accumulator: exact int64 addition on the device
@pytest.mark.parametrize("mode", ["softmax", "softmax_ignore", "regions_ignore"])
def test_accumulation_is_exact_in_int64(mode):
    d = dev()
    logits, lab, regions, ignore = _inputs((2, 3, 64, 64), mode, 0.3, seed=13)
    accum = torch.full((3, 3), 2 ** 40 + 1, dtype=torch.int64, device=d)
    _, counts = _hip(logits.to(d), lab.to(d), regions, ignore, accum=accum)
    assert int(counts.sum()) > 0
    assert torch.equal(accum - (2 ** 40 + 1), counts)
    _hip(logits.to(d), lab.to(d), regions, ignore, accum=accum)
    assert torch.equal(accum - (2 ** 40 + 1), 2 * counts)


# ---- (f) ValStep: captured vs eager, replay after a TrainStep update, training flag
def _net(num_classes, d):
    from oracle import weights
    from oracle.refshim import PLANS_2D
    from dinounet_amd.dinov3.adapter import DropPath
    from dinounet_amd.network_architecture import DinoUNet
    net = DinoUNet.from_config(PLANS_2D, 3, num_classes, dinov3_pretrained_path=None, dinov3_model_name="dinounet_s", precision="bf16")
    ks = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    net.load_state_dict(weights.make_state_dict(ks, seed=0), strict=True)
    net = net.to(d).train()
    for m in net.modules():
        if isinstance(m, DropPath):
            m.drop_prob = 0.0
    net.encoder.dinov3_adapter.backbone.rope_embed.rescale_coords = None
    return net


def _batches(n, ignore, d):
    from oracle import weights
    out = []
    for i in range(n):
        x = weights.make_input(4, 3, 128, 128, seed=20 + i)
        lab = weights.make_target(4, 128, 128, 3, seed=20 + i)
        g = torch.Generator().manual_seed(30 + i)
        if ignore is not None:
            lab = torch.where(torch.rand(lab.shape, generator=g) < 0.3, torch.full_like(lab, ignore), lab)
        out.append((x.to(d), lab.to(d)))
    return out


def _loss(cfg):
    """the ValStep / TrainStep `loss` argument: None (plain labels, the default) unless the configuration has an ignore label or regions"""
    from dinounet_amd.training import build_loss
    return build_loss(**cfg) if len(cfg) > 1 else None


@pytest.mark.parametrize("cfg", [dict(num_classes=3), dict(num_classes=3, ignore_label=3),
                                 dict(num_classes=2, regions=[(1, 2), (2,)], ignore_label=3)])
def test_val_step_hipgraph_matches_eager_and_follows_train_step(cfg):
    """three steps with different inputs, captured (one eager warm-up step, the capture and its replay, a replay) against eager: identical counts
    and loss bits, identical accumulators; then ONE TrainStep update of the same net: the replay reads the new weights in place and
    equals a fresh eager validation; net.training is restored after every step"""
    from dinounet_amd.optim import FusedClipSGD
    from dinounet_amd.training import TrainStep, ValStep
    d = dev()
    net = _net(cfg["num_classes"], d)
    data = _batches(4, cfg.get("ignore_label"), d)
    x_shape, t_shape = data[0][0].shape, data[0][1].shape
    steps = {}
    for graph in (False, True):
        vs = ValStep(net, x_shape, t_shape, d, loss=_loss(cfg), graph=graph, warmup=1)
        recs = []
        for x, lab in data[:3]:
            loss = vs(x, lab)
            assert net.training is True
            recs.append((loss.clone(), vs.step_counts.clone()))
        torch.cuda.synchronize()
        assert (vs.graph is not None) == graph and vs.steps == 3
        steps[graph] = (vs, recs, vs.counts.clone(), vs.loss_sum.clone())
    for (l0, c0), (l1, c1) in zip(steps[False][1], steps[True][1]):
        assert torch.equal(c0, c1), (c0, c1)
        assert torch.equal(l0, l1), (float(l0), float(l1))
    assert len({float(l) for l, _ in steps[True][1]}) == 3                      # different inputs, different steps
    assert torch.equal(steps[False][2], steps[True][2]) and torch.equal(steps[False][3], steps[True][3])
    assert torch.equal(steps[True][2], sum(c for _, c in steps[True][1])) and int(steps[True][2].sum()) > 0
    last = steps[True][0].last()
    assert last["tp_hard"].shape == (2,) and np.array_equal(        # K = 3 without the background / R = 2
        last["tp_hard"], steps[True][1][-1][1][0].cpu().numpy()[(0 if "regions" in cfg else 1):])
    # one optimiser step on the same net, then the captured validation against a fresh eager one
    params = [p for p in net.parameters() if p.requires_grad]
    before = [p.detach().clone() for p in params]
    ts = TrainStep(net, FusedClipSGD(params, 1e-2, momentum=0.99, nesterov=True, weight_decay=3e-5), params, x_shape, t_shape, d,
                   graph=False, loss=_loss(cfg))
    ts(*data[3])
    torch.cuda.synchronize()
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, params))
    vs_g = steps[True][0]
    old_loss = steps[True][1][0][0]
    l_g = vs_g(*data[0]).clone()
    c_g = vs_g.step_counts.clone()
    fresh = ValStep(net, x_shape, t_shape, d, loss=_loss(cfg), graph=False)
    l_e = fresh(*data[0])
    torch.cuda.synchronize()
    assert vs_g.graph is not None and net.training is True
    assert torch.equal(l_g, l_e) and torch.equal(c_g, fresh.step_counts), (float(l_g), float(l_e))
    assert not torch.equal(l_g, old_loss)                                       # the update is visible to the replay
    out = vs_g.epoch_end()
    assert out["steps"] == 4 and int(vs_g.counts.abs().sum()) == 0
