"""GPU tests (-m gpu) of the fused ignore-label and region losses (csrc/loss.hip du_dice_ce_masked_* / du_dice_bce_* /
du_labels_to_regions, training.build_loss): against the reference's fp64 fixture (tests/golden/seg_loss_reference.npz), against the fp64
CPU formula across a sweep, exact properties (ignored pixels, all-ignored batch, bit-reproducibility), the region conversion bit for
bit, TrainStep with build_loss captured vs eager, and two ranks over gloo.

Bounds: |loss - ref| <= 2e-5 max(1, |ref|), gradient rel (test_gpu_ops.rel) <= 2e-4 -- the bounds test_fused_dice_ce_loss applies to the
same kernel family.  The reference classes themselves in fp32 stay within 2.2e-8 (loss) / 4.3e-7 (gradient) of fp64 at (8,3..4,512,512),
so the bounds leave >= 400x room over fp32 rounding."""
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from test_gpu_ops import dev, rel

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seg_loss_reference.npz")
LOSS_TOL, GRAD_TOL = 2e-5, 2e-4


def _fixture():
    g = np.load(GOLD)
    return g, json.loads(str(g["meta"]))


def _regions(c):
    return None if c["regions"] is None else [r if isinstance(r, int) else tuple(r) for r in c["regions"]]


def hip_loss(kind, logits, labels, regions, ignore_label, go=1.0, group=None):
    """fused HIP loss and d (go * loss) / d logits on the GPU (logits fp32 CPU or GPU, labels (B,1,H,W) int64)"""
    from dinounet_amd import ops, training as T
    d = dev()
    x = logits.to(d).float().requires_grad_(True)
    lab = labels.to(d)
    if kind == "regions":
        onehot = T.labels_to_regions(lab, regions, ignore_label)
        loss = ops.dice_bce_loss(x, onehot, ignore_label is not None, 1e-5, group)
    else:
        loss = ops.dice_ce_masked_loss(x, lab, ignore_label, 1e-5, group)
    (loss * go).backward()
    torch.cuda.synchronize()
    return loss.detach(), x.grad


def cpu_ref(kind, logits, labels, regions, ignore_label, go=1.0):
    """the product's fp64 torch formula (pinned to the reference classes by tests/test_cpu_seg_loss.py)"""
    from dinounet_amd import training as T
    x = logits.detach().cpu().double().requires_grad_(True)
    lab = labels.cpu()
    if kind == "regions":
        loss = T.dc_and_bce_loss(x, T.labels_to_regions(lab, regions, ignore_label), use_ignore_label=ignore_label is not None, ddp=False)
    else:
        loss = T.dc_and_ce_loss(x, lab, ddp=False, ignore_label=ignore_label)
    (g,) = torch.autograd.grad(loss * go, x)
    return float(loss.detach()), g


def _assert_close(loss, grad, ref_loss, ref_grad, what):
    dl = abs(float(loss) - ref_loss)
    rg = rel(grad, torch.as_tensor(ref_grad))
    print(f"{what}: |dloss| {dl:.3e} (ref {ref_loss:.6f})  grad rel {rg:.3e}")
    assert dl <= LOSS_TOL * max(1.0, abs(ref_loss)), (what, float(loss), ref_loss)
    assert rg <= GRAD_TOL, (what, rg)


# ---- (a) every fixture case (world 1)
@pytest.mark.parametrize("name", ["ce_ignore", "ce_all_ignored", "regions_ignore", "regions_tail"])
def test_hip_matches_reference_fixture(name):
    g, meta = _fixture()
    c = [c for c in meta["cases"] if c["name"] == name][0]
    logits = torch.from_numpy(g[f"{name}/logits"])
    labels = torch.from_numpy(g[f"{name}/labels"].astype(np.int64))
    loss, grad = hip_loss(c["kind"], logits, labels, _regions(c), c["ignore_label"])
    _assert_close(loss, grad.cpu(), float(g[f"{name}/loss"]), g[f"{name}/grad"], name)


# ---- (b) sweep against the fp64 CPU formula
SHAPES = [(2, 2, 64, 64), (3, 4, 48, 40), (8, 3, 512, 512), (1, 8, 32, 32), (2, 3, 17, 23)]
FRACS = [0.0, 0.3, 1.0]
REGION_SETS = {1: [(1, 2)], 2: [1, (1, 2)], 3: [(1, 2, 3), (2, 3), (3,)], 4: [1, 2, 3, (1, 2, 3)],
               8: [1, 2, 3, 4, (1, 2), (3, 4), (5, 6), (1, 2, 3, 4, 5, 6)]}


def _inputs(shape, kind, regions, ignore_label, frac, seed):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(shape, generator=g) * 2.0
    top = C if kind == "softmax" else max(max((r,) if isinstance(r, int) else r) for r in regions) + 1
    lab = torch.randint(0, top, (B, 1, H, W), generator=g)
    if ignore_label is not None:
        lab = torch.where(torch.rand((B, 1, H, W), generator=g) < frac, torch.full_like(lab, ignore_label), lab)
    return logits, lab


@pytest.mark.parametrize("frac", FRACS)
@pytest.mark.parametrize("shape", SHAPES)
def test_masked_softmax_sweep_matches_fp64_formula(shape, frac):
    K = shape[1]
    logits, lab = _inputs(shape, "softmax", None, K, frac, seed=hash((shape, frac)) % 1000)
    loss, grad = hip_loss("softmax", logits, lab, None, K, go=1.7)
    ref_loss, ref_grad = cpu_ref("softmax", logits, lab, None, K, go=1.7)
    _assert_close(loss, grad.cpu(), ref_loss, ref_grad, f"softmax+ignore {shape} frac {frac}")


def _region_cases():
    out = []
    for shape in SHAPES:
        for frac in FRACS:                               # with the ignore channel
            out.append((shape, True, frac))
        out.append((shape, False, 0.0))                  # without
    for R in (1, 3, 8):
        for ign in (True, False):
            out.append(((2, R, 40, 36), ign, 0.3 if ign else 0.0))
    return out


@pytest.mark.parametrize("shape,with_ignore,frac", _region_cases())
def test_regions_sweep_matches_fp64_formula(shape, with_ignore, frac):
    R = shape[1]
    regions = REGION_SETS[R]
    ig = 9 if with_ignore else None
    logits, lab = _inputs(shape, "regions", regions, ig, frac, seed=hash((shape, with_ignore, frac)) % 1000)
    loss, grad = hip_loss("regions", logits, lab, regions, ig, go=1.7)
    ref_loss, ref_grad = cpu_ref("regions", logits, lab, regions, ig, go=1.7)
    _assert_close(loss, grad.cpu(), ref_loss, ref_grad, f"regions {shape} ignore {with_ignore} frac {frac}")


# ---- (c) exact properties
@pytest.mark.parametrize("kind", ["softmax", "regions"])
def test_ignored_pixels_have_exactly_zero_gradient(kind):
    shape = (2, 3, 33, 31)
    regions = REGION_SETS[3] if kind == "regions" else None
    logits, lab = _inputs(shape, kind, regions, 7, 0.4, seed=5)
    _, grad = hip_loss(kind, logits, lab, regions, 7)
    ign = (lab == 7).expand(-1, 3, -1, -1)
    g = grad.cpu()
    assert int(ign.sum()) > 0
    assert bool((g[ign] == 0.0).all())
    assert float(g[~ign].abs().max()) > 0


@pytest.mark.parametrize("kind,shape", [("softmax", (1, 3, 16, 16)), ("softmax", (2, 8, 17, 23)), ("regions", (2, 3, 32, 32)),
                                        ("regions", (1, 8, 9, 7))])
def test_all_ignored_batch_is_exactly_minus_one(kind, shape):
    regions = REGION_SETS[shape[1]] if kind == "regions" else None
    logits, lab = _inputs(shape, kind, regions, 9, 1.0, seed=6)
    loss, grad = hip_loss(kind, logits, lab, regions, 9)
    assert float(loss) == -1.0                               # s / s = 1 in fp32 per class, CE / BCE skipped on the device
    assert float(grad.abs().max()) == 0.0


@pytest.mark.parametrize("kind,shape", [("softmax", (8, 4, 512, 512)), ("regions", (8, 3, 512, 512)), ("regions", (2, 3, 17, 23))])
def test_two_calls_are_bit_identical(kind, shape):
    regions = REGION_SETS[shape[1]] if kind == "regions" else None
    ig = shape[1] if kind == "softmax" else 9
    logits, lab = _inputs(shape, kind, regions, ig, 0.3, seed=7)
    l1, g1 = hip_loss(kind, logits, lab, regions, ig)
    l2, g2 = hip_loss(kind, logits, lab, regions, ig)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)


# ---- (d) region conversion on the device, bit for bit
@pytest.mark.parametrize("shape,regions,ig", [((2, 1, 64, 64), [(1, 2, 3), (2, 3), (3,)], 4), ((3, 1, 17, 23), [1, (1, 2)], None),
                                              ((1, 1, 33, 8), [(0, 63), 5, (62, 63), 7, 8, 9, 10, (11, 12)], 64),
                                              ((2, 1, 5, 3), [(2,)], -1)])
def test_hip_labels_to_regions_matches_cpu(shape, regions, ig):
    from dinounet_amd.training import labels_to_regions
    d = dev()
    g = torch.Generator().manual_seed(8)
    lab = torch.randint(-3, 70, shape, generator=g)          # includes -1, labels >= 64 and 63
    lab.view(-1)[:4] = torch.tensor([-1, 64, 63, 200])
    got = labels_to_regions(lab.to(d), regions, ig)
    want = labels_to_regions(lab, regions, ig)
    assert got.dtype == torch.uint8 and torch.equal(got.cpu(), want)


# ---- (e) TrainStep with build_loss: the captured step against eager
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


@pytest.mark.parametrize("cfg", [dict(num_classes=2, regions=[(1, 2), (2,)], ignore_label=3), dict(num_classes=3, ignore_label=3)])
def test_train_step_with_build_loss_hipgraph_matches_eager(cfg):
    """8 steps eager vs captured (the bound of test_train_step_hipgraph_matches_eager); every gradient finite."""
    from oracle import weights
    from dinounet_amd.training import TrainStep, build_loss
    from dinounet_amd.optim import FusedClipSGD
    d = dev()
    x = weights.make_input(4, 3, 128, 128, seed=3).to(d)
    lab = weights.make_target(4, 128, 128, 3, seed=3)
    g = torch.Generator().manual_seed(9)
    lab = torch.where(torch.rand(lab.shape, generator=g) < 0.3, torch.full_like(lab, cfg["ignore_label"]), lab).to(d)
    losses = {}
    for mode in (False, True):
        net = _net(cfg["num_classes"], d)
        params = [p for p in net.parameters() if p.requires_grad]
        if mode:
            opt = FusedClipSGD(params, 1e-3, momentum=0.99, nesterov=True, weight_decay=3e-5)
        else:
            opt = torch.optim.SGD(params, 1e-3, momentum=0.99, nesterov=True, weight_decay=3e-5)
        loss_fn = build_loss(**cfg)
        ts = TrainStep(net, opt, params, x.shape, lab.shape, d, graph=mode, warmup=2, loss=loss_fn)
        ls = [float(ts(x, lab))] + [float(ts()) for _ in range(7)]
        torch.cuda.synchronize()
        if mode:
            assert ts.capture_mode == "whole_step", ts.capture_mode
        assert all(np.isfinite(ls)), (mode, ls)
        assert all(torch.isfinite(p.grad).all() for p in params if p.grad is not None)
        losses[mode] = ls
    print(cfg, "eager", losses[False], "graph", losses[True])
    assert max(abs(a - b) for a, b in zip(losses[False], losses[True])) < 5e-3


# ---- (f) two ranks on one GPU over gloo against the reference's world-2 run (fixture case 5)
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
            loss, grad = hip_loss(c["kind"], logits, labels, _regions(c), c["ignore_label"], group=dist.group.WORLD)
            out[n] = (float(loss), grad.cpu().numpy().copy())
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
            loss, grad = res[r][n]
            _assert_close(loss, torch.from_numpy(grad), float(g[f"{n}/loss"][r]), g[f"{n}/grad"][r:r + 1], f"{n} rank {r}")
