"""GPU tests (-m gpu) of the fused deep-supervision loss (csrc/loss.hip du_ds_loss_* / du_downsample_seg, ops.ds_seg_loss,
training.DeepSupervisionLoss): against the reference's fp64 DeepSupervisionWrapper fixture (tests/golden/deep_supervision_reference.npz),
against the fp64 CPU formula across a sweep of the three label modes, exact properties (S = 1, a NaN zero-weight scale, one all-ignored
scale, bit-reproducibility, the launch count), the materialised pyramid bit for bit, TrainStep captured vs eager, ValStep, two ranks.

Bounds: |loss - ref| <= 2e-5 max(1, |ref|), per-scale gradient rel (test_gpu_ops.rel) <= 2e-4: the bounds test_gpu_seg_loss.py applies
to the same per-pixel arithmetic."""
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from test_gpu_ops import dev, rel

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deep_supervision_reference.npz")
LOSS_TOL, GRAD_TOL = 2e-5, 2e-4
REGION_SETS = {1: [(1, 2)], 2: [1, (1, 2)], 3: [(1, 2, 3), (2, 3), (3,)],
               8: [1, 2, 3, 4, (1, 2), (3, 4), (5, 6), (1, 2, 3, 4, 5, 6)]}


def _fixture():
    g = np.load(GOLD)
    return g, json.loads(str(g["meta"]))


def _regions(c):
    return None if c["regions"] is None else [r if isinstance(r, int) else tuple(r) for r in c["regions"]]


def _module(C_, regions, ignore_label, weights, ddp=False, group=None):
    from dinounet_amd.training import build_loss
    return build_loss(C_, regions=regions, ignore_label=ignore_label, ddp=ddp, group=group, deep_supervision_weights=weights)


def hip_loss(mod, logits, labels, go=1.0):
    """fused loss, per-scale losses and d (go * loss) / d logits_s on the GPU"""
    d = dev()
    xs = [x.to(d).float().requires_grad_(True) for x in logits]
    loss, losses = mod(xs, labels.to(d), return_scale_losses=True)
    (loss * go).backward()
    torch.cuda.synchronize()
    return loss.detach(), losses.detach().cpu(), [x.grad for x in xs]


def cpu_ref(mod, logits, labels, go=1.0):
    """the product's fp64 torch formula (pinned to the reference's wrapper by tests/test_cpu_deep_supervision.py)"""
    xs = [x.detach().cpu().double().requires_grad_(True) for x in logits]
    loss = mod(xs, labels.cpu())
    (loss * go).backward()
    return float(loss.detach()), [x.grad for x in xs]


def _assert_close(weights, loss, grads, ref_loss, ref_grads, what):
    dl = abs(float(loss) - ref_loss)
    print(f"{what}: |dloss| {dl:.3e} (ref {ref_loss:.6f})")
    assert dl <= LOSS_TOL * max(1.0, abs(ref_loss)), (what, float(loss), ref_loss)
    for s, w in enumerate(weights):
        if w == 0.0:
            assert grads[s] is None and ref_grads[s] is None, (what, s)
            continue
        rg = rel(grads[s], torch.as_tensor(ref_grads[s]))
        print(f"    scale {s}: grad rel {rg:.3e}")
        assert rg <= GRAD_TOL, (what, s, rg)


# ---- (a) every fixture case (world 1)
@pytest.mark.parametrize("name", ["ds_plain", "ds_ce_ignore", "ds_regions_ignore"])
def test_hip_matches_reference_fixture(name):
    g, meta = _fixture()
    c = [c for c in meta["cases"] if c["name"] == name][0]
    S = 1 + len(c["lower"])
    logits = [torch.from_numpy(g[f"{name}/logits{s}"]) for s in range(S)]
    labels = torch.from_numpy(g[f"{name}/labels"].astype(np.int64))
    mod = _module(c["shape"][1], _regions(c), c["ignore_label"], c["weights"])
    loss, _, grads = hip_loss(mod, logits, labels)
    ref_grads = [g[f"{name}/grad{s}"] if f"{name}/grad{s}" in g.files else None for s in range(S)]
    _assert_close(c["weights"], loss, grads, float(g[f"{name}/loss"]), ref_grads, name)


# ---- (b) sweep against the fp64 CPU formula: partial quads, quads that straddle rows, w_s < 4, HW % 4 != 0
def _pyramid(H, W, S):
    out = [(H, W)]
    for _ in range(S - 1):
        out.append((max(1, round(out[-1][0] * 0.5)), max(1, round(out[-1][1] * 0.5))))
    return out


def _inputs(shape, S, mode, regions, ignore_label, seed, frac=0.3):
    B, C_, H, W = shape
    g = torch.Generator().manual_seed(seed)
    logits = [torch.randn((B, C_, h, w), generator=g) * 2.0 for h, w in _pyramid(H, W, S)]
    top = C_ if not mode.startswith("regions") else max(max((r,) if isinstance(r, int) else r) for r in regions) + 1
    lab = torch.randint(0, top, (B, 1, H, W), generator=g)
    if ignore_label is not None:
        lab = torch.where(torch.rand((B, 1, H, W), generator=g) < frac, torch.full_like(lab, ignore_label), lab)
    return logits, lab


def _sweep():
    from dinounet_amd.training import deep_supervision_weights
    out = []
    for mode in ("softmax", "softmax_ignore", "regions", "regions_ignore"):
        for shape in [(2, 3, 16, 16), (1, 2, 20, 12), (2, 8, 18, 10), (1, 1, 9, 7)]:
            if shape[1] == 1 and not mode.startswith("regions"):
                continue                                   # one output plane exists in region mode only
            for S, ddpw in ((1, True), (2, True), (3, True), (3, False)):
                out.append(pytest.param(mode, shape, tuple(deep_supervision_weights(S, ddp=ddpw)), id=f"{mode}-{shape}-S{S}{'d' if ddpw else ''}"))
    return out


@pytest.mark.parametrize("mode,shape,weights", _sweep())
def test_sweep_matches_fp64_formula(mode, shape, weights):
    C_ = shape[1]
    regions = REGION_SETS[C_] if mode.startswith("regions") else None
    ig = None if mode in ("softmax", "regions") else (C_ if regions is None else 9)       # 9: in no region, above every class count
    logits, lab = _inputs(shape, len(weights), mode, regions, ig, seed=sum(shape) + len(weights))
    mod = _module(C_, regions, ig, weights)
    loss, _, grads = hip_loss(mod, logits, lab, go=1.7)
    ref_loss, ref_grads = cpu_ref(mod, logits, lab, go=1.7)
    _assert_close(weights, loss, grads, ref_loss, ref_grads, f"{mode} {shape} {weights}")


# ---- (c) exact properties
@pytest.mark.parametrize("mode", ["softmax", "softmax_ignore", "regions"])
def test_one_scale_with_weight_one_is_the_single_scale_loss(mode):
    from dinounet_amd.training import build_loss
    shape = (2, 3, 18, 10)
    regions = REGION_SETS[3] if mode == "regions" else None
    ig = 3 if mode == "softmax_ignore" else (4 if mode == "regions" else None)
    logits, lab = _inputs(shape, 1, mode, regions, ig, seed=5)
    d = dev()
    single = build_loss(3, regions=regions, ignore_label=ig)(logits[0].to(d), lab.to(d))
    loss, losses, _ = hip_loss(_module(3, regions, ig, [1.0]), logits, lab)
    ref = float(single)
    assert abs(float(loss) - ref) <= LOSS_TOL * max(1.0, abs(ref)), (float(loss), ref)
    assert abs(float(losses[0]) - ref) <= LOSS_TOL * max(1.0, abs(ref))


def test_zero_weight_scale_of_nans_is_never_read():
    logits, lab = _inputs((2, 3, 16, 16), 3, "softmax", None, None, seed=11)
    logits[2] = torch.full_like(logits[2], float("nan"))
    loss, losses, grads = hip_loss(_module(3, None, None, [2 / 3, 1 / 3, 0.0]), logits, lab)
    assert torch.isfinite(loss) and torch.isfinite(losses).all()
    assert grads[2] is None and torch.isfinite(grads[0]).all() and torch.isfinite(grads[1]).all()


@pytest.mark.parametrize("mode", ["softmax_ignore", "regions"])
def test_one_all_ignored_scale_is_exactly_minus_one_with_zero_gradient(mode):
    """the ignore label on exactly the odd-row, odd-column pixels of a 16 x 16 map: scale 1 (8 x 8) samples rows / columns 1, 3, 5, ...
    and is all-ignored; scale 0 keeps three quarters of its pixels, scale 2 (4 x 4) samples rows / columns 2, 6, 10, 14"""
    regions = REGION_SETS[3] if mode == "regions" else None
    ig = 3 if mode == "softmax_ignore" else 7
    logits, lab = _inputs((2, 3, 16, 16), 3, mode, regions, None, seed=21)
    lab[:, :, 1::2, 1::2] = ig
    loss, losses, grads = hip_loss(_module(3, regions, ig, [0.5, 0.3, 0.2]), logits, lab)
    assert float(losses[1]) == -1.0, losses
    assert grads[1].abs().max().item() == 0.0
    assert float(losses[0]) != -1.0 and float(losses[2]) != -1.0 and grads[0].abs().max() > 0 and grads[2].abs().max() > 0
    assert torch.isfinite(loss)


@pytest.mark.parametrize("mode,shape", [("softmax", (2, 3, 64, 64)), ("regions", (2, 3, 18, 10))])
def test_two_calls_are_bit_identical(mode, shape):
    regions = REGION_SETS[3] if mode == "regions" else None
    ig = 4 if mode == "regions" else None
    logits, lab = _inputs(shape, 3, mode, regions, ig, seed=31)
    mod = _module(3, regions, ig, [0.5, 0.3, 0.2])
    a = hip_loss(mod, logits, lab)
    b = hip_loss(mod, logits, lab)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(x, y) for x, y in zip(a[2], b[2]))


def test_three_scales_cost_four_launches(monkeypatch):
    """the count is derived from the design (du_ds_loss_sums: partial rows + per-scale row sums, du_ds_loss_finish, du_ds_loss_bwd, one
    launch each as include/dinounet_hip.h states) and checked by counting the library calls the autograd function makes"""
    from dinounet_amd import _lib, ops
    launches = {"du_ds_loss_sums": 2, "du_ds_loss_finish": 1, "du_ds_loss_bwd": 1, "du_ds_loss_ws_elems": 0}
    real, calls = _lib.lib(), []

    class Counting:
        def __getattr__(self, name):
            fn = getattr(real, name)

            def call(*a):
                calls.append(name)
                return fn(*a)
            return call

    logits, lab = _inputs((2, 3, 16, 16), 3, "softmax", None, None, seed=41)
    mod = _module(3, None, None, [0.5, 0.3, 0.2])
    monkeypatch.setattr(ops._lib, "lib", lambda: Counting())
    hip_loss(mod, logits, lab)
    monkeypatch.undo()
    calls = [c for c in calls if c != "du_device_ok"]               # (dev() asks the library for the device)
    assert sorted(set(calls)) == sorted(launches), calls            # no other library call (no labels_to_regions, no per-scale loss)
    assert sum(launches[c] for c in calls) == 4, calls


# ---- (d) the materialised pyramid, bit for bit (labels -1 and >= 64 included)
@pytest.mark.parametrize("shape", [(2, 1, 20, 12), (1, 1, 9, 7), (1, 1, 148, 37)])
def test_downsample_seg_for_ds_is_bit_equal_to_host_indexing(shape):
    """(148 -> 18 holds a tie that scipy's fp64 rounding decides downwards: the kernel's fp64 steps must not be contracted)"""
    from dinounet_amd.dataloading import downsample_seg_for_ds
    g = torch.Generator().manual_seed(3)
    seg = torch.randint(-1, 70, shape, generator=g)
    entries = [[1.0, 1.0], [0.5, 0.5], [0.25, 0.25], 0.125, (3, 2)]
    want = downsample_seg_for_ds(seg, entries)
    got = downsample_seg_for_ds(seg.to(dev()), entries)
    torch.cuda.synchronize()
    assert len(got) == len(want) == 5 and got[0].is_cuda
    for a, b in zip(got, want):
        assert a.dtype == torch.int64 and a.shape == b.shape and torch.equal(a.cpu(), b)


# ---- (e) TrainStep / ValStep with the deep-supervision network
def _net(num_classes, d):
    from oracle import weights
    from oracle.refshim import PLANS_2D
    from dinounet_amd.dinov3.adapter import DropPath
    from dinounet_amd.network_architecture import DinoUNet
    plans = dict(PLANS_2D, architecture=dict(PLANS_2D["architecture"], deep_supervision=True))
    net = DinoUNet.from_config(plans, 3, num_classes, dinov3_pretrained_path=None, dinov3_model_name="dinounet_s", precision="bf16")
    assert net.decoder.deep_supervision is True
    ks = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    net.load_state_dict(weights.make_state_dict(ks, seed=0), strict=True)
    net = net.to(d).train()
    for m in net.modules():
        if isinstance(m, DropPath):
            m.drop_prob = 0.0
    net.encoder.dinov3_adapter.backbone.rope_embed.rescale_coords = None
    return net


def test_train_step_with_deep_supervision_hipgraph_matches_eager():
    """8 steps eager vs captured (bound and set-up of test_train_step_with_build_loss_hipgraph_matches_eager); every gradient finite,
    the second segmentation head's included"""
    from oracle import weights
    from dinounet_amd.training import TrainStep, build_loss, deep_supervision_weights
    from dinounet_amd.optim import FusedClipSGD
    d = dev()
    x = weights.make_input(4, 3, 128, 128, seed=3).to(d)
    lab = weights.make_target(4, 128, 128, 3, seed=3)
    g = torch.Generator().manual_seed(9)
    lab = torch.where(torch.rand(lab.shape, generator=g) < 0.3, torch.full_like(lab, 3), lab).to(d)
    losses = {}
    for mode in (False, True):
        net = _net(3, d)
        params = [p for p in net.parameters() if p.requires_grad]
        if mode:
            opt = FusedClipSGD(params, 1e-3, momentum=0.99, nesterov=True, weight_decay=3e-5)
        else:
            opt = torch.optim.SGD(params, 1e-3, momentum=0.99, nesterov=True, weight_decay=3e-5)
        loss_fn = build_loss(3, ignore_label=3, deep_supervision_weights=deep_supervision_weights(3))
        ts = TrainStep(net, opt, params, x.shape, lab.shape, d, graph=mode, warmup=2, loss=loss_fn)
        ls = [float(ts(x, lab))] + [float(ts()) for _ in range(7)]
        torch.cuda.synchronize()
        if mode:
            assert ts.capture_mode == "whole_step", ts.capture_mode
        assert all(np.isfinite(ls)), (mode, ls)
        assert all(torch.isfinite(p.grad).all() for p in params if p.grad is not None)
        head1 = dict(net.named_parameters())["decoder.seg_layers.1.weight"]
        assert head1.grad is not None and torch.isfinite(head1.grad).all() and head1.grad.abs().max() > 0
        losses[mode] = ls
    print("eager", losses[False], "graph", losses[True])
    assert max(abs(a - b) for a, b in zip(losses[False], losses[True])) < 5e-3


def test_val_step_reports_the_multi_scale_loss_and_full_resolution_counts():
    from oracle import weights
    from dinounet_amd.training import ValStep, build_loss, deep_supervision_weights, validation_counts
    d = dev()
    x = weights.make_input(2, 3, 128, 128, seed=4).to(d)
    lab = weights.make_target(2, 128, 128, 3, seed=4)
    g = torch.Generator().manual_seed(10)
    lab = torch.where(torch.rand(lab.shape, generator=g) < 0.3, torch.full_like(lab, 3), lab).to(d)
    net = _net(3, d)
    loss_fn = build_loss(3, ignore_label=3, deep_supervision_weights=deep_supervision_weights(3))
    vs = ValStep(net, x.shape, lab.shape, d, loss=loss_fn, graph=False)
    got = float(vs(x, lab))
    net.eval()
    with torch.no_grad():
        outs = net(x)
        want = float(loss_fn(outs, lab))
        single = float(loss_fn.base(outs[0], lab))
    net.train()
    tp, fp, fn = validation_counts(outs[0], lab, ignore_label=3)
    torch.cuda.synchronize()
    assert abs(got - want) <= LOSS_TOL * max(1.0, abs(want)), (got, want)
    assert abs(want - single) > 1e-4, "the multi-scale loss must differ from the single-scale loss for this to show anything"
    assert torch.equal(vs.step_counts.cpu(), torch.stack([tp, fp, fn]).cpu())


# ---- (f) two ranks on one GPU over gloo against the reference's world-2 run
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
            S = 1 + len(c["lower"])
            logits = [torch.from_numpy(g[f"{n}/logits{s}"])[rank:rank + 1] for s in range(S)]
            labels = torch.from_numpy(g[f"{n}/labels"].astype(np.int64))[rank:rank + 1]
            mod = _module(c["shape"][1], _regions(c), c["ignore_label"], c["weights"], ddp=True, group=dist.group.WORLD)
            loss, _, grads = hip_loss(mod, logits, labels)
            out[n] = (float(loss), [x.cpu().numpy().copy() for x in grads])
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
            loss, grads = res[r][n]
            ref = [g[f"{n}/grad{s}"][r:r + 1] for s in range(len(grads))]
            _assert_close(c["weights"], loss, [torch.from_numpy(x) for x in grads], float(g[f"{n}/loss"][r]), ref, f"{n} rank {r}")
