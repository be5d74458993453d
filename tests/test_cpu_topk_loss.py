"""CPU suite (-m "not gpu") of the top-k losses (training.topk_ce_loss / dc_and_topk_loss, build_loss(topk_percent=...); the
reference's TopKLoss, robust_ce_loss.py:19-32, and DC_and_topk_loss, compound_losses.py:102-150): the torch formulas in fp64 against the
reference's own classes (tests/golden/topk_loss_reference.npz, tools/make_golden_topk_loss.py) with the world-2 gloo case, the k_vox
arithmetic and host validation, the deep-supervision composition, k = 100 against dc_and_ce_loss, and the C-ABI argument checks.

Tolerance 1e-10 (relative), the bound tests/test_cpu_seg_loss.py applies to its fixture: both sides are fp64 and differ only in
summation order.  Every fixture threshold is isolated by >= 1e-3 (asserted by the generator), so both sides select the same voxels."""
import ctypes
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "topk_loss_reference.npz")
TOL = 1e-10


def _fixture():
    g = np.load(GOLD)
    return g, json.loads(str(g["meta"]))


def _cases(world):
    return [c for c in _fixture()[1]["cases"] if c["world"] == world]


def cpu_loss(kind, logits, labels, ignore_label, k, ddp=False):
    """the product's torch formula (CPU path) in fp64: loss, d loss / d logits"""
    from dinounet_amd import training as T
    x = logits.double().requires_grad_(True)
    if kind == "topk":
        loss = T.topk_ce_loss(x, labels, k, ignore_label=ignore_label)
    else:
        loss = T.dc_and_topk_loss(x, labels, k, ddp=ddp, ignore_label=ignore_label)
    (g,) = torch.autograd.grad(loss, x)
    return float(loss.detach()), g


def _check(loss, grad, ref_loss, ref_grad, what):
    ref_grad = torch.as_tensor(ref_grad)
    assert abs(loss - ref_loss) <= TOL * abs(ref_loss), (what, loss, ref_loss)
    gmax = float(ref_grad.abs().max())
    err = float((grad - ref_grad).abs().max())
    assert err <= TOL * gmax, (what, err, gmax)          # an all-zero reference gradient must be matched exactly


@pytest.mark.parametrize("name", [c["name"] for c in _cases(1)])
def test_cpu_formula_matches_reference_fixture(name):
    g, meta = _fixture()
    c = [c for c in meta["cases"] if c["name"] == name][0]
    logits = torch.from_numpy(g[f"{name}/logits"])
    labels = torch.from_numpy(g[f"{name}/labels"].astype(np.int64))
    loss, grad = cpu_loss(c["kind"], logits, labels, c["ignore_label"], c["k"])
    _check(loss, grad, float(g[f"{name}/loss"]), g[f"{name}/grad"], name)


def test_fixture_cases_and_gaps():
    """the cases the fixture must hold, k_vox in the reference's arithmetic, and an isolated threshold wherever gradients are compared"""
    from dinounet_amd.training import topk_voxels
    g, meta = _fixture()
    want = {"plain": ((2, 3, 32, 32), None, 10, 204), "ignore": ((2, 4, 32, 32), 4, 10, 204), "tail": ((3, 4, 17, 23), None, 10, 117),
            "k8": ((1, 8, 32, 32), None, 25, 256), "half_ignore": ((1, 3, 16, 16), 3, 50, 128)}
    by_name = {c["name"]: c for c in meta["cases"]}
    for n, (shape, ig, k, k_vox) in want.items():
        c = by_name[n]
        assert (tuple(c["shape"]), c["ignore_label"], c["k"]) == (shape, ig, k) and int(g[f"{n}/k_vox"]) == k_vox
    assert {"all_ignored", "topk_only", "ddp"} <= set(by_name) and by_name["topk_only"]["kind"] == "topk" and by_name["ddp"]["world"] == 2
    for c in meta["cases"]:
        n = c["name"]
        B, _, H, W = c["shape"]
        assert np.all(g[f"{n}/k_vox"] == topk_voxels((B // c["world"]) * H * W, c["k"]))
        if n != "all_ignored":
            assert np.all(g[f"{n}/gap"] >= 1e-3), (n, g[f"{n}/gap"])
    # every voxel ignored: CE part 0, Dice 1 per class, no gradient
    assert float(g["all_ignored/loss"]) == -1.0 and float(np.abs(g["all_ignored/grad"]).max()) == 0.0


def test_k_vox_arithmetic_and_value_errors():
    from dinounet_amd import training as T
    assert T.topk_voxels(2048, 10) == 204 and T.topk_voxels(1173, 10) == 117 and T.topk_voxels(256, 50) == 128
    assert T.topk_voxels(16, 100) == 16 and T.topk_voxels(8 * 512 * 512, 10) == 209715 and T.topk_voxels(1000, 0.1) == 1
    assert T.topk_voxels(2 ** 31 - 1, 100) == 2 ** 31 - 1
    for n, k in [(2048, 10), (391, 33.3), (1173, 7), (16, 6.25)]:
        assert T.topk_voxels(n, k) == int(np.int64(n) * k / 100)
    for bad in (0, -1, 100.5, 1000, float("nan"), None, "10", True):
        with pytest.raises(ValueError):
            T.topk_voxels(1000, bad)
    with pytest.raises(ValueError):                     # the reference returns nan (the mean of an empty topk)
        T.topk_voxels(9, 10)
    x, t = torch.randn(1, 3, 3, 3, dtype=torch.float64), torch.randint(0, 3, (1, 1, 3, 3))
    for fn in (T.topk_ce_loss, T.dc_and_topk_loss):
        with pytest.raises(ValueError):
            fn(x, t, 10)                                # 9 voxels: k_vox = 0
        with pytest.raises(ValueError):
            fn(x, t, 0)
        with pytest.raises(ValueError):
            fn(x, t, 101)
    with pytest.raises(ValueError):
        T.build_loss(3, topk_percent=0)
    with pytest.raises(ValueError):
        T.build_loss(3, topk_percent=150)
    with pytest.raises(ValueError):                     # the reference has no region-based top-k loss
        T.build_loss(2, regions=[1, (1, 2)], topk_percent=10)
    with pytest.raises(ValueError):
        T.SegLoss(2, regions=[1, (1, 2)], ignore_label=3, topk_percent=10)


def test_build_loss_modes_and_module_equals_the_functions():
    from dinounet_amd import training as T
    assert T.build_loss(3, topk_percent=10).mode == "topk" and T.build_loss(3, ignore_label=3, topk_percent=10).mode == "topk_ignore"
    assert T.build_loss(3).mode == "softmax" and T.build_loss(3, ignore_label=3).mode == "softmax_ignore"      # unchanged
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 10, 12, generator=g, dtype=torch.float64)
    t = torch.randint(0, 4, (2, 1, 10, 12), generator=g)
    t3 = t.clamp_max(2)
    assert float(T.build_loss(3, topk_percent=20)(x, t3)) == float(T.dc_and_topk_loss(x, t3, 20))
    assert float(T.build_loss(3, ignore_label=3, topk_percent=20)(x, t)) == float(T.dc_and_topk_loss(x, t, 20, ignore_label=3))
    # the loss is the top-k mean of the per-voxel CE minus the Dice term of the masked Dice + CE loss
    v = torch.nn.functional.cross_entropy(x, t[:, 0], reduction="none", ignore_index=3).reshape(-1)
    k_vox = T.topk_voxels(v.numel(), 20)
    m = t[:, 0] != 3
    ce_masked = v.sum() / m.sum()
    dice = ce_masked - T.dc_and_ce_loss(x, t, ignore_label=3)
    want = torch.sort(v, descending=True)[0][:k_vox].mean() - dice
    assert abs(float(T.dc_and_topk_loss(x, t, 20, ignore_label=3)) - float(want)) <= 1e-12


def test_build_loss_accepts_every_percentage_in_range_whatever_100_voxels_would_give():
    """the constructor checks the range only; k_vox is a matter of the shape of each call (0.5 % of 240 voxels is 1 voxel, of 100 none)"""
    from dinounet_amd import training as T
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 3, 10, 12, generator=g, dtype=torch.float64)
    t = torch.randint(0, 3, (2, 1, 10, 12), generator=g)
    for k in (0.5, 0.99, 1e-3, 100):
        m = T.build_loss(3, topk_percent=k)
        assert m.mode == "topk" and m.topk_percent == k
        T.build_loss(3, ignore_label=3, topk_percent=k, deep_supervision_weights=T.deep_supervision_weights(3))
    assert T.topk_voxels(240, 0.5) == 1
    loss = T.build_loss(3, topk_percent=0.5)(x, t)
    v = torch.nn.functional.cross_entropy(x, t[:, 0], reduction="none")
    assert float(loss) == float(T.dc_and_topk_loss(x, t, 0.5)) and torch.isfinite(loss)
    assert abs(float(loss) - float(v.max() - T._soft_dice_torch(x, t, None, 1e-5, False, None))) <= 1e-12
    with pytest.raises(ValueError):                     # a valid k that selects nothing AT THIS SHAPE: raised by the call, not the constructor
        T.build_loss(3, topk_percent=0.1)(x, t)
    for bad in (0, -1, 100.5, float("nan"), None, "10", True):
        with pytest.raises(ValueError):
            T.check_topk_percent(bad)


def test_fused_route_limits():
    """the fused kernels serve a GPU tensor with 2..8 classes and fewer than 2^31 voxels; everything else takes the torch formula"""
    from dinounet_amd.training import topk_fused
    assert topk_fused(True, 2, 16) and topk_fused(True, 8, 2 ** 31 - 1)
    assert not topk_fused(True, 3, 2 ** 31) and not topk_fused(True, 3, 2 ** 33)
    assert not topk_fused(True, 9, 1024) and not topk_fused(True, 1, 1024) and not topk_fused(False, 3, 1024)


def test_k100_without_ignore_label_equals_dc_and_ce_loss():
    from dinounet_amd import training as T
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 4, 9, 11, generator=g, dtype=torch.float64).requires_grad_(True)
    t = torch.randint(0, 4, (2, 1, 9, 11), generator=g)
    a, b = T.dc_and_topk_loss(x, t, 100), T.dc_and_ce_loss(x, t)
    assert abs(float(a.detach()) - float(b.detach())) <= 1e-12 * abs(float(b.detach()))
    (ga,), (gb,) = torch.autograd.grad(a, x), torch.autograd.grad(b, x)
    assert float((ga - gb).abs().max()) <= 1e-12 * float(gb.abs().max())


def test_deep_supervision_composes_the_per_scale_topk_losses():
    from dinounet_amd import training as T
    g = torch.Generator().manual_seed(7)
    outs = [torch.randn(2, 3, h, w, generator=g, dtype=torch.float64) for h, w in ((24, 20), (12, 10), (6, 5))]
    t = torch.randint(0, 4, (2, 1, 24, 20), generator=g)
    w = T.deep_supervision_weights(3)
    m = T.build_loss(3, ignore_label=3, deep_supervision_weights=w, topk_percent=10)
    assert isinstance(m, T.DeepSupervisionLoss) and m.mode == "topk_ignore" and not m.fused(outs)
    want = sum(wi * T.dc_and_topk_loss(o, T.downsample_target(t, o.shape[-2:]), 10, ignore_label=3) for wi, o in zip(w, outs) if wi != 0)
    assert float(m(outs, t)) == float(want)
    # every scale has its own N and k_vox: the lowest scale (60 voxels at 10 %) would select 6
    assert T.topk_voxels(2 * 6 * 5, 10) == 6 and T.topk_voxels(2 * 24 * 20, 10) == 96


# ---- world 2 over gloo: the torch formula with ddp=True against the reference's ddp=True run
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _ddp_worker(rank, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=2)
        g, meta = _fixture()
        out = {}
        for c in [c for c in meta["cases"] if c["world"] == 2]:
            n = c["name"]
            logits = torch.from_numpy(g[f"{n}/logits"])[rank:rank + 1]
            labels = torch.from_numpy(g[f"{n}/labels"].astype(np.int64))[rank:rank + 1]
            loss, grad = cpu_loss(c["kind"], logits, labels, c["ignore_label"], c["k"], ddp=True)
            out[n] = (loss, grad.numpy().copy())
        q.put((rank, out))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc()))


def test_ddp_world2_formula_matches_reference_fixture():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_ddp_worker, args=(r, port, q)) for r in range(2)]
    [p.start() for p in procs]
    res = dict(q.get(timeout=180) for _ in range(2))
    [p.join(timeout=60) for p in procs]
    for r in range(2):
        assert not isinstance(res[r], str), res[r]
    assert all(p.exitcode == 0 for p in procs)
    g, _ = _fixture()
    for c in _cases(2):
        n = c["name"]
        for r in range(2):
            loss, grad = res[r][n]
            _check(loss, torch.from_numpy(grad), float(g[f"{n}/loss"][r]), g[f"{n}/grad"][r:r + 1], (n, r))


# ---- C ABI: bad arguments are refused before any launch, so this runs without a device
def test_topk_loss_c_abi_argument_validation_without_gpu():
    from dinounet_amd import _lib
    L = _lib.lib()
    BAD, UNS = -1, -2
    fake = ctypes.c_void_p(256)           # never dereferenced: every call below is refused before a launch
    big = 1 << 24
    assert L.du_topk_loss_ws_elems(2, 4, 1024) > 0 and L.du_topk_loss_ws_elems(2, 9, 1024) == 0 and L.du_topk_loss_ws_elems(2, 1, 64) == 0
    assert L.du_topk_loss_ws_elems(0, 3, 64) == 0 and L.du_topk_loss_ws_elems(2, 3, 0) == 0
    assert L.du_topk_loss_ws_elems(1, 3, 2 ** 31 - 1) > 0 and L.du_topk_loss_ws_elems(2, 3, 2 ** 30) == 0       # B HW < 2^31
    need = L.du_topk_loss_ws_elems(2, 4, 64)
    # forward: (logits, target, values, sums, B, K, HW, has_ignore, ignore_label, k_vox, ws, ws_elems, stream)
    assert L.du_topk_loss_fwd(None, fake, fake, fake, 2, 4, 64, 0, 0, 12, fake, big, None) == BAD
    assert L.du_topk_loss_fwd(fake, None, fake, fake, 2, 4, 64, 0, 0, 12, fake, big, None) == BAD
    assert L.du_topk_loss_fwd(fake, fake, None, fake, 2, 4, 64, 0, 0, 12, fake, big, None) == BAD
    assert L.du_topk_loss_fwd(fake, fake, fake, None, 2, 4, 64, 0, 0, 12, fake, big, None) == BAD
    assert L.du_topk_loss_fwd(fake, fake, fake, fake, 2, 4, 64, 0, 0, 12, None, big, None) == BAD
    assert L.du_topk_loss_fwd(fake, fake, fake, fake, 0, 4, 64, 0, 0, 12, fake, big, None) == BAD
    assert L.du_topk_loss_fwd(fake, fake, fake, fake, 2, 4, 2 ** 30, 0, 0, 12, fake, big, None) == BAD           # B HW >= 2^31
    assert L.du_topk_loss_fwd(fake, fake, fake, fake, 2, 4, 64, 2, 4, 12, fake, big, None) == BAD                # has_ignore is 0 or 1
    assert L.du_topk_loss_fwd(fake, fake, fake, fake, 2, 4, 64, 0, 0, 0, fake, big, None) == BAD                 # k_vox outside 1..N
    assert L.du_topk_loss_fwd(fake, fake, fake, fake, 2, 4, 64, 0, 0, 129, fake, big, None) == BAD
    assert L.du_topk_loss_fwd(fake, fake, fake, fake, 2, 4, 64, 0, 0, -3, fake, big, None) == BAD
    assert L.du_topk_loss_fwd(fake, fake, fake, fake, 2, 4, 64, 0, 0, 12, fake, need - 1, None) == BAD           # scratch too small
    assert L.du_topk_loss_fwd(fake, fake, fake, fake, 2, 4, 64, 0, 0, 12, ctypes.c_void_p(260), big, None) == BAD   # scratch alignment
    assert L.du_topk_loss_fwd(fake, fake, fake, fake, 2, 9, 64, 0, 0, 12, fake, big, None) == UNS
    assert L.du_topk_loss_fwd(fake, fake, fake, fake, 2, 1, 64, 0, 0, 12, fake, big, None) == UNS
    # finish: (sums, values, ws, ws_elems, sel, loss, coef, info, B, K, HW, k_vox, dice, smooth, grad_mult, stream)
    assert L.du_topk_loss_finish(None, fake, fake, big, fake, fake, fake, fake, 2, 4, 64, 12, 1, 1e-5, 1.0, None) == BAD
    assert L.du_topk_loss_finish(fake, fake, fake, big, None, fake, fake, fake, 2, 4, 64, 12, 1, 1e-5, 1.0, None) == BAD
    assert L.du_topk_loss_finish(fake, fake, fake, big, fake, fake, fake, None, 2, 4, 64, 12, 1, 1e-5, 1.0, None) == BAD
    assert L.du_topk_loss_finish(fake, fake, fake, big, fake, fake, fake, fake, 2, 4, 64, 0, 1, 1e-5, 1.0, None) == BAD
    assert L.du_topk_loss_finish(fake, fake, fake, big, fake, fake, fake, fake, 2, 4, 64, 129, 1, 1e-5, 1.0, None) == BAD
    assert L.du_topk_loss_finish(fake, fake, fake, big, fake, fake, fake, fake, 2, 4, 64, 12, 2, 1e-5, 1.0, None) == BAD
    assert L.du_topk_loss_finish(fake, fake, fake, need - 1, fake, fake, fake, fake, 2, 4, 64, 12, 1, 1e-5, 1.0, None) == BAD
    assert L.du_topk_loss_finish(fake, fake, fake, big, fake, fake, fake, fake, 2, 9, 64, 12, 1, 1e-5, 1.0, None) == UNS
    # backward: (logits, target, sel, coef, grad_out, dlogits, B, K, HW, has_ignore, ignore_label, stream)
    assert L.du_topk_loss_bwd(fake, fake, None, fake, None, fake, 2, 4, 64, 0, 0, None) == BAD
    assert L.du_topk_loss_bwd(fake, fake, fake, fake, None, None, 2, 4, 64, 0, 0, None) == BAD
    assert L.du_topk_loss_bwd(fake, fake, fake, fake, None, fake, 2, 4, 0, 0, 0, None) == BAD
    assert L.du_topk_loss_bwd(fake, fake, fake, fake, None, fake, 2, 4, 64, 3, 0, None) == BAD
    assert L.du_topk_loss_bwd(fake, fake, fake, fake, None, fake, 2, 16, 64, 0, 0, None) == UNS
