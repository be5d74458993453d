"""CPU suite (-m "not gpu") of the loss options (training.build_loss / SegLoss weight_ce, weight_dice, batch_dice, do_bg,
ce_class_weights; csrc/loss_opt.hip): the fp64 oracle of tests/_loss_opt_ref.py against what the reference's own classes return
(tests/golden/loss_options.json, tools/make_golden_loss_options.py), the package's torch formulas and the closed form of the bounds
against that oracle, the identities between option sets, the host validation, the unchanged default object graph, the C-ABI refusals,
the trainer's loss_options and the world-2 gloo path.

Tolerance 1e-10 (relative): both sides are fp64 and differ only in summation order; a formula error (a missing mask, the wrong
denominator or divisor) is >= 1e-3."""
import ctypes
import json
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import _loss_opt_ref as O
import _loss_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_options.json")
TOL = 1e-10
IGN = R.IGNORE


def _golden():
    return json.load(open(GOLD))["cases"]


def _flat(c):
    """the case's inputs as the oracle takes them: x (B, N, HW), t (B, HW) or (B, R + u, HW), and the oracle's keyword arguments"""
    x, t = O.golden_inputs(c)
    B, N, H, W = c["shape"]
    o = c["options"]
    kw = dict(regions=c["regions"], weight_ce=o["weight_ce"], weight_dice=o["weight_dice"], batch_dice=o["batch_dice"], do_bg=o["do_bg"],
              class_w=o["class_w"], smooth=1e-5)
    if c["regions"]:
        kw["has_ignore"] = c["has_ignore"]
        return x.reshape(B, N, H * W), t.reshape(B, -1, H * W), kw
    kw["ignore"] = IGN if c["has_ignore"] else None
    return x.reshape(B, N, H * W), t.reshape(B, H * W), kw


def _close(a, b, what):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    scale = float(b.abs().max())
    assert float((a - b).abs().max()) <= TOL * max(scale, 1e-300) or (scale == 0 and bool((a == 0).all())), (what, a, b)


def _package_loss(c, x64):
    """the package's torch formula (the CPU path) in fp64 through the public functions"""
    from dinounet_amd import training as T
    _, t = O.golden_inputs(c)
    o = c["options"]
    if c["regions"]:
        return T.dc_and_bce_loss(x64, t, use_ignore_label=c["has_ignore"], ddp=False, weight_ce=o["weight_ce"], weight_dice=o["weight_dice"],
                                 batch_dice=o["batch_dice"])
    return T.dc_and_ce_loss(x64, t, ddp=False, ignore_label=IGN if c["has_ignore"] else None, weight_ce=o["weight_ce"],
                            weight_dice=o["weight_dice"], batch_dice=o["batch_dice"], do_bg=o["do_bg"], ce_class_weights=o["class_w"])


@pytest.mark.parametrize("name", [c["name"] for c in _golden()])
def test_oracle_package_formula_and_closed_form_match_the_reference_classes(name):
    c = next(c for c in _golden() if c["name"] == name)
    x, t, kw = _flat(c)
    loss, grad = O.ref_loss(x, t, **kw)
    idx = c["grad_index"]
    _close(loss, c["loss"], (name, "oracle loss"))
    _close(grad.reshape(-1)[idx], c["grad"], (name, "oracle grad"))
    _close(grad.abs().sum(), c["grad_abs_sum"], (name, "oracle |grad|"))
    # the closed form the bounds are built on
    cf = O.opt_ref(x, t, **kw)
    _close(cf.loss, loss, (name, "closed-form loss"))
    _close(cf.grad, grad, (name, "closed-form grad"))
    # the package's CPU path
    x64 = O.golden_inputs(c)[0].double().requires_grad_(True)
    pl = _package_loss(c, x64)
    (pg,) = torch.autograd.grad(pl, x64)
    _close(pl.detach(), c["loss"], (name, "package loss"))
    _close(pg.reshape(-1)[idx], c["grad"], (name, "package grad"))
    _close(pg.reshape(grad.shape), grad, (name, "package grad, whole"))


def test_golden_covers_every_option_and_the_all_ignored_case():
    cs = _golden()
    o = [c["options"] for c in cs]
    assert any(v["weight_ce"] == 0 for v in o) and any(v["weight_dice"] == 0 for v in o) and any(not v["batch_dice"] for v in o)
    assert any(v["do_bg"] and not c["regions"] for v, c in zip(o, cs)) and any(v["class_w"] is not None for v in o)
    assert any(c["regions"] for c in cs) and any(c["has_ignore"] for c in cs)
    ai = next(c for c in cs if c["name"] == "all_ignored")
    assert ai["loss"] == -1.0 and ai["grad_abs_sum"] == 0.0          # CE exactly 0, every Dice exactly 1


@pytest.mark.parametrize("regions", [False, True])
def test_identities_between_option_sets(regions):
    N = 3
    x = R.general_draw(1, N, 35, 11)
    if regions:
        t = torch.cat((torch.randint(0, 2, (1, N, 35), generator=torch.Generator().manual_seed(12)), (~R.mask_draw(1, 35, 13, 0.3)).long()[:, None]), 1)
        base = dict(regions=True, has_ignore=True)
    else:
        t = R.labels_draw(1, N, 35, 12, ignore_frac=0.3)
        base = dict(ignore=IGN, class_w=[0.5, 1.0, 2.0], do_bg=True)
    # B = 1: per-sample Dice is batch Dice
    a, ga = O.ref_loss(x, t, batch_dice=False, **base)
    b, gb = O.ref_loss(x, t, batch_dice=True, **base)
    assert float(a) == float(b) and torch.equal(ga, gb)
    # weight 0 drops the term: full = wce CE-only + wd Dice-only
    ce, gce = O.ref_loss(x, t, weight_dice=0.0, **base)
    dc, gdc = O.ref_loss(x, t, weight_ce=0.0, **base)
    full, gf = O.ref_loss(x, t, weight_ce=0.5, weight_dice=2.0, **base)
    _close(full, 0.5 * ce + 2.0 * dc, "loss = 0.5 CE + 2 Dice")
    _close(gf, 0.5 * gce + 2.0 * gdc, "grad = 0.5 CE + 2 Dice")
    if not regions:       # the CE-only loss is torch's weighted cross entropy, the Dice-only gradient knows no class weight
        w = torch.tensor(base["class_w"], dtype=torch.float64)
        _close(ce, torch.nn.functional.cross_entropy(x.double(), t, weight=w, ignore_index=IGN), "CE only")
        _, gdc2 = O.ref_loss(x, t, weight_ce=0.0, **dict(base, class_w=[4.0, 0.25, 1.0]))
        assert torch.equal(gdc, gdc2)


def test_regime_formulas():
    assert O.sums_blocks(3, 8) == 1 and O.sums_blocks(8, 512 * 512) == 128 and O.bwd_blocks(8, 512 * 512) == 256
    B, H, W = O.BIG
    assert O.sums_blocks(B, H * W) == 1 and O.bwd_blocks(B, H * W) == 4
    assert O.trips(B, H * W, False) == 5 > 2 and O.trips(B, H * W, True) == 2 > 1 and (H * W) % 4 == 1
    assert O.ws_elems(3, 8, 8, False, True) == 3 * 26 and O.ws_elems(2, 3, 35, False, False) == 2 * 8


# ---------------------------------------------------------------------------------------------------- public interface
BAD = [dict(weight_ce=0.0, weight_dice=0.0), dict(weight_ce=-1.0), dict(weight_dice=-0.5), dict(weight_ce=float("nan")),
       dict(weight_dice=float("inf")), dict(ce_class_weights=[1.0, 0.0, 1.0]), dict(ce_class_weights=[1.0, -2.0, 1.0]),
       dict(ce_class_weights=[1.0, float("inf"), 1.0]), dict(ce_class_weights=[1.0, 2.0]), dict(ce_class_weights=[1.0, 2.0, 3.0, 4.0]),
       dict(regions=[1, 2, (1, 2)], ce_class_weights=[1.0, 2.0, 3.0]), dict(regions=[1, 2, (1, 2)], do_bg=False),
       dict(topk_percent=10, weight_ce=0.5), dict(topk_percent=10, weight_dice=2.0), dict(topk_percent=10, batch_dice=False),
       dict(topk_percent=10, do_bg=True), dict(topk_percent=10, ce_class_weights=[1.0, 2.0, 3.0])]


@pytest.mark.parametrize("kw", BAD, ids=[",".join(f"{k}={v}" for k, v in kw.items()) for kw in BAD])
def test_build_loss_rejects_bad_options(kw):
    from dinounet_amd.training import SegLoss, build_loss
    with pytest.raises(ValueError):
        build_loss(3, **kw)
    with pytest.raises(ValueError):
        SegLoss(3, **kw)


def test_functional_forms_reject_bad_options():
    from dinounet_amd import training as T
    x, t = torch.zeros(1, 3, 2, 2), torch.zeros(1, 1, 2, 2, dtype=torch.long)
    for kw in (dict(weight_ce=0.0, weight_dice=0.0), dict(weight_ce=-1.0), dict(ce_class_weights=[1.0, 2.0]), dict(ce_class_weights=[1.0, 0.0, 2.0])):
        with pytest.raises(ValueError):
            T.dc_and_ce_loss(x, t, **kw)
    y = torch.zeros(1, 3, 2, 2, dtype=torch.uint8)
    for kw in (dict(weight_ce=0.0, weight_dice=0.0), dict(weight_dice=float("nan"))):
        with pytest.raises(ValueError):
            T.dc_and_bce_loss(x, y, **kw)


def test_defaults_are_the_module_of_today():
    from dinounet_amd.training import DeepSupervisionLoss, SegLoss, build_loss
    for kw in (dict(), dict(ignore_label=3), dict(regions=[1, 2, (1, 2)]), dict(topk_percent=10),
               dict(weight_ce=1.0, weight_dice=1, batch_dice=True, do_bg=None, ce_class_weights=None), dict(do_bg=False),
               dict(regions=[1, 2, (1, 2)], do_bg=True)):
        l = build_loss(3, **kw)
        assert type(l) is SegLoss and l.options_default, kw
        assert not hasattr(l, "class_w") and [n for n, _ in l.named_buffers()] == (["table"] if "regions" in kw else [])
    ds = build_loss(3, deep_supervision_weights=[2 / 3, 1 / 3, 0.0])
    assert type(ds) is DeepSupervisionLoss and ds.base.options_default
    x = R.general_draw(2, 3, 35, 5).view(2, 3, 5, 7).double()
    t = R.labels_draw(2, 3, 35, 6).view(2, 1, 5, 7)
    from dinounet_amd import training as T
    assert float(build_loss(3)(x, t)) == float(T.dc_and_ce_loss(x, t)) == float(build_loss(3, do_bg=False, weight_ce=1)(x, t))
    assert not build_loss(3, weight_ce=0.5).options_default and not build_loss(3, do_bg=True).options_default
    assert not build_loss(3, batch_dice=False).options_default and not build_loss(3, ce_class_weights=[1, 1, 1]).options_default
    l = build_loss(3, ce_class_weights=[1, 2, 4], ignore_label=IGN)
    assert l.mode == "softmax_ignore" and l.class_w.dtype == torch.float32 and l.class_w.tolist() == [1.0, 2.0, 4.0]
    assert "class_w" not in l.state_dict()


def test_deep_supervision_with_options_composes_the_per_scale_losses():
    from dinounet_amd.training import build_loss, downsample_target
    opt = dict(weight_ce=0.5, weight_dice=2.0, batch_dice=False, ce_class_weights=[1.0, 2.0, 0.5])
    w = [4 / 7, 2 / 7, 1 / 7]
    l = build_loss(3, ignore_label=IGN, deep_supervision_weights=w, **opt)
    outs = [R.general_draw(2, 3, h * wd, 30 + i).view(2, 3, h, wd).double() for i, (h, wd) in enumerate(R.DS_EXACT)]
    t = R.labels_draw(2, 3, 18 * 10, 33, ignore_frac=0.2).view(2, 1, 18, 10)
    assert not l.fused(outs) and not l.fused([o.to("meta") for o in outs])
    want = 0.0
    for ws, o in zip(w, outs):
        ts = downsample_target(t, o.shape[-2:])
        want = want + ws * O.ref_loss(o.reshape(2, 3, -1), ts.reshape(2, -1), ignore=IGN, weight_ce=0.5, weight_dice=2.0, batch_dice=False,
                                      class_w=opt["ce_class_weights"])[0]
    _close(l(outs, t), want, "deep supervision")


# ---------------------------------------------------------------------------------------------------- C ABI
def _opt(**kw):
    from dinounet_amd import _lib
    d = dict(n=3, regions=0, has_ignore=0, ignore=0, do_bg=0, batch_dice=1, weight_ce=1.0, weight_dice=1.0, class_w=None)
    d.update(kw)
    return _lib.LossOpt(*[d[f] for f, _ in _lib.LossOpt._fields_])


def test_loss_opt_c_abi_refuses_bad_arguments_without_a_launch():
    from dinounet_amd import _lib
    L = _lib.lib()
    BADA, UNS = -1, -2
    fake = ctypes.c_void_p(256)           # never dereferenced: every call below is refused before a launch
    big = 1 << 20

    def sums(o, logits=fake, target=fake, out=fake, B=2, HW=64, ws=fake, n=big):
        return L.du_loss_opt_sums(ctypes.byref(o) if o is not None else None, logits, target, out, B, HW, ws, n, None)

    def finish(o, s=fake, loss=fake, coef=fake, B=2):
        return L.du_loss_opt_finish(ctypes.byref(o) if o is not None else None, s, loss, coef, B, 1e-5, 1.0, None)

    def bwd(o, logits=fake, target=fake, coef=fake, dl=fake, B=2, HW=64):
        return L.du_loss_opt_bwd(ctypes.byref(o) if o is not None else None, logits, target, coef, None, dl, B, HW, None)

    for o in (_opt(n=1), _opt(n=9), _opt(n=0, regions=1, do_bg=1), _opt(n=9, regions=1, do_bg=1)):
        assert sums(o) == UNS and finish(o) == UNS and bwd(o) == UNS
        assert L.du_loss_opt_ws_elems(ctypes.byref(o), 2, 64) == 0
    for o in (_opt(weight_ce=0.0, weight_dice=0.0), _opt(weight_ce=-1.0), _opt(weight_dice=float("nan")), _opt(weight_ce=float("inf")),
              _opt(regions=1, do_bg=1, class_w=256), _opt(regions=1, do_bg=0), _opt(regions=2), _opt(has_ignore=2), _opt(do_bg=3),
              _opt(batch_dice=-1)):
        assert sums(o) == BADA and finish(o) == BADA and bwd(o) == BADA
        assert L.du_loss_opt_ws_elems(ctypes.byref(o), 2, 64) == 0
    ok = _opt(do_bg=1, batch_dice=0, class_w=256)
    assert sums(None) == BADA and sums(ok, logits=None) == BADA and sums(ok, target=None) == BADA and sums(ok, out=None) == BADA
    assert sums(ok, ws=None) == BADA and sums(ok, B=0) == BADA and sums(ok, HW=0) == BADA
    need = int(L.du_loss_opt_ws_elems(ctypes.byref(ok), 2, 64))
    assert need == O.ws_elems(2, 3, 64, False, True) == 2 * 11
    assert sums(ok, n=need - 1) == BADA and sums(ok, n=0) == BADA                  # scratch too small
    assert finish(None) == BADA and finish(ok, s=None) == BADA and finish(ok, loss=None) == BADA and finish(ok, coef=None) == BADA
    assert finish(ok, B=0) == BADA
    assert bwd(None) == BADA and bwd(ok, logits=None) == BADA and bwd(ok, target=None) == BADA and bwd(ok, coef=None) == BADA
    assert bwd(ok, dl=None) == BADA and bwd(ok, B=0) == BADA and bwd(ok, HW=0) == BADA
    for B, N, HW, reg, bg in ((3, 8, 8, False, True), (2, 3, 35, False, False), (8, 3, 512 * 512, False, False), (2048, 2, 4225, True, True)):
        o = _opt(n=N, regions=int(reg), do_bg=int(bg))
        assert int(L.du_loss_opt_ws_elems(ctypes.byref(o), B, HW)) == O.ws_elems(B, N, HW, reg, bg)


# ---------------------------------------------------------------------------------------------------- trainer
def _cases(n=6, size=32):
    from dinounet_amd import dataloading as DL
    ds = DL.DeviceDataset()
    for i in range(n):
        rng = np.random.RandomState(50 + i)
        img = rng.randn(1, 1, size, size).astype(np.float32)
        seg = (img > 0.5).astype(np.int16)
        s = torch.from_numpy(seg)
        ds.add(f"case_{i:03d}", torch.from_numpy(img), s, DL.add_class_locations(s, {}, [1]))
    return ds


def _trainer(ds, folder=None, **kw):
    from dinounet_amd import dataloading as DL
    from dinounet_amd import trainer as TR
    torch.manual_seed(0)
    net = torch.nn.Conv2d(1, 2, 3, padding=1)
    tb = DL.TrainBatches(ds, (24, 24), 2, seed=3, val=True)
    return TR.Trainer(net, ds, fold=0, patch_size=(24, 24), batch_size=2, num_classes=2, num_epochs=1, num_iterations_per_epoch=2,
                      num_val_iterations_per_epoch=2, save_every=1, output_folder=folder, graph=False, train_batches=tb, val_batches=tb, **kw)


TODAY_KEYS = {"fold", "splits", "patch_size", "batch_size", "num_classes", "regions", "ignore_label", "all_labels", "num_epochs",
              "num_iterations_per_epoch", "num_val_iterations_per_epoch", "initial_lr", "weight_decay", "oversample_foreground_percent",
              "save_every", "seed", "graph", "interpolation", "use_mask_for_norm", "deep_supervision", "topk_percent", "world"}


def test_trainer_loss_options_init_args_and_checkpoint_round_trip(tmp_path):
    from dinounet_amd import checkpoint as CK
    from dinounet_amd import trainer as TR
    ds = _cases()
    t0 = _trainer(ds)
    assert set(t0.init_args) == TODAY_KEYS and t0.loss.options_default and t0.loss_options is None
    opts = dict(weight_ce=0.5, weight_dice=2.0, batch_dice=False, do_bg=True, ce_class_weights=(1.0, 4.0))
    t = _trainer(ds, folder=str(tmp_path), loss_options=opts)
    assert set(t.init_args) == TODAY_KEYS | {"loss_options"}
    l = t.loss
    assert not l.options_default and (l.weight_ce, l.weight_dice, l.batch_dice, l.do_bg, l.ce_class_weights) == (0.5, 2.0, False, True, (1.0, 4.0))
    t.run_training()
    assert math.isfinite(t.log["train_losses"][0]) and math.isfinite(t.log["val_losses"][0])
    path = t.save_checkpoint("ck.pth")
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert ck["init_args"]["loss_options"] == dict(opts, ce_class_weights=[1.0, 4.0])
    t2 = _trainer(ds, loss_options=ck["init_args"]["loss_options"])
    assert t2.init_args["loss_options"] == t.init_args["loss_options"]
    assert (t2.loss.weight_ce, t2.loss.batch_dice, t2.loss.ce_class_weights) == (0.5, False, (1.0, 4.0))
    with pytest.raises(ValueError):
        _trainer(ds, loss_options=dict(weight_ce=0.0, weight_dice=0.0))
    with pytest.raises(ValueError):
        _trainer(ds, loss_options=dict(label_smoothing=0.1))
    with pytest.raises(ValueError):
        _trainer(ds, topk_percent=10, loss_options=dict(batch_dice=False))


def test_val_step_with_options_on_the_cpu():
    from dinounet_amd.training import ValStep, build_loss
    torch.manual_seed(0)
    net = torch.nn.Conv2d(1, 3, 1)
    x = torch.randn(2, 1, 5, 7)
    t = R.labels_draw(2, 3, 35, 8, ignore_frac=0.2).view(2, 1, 5, 7)
    l = build_loss(3, ignore_label=IGN, weight_ce=0.5, batch_dice=False, ce_class_weights=[1, 2, 4])
    v0 = ValStep(net, x.shape, t.shape, "cpu", loss=build_loss(3, ignore_label=IGN), graph=False)
    v = ValStep(net, x.shape, t.shape, "cpu", loss=l, graph=False)
    v0(x, t)
    got = v(x, t)
    assert torch.equal(v.counts, v0.counts) and float(got) == float(l(net(x), t).detach())
    assert float(got) != float(v0.loss)


# ---------------------------------------------------------------------------------------------------- world 2 over gloo
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _ddp_inputs():
    x = R.general_draw(4, 3, 35, 21).view(4, 3, 5, 7)
    t = R.labels_draw(4, 3, 35, 22, ignore_frac=0.2).view(4, 1, 5, 7)
    return x, t


PER_SAMPLE = dict(weight_ce=0.5, weight_dice=2.0, batch_dice=False, ce_class_weights=[1.0, 2.0, 0.5])
BATCH = dict(weight_ce=0.5, weight_dice=2.0, do_bg=True)


def _ddp_worker(rank, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=2)
        from dinounet_amd import training as T
        calls = []
        real = dist.all_reduce

        def counting(*a, **k):
            calls.append(1)
            return real(*a, **k)

        dist.all_reduce = counting
        x, t = _ddp_inputs()
        out = {}
        for name, opt in (("per_sample", PER_SAMPLE), ("batch", BATCH)):
            xr = x[2 * rank:2 * rank + 2].double().requires_grad_(True)
            del calls[:]
            loss = T.build_loss(3, ignore_label=IGN, ddp=True, **opt)(xr, t[2 * rank:2 * rank + 2])
            n_fwd = len(calls)
            (g,) = torch.autograd.grad(loss, xr)
            out[name] = (float(loss.detach()), g.numpy().copy(), n_fwd, len(calls))
        dist.all_reduce = real
        q.put((rank, out))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc()))


def test_ddp_world2_per_sample_dice_is_local_and_batch_dice_is_global():
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
    x, t = _ddp_inputs()
    xf, tf = x.reshape(4, 3, 35), t.reshape(4, 35)
    for r in range(2):
        sl = slice(2 * r, 2 * r + 2)
        # per-sample Dice: no collective in the forward or the backward pass; the single-process value of the rank's own batch
        loss, grad, n_fwd, n_all = res[r]["per_sample"]
        assert n_fwd == 0 and n_all == 0
        want, wg = O.ref_loss(xf[sl], tf[sl], ignore=IGN, weight_ce=0.5, weight_dice=2.0, batch_dice=False, class_w=PER_SAMPLE["ce_class_weights"])
        _close(loss, want, ("per_sample", r))
        _close(torch.from_numpy(grad).reshape(wg.shape), wg, ("per_sample grad", r))
        # batch Dice + weights: the global-sums formula = 0.5 CE(local) - 2 Dice(all four images); the three Dice sums are gathered
        loss, grad, n_fwd, n_all = res[r]["batch"]
        assert n_fwd == 3 and n_all == 5          # forward: I, P, G; backward: I and P (G carries no gradient)
        ce = O.ref_loss(xf[sl], tf[sl], ignore=IGN, weight_dice=0.0)[0]
        dc = O.ref_loss(xf, tf, ignore=IGN, weight_ce=0.0, do_bg=True)[0]
        _close(loss, 0.5 * ce + 2.0 * dc, ("batch", r))
        # its gradient: the local CE's, plus the global Dice's on this rank's slice times the world size (all-reduced backward)
        gce = O.ref_loss(xf[sl], tf[sl], ignore=IGN, weight_dice=0.0)[1]
        gdc = O.ref_loss(xf, tf, ignore=IGN, weight_ce=0.0, do_bg=True)[1][sl]
        _close(torch.from_numpy(grad).reshape(gce.shape), 0.5 * gce + 2.0 * 2 * gdc, ("batch grad", r))
