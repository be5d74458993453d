"""CPU tests of the deep-supervision loss (training.DeepSupervisionLoss, deep_supervision_weights / _scales, the target index formula,
dataloading.downsample_seg_for_ds, the du_ds_loss_* / du_downsample_seg argument checks): the torch formula in fp64 against the
reference's own DeepSupervisionWrapper run (tests/golden/deep_supervision_reference.npz, tools/make_golden_deep_supervision.py).

Bound: 1e-10 relative on loss and gradients, the bound of test_cpu_seg_loss.py -- both sides evaluate the same formula in fp64."""
import ctypes
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deep_supervision_reference.npz")
TOL = 1e-10


def _fixture():
    g = np.load(GOLD)
    return g, json.loads(str(g["meta"]))


def _cases(world):
    return [c for c in _fixture()[1]["cases"] if c["world"] == world]


def _regions(c):
    return None if c["regions"] is None else [r if isinstance(r, int) else tuple(r) for r in c["regions"]]


def _loss_module(c, ddp=False):
    from dinounet_amd.training import build_loss
    return build_loss(c["shape"][1], regions=_regions(c), ignore_label=c["ignore_label"], ddp=ddp, deep_supervision_weights=c["weights"])


def _case_tensors(g, c, rows=slice(None)):
    n = c["name"]
    S = 1 + len(c["lower"])
    logits = [torch.from_numpy(g[f"{n}/logits{s}"])[rows] for s in range(S)]
    labels = torch.from_numpy(g[f"{n}/labels"].astype(np.int64))[rows]
    return logits, labels


def cpu_loss(c, logits, labels, ddp=False):
    xs = [x.double().requires_grad_(True) for x in logits]
    loss = _loss_module(c, ddp)(xs, labels)
    loss.backward()
    return float(loss.detach()), [None if x.grad is None else x.grad for x in xs]


def _check(c, loss, grads, ref_loss, ref_grads, what):
    assert abs(loss - ref_loss) <= TOL * max(1.0, abs(ref_loss)), (what, loss, ref_loss)
    for s, (w, gr, rg) in enumerate(zip(c["weights"], grads, ref_grads)):
        if w == 0.0:
            assert gr is None and rg is None, (what, s)        # the wrapper skips the scale: no gradient on either side
            continue
        rg = torch.as_tensor(rg)
        err = float((gr - rg).abs().max() / rg.abs().max())
        assert err <= TOL, (what, s, err)


@pytest.mark.parametrize("name", [c["name"] for c in _cases(1)])
def test_cpu_formula_matches_reference_fixture(name):
    g, meta = _fixture()
    c = [c for c in meta["cases"] if c["name"] == name][0]
    logits, labels = _case_tensors(g, c)
    loss, grads = cpu_loss(c, logits, labels)
    ref_grads = [g[f"{name}/grad{s}"] if f"{name}/grad{s}" in g.files else None for s in range(len(logits))]
    _check(c, loss, grads, float(g[f"{name}/loss"]), ref_grads, name)


def test_fixture_covers_the_cases_of_the_issue():
    _, meta = _fixture()
    by = {c["name"]: c for c in meta["cases"]}
    assert by["ds_plain"]["shape"] == [2, 3, 16, 16] and by["ds_plain"]["lower"] == [[8, 8], [4, 4]]
    assert by["ds_plain"]["weights"] == [2 / 3, 1 / 3, 0.0]
    assert by["ds_ce_ignore"]["shape"] == [2, 4, 20, 12] and by["ds_ce_ignore"]["lower"] == [[10, 6], [5, 3]]
    assert all(w != 0.0 for w in by["ds_ce_ignore"]["weights"])
    assert by["ds_regions_ignore"]["shape"] == [2, 3, 18, 10] and by["ds_regions_ignore"]["lower"] == [[9, 5], [4, 2]]
    assert by["ds_ddp_ce_ignore"]["world"] == 2 and by["ds_ddp_ce_ignore"]["lower"] == [[8, 8]]


# ---- the index formula against scipy's zoom (= skimage resize(order=0, mode="edge", anti_aliasing=False) = resize_segmentation(order=0))
def test_index_formula_equals_scipy_zoom_order0():
    from scipy import ndimage
    from dinounet_amd.training import ds_target_index
    checked = 0
    for n in range(1, 257):
        a = np.arange(n, dtype=np.int64)
        for s in (1 / 2, 1 / 4, 1 / 8, 1 / 3):
            m = int(np.round(n * s))
            if m < 1:
                continue
            want = ndimage.zoom(a, m / n, order=0, mode="nearest", grid_mode=True)
            got = ds_target_index(m, n).numpy()
            assert want.shape == (m,) and np.array_equal(got, want), (n, m)
            checked += 1
        assert np.array_equal(ds_target_index(n, n).numpy(), a)           # the identity at scale 0
    assert checked > 900


def test_downsample_seg_for_ds_cpu_matches_scipy_zoom_2d():
    from scipy import ndimage
    from dinounet_amd.dataloading import downsample_seg_for_ds
    g = torch.Generator().manual_seed(0)
    seg = torch.randint(-1, 70, (2, 1, 20, 12), generator=g)
    outs = downsample_seg_for_ds(seg, [[1.0, 1.0], [0.5, 0.5], (5, 3), 0.125])
    assert outs[0] is seg
    assert [tuple(o.shape[2:]) for o in outs] == [(20, 12), (10, 6), (5, 3), (2, 2)]      # np.round(2.5) = 2, np.round(1.5) = 2
    for o in outs[1:]:
        h, w = o.shape[2:]
        for b in range(2):
            want = ndimage.zoom(seg[b, 0].numpy(), (h / 20, w / 12), order=0, mode="nearest", grid_mode=True)
            assert np.array_equal(o[b, 0].numpy(), want)


# ---- weights and scales against the values the generator computed the trainer's way
def test_weights_and_scales_match_the_trainer_formulas():
    from dinounet_amd.training import deep_supervision_scales, deep_supervision_weights
    _, meta = _fixture()
    for key, want in meta["weights"].items():
        n, ddp = key.split("/")
        assert deep_supervision_weights(int(n), ddp=bool(int(ddp))) == want, key
    assert deep_supervision_weights(3) == [2 / 3, 1 / 3, 0.0]
    for e in meta["scales"]:
        assert deep_supervision_scales(e["pool"]) == e["scales"], e["pool"]
    with pytest.raises(ValueError):
        deep_supervision_weights(1)
    with pytest.raises(ValueError):
        deep_supervision_weights(0)


def test_build_loss_wraps_only_when_weights_are_given():
    from dinounet_amd.training import DeepSupervisionLoss, SegLoss, build_loss
    plain = build_loss(3)
    assert type(plain) is SegLoss
    ds = build_loss(3, regions=[1, (1, 2), 2], ignore_label=3, deep_supervision_weights=[2 / 3, 1 / 3, 0])
    assert isinstance(ds, DeepSupervisionLoss) and ds.weights == (2 / 3, 1 / 3, 0.0)
    assert ds.mode == "regions" and ds.regions == [1, (1, 2), 2] and ds.ignore_label == 3 and ds.smooth == 1e-5
    assert ds.ddp is None and ds.group is None and ds.table.dtype == torch.int64 and ds.table.numel() == 3
    with pytest.raises(ValueError):
        build_loss(3, deep_supervision_weights=[0, 0, 0])


def test_list_target_and_mismatched_outputs_raise():
    from dinounet_amd.training import build_loss
    loss = build_loss(3, deep_supervision_weights=[2 / 3, 1 / 3, 0])
    outs = [torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 2, 2)]
    tgt = torch.zeros(1, 1, 8, 8, dtype=torch.long)
    with pytest.raises(ValueError, match="first element"):
        loss(outs, [tgt, tgt[:, :, ::2, ::2], tgt[:, :, ::4, ::4]])
    with pytest.raises(ValueError):
        loss(outs[:2], tgt)
    with pytest.raises(ValueError):
        loss(outs[1:] + outs[:1], tgt)                      # outs[0] must have the target's size
    with pytest.raises(TypeError):
        loss(outs[0], tgt)


def test_zero_weight_scale_is_never_read_on_the_cpu():
    from dinounet_amd.training import build_loss
    loss = build_loss(3, deep_supervision_weights=[2 / 3, 1 / 3, 0])
    g = torch.Generator().manual_seed(1)
    outs = [torch.randn(1, 3, 8, 8, generator=g).requires_grad_(True), torch.randn(1, 3, 4, 4, generator=g).requires_grad_(True),
            torch.full((1, 3, 2, 2), float("nan")).requires_grad_(True)]
    tgt = torch.randint(0, 3, (1, 1, 8, 8), generator=g)
    l = loss(outs, tgt)
    l.backward()
    assert torch.isfinite(l) and outs[2].grad is None and outs[0].grad is not None


def test_train_step_rejects_a_list_output_without_a_deep_supervision_loss():
    from dinounet_amd.training import TrainStep, build_loss

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.ones(1))

        def forward(self, x):
            y = x * self.w
            return [y, y[:, :, ::2, ::2]]

    net = Net()
    params = list(net.parameters())
    opt = torch.optim.SGD(params, 1e-3)
    x = torch.randn(1, 3, 8, 8)
    tgt = torch.randint(0, 3, (1, 1, 8, 8))
    for bad in (None, build_loss(3)):
        ts = TrainStep(net, opt, params, x.shape, tgt.shape, "cpu", graph=False, loss=bad)
        with pytest.raises(TypeError, match="deep supervision"):
            ts(x, tgt)
    ts = TrainStep(net, opt, params, x.shape, tgt.shape, "cpu", graph=False, loss=build_loss(3, deep_supervision_weights=[0.75, 0.25]))
    assert torch.isfinite(ts(x, tgt))


# ---- world 2 over gloo: the torch formula with ddp=True against the reference's ddp=True run
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _ddp_worker(rank, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=2)
        g, _ = _fixture()
        out = {}
        for c in _cases(2):
            logits, labels = _case_tensors(g, c, slice(rank, rank + 1))
            loss, grads = cpu_loss(c, logits, labels, ddp=True)
            out[c["name"]] = (loss, [gr.numpy().copy() for gr in grads])
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
            loss, grads = res[r][n]
            ref = [g[f"{n}/grad{s}"][r:r + 1] for s in range(len(grads))]
            _check(c, loss, [torch.from_numpy(x) for x in grads], float(g[f"{n}/loss"][r]), ref, (n, r))


# ---- C ABI: bad arguments are rejected before any launch, so this runs without a device
def test_ds_loss_c_abi_argument_validation_without_gpu():
    from dinounet_amd import _lib
    L = _lib.lib()
    BAD, UNS = -1, -2
    fake = ctypes.c_void_p(256)           # never dereferenced: every call below is refused before a launch

    def ints(*v):
        return (ctypes.c_int * len(v))(*v)

    def flts(*v):
        return (ctypes.c_float * len(v))(*v)

    def ptrs(*v):
        return (ctypes.c_void_p * len(v))(*v)

    hs, wd, w3 = ints(16, 8, 4), ints(16, 8, 4), flts(2 / 3, 1 / 3, 0.0)
    p3 = ptrs(256, 256, None)             # the zero-weight scale may be NULL
    n = L.du_ds_loss_ws_elems(0, 2, 3, 16, 16, 3, hs, wd, w3)
    assert n > 0
    assert L.du_ds_loss_ws_elems(0, 2, 9, 16, 16, 3, hs, wd, w3) == 0 and L.du_ds_loss_ws_elems(1, 2, 0, 16, 16, 3, hs, wd, w3) == 0
    assert L.du_ds_loss_ws_elems(0, 2, 3, 16, 16, 5, ints(16, 8, 4, 2, 1), ints(16, 8, 4, 2, 1), flts(1, 1, 1, 1, 1)) == 0
    sums = lambda **kw: L.du_ds_loss_sums(*[kw.get(k, d) for k, d in (  # noqa: E731
        ("mode", 0), ("logits", p3), ("target", fake), ("table", None), ("sums", fake), ("B", 2), ("C", 3), ("H", 16), ("W", 16), ("S", 3),
        ("hs", hs), ("wd", wd), ("weights", w3), ("u", 0), ("ig", 0), ("ws", fake), ("n", n), ("stream", None))])
    assert sums(S=0) == BAD                                                        # S outside 1..4
    assert sums(S=5, hs=ints(16, 8, 4, 2, 1), wd=ints(16, 8, 4, 2, 1), weights=flts(1, 1, 1, 1, 1), logits=ptrs(256, 256, 256, 256, 256)) == UNS
    assert sums(hs=ints(16, 32, 4)) == BAD                                         # a scale larger than the target
    assert sums(wd=ints(17, 8, 4)) == BAD
    assert sums(logits=ptrs(256, None, None)) == BAD                               # NULL pointer of an active scale
    assert sums(n=n - 1) == BAD                                                    # workspace too small
    assert sums(weights=flts(0, 0, 0)) == BAD                                      # the wrapper's assertion
    assert sums(C=9) == UNS and sums(C=1) == UNS and sums(mode=2) == BAD
    assert sums(mode=1, table=None) == BAD and sums(mode=1, table=fake, C=9) == UNS
    assert sums(target=None) == BAD and sums(u=2) == BAD
    assert L.du_ds_loss_finish(0, None, fake, fake, 3, 3, w3, 0, 1e-5, 1.0, None) == BAD
    assert L.du_ds_loss_finish(0, fake, fake, fake, 3, 0, w3, 0, 1e-5, 1.0, None) == BAD
    assert L.du_ds_loss_finish(0, fake, fake, fake, 3, 5, w3, 0, 1e-5, 1.0, None) == UNS
    assert L.du_ds_loss_finish(0, fake, fake, fake, 9, 3, w3, 0, 1e-5, 1.0, None) == UNS
    bwd = lambda **kw: L.du_ds_loss_bwd(*[kw.get(k, d) for k, d in (  # noqa: E731
        ("mode", 0), ("logits", p3), ("target", fake), ("table", None), ("coef", fake), ("go", None), ("dl", p3), ("B", 2), ("C", 3),
        ("H", 16), ("W", 16), ("S", 3), ("hs", hs), ("wd", wd), ("weights", w3), ("u", 0), ("ig", 0), ("stream", None))])
    assert bwd(S=0) == BAD and bwd(dl=ptrs(256, None, None)) == BAD and bwd(hs=ints(32, 8, 4)) == BAD and bwd(C=9) == UNS
    assert bwd(coef=None) == BAD and bwd(mode=1) == BAD
    o2 = ptrs(256, 256)
    assert L.du_downsample_seg(None, o2, 2, 16, 16, 2, ints(8, 4), ints(8, 4), None) == BAD
    assert L.du_downsample_seg(fake, o2, 2, 16, 16, 0, ints(8, 4), ints(8, 4), None) == BAD
    assert L.du_downsample_seg(fake, ptrs(256, None), 2, 16, 16, 2, ints(8, 4), ints(8, 4), None) == BAD
    assert L.du_downsample_seg(fake, o2, 2, 16, 16, 2, ints(8, 17), ints(8, 4), None) == BAD
    assert L.du_downsample_seg(fake, ptrs(1, 1, 1, 1, 1), 2, 16, 16, 5, ints(8, 4, 2, 1, 1), ints(8, 4, 2, 1, 1), None) == UNS
