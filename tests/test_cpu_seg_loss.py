"""CPU suite (-m "not gpu") of the ignore-label and region losses (training.build_loss, nnUNetTrainer._build_loss,
nnUNetTrainer.py:355-365): the torch formulas in fp64 against the reference's own classes (tests/golden/seg_loss_reference.npz,
tools/make_golden_seg_loss.py), the region conversion, build_loss's mode choice and host validation, the world-2 gloo path, and the
C-ABI argument checks of the new entry points.

Tolerance 1e-10 (relative): both sides are fp64 and differ only in summation order; a formula error (a missing mask, the wrong
denominator) is >= 1e-3."""
import ctypes
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seg_loss_reference.npz")
TOL = 1e-10


def _fixture():
    g = np.load(GOLD)
    meta = json.loads(str(g["meta"]))
    return g, meta


def _cases(world):
    g, meta = _fixture()
    return [c for c in meta["cases"] if c["world"] == world]


def _regions(c):
    return None if c["regions"] is None else [r if isinstance(r, int) else tuple(r) for r in c["regions"]]


def cpu_loss(kind, logits, labels, regions, ignore_label, ddp=False):
    """the product's torch formula (CPU path) in fp64: loss, d loss / d logits"""
    from dinounet_amd import training as T
    x = logits.double().requires_grad_(True)
    if kind == "regions":
        onehot = T.labels_to_regions(labels, regions, ignore_label)
        loss = T.dc_and_bce_loss(x, onehot, use_ignore_label=ignore_label is not None, ddp=ddp)
    else:
        loss = T.dc_and_ce_loss(x, labels, ddp=ddp, ignore_label=ignore_label)
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
    loss, grad = cpu_loss(c["kind"], logits, labels, _regions(c), c["ignore_label"])
    _check(loss, grad, float(g[f"{name}/loss"]), g[f"{name}/grad"], name)


def test_all_ignored_fixture_is_exactly_minus_one():
    g, _ = _fixture()
    assert float(g["ce_all_ignored/loss"]) == -1.0
    logits = torch.from_numpy(g["ce_all_ignored/logits"])
    labels = torch.from_numpy(g["ce_all_ignored/labels"].astype(np.int64))
    loss, grad = cpu_loss("softmax", logits, labels, None, 3)
    assert loss == -1.0 and float(grad.abs().max()) == 0.0


@pytest.mark.parametrize("name", [c["name"] for c in _cases(1) if c["kind"] == "regions"] +
                         [c["name"] for c in _cases(2) if c["kind"] == "regions"])
def test_cpu_labels_to_regions_matches_fixture_onehot(name):
    from dinounet_amd.training import labels_to_regions
    g, meta = _fixture()
    c = [c for c in meta["cases"] if c["name"] == name][0]
    labels = torch.from_numpy(g[f"{name}/labels"].astype(np.int64))
    got = labels_to_regions(labels, _regions(c), c["ignore_label"])
    assert got.dtype == torch.uint8
    assert np.array_equal(got.numpy(), g[f"{name}/onehot"])


# fresh seeds against the reference classes themselves (only where the reference tree is)
def _reference_available():
    from oracle import refshim
    return refshim.reference_available()


FRESH = [("softmax", (2, 3, 24, 20), None, 3, 0.3), ("softmax", (1, 5, 16, 16), None, 7, 0.6), ("softmax", (2, 4, 8, 8), None, 4, 1.0),
         ("regions", (2, 3, 24, 20), [(1, 2, 3), (2, 3), (3,)], 4, 0.3), ("regions", (3, 2, 13, 11), [1, (1, 2)], None, 0.0),
         ("regions", (1, 1, 16, 16), [(2,)], 5, 1.0), ("regions", (2, 8, 12, 12), [1, 2, 3, 4, (1, 2), (3, 4), (5, 6), (1, 6)], 7, 0.2)]


@pytest.mark.skipif(not _reference_available(), reason="needs the reference tree (build machine only)")
@pytest.mark.parametrize("i", range(len(FRESH)))
def test_cpu_formula_matches_reference_classes_fresh_seeds(i):
    import tools.make_golden_seg_loss as M
    kind, shape, regions, ig, frac = FRESH[i]
    g = torch.Generator().manual_seed(500 + i)
    logits = (torch.randn(shape, generator=g) * 2.0).float()
    labels = M.make_labels(shape, kind, regions, ig, 600 + i, ignored_frac=frac)
    ref_loss, ref_grad = M.reference_eval(kind, logits, labels, regions, ig)
    loss, grad = cpu_loss(kind, logits, labels, regions, ig)
    _check(loss, grad, ref_loss, ref_grad, FRESH[i])


# ---- build_loss: mode and host validation
def test_build_loss_picks_the_mode():
    from dinounet_amd.training import SegLoss, build_loss
    assert build_loss(3).mode == "softmax"
    assert build_loss(3, ignore_label=3).mode == "softmax_ignore"
    m = build_loss(3, regions=[(1, 2, 3), (2, 3), 3], ignore_label=4)
    assert isinstance(m, SegLoss) and isinstance(m, torch.nn.Module) and m.mode == "regions"
    assert m.table.dtype == torch.int64 and m.table.cpu().tolist() == [0b1110, 0b1100, 0b1000]
    assert build_loss(2, regions=[1, (1, 2)]).mode == "regions"
    assert build_loss(1, regions=[(0, 63)]).table.cpu().tolist() == [1 - (1 << 63)]       # label 63 is the int64 sign bit
    # plain labels: exactly today's dc_and_ce_loss
    from dinounet_amd.training import dc_and_ce_loss
    x = torch.randn(2, 3, 8, 8, dtype=torch.float64)
    t = torch.randint(0, 3, (2, 1, 8, 8))
    assert float(build_loss(3)(x, t)) == float(dc_and_ce_loss(x, t))


def test_build_loss_module_equals_the_functions():
    from dinounet_amd.training import build_loss, dc_and_bce_loss, dc_and_ce_loss, labels_to_regions
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, 10, 12, generator=g, dtype=torch.float64)
    t = torch.randint(0, 5, (2, 1, 10, 12), generator=g)              # labels 0..3, 4 = ignore
    t3 = torch.where(t == 3, torch.full_like(t, 2), t)                   # 3 classes + the ignore label
    assert float(build_loss(3, ignore_label=4)(x, t3)) == float(dc_and_ce_loss(x, t3, ignore_label=4))
    regs = [(1, 2, 3), (2, 3), (3,)]
    want = dc_and_bce_loss(x, labels_to_regions(t, regs, 4), use_ignore_label=True)
    assert float(build_loss(3, regions=regs, ignore_label=4)(x, t)) == float(want)


@pytest.mark.parametrize("kw", [dict(num_classes=3, ignore_label=2), dict(num_classes=3, ignore_label=0),
                                dict(num_classes=9, regions=list(range(1, 10))),
                                dict(num_classes=2, regions=[1, 64]), dict(num_classes=2, regions=[1, (2, -1)]),
                                dict(num_classes=2, regions=[(1, 2), (2, 3)], ignore_label=3),
                                dict(num_classes=2, regions=[1, 2], ignore_label=1),
                                dict(num_classes=3, regions=[1, 2]), dict(num_classes=0, regions=[])])
def test_build_loss_rejects_bad_configurations(kw):
    from dinounet_amd.training import build_loss
    with pytest.raises(ValueError):
        build_loss(**kw)


# ---- world 2 over gloo: the torch formulas with ddp=True against the reference's ddp=True run (fixture case 5)
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
            loss, grad = cpu_loss(c["kind"], logits, labels, _regions(c), c["ignore_label"], ddp=True)
            out[n] = (loss, grad.numpy().copy())
        q.put((rank, out))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc()))


def test_ddp_world2_formulas_match_reference_fixture():
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


# ---- C ABI: bad arguments are rejected before any launch, so this runs without a device
def test_seg_loss_c_abi_argument_validation_without_gpu():
    from dinounet_amd import _lib
    L = _lib.lib()
    BAD, UNS = -1, -2
    fake = ctypes.c_void_p(256)           # never dereferenced: every call below is refused before a launch
    assert L.du_dice_ce_masked_ws_elems(2, 4, 1024) > 0 and L.du_dice_ce_masked_ws_elems(2, 9, 1024) == 0
    assert L.du_dice_bce_ws_elems(2, 8, 1024) > 0 and L.du_dice_bce_ws_elems(2, 9, 1024) == 0 and L.du_dice_bce_ws_elems(2, 0, 64) == 0
    # masked softmax
    assert L.du_dice_ce_masked_sums(None, fake, fake, 2, 4, 64, 4, fake, 1 << 20, None) == BAD
    assert L.du_dice_ce_masked_sums(fake, fake, fake, 0, 4, 64, 4, fake, 1 << 20, None) == BAD
    assert L.du_dice_ce_masked_sums(fake, fake, fake, 2, 9, 64, 9, fake, 1 << 20, None) == UNS
    assert L.du_dice_ce_masked_sums(fake, fake, fake, 2, 1, 64, 1, fake, 1 << 20, None) == UNS
    assert L.du_dice_ce_masked_sums(fake, fake, fake, 2, 4, 64, 4, fake, 0, None) == BAD              # scratch too small
    assert L.du_dice_ce_masked_finish(None, fake, fake, 4, 1e-5, 1.0, None) == BAD
    assert L.du_dice_ce_masked_finish(fake, fake, fake, 9, 1e-5, 1.0, None) == UNS
    assert L.du_dice_ce_masked_bwd(fake, fake, fake, None, None, 2, 4, 64, 4, None) == BAD
    assert L.du_dice_ce_masked_bwd(fake, fake, fake, None, fake, 2, 16, 64, 16, None) == UNS
    # regions
    assert L.du_dice_bce_sums(fake, None, fake, 2, 3, 64, 1, fake, 1 << 20, None) == BAD
    assert L.du_dice_bce_sums(fake, fake, fake, 2, 3, 64, 2, fake, 1 << 20, None) == BAD             # has_ignore is 0 or 1
    assert L.du_dice_bce_sums(fake, fake, fake, 2, 9, 64, 1, fake, 1 << 20, None) == UNS
    assert L.du_dice_bce_sums(fake, fake, fake, 2, 0, 64, 0, fake, 1 << 20, None) == UNS
    assert L.du_dice_bce_sums(fake, fake, fake, 2, 3, 64, 1, fake, 0, None) == BAD
    assert L.du_dice_bce_finish(fake, fake, None, 3, 1, 1e-5, 1.0, None) == BAD
    assert L.du_dice_bce_finish(fake, fake, fake, 9, 1, 1e-5, 1.0, None) == UNS
    assert L.du_dice_bce_bwd(fake, fake, fake, None, fake, 2, 3, 0, 1, None) == BAD
    assert L.du_dice_bce_bwd(fake, fake, fake, None, fake, 2, 9, 64, 1, None) == UNS
    # region conversion
    assert L.du_labels_to_regions(fake, None, fake, 2, 3, 64, 1, 4, None) == BAD
    assert L.du_labels_to_regions(fake, fake, fake, 2, 3, 64, 3, 4, None) == BAD
    assert L.du_labels_to_regions(fake, fake, fake, 2, 9, 64, 1, 4, None) == UNS
    assert L.du_labels_to_regions(fake, fake, fake, 2, 0, 64, 0, 4, None) == UNS
