"""CPU tests of the validation step (training.validation_counts / training.ValStep; nnUNetTrainer.validation_step and
on_validation_epoch_end, nnUNetTrainer.py:946-1052): the torch restatement of the counts against the reference's own get_tp_fp_fn_tn
(tests/golden/val_counts_reference.npz, tools/make_golden_val_counts.py) -- exactly, they are integers --, the epoch values, the nan /
nanmean rule for an empty class, the background drop of last(), and two gloo ranks against one process on the concatenated batches.

Bounds.  Counts: ==.  Dice per class: the fixture holds the reference's fp32 quotient (three fp32 roundings: <= 3 * 2^-24 = 1.8e-7
relative), ValStep divides in float64: 2.5e-7 relative.  Losses: the fixture's is fp64 on fp32 logits, the CPU path runs in fp32:
2e-5 * max(1, |ref|), the bound tests/test_gpu_seg_loss.py applies to the same formulas."""
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "val_counts_reference.npz")
CASES = ["softmax", "softmax_ignore", "softmax_all_ignored", "regions_ignore", "regions_tail", "softmax_ties", "regions_ties"]
EPOCHS = ["epoch_softmax", "epoch_softmax_ignore", "epoch_regions_ignore", "epoch_regions_tail", "epoch_regions_ties"]
DICE_TOL, LOSS_TOL = 2.5e-7, 2e-5


def _fixture():
    g = np.load(GOLD)
    return g, json.loads(str(g["meta"]))


def _case(g, meta, name):
    c = [c for c in meta["cases"] if c["name"] == name][0]
    regions = None if c["regions"] is None else [r if isinstance(r, int) else tuple(r) for r in c["regions"]]
    return c, torch.from_numpy(g[f"{name}/logits"]), torch.from_numpy(g[f"{name}/labels"].astype(np.int64)), regions


def _val_step(c, logits, labels, regions):
    """ValStep on the CPU around an identity network: the static input buffer IS the logits"""
    from dinounet_amd.training import ValStep, build_loss
    loss = None
    if regions is not None or c["ignore_label"] is not None:
        loss = build_loss(logits.shape[1], regions=regions, ignore_label=c["ignore_label"], ddp=False)
        if regions is not None:
            loss = loss.cpu()
    return ValStep(torch.nn.Identity(), logits.shape, labels.shape, "cpu", loss=loss, graph=False)


def test_fixture_is_complete():
    g, meta = _fixture()
    assert [c["name"] for c in meta["cases"]] == CASES and [e["name"] for e in meta["epochs"]] == EPOCHS
    for c in meta["cases"]:
        assert g[f"{c['name']}/logits"].dtype == np.float32 and g[f"{c['name']}/labels"].dtype == np.int16
        assert tuple(g[f"{c['name']}/logits"].shape) == tuple(c["shape"])


@pytest.mark.parametrize("name", CASES)
def test_cpu_counts_reproduce_reference_fixture(name):
    from dinounet_amd.training import validation_counts
    g, meta = _fixture()
    c, logits, labels, regions = _case(g, meta, name)
    tp, fp, fn = validation_counts(logits, labels, regions=regions, ignore_label=c["ignore_label"])
    for got, key in ((tp, "tp"), (fp, "fp"), (fn, "fn")):
        assert got.dtype == torch.int64 and got.shape == (logits.shape[1],)
        want = g[f"{name}/{key}"]
        assert np.array_equal(want, np.round(want))                       # the reference's fp32 sums are whole numbers < 2^24
        assert np.array_equal(got.numpy(), want.astype(np.int64)), (name, key, got, want)
    if name == "softmax_all_ignored":
        assert int(tp.sum() + fp.sum() + fn.sum()) == 0


@pytest.mark.parametrize("ename", EPOCHS)
def test_epoch_end_matches_reference_fixture(ename):
    g, meta = _fixture()
    e = [e for e in meta["epochs"] if e["name"] == ename][0]
    vs = None
    for name in e["cases"]:                                               # one validation step per case; another shape: another ValStep
        c, logits, labels, regions = _case(g, meta, name)
        step = _val_step(c, logits, labels, regions)
        step(logits, labels)
        last = step.last()
        drop = 0 if regions is not None else 1
        assert np.array_equal(last["tp_hard"], g[f"{name}/tp"][drop:].astype(np.int64))
        assert abs(float(last["loss"]) - float(g[f"{name}/loss"])) <= LOSS_TOL * max(1.0, abs(float(g[f"{name}/loss"])))
        if vs is not None:
            step.absorb(vs)
            assert vs.steps == 0 and int(vs.counts.abs().sum()) == 0
        vs = step
    out = vs.epoch_end()
    drop = 0 if regions is not None else 1
    assert out["steps"] == len(e["cases"])
    for key in ("tp", "fp", "fn"):
        want = sum(g[f"{n}/{key}"][drop:].astype(np.int64) for n in e["cases"])
        assert np.array_equal(out[key], want), (ename, key)
    want_dice = g[f"{ename}/dice"]
    got_dice = np.array(out["dice_per_class_or_region"])
    assert got_dice.dtype == np.float64 and got_dice.shape == want_dice.shape
    assert np.all(np.abs(got_dice - want_dice) <= DICE_TOL * np.abs(want_dice)), (got_dice, want_dice)
    assert abs(out["mean_fg_dice"] - float(g[f"{ename}/mean_fg_dice"])) <= DICE_TOL * float(g[f"{ename}/mean_fg_dice"])
    ref_loss = float(g[f"{ename}/val_loss"])
    assert abs(out["val_loss"] - ref_loss) <= LOSS_TOL * max(1.0, abs(ref_loss))
    # the accumulators are zeroed afterwards
    assert vs.steps == 0 and int(vs.counts.abs().sum()) == 0 and float(vs.loss_sum) == 0.0


def test_empty_class_is_nan_and_mean_is_nanmean():
    """class 2 is neither predicted nor labelled: 0 / 0 = nan in dice_per_class_or_region, left out of mean_fg_dice (np.nanmean,
    nnUNetTrainer.py:1046-1047); a batch with nothing but ignored pixels gives nan everywhere"""
    from dinounet_amd.training import ValStep, build_loss
    logits = torch.zeros(1, 3, 4, 4)
    logits[:, 1, :2] = 1.0                                                # rows 0-1 predict class 1, rows 2-3 class 0 (all-equal: lowest index)
    labels = torch.zeros(1, 1, 4, 4, dtype=torch.long)
    labels[:, :, 1:3] = 1                                                 # rows 1-2 are class 1
    vs = ValStep(torch.nn.Identity(), logits.shape, labels.shape, "cpu", graph=False)
    vs(logits, labels)
    assert vs.counts.tolist() == [[4, 4, 0], [4, 4, 0], [4, 4, 0]]        # [tp | fp | fn] x (class 0, 1, 2)
    out = vs.epoch_end()
    d = out["dice_per_class_or_region"]
    assert len(d) == 2 and d[0] == 0.5 and np.isnan(d[1]) and out["mean_fg_dice"] == 0.5
    vs = ValStep(torch.nn.Identity(), logits.shape, labels.shape, "cpu", loss=build_loss(3, ignore_label=3), graph=False)
    vs(logits, torch.full_like(labels, 3))
    out = vs.epoch_end()
    assert all(np.isnan(v) for v in out["dice_per_class_or_region"]) and np.isnan(out["mean_fg_dice"])
    assert out["val_loss"] == -1.0                                        # CE 0, every dice term s / s


def test_last_drops_background_only_in_softmax_modes():
    g, meta = _fixture()
    for name, n_out in (("softmax", 3), ("softmax_ignore", 2), ("regions_ignore", 3), ("regions_tail", 2)):
        c, logits, labels, regions = _case(g, meta, name)
        vs = _val_step(c, logits, labels, regions)
        assert vs.steps == 0
        vs(logits, labels)
        last = vs.last()
        assert sorted(last) == ["fn_hard", "fp_hard", "loss", "tp_hard"]
        assert all(isinstance(last[k], np.ndarray) for k in last) and last["loss"].shape == ()
        assert last["tp_hard"].shape == (n_out,) and vs.counts.shape == (3, logits.shape[1]) and vs.steps == 1
        full = np.stack([g[f"{name}/{k}"] for k in ("tp", "fp", "fn")]).astype(np.int64)
        assert np.array_equal(vs.counts.numpy(), full)
        vs.reset()
        assert vs.steps == 0 and int(vs.counts.sum()) == 0 and float(vs.loss_sum) == 0.0


def test_training_mode_is_restored_and_no_grad():
    from dinounet_amd.training import ValStep
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 2, 1), torch.nn.BatchNorm2d(2))
    before = net[1].running_mean.clone()
    vs = ValStep(net, (2, 3, 8, 8), (2, 1, 8, 8), "cpu", graph=False)
    for mode in (True, False):
        net.train(mode)
        loss = vs(torch.randn(2, 3, 8, 8), torch.randint(0, 2, (2, 1, 8, 8)))
        assert net.training is mode and not loss.requires_grad
    assert torch.equal(net[1].running_mean, before)                      # eval-mode forward: statistics untouched


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _epoch_inputs():
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(3, 4, 3, 12, 10, generator=g) * 2.0             # 3 steps of batch 4
    labels = torch.randint(0, 3, (3, 4, 1, 12, 10), generator=g)
    return logits, labels


def _worker(rank, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=2)
    from dinounet_amd.training import ValStep, build_loss
    logits, labels = _epoch_inputs()
    vs = ValStep(torch.nn.Identity(), (2, 3, 12, 10), (2, 1, 12, 10), "cpu", loss=build_loss(3, ddp=True), graph=False)
    for s in range(3):
        vs(logits[s, 2 * rank:2 * rank + 2], labels[s, 2 * rank:2 * rank + 2])
    out = vs.epoch_end(group=dist.group.WORLD)
    q.put((rank, {k: (np.asarray(v) if not isinstance(v, (int, float)) else v) for k, v in out.items()}))
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_epoch_end_equals_single_process():
    from dinounet_amd.training import ValStep, build_loss
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, port, q)) for r in range(2)]
    [p.start() for p in procs]
    res = dict(q.get(timeout=120) for _ in range(2))
    [p.join(timeout=60) for p in procs]
    assert all(p.exitcode == 0 for p in procs)
    logits, labels = _epoch_inputs()
    vs = ValStep(torch.nn.Identity(), (4, 3, 12, 10), (4, 1, 12, 10), "cpu", loss=build_loss(3, ddp=False), graph=False)
    for s in range(3):
        vs(logits[s], labels[s])
    want = vs.epoch_end()
    for r in range(2):
        got = res[r]
        assert got["steps"] == 6 and want["steps"] == 3                  # 3 steps on each of 2 ranks
        for key in ("tp", "fp", "fn"):
            assert np.array_equal(got[key], want[key]), (r, key)
        assert np.array_equal(got["dice_per_class_or_region"], np.array(want["dice_per_class_or_region"]))
        assert got["mean_fg_dice"] == want["mean_fg_dice"]
        # mean over ranks of (local CE - global Dice) = the loss of the concatenated batch (equal halves), up to fp32 rounding
        assert abs(got["val_loss"] - want["val_loss"]) <= LOSS_TOL * max(1.0, abs(want["val_loss"]))


# ---- C ABI: bad arguments are rejected before any launch, so this runs without a device
def test_val_c_abi_argument_validation_without_gpu():
    import ctypes
    from dinounet_amd import _lib
    L = _lib.lib()
    BAD, UNS = -1, -2
    fake = ctypes.c_void_p(256)           # never dereferenced: every call below is refused before a launch
    big = 1 << 40
    # workspace queries: a function of the shape only, 0 outside the supported class / region counts
    assert L.du_val_dice_ce_ws_elems(2, 4, 1024) == L.du_val_dice_ce_ws_elems(2, 4, 1024) > 0
    assert L.du_val_dice_ce_ws_elems(2, 9, 1024) == 0 and L.du_val_dice_ce_masked_ws_elems(2, 1, 1024) == 0
    assert L.du_val_dice_bce_ws_elems(2, 9, 1024) == 0 and L.du_val_dice_bce_ws_elems(2, 0, 1024) == 0
    # room for the float rows and the int32 count rows of every block
    assert L.du_val_dice_ce_masked_ws_elems(2, 3, 1024) == L.du_dice_ce_masked_ws_elems(2, 3, 1024) // 8 * (8 + 9)
    assert L.du_val_dice_bce_ws_elems(2, 3, 1024) == L.du_dice_bce_ws_elems(2, 3, 1024) // 11 * (11 + 9)
    assert L.du_val_dice_ce_ws_elems(2, 3, 1024) == L.du_dice_ce_ws_elems(2, 3, 1024) // 7 * (7 + 9)
    # K / R outside the limits, and B * HW >= 2^31 (int32 block partials)
    assert L.du_val_dice_ce(fake, fake, fake, fake, None, 2, 9, 1024, fake, big, None) == UNS
    assert L.du_val_dice_ce_masked(fake, fake, fake, fake, None, 2, 1, 1024, 3, fake, big, None) == UNS
    assert L.du_val_dice_bce(fake, fake, fake, fake, None, 2, 9, 1024, 1, fake, big, None) == UNS
    assert L.du_val_dice_ce(fake, fake, fake, fake, None, 2, 3, 1 << 30, fake, big, None) == UNS
    assert L.du_val_dice_ce_masked(fake, fake, fake, fake, None, 2, 3, 1 << 30, 3, fake, big, None) == UNS
    assert L.du_val_dice_bce(fake, fake, fake, fake, None, 2, 3, 1 << 30, 0, fake, big, None) == UNS
    # null pointers, a short workspace, a has_ignore that is no flag
    assert L.du_val_dice_ce(fake, fake, fake, None, None, 2, 3, 1024, fake, big, None) == BAD
    assert L.du_val_dice_ce(fake, fake, fake, fake, None, 2, 3, 1024, fake, 1, None) == BAD
    assert L.du_val_dice_ce_masked(fake, fake, fake, fake, None, 2, 3, 1024, 3, fake, 1, None) == BAD
    assert L.du_val_dice_bce(fake, fake, fake, fake, None, 2, 3, 1024, 2, fake, big, None) == BAD
    assert L.du_val_dice_bce(fake, fake, fake, fake, None, 2, 3, 1024, 1, fake, 1, None) == BAD
