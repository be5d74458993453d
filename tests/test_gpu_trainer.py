"""dinounet_amd.trainer on the MI355X (-m gpu): a fold of six small synthetic cases through loader, augmentation, captured train step,
captured validation step, checkpoints and the sliding-window validation in one process.  dinounet_s with seeded random weights, patch
64 x 64, batch 2; DropPath and the RoPE rescale stay on, so the device generator takes part."""
import copy
import json
import math
import os

import numpy as np
import pytest
import torch

from oracle import weights
from oracle.refshim import PLANS_2D

pytestmark = pytest.mark.gpu
PATCH, BATCH = (64, 64), 2


def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def base_net():
    """dinounet_s as tests/test_gpu_e2e.py builds it, kept on the host: every trainer gets its own copy"""
    from dinounet_amd.network_architecture import DinoUNet
    net = DinoUNet.from_config(PLANS_2D, 3, 2, dinov3_pretrained_path=None, dinov3_model_name="dinounet_s", precision="bf16")
    ks = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    net.load_state_dict(weights.make_state_dict(ks, seed=0), strict=True)
    return net


@pytest.fixture(scope="module")
def dataset():
    """six cases of 3 channels, one slice of 80 x 72; class 1 is a thresholded blob of the image"""
    from dinounet_amd import dataloading as DL
    ds = DL.DeviceDataset()
    yy, xx = np.mgrid[0:80, 0:72]
    for i in range(6):
        rng = np.random.RandomState(300 + i)
        cy, cx, r = rng.randint(20, 60), rng.randint(20, 52), rng.uniform(8, 16)
        blob = np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r))
        img = (0.3 * rng.randn(3, 1, 80, 72) + 2.0 * blob[None, None]).astype(np.float32)
        seg = (blob > 0.5).astype(np.int16)[None, None]
        d, s = torch.from_numpy(img).to(dev()), torch.from_numpy(seg).to(dev())
        ds.add(f"case_{i:03d}", d, s, DL.add_class_locations(s, {}, [1]))
    return ds


class _Recorded:
    """an iterator of batches that keeps the decisions behind every batch; everything else is the wrapped TrainBatches'"""

    def __init__(self, inner):
        self.inner, self.draws = inner, []

    def __getattr__(self, name):
        return getattr(self.inner, name)

    def __iter__(self):
        return self

    def __next__(self):
        out = next(self.inner)
        self.draws.append(self.inner.last_draw)
        return out


def _trainer(base_net, dataset, cls=None, record=False, **kw):
    from dinounet_amd.trainer import Trainer
    args = dict(fold=0, patch_size=PATCH, batch_size=BATCH, num_classes=2, num_epochs=2, num_iterations_per_epoch=4,
                num_val_iterations_per_epoch=2, seed=5, graph=True)
    args.update(kw)
    t = (cls or Trainer)(copy.deepcopy(base_net).to(dev()), dataset, **args)
    if record:
        t.train_batches = _Recorded(t.train_batches)
    return t


def _same(a, b):
    """equality through dicts, lists and arrays that takes nan for equal to nan"""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=np.asarray(a).dtype.kind == "f")
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    return a == b


# ---- 1. two epochs end to end ----------------------------------------------------------------------------------------------------
def test_run_training_two_epochs_log_and_checkpoints(base_net, dataset, tmp_path):
    from dinounet_amd.trainer import LOG_KEYS, Trainer, poly_lr
    seen = []

    class Watched(Trainer):
        def on_epoch_end(self):
            super().on_epoch_end()
            seen.append({f: torch.load(os.path.join(self.output_folder, f), weights_only=False)["current_epoch"]
                         for f in sorted(os.listdir(self.output_folder))})

    t = _trainer(base_net, dataset, cls=Watched, output_folder=str(tmp_path / "fold_0"), save_every=1)
    assert len(t.train_keys) == 4 and len(t.val_keys) == 2
    t.run_training()
    log = t.log.get_checkpoint()
    assert set(log) == set(LOG_KEYS) and all(len(v) == 2 for v in log.values()), {k: len(v) for k, v in log.items()}
    assert log["lrs"] == [poly_lr(1e-2, 0, 2), poly_lr(1e-2, 1, 2)]
    assert float(t.optimizer._hyper_host[0]) == np.float32(poly_lr(1e-2, 1, 2))      # what the replayed step read in the last epoch
    assert all(np.isfinite(v) for v in log["train_losses"] + log["val_losses"]), log
    assert log["train_losses"][0].dtype == np.float32
    assert all(len(d) == 1 for d in log["dice_per_class_or_region"])                   # one foreground class
    assert t.ts.graph is not None and t.ts.capture_mode == "whole_step" and t.vs.graph is not None
    # latest after every epoch but the last (save_every = 1); best in the first epoch and whenever the EMA rises; final at the end
    ema = log["ema_fg_dice"]
    best_written = 2 if ema[1] > ema[0] else 1
    assert seen[0] == {"checkpoint_best.pth": 1, "checkpoint_latest.pth": 1}, seen
    assert seen[1] == {"checkpoint_best.pth": best_written, "checkpoint_latest.pth": 1}, seen
    assert sorted(os.listdir(t.output_folder)) == ["checkpoint_best.pth", "checkpoint_final.pth"]
    final = torch.load(os.path.join(t.output_folder, "checkpoint_final.pth"), weights_only=False)
    assert final["current_epoch"] == 2 and t.current_epoch == 2 and tuple(final["inference_allowed_mirroring_axes"]) == (0, 1)
    assert final["trainer_name"] == "Watched" and _same(float(final["_best_ema"]), float(ema[1] if ema[1] > ema[0] else ema[0]))
    assert set(final["rng_states"]) >= {"loader", "augment", "device"} and final["rng_states"]["augment"] is not None
    assert len(final["network_weights"]) < len(t.net.state_dict())                     # the compact weights of checkpoint.save_checkpoint
    from dinounet_amd.checkpoint import to_reference_checkpoint
    assert to_reference_checkpoint(final, t.net)["network_weights"].keys() == t.net.state_dict().keys()


# ---- 2. no read-back inside the loops --------------------------------------------------------------------------------------------
class _Counters:
    """counting wrappers around everything that makes the host wait for the device"""
    TARGETS = [(torch.Tensor, "cpu"), (torch.Tensor, "item"), (torch.Tensor, "tolist"), (torch.Tensor, "numpy"), (torch.cuda, "synchronize"),
               (torch.cuda.Stream, "synchronize"), (torch.cuda.Event, "synchronize")]

    def __init__(self):
        self.n = 0
        self.saved = []

    def __enter__(self):
        for owner, name in self.TARGETS:
            orig = getattr(owner, name)
            self.saved.append((owner, name, orig, name in vars(owner)))

            def counting(*a, _orig=orig, **k):
                self.n += 1
                return _orig(*a, **k)
            setattr(owner, name, counting)
        return self

    def __exit__(self, *exc):
        for owner, name, orig, own in self.saved:
            if own:
                setattr(owner, name, orig)
            else:
                delattr(owner, name)                        # inherited (torch.Tensor.cpu is TensorBase's): the wrapper alone goes


def _counted_run(base_net, dataset, n_train, n_val):
    from dinounet_amd.trainer import Trainer
    marks, strict = [], []

    class Marked(Trainer):
        def on_epoch_start(self):
            marks.append(("epoch_start", self.current_epoch, counters.n))
            super().on_epoch_start()

        # from the second epoch on (both captures exist) the two loops also run under torch's sync debug mode "error": any call that makes
        # the host wait for the stream raises there -- a synchronous copy from pageable memory, float(tensor), .to("cpu") -- not only
        # the calls the counters wrap
        def on_train_epoch_start(self):
            marks.append(("train_start", self.current_epoch, counters.n))
            if self.current_epoch >= 1:
                torch.cuda.set_sync_debug_mode("error")
            super().on_train_epoch_start()

        def run_train_loop(self):
            try:
                super().run_train_loop()
            finally:
                torch.cuda.set_sync_debug_mode("default")
            marks.append(("train_loop_end", self.current_epoch, counters.n))
            strict.append(("train", self.current_epoch))

        def run_validation_loop(self):
            marks.append(("val_loop_start", self.current_epoch, counters.n))
            if self.current_epoch >= 1:
                torch.cuda.set_sync_debug_mode("error")
            try:
                super().run_validation_loop()
            finally:
                torch.cuda.set_sync_debug_mode("default")
            marks.append(("val_loop_end", self.current_epoch, counters.n))
            strict.append(("val", self.current_epoch))

        def on_epoch_end(self):
            epoch = self.current_epoch
            super().on_epoch_end()
            marks.append(("epoch_end", epoch, counters.n))

    t = _trainer(base_net, dataset, cls=Marked, num_iterations_per_epoch=n_train, num_val_iterations_per_epoch=n_val)
    with _Counters() as counters:
        probe = torch.zeros(2, device=dev())
        probe.cpu(), probe[0].item(), probe.tolist(), probe.cpu().numpy(), torch.cuda.synchronize()
        e = torch.cuda.Event()
        e.record()
        e.synchronize()
        torch.cuda.current_stream().synchronize()
        assert counters.n == 8                                                         # every wrapper counts
        torch.cuda.set_sync_debug_mode("error")
        try:                                                                           # and the debug mode sees a pageable upload
            with pytest.raises(RuntimeError):
                torch.from_numpy(np.zeros(4, np.float32)).to(dev())
        finally:
            torch.cuda.set_sync_debug_mode("default")
        t.run_training()
    assert strict == [("train", 0), ("val", 0), ("train", 1), ("val", 1)] and torch.cuda.get_sync_debug_mode() == 0
    assert t.ts.graph is not None and t.vs.graph is not None
    at = {(what, epoch): n for what, epoch, n in marks}
    return t, at


def test_no_read_back_inside_the_loops(base_net, dataset):
    deltas = {}
    for n_train, n_val in ((4, 2), (8, 4)):
        t, at = _counted_run(base_net, dataset, n_train, n_val)
        # the second epoch: both steps were captured in the first
        assert at[("train_loop_end", 1)] == at[("train_start", 1)], (n_train, at)
        assert at[("val_loop_end", 1)] == at[("val_loop_start", 1)], (n_train, at)
        deltas[n_train] = at[("epoch_end", 1)] - at[("epoch_start", 1)]
        assert len(t.log["train_losses"]) == 2 and np.isfinite(t.log["train_losses"][1])
    print("host waits per epoch:", deltas)
    assert deltas[4] == deltas[8] and deltas[4] > 0, deltas


# ---- 3. resume -------------------------------------------------------------------------------------------------------------------
class _Interrupt(Exception):
    pass


def test_resume_on_the_device(base_net, dataset, tmp_path):
    from dinounet_amd.trainer import Trainer

    class Interrupted(Trainer):
        def on_epoch_start(self):
            if self.current_epoch == 2:
                raise _Interrupt
            super().on_epoch_start()

    def third_epoch(t):
        return t.train_batches.draws[-4:]

    runs = []
    for _ in range(2):
        t = _trainer(base_net, dataset, record=True, num_epochs=3)
        seeded = torch.cuda.get_rng_state(dev())
        t.run_training()
        assert not torch.equal(seeded, torch.cuda.get_rng_state(dev()))                # the steps draw from the device generator
        runs.append(t)
    a, b = runs
    assert len(a.train_batches.draws) == 12
    loss_a = float(a.log["train_losses"][2])
    d0 = abs(loss_a - float(b.log["train_losses"][2]))
    folder = str(tmp_path / "interrupted")
    c = _trainer(base_net, dataset, cls=Interrupted, num_epochs=3, save_every=1, output_folder=folder)
    with pytest.raises(_Interrupt):
        c.run_training()
    assert c.current_epoch == 2 and sorted(os.listdir(folder)) == ["checkpoint_best.pth", "checkpoint_latest.pth"]
    saved = torch.load(os.path.join(folder, "checkpoint_latest.pth"), weights_only=False)
    assert saved["current_epoch"] == 2
    r = _trainer(base_net, dataset, record=True, num_epochs=3, seed=77)                # other seeds: the checkpoint's states must win
    r.load_checkpoint(os.path.join(folder, "checkpoint_latest.pth"))
    assert r.current_epoch == 2 and r.ts is None and r.vs is None
    r.run_training()
    assert len(r.train_batches.draws) == 4
    for (la, aa), (lr, ar) in zip(third_epoch(a), r.train_batches.draws):
        assert _same(la, lr), (la, lr)                                                 # the loader's decisions
        assert _same(aa, ar), (aa, ar)                                                 # the augmentation's decisions
    rlog = r.log.get_checkpoint()
    assert all(len(v) == 3 for v in rlog.values())
    assert _same({k: v[:2] for k, v in rlog.items()}, saved["logging"])
    assert rlog["lrs"] == a.log["lrs"]
    loss_r = float(rlog["train_losses"][2])
    print(f"resume: d0 = {d0:.3e}, uninterrupted {loss_a:.7f}, second run {float(b.log['train_losses'][2]):.7f}, resumed {loss_r:.7f}, "
          f"|resumed - uninterrupted| = {abs(loss_r - loss_a):.3e}")
    if d0 == 0:
        assert loss_r == loss_a
    else:
        assert abs(loss_r - loss_a) <= 4 * d0 + 1e-6 * abs(loss_a), (loss_r, loss_a, d0)


# ---- 4. it learns ----------------------------------------------------------------------------------------------------------------
def test_it_learns(base_net, dataset):
    t = _trainer(base_net, dataset, num_epochs=3, num_iterations_per_epoch=20)
    t.run_training()
    losses = [float(v) for v in t.log["train_losses"]]
    print("train_losses:", losses, "mean_fg_dice:", t.log["mean_fg_dice"])
    assert all(np.isfinite(losses)) and losses[2] < losses[0], losses


# ---- 5. the final validation -----------------------------------------------------------------------------------------------------
def test_perform_actual_validation_summary(base_net, dataset, tmp_path):
    from dinounet_amd.export import case_metrics
    from dinounet_amd.inference import predict_cases_segmentation
    from dinounet_amd.trainer import load_summary_json
    t = _trainer(base_net, dataset, output_folder=str(tmp_path / "fold_0"))
    os.makedirs(t.output_folder)
    refs = {k: dataset[k][1][0].to(torch.uint8) for k in dataset}                      # (D, H, W) label maps
    spacing = (1.0, 0.8, 0.8)
    summary = t.perform_actual_validation(refs, spacings=spacing)
    assert len(t.val_keys) == 2 and [c["case"] for c in summary["metric_per_case"]] == list(t.val_keys)
    segs = predict_cases_segmentation(t.net, [dataset[k][0] for k in t.val_keys], PATCH, 0.5, True, 8, True, None)
    by_hand = [case_metrics(s, refs[k], [1], None, spacing) for k, s in zip(t.val_keys, segs)]
    names = list(by_hand[0][1].keys())
    assert names[:7] == ["Dice", "IoU", "Sensitivity", "Specificity", "Precision", "HD95", "ASD"]
    for c, m in zip(summary["metric_per_case"], by_hand):
        assert _same(c["metrics"], {1: {n: (float(v) if isinstance(v, float) else v) for n, v in m[1].items()}}), (c, m)
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            mean = {1: {n: float(np.nanmean([m[1][n] for m in by_hand])) for n in names}}
    assert _same(summary["mean"], mean), (summary["mean"], mean)
    assert _same(summary["foreground_mean"], {n: float(np.mean([mean[1][n]])) for n in names})
    assert summary["mean"][1]["TP"] + summary["mean"][1]["FN"] == np.mean([int((refs[k] == 1).sum()) for k in t.val_keys])
    path = os.path.join(t.output_folder, "validation", "summary.json")
    assert _same(load_summary_json(path), summary)
    assert set(json.load(open(path))["mean"].keys()) == {"1"}


# ---- 6. the captured validation step reads the live weights ----------------------------------------------------------------------
def test_captured_val_step_reads_the_live_weights(base_net, dataset):
    from dinounet_amd.training import validation_counts
    t = _trainer(base_net, dataset)
    before = [p.detach().clone() for p in t.params]
    t.run_training()
    assert t.vs.graph is not None and t.vs.steps == 0                                  # captured in epoch 0 (one eager step, then the capture)
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, t.params))
    last = t.vs.last()                                                                 # the last replay of epoch 1
    t.net.eval()
    with torch.no_grad():
        logits = t.net(t.vs.x)
    tp, fp, fn = validation_counts(logits, t.vs.tgt)
    assert np.array_equal(last["tp_hard"], tp.cpu().numpy()[1:]), (last, tp)
    assert np.array_equal(last["fp_hard"], fp.cpu().numpy()[1:]) and np.array_equal(last["fn_hard"], fn.cpu().numpy()[1:])
    assert int(tp.sum() + fp.sum() + fn.sum()) > 0
