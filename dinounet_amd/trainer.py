"""A fold trained end to end on the device: the epoch loop of the reference trainer (nnUNetTrainer.run_training,
dinounet/training/nnUNetTrainer/nnUNetTrainer.py:1295-1318) over the pieces this package already has -- DeviceDataset / TrainBatches for
the batches, TrainStep / ValStep for the two captured steps, FusedClipSGD, checkpoint.save_checkpoint, predict_cases_segmentation and
case_metrics for the final validation -- so that a fold trains where the reference is not installed.

    poly_lr                     PolyLRScheduler.step (lr_scheduler/polylr.py:18)
    TrainLog                    nnUNetLogger without the plots (logging/nnunet_logger.py:18-52, 99-103)
    generate_crossval_split     utilities/crossval_split.py, KFold(shuffle=True) restated in numpy
    do_split                    nnUNetTrainer.do_split (:530-585) on a list of keys
    Trainer                     on_train_start .. on_train_end, run_training, save / load_checkpoint, perform_actual_validation

The loop adds no kernel.  What it adds is that the host never waits for the device inside an epoch: the reference reads every step's loss
back (`l.detach().cpu().numpy()`, :929); here the step's loss scalar is copied device-to-device into a slot of a per-epoch ring, and an
epoch has two read-back points whatever the iteration counts are -- the ring at the end of the training loop, ValStep.epoch_end at the
end of the validation loop."""
import json
import os
import time
import warnings

import numpy as np
import torch
import torch.distributed as dist

from . import checkpoint as _checkpoint

LOG_KEYS = ("mean_fg_dice", "ema_fg_dice", "dice_per_class_or_region", "train_losses", "val_losses", "lrs", "epoch_start_timestamps",
            "epoch_end_timestamps")


# ------------------------------------------------------------------------------------------------ the host-side pieces
def poly_lr(initial_lr, epoch, num_epochs, exponent=0.9):
    """the learning rate of `epoch` (polylr.py:18), in the reference's floating-point operations"""
    return initial_lr * (1 - epoch / num_epochs) ** exponent


class TrainLog:
    """nnUNetLogger's eight per-epoch lists (nnunet_logger.py:18-27) without the plots.  log(key, value, epoch) appends the value of a new
    epoch and overwrites the value of the current one (:40-46); any other epoch raises.  Logging 'mean_fg_dice' also logs 'ema_fg_dice' =
    0.9 * previous + 0.1 * value, the first value as it is (:49-52).  get_checkpoint() is the dict of lists itself, which is what the
    reference's logger loads."""

    def __init__(self, verbose=False):
        self.lists = {k: [] for k in LOG_KEYS}
        self.verbose = verbose

    def __getitem__(self, key):
        return self.lists[key]

    def log(self, key, value, epoch):
        if key not in self.lists:
            raise KeyError(f"TrainLog: {key!r} is not one of {LOG_KEYS}")
        values = self.lists[key]
        if self.verbose:
            print(f"logging {key}: {value} for epoch {epoch}")
        if len(values) < epoch + 1:
            values.append(value)
        elif len(values) == epoch + 1:
            values[epoch] = value
        else:
            raise ValueError(f"TrainLog: {key!r} holds {len(values)} epochs, epoch {epoch} can be neither appended nor overwritten")
        if key == "mean_fg_dice":
            ema = self.lists["ema_fg_dice"]
            self.log("ema_fg_dice", ema[epoch - 1] * 0.9 + 0.1 * value if len(ema) > 0 else value, epoch)

    def get_checkpoint(self):
        return self.lists

    def load_checkpoint(self, lists):
        missing = [k for k in LOG_KEYS if k not in lists]
        if missing:
            raise KeyError(f"TrainLog: the checkpointed log lacks {missing}")
        self.lists = {k: list(v) for k, v in lists.items()}


def generate_crossval_split(identifiers, seed=12345, n_splits=5):
    """crossval_split.py without sklearn: KFold(n_splits, shuffle=True, random_state=seed).split(identifiers) shuffles arange(n) with
    RandomState(seed) and cuts it into n_splits consecutive folds, the first n % n_splits of them one element longer; a fold's members are
    the validation cases, all others the training cases, both in ascending index order.  -> [{'train': [...], 'val': [...]}, ...]"""
    identifiers = list(identifiers)
    n, k = len(identifiers), int(n_splits)
    if k < 2 or k > n:
        raise ValueError(f"cannot cut {n} cases into {k} folds")
    order = np.arange(n)
    np.random.RandomState(seed).shuffle(order)
    sizes = [n // k + (1 if f < n % k else 0) for f in range(k)]
    splits, at = [], 0
    for size in sizes:
        held_out = np.zeros(n, bool)
        held_out[order[at:at + size]] = True
        at += size
        splits.append({"train": [identifiers[i] for i in range(n) if not held_out[i]],
                       "val": [identifiers[i] for i in range(n) if held_out[i]]})
    return splits


def do_split(keys, fold, splits=None):
    """nnUNetTrainer.do_split (:530-585) -> (train keys, validation keys).  fold "all": every key trains and validates.  `splits`: the
    content of a splits file (a list of {'train', 'val'}); None: the five-fold split of the sorted keys (generate_crossval_split).  A fold
    inside the splits is used as listed; one beyond them gives the seeded 80:20 split of the sorted keys, RandomState(12345 + fold)."""
    keys = list(keys)
    if fold == "all":
        return keys, list(keys)
    fold = int(fold)
    ordered = sorted(keys)
    if splits is None:
        splits = generate_crossval_split(ordered, seed=12345, n_splits=5)
    if fold < len(splits):
        return list(splits[fold]["train"]), list(splits[fold]["val"])
    rnd = np.random.RandomState(seed=12345 + fold)
    chosen = rnd.choice(len(ordered), int(len(ordered) * 0.8), replace=False)
    taken = set(int(i) for i in chosen)
    return [ordered[int(i)] for i in chosen], [ordered[i] for i in range(len(ordered)) if i not in taken]


# ------------------------------------------------------------------------------------------------ the summary of the final validation
def _plain(v):
    """numpy scalars and arrays -> Python numbers and lists (what json takes), recursively"""
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, np.ndarray):
        return _plain(v.tolist())
    if isinstance(v, (np.floating, np.integer, np.bool_)):
        return v.item()
    return v


def _label_key(s):
    """the inverse of str() on a label (int) or a region (tuple of ints)"""
    try:
        return int(s)
    except ValueError:
        return tuple(int(p) for p in s.strip("()").split(",") if p.strip())


def summarise_cases(metric_per_case, labels_or_regions):
    """compute_metrics_on_folder's result (evaluate_predictions.py:278-299) from the per-case metrics: 'mean'[label][metric] is np.nanmean
    over the cases, 'foreground_mean'[metric] np.mean of those over the labels (a label 0 left out), all as Python numbers"""
    keys = [tuple(r) if isinstance(r, list) else r for r in labels_or_regions]
    names = list(metric_per_case[0]["metrics"][keys[0]].keys())
    means = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # a metric that is nan in every case: its mean is nan
        for r in keys:
            means[r] = {m: np.nanmean([c["metrics"][r][m] for c in metric_per_case]) for m in names}
        fg = {m: np.mean([means[r][m] for r in keys if r != 0 and r != "0"]) for m in names}
    return {"metric_per_case": _plain(metric_per_case), "mean": _plain(means), "foreground_mean": _plain(fg)}


def save_summary_json(summary, path):
    """json has no int or tuple keys: labels and regions are written as their str() (evaluate_predictions.py:42-56)"""
    out = dict(summary)
    out["mean"] = {str(k): v for k, v in summary["mean"].items()}
    out["metric_per_case"] = [dict(c, metrics={str(k): v for k, v in c["metrics"].items()}) for c in summary["metric_per_case"]]
    with open(path, "w") as f:
        json.dump(out, f, sort_keys=True, indent=4)


def load_summary_json(path):
    with open(path) as f:
        s = json.load(f)
    s["mean"] = {_label_key(k): v for k, v in s["mean"].items()}
    for c in s["metric_per_case"]:
        c["metrics"] = {_label_key(k): v for k, v in c["metrics"].items()}
    return s


# ------------------------------------------------------------------------------------------------ the trainer
def _view(dataset, keys):
    """the cases of a DeviceDataset under a list of keys, in that order: a DeviceDataset that shares the tensors"""
    from .dataloading import DeviceDataset
    view = DeviceDataset()
    for k in keys:
        view._cases[k] = dataset[k]                         # already validated and contiguous: shared, not copied
    return view


class Trainer:
    """nnUNetTrainer's training loop for one fold of a DeviceDataset (defaults: nnUNetTrainer.py:146-151, 187).

    net: the network, already on its device (the trainable parameters are those with requires_grad).  dataset: a DeviceDataset; do_split
    (fold, splits) selects the training and the validation cases.  The loss is build_loss(num_classes, regions, ignore_label, topk_percent,
    **loss_options) (loss_options: None or a dict of build_loss's weight_ce, weight_dice, batch_dice, do_bg, ce_class_weights; kept in init_args),
    with deep_supervision wrapped with deep_supervision_weights(number of decoder outputs, world > 1).  The optimiser is FusedClipSGD(initial_lr,
    momentum 0.99, nesterov, weight_decay) on the GPU and torch.optim.SGD with the same numbers on the CPU, unless `optimizer` is given.
    The batches are TrainBatches(val=False) seeded with `seed` (augmentation: seed + 1) and TrainBatches(val=True) seeded with seed + 2,
    unless `train_batches` / `val_batches` are given: any iterators of (x, target); that is how a CPU run (GPUAugment2D has no CPU path)
    or another pipeline comes in.  TrainStep and ValStep are built on the shapes of the first batches.  With a `seed` the device
    generator (DropPath masks, RoPE rescale) is seeded too.

    run_training() continues at current_epoch, which load_checkpoint sets.  Per epoch the host reads the device twice: the ring of the
    training losses, and ValStep.epoch_end.  Only rank 0 writes files, and only with an output_folder."""

    def __init__(self, net, dataset, *, fold=0, splits=None, patch_size, batch_size, num_classes, regions=None, ignore_label=None,
                 all_labels=None, num_epochs=1000, num_iterations_per_epoch=250, num_val_iterations_per_epoch=10, initial_lr=1e-2,
                 weight_decay=3e-5, oversample_foreground_percent=0.33, save_every=50, output_folder=None, seed=None, graph=True,
                 interpolation="keys", use_mask_for_norm=None, deep_supervision=False, topk_percent=None, reducer=None, rank=0, world=1,
                 train_batches=None, val_batches=None, optimizer=None, loss_options=None):
        from .dataloading import TrainBatches
        from .training import build_loss, deep_supervision_weights
        self.net, self.dataset = net, dataset
        self.device = next(net.parameters()).device
        self.fold, self.splits = fold, splits
        self.patch_size = tuple(int(v) for v in patch_size)
        self.batch_size, self.num_classes = int(batch_size), int(num_classes)
        self.regions, self.ignore_label, self.all_labels = regions, ignore_label, all_labels
        self.num_epochs, self.num_iterations_per_epoch = int(num_epochs), int(num_iterations_per_epoch)
        self.num_val_iterations_per_epoch = int(num_val_iterations_per_epoch)
        if self.num_epochs < 1 or self.num_iterations_per_epoch < 1 or self.num_val_iterations_per_epoch < 1 or int(save_every) < 1:
            raise ValueError("num_epochs, the two iteration counts and save_every must be positive")
        self.initial_lr, self.weight_decay = float(initial_lr), float(weight_decay)
        self.oversample_foreground_percent = float(oversample_foreground_percent)
        self.save_every = int(save_every)
        self.output_folder = None if output_folder is None else str(output_folder)
        self.seed = seed
        self.use_graph = bool(graph) and self.device.type == "cuda"
        self.reducer, self.rank, self.world = reducer, int(rank), int(world)
        self.group = dist.group.WORLD if self.world > 1 else None
        self.inference_allowed_mirroring_axes = (0, 1)
        self.init_args = dict(fold=fold, splits=splits, patch_size=self.patch_size, batch_size=self.batch_size, num_classes=self.num_classes,
                              regions=regions, ignore_label=ignore_label, all_labels=all_labels, num_epochs=self.num_epochs,
                              num_iterations_per_epoch=self.num_iterations_per_epoch,
                              num_val_iterations_per_epoch=self.num_val_iterations_per_epoch, initial_lr=self.initial_lr,
                              weight_decay=self.weight_decay, oversample_foreground_percent=self.oversample_foreground_percent,
                              save_every=self.save_every, seed=seed, graph=bool(graph), interpolation=interpolation,
                              use_mask_for_norm=use_mask_for_norm, deep_supervision=bool(deep_supervision), topk_percent=topk_percent,
                              world=self.world)
        # the options of the reference's loss classes (build_loss: weight_ce, weight_dice, batch_dice, do_bg, ce_class_weights) as plain
        # Python values; None leaves init_args, and so the checkpoint, without the key
        self.loss_options = None
        if loss_options is not None:
            unknown = set(loss_options) - {"weight_ce", "weight_dice", "batch_dice", "do_bg", "ce_class_weights"}
            if unknown:
                raise ValueError(f"loss_options: unknown keys {sorted(unknown)}")
            self.loss_options = {k: ([float(w) for w in v] if k == "ce_class_weights" and v is not None else v)
                                 for k, v in loss_options.items()}
            self.init_args["loss_options"] = self.loss_options
        if seed is not None:
            # the default generator of the trainer's device alone (the steps draw from it): no other generator of the process is touched
            if self.device.type == "cuda":
                index = torch.cuda.current_device() if self.device.index is None else self.device.index
                torch.cuda.default_generators[index].manual_seed(int(seed))
            else:
                torch.default_generator.manual_seed(int(seed))

        self.train_keys, self.val_keys = do_split(list(dataset.keys()), fold, splits)
        ds_weights = None
        if deep_supervision:
            heads = getattr(getattr(net, "decoder", None), "seg_layers", None)
            if heads is None:
                raise ValueError("deep_supervision: the number of outputs is read from net.decoder.seg_layers, which this network lacks")
            ds_weights = deep_supervision_weights(len(heads), ddp=self.world > 1)
        self.loss = build_loss(self.num_classes, regions=regions, ignore_label=ignore_label, ddp=True if self.world > 1 else None,
                               group=None, deep_supervision_weights=ds_weights, topk_percent=topk_percent, **(self.loss_options or {}))
        self.params = [p for p in net.parameters() if p.requires_grad]
        if optimizer is not None:
            self.optimizer = optimizer
        elif self.device.type == "cuda":
            from .optim import FusedClipSGD
            self.optimizer = FusedClipSGD(self.params, lr=self.initial_lr, momentum=0.99, nesterov=True, weight_decay=self.weight_decay)
        else:
            self.optimizer = torch.optim.SGD(self.params, lr=self.initial_lr, momentum=0.99, nesterov=True, weight_decay=self.weight_decay)

        def batches(keys, val, s):
            return TrainBatches(_view(dataset, keys), self.patch_size, self.batch_size, self.oversample_foreground_percent,
                                all_labels=all_labels, ignore_label=ignore_label, seed=s, rank=self.rank, world=self.world, val=val,
                                interpolation=interpolation, use_mask_for_norm=use_mask_for_norm)
        self.train_batches = train_batches if train_batches is not None else batches(self.train_keys, False, seed)
        self.val_batches = val_batches if val_batches is not None else batches(self.val_keys, True, None if seed is None else int(seed) + 2)

        self.log = TrainLog()
        self.current_epoch = 0
        self._best_ema = None
        self.ts = self.vs = None                            # built on the first batches (on their shapes)
        self._ring = torch.zeros(self.num_iterations_per_epoch, dtype=torch.float32, device=self.device)
        self._slots = list(self._ring.unbind(0))            # views made once: the loop only issues the copies

    # ---- what only rank 0 does ---------------------------------------------------------------------------------------------------
    def _writes(self):
        return self.rank == 0 and self.output_folder is not None

    def _path(self, name):
        return os.path.join(self.output_folder, name)

    def _stamp(self):
        """time(); with several ranks rank 0's, so that every rank keeps the same log"""
        t = [time.time()]
        if self.world > 1:
            dist.broadcast_object_list(t, src=0)
        return t[0]

    # ---- the steps ---------------------------------------------------------------------------------------------------------------
    def _train_step(self, x, target):
        if self.ts is None:
            from .training import TrainStep
            self.ts = TrainStep(self.net, self.optimizer, self.params, tuple(x.shape), tuple(target.shape), self.device,
                                reducer=self.reducer, graph=self.use_graph, warmup=3, loss=self.loss)
        return self.ts(x, target)

    def _val_step(self, x, target):
        if self.vs is None:
            from .training import ValStep
            # (one eager step, then the capture: with the reference's 10 validation iterations both captures exist after the first epoch)
            self.vs = ValStep(self.net, tuple(x.shape), tuple(target.shape), self.device, loss=self.loss, graph=self.use_graph, warmup=1)
        return self.vs(x, target)

    def _drop_captures(self):
        """forget the captured steps (and the sliding-window forwards cached on the network): the next step builds them again"""
        from .inference import clear_window_cache
        for step in (self.ts, self.vs):
            g = getattr(step, "graph", None)
            if g is not None:
                g.reset()
        self.ts = self.vs = None
        clear_window_cache(self.net)

    # ---- the reference's hooks ---------------------------------------------------------------------------------------------------
    def on_train_start(self):
        if self._writes():
            os.makedirs(self.output_folder, exist_ok=True)
        if self.world > 1:
            dist.barrier()

    def on_epoch_start(self):
        self.log.log("epoch_start_timestamps", self._stamp(), self.current_epoch)

    def on_train_epoch_start(self):
        self.net.train()
        lr = poly_lr(self.initial_lr, self.current_epoch, self.num_epochs)
        self.optimizer.param_groups[0]["lr"] = lr           # FusedClipSGD carries it into a replayed graph (its pinned buffer)
        self.log.log("lrs", lr, self.current_epoch)

    def run_train_loop(self):
        """num_iterations_per_epoch steps; the host reads nothing back: step i's loss goes device-to-device into ring slot i"""
        batches, slots = self.train_batches, self._slots
        for i in range(self.num_iterations_per_epoch):
            x, target = next(batches)
            slots[i].copy_(self._train_step(x, target), non_blocking=True)

    def on_train_epoch_end(self):
        """train_losses = np.mean of the epoch's losses as float32 (:939); with several ranks over every rank's ring (:934-937)"""
        ring = self._ring
        if self.world > 1:
            rings = [torch.empty_like(ring) for _ in range(self.world)]
            dist.all_gather(rings, ring, group=self.group)
            ring = torch.stack(rings)
        self.log.log("train_losses", np.mean(ring.cpu().numpy()), self.current_epoch)            # the read-back

    def on_validation_epoch_start(self):
        pass                                                # ValStep puts the network into eval mode for its step and restores it

    def run_validation_loop(self):
        batches = self.val_batches
        for _ in range(self.num_val_iterations_per_epoch):
            x, target = next(batches)
            self._val_step(x, target)

    def on_validation_epoch_end(self):
        out = self.vs.epoch_end(group=self.group)           # the read-back; zeroes the accumulators
        self.log.log("mean_fg_dice", out["mean_fg_dice"], self.current_epoch)
        self.log.log("dice_per_class_or_region", out["dice_per_class_or_region"], self.current_epoch)
        self.log.log("val_losses", out["val_loss"], self.current_epoch)

    def on_epoch_end(self):
        """the checkpoint policy of :1067-1081"""
        self.log.log("epoch_end_timestamps", self._stamp(), self.current_epoch)
        epoch = self.current_epoch
        if (epoch + 1) % self.save_every == 0 and epoch != self.num_epochs - 1:
            self.save_checkpoint("checkpoint_latest.pth")
        ema = self.log["ema_fg_dice"][-1]
        if self._best_ema is None or ema > self._best_ema:
            self._best_ema = ema
            self.save_checkpoint("checkpoint_best.pth")
        self.current_epoch += 1

    def on_train_end(self):
        self.current_epoch -= 1                             # save_checkpoint stores current_epoch + 1 = num_epochs (:864-868)
        self.save_checkpoint("checkpoint_final.pth")
        self.current_epoch += 1
        if self._writes() and os.path.isfile(self._path("checkpoint_latest.pth")):
            os.remove(self._path("checkpoint_latest.pth"))

    def run_training(self):
        self.on_train_start()
        for _ in range(self.current_epoch, self.num_epochs):
            self.on_epoch_start()
            self.on_train_epoch_start()
            self.run_train_loop()
            self.on_train_epoch_end()
            self.on_validation_epoch_start()
            self.run_validation_loop()
            self.on_validation_epoch_end()
            self.on_epoch_end()
        self.on_train_end()

    # ---- checkpoints -------------------------------------------------------------------------------------------------------------
    def _rng_states(self):
        """what a resume needs beyond the reference's fields: the host RandomStates of the loaders and of the augmentation, and the state
        of the device's generator"""
        def host(obj, *path):
            for name in path:
                obj = getattr(obj, name, None)
            return None if obj is None else obj.get_state()
        dev = torch.cuda.get_rng_state(self.device) if self.device.type == "cuda" else torch.get_rng_state()
        return {"loader": host(self.train_batches, "loader", "rs"), "augment": host(self.train_batches, "augment", "rs"),
                "val_loader": host(self.val_batches, "loader", "rs"), "device": dev}

    def _set_rng_states(self, states):
        def host(state, obj, *path):
            for name in path:
                obj = getattr(obj, name, None)
            if state is not None and obj is not None:
                obj.set_state(state)
        host(states.get("loader"), self.train_batches, "loader", "rs")
        host(states.get("augment"), self.train_batches, "augment", "rs")
        host(states.get("val_loader"), self.val_batches, "loader", "rs")
        if states.get("device") is not None:
            dev = states["device"].cpu()
            if self.device.type == "cuda":
                torch.cuda.set_rng_state(dev, self.device)
            else:
                torch.set_rng_state(dev)

    def save_checkpoint(self, path):
        """nnUNetTrainer.save_checkpoint (:1083-1106) through checkpoint.save_checkpoint (the compact network weights); a bare file name
        lands in output_folder.  Rank 0 alone writes, and only with an output folder (or an absolute path)."""
        path = str(path)
        if not os.path.isabs(path) and os.path.dirname(path) == "":
            if self.output_folder is None:
                return None
            path = self._path(path)
        if self.rank != 0:
            return None
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        _checkpoint.save_checkpoint(path, self.net, self.optimizer, logging=self.log.get_checkpoint(), _best_ema=self._best_ema,
                                    current_epoch=self.current_epoch + 1, init_args=self.init_args, trainer_name=type(self).__name__,
                                    inference_allowed_mirroring_axes=self.inference_allowed_mirroring_axes, rng_states=self._rng_states())
        return path

    def load_checkpoint(self, path_or_dict):
        """nnUNetTrainer.load_checkpoint (:1108-1144) and the three random states.  Weights and momentum buffers are restored before any
        capture; captures that exist are dropped, so the graphs are built again against the restored tensors."""
        self._drop_captures()
        src = path_or_dict if isinstance(path_or_dict, dict) else str(path_or_dict)
        ckpt = _checkpoint.load_checkpoint(src, self.net, self.optimizer, map_location=self.device)
        self.log.load_checkpoint(ckpt["logging"])
        self.current_epoch = int(ckpt["current_epoch"])
        self._best_ema = ckpt["_best_ema"]
        self.inference_allowed_mirroring_axes = ckpt.get("inference_allowed_mirroring_axes", self.inference_allowed_mirroring_axes)
        if ckpt.get("rng_states") is not None:
            self._set_rng_states(ckpt["rng_states"])
        return ckpt

    # ---- the final validation ----------------------------------------------------------------------------------------------------
    def perform_actual_validation(self, references, spacings=None, labels_or_regions=None, regions_class_order=None, tile_step_size=0.5,
                                  batch_size=8, graph=None):
        """nnUNetTrainer.perform_actual_validation (:1146-1290) without files: the validation cases of the fold go through the
        sliding-window predictor (tile step 0.5, Gaussian weights, no mirroring) and the export to label maps -- in the raw geometry where
        a case's properties describe it --, then export.case_metrics against references[key] (a uint8 label map of the prediction's
        shape, a leading axis of 1 allowed).  spacings: None, three floats for every case, or a dict key -> three floats; with a spacing
        HD95 and ASD are computed.  labels_or_regions defaults to the regions, else the foreground classes 1..num_classes-1.
        -> compute_metrics_on_folder's dict ('metric_per_case', 'mean', 'foreground_mean'; summarise_cases), on every rank; rank 0 writes it
        to <output_folder>/validation/summary.json.  With several ranks rank r predicts val_keys[r::world]."""
        from .export import case_metrics
        from .inference import predict_cases_segmentation
        if labels_or_regions is None:
            labels_or_regions = list(self.regions) if self.regions is not None else list(range(1, self.num_classes))
        labels_or_regions = [tuple(r) if isinstance(r, list) else r for r in labels_or_regions]
        keys = list(self.val_keys)[self.rank::self.world] if self.world > 1 else list(self.val_keys)
        per_case = []
        if keys:
            props = [self.dataset[k][2] for k in keys]
            raw = all(isinstance(p, dict) and "shape_after_cropping_and_before_resampling" in p for p in props)
            segs = predict_cases_segmentation(self.net, [self.dataset[k][0] for k in keys], self.patch_size, tile_step_size, True,
                                              batch_size, self.use_graph if graph is None else bool(graph), None,
                                              regions_class_order=regions_class_order, properties=props if raw else None)
            for k, seg in zip(keys, segs):
                ref = torch.as_tensor(references[k]).to(device=seg.device, dtype=torch.uint8).reshape(seg.shape)
                spacing = spacings.get(k) if isinstance(spacings, dict) else spacings
                per_case.append({"case": k, "metrics": case_metrics(seg, ref, labels_or_regions, self.ignore_label, spacing)})
        if self.world > 1:
            shares = [None] * self.world
            dist.all_gather_object(shares, per_case)
            by_key = {c["case"]: c for share in shares for c in share}
            per_case = [by_key[k] for k in self.val_keys]
        summary = summarise_cases(per_case, labels_or_regions)
        if self._writes():
            os.makedirs(self._path("validation"), exist_ok=True)
            save_summary_json(summary, os.path.join(self._path("validation"), "summary.json"))
        return summary
