#!/usr/bin/env python
"""What the epoch loop of dinounet_amd.trainer.Trainer costs over the bare training step: the configuration of bench.py (`dinounet_l`,
512 x 512 patches, batch 8, 3 channels, bf16) on the synthetic resident dataset of tools/dataload_bench.py, a few epochs.

  epoch                 wall time of every epoch (host clock; an epoch ends in ValStep.epoch_end, which waits for the device)
  training loop         on_train_epoch_start .. on_train_epoch_end (the read-back of the loss ring waits for the device): iterations / s
  validation loop       run_validation_loop .. on_validation_epoch_end
  TrainStep replayed    the trainer's own captured step on a static batch (HIP events): the floor of an iteration
  next(train_batches)   the loader and GPUAugment2D alone (HIP events)

    python tools/train_fold.py [--epochs 3] [--iterations 50] [--out profiles/trainer.txt]

One process.  The first epoch holds the eager warm-up steps and both captures and is reported apart from the others.  A watchdog thread
ends the process if a phase does not come back within its limit, so nothing more is started on the GPU after a hang.  A report, not a
threshold."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=24)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--model", default="dinounet_l")
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=50)
    ap.add_argument("--val-iterations", type=int, default=10)
    ap.add_argument("--calls", type=int, default=30, help="timed replays of the bare step / calls of the batch iterator")
    ap.add_argument("--limit", type=float, default=300.0, help="seconds a phase (an epoch, a timed block) may take")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from dataload_bench import limited, synthetic_case
    from dinounet_amd import dataloading as DL
    from dinounet_amd.network_architecture import DinoUNet
    from dinounet_amd.plans import PLANS_2D
    from dinounet_amd.trainer import Trainer
    if not torch.cuda.is_available():
        raise SystemExit("train_fold needs the GPU: no timing is taken without it")
    dev = torch.device("cuda", 0)
    patch = (a.size, a.size)

    ds = DL.DeviceDataset()
    for i in range(a.cases):
        d, s = synthetic_case(i, a.size)
        d, s = torch.from_numpy(d).to(dev), torch.from_numpy(s).to(dev)
        ds.add(f"case{i:03d}", d, s, limited(a.limit, lambda: DL.add_class_locations(s, {}, [1])))
    torch.manual_seed(1234)
    net = DinoUNet.from_config(PLANS_2D, 3, 2, dinov3_pretrained_path=None, dinov3_model_name=a.model, precision="bf16").to(dev).train()

    phases = []

    class Timed(Trainer):
        def on_epoch_start(self):
            torch.cuda.synchronize()
            self._t = {"epoch": time.perf_counter()}
            super().on_epoch_start()

        def on_train_epoch_start(self):
            self._t["train"] = time.perf_counter()
            super().on_train_epoch_start()

        def on_train_epoch_end(self):
            super().on_train_epoch_end()                  # reads the ring back: the loop's work is done
            self._t["train"] = time.perf_counter() - self._t["train"]

        def run_validation_loop(self):
            self._t["val"] = time.perf_counter()
            super().run_validation_loop()

        def on_validation_epoch_end(self):
            super().on_validation_epoch_end()             # epoch_end waits for the device
            self._t["val"] = time.perf_counter() - self._t["val"]

        def on_epoch_end(self):
            super().on_epoch_end()
            self._t["epoch"] = time.perf_counter() - self._t["epoch"]
            phases.append(dict(self._t))

        def run_training(self):
            self.on_train_start()
            for _ in range(self.current_epoch, self.num_epochs):          # the reference's loop, every epoch under the watchdog
                limited(a.limit, self._one_epoch)
            self.on_train_end()

        def _one_epoch(self):
            self.on_epoch_start()
            self.on_train_epoch_start()
            self.run_train_loop()
            self.on_train_epoch_end()
            self.on_validation_epoch_start()
            self.run_validation_loop()
            self.on_validation_epoch_end()
            self.on_epoch_end()

    t = Timed(net, ds, fold=0, patch_size=patch, batch_size=a.batch, num_classes=2, num_epochs=a.epochs,
              num_iterations_per_epoch=a.iterations, num_val_iterations_per_epoch=a.val_iterations, seed=1, graph=True)
    t.run_training()
    log = t.log.get_checkpoint()

    def timed(fn):
        def block():
            for _ in range(3):
                fn()
            times = []
            for _ in range(a.calls):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1))
            return times
        return limited(a.limit, block)

    fmt = lambda ts: f"{statistics.median(ts):.3f} ms  [{min(ts):.3f} .. {max(ts):.3f}]"
    t_step = timed(lambda: t.ts())                         # the captured step on the batch that is in its static buffers
    t_batch = timed(lambda: next(t.train_batches))
    t_vstep = timed(lambda: t.vs())
    t.vs.reset()
    step, batch, vstep = (statistics.median(v) for v in (t_step, t_batch, t_vstep))
    steady = phases[1:] if len(phases) > 1 else phases
    it_ms = statistics.median(1e3 * p["train"] / a.iterations for p in steady)
    val_ms = statistics.median(1e3 * p["val"] / a.val_iterations for p in steady)
    lines = [f"# Trainer.run_training, {a.model} bf16, patch {patch}, batch {a.batch}, {a.cases} resident synthetic cases "
             f"({len(t.train_keys)} train / {len(t.val_keys)} val), {a.epochs} epochs x {a.iterations} + {a.val_iterations} iterations; "
             f"train step {t.ts.capture_mode}, validation step {'captured' if t.vs.graph is not None else 'eager'}"]
    for e, p in enumerate(phases):
        lines.append(f"epoch {e}: {p['epoch']:.3f} s wall; training loop {p['train']:.3f} s = {a.iterations / p['train']:.2f} it/s "
                     f"({1e3 * p['train'] / a.iterations:.2f} ms / it); validation loop {p['val']:.3f} s "
                     f"({1e3 * p['val'] / a.val_iterations:.2f} ms / it); train loss {float(log['train_losses'][e]):.4f}, "
                     f"val loss {float(log['val_losses'][e]):.4f}, lr {log['lrs'][e]:.5f}"
                     + ("   <- eager warm-up steps and both captures" if e == 0 else ""))
    lines += [f"TrainStep replayed on a static batch ({a.calls} calls, HIP events): {fmt(t_step)} = {a.batch / step * 1e3:.1f} slices/s",
              f"next(train_batches) alone (loader + GPUAugment2D): {fmt(t_batch)}",
              f"ValStep replayed on a static batch: {fmt(t_vstep)}",
              f"training iteration in the loop, epochs 1.. (median): {it_ms:.3f} ms = {a.batch / it_ms * 1e3:.1f} slices/s; "
              f"over the bare step {it_ms - step:+.3f} ms ({100 * (it_ms / step - 1):+.1f} %); loader + augmentation alone {batch:.3f} ms; "
              f"not accounted for by them {it_ms - step - batch:+.3f} ms",
              f"validation iteration in the loop, epochs 1.. (median): {val_ms:.3f} ms; over the bare validation step {val_ms - vstep:+.3f} ms"]
    lines.append(json.dumps({"epochs": phases, "step_ms": [round(v, 3) for v in t_step], "batch_ms": [round(v, 3) for v in t_batch],
                             "val_step_ms": [round(v, 3) for v in t_vstep], "iteration_ms": round(it_ms, 3),
                             "val_iteration_ms": round(val_ms, 3), "capture_mode": t.ts.capture_mode}))
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
