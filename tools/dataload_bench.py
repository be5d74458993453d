#!/usr/bin/env python
"""What producing a training batch on the device costs next to the training step it feeds: the `dinounet_l` configuration of bench.py
(512 x 512 patches, batch 8, 3 channels) on synthetic cases that stay resident on the GPU (dinounet_amd.dataloading.DeviceDataset).

  add_class_locations   per case: count the masks, read the totals back, draw the ranks on the host, select by rank, mirror the tables
  next(loader)          DataLoader2D at the initial patch size (602 x 602): the host draws, one job table upload, one gather launch
  next(TrainBatches)    the loader, GPUAugment2D and the cast of the labels: what TrainStep is handed
  TrainStep             the captured step of bench.py on the batch TrainBatches made, and the two in a loop (batch, then step)

    python tools/dataload_bench.py [--cases 24] [--calls 20] [--out profiles/dataload.txt]

One process.  Every timed region lies between two HIP events on the current stream and is read after a synchronisation; the host work
of a region (the draws, the read-back of the totals) is inside it, because the stream waits for it.  The median of `--calls` timed calls
after `--warmup` untimed ones.  Every device step runs under its own time limit: a watchdog thread
(faulthandler.dump_traceback_later(limit, exit=True)) ends the process if a step does not come back, so nothing more is started on the
GPU after a hang.  No threshold is set: the tool records the loader's share of a step."""
import argparse
import faulthandler
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic_case(i, size):
    """(data (3, D, H, W) fp32, seg (1, D, H, W) int16): a natural-image-like case a little larger or smaller than the patch, one
    foreground class in a few blobs; every fourth case is a short stack of slices"""
    import numpy as np
    rng = np.random.RandomState(1000 + i)
    D = 4 if i % 4 == 3 else 1
    H, W = (int(size * f) for f in rng.uniform(0.8, 1.4, 2))
    data = rng.randn(3, D, H, W).astype(np.float32)
    seg = np.zeros((1, D, H, W), np.int16)
    yy, xx = np.mgrid[0:H, 0:W]
    for _ in range(3):
        z, cy, cx, r = rng.randint(0, D), rng.randint(0, H), rng.randint(0, W), rng.randint(size // 16, size // 4)
        seg[0, z][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 1
    return data, seg


def limited(limit, fn):
    """fn() under a time limit of its own: the watchdog ends the process if it does not return"""
    faulthandler.dump_traceback_later(limit, exit=True)
    try:
        return fn()
    finally:
        faulthandler.cancel_dump_traceback_later()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=24)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--model", default="dinounet_l")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-limit", type=float, default=120.0, help="seconds every device step may take")
    ap.add_argument("--no-step", action="store_true", help="time the loader only, without the network")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from dinounet_amd import dataloading as DL
    if not torch.cuda.is_available():
        raise SystemExit("dataload_bench needs the GPU: no timing is taken without it")
    dev = torch.device("cuda", 0)

    def timed(fn, calls=a.calls, warmup=a.warmup):
        def once():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize()
            return out, e0.elapsed_time(e1)
        for _ in range(warmup):
            out, _ = limited(a.step_limit, once)
        times = []
        for _ in range(calls):
            out, t = limited(a.step_limit, once)
            times.append(t)
        return out, times

    def fmt(times):
        return f"{statistics.median(times):.3f} ms  [{min(times):.3f} .. {max(times):.3f}]"

    patch = (a.size, a.size)
    raw = [synthetic_case(i, a.size) for i in range(a.cases)]
    on_dev = limited(a.step_limit, lambda: [(torch.from_numpy(d).to(dev), torch.from_numpy(s).to(dev)) for d, s in raw])
    ds = DL.DeviceDataset()
    t_loc, rows = [], 0
    for i, (d, s) in enumerate(on_dev):
        props, t = timed(lambda: DL.add_class_locations(s, {}, [1]), calls=3, warmup=1 if i else a.warmup)
        t_loc.append(statistics.median(t))
        rows += len(props["class_locations"][1])
        ds.add(f"case{i:03d}", d, s, props)
    voxels = sum(s.numel() for _, s in on_dev)
    lines = [f"# training batches on the device, ms per call, median [min .. max] of {a.calls} calls after {a.warmup}; HIP events",
             f"dataset: {a.cases} cases, 3 channels, {voxels / 1e6:.1f} M voxels, {ds.nbytes() / 1e6:.1f} MB resident, {rows} table rows",
             f"add_class_locations per case (median of 3 calls each, over the cases): {fmt(t_loc)}"]
    record = {"cases": a.cases, "resident_bytes": ds.nbytes(), "class_locations_ms": [round(t, 3) for t in t_loc]}

    init = DL.initial_patch_size(patch)
    loader = DL.DataLoader2D(ds, a.batch, init, patch, (0, 1), False, seed=1)
    batch, t_loader = timed(lambda: next(loader))
    draw = loader.draw()
    _, t_gather = timed(lambda: loader.assemble(draw))
    nbytes = batch["data"].numel() * 4 + batch["seg"].numel() * 2
    lines += [f"next(DataLoader2D), batch {a.batch}, patch {init} -> data {tuple(batch['data'].shape)}: {fmt(t_loader)}",
              f"  of which assemble (job table upload + du_dl_gather, {nbytes / 1e6:.1f} MB written): {fmt(t_gather)}"]
    tb = DL.TrainBatches(ds, patch, a.batch, seed=1)
    (x, tgt), t_tb = timed(lambda: next(tb))
    lines.append(f"next(TrainBatches) -> x {tuple(x.shape)} {x.dtype}, target {tuple(tgt.shape)} {tgt.dtype}: {fmt(t_tb)}")
    record.update(loader_ms=[round(t, 3) for t in t_loader], gather_ms=[round(t, 3) for t in t_gather],
                  train_batches_ms=[round(t, 3) for t in t_tb])

    if not a.no_step:
        from dinounet_amd.network_architecture import DinoUNet
        from dinounet_amd.optim import FusedClipSGD
        from dinounet_amd.plans import PLANS_2D
        from dinounet_amd.training import TrainStep
        torch.manual_seed(1234)
        net = DinoUNet.from_config(PLANS_2D, 3, 2, dinov3_pretrained_path=None, dinov3_model_name=a.model, precision="bf16").to(dev).train()
        params = [p for p in net.parameters() if p.requires_grad]
        opt = FusedClipSGD(params, lr=1e-3, momentum=0.99, nesterov=True, weight_decay=3e-5, max_norm=12.0)
        ts = TrainStep(net, opt, params, x.shape, tgt.shape, dev, graph=True, warmup=3)
        for _ in range(5):                                                            # eager warm-up, then the capture
            limited(4 * a.step_limit, lambda: (ts(x, tgt), torch.cuda.synchronize()))
        _, t_step = timed(lambda: ts(x, tgt))

        def iteration():
            xb, tb_ = next(tb)
            return ts(xb, tb_)
        loss, t_iter = timed(iteration)
        ms, mb, ml, mi = (statistics.median(t) for t in (t_step, t_tb, t_loader, t_iter))
        lines += [f"TrainStep ({a.model}, {ts.capture_mode}), its inputs copied in: {fmt(t_step)} = {a.batch / ms * 1e3:.1f} slices/s",
                  f"next(TrainBatches) + TrainStep in a loop: {fmt(t_iter)} = {a.batch / mi * 1e3:.1f} slices/s; loss {float(loss):.4f}",
                  f"share of a step: loader {100 * ml / ms:.1f} %, loader + augmentation {100 * mb / ms:.1f} %, "
                  f"loop over step alone {100 * (mi / ms - 1):+.1f} %"]
        record.update(step_ms=[round(t, 3) for t in t_step], iteration_ms=[round(t, 3) for t in t_iter], capture_mode=ts.capture_mode)
    lines.append(json.dumps(record))
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
