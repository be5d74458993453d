#!/usr/bin/env python
"""What ensembling costs, in two parts (synthetic data; no trained weights).

merge   M = 5 member probability volumes (K = 4 classes, D = 64 slices of 512 x 512; softmax of N(0, 2) logits), fp32 and fp16 members,
        to the uint8 label map on the host, three paths:
          a. fused: du_ensemble_merge (csrc/ensemble.hip) through ensemble.merge_probabilities + the copy of the uint8 volume;
          b. the same work as stock torch ops ON THE DEVICE: torch.stack(members).float().mean(0).argmax(0).to(uint8) + that copy;
          c. the reference's route: every member to the host, numpy `avg += p; avg /= M` and argmax there (ensemble.py:17-46 without the
             file reads and without its second softmax).
        `a_kernel` is du_ensemble_merge alone between two device events; bytes are counted from the shapes (M K 4 or 2 read, 1 written).

folds   F = 5 parameter sets of one network (dinounet_l, 512 x 512 windows in batches of 8, bf16; cases of D = 8 and D = 32 slices = 1 and
        4 window batches), label map on the device:
          a. inference.EnsemblePredictor.predict_segmentation: one backbone pass per window batch, F heads, one export pass;
          b. what the API offered before: F sequential export.predict_segmentation(..., return_probabilities=True) calls, each on a whole
             network (its own backbone pass), then torch.stack(probabilities).mean(0).argmax(0).
          c. one such call without probabilities: what one fold costs.
        All with graph=True (captured window forwards; the captures happen in the warm-up) and with graph=False.  Every predict call
        computes its Gaussian importance map on the host first; that set-up is timed on its own and reported, because b pays it F times.

    python tools/ensemble_bench.py [--part merge|folds|both] [--rounds 5] [--iters 3] [--out profiles/ensemble.txt]

The legs of a part alternate (a b c a b c ...) in one process on one device; a sample is the wall time of `iters` calls between two device
synchronisations (`--merge-iters` for the two merge legs that take about a millisecond a call) after `--warmup` untimed calls per leg; the figure per leg is the median over the rounds with min .. max."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("DINOUNET_ALLOW_RANDOM_BACKBONE", "1")   # synthetic benchmark: random-init weights of the named architecture


def alternate(legs, rounds, warmup, torch):
    """legs: (name, function, calls per sample)"""
    samples = {n: [] for n, _, _ in legs}
    for _, f, _ in legs:
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for n, f, iters in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                f()
            torch.cuda.synchronize()
            samples[n].append((time.perf_counter() - t0) * 1e3 / iters)
    return samples


class Lines(list):
    """the report: every line is printed as it is made (a long run shows where it is)"""

    def append(self, line):
        print(line, flush=True)
        super().append(line)


def report(tag, samples, lines):
    for n, v in samples.items():
        lines.append(f"[{tag}] {n}: {statistics.median(v):.3f} ms  [{min(v):.3f} .. {max(v):.3f}]")


def part_merge(a, torch, lines, record):
    import numpy as np
    from dinounet_amd import _lib, ensemble as ENS
    dev = torch.device("cuda", 0)
    M, K, D, H, W = a.members, a.classes, a.slices, a.size, a.size
    n = D * H * W
    g = torch.Generator().manual_seed(7)
    base = [torch.softmax(torch.randn((K, D, H, W), generator=g) * 2.0, 0) for _ in range(M)]
    lines.append(f"# merge: M = {M} members, K = {K}, D = {D}, {H} x {W}; {a.rounds} rounds a b c interleaved, {a.merge_iters} calls per sample "
                 f"(c: {a.iters}), {a.warmup} warm-up calls per leg; ms per call (uint8 label map on the host), median [min .. max]")
    for dtype, es in ((torch.float32, 4), (torch.float16, 2)):
        tag = "merge fp32" if es == 4 else "merge fp16"
        members = [m.to(dtype).to(dev) for m in base]

        def fused():
            return ENS.merge_probabilities(members).cpu()

        def stock_device():
            return torch.stack(members).float().mean(0).argmax(0).to(torch.uint8).cpu()

        def host_route():
            avg = None
            for m in members:
                p = m.cpu().numpy()
                if avg is None:
                    avg = p if p.dtype == np.float32 else p.astype(np.float32)
                else:
                    avg += p
            avg /= M
            return avg.argmax(0).astype(np.uint8)

        differ = float((fused() != stock_device()).float().mean())
        lines.append(f"[{tag}] share of voxels on which a and b differ (b: torch's mean, another summation): {differ:.2e}")
        # a and b take about a millisecond a call: a sample is --merge-iters of them, so that it is not the clock that is measured
        samples = alternate([("a_fused", fused, a.merge_iters), ("b_stock_torch_device", stock_device, a.merge_iters),
                             ("c_reference_route_host", host_route, a.iters)], a.rounds, a.warmup, torch)
        report(tag, samples, lines)
        # the kernel alone, device events; with and without the mean
        L = _lib.lib()
        table = torch.tensor([m.data_ptr() for m in members], dtype=torch.int64).to(dev)
        seg = torch.empty((D, H, W), dtype=torch.uint8, device=dev)
        mean = torch.empty((K, D, H, W), dtype=torch.float32, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        st = torch.cuda.current_stream().cuda_stream
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        record[tag] = {"samples_ms": {k: [round(s, 4) for s in v] for k, v in samples.items()}}
        for what, mean_ptr, bytes_per_voxel in (("labels", None, M * K * es + 1), ("labels + mean", mean.data_ptr(), M * K * es + 1 + 4 * K)):
            ktimes = []
            for i in range(a.warmup + 20):
                e0.record()
                _lib.check(L.du_ensemble_merge(table.data_ptr(), M, es, K, n, 0, 0, seg.data_ptr(), mean_ptr, flag.data_ptr(), st),
                           "du_ensemble_merge")
                e1.record()
                e1.synchronize()
                if i >= a.warmup:
                    ktimes.append(e0.elapsed_time(e1))
            kmed = statistics.median(ktimes)
            lines.append(f"[{tag}] a_kernel {what} (du_ensemble_merge alone, device events, 20 calls; {bytes_per_voxel} bytes per voxel): "
                         f"{kmed:.3f} ms  [{min(ktimes):.3f} .. {max(ktimes):.3f}] = {bytes_per_voxel * n / (kmed * 1e-3) / 1e12:.2f} TB/s")
            record[tag]["kernel_ms " + what] = [round(t, 4) for t in ktimes]
        del members, table, seg, mean


def part_folds(a, torch, lines, record):
    from dinounet_amd import export as EX
    from dinounet_amd import inference as INF
    from dinounet_amd.network_architecture import DinoUNet
    from dinounet_amd.plans import PLANS_2D
    dev = torch.device("cuda", 0)
    F, P, B = a.folds, a.patch, a.fold_batch
    torch.manual_seed(0)                                       # the random-init weights of the network
    net = DinoUNet.from_config(PLANS_2D, 3, a.classes, dinov3_pretrained_path=None, dinov3_model_name=a.model, precision=a.precision)
    net = net.to(dev).eval()
    trainable = sorted(n for n, p in net.named_parameters() if p.requires_grad)
    sets = []
    for f in range(F):
        g = torch.Generator().manual_seed(100 + f)
        sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
        for k in trainable:
            sd[k] += 0.05 * float(sd[k].abs().mean()) * torch.randn(sd[k].shape, generator=g).to(dev)
        for k in sd:
            if k.startswith("decoder.encoder."):
                sd[k] = sd["encoder." + k[len("decoder.encoder."):]]
        sets.append(sd)
    pred = INF.EnsemblePredictor(net, sets)
    del sets
    # what every predict call pays on the host before its first window: the Gaussian importance map (scipy, once per call)
    gtimes = []
    for _ in range(5):
        t0 = time.perf_counter()
        INF.compute_gaussian((P, P), sigma_scale=1.0 / 8, value_scaling_factor=10, device=dev)
        torch.cuda.synchronize()
        gtimes.append((time.perf_counter() - t0) * 1e3)
    lines.append(f"# folds: {a.model} {a.precision}, F = {F} parameter sets, {P} x {P} windows in batches of {B}; {a.rounds} rounds a b c "
                 f"interleaved, {a.iters} calls per sample, {a.warmup} warm-up calls per leg; ms per case (label map on the device), median "
                 f"[min .. max].  Host set-up inside every predict call (compute_gaussian, scipy): {statistics.median(gtimes):.1f} ms")
    for D in a.fold_slices:
        data = torch.randn((3, D, P, P), generator=torch.Generator().manual_seed(3)).to(dev)
        for graph in (True, False):
            kw = dict(tile_step_size=0.5, use_gaussian=True, batch_size=B, graph=graph)

            def shared():
                return pred.predict_segmentation(data, (P, P), **kw)

            def sequential():
                probs = [EX.predict_segmentation(rep, data, (P, P), return_probabilities=True, **kw)[1] for rep in pred.nets]
                return torch.stack(probs).mean(0).argmax(0).to(torch.uint8)

            def one_fold():
                return EX.predict_segmentation(pred.nets[0], data, (P, P), **kw)

            tag = f"folds D={D} graph={graph}"
            differ = float((shared() != sequential()).float().mean())
            lines.append(f"[{tag}] {-(-D // B)} window batches; share of voxels on which a and b differ (a: mean of logits, b: mean of "
                         f"probabilities -- two ensembles, not two roundings): {differ:.2e}")
            samples = alternate([("a_shared_backbone", shared, a.iters), ("b_sequential_predict_segmentation", sequential, a.iters),
                                 ("c_one_fold_predict_segmentation", one_fold, a.iters)], a.rounds, a.warmup, torch)
            report(tag, samples, lines)
            record[tag] = {"samples_ms": {k: [round(s, 4) for s in v] for k, v in samples.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="both", choices=["merge", "folds", "both"])
    ap.add_argument("--members", type=int, default=5)
    ap.add_argument("--classes", type=int, default=4)
    ap.add_argument("--slices", type=int, default=64)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--model", default="dinounet_l")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--patch", type=int, default=512)
    ap.add_argument("--fold-slices", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--fold-batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--merge-iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ensemble_bench needs the GPU: no timing is taken on the host")
    torch.set_num_threads(16)
    lines, record = Lines(), {}
    if a.part in ("merge", "both"):
        part_merge(a, torch, lines, record)
    if a.part in ("folds", "both"):
        part_folds(a, torch, lines, record)
    lines.append(json.dumps(record))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
