#!/usr/bin/env python
"""What the export tail costs: window accumulators -> uint8 label map on the host, K = 4 heads, D = 64 slices of 512 x 512, synthetic
accumulators (N(0, 2) logits; no network, no data), three variants

  plain      no resampling, softmax heads
  resample   in-plane resampling to 768 x 640, softmax heads
  regions    no resampling, 4 region heads with an unsorted regions_class_order

and three paths per variant

  a. fused: du_export_seg (csrc/export.hip) on the accumulators + the copy of the uint8 volume to the host
     (export.logits_to_segmentation(...).cpu());
  b. the same label map from the kernels inference.predict_sliding_window_logits runs today plus stock torch ON THE DEVICE:
     du_window_normalize, the isfinite check (abs().max() read back), the un-padding slice, F.interpolate(bilinear,
     align_corners=False) where resampling, argmax + cast / the threshold loop, paste into a zero volume, the uint8 copy to the host;
  c. the reference's route: normalise + isfinite as in b, all K fp32 planes to the host, torch softmax + argmax / sigmoid + threshold loop
     there on 16 threads (export_prediction.py:36-48).  Its float64 skimage resampling on the host is NOT run: for `resample`, c is a
     lower bound of the reference's cost and labels the un-resampled volume.

    python tools/export_bench.py [--rounds 5] [--iters 5] [--out profiles/export_tail.txt]

The legs alternate (a b c a b c ...) in one process on one device; a sample is the wall time of `iters` calls, each ending with its result
on the host, between two device synchronisations, after `--warmup` untimed calls per leg; the figure per leg is the median over the
rounds, with min .. max.  The timed accumulators hold n_predictions = 1 so that b's in-place normalisation leaves them unchanged from call
to call (no kernel's time depends on the values); agreement of a and b is checked once beforehand on accumulators with a real
n_predictions map.  `a_kernel` is du_export_seg alone between two device events.  Bytes per voxel are counted from the shapes (unique bytes
each pass has to move, caches ideal), per voxel of the source window."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", type=int, default=4)
    ap.add_argument("--slices", type=int, default=64)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--resample-to", type=int, nargs=2, default=(768, 640))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from dinounet_amd import _lib, export as EX
    if not torch.cuda.is_available():
        raise SystemExit("export_bench needs the GPU: no timing is taken on the host")
    torch.set_num_threads(16)
    dev = torch.device("cuda", 0)
    K, D, H, W = a.classes, a.slices, a.size, a.size
    Ho, Wo = a.resample_to
    L = _lib.lib()
    g = torch.Generator().manual_seed(7)
    logits = (torch.randn((K, D, H, W), generator=g) * 2.0).to(dev)
    order = [3, 1, 4, 2][:K] if K <= 4 else list(range(K, 0, -1))
    variants = {"plain": (None, (H, W)), "resample": (None, (Ho, Wo)), "regions": (order, (H, W))}

    def props(out_hw):
        return {"shape_before_cropping": [D, *out_hw], "bbox_used_for_cropping": [[0, D], [0, out_hw[0]], [0, out_hw[1]]],
                "shape_after_cropping_and_before_resampling": [D, *out_hw]}

    def fused(sums, npred, order, out_hw):
        return EX.logits_to_segmentation(sums, npred, regions_class_order=order, properties=props(out_hw))

    def stock_device(sums, npred, order, out_hw):
        st = torch.cuda.current_stream().cuda_stream
        _lib.check(L.du_window_normalize(sums.data_ptr(), npred.data_ptr(), K, npred.numel(), st), "du_window_normalize")
        if not torch.isfinite(sums.abs().max()).item():
            raise RuntimeError("Encountered inf in predicted array")
        x = sums[:, :, 0:H, 0:W]
        if tuple(out_hw) != (H, W):
            x = F.interpolate(x, size=out_hw, mode="bilinear", align_corners=False)        # (K, D, H, W): K as batch, D as channels
        if order is None:
            lab = x.argmax(0).to(torch.uint8)
        else:
            lab = torch.zeros(x.shape[1:], dtype=torch.uint8, device=x.device)
            for i, c in enumerate(order):
                lab[x[i] > 0] = c
        out = torch.zeros((D, *out_hw), dtype=torch.uint8, device=x.device)
        out[:, :out_hw[0], :out_hw[1]] = lab
        return out

    def reference_route(sums, npred, order, out_hw):
        st = torch.cuda.current_stream().cuda_stream
        _lib.check(L.du_window_normalize(sums.data_ptr(), npred.data_ptr(), K, npred.numel(), st), "du_window_normalize")
        if not torch.isfinite(sums.abs().max()).item():
            raise RuntimeError("Encountered inf in predicted array")
        x = sums[:, :, 0:H, 0:W].cpu()
        if order is None:
            lab = torch.softmax(x, 0).argmax(0).to(torch.uint8)
        else:
            p = torch.sigmoid(x)
            lab = torch.zeros(x.shape[1:], dtype=torch.uint8)
            for i, c in enumerate(order):
                lab[p[i] > 0.5] = c
        out = torch.zeros((D, H, W), dtype=torch.uint8)
        out[:] = lab
        return out

    # bytes per source voxel, from the shapes: reads + writes every pass needs when each byte moves once
    def budget(order, out_hw):
        r = out_hw[0] * out_hw[1] / (H * W)
        res = tuple(out_hw) != (H, W)
        fused_b = 4 * K + (4 if res else 0) + r
        stock = (4 * K + 4 + 4 * K) + (4 * K + 4 * K + 4 * K)                  # normalise (in place); abs (read, write) + max (read)
        if res:
            stock += 4 * K + 4 * K * r                                          # interpolate: read the window, write the resampled planes
        if order is None:
            stock += 4 * K * r + 8 * r + 8 * r + r                              # argmax (int64 out), cast
        else:
            stock += r + K * (4 * r + r + r)                                    # zeros; per region: compare (read fp32, write mask), masked store
        stock += r + r + r                                                       # zero volume, paste (read, write)
        return fused_b, stock

    # a and b agree (real n_predictions map; fresh accumulators for each, b normalises in place)
    npred_real = (torch.rand((D, H, W), generator=g) * 30.0 + 0.5).to(dev)
    agree = {}
    for name, (order_v, out_hw) in variants.items():
        sums = logits * npred_real
        got = fused(sums, npred_real, order_v, out_hw).cpu()
        want = stock_device(sums.clone(), npred_real, order_v, out_hw).cpu()
        agree[name] = float((got != want).float().mean())
    del npred_real, sums

    ones = torch.ones((D, H, W), device=dev)
    lines = [f"# export tail, K = {K}, D = {D}, {H} x {W}; resample to {Ho} x {Wo}; {a.rounds} rounds a b c interleaved, {a.iters} calls per "
             f"sample, {a.warmup} warm-up calls per leg; ms per call (result on the host), median [min .. max]",
             "# share of voxels on which a and b differ (b: fp32 scale factor in F.interpolate, reciprocal-multiply normalisation): "
             + ", ".join(f"{n} {v:.2e}" for n, v in agree.items())]
    record = {}
    for name, (order_v, out_hw) in variants.items():
        legs = [("a_fused", lambda: fused(logits, ones, order_v, out_hw).cpu()),
                ("b_stock_torch_device", lambda: stock_device(logits, ones, order_v, out_hw).cpu()),
                ("c_reference_route_host", lambda: reference_route(logits, ones, order_v, out_hw))]
        samples = {n: [] for n, _ in legs}
        for _, f in legs:
            for _ in range(a.warmup):
                f()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for n, f in legs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.iters):
                    f()
                torch.cuda.synchronize()
                samples[n].append((time.perf_counter() - t0) * 1e3 / a.iters)
        # the kernel alone, device events
        seg = torch.empty((D, *out_hw), dtype=torch.uint8, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        packed = 0 if order_v is None else sum(c << (8 * i) for i, c in enumerate(order_v))
        st = torch.cuda.current_stream().cuda_stream
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ktimes = []
        for i in range(a.warmup + 20):
            e0.record()
            _lib.check(L.du_export_seg(logits.data_ptr(), ones.data_ptr(), seg.data_ptr(), None, flag.data_ptr(), K, D, H, W, 0, 0, H, W,
                                       out_hw[0], out_hw[1], D, out_hw[0], out_hw[1], 0, 0, 0, 0 if order_v is None else 1, packed, st),
                       "du_export_seg")
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                ktimes.append(e0.elapsed_time(e1))
        fb, sb = budget(order_v, out_hw)
        nvox = D * H * W
        kmed = statistics.median(ktimes)
        lines.append(f"[{name}] bytes per source voxel: a {fb:.1f}, b {sb:.1f}")
        for n, _ in legs:
            v = samples[n]
            lines.append(f"[{name}] {n}: {statistics.median(v):.3f} ms  [{min(v):.3f} .. {max(v):.3f}]")
        lines.append(f"[{name}] a_kernel (du_export_seg alone, device events, 20 calls): {kmed:.3f} ms  [{min(ktimes):.3f} .. {max(ktimes):.3f}]"
                     f" = {fb * nvox / (kmed * 1e-3) / 1e12:.2f} TB/s of the byte budget")
        record[name] = {"samples_ms": {n: [round(s, 4) for s in v] for n, v in samples.items()}, "kernel_ms": [round(t, 4) for t in ktimes]}
    lines.append(json.dumps(record))
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
