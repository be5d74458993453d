#!/usr/bin/env python
"""What "keep only the largest component" costs: one synthetic case, D = 128 slices of 512 x 512 with 4 labels (ellipsoid blobs plus a
few percent of single-voxel speckle, so there are many small components), the mask = the union of the 4 foreground labels, two legs

  a. device: postprocessing.remove_all_but_largest_component_from_segmentation on the label map that already sits on the GPU
     (csrc/cc.hip: tile, merge, flatten, select, stats, apply; no synchronisation of its own);
  b. host:   the scipy restatement (the same function on the CPU tensor: scipy.ndimage.label with the 3 x 3 x 3 structure, np.bincount,
     the tie rule) on this box's cores.

    python tools/postprocess_bench.py [--calls 10] [--host-calls 10] [--out profiles/postprocessing.txt]
    rocprofv3 --kernel-trace --stats -d pp_trace -o pp --output-format csv -- python tools/postprocess_bench.py --device-only --calls 3

Leg a: the median of `--calls` timed calls after `--warmup` untimed ones, each between two device synchronisations (the workspace
allocation of every call included).  Leg b: the median of `--host-calls` calls after the same number of untimed ones.  Per-kernel
times come from the separate rocprofv3 run; the bytes every phase has to move, per voxel: tile 1 + 8 (label map in, parent and size
out), merge 0 .. 4 (tile faces only), flatten 4 + 4 (+ the walk), select 4, apply 1 + 4 + 1."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic_case(D, H, W, n_labels, speckle, seed):
    import numpy as np
    import torch
    rng = np.random.RandomState(seed)
    zz, yy, xx = np.meshgrid(np.arange(D, dtype=np.float32), np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    seg = np.zeros((D, H, W), dtype=np.uint8)
    for i in range(3 * n_labels):
        c = (rng.uniform(0, D), rng.uniform(0, H), rng.uniform(0, W))
        r = (D * rng.uniform(0.1, 0.3), H * rng.uniform(0.05, 0.2), W * rng.uniform(0.05, 0.2))
        seg[((zz - c[0]) / r[0]) ** 2 + ((yy - c[1]) / r[1]) ** 2 + ((xx - c[2]) / r[2]) ** 2 <= 1.0] = 1 + i % n_labels
    del zz, yy, xx
    noise = rng.random_sample((D, H, W)) < speckle
    seg[noise] = rng.randint(1, n_labels + 1, size=int(noise.sum())).astype(np.uint8)
    return torch.from_numpy(seg)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slices", type=int, default=128)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--labels", type=int, default=4)
    ap.add_argument("--speckle", type=float, default=0.03)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--host-calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from dinounet_amd import postprocessing as PP
    if not torch.cuda.is_available():
        raise SystemExit("postprocess_bench needs the GPU: no timing is taken without it")
    torch.set_num_threads(16)
    dev = torch.device("cuda", 0)
    D, H, W = a.slices, a.size, a.size
    fg = list(range(1, a.labels + 1))
    seg = synthetic_case(D, H, W, a.labels, a.speckle, 3)
    seg_d = seg.to(dev)
    nvox = D * H * W
    remove = PP.remove_all_but_largest_component_from_segmentation

    for _ in range(a.warmup):
        got = remove(seg_d, fg)
    times_a = []
    for _ in range(a.calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = remove(seg_d, fg)
        torch.cuda.synchronize()
        times_a.append((time.perf_counter() - t0) * 1e3)
    _, stats = PP.component_ids(seg_d, fg)

    ma = statistics.median(times_a)
    lines = [f"# keep the largest component of the union of {a.labels} labels, D = {D}, {H} x {W}, speckle {a.speckle}; ms per call, median [min .. max]",
             f"# mask voxels {int((seg != 0).sum())} of {nvox}; components {stats['n_components']}, the largest {stats['largest_size']} voxels (id {stats['largest_id']})",
             f"a_device remove_all_but_largest_component_from_segmentation ({a.calls} calls after {a.warmup}): {ma:.3f} ms  "
             f"[{min(times_a):.3f} .. {max(times_a):.3f}] = {nvox / (ma * 1e-3) / 1e9:.1f} G voxels / s"]
    record = {"device_ms": [round(t, 3) for t in times_a]}
    if not a.device_only:
        times_b = []
        for _ in range(a.warmup):
            want = remove(seg, fg)
        for _ in range(a.host_calls):
            t0 = time.perf_counter()
            want = remove(seg, fg)
            times_b.append((time.perf_counter() - t0) * 1e3)
        mb = statistics.median(times_b)
        lines.append(f"b_host scipy restatement ({a.host_calls} calls after {a.warmup}, {torch.get_num_threads()} threads allowed; scipy.ndimage runs on one): "
                     f"{mb:.1f} ms  [{min(times_b):.1f} .. {max(times_b):.1f}]")
        lines.append(f"ratio b / a: {mb / ma:.1f}")
        lines.append(f"a against b: maps differ at {int((got.cpu() != want).sum())} voxels; {int((want != seg).sum())} voxels removed")
        record["host_ms"] = [round(t, 2) for t in times_b]
    lines.append(json.dumps(record))
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
