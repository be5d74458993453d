#!/usr/bin/env python
"""What the surface metrics cost: HD95 / ASD of one synthetic case, D = 128 slices of 512 x 512 with 4 labels (ellipsoid blobs; the
prediction is a shifted copy with a few small false positives and holes), spacing (2.5, 0.75, 0.75), two legs

  a. device: export.surface_metrics on the label maps that already sit on the GPU (csrc/surface.hip: border bits, then per field an x,
     a y and a z pass, torch.sort on the compacted distances, two synchronisations);
  b. host:   the scipy / numpy restatement of medpy.metric.hd95 / asd (export.surface_metrics on CPU tensors) on this box's cores: per
     label two binary_erosion and two distance_transform_edt over the whole volume and one percentile (medpy's hd95 and asd each run
     their own erosions and transforms, three transforms per label: the restatement is the cheaper form of the reference's method).

    python tools/surface_bench.py [--calls 10] [--host-calls 3] [--out profiles/surface_metrics.txt]
    rocprofv3 --kernel-trace --stats -d surface_trace -o surface --output-format csv -- python tools/surface_bench.py --device-only --calls 3

Leg a: the median of `--calls` timed calls after `--warmup` untimed ones, each between two device synchronisations.  Leg b: the median of
`--host-calls` calls.  `passes`: each kernel family alone between device events for ONE field (du_surface_field on a border bit set),
with the bytes every pass has to move counted from the shapes, per voxel: border 2 + 2 (two label maps in, bit sets out; neighbours from
cache), x 2 + 2, y 2 + 4, z 4 + 8 (dense field) or 4 + 2 (gather: the bit sets instead of the field)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic_case(D, H, W, n_labels, seed):
    import numpy as np
    import torch
    rng = np.random.RandomState(seed)
    zz, yy, xx = np.meshgrid(np.arange(D, dtype=np.float32), np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    ref = np.zeros((D, H, W), dtype=np.uint8)
    for i in range(3 * n_labels):
        c = (rng.uniform(0, D), rng.uniform(0, H), rng.uniform(0, W))
        r = (D * rng.uniform(0.1, 0.3), H * rng.uniform(0.05, 0.2), W * rng.uniform(0.05, 0.2))
        ref[((zz - c[0]) / r[0]) ** 2 + ((yy - c[1]) / r[1]) ** 2 + ((xx - c[2]) / r[2]) ** 2 <= 1.0] = 1 + i % n_labels
    pred = np.roll(ref, (1, 3, -2), axis=(0, 1, 2)).copy()
    for i in range(2 * n_labels):                                                     # small false positives and holes
        c = (rng.uniform(0, D), rng.uniform(0, H), rng.uniform(0, W))
        r = (max(1.0, D * 0.02), H * rng.uniform(0.01, 0.03), W * rng.uniform(0.01, 0.03))
        pred[((zz - c[0]) / r[0]) ** 2 + ((yy - c[1]) / r[1]) ** 2 + ((xx - c[2]) / r[2]) ** 2 <= 1.0] = i % (n_labels + 1)
    return torch.from_numpy(pred), torch.from_numpy(ref)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slices", type=int, default=128)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--labels", type=int, default=4)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--host-calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from dinounet_amd import _lib, export as EX
    if not torch.cuda.is_available():
        raise SystemExit("surface_bench needs the GPU: no timing is taken without it")
    torch.set_num_threads(16)
    dev = torch.device("cuda", 0)
    D, H, W = a.slices, a.size, a.size
    spacing = (2.5, 0.75, 0.75)
    lors = list(range(1, a.labels + 1))
    pred, ref = synthetic_case(D, H, W, a.labels, 3)
    pred_d, ref_d = pred.to(dev), ref.to(dev)
    nvox = D * H * W

    def device_call():
        return EX.surface_metrics(pred_d, ref_d, lors, spacing)

    for _ in range(a.warmup):
        got = device_call()
    times_a = []
    for _ in range(a.calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = device_call()
        torch.cuda.synchronize()
        times_a.append((time.perf_counter() - t0) * 1e3)

    # one field, pass by pass, device events: the border kernel, then du_surface_field = x + y + z (dense field)
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t_border, t_field = [], []
    ws, ws_elems = EX._surface_ws(ref_d.shape, dev)
    field = torch.empty((D, H, W), dtype=torch.float64, device=dev)
    masks = [EX._region_mask_bits(r) for r in lors]
    for i in range(a.warmup + a.calls):
        e0.record()
        bits, _ = EX._surface_border_hip(pred_d, ref_d, masks)
        e1.record()
        e1.synchronize()
        tb = e0.elapsed_time(e1)
        e0.record()
        _lib.check(L.du_surface_field(bits.data_ptr(), field.data_ptr(), D, H, W, 8, spacing[0], spacing[1], spacing[2], ws.data_ptr(),
                                      ws_elems, st), "du_surface_field")
        e1.record()
        e1.synchronize()
        if i >= a.warmup:
            t_border.append(tb)
            t_field.append(e0.elapsed_time(e1))
    del field

    lines = [f"# surface metrics (HD95 / ASD), {a.labels} labels, D = {D}, {H} x {W}, spacing {spacing}; ms per call, median [min .. max]",
             "# surface voxels pred / ref per label: " + ", ".join(f"{r}: {got[r]['n_surface_pred']} / {got[r]['n_surface_ref']}" for r in lors)]
    lines.append(f"a_device surface_metrics ({a.calls} calls after {a.warmup}): {statistics.median(times_a):.2f} ms  "
                 f"[{min(times_a):.2f} .. {max(times_a):.2f}]")
    kb, kf = statistics.median(t_border), statistics.median(t_field)
    lines.append(f"passes: border kernel + counts ({a.labels} regions): {kb:.3f} ms = {4 * nvox / (kb * 1e-3) / 1e12:.2f} TB/s of 4 B / voxel")
    lines.append(f"passes: one dense field (x + y + z, du_surface_field): {kf:.3f} ms = {22 * nvox / (kf * 1e-3) / 1e12:.2f} TB/s of "
                 f"22 B / voxel (x 2 + 2, y 2 + 4, z 4 + 8); the volume itself is {nvox / 1e6:.1f} M voxels")
    record = {"device_ms": [round(t, 3) for t in times_a], "border_ms": [round(t, 4) for t in t_border], "field_ms": [round(t, 4) for t in t_field]}
    if not a.device_only:
        times_b = []
        for _ in range(a.host_calls):
            t0 = time.perf_counter()
            want = EX.surface_metrics(pred, ref, lors, spacing)
            times_b.append((time.perf_counter() - t0) * 1e3)
        mb, ma = statistics.median(times_b), statistics.median(times_a)
        lines.append(f"b_host scipy restatement ({a.host_calls} calls, {torch.get_num_threads()} threads allowed; scipy.ndimage runs on one): "
                     f"{mb:.1f} ms  [{min(times_b):.1f} .. {max(times_b):.1f}]")
        lines.append(f"ratio b / a: {mb / ma:.1f}")
        worst = max(abs(got[r][k] - want[r][k]) / max(abs(want[r][k]), 1e-300) for r in lors for k in ("HD95", "ASD"))
        lines.append("a against b: " + ", ".join(f"{r}: HD95 {got[r]['HD95']:.6f} / {want[r]['HD95']:.6f}, ASD {got[r]['ASD']:.6f} / "
                                                 f"{want[r]['ASD']:.6f}" for r in lors) + f"; largest relative difference {worst:.2e}")
        record["host_ms"] = [round(t, 2) for t in times_b]
    lines.append(json.dumps(record))
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
