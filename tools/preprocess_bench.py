#!/usr/bin/env python
"""What preprocessing a raw case costs, on the device and on the host: two synthetic cases, each through preprocessing.run_case

  natural  (3, 1, 512, 512): an RGB-valued image inside a zero frame, ZScoreNormalization per channel, spacing (999, 1, 1) -> (1.25, 1.25),
           i.e. 0.8 x in-plane
  ct       (1, 128, 512, 512): CT-like values inside a cylindrical field of view, zero outside it, a few zero pockets inside (the holes
           binary_fill_holes closes), CTNormalization, spacing (2.5, 0.8, 0.8) -> (2.5, 1.0, 1.0): 0.8 x in-plane, resized per slice
           (2.5 / 0.8 > ANISO_THRESHOLD), as the reference predictor does before the first window is predicted

  a. device: run_case on the raw array that already sits on the GPU (csrc/preprocess.hip), and each of its stages alone;
  b. host:   the numpy / scipy restatement (the same functions on CPU tensors) on this box's cores.

    python tools/preprocess_bench.py [--calls 10] [--host-calls 3] [--out profiles/preprocessing.txt]
    rocprofv3 --kernel-trace --stats -d pre_trace -o pre --output-format csv -- python tools/preprocess_bench.py --device-only --calls 3

One process.  Every device step runs under its own time limit: a watchdog thread (faulthandler.dump_traceback_later(limit, exit=True))
ends the process if a step does not come back, so nothing more is started on the GPU after a hang.  Leg a: the median of `--calls` timed
calls after `--warmup` untimed ones, each between two device synchronisations, allocations included.  Leg b: the median of
`--host-calls` calls after one untimed call."""
import argparse
import faulthandler
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def natural_case(size, seed):
    import numpy as np
    rng = np.random.RandomState(seed)
    img = rng.randint(1, 256, size=(3, 1, size, size)).astype(np.float32)
    f = size // 16
    img[:, :, :f], img[:, :, -f:], img[:, :, :, :f], img[:, :, :, -f:] = 0, 0, 0, 0
    return img, dict(transpose_forward=(0, 1, 2), spacing=[1.25, 1.25], normalization_schemes=["ZScoreNormalization"] * 3,
                     use_mask_for_norm=[False] * 3, foreground_intensity_properties_per_channel=None), (999.0, 1.0, 1.0)


def ct_case(slices, size, seed):
    import numpy as np
    rng = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.arange(size, dtype=np.float32), np.arange(size, dtype=np.float32), indexing="ij")
    fov = (yy - size / 2) ** 2 + (xx - size / 2) ** 2 <= (0.47 * size) ** 2
    img = np.round(rng.randn(1, slices, size, size) * 200 - 300).astype(np.float32)
    img[img == 0] = 1
    img[:, :, ~fov] = 0
    img[0][rng.random_sample((slices, size, size)) < 0.01] = 0
    ip = {"0": {"mean": -120.0, "std": 210.0, "percentile_00_5": -990.0, "percentile_99_5": 420.0}}
    return img, dict(transpose_forward=(0, 1, 2), spacing=[2.5, 1.0, 1.0], normalization_schemes=["CTNormalization"],
                     use_mask_for_norm=[False], foreground_intensity_properties_per_channel=ip), (2.5, 0.8, 0.8)


def limited(limit, fn):
    """fn() under a time limit of its own: the watchdog ends the process if it does not return"""
    faulthandler.dump_traceback_later(limit, exit=True)
    try:
        return fn()
    finally:
        faulthandler.cancel_dump_traceback_later()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slices", type=int, default=128)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--host-calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-limit", type=float, default=60.0, help="seconds every device step may take")
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from dinounet_amd import preprocessing as P
    if not torch.cuda.is_available():
        raise SystemExit("preprocess_bench needs the GPU: no timing is taken without it")
    torch.set_num_threads(16)
    dev = torch.device("cuda", 0)

    def timed(fn, calls, warmup):
        def once():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            return out, (time.perf_counter() - t0) * 1e3
        for _ in range(warmup):
            out, _ = limited(a.step_limit, once)
        times = []
        for _ in range(calls):
            out, t = limited(a.step_limit, once)
            times.append(t)
        return out, times

    def fmt(times):
        return f"{statistics.median(times):.3f} ms  [{min(times):.3f} .. {max(times):.3f}]"

    lines, record = [f"# preprocessing.run_case, ms per call, median [min .. max]; device: {a.calls} calls after {a.warmup}"], {}
    for name, (img, kw, spacing) in (("natural", natural_case(a.size, 1)), ("ct", ct_case(a.slices, a.size, 2))):
        raw = torch.from_numpy(img)
        raw_d = limited(a.step_limit, lambda: raw.to(dev))
        props_d = {"spacing": spacing}
        (got, got_seg), t_all = timed(lambda: P.run_case(raw_d, None, props_d, **kw), a.calls, a.warmup)
        # the stages alone, on the device
        (crop, crop_seg, _), t_crop = timed(lambda: P.crop_to_nonzero(raw_d), a.calls, a.warmup)
        _, t_norm = timed(lambda: P.normalize(crop.clone(), crop_seg, kw["normalization_schemes"], kw["use_mask_for_norm"],
                                              kw["foreground_intensity_properties_per_channel"]), a.calls, a.warmup)
        _, t_clone = timed(lambda: crop.clone(), a.calls, a.warmup)
        sp = [spacing[0]] + kw["spacing"][-2:]
        new_shape = P.compute_new_shape(crop.shape[1:], spacing, sp)
        _, t_img = timed(lambda: P.resample_data_or_seg_to_shape(crop, new_shape, spacing, sp), a.calls, a.warmup)
        _, t_seg = timed(lambda: P.resample_data_or_seg_to_shape(crop_seg, new_shape, spacing, sp, is_seg=True, order=1), a.calls, a.warmup)
        nvox = raw[0].numel()
        ma = statistics.median(t_all)
        lines += [f"## {name}: raw {tuple(raw.shape)} {raw.dtype}, bbox {props_d['bbox_used_for_cropping']}, out {tuple(got.shape)}",
                  f"a_device run_case: {fmt(t_all)} = {nvox / (ma * 1e-3) / 1e9:.2f} G raw voxels / s per channel volume",
                  f"a_device   crop_to_nonzero (mask, fill, bbox read-back, crop): {fmt(t_crop)}",
                  f"a_device   normalize (statistics and in-place pass; with a clone of {statistics.median(t_clone):.3f} ms): {fmt(t_norm)}",
                  f"a_device   resample image, order 3 (statistics for the clip, prefilter and taps): {fmt(t_img)}",
                  f"a_device   resample segmentation, order 1: {fmt(t_seg)}"]
        record[name] = {"device_ms": [round(t, 3) for t in t_all], "crop_ms": round(statistics.median(t_crop), 3),
                        "normalize_ms": round(statistics.median(t_norm), 3), "resample_image_ms": round(statistics.median(t_img), 3),
                        "resample_seg_ms": round(statistics.median(t_seg), 3)}
        if not a.device_only:
            t_host = []
            for i in range(1 + a.host_calls):                   # the first call is not timed
                props_h = {"spacing": spacing}
                t0 = time.perf_counter()
                want, want_seg = P.run_case(raw, None, props_h, **kw)
                if i > 0:
                    t_host.append((time.perf_counter() - t0) * 1e3)
            mb = statistics.median(t_host)
            err = float((got.cpu().double() - want.double()).abs().max())
            lines += [f"b_host numpy / scipy restatement ({a.host_calls} calls after 1, {torch.get_num_threads()} threads allowed): {mb:.1f} ms  "
                      f"[{min(t_host):.1f} .. {max(t_host):.1f}]",
                      f"ratio b / a: {mb / ma:.1f}",
                      f"a against b: max |image difference| {err:.3e} (max |image| {float(want.abs().max()):.3f}); segmentations differ at "
                      f"{int((got_seg.cpu() != want_seg).sum())} voxels; properties equal: {props_h == props_d}"]
            record[name]["host_ms"] = [round(t, 1) for t in t_host]
        del raw_d, got, got_seg, crop, crop_seg
    lines.append(json.dumps(record))
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
