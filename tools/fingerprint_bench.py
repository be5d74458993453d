#!/usr/bin/env python
"""What the dataset fingerprint costs on the device next to its numpy restatement on the same box (dinounet_amd.fingerprint).

  case      collect_foreground_intensities on one CT-like case (1, 128, 512, 512), about 5 % foreground in a few blobs, integer HU values,
            num_samples = 10^6: the moments sweep, the read-back, four histogram sweeps, the member counts and 10^6 selects
  dataset   intensity_statistics on (1, 10^8) samples, every element a member: two moment sweeps and four histogram sweeps

    python tools/fingerprint_bench.py [--calls 10] [--warmup 2] [--out profiles/fingerprint.txt] [--kernel-stats CASE.csv DATASET.csv]
    python tools/fingerprint_bench.py --once --only case|dataset     # two calls of the whole function, for a profiler run of its own

One process.  A device call is timed on the host clock between two synchronisations, so its allocations, uploads and read-backs are
inside; the three operations are also timed one by one.  The median of `--calls` timed calls after `--warmup` untimed ones; the host
figure is the restatement on CPU tensors, median of 3 after 1.  Beside every sweep stand its bytes and what they take at 8 TB/s.  Every
device step runs under its own time limit: a watchdog thread (faulthandler.dump_traceback_later(limit, exit=True)) ends the process if a
step does not come back, so nothing more is started on the GPU after a hang.  No threshold is set: nobody had measured these.
--kernel-stats appends the fingerprint kernels' rows of the kernel_stats.csv of two `rocprofv3 --kernel-trace --stats -- python
tools/fingerprint_bench.py --once --only ...` runs, which are runs of their own."""
import argparse
import csv
import faulthandler
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8e12                                                                           # bytes per second


def ct_case(shape, seed=0):
    """(img (1, D, H, W) fp32 integer HU values, seg (1, D, H, W) int16 with about 5 % foreground in three balls)"""
    import numpy as np
    rng = np.random.RandomState(seed)
    D, H, W = shape
    img = rng.randint(-1024, 3072, (1, D, H, W)).astype(np.float32)
    seg = np.zeros((1, D, H, W), np.int16)
    zz, yy, xx = np.ogrid[0:D, 0:H, 0:W]
    r = (0.05 * D * H * W / (2 * np.pi)) ** (1 / 3)                                   # three ellipsoids of half height: 3 (4/3) pi r^3 / 2
    for k, (cz, cy, cx) in enumerate(((0.5, 0.3, 0.3), (0.4, 0.7, 0.6), (0.6, 0.5, 0.8))):
        ball = ((zz - cz * D) * 2.0) ** 2 + (yy - cy * H) ** 2 + (xx - cx * W) ** 2 <= r * r
        seg[0][ball] = k + 1
    img[0][seg[0] > 0] += 40                                                          # the organ is a little brighter: still integers
    return img, seg


def limited(limit, fn):
    """fn() under a time limit of its own: the watchdog ends the process if it does not return"""
    faulthandler.dump_traceback_later(limit, exit=True)
    try:
        return fn()
    finally:
        faulthandler.cancel_dump_traceback_later()


def kernel_rows(path):
    """the rows of a rocprofv3 kernel_stats.csv that belong to csrc/fingerprint.hip"""
    rows = []
    for r in csv.DictReader(open(path)):
        name = r.get("Name", "")
        if any(k in name for k in ("mom_partial", "mom_final", "os_init", "os_hist", "os_pick", "sm_count", "sm_scan", "sm_select", "sm_gather")):
            short = name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
            rows.append(f"  {short:<32} calls {r.get('Calls', '?'):>4}  total {float(r.get('TotalDurationNs', 0)) / 1e3:10.1f} us  "
                        f"average {float(r.get('AverageNs', 0)) / 1e3:9.1f} us  [{float(r.get('MinNs', 0)) / 1e3:.1f} .. "
                        f"{float(r.get('MaxNs', 0)) / 1e3:.1f}]")
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=(128, 512, 512))
    ap.add_argument("--samples", type=int, default=10 ** 6)
    ap.add_argument("--dataset", type=int, default=10 ** 8)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-limit", type=float, default=120.0, help="seconds every device step may take")
    ap.add_argument("--once", action="store_true", help="one warm call of each case and no host figure: what a profiler run wraps")
    ap.add_argument("--only", choices=("case", "dataset"), default=None, help="one of the two cases: a profiler run per case keeps them apart")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--kernel-stats", nargs=2, default=None, metavar=("CASE_CSV", "DATASET_CSV"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.once:
        a.calls, a.warmup, a.no_host = 1, 1, True
    import numpy as np
    import torch
    from dinounet_amd import fingerprint as FP
    if not torch.cuda.is_available():
        raise SystemExit("fingerprint_bench needs the GPU: no timing is taken without it")
    dev = torch.device("cuda", 0)

    def device_ms(fn, calls=a.calls, warmup=a.warmup):
        out = None

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

    def host_ms(fn, calls=3, warmup=1):
        times = []
        for i in range(warmup + calls):
            t0 = time.perf_counter()
            out = fn()
            if i >= warmup:
                times.append((time.perf_counter() - t0) * 1e3)
        return out, times

    def fmt(times):
        if not times:
            return "not timed"
        return f"{statistics.median(times):.3f} ms  [{min(times):.3f} .. {max(times):.3f}]"

    def floor(nbytes):
        return f"{nbytes / 1e6:.0f} MB = {nbytes / PEAK * 1e6:.1f} us at 8 TB/s"

    lines = [f"# dataset fingerprint on the device, ms per call on the host clock between two synchronisations, median [min .. max] of "
             f"{a.calls} calls after {a.warmup}; host: the numpy restatement on the same box, median of 3 after 1"]
    record = {}

    if a.only != "dataset":                                                           # one case
        img, seg = ct_case(tuple(a.shape))
        n = seg.size
        n_fg = int((seg > 0).sum())
        it, st = torch.from_numpy(img), torch.from_numpy(seg)
        idev, sdev = limited(a.step_limit, lambda: (it.to(dev), st.to(dev)))
        (inten, stats), t_case = device_ms(lambda: FP.collect_foreground_intensities(sdev, idev, num_samples=a.samples))
        flat, sflat = idev.reshape(1, -1), sdev.reshape(-1)
        ranks6 = torch.tensor([FP._rank_plan(n_fg)[0]], dtype=torch.int64, device=dev)
        draws = torch.from_numpy(np.random.RandomState(1234).randint(0, n_fg, (1, a.samples)).astype(np.int64)).to(dev)
        parts = 0 if a.once else a.calls                                              # --once: the whole function only
        _, t_mom = device_ms(lambda: FP.foreground_moments(flat, sflat), parts, min(parts, a.warmup))
        _, t_ord = device_ms(lambda: FP.foreground_order_stats(flat, sflat, ranks6), parts, min(parts, a.warmup))
        _, t_smp = device_ms(lambda: FP.foreground_sample(flat, sflat, draws), parts, min(parts, a.warmup))
        lines += [f"case {tuple(img.shape)}: {n / 1e6:.1f} M voxels, {n_fg} foreground ({100 * n_fg / n:.1f} %), num_samples {a.samples}",
                  f"  collect_foreground_intensities, device: {fmt(t_case)}",
                  f"    du_fp_moments       (1 sweep over img and seg, {floor(6 * n)}): {fmt(t_mom)}",
                  f"    du_fp_order_stats   (4 sweeps over img and seg, each {floor(6 * n)}; 6 ranks): {fmt(t_ord)}",
                  f"    du_fp_sample        (1 sweep over seg, {floor(2 * n)}, then {a.samples} selects): {fmt(t_smp)}"]
        if 6 * n < 256 * 2 ** 20:
            lines.append(f"    note: img + seg = {6 * n / 1e6:.0f} MB fit the 256 MiB Infinity Cache and are swept again and again here: the case's "
                         f"kernel times are those of a cache-resident working set, not HBM streaming times")
        record.update(case_ms=[round(t, 3) for t in t_case], case_moments_ms=[round(t, 3) for t in t_mom],
                      case_order_ms=[round(t, 3) for t in t_ord], case_sample_ms=[round(t, 3) for t in t_smp])
        if not a.no_host:
            (h_inten, h_stats), t_host = host_ms(lambda: FP.collect_foreground_intensities(st, it, num_samples=a.samples))
            same = torch.equal(h_inten.view(torch.int32), inten.cpu().view(torch.int32)) and h_stats == stats
            lines.append(f"  collect_foreground_intensities, host:   {fmt(t_host)}  = {statistics.median(t_host) / statistics.median(t_case):.1f} x; "
                         f"samples and statistics {'equal to the bit' if same else 'DIFFER'}")
            record.update(case_host_ms=[round(t, 3) for t in t_host], case_equal=same)
        del idev, sdev, flat, sflat, inten, draws

    if a.only != "case":                                                              # the dataset step: the concatenated samples of many such cases
        N = int(a.dataset)
        rng = np.random.RandomState(7)
        samples = torch.from_numpy(rng.randint(-1024, 3072, (1, N)).astype(np.float32))
        sdev = limited(a.step_limit, lambda: samples.to(dev))
        dstats, t_ds = device_ms(lambda: FP.intensity_statistics(sdev))
        rk = torch.tensor([FP._rank_plan(N)[0]], dtype=torch.int64, device=dev)
        parts = 0 if a.once else a.calls
        _, t_mom = device_ms(lambda: FP.foreground_moments(sdev, None, with_std=True), parts, min(parts, a.warmup))
        _, t_ord = device_ms(lambda: FP.foreground_order_stats(sdev, None, rk), parts, min(parts, a.warmup))
        lines += [f"dataset step on {tuple(samples.shape)} samples, every element a member",
                  f"  intensity_statistics, device: {fmt(t_ds)}",
                  f"    du_fp_moments x 2   (2 sweeps over img, each {floor(4 * N)}): {fmt(t_mom)}",
                  f"    du_fp_order_stats   (4 sweeps over img, each {floor(4 * N)}; 6 ranks): {fmt(t_ord)}"]
        record.update(dataset_ms=[round(t, 3) for t in t_ds], dataset_moments_ms=[round(t, 3) for t in t_mom],
                      dataset_order_ms=[round(t, 3) for t in t_ord])
        if not a.no_host:
            hstats, t_host = host_ms(lambda: FP.intensity_statistics(samples))
            same = all(hstats[0][k] == dstats[0][k] for k in ("median", "min", "max", "percentile_00_5", "percentile_99_5", "mean"))
            lines.append(f"  intensity_statistics, host:   {fmt(t_host)}  = {statistics.median(t_host) / statistics.median(t_ds):.1f} x; order "
                         f"statistics and mean {'equal to the bit' if same else 'DIFFER'}; std device - host {dstats[0]['std'] - hstats[0]['std']:.3e}")
            record.update(dataset_host_ms=[round(t, 3) for t in t_host], dataset_equal=same)
    if a.kernel_stats:
        for what, path in zip(("case", "dataset"), a.kernel_stats):
            lines.append(f"per kernel, {what}: a separate `rocprofv3 --kernel-trace --stats -- python tools/fingerprint_bench.py --once --only "
                         f"{what}` run = two calls of the whole function, one warm-up and one timed")
            lines += kernel_rows(path)
    lines.append(json.dumps(record))
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
