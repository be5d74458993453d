#!/usr/bin/env python
"""What batching windows across cases buys on a list of small 2-D cases: 64 seeded cases of (3, 1, 600, 450), 512 x 512 windows at step
0.5 (2 windows per case), window batch 12, the benchmark network (dinounet_l, bf16), captured forward (graph=True), two arms

  a. the per-case loop: inference.predict_segmentation case by case -- 64 forwards of 12 slots, 10 of them zero windows;
  b. the cases path:    inference.predict_cases_segmentation on the list -- the 128 windows in ceil(128 / 12) = 11 forwards.

    python tools/bench_predict_cases.py [--precision bf16|fp32] [--cases 64] [--reps 5] [--out profiles/predict_cases.txt]

Before any timing the two arms' label maps are compared case by case: every differing voxel must lie in the tie band of the single-case
logits (float64 top-two gap below 1e-5 * max|logit|, tests/test_gpu_export.py) and their share must be below 1e-4.  Then both arms are
warmed (captures, allocator) and alternate (a b a b ...) in one process on one device; a sample is the wall time of one pass over the
list between two device synchronisations, label maps left on the device; the figure per arm is the median over the repetitions with
min .. max.  The forwards per list are counted at the captured forward's replay, not derived."""
import argparse
import json
import os
os.environ.setdefault("DINOUNET_ALLOW_RANDOM_BACKBONE", "1")
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="dinounet_l")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--cases", type=int, default=64)
    ap.add_argument("--shape", type=int, nargs=2, default=(600, 450))
    ap.add_argument("--patch", type=int, default=512)
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from dinounet_amd.plans import PLANS_2D
    from dinounet_amd.network_architecture import DinoUNet
    from dinounet_amd import inference as INF
    if not torch.cuda.is_available():
        raise SystemExit("bench_predict_cases needs the GPU: no timing is taken on the host")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    net = DinoUNet.from_config(PLANS_2D, 3, 2, dinov3_pretrained_path=None, dinov3_model_name=a.model, precision=a.precision).to(dev).eval()
    patch = (a.patch, a.patch)
    cases = [torch.randn(3, 1, *a.shape, generator=torch.Generator().manual_seed(100 + i)).to(dev) for i in range(a.cases)]
    kw = dict(tile_step_size=0.5, use_gaussian=True, batch_size=a.batch, graph=True)

    replays = [0]
    replay = INF._WindowForward.__call__

    def counted(self, x):
        replays[0] += 1
        return replay(self, x)
    INF._WindowForward.__call__ = counted

    def arm_a():
        return [INF.predict_segmentation(net, c, patch, **kw) for c in cases]

    def arm_b():
        return INF.predict_cases_segmentation(net, cases, patch, **kw)

    # ---- agreement first (and the first warm-up: the capture happens here)
    forwards = {}
    segs = {}
    for name, arm in (("a", arm_a), ("b", arm_b)):
        replays[0] = 0
        segs[name] = arm()
        torch.cuda.synchronize()
        forwards[name] = replays[0]
    differing = outside = voxels = 0
    for c, sa, sb in zip(cases, segs["a"], segs["b"]):
        z = INF.predict_sliding_window_logits(net, c, patch, **kw).double()
        top = z.topk(2, dim=0).values
        band = (top[0] - top[1]) < 1e-5 * float(z.abs().max())
        diff = sa != sb
        differing += int(diff.sum())
        outside += int((diff & ~band).sum())
        voxels += diff.numel()
    agree = outside == 0 and differing / voxels < 1e-4
    lines = [f"bench_predict_cases: {a.model} {a.precision}, {a.cases} cases of (3, 1, {a.shape[0]}, {a.shape[1]}), patch {a.patch}^2, step 0.5, "
             f"window batch {a.batch}, graph=True",
             f"label maps a vs b: {differing} of {voxels} voxels differ, {outside} outside the tie band -> {'agree' if agree else 'DISAGREE'}",
             f"forwards per list (counted replays): a {forwards['a']}, b {forwards['b']}; planned for b "
             f"{INF.count_case_forwards(INF.plan_case_batches([c.shape[1:] for c in cases], patch, 0.5, a.batch))}"]
    if not agree:                                              # the timings below are then of two different results: exit status 1
        lines.append("THE TWO ARMS DISAGREE: the timings that follow compare different results")

    # ---- warm both arms once more, then alternate
    for arm in (arm_a, arm_b):
        arm()
    torch.cuda.synchronize()
    samples = {"a": [], "b": []}
    for _ in range(a.reps):
        for name, arm in (("a", arm_a), ("b", arm_b)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            arm()
            torch.cuda.synchronize()
            samples[name].append(time.perf_counter() - t0)
    res = {"model": a.model, "dtype": a.precision, "cases": a.cases, "case_shape": [3, 1, *a.shape], "patch": list(patch), "window_batch": a.batch,
           "reps": a.reps, "forwards_per_list": forwards}
    for name in ("a", "b"):
        s = samples[name]
        med = statistics.median(s)
        res[name] = {"median_s": round(med, 4), "min_s": round(min(s), 4), "max_s": round(max(s), 4), "cases_per_s": round(a.cases / med, 1),
                     "samples_s": [round(v, 4) for v in s]}
        lines.append(f"{name}: median {med * 1e3:8.1f} ms per list  (min {min(s) * 1e3:.1f} .. max {max(s) * 1e3:.1f}), {a.cases / med:7.1f} cases/s, "
                     f"{med / forwards[name] * 1e3:.2f} ms per forward")
    spread_a = max(samples["a"]) - min(samples["a"])
    gain = res["a"]["median_s"] - res["b"]["median_s"]
    res["a_spread_s"], res["a_over_b"] = round(spread_a, 4), round(res["a"]["median_s"] / res["b"]["median_s"], 3)
    lines.append(f"a - b = {gain * 1e3:.1f} ms per list, spread of a (max - min) {spread_a * 1e3:.1f} ms, a / b = {res['a_over_b']:.2f}")
    lines.append(json.dumps(res))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if not agree:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
