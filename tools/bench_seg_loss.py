#!/usr/bin/env python
"""Interleaved same-box A/B of the ignore-label / region losses (csrc/loss.hip du_dice_ce_masked_*, du_dice_bce_*, du_labels_to_regions)
against a PARENT tree's library (the commit before them: built from `git archive` of it, `python -m dinounet_amd._build` inside).

    python tools/bench_seg_loss.py --parent <parent tree> [--rounds 5] [--out profiles/seg_loss_ab.txt]

Legs (A = parent, B = this tree; A B A B ... for --rounds alternations; spread = max - min of one side's samples):
  1. masked softmax pair (sums + finish + backward, 30 % ignored) vs the parent's du_dice_ce pair at (8, 4, 512, 512): same bytes, so
     the bar is B's median <= A's median + the larger spread.
  2. region pair + du_labels_to_regions at (8, 3, 512, 512) + ignore vs the parent's softmax pair at K = 3, as GB/s of algorithmic bytes
     (softmax pair 2 (4K + 8) + 4K B/px; regions (8 + (R+1)) + (4R + R+1) + (4R + R+1 + 4R) B/px): bar B >= A - spread.
  3. the captured dinounet_l 512^2 batch-8 bf16 train step: this tree with build_loss(3, regions of 3, ignore) vs the parent's default
     step with num_classes = 3, ms per step, one fresh process per sample: bar B <= A + spread + the kernel-time difference of leg 2.
Kernel legs: each side's launch sequence is captured ITERS times into a hipGraph and timed by HIP events around the replay (ctypes launches
from Python are slower than the kernels)."""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _digest(tree):
    lib = os.path.join(tree, "dinounet_amd", "libdinounet_hip.so")
    stamp = lib + ".stamp"
    return {"lib_sha256": hashlib.sha256(open(lib, "rb").read()).hexdigest()[:16],
            "source_digest": open(stamp).read()[:16] if os.path.exists(stamp) else None}


def _load(tree):
    sys.path.insert(0, ROOT)
    from dinounet_amd import _lib
    l = C.CDLL(os.path.join(tree, "dinounet_amd", "libdinounet_hip.so"))
    for name, (ret, types) in _lib.header_prototypes(os.path.join(tree, "include", "dinounet_hip.h")).items():
        fn = getattr(l, name)
        fn.restype, fn.argtypes = ret, types
    return l


def kernel_legs(parent, rounds, iters, say):
    import torch
    d = torch.device("cuda", 0)
    A, Bl = _load(parent), _load(ROOT)
    p = lambda t: C.c_void_p(t.data_ptr())

    def chk(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} -> {rc}")

    def softmax_pair(L, K, masked, B=8, H=512, W=512):
        HW = H * W
        g = torch.Generator().manual_seed(K)
        x = (torch.randn(B, K, H, W, generator=g) * 2).to(d)
        t = torch.randint(0, K, (B, HW), generator=g)
        if masked:
            t = torch.where(torch.rand(B, HW, generator=g) < 0.3, torch.full_like(t, K), t)
        t = t.to(d)
        dl = torch.empty_like(x)
        n = int((L.du_dice_ce_masked_ws_elems if masked else L.du_dice_ce_ws_elems)(B, K, HW))
        ws = torch.empty(n, device=d)
        sums = torch.empty(2 + 3 * (K - 1), device=d)
        loss = torch.empty(1, device=d)
        coef = torch.empty(2 * (K - 1) + 1, device=d)

        st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if masked:
            run = [("sums", lambda: chk(L.du_dice_ce_masked_sums(p(x), p(t), p(sums), B, K, HW, K, p(ws), n, st()), "masked_sums")),
                   ("finish", lambda: chk(L.du_dice_ce_masked_finish(p(sums), p(loss), p(coef), K, 1e-5, 1.0, st()), "masked_finish")),
                   ("bwd", lambda: chk(L.du_dice_ce_masked_bwd(p(x), p(t), p(coef), None, p(dl), B, K, HW, K, st()), "masked_bwd"))]
        else:
            run = [("sums", lambda: chk(L.du_dice_ce_sums(p(x), p(t), p(sums), B, K, HW, p(ws), n, st()), "sums")),
                   ("finish", lambda: chk(L.du_dice_ce_finish(p(sums), p(loss), p(coef), K, B * HW, 1e-5, 1.0, st()), "finish")),
                   ("bwd", lambda: chk(L.du_dice_ce_bwd(p(x), p(t), p(coef), None, p(dl), B, K, HW, st()), "bwd"))]
        return run, (x, t, dl, ws, sums, loss, coef), B * HW * (2 * (4 * K + 8) + 4 * K)

    def region_pair(L, R=3, B=8, H=512, W=512):
        HW = H * W
        g = torch.Generator().manual_seed(100 + R)
        x = (torch.randn(B, R, H, W, generator=g) * 2).to(d)
        lab = torch.randint(0, 4, (B, HW), generator=g)
        lab = torch.where(torch.rand(B, HW, generator=g) < 0.3, torch.full_like(lab, 4), lab).to(d)
        table = torch.tensor([0b1110, 0b1100, 0b1000][:R], dtype=torch.int64, device=d)
        oh = torch.empty(B, R + 1, HW, dtype=torch.uint8, device=d)
        dl = torch.empty_like(x)
        n = int(L.du_dice_bce_ws_elems(B, R, HW))
        ws = torch.empty(n, device=d)
        sums = torch.empty(2 + 3 * R, device=d)
        loss = torch.empty(1, device=d)
        coef = torch.empty(2 * R + 1, device=d)

        st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
        run = [("labels_to_regions", lambda: chk(L.du_labels_to_regions(p(lab), p(table), p(oh), B, R, HW, 1, 4, st()), "labels_to_regions")),
               ("sums", lambda: chk(L.du_dice_bce_sums(p(x), p(oh), p(sums), B, R, HW, 1, p(ws), n, st()), "bce_sums")),
               ("finish", lambda: chk(L.du_dice_bce_finish(p(sums), p(loss), p(coef), R, 1, 1e-5, 1.0, st()), "bce_finish")),
               ("bwd", lambda: chk(L.du_dice_bce_bwd(p(x), p(oh), p(coef), None, p(dl), B, R, HW, 1, st()), "bce_bwd"))]
        nbytes = B * HW * ((8 + (R + 1)) + (4 * R + R + 1) + (4 * R + R + 1 + 4 * R))
        return run, (x, lab, table, oh, dl, ws, sums, loss, coef), nbytes

    def graphed(launches):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(3):
                for _, f in launches:
                    f()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for _ in range(iters):
                for _, f in launches:
                    f()
        return gr

    def time_us(gr):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        gr.replay()
        e0.record()
        gr.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / iters

    res = {}
    legs = [("1_masked_softmax_K4", softmax_pair(A, 4, False), softmax_pair(Bl, 4, True)),
            ("2_regions_R3_ignore", softmax_pair(A, 3, False), region_pair(Bl, 3))]
    for name, (ra, keep_a, by_a), (rb, keep_b, by_b) in legs:
        ga, gb = graphed(ra), graphed(rb)
        sa, sb = [], []
        for _ in range(rounds):
            sa.append(time_us(ga))
            sb.append(time_us(gb))
        ma, mb = statistics.median(sa), statistics.median(sb)
        spread = max(max(sa) - min(sa), max(sb) - min(sb))
        gba, gbb = by_a / ma / 1e3, by_b / mb / 1e3
        spread_gbs = max(by_a / min(sa) - by_a / max(sa), by_b / min(sb) - by_b / max(sb)) / 1e3
        r = {"parent_us": sa, "new_us": sb, "parent_median_us": round(ma, 2), "new_median_us": round(mb, 2), "spread_us": round(spread, 2),
             "parent_bytes": by_a, "new_bytes": by_b, "parent_GBs": round(gba, 1), "new_GBs": round(gbb, 1), "spread_GBs": round(spread_gbs, 1)}
        if name.startswith("1"):
            r["bar"] = "new_median_us <= parent_median_us + spread_us"
            r["pass"] = mb <= ma + spread
        else:
            r["bar"] = "new_GBs >= parent_GBs - spread_GBs"
            r["pass"] = gbb >= gba - spread_gbs
            r["kernel_time_diff_us"] = round(mb - ma, 2)
        # per-launch breakdown (each launch alone, `iters` times per replay; the sums entry includes the single-block partial-sum kernel)
        r["parent_breakdown_us"] = {k: round(time_us(graphed([(k, f)])), 2) for k, f in ra}
        r["new_breakdown_us"] = {k: round(time_us(graphed([(k, f)])), 2) for k, f in rb}
        res[name] = r
        say(f"{name}: parent {ma:.2f} us ({gba:.0f} GB/s)  new {mb:.2f} us ({gbb:.0f} GB/s)  spread {spread:.2f} us / {spread_gbs:.0f} GB/s  "
            f"pass={r['pass']}")
        say(f"  parent samples {[round(v, 2) for v in sa]}  new samples {[round(v, 2) for v in sb]}")
        say(f"  per launch: parent {r['parent_breakdown_us']}  new {r['new_breakdown_us']}")
        del ga, gb, keep_a, keep_b
    return res


def step_worker(tree, seg, steps, warmup):
    """one sample of leg 3, in a fresh process whose dinounet_amd is `tree`'s"""
    sys.path.insert(0, tree)
    os.environ.setdefault("DINOUNET_ALLOW_RANDOM_BACKBONE", "1")
    import torch
    from dinounet_amd.plans import PLANS_2D
    from dinounet_amd.network_architecture import DinoUNet
    from dinounet_amd.optim import FusedClipSGD
    from dinounet_amd import training as T
    import dinounet_amd
    assert os.path.realpath(os.path.dirname(dinounet_amd.__file__)) == os.path.realpath(os.path.join(tree, "dinounet_amd"))
    dev = torch.device("cuda", 0)
    torch.manual_seed(1234)
    net = DinoUNet.from_config(PLANS_2D, 3, 3, dinov3_pretrained_path=None, dinov3_model_name="dinounet_l", precision="bf16").to(dev).train()
    params = [p for p in net.parameters() if p.requires_grad]
    opt = FusedClipSGD(params, lr=1e-3, momentum=0.99, nesterov=True, weight_decay=3e-5, max_norm=12.0)
    g = torch.Generator().manual_seed(100)
    x = torch.randn(8, 3, 512, 512, generator=g).to(dev)
    if seg:
        lab = torch.randint(0, 4, (8, 1, 512, 512), generator=g)
        lab = torch.where(torch.rand(lab.shape, generator=g) < 0.3, torch.full_like(lab, 4), lab)
        ts = T.TrainStep(net, opt, params, x.shape, lab.shape, dev, graph=True, warmup=3,
                         loss=T.build_loss(3, regions=[(1, 2, 3), (2, 3), (3,)], ignore_label=4))
    else:
        lab = torch.randint(0, 3, (8, 1, 512, 512), generator=g)
        ts = T.TrainStep(net, opt, params, x.shape, lab.shape, dev, graph=True, warmup=3)
    ts(x, lab.to(dev))
    for _ in range(warmup):
        ts()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = ts()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    print(json.dumps({"ms_per_step": ms, "capture": ts.capture_mode, "loss": float(loss)}), flush=True)


def step_leg(parent, rounds, steps, warmup, timeout, say):
    def run(tree, seg):
        cmd = [sys.executable, os.path.abspath(__file__), "--step-worker", tree, "--steps", str(steps), "--warmup", str(warmup)]
        if seg:
            cmd.append("--seg")
        e = dict(os.environ)
        e.pop("PYTHONPATH", None)
        r = subprocess.run(cmd, cwd=tree, env=e, capture_output=True, text=True, timeout=timeout)
        js = [l for l in r.stdout.splitlines() if l.startswith("{")]
        if r.returncode != 0 or not js:
            raise RuntimeError(f"step worker ({tree}, seg={seg}) rc {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}")
        return json.loads(js[-1])

    sa, sb = [], []
    for i in range(rounds):
        a = run(parent, False)
        b = run(ROOT, True)
        sa.append(a["ms_per_step"])
        sb.append(b["ms_per_step"])
        say(f"  round {i}: parent {a['ms_per_step']:.3f} ms ({a['capture']})  new {b['ms_per_step']:.3f} ms ({b['capture']})")
    ma, mb = statistics.median(sa), statistics.median(sb)
    spread = max(max(sa) - min(sa), max(sb) - min(sb))
    return {"parent_ms": sa, "new_ms": sb, "parent_median_ms": round(ma, 3), "new_median_ms": round(mb, 3), "spread_ms": round(spread, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="parent tree with its library built")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50, help="kernel legs: launch sequences per timed graph replay")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--no-step", action="store_true", help="kernel legs only")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step-worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--seg", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step_worker:
        return step_worker(os.path.abspath(a.step_worker), a.seg, a.steps, a.warmup)
    parent = os.path.abspath(a.parent)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# seg-loss A/B, {a.rounds} alternations (parent first in each), kernel legs {a.iters} launch sequences per graph replay")
    say(f"# parent {json.dumps(_digest(parent))}  new {json.dumps(_digest(ROOT))}")
    out = {"parent": _digest(parent), "new": _digest(ROOT), "rounds": a.rounds}
    out["kernels"] = kernel_legs(parent, a.rounds, a.iters, say)
    if not a.no_step:
        say(f"3_step: dinounet_l 512^2 batch 8 bf16 captured step, --steps {a.steps} --warmup {a.warmup}, fresh process per sample")
        st = step_leg(parent, a.rounds, a.steps, a.warmup, a.timeout, say)
        kd_ms = out["kernels"]["2_regions_R3_ignore"]["kernel_time_diff_us"] / 1e3
        st["kernel_time_diff_ms"] = round(kd_ms, 4)
        st["bar"] = "new_median_ms <= parent_median_ms + spread_ms + max(kernel_time_diff_ms, 0)"
        st["pass"] = st["new_median_ms"] <= st["parent_median_ms"] + st["spread_ms"] + max(kd_ms, 0.0)
        out["step"] = st
        say(f"3_step: parent {st['parent_median_ms']:.3f} ms  new {st['new_median_ms']:.3f} ms  spread {st['spread_ms']:.3f} ms  "
            f"kernel diff {kd_ms * 1e3:.1f} us  pass={st['pass']}")
    say(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
