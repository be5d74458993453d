#!/usr/bin/env python
"""Forward + backward time of the fused option losses (csrc/loss_opt.hip) at batch 8, 512 x 512, K = 3 and K = 8, for three option sets
(weights only; per-sample Dice; class weights + ignore label), each against two yardsticks on the same inputs: the default fused loss
of this package at the same shape (du_dice_ce_* without, du_dice_ce_masked_* with an ignore label: the kernels every default module
runs) and the torch formula for the same options on the GPU (training._dc_and_ce_opt_torch, eager, forward + backward).

    python tools/bench_loss_options.py [--rounds 5] [--iters 50] [--out profiles/loss_options.txt]

Method: the launch sequence of a kernel leg (sums, finish, backward through the C ABI) is captured `iters` times into a hipGraph and timed
with device events around one replay (ctypes launches from Python are slower than the kernels); the legs alternate for `rounds` rounds
after a warm-up; median and spread (max - min) per leg.  The torch formula is timed eager with device events around `iters` forward +
backward passes after a warm-up (it allocates; its time includes the launch path, which is what a user of the formula pays).
Algorithmic bytes per pixel: forward 4 K + 8, backward 4 K + 8 + 4 K."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETS = [("weights", dict(weight_ce=0.5, weight_dice=2.0), False),
        ("per_sample", dict(batch_dice=False), False),
        ("class_w_ignore", dict(class_w=True), True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from dinounet_amd import _lib
    from dinounet_amd import training as T
    if not torch.cuda.is_available():
        raise SystemExit("bench_loss_options: no GPU (times are measured on the device or not at all)")
    d = torch.device("cuda", 0)
    L = _lib.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def chk(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} -> {rc}")

    def graphed(launches):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(3):
                for f in launches:
                    f()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for _ in range(a.iters):
                for f in launches:
                    f()
        return gr

    def time_graph(gr):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        gr.replay()
        e0.record()
        gr.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.iters

    def time_eager(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.iters

    B, H, W = 8, 512, 512
    HW = H * W
    say(f"# loss options, forward + backward, batch {B}, {H} x {W}; {a.rounds} alternating rounds, {a.iters} sequences per timed replay; us")
    say(f"# {torch.cuda.get_device_name(0)}")
    for K in (3, 8):
        g = torch.Generator().manual_seed(K)
        x = (torch.randn(B, K, H, W, generator=g) * 2).to(d)
        lab = torch.randint(0, K, (B, HW), generator=g)
        lab_ign = torch.where(torch.rand(B, HW, generator=g) < 0.3, torch.full_like(lab, 255), lab).to(d)
        lab = lab.to(d)
        dl = torch.empty_like(x)
        cw = torch.tensor([0.5 + 0.25 * k for k in range(K)], dtype=torch.float32, device=d)
        nbytes = B * HW * (2 * (4 * K + 8) + 4 * K)
        keep = []
        for name, opt, ign in SETS:
            t = lab_ign if ign else lab
            o = _lib.LossOpt(K, 0, int(ign), 255, 0, int(opt.get("batch_dice", True)), opt.get("weight_ce", 1.0), opt.get("weight_dice", 1.0),
                             cw.data_ptr() if opt.get("class_w") else None)
            ref = C.byref(o)
            rows = 1 if o.batch_dice else B
            n = int(L.du_loss_opt_ws_elems(ref, B, HW))
            ws, sums = torch.empty(n, device=d), torch.empty(rows * (2 + 3 * (K - 1)), device=d)
            loss, coef = torch.empty(1, device=d), torch.empty(rows * 2 * (K - 1) + 1, device=d)
            new = [lambda: chk(L.du_loss_opt_sums(ref, p(x), p(t), p(sums), B, HW, p(ws), n, st()), "opt_sums"),
                   lambda: chk(L.du_loss_opt_finish(ref, p(sums), p(loss), p(coef), B, 1e-5, 1.0, st()), "opt_finish"),
                   lambda: chk(L.du_loss_opt_bwd(ref, p(x), p(t), p(coef), None, p(dl), B, HW, st()), "opt_bwd")]
            n0 = int((L.du_dice_ce_masked_ws_elems if ign else L.du_dice_ce_ws_elems)(B, K, HW))
            ws0, sums0, coef0 = torch.empty(n0, device=d), torch.empty(2 + 3 * (K - 1), device=d), torch.empty(2 * (K - 1) + 1, device=d)
            if ign:
                base = [lambda: chk(L.du_dice_ce_masked_sums(p(x), p(t), p(sums0), B, K, HW, 255, p(ws0), n0, st()), "masked_sums"),
                        lambda: chk(L.du_dice_ce_masked_finish(p(sums0), p(loss), p(coef0), K, 1e-5, 1.0, st()), "masked_finish"),
                        lambda: chk(L.du_dice_ce_masked_bwd(p(x), p(t), p(coef0), None, p(dl), B, K, HW, 255, st()), "masked_bwd")]
            else:
                base = [lambda: chk(L.du_dice_ce_sums(p(x), p(t), p(sums0), B, K, HW, p(ws0), n0, st()), "sums"),
                        lambda: chk(L.du_dice_ce_finish(p(sums0), p(loss), p(coef0), K, B * HW, 1e-5, 1.0, st()), "finish"),
                        lambda: chk(L.du_dice_ce_bwd(p(x), p(t), p(coef0), None, p(dl), B, K, HW, st()), "bwd")]
            keep.append((o, ws, sums, coef, ws0, sums0, coef0))
            xg = x.clone().requires_grad_(True)
            t4 = t.view(B, 1, H, W)

            def torch_formula():
                xg.grad = None
                T._dc_and_ce_opt_torch(xg, t4, 255 if ign else None, 1e-5, False, None, opt.get("weight_ce", 1.0), opt.get("weight_dice", 1.0),
                                       opt.get("batch_dice", True), False, cw if opt.get("class_w") else None).backward()

            gn, gb = graphed(new), graphed(base)
            parts = [round(time_graph(graphed([f])), 2) for f in new]
            sn, sb, stc = [], [], []
            for _ in range(a.rounds):
                sb.append(time_graph(gb))
                sn.append(time_graph(gn))
                stc.append(time_eager(torch_formula))
            mn, mb, mt = statistics.median(sn), statistics.median(sb), statistics.median(stc)
            say(f"K={K} {name:15s} new {mn:8.2f} (spread {max(sn) - min(sn):.2f}, {nbytes / mn / 1e3:.0f} GB/s; sums / finish / bwd {parts})  "
                f"default fused {mb:8.2f} (spread {max(sb) - min(sb):.2f}, {'masked' if ign else 'plain'})  torch formula {mt:9.2f} "
                f"(spread {max(stc) - min(stc):.2f})  new / default {mn / mb:.2f}  torch / new {mt / mn:.1f}")
            del gn, gb
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
