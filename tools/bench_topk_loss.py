#!/usr/bin/env python
"""Forward + backward of the top-k loss (csrc/loss_topk.hip, training.dc_and_topk_loss) on one GPU, three routes on the same inputs,
alternated round by round (spread = max - min of one route's samples):

  fused      ops.dice_topk_loss                       (values + radix select + selection map, one backward pass)
  torch      the torch formula of training.py on the GPU (cross_entropy(reduction="none") + torch.topk + the Dice code, autograd)
  dice_ce    ops.dice_ce_loss, the fused Dice + CE pair: the floor (two passes over the logits, no selection)

at (8, 3, 512, 512) and (8, 4, 512, 512), k = 10 %, fp32 logits, plain labels.

    python tools/bench_topk_loss.py [--rounds 7] [--iters 50] [--out profiles/topk_loss.txt]

Each route's forward + backward is captured ITERS times into one hipGraph (after warm-up on a side stream) and timed with HIP events
around REPS replays (1000 forward + backward, about 0.1 s, per window).  Every route is also timed eagerly (events around as many
back-to-back calls), which is what a step outside a graph pays,
host launch path included; the torch route is timed eagerly only (its torch.topk must not be captured, see training._topk_ce_torch).  The fused route's three
entry points (du_topk_loss_fwd / _finish / _bwd) are timed one by one.  Outputs are compared before timing: the loss of the fused route
against the torch route."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(8, 3, 512, 512), (8, 4, 512, 512)]
K_PERCENT = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50, help="forward + backward per graph / per eager burst")
    ap.add_argument("--reps", type=int, default=20, help="graph replays / eager bursts per timed window (a window is iters * reps calls)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--routes", default="fused,torch,dice_ce", help="comma-separated subset of the routes")
    ap.add_argument("--shapes", type=int, default=len(SHAPES), help="the first n of the shapes")
    a = ap.parse_args()
    import torch
    from dinounet_amd import _lib, ops, training as T
    assert torch.cuda.is_available(), "the benchmark needs the GPU"
    d = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / (a.iters * a.reps)

    def eager_timer(step):
        def many():
            for _ in range(a.iters):
                step()
        many()
        return lambda: events(many)

    def graph_timer(step):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(3):
                step()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for _ in range(a.iters):
                step()
        gr.replay()
        torch.cuda.synchronize()
        return lambda: events(gr.replay)

    say(f"# top-k loss forward + backward, k = {K_PERCENT} %, {a.rounds} alternated rounds, {a.iters * a.reps} forward + backward per timed window ({a.reps} replays of a graph of "
        f"{a.iters}); us per "
        "forward + backward, median (spread)")
    out = {}
    for shape in SHAPES[:a.shapes]:
        B, K, H, W = shape
        HW = H * W
        g = torch.Generator().manual_seed(K)
        x = (torch.randn(shape, generator=g) * 2).to(d).requires_grad_(True)
        lab = torch.randint(0, K, (B, 1, H, W), generator=g).to(d)

        def fb(loss_fn):
            def step():
                loss = loss_fn()
                (gx,) = torch.autograd.grad(loss, x)
                return loss, gx
            return step

        routes = {"fused": fb(lambda: ops.dice_topk_loss(x, lab, K_PERCENT)),
                  "torch": fb(lambda: T._topk_ce_torch(x, lab, K_PERCENT, None) - T._soft_dice_torch(x, lab, None, 1e-5, False, None)),
                  "dice_ce": fb(lambda: ops.dice_ce_loss(x, lab))}
        # (nothing of these two calls may stay alive: a loss kept here keeps x's AccumulateGrad node of THIS stream alive, the backward
        #  of a later capture then synchronises with this stream, which a capture does not allow)
        lf, gf = routes["fused"]()
        lt, gt = routes["torch"]()
        torch.cuda.synchronize()
        gdiff = float((gf - gt).abs().max() / gt.abs().max())
        lf, lt = float(lf.detach()), float(lt.detach())
        del gf, gt
        say(f"{shape}: fused loss {lf:.6f}  torch loss {lt:.6f}  gradient max |diff| / max |torch| {gdiff:.2e} "
            "(the two may select different voxels among near-equal values)")
        routes = {k: v for k, v in routes.items() if k in a.routes.split(",")}
        timers, captured = {}, {}
        for name, step in routes.items():
            # the torch route is never captured: the sort inside torch.topk (rocprim's onesweep radix sort) faulted with an illegal memory
            # access when a graph holding it was replayed -- training._topk_ce_torch refuses a capture for the same reason
            captured[name] = name != "torch"
            if captured[name]:
                timers[name + "/graph"] = graph_timer(step)
            timers[name + "/eager"] = eager_timer(step)
        # the fused route's three entry points, one by one (graphs of ITERS launches of one entry point)
        L = _lib.lib()
        p = lambda t: C.c_void_p(t.data_ptr())
        st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
        xd = x.detach()
        tgt = lab.reshape(B, HW).contiguous()
        n = int(L.du_topk_loss_ws_elems(B, K, HW))
        k_vox = T.topk_voxels(B * HW, K_PERCENT)
        ws = torch.empty(n, dtype=torch.int32, device=d)
        values = torch.empty(B, HW, device=d)
        sel = torch.empty(B, HW, dtype=torch.uint8, device=d)
        sums, loss, coef = torch.empty(2 + 3 * (K - 1), device=d), torch.empty(1, device=d), torch.empty(2 * (K - 1) + 1, device=d)
        info = torch.empty(4, dtype=torch.int32, device=d)
        dl = torch.empty_like(xd)
        parts = {"fwd": lambda: _lib.check(L.du_topk_loss_fwd(p(xd), p(tgt), p(values), p(sums), B, K, HW, 0, 0, k_vox, p(ws), n, st()), "fwd"),
                 "finish": lambda: _lib.check(L.du_topk_loss_finish(p(sums), p(values), p(ws), n, p(sel), p(loss), p(coef), p(info), B, K, HW,
                                                                    k_vox, 1, 1e-5, 1.0, st()), "finish"),
                 "bwd": lambda: _lib.check(L.du_topk_loss_bwd(p(xd), p(tgt), p(sel), p(coef), None, p(dl), B, K, HW, 0, 0, st()), "bwd")}
        for f in parts.values():
            f()
        torch.cuda.synchronize()
        for name, f in parts.items():
            timers["fused." + name + "/graph"] = graph_timer(f)
        samples = {k: [] for k in timers}
        for _ in range(a.rounds):
            for k, t in timers.items():
                samples[k].append(t())
        res = {}
        for k, v in samples.items():
            res[k] = {"median_us": round(statistics.median(v), 2), "spread_us": round(max(v) - min(v), 2), "samples_us": [round(s, 2) for s in v]}
            say(f"  {k:22s} {res[k]['median_us']:10.2f} us  ({res[k]['spread_us']:.2f})")
        # algorithmic bytes: values pass K*4 + 8 read + 4 written, two sweeps + count + select over 4 B (+ 1 B written), backward K*4 + 8 + 1
        # read and K*4 written
        nbytes = B * HW * ((4 * K + 8 + 4) + 4 * 4 + 1 + (4 * K + 8 + 1) + 4 * K)
        if captured.get("fused"):
            res["fused_GBs_algorithmic"] = round(nbytes / res["fused/graph"]["median_us"] / 1e3, 1)
            say(f"  fused route: {nbytes / 1e6:.1f} MB algorithmic -> {res['fused_GBs_algorithmic']} GB/s over the graphed time")
        res["captured"] = captured
        out[str(shape)] = res
        del timers
    say(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
