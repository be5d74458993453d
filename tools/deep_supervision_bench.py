#!/usr/bin/env python
"""What the fused deep-supervision loss (csrc/loss.hip du_ds_loss_*, training.DeepSupervisionLoss) buys, measured on one MI355X.

    python tools/deep_supervision_bench.py [--out profiles/deep_supervision.txt] [--rounds 7]

The driver starts every leg as a fresh child process under its own time limit and stops at the first leg that fails.
 (a) loss A/B, forward + backward at (8,3,512,512) -> 256^2 -> 128^2, weights [2/3,1/3,0] and the DDP weights (all three active):
     A = the composition of the kernels this tree had before the fused pass -- per active scale a strided slice of the label map (the
         index formula at exact 2x / 4x pooling is rows / columns 1::2 and 2::4), ops.dice_ce_loss, and the weighted sum in torch;
     B = DeepSupervisionLoss (ops.ds_seg_loss).
     Each side is captured once into a hipGraph; the two are alternated A B A B ... in one process, `--iters` replays per sample between
     two device events.  spread = max - min over one side's samples of identical runs; B counts as faster only if
     median(A) - median(B) exceeds the larger of the two spreads.  The kernel nodes of either graph are counted (hipGraphGetNodes).
 (b) the dinounet_l bf16 batch-8 512^2 TrainStep without and with deep supervision (plain labels, weights [2/3,1/3,0]): slices/s over
     `--steps` replayed steps and the kernel nodes of the captured step."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("DINOUNET_ALLOW_RANDOM_BACKBONE", "1")


def _keep_graphs():
    """every torch.cuda.CUDAGraph made from here on keeps its hipGraph_t so that its nodes can be counted"""
    import torch
    orig = torch.cuda.CUDAGraph
    torch.cuda.CUDAGraph = lambda *a, **k: orig(*a, **dict(k, keep_graph=True))


def kernel_nodes(graph):
    """(all nodes, kernel nodes) of a captured graph, or None where the runtime library or the raw graph cannot be reached"""
    try:
        path = None
        for ln in open("/proc/self/maps"):
            if "libamdhip64.so" in ln:
                path = ln.split()[-1]
                break
        if path is None:
            return None
        hip = ctypes.CDLL(path)                    # the copy torch already loaded: same handle
        raw = ctypes.c_void_p(int(graph.raw_cuda_graph()))
        n = ctypes.c_size_t(0)
        hip.hipGraphGetNodes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
        hip.hipGraphNodeGetType.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
        if hip.hipGraphGetNodes(raw, None, ctypes.byref(n)) != 0 or n.value == 0:
            return None
        nodes = (ctypes.c_void_p * n.value)()
        if hip.hipGraphGetNodes(raw, nodes, ctypes.byref(n)) != 0:
            return None
        kern = 0
        for nd in nodes:
            t = ctypes.c_int(-1)
            if hip.hipGraphNodeGetType(ctypes.c_void_p(nd), ctypes.byref(t)) == 0 and t.value == 0:      # hipGraphNodeTypeKernel
                kern += 1
        return n.value, kern
    except Exception as e:  # noqa: BLE001
        return f"not counted ({e!r})"


def leg_loss(args):
    import torch
    from dinounet_amd import ops
    from dinounet_amd.training import build_loss, deep_supervision_weights
    _keep_graphs()
    d = torch.device("cuda", 0)
    B, K, H = 8, 3, 512
    g = torch.Generator().manual_seed(0)
    outs = [(torch.randn(B, K, H >> s, H >> s, generator=g) * 2).to(d).requires_grad_(True) for s in range(3)]
    lab = torch.randint(0, K, (B, 1, H, H), generator=g).to(d)
    res = {}
    for wname, w in (("[2/3,1/3,0]", deep_supervision_weights(3)), ("ddp weights", deep_supervision_weights(3, ddp=True))):
        mod = build_loss(K, deep_supervision_weights=w)
        act = [o for o, wi in zip(outs, w) if wi != 0.0]

        def fused():
            return torch.autograd.grad(mod(outs, lab), act)

        def composed():
            total = None
            for s, (o, wi) in enumerate(zip(outs, w)):
                if wi == 0.0:
                    continue
                st = 1 << s
                l = wi * ops.dice_ce_loss(o, lab[:, :, st // 2::st, st // 2::st])
                total = l if total is None else total + l
            return torch.autograd.grad(total, act)

        ga = fused()
        gb = composed()
        torch.cuda.synchronize()
        agree = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(ga, gb))
        graphs = {}
        for name, fn in (("A composition", composed), ("B fused", fused)):
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for _ in range(3):
                    fn()
            torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                keep = fn()
            graphs[name] = (gr, keep)
        samples = {k: [] for k in graphs}
        for name, (gr, _) in graphs.items():
            for _ in range(20):
                gr.replay()
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for name, (gr, _) in graphs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.iters):
                    gr.replay()
                e1.record()
                torch.cuda.synchronize()
                samples[name].append(e0.elapsed_time(e1) * 1e3 / args.iters)
        res[wname] = {"gradients_agree_rel": agree,
                      "sides": {k: {"us": [round(v, 2) for v in samples[k]], "median_us": round(statistics.median(samples[k]), 2),
                                    "spread_us": round(max(samples[k]) - min(samples[k]), 2), "nodes": None}
                                for k in graphs}}
        print("RESULT " + json.dumps(res), flush=True)          # the timings first: counting nodes goes through the raw graph handle
        for k in graphs:
            res[wname]["sides"][k]["nodes"] = kernel_nodes(graphs[k][0])
    print("RESULT " + json.dumps(res), flush=True)


def leg_step(args, ds):
    import torch
    from oracle import weights
    from oracle.refshim import PLANS_2D
    from dinounet_amd.network_architecture import DinoUNet
    from dinounet_amd.optim import FusedClipSGD
    from dinounet_amd.training import TrainStep, build_loss, deep_supervision_weights
    _keep_graphs()
    d = torch.device("cuda", 0)
    plans = dict(PLANS_2D, architecture=dict(PLANS_2D["architecture"], deep_supervision=bool(ds)))
    net = DinoUNet.from_config(plans, 3, 3, dinov3_pretrained_path=None, dinov3_model_name="dinounet_l", precision="bf16").to(d).train()
    params = [p for p in net.parameters() if p.requires_grad]
    opt = FusedClipSGD(params, 1e-3, momentum=0.99, nesterov=True, weight_decay=3e-5)
    x = weights.make_input(8, 3, 512, 512, seed=3).to(d)
    lab = weights.make_target(8, 512, 512, 3, seed=3).to(d)
    loss = build_loss(3, deep_supervision_weights=deep_supervision_weights(3) if ds else None)
    ts = TrainStep(net, opt, params, x.shape, lab.shape, d, graph=True, warmup=3, loss=loss)
    ts(x, lab)
    for _ in range(3 + 5):
        ts()
    torch.cuda.synchronize()
    rates = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            ts()
        e1.record()
        torch.cuda.synchronize()
        rates.append(8 * args.steps / (e0.elapsed_time(e1) * 1e-3))
    r = {"deep_supervision": bool(ds), "capture_mode": ts.capture_mode, "loss": float(ts.loss), "slices_per_s": [round(v, 1) for v in rates],
         "nodes": None}
    print("RESULT " + json.dumps(r), flush=True)
    if ts.capture_mode == "whole_step":
        r["nodes"] = kernel_nodes(ts.graph)
    print("RESULT " + json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default=None, choices=["loss", "step_plain", "step_ds"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deep_supervision.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    if args.leg == "loss":
        return leg_loss(args)
    if args.leg in ("step_plain", "step_ds"):
        return leg_step(args, args.leg == "step_ds")
    lines = ["# tools/deep_supervision_bench.py: one MI355X, every leg a fresh process", ""]
    results = {}
    for leg, limit in (("loss", 240), ("step_plain", 300), ("step_ds", 300)):
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--rounds", str(args.rounds), "--iters", str(args.iters),
               "--steps", str(args.steps)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            lines.append(f"leg {leg}: no result within {limit} s; the legs after it were not started")
            break
        got = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if got:
            results[leg] = json.loads(got[-1][7:])
        if p.returncode != 0:
            lines.append(f"leg {leg}: exit status {p.returncode}{' after its timings' if got else ''}; the legs after it were not started")
            lines += ["    " + ln for ln in (p.stderr or p.stdout).splitlines()[-12:]]
            break
    if "loss" in results:
        lines.append(f"(a) loss forward + backward, (8,3,512,512) -> 256^2 -> 128^2, {args.rounds} alternations x {args.iters} replays of a captured graph")
        for wname, r in results["loss"].items():
            a, b = r["sides"]["A composition"], r["sides"]["B fused"]
            spread = max(a["spread_us"], b["spread_us"])
            gain = a["median_us"] - b["median_us"]
            verdict = "fused is faster by more than the spread" if gain > spread else "no difference beyond the spread"
            lines.append(f"  weights {wname}: gradients of the two sides agree to {r['gradients_agree_rel']:.1e}")
            for k, v in r["sides"].items():
                lines.append(f"    {k:14s} median {v['median_us']:8.2f} us  spread {v['spread_us']:6.2f} us  (graph nodes, kernel nodes) {v['nodes']}  samples {v['us']}")
            lines.append(f"    A - B = {gain:.2f} us ({a['median_us'] / b['median_us']:.3f}x), larger spread {spread:.2f} us: {verdict}")
    for leg in ("step_plain", "step_ds"):
        if leg in results:
            r = results[leg]
            lines.append(f"(b) dinounet_l bf16 batch 8 512^2 TrainStep, deep supervision {r['deep_supervision']}: capture {r['capture_mode']}, "
                         f"slices/s {r['slices_per_s']} (median {statistics.median(r['slices_per_s']):.1f}), (graph nodes, kernel nodes) {r['nodes']}, "
                         f"loss {r['loss']:.4f}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(text)
    print(text)
    return 0 if len(results) == 3 else 1


if __name__ == "__main__":
    sys.exit(main())
