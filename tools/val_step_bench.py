#!/usr/bin/env python
"""What the validation step costs on top of the eval forward: dinounet_l 512^2 batch 8 bf16, K = 3 classes + an ignore label (30 % of
the pixels), per step

  a. the captured eval-mode forward alone (hipGraph replay);
  b. a training.ValStep replay: the same forward + the fused loss / tp / fp / fn pass (csrc/loss.hip), nothing read back;
  c. the forward of (a) followed by the stock-torch restatement of nnUNetTrainer.validation_step's tail (nnUNetTrainer.py:966-1008):
     the DC+CE loss with an ignore label in torch ops, argmax, scatter_, the three products, the tiled mask, three reductions and the
     per-step .cpu() of loss / tp / fp / fn.

    python tools/val_step_bench.py [--rounds 7] [--iters 50] [--out profiles/val_step.txt]

The three legs alternate (a b c a b c ...) in one process on one device; each sample is the wall time of `iters` steps between two
device synchronisations, after `--warmup` untimed steps per leg; the figure per leg is the median over the rounds, the spread max - min.
The expectation to confirm or refute: (b - a) is a small fraction of (c - a)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("DINOUNET_ALLOW_RANDOM_BACKBONE", "1")


def stock_validation_tail(logits, target, ignore_label, smooth=1e-5):
    """loss (DC_and_CE_loss with an ignore label, batch dice, no background) and the hard tp / fp / fn the way the reference computes
    them, in stock torch ops with full-size float one-hot temporaries, read back to the host"""
    import torch
    import torch.nn.functional as F
    logits = logits.float()
    mask = target != ignore_label
    lab = torch.where(mask, target, torch.zeros_like(target))
    mf = mask.float()
    nll = F.cross_entropy(logits, lab[:, 0], reduction="none")[:, None]
    ce = (nll * mf).sum() / mf.sum().clamp_min(1)
    prob = torch.softmax(logits, 1)
    onehot = torch.zeros_like(prob).scatter_(1, lab, 1)
    p, y = prob[:, 1:] * mf, onehot[:, 1:] * mf
    dc = (2 * (p * y).sum((0, 2, 3)) + smooth) / torch.clip(y.sum((0, 2, 3)) + p.sum((0, 2, 3)) + smooth, 1e-8)
    loss = ce - dc.mean()
    pred = torch.zeros_like(logits).scatter_(1, logits.argmax(1)[:, None], 1)
    tiled = torch.tile(mf, (1, logits.shape[1], 1, 1))
    tp = (pred * onehot * tiled).sum((0, 2, 3))
    fp = (pred * (1 - onehot) * tiled).sum((0, 2, 3))
    fn = ((1 - pred) * onehot * tiled).sum((0, 2, 3))
    return loss.cpu().numpy(), tp.cpu().numpy()[1:], fp.cpu().numpy()[1:], fn.cpu().numpy()[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="dinounet_l")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from dinounet_amd import ops
    from dinounet_amd.network_architecture import DinoUNet
    from dinounet_amd.plans import PLANS_2D
    from dinounet_amd.training import ValStep, build_loss
    dev = torch.device("cuda", 0)
    K, ignore = 3, 3
    torch.manual_seed(1234)
    net = DinoUNet.from_config(PLANS_2D, 3, K, dinov3_pretrained_path=None, dinov3_model_name=a.model, precision="bf16").to(dev).train()
    g = torch.Generator().manual_seed(100)
    x = torch.randn(a.batch, 3, a.size, a.size, generator=g).to(dev)
    lab = torch.randint(0, K, (a.batch, 1, a.size, a.size), generator=g)
    lab = torch.where(torch.rand(lab.shape, generator=g) < 0.3, torch.full_like(lab, ignore), lab).to(dev)

    # b: the product's validation step (two eager steps, then the capture)
    vs = ValStep(net, x.shape, lab.shape, dev, loss=build_loss(K, ignore_label=ignore), graph=True, warmup=2)
    for _ in range(3):
        vs(x, lab)
    torch.cuda.synchronize()
    assert vs.graph is not None
    # a: the same eval forward alone, captured the same way
    net.eval()
    fx = x.clone()
    with torch.no_grad():
        fgraph = torch.cuda.CUDAGraph()
        with ops.capture(fgraph):
            logits = net(fx)
    net.train()

    def leg_a():
        fgraph.replay()

    def leg_b():
        vs()

    stock = {}

    def leg_c():
        fgraph.replay()
        stock["out"] = stock_validation_tail(logits, lab, ignore)

    # the three legs compute the same thing
    leg_c()
    last = vs.last()
    torch.cuda.synchronize()
    same = all(np.array_equal(last[k], stock["out"][i + 1].astype(np.int64)) for i, k in enumerate(("tp_hard", "fp_hard", "fn_hard")))
    dloss = abs(float(last["loss"]) - float(stock["out"][0]))

    legs = [("a_forward", leg_a), ("b_val_step", leg_b), ("c_forward_plus_stock_torch", leg_c)]
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
    med = {n: statistics.median(v) for n, v in samples.items()}
    lines = [f"# validation step, {a.model} {a.size}^2 batch {a.batch} bf16, K = {K} + ignore label (30 % ignored); {a.rounds} rounds a b c "
             f"interleaved, {a.iters} steps per sample, {a.warmup} warm-up steps per leg; ms per step, median [min .. max]",
             f"# counts of b == counts of c: {same}; |loss_b - loss_c| = {dloss:.2e}"]
    for n, _ in legs:
        v = samples[n]
        lines.append(f"{n}: {med[n]:.3f} ms  [{min(v):.3f} .. {max(v):.3f}]")
    extra_b, extra_c = med["b_val_step"] - med["a_forward"], med["c_forward_plus_stock_torch"] - med["a_forward"]
    lines.append(f"b - a = {extra_b * 1e3:.1f} us   c - a = {extra_c * 1e3:.1f} us   (b - a) / (c - a) = {extra_b / extra_c:.3f}")
    lines.append(json.dumps({"samples_ms": {n: [round(s, 4) for s in v] for n, v in samples.items()}, "counts_equal": same}))
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")
    vs.epoch_end()


if __name__ == "__main__":
    main()
