#!/usr/bin/env python
"""Does a window's logits depend on its slot in the window batch, or on what else is in the batch?  Forwards only: one seeded
(batch, 3, size, size) batch through the eval-mode network, then the same windows permuted, alone among zeros, and with one window
zeroed.  Every line gives, per ORIGINAL window, the maximum |difference| of its logits against the first forward, and the share of all
voxels whose argmax changed.  In bf16 the same network is then switched to its fp32 kernels (set_precision: the same weights) and the bf16
logits of the first and the last window are measured against it twice -- in an ordinary slot and in the last slot (natural order against
the batch rotated by one) -- which tells an alternative route of bf16 accuracy from a defect of the route the last slot takes.
DESIGN section 3i reads the output (profiles/predict_cases.txt).

    python tools/probe_batch_slots.py [--model dinounet_l] [--precision bf16|fp32] [--batch 12] [--size 512]"""
import argparse
import os
os.environ.setdefault("DINOUNET_ALLOW_RANDOM_BACKBONE", "1")
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="dinounet_l")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from dinounet_amd.plans import PLANS_2D
    from dinounet_amd.network_architecture import DinoUNet
    if not torch.cuda.is_available():
        raise SystemExit("probe_batch_slots needs the GPU")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    net = DinoUNet.from_config(PLANS_2D, 3, 2, dinov3_pretrained_path=None, dinov3_model_name=a.model, precision=a.precision).to(dev).eval()
    B = a.batch
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def fwd(x):
        with torch.no_grad():
            y = net(x)
        return (y[0] if isinstance(y, (list, tuple)) else y).float().clone()

    def line(name, got, want, total=None):
        """got, want: logits of the same windows; total: windows the flip share is taken over (default: those given)"""
        per = " ".join(f"{float((got[i] - want[i]).abs().max()):.1e}" for i in range(got.shape[0]))
        flips = int((got.argmax(1) != want.argmax(1)).sum()) / ((total or got.shape[0]) * got.shape[2] * got.shape[3])
        say(f"{name + ':':34s} {per}   argmax flips {flips:.3e}")

    X = torch.randn(B, 3, a.size, a.size, generator=torch.Generator().manual_seed(1)).to(dev)
    Y = fwd(X)
    say(f"probe_batch_slots: {a.model} {a.precision}, batch {B} of {a.size} x {a.size}, max |logit| {float(Y.abs().max()):.3e}; "
        f"max |difference| per original window 0 .. {B - 1}")
    line("the same batch again", fwd(X), Y)
    rotated = [*range(1, B), 0]
    perms = {"swap slots 0 and 1": [1, 0, *range(2, B)], f"swap slots 0 and {B - 1}": [B - 1, *range(1, B - 1), 0],
             "rotate by one": rotated, f"rotate by {B // 2}": [*range(B // 2, B), *range(B // 2)],
             "a seeded random permutation": torch.randperm(B, generator=torch.Generator().manual_seed(2)).tolist()}
    Yrot = None
    for name, perm in perms.items():
        p = torch.tensor(perm).to(dev)
        Yp = fwd(X[p])[torch.argsort(p)]
        if perm == rotated:
            Yrot = Yp
        line(name, Yp, Y)
    mid = B // 2
    Xz = torch.zeros_like(X)
    Xz[0] = X[mid]
    line(f"window {mid} alone in slot 0", fwd(Xz)[0:1], Y[mid:mid + 1])
    Xz = torch.zeros_like(X)
    Xz[mid] = X[mid]
    line(f"window {mid} alone in its slot", fwd(Xz)[mid:mid + 1], Y[mid:mid + 1])
    Xz = X.clone()
    Xz[mid] = 0
    keep = [i for i in range(B) if i != mid]
    line(f"window {mid} zeroed, the {B - 1} others", fwd(Xz)[keep], Y[keep])

    if a.precision == "bf16":
        net.set_precision("fp32")
        R = fwd(X)
        say(f"against the fp32 kernels with the same weights (max |logit| {float(R.abs().max()):.3e}): max |bf16 - fp32|, mean |bf16 - fp32|")

        def err(name, got, want):
            d = (got - want).abs()
            say(f"  {name + ':':44s} max {float(d.max()):.3e}  mean {float(d.mean()):.3e}")
        err("window 0 in slot 0 (natural order)", Y[0], R[0])
        err(f"window 0 in slot {B - 1} (rotated by one)", Yrot[0], R[0])
        err(f"window {B - 1} in slot {B - 1} (natural order)", Y[B - 1], R[B - 1])
        err(f"window {B - 1} in slot {B - 2} (rotated by one)", Yrot[B - 1], R[B - 1])
        err(f"windows 1 .. {B - 2} in their slots", Y[1:B - 1], R[1:B - 1])
    torch.cuda.synchronize()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
