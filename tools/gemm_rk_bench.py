#!/usr/bin/env python
"""Resident-weights streaming GEMM for short contractions (csrc/gemm_rk.hip) against the kernels it replaces (du_set_option(12, 0): the
128 x 128 direct-to-LDS kernel, the generic bf16 engine, the multi-phase kernels), on the shapes of a dinounet_l train step: full-matrix
check against an fp32 product of the same bf16 operands (and against the old path), repeat-run determinism, interleaved timing of
hipGraph-captured launches, achieved algorithmic GB/s = (M K + N K + M N) * 2 bytes / time.

usage: python tools/gemm_rk_bench.py [rounds]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from dinounet_amd import _lib, ops  # noqa: E402

dev = torch.device("cuda", 0)
bf = torch.bfloat16
L = _lib.lib()
g = torch.Generator(device="cpu").manual_seed(0)
rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(dev)


def cases():
    out = []
    # plain NT (1x1 projections; the MSDA offsets + weights data gradient at K = 192; K = 256 behind du_set_option(12, 2))
    for M, N, K in [(131072, 1024, 64), (524288, 128, 64), (131072, 256, 128), (32768, 256, 64), (32768, 1024, 128), (131072, 256, 64),
                    (8192, 128, 128), (43008, 1024, 192), (43008, 1024, 256), (131072, 512, 256), (5000, 96, 64)]:
        x, w, b = rnd(M, K).to(bf), rnd(N, K, scale=K ** -0.5).to(bf), rnd(N)
        ref = lambda x=x, w=w, b=b: x.float() @ w.float().t() + b
        out.append((f"nt M{M} N{N} K{K}", lambda x=x, w=w, b=b: ops.mm(x, w, bias=b), ref, 2.0 * (M * K + N * K + M * N), K == 256))
    # data-gradient form: W given as [K][N]
    for M, N, K in [(131072, 256, 32), (131072, 32, 256), (524288, 64, 32)]:
        dy, w = rnd(M, K).to(bf), rnd(K, N, scale=K ** -0.5).to(bf)
        out.append((f"dgrad M{M} N{N} K{K}", lambda dy=dy, w=w: ops.mm_dgrad(dy, w), lambda dy=dy, w=w: dy.float() @ w.float(),
                    2.0 * (M * K + N * K + M * N), K == 256))
    # ConvTranspose2d k2 s2: forward = pixel-shuffle store, data gradient = 2 x 2 patch gather
    for B, H, W, Ci, Co in [(8, 256, 256, 32, 32), (8, 256, 256, 64, 32), (8, 128, 128, 128, 64), (8, 128, 128, 64, 64), (2, 64, 64, 16, 32)]:
        x = rnd(B, H, W, Ci).to(bf)
        w, b = rnd(Ci, Co, 2, 2, scale=Ci ** -0.5), rnd(Co)
        dy = rnd(B, 2 * H, 2 * W, Co).to(bf)

        def fwd(x=x, w=w, b=b):
            return ops.conv_transpose2x2(x, w, b)

        def fwd_ref(x=x, w=w, b=b):
            return F.conv_transpose2d(x.float().permute(0, 3, 1, 2), w.to(bf).float(), b, stride=2).permute(0, 2, 3, 1)

        M, N, K = B * H * W, 4 * Co, Ci
        out.append((f"convT fwd {Ci}->{Co} @{H}", fwd, fwd_ref, 2.0 * (M * K + N * K + M * N), False))
        if 4 * Co <= 256:
            xg = x.clone().requires_grad_(True)

            def bwd(xg=xg, w=w, b=b, dy=dy):
                xg.grad = None
                ops.conv_transpose2x2(xg, w, b).backward(dy)
                return xg.grad

            def bwd_ref(x=x, w=w, dy=dy):
                return F.conv2d(dy.float().permute(0, 3, 1, 2), w.to(bf).float().permute(0, 1, 2, 3), stride=2).permute(0, 2, 3, 1)

            out.append((f"convT dgrad {Co}->{Ci} @{H}", bwd, bwd_ref, 2.0 * (M * 4 * Co + Ci * 4 * Co + M * Ci), 4 * Co == 256))
    return out


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    ok = True
    print(f"{'case':>34} {'old us':>9} {'new us':>9} {'speedup':>8} {'new GB/s':>9} {'of 8 TB/s':>9}   err_new  err_old  new-vs-old  deterministic")
    for name, fn, ref, nbytes, k256 in cases():
        mode_new = 3          # wherever legal: the table shows where it pays (the library's default rule takes the winners)
        r = ref().float()
        scale = r.abs().max().item()
        L.du_set_option(12, 0)
        y_old = fn().float()
        L.du_set_option(12, mode_new)
        y_new = fn().float()
        same = all(torch.equal(fn().float(), y_new) for _ in range(8))
        e_new, e_old = (y_new - r).abs().max().item() / scale, (y_old - r).abs().max().item() / scale
        d = (y_new - y_old).abs().max().item() / scale
        good = e_new < 1e-2 and same and e_new < 2.0 * e_old + 1e-6
        ok &= good
        graphs = {}
        timed = "dgrad" not in name or name.startswith("dgrad")       # (the ConvT dgrad case times forward + backward: reported, not compared)
        for tag, mode in (("old", 0), ("new", mode_new)):
            L.du_set_option(12, mode)
            fn()
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with ops.capture(gr):
                for _ in range(5):
                    fn()
            graphs[tag] = gr
        t0 = time.time()
        while time.time() - t0 < 0.2:
            graphs["old"].replay()
        torch.cuda.synchronize()
        ts = {"old": [], "new": []}
        for _ in range(rounds):
            for tag in ("old", "new"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                graphs[tag].replay()
                e1.record()
                torch.cuda.synchronize()
                ts[tag].append(e0.elapsed_time(e1) / 5 * 1e3)
        med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
        gbs = nbytes / med["new"] / 1e3
        print(f"{name:>34} {med['old']:9.1f} {med['new']:9.1f} {med['old'] / med['new']:8.2f} {gbs:9.0f} {gbs / 8000:9.3f}   {e_new:.2e} {e_old:.2e} {d:.2e}  {same}"
              f"{'' if good else '  <-- FAIL'}{'' if timed else '  (forward + backward)'}", flush=True)
    L.du_set_option(12, 1)
    print("CHECK", "PASSED" if ok else "FAILED")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
