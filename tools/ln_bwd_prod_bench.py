#!/usr/bin/env python
"""du_layernorm_bwd_prod (csrc/norm_gemm.hip) against the two kernels it replaces -- the data-gradient product ops.mm(G, Wt) followed by
du_layernorm_bwd -- at the adapter's shapes of a dinounet_l 512^2 batch-8 step: 43008 x 1024 rows, K = 192 (query_norm -> offsets | weights)
and K = 256 (ffn_norm -> fc1), with the residual gradient.  Times are per call, from a replayed graph of six calls that rotate over three
operand sets (1 GB: nothing is served by the 256 MB Infinity Cache from the call before).  Bytes = x, G, dres read once and dx written
once (the fused kernel's algorithmic traffic; the unfused pair moves 2 x rows x D x 2 more); FLOPs = the product's 2 rows D K.
Roofs: 8 TB/s, 2.5 PFLOP/s.
usage: python tools/ln_bwd_prod_bench.py [rounds]"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from dinounet_amd import _lib, ops  # noqa: E402

dev = torch.device("cuda", 0)
bf = torch.bfloat16
D = 1024
PEAK_BW, PEAK_FL = 8e12, 2.5e15


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def timeit(fn, rounds, calls=6):
    for i in range(3):
        fn(i)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with ops.capture(g):
        for i in range(calls):
            fn(i)
    ts = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); g.replay(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / calls * 1e3)
    return sorted(ts)[len(ts) // 2]


def main(rounds):
    L = _lib.lib()
    print(f"{'rows':>6} {'K':>4} | {'mm us':>7} {'ln_bwd us':>9} {'pair us':>8} | {'fused us':>8} {'TB/s':>5} {'of 8':>5} {'TF/s':>6} {'of 2500':>7} | {'x pair':>6}")
    for rows, K in [(43008, 192), (43008, 256), (8192, 256)]:
        sets = []
        for s in range(3):
            x = (torch.randn(rows, D, device=dev) * 1.5 + 0.3).to(bf)
            w, b = 1 + 0.1 * torch.randn(D, device=dev), 0.1 * torch.randn(D, device=dev)
            _, mean, rstd = ops.layernorm_raw(x, w, b, 1e-6, bf, want_stats=True)
            sets.append(dict(x=x, w=w, mean=mean, rstd=rstd, G=torch.randn(rows, K, device=dev).to(bf), dres=torch.randn(rows, D, device=dev).to(bf),
                             dx=torch.empty(rows, D, device=dev, dtype=bf), dy=torch.empty(rows, D, device=dev, dtype=bf),
                             dwdb=torch.empty(2, D, device=dev)))
        Wt = (torch.randn(D, K, device=dev) / K ** 0.5).to(bf)
        plan = ops.layernorm_bwd_prod_plan(sets[0]["x"], sets[0]["G"], Wt, sets[0]["dx"], sets[0]["dres"])
        assert plan is not None
        ws_f = torch.empty(plan[4], device=dev)
        ws_u, n_u = ops._reduce_ws(bf, 1, rows, D, dev)
        st = lambda: ops._st()

        def product(i):
            t = sets[i % 3]
            ops.mm(t["G"], Wt, out=t["dy"])

        def ln_bwd(i):
            t = sets[i % 3]
            _lib.check(L.du_layernorm_bwd(1, _p(t["x"]), _p(t["dy"]), _p(t["w"]), _p(t["mean"]), _p(t["rstd"]), _p(t["dx"]), _p(t["dwdb"]), rows, D,
                                          _p(ws_u), n_u, _p(t["dres"]), st()), "du_layernorm_bwd")

        def pair(i):
            product(i); ln_bwd(i)

        def fused(i):
            t = sets[i % 3]
            _lib.check(L.du_layernorm_bwd_prod(1, _p(t["x"]), _p(t["G"]), K, _p(Wt), K, K, _p(t["w"]), _p(t["mean"]), _p(t["rstd"]), _p(t["dx"]),
                                               _p(t["dwdb"]), rows, D, _p(ws_f), plan[4], _p(t["dres"]), st()), "du_layernorm_bwd_prod")

        t_mm, t_ln, t_pair, t_f = (timeit(f, rounds) for f in (product, ln_bwd, pair, fused))
        nbytes, flops = 2.0 * (3 * rows * D + rows * K), 2.0 * rows * D * K
        bw, fl = nbytes / (t_f * 1e-6), flops / (t_f * 1e-6)
        print(f"{rows:6d} {K:4d} | {t_mm:7.1f} {t_ln:9.1f} {t_pair:8.1f} | {t_f:8.1f} {bw / 1e12:5.2f} {bw / PEAK_BW:5.2f} {fl / 1e12:6.1f} {fl / PEAK_FL:7.3f} | "
              f"{t_pair / t_f:6.2f}", flush=True)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 7)
