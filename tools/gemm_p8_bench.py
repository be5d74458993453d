#!/usr/bin/env python
"""256 x 256 multi-phase NT GEMM (csrc/gemm_p8.hip) against the 128 x 128 kernel (csrc/gemm_glds.hip): full-matrix correctness vs an
fp32 product of the same bf16 operands, a repeat-run race screen (the kernel is deterministic: any run-to-run difference is a
pipeline race), and within-process interleaved timing of the variants on the ViT shapes (random normal operands).
usage: python tools/gemm_p8_bench.py [rounds]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from dinounet_amd import _lib, ops  # noqa: E402

dev = torch.device("cuda", 0)
bf = torch.bfloat16
L = _lib.lib()


def opt(mode=-1, sched=1, group=4, debug=0):
    L.du_set_option(0, mode)
    L.du_set_option(1, sched)
    L.du_set_option(2, group)
    L.du_set_option(3, debug)


def run(x, w, od, bias=None, gamma=None, res=None, act=0):
    out = torch.empty((x.shape[0], w.shape[0]), dtype=od, device=dev)
    return ops.mm(x, w, out=out, bias=bias, gamma=gamma, residual=res, act=act)


def check():
    g = torch.Generator(device="cpu").manual_seed(1)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)
    ok = True
    cases = [(256, 256, 256, bf, 0), (512, 512, 256, torch.float32, 0), (768, 640, 384, bf, 0), (1000, 516, 512, torch.float32, 1),
             (8232, 3072, 1024, bf, 0), (8232, 1024, 1024, torch.float32, 2), (8232, 4096, 1024, bf, 3), (8232, 1024, 4096, torch.float32, 2),
             (2048, 384, 1536, bf, 0), (8192, 3072, 1024, bf, 2), (8192, 3072, 1024, torch.float32, 0), (4096, 4096, 512, bf, 0),
             (8232, 1280, 256, bf, 3), (8232, 1000, 512, torch.float32, 1),
             # persistent kernel: several tiles per workgroup with ragged last tile rows / columns, K at its lower limit, bias and GELU
             (70000, 264, 512, bf, 1), (33000, 1000, 640, bf, 3), (43008, 1024, 512, bf, 1), (5000, 136, 2048, bf, 0),
             # ... its K = 256 form (four K-steps per tile, three bias slots) and K = 384
             (43008, 1024, 256, bf, 1), (70000, 264, 256, bf, 3), (9000, 1000, 256, bf, 0), (33000, 520, 384, bf, 1)]
    for M, N, K, od, epi in cases:
        x, w = rnd(M, K).to(bf), (rnd(N, K) * 0.05).to(bf)
        bias = rnd(N) if epi else None
        gamma = rnd(N) if epi == 2 else None
        res = rnd(M, N).to(od) if epi == 2 else None
        act = 1 if epi == 3 else 0
        ref = x.float() @ w.float().t()
        if bias is not None:
            ref = ref + bias
        if act:
            ref = torch.nn.functional.gelu(ref)
        if gamma is not None:
            ref = ref * gamma
        if res is not None:
            ref = ref + res.float()
        opt(mode=0)
        y_old = run(x, w, od, bias, gamma, res, act).float()
        scale = ref.abs().max().item()
        e_old = (y_old - ref).abs().max().item() / scale
        for mode, tag in ((1, "256x256"), (2, "256x128"), (3, "256x128 4-wave"), (4, "256x128 persistent")):
            opt(mode=mode)
            y_new = run(x, w, od, bias, gamma, res, act).float()
            e_new = (y_new - ref).abs().max().item() / scale
            d = (y_new - y_old).abs().max().item() / scale
            # race screen: 30 repeats must be bit-identical
            same = True
            for it in range(30):
                y_it = run(x, w, od, bias, gamma, res, act).float()
                if not torch.equal(y_it, y_new):
                    if same:       # first mismatch: where is it?
                        bad = (y_it != y_new).nonzero()
                        tiles = sorted({(int(r) // 256, int(c) // 256) for r, c in bad[:20000].tolist()})
                        print(f"   repeat {it}: {bad.shape[0]} elements differ, rows {int(bad[:, 0].min())}..{int(bad[:, 0].max())}, "
                              f"max |diff| {(y_it - y_new).abs().max().item():.3e} (scale {scale:.2f}), tiles {tiles[:24]}", flush=True)
                    same = False
            tol = 1e-2 if od == bf else 2e-3
            good = e_new < tol and same and e_new < 2.0 * e_old + 1e-6
            ok &= good
            print(f"check {tag} M{M} N{N} K{K} {'bf16' if od == bf else 'f32 '} epi{epi}: err_new {e_new:.2e} err_old {e_old:.2e} new-old {d:.2e} "
                  f"deterministic {same} -> {'OK' if good else 'FAIL'}", flush=True)
    opt()
    return ok


def check_pairs():
    """the K-split pair kernel (mode 5): against the fp32 product, 30 bit-identical repeats, every way through the exchange (test aids: bit 3 = the
    first half leaves as if its peer had not started, bit 4 = the second half looks late), scratch state back to zero, error word clear"""
    g = torch.Generator(device="cpu").manual_seed(2)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)
    ok = True
    for M, N, K in ((8232, 1024, 4096), (8232, 1024, 1024), (8192, 1024, 2048), (4096, 2048, 1024), (4136, 1024, 1024)):
        x, w = rnd(M, K).to(bf), (rnd(N, K) * 0.05).to(bf)
        bias, gamma, res = rnd(N), rnd(N), rnd(M, N)
        ref = (x.float() @ w.float().t() + bias) * gamma + res
        scale = ref.abs().max().item()
        opt(mode=2)
        y2 = run(x, w, torch.float32, bias, gamma, res)
        outs = []
        for dbg in (0, 8, 24, 16):
            opt(mode=5, debug=dbg)
            ops.TRACK_ROUTE = True
            y = run(x, w, torch.float32, bias, gamma, res)
            ops.TRACK_ROUTE = False
            route = ops.LAST_GEMM_ROUTE
            same = all(torch.equal(run(x, w, torch.float32, bias, gamma, res), y) for _ in range(30 if dbg == 0 else 3))
            torch.cuda.synchronize()
            st = next(iter(ops._KS_SCRATCH.values()))[:131072].view(torch.int32)
            clean = int(st.abs().sum().item()) == 0
            e = (y - ref).abs().max().item() / scale
            good = route == 8 and same and clean and e < 2e-3
            ok &= good
            outs.append(y)
            print(f"check pair M{M} N{N} K{K} aid {dbg:2d}: route {route} err {e:.2e} vs 256x128 {(y - y2).abs().max().item() / scale:.2e} deterministic {same} "
                  f"state clean {clean} -> {'OK' if good else 'FAIL'}", flush=True)
        same_all = all(torch.equal(o, outs[0]) for o in outs[1:])
        ok &= same_all
        print(f"   every way through the exchange gives the same bits: {same_all}", flush=True)
    opt()
    return ok


def time_variants(rounds):
    g = torch.Generator(device="cpu").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev).to(bf)
    variants = [("old128", dict(mode=0)), ("256x256", dict(mode=1)), ("256 nostore", dict(mode=1, debug=1)), ("256 noepi", dict(mode=1, debug=2)),
                ("256x128", dict(mode=2)), ("128 nostore", dict(mode=2, debug=1)), ("128 noepi", dict(mode=2, debug=2)), ("128 nopre", dict(mode=2, debug=4)),
                ("4wave", dict(mode=3)), ("4w noepi", dict(mode=3, debug=2)), ("persist", dict(mode=4)), ("pp nostore", dict(mode=4, debug=1)), 
                ("auto", dict(mode=-1))]
    if "--quick" in sys.argv:
        variants = [v for v in variants if v[0] in ("256x256", "256x128", "256 noepi", "128 noepi", "persist", "pp nostore", "auto")]
    shapes = [(8232, 3072, 1024, bf, "qkv"), (8232, 4096, 1024, bf, "fc1"), (8232, 1024, 4096, torch.float32, "fc2"),
              (8232, 1024, 1024, torch.float32, "proj"), (8192, 3072, 1024, bf, "qkv8192"), (8192, 4096, 1024, bf, "fc1_8192"),
              (4096, 4096, 4096, bf, "4096^3"), (8192, 8192, 8192, bf, "8192^3"), (8232, 2304, 768, bf, "qkv_b"), (8232, 3072, 768, bf, "fc1_b"),
              (43008, 1024, 512, bf, "adapter"), (43008, 1024, 256, bf, "adapterK256"), (131072, 512, 1024, bf, "fapm"),
              (16644, 12288, 4096, bf, "7b_qkv"), (16644, 4096, 4096, torch.float32, "7b_proj"),
              (43008, 192, 1024, bf, "msda_offs"), (43008, 256, 1024, bf, "msda_vproj"), (43008, 512, 1024, bf, "adapter_n512")]
    if "--narrow" in sys.argv:
        shapes = shapes[-3:]
    if "--residual" in sys.argv:     # the adapter's products into the fp32 query stream (LayerScale + residual epilogue: 350 MB of epilogue traffic)
        shapes = [(43008, 1024, 256, torch.float32, "ffn_fc2_res"), (43008, 1024, 512, torch.float32, "oproj_res"), (8232, 1024, 1024, torch.float32, "proj"),
                  (8232, 1024, 4096, torch.float32, "fc2"), (8192, 1024, 1024, torch.float32, "proj8192")]
        variants = [v for v in variants if v[0] in ("256x256", "256 noepi", "256x128", "128 noepi", "4wave", "4w noepi", "auto")]
    if "--kspair" in sys.argv:       # round 6: fp32-result products with <= 128 tiles of 256 x 256 as K-split pairs (du_set_option key 16 / mode 5)
        shapes = [(8232, 1024, 4096, torch.float32, "fc2"), (8232, 1024, 1024, torch.float32, "proj"), (8192, 1024, 4096, torch.float32, "fc2_8192"),
                  (8192, 1024, 1024, torch.float32, "proj8192"), (4096, 2048, 2048, torch.float32, "sq_128t"), (8232, 768, 3072, torch.float32, "fc2_b")]
        variants = [v for v in variants if v[0] in ("256x256", "256 noepi", "256x128", "128 noepi", "auto")] + [
            ("pair", dict(mode=5)), ("pair noepi", dict(mode=5, debug=2))]
    bf16res = "--bf16res" in sys.argv
    if bf16res:      # round 6: the adapter's products into the bf16 query stream as the model issues them (bias + bf16 residual, fc2: + DropPath scale)
        shapes = [(43008, 1024, 256, bf, "ffn_fc2_res"), (43008, 1024, 512, bf, "oproj_res"), (43008, 1024, 1024, bf, "k1024_res"),
                  (21504, 1024, 256, bf, "fc2_res_b4"), (43008, 768, 384, bf, "b_oproj_res"), (32768, 4096, 1024, bf, "convt_up")]
        variants = [v for v in variants if v[0] in ("256x256", "256x128", "persist", "auto")] + [("auto r5", dict(mode=-1))]
    print(f"{'shape':>34} " + " ".join(f"{n:>11}" for n, _ in variants) + "   (us median | TF/s of `auto` = what ships, fraction of 2.5 PF | best complete variant)")
    import time
    for M, N, K, od, name in shapes:
        x, w = rnd(M, K), rnd(N, K)
        out = torch.empty((M, N), dtype=od, device=dev)
        # the epilogues the ViT uses: bias (+ GELU for fc1) for bf16 results, bias + LayerScale + in-place fp32 residual otherwise
        kwargs = dict(bias=torch.randn(N, device=dev))
        if od == bf and N >= 4096:
            kwargs["act"] = 1
        if od != bf:
            kwargs.update(gamma=torch.randn(N, device=dev), residual=out)
        if bf16res:
            kwargs.update(residual=torch.randn(M, N, device=dev).to(bf))
            if name.startswith("f"):      # ConvFFN fc2: DropPath's per-sample scale (5376 rows per sample)
                kwargs.update(row_scale=(torch.arange(M // 5376, device=dev) % 3 != 0).float() / 0.7, rs_rows=5376)
        call = lambda: ops.mm(x, w, out=out, **kwargs)
        if bf16res and name == "convt_up":        # the adapter's `up` + c1: pixel-shuffle store, residual in the output layout
            out = torch.empty((4 * M, N // 4), dtype=od, device=dev)
            cres, cbias = torch.randn(4 * M, N // 4, device=dev).to(bf), torch.randn(N, device=dev)
            call = lambda: ops.gemm_raw(dtype=_lib.DU_BF16, out_dtype=_lib.DU_BF16, a_mode=ops.PLAIN_ROW, b_mode=ops.PLAIN_ROW, M=M, N=N, K=K,
                                        A=x.data_ptr(), lda=K, B=w.data_ptr(), ldb=K, Cmat=out.data_ptr(), ldc=N // 4, bias=cbias.data_ptr(),
                                        residual=cres.data_ptr(), ldr=N // 4, store_mode=ops.STORE_PIXEL_SHUFFLE2, ps=(64, 64, N // 4))
        ts = {n: [] for n, _ in variants}
        graphs = {}
        for n, kw in variants:                     # warm-up, then capture 10 back-to-back launches per variant (no host time in the number)
            opt(**kw)
            L.du_set_option(14, 0 if n == "auto r5" else 1)
            call()
            torch.cuda.synchronize()
            g_ = torch.cuda.CUDAGraph()
            with ops.capture(g_):
                for _ in range(10):
                    call()
            graphs[n] = g_
        torch.cuda.synchronize()
        t0 = time.time()                            # warm the clocks: a cold chip runs the first variants ~10 % slower than the last
        while time.time() - t0 < 0.3:
            graphs[variants[0][0]].replay()
        torch.cuda.synchronize()
        for _ in range(rounds):
            for n, kw in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                graphs[n].replay()
                e1.record()
                torch.cuda.synchronize()
                ts[n].append(e0.elapsed_time(e1) / 10 * 1e3)
        med = {n: sorted(v)[len(v) // 2] for n, v in ts.items()}
        # "best" = the fastest COMPLETE variant (the nostore / noepi / nopre builds skip work: they are ablations, not performance figures)
        complete = {n: t for (n, kw), t in zip(variants, [med[n] for n, _ in variants]) if not kw.get("debug")}
        bn = min(complete, key=complete.get)
        fl = 2.0 * M * N * K
        print(f"{name:>10} M{M:>6} N{N:>5} K{K:>5} " + " ".join(f"{med[n]:11.1f}" for n, _ in variants)
              + f"   | auto {fl / med['auto'] / 1e6:7.1f} TF/s ({fl / med['auto'] / 1e6 / 2500:.3f}) | best {bn} {fl / complete[bn] / 1e6:7.1f}", flush=True)
    opt()
    L.du_set_option(14, 1)


if __name__ == "__main__":
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    ok = check_pairs() if "--kspair" in sys.argv else (True if "--narrow" in sys.argv else check())
    if rounds > 0:
        time_variants(rounds)
    print("CHECK", "PASSED" if ok else "FAILED")
    sys.exit(0 if ok else 1)
