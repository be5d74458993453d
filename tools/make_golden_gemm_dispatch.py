"""Writes tests/golden/gemm_dispatch.npz: du_gemm's dispatch over a sweep of argument sets, pinned from the commit BEFORE du_gemm_plan.

Two tables over the same rows (tests/test_cpu_gemm_plan.py holds du_gemm_plan_describe to both):
  reported -- what that library's du_gemm_route / du_gemm_ws_elems / du_gemm_ks_ws_bytes answered;
  executed -- what its du_gemm launched: from a recorder build of the same commit, in which every launcher (launch_p8, launch_pp,
              launch_p4, launch_p8ks, launch_p8_tn, rk_launch, gemm_glds.hip's launch, launch_skinny_fused, the partial + finish pair,
              both launch_cfg engines) appends (launcher, M, tail_rows, splits, gather) to a list and returns DU_OK.  The list is read
              back through `int du_rec_read(int* out)` (5 ints per launch, returns the count and clears it).
Both libraries are host-only builds with -DDU_DEBUG_KNOBS (the environment knobs are read once per process: one child process per knob).
Nothing is dereferenced: the operands are fake addresses.

  python tools/make_golden_gemm_dispatch.py --reported libparent.so --executed librecorder.so [--out tests/golden/gemm_dispatch.npz]
  python tools/make_golden_gemm_dispatch.py --check libnew.so      # a -DDU_DEBUG_KNOBS build of the current tree against the fixture, environment rows included
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dinounet_amd._lib import (ACT_GELU, ACT_SWIGLU, DU_BF16, DU_F32, IM2COL_COL, IM2COL_ROW, PLAIN_COL, PLAIN_ROW, STORE_MSDA_PREP,  # noqa: E402
                               STORE_PIXEL_SHUFFLE2, STORE_QKV_HEADS, STORE_QKV_ROPE, STORE_SLABS, GemmArgs)

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "gemm_dispatch.npz")

# integer columns of a row: the du_gemm_args fields (geom flattened), the du_set_option values and the environment knob
ARG_FIELDS = ["dtype", "out_dtype", "a_mode", "b_mode", "M", "N", "K", "A", "lda", "a_batch_stride", "B", "ldb", "b_batch_stride", "C", "ldc",
              "c_batch_stride", "batch", "split_k", "bias", "act", "gamma", "row_scale", "rs_rows", "residual", "ldr", "store_mode", "ps_H", "ps_W",
              "ps_C", "ws", "ws_elems", "rope_sin", "rope_cos", "rope_prefix", "a_colsum", "b_colsum", "C2", "ks_ws", "ks_ws_bytes"]
GEOM_FIELDS = ["p2", "ld2", "C1", "Hi", "Wi", "C", "KH", "KW", "stride", "pad", "Ho", "Wo", "transposed"]
OPT_DEFAULTS = {0: -1, 5: 1, 9: 1, 10: 1, 12: 1, 14: 1, 15: 0, 16: 0, 17: 1}
OPT_KEYS = sorted(OPT_DEFAULTS)
ENVS = ["", "DU_GEMM_GENERIC=1", "DU_GEMM_NO_GLDS=1", "DU_GEMM_NO_RAGGED_SPLIT=1", "DU_P8_NO_TAIL=1", "DU_SKINNY_NO_FUSE=1", "DU_SKINNY_FUSE_KMAX=1024"]
COLUMNS = ARG_FIELDS + ["geom." + f for f in GEOM_FIELDS] + [f"opt{k}" for k in OPT_KEYS] + ["env"]
# executed / described columns
PLAN = ["rc", "family", "variant", "gather", "tail_rows", "tail_form", "tn_splits"]
TAIL_NONE, TAIL_RIDES, TAIL_SKINNY_FUSED, TAIL_SKINNY_PAIR, TAIL_TILE_ENGINE = 0, 1, 2, 3, 4

PA, PB, PC, PBIAS, PGAMMA, PRS, PRES, PWS, PKS, PSIN, PCOS, PC2, PACS, PBCS = (0x10000000 * (i + 1) for i in range(14))   # fake addresses


def row(name, M, N, K, am=PLAIN_ROW, bm=PLAIN_ROW, dt=DU_BF16, od=DU_BF16, ws=True, ks=True, opts=None, env=0, geom=None, **kw):
    r = dict.fromkeys(COLUMNS, 0)
    r.update(dtype=dt, out_dtype=od, a_mode=am, b_mode=bm, M=M, N=N, K=K, A=PA, B=PB, C=PC, batch=1, split_k=1, ldc=N,
             lda=(K if am in (PLAIN_ROW, IM2COL_ROW) else M), ldb=(K if bm == PLAIN_ROW else N))
    if ws:
        r.update(ws=PWS, ws_elems=1 << 26)
    if ks:
        r.update(ks_ws=PKS, ks_ws_bytes=1 << 30)
    for k, v in OPT_DEFAULTS.items():
        r[f"opt{k}"] = v
    for k, v in (opts or {}).items():
        r[f"opt{k}"] = v
    for k, v in (geom or {}).items():
        r["geom." + k] = v
    r["env"] = env
    alpha = kw.pop("alpha", 1.0)
    for k, v in kw.items():
        assert k in r, k
        r[k] = v
    tag = "".join(f" {k}={v}" for k, v in sorted({**kw, **({'geom': 1} if geom else {})}.items()))
    otag = "".join(f" o{k}={v}" for k, v in sorted((opts or {}).items()))
    r["_name"] = f"{name} {M}x{N}x{K} m{am}{bm} d{dt}{od} ws{int(ws)} ks{int(ks)}{tag}{otag}" + (f" a{alpha}" if alpha != 1.0 else "") + (f" [{ENVS[env]}]" if env else "")
    r["_alpha"] = alpha
    return r


def convt_geom(C_, Ho, Wo):
    return dict(Hi=2 * Ho, Wi=2 * Wo, C=C_, C1=C_, KH=2, KW=2, stride=2, pad=0, Ho=Ho, Wo=Wo, transposed=0)


def epilogue_variants(M):
    rs = 256 if M % 256 == 0 else (M // 8 if M % 8 == 0 else M)
    return [dict(), dict(bias=PBIAS), dict(bias=PBIAS, act=ACT_GELU), dict(bias=PBIAS, act=ACT_SWIGLU), dict(residual=PRES, ldr=None),
            dict(residual=PRES, ldr=None, row_scale=PRS, rs_rows=rs), dict(row_scale=PRS, rs_rows=rs), dict(gamma=PGAMMA),
            dict(bias=PBIAS, gamma=PGAMMA, residual=PRES, ldr=None), dict(act=ACT_SWIGLU), dict(alpha=0.5)]


GRID_M = [64, 256, 1024, 1064, 4096, 8192, 8232, 43008, 131072]
GRID_N = [32, 96, 128, 192, 256, 512, 1024, 3072, 4096]
GRID_K = [32, 64, 128, 192, 256, 384, 512, 768, 1024, 2048, 4096]
SMALL = [(M, N, K) for M in (256, 1064, 8232, 43008) for N in (128, 3072) for K in (256, 1024, 4096)]


def ragged(M):
    return 0 < M % 128 <= 64


def nt_rows(env=0, full=True):
    """plain NT products: the shape grid, the epilogue terms, the scratch present / absent"""
    rows = []
    grid = [(M, N, K) for M in GRID_M for N in GRID_N for K in GRID_K] if full else SMALL
    for M, N, K in grid:
        rows.append(row("nt", M, N, K, env=env))
        if ragged(M):
            rows.append(row("nt", M, N, K, ws=False, ks=False, env=env))
        if M in (1064, 8192, 8232, 43008) and (full or K >= 1024):
            rows.append(row("nt", M, N, K, od=DU_F32, env=env))
    for M, N, K in SMALL:
        for i, e in enumerate(epilogue_variants(M)):
            e = dict(e)
            if "ldr" in e:
                e["ldr"] = N
            if env and i not in (2, 3, 5):
                continue
            rows.append(row("epi", M, N, K, env=env, **e))
            if ragged(M):
                rows.append(row("epi", M, N, K, ws=False, ks=False, env=env, **e))
            if not env:
                rows.append(row("epi", M, N, K, od=DU_F32, env=env, **e))
    return rows


def workload_rows(env=0):
    """the shapes of tests/test_cpu_oracle_and_boundary.py::test_gemm_dispatch_host_logic_without_gpu (a dinounet_l 512^2 batch-8 step)"""
    rows = []
    for ws in (True, False):
        w = dict(ws=ws, ks=ws, env=env)
        for M, N, K in [(8232, 3072, 1024), (8232, 2304, 768), (8232, 4096, 1024), (4096, 4096, 4096), (131072, 512, 1024), (8192, 3072, 1024),
                        (43008, 1024, 192), (131072, 1024, 64), (524288, 128, 64), (32768, 256, 64), (2048, 256, 256), (43008, 1024, 256),
                        (131072, 512, 256), (43008, 1024, 512), (43008, 192, 1024)]:
            rows.append(row("wl", M, N, K, **w))
        rows.append(row("wl", 8232, 4096, 1024, act=ACT_GELU, **w))
        rows.append(row("wl", 8232, 1024, 4096, od=DU_F32, **w))
        rows.append(row("wl", 8232, 1024, 1024, od=DU_F32, **w))
        rows.append(row("wl", 8232, 3072, 1024, dt=DU_F32, od=DU_F32, **w))
    return rows


def mode_rows(env=0):
    """the other operand-mode pairs: data gradients (ROW x COL), weight gradients (COL x COL, split-K), the ConvTranspose k2s2 gathers, 3x3 s2"""
    rows = []
    for M, N, K in SMALL:
        rows.append(row("nn", M, N, K, bm=PLAIN_COL, env=env))
        rows.append(row("nn", M, N, K, bm=PLAIN_COL, od=DU_F32, env=env))
        rows.append(row("f32", M, N, K, dt=DU_F32, od=DU_F32, env=env))
        rows.append(row("f32", M, N, K, dt=DU_F32, od=DU_BF16, env=env))
        rows.append(row("badpair", M, N, K, am=PLAIN_COL, bm=PLAIN_ROW, env=env))
    for M, N, K in [(1024, 512, 43008), (512, 1024, 131072), (256, 256, 8192), (1024, 1024, 8232), (128, 1024, 43008), (1024, 4096, 8192),
                    (3072, 1024, 8232), (64, 64, 131072), (512, 512, 2048), (1024, 1024, 384)]:
        for split in (1, 4, 16):
            for opts in (None, {5: 0}, {5: 2}, {0: 0}):
                rows.append(row("tn", M, N, K, am=PLAIN_COL, bm=PLAIN_COL, od=DU_F32, split_k=split, opts=opts, env=env))
            rows.append(row("tn", M, N, K, am=PLAIN_COL, bm=PLAIN_COL, od=DU_F32, split_k=split, row_scale=PRS, rs_rows=K // 8 if K % 512 == 0 else 1029, env=env))
            rows.append(row("tn", M, N, K, am=PLAIN_COL, bm=PLAIN_COL, od=DU_F32, split_k=split, a_colsum=PACS, env=env))
            rows.append(row("tn", M, N, K, am=PLAIN_COL, bm=PLAIN_COL, od=DU_F32, split_k=split, store_mode=STORE_SLABS, env=env))
            rows.append(row("tn", M, N, K, am=PLAIN_COL, bm=PLAIN_COL, od=DU_F32, split_k=split, store_mode=STORE_SLABS, batch=2, env=env))
            rows.append(row("tn", M, N, K, am=PLAIN_COL, bm=PLAIN_COL, od=DU_BF16, split_k=split, env=env))
            rows.append(row("tn", M, N, K, am=PLAIN_COL, bm=PLAIN_COL, od=DU_F32, split_k=split, bias=PBIAS, env=env))
            rows.append(row("tn", M, N, K, am=PLAIN_COL, bm=PLAIN_COL, od=DU_F32, split_k=split, a_colsum=PACS, C=PC + 4, env=env))
            rows.append(row("tn", M, N, K, am=PLAIN_COL, bm=PLAIN_COL, od=DU_F32, split_k=split, row_scale=PRS, rs_rows=K // 8 if K % 512 == 0 else 1029, c_batch_stride=2, env=env))
    # ConvTranspose2d k2 s2: data gradient (A rows gathered from dY) and weight gradient (B gathered from dY), batch 8
    for Cc, Ho in [(1024, 64), (256, 64), (64, 128), (128, 32), (96, 64), (16, 256)]:
        pix = 8 * Ho * Ho
        g = convt_geom(Cc, Ho, Ho)
        for Cin in (128, 1024):
            for opts in (None, {0: 0}, {0: 1}, {5: 0}, {12: 0}, {12: 3}):
                rows.append(row("convt_dgrad", pix, Cin, 4 * Cc, am=IM2COL_ROW, lda=Cc, geom=g, opts=opts, env=env))
            rows.append(row("convt_dgrad", pix, Cin, 4 * Cc, am=IM2COL_ROW, lda=Cc, geom=g, bias=PBIAS, act=ACT_GELU, env=env))
            rows.append(row("convt_dgrad_badK", pix, Cin, 2 * Cc, am=IM2COL_ROW, lda=Cc, geom=g, env=env))
            for split in (1, 4, 16):
                for opts in (None, {5: 0}, {5: 2}):
                    rows.append(row("convt_wgrad", Cin, 4 * Cc, pix, am=PLAIN_COL, bm=IM2COL_COL, od=DU_F32, split_k=split, lda=Cin, ldb=Cc, geom=g, opts=opts, env=env))
                rows.append(row("convt_wgrad", Cin, 4 * Cc, pix, am=PLAIN_COL, bm=IM2COL_COL, od=DU_F32, split_k=split, lda=Cin, ldb=Cc, geom=g, b_colsum=PBCS, env=env))
                rows.append(row("convt_wgrad", Cin, 4 * Cc, pix, am=PLAIN_COL, bm=IM2COL_COL, od=DU_F32, split_k=split, lda=Cin, ldb=Cc, geom=g, a_colsum=PACS, b_colsum=PBCS, env=env))
    # 3 x 3 stride 2 (the stem / down convolutions): forward as an im2col NT product, weight gradient with the gathered B
    for Cc, Hi in [(64, 512), (128, 256), (32, 512)]:
        Ho = Hi // 2
        g3 = dict(Hi=Hi, Wi=Hi, C=Cc, C1=Cc, KH=3, KW=3, stride=2, pad=1, Ho=Ho, Wo=Ho, transposed=0)
        pix = 8 * Ho * Ho
        for Cout in (64, 128):
            rows.append(row("conv3s2", pix, Cout, 9 * Cc, am=IM2COL_ROW, lda=Cc, geom=g3, bias=PBIAS, env=env))
            rows.append(row("conv3s2", pix, Cout, 9 * Cc, am=IM2COL_ROW, lda=Cc, geom=g3, od=DU_F32, env=env))
            for split in (1, 64):
                rows.append(row("conv3s2_wgrad", Cout, 9 * Cc, pix, am=PLAIN_COL, bm=IM2COL_COL, od=DU_F32, split_k=split, lda=Cout, ldb=Cc, geom=g3, env=env))
                rows.append(row("conv3s2_wgrad", Cout, 9 * Cc, pix, am=PLAIN_COL, bm=IM2COL_COL, od=DU_F32, split_k=split, lda=Cout, ldb=Cc, geom=g3, b_colsum=PBCS, env=env))
        rows.append(row("conv3s2_badgeom", pix, 64, 9 * Cc, am=IM2COL_ROW, lda=Cc, geom=dict(g3, KH=0), env=env))
    return rows


def store_rows(env=0):
    """the fused-store modes, each with valid fields and with one invalid field"""
    rows = []
    for ws in (True, False):
        w = dict(ws=ws, ks=ws, env=env)
        # ConvTranspose2d k2 s2 forward (+ skip): pixel-shuffle store
        for Hh, Cout, K in [(64, 256, 1024), (64, 128, 256), (128, 32, 128), (32, 1024, 1024), (64, 96, 512)]:
            M = 8 * Hh * Hh
            ps = dict(store_mode=STORE_PIXEL_SHUFFLE2, ps_H=Hh, ps_W=Hh, ps_C=Cout, ldc=Cout)
            rows.append(row("ps2", M, 4 * Cout, K, bias=PBIAS, **ps, **w))
            rows.append(row("ps2", M, 4 * Cout, K, bias=PBIAS, residual=PRES, ldr=Cout, **ps, **w))
            rows.append(row("ps2", M, 4 * Cout, K, bias=PBIAS, residual=PRES, ldr=Cout, od=DU_F32, **ps, **w))
            rows.append(row("ps2_badC", M, 4 * Cout, K, **dict(ps, ps_C=0), **w))
            rows.append(row("ps2_badN", M, 2 * Cout, K, **ps, **w))
            rows.append(row("ps2_badM", M + 8, 4 * Cout, K, **ps, **w))
            rows.append(row("ps2_swiglu", M, 4 * Cout, K, act=ACT_SWIGLU, **ps, **w))
        # qkv projections of the ViT: B = 8 images of 1029 tokens (5 prefix + 32 x 32), 16 heads of 64
        for M, K, Hd in [(8192, 1024, 16), (8232, 1024, 16), (1024, 1024, 16), (1064, 256, 16), (1064, 384, 16), (8232, 768, 12), (8200, 1024, 16), (8392, 1024, 16), (8232, 8192, 16)]:
            q = dict(store_mode=STORE_QKV_HEADS, ps_H=1029, ps_W=1032, ps_C=Hd, ldc=8 * Hd * 1032 * 64, bias=PBIAS)
            for opts in (None, {0: 0}, {0: 2}, {10: 0}, {15: 1}):
                rows.append(row("qkv_heads", M, 3 * Hd * 64, K, opts=opts, **q, **w))
            rows.append(row("qkv_heads_badC", M, 3 * Hd * 64, K, **dict(q, ps_C=0), **w))
            rows.append(row("qkv_heads_f32", M, 3 * Hd * 64, K, od=DU_F32, **q, **w))
            rows.append(row("qkv_heads_split", M, 3 * Hd * 64, K, split_k=4, od=DU_F32, **q, **w))
            rope = dict(q, store_mode=STORE_QKV_ROPE, rope_sin=PSIN, rope_cos=PCOS, rope_prefix=5)
            gr = dict(Hi=32, Wi=32)
            for opts in (None, {0: 0}, {0: 2}, {0: 4}, {10: 0}, {10: 2}, {9: 2}):
                rows.append(row("qkv_rope", M, 3 * Hd * 64, K, geom=gr, opts=opts, **rope, **w))
            rows.append(row("qkv_rope_nogrid", M, 3 * Hd * 64, K, **rope, **w))
            rows.append(row("qkv_rope_nosin", M, 3 * Hd * 64, K, geom=gr, **dict(rope, rope_sin=0), **w))
            rows.append(row("qkv_rope_nt_cols", M, 3 * Hd * 64, K, geom=gr, bm=PLAIN_COL, **rope, **w))
        # MSDeformAttn's offsets | weights product
        for M, N, K in [(43008, 192, 1024), (43008, 96, 256), (8232, 192, 1024), (1024, 192, 1024), (43008, 192, 192), (43008, 264, 1024)]:
            ms = dict(store_mode=STORE_MSDA_PREP, od=DU_F32, ps_H=64, ps_W=64, ps_C=5376, rope_sin=PSIN, C2=PC2, bias=PBIAS)
            for opts in (None, {0: 0}, {0: 2}):
                rows.append(row("msda_prep", M, N, K, opts=opts, **ms, **w))
            rows.append(row("msda_prep_noC2", M, N, K, **dict(ms, C2=0), **w))
            rows.append(row("msda_prep_bf16out", M, N, K, **dict(ms, od=DU_BF16), **w))
            rows.append(row("msda_prep_f32in", M, N, K, dt=DU_F32, **ms, **w))
    return rows


def misaligned_rows(env=0):
    """one pointer / stride off the 16-byte rule: the generic kernel (or DU_ERR_BAD_ARG for the operands)"""
    rows = []
    for M, N, K in SMALL[::2] + [(131072, 1024, 64), (43008, 1024, 192)]:
        base = dict(bias=PBIAS, gamma=PGAMMA, residual=PRES, ldr=N, env=env)
        rows.append(row("aligned", M, N, K, **base))
        for f in ("bias", "gamma", "residual", "C", "A", "B"):
            v = {"bias": PBIAS, "gamma": PGAMMA, "residual": PRES, "C": PC, "A": PA, "B": PB}[f] + 4
            rows.append(row("off4_" + f, M, N, K, **{**base, f: v}))
        rows.append(row("ldr_odd", M, N, K, **{**base, "ldr": N + 2}))
        rows.append(row("ldc_odd", M, N, K, **base, ldc=N + 2))
        rows.append(row("cbs_odd", M, N, K, **base, c_batch_stride=2))
        rows.append(row("lda_odd", M, N, K, **base, lda=K + 4))
        rows.append(row("swiglu_off4_bias", M, N, K, bias=PBIAS + 4, act=ACT_SWIGLU, env=env))
        rows.append(row("N_odd", M, N + 2, K, env=env))
        rows.append(row("batch2", M, N, K, batch=2, a_batch_stride=M * K, c_batch_stride=M * N, env=env))
    rows.append(row("nullA", 256, 128, 256, A=0, env=env))
    rows.append(row("M0", 0, 128, 256, env=env))
    rows.append(row("bad_dtype", 256, 128, 256, dt=3, env=env))
    return rows


def option_rows():
    rows = []
    shapes = SMALL + [(8192, 4096, 1024), (4096, 4096, 4096), (43008, 1024, 512), (43008, 1024, 192), (131072, 512, 256), (8232, 2304, 768)]
    optsets = [{0: v} for v in range(0, 6)] + [{9: 2}, {9: 4}, {10: 0}, {10: 2}, {12: 0}, {12: 2}, {12: 3}, {14: 0}, {15: 1}, {16: 1}, {17: 0}, {17: 2},
                                                {0: 5, 16: 1}, {15: 1, 9: 2}, {0: 2, 15: 1}]
    for M, N, K in shapes:
        for o in optsets:
            rows.append(row("opt", M, N, K, opts=o))
            if ragged(M):
                rows.append(row("opt", M, N, K, opts=o, ws=False, ks=False))
            if K >= 1024:
                rows.append(row("opt", M, N, K, opts=o, od=DU_F32))
                rows.append(row("opt", M, N, K, opts=o, od=DU_F32, ks=False))
            if 0 in o or 10 in o:
                rows.append(row("opt", M, N, K, opts=o, bias=PBIAS, act=ACT_GELU))
                rows.append(row("opt", M, N, K, opts=o, bias=PBIAS, act=ACT_SWIGLU))
            if 0 in o or 14 in o or 10 in o:
                rows.append(row("opt", M, N, K, opts=o, residual=PRES, ldr=N))
    return rows


def all_rows():
    rows = nt_rows() + workload_rows() + mode_rows() + store_rows() + misaligned_rows() + option_rows()
    for e in range(1, len(ENVS)):
        rows += nt_rows(env=e, full=False) + workload_rows(env=e) + mode_rows(env=e)[::4] + store_rows(env=e)[::3] + misaligned_rows(env=e)[::3]
    names = [r["_name"] for r in rows]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1][:5]
    return rows


# ------------------------------------------------------------------------------------------------ running a table through a library
def to_args(cols, vals, alpha):
    a = GemmArgs()
    for c, v in zip(cols, vals):
        v = int(v)
        if c.startswith("opt") or c == "env":
            continue
        if c.startswith("geom."):
            setattr(a.geom, c[5:], v)
        else:
            setattr(a, c, v)
    a.alpha = float(alpha)
    a.rope_qscale = 1.0
    return a


def set_options(L, cols, vals):
    for c, v in zip(cols, vals):
        if c.startswith("opt"):
            L.du_set_option(int(c[3:]), int(v))


def summarise(rc, recs, M):
    """the launch list of one du_gemm call of the recorder library -> the PLAN columns"""
    if rc != 0:
        assert not recs, (rc, recs)
        return [rc, 0, 0, 0, 0, 0, 0]
    head = {1: (0, 0), 2: (1, 0), 3: (2, 0), 4: (3, 1), 5: (3, 1), 6: (4, 2), 7: (5, 3), 8: (6, 4), 9: (8, 5), 10: (5, 0), 11: (7, 0)}
    lid, hM, tr, splits, ga = recs[0]
    fam, var = head[lid]
    tail_rows, form = 0, TAIL_NONE
    if tr > 0:
        assert len(recs) == 1
        tail_rows, form = tr, TAIL_RIDES
    elif len(recs) > 1:
        assert len(recs) == 2
        tid, tM = recs[1][0], recs[1][1]
        tail_rows, form = tM, {12: TAIL_SKINNY_FUSED, 13: TAIL_SKINNY_PAIR, 2: TAIL_TILE_ENGINE}[tid]
    assert hM + tail_rows == M, (recs, M)
    return [0, fam, var, ga, tail_rows, form, splits]


def run_rows(path, table, alphas, mode):
    """mode 'reported': (route, ws_elems, ks_ws_bytes); 'executed': PLAN columns from the recorder library; 'describe': du_gemm_plan_describe"""
    L = C.CDLL(path)
    L.du_gemm_ws_elems.restype = C.c_int64
    L.du_gemm_ks_ws_bytes.restype = C.c_int64
    out = []
    buf = (C.c_int * (64 * 5))()
    d = (C.c_int64 * 16)()
    for vals, alpha in zip(table, alphas):
        a = to_args(COLUMNS, vals, alpha)
        set_options(L, COLUMNS, vals)
        if mode == "reported":
            out.append([L.du_gemm_route(C.byref(a)), L.du_gemm_ws_elems(C.byref(a)), L.du_gemm_ks_ws_bytes(C.byref(a))])
        elif mode == "executed":
            rc = L.du_gemm(C.byref(a), None)
            n = L.du_rec_read(buf)
            out.append(summarise(rc, [tuple(buf[5 * i:5 * i + 5]) for i in range(n)], int(a.M)))
        else:
            n = L.du_gemm_plan_describe(C.byref(a), d, 16)
            assert n == len(PLAN) + 2, n
            out.append(list(d[:n]) + [L.du_gemm_route(C.byref(a)), L.du_gemm_ws_elems(C.byref(a)), L.du_gemm_ks_ws_bytes(C.byref(a))])
    return out


def run_by_env(path, table, alphas, mode):
    """every environment knob in a process of its own (the library reads them once)"""
    res = np.zeros((len(table), 12), dtype=np.int64)
    envcol = COLUMNS.index("env")
    for e, spec in enumerate(ENVS):
        idx = [i for i in range(len(table)) if table[i][envcol] == e]
        env = dict(os.environ)
        if spec:
            k, v = spec.split("=")
            env[k] = v
        req = json.dumps({"path": path, "mode": mode, "table": [list(map(int, table[i])) for i in idx], "alphas": [float(alphas[i]) for i in idx]})
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], input=req, capture_output=True, text=True, env=env)
        if p.returncode != 0:
            raise RuntimeError(p.stderr)
        got = json.loads(p.stdout.strip().splitlines()[-1])
        for i, g in zip(idx, got):
            res[i, :len(g)] = g
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reported")
    ap.add_argument("--executed")
    ap.add_argument("--check")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        req = json.loads(sys.stdin.read())
        print(json.dumps(run_rows(req["path"], req["table"], req["alphas"], req["mode"])))
        return
    if a.check:
        g = np.load(a.out)
        got = run_by_env(os.path.abspath(a.check), g["rows"], g["alpha"], "describe")
        bad_exec = [i for i in range(len(got)) if list(got[i, :7]) != list(g["executed"][i]) and not (g["executed"][i][0] != 0 and got[i, 0] == g["executed"][i][0])]
        bad_route = [i for i in range(len(got)) if got[i, 9] != got[i, 1]]
        bad_ws = [i for i in range(len(got)) if list(got[i, 10:12]) != list(g["reported"][i][1:]) or list(got[i, 7:9]) != list(g["reported"][i][1:])]
        for tag, bad in (("executed", bad_exec), ("route != family", bad_route), ("scratch", bad_ws)):
            print(tag, len(bad), "rows differ")
            for i in bad[:12]:
                print("   ", g["names"][i], "got", list(got[i]), "executed", list(g["executed"][i]), "reported", list(g["reported"][i]))
        sys.exit(1 if bad_exec or bad_route or bad_ws else 0)
    rows = all_rows()
    table = np.array([[r[c] for c in COLUMNS] for r in rows], dtype=np.int64)
    alphas = np.array([r["_alpha"] for r in rows], dtype=np.float64)
    reported = run_by_env(os.path.abspath(a.reported), table, alphas, "reported")[:, :3]
    executed = run_by_env(os.path.abspath(a.executed), table, alphas, "executed")[:, :len(PLAN)]
    np.savez_compressed(a.out, columns=np.array(COLUMNS), plan=np.array(PLAN), envs=np.array(ENVS), names=np.array([r["_name"] for r in rows]),
                        rows=table, alpha=alphas, reported=reported, executed=executed)
    fam = executed[:, 1][executed[:, 0] == 0]
    print(f"{len(rows)} rows -> {a.out} ({os.path.getsize(a.out)} bytes); refused {int((executed[:, 0] != 0).sum())}; families {np.bincount(fam).tolist()}; "
          f"tail forms {np.bincount(executed[:, 5]).tolist()}; reported != executed family on {int(((reported[:, 0] != executed[:, 1]) & (executed[:, 0] == 0)).sum())} launched rows")


if __name__ == "__main__":
    main()
