"""du_layernorm_bwd_prod_plan (csrc/norm_gemm_plan.h, norm_gemm.hip): which calls the row-owning "LayerNorm backward of a product" kernel
serves and how it cuts them.  Pure host logic: no GPU, fake operand addresses."""
import ctypes as C

F32, BF16 = 0, 1
BAD_ARG, UNSUPPORTED = -1, -2
X, G, WT, DX, DRES, W, MEAN, RSTD, DWDB, WS = (0x10000000 * (i + 1) for i in range(10))


def plan(L, dtype=BF16, x=X, g=G, ldg=None, wt=WT, ldw=None, K=256, dx=DX, dres=DRES, rows=43008, D=1024):
    d = (C.c_int64 * 6)()
    assert L.du_layernorm_bwd_prod_plan(dtype, x, g, K if ldg is None else ldg, wt, K if ldw is None else ldw, K, dx, dres, rows, D, d, 6) == 6
    return list(d)


def test_plan_accepts_the_steps_shapes():
    from dinounet_amd import _lib
    L = _lib.lib()
    # 43008 query tokens of dinounet_l at 512^2, batch 8: 256 workgroups of 168 rows, blocks of 64 rows, one partial row per workgroup
    assert plan(L, K=256) == [1, 64, 256, 168, 256 * 1024 * 2, 64 * 1024 * 2 + 64 * 256 * 2]
    assert plan(L, K=192) == [1, 64, 256, 168, 256 * 1024 * 2, 64 * 1024 * 2 + 64 * 192 * 2]
    assert plan(L, K=192, dres=None)[0] == 1 and plan(L, K=256, dres=None)[0] == 1
    # a workgroup owns at least 64 rows; a short call has one workgroup
    assert plan(L, rows=1)[:4] == [1, 64, 1, 64] and plan(L, rows=65)[:4] == [1, 64, 2, 64] and plan(L, rows=4116)[:4] == [1, 64, 65, 64]
    assert plan(L, rows=16384 + 1)[:4] == [1, 64, 253, 65]
    assert plan(L, K=64)[0] == 1 and plan(L, K=128)[0] == 1
    assert plan(L, K=192, ldg=256, ldw=200)[0] == 1             # row strides: multiples of 8, at least K


def test_plan_declines():
    from dinounet_amd import _lib
    L = _lib.lib()
    none = [0, 0, 0, 0, 0, 0]
    assert plan(L, D=768) == none and plan(L, D=1032) == none and plan(L, D=512) == none
    assert plan(L, K=512) == none and plan(L, K=320) == none and plan(L, K=96) == none and plan(L, K=200) == none      # the injector's K = 512 stays unfused
    assert plan(L, dtype=F32) == none and plan(L, dtype=7) == none
    for name in ("x", "g", "wt", "dx", "dres"):
        assert plan(L, **{name: 0x10000000 + 8}) == none, name
    assert plan(L, ldg=260) == none and plan(L, ldw=250) == none and plan(L, K=192, ldg=128) == none
    assert plan(L, rows=0) == none and plan(L, x=None) == none and plan(L, g=None) == none and plan(L, wt=None) == none and plan(L, dx=None) == none
    d = (C.c_int64 * 6)()
    assert L.du_layernorm_bwd_prod_plan(BF16, X, G, 256, WT, 256, 256, DX, DRES, 43008, 1024, None, 6) == BAD_ARG
    assert L.du_layernorm_bwd_prod_plan(BF16, X, G, 256, WT, 256, 256, DX, DRES, 43008, 1024, d, 5) == BAD_ARG


def test_entry_checks_before_launching():
    """what the plan declines is DU_ERR_UNSUPPORTED from the entry, scratch one float short is DU_ERR_BAD_ARG: nothing launches (no device here)"""
    from dinounet_amd import _lib
    L = _lib.lib()
    n = plan(L)[4]
    call = lambda **kw: L.du_layernorm_bwd_prod(kw.get("dtype", BF16), X, G, 256, WT, 256, kw.get("K", 256), W, MEAN, RSTD, DX, DWDB, 43008,
                                                kw.get("D", 1024), kw.get("ws", WS), kw.get("n", n), DRES, None)
    assert call(dtype=F32) == UNSUPPORTED and call(D=768) == UNSUPPORTED and call(K=512) == UNSUPPORTED
    assert call(n=n - 1) == BAD_ARG and call(ws=None) == BAD_ARG
