"""Exact-input parity tests (-m gpu): the sum-of-products kernels must match an fp64 reference TO THE BIT.

What each instrument of the suite is for:
  * exact inputs (this file): indexing and completeness of the sum.  Operands are ternary / small integers, every product and partial sum is
    an integer (or a dyadic fraction) below 2^24 granules, so fp32 accumulation is exact in any order and the result must equal the cast of the
    fp64 reference.  One missing, doubled or misplaced term fails; no tolerance exists to hide it.  The conditions (2^24 bound, >= 95 % of a
    bf16 reference exactly representable, operands random and from different seeds) are asserted on the reference before the kernel's
    output is looked at; tests/test_cpu_exact.py asserts them for every shape list below and shows that the gate rejects broken kernels.
  * random inputs (tests/test_gpu_ops.py): rounding behaviour and realistic magnitudes, against fp32 / fp64 products within a tolerance.
  * where the epilogue is not linear (GELU, SwiGLU, softmax) the pre-activation is exact and the gate is a derived bound per element
    (tests/_exact.py: act_excess, attention_ref64).

Every case goes through the entry the product path uses.  A case that forces a kernel family does it the way the existing test of that
family does (du_set_option, restored on exit) and asserts the route that ran (ops.TRACK_ROUTE / LAST_GEMM_ROUTE); the convolution,
ConvTranspose-generic, depthwise, segmentation-head and MSDA cases go through the default dispatch (one kernel per such shape)."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

import _exact as X

pytestmark = pytest.mark.gpu

bf, f32 = torch.bfloat16, torch.float32


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from dinounet_amd import _lib
    assert _lib.lib().du_device_ok() == 1, "libdinounet_hip.so kernels are built for gfx950 only"
    return torch.device("cuda:0")


class forced:
    """du_set_option(key, value) pairs for the body, defaults restored on exit; ops.TRACK_ROUTE on, ops.ROUTES cleared"""
    DEFAULTS = {0: -1, 3: 0, 5: 1, 10: 1, 12: 1, 13: 1, 14: 1, 15: 0, 16: 0, 17: 1}

    def __init__(self, **kv):
        self.kv = {int(k[1:]): v for k, v in kv.items()}

    def __enter__(self):
        from dinounet_amd import _lib, ops
        for k, v in self.kv.items():
            _lib.lib().du_set_option(k, v)
        ops.TRACK_ROUTE, ops.ROUTES[:] = True, []
        return ops

    def __exit__(self, *exc):
        from dinounet_amd import _lib, ops
        ops.TRACK_ROUTE = False
        for k in self.kv:
            _lib.lib().du_set_option(k, self.DEFAULTS[k])
        return False


def ks_state(ops):
    """the 128 KB of state words (tickets, pair flags) at the head of the current stream's du_gemm_args.ks_ws scratch"""
    key = (torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream)
    assert key in ops._KS_SCRATCH, "no ks_ws scratch was lent on this stream: the product did not run the form under test"
    return ops._KS_SCRATCH[key][:131072].view(torch.int32)


# ==================================================================================================== 1. NT products
# the shapes of test_gemm_multiphase_nt, all of them (ragged tile rows / columns, K at the drain limits 256 / 384 / 512 / 896 / 2048, one
# tile per workgroup); its "gelu" rows are the GELU cases of part 2 below
NT_SHAPES = [(8232, 3072, 1024, False, "bias"), (8232, 1024, 4096, True, "ls_res"), (8232, 1024, 1024, True, "ls_res"),
             (1000, 516, 512, True, "bias"), (768, 640, 384, False, "none"), (2048, 384, 1536, False, "rs"),
             (70000, 264, 512, False, "bias"), (43008, 1024, 512, False, "none"), (5000, 136, 2048, False, "bias"),
             (43008, 1024, 256, False, "bias"), (33000, 520, 384, False, "bias"),
             (43008, 1024, 256, False, "res_rs"), (43008, 1024, 512, False, "res"), (33000, 1024, 384, False, "res"),
             (10752, 256, 256, False, "res_rs"), (21504, 640, 1024, False, "res_rs"), (5000, 128, 512, False, "res"),
             (16424, 512, 512, False, "res"),
             # the fp32 in-place residual stream and a bf16 result of the same LayerScale-free epilogue on a ragged shape
             (1000, 516, 512, True, "ls_res_inplace"), (8232, 1024, 1024, True, "ls_res_inplace")]
GELU_SHAPES = [(8232, 4096, 1024), (33000, 1000, 896), (33000, 1000, 640), (70000, 264, 256)]
SENSITIVITY_SHAPES = {(1000, 516, 512, True, "bias"), (768, 640, 384, False, "none"), (5000, 128, 512, False, "res")}

_CASE = {}


def nt_case(M, N, K, f32out, epi, rows="default"):
    """operands (CPU, fp32 holding exact values), keyword arguments of the epilogue, the fp64 reference on the compared rows; conditions
    asserted here, on the CPU side, before any kernel output exists.  One entry is cached: the modes of a shape run back to back.
    Bias: integers in [-4, 4] for a bf16 result; for an fp32 result multiples of 1/256 up to +-4 (11 significant bits: a bias that went
    through bf16 on its way changes the result)."""
    key = (M, N, K, f32out, epi, rows if isinstance(rows, str) else "sample")
    if _CASE.get("key") == key:
        return _CASE["val"]
    x, w = X.ternary(M, K, seed=11), X.ternary(N, K, seed=12)
    b = X.integers(N, seed=13, lo=-1024, hi=1024) / 256 if f32out else X.integers(N, seed=13, lo=-4, hi=4)
    gam = X.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], N, seed=14)
    X.require_random(x, w, b, gam)
    if isinstance(rows, str):
        rows = X.check_rows(M)
    xr = x if rows is None else x[rows]
    ridx = torch.arange(M) if rows is None else rows
    ref = xr.double() @ w.double().t()
    bound, granule = X.sum_bound(x, w), (1.0 / 256 if f32out else 1.0)
    kw, cpu = {}, {}
    if epi in ("bias", "ls_res", "ls_res_inplace", "res", "res_rs"):
        cpu["bias"] = b
        ref = ref + b.double()
        bound += 4
    if epi in ("ls_res", "ls_res_inplace"):
        res = X.integers(M, N, seed=15, lo=-256, hi=256)
        cpu.update(gamma=gam, residual=res)
        ref = ref * gam.double() + res[ridx].double()
        bound, granule = bound * 2 + 256, granule / 2
    if epi == "rs":
        rs = X.choice([0.0, 1.5, 2.0], (M + 7) // 8, seed=16)
        cpu.update(row_scale=rs)
        kw["rs_rows"] = 8
        ref = ref * rs.repeat_interleave(8)[:M][ridx, None].double()
        bound, granule = bound * 2, granule / 2
    if epi in ("res", "res_rs"):                  # y = s (x w^T + b) + r, r in the result's dtype (bf16: |r| <= 256 is exact in bf16 too)
        if epi == "res_rs":
            nb = (M + 5375) // 5376
            rs = torch.tensor([0.0, 1.5, 2.0])[torch.arange(nb) % 3]
            cpu.update(row_scale=rs)
            kw["rs_rows"] = 5376
            ref = ref * rs.repeat_interleave(5376)[:M][ridx, None].double()
            bound, granule = bound * 2, granule / 2
        res = X.integers(M, N, seed=15, lo=-32, hi=32)
        cpu["residual"] = res
        ref = ref + res[ridx].double()
        bound += 32
    X.require_exact(bound, granule)
    if not f32out:
        X.require_bf16_share(ref)
    _CASE["key"], _CASE["val"] = key, (x, w, cpu, kw, ref, rows)
    return _CASE["val"]


def run_nt(ops, d, x, w, cpu, kw, M, N, od, inplace=False, **more):
    """one ops.mm launch into a sentinel-filled, guarded buffer; returns (whole buffer, result view)"""
    k2 = dict(kw, **more)
    for name in ("bias", "gamma", "row_scale"):
        if name in cpu:
            k2[name] = cpu[name].to(d)
    fill = None
    if "residual" in cpu:
        r = cpu["residual"].to(d, od)
        if inplace:
            fill = r
        else:
            k2["residual"] = r
    whole, out = X.guarded(M, N, od, d, fill=fill)
    if inplace:
        k2["residual"] = out
    y = ops.mm(x, w, out=out, **k2)
    assert y.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    return whole, out


def expect_route(mode, N, K, od, cpu, rs_rows=0):
    """the kernel family du_set_option(0, mode) must give these products (gemm.hip: du_gemm_plan; gemm_p8.hip: pp_legal)"""
    if mode == 0:
        return 2 if (K % 64 == 0 and N >= 96) else 1
    if mode == 1:
        return 3
    if mode == 2:
        return 4
    pp = od == bf and "gamma" not in cpu and N % 8 == 0 and (K == 256 or K >= 384)
    if "residual" in cpu:
        pp = pp and N % 128 == 0 and ("row_scale" not in cpu or rs_rows % 256 == 0)
    else:
        pp = pp and "row_scale" not in cpu
    return 6 if pp else 4


@pytest.mark.parametrize("mode", [0, 1, 2, 4])
@pytest.mark.parametrize("M,N,K,f32out,epi", NT_SHAPES)
def test_nt_products_every_route(mode, M, N, K, f32out, epi):
    """x w^T + every linear epilogue of the ViT / adapter on the 128 x 128 tile kernels (mode 0: gemm_bf16_kernel or gemm_nt_glds_kernel,
    routes 1 / 2), the 256 x 256 (route 3), 256 x 128 (route 4) and persistent (route 6) multi-phase kernels: bit-equal to the fp64
    product of the same integers.  For M >= 33000 the rows of _exact.check_rows are compared (first / middle / last 256-row block, the ragged
    rows, every 97th row: whole rows); sentinel and guard band are checked over the whole buffer.  One perturbed input element must fail."""
    d = dev()
    x, w, cpu, kw, ref, rows = nt_case(M, N, K, f32out, epi)
    od = f32 if f32out else bf
    xd, wd = x.to(d, bf), w.to(d, bf)
    what = f"mode {mode} {M}x{N}x{K} {epi} {'f32' if f32out else 'bf16'}"
    with forced(k0=mode) as ops:
        whole, out = run_nt(ops, d, xd, wd, cpu, kw, M, N, od, inplace=epi.endswith("inplace"))
        route = ops.LAST_GEMM_ROUTE
        assert route == expect_route(mode, N, K, od, cpu, kw.get("rs_rows", 0)), (what, route)
        X.assert_guard(whole, M, what)
        got = out if rows is None else out[rows.to(d)]
        X.assert_exact(got, ref, what)
        if (M, N, K, f32out, epi) in SENSITIVITY_SHAPES:
            # sensitivity through the real kernel and store path: one changed INPUT element of the last row, same reference -> must fail
            x2 = xd.clone()
            x2[M - 1, K - 1] = 3.0
            whole2, out2 = run_nt(ops, d, x2, wd, cpu, kw, M, N, od)
            assert not X.is_exact(out2, ref), what + ": the gate did not see one changed term"
            assert torch.equal(out2[:M - 1], out[:M - 1]), what + ": a change in the last row reached other rows"


ROUTE1_SHAPES = [(1000, 64, 512), (1029, 520, 96), (4100, 72, 1056)]


@pytest.mark.parametrize("M,N,K", ROUTE1_SHAPES)
def test_nt_route_1_exact(M, N, K):
    """gemm_bf16_kernel (route 1: the 128 x 128 register-tile kernel the others fall back to) under the default dispatch: fewer than 96
    columns, or a contraction that is no multiple of 64 -- bias (bf16 result), LayerScale + fp32 residual, and one perturbed input element"""
    d = dev()
    with forced() as ops:
        for f32out, epi in ((False, "bias"), (True, "ls_res")):
            x, w, cpu, kw, ref, _ = nt_case(M, N, K, f32out, epi)
            xd, wd = x.to(d, bf), w.to(d, bf)
            od = f32 if f32out else bf
            whole, out = run_nt(ops, d, xd, wd, cpu, kw, M, N, od)
            assert ops.LAST_GEMM_ROUTE == 1, ops.LAST_GEMM_ROUTE
            X.assert_guard(whole, M, epi)
            X.assert_exact(out, ref, f"route 1 {M}x{N}x{K} {epi}")
            x2 = xd.clone()
            x2[M - 1, K - 1] = 3.0
            _, out2 = run_nt(ops, d, x2, wd, cpu, kw, M, N, od)
            assert ops.LAST_GEMM_ROUTE == 1
            assert not X.is_exact(out2, ref) and torch.equal(out2[:M - 1], out[:M - 1]), "the gate did not see one changed term"


def test_persistent_residual_in_place_exact():
    """as test_gemm_persistent_residual_in_place: the bf16 residual of the persistent kernel's residual form IS the output buffer"""
    d = dev()
    M, N, K = 43008, 1024, 256
    x, w, cpu, kw, ref, rows = nt_case(M, N, K, False, "res_rs")
    with forced() as ops:
        whole, out = run_nt(ops, d, x.to(d, bf), w.to(d, bf), cpu, kw, M, N, bf, inplace=True)
        assert ops.LAST_GEMM_ROUTE == 6, ops.LAST_GEMM_ROUTE
        whole2, out2 = run_nt(ops, d, x.to(d, bf), w.to(d, bf), cpu, kw, M, N, bf)
        assert ops.LAST_GEMM_ROUTE == 6, ops.LAST_GEMM_ROUTE
    X.assert_guard(whole, M, "in place")
    X.assert_guard(whole2, M, "out of place")
    X.assert_exact(out2[rows.to(d)], ref, "persistent kernel, residual out of place")
    X.assert_exact(out[rows.to(d)], ref, "persistent kernel, residual in place")
    # every row: the in-place buffer started as the residual, not the sentinel, so a row left unwritten outside the compared sample would
    # keep a plausible value -- the out-of-place run went into a sentinel-filled buffer (checked above) and must agree everywhere
    assert torch.equal(out, out2), "in place and out of place differ: " + X.mismatch_report(out.float().cpu(), out2.float().cpu())


# ---------------------------------------------------------------------------------------------------- the ViT rows: M = 8 x 1029 = 32 x 256 + 40
VIT_M = 8232


def vit_case(N, K, od, epi):
    return nt_case(VIT_M, N, K, od == f32, epi)


@pytest.mark.parametrize("inline", [0, 1])
@pytest.mark.parametrize("N,K", [(1024, 1024), (3072, 1024), (1024, 4096)])
def test_vit_ragged_rows_as_skinny_tail(N, K, inline):
    """the 40 ragged rows on the K-parallel skinny kernels, as extra workgroups (key 15 = 0) and inside the tile workgroups (1): bias (bf16),
    LayerScale + DropPath scale + fp32 residual in place, and the plain fp32 product"""
    from dinounet_amd import _lib
    d = dev()
    M = VIT_M
    a = _lib.GemmArgs()
    a.dtype, a.out_dtype, a.a_mode, a.b_mode, a.M, a.N, a.K = _lib.DU_BF16, _lib.DU_BF16, 0, 0, M, N, K
    a.lda, a.ldb, a.ldc, a.batch, a.split_k = K, K, N, 1, 1
    assert int(_lib.lib().du_gemm_ws_elems(C.byref(a))) > 0          # the library asks for the tail kernels' scratch on this shape
    x, w, cpu, kw, ref, _ = nt_case(M, N, K, False, "bias")
    xd, wd = x.to(d, bf), w.to(d, bf)
    with forced(k15=inline) as ops:
        whole, out = run_nt(ops, d, xd, wd, cpu, kw, M, N, bf)
        X.assert_guard(whole, M, "bias")
        X.assert_exact(out, ref, f"tail inline {inline} bias bf16")
        x2 = xd.clone()
        x2[M - 1, K - 1] = 3.0                                       # sensitivity: one element of the last ragged row
        _, out2 = run_nt(ops, d, x2, wd, cpu, kw, M, N, bf)
        assert not X.is_exact(out2, ref) and torch.equal(out2[:M - 1], out[:M - 1])
        # LayerScale, one DropPath scale per 8 rows (1029 blocks: the split keeps them aligned), fp32 residual stream in place
        gam, res = X.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], N, seed=14), X.integers(M, N, seed=15, lo=-256, hi=256)
        rs = X.choice([0.0, 1.5, 2.0], 1029, seed=16)
        prod = x.double() @ w.double().t()
        ref2 = (prod + cpu["bias"].double()) * gam.double() * rs.repeat_interleave(8)[:, None].double() + res.double()
        X.require_exact((X.sum_bound(x, w) + 4) * 4 + 256, 0.25)
        c2 = dict(bias=cpu["bias"], gamma=gam, row_scale=rs, residual=res)
        whole, out = run_nt(ops, d, xd, wd, c2, dict(rs_rows=8), M, N, f32, inplace=True)
        X.assert_guard(whole, M, "ls")
        X.assert_exact(out, ref2, f"tail inline {inline} LayerScale + row scale + residual in place, fp32")
        whole, out = run_nt(ops, d, xd, wd, {}, {}, M, N, f32)
        X.assert_guard(whole, M, "plain")
        X.assert_exact(out, prod, f"tail inline {inline} plain fp32")


@pytest.mark.parametrize("K", [4096, 2048])
@pytest.mark.parametrize("od", [f32, bf])
def test_vit_ragged_rows_as_k_sliced_units(od, K):
    """fc2 (K = 4096) and K = 2048: the 40 ragged rows as (32 columns, K slice) units that meet through du_gemm_args.ks_ws -- slabs, a ticket,
    the last arriver adds the slices (key 17, default on): one slice added twice, one left out or one stale slab changes the integer.
    Tickets back at zero.  With key 17 = 0 (one unit per column block) the same bits."""
    from dinounet_amd import _lib, ops as ops_
    d = dev()
    L = _lib.lib()
    M, N = VIT_M, 1024
    epi = "ls_res" if od == f32 else "res"
    x, w, cpu, kw, ref, _ = nt_case(M, N, K, od == f32, epi)
    xd, wd = x.to(d, bf), w.to(d, bf)
    a = _lib.GemmArgs()
    a.dtype, a.out_dtype, a.a_mode, a.b_mode = _lib.DU_BF16, _lib.DU_F32 if od == f32 else _lib.DU_BF16, 0, 0
    a.M, a.N, a.K, a.batch, a.split_k, a.alpha = M, N, K, 1, 1, 1.0
    a.A, a.lda, a.B, a.ldb, a.C, a.ldc = xd.data_ptr(), K, wd.data_ptr(), K, xd.data_ptr(), N
    assert int(L.du_gemm_ks_ws_bytes(C.byref(a))) > 131072, "the K-sliced units were not offered for this shape"
    with forced(k17=1) as ops:
        whole, out = run_nt(ops, d, xd, wd, cpu, kw, M, N, od)
        state = ks_state(ops_)
        assert int(state.abs().sum().item()) == 0, "tickets not back at zero"
        X.assert_guard(whole, M, "k-sliced")
        X.assert_exact(out, ref, f"K-sliced units K {K}")
        x2 = xd.clone()
        x2[M - 1, K - 1] = 3.0
        _, out2 = run_nt(ops, d, x2, wd, cpu, kw, M, N, od)
        assert not X.is_exact(out2, ref) and torch.equal(out2[:M - 1], out[:M - 1])
    with forced(k17=0) as ops:
        assert int(L.du_gemm_ks_ws_bytes(C.byref(a))) == 0
        whole, out = run_nt(ops, d, xd, wd, cpu, kw, M, N, od)
        X.assert_guard(whole, M, "one unit per column block")
        X.assert_exact(out, ref, f"one unit per column block K {K}")


@pytest.mark.parametrize("M,N,K", [(4136, 1024, 1024), (8232, 1024, 4096), (4096, 2048, 1024)])
def test_k_split_pairs_exact(M, N, K):
    """gemm_nt_p8ks_kernel (key 16): K-split pairs of workgroups that exchange fp32 halves inside the launch; the three ways through the
    exchange as test_gemm_k_split_pairs_every_way_through_the_exchange forces them (key 3 = 8 / 24 / 16, nothing else from key 3).  A half
    added twice or taken from a stale exchange buffer changes the integer.
    4136 x 1024 x 1024 through ops.mm runs the 128 x 128 kernel (2), as it always did (tests/test_cpu_gemm_plan.py: CORRECTED,
    'ragged rows without ws', and test_plan_of_the_k_split_pair_shapes_as_ops_lends_scratch): ops.gemm_raw asks for the ragged rows' ws before it lends ks_ws, the pair kernel is not yet legal for
    the 4096-row head then, no ws is lent, and all 4136 rows (17 x 4 tiles: no whole pairs) stay in one grid."""
    from dinounet_amd import ops as ops_
    d = dev()
    x, w, cpu, kw, ref, _ = nt_case(M, N, K, True, "ls_res")
    xd, wd = x.to(d, bf), w.to(d, bf)
    route = 2 if (M, N, K) == (4136, 1024, 1024) else 8
    with forced(k16=1, k3=0) as ops:
        from dinounet_amd import _lib
        for aid in (0, 8, 24, 16):
            _lib.lib().du_set_option(3, aid)
            whole, out = run_nt(ops, d, xd, wd, cpu, kw, M, N, f32)
            assert ops.LAST_GEMM_ROUTE == route, (aid, ops.LAST_GEMM_ROUTE)
            state = ks_state(ops_)
            assert int(state.abs().sum().item()) == 0, f"aid {aid}: pair state not restored (error word {int(state[16380].item())})"
            X.assert_guard(whole, M, f"aid {aid}")
            X.assert_exact(out, ref, f"K-split pairs, exchange order {aid}")
        _lib.lib().du_set_option(3, 0)
        x2 = xd.clone()
        x2[M - 1, K - 1] = 3.0
        _, out2 = run_nt(ops, d, x2, wd, cpu, kw, M, N, f32)
        assert ops.LAST_GEMM_ROUTE == route
        assert not X.is_exact(out2, ref) and torch.equal(out2[:M - 1], out[:M - 1])


def test_ks_scratch_is_never_created_under_capture():
    """ops._ks_scratch hands du_gemm the scratch whose first 128 KB (tickets of the K-sliced units, pair state) must be zero.  Created inside
    a capture, its zeroing is only a node of that graph: if the graph is discarded unreplayed the zeroing never runs while the buffer stays
    cached under its stream key.  So: a K-sliced exact product (fc2, default option keys) captured as the FIRST use of a fresh stream key, that
    graph discarded, a second one captured and replayed -- (a) no buffer may exist under that key afterwards (ops._KS_SCRATCH), (b) the replay is
    bit-equal to the exact reference.  Then with the buffer prepared before the capture (as training.TrainStep does): the units run inside
    the graph, tickets back at zero after every replay, same bits."""
    from dinounet_amd import ops
    d = dev()
    M, N, K = VIT_M, 1024, 4096
    x, w, cpu, kw, ref, _ = nt_case(M, N, K, False, "res")
    xd, wd, b, r = x.to(d, bf), w.to(d, bf), cpu["bias"].to(d), cpu["residual"].to(d, bf)
    whole, out = X.guarded(M, N, bf, d)
    run = lambda: ops.mm(xd, wd, out=out, bias=b, residual=r)
    for _ in range(64):                                # torch hands out streams from a pool: take one whose key has never had a buffer
        s = torch.cuda.Stream()
        key = (d.index, s.cuda_stream)
        if key not in ops._KS_SCRATCH:
            break
    if key in ops._KS_SCRATCH:
        ops._KS_RETIRED.append(ops._KS_SCRATCH.pop(key))          # (kept alive: an earlier graph may hold its address)
    assert key not in ops._KS_SCRATCH
    torch.cuda.synchronize()
    g1 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g1, stream=s):
        run()
    del g1                                             # discarded, never replayed
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2, stream=s):
        run()
    assert key not in ops._KS_SCRATCH, "a ks_ws buffer was created (and its zeroing recorded) under capture"
    whole.fill_(X.SENTINEL)
    g2.replay()
    torch.cuda.synchronize()
    X.assert_guard(whole, M, "replay without ks_ws")
    X.assert_exact(out, ref, "replay of the second capture")
    ops.ks_scratch_prepare(s)
    assert key in ops._KS_SCRATCH
    g3 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g3, stream=s):
        run()
    for i in range(2):
        whole.fill_(X.SENTINEL)
        g3.replay()
        torch.cuda.synchronize()
        assert int(ops._KS_SCRATCH[key][:131072].view(torch.int32).abs().sum().item()) == 0, "tickets not back at zero"
        X.assert_guard(whole, M, f"replay {i} with ks_ws")
        X.assert_exact(out, ref, f"replay {i}, K-sliced units inside the graph")


RK_SHAPES = [(5000, 96, 64, "nt"), (4100, 288, 32, "nt_relu"), (9000, 1024, 192, "nt"), (4096, 512, 256, "nt"), (6000, 160, 128, "nt_nobias"),
             (7000, 256, 32, "dgrad"), (4500, 64, 256, "dgrad"), (131072, 256, 64, "nt")]


@pytest.mark.parametrize("M,N,K,form", RK_SHAPES)
def test_resident_weights_kernel_exact(M, N, K, form):
    """gemm_nt_rk_kernel (route 7, forced with key 12 = 3) at the shapes of test_gemm_resident_weights_streaming_kernel: ragged M, column
    chunks of unequal size, W as [N][K] and as [K][N], bias / ReLU (exact: max(0, integer))."""
    from dinounet_amd._lib import ACT_RELU
    d = dev()
    rows = X.check_rows(M)
    ridx = torch.arange(M) if rows is None else rows
    x = X.ternary(M, K, seed=21)
    if form == "dgrad":
        w = X.ternary(K, N, seed=22)
        ref = x[ridx].double() @ w.double()
        X.require_exact(X.sum_bound(x))
    else:
        w = X.ternary(N, K, seed=22)
        b = None if form == "nt_nobias" else X.integers(N, seed=23, lo=-4, hi=4)
        ref = x[ridx].double() @ w.double().t()
        if b is not None:
            ref = ref + b.double()
        if form == "nt_relu":
            ref = ref.clamp_min(0)
        X.require_exact(X.sum_bound(x, w) + 4)
    X.require_random(x, w)
    X.require_bf16_share(ref)
    xd, wd = x.to(d, bf), w.to(d, bf)
    with forced(k12=3) as ops:
        if form == "dgrad":
            whole, out = X.guarded(M, N, bf, d)
            ops.mm_dgrad(xd, wd, out=out)
        else:
            whole, out = X.guarded(M, N, bf, d)
            ops.mm(xd, wd, out=out, bias=None if b is None else b.to(d), act=ACT_RELU if form == "nt_relu" else 0)
        assert ops.LAST_GEMM_ROUTE == 7, ops.LAST_GEMM_ROUTE
        torch.cuda.synchronize()
        X.assert_guard(whole, M, form)
        X.assert_exact(out if rows is None else out[rows.to(d)], ref, f"resident weights {M}x{N}x{K} {form}")
        if (M, N, K) == (5000, 96, 64):                # sensitivity through this kernel: one changed input element of the last row
            x2 = xd.clone()
            x2[M - 1, K - 1] = 3.0
            _, out2 = X.guarded(M, N, bf, d)
            ops.mm(x2, wd, out=out2, bias=b.to(d))
            assert ops.LAST_GEMM_ROUTE == 7
            assert not X.is_exact(out2, ref) and torch.equal(out2[:M - 1], out[:M - 1])


PLAIN_SHAPES = [(1029, 1152, 384), (300, 32, 64), (257, 64, 128), (128, 128, 64), (4096, 2, 32), (70, 200, 1024)]


@pytest.mark.parametrize("dt", [f32, bf])
@pytest.mark.parametrize("M,N,K", PLAIN_SHAPES)
def test_plain_epilogues_exact(dt, M, N, K):
    """test_gemm_plain_epilogues' small / skinny shapes under the default dispatch, both operand types: bias, ReLU, LayerScale + fp32
    residual in place.  The fp32 engine (route 0) multiplies fp32 operands on the MFMA / FMA units with fp32 accumulation: on integers below
    2^24 every step is exact whatever its order, so it has to be bit-equal as well."""
    from dinounet_amd._lib import ACT_RELU
    d = dev()
    x, w = X.ternary(M, K, seed=31), X.ternary(N, K, seed=32)
    b, gam = X.integers(N, seed=33, lo=-4, hi=4), X.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], N, seed=34)
    res = X.integers(M, N, seed=35, lo=-256, hi=256)
    X.require_random(x, w, b, gam, res)
    X.require_exact((X.sum_bound(x, w) + 4) * 2 + 256, 0.5)
    s = x.double() @ w.double().t() + b.double()
    if dt == bf:
        X.require_bf16_share(s)
    xd, wd = x.to(d, dt), w.to(d, dt)
    with forced() as ops:
        whole, out = X.guarded(M, N, dt, d)
        ops.mm(xd, wd, out=out, bias=b.to(d))
        assert (ops.LAST_GEMM_ROUTE == 0) == (dt == f32 or N % 4 != 0), ops.LAST_GEMM_ROUTE
        X.assert_guard(whole, M, "bias")
        X.assert_exact(out, s, f"{dt} bias")
        whole, out = X.guarded(M, N, dt, d)
        ops.mm(xd, wd, out=out, bias=b.to(d), act=ACT_RELU)
        X.assert_guard(whole, M, "relu")
        X.assert_exact(out, s.clamp_min(0), f"{dt} bias + ReLU")
        whole, out = X.guarded(M, N, f32, d, fill=res.to(d))
        y = ops.mm(xd, wd, bias=b.to(d), gamma=gam.to(d), residual=out, out=out)
        assert y.dtype == f32
        X.assert_guard(whole, M, "ls_res")
        X.assert_exact(out, s * gam.double() + res.double(), f"{dt} LayerScale + residual in place")


# ---------------------------------------------------------------------------------------------------- store modes
def qkv_reference(h, w, bias, sin, cos, B, N, H, Dh, prefix, qscale):
    """fp64 planes (3, B, H, N, Dh): projection rounded to bf16 (exact here), RoPE with the given tables on q and k behind the prefix, q scaled"""
    qkv = (h.double() @ w.double().t() + bias.double()).view(B, N, 3, H, Dh).permute(2, 0, 3, 1, 4)

    def rope(t):
        a = t[:, :, prefix:]
        x1, x2 = a.chunk(2, -1)
        return torch.cat([t[:, :, :prefix], a * cos.double() + torch.cat([-x2, x1], -1) * sin.double()], 2)

    return qkv, torch.stack([rope(qkv[0]) * qscale, rope(qkv[1]), qkv[2]])


QKV_SHAPES = [(8, 16, 1029, 1024), (2, 6, 1029, 384), (3, 12, 261, 768), (9, 16, 1029, 1024), (1, 16, 1024, 1024)]


def rope_tables(N, prefix, Dh, seed):
    """sin / cos tables whose entries are 0 and +-1 (the kernels take the tables, not the angles): a quarter turn per entry"""
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(0, 4, (N - prefix, Dh), generator=g)
    return torch.tensor([0.0, 1.0, 0.0, -1.0])[k].contiguous(), torch.tensor([1.0, 0.0, -1.0, 0.0])[k].contiguous()


@pytest.mark.parametrize("B,H,N,D", QKV_SHAPES)
def test_qkv_head_major_store_and_in_place_rope_exact(B, H, N, D):
    """DU_STORE_QKV_HEADS from the persistent kernel's drain (route 6; the ragged rows in the same launch; tiles that straddle samples at
    B = 9; no ragged rows at N = 1024), then du_qkv_rope_inplace through the C ABI with 0 / +-1 tables and a power-of-two q scale: the three
    planes bit-equal to the fp64 projection, before and after the rotation."""
    from dinounet_amd import _lib
    d = dev()
    Dh, prefix, qscale = 64, 5, 0.125
    M, Npad = B * N, (N + 7) // 8 * 8
    h, w = X.ternary(M, D, seed=41), X.ternary(3 * H * Dh, D, seed=42)
    bias = X.integers(3 * H * Dh, seed=43, lo=-4, hi=4)
    sin, cos = rope_tables(N, prefix, Dh, seed=44)
    X.require_random(h, w, bias, sin, cos)
    X.require_exact(2 * (X.sum_bound(h, w) + 4), qscale)
    proj, want = qkv_reference(h, w, bias, sin, cos, B, N, H, Dh, prefix, qscale)
    X.require_bf16_share(proj)
    X.require_bf16_share(want)
    hd, wd = h.to(d, bf), w.to(d, bf)
    plane = B * H * Npad * Dh
    whole = torch.full((3 * plane + X.GUARD_ROWS * Dh,), X.SENTINEL, dtype=bf, device=d)
    qkv3 = whole[:3 * plane].view(3, B, H, Npad, Dh)
    with forced(k0=4) as ops:
        ops.gemm_raw(dtype=_lib.DU_BF16, out_dtype=_lib.DU_BF16, a_mode=ops.PLAIN_ROW, b_mode=ops.PLAIN_ROW, M=M, N=3 * H * Dh, K=D, A=hd.data_ptr(),
                     lda=D, B=wd.data_ptr(), ldb=D, Cmat=qkv3.data_ptr(), ldc=plane, bias=bias.to(d).data_ptr(), store_mode=ops.STORE_QKV_HEADS,
                     ps=(N, Npad, H))
        assert ops.LAST_GEMM_ROUTE == 6, ops.LAST_GEMM_ROUTE
        torch.cuda.synchronize()
    sent = torch.tensor(X.SENTINEL).to(bf)
    assert bool((whole[3 * plane:] == sent.to(d)).all()), "write behind the v plane"
    assert not bool((qkv3[:, :, :, :N] == sent.to(d)).any()), "unwritten token rows"
    X.assert_exact(qkv3[:, :, :, :N], proj, "head-major store")
    sd, cd = sin.to(d), cos.to(d)
    _lib.check(_lib.lib().du_qkv_rope_inplace(_lib.DU_BF16, C.c_void_p(qkv3[0].data_ptr()), C.c_void_p(qkv3[1].data_ptr()), C.c_void_p(sd.data_ptr()),
                                              C.c_void_p(cd.data_ptr()), B, N, Npad, H, Dh, prefix, C.c_float(qscale), M,
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream)), "du_qkv_rope_inplace")
    torch.cuda.synchronize()
    assert bool((whole[3 * plane:] == sent.to(d)).all()), "du_qkv_rope_inplace wrote behind the planes"
    X.assert_exact(qkv3[:, :, :, :N], want, "in-place RoPE")


def rope_store_case(B, H, N, D, sin, cos, mode, route, grid=None):
    """one DU_STORE_QKV_ROPE launch on the full 256-row tiles, as ops.qkv_attention makes it (rows behind them are another launch there):
    RoPE with 0 / +-1 tables, q scale 2^-3, head-major planes: bit-equal (one rounding of an exactly known value)"""
    from dinounet_amd import _lib
    d = dev()
    Dh, prefix, qscale = 64, 5, 0.125
    M, Npad = B * N, (N + 7) // 8 * 8
    M0 = M - M % 256
    h, w = X.ternary(M, D, seed=41), X.ternary(3 * H * Dh, D, seed=42)
    bias = X.integers(3 * H * Dh, seed=43, lo=-4, hi=4)
    X.require_random(h, w, sin, cos)
    X.require_exact(2 * (X.sum_bound(h, w) + 4), qscale)
    _, want = qkv_reference(h, w, bias, sin, cos, B, N, H, Dh, prefix, qscale)
    X.require_bf16_share(want)
    hd, wd, sd, cd = h.to(d, bf), w.to(d, bf), sin.to(d), cos.to(d)
    plane = B * H * Npad * Dh
    whole = torch.full((3 * plane + X.GUARD_ROWS * Dh,), X.SENTINEL, dtype=bf, device=d)
    qkv3 = whole[:3 * plane].view(3, B, H, Npad, Dh)
    more = {}
    if grid is not None:
        g = _lib.ConvGeom()
        g.Hi, g.Wi = grid
        more["geom"] = g
    with forced(k0=mode) as ops:
        ops.gemm_raw(dtype=_lib.DU_BF16, out_dtype=_lib.DU_BF16, a_mode=ops.PLAIN_ROW, b_mode=ops.PLAIN_ROW, M=M0, N=3 * H * Dh, K=D, A=hd.data_ptr(),
                     lda=D, B=wd.data_ptr(), ldb=D, Cmat=qkv3.data_ptr(), ldc=plane, bias=bias.to(d).data_ptr(), store_mode=ops.STORE_QKV_ROPE,
                     ps=(N, Npad, H), rope=(sd.data_ptr(), cd.data_ptr(), prefix, qscale), **more)
        assert ops.LAST_GEMM_ROUTE == route, ops.LAST_GEMM_ROUTE
        torch.cuda.synchronize()
    sent = torch.tensor(X.SENTINEL).to(bf).to(d)
    assert bool((whole[3 * plane:] == sent).all()), "write behind the v plane"
    # token (b, n) is row b N + n of the product: rows < M0 are written, the others keep the sentinel
    tok = (torch.arange(B)[:, None] * N + torch.arange(N)[None, :]) < M0                       # (B, N)
    got = qkv3[:, :, :, :N].cpu()
    m = tok[None, :, None, :, None].expand_as(got)
    assert bool((got[~m] == sent.cpu()).all()), "rows behind the last full tile were written by a launch of M0 rows"
    assert torch.equal(got[m], X.expected(want, bf)[m]), "RoPE store: " + X.mismatch_report(got.reshape(-1, Dh), torch.where(m, X.expected(want, bf), got).reshape(-1, Dh))


@pytest.mark.parametrize("B,H,N,D", QKV_SHAPES[:3])
def test_qkv_rope_store_exact(B, H, N, D):
    """DU_STORE_QKV_ROPE in the 256 x 128 kernel's epilogue (route 4); a table entry per (token, dimension)"""
    sin, cos = rope_tables(N, 5, 64, seed=44)
    rope_store_case(B, H, N, D, sin, cos, mode=2, route=4)


@pytest.mark.parametrize("B,H,hp,wp,D", [(8, 16, 32, 32, 1024), (2, 6, 32, 32, 384), (3, 12, 16, 24, 768), (9, 16, 32, 32, 1024)])
def test_qkv_rope_in_the_persistent_kernels_drain_exact(B, H, hp, wp, D):
    """DU_STORE_QKV_ROPE in the DRAIN of the persistent kernel (gemm_nt_pp_kernel<.., ROPE>, route 6; the shapes of
    test_vit_qkv_rope_in_the_persistent_kernels_drain): the rotation comes from a factorised table -- dimensions 0..15 of a head follow the
    token's row, 16..31 its column, 32..63 repeat them -- so the 0 / +-1 tables are separable the same way: a random quarter turn per
    (row, dimension) and per (column, dimension).  A row / column mix-up or a wrong half changes the rotated integer."""
    g = torch.Generator().manual_seed(45)
    kr, kc = torch.randint(0, 4, (hp, 16), generator=g), torch.randint(0, 4, (wp, 16), generator=g)
    k = torch.cat([kr[:, None, :].expand(hp, wp, 16), kc[None, :, :].expand(hp, wp, 16)], -1).flatten(0, 1).tile(2)       # (hp wp, 64)
    sin, cos = torch.tensor([0.0, 1.0, 0.0, -1.0])[k].contiguous(), torch.tensor([1.0, 0.0, -1.0, 0.0])[k].contiguous()
    rope_store_case(B, H, 5 + hp * wp, D, sin, cos, mode=4, route=6, grid=(hp, wp))


# ==================================================================================================== 2. backward products
@pytest.mark.parametrize("dt", [f32, bf])
def test_dgrad_wgrad_colsum_exact(dt):
    """test_gemm_dgrad_wgrad's shape: data gradient (W read column-wise), weight gradient (split-K, fp32 atomics: exact in any order), column sums"""
    d = dev()
    M, N, K = 5376 * 2, 192, 384
    x, w, dy = X.ternary(M, K, seed=51), X.ternary(N, K, seed=52), X.ternary(M, N, seed=53)
    X.require_random(x, w, dy)
    X.require_exact(max(X.sum_bound(dy), float(dy.abs().sum(0).max())))
    with forced() as ops:
        dx = ops.mm_dgrad(dy.to(d, dt), w.to(d, dt))
        ref = dy.double() @ w.double()
        if dt == bf:
            X.require_bf16_share(ref)
        X.assert_exact(dx, ref, f"{dt} data gradient")
        dw = ops.mm_wgrad(dy.to(d, dt), x.to(d, dt))
        assert dw.dtype == f32
        X.assert_exact(dw, dy.double().t() @ x.double(), f"{dt} weight gradient")
        X.assert_exact(ops.colsum(dy.to(d, dt)), dy.double().sum(0), f"{dt} column sums")


WGRAD_SHAPES = [(2048, 256, 1024), (4224, 192, 520), (43008, 512, 1024), (8192, 1024, 384), (2304, 320, 264)]


@pytest.mark.parametrize("rows,N,K", WGRAD_SHAPES)
def test_multiphase_wgrad_exact(rows, N, K):
    """weight gradients on gemm_tn_p8_kernel (route 5, key 5 = 2: transpose-read fragments, K-tile pairs over <= 256 workgroups, fp32 atomics)
    and on the 128 x 128 kernel (key 5 = 0), with the bias gradient from the dY fragments (a_colsum); rows = 43008 and the odd K = 520 / 264"""
    d = dev()
    dy, x = X.ternary(rows, N, seed=61), X.ternary(rows, K, seed=62)
    X.require_random(dy, x)
    X.require_exact(float(dy.abs().sum(0).max()))           # column sums bound both the products (|x| <= 1) and the bias gradient
    ref, refb = dy.double().t() @ x.double(), dy.double().sum(0)
    for flag in (2, 0):
        with forced(k5=flag) as ops:
            dw, db = ops.mm_wgrad(dy.to(d, bf), x.to(d, bf), with_colsum=True)
            assert (ops.LAST_GEMM_ROUTE == 5) == (flag == 2), ops.LAST_GEMM_ROUTE
            X.assert_exact(dw, ref, f"key 5 = {flag} weight gradient")
            X.assert_exact(db, refb, f"key 5 = {flag} bias gradient")
            if flag == 2:
                x2 = x.to(d, bf)
                x2[rows - 1, K - 1] = 3.0
                assert not X.is_exact(ops.mm_wgrad(dy.to(d, bf), x2), ref), "the gate did not see one changed term"


TN_GROUP_SHAPES = [(43008, 1024, 512, True), (43008, 192, 1024, True), (8192, 512, 1024, False), (5376, 72, 256, True), (512, 256, 384, True),
                   (2688, 8, 32, False), (16384, 320, 264, True), (1024, 1024, 1024, False)]


def test_tn_group_exact():
    """du_gemm_tn_group: the eight products of test_gemm_tn_group_many_products_one_launch queued and run by ONE launch (one a column slice
    of a wider dY), bias gradients riding along, then every product alone: bit-equal each time"""
    from dinounet_amd import ops
    d = dev()
    ins, refs = [], []
    for i, (rows, N, K, cs) in enumerate(TN_GROUP_SHAPES):
        dy, x = X.ternary(rows, N + (8 if i == 3 else 0), seed=70 + i), X.ternary(rows, K, seed=90 + i)
        dyd = dy.to(d, bf)
        if i == 3:
            dy, dyd = dy[:, :N], dyd[:, :N]
        X.require_exact(float(dy.abs().sum(0).max()))
        ins.append((dyd, x.to(d, bf), cs))
        refs.append((dy.double().t() @ x.double(), dy.double().sum(0)))
    W = ops.WGRAD
    assert W.enabled
    l0 = W.launches
    hold = W._arm
    W._arm = lambda: True
    try:
        outs = [ops.mm_wgrad(a, b, with_colsum=cs, defer=True) for a, b, cs in ins]
        assert len(W.jobs) == len(TN_GROUP_SHAPES)
    finally:
        W._arm = hold
    W.flush()
    assert W.launches - l0 == 1 and not W.jobs
    for (rows, N, K, cs), o, (rw, rb) in zip(TN_GROUP_SHAPES, outs, refs):
        dw, db = (o if cs else (o, None))
        X.assert_exact(dw, rw, f"grouped {rows}x{N}x{K}")
        if cs:
            X.assert_exact(db, rb, f"grouped bias gradient {rows}x{N}x{K}")
    for (rows, N, K, cs), (a, b, _), (rw, rb) in zip(TN_GROUP_SHAPES, ins, refs):
        l1 = W.launches
        X.assert_exact(ops.mm_wgrad(a, b, defer=True), rw, f"alone {rows}x{N}x{K}")
        assert W.launches == l1 + 1
    assert not W.jobs


def test_droppath_scale_inside_backward_gemms_exact():
    """test_linear_droppath_scale_inside_backward_gemms with exact scales {0, 1.5, 2}: from the second step on the per-sample scale is
    applied inside the GEMMs (output rows of the data gradient, contraction rows of the weight gradient on the grouped launch, bias gradient
    from the scaled fragments); all four gradients and the output bit-equal."""
    from dinounet_amd import ops
    d = dev()
    B, T, K, N = 4, 1280, 256, 192
    x, res = X.ternary(B, T, K, seed=101), X.integers(B, T, N, seed=104, lo=-32, hi=32)
    w0, b0 = X.ternary(N, K, seed=102), X.integers(N, seed=103, lo=-4, hi=4)
    mask = torch.tensor([0.0, 1.5, 2.0, 0.0])
    go = X.ternary(B, T, N, seed=105)
    X.require_exact(2 * (K + 4) + 32, 0.5)
    X.require_exact(2.0 * B * T, 0.5)
    xr, wr, br, rr = (t.double().requires_grad_(True) for t in (x, w0, b0, res))
    yr = F.linear(xr, wr, br) * mask.double().view(-1, 1, 1) + rr
    gr = torch.autograd.grad(yr, (xr, wr, br, rr), go.double())
    X.require_bf16_share(yr.detach())
    X.require_bf16_share(gr[0])
    w, b = torch.nn.Parameter(w0.to(d)), torch.nn.Parameter(b0.to(d))

    def step():
        xg, rg = x.to(d, bf).requires_grad_(True), res.to(d, bf).requires_grad_(True)
        ops.TRACK_ROUTE, ops.ROUTES[:] = True, []
        try:
            y = ops.linear(xg, w, b, residual=rg, row_scale=mask.to(d), rs_rows=T)
            g = torch.autograd.grad(y, (xg, w, b, rg), go.to(d, bf))
        finally:
            ops.TRACK_ROUTE = False
        return y, g

    ops.PACK.refresh()
    y0, g0 = step()
    ops.PACK.refresh()
    nq = ops.WGRAD.queued
    y1, g1 = step()
    assert ops.WGRAD.queued == nq + 1 and not ops.WGRAD.jobs                                   # one job per sample on the grouped launch
    assert (ops.PLAIN_ROW, ops.PLAIN_COL) not in [(am, bm) for am, bm, _ in ops.ROUTES]          # W^T packed: scale inside the data gradient
    for tag, y, g in (("first step", y0, g0), ("scale inside the GEMMs", y1, g1)):
        X.assert_exact(y, yr.detach(), tag + ": output")
        for name, a, r_ in zip(("dx", "dw", "db", "dres"), g, gr):
            X.assert_exact(a, r_, f"{tag}: {name}")


# ==================================================================================================== 3. convolutions as implicit GEMMs
def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


CONV3_CFGS = [dict(B=2, H=24, W=16, Cin=64, Cout=32, s=1), dict(B=1, H=32, W=32, Cin=8, Cout=64, s=2),
              dict(B=2, H=17, W=9, Cin=128, Cout=256, s=2), dict(B=1, H=64, W=64, Cin=32, Cout=32, s=1),
              dict(B=2, H=32, W=32, Cin=256, Cout=256, s=2, nobias=True), dict(B=8, H=32, W=32, Cin=128, Cout=256, s=2, nobias=True)]


@pytest.mark.parametrize("dt", [f32, bf])
@pytest.mark.parametrize("cfg", CONV3_CFGS, ids=lambda c: "-".join(str(v) for v in c.values()))
def test_conv3x3_fwd_bwd_exact(dt, cfg):
    """3 x 3 convolution through autograd at test_conv3x3_fwd_bwd's shapes (stride 1 / 2, odd sizes, the SPM's split-K layers: fp32 slabs
    + the in-order slab reduce, DU_STORE_SLABS): output, data gradient, weight gradient, bias gradient bit-equal to fp64 conv2d"""
    from dinounet_amd import ops
    d = dev()
    B, H, W, Cin, Cout, s = (cfg[k] for k in ("B", "H", "W", "Cin", "Cout", "s"))
    x, w = X.ternary(B, Cin, H, W, seed=111), X.ternary(Cout, Cin, 3, 3, seed=112)
    b = None if cfg.get("nobias") else X.integers(Cout, seed=113, lo=-4, hi=4)
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    br = None if b is None else b.double().requires_grad_(True)
    yr = F.conv2d(xr, wr, br, s, 1)
    go = X.ternary(*yr.shape, seed=114)
    X.require_random(x, w, go)
    X.require_exact(max(9 * Cin + 4, 9 * Cout, float(go.abs().sum((0, 2, 3)).max())))
    gr = torch.autograd.grad(yr, (xr, wr) if b is None else (xr, wr, br), go.double())
    if dt == bf:
        X.require_bf16_share(yr.detach())
        X.require_bf16_share(gr[0])
    xg, wg = nhwc(x).to(d, dt).requires_grad_(True), w.to(d).requires_grad_(True)
    bg = None if b is None else b.to(d).requires_grad_(True)
    if cfg.get("nobias") and dt == bf:
        M, Kc = B * (H // 2) * (W // 2), 9 * Cin
        assert ops._im2col_split(M, Cout, Kc) >= 2, "this shape was meant to take the split-K slabs"
    y = ops.conv2d(xg, wg, bg, stride=s, pad=1)
    gg = torch.autograd.grad(y, (xg, wg) if b is None else (xg, wg, bg), nhwc(go).to(d, dt))
    X.assert_exact(y.permute(0, 3, 1, 2), yr.detach(), f"{dt} forward")
    X.assert_exact(gg[0].permute(0, 3, 1, 2), gr[0], f"{dt} data gradient")
    X.assert_exact(gg[1], gr[1], f"{dt} weight gradient")
    if b is not None:
        X.assert_exact(gg[2], gr[2], f"{dt} bias gradient")


@pytest.mark.parametrize("dt", [f32, bf])
def test_conv3x3_fused_concat_exact(dt):
    """conv over cat(up, skip) read through two pointers: both sources' gradients"""
    from dinounet_amd import ops
    d = dev()
    B, H, W, C1, C2, Cout = 2, 32, 32, 32, 32, 32
    a, s2 = X.ternary(B, C1, H, W, seed=121), X.ternary(B, C2, H, W, seed=122)
    w, b = X.ternary(Cout, C1 + C2, 3, 3, seed=123), X.integers(Cout, seed=124, lo=-4, hi=4)
    ar, sr, wr = (t.double().requires_grad_(True) for t in (a, s2, w))
    yr = F.conv2d(torch.cat([ar, sr], 1), wr, b.double(), 1, 1)
    go = X.ternary(*yr.shape, seed=125)
    X.require_random(a, s2, go)
    X.require_exact(max(9 * (C1 + C2) + 4, 9 * Cout, B * H * W))
    gr = torch.autograd.grad(yr, (ar, sr, wr), go.double())
    ag, sg, wg = nhwc(a).to(d, dt).requires_grad_(True), nhwc(s2).to(d, dt).requires_grad_(True), w.to(d).requires_grad_(True)
    y = ops.conv2d(ag, wg, b.to(d), 1, 1, x2=sg)
    gg = torch.autograd.grad(y, (ag, sg, wg), nhwc(go).to(d, dt))
    X.assert_exact(y.permute(0, 3, 1, 2), yr.detach(), "forward")
    X.assert_exact(gg[0].permute(0, 3, 1, 2), gr[0], "gradient of the first source")
    X.assert_exact(gg[1].permute(0, 3, 1, 2), gr[1], "gradient of the second source")
    X.assert_exact(gg[2], gr[2], "weight gradient")


# test_conv3x3_halo_kernel_fwd_bwd_stats' shapes, all of them: the last four are the production sizes (the decoder's 512 x 512 x 32-channel
# layers: several rounds of workgroups per CU, the largest tile and stats_part indices)
HALO_SHAPES = [(2, 16, 32, 64, 0, 32), (1, 24, 16, 32, 32, 32), (2, 8, 16, 64, 64, 64), (1, 16, 16, 128, 128, 128), (1, 32, 48, 32, 0, 64),
               (3, 8, 16, 128, 0, 64), (1, 8, 128, 32, 0, 32), (2, 24, 256, 32, 0, 32), (2, 40, 384, 32, 0, 64), (8, 64, 128, 32, 0, 32),
               (1, 16, 128, 64, 0, 32), (2, 24, 256, 32, 32, 32), (2, 40, 128, 64, 0, 64), (3, 64, 128, 32, 32, 64),
               (8, 512, 512, 32, 0, 32), (8, 512, 512, 32, 32, 32), (8, 512, 512, 32, 0, 64), (8, 256, 256, 64, 0, 64)]
HALO_DENSITY = 0.25          # sparser draw: the second moment of a channel over an image has to stay below 2^24 as well


@pytest.mark.parametrize("B,H,W,C1,C2,Cout", HALO_SHAPES)
def test_conv3x3_halo_and_strip_kernels_exact(B, H, W, C1, C2, Cout):
    """LDS-tiled direct conv and the streaming strip kernel (bf16): forward (+ fused concat), flipped-weight data gradient, weight and bias
    gradient, and the statistics the epilogue emits.  The kernel accumulates the plain value and the plain square of the bf16-rounded output
    (conv_halo.hip: s1 += vq; s2 += vq * vq), so both moments are sums of integers: exact while sum y^2 over an image stays below 2^24,
    which is asserted on the reference (a sparser draw keeps it there; at 512 x 512 the largest second moment is 1.1e7)."""
    from dinounet_amd import ops, _lib
    d = dev()
    Cin = C1 + C2
    x = X.ternary(B, H, W, C1, seed=131, density=HALO_DENSITY)
    x2 = X.ternary(B, H, W, C2, seed=132, density=HALO_DENSITY) if C2 else None
    w, bias = X.ternary(Cout, Cin, 3, 3, seed=133, density=HALO_DENSITY), X.integers(Cout, seed=134, lo=-2, hi=2)
    go = X.ternary(B, H, W, Cout, seed=135)
    xin = torch.cat([x, x2], -1) if C2 else x
    yr, *gr = X.conv3x3_ref64(xin, w, bias, go)          # fp64, the whole tensor at every size (nine shifted products)
    X.require_random(x, w, go)
    X.require_exact(max(9 * Cin + 2, 9 * Cout, B * H * W))
    X.require_bf16_share(yr, least=1.0)              # the statistics are taken of the stored bf16 values: every one must be the true value
    X.require_bf16_share(gr[0])
    s1, s2 = yr.sum((1, 2)), (yr * yr).sum((1, 2))                          # (B, Cout)
    X.require_exact(float(max(yr.abs().sum((1, 2)).max(), s2.max())))
    xg = x.to(d, bf).requires_grad_(True)
    x2g = x2.to(d, bf).requires_grad_(True) if C2 else None
    wg, bg = w.to(d).requires_grad_(True), bias.to(d).requires_grad_(True)
    y, part = ops.conv2d_stats(xg, wg, bg, 1, 1, x2g)
    assert part is not None, "shape should be served by the halo / strip kernel, statistics included"
    gg = torch.autograd.grad(y, (xg, x2g, wg, bg) if C2 else (xg, wg, bg), go.to(d, bf))
    X.assert_exact(y, yr, "forward")
    gx = torch.cat([gg[0], gg[1]], -1) if C2 else gg[0]
    X.assert_exact(gx, gr[0], "data gradient")
    X.assert_exact(gg[-2], gr[1], "weight gradient")
    X.assert_exact(gg[-1], gr[2], "bias gradient")
    sums = torch.empty((B, Cout, 2), dtype=f32, device=d)
    _lib.check(_lib.lib().du_strip_finalize(C.c_void_p(part.data_ptr()), C.c_void_p(sums.data_ptr()), B, part.shape[0] // B, Cout,
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)), "du_strip_finalize")
    X.assert_exact(sums.view(B, Cout, 2)[..., 0], s1, "statistics: sums", sentinel=False)
    X.assert_exact(sums.view(B, Cout, 2)[..., 1], s2, "statistics: second moments", sentinel=False)


@pytest.mark.parametrize("Cin,Cout,off,wide", [(32, 32, 32, 96), (64, 64, 16, 96), (64, 32, 0, 72), (32, 64, 8, 40)])
def test_conv3x3_strip_kernel_on_channel_slices_exact(Cin, Cout, off, wide):
    """a channel slice of a wider NHWC tensor read in place through the pixel pitch: the neighbouring channels are random too, so a wrong
    pitch or offset changes the sum"""
    from dinounet_amd import ops
    d = dev()
    B, H, W = 2, 24, 256
    xw = X.ternary(B, H, W, wide, seed=141)
    w, bias = X.ternary(Cout, Cin, 3, 3, seed=142), X.integers(Cout, seed=143, lo=-4, hi=4)
    X.require_exact(9 * Cin + 4)
    yr = F.conv2d(xw[..., off:off + Cin].double().permute(0, 3, 1, 2), w.double(), bias.double(), 1, 1).permute(0, 2, 3, 1)
    X.require_bf16_share(yr)
    x = xw.to(d, bf)[..., off:off + Cin]
    assert not x.is_contiguous()
    y, part = ops.conv2d_stats(x, w.to(d), bias.to(d), 1, 1)
    assert part is not None
    X.assert_exact(y, yr, "strip kernel on a channel slice")


ROWS_SHAPES = [(1, 8, 16, 32, 0, 32), (1, 8, 32, 64, 0, 64), (3, 40, 80, 96, 0, 32), (2, 24, 16, 32, 32, 64), (5, 64, 64, 64, 64, 64),
               (2, 16, 48, 64, 0, 32), (7, 8, 16, 32, 0, 64), (2, 128, 256, 64, 0, 64), (4, 264, 272, 32, 0, 32),
               (1, 8, 16, 128, 0, 128), (2, 64, 64, 128, 128, 128), (3, 128, 128, 128, 0, 128), (1, 16, 32, 96, 32, 128)]


@pytest.mark.parametrize("B,H,W,C1,C2,Cout", ROWS_SHAPES)
def test_conv3x3_weight_gradient_rows_kernel_exact(B, H, W, C1, C2, Cout):
    """du_conv3x3_wgrad_halo: the round-5 rows kernel (key 13 = 2) and the round-3 kernel (0; it does not serve 128 outputs), with and
    without the bias-gradient sums: (Cout, 9 Cin) bit-equal.  Reference: nine shifted fp64 products, one per tap."""
    from dinounet_amd import ops
    d = dev()
    Cin = C1 + C2
    x = X.ternary(B, H, W, C1, seed=151)
    x2 = X.ternary(B, H, W, C2, seed=152) if C2 else None
    go = X.ternary(B, H, W, Cout, seed=153)
    X.require_random(x, go)
    X.require_exact(B * H * W)
    xin = (torch.cat([x, x2], -1) if C2 else x).double()
    xp = F.pad(xin, (0, 0, 1, 1, 1, 1))
    g2 = go.double().reshape(-1, Cout)
    ref = torch.stack([g2.t() @ xp[:, ky:ky + H, kx:kx + W].reshape(-1, Cin) for ky in range(3) for kx in range(3)], 1).reshape(Cout, 9 * Cin)
    ref_db = go.double().sum((0, 1, 2))
    xd, gd, x2d = x.to(d, bf), go.to(d, bf), (x2.to(d, bf) if C2 else None)
    for mode in ((2,) if Cout == 128 else (2, 0)):
        with forced(k13=mode) as ops:
            for with_db in (False, True):
                r = ops.conv3x3_wgrad_halo(xd, gd, x2d, with_db=with_db)
                assert r is not None
                dw, db = r if with_db else (r, None)
                X.assert_exact(dw, ref, f"key 13 = {mode}, with_db {with_db}")
                if with_db:
                    X.assert_exact(db, ref_db, f"key 13 = {mode} bias gradient")


GROUPED3_SHAPES = [(1, 64, 64, 128, 128, 128, True), (2, 32, 64, 128, 0, 128, True), (1, 64, 128, 256, 0, 128, False), (2, 16, 64, 40, 24, 128, True)]


@pytest.mark.parametrize("B,H,W,C1,C2,Cout,bias", GROUPED3_SHAPES)
def test_conv3x3_weight_gradient_on_the_grouped_launch_exact(B, H, W, C1, C2, Cout, bias):
    """3 x 3 weight gradient of the 128-output layers as queued jobs of du_gemm_tn_group (gather = 3: per-lane tap offsets, zero padding by
    a border mask, one job per source of the concat, (Cout, Cin, 3, 3) written directly)"""
    from dinounet_amd import ops
    d = dev()
    Cin = C1 + C2
    x = X.ternary(B, H, W, C1, seed=161)
    x2 = X.ternary(B, H, W, C2, seed=162) if C2 else None
    w, bv = X.ternary(Cout, Cin, 3, 3, seed=163), X.integers(Cout, seed=164, lo=-4, hi=4)
    go = X.ternary(B, H, W, Cout, seed=165)
    X.require_exact(B * H * W)
    xin = torch.cat([x, x2], -1) if C2 else x
    wr, br = w.double().requires_grad_(True), bv.double().requires_grad_(True)
    yr = F.conv2d(xin.double().permute(0, 3, 1, 2), wr, br if bias else None, 1, 1).permute(0, 2, 3, 1)
    gr = torch.autograd.grad(yr, (wr, br) if bias else (wr,), go.double())
    xg = x.to(d, bf).requires_grad_(True)
    x2g = x2.to(d, bf).requires_grad_(True) if C2 else None
    wg = torch.nn.Parameter(w.to(d))
    bg = torch.nn.Parameter(bv.to(d)) if bias else None
    n0 = ops.WGRAD.queued
    y = ops.conv2d(xg, wg, bg, 1, 1, x2g)
    gg = torch.autograd.grad(y, (wg, bg) if bias else (wg,), go.to(d, bf))
    assert ops.WGRAD.queued == n0 + 1 and not ops.WGRAD.jobs
    X.assert_exact(gg[0], gr[0], "grouped 3 x 3 weight gradient")
    if bias:
        X.assert_exact(gg[1], gr[1], "bias gradient")


# ---------------------------------------------------------------------------------------------------- ConvTranspose 2 x 2, every kernel it has
CONVT_SHAPES = {"generic": [(2, 16, 16, 256, 128), (1, 8, 12, 32, 32), (2, 4, 4, 384, 384)],
                "gather": [(8, 16, 16, 256, 256), (4, 16, 32, 384, 512)],
                "streaming": [(2, 64, 64, 32, 32), (1, 96, 64, 64, 32), (4, 32, 32, 128, 64), (5, 40, 24, 64, 64)],
                "persistent": [(2, 64, 64, 1024, 1024), (1, 32, 64, 384, 256), (3, 16, 32, 512, 128)],
                "grouped": [(2, 16, 16, 256, 128), (2, 16, 32, 32, 32), (4, 16, 16, 384, 384), (2, 32, 32, 64, 32), (1, 32, 64, 24, 40)]}


def convt_case(B, H, W, Cin, Cout, seed, bias=True, residual=False):
    x, w = X.ternary(B, Cin, H, W, seed=seed), X.ternary(Cin, Cout, 2, 2, seed=seed + 1)
    b = X.integers(Cout, seed=seed + 2, lo=-4, hi=4) if bias else None
    res = X.integers(B, Cout, 2 * H, 2 * W, seed=seed + 3, lo=-32, hi=32) if residual else None
    go = X.ternary(B, Cout, 2 * H, 2 * W, seed=seed + 4)
    X.require_random(x, w, go)
    X.require_exact(max(Cin + 4 + 32, 4 * Cout, 4.0 * B * H * W))
    leaves = [t.double().requires_grad_(True) for t in (x, w)] + ([b.double().requires_grad_(True)] if bias else [])
    yr = F.conv_transpose2d(leaves[0], leaves[1], leaves[2] if bias else None, stride=2)
    if residual:
        yr = yr + res.double()
    gr = torch.autograd.grad(yr, leaves, go.double())
    return x, w, b, res, go, yr.detach(), gr


def convt_check(dt, y, gg, yr, gr, what):
    if dt == bf:
        X.require_bf16_share(yr)
        X.require_bf16_share(gr[0])
    X.assert_exact(y.permute(0, 3, 1, 2), yr, what + ": forward")
    X.assert_exact(gg[0].permute(0, 3, 1, 2), gr[0], what + ": data gradient")
    for name, a, r_ in zip(("weight gradient", "bias gradient"), gg[1:], gr[1:]):
        X.assert_exact(a, r_, f"{what}: {name}")


@pytest.mark.parametrize("dt", [f32, bf])
@pytest.mark.parametrize("B,H,W,Cin,Cout", CONVT_SHAPES["generic"])
def test_conv_transpose2x2_generic_exact(dt, B, H, W, Cin, Cout):
    from dinounet_amd import ops
    d = dev()
    x, w, b, _, go, yr, gr = convt_case(B, H, W, Cin, Cout, seed=171)
    xg, wg, bg = nhwc(x).to(d, dt).requires_grad_(True), w.to(d).requires_grad_(True), b.to(d).requires_grad_(True)
    y = ops.conv_transpose2x2(xg, wg, bg)
    gg = torch.autograd.grad(y, (xg, wg, bg), nhwc(go).to(d, dt))
    convt_check(dt, y, gg, yr, gr, f"{dt} generic")


@pytest.mark.parametrize("B,H,W,Cin,Cout", CONVT_SHAPES["gather"])
def test_conv_transpose2x2_gather_kernels_exact(B, H, W, Cin, Cout):
    """backward on the multi-phase kernels' gather forms (key 0 = 1, key 5 = 2: routes 3 and 5) and on the im2col kernels (0 / 0: route 1)"""
    d = dev()
    x, w, _, _, go, yr, gr = convt_case(B, H, W, Cin, Cout, seed=181, bias=False)
    for mode in (1, 0):
        with forced(k0=mode, k5=2 if mode else 0) as ops:
            xg, wg = nhwc(x).to(d, bf).requires_grad_(True), w.to(d).requires_grad_(True)
            y = ops.conv_transpose2x2(xg, wg, None)
            ops.ROUTES[:] = []
            gg = torch.autograd.grad(y, (xg, wg), nhwc(go).to(d, bf))
            routes = {(am, bm): r for am, bm, r in ops.ROUTES}
            want = (3, 5) if mode else (1, 1)
            assert (routes[(ops.IM2COL_ROW, ops.PLAIN_ROW)], routes[(ops.PLAIN_COL, ops.IM2COL_COL)]) == want, routes
            convt_check(bf, y, gg, yr, gr, f"gather kernels key 0 = {mode}")


@pytest.mark.parametrize("B,H,W,Ci,Co", CONVT_SHAPES["streaming"])
def test_conv_transpose2x2_streaming_kernel_exact(B, H, W, Ci, Co):
    """through gemm_nt_rk_kernel (key 12 = 3): the forward's pixel-shuffle store and the data gradient's 2 x 2 patch gather"""
    d = dev()
    x, w, b, _, go, yr, gr = convt_case(B, H, W, Ci, Co, seed=191)
    with forced(k12=3) as ops:
        xg, wg, bg = nhwc(x).to(d, bf).requires_grad_(True), w.to(d).requires_grad_(True), b.to(d).requires_grad_(True)
        y = ops.conv_transpose2x2(xg, wg, bg)
        gg = torch.autograd.grad(y, (xg, wg, bg), nhwc(go).to(d, bf))
        routes = [r for _, _, r in ops.ROUTES]
        assert routes.count(7) >= (2 if 4 * Co <= 256 else 1), routes
        convt_check(bf, y, gg, yr, gr, "streaming kernel")


@pytest.mark.parametrize("B,H,W,Cin,Cout", CONVT_SHAPES["persistent"])
def test_conv_transpose2x2_residual_persistent_kernel_exact(B, H, W, Cin, Cout):
    """DU_STORE_PIXEL_SHUFFLE2 with the bf16 residual read through the same pixel mapping as two more K-steps (route 6, key 0 = 4), and on
    the one-shot kernel (key 0 = 1, key 14 = 0: route 3)"""
    d = dev()
    x, w = X.ternary(B, Cin, H, W, seed=201), X.ternary(Cin, Cout, 2, 2, seed=202)
    b, res = X.integers(Cout, seed=203, lo=-4, hi=4), X.integers(B, Cout, 2 * H, 2 * W, seed=204, lo=-32, hi=32)
    X.require_random(x, w, res)
    X.require_exact(Cin + 4 + 32)
    ref = F.conv_transpose2d(x.double(), w.double(), b.double(), stride=2) + res.double()
    X.require_bf16_share(ref)
    xg, rg = nhwc(x).to(d, bf), nhwc(res).to(d, bf)
    for mode, k14, route in ((4, 1, 6), (1, 0, 3)):
        with forced(k0=mode, k14=k14) as ops:
            with torch.no_grad():
                y = ops.conv_transpose2x2(xg, w.to(d), b.to(d), residual=rg)
            assert ops.LAST_GEMM_ROUTE == route, (mode, ops.LAST_GEMM_ROUTE)
            X.assert_exact(y.permute(0, 3, 1, 2), ref, f"pixel-shuffle store + residual, route {route}")


@pytest.mark.parametrize("B,H,W,Cin,Cout,bias", [c + (c != (4, 16, 16, 384, 384),) for c in CONVT_SHAPES["grouped"]])
def test_conv_transpose2x2_weight_gradient_grouped_launch_exact(B, H, W, Cin, Cout, bias):
    """weight (and bias) gradient as a queued job of du_gemm_tn_group (gather = 2), written in the parameter's (Cin, Cout, 2, 2) layout"""
    from dinounet_amd import ops
    d = dev()
    x, w, b, _, go, yr, gr = convt_case(B, H, W, Cin, Cout, seed=211, bias=bias)
    xg = nhwc(x).to(d, bf).requires_grad_(True)
    wg = torch.nn.Parameter(w.to(d))
    bg = torch.nn.Parameter(b.to(d)) if bias else None
    n0 = ops.WGRAD.queued
    y = ops.conv_transpose2x2(xg, wg, bg)
    gg = torch.autograd.grad(y, (wg, bg) if bias else (wg,), nhwc(go).to(d, bf))
    assert ops.WGRAD.queued == n0 + 1 and not ops.WGRAD.jobs
    assert gg[0].shape == wg.shape and gg[0].is_contiguous()
    X.assert_exact(gg[0], gr[1], "grouped ConvTranspose weight gradient")
    if bias:
        X.assert_exact(gg[1], gr[2], "bias gradient")


@pytest.mark.parametrize("dt", [f32, bf])
def test_conv_transpose2x2_fused_residual_exact(dt):
    """skip add in the epilogue on the generic kernels: the residual has the output (pixel-shuffled) layout; its gradient is dy itself"""
    from dinounet_amd import ops
    d = dev()
    B, H, W, Cin, Cout = 2, 8, 12, 64, 64
    x, w, b, res, go, yr, gr = convt_case(B, H, W, Cin, Cout, seed=221, residual=True)
    xg, rg = nhwc(x).to(d, dt).requires_grad_(True), nhwc(res).to(d, dt).requires_grad_(True)
    y = ops.conv_transpose2x2(xg, w.to(d), b.to(d), residual=rg)
    gg = torch.autograd.grad(y, (xg, rg), nhwc(go).to(d, dt))
    X.assert_exact(y.permute(0, 3, 1, 2), yr, "forward + residual")
    X.assert_exact(gg[0].permute(0, 3, 1, 2), gr[0], "data gradient")
    X.assert_exact(gg[1].permute(0, 3, 1, 2), go.double(), "gradient of the residual")


# ---------------------------------------------------------------------------------------------------- segmentation head, depthwise 3 x 3
@pytest.mark.parametrize("B,H,W,K,ld", [(2, 24, 40, 2, 32), (1, 17, 13, 1, 32), (3, 8, 16, 3, 32), (2, 33, 9, 4, 32), (2, 16, 16, 2, 64)])
def test_seg_head_streaming_kernels_exact(B, H, W, K, ld):
    """32 channels -> K classes as one streaming pass: fp32 logits, dx (bf16), dw, db from ONE backward pass.  The logit gradient is fp32, so it
    is drawn from integers in [-3, 3] (products with ternary weights / features stay integers)."""
    from dinounet_amd import ops
    d = dev()
    xfull = X.ternary(B, H, W, ld, seed=231)
    w, b = X.ternary(K, 32, 1, 1, seed=232), X.integers(K, seed=233, lo=-4, hi=4)
    go = X.integers(B, K, H, W, seed=234, lo=-3, hi=3)
    X.require_exact(max(32 + 4, 3 * K, 3.0 * B * H * W))
    xr, wr, br = xfull[..., :32].double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    yr = F.conv2d(xr.permute(0, 3, 1, 2), wr, br)
    gr = torch.autograd.grad(yr, (xr, wr, br), go.double())
    xg_full = xfull.to(d, bf).requires_grad_(True)
    xg = xg_full[..., :32]
    assert ops.seg_head_ok(xg, K)
    wg, bg = w.to(d).requires_grad_(True), b.to(d).requires_grad_(True)
    y = ops.seg_head(xg, wg, bg)
    assert y.shape == (B, K, H, W) and y.dtype == f32
    X.assert_exact(y, yr.detach(), "logits")
    gx, gw, gb = torch.autograd.grad(y, (xg_full, wg, bg), go.to(d))
    X.assert_exact(gx[..., :32], gr[0], "dx")
    if ld > 32:
        assert float(gx[..., 32:].abs().max()) == 0.0, "gradient written outside the 32-channel slice"
    X.assert_exact(gw, gr[1], "dw")
    X.assert_exact(gb, gr[2], "db")


@pytest.mark.parametrize("dt", [f32, bf])
def test_dwconv3x3_exact(dt):
    """depthwise 3 x 3 on an NHWC tensor (odd 9 x 7 grid) and on the adapter's token pyramid (three grids in one token axis), no activation
    in the exact part: output, input gradient, weight and bias gradient"""
    from dinounet_amd import ops
    from dinounet_amd._lib import ACT_NONE
    d = dev()
    B, H, W, Cc = 2, 4, 6, 96
    n = H * W // 4
    N = 21 * n
    x, w, b = X.ternary(B, N, Cc, seed=241), X.ternary(Cc, 1, 3, 3, seed=242), X.integers(Cc, seed=243, lo=-4, hi=4)
    go = X.ternary(B, N, Cc, seed=244)
    X.require_exact(max(9 + 4, 9, B * N))
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    outs = []
    for (lo, hi, h, ww) in ((0, 16 * n, 2 * H, 2 * W), (16 * n, 20 * n, H, W), (20 * n, N, H // 2, W // 2)):
        t = xr[:, lo:hi].transpose(1, 2).reshape(B, Cc, h, ww)
        outs.append(F.conv2d(t, wr, br, 1, 1, groups=Cc).flatten(2).transpose(1, 2))
    yr = torch.cat(outs, 1)
    gr = torch.autograd.grad(yr, (xr, wr, br), go.double())
    xg, wg, bg = x.to(d, dt).requires_grad_(True), w.to(d).requires_grad_(True), b.to(d).requires_grad_(True)
    y = ops.dwconv_tokens(xg, wg, bg, H, W, ACT_NONE)
    gg = torch.autograd.grad(y, (xg, wg, bg), go.to(d, dt))
    X.assert_exact(y, yr.detach(), "token pyramid forward")
    for name, a, r_ in zip(("dx", "dw", "db"), gg, gr):
        X.assert_exact(a, r_, "token pyramid " + name)
    x4 = X.ternary(B, Cc, 9, 7, seed=245)
    y4 = ops.dwconv3x3(nhwc(x4).to(d, dt), w.to(d), b.to(d), ACT_NONE)
    X.assert_exact(y4.permute(0, 3, 1, 2), F.conv2d(x4.double(), w.double(), b.double(), 1, 1, groups=Cc), "NHWC forward")


# ==================================================================================================== part 2: derived per-element bounds
# Non-linear epilogues: the pre-activation s is exact (ternary A, B in {-1, 0, 1} / 32, bias in 1/32 steps: sums are multiples of 1/32 with a
# spread of 0.3 .. 1.3), so the only errors left are the activation's evaluation and the output rounding:
#     |out - act64(s)| <= u_out |act64(s)| + e_act max(1, |s|)          per element (tests/_exact.py: E_ACT_*, measured, capped at 2^-12)
def gelu_case(M, N, K):
    key = ("gelu", M, N, K)
    if _CASE.get("key") == key:
        return _CASE["val"]
    x, w = X.ternary(M, K, seed=251), X.ternary(N, K, seed=252) / 32
    b = X.integers(N, seed=253, lo=-16, hi=16) / 32
    X.require_random(x, w, b)
    X.require_exact(X.sum_bound(x, w) + 0.5, 1.0 / 32)
    rows = X.check_rows(M)
    s = (x if rows is None else x[rows]).double() @ w.double().t() + b.double()
    _CASE["key"], _CASE["val"] = key, (x, w, b, s, X.gelu64(s), rows)
    return _CASE["val"]


@pytest.mark.parametrize("mode", [0, 1, 2, 4])
@pytest.mark.parametrize("M,N,K", GELU_SHAPES)
def test_gelu_epilogue_per_element_bound(mode, M, N, K):
    """fc1 + bias + erf-GELU (K = 1024; 896 / 640: the persistent kernel's drain over 8 K-steps; 256: the four-K-step form) on every NT
    family, bf16 results and -- where the family has an fp32 store -- fp32 results, against gelu in fp64 of the exact pre-activation.  The
    fp32 launches print the figure E_ACT_GELU is derived from.  (tanh-GELU fails this gate on the CPU emulation, tests/test_cpu_exact.py.)"""
    from dinounet_amd._lib import ACT_GELU
    d = dev()
    x, w, b, s, ref, rows = gelu_case(M, N, K)
    xd, wd, bd = x.to(d, bf), w.to(d, bf), b.to(d)
    with forced(k0=mode) as ops:
        for od in (bf, f32):
            whole, out = X.guarded(M, N, od, d)
            ops.mm(xd, wd, out=out, bias=bd, act=ACT_GELU)
            route = ops.LAST_GEMM_ROUTE
            assert route == expect_route(mode, N, K, od, {"bias": 1}), (mode, od, route)
            torch.cuda.synchronize()
            X.assert_guard(whole, M, f"gelu mode {mode} {od}")
            got = out if rows is None else out[rows.to(d)]
            if od == f32:
                print(f"gelu mode {mode} route {route} {M}x{N}x{K} fp32: measured e_act {X.measured_e_act(got, ref, s):.3e} (max |s| {float(s.abs().max()):.2f})")
            X.assert_act(got, ref, s, X.E_ACT_GELU, f"gelu mode {mode} route {route} {od}")


@pytest.mark.parametrize("mode", [1, 2])
def test_swiglu_epilogue_per_element_bound(mode):
    """SwiGLU on the interleaved projection at the 7B width (D 4096 -> 2 x 8192 columns, gate and value in neighbouring columns; the gate
    epilogue exists on the multi-phase kernels only, bf16 results): silu(g) v against fp64 of the exact g, v; the allowance scales with
    |g v| (sigmoid's relative error times the product)."""
    from dinounet_amd._lib import ACT_SWIGLU, DU_BF16
    d = dev()
    M, K, h = 1029, 4096, 8192
    x = X.ternary(M, K, seed=261)
    w12 = X.ternary(2 * h, K, seed=262) / 32
    b12 = X.integers(2 * h, seed=263, lo=-16, hi=16) / 32
    X.require_random(x, w12, b12)
    X.require_exact(X.sum_bound(x, w12) + 0.5, 1.0 / 32)
    u = x.double() @ w12.double().t() + b12.double()
    g, v = u[:, 0::2], u[:, 1::2]                      # ops.interleave_pairs: rows (2j, 2j + 1) = (w1[j], w2[j])
    ref = X.swiglu64(g, v)
    xd, wd, bd = x.to(d, bf), w12.to(d, bf), b12.to(d)
    with forced(k0=mode) as ops:
        route = ops.gemm_route(dtype=DU_BF16, out_dtype=DU_BF16, a_mode=ops.PLAIN_ROW, b_mode=ops.PLAIN_ROW, M=M, N=2 * h, K=K, A=xd.data_ptr(), lda=K,
                               B=wd.data_ptr(), ldb=K, Cmat=xd.data_ptr(), ldc=h, bias=bd.data_ptr(), act=ACT_SWIGLU)
        assert route in (3, 4), route                  # the gate runs in a multi-phase kernel's epilogue, not as du_swiglu_pairs behind a plain product
        n0 = len(ops.ROUTES)
        out = ops.mm_swiglu(xd, wd, bd)
        assert len(ops.ROUTES) == n0, "mm_swiglu fell back to the plain product + du_swiglu_pairs"
        torch.cuda.synchronize()
    o = out.cpu()
    exact = ref.float().to(bf).double() == ref
    excess = ((o.double() - ref).abs() - X.U_BF16 * ref.abs()).clamp_min(0) / (g * v).abs().clamp_min(1.0)
    print(f"swiglu mode {mode} route {route}: measured e_act on the {int(exact.sum())} elements bf16 holds exactly "
          f"{float(((o.double() - ref).abs() / (g * v).abs().clamp_min(1.0))[exact].max()):.3e}; excess over the output rounding elsewhere {float(excess.max()):.3e}")
    X.assert_act(out, ref, g * v, X.E_ACT_SWIGLU, f"swiglu mode {mode}")


# ---------------------------------------------------------------------------------------------------- attention at the size its configuration names
ATTN_KERNELS = [(0, 0, "product"), (1, 0, "round 3"), (0, 1, "64 q per wave"), (0, 9, "slot-pipelined")]       # as tests/test_gpu_ops.py


def attn_raw(q_, k_, v_, B, H, N, Dh):
    from dinounet_amd import _lib
    Npad = q_.shape[2]
    out = torch.full((B * N + X.GUARD_ROWS, H * Dh), X.SENTINEL, dtype=bf, device=q_.device)
    _lib.check(_lib.lib().du_attention_fwd(C.c_void_p(q_.data_ptr()), C.c_void_p(k_.data_ptr()), C.c_void_p(v_.data_ptr()), C.c_void_p(out.data_ptr()),
                                          B, H, N, Npad, Dh, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "du_attention_fwd")
    torch.cuda.synchronize()
    X.assert_guard(out, B * N, "attention")
    return out[:B * N]


def attn_check(out, q_, k_, v_, B, H, N, Dh, heads, what):
    """all heads finite; the listed heads of every batch entry against the fp64 softmax within the derived bound (tests/_exact.py:
    attention_ref64).  Returns the worst |out - ref| / bound."""
    o = out.float().cpu().view(B, N, H, Dh)
    assert bool(torch.isfinite(o).all()), what
    qc, kc, vc = q_.cpu(), k_.cpu(), v_.cpu()
    worst = 0.0
    for b in range(B):
        for h in heads:
            ref, bound = X.attention_ref64(qc[b, h], kc[b, h], vc[b, h], N)
            ratio = (o[b, :, h].double() - ref).abs() / bound
            worst = max(worst, float(ratio.max()))
            assert float(ratio.max()) <= 1.0, (f"{what}: batch {b} head {h}: {int((ratio > 1).sum())} elements outside the bound, worst ratio {float(ratio.max()):.3f} at "
                                               f"(query, dim) {divmod(int(ratio.argmax()), Dh)}")
    return worst


@pytest.mark.parametrize("impl,var,name", ATTN_KERNELS)
@pytest.mark.parametrize("B,H,N,Dh", [(1, 32, 4101, 128), (2, 16, 4101, 64)])
def test_attention_at_4101_tokens(impl, var, name, B, H, N, Dh):
    """N = 4101 tokens (a 1024 x 1024 input: 64 x 64 patches + 5 prefix tokens), d_head 128 at 32 heads and d_head 64 at 16: random bf16
    operands as test_attention_kernels_vs_fp64_softmax draws them (padding keys random, not zero); all heads run and are checked for
    finiteness, heads 0, 1, the middle one and H - 1 of every batch entry against the fp64 softmax:
        |out - ref| <= 2^-8 |ref| + (2^-8 + N 2^-24 + c_s) sum_k p_k |v_k|."""
    from dinounet_amd import _lib
    L = _lib.lib()
    d = dev()
    Npad = (N + 7) // 8 * 8
    g = torch.Generator().manual_seed(N + Dh)
    q_ = (torch.randn(B, H, Npad, Dh, generator=g) * Dh ** -0.5 * math.log2(math.e)).to(d, bf)
    k_ = torch.randn(B, H, Npad, Dh, generator=g).to(d, bf)
    v_ = torch.randn(B, H, Npad, Dh, generator=g).to(d, bf)
    L.du_set_option(6, impl); L.du_set_option(8, var)
    try:
        out = attn_raw(q_, k_, v_, B, H, N, Dh)
    finally:
        L.du_set_option(6, 0); L.du_set_option(8, 0)
    worst = attn_check(out, q_, k_, v_, B, H, N, Dh, sorted({0, 1, H // 2, H - 1}), name)
    print(f"attention {name} B{B} H{H} N{N} Dh{Dh}: worst |out - ref| / bound {worst:.3f}")


@pytest.mark.parametrize("impl,var,name", ATTN_KERNELS)
@pytest.mark.parametrize("Dh", [64, 128])
def test_attention_spiked_keys_beyond_1029(impl, var, name, Dh):
    """the spiked-key cases of test_attention_spiked_keys_and_forced_rescale at N = 4101 with the spikes in the first tile, in middle tiles
    beyond key 1029 and in the last ragged tile (keys 4096-4100): scores 100 - 600 (log2 units) above everything seen so far"""
    from dinounet_amd import _lib
    L = _lib.lib()
    d = dev()
    B, H, N = 1, 2, 4101
    Npad = (N + 7) // 8 * 8
    g = torch.Generator().manual_seed(5)
    cases = [[(5, 10, 300.0)], [(5, 2052, 300.0)], [(5, 4098, 300.0)], [(5, 100, 140.0), (40, 2708, 600.0), (70, 4100, 250.0)],
             [(5, 1500, 100.0), (5, 3000, 300.0)], [(4099, 64, 200.0), (300, 4096, 200.0)]]
    L.du_set_option(6, impl); L.du_set_option(8, var)
    try:
        for spikes in cases:
            q_ = (torch.randn(B, H, Npad, Dh, generator=g) * 0.05).to(d, bf)
            k_ = (torch.randn(B, H, Npad, Dh, generator=g) * 0.05).to(d, bf)
            v_ = torch.randn(B, H, Npad, Dh, generator=g).to(d, bf)
            for h in range(H):
                for qrow, key, val in spikes:
                    q_[0, h, qrow] = 0; q_[0, h, qrow, (qrow + h) % Dh] = 1.0
                for qrow, key, val in spikes:
                    k_[0, h, key, (qrow + h) % Dh] = val
            out = attn_raw(q_, k_, v_, B, H, N, Dh)
            attn_check(out, q_, k_, v_, B, H, N, Dh, range(H), f"{name} {spikes}")
    finally:
        L.du_set_option(6, 0); L.du_set_option(8, 0)


# ==================================================================================================== 4. multi-scale deformable attention
def msda_ref64(value, shapes, loc, attn, go):
    """ms_deform_attn_core_pytorch in fp64 with its autograd gradients (value (N, S, M, D), loc (N, Lq, M, L, P, 2) as (x, y) in [0, 1],
    attn (N, Lq, M, L, P)) -> out (N, Lq, M D), grad_value, grad_loc, grad_attn.  On the inputs below every term is a dyadic fraction."""
    v, l, a = (t.double().requires_grad_(True) for t in (value, loc, attn))
    N, S, M, D = v.shape
    _, Lq, _, L, P, _ = l.shape
    grids, outs, start = 2 * l - 1, [], 0
    for lvl, (H, W) in enumerate(shapes):
        vl = v[:, start:start + H * W].permute(0, 2, 3, 1).reshape(N * M, D, H, W)
        g = grids[:, :, :, lvl].transpose(1, 2).flatten(0, 1)
        outs.append(F.grid_sample(vl, g, mode="bilinear", padding_mode="zeros", align_corners=False))
        start += H * W
    a2 = a.transpose(1, 2).reshape(N * M, 1, Lq, L * P)
    out = (torch.stack(outs, -2).flatten(-2) * a2).sum(-1).view(N, M * D, Lq).transpose(1, 2)
    gv, gl, ga = torch.autograd.grad(out, (v, l, a), go.double())
    return out.detach(), gv, gl, ga


@pytest.mark.parametrize("dt", [f32, bf])
@pytest.mark.parametrize("N,M,D,levels", [(2, 16, 32, ((64, 64), (32, 32), (16, 16))), (1, 6, 12, ((32, 32),)), (2, 4, 8, ((16, 32), (8, 8)))])
def test_msda_exact(dt, N, M, D, levels):
    """forward, grad_value, grad of the sampling locations and of the attention weights on power-of-two level sizes (the production levels
    64 / 32 / 16 are): integer values and output gradients, attention weights in sixteenths, sampling locations (m / 4 + 0.5) / W so that pixel
    coordinates are quarters and every bilinear weight a multiple of 1 / 16 -- every term a multiple of 2^-8 (times the power-of-two level
    size in grad_loc), exact in any atomic order.  Locations lie inside, on the border (x = -0.75 .. 0, W - 1 .. W) and fully outside on
    both sides (x down to -2.5 and up to W + 2.5); x = -1 exactly is left out: the bilinear derivative is one-sided there and the kernel
    (sample skipped) and grid_sample (zero-weight corner differentiated) pick different sides.  bf16: halves instead of quarters and weights in quarters, so that the results
    the kernel stores in bf16 are numbers bf16 holds (asserted)."""
    from dinounet_amd import ops
    d = dev()
    L, P = len(levels), 4
    S = sum(h * w for h, w in levels)
    Lq = S
    step = 1 if dt == f32 else 2                       # quarters / halves of a pixel
    value = X.ternary(N, S, M, D, seed=271)
    g = torch.Generator().manual_seed(272)
    loc = torch.empty(N, Lq, M, L, P, 2)
    for lvl, (H, W) in enumerate(levels):
        for axis, size in ((0, W), (1, H)):
            m = torch.randint(-(10 // step), (4 * size + 10) // step + 1, (N, Lq, M, P), generator=g) * step       # x = m / 4 in [-2.5, size + 2.5]
            m[m == -4] = -4 - step                     # (x = -1 exactly: see above)
            loc[:, :, :, lvl, :, axis] = (m.float() / 4 + 0.5) / size
    attn = X.integers(N, Lq, M, L, P, seed=273, lo=0, hi=4) / 16 if dt == f32 else X.integers(N, Lq, M, L, P, seed=273, lo=0, hi=2) / 4
    go = X.ternary(N, Lq, M * D, seed=274)
    X.require_random(value, go)
    out, gv, gl, ga = msda_ref64(value, levels, loc, attn, go)
    # every term is a multiple of 2^-8; magnitudes: |out| <= L P max(attn); a pixel's gradient sums over the samples that touch it
    X.require_exact(max(float(out.abs().max()), float(gv.abs().max()), float(gl.abs().max()), float(ga.abs().max())) * 64, 2.0 ** -8)
    if dt == bf:
        X.require_bf16_share(out)
        X.require_bf16_share(gv)
    shapes = torch.tensor(levels, device=d)
    lsi = torch.tensor([0] + [h * w for h, w in levels], device=d).cumsum(0)[:-1].contiguous()
    vg, lg, ag = value.to(d, dt).requires_grad_(True), loc.to(d).requires_grad_(True), attn.to(d).requires_grad_(True)
    y = ops.msda(vg, shapes, lsi, lg, ag)
    ggv, ggl, gga = torch.autograd.grad(y, (vg, lg, ag), go.to(d, dt))
    X.assert_exact(y, out, f"{dt} forward")
    X.assert_exact(ggv, gv, f"{dt} grad_value")
    X.assert_exact(gga, ga, f"{dt} grad of the attention weights")
    X.assert_exact(ggl, gl, f"{dt} grad of the sampling locations")
