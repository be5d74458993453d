"""Keeps the exact-input instrument honest without a GPU: the helpers of tests/_exact.py against emulated kernels in plain torch.  An honest
kernel (blocked fp32 accumulation in any order, split-K slabs, plain-cast stores) must pass the exact gate and the per-element bounds; every
mutant below -- each a bug a tile kernel can have and the old `rel < 3e-2` gate let through -- must fail them.  Also asserts the stated
conditions (2^24 bound, >= 95 % of a bf16 reference exactly representable) for every shape list tests/test_gpu_exact.py uses, so a later
edit of a shape list cannot silently void the exactness."""
import math

import pytest
import torch

import _exact as X
import test_gpu_exact as G

bf, f32 = torch.bfloat16, torch.float32


def case(M=261, N=72, K=4096, fine_bias=False, seed=0):
    a, b = X.ternary(M, K, seed=seed + 1), X.ternary(N, K, seed=seed + 2)
    bias = X.integers(N, seed=seed + 3, lo=-1024, hi=1024) / 256 if fine_bias else X.integers(N, seed=seed + 3, lo=-4, hi=4)
    X.require_random(a, b, bias)
    X.require_exact(X.sum_bound(a, b) + 4, 1.0 / 256 if fine_bias else 1.0)
    return a, b, bias, a.double() @ b.double().t() + bias.double()


def kernel(a, b, bias, od, mutant=None, bk=64):
    """emulated tile kernel: fp32 accumulation over K blocks in a scrambled order, fp32 epilogue, plain cast"""
    K = a.shape[1]
    nb = (K + bk - 1) // bk
    order = torch.randperm(nb, generator=torch.Generator().manual_seed(7)).tolist()
    if mutant == "drop_last_k":
        a = a.clone()
        a[:, -1] = 0
    if mutant == "last_row_misses_8k":
        a = a.clone()
        a[-1, -8:] = 0
    acc = X.blocked_mm(a, b, bk, order)
    if mutant == "slice_twice":                      # a slab reduce that adds one K slice twice
        acc += a[:, :bk].float() @ b[:, :bk].float().t()
    bias = bias.float()
    if mutant == "bias_shifted":
        bias = torch.roll(bias, 1)
    if mutant == "bias_bf16":
        bias = bias.to(bf).float()
    out = acc + bias
    if mutant == "dup_last_col":
        out[:, -1] = out[:, -2]
    whole, view = X.guarded(a.shape[0], b.shape[0], od, "cpu")
    view.copy_(out.to(od))
    if mutant == "row_unwritten":
        view[a.shape[0] // 2] = X.SENTINEL
    if mutant == "write_past_end":
        whole[a.shape[0]] = 0
    return whole, view


def passes(whole, view, ref):
    try:
        X.assert_guard(whole, view.shape[0])
        X.assert_exact(view, ref)
    except AssertionError:
        return False
    return True


@pytest.mark.parametrize("od", [f32, bf])
@pytest.mark.parametrize("K", [1024, 4096])
def test_honest_emulation_passes_the_exact_gate(od, K):
    a, b, bias, ref = case(K=K, fine_bias=od == f32)
    if od == bf:
        X.require_bf16_share(ref)
    for bk in (32, 64, 256):
        assert passes(*kernel(a, b, bias, od, bk=bk), ref), bk
    # any order: whole-K rows summed one element at a time from the far end
    acc = torch.zeros(a.shape[0], b.shape[0])
    for k in range(K - 1, K - 65, -1):
        acc += a[:, k:k + 1] @ b[:, k:k + 1].t()
    acc += X.blocked_mm(a[:, :K - 64], b[:, :K - 64], 128)
    assert X.is_exact((acc + bias).to(od), ref)


@pytest.mark.parametrize("od", [f32, bf])
@pytest.mark.parametrize("mutant", ["drop_last_k", "last_row_misses_8k", "dup_last_col", "bias_shifted", "slice_twice", "row_unwritten", "write_past_end"])
def test_mutants_fail_the_exact_gate(od, mutant):
    """K = 4096: the shape at which `rel < 3e-2` passed a K loop that stops one element or one 8-wide fragment short"""
    a, b, bias, ref = case(K=4096, fine_bias=od == f32)
    assert not passes(*kernel(a, b, bias, od, mutant=mutant), ref), mutant


def test_bias_rounded_to_bf16_fails_on_fp32_results():
    """an integer bias in [-4, 4] is a bf16 number, so the fp32-result cases draw it in 1/256 steps (11 significant bits)"""
    a, b, bias, ref = case(K=1024, fine_bias=True)
    assert not torch.equal(bias.to(bf).float(), bias)
    assert passes(*kernel(a, b, bias, f32), ref)
    assert not passes(*kernel(a, b, bias, f32, mutant="bias_bf16"), ref)


def test_mismatch_report_names_rows_columns_and_difference():
    a, b, bias, ref = case(K=512)
    _, out = kernel(a, b, bias, f32, mutant="last_row_misses_8k")
    msg = X.mismatch_report(out, X.expected(ref, f32))
    assert "rows 260..260" in msg and "distinct differences" in msg
    with pytest.raises(AssertionError, match="not bit-equal"):
        X.assert_exact(out, ref, "mutant")


def test_check_rows_covers_blocks_ragged_rows_and_a_stride():
    assert X.check_rows(32999) is None
    for M in (33000, 43008, 70000, 131072):
        r = X.check_rows(M)
        s = set(r.tolist())
        full = M // 256
        assert set(range(256)) <= s and set(range((full - 1) * 256, M)) <= s and set(range(0, M, 97)) <= s
        assert set(range((full // 2) * 256, (full // 2) * 256 + 256)) <= s
        assert len(s) < M // 20 + 1100 and r.tolist() == sorted(s)


# ---------------------------------------------------------------------------------------------------- per-element bounds
def gelu_case(K=1024, od=bf):
    a, b = X.ternary(300, K, seed=5), X.ternary(256, K, seed=6) / 32
    bias = X.integers(256, seed=7, lo=-16, hi=16) / 32
    X.require_exact(X.sum_bound(a, b) + 0.5, 1.0 / 32)
    s = a.double() @ b.double().t() + bias.double()
    s32 = X.blocked_mm(a, b, 64) + bias
    assert torch.equal(s32.double(), s)
    return s, s32


@pytest.mark.parametrize("od", [f32, bf])
def test_gelu_bound_accepts_erf_and_rejects_tanh(od):
    s, s32 = gelu_case()
    ref = X.gelu64(s)
    honest = torch.nn.functional.gelu(s32).to(od)                    # fp32 erf-GELU, one rounding to the result format
    X.assert_act(honest, ref, s, X.E_ACT_GELU, "erf")
    tanh = torch.nn.functional.gelu(s32, approximate="tanh").to(od)
    u = X.U_BF16 if od == bf else X.U_F32
    share = float((X.act_excess(tanh, ref, s, u, X.E_ACT_GELU) > 0).double().mean())
    assert share > 0.001, share                                    # not one stray element; the old gate saw nothing here (rel 2.2e-3 for both)
    with pytest.raises(AssertionError):
        X.assert_act(tanh, ref, s, X.E_ACT_GELU, "tanh")
    assert X.E_ACT_GELU <= X.E_ACT_CAP and X.E_ACT_SWIGLU <= X.E_ACT_CAP


def test_swiglu_bound_accepts_the_honest_gate():
    g, _ = gelu_case(K=640)
    v, _ = gelu_case(K=896)
    v = v.flip(0)
    ref = X.swiglu64(g, v)
    honest = (torch.nn.functional.silu(g.float()) * v.float()).to(bf)
    X.assert_act(honest, ref, g * v, X.E_ACT_SWIGLU, "swiglu")
    broken = (torch.nn.functional.silu(g.float()) * v.float().roll(1, 1)).to(bf)          # the gate paired with the wrong value column
    with pytest.raises(AssertionError):
        X.assert_act(broken, ref, g * v, X.E_ACT_SWIGLU, "swiglu")


@pytest.mark.parametrize("N,Dh", [(1029, 64), (300, 128)])
def test_attention_bound_accepts_flash_emulation_and_rejects_lost_keys(N, Dh):
    g = torch.Generator().manual_seed(N + Dh)
    q = (torch.randn(N, Dh, generator=g) * Dh ** -0.5 * math.log2(math.e)).to(bf)
    k, v = torch.randn(N, Dh, generator=g).to(bf), torch.randn(N, Dh, generator=g).to(bf)
    ref, bound = X.attention_ref64(q, k, v, N)
    err = lambda o: ((o.double() - ref).abs() / bound).max().item()
    honest = err(X.flash_attention_emulated(q, k, v, N))
    assert honest < 0.5, honest                  # an honest kernel uses a fraction of the bound
    assert err(X.flash_attention_emulated(q, k, v, N, drop_last_key=True)) > 1
    assert err(X.flash_attention_emulated(q, k, v, N, drop_last_tile=True)) > 1


# ---------------------------------------------------------------------------------------------------- the GPU file's shape lists keep the conditions
@pytest.mark.parametrize("M,N,K,f32out,epi", G.NT_SHAPES)
def test_conditions_hold_for_the_nt_shapes(M, N, K, f32out, epi):
    """nt_case asserts the 2^24 bound on the whole operands and the representable share on the reference rows it is given: here a sample of
    ~128 rows (the share is a statistic of the draw, the same for every row)"""
    rows = torch.arange(0, M, max(1, M // 128))
    G.nt_case(M, N, K, f32out, epi, rows=rows)


def sample(M, n=128):
    return torch.arange(0, M, max(1, M // n))


@pytest.mark.parametrize("M,N,K", G.ROUTE1_SHAPES)
def test_conditions_hold_for_the_route_1_shapes(M, N, K):
    G.nt_case(M, N, K, False, "bias", rows=sample(M))
    G.nt_case(M, N, K, True, "ls_res", rows=sample(M))


def test_conditions_hold_for_the_other_gemm_shape_lists():
    """the draws of the GPU tests (same seeds, same densities), the 2^24 bound on the whole operands, the bf16 share on a row sample"""
    for (M, N, K) in G.GELU_SHAPES:                                   # per-element bound: exact pre-activation only
        x, w = X.ternary(M, K, seed=251), X.ternary(N, K, seed=252) / 32
        X.require_exact(X.sum_bound(x, w) + 0.5, 1.0 / 32)
    for (M, N, K, form) in G.RK_SHAPES:
        x, w = X.ternary(M, K, seed=21), X.ternary(N, K, seed=22)
        X.require_exact(X.sum_bound(x, w) + 4)
        X.require_bf16_share(x[sample(M)].double() @ w.double().t() + 4)
    for (M, N, K) in G.PLAIN_SHAPES:
        x, w, b = X.ternary(M, K, seed=31), X.ternary(N, K, seed=32), X.integers(N, seed=33, lo=-4, hi=4)
        X.require_exact((X.sum_bound(x, w) + 4) * 2 + 256, 0.5)
        X.require_bf16_share(x[sample(M)].double() @ w.double().t() + b.double())
    for i, (rows, N, K) in enumerate(G.WGRAD_SHAPES):                 # fp32 results: the bound is the column sum of |dy|
        X.require_exact(float(X.ternary(rows, N, seed=61).abs().sum(0).max()))
    for i, (rows, N, K, cs) in enumerate(G.TN_GROUP_SHAPES):
        X.require_exact(float(X.ternary(rows, N, seed=70 + i).abs().sum(0).max()))
    for (B, H, N, D) in G.QKV_SHAPES:                                 # the first sample's tokens stand for all
        h, w = X.ternary(B * N, D, seed=41), X.ternary(3 * H * 64, D, seed=42)
        bias = X.integers(3 * H * 64, seed=43, lo=-4, hi=4)
        sin, cos = G.rope_tables(N, 5, 64, seed=44)
        X.require_exact(2 * (X.sum_bound(h, w) + 4), 0.125)
        proj, want = G.qkv_reference(h[:N], w, bias, sin, cos, 1, N, H, 64, 5, 0.125)
        X.require_bf16_share(proj)
        X.require_bf16_share(want)


def test_conditions_hold_for_the_convolution_shape_lists():
    """the bound with the real pixel counts; the shares on the first image (cropped to 64 rows where it is larger) of the GPU tests' draws"""
    import torch.nn.functional as F
    for c in G.CONV3_CFGS:
        B, H, W, Cin, Cout, s_ = (c[k] for k in ("B", "H", "W", "Cin", "Cout", "s"))
        x, w = X.ternary(B, Cin, H, W, seed=111)[:1], X.ternary(Cout, Cin, 3, 3, seed=112)
        X.require_exact(max(9 * Cin + 4, 9 * Cout, B * H * W))
        xr = x.double().requires_grad_(True)
        yr = F.conv2d(xr, w.double(), None, s_, 1)
        go = X.ternary(B, *yr.shape[1:], seed=114)[:1]
        X.require_bf16_share(yr.detach())
        X.require_bf16_share(torch.autograd.grad(yr, xr, go.double())[0])
    for (B, H, W, C1, C2, Cout) in G.HALO_SHAPES:
        x = X.ternary(B, H, W, C1, seed=131, density=G.HALO_DENSITY)[:1]
        if C2:
            x = torch.cat([x, X.ternary(B, H, W, C2, seed=132, density=G.HALO_DENSITY)[:1]], -1)
        w, bias = X.ternary(Cout, C1 + C2, 3, 3, seed=133, density=G.HALO_DENSITY), X.integers(Cout, seed=134, lo=-2, hi=2)
        go = X.ternary(B, H, W, Cout, seed=135)[:1]
        X.require_exact(max(9 * (C1 + C2) + 2, 9 * Cout, B * H * W))
        y = X.conv3x3_ref64(x, w, bias)                                  # the whole first image: its second moment is the condition
        X.require_bf16_share(y, least=1.0)
        X.require_exact(float(max(y.abs().sum((1, 2)).max(), (y * y).sum((1, 2)).max())))
        X.require_bf16_share(X.conv3x3_ref64(x[:, :64], w, bias, go[:, :64])[1])
    for (B, H, W, C1, C2, Cout) in G.ROWS_SHAPES:                      # fp32 results of ternary operands: |sum| <= pixels
        X.require_exact(B * H * W)
    for (B, H, W, C1, C2, Cout, bias) in G.GROUPED3_SHAPES:
        X.require_exact(B * H * W)
    for name, shapes in G.CONVT_SHAPES.items():
        for (B, H, W, Cin, Cout) in shapes:
            X.require_exact(max(Cin + 4 + 32, 4 * Cout, 4.0 * B * H * W))
            x, w, b, res, go, yr, gr = G.convt_case(1, min(H, 16), min(W, 16), Cin, Cout, seed=171, residual=name == "persistent")
            X.require_bf16_share(yr)
            X.require_bf16_share(gr[0])


def test_conv3x3_ref64_is_conv2d():
    import torch.nn.functional as F
    x, w, b, go = X.ternary(2, 7, 9, 8, seed=1), X.ternary(5, 8, 3, 3, seed=2), X.integers(5, seed=3, lo=-2, hi=2), X.ternary(2, 7, 9, 5, seed=4)
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    yr = F.conv2d(xr.permute(0, 3, 1, 2), wr, br, 1, 1).permute(0, 2, 3, 1)
    gr = torch.autograd.grad(yr, (xr, wr, br), go.double())
    y, gx, gw, gb = X.conv3x3_ref64(x, w, b, go)
    assert torch.equal(y, yr.detach()) and torch.equal(gx, gr[0]) and torch.equal(gw, gr[1]) and torch.equal(gb, gr[2])


def test_the_longest_contraction_keeps_its_share():
    """K = 43008: the share the ternary draw was chosen for"""
    x, w = X.ternary(64, 43008, seed=1), X.ternary(64, 43008, seed=2)
    ref = x.double() @ w.double().t()
    assert float(ref.abs().max()) < 1000 and X.bf16_share(ref) >= 0.95
