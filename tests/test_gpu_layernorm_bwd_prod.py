"""du_layernorm_bwd_prod (csrc/norm_gemm.hip; -m gpu): the LayerNorm backward that takes its dy as a product G Wt^T and never writes it,
against the two kernels it replaces.

References, per shape: dy = ops.mm(G, Wt) rounded to bf16 (what the unfused path hands on), then (a) du_layernorm_bwd on that dy and (b) the
fp64 formula on the same dy, x, mean and rstd.  The bound: the new entry's error against (b) may exceed the error of (a) against (b) by at
most a factor of 2 -- the two paths differ only in the order of the fp32 K-sum before the one bf16 rounding, so isolated 1-ulp flips of dy
are the only source of difference.  (One such flip moves a dw / db column of a few dozen rows by 1e-6 .. 3e-5 of the maximum, far past
twice the 1e-7 of an fp32 sum: the bound holds because the kernel runs its K-sum in the order of the unfused data-gradient kernels --
k-steps of 16 ascending into one accumulator -- and dy comes out with the same bits.)  Error = max |got - ref| / max |ref| per tensor
(dx, dw, db).  Both errors of every shape are printed (pytest -s; the table of one run is profiles/r10_ln_bwd_prod_errors_v1.txt).  With
integer-valued G and Wt the K-sum is exact in any order, dy has the same bits on both paths, and dx must then be bit-identical: both
kernels take the row arithmetic from csrc/ln_bwd_row.h."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

D = 1024
ROWS = [1, 63, 64, 65, 200, 4 * 1029]
KS = [64, 192, 256]          # 64: the smallest K the kernel accepts; 192 and 256: the step's two


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from dinounet_amd import _lib
    assert _lib.lib().du_device_ok() == 1
    return torch.device("cuda:0")


def gen(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def make(rows, K, with_res, seed=0, integer=False):
    """x, G, Wt, w, mean, rstd, dres on the device (bf16 data, fp32 LayerNorm weight and statistics)"""
    from dinounet_amd import ops
    d = dev()
    if rows > 8192:       # the step-sized cases draw on the device: 44 M host randn per tensor would be most of the test's time
        rnd = lambda *shape, seed: torch.randn(*shape, generator=torch.Generator(device=d).manual_seed(seed), device=d)
        rint = lambda lo, hi, shape, seed: torch.randint(lo, hi, shape, generator=torch.Generator(device=d).manual_seed(seed), device=d)
    else:
        rnd = gen
        rint = lambda lo, hi, shape, seed: torch.randint(lo, hi, shape, generator=torch.Generator().manual_seed(seed))
    x = (rnd(rows, D, seed=seed + 1) * 1.5 + 0.3).to(d, torch.bfloat16)
    if integer:      # |G| <= 4, Wt with at most 8 non-zeros per row, |Wt| <= 2: every K-sum is an integer of magnitude <= 64 -- exact in fp32 in
        # any order, and exact in bf16 (which holds the integers up to 256)
        G = rint(-4, 5, (rows, K), seed + 2).float()
        Wt = torch.zeros(D, K)
        idx = torch.randint(0, K, (D, 8), generator=torch.Generator().manual_seed(seed + 3))
        Wt.scatter_(1, idx, torch.randint(-2, 3, (D, 8), generator=torch.Generator().manual_seed(seed + 4)).float())
    else:
        G = rnd(rows, K, seed=seed + 2)
        Wt = gen(D, K, seed=seed + 3) / K ** 0.5
    G, Wt = G.to(d, torch.bfloat16), Wt.to(d, torch.bfloat16)
    w = (1 + 0.1 * gen(D, seed=seed + 5)).to(d)
    b = (0.1 * gen(D, seed=seed + 6)).to(d)
    _, mean, rstd = ops.layernorm_raw(x, w, b, 1e-6, torch.bfloat16, want_stats=True)
    dres = rnd(rows, D, seed=seed + 7).to(d, torch.bfloat16) if with_res else None
    return x, G, Wt, w, mean, rstd, dres


def unfused(x, dy, w, mean, rstd, dres):
    """(a): today's du_layernorm_bwd on the materialised dy"""
    from dinounet_amd import _lib, ops
    rows = x.shape[0]
    dx = torch.empty_like(x)
    dwdb = torch.empty((2, D), dtype=torch.float32, device=x.device)
    ws, n = ops._reduce_ws(x.dtype, 1, rows, D, x.device)
    _lib.check(_lib.lib().du_layernorm_bwd(ops._code(x.dtype), _p(x), _p(dy), _p(w), _p(mean), _p(rstd), _p(dx), _p(dwdb), rows, D, _p(ws), n,
                                           _p(dres), ops._st()), "du_layernorm_bwd")
    return dx, dwdb[0], dwdb[1]


def fused(x, G, Wt, w, mean, rstd, dres):
    from dinounet_amd import _lib, ops
    rows, K = G.shape
    dx = torch.empty_like(x)
    plan = ops.layernorm_bwd_prod_plan(x, G, Wt, dx, dres)
    assert plan is not None and plan[1] == 64 and plan[2] == max(1, -(-rows // max(64, -(-rows // 256)))), plan
    dwdb = torch.empty((2, D), dtype=torch.float32, device=x.device)
    ws = torch.empty(plan[4], dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().du_layernorm_bwd_prod(ops._code(x.dtype), _p(x), _p(G), G.stride(0), _p(Wt), Wt.stride(0), K, _p(w), _p(mean), _p(rstd),
                                                _p(dx), _p(dwdb), rows, D, _p(ws), plan[4], _p(dres), ops._st()), "du_layernorm_bwd_prod")
    return dx, dwdb[0], dwdb[1]


def ref64(x, dy, w, mean, rstd, dres):
    """(b): the formula in fp64 on the same bf16 dy and the same fp32 statistics"""
    x, dy, w, mean, rstd = (t.double() for t in (x, dy, w, mean, rstd))
    xh = (x - mean[:, None]) * rstd[:, None]
    g = dy * w
    c1, c2 = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
    dx = rstd[:, None] * (g - c1 - xh * c2)
    if dres is not None:
        dx = dx + dres.double()
    return dx, (dy * xh).sum(0), dy.sum(0)


def err(a, r):
    assert torch.isfinite(a).all()
    return float((a.double() - r).abs().max() / r.abs().max().clamp_min(1e-30))


def check_against_unfused(tag, x, G, Wt, w, mean, rstd, dres):
    from dinounet_amd import ops
    dy = ops.mm(G, Wt)
    assert dy.dtype == torch.bfloat16
    old, new, ref = unfused(x, dy, w, mean, rstd, dres), fused(x, G, Wt, w, mean, rstd, dres), ref64(x, dy, w, mean, rstd, dres)
    figs = [(n, err(o, r), err(f, r)) for n, o, f, r in zip(("dx", "dw", "db"), old, new, ref)]
    print(f"ln_bwd_prod {tag}: " + "  ".join(f"{n} unfused {eo:.3e} fused {ef:.3e}" for n, eo, ef in figs))
    for n, eo, ef in figs:
        assert ef <= 2 * eo, (tag, n, eo, ef)


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("rows", ROWS)
def test_fused_vs_unfused(rows, K, with_res):
    check_against_unfused(f"rows {rows} K {K} dres {int(with_res)}", *make(rows, K, with_res))


# The launches of the train step: more than 16384 rows, so a workgroup owns more than one 64-row block (rows_per_wg = ceil(rows / 256)) and
# walks them through the same LDS, with the next block's x and statistics requested under the current block's last row pair.
#   43008 (dinounet_l at 512^2, batch 8): 256 workgroups x 168 rows = blocks of 64, 64, 40
#   20000: 254 workgroups x 79 rows = blocks of 64, 15; the last workgroup holds 13 rows
STEP_ROWS = [(43008, 192), (43008, 256), (20000, 192), (20000, 256)]


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("rows,K", STEP_ROWS)
def test_fused_vs_unfused_several_blocks_per_workgroup(rows, K, with_res):
    from dinounet_amd import ops
    x, G, Wt, w, mean, rstd, dres = make(rows, K, with_res, seed=80)
    per = ops.layernorm_bwd_prod_plan(x, G, Wt, torch.empty_like(x), dres)[3]
    assert per == -(-rows // 256) and per > 64
    check_against_unfused(f"rows {rows} K {K} dres {int(with_res)} ({per} rows per workgroup)", x, G, Wt, w, mean, rstd, dres)


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("rows,K", STEP_ROWS)
def test_exact_product_gives_identical_dx_several_blocks_per_workgroup(rows, K, with_res):
    check_exact(rows, K, with_res)


def test_ragged_rows_offset_dres_strided_g():
    """rows that are no multiple of the 64-row block, dres a view that starts one row into its buffer, G a column slice of a wider matrix"""
    rows, K = 200 + 37, 192
    x, G, Wt, w, mean, rstd, _ = make(rows, K, False, seed=20)
    big = gen(rows + 1, D, seed=27).to(x.device, torch.bfloat16)
    wide = torch.zeros(rows, K + 64, dtype=torch.bfloat16, device=x.device)
    wide[:, :K] = G
    check_against_unfused("rows 237 K 192 dres offset by one row, ldg 256", x, wide[:, :K], Wt, w, mean, rstd, big[1:])


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("rows,K", [(65, 64), (200, 192), (4 * 1029, 256)])
def test_exact_product_gives_identical_dx(rows, K, with_res):
    """integer G and Wt whose K-sums are exact and fit bf16: both paths hold the same dy bits, so dx is the same to the bit"""
    check_exact(rows, K, with_res)


def check_exact(rows, K, with_res):
    from dinounet_amd import ops
    x, G, Wt, w, mean, rstd, dres = make(rows, K, with_res, seed=40, integer=True)
    dy = ops.mm(G, Wt)
    exact = G.double() @ Wt.double().t()
    assert float(exact.abs().max()) <= 256 and torch.equal(dy.double(), exact)        # the premise: dy is exact on the unfused path
    old, new = unfused(x, dy, w, mean, rstd, dres), fused(x, G, Wt, w, mean, rstd, dres)
    assert torch.equal(old[0], new[0])
    ref = ref64(x, dy, w, mean, rstd, dres)
    for n, o, f, r in zip(("dw", "db"), old[1:], new[1:], ref[1:]):                       # the same terms summed in another order
        assert err(f, r) <= 2 * max(err(o, r), 2.0 ** -24), n


def _two_node_ffn(x, ln, fc):
    from dinounet_amd import ops
    f, fres = ops.layer_norm_res(x, ln.weight, ln.bias, ln.eps)
    return ops.linear(f, fc.weight, fc.bias), fres


def _one_node_ffn(x, ln, fc):
    from dinounet_amd import ops
    return ops.layer_norm_linear(x, ln.weight, ln.bias, ln.eps, fc.weight, fc.bias)


def _two_node_offsets(x, ln, so, aw, ref, geo):
    from dinounet_amd import ops
    q, qres = ops.layer_norm_res(x, ln.weight, ln.bias, ln.eps)
    loc, attn = ops.offsets_prep(q, so.weight, aw.weight, so.bias, aw.bias, ref, *geo)
    return loc, attn, qres


def _one_node_offsets(x, ln, so, aw, ref, geo):
    from dinounet_amd import ops
    return ops.layer_norm_offsets_prep(x, ln.weight, ln.bias, ln.eps, so.weight, aw.weight, so.bias, aw.bias, ref, *geo)


@pytest.mark.parametrize("which", ["ffn_norm+fc1", "query_norm+offsets_prep"])
def test_autograd_node_matches_the_two_nodes(which):
    """each new node against the two-node form it replaces, weights served by the per-step pack (W^T, so the node takes the product
    path): same outputs to the bit, the consumer's weight / bias gradients to the bit (same kernels on the same operands), the
    LayerNorm's dx / dw / db within the bound of this file"""
    from dinounet_amd import ops
    d = dev()
    torch.manual_seed(0)
    N, Hq, Wq, M, P = 2, 12, 11, 16, 4
    Lq = Hq * Wq                                   # 264 rows: more than one block, the last one ragged
    ln = torch.nn.LayerNorm(D, eps=1e-6).to(d)
    with torch.no_grad():
        ln.weight.add_(0.1 * torch.randn(D, device=d)); ln.bias.add_(0.1 * torch.randn(D, device=d))
    x0 = (gen(N, Lq, D, seed=61) * 1.5 + 0.3).to(d, torch.bfloat16)
    if which == "ffn_norm+fc1":
        fc = torch.nn.Linear(D, 256).to(d)
        mods, params = (ln, fc), [ln.weight, ln.bias, fc.weight, fc.bias]
        two, one = (lambda x: _two_node_ffn(x, ln, fc)), (lambda x: _one_node_ffn(x, ln, fc))
        gouts = [gen(N, Lq, 256, seed=62).to(d, torch.bfloat16), gen(N, Lq, D, seed=63).to(d, torch.bfloat16)]
        srcs = fc.weight
    else:
        so, aw = torch.nn.Linear(D, M * P * 2).to(d), torch.nn.Linear(D, M * P).to(d)
        ref = torch.rand(Lq, 2, generator=torch.Generator().manual_seed(64)).to(d)
        geo = (Lq, M, P, 24, 22)
        mods, params = (ln, so, aw), [ln.weight, ln.bias, so.weight, aw.weight, so.bias, aw.bias]
        two, one = (lambda x: _two_node_offsets(x, ln, so, aw, ref, geo)), (lambda x: _one_node_offsets(x, ln, so, aw, ref, geo))
        gouts = [gen(N * Lq, M, P, 2, seed=65).to(d), gen(N * Lq, M, P, seed=66).to(d), gen(N, Lq, D, seed=63).to(d, torch.bfloat16)]
        srcs = (so.weight, aw.weight)

    def run(form):
        x = x0.clone().requires_grad_(True)
        outs = form(x)
        grads = torch.autograd.grad(outs, [x, *params], gouts)
        torch.cuda.synchronize()
        return outs, grads

    run(two)                                        # registers the weights with the pack ...
    ops.PACK.refresh()                              # ... which now holds their bf16 cast and W^T
    wT = ops.PACK.get(srcs, ops.PK_TRANSPOSE, torch.bfloat16)
    assert wT is not None and wT.shape[0] == D
    o2, g2 = run(two)
    prof = ops.KernelProfile()
    ops.PROFILE = prof
    try:
        o1, g1 = run(one)
    finally:
        ops.PROFILE = None
    # the node itself took the product path: its launch of du_layernorm_bwd_prod is on the profile, under the consumer's K
    Kc = 256 if which == "ffn_norm+fc1" else M * P * 3
    assert [r[0] for r in prof.rec].count(f"layernorm_bwd_prod<K{Kc}>") == 1, [r[0] for r in prof.rec]
    for a, b in zip(o1, o2):
        assert torch.equal(a, b)
    for a, b in zip(g1[3:], g2[3:]):               # the consumer's parameters
        assert torch.equal(a, b)
    xc = x0.view(-1, D)
    # fp64 reference on the unfused dy
    wf = ln.weight.detach().float()
    _, mean, rstd = ops.layernorm_raw(xc, wf, ln.bias.detach().float(), 1e-6, torch.bfloat16, want_stats=True)
    if which == "ffn_norm+fc1":
        G = gouts[0].view(-1, 256)
    else:
        attn = o2[1].detach()
        G = torch.empty((xc.shape[0], M * P * 3), dtype=torch.bfloat16, device=d)
        from dinounet_amd import _lib
        _lib.check(_lib.lib().du_msda_prep_bwd(ops._code(G.dtype), _p(attn), _p(gouts[0].contiguous()), _p(gouts[1].contiguous()), _p(G),
                                               M * P * 3, xc.shape[0], M, P, 24, 22, ops._st()), "du_msda_prep_bwd")
    r = ref64(xc, ops.mm(G, wT), wf, mean, rstd, gouts[-1].view(-1, D))
    for n, a, b, rr in zip(("dx", "dw", "db"), g1[:3], g2[:3], r):
        e1, e2 = err(a.reshape(rr.shape), rr), err(b.reshape(rr.shape), rr)
        print(f"ln_bwd_prod node {which}: {n} two nodes {e2:.3e} one node {e1:.3e}")
        assert e1 <= 2 * e2, (which, n, e2, e1)
