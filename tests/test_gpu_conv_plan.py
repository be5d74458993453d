"""The 3 x 3 convolution plans on the device (-m gpu): what du_conv3x3_plan_describe / du_conv3x3_wgrad_plan_describe say a call writes is what
du_conv3x3_halo / du_conv3x3_wgrad_halo write -- rows of partial statistics, partial dW slabs -- and the kernel ops.KernelProfile is told."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from test_gpu_ops import dev, gen, q, rel

pytestmark = pytest.mark.gpu

STRIP, HALO, ROWS, ROUND3 = 1, 2, 1, 2
NAMES = {STRIP: "conv3x3_strip_kernel<bf16>", HALO: "conv3x3_halo_kernel<bf16>"}
WNAMES = {ROWS: "conv3x3_wgrad_rows_kernel<bf16>", ROUND3: "conv3x3_wgrad_halo_kernel<bf16>"}


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# the smallest call of each planned form: (C1, C2, Cout, B, H, W, width of the tensor x is a slice of, planned [kernel, variant])
@pytest.mark.parametrize("C1,C2,Cout,B,H,W,wide,want", [
    (32, 0, 32, 1, 8, 128, 0, [STRIP, 11]), (32, 0, 64, 1, 8, 128, 0, [STRIP, 12]), (64, 0, 32, 1, 8, 128, 0, [STRIP, 21]),
    (32, 32, 64, 1, 8, 128, 0, [STRIP, 22]), (32, 0, 32, 1, 8, 16, 0, [HALO, 321]), (64, 0, 64, 1, 8, 16, 0, [HALO, 642]),
    # 128 outputs run on <32, 4>: from two input chunks up.  With ONE chunk (32 -> 128) the weights stay resident beside the halo and the
    # fp32 tile, 175 KB of LDS: the plan declines, as the launcher did -- the call must then write nothing at all
    (64, 0, 128, 1, 8, 16, 0, [HALO, 324]), (32, 0, 128, 1, 8, 16, 0, None),
    (64, 64, 64, 2, 8, 16, 0, [HALO, 642]), (32, 0, 32, 1, 8, 128, 96, [STRIP, 11])])
def test_conv3x3_plan_statistics_rows_are_the_rows_written(C1, C2, Cout, B, H, W, wide, want):
    from dinounet_amd import _lib, ops
    d, dt, L = dev(), torch.bfloat16, _lib.lib()
    Cin = C1 + C2
    x = q(gen(B, H, W, wide or C1, seed=61), dt).to(d, dt)[..., (32 if wide else 0):(32 if wide else 0) + C1]
    x2 = q(gen(B, H, W, C2, seed=62), dt).to(d, dt) if C2 else None
    w, bias = gen(Cout, Cin, 3, 3, seed=63, scale=0.1), gen(Cout, seed=64, scale=0.1).to(d)
    wp = ops.pack_conv_weight(w.to(d), dt)
    y = torch.full((B, H, W, Cout), float("nan"), dtype=dt, device=d)
    shape = (_ptr(x), x.stride(2), _ptr(x2), C2, C1, Cin, Cout, B, H, W)
    plan = (C.c_int64 * 4)()
    assert L.du_conv3x3_plan_describe(*shape, _ptr(wp), _ptr(y), Cout, 1, plan, 4) == 4
    rc, kernel, variant, parts = plan
    part = torch.full((parts + 4, Cout, 2), float("nan"), dtype=torch.float32, device=d)
    got = L.du_conv3x3_halo(*shape, _ptr(wp), _ptr(bias), _ptr(y), Cout, _ptr(part), _stream())
    if want is None:
        assert rc == -2 and list(plan)[1:] == [0, 0, 0] and got == -2
        assert bool(torch.isnan(y).all()) and bool(torch.isnan(part).all())
        assert ops.conv3x3_halo(x, wp, bias, x2, want_stats=True) is None
        return
    assert [rc, kernel, variant] == [0] + want and got == 0, (list(plan), got)
    assert parts == (B * (H // 8) * (W // 32) if kernel == STRIP else B * (H // 8) * (W // 16))
    xin = torch.cat([x, x2], -1) if C2 else x
    yr = F.conv2d(xin.float().cpu().permute(0, 3, 1, 2), q(w, dt), bias.cpu(), 1, 1).permute(0, 2, 3, 1)
    assert rel(y, yr) < 3e-2
    # the first stats_parts rows are written and finalize to the statistics of y; the guard rows behind them are untouched
    assert bool(torch.isfinite(part[:parts]).all()) and bool(torch.isnan(part[parts:]).all())
    sums_ref, _ = ops.chan_stats(y, B)
    sums = torch.empty_like(sums_ref)
    _lib.check(L.du_strip_finalize(_ptr(part), _ptr(sums), B, parts // B, Cout, _stream()), "du_strip_finalize")
    print(f"statistics rel {rel(sums, sums_ref):.3e}")
    assert rel(sums, sums_ref) < 1e-4
    # ops asks the same plan: same output bits, a statistics buffer of exactly the planned rows, the planned kernel's name in the profile
    prof, ops.PROFILE = ops.PROFILE, ops.KernelProfile()
    try:
        y2, part2 = ops.conv3x3_halo(x, wp, bias, x2, want_stats=True)
        names = [r[0] for r in ops.PROFILE.rec]
    finally:
        ops.PROFILE = prof
    assert torch.equal(y2, y) and part2.shape == (parts, Cout, 2) and torch.equal(part2, part[:parts])
    assert names == ["conv3x3_halo_c128_kernel<bf16>" if Cout == 128 else NAMES[kernel]], names


# option 13: 0 = the round-3 kernel, 1 = the rows kernel for 32 / 64 outputs, 2 = for 128 too.  (C1, C2, Cout) -> planned [kernel, variant] per option
@pytest.mark.parametrize("C1,C2,Cout,want", [
    (32, 0, 32, {0: [ROUND3, 321], 1: [ROWS, 321], 2: [ROWS, 321]}), (64, 0, 32, {0: [ROUND3, 641], 1: [ROWS, 641], 2: [ROWS, 641]}),
    (64, 0, 64, {0: [ROUND3, 322], 1: [ROWS, 642], 2: [ROWS, 642]}), (32, 32, 64, {0: [ROUND3, 322], 1: [ROWS, 322], 2: [ROWS, 322]}),
    (64, 0, 128, {0: None, 1: None, 2: [ROWS, 324]})])
def test_conv3x3_wgrad_plan_slabs_are_the_slabs_written(C1, C2, Cout, want):
    from dinounet_amd import _lib, ops
    d, dt, L = dev(), torch.bfloat16, _lib.lib()
    B, H, W = 2, 8, 32
    Cin = C1 + C2
    x, go = q(gen(B, H, W, C1, seed=71), dt), q(gen(B, H, W, Cout, seed=73), dt)
    x2 = q(gen(B, H, W, C2, seed=72), dt) if C2 else None
    xin = (torch.cat([x, x2], -1) if C2 else x).permute(0, 3, 1, 2)
    wr = torch.zeros(Cout, Cin, 3, 3, requires_grad=True)
    (F.conv2d(xin, wr, None, 1, 1) * go.permute(0, 3, 1, 2)).sum().backward()
    ref = torch.cat([wr.grad.permute(0, 2, 3, 1).reshape(-1), go.sum((0, 1, 2))])          # dw in (tap, ci) column order, db behind it
    xd, gd, x2d = x.to(d, dt), go.to(d, dt), (x2.to(d, dt) if C2 else None)
    nel = Cout * 9 * Cin + Cout
    shape = (_ptr(xd), C1, _ptr(x2d), C2, C1, Cin, Cout, B, H, W, _ptr(gd), Cout)
    plan = (C.c_int64 * 4)()
    try:
        for opt in (0, 1, 2):
            L.du_set_option(13, opt)
            assert L.du_conv3x3_wgrad_plan_describe(*shape, plan, 4) == 4
            rc, kernel, variant, blocks = plan
            part = torch.full((blocks + 1, nel), float("nan"), dtype=torch.float32, device=d)
            out = torch.full((nel,), float("nan"), dtype=torch.float32, device=d)
            got = L.du_conv3x3_wgrad_halo(*shape, _ptr(part), _ptr(out), 1, _stream())
            if want[opt] is None:
                assert list(plan) == [-2, 0, 0, 0] and got == -2 and bool(torch.isnan(part).all()) and bool(torch.isnan(out).all())
                assert ops.conv3x3_wgrad_halo(xd, gd, x2d, with_db=True) is None
                continue
            assert [rc, kernel, variant, blocks] == [0] + want[opt] + [B * (H // 8) * (W // 16)] and got == 0, (opt, list(plan), got)
            # the planned slabs are written, the guard slab is not; their sum is the gradient (fp32 accumulation of exact bf16 products: 2e-5, bias
            # gradient 1e-5, the bounds of test_conv3x3_weight_gradient_rows_kernel)
            assert bool(torch.isfinite(part[:blocks]).all()) and bool(torch.isnan(part[blocks:]).all())
            nw = Cout * 9 * Cin
            err, err_db = (float((out.cpu()[s_] - ref[s_]).abs().max()) / float(ref[s_].abs().max()) for s_ in (slice(0, nw), slice(nw, nel)))
            print(f"option 13 = {opt}: weight gradient rel {err:.3e}, bias gradient rel {err_db:.3e}")
            assert err < 2e-5 and err_db < 1e-5, opt
            prof, ops.PROFILE = ops.PROFILE, ops.KernelProfile()
            try:
                dw, db = ops.conv3x3_wgrad_halo(xd, gd, x2d, with_db=True)
                names = [r[0] for r in ops.PROFILE.rec]
            finally:
                ops.PROFILE = prof
            assert torch.equal(torch.cat([dw.reshape(-1), db]), out) and names == [WNAMES[kernel]], (opt, names)
    finally:
        L.du_set_option(13, 1)
