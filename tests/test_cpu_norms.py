"""Keeps the instruments of tests/_norm_ref.py honest without a GPU.  The fp64 restatements agree with torch's fp64 layer_norm,
instance_norm and batch_norm and their autograd (running statistics included); every exactness condition, the |z| >= 0.25 condition
and every regime predicate hold for every entry of the GPU shape lists; an honest fp32 emulation of the kernels (blocked sums in
scrambled strip order, the one-pass variance, fp32 elementwise arithmetic) passes every gate; and each of twelve deliberately broken
emulations is rejected by the gate meant for it."""
import pytest
import torch
import torch.nn.functional as F

import _exact as X
import _norm_ref as R

bf, f32 = R.bf, R.f32


def exact(out, ref64):
    try:
        X.assert_exact(out, ref64)
    except AssertionError:
        return False
    return True


def inside(out, ref64, bound):
    return R.within(out, ref64, bound)[0]


def share(out, ref64, bound):
    return float(((out.double() - ref64).abs() / torch.as_tensor(bound, dtype=torch.float64).expand_as(ref64).clamp_min(1e-300)).max())


# ---------------------------------------------------------------------------------------------------- references against torch
@pytest.mark.parametrize("rows,D", [(5, 8), (9, 260), (3, 1028)])
def test_layernorm_restatements_agree_with_torch(rows, D):
    x, m, a, w, b = R.ln_draw(rows, D, seed=D)
    xr, wr, br = (t.double().clone().requires_grad_(True) for t in (x, w, b))
    yt = F.layer_norm(xr, (D,), wr, br, R.EPS_LN)
    y, mean, rstd = R.ln_fwd64(x, w, b, R.EPS_LN)
    assert torch.equal(mean, m.double()) and float((rstd - 1 / torch.sqrt(a.double() ** 2 + R.EPS_LN)).abs().max()) < 1e-15
    assert float((y - yt.detach()).abs().max()) < 1e-13
    dy, dres = X.integers(rows, D, seed=1, lo=-4, hi=4), X.integers(rows, D, seed=2, lo=-4, hi=4)
    gx, gw, gb = torch.autograd.grad(yt, (xr, wr, br), dy.double())
    dx, dwdb, _ = R.ln_bwd64(x, dy, w, mean, rstd, dres)
    assert float((dx - (gx + dres.double())).abs().max()) < 1e-11
    assert float((dwdb[0] - gw).abs().max()) < 1e-10 and float((dwdb[1] - gb).abs().max()) < 1e-12


@pytest.mark.parametrize("mode", R.NORM_ACT_MODES)
@pytest.mark.parametrize("actname", list(R.ACTS))
def test_norm_act_restatements_agree_with_torch(actname, mode):
    """norm_formulas64 (the kernels' formulas, which the bounds are written over) against F.instance_norm / F.batch_norm + activation
    and autograd, the running statistics of stats_finalize64 against batch_norm's update.  One group of an InstanceNorm included: there a
    (1, C, P, 1) view of the (1, P, C) data has ambiguous strides, and torch's backward read it in the wrong order until
    torch_norm_act64 made its operands contiguous"""
    act = R.ACTS[actname]
    for G, Pn, Cc in ([(3, 10, 8), (1, 130, 12)] if mode == "in" else [(1, 30, 8)]):
        restatement_case(act, mode, G, Pn, Cc)


def restatement_case(act, mode, G, Pn, Cc):
    x, m, s = R.two_value_draw(G, Pn, Cc, seed=5)
    w, b = R.affine_for(Cc, seed=2)
    dy = X.integers(G, Pn, Cc, seed=3, lo=-4, hi=4)
    rm0, rv0 = X.integers(Cc, seed=4, lo=-3, hi=3), X.integers(Cc, seed=5, lo=1, hi=3)
    if mode == "bn-eval":
        b = R.bias_for_eval(m[0], rm0, rv0, w, R.EPS_N)
        f = R.norm_formulas64(x, dy, w, b, act, R.EPS_N, mean=rm0.double()[None], var=rv0.double()[None], use_batch=False)
    else:
        f = R.norm_formulas64(x, dy, w, b, act, R.EPS_N)
        assert torch.equal(f["mean"], m.double()) and torch.equal(f["var"], s.double() ** 2)
    kind = "in" if mode == "in" else "bn"
    y, dx, dw, db, rm, rv = R.torch_norm_act64(x, dy, w, b, kind, act, R.EPS_N, mode != "bn-eval", None if kind == "in" else rm0, None if kind == "in" else rv0)
    assert float(f["z"].abs().min()) >= 0.25
    for a_, b_ in ((f["y"], y), (f["dx"], dx), (f["dw"], dw), (f["db"], db)):
        assert float((a_ - b_).abs().max()) < 1e-11
    if mode == "bn-train":
        st = R.stats_finalize64(R.stats64(x), float(Pn), R.EPS_N, rm0, rv0, 0.1)
        assert float((st[4] - rm).abs().max()) < 1e-14 and float((st[5] - rv).abs().max()) < 1e-13
        biased = R.stats_finalize64(R.stats64(x), float(Pn), R.EPS_N, rm0, rv0, 0.1, biased=True)
        assert float((biased[5] - rv).abs().max()) > 1e-3
    elif mode == "bn-eval":
        assert torch.equal(rm, rm0.double()) and torch.equal(rv, rv0.double())


# ---------------------------------------------------------------------------------------------------- conditions and regimes of the GPU lists
def test_channel_reduction_lists_reach_their_regimes_and_stay_exact():
    seen = set()
    for dt, Cc, name in R.CHAN_CASES:
        assert Cc % R.VEC[dt] == 0 and R.chan_regime_ok(dt, Cc, name), (dt, Cc, name)
        for G, Pn, what in R.chan_gp(dt, Cc):
            assert R.gp_regime_ok(dt, Cc, G, Pn, what), (dt, Cc, G, Pn, what)
            R.require_sums_exact(Pn, 16.0)
            X.require_exact(G * Pn * 48.0, 0.5)
            assert G * Pn * Cc * 8 <= 16 << 20                       # fp64 bytes of the largest tensor
            seen.add(what)
    assert seen == {"P=1", "P<np", "short-strip", "strip+1", "multi", "per_group=1"}
    assert R.lanes(4, f32) == (1, 256) and R.pick_strip(1, 129, 32, f32) == 128 and R.strips(1, 129, 32, f32) == 2       # the issue's example
    assert R.passes(1028, f32) == 2 and 1028 // 4 - 256 == 1                                                             # one valid vector
    for dt in R.DTS:
        Cc, Un = R.UNROLL[dt]
        assert R.lanes(Cc, dt)[1] == 4
        assert {min(Pn, 16) % (Un * 4) for Pn in range(1, 2 * Un * 4)} == set(range(Un * 4))
    x, dy, mean, rstd, w, b = R.bwd_exact_inputs(3, 50, 16, seed=1)
    for act in (R.ACT_NONE, R.ACT_RELU):
        xh, z, dz = R.norm_terms64(x, dy, mean, rstd, w, b, act)
        assert float(z.abs().min()) >= 0.125 and float(((z * 8) % 2 - 1).abs().max()) == 0              # odd multiples of 1/8
        assert float(xh.abs().max()) <= 12 and float((dz * xh).abs().max()) <= 48 and float(((dz * xh * 2) % 1).abs().max()) == 0


def test_finalize_lists_sit_on_both_sides_of_the_switches():
    for cols, G, Cc, n in R.FIN_CASES:
        assert R.finalize_cols(G * Cc * 2, 4096) == cols
        X.require_exact(n * 12.0)
    assert {c[3] for c in R.FIN_CASES if c[0] == 4} >= set(R.FIN_STRIPS[4]) and {c[3] for c in R.FIN_CASES if c[0] == 32} >= set(R.FIN_STRIPS[32])
    assert (4, 1, 2047, 3) in R.FIN_CASES and (32, 1, 2048, 9) in R.FIN_CASES                         # G C 2 = 4094 and 4096
    assert any(c[1] > 1 for c in R.FIN_CASES if c[0] == 4) and any(c[1] > 1 for c in R.FIN_CASES if c[0] == 32)
    for dt, G, Pn, Cc, cols, least in R.GRADS_CASES:
        assert R.finalize_cols(Cc * 2, 512) == cols and R.strips(G, Pn, Cc, dt) >= least and Cc % R.VEC[dt] == 0
    assert {c[3] for c in R.GRADS_CASES} >= {248, 252, 256} and any(c[5] > 2 * 64 for c in R.GRADS_CASES) and any(c[1] > 1 for c in R.GRADS_CASES)


def test_layernorm_lists_reach_their_regimes():
    for dt in R.DTS:
        assert {R.ln_maxv(D, dt) for D in R.LN_D[dt]} == {1, 2, 4, 5, 8, 16}
        assert any((D // R.VEC[dt]) % 64 for D in R.LN_D[dt])                                          # a partly filled last vector round
        assert R.ln_route(R.LN_D_REFUSED[dt], dt) == "unsupported" and R.ln_maxv(R.LN_D_REFUSED[dt], dt) == 17
        assert [D for D in R.LN_D[dt] if R.ln_route(D, dt) == "pair"][0] == R.LN_FIRST_PAIR[dt]
        D = R.LN_BWD_D[dt]
        assert R.ln_route(D, dt) == "fused" and all(R.pick_strip(1, r, D, dt) == min(r, 16) for r in R.LN_BWD_ROWS)
        rows, D = R.LN_TWO_TRIPS[dt]
        assert R.ln_route(D, dt) == "fused" and R.pick_strip(1, rows, D, dt) >= 9 and R.ln_rows_per_wave(rows, D, dt) >= 3
        for D in R.LN_D[dt]:
            X.require_exact(37 * 48.0, 0.25)
            X.require_exact(D * 96.0, 0.25)
            R.require_sums_exact(D, 49.0)
    assert 24 * 2048 == 48 * 1024 and R.ln_route(2048, bf) == "fused"


def test_elementwise_lists_run_the_loops_they_name():
    assert R.elementwise_loops(1, 4 * 512 + 2 * 512 + 1, 1024, f32, True) == ({4, 2, 1}, True)
    assert R.elementwise_loops(64, 32 * 6 + 1, 512, bf, True) == ({4, 2, 1}, True)
    assert R.elementwise_loops(64, 4 * 64 + 1, 1024, f32) == ({4, 1}, True)
    for dt in R.DTS:
        for G, Pn in ((1, 3), (3, 192)):
            assert R.elementwise_loops(G, Pn, 4 * R.VEC[dt], dt) == ({1}, False) and 4 not in R.elementwise_loops(G, Pn, 4 * R.VEC[dt], dt, True)[0]


@pytest.mark.parametrize("mode", R.NORM_ACT_MODES)
def test_no_element_of_the_norm_act_lists_sits_at_the_kink(mode):
    for dt, G, Pn, Cc in R.NORM_ACT_SHAPES:
        Gn, Pg = (G, Pn) if mode == "in" else (1, G * Pn)
        assert Pg % 2 == 0 and Cc % R.VEC[dt] == 0
        x, m, s = R.two_value_draw(Gn, Pg, Cc, seed=Pn + Cc)
        assert torch.equal(R.quant(x, dt), x)
        R.require_sums_exact(Pg, 49.0)
        w, b = R.affine_for(Cc, seed=Cc)
        rm0, rv0 = X.integers(Cc, seed=4, lo=-3, hi=3), X.integers(Cc, seed=5, lo=1, hi=3)
        if mode == "bn-eval":
            b = R.bias_for_eval(m[0], rm0, rv0, w, R.EPS_N)
            f = R.norm_formulas64(x, x, w, b, R.ACT_NONE, R.EPS_N, mean=rm0.double()[None], var=rv0.double()[None], use_batch=False)
        else:
            f = R.norm_formulas64(x, x, w, b, R.ACT_NONE, R.EPS_N)
            assert torch.equal(f["mean"], m.double()) and torch.equal(f["var"], s.double() ** 2)
        assert float(f["z"].abs().min()) >= 0.25, (mode, dt, G, Pn, Cc)
        assert bool((f["z"] > 0).any()) and bool((f["z"] < 0).any())
        assert float(w.abs().min()) >= 0.5 and w.unique().numel() > 1 and b.unique().numel() > 1


# ---------------------------------------------------------------------------------------------------- honest emulations pass, mutants fail
CHAN_EMU = [(f32, 3, 67, 8, 16, 4), (bf, 2, 41, 16, 8, 8)]              # (dt, G, P, C, STRIP, np)


@pytest.mark.parametrize("dt,G,Pn,Cc,S,np_", CHAN_EMU)
def test_exact_sums_gate_sees_every_lost_or_misplaced_term(dt, G, Pn, Cc, S, np_):
    a, b = R.chan_inputs(G, Pn, Cc, seed=7)
    want = R.dot64(a, b)
    for seed in (0, 1):
        assert exact(R.emu_strip_sums(a * b, a, S, np_, seed=seed), want)
    assert not exact(R.emu_strip_sums(a * b, a, S, np_, drop_last_pixel=True), want)                  # last pixel of a strip dropped
    assert not exact(R.emu_strip_sums(a * b, a, S, np_, skip_strip=1), want)                          # one strip left out of a finalize
    assert not exact(R.emu_strip_sums(a * b, a, S, np_, slot_shift=1), want)                          # a channel vector in the next slot
    assert not exact(R.emu_strip_sums(a * b, a, S, np_, group_shift=1), want)                         # group boundary off by one pixel
    x, dy, mean, rstd, w, bb = R.bwd_exact_inputs(G, Pn, Cc, seed=9)
    for act in (R.ACT_NONE, R.ACT_RELU):
        bs64, dw64, db64 = R.bwd_stats64(x, dy, mean, rstd, w, bb, act)
        _, bs, dw, db = R.emu_norm_bwd(x, dy, mean, rstd, w, bb, act, float(Pn), dt, S, np_)
        assert exact(bs, bs64) and exact(dw, dw64) and exact(db, db64)
        _, bs, dw, db = R.emu_norm_bwd(x, dy, mean, rstd, w, bb, act, float(Pn), dt, S, np_, drop_last_pixel=True)
        assert not exact(bs, bs64) and not (exact(dw, dw64) and exact(db, db64))


def test_layernorm_backward_gates():
    """honest: dw, db to the bit in any strip order, dx inside its bound in fp32 and bf16.  Rejected: a strip's last row missing from
    dw / db (dx is right: only the exact gate sees it), dw and db swapped, c1 over D - VEC columns, an unwritten row"""
    rows, D, S = 37, 24, 16
    x, dy, mean, rstd, w, dres = R.ln_bwd_inputs(rows, D, seed=3)
    for dt in R.DTS:
        for dr in (None, dres):
            dx64, dwdb64, (g, c1, c2, xh) = R.ln_bwd64(x, dy, w, mean, rstd, dr)
            bound = R.ln_dx_bound(dx64, rstd.double(), g, c1, c2, xh, dr, R.U[dt])
            for seed in (0, 1):
                dx, dwdb = R.emu_ln_bwd(x, dy, w, mean, rstd, dr, dt, S, seed=seed)
                assert exact(dwdb, dwdb64) and inside(dx, dx64, bound)
            dx, dwdb = R.emu_ln_bwd(x, dy, w, mean, rstd, dr, dt, S, tail_row_missing=True)
            assert inside(dx, dx64, bound) and not exact(dwdb, dwdb64)
            dx, dwdb = R.emu_ln_bwd(x, dy, w, mean, rstd, dr, dt, S, swapped=True)
            assert not exact(dwdb, dwdb64)
            dx, _ = R.emu_ln_bwd(x, dy, w, mean, rstd, dr, dt, S, c1_short=R.VEC[dt])
            assert not inside(dx, dx64, bound)
            dx, _ = R.emu_ln_bwd(x, dy, w, mean, rstd, dr, dt, S, unwritten_row=rows - 1)
            assert not inside(dx, dx64, bound)
    # the bound of the wide rows the GPU file uses still sees c1 over D - VEC columns
    x, dy, mean, rstd, w, dres = R.ln_bwd_inputs(5, 4096, seed=4)
    dx64, _, (g, c1, c2, xh) = R.ln_bwd64(x, dy, w, mean, rstd, None)
    bound = R.ln_dx_bound(dx64, rstd.double(), g, c1, c2, xh, None, R.U[f32])
    assert inside(R.emu_ln_bwd(x, dy, w, mean, rstd, None, f32, 4)[0], dx64, bound)
    assert not inside(R.emu_ln_bwd(x, dy, w, mean, rstd, None, f32, 4, c1_short=4)[0], dx64, bound)


@pytest.mark.parametrize("odt", R.DTS, ids=["f32", "bf16"])
def test_layernorm_forward_gates(odt):
    """honest fp32 arithmetic: mean to the bit, rstd and y inside their bounds; an element computed with its neighbour row's statistics
    or its neighbour column's weight is outside"""
    for rows, D in ((9, 8), (5, 260), (3, 4096)):
        x, m, a, w, b = R.ln_draw(rows, D, seed=D)
        y64, m64, r64 = R.ln_fwd64(x, w, b, R.EPS_LN)
        yb = R.y_bound(y64, x.double(), m64[:, None], r64[:, None], w.double(), b.double(), R.U[odt])
        y, mean, rstd = R.emu_ln_fwd(x, w, b, R.EPS_LN, odt)
        assert exact(mean, m64) and inside(rstd, r64, 4 * R.UF * r64) and inside(y, y64, yb)
        assert not inside(R.emu_ln_fwd(x, w.roll(1), b, R.EPS_LN, odt)[0], y64, yb)
        assert not inside(y.roll(1, 0), y64, yb)


@pytest.mark.parametrize("dt", R.DTS, ids=["f32", "bf16"])
@pytest.mark.parametrize("actname", list(R.ACTS))
def test_norm_act_gates(dt, actname):
    """the chain statistics -> y -> backward sums -> dx in honest fp32 passes the gates of test_norm_act_bounds; rejected: the leaky
    slope applied at z = 0 only, the mean taken through bf16, the biased running variance, a write behind the buffer"""
    act = R.ACTS[actname]
    G, Pn, Cc, S, np_ = 2, 90, 8, 32, 8
    x, m, s = R.two_value_draw(G, Pn, Cc, seed=11)
    w, b = R.affine_for(Cc, seed=3)
    dy = X.integers(G, Pn, Cc, seed=3, lo=-4, hi=4)
    f = R.norm_formulas64(x, dy, w, b, act, R.EPS_N)
    sums = R.emu_strip_sums(x, x * x, S, np_, seed=1)
    assert exact(sums, R.stats64(x))
    mean, rstd = R.emu_stats_finalize(sums, float(Pn), R.EPS_N)
    assert inside(mean, f["mean"], R.mean_bound(x.double().abs().mean(1), False))                      # exact sums: depth 0
    assert inside(rstd, f["rstd"], R.rstd_bound(f["rstd"], f["var"], f["ex2"], f["mean"], R.EPS_N, False))
    yb = R.y_bound(f["y"], x.double(), f["mean"][:, None], f["rstd"][:, None], w.double(), b.double(), R.U[dt])
    assert inside(R.emu_norm_fwd(x, mean, rstd, w, b, act, dt), f["y"], yb)
    depth = R.cdiv(S, np_) + np_ + R.cdiv(Pn, S)
    db_ = R.dx_bound(f["dx"], w.double(), f["rstd"][:, None], f["dz"], f["k1"][:, None], f["k2"][:, None], f["xh"], R.U[dt], depth, f["mdz"][:, None],
                     f["mdzxh"][:, None])
    dx, bs, dw, db = R.emu_norm_bwd(x, dy, mean, rstd, w, b, act, float(Pn), dt, S, np_, seed=2)
    assert inside(dx, f["dx"], db_)
    assert inside(dw, f["dw"], (8 + depth + G) * R.UF * (f["dz"] * f["xh"]).abs().sum((0, 1)))
    assert inside(db, f["db"], (1 + depth + G) * R.UF * f["dz"].abs().sum((0, 1)))
    if act == R.ACT_LEAKY:
        dx, _, dw, _ = R.emu_norm_bwd(x, dy, mean, rstd, w, b, act, float(Pn), dt, S, np_, leaky_at_zero_only=True)
        assert not inside(dx, f["dx"], db_) and not inside(dw, f["dw"], (8 + depth + G) * R.UF * (f["dz"] * f["xh"]).abs().sum((0, 1)))
    # the mean through bf16: m in [-3, 3] survives bf16, so the draw that shows it has a mean bf16 cannot hold
    x2 = x + 1.0 / 256
    f2 = R.norm_formulas64(x2, dy, w, b, act, R.EPS_N)
    s2 = R.emu_strip_sums(x2, x2 * x2, S, np_)
    ok_, bad = R.emu_stats_finalize(s2, float(Pn), R.EPS_N), R.emu_stats_finalize(s2, float(Pn), R.EPS_N, mean_bf16=True)
    mb = R.mean_bound(x2.double().abs().mean(1), False)
    assert inside(ok_[0], f2["mean"], mb) and not inside(bad[0], f2["mean"], mb)
    # running statistics: unbiased passes, biased is outside
    rm0, rv0 = X.integers(Cc, seed=4, lo=-3, hi=3), X.integers(Cc, seed=5, lo=1, hi=3)
    x1 = R.two_value_draw(1, Pn, Cc, seed=12)[0]
    f1 = R.norm_formulas64(x1, x1, w, b, R.ACT_NONE, R.EPS_N)
    st, wrong = (R.stats_finalize64(R.stats64(x1), float(Pn), R.EPS_N, rm0, rv0, 0.1, biased=k) for k in (False, True))
    _, _, rm, rv = R.emu_stats_finalize(R.emu_strip_sums(x1, x1 * x1, S, np_), float(Pn), R.EPS_N, rm0, rv0, 0.1)
    unb = Pn / (Pn - 1.0)
    vb = R.run_bound(rv0.double(), f1["var"][0] * unb) + 0.1 * unb * R.var_bound(f1["ex2"][0], f1["mean"][0])
    assert inside(rm, st[4], R.run_bound(rm0.double(), f1["mean"][0]) + 0.1 * R.mean_bound(x1.double().abs().mean(1)[0], False))
    assert inside(rv, st[5], vb) and not inside(wrong[5].float(), st[5], vb)


def test_guard_band_sees_an_unwritten_element_and_a_write_behind_the_buffer():
    whole = torch.full((10 + X.GUARD_ROWS,), X.SENTINEL)
    s = torch.tensor(X.SENTINEL)
    whole[:10] = 1.0
    assert bool((whole[10:] == s).all()) and not bool((whole[:10] == s).any())
    whole[10] = 0.0                                                    # a write behind the buffer
    assert not bool((whole[10:] == s).all())
    w2, v2 = X.guarded(4, 8, bf, "cpu")
    v2[:3] = 1.0                                                       # an unwritten row
    with pytest.raises(AssertionError):
        X.assert_guard(w2, 4)
    v2[3] = 1.0
    X.assert_guard(w2, 4)
    w2[4, 0] = 0.0
    with pytest.raises(AssertionError):
        X.assert_guard(w2, 4)


# ---------------------------------------------------------------------------------------------------- offset statistics
@pytest.mark.parametrize("m", R.OFFSETS, ids=lambda m: f"m{int(m)}")
@pytest.mark.parametrize("dt", R.DTS, ids=["f32", "bf16"])
def test_one_pass_variance_stays_inside_its_bound(dt, m):
    """blocked fp32 sums and E[x^2] - mean^2 on N(+-m, 1) and a constant channel: mean, rstd and y inside the bounds the GPU test uses
    (the formula's own error, not a kernel's)"""
    Cc, Pn = 8, 1024
    w, b = R.affine_for(Cc, seed=1)
    x = R.offset_draw(Pn, Cc, m, seed=int(m))
    f, dm, dr, yb = R.offset_bounds(x, w, b, R.EPS_N, R.U[dt], 16 + 4 + 16)        # 16 pixels per lane, 4 lanes, 16 strips
    assert float(f["var"][0, -1]) == 0.0
    mean, rstd = R.emu_stats_finalize(R.emu_strip_sums(x, x * x, 64, 4, seed=1), float(Pn), R.EPS_N)
    print(f"[share] emulated offset m {m}: mean {share(mean, f['mean'], dm):.3f} rstd {share(rstd, f['rstd'], dr):.3f}")
    assert inside(mean, f["mean"], dm) and inside(rstd, f["rstd"], dr)
    assert inside(R.emu_norm_fwd(x, mean, rstd, w, b, R.ACT_NONE, dt), f["y"], yb)
    if m >= 8:                                                          # the gate is not vacuous: a mean through bf16 is outside
        bad = R.emu_stats_finalize(R.emu_strip_sums(x, x * x, 64, 4, seed=1), float(Pn), R.EPS_N, mean_bf16=True)
        assert not inside(bad[0], f["mean"], dm)
