"""The kernels of csrc/norm.hip against exact and fp64 references (tests/_norm_ref.py, kept honest by tests/test_cpu_norms.py) at the
edges of their regimes: the shuffle and LDS combines of the strip reductions, idle pixel lanes, several channel passes, one strip, a
last strip of one pixel, the unrolled pixel loops under the slot caps, the finalize kernels at the edges of their strip unrolling and on
both sides of their column-count switches, every vector count of the LayerNorm kernels and the row counts at which a wave of the fused
backward takes its first, second and no row.

Instruments.  Exact inputs (small integers, dyadic statistics and weights): every sum must equal the fp64 value bit for bit.  Where a
result passes through rsqrtf, a count that is no power of two or a bf16 rounding: a per-element bound derived in _norm_ref.py; the worst
share of each bound is printed.  Every case names its regime and asserts, through du_reduce_ws_elems and the formulas restated in
_norm_ref.py, that it is reached.  Every buffer a kernel writes directly through the C ABI is pre-filled with the sentinel and followed
by a guard band: every element must have been written and nothing behind the buffer touched.

Not covered: the scratch-less atomic fall-backs of strip_launch (no caller reaches them), layernorm_bwd_prod of norm_gemm.hip (its own
file), the multi-process SyncBN collectives."""
import pytest
import torch

import _exact as X
import _norm_ref as R
from test_gpu_ops import dev
from test_gpu_small_ops import L, assert_flat_guard, call, code, flat_guarded, ok, untouched
from test_gpu_small_ops import P as ptr

pytestmark = pytest.mark.gpu

bf, f32 = R.bf, R.f32
DT_IDS = ["f32", "bf16"]
SHARES = {}


def gate(out, ref64, bound, what):
    """the per-element gate; prints the worst share of the bound"""
    good, msg = R.within(out, ref64, bound, what)
    share = float(((out.detach().cpu().double() - ref64).abs() / torch.as_tensor(bound, dtype=torch.float64).expand_as(ref64).clamp_min(1e-300)).max())
    key = what.split(":")[0]
    if share > SHARES.get(key, -1.0):
        SHARES[key] = share
        print(f"[share] {key}: {share:.3f} ({what})")
    assert good, msg


def fbuf(n, d, dt=f32):
    return flat_guarded(n, dt, d)


def nhwc(t, d, dt):
    """(G, P, C) on the CPU -> (G, 1, P, C) NHWC on the device"""
    return t.to(d, dt).unsqueeze(1).contiguous()


def wide(t, lo=None):
    """t (..., C) as a channel slice of a tensor twice as wide (pitch 2 C), one 16-byte vector in unless lo says otherwise"""
    Cc = t.shape[-1]
    lo = R.VEC[t.dtype] if lo is None else lo
    w = torch.full(t.shape[:-1] + (2 * Cc,), 99.0, dtype=t.dtype, device=t.device)
    v = w[..., lo:lo + Cc]
    v.copy_(t)
    assert v.data_ptr() % 16 == 0 and (2 * Cc) % R.VEC[t.dtype] == 0
    return v


def scratch(dt, G, Pn, Cc, d):
    """(ws, n): the scratch du_reduce_ws_elems asks for; n must be what the restated pick_strip gives"""
    n = int(L().du_reduce_ws_elems(code(dt), G, Pn, Cc))
    assert n == R.ws_elems(G, Pn, Cc, dt), f"pick_strip has changed: {n} scratch floats, the restated formula gives {R.ws_elems(G, Pn, Cc, dt)}"
    return torch.full((n + X.GUARD_ROWS,), X.SENTINEL, dtype=f32, device=d), n


# ---------------------------------------------------------------------------------------------------- 1. channel sums to the bit
@pytest.mark.parametrize("case", R.CHAN_CASES, ids=R.chan_id)
def test_chan_sums_to_the_bit(case):
    """du_chan_stats (and ops.chan_stats), du_chan_dot and du_colsum (and ops.colsum) on integers in [-4, 4]: (sum, sum of squares),
    (sum a b, sum a) and the column sums equal the fp64 sums bit for bit; contiguous and as a channel slice of a wider tensor.  (The sums of
    squares of a few thousand pixels pass the sentinel's magnitude: the comparison is exact either way, and no sum of these draws equals it.)"""
    from dinounet_amd import ops
    dt, Cc, name = case
    d = dev()
    assert R.chan_regime_ok(dt, Cc, name), case
    for G, Pn, what in R.chan_gp(dt, Cc):
        tag = f"{R.chan_id(case)} G {G} P {Pn} ({what})"
        assert R.gp_regime_ok(dt, Cc, G, Pn, what), tag
        R.require_sums_exact(Pn, 16.0)
        a, b = R.chan_inputs(G, Pn, Cc, seed=Cc + G + Pn)
        ws, n = scratch(dt, G, Pn, Cc, d)
        for slice_ in (False, True):
            ag, bg = nhwc(a, d, dt), nhwc(b, d, dt)
            if slice_:
                ag, bg = wide(ag), wide(bg, 0)
            lda = ldb = 2 * Cc if slice_ else Cc
            sw, sv = fbuf(G * Cc * 2, d)
            ok("du_chan_stats", code(dt), ptr(ag), lda, ptr(sv), G, Pn, Cc, ptr(ws), n)
            assert_flat_guard(sw, G * Cc * 2, what=tag + " stats")
            X.assert_exact(sv.view(G, Cc, 2), R.stats64(a), tag + f" stats slice {slice_}", sentinel=False)
            s2, p2 = ops.chan_stats(ag, G)
            assert p2 == Pn and torch.equal(s2, sv.view(G, Cc, 2)), tag
            dw_, dv = fbuf(G * Cc * 2, d)
            ok("du_chan_dot", code(dt), ptr(ag), lda, ptr(bg), ldb, ptr(dv), G, Pn, Cc, ptr(ws), n)
            assert_flat_guard(dw_, G * Cc * 2, what=tag + " dot")
            X.assert_exact(dv.view(G, Cc, 2), R.dot64(a, b), tag + f" dot slice {slice_}", sentinel=False)
            if G == 1:
                cw, cv = fbuf(Cc, d)
                ok("du_colsum", code(dt), ptr(ag), lda, ptr(cv), Pn, Cc, ptr(ws), n)
                assert_flat_guard(cw, Cc, what=tag + " colsum")
                X.assert_exact(cv, a.double().sum((0, 1)), tag + f" colsum slice {slice_}", sentinel=False)
                assert torch.equal(ops.colsum(ag.view(Pn, Cc) if not slice_ else ag[0, 0]), cv), tag
        assert bool((ws[n:] == X.SENTINEL).all()), tag + ": a write behind the scratch"


# ---------------------------------------------------------------------------------------------------- 2. backward sums to the bit
def bwd_stats_both_routes(dt, G, Pn, Cc, act, d, seed, tag):
    """du_norm_act_bwd_stats_grads against du_norm_act_bwd_stats + du_norm_param_grads against fp64, all bit for bit"""
    x, dy, mean, rstd, w, b = R.bwd_exact_inputs(G, Pn, Cc, seed)
    X.require_exact(G * Pn * 48.0, 0.5)
    xh, z, _ = R.norm_terms64(x, dy, mean, rstd, w, b, act)
    assert float(z.abs().min()) >= 0.125, tag
    bs64, dw64, db64 = R.bwd_stats64(x, dy, mean, rstd, w, b, act)
    xg, dyg = nhwc(x, d, dt), wide(nhwc(dy, d, dt))
    mg, rg, wg, bg = (t.to(d).contiguous() for t in (mean, rstd, w, b))
    ws, n = scratch(dt, G, Pn, Cc, d)
    res = []
    for fused in (True, False):
        bw, bv = fbuf(G * Cc * 2, d)
        ww, wv = fbuf(Cc, d)
        dbw, dbv = fbuf(Cc, d)
        if fused:
            ok("du_norm_act_bwd_stats_grads", code(dt), ptr(xg), Cc, ptr(dyg), 2 * Cc, ptr(mg), ptr(rg), ptr(wg), ptr(bg), ptr(bv), ptr(wv), ptr(dbv),
               G, Pn, Cc, act, ptr(ws), n)
        else:
            ok("du_norm_act_bwd_stats", code(dt), ptr(xg), Cc, ptr(dyg), 2 * Cc, ptr(mg), ptr(rg), ptr(wg), ptr(bg), ptr(bv), G, Pn, Cc, act, ptr(ws), n)
            ok("du_norm_param_grads", ptr(bv), ptr(wv), ptr(dbv), G, Cc)
        for whole, view, ref, nm in ((bw, bv.view(G, Cc, 2), bs64, "bsums"), (ww, wv, dw64, "dw"), (dbw, dbv, db64, "db")):
            assert_flat_guard(whole, view.numel(), what=f"{tag} {nm} fused {fused}")
            X.assert_exact(view, ref, f"{tag} {nm} fused {fused}")
        res.append((bv.clone(), wv.clone(), dbv.clone()))
    assert all(torch.equal(p, q) for p, q in zip(*res)), tag + ": the two routes differ"
    assert bool((ws[n:] == X.SENTINEL).all()), tag + ": a write behind the scratch"


@pytest.mark.parametrize("actname", ["none", "relu"])
@pytest.mark.parametrize("case", R.CHAN_CASES, ids=R.chan_id)
def test_bwd_stats_to_the_bit(case, actname):
    """chosen statistics (integer mean, rstd in {0.5, 1, 2}, dyadic w, b an odd multiple of 1/8) make xhat and z exact and z never 0:
    bsums, dw and db equal the fp64 sums bit for bit on both routes"""
    dt, Cc, name = case
    d = dev()
    assert R.chan_regime_ok(dt, Cc, name), case
    for G, Pn, what in R.chan_gp(dt, Cc):
        assert R.gp_regime_ok(dt, Cc, G, Pn, what)
        bwd_stats_both_routes(dt, G, Pn, Cc, R.ACTS[actname], d, Cc + G + Pn, f"{R.chan_id(case)} G {G} P {Pn} ({what}) {actname}")


@pytest.mark.parametrize("dt", R.DTS, ids=DT_IDS)
def test_bwd_stats_every_residue_of_the_unrolled_loop(dt):
    """one strip of 1 .. U np pixels at np = 4 (U = 4 for bf16, 2 for fp32), and U np + 1 .. 2 U np - 1 in two strips"""
    Cc, Un = R.UNROLL[dt]
    d = dev()
    assert R.lanes(Cc, dt)[1] == 4
    for Pn in range(1, 2 * Un * 4):
        S = R.pick_strip(1, Pn, Cc, dt)
        assert S == min(Pn, 16)
        bwd_stats_both_routes(dt, 2, Pn, Cc, R.ACT_RELU, d, Pn, f"P {Pn}")


@pytest.mark.parametrize("case", R.GRADS_CASES, ids=lambda c: f"{'f32' if c[0] == f32 else 'bf16'}-G{c[1]}-P{c[2]}-C{c[3]}-cols{c[4]}")
def test_finalize_grads_switch_and_strip_unrolling(case):
    """finalize_grads_kernel on both sides of C 2 = 512, with more strips than two trips of its strip lanes, and over several groups"""
    dt, G, Pn, Cc, cols, least = case
    assert R.finalize_cols(Cc * 2, 512) == cols
    n = R.strips(G, Pn, Cc, dt)
    assert n >= least, (n, case)
    bwd_stats_both_routes(dt, G, Pn, Cc, R.ACT_RELU, dev(), Pn, str(case) + f" strips {n}")


# ---------------------------------------------------------------------------------------------------- 3. finalize kernels on synthetic partials
@pytest.mark.parametrize("case", R.FIN_CASES, ids=lambda c: f"cols{c[0]}-G{c[1]}-C{c[2]}-strips{c[3]}")
def test_finalize_on_synthetic_partials(case):
    """du_strip_finalize (first_only 0) and du_strip_finalize_norm: totals to the bit; with a power-of-two count the mean to the bit;
    rstd and the running statistics within their bounds"""
    cols, G, Cc, n = case
    d = dev()
    assert R.finalize_cols(G * Cc * 2, 4096) == cols
    part = R.fin_inputs(G, n, Cc, seed=n + Cc)
    X.require_exact(n * 12.0)
    tot = R.fin64(part, G)
    pg = part.to(d)
    ow, ov = fbuf(G * Cc * 2, d)
    ok("du_strip_finalize", ptr(pg), ptr(ov), G, n, Cc)
    assert_flat_guard(ow, G * Cc * 2, what=f"{case} out")
    X.assert_exact(ov.view(G, Cc, 2), tot, f"{case} totals")
    for count in (float(2 ** (n * 8).bit_length()), float(n * 8 + 3)):
        pow2 = count == 2 ** (n * 8).bit_length()
        for run in ((True, False) if G == 1 else (False,)):
            sw, sv = fbuf(G * Cc * 2, d)
            mw, mv = fbuf(G * Cc, d)
            rw, rv_ = fbuf(G * Cc, d)
            rm0, rv0 = X.integers(Cc, seed=1, lo=-4, hi=4) / 4, X.integers(Cc, seed=2, lo=1, hi=8) / 4
            rmg, rvg = rm0.to(d).clone(), rv0.to(d).clone()
            ok("du_strip_finalize_norm", ptr(pg), ptr(sv), G, n, Cc, count, R.EPS_N, ptr(mv), ptr(rv_), ptr(rmg) if run else None,
               ptr(rvg) if run else None, 0.1)
            for whole, k in ((sw, G * Cc * 2), (mw, G * Cc), (rw, G * Cc)):
                assert_flat_guard(whole, k, what=f"{case} count {count}")
            X.assert_exact(sv.view(G, Cc, 2), tot, f"{case} sums of finalize_norm")
            st = R.stats_finalize64(tot, count, R.EPS_N, rm0 if run else None, rv0 if run else None, 0.1)
            m64, var64, r64, ex2 = st[:4]
            unb = count / (count - 1.0)
            if pow2:
                X.assert_exact(mv.view(G, Cc), m64, f"{case} mean")
            gate(mv.view(G, Cc), m64, 2 * R.UF * m64.abs(), f"finalize mean: {case} count {count}")
            gate(rv_.view(G, Cc), r64, R.rstd_bound(r64, var64, ex2, m64, R.EPS_N, exact=False), f"finalize rstd: {case} count {count}")
            if run:
                gate(rmg, st[4], R.run_bound(rm0.double(), m64[0]), f"finalize run_mean: {case}")
                gate(rvg, st[5], R.run_bound(rv0.double(), var64[0] * unb) + 0.1 * unb * R.var_bound(ex2[0], m64[0]), f"finalize run_var: {case}")


# ---------------------------------------------------------------------------------------------------- 4. LayerNorm forward
def ln_fwd_direct(xg, ldx, w, b, rows, D, idt, odt, d, stats=True):
    yw, yv = X.guarded(rows, D, odt, d)
    mw, mv = fbuf(rows, d)
    rw, rv = fbuf(rows, d)
    rc = call("du_layernorm_fwd", code(idt), code(odt), ptr(xg), ldx, ptr(w), ptr(b), ptr(yv), D, ptr(mv) if stats else None, ptr(rv) if stats else None,
              rows, D, R.EPS_LN)
    return rc, (yw, yv), (mw, mv), (rw, rv)


@pytest.mark.parametrize("pair", R.LN_PAIRS, ids=lambda p: "-".join("f32" if t == f32 else "bf16" for t in p))
def test_layernorm_fwd_bounds(pair):
    """every D of the list (MAXV 1 .. 16, a partly filled last vector round) x rows 1 .. 9 on the two-value draw: mean to the bit, rstd
    and y within their bounds; as a column slice of a wider tensor; with and without the statistics; one row per wave and two"""
    idt, odt = pair
    d = dev()
    seen = set()
    try:
        for D in R.LN_D[idt]:
            seen.add(R.ln_maxv(D, idt))
            for rows in R.LN_FWD_ROWS:
                x, m, a, w, b = R.ln_draw(rows, D, seed=D + rows)
                R.require_sums_exact(D, 49.0)
                y64, m64, r64 = R.ln_fwd64(x, w, b, R.EPS_LN)
                assert torch.equal(m64, m.double())
                yb = R.y_bound(y64, x.double(), m64[:, None], r64[:, None], w.double(), b.double(), R.U[odt])
                wg, bg = w.to(d), b.to(d)
                first = None
                for opt in (0, 2):
                    L().du_set_option(18, opt)
                    for slice_ in (False, True):
                        xg = x.to(d, idt)
                        xg = wide(xg) if slice_ else xg
                        tag = f"D {D} rows {rows} option {opt} slice {slice_}"
                        rc, (yw, yv), (mw, mv), (rw, rv) = ln_fwd_direct(xg, 2 * D if slice_ else D, wg, bg, rows, D, idt, odt, d)
                        assert rc == 0, tag
                        X.assert_guard(yw, rows, tag + " y")
                        assert_flat_guard(mw, rows, what=tag + " mean")
                        assert_flat_guard(rw, rows, what=tag + " rstd")
                        X.assert_exact(mv, m64, tag + " mean")
                        gate(rv, r64, 4 * R.UF * r64, f"LayerNorm rstd: {tag}")
                        gate(yv, y64, yb, f"LayerNorm y {'bf16' if odt == bf else 'f32'}: {tag}")
                        if first is None:
                            first = (yv.clone(), rv.clone())
                        assert torch.equal(yv, first[0]) and torch.equal(rv, first[1]), tag + ": differs from the one-row contiguous launch"
                    rc, (yw, yv), (mw, _), (rw, _) = ln_fwd_direct(x.to(d, idt), D, wg, bg, rows, D, idt, odt, d, stats=False)
                    assert rc == 0 and untouched(mw) and untouched(rw)
                    X.assert_guard(yw, rows, f"D {D} rows {rows} without statistics")
                    assert torch.equal(yv, first[0])
    finally:
        L().du_set_option(18, 1)
    assert seen == {1, 2, 4, 5, 8, 16}, seen


@pytest.mark.parametrize("dt", R.DTS, ids=DT_IDS)
def test_layernorm_refuses_more_than_16_vectors_per_lane(dt):
    D = R.LN_D_REFUSED[dt]
    assert R.ln_route(D, dt) == "unsupported"
    d = dev()
    x = torch.zeros(2, D, dtype=dt, device=d)
    w = torch.ones(D, device=d)
    rc, (yw, _), (mw, _), (rw, _) = ln_fwd_direct(x, D, w, w, 2, D, dt, dt, d)
    assert rc == -2
    dxw, dxv = X.guarded(2, D, dt, d)
    gw, gv = fbuf(2 * D, d)
    ws, n = scratch(dt, 1, 2, D, d)
    st = torch.ones(2, device=d)
    assert call("du_layernorm_bwd", code(dt), ptr(x), ptr(x), ptr(w), ptr(st), ptr(st), ptr(dxv), ptr(gv), 2, D, ptr(ws), n, None) == -2
    torch.cuda.synchronize()
    assert all(untouched(t) for t in (yw, mw, rw, dxw, gw, ws))


# ---------------------------------------------------------------------------------------------------- 5. LayerNorm backward
def ln_bwd_case(dt, rows, D, d, with_res):
    tag = f"{'bf16' if dt == bf else 'f32'} rows {rows} D {D} dres {with_res} ({R.ln_route(D, dt)})"
    x, dy, mean, rstd, w, dres = R.ln_bwd_inputs(rows, D, seed=rows + D)
    X.require_exact(rows * 48.0, 0.25)
    X.require_exact(D * 96.0, 0.25)
    dx64, dwdb64, (g, c1, c2, xh) = R.ln_bwd64(x, dy, w, mean, rstd, dres if with_res else None)
    dxw, dxv = X.guarded(rows, D, dt, d)
    gw, gv = fbuf(2 * D, d)
    ws, n = scratch(dt, 1, rows, D, d)
    xg, dyg, drg = x.to(d, dt), dy.to(d, dt), dres.to(d, dt)
    wg, mg, rg = w.to(d), mean.to(d), rstd.to(d)
    ok("du_layernorm_bwd", code(dt), ptr(xg), ptr(dyg), ptr(wg), ptr(mg), ptr(rg), ptr(dxv), ptr(gv), rows, D, ptr(ws), n,
       ptr(drg) if with_res else None)
    X.assert_guard(dxw, rows, tag + " dx")
    assert_flat_guard(gw, 2 * D, what=tag + " dwdb")
    assert bool((ws[n:] == X.SENTINEL).all()), tag + ": a write behind the scratch"
    X.assert_exact(gv.view(2, D), dwdb64, tag + " (dw, db) planar")
    gate(dxv, dx64, R.ln_dx_bound(dx64, rstd.double(), g, c1, c2, xh, dres if with_res else None, R.U[dt]),
         f"LayerNorm dx {'bf16' if dt == bf else 'f32'} {R.ln_route(D, dt)}: {tag}")


@pytest.mark.parametrize("dt", R.DTS, ids=DT_IDS)
def test_layernorm_bwd_every_vector_count(dt):
    """every accepted D (fused up to maxv 4, the dx + column-reduction pair above) at 37 rows: dw, db planar and to the bit, dx within
    its bound, with and without dres"""
    d = dev()
    routes = set()
    for D in R.LN_D[dt]:
        routes.add(R.ln_route(D, dt))
        assert (R.ln_route(D, dt) == "pair") == (D >= R.LN_FIRST_PAIR[dt])
        for with_res in (False, True):
            ln_bwd_case(dt, 37, D, d, with_res)
    assert routes == {"fused", "pair"}


@pytest.mark.parametrize("dt", R.DTS, ids=DT_IDS)
def test_layernorm_bwd_rows_of_a_strip(dt):
    """strips of 16 rows: a wave's second row live or not, a last strip of one row, three strips"""
    D = R.LN_BWD_D[dt]
    d = dev()
    assert R.ln_route(D, dt) == "fused" and R.lanes(D, dt)[1] == 4
    for rows in R.LN_BWD_ROWS:
        assert R.pick_strip(1, rows, D, dt) == min(rows, 16)
        for with_res in (False, True):
            ln_bwd_case(dt, rows, D, d, with_res)


@pytest.mark.parametrize("dt", R.DTS, ids=DT_IDS)
def test_layernorm_bwd_second_trip_of_a_wave(dt):
    rows, D = R.LN_TWO_TRIPS[dt]
    assert R.ln_route(D, dt) == "fused" and R.ln_rows_per_wave(rows, D, dt) >= 3 and R.pick_strip(1, rows, D, dt) >= 9
    ln_bwd_case(dt, rows, D, dev(), True)


# ---------------------------------------------------------------------------------------------------- 6. norm_act through ops and autograd
@pytest.mark.parametrize("mode", R.NORM_ACT_MODES)
@pytest.mark.parametrize("actname", list(R.ACTS))
@pytest.mark.parametrize("shape", R.NORM_ACT_SHAPES, ids=lambda s: f"{'f32' if s[0] == f32 else 'bf16'}-G{s[1]}-P{s[2]}-C{s[3]}")
def test_norm_act_bounds(shape, actname, mode):
    """ops.norm_act forward and backward against fp64 F.instance_norm / F.batch_norm + activation on the two-value draw: y, dx, dw, db
    per element, the running statistics of training BatchNorm, eval forward and eval backward (dx = dz w rstd)"""
    from dinounet_amd import ops
    dt, G, Pn, Cc = shape
    act = R.ACTS[actname]
    d = dev()
    kind = "in" if mode == "in" else "bn"
    Gn, Pg = (G, Pn) if kind == "in" else (1, G * Pn)                  # BatchNorm: one group of all the pixels
    x, m, s = R.two_value_draw(Gn, Pg, Cc, seed=Pn + Cc)
    w, b = R.affine_for(Cc, seed=Cc)
    dy = X.integers(Gn, Pg, Cc, seed=3, lo=-4, hi=4)
    rm0, rv0 = X.integers(Cc, seed=4, lo=-3, hi=3), X.integers(Cc, seed=5, lo=1, hi=3)
    training = mode != "bn-eval"
    if not training:
        b = R.bias_for_eval(m[0], rm0, rv0, w, R.EPS_N)
    y64, dx64, dw64, db64, rm64, rv64 = R.torch_norm_act64(x, dy, w, b, kind, act, R.EPS_N, training, None if kind == "in" else rm0,
                                                             None if kind == "in" else rv0)
    if training:
        f = R.norm_formulas64(x, dy, w, b, act, R.EPS_N)
    else:
        f = R.norm_formulas64(x, dy, w, b, act, R.EPS_N, mean=rm0.double()[None], var=rv0.double()[None], use_batch=False)
    assert float(f["z"].abs().min()) >= 0.25
    assert float((f["y"] - y64).abs().max()) < 1e-12 and float((f["dx"] - dx64).abs().max()) < 1e-11
    xg = x.to(d, dt).view(Gn, 1, Pg, Cc).requires_grad_(True)
    wg, bg = w.to(d).requires_grad_(True), b.to(d).requires_grad_(True)
    rmg, rvg = rm0.to(d).clone(), rv0.to(d).clone()
    y = ops.norm_act(xg, wg, bg, kind, act, R.EPS_N, training, None if kind == "in" else rmg, None if kind == "in" else rvg, 0.1, None)
    dx, dw, db = torch.autograd.grad(y, (xg, wg, bg), dy.to(d, dt).view(Gn, 1, Pg, Cc))
    tag = f"{mode} {actname} {shape}"
    name = "bf16" if dt == bf else "f32"
    mean, rstd = f["mean"][:, None], f["rstd"][:, None]
    gate(y.detach().view(Gn, Pg, Cc), y64, R.y_bound(y64, x.double(), mean, rstd, w.double(), b.double(), R.U[dt]), f"norm_act y {name}: {tag}")
    depth = R.sum_depth(Gn, Pg, Cc, dt)
    gate(dx.view(Gn, Pg, Cc), dx64, R.dx_bound(dx64, w.double(), rstd, f["dz"], f["k1"][:, None], f["k2"][:, None], f["xh"], R.U[dt], depth,
                                                f["mdz"][:, None], f["mdzxh"][:, None]), f"norm_act dx {name}: {tag}")
    terms = (f["dz"] * f["xh"]).abs().sum((0, 1))
    gate(dw, dw64, (8 + depth + Gn) * R.UF * terms, f"norm_act dw: {tag}")        # the terms' 8 roundings (dx_bound) and the additions
    gate(db, db64, (1 + depth + Gn) * R.UF * f["dz"].abs().sum((0, 1)), f"norm_act db: {tag}")
    if mode == "bn-train":
        pow2 = (Pg & (Pg - 1)) == 0
        unb = Pg / (Pg - 1.0)
        gate(rmg, rm64, R.run_bound(rm0.double(), f["mean"][0]), f"run_mean: {tag}")
        gate(rvg, rv64, R.run_bound(rv0.double(), f["var"][0] * unb) + (0 if pow2 else 0.1 * unb * R.var_bound(f["ex2"][0], f["mean"][0])), f"run_var: {tag}")
    elif kind == "bn":
        assert torch.equal(rmg.cpu(), rm0) and torch.equal(rvg.cpu(), rv0), "eval changed the running statistics"


# ---------------------------------------------------------------------------------------------------- 7. the unrolled pixel loops under the slot caps
def elementwise_case(dt, G, Pn, Cc, d, fwd, bwd):
    x, dy, mean, rstd, w, b = R.bwd_exact_inputs(G, Pn, Cc, seed=Pn)
    act = R.ACT_LEAKY
    xh, z, dz = R.norm_terms64(x, dy, mean, rstd, w, b, act)
    xg, dyg = x.to(d, dt).view(G * Pn, Cc), dy.to(d, dt).view(G * Pn, Cc)
    mg, rg, wg, bg = (t.to(d).contiguous() for t in (mean, rstd, w, b))
    name = "bf16" if dt == bf else "f32"
    if fwd:
        yw, yv = X.guarded(G * Pn, Cc, dt, d)
        ok("du_norm_act_fwd", code(dt), ptr(xg), Cc, ptr(yv), Cc, ptr(mg), ptr(rg), ptr(wg), ptr(bg), G, Pn, Cc, act)
        X.assert_guard(yw, G * Pn, "y")
        y64 = R.act64(z, act)
        gate(yv.view(G, Pn, Cc), y64, R.y_bound(y64, x.double(), mean.double()[:, None], rstd.double()[:, None], w.double(), b.double(), R.U[dt]),
             f"norm_act y {name}: loops G {G} P {Pn} C {Cc}")
    if bwd:
        bs64, _, _ = R.bwd_stats64(x, dy, mean, rstd, w, b, act)
        k1, k2 = bs64[..., 0] / Pn, bs64[..., 1] / Pn
        dx64 = (w.double() * rstd.double())[:, None] * (dz - k1[:, None] - xh * k2[:, None])
        dxw, dxv = X.guarded(G * Pn, Cc, dt, d)
        bsg = bs64.float().to(d)
        ok("du_norm_act_bwd_dx", code(dt), ptr(xg), Cc, ptr(dyg), Cc, ptr(dxv), Cc, ptr(mg), ptr(rg), ptr(wg), ptr(bg), ptr(bsg), G, Pn, Cc, act,
           float(Pn), 1)
        X.assert_guard(dxw, G * Pn, "dx")
        # bsums handed in as fp32(fp64 sums): one rounding each, inside K
        gate(dxv.view(G, Pn, Cc), dx64, R.dx_bound(dx64, w.double(), rstd.double()[:, None], dz, k1[:, None], k2[:, None], xh, R.U[dt], 0, 0.0, 0.0),
             f"norm_act dx {name}: loops G {G} P {Pn} C {Cc}")


@pytest.mark.parametrize("dt", R.DTS, ids=DT_IDS)
def test_elementwise_tail_loop_only(dt):
    Cc = 4 * R.VEC[dt]
    for G, Pn in ((1, 3), (3, 64 * 3)):
        lf, capf = R.elementwise_loops(G, Pn, Cc, dt)
        lb, capb = R.elementwise_loops(G, Pn, Cc, dt, True)
        assert lf == {1} and 4 not in lb and not capf and not capb, (lf, lb)
        elementwise_case(dt, G, Pn, Cc, dev(), True, True)


def test_elementwise_bwd_all_loops_under_the_cap():
    """fp32 C = 1024 (np = 1), G = 1: the cap of 512 slots binds and a thread walks 7 or 6 pixels: the 4x, 2x and 1x loops in one launch"""
    G, Pn, Cc = 1, 4 * 512 + 2 * 512 + 1, 1024
    loops, cap = R.elementwise_loops(G, Pn, Cc, f32, True)
    assert loops == {4, 2, 1} and cap
    elementwise_case(f32, G, Pn, Cc, dev(), False, True)
    assert R.elementwise_loops(64, 32 * 6 + 1, 512, bf, True) == ({4, 2, 1}, True)       # np = 4, 8 slots per group, 7 or 6 pixels
    elementwise_case(bf, 64, 32 * 6 + 1, 512, dev(), False, True)


def test_elementwise_fwd_all_loops_under_the_cap():
    """fp32 C = 1024 (np = 1), G = 64: the cap of 64 slots per group binds and a thread walks 5 or 4 pixels: the 4x loop and the tail"""
    G, Pn, Cc = 64, 4 * 64 + 1, 1024
    loops, cap = R.elementwise_loops(G, Pn, Cc, f32)
    assert loops == {4, 1} and cap
    elementwise_case(f32, G, Pn, Cc, dev(), True, False)


# ---------------------------------------------------------------------------------------------------- 8. two routes to the same statistics
@pytest.mark.parametrize("draw", ["two-value", "randn"])
@pytest.mark.parametrize("dt,G,Pn,Cc", [(f32, 1, 256, 32), (f32, 1, 130, 1028), (f32, 1, 64, 2048), (bf, 1, 1024, 64), (bf, 3, 66, 24), (f32, 4, 64, 512)],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_two_routes_to_the_same_statistics(dt, G, Pn, Cc, draw):
    """du_chan_stats + du_norm_stats_finalize (the SyncBN path) and du_chan_stats_norm on the same input: on the two-value draw mean,
    rstd and the running statistics agree bit for bit and the mean equals the fp64 mean; on randn each stays within its bound"""
    d = dev()
    if draw == "two-value":
        x, m, s = R.two_value_draw(G, Pn, Cc, seed=Cc)
        R.require_sums_exact(Pn, 49.0)
    else:
        x = R.quant(torch.randn(G, Pn, Cc, generator=torch.Generator().manual_seed(Cc)) * 1.5 + 0.3, dt)
    run = G == 1
    rm0, rv0 = X.integers(Cc, seed=4, lo=-3, hi=3), X.integers(Cc, seed=5, lo=1, hi=16)
    xg = nhwc(x, d, dt)
    ws, n = scratch(dt, G, Pn, Cc, d)
    got = []
    for route in (1, 2):
        sw, sv = fbuf(G * Cc * 2, d)
        mw, mv = fbuf(G * Cc, d)
        rw, rv = fbuf(G * Cc, d)
        rmg, rvg = rm0.to(d).clone(), rv0.to(d).clone()
        rp, vp = (ptr(rmg), ptr(rvg)) if run else (None, None)
        if route == 1:
            ok("du_chan_stats", code(dt), ptr(xg), Cc, ptr(sv), G, Pn, Cc, ptr(ws), n)
            ok("du_norm_stats_finalize", ptr(sv), float(Pn), R.EPS_N, ptr(mv), ptr(rv), G, Cc, rp, vp, 0.1)
        else:
            ok("du_chan_stats_norm", code(dt), ptr(xg), Cc, ptr(sv), G, Pn, Cc, ptr(ws), n, float(Pn), R.EPS_N, ptr(mv), ptr(rv), rp, vp, 0.1)
        for whole, k in ((sw, G * Cc * 2), (mw, G * Cc), (rw, G * Cc)):
            assert_flat_guard(whole, k, what=f"route {route}")
        got.append((sv.clone(), mv.clone(), rv.clone(), rmg, rvg))
    f = R.norm_formulas64(x, torch.zeros_like(x), torch.ones(Cc), torch.zeros(Cc), R.ACT_NONE, R.EPS_N)
    exact = draw == "two-value" and (Pn & (Pn - 1)) == 0
    if draw == "two-value":
        assert all(torch.equal(p, q) for p, q in zip(*got)), "the two routes differ"
        X.assert_exact(got[0][0].view(G, Cc, 2), R.stats64(x), "sums", sentinel=False)
        if exact:
            X.assert_exact(got[0][1].view(G, Cc), f["mean"], "mean")
    unb = Pn / (Pn - 1.0)
    depth = 0 if draw == "two-value" else R.sum_depth(G, Pn, Cc, dt)        # the two-value sums are exact
    absx = x.double().abs().mean(1)
    for sv, mv, rv, rmg, rvg in got:
        gate(mv.view(G, Cc), f["mean"], R.mean_bound(absx, exact, depth), f"stats mean {draw}: {Pn} x {Cc}")
        gate(rv.view(G, Cc), f["rstd"], R.rstd_bound(f["rstd"], f["var"], f["ex2"], f["mean"], R.EPS_N, exact, depth), f"stats rstd {draw}: {Pn} x {Cc}")
        if run:
            gate(rmg, 0.9 * rm0.double() + 0.1 * f["mean"][0], R.run_bound(rm0.double(), f["mean"][0]) + 0.1 * R.mean_bound(absx[0], exact, depth),
                 f"stats run_mean {draw}: {Pn} x {Cc}")
            gate(rvg, 0.9 * rv0.double() + 0.1 * f["var"][0] * unb, R.run_bound(rv0.double(), f["var"][0] * unb) +
                 (0 if exact else 0.1 * unb * R.var_bound(f["ex2"][0], f["mean"][0], depth)), f"stats run_var {draw}: {Pn} x {Cc}")


# ---------------------------------------------------------------------------------------------------- 9. offset statistics
@pytest.mark.parametrize("m", R.OFFSETS, ids=lambda m: f"m{int(m)}")
@pytest.mark.parametrize("dt", R.DTS, ids=DT_IDS)
def test_offset_statistics(dt, m):
    """bf16-held N(+-m, 1) and one constant channel, P = 4096 and 4090, through the fp32 and the bf16 kernels: the one-pass variance
    E[x^2] - mean^2 stays within K U_F32 (E[x^2] + mean^2), K = 4, of the two-pass fp64 variance, rstd and y within the bounds that follow
    from it.  Printed, not gated: the same on data with fp32's whole mantissa, where the sums themselves round (recorded in DESIGN.md)"""
    from dinounet_amd import ops
    d = dev()
    Cc = 32
    w, b = R.affine_for(Cc, seed=1)
    for Pn in (4096, 4090):
        x = R.offset_draw(Pn, Cc, m, seed=int(m) + Pn)
        f, dm, dr, yb = R.offset_bounds(x, w, b, R.EPS_N, R.U[dt], R.sum_depth(1, Pn, Cc, dt))
        assert float(f["var"][0, -1]) == 0.0 and abs(float(f["mean"][0, -1])) >= 3
        xg = nhwc(x, d, dt)
        ws, n = scratch(dt, 1, Pn, Cc, d)
        mw, mv = fbuf(Cc, d)
        rw, rv = fbuf(Cc, d)
        ok("du_chan_stats_norm", code(dt), ptr(xg), Cc, None, 1, Pn, Cc, ptr(ws), n, float(Pn), R.EPS_N, ptr(mv), ptr(rv), None, None, 0.1)
        assert_flat_guard(mw, Cc, what="mean")
        assert_flat_guard(rw, Cc, what="rstd")
        name = "bf16" if dt == bf else "f32"
        gate(mv.view(1, Cc), f["mean"], dm, f"offset mean {name} m {int(m)}: P {Pn}")
        gate(rv.view(1, Cc)[:, :-1], f["rstd"][:, :-1], dr[:, :-1], f"offset rstd {name} m {int(m)}: P {Pn}")
        gate(rv.view(1, Cc)[:, -1:], f["rstd"][:, -1:], dr[:, -1:], f"constant-channel rstd {name} m {int(m)}: P {Pn}")
        y = ops.norm_act(xg, w.to(d), b.to(d), "in", R.ACT_NONE, R.EPS_N)
        gate(y.view(1, Pn, Cc)[..., :-1], f["y"][..., :-1], yb[..., :-1], f"offset y {name} m {int(m)}: P {Pn}")
        gate(y.view(1, Pn, Cc)[..., -1:], f["y"][..., -1:], yb[..., -1:], f"constant-channel y {name} m {int(m)}: P {Pn}")
        if dt == f32:
            xf = R.offset_draw(Pn, Cc, m, seed=int(m) + Pn, full=True)
            ff, _, drf, _ = R.offset_bounds(xf, w, b, R.EPS_N, R.U[dt], 0)
            xfg = nhwc(xf, d, dt)
            ok("du_chan_stats_norm", code(dt), ptr(xfg), Cc, None, 1, Pn, Cc, ptr(ws), n, float(Pn), R.EPS_N, ptr(mv), ptr(rv), None, None, 0.1)
            s_ = ((rv.view(1, Cc).cpu().double() - ff["rstd"]).abs() / drf)[:, :-1].max()
            print(f"[info] rstd on fp32-mantissa data, share of the K = 4 bound, m {int(m)} P {Pn}: {float(s_):.3f}")


# ---------------------------------------------------------------------------------------------------- 10. refusals
@pytest.mark.parametrize("dt", R.DTS, ids=DT_IDS)
def test_refusals(dt):
    """return codes only: nothing is launched, every output buffer keeps the sentinel"""
    d = dev()
    V = R.VEC[dt]
    Cr = V + V // 2                                                   # ragged C % VEC
    x = torch.zeros(8, 4 * V, dtype=dt, device=d)
    st = torch.ones(4 * V, device=d)
    ow, ov = fbuf(8 * V, d)
    yw, yv = X.guarded(8, 4 * V, dt, d)
    ws, n = scratch(dt, 1, 8, 4 * V, d)
    c = code(dt)
    rcs = [call("du_chan_stats", c, ptr(x), 4 * V, ptr(ov), 1, 8, Cr, ptr(ws), n),
           call("du_chan_stats", c, ptr(x), 4 * V + 1, ptr(ov), 1, 8, 2 * V, ptr(ws), n),                    # ragged ldx % VEC
           call("du_chan_dot", c, ptr(x), 4 * V, ptr(x), 4 * V, ptr(ov), 1, 8, Cr, ptr(ws), n),
           call("du_chan_dot", c, ptr(x), 4 * V, ptr(x), 4 * V + 2, ptr(ov), 1, 8, 2 * V, ptr(ws), n),
           call("du_colsum", c, ptr(x), 4 * V, ptr(ov), 8, Cr, ptr(ws), n),
           call("du_colsum", c, ptr(x), 4 * V, ptr(ov), 8, 4 * V, None, 0),                                  # no scratch
           call("du_chan_stats_norm", c, ptr(x), 4 * V, None, 1, 8, 4 * V, ptr(ws), n - 1, 8.0, 1e-5, ptr(ov), ptr(ov[4 * V:]), None, None, 0.1),
           call("du_chan_stats_norm", c, ptr(x), 4 * V, None, 1, 8, Cr, ptr(ws), n, 8.0, 1e-5, ptr(ov), ptr(ov[4 * V:]), None, None, 0.1),
           call("du_norm_act_bwd_stats_grads", c, ptr(x), 4 * V, ptr(x), 4 * V, ptr(st), ptr(st), ptr(st), ptr(st), ptr(ov), ptr(ov), ptr(ov), 1, 8, 4 * V, 0,
                ptr(ws), n - 1),
           call("du_norm_act_fwd", c, ptr(x), 4 * V, ptr(yv), 4 * V, ptr(st), ptr(st), ptr(st), ptr(st), 1, 8, Cr, 0),
           call("du_norm_act_fwd", c, ptr(x), 4 * V + 1, ptr(yv), 4 * V, ptr(st), ptr(st), ptr(st), ptr(st), 1, 8, 4 * V, 0),
           call("du_norm_act_bwd_dx", c, ptr(x), 4 * V, ptr(x), 4 * V, ptr(yv), 4 * V + 1, ptr(st), ptr(st), ptr(st), ptr(st), ptr(st), 1, 8, 4 * V, 0, 8.0, 1),
           call("du_layernorm_fwd", c, c, ptr(x), 4 * V, ptr(st), ptr(st), ptr(yv), 4 * V, None, None, 8, Cr, 1e-6),
           call("du_layernorm_fwd", c, c, ptr(x), 4 * V + 1, ptr(st), ptr(st), ptr(yv), 4 * V, None, None, 8, 2 * V, 1e-6),
           call("du_layernorm_bwd", c, ptr(x), ptr(x), ptr(st), ptr(st), ptr(st), ptr(yv), ptr(ov), 8, Cr, ptr(ws), n, None)]
    torch.cuda.synchronize()
    assert all(rc == -1 for rc in rcs), rcs
    assert untouched(ow) and untouched(yw) and untouched(ws)
