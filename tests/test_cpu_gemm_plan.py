"""du_gemm_plan (csrc/gemm_plan.h, gemm.hip) against the dispatch pinned from the commit before it: tests/golden/gemm_dispatch.npz, written by
tools/make_golden_gemm_dispatch.py -- for ~10^4 argument sets what that commit's du_gemm LAUNCHED (a recorder build: every launcher
appends to a list instead of launching) and what its du_gemm_route / du_gemm_ws_elems / du_gemm_ks_ws_bytes REPORTED.  Pure host logic:
no GPU, fake operand addresses."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "gemm_dispatch.npz")
OPT_DEFAULTS = {0: -1, 5: 1, 9: 1, 10: 1, 12: 1, 14: 1, 15: 0, 16: 0, 17: 1}
RC, FAMILY = 0, 1            # columns of `executed` = du_gemm_plan_describe's first seven: rc, family, variant, gather, tail_rows, tail_form, tn_splits
SWIGLU, PLAIN_COL = 4, 1


def evaluate(env_index):
    """[du_gemm_plan_describe's nine values + du_gemm_route + du_gemm_ws_elems + du_gemm_ks_ws_bytes] for every fixture row of one environment"""
    from dinounet_amd import _lib
    L = _lib.lib()
    g = np.load(FIXTURE)
    cols, rows, alphas = [str(c) for c in g["columns"]], g["rows"], g["alpha"]
    out = {}
    d = (C.c_int64 * 9)()
    try:
        for i in np.where(rows[:, cols.index("env")] == env_index)[0]:
            a = _lib.GemmArgs()
            for c, v in zip(cols, rows[i]):
                if c.startswith("opt"):
                    L.du_set_option(int(c[3:]), int(v))
                elif c.startswith("geom."):
                    setattr(a.geom, c[5:], int(v))
                elif c != "env":
                    setattr(a, c, int(v))
            a.alpha, a.rope_qscale = float(alphas[i]), 1.0
            assert L.du_gemm_plan_describe(C.byref(a), d, 9) == 9
            out[int(i)] = list(d) + [int(L.du_gemm_route(C.byref(a))), int(L.du_gemm_ws_elems(C.byref(a))), int(L.du_gemm_ks_ws_bytes(C.byref(a)))]
    finally:
        for k, v in OPT_DEFAULTS.items():
            L.du_set_option(k, v)
    return out


# The rows on which the old du_gemm_route disagreed with what the old du_gemm launched, by cause (first match), with the number of fixture
# rows of each: du_gemm_route now reports the launched family on all of them.  A regenerated fixture with a disagreement of another kind, or
# more of one kind, fails here.
def _misaligned(r):
    return bool(r["bias"] & 15 or r["gamma"] & 15 or r["residual"] & 15 or (r["residual"] and r["ldr"] % 4) or r["c_batch_stride"] % 4)


CORRECTED = [
    # DU_GEMM_GENERIC (debug builds) was not consulted by the fused-store / SwiGLU special cases, yet the route said 0: 3 / 4 / 6 ran
    ("DU_GEMM_GENERIC set, fused store or SwiGLU: a multi-phase kernel ran, 0 reported", lambda r: r["env"] == 1, 100),
    # the gate epilogue forces the 256 x 128 kernel where the heuristic declines (256 x 128 x 256: 4 ran, 2 reported)
    ("SwiGLU below the tile heuristic's threshold: 256 x 128 tiles (4) ran, 2 / 1 reported", lambda r: r["act"] == SWIGLU, 274),
    # bias / gamma / residual pointer off 16 bytes, ldr or c_batch_stride off 4 elements: the generic kernel (0) ran, 1 .. 8 reported
    ("misaligned epilogue pointer or stride: the generic kernel (0) ran, a bf16 family reported", _misaligned, 211),
    # no ws passed: the ragged rows stay in the tile grid and the tile choice is made for the whole M (8232 x 3072 x 1024: 3 ran, 6 reported)
    ("ragged rows without ws: the choice for the whole M ran, the choice for the head was reported", lambda r: r["ws"] == 0 and 0 < r["M"] % 256 <= 64, 74),
]
# One deliberate change of what runs: DropPath's scale on the contraction rows (row_scale with a_mode PLAIN_COL) exists in the bf16 tile engine
# only.  With c_batch_stride off the 4-element rule the old du_gemm checked the mirror (1), then ran the generic kernel, which applied the scale
# to the OUTPUT rows.  The check now reads the plan's family: DU_ERR_UNSUPPORTED.
KSCALE_ON_GENERIC = 21


def test_plan_matches_pinned_dispatch():
    from dinounet_amd import _lib
    g = np.load(FIXTURE)
    cols = [str(c) for c in g["columns"]]
    rows, names, executed, reported, alphas, envs = g["rows"], g["names"], g["executed"], g["reported"], g["alpha"], [str(e) for e in g["envs"]]
    env = rows[:, cols.index("env")]
    assert len(rows) >= 3000 and len(envs) == 7
    # the release library has no environment knobs (csrc/common.h): there a row with a knob must plan as its twin without one
    knobs = b"DU_GEMM_NO_RAGGED_SPLIT" in open(_lib.LIB_PATH, "rb").read()
    twin = {tuple(rows[i][:-1]) + (float(alphas[i]),): i for i in np.where(env == 0)[0]}
    got = evaluate(0)
    for e in range(1, len(envs)):       # the knobs are read once per process: one child each
        k, v = envs[e].split("=")
        p = subprocess.run([sys.executable, os.path.abspath(__file__), str(e)], capture_output=True, text=True, env={**os.environ, k: v})
        assert p.returncode == 0, p.stderr
        got.update({int(i): r for i, r in json.loads(p.stdout.strip().splitlines()[-1]).items()})
    assert sorted(got) == list(range(len(rows)))
    refused_kscale = 0
    for i in range(len(rows)):
        j = i if knobs or env[i] == 0 else twin[tuple(rows[i][:-1]) + (float(alphas[i]),)]
        plan, route, ws, ks = got[i][:7], got[i][9], got[i][10], got[i][11]
        r = dict(zip(cols, (int(v) for v in rows[i])))
        if executed[j][RC] == 0 and plan[RC] == -2 and executed[j][FAMILY] == 0 and r["row_scale"] and r["a_mode"] == PLAIN_COL and _misaligned(r):
            refused_kscale += int(env[i] == 0)
        elif executed[j][RC] == 0:
            assert plan == list(executed[j]), (names[i], plan, list(executed[j]))      # family, variant, gather, tail rows and form, splits: what ran
        else:
            assert plan[RC] == executed[j][RC], (names[i], plan, list(executed[j]))      # refused with the same code
        assert route == plan[FAMILY], (names[i], route, plan)
        assert got[i][7] == ws == reported[j][1] and got[i][8] == ks == reported[j][2], (names[i], got[i], list(reported[j]))
    assert refused_kscale == KSCALE_ON_GENERIC
    # where the old route was wrong: every such row has one of the causes above, and no more rows than were counted when the fixture was written
    counts = [0] * len(CORRECTED)
    for i in np.where((executed[:, RC] == 0) & (reported[:, 0] != executed[:, FAMILY]))[0]:
        r = dict(zip(cols, (int(v) for v in rows[i])))
        hit = [n for n, (_, pred, _) in enumerate(CORRECTED) if pred(r)]
        assert hit, f"du_gemm_route disagreed with du_gemm for an unlisted reason: {names[i]} reported {reported[i][0]} ran {executed[i][FAMILY]}"
        counts[hit[0]] += 1
    assert counts == [c for _, _, c in CORRECTED], counts


def test_plan_describe_rejects_bad_calls_and_names_the_vit_products():
    """the ViT's qkv product as ops.gemm_raw passes it: persistent kernel, 40 rows riding in its launch; without ws the whole M on 256 x 256 tiles"""
    from dinounet_amd import _lib
    L = _lib.lib()
    a = _lib.GemmArgs()
    a.dtype = a.out_dtype = _lib.DU_BF16
    a.M, a.N, a.K, a.lda, a.ldb, a.ldc, a.batch, a.split_k, a.alpha = 8232, 3072, 1024, 1024, 1024, 3072, 1, 1, 1.0
    a.A, a.B, a.C = 0x100000, 0x200000, 0x300000
    d = (C.c_int64 * 9)()
    assert L.du_gemm_plan_describe(None, d, 9) == -1 and L.du_gemm_plan_describe(C.byref(a), d, 8) == -1 and L.du_gemm_plan_describe(C.byref(a), None, 9) == -1
    assert L.du_gemm_plan_describe(C.byref(a), d, 9) == 9
    assert list(d)[:7] == [0, 3, 1, 0, 0, 0, 0] and d[7] > 0
    a.ws, a.ws_elems = 0x400000, d[7]
    assert L.du_gemm_plan_describe(C.byref(a), d, 9) == 9
    assert list(d)[:7] == [0, 6, 4, 0, 40, 1, 0]
    a.M = 0
    assert L.du_gemm_plan_describe(C.byref(a), d, 9) == 9 and d[0] == -1


def test_plan_of_the_k_split_pair_shapes_as_ops_lends_scratch():
    """du_set_option(16, 1), the three proj / fc2 shapes of the K-split pair tests, scratch lent in ops.gemm_raw's order: ws is asked for
    before ks_ws is passed.  4136 x 1024 x 1024: without ks_ws the pair kernel is not legal for the 4096-row head and its 16 x 8 narrow
    tiles are below the heuristic's 192, so no ragged rows are named and no ws is lent; du_gemm then keeps all 4136 rows in one grid --
    17 x 4 tiles are no whole pairs -- on the 128 x 128 kernel (2).  The old du_gemm_route, asked once ks_ws was there, split the rows
    regardless of ws and said 8.  With ws the head runs as pairs and the 40 rows ride in its launch."""
    from dinounet_amd import _lib
    L = _lib.lib()
    d = (C.c_int64 * 9)()
    want = {(4136, 1024, 1024): [0, 2, 0, 0, 0, 0, 0], (8232, 1024, 4096): [0, 8, 5, 0, 40, 1, 0], (4096, 2048, 1024): [0, 8, 5, 0, 0, 0, 0]}
    L.du_set_option(16, 1)
    try:
        for (M, N, K), plan in want.items():
            a = _lib.GemmArgs()
            a.dtype, a.out_dtype = _lib.DU_BF16, _lib.DU_F32
            a.M, a.N, a.K, a.lda, a.ldb, a.ldc, a.ldr, a.batch, a.split_k, a.alpha = M, N, K, K, K, N, N, 1, 1, 1.0
            a.A, a.B, a.C, a.bias, a.gamma, a.residual = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000
            ws = int(L.du_gemm_ws_elems(C.byref(a)))
            if ws > 0:
                a.ws, a.ws_elems = 0x700000, ws
            ks = int(L.du_gemm_ks_ws_bytes(C.byref(a)))
            assert ks > 0
            a.ks_ws, a.ks_ws_bytes = 0x10000000, ks
            assert L.du_gemm_plan_describe(C.byref(a), d, 9) == 9
            assert list(d)[:7] == plan and L.du_gemm_route(C.byref(a)) == plan[FAMILY], (M, N, K, list(d))
            if (M, N, K) == (4136, 1024, 1024):
                assert ws == 0 and d[7] > 0
                a.ws, a.ws_elems = 0x700000, d[7]
                assert L.du_gemm_plan_describe(C.byref(a), d, 9) == 9
                assert list(d)[:7] == [0, 8, 5, 0, 40, 1, 0], list(d)
    finally:
        L.du_set_option(16, OPT_DEFAULTS[16])


if __name__ == "__main__":
    print(json.dumps(evaluate(int(sys.argv[1]))))
