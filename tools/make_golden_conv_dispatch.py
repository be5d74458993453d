"""Writes tests/golden/conv3x3_dispatch.npz: the dispatch of du_conv3x3_halo and du_conv3x3_wgrad_halo over a sweep of calls, pinned from
the commit BEFORE du_conv3x3_plan / du_conv3x3_wgrad_plan (csrc/conv_plan.h).

Two tables over the same rows (tests/test_cpu_conv_plan.py holds the two *_plan_describe entries to both):
  reported -- what that library's du_conv3x3_halo_parts / du_conv3x3_wgrad_halo_blocks answered (they see channel counts and the image only);
  executed -- what its entry points launched: from a recorder build of the same commit, in which each of the four launchers (strip_launch,
              launch, launch_wgrad_rows, launch_wgrad) appends (launcher 1..4, its two template parameters, grid, rows of partial statistics
              or slabs it would write, statistics flag, bias flag) to a list and returns DU_OK in place of hipFuncSetAttribute / the launch;
              the declines in front of the launch are kept.  The list is read back through `int du_rec_read(int* out)` (7 ints per launch,
              returns the count and clears it).  A forward row is run twice: executed[:, 0] without stats_part, executed[:, 1] with one.
Both libraries are builds with -DDU_DEBUG_KNOBS (the environment knobs are read once per process: one child process per knob).  Nothing is
dereferenced: the operands are fake addresses.

  python tools/make_golden_conv_dispatch.py --reported libparent.so --executed librecorder.so [--out tests/golden/conv3x3_dispatch.npz]
  python tools/make_golden_conv_dispatch.py --check libnew.so      # a -DDU_DEBUG_KNOBS build of the current tree against the fixture, environment rows included
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "conv3x3_dispatch.npz")
# a row: op 0 = du_conv3x3_halo (y, ldy; stats = statistics wanted), 1 = du_conv3x3_wgrad_halo (y / ldy are dy / lddy)
COLUMNS = ["op", "x", "ldx", "x2", "ldx2", "C1", "Cin", "Cout", "B", "H", "W", "w", "y", "ldy", "stats", "bias", "opt13", "env", "tag"]
TAGS = []                # what a row is there for (the fixture's `tags`; column "tag" indexes it): a row's name is made of it and of the row
ENVS = ["", "DU_CONV_STRIP=0", "DU_HALO_CK32=1", "DU_HALO_WGRAD_BLOCKS=64"]
EXEC = ["rc", "kernel", "variant", "rows", "grid", "stats", "bias"]      # rows: partial-statistics rows (forward), slabs (weight gradient)
RC, KERNEL, VARIANT, ROWS = 0, 1, 2, 3
PX, PX2, PW, PY, PSTATS, PBIAS, PPART, PDW = (0x10000000 * (i + 1) for i in range(8))      # fake addresses
CH = [8, 16, 24, 32, 48, 64, 96, 128, 192, 256, 384]
BS, HS, WS = [1, 2, 8], [8, 12, 16, 40, 128, 256, 512, 1024], [16, 32, 48, 128, 384, 512, 1024]


def row(name, op, C1, C2, Cout, B, H, W, ld=None, ld2=None, ldy=None, stats=0, bias=0, opt13=1, env=0, **ptr):
    Cin = C1 + C2
    r = dict(op=op, x=PX, ldx=C1 if ld is None else ld, x2=PX2 if C2 else 0, ldx2=(C2 if ld2 is None else ld2) if C2 else 0, C1=C1, Cin=Cin,
             Cout=Cout, B=B, H=H, W=W, w=PW, y=PY, ldy=Cout if ldy is None else ldy, stats=stats, bias=bias, opt13=opt13, env=env)
    r.update(ptr)
    if name not in TAGS:
        TAGS.append(name)
    r["tag"] = TAGS.index(name)
    return r


def row_name(r, tags=TAGS):
    C1, C2, Cout = r["C1"], r["Cin"] - r["C1"], r["Cout"]
    t = f" ld{r['ldx']}/{r['ldx2']}/{r['ldy']}" if (r["ldx"], r["ldx2"], r["ldy"]) != (C1, C2, Cout) else ""
    t += "".join(f" {k}+{v - d}" for k, v, d in (("x", r["x"], PX), ("x2", r["x2"], PX2 if C2 else 0), ("w", r["w"], PW), ("y", r["y"], PY)) if v != d)
    return (f"{tags[r['tag']]} {'wgrad' if r['op'] else 'fwd'} {C1}+{C2}->{Cout} {r['B']}x{r['H']}x{r['W']}{t} s{r['stats']} b{r['bias']}"
            + (f" o13={r['opt13']}" if r["op"] else "") + (f" [{ENVS[r['env']]}]" if r["env"] else ""))


def both(name, *a, **kw):
    """the forward call with and without statistics / bias, the weight gradient under the three values of option 13"""
    return [row(name, 0, *a, stats=s, bias=b, **kw) for s, b in ((0, 0), (1, 1))] + [row(name, 1, *a, opt13=o, **kw) for o in (0, 1, 2)]


# channel forms each kernel instantiation is reached by, and a few neither serves: (C1, C2, Cout)
FORMS = [(32, 0, 32), (32, 0, 64), (64, 0, 32), (64, 0, 64), (32, 32, 32), (32, 32, 64), (64, 64, 64), (64, 64, 32), (96, 0, 32), (64, 32, 64),
         (128, 0, 128), (128, 128, 128), (64, 0, 128), (32, 0, 128), (256, 0, 64), (128, 0, 32), (192, 192, 64), (256, 0, 256), (48, 0, 32)]


def stride_variants(C1, C2, Cout):
    """dense, +8, a slice of a 512-wide tensor, +4 (misaligned): for every tensor alone and for all of them"""
    v = [dict(ld=C1 + 8), dict(ldy=Cout + 8), dict(ld=C1 + 8, ld2=C2 + 8, ldy=Cout + 8), dict(ld=512), dict(ldy=512), dict(ld=512, ld2=512, ldy=512),
         dict(ld=C1 + 4), dict(ldy=Cout + 4)]
    return v + ([dict(ld2=C2 + 8), dict(ld2=512), dict(ld2=C2 + 4)] if C2 else [])


def network_rows(env=0):
    """the decoder's 3 x 3 convolutions (features 32 / 64 / 128 / 256 at 512^2 .. 64^2: the same for dinounet_s / b / l) at batch 8 and 16:
    forward, weight gradient, and the data gradients -- the same kernel on dY with the flipped weight, for a concat layer one call per
    source on the row slices wf[:C1] / wf[C1:] (contiguous rows: a plain Cout -> C1 convolution)"""
    rows = []
    for model in ("dinounet_s", "dinounet_b", "dinounet_l"):
        for B in (8, 16):
            for S, Cf in ((512, 32), (256, 64), (128, 128), (64, 256)):
                rows += both(f"{model} decoder", Cf, 0, Cf, B, S, S, env=env)
                rows += both(f"{model} decoder concat", Cf, Cf, Cf, B, S, S, env=env)
                rows += [row(f"{model} decoder dgrad", 0, Cf, 0, Cf, B, S, S, env=env), row(f"{model} decoder dgrad wf[:C1] / wf[C1:]", 0, Cf, 0, Cf, B, S, S, w=PW + 9 * Cf * Cf * 2, env=env)]
    return rows


def all_rows():
    rows = []
    # every channel triple at three images: strip-sized, a production stage, tiles only
    for C1 in CH:
        for C2 in [0] + CH:
            for Cout in CH:
                rows += both("ch", C1, C2, Cout, 8, 256, 256)
                rows += both("ch", C1, C2, Cout, 1, 8, 128)
                rows += both("ch", C1, C2, Cout, 2, 16, 48)
    # every image at the channel forms
    for C1, C2, Cout in FORMS:
        for B in BS:
            for H in HS:
                for W in WS:
                    rows += both("img", C1, C2, Cout, B, H, W)
    # strides and misaligned pointers
    for C1, C2, Cout in FORMS[:14]:
        for B, H, W in [(8, 256, 256), (8, 512, 512), (2, 1024, 1024), (8, 1024, 1024), (8, 512, 1024), (1, 8, 128), (2, 16, 48)]:
            for sv in stride_variants(C1, C2, Cout):
                rows += both("ld", C1, C2, Cout, B, H, W, **sv)
            for k, base in (("x", PX), ("w", PW), ("y", PY)) + ((("x2", PX2),) if C2 else ()):
                rows += both("ptr", C1, C2, Cout, B, H, W, **{k: base + 8})
    rows += both("null", 32, 0, 32, 1, 8, 128, x=0) + both("null", 32, 0, 32, 1, 8, 128, y=0) + [row("null", 0, 32, 0, 32, 1, 8, 128, w=0)]
    rows += both("B0", 32, 0, 32, 0, 8, 128) + both("H0", 32, 0, 32, 1, 0, 128)
    # tests/test_cpu_oracle_and_boundary.py::test_conv3x3_kernel_choice_host_logic_without_gpu: a 32-channel slice of a 512-wide tensor, 1 GiB per image
    rows += both("1GiB", 32, 0, 32, 2, 1024, 1024, ld=512)
    rows += network_rows()
    for e in range(1, len(ENVS)):
        for C1, C2, Cout in FORMS:
            for B, H, W in [(8, 256, 256), (8, 512, 512), (1, 8, 128), (2, 16, 48), (2, 40, 384)]:
                rows += both("img", C1, C2, Cout, B, H, W, env=e)
            if (C1, C2, Cout) in FORMS[:14]:
                rows += both("ld", C1, C2, Cout, 8, 512, 1024, ld=512, ld2=512, ldy=512, env=e)
        rows += network_rows(env=e)
    names = [row_name(r) for r in rows]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1][:5]
    return rows


# ------------------------------------------------------------------------------------------------ running a table through a library
def _proto(L):
    P, I, Q = C.c_void_p, C.c_int, C.c_int64
    shape = [P, Q, P, Q, I, I, I, I, I, I]
    L.du_conv3x3_halo.argtypes = shape + [P, P, P, Q, P, P]
    L.du_conv3x3_wgrad_halo.argtypes = shape + [P, Q, P, P, I, P]
    if hasattr(L, "du_conv3x3_plan_describe"):
        L.du_conv3x3_plan_describe.argtypes = shape + [P, P, Q, I, P, I]
        L.du_conv3x3_wgrad_plan_describe.argtypes = shape + [P, Q, P, I]


def summarise(rc, recs):
    """the launch list of one call of the recorder library -> the EXEC columns"""
    if rc != 0:
        assert not recs, (rc, recs)
        return [rc, 0, 0, 0, 0, 0, 0]
    assert len(recs) == 1, recs
    lid, p1, p2, grid, rows, stats, bias = recs[0]
    return [0, {1: 1, 2: 2, 3: 1, 4: 2}[lid], p1 * 10 + p2, rows, grid, stats, bias]


def run_rows(path, table, mode):
    """mode 'reported': [parts or blocks]; 'executed': the EXEC columns twice (forward: without / with stats_part) from the recorder library;
    'describe': the plan's four values + the dense reader (du_conv3x3_halo_parts / du_conv3x3_wgrad_halo_blocks)"""
    L = C.CDLL(path)
    _proto(L)
    out, buf, d = [], (C.c_int * (16 * 7))(), (C.c_int64 * 8)()
    for vals in table:
        r = dict(zip(COLUMNS, (int(v) for v in vals)))
        shape = (r["x"] or None, r["ldx"], r["x2"] or None, r["ldx2"], r["C1"], r["Cin"], r["Cout"], r["B"], r["H"], r["W"])
        dense = (r["C1"], r["Cin"], r["Cout"], r["B"], r["H"], r["W"])
        L.du_set_option(13, r["opt13"])
        reader = L.du_conv3x3_wgrad_halo_blocks(*dense) if r["op"] else L.du_conv3x3_halo_parts(*dense)
        if mode == "reported":
            out.append([reader])
        elif mode == "executed":
            res = []
            for st in (0, 1):
                if r["op"]:
                    rc = L.du_conv3x3_wgrad_halo(*shape, r["y"] or None, r["ldy"], PPART, PDW, r["bias"], None)
                else:
                    rc = L.du_conv3x3_halo(*shape, r["w"] or None, PBIAS if r["bias"] else None, r["y"] or None, r["ldy"], PSTATS if st else None, None)
                n = L.du_rec_read(buf)
                res.append(summarise(rc, [tuple(buf[7 * i:7 * i + 7]) for i in range(n)]))
            out.append(res)
        else:
            if r["op"]:
                n = L.du_conv3x3_wgrad_plan_describe(*shape, r["y"] or None, r["ldy"], d, 8)
            else:
                n = L.du_conv3x3_plan_describe(*shape, r["w"] or None, r["y"] or None, r["ldy"], r["stats"], d, 8)
            assert n == 4, n
            out.append(list(d[:4]) + [reader])
        L.du_set_option(13, 1)
    return out


def run_by_env(path, table, mode, envs=None):
    """every environment knob in a process of its own (the library reads them once) -> one result per row, in row order"""
    res = [None] * len(table)
    envcol = COLUMNS.index("env")
    for e, spec in enumerate(ENVS):
        idx = [i for i in range(len(table)) if table[i][envcol] == e]
        if not idx or (envs is not None and e not in envs):
            continue
        env = dict(os.environ)
        if spec:
            k, v = spec.split("=")
            env[k] = v
        req = json.dumps({"path": path, "mode": mode, "table": [list(map(int, table[i])) for i in idx]})
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], input=req, capture_output=True, text=True, env=env)
        if p.returncode != 0:
            raise RuntimeError(p.stderr)
        for i, g in zip(idx, json.loads(p.stdout.strip().splitlines()[-1])):
            res[i] = g
    return res


# ------------------------------------------------------------------------------------------------ the fixture against a library's plans
def dense_aligned(r):
    return (r["ldx"], r["ldx2"], r["ldy"]) == (r["C1"], r["Cin"] - r["C1"], r["Cout"]) and not ((r["x"] | r["x2"] | r["w"] | r["y"]) & 15) and r["x"] and r["y"] and r["w"]


# Weight-gradient rows whose slab count the old code keyed on another kernel than the one it ran: du_conv3x3_wgrad_halo_blocks judged "small
# enough for the rows kernel's 32-bit offsets" on dense tensors (one tensor of Cin channels), du_conv3x3_wgrad_halo on the strides it was
# given.  The plan judges once, on the strides, and keys the cap on the kernel it names.  By cause, with the number of fixture rows
# (environment 0) of each: another kind of disagreement, or more rows of one kind, fails.
def _dense_small(r):
    pix = r["B"] * r["H"] * r["W"]
    return pix * max(r["Cin"], r["C1"]) * 2 < 0x7fffffff and pix * r["Cout"] * 2 < 0x7fffffff


CORRECTED = [
    ("strides past the offset limit, dense tensors within it: the round-3 kernel ran with the rows kernel's workgroup cap",
     lambda r, ex: ex[KERNEL] == 2 and r["opt13"] != 0 and _dense_small(r), 48),
]


def compare(g, got, knobs=True):
    """got[i] = run_rows(..., 'describe') of row i -> (list of failures, CORRECTED counts).  knobs False: a release library, which has no
    environment knobs -- a row with one must plan as its twin without."""
    cols = [str(c) for c in g["columns"]]
    rows, executed, reported, tags = g["rows"], g["executed"], g["reported"], [str(t) for t in g["tags"]]
    envcol = cols.index("env")
    twin = {tuple(rows[i][:envcol]): i for i in range(len(rows)) if rows[i][envcol] == 0}
    bad, counts = [], [0] * len(CORRECTED)
    for i in range(len(rows)):
        if got[i] is None:
            continue
        r = dict(zip(cols, (int(v) for v in rows[i])))
        name = row_name(r, tags)
        j = i if knobs or r["env"] == 0 else twin.get(tuple(rows[i][:envcol]))
        if j is None:
            continue
        plan, reader = [int(v) for v in got[i][:4]], int(got[i][4])
        named = name.startswith("dinounet_")
        if r["op"] == 0:
            ex = [int(v) for v in executed[j][1 if plan[ROWS] > 0 else 0]]      # the call with stats_part set exactly when the plan serves statistics
            if plan[:4] != ex[:4] or (plan[ROWS] > 0) != bool(ex[5]) or (plan[ROWS] > 0 and not r["stats"]):
                bad.append(f"{name}: plan {plan} executed {ex}")
            if dense_aligned(r) and r["stats"] and reader != plan[ROWS]:
                bad.append(f"{name}: du_conv3x3_halo_parts {reader} plan {plan}")
            if dense_aligned(r) and r["stats"] and plan[ROWS] > 0 and int(reported[j][0]) != plan[ROWS]:
                bad.append(f"{name}: the old du_conv3x3_halo_parts said {int(reported[j][0])}, plan {plan}")
        else:
            ex = [int(v) for v in executed[j][0]]
            if plan[:3] != ex[:3]:
                bad.append(f"{name}: plan {plan} executed {ex}")
            elif plan[ROWS] != ex[ROWS]:
                hit = [n for n, (_, pred, _) in enumerate(CORRECTED) if pred(r, ex)]
                if not hit or named:
                    bad.append(f"{name}: blocks {plan[ROWS]}, executed {ex[ROWS]}: not a listed correction")
                elif r["env"] == 0:
                    counts[hit[0]] += 1
            if dense_aligned(r) and reader != plan[ROWS]:
                bad.append(f"{name}: du_conv3x3_wgrad_halo_blocks {reader} plan {plan}")
    return bad, counts


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
        print(json.dumps(run_rows(req["path"], req["table"], req["mode"])))
        return
    if a.check:
        g = np.load(a.out)
        bad, counts = compare(g, run_by_env(os.path.abspath(a.check), g["rows"], "describe"))
        print(len(g["rows"]), "rows;", len(bad), "differ; corrected", counts, "expected", [c for _, _, c in CORRECTED])
        for b in bad[:20]:
            print("   ", b)
        sys.exit(1 if bad or counts != [c for _, _, c in CORRECTED] else 0)
    rows = all_rows()
    table = np.array([[r[c] for c in COLUMNS] for r in rows], dtype=np.int64)
    reported = np.array(run_by_env(os.path.abspath(a.reported), table, "reported"), dtype=np.int32)
    executed = np.array(run_by_env(os.path.abspath(a.executed), table, "executed"), dtype=np.int32)
    np.savez_compressed(a.out, columns=np.array(COLUMNS), exec_columns=np.array(EXEC), envs=np.array(ENVS), tags=np.array(TAGS),
                        rows=table.astype(np.int32), reported=reported, executed=executed)
    fwd = table[:, 0] == 0
    print(f"{len(rows)} rows -> {a.out} ({os.path.getsize(a.out)} bytes); forward: refused {int((executed[fwd, 0, 0] != 0).sum())}, "
          f"variants {sorted(set(executed[fwd, 0, 2].tolist()))}, refused only with stats_part {int(((executed[fwd, 0, 0] == 0) & (executed[fwd, 1, 0] != 0)).sum())}; "
          f"weight gradient: refused {int((executed[~fwd, 0, 0] != 0).sum())}, (kernel, variant) {sorted(set(map(tuple, executed[~fwd, 0, 1:3].tolist())))}")


if __name__ == "__main__":
    main()
