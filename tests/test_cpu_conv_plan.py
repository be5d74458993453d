"""du_conv3x3_plan / du_conv3x3_wgrad_plan (csrc/conv_plan.h, conv_halo.hip) against the dispatch pinned from the commit before them:
tests/golden/conv3x3_dispatch.npz, written by tools/make_golden_conv_dispatch.py -- for ~4 x 10^4 calls what that commit's du_conv3x3_halo /
du_conv3x3_wgrad_halo LAUNCHED (a recorder build: every launcher appends to a list instead of launching) and what its
du_conv3x3_halo_parts / du_conv3x3_wgrad_halo_blocks REPORTED.  Pure host logic: no GPU, fake operand addresses."""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
_spec = importlib.util.spec_from_file_location("make_golden_conv_dispatch", os.path.join(ROOT, "tools", "make_golden_conv_dispatch.py"))
tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tool)


def test_plans_match_pinned_dispatch():
    """Forward: describe's {rc, kernel, variant} is what the old entry point launched for the call with stats_part set exactly when the
    plan's stats_parts > 0, stats_parts the rows that launcher would write, du_conv3x3_halo_parts the same number on dense aligned rows: no
    exception.  Weight gradient: {rc, kernel, variant} what was launched; blocks too, except the rows tool.CORRECTED lists by cause and
    count (the old slab cap was chosen on dense tensors, the kernel on the strides): none of them a network shape."""
    from dinounet_amd import _lib
    g = np.load(tool.OUT)
    rows, envs = g["rows"], [str(e) for e in g["envs"]]
    assert len(rows) >= 40000 and envs == tool.ENVS and [str(c) for c in g["columns"]] == tool.COLUMNS
    assert sum(str(t).startswith("dinounet_") for t in g["tags"]) >= 9
    # the release library has no environment knobs (csrc/common.h): there a row with a knob must plan as its twin without one
    knobs = b"DU_HALO_WGRAD_BLOCKS" in open(_lib.LIB_PATH, "rb").read()
    got = tool.run_by_env(_lib.LIB_PATH, rows, "describe")      # the knobs are read once per process: one child each
    assert all(r is not None for r in got)
    bad, counts = tool.compare(g, got, knobs)
    assert not bad, (len(bad), bad[:10])
    assert counts == [c for _, _, c in tool.CORRECTED], counts


def test_plan_describe_rejects_bad_calls_and_names_the_decoder_layers():
    from dinounet_amd import _lib
    L = _lib.lib()
    d = (C.c_int64 * 4)()
    X, X2, Wp, Y = 0x100000, 0x200000, 0x300000, 0x400000
    fwd = lambda C1, C2, Cout, B, H, W, stats=1, ld=None: (L.du_conv3x3_plan_describe(X, ld or C1, X2 if C2 else None, C2, C1, C1 + C2, Cout, B, H, W, Wp, Y, Cout, stats, d, 4), list(d))[1]
    wg = lambda C1, C2, Cout, B, H, W, ld=None: (L.du_conv3x3_wgrad_plan_describe(X, ld or C1, X2 if C2 else None, C2, C1, C1 + C2, Cout, B, H, W, Y, Cout, d, 4), list(d))[1]
    assert L.du_conv3x3_plan_describe(X, 32, None, 0, 32, 32, 32, 1, 8, 128, Wp, Y, 32, 1, None, 4) == -1
    assert L.du_conv3x3_plan_describe(X, 32, None, 0, 32, 32, 32, 1, 8, 128, Wp, Y, 32, 1, d, 3) == -1
    assert L.du_conv3x3_wgrad_plan_describe(X, 32, None, 0, 32, 32, 32, 1, 8, 128, Y, 32, None, 4) == -1
    assert L.du_conv3x3_wgrad_plan_describe(X, 32, None, 0, 32, 32, 32, 1, 8, 128, Y, 32, d, 3) == -1
    assert L.du_conv3x3_plan_describe(None, 32, None, 0, 32, 32, 32, 1, 8, 128, Wp, Y, 32, 1, d, 4) == 4 and d[0] == -1      # the call's own DU_ERR_BAD_ARG
    # the dinounet_l decoder at batch 8: strip kernel at 512^2 / 256^2 (but 64 + 64: tiles, 64-channel chunks), tiles with 32-channel chunks at 128 outputs
    assert fwd(32, 0, 32, 8, 512, 512) == [0, 1, 11, 8 * 16 * 16] and fwd(32, 32, 32, 8, 512, 512) == [0, 1, 21, 8 * 8 * 16]
    assert fwd(64, 0, 64, 8, 256, 256) == [0, 1, 22, 8 * 16 * 8] and fwd(64, 64, 64, 8, 256, 256) == [0, 2, 642, 8 * 32 * 16]
    assert fwd(128, 0, 128, 8, 128, 128) == [0, 2, 324, 8 * 16 * 8] and fwd(128, 128, 128, 8, 128, 128, stats=0) == [0, 2, 324, 0]
    assert fwd(32, 0, 128, 1, 8, 16) == [-2, 0, 0, 0]           # one chunk at 128 outputs: weights + halo + fp32 tile do not fit the LDS
    assert fwd(256, 0, 256, 8, 64, 64) == [-2, 0, 0, 0]
    # a 32-channel slice of a 512-wide tensor at 1024^2: a strip shape, 1 GiB per image: the tile kernel, and no statistics from this call
    assert fwd(32, 0, 32, 2, 1024, 1024, ld=512) == [0, 2, 321, 0]
    assert wg(32, 0, 32, 8, 512, 512) == [0, 1, 321, 512] and wg(64, 0, 32, 8, 512, 512) == [0, 1, 641, 256] and wg(64, 64, 64, 8, 256, 256) == [0, 1, 642, 256]
    assert wg(128, 0, 128, 8, 128, 128) == [-2, 0, 0, 0]
    # past the rows kernel's 32-bit offsets on the strides passed: the round-3 kernel and ITS workgroup count (the old cap, judged dense, said 256)
    assert wg(64, 0, 32, 8, 512, 1024, ld=512) == [0, 2, 641, 512]
    try:
        L.du_set_option(13, 2)
        assert wg(128, 128, 128, 8, 128, 128) == [0, 1, 324, 128]
        L.du_set_option(13, 0)
        assert wg(64, 0, 64, 8, 256, 256) == [0, 2, 322, 256] and wg(32, 0, 64, 8, 256, 256) == [0, 2, 322, 512]
    finally:
        L.du_set_option(13, 1)
