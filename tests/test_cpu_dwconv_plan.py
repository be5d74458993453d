"""du_dwconv_plan (csrc/dwconv_plan.h, dwconv.hip) against the dispatch pinned from the commit before it: tests/golden/dwconv_dispatch.npz,
written by tools/make_golden_dwconv_dispatch.py -- what that commit's du_dwconv_band_ok, du_dwconv_band_ws_elems and
du_dwconv_wgrad_ws_elems answered over ~10^5 shapes, where its Python caller then forked on them.  Pure host logic: no GPU, fake operand
addresses."""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
_spec = importlib.util.spec_from_file_location("make_golden_dwconv_dispatch", os.path.join(ROOT, "tools", "make_golden_dwconv_dispatch.py"))
tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tool)

F32, BF16 = 0, 1
NONE, GELU = 0, 1
ROW, ROW4, BAND = 1, 2, 3                     # out[1]
BAD_ARG, UNSUPPORTED = -1, -2


def describe(L, *call):
    d = (C.c_int64 * 7)()
    assert L.du_dwconv3x3_plan_describe(*call, d, 7) == 7
    return list(d)


def test_plan_matches_pinned_dispatch():
    """Band family exactly when the old query said ok and (pyramid or no activation) and, on the NHWC strides the sweep adds, ld % 8 == 0
    and bs % 8 == 0; du_dwconv3x3_bwd_ws_elems the old band or row figure accordingly: no exception."""
    from dinounet_amd import _lib
    L = _lib.lib()
    g = np.load(tool.OUT)
    for name, axis in (("opt19", tool.OPT19), ("dtypes", tool.DTYPES), ("pyramid", tool.PYRAMID), ("bs", tool.BS), ("hw", tool.HW), ("ch", tool.CH)):
        assert g[name].tolist() == axis, name
    ok, band_ws, row_ws = g["band_ok"], g["band_ws"], g["row_ws"]
    assert ok.size >= 90000 and ok.shape == tuple(len(a) for a in tool.AXES)
    assert 0 < int(ok.sum()) < ok.size and int((row_ws > 0).sum()) > ok.size // 2
    bad, nband = [], 0
    d = (C.c_int64 * 7)()
    try:
        for idx, opt, dt, pyr, B, H, W, Cc in tool.sweep():
            L.du_set_option(tool.KEY, opt)
            pix = 21 * (H * W // 4) if pyr else H * W
            for ld in ((Cc,) if pyr else (Cc, Cc + 4, Cc + 8)):
                bs = pix * ld
                for act in (NONE, GELU):
                    call = (dt, ld, bs, B, H, W, Cc, pyr, act)
                    assert L.du_dwconv3x3_plan_describe(*call, d, 7) == 7
                    band = bool(ok[idx]) and (pyr == 1 or act == NONE) and ld % 8 == 0 and bs % 8 == 0
                    want = int(band_ws[idx] if band else row_ws[idx])
                    nband += band
                    if (d[1] == BAND) != band or int(L.du_dwconv3x3_bwd_ws_elems(*call)) != want or d[6] != want:
                        bad.append((opt, *call, list(d), band, want))
    finally:
        L.du_set_option(tool.KEY, 1)
    assert not bad, (len(bad), bad[:10])
    assert nband > 10000


def test_plan_names_the_kernels_and_rejects_bad_calls():
    from dinounet_amd import _lib
    L = _lib.lib()
    d = (C.c_int64 * 7)()
    tok = lambda dt, B, H, W, Cc, act=GELU: describe(L, dt, Cc, 21 * (H * W // 4) * Cc, B, H, W, Cc, 1, act)
    img = lambda dt, B, H, W, Cc, act=NONE, ld=None: describe(L, dt, ld or Cc, H * W * (ld or Cc), B, H, W, Cc, 0, act)
    call = (BF16, 256, 21 * 256 * 256, 8, 32, 32, 256, 1, GELU)
    assert L.du_dwconv3x3_plan_describe(*call, None, 7) == BAD_ARG
    assert L.du_dwconv3x3_plan_describe(*call, d, 6) == BAD_ARG
    # ConvFFN of dinounet_l at 512^2, batch 8: bands of 6 rows, GELU's derivative on load, 118 partial rows
    assert describe(L, *call) == [0, BAND, 6, 2, 4, 118, 118 * 10 * 256]
    assert tok(BF16, 8, 32, 32, 256, NONE)[:5] == [0, BAND, 6, 0, 4]
    # the decoder's depthwise convolutions: NHWC, no activation -> band; with an activation the band family declines
    assert img(BF16, 2, 12, 20, 32)[:2] == [0, BAND] and img(BF16, 2, 12, 20, 32, GELU)[:5] == [0, ROW, 0, 1, 1]
    try:
        L.du_set_option(tool.KEY, 0)
        # the row family's own fork: 4 pixels per thread for the bf16 pyramid with W % 8 == 0, and nowhere else
        assert tok(BF16, 8, 32, 32, 256)[:5] == [0, ROW4, 0, 1, 3] and tok(BF16, 3, 8, 8, 64)[:5] == [0, ROW4, 0, 1, 3]
        assert tok(BF16, 2, 8, 20, 64)[:5] == [0, ROW, 0, 1, 2] and tok(BF16, 2, 8, 12, 64)[:5] == [0, ROW, 0, 1, 2]
        assert tok(F32, 3, 8, 8, 64)[:5] == [0, ROW, 0, 1, 2] and tok(F32, 3, 8, 8, 64, NONE)[:5] == [0, ROW, 0, 0, 2]
        assert img(BF16, 2, 16, 16, 64)[:5] == [0, ROW, 0, 0, 1] and img(F32, 2, 9, 7, 4)[:5] == [0, ROW, 0, 0, 1]
        # 8 x 21 x 256 pixels in strips of 84: 512 workgroups
        assert tok(BF16, 8, 32, 32, 256)[5:] == [512, 512 * 10 * 256]
    finally:
        L.du_set_option(tool.KEY, 1)
    # a call's own error is out[0]
    assert tok(BF16, 3, 8, 8, 60)[0] == BAD_ARG and tok(F32, 3, 8, 7, 64)[0] == BAD_ARG and tok(BF16, 0, 8, 8, 64)[0] == BAD_ARG
    assert describe(L, 7, 64, 64 * 64, 1, 8, 8, 64, 0, NONE)[0] == BAD_ARG                                 # no such dtype
    assert describe(L, BF16, 64, 21 * 16 * 64 + 8, 3, 8, 8, 64, 1, GELU)[0] == BAD_ARG                      # a pyramid is contiguous
    assert img(BF16, 2, 12, 20, 32, ld=36)[:2] == [BAD_ARG, ROW] and img(F32, 2, 12, 20, 32, ld=36)[:2] == [0, ROW]
    # band-shaped but strided, with an activation: the row family's separate pass wants dense tensors
    assert img(BF16, 2, 12, 20, 32, GELU, ld=40)[:2] == [UNSUPPORTED, ROW] and img(BF16, 2, 12, 20, 32, NONE, ld=40)[:2] == [0, BAND]


def test_bwd_checks_scratch_before_launching():
    """one float short of du_dwconv3x3_bwd_ws_elems: DU_ERR_BAD_ARG, from both families, with nothing launched (there is no device here)"""
    from dinounet_amd import _lib
    L = _lib.lib()
    Z, DY, X, Wp, DX, DW, DB, DZ, WS = (0x10000000 * (i + 1) for i in range(9))
    for call in ((BF16, 64, 21 * 16 * 64, 3, 8, 8, 64, 1, GELU), (F32, 64, 21 * 16 * 64, 3, 8, 8, 64, 1, GELU), (BF16, 32, 63 * 32, 2, 9, 7, 32, 0, NONE)):
        n = int(L.du_dwconv3x3_bwd_ws_elems(*call))
        assert n > 0
        assert L.du_dwconv3x3_bwd(call[0], Z, DY, X, Wp, DX, DW, DB, DZ, *call[1:], WS, n - 1, None) == BAD_ARG
        assert L.du_dwconv3x3_bwd(call[0], Z, DY, X, Wp, DX, DW, DB, DZ, *call[1:], None, n, None) == BAD_ARG
    # z and dz are required exactly when there is an activation
    call = (BF16, 64, 21 * 16 * 64, 3, 8, 8, 64, 1, GELU)
    n = int(L.du_dwconv3x3_bwd_ws_elems(*call))
    assert L.du_dwconv3x3_bwd(BF16, None, DY, X, Wp, DX, DW, DB, DZ, *call[1:], WS, n, None) == BAD_ARG
    assert L.du_dwconv3x3_bwd(BF16, Z, DY, X, Wp, DX, DW, DB, None, *call[1:], WS, n, None) == BAD_ARG
