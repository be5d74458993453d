"""Writes tests/golden/dwconv_dispatch.npz: what the library of the commit BEFORE du_dwconv_plan (csrc/dwconv_plan.h) answered to its three
depthwise queries over a sweep of shapes -- du_dwconv_band_ok, du_dwconv_band_ws_elems and du_dwconv_wgrad_ws_elems (for the token pyramid
the (B, 21 n, 1, C) query its caller made).  tests/test_cpu_dwconv_plan.py holds du_dwconv3x3_plan_describe / _bwd_ws_elems to it.  Pure
host logic: nothing launches.

  python tools/make_golden_dwconv_dispatch.py --parent libparent.so [--out tests/golden/dwconv_dispatch.npz]
"""
import argparse
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "dwconv_dispatch.npz")
KEY = 19
# the axes of the sweep, in the order of the arrays' dimensions
DTYPES = [0, 1]                                   # DU_F32, DU_BF16
PYRAMID = [0, 1]
BS = [1, 2, 3, 8]
HW = [2, 3, 6, 7, 8, 9, 12, 16, 20, 32, 40, 64, 128]
CH = [4, 8, 32, 60, 64, 72, 128, 256, 1024]
OPT19 = [0, 1, 8, 0x0800 | 1]
AXES = (OPT19, DTYPES, PYRAMID, BS, HW, HW, CH)


def sweep():
    """(index tuple, opt19, dtype, pyramid, B, H, W, C) of every row, option 19 slowest"""
    for idx in np.ndindex(*(len(a) for a in AXES)):
        yield (idx, *(a[i] for a, i in zip(AXES, idx)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    L = C.CDLL(os.path.abspath(a.parent))
    I = C.c_int
    L.du_dwconv_band_ok.argtypes = [I] * 6
    L.du_dwconv_band_ws_elems.argtypes, L.du_dwconv_band_ws_elems.restype = [I] * 6, C.c_int64
    L.du_dwconv_wgrad_ws_elems.argtypes, L.du_dwconv_wgrad_ws_elems.restype = [I] * 5, C.c_int64
    shape = tuple(len(x) for x in AXES)
    ok, band_ws, row_ws = np.zeros(shape, np.uint8), np.zeros(shape, np.int64), np.zeros(shape, np.int64)
    try:
        for idx, opt, dt, pyr, B, H, W, Cc in sweep():
            L.du_set_option(KEY, opt)
            ok[idx] = L.du_dwconv_band_ok(dt, B, H, W, Cc, pyr)
            band_ws[idx] = L.du_dwconv_band_ws_elems(dt, B, H, W, Cc, pyr)
            row_ws[idx] = L.du_dwconv_wgrad_ws_elems(dt, B, 21 * (H * W // 4), 1, Cc) if pyr else L.du_dwconv_wgrad_ws_elems(dt, B, H, W, Cc)
    finally:
        L.du_set_option(KEY, 1)
    np.savez_compressed(a.out, opt19=np.array(OPT19), dtypes=np.array(DTYPES), pyramid=np.array(PYRAMID), bs=np.array(BS), hw=np.array(HW),
                        ch=np.array(CH), band_ok=ok, band_ws=band_ws, row_ws=row_ws)
    print(f"{ok.size} rows -> {a.out} ({os.path.getsize(a.out)} bytes); band ok {int(ok.sum())}, row scratch > 0 {int((row_ws > 0).sum())}")


if __name__ == "__main__":
    main()
