"""The host restatements of csrc/augment_spline.hip (dinounet_amd.augment._*_numpy) against scipy itself, which is what batchgenerators
calls, in fp64: bound 1e-12 absolute on O(1) data.  Plus the constructor's checks, the draws of the two modes and the argument checks of
the C entries (fake operand addresses: nothing is launched, no device is needed)."""
import ctypes as C

import numpy as np
import pytest
from scipy import ndimage

from dinounet_amd import augment as A
from oracle import augment_oracle as AO

BOUND = 1e-12
BAD_ARG, UNSUPPORTED = -1, -2


def matrix(angle, scale, fy=0, fx=0):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([c * scale, -s * scale, s * scale, c * scale, fy, fx], np.float32)


ROTATIONS = {"0.6x0.8": matrix(0.6, 0.8, 1, 0), "-2.3x1.3": matrix(-2.3, 1.3, 0, 1), "0.3x1.0": matrix(0.3, 1.0)}
# coordinates that are exactly the integers 0 .. n - 1 (patch = plane): the half turn; and rows kept, columns scaled
EXACT = {"half_turn": np.array([-1, 0, 0, -1, 0, 0], np.float32), "x_scaled": np.array([1, 0, 0, 0.8, 0, 1], np.float32)}
PLANES = [(9, 11), (37, 53), (2, 40), (1, 5)]


@pytest.mark.parametrize("n", [1, 2, 3, 5, 17, 40, 100])
def test_coefficients_vs_spline_filter(n):
    x = np.random.RandomState(n).randn(n, 7) + 0.5
    want = ndimage.spline_filter1d(x, 3, axis=0, mode="mirror")
    got = A._spline_coeffs_numpy(x[:, :1])[:, 0]                                          # one column: the other axis has length 1
    err = float(np.abs(got - want[:, 0]).max())
    print(f"n = {n}: |coefficients - spline_filter1d| max {err:.2e}")
    assert err <= BOUND
    if n == 1:
        assert np.array_equal(got, x[:, 0])                                               # a line of length 1 is its own coefficient
    both = ndimage.spline_filter(x, 3, mode="mirror")
    assert float(np.abs(A._spline_coeffs_numpy(x) - both).max()) <= BOUND
    assert float(np.abs(A._spline_coeffs_numpy(x.T) - both.T).max()) <= BOUND


@pytest.mark.parametrize("shape", PLANES, ids=str)
@pytest.mark.parametrize("name", list(ROTATIONS) + list(EXACT))
def test_spatial_restatement_vs_map_coordinates(name, shape):
    Hi, Wi = shape
    prm = (ROTATIONS[name] if name in ROTATIONS else EXACT[name])[None]
    patch = (Hi + 3, Wi + 2) if name in ROTATIONS else (Hi, Wi)
    data = (np.random.RandomState(Hi * Wi).randn(1, 2, Hi, Wi) + 0.5).astype(np.float32)
    y, x = AO._coords(prm[0], Hi, Wi, *patch)
    ry, rx = A._coords_float64(prm[0], Hi, Wi, *patch)
    assert np.array_equal(y, ry) and np.array_equal(x, rx)
    if name in EXACT:                                                                     # the borders themselves are hit, and are inside
        assert (y == 0).any() and (y == Hi - 1).any()
        assert name != "half_turn" or ((x == 0).any() and (x == Wi - 1).any())
    want = AO.spatial_scipy_order3(data, prm, patch)
    got = A._spatial_spline_numpy(data, prm, patch)
    inside = (y >= 0) & (y <= Hi - 1) & (x >= 0) & (x <= Wi - 1)
    err = float(np.abs(got - want).max())
    print(f"{name} {shape} -> {patch}: {int(inside.sum())} pixels inside, |restatement - map_coordinates| max {err:.2e}")
    assert err <= BOUND
    assert not got[0][:, ~inside].any()
    if name in EXACT:
        assert inside.all() and np.abs(got).min() > 0


def label_pattern(Hi=45, Wi=52):
    """blocks of the labels 0..3 inside a frame of -1 (8 rows, 12 columns: the centre crop to 32 x 32 still shows it): loader padding /
    crop_to_nonzero's nonzero_label"""
    yy, xx = np.meshgrid(np.arange(Hi), np.arange(Wi), indexing="ij")
    seg = ((yy // 7 + xx // 9) % 4).astype(np.float32)
    seg[:8], seg[-8:], seg[:, :12], seg[:, -12:] = -1, -1, -1, -1
    return seg[None, None]


def scipy_label_loop(seg, prm, patch):
    """batchgenerators' interpolate_img(is_seg=True, order=1, cval=-1) -> (labels with -1 kept, tie band: some label's |m - 1/2| < 1e-9)"""
    Hi, Wi = seg.shape
    y, x = AO._coords(prm, Hi, Wi, *patch)
    res, band = np.zeros(patch), np.zeros(patch, bool)
    for lab in np.sort(np.unique(seg)):
        m = ndimage.map_coordinates((seg == lab).astype(np.float64), [y, x], order=1, mode="constant", cval=-1.0)
        res[m >= 0.5] = lab
        band |= np.abs(m - 0.5) < 1e-9
    return res, band


LABEL_TRANSFORMS = [matrix(0.6, 0.8, 1, 0), matrix(-2.3, 1.3, 0, 1), matrix(0.3, 1.0), matrix(0.0, 0.77, 1, 1)]


def test_label_restatement_vs_scipy_loop():
    seg = label_pattern()
    patch = (32, 32)
    minus = 0
    for prm in LABEL_TRANSFORMS:
        want, band = scipy_label_loop(seg[0, 0], prm, patch)
        got = A._labels_order1_numpy(seg, prm[None], patch)[0, 0]
        frac = float(band.mean())
        print(f"matrix {prm[:4]}: tie band {int(band.sum())} pixels, {int((want == -1).sum())} pixels -1")
        assert frac <= 1e-3
        assert np.array_equal(got[~band], want[~band])
        assert (want > 0).any()
        minus += int((want == -1).sum())
    assert minus > 100


@pytest.mark.parametrize("shape", [(40, 33), (64, 64)], ids=str)
def test_lowres_restatement_vs_zoom(shape):
    H, W = shape
    zooms = np.array([[0.5, 0.51, 0.61], [0.77, 0.93, 0.0]], np.float32)
    x = (np.random.RandomState(H).randn(2, 3, H, W) + 0.5).astype(np.float32)
    got = A._lowres_spline_numpy(x, zooms)
    clipped = 0
    for b, c in np.ndindex(2, 3):
        z = zooms[b, c]
        if z == 0:
            assert np.array_equal(got[b, c], x[b, c].astype(np.float64))
            continue
        Hl, Wl = (int(v) for v in A._lowres_sizes(zooms, H, W).reshape(2, 3, 2)[b, c])
        assert (Hl, Wl) == (max(int(np.rint(H * float(z))), 1), max(int(np.rint(W * float(z))), 1))
        low = ndimage.zoom(x[b, c].astype(np.float64), (Hl / H, Wl / W), order=0, mode="nearest", grid_mode=True)
        assert low.shape == (Hl, Wl)
        up = ndimage.zoom(low, (H / Hl, W / Wl), order=3, mode="nearest", grid_mode=True)
        assert up.shape == (H, W)
        clipped += int((up < low.min()).any() or (up > low.max()).any())
        err = float(np.abs(got[b, c] - np.clip(up, low.min(), low.max())).max())
        print(f"{shape} zoom {z:.2f}: low grid {(Hl, Wl)}, |restatement - zoom round trip| max {err:.2e}")
        assert err <= BOUND
    assert clipped > 0


@pytest.mark.parametrize("patch", [(32, 32), (33, 40)], ids=str)                        # 45 - 32 odd, 52 - 32 even; 45 - 33 even, 52 - 40 even
def test_identity_is_the_integer_centre_crop(patch):
    Hi, Wi = 45, 52
    data = np.random.RandomState(1).randn(4, 2, Hi, Wi).astype(np.float32)
    seg = np.tile(label_pattern(), (4, 1, 1, 1))
    prm = np.array([[1, 0, 0, 1, fy, fx] for fy, fx in ((0, 0), (1, 0), (0, 1), (1, 1))], np.float32)
    got, lab = A._spatial_spline_numpy(data, prm, patch), A._labels_order1_numpy(seg, prm, patch)
    y0, x0 = (Hi - patch[0]) // 2, (Wi - patch[1]) // 2
    for b in range(4):
        want, wl = data[b, :, y0:y0 + patch[0], x0:x0 + patch[1]], seg[b, :, y0:y0 + patch[0], x0:x0 + patch[1]]
        if prm[b, 4]:
            want, wl = want[:, ::-1], wl[:, ::-1]
        if prm[b, 5]:
            want, wl = want[:, :, ::-1], wl[:, :, ::-1]
        assert np.array_equal(got[b], want.astype(np.float64)) and np.array_equal(lab[b], wl.astype(np.float64))
    assert (lab == -1).any()


def test_mask_restatement():
    data = np.ones((2, 3, 4, 5), np.float32)
    lab = np.zeros((2, 1, 4, 5), np.float32)
    lab[0, 0, 1, 2], lab[1, 0, 3, 4], lab[1, 0, 0, 0] = -1, -1, 2
    d, l = A._mask_numpy(data, lab, [0, 2])
    assert d[0, 0, 1, 2] == 0 and d[0, 2, 1, 2] == 0 and d[0, 1, 1, 2] == 1 and d[1, 0, 3, 4] == 0 and d.sum() == data.sum() - 4
    assert l.min() == 0 and l[1, 0, 0, 0] == 2 and data.min() == 1


def test_constructor_checks_and_same_draws():
    with pytest.raises(ValueError):
        A.GPUAugment2D((32, 32), interpolation="linear")
    with pytest.raises(ValueError):
        A.GPUAugment2D((32, 32), mask_channels=[0])
    with pytest.raises(ValueError):
        A.GPUAugment2D((32, 32), interpolation="keys", mask_channels=[True, False])
    with pytest.raises(ValueError):
        A.GPUAugment2D((32, 32), interpolation="spline", mask_channels=[63])
    assert A.GPUAugment2D((32, 32), interpolation="spline", mask_channels=[True, False, True]).mask_channels == [0, 2]
    assert A.GPUAugment2D((32, 32), interpolation="spline", mask_channels=[2, 0]).mask_channels == [0, 2]
    assert A.GPUAugment2D((32, 32), interpolation="spline", mask_channels=[False, False]).mask_channels is None
    assert A.GPUAugment2D((32, 32)).interpolation == "keys"
    a, b = A.GPUAugment2D((32, 40), seed=5), A.GPUAugment2D((32, 40), seed=5, interpolation="spline", mask_channels=[0])
    for _ in range(3):
        da, db = a.draw(6, 2), b.draw(6, 2)
        assert da.keys() == db.keys() and all(np.array_equal(da[k], db[k]) for k in da)


def test_entries_check_before_launching():
    from dinounet_amd import _lib
    L = _lib.lib()
    X, Y, IDX, WS, PRM, SEG, SOUT, BND = (0x10000000 * (i + 1) for i in range(8))
    big = (65536, 32768)                                                                 # a plane of 2^31 elements
    assert L.du_aug_spline_ws_elems(6, 40, 50) == 2 * 6 * 40 * 50
    assert L.du_aug_spline_ws_elems(0, 40, 50) == BAD_ARG and L.du_aug_spline_ws_elems(1, 0, 5) == BAD_ARG and L.du_aug_spline_ws_elems(1, 5, -1) == BAD_ARG
    assert L.du_aug_spline_ws_elems(1, *big) == UNSUPPORTED

    n = 2 * 6 * 40 * 50
    coeffs = lambda x=X, P=6, idx=IDX, k=6, H=40, W=50, ws=WS, n=n: L.du_aug_spline_coeffs(x, P, idx, k, H, W, ws, n, None)
    assert coeffs(x=None) == BAD_ARG and coeffs(idx=None) == BAD_ARG and coeffs(ws=None) == BAD_ARG and coeffs(n=n - 1) == BAD_ARG
    assert coeffs(P=0) == BAD_ARG and coeffs(k=0) == BAD_ARG and coeffs(H=0) == BAD_ARG and coeffs(W=-3) == BAD_ARG
    assert coeffs(H=big[0], W=big[1], n=1 << 40) == UNSUPPORTED

    def spatial(data=X, seg=SEG, prm=PRM, coef=WS, planes=6, slots=IDX, out=Y, sout=SOUT, B=3, Cc=2, Hi=40, Wi=50, Ho=32, Wo=32):
        return L.du_aug_spatial_spline(data, seg, prm, coef, planes, slots, out, sout, B, Cc, Hi, Wi, Ho, Wo, None)
    for name in ("data", "prm", "coef", "slots", "out", "sout"):
        assert spatial(**{name: None}) == BAD_ARG, name
    for name in ("B", "Cc", "Hi", "Wi", "Ho", "Wo"):
        assert spatial(**{name: 0}) == BAD_ARG, name
    assert spatial(planes=-1) == BAD_ARG
    assert spatial(Hi=big[0], Wi=big[1]) == UNSUPPORTED and spatial(Ho=big[0], Wo=big[1]) == UNSUPPORTED

    def lowres(x=X, y=Y, sizes=IDX, bounds=BND, tmp=WS, P=6, H=64, W=64):
        return L.du_aug_lowres_spline(x, y, sizes, bounds, tmp, P, H, W, None)
    for name in ("x", "y", "sizes", "bounds", "tmp"):
        assert lowres(**{name: None}) == BAD_ARG, name
    assert lowres(y=X) == BAD_ARG and lowres(P=0) == BAD_ARG and lowres(H=0) == BAD_ARG and lowres(W=0) == BAD_ARG
    assert lowres(H=big[0], W=big[1]) == UNSUPPORTED and lowres(P=65536) == UNSUPPORTED

    mask = lambda data=X, lab=SEG, bits=1, B=3, Cc=2, n=1024: L.du_aug_mask(data, lab, bits, B, Cc, n, None)
    assert mask(data=None) == BAD_ARG and mask(lab=None) == BAD_ARG and mask(B=0) == BAD_ARG and mask(Cc=0) == BAD_ARG and mask(n=0) == BAD_ARG
    assert mask(bits=4) == BAD_ARG and mask(bits=-1) == BAD_ARG                          # a channel the data does not have
    assert mask(n=1 << 31) == UNSUPPORTED
