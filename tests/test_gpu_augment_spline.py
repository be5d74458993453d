"""GPU tests (-m gpu) of csrc/augment_spline.hip through GPUAugment2D(..., interpolation="spline").apply with explicit parameter dicts,
against scipy directly (what batchgenerators calls).  Image values: max |gpu - scipy| <= 2^-22 max|x|, the bound of
test_gpu_preprocessing.py::test_cubic_resampling for the same policy (fp64 arithmetic, one rounding to fp32: half an ulp of a value that
may overshoot max|x| a little).  Labels, crops and untouched planes are exact."""
import functools

import numpy as np
import pytest
import torch
from scipy import ndimage

from dinounet_amd import _lib
from dinounet_amd import augment as A
from dinounet_amd import dataloading as DL
from oracle import augment_oracle as AO
from test_cpu_augment_spline import LABEL_TRANSFORMS, label_pattern, matrix, scipy_label_loop
from test_cpu_dataloading import make_dataset
from test_gpu_ops import dev

pytestmark = pytest.mark.gpu


def off(B, Cc, **kw):
    z, o = np.zeros((B, Cc), np.float32), np.ones((B, Cc), np.float32)
    return dict(dict(noise_sigma=z, blur_sigma=z, mult=o, contrast=o, zoom=z, gamma_inv=z, gamma=z, seed=7), **kw)


def crop(x, prm, patch):
    """batchgenerators' centre crop of an identity sample, flips applied to the result"""
    y0, x0 = (x.shape[-2] - patch[0]) // 2, (x.shape[-1] - patch[1]) // 2
    out = x[..., y0:y0 + patch[0], x0:x0 + patch[1]]
    dims = [d for d, f in ((-2, prm[4]), (-1, prm[5])) if f]
    return torch.flip(out, dims) if dims else out


# (Hi, Wi) -> (H, W): odd and even differences, more than one 16 x 16 tile, edge tiles, lines shorter than the prefilter horizon
SHAPES = [((45, 52), (32, 32)), ((80, 72), (64, 64)), ((33, 150), (32, 128)), ((70, 31), (64, 24))]


@pytest.mark.parametrize("shapes", SHAPES, ids=str)
def test_image_vs_map_coordinates(shapes):
    (Hi, Wi), patch = shapes
    B, Cc = 3, 2
    data = torch.randn(B, Cc, Hi, Wi, generator=torch.Generator().manual_seed(Hi)) + 0.5            # white noise: Keys and B-spline differ
    prm = np.stack([matrix(0.7, 1.23, 1, 0), matrix(0.0, 0.8, 0, 1), np.array([1, 0, 0, 1, 1, 1], np.float32)])   # both; scale only; identity
    want = AO.spatial_scipy_order3(data.numpy(), prm, patch)
    bound = 2.0 ** -22 * float(data.abs().max())
    d = off(B, Cc, spatial=prm)
    got, _ = A.GPUAugment2D(patch, interpolation="spline").apply(data.to(dev()), None, d)
    got = got.cpu()
    err = float(np.abs(got[:2].numpy().astype(np.float64) - want[:2]).max())
    keys, _ = A.GPUAugment2D(patch).apply(data.to(dev()), None, d)
    err_keys = float(np.abs(keys[:2].cpu().numpy().astype(np.float64) - want[:2]).max())
    inside = int((want[:2, 0] != 0).sum())
    print(f"{shapes}: {inside} pixels inside; spline max |gpu - scipy| {err:.3e} (bound {bound:.3e}); Keys path {err_keys:.3e}")
    assert inside > 50
    assert err <= bound
    assert err_keys > 100 * bound                                                                  # the input tells the two kernels apart
    assert torch.equal(got[2], crop(data[2], prm[2], patch))                                        # the identity sample: bits copied


def test_identity_samples_are_cropped():
    """integer lower bounds (Hi - Ho) // 2 with an odd and an even difference, every flip, image and labels"""
    Hi, Wi, patch = 45, 52, (32, 32)
    data = torch.randn(4, 2, Hi, Wi, generator=torch.Generator().manual_seed(2))
    seg = torch.from_numpy(np.tile(label_pattern(), (4, 1, 1, 1)))
    prm = np.array([[1, 0, 0, 1, fy, fx] for fy, fx in ((0, 0), (1, 0), (0, 1), (1, 1))], np.float32)
    aug = A.GPUAugment2D(patch, interpolation="spline")
    aug._keep_raw_labels = True
    got, lab = aug.apply(data.to(dev()), seg.to(dev()), off(4, 2, spatial=prm))
    for b in range(4):
        assert torch.equal(got[b].cpu(), crop(data[b], prm[b], patch))
        assert torch.equal(aug._raw_labels[b].cpu(), crop(seg[b], prm[b], patch))
    assert (aug._raw_labels == -1).any() and not (lab < 0).any()
    assert torch.equal(lab, aug._raw_labels.clamp_min(0))


@functools.lru_cache(maxsize=None)
def label_case():
    """the 45 x 52 pattern under the four transforms, the scipy loop's labels (-1 kept) and its tie band: computed once, not modified"""
    seg = label_pattern()
    B = len(LABEL_TRANSFORMS)
    prm = np.stack(LABEL_TRANSFORMS)
    ref = [scipy_label_loop(seg[0, 0], prm[b], (32, 32)) for b in range(B)]
    want, band = np.stack([r[0] for r in ref])[:, None], np.stack([r[1] for r in ref])[:, None]
    return torch.from_numpy(np.tile(seg, (B, 1, 1, 1))), prm, want, band


def test_labels_vs_scipy_loop():
    seg, prm, want, band = label_case()
    B = len(prm)
    aug = A.GPUAugment2D((32, 32), interpolation="spline")
    aug._keep_raw_labels = True
    data = torch.ones(B, 1, 45, 52)
    _, lab = aug.apply(data.to(dev()), seg.to(dev()), off(B, 1, spatial=prm))
    raw, lab = aug._raw_labels.cpu().numpy(), lab.cpu().numpy()
    frac = float(band.mean())
    print(f"tie band: {int(band.sum())} of {band.size} pixels; -1 before the mask pass: {int((raw == -1).sum())} pixels (scipy {int((want == -1).sum())})")
    assert frac <= 1e-3
    assert np.array_equal(raw[~band], want[~band])                                                  # -1 inside the frame is a label of its own
    assert np.array_equal(lab[~band], np.where(want < 0, 0, want)[~band])
    assert (want == -1).sum() > 100 and lab.min() == 0


def test_mask_transform():
    seg, prm, want, band = label_case()
    B = len(prm)
    data = torch.randn(B, 2, 45, 52, generator=torch.Generator().manual_seed(5)) + 0.5
    sg, mu, gm = np.full((B, 2), 0.3, np.float32), np.full((B, 2), 1.2, np.float32), np.full((B, 2), 0.7, np.float32)
    d = off(B, 2, spatial=prm, noise_sigma=sg, mult=mu, gamma=gm)
    masked, lab = A.GPUAugment2D((32, 32), interpolation="spline", mask_channels=[0]).apply(data.to(dev()), seg.to(dev()), d)
    plain, lab0 = A.GPUAugment2D((32, 32), interpolation="spline").apply(data.to(dev()), seg.to(dev()), d)
    masked, plain = masked.cpu().numpy(), plain.cpu().numpy()
    neg = (want[:, 0] < 0) & ~band[:, 0]                                                            # label < 0 before the rewrite, from scipy
    keep = (want[:, 0] >= 0) & ~band[:, 0]
    print(f"masked set: {int(neg.sum())} pixels; |plain| there: min {np.abs(plain[:, 0][neg]).min():.3f}")
    assert neg.sum() > 100 and np.abs(plain[:, 0][neg]).min() > 0                                   # noise, brightness and gamma reached the region
    assert not masked[:, 0][neg].any()
    assert np.array_equal(masked[:, 0][keep], plain[:, 0][keep])
    assert np.array_equal(masked[:, 1], plain[:, 1])                                                # the other channel: bit-identical
    assert not (lab < 0).any() and torch.equal(lab, lab0)


@pytest.mark.parametrize("shape", [(40, 33), (64, 64)], ids=str)
def test_lowres_vs_zoom(shape):
    H, W = shape
    zooms = np.array([[0.5, 0], [0.77, 0.93], [0, 0.61]], np.float32)
    x = torch.randn(3, 2, H, W, generator=torch.Generator().manual_seed(W)) + 0.5
    ident = np.tile(np.array([1, 0, 0, 1, 0, 0], np.float32), (3, 1))
    got, _ = A.GPUAugment2D(shape, interpolation="spline").apply(x.to(dev()), None, off(3, 2, spatial=ident, zoom=zooms))
    got = got.cpu()
    bound = 2.0 ** -22 * float(x.abs().max())
    clipped = 0
    for b, c in np.ndindex(3, 2):
        z = float(zooms[b, c])
        if z == 0:
            assert torch.equal(got[b, c], x[b, c])
            continue
        Hl, Wl = max(int(np.rint(H * z)), 1), max(int(np.rint(W * z)), 1)
        low = ndimage.zoom(x[b, c].numpy().astype(np.float64), (Hl / H, Wl / W), order=0, mode="nearest", grid_mode=True)
        up = ndimage.zoom(low, (H / Hl, W / Wl), order=3, mode="nearest", grid_mode=True)
        assert low.shape == (Hl, Wl) and up.shape == (H, W)
        clipped += int((up < low.min()).any() or (up > low.max()).any())
        err = float(np.abs(got[b, c].numpy().astype(np.float64) - np.clip(up, low.min(), low.max())).max())
        print(f"{shape} zoom {z:.2f}: low grid {(Hl, Wl)}, max |gpu - zoom round trip| {err:.3e} (bound {bound:.3e})")
        assert err <= bound
    assert clipped > 0


def test_coefficients_across_segments_and_tiles():
    """du_aug_spline_coeffs itself at 70 x 300: two row segments (256 + 44), two column tiles (64 + 6); planes listed out of order"""
    L = _lib.lib()
    x = torch.randn(3, 70, 300, generator=torch.Generator().manual_seed(9)) + 0.5
    idx = torch.tensor([2, 0], dtype=torch.int32)
    n = int(L.du_aug_spline_ws_elems(2, 70, 300))
    assert n == 2 * 2 * 70 * 300
    xd, idxd, ws = x.to(dev()), idx.to(dev()), torch.zeros(n, dtype=torch.float64, device=dev())
    _lib.check(L.du_aug_spline_coeffs(A._p(xd), 3, A._p(idxd), 2, 70, 300, A._p(ws), n, A._st()), "du_aug_spline_coeffs")
    got = ws[:2 * 70 * 300].view(2, 70, 300).cpu().numpy()
    for j, p in enumerate((2, 0)):
        want = ndimage.spline_filter(x[p].numpy().astype(np.float64), 3, mode="mirror")
        err = float(np.abs(got[j] - want).max())
        print(f"plane {p}: max |coefficients - spline_filter| {err:.2e}")
        assert err <= 1e-12


def test_train_batches_spline():
    gpu = make_dataset(dev())
    patch, B = (32, 40), 4
    mk = lambda **kw: DL.TrainBatches(gpu, patch, B, seed=3, **kw)
    a, b, k = mk(interpolation="spline", use_mask_for_norm=[True, False]), mk(interpolation="spline", use_mask_for_norm=[True, False]), mk()
    assert a.augment.interpolation == "spline" and a.augment.mask_channels == [0] and k.augment.interpolation == "keys"
    a.augment._keep_raw_labels = True
    padded = 0
    for _ in range(2):
        (xa, ta), (xb, tb), _ = next(a), next(b), next(k)
        assert torch.equal(xa, xb) and torch.equal(ta, tb)                                          # reproducible from the seed
        assert ta.dtype == torch.int64 and tuple(ta.shape) == (B, 1, *patch) and not (ta < 0).any()
        for got, want in zip(a.last_draw, k.last_draw):                                             # the same decisions in either mode
            assert got.keys() == want.keys()
            for key in got:
                assert np.array_equal(np.asarray(got[key]), np.asarray(want[key])), key
        neg = a.augment._raw_labels[:, 0] < 0
        padded += int(neg.sum())
        assert not xa[:, 0][neg].any()                                                              # the masked channel is 0 on the padding
    assert padded > 0


def test_entries_decline_without_launching():
    L = _lib.lib()
    x = torch.randn(2, 2, 8, 8, device=dev())
    lab = torch.full((2, 1, 8, 8), -1.0, device=dev())
    before = x.clone()
    assert L.du_aug_mask(A._p(x), A._p(lab), 4, 2, 2, 64, A._st()) == -1                            # channel 2 of 2
    assert L.du_aug_mask(A._p(x), A._p(lab), 1, 2, 2, 1 << 31, A._st()) == -2
    assert L.du_aug_mask(A._p(x), None, 1, 2, 2, 64, A._st()) == -1
    assert L.du_aug_spline_coeffs(A._p(x), 4, A._p(lab), 4, 8, 8, A._p(x), 2 * 4 * 64 - 1, A._st()) == -1
    assert L.du_aug_spatial_spline(A._p(x), None, A._p(x), A._p(x), 0, A._p(x), A._p(x), None, 2, 2, 8, 0, 8, 8, A._st()) == -1
    assert L.du_aug_lowres_spline(A._p(x), A._p(x), A._p(lab), A._p(lab), A._p(lab), 4, 8, 8, A._st()) == -1     # in place
    torch.cuda.synchronize()
    assert torch.equal(x, before) and bool((lab == -1).all())
    with pytest.raises(ValueError):
        A.GPUAugment2D((8, 8), interpolation="spline", mask_channels=[2]).apply(x, lab, off(2, 2, spatial=np.tile(matrix(0.3, 1.0), (2, 1))))
    with pytest.raises(ValueError):                                                                  # MaskTransform without a segmentation
        A.GPUAugment2D((8, 8), interpolation="spline", mask_channels=[0]).apply(x, None, off(2, 2, spatial=np.tile(matrix(0.3, 1.0), (2, 1))))
    with pytest.raises(RuntimeError):
        _lib.check(L.du_aug_mask(A._p(x), A._p(lab), 4, 2, 2, 64, A._st()), "du_aug_mask")
