"""GPU-side training augmentation for 2D slices.

`GPUAugment2D` applies the transform list of the reference trainer -- `nnUNetTrainer.get_training_transforms`
(dinounet/training/nnUNetTrainer/nnUNetTrainer.py:684-776) with the 2D configuration of
`configure_rotation_dummyDA_mirroring_and_inital_patch_size` (:391-441) -- to a batch that is already on the MI355X, through the HIP
kernels of csrc/augment.hip (C ABI `du_aug_*`).  The random decisions (which sample gets which transform, with which parameter) are
drawn on the host from a numpy RandomState exactly as batchgenerators does it (`np.random.uniform() < p_per_sample`, uniform parameter
ranges); only the per-pixel work runs on the GPU.  The reference hands the transforms to the `batchgenerators` package, which is not
vendored in the reference tree: parity is unpinned against it (tests compare the kernels with a numpy / scipy restatement,
oracle/augment_oracle.py).  Order and probabilities:

    SpatialTransform   rotation U(-180deg, 180deg) (|angle| <= 15deg for patches with aspect > 1.5), p 0.2; scale p 0.2, log-symmetric
                       draw from (0.7, 1.4) as batchgenerators does (U(0.7,1) or U(1,1.4) with probability 1/2 each); centre crop
    GaussianNoise      p 0.1, variance U(0, 0.1)
    GaussianBlur       p 0.2 per sample, p 0.5 per channel, sigma U(0.5, 1) per channel
    BrightnessMult     p 0.15, multiplier U(0.75, 1.25) per channel (per_channel=True is batchgenerators' default)
    Contrast           p 0.15, factor from (0.75, 1.25) (U(0.75,1) or U(1,1.25)), preserve_range, per channel
    SimulateLowRes     p 0.25 per sample, p 0.5 per channel, zoom U(0.5, 1)
    Gamma (inverted)   p 0.1, gamma from (0.7, 1.5), retain_stats
    Gamma              p 0.3, same
    Mirror             each axis with p 0.5
    RemoveLabel(-1,0)  (out-of-image labels are already 0)

Two interpolation modes.  The default "keys" resamples the image with the Keys bicubic kernel and counts an in-image label -1 as "outside
the image" (csrc/augment.hip).  "spline" computes what batchgenerators computes (csrc/augment_spline.hip): the image by
scipy's map_coordinates(order=3, mode="constant") -- prefiltered cubic B-spline, fp64, one rounding --, samples that drew neither rotation
nor scale by the integer centre crop, labels with -1 as a label of its own, the low-resolution simulation's up-sampling by skimage's resize
(scipy zoom order 3, mode "nearest", grid_mode, clipped), and MaskTransform (mask_channels) + RemoveLabel(-1, 0) as the last pass.  Both
modes draw the same random numbers in the same order.  The `_*_numpy` functions restate the spline-mode device algorithms on the host in
fp64; tests/test_cpu_augment_spline.py checks them against scipy.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- host restatements of csrc/augment_spline.hip (fp64) -------------------------------------------------------------------------
_HORIZON = 32                       # the prefilter sqrt(3) z^|k|, z = sqrt(3) - 2, is cut at |k| <= 32: |z|^33 < 2e-19


def _mirror(i, n):
    """scipy's "mirror" extension (d c b | a b c d | c b a) of indices at any distance from a line of n samples"""
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.abs(i) % p
    return np.where(i >= n, p - i, i)


def _bspline_weights(t):
    u = 1.0 - t
    return (u * u * u / 6.0, (4.0 - 6.0 * t * t + 3.0 * t * t * t) / 6.0, (4.0 - 6.0 * u * u + 3.0 * u * u * u) / 6.0, t * t * t / 6.0)


def _is_identity(prm):
    """no rotation and no scale were drawn: the matrix part is exactly [1, 0, 0, 1]"""
    return bool(prm[0] == 1 and prm[1] == 0 and prm[2] == 0 and prm[3] == 1)


def _spline_coeffs_numpy(x):
    """cubic B-spline coefficients of the plane x along both axes (scipy.ndimage.spline_filter(x, 3, mode="mirror")), no padding"""
    c = np.asarray(x, np.float64)
    k = np.arange(-_HORIZON, _HORIZON + 1)
    w = np.sqrt(3.0) * (np.sqrt(3.0) - 2.0) ** np.abs(k)
    for _ in range(2):                                                              # along x, then along y: filter axis 1, transpose
        n = c.shape[1]
        if n > 1:                                                                   # a line of length 1 is its own coefficient
            c = (c[:, _mirror(np.arange(n)[:, None] + k[None, :], n)] * w).sum(2)
        c = c.T
    return c


def _coords_float64(prm, Hi, Wi, Ho, Wo):
    """input coordinates of the output pixels, MirrorTransform folded in: the six fp32 parameters of one sample, then fp64 throughout
    (batchgenerators' zero-centred mesh, rotation and scale as one matrix, + the input's centre)"""
    ys, xs = np.meshgrid(np.arange(Ho, dtype=np.float64), np.arange(Wo, dtype=np.float64), indexing="ij")
    if prm[4]:
        ys = Ho - 1 - ys
    if prm[5]:
        xs = Wo - 1 - xs
    m = np.asarray(prm[:4], np.float32).astype(np.float64)
    cy, cx = ys - 0.5 * (Ho - 1), xs - 0.5 * (Wo - 1)
    return m[0] * cy + m[1] * cx + (Hi / 2.0 - 0.5), m[2] * cy + m[3] * cx + (Wi / 2.0 - 0.5)


def _centre_crop(x, prm, patch):
    """what an identity sample gets: rows / columns (n_in - n_out) // 2 onwards, flipped"""
    Ho, Wo = patch
    y0, x0 = (x.shape[-2] - Ho) // 2, (x.shape[-1] - Wo) // 2
    out = x[..., y0:y0 + Ho, x0:x0 + Wo]
    if prm[4]:
        out = out[..., ::-1, :]
    if prm[5]:
        out = out[..., :, ::-1]
    return out


def _spatial_spline_numpy(data, prm, patch):
    """SpatialTransform + MirrorTransform on the image as du_aug_spatial_spline computes it: data (B, C, Hi, Wi) -> float64 (B, C, *patch)
    (the device result is this rounded to fp32).  Identity samples are cropped; the others are map_coordinates(order=3, mode="constant",
    cval=0): 0 outside [0, Hi - 1] x [0, Wi - 1], else the 4 x 4 B-spline sum over the mirror-prefiltered coefficients, taps mirrored."""
    B, Cc, Hi, Wi = data.shape
    Ho, Wo = patch
    out = np.zeros((B, Cc, Ho, Wo), np.float64)
    for b in range(B):
        if _is_identity(prm[b]):
            out[b] = _centre_crop(np.asarray(data[b], np.float64), prm[b], patch)
            continue
        y, x = _coords_float64(prm[b], Hi, Wi, Ho, Wo)
        inside = (y >= 0) & (y <= Hi - 1) & (x >= 0) & (x <= Wi - 1)
        y0, x0 = np.floor(y).astype(np.int64), np.floor(x).astype(np.int64)
        wy, wx = _bspline_weights(y - y0), _bspline_weights(x - x0)
        for c in range(Cc):
            coef = _spline_coeffs_numpy(data[b, c])
            acc = np.zeros((Ho, Wo))
            for j in range(4):
                row = np.zeros((Ho, Wo))
                for i in range(4):
                    row += wx[i] * coef[_mirror(y0 - 1 + j, Hi), _mirror(x0 - 1 + i, Wi)]
                acc += wy[j] * row
            out[b, c] = np.where(inside, acc, 0.0)
    return out


def _labels_order1_numpy(seg, prm, patch):
    """the labels of du_aug_spatial_spline BEFORE the mask pass: seg (B, 1, Hi, Wi) -> float64 (B, 1, *patch), -1 possible.  Identity
    samples are cropped.  Otherwise 0 outside the image; inside, the largest label (-1 included) whose four bilinear taps carry a weight
    >= 1/2, else 0: batchgenerators' interpolate_img(is_seg=True, order=1, cval=-1) on every one-hot map, ascending labels overwriting."""
    B, _, Hi, Wi = seg.shape
    Ho, Wo = patch
    out = np.zeros((B, 1, Ho, Wo), np.float64)
    for b in range(B):
        s = np.asarray(seg[b, 0], np.float64)
        if _is_identity(prm[b]):
            out[b, 0] = _centre_crop(s, prm[b], patch)
            continue
        y, x = _coords_float64(prm[b], Hi, Wi, Ho, Wo)
        inside = (y >= 0) & (y <= Hi - 1) & (x >= 0) & (x <= Wi - 1)
        y0, x0 = np.clip(np.floor(y).astype(np.int64), 0, Hi - 1), np.clip(np.floor(x).astype(np.int64), 0, Wi - 1)
        fy, fx = y - y0, x - x0
        y1, x1 = np.minimum(y0 + 1, Hi - 1), np.minimum(x0 + 1, Wi - 1)           # weight 0 where clamped
        w = [(1 - fy) * (1 - fx), (1 - fy) * fx, fy * (1 - fx), fy * fx]
        lab = [s[y0, x0], s[y0, x1], s[y1, x0], s[y1, x1]]
        best, found = np.zeros((Ho, Wo)), np.zeros((Ho, Wo), bool)
        for k in range(4):
            total = np.zeros((Ho, Wo))
            for m_ in range(4):
                total += np.where(lab[m_] == lab[k], w[m_], 0.0)
            take = (total >= 0.5) & (~found | (lab[k] > best))
            best = np.where(take, lab[k], best)
            found |= take
        out[b, 0] = np.where(inside, best, 0.0)
    return out


def _lowres_sizes(zoom, H, W):
    """(P, 2) int32 low grids of SimulateLowResolutionTransform, max(rint(size * zoom), 1) in fp32 as du_aug_lowres; (0, 0) = plane left alone"""
    z = np.asarray(zoom, np.float32).reshape(-1)
    on = (z > 0) & (z < 1)
    hl = np.maximum(np.rint(np.float32(H) * z), 1).astype(np.int32)
    wl = np.maximum(np.rint(np.float32(W) * z), 1).astype(np.int32)
    return np.stack([np.where(on, hl, 0), np.where(on, wl, 0)], 1).astype(np.int32)


def _nearest_src(nl, n):
    """source pixels of the nl low-grid samples of a line of n: floor((i + 1/2) n / nl), in the fp64 operations of scipy's
    zoom(order=0, mode="nearest", grid_mode=True) -- where that quotient is an integer, the rounding of n / nl picks the pixel"""
    cc = ((np.arange(nl, dtype=np.float64) + 0.5) * (n / nl) - 0.5) + 0.5
    return np.clip(np.floor(cc).astype(np.int64), 0, n - 1)


def _lowres_spline_numpy(x, zoom):
    """SimulateLowResolutionTransform as du_aug_lowres_spline computes it: x (B, C, H, W) -> float64.  Down by the nearest source pixel
    (_nearest_src), up by preprocessing._resize_cubic_float64 (scipy zoom order 3, mode "nearest", grid_mode), clipped to the low
    grid's range (skimage's clip=True).  Planes with zoom outside (0, 1) are untouched."""
    from .preprocessing import _resize_cubic_float64
    B, Cc, H, W = x.shape
    out = np.asarray(x, np.float64).copy()
    sizes = _lowres_sizes(zoom, H, W).reshape(B, Cc, 2)
    for b in range(B):
        for c in range(Cc):
            Hl, Wl = (int(v) for v in sizes[b, c])
            if Hl == 0:
                continue
            low = out[b, c][np.ix_(_nearest_src(Hl, H), _nearest_src(Wl, W))]
            out[b, c] = np.clip(_resize_cubic_float64(low, (H, W)), low.min(), low.max())
    return out


def _mask_numpy(data, labels, mask_channels):
    """MaskTransform + RemoveLabelTransform(-1, 0): (data with the masked channels 0 where labels < 0, labels with the negatives 0)"""
    data, neg = np.array(data), np.asarray(labels)[:, 0] < 0
    for c in mask_channels:
        data[:, c][neg] = 0
    return data, np.where(np.asarray(labels) < 0, 0, labels)


def _channel_list(mask_channels):
    """channel indices from a list of indices or a list of bools (use_mask_for_norm)"""
    m = list(mask_channels)
    if all(isinstance(v, (bool, np.bool_)) for v in m):
        return [i for i, v in enumerate(m) if v]
    return sorted({int(v) for v in m})


class GPUAugment2D:
    def __init__(self, patch_size, seed=None, *, interpolation="keys", mask_channels=None):
        self.patch = tuple(int(v) for v in patch_size)
        assert len(self.patch) == 2
        if interpolation not in ("keys", "spline"):
            raise ValueError(f"interpolation must be 'keys' or 'spline', not {interpolation!r}")
        self.interpolation = interpolation
        self.mask_channels = (None if mask_channels is None else _channel_list(mask_channels)) or None       # no channel named: no MaskTransform
        if self.mask_channels is not None and interpolation != "spline":
            raise ValueError("mask_channels needs interpolation='spline': the Keys path cannot produce the label -1 that MaskTransform reads")
        if self.mask_channels is not None and any(c < 0 or c > 62 for c in self.mask_channels):
            raise ValueError("mask_channels must lie in 0 .. 62")
        self._keep_raw_labels, self._raw_labels = False, None                     # tests: the labels before the mask pass
        lim = 15.0 if max(self.patch) / min(self.patch) > 1.5 else 180.0            # nnUNetTrainer.py:401-412
        self.angle = (-lim / 360 * 2 * np.pi, lim / 360 * 2 * np.pi)
        self.rs = np.random.RandomState(seed)

    # ---- parameter draws (host) ---------------------------------------------------------------------------------------------
    def _two_sided(self, lo, hi):
        """batchgenerators' draw for ranges straddling 1 (scale, contrast, gamma): below / above 1 with probability 1/2"""
        if self.rs.random_sample() < 0.5 and lo < 1:
            return self.rs.uniform(lo, 1)
        return self.rs.uniform(max(lo, 1), hi)

    def draw(self, B, Cc):
        """All random decisions of one batch -> dict of numpy arrays (also the input of the oracle restatement)."""
        rs = self.rs
        prm = np.zeros((B, 6), np.float32)
        for b in range(B):
            ang = rs.uniform(*self.angle) if rs.uniform() < 0.2 else 0.0
            sc = self._two_sided(0.7, 1.4) if rs.uniform() < 0.2 else 1.0
            c, s = np.cos(ang), np.sin(ang)
            prm[b, :4] = np.array([c, -s, s, c]) * sc          # coords = R(angle) @ coords, then * scale (rotate_coords_2d, scale_coords)
        noise = np.zeros((B, Cc), np.float32)
        for b in range(B):
            if rs.uniform() < 0.1:
                # batchgenerators' augment_gaussian_noise draws `variance = uniform(0, 0.1)` and hands it to np.random.normal as the
                # STANDARD DEVIATION (scale): the noise std is U(0, 0.1), not its square root (per_channel=False: one draw per sample)
                noise[b] = rs.uniform(0, 0.1)
        blur = np.zeros((B, Cc), np.float32)
        for b in range(B):
            if rs.uniform() < 0.2:
                for c_ in range(Cc):
                    if rs.uniform() <= 0.5:
                        blur[b, c_] = rs.uniform(0.5, 1.0)
        mult = np.ones((B, Cc), np.float32)
        for b in range(B):
            if rs.uniform() < 0.15:
                mult[b] = rs.uniform(0.75, 1.25, Cc)
        contrast = np.ones((B, Cc), np.float32)
        for b in range(B):
            if rs.uniform() < 0.15:
                contrast[b] = [self._two_sided(0.75, 1.25) for _ in range(Cc)]
        zoom = np.zeros((B, Cc), np.float32)
        for b in range(B):
            if rs.uniform() < 0.25:
                for c_ in range(Cc):
                    if rs.uniform() < 0.5:
                        zoom[b, c_] = rs.uniform(0.5, 1.0)
        gam = []
        for p_ in (0.1, 0.3):
            g = np.zeros((B, Cc), np.float32)
            for b in range(B):
                if rs.uniform() < p_:
                    g[b] = [self._two_sided(0.7, 1.5) for _ in range(Cc)]
            gam.append(g)
        for b in range(B):
            prm[b, 4] = float(rs.uniform() < 0.5)
            prm[b, 5] = float(rs.uniform() < 0.5)
        return dict(spatial=prm, noise_sigma=noise, blur_sigma=blur, mult=mult, contrast=contrast, zoom=zoom, gamma_inv=gam[0], gamma=gam[1],
                    seed=int(rs.randint(0, 2 ** 31 - 1)))

    # ---- device work --------------------------------------------------------------------------------------------------------
    def apply(self, data, seg, d):
        """data (B, C, Hi, Wi) fp32 cuda, seg (B, 1, Hi, Wi) fp32 labels (or None), d = draw(...) -> (data_aug (B,C,H,W), target (B,1,H,W))"""
        if not data.is_cuda:
            raise RuntimeError("GPUAugment2D runs on the MI355X through libdinounet_hip.so (no CPU fallback)")
        L = _lib.lib()
        B, Cc, Hi, Wi = data.shape
        H, W = self.patch
        dev = data.device
        data = data.contiguous().float()
        seg = None if seg is None else seg.contiguous().float()
        out = torch.empty((B, Cc, H, W), dtype=torch.float32, device=dev)
        sout = None if seg is None else torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
        # every parameter array is a named device tensor that outlives its launch (a temporary handed to ctypes as a raw pointer would be
        # freed -- and its block re-used by the next upload -- before the kernel is even enqueued).  All of them travel in one pinned buffer
        # with one asynchronous copy (_lib.upload): an upload from pageable memory would make the host wait for the stream, i.e. for the
        # training step that is still running there
        ones = np.ones((B, Cc), np.float32)
        gam_on = {key: (d[key] > 0).astype(np.float32) for key in ("gamma_inv", "gamma")}
        (t_sp, t_noise, t_one, t_zero, t_blur, t_mult, t_con, t_zoom, t_gi, t_gi_inv, t_gi_on, t_g, t_g_inv, t_g_on) = _lib.upload(
            [d["spatial"], d["noise_sigma"], ones, 0 * ones, d["blur_sigma"], d["mult"], d["contrast"], d["zoom"],
             d["gamma_inv"], gam_on["gamma_inv"] * 1.0, gam_on["gamma_inv"], d["gamma"], gam_on["gamma"] * 0.0, gam_on["gamma"]], np.float32, dev)
        t_gamma = {"gamma_inv": (t_gi, t_gi_inv, t_gi_on.view(-1)), "gamma": (t_g, t_g_inv, t_g_on.view(-1))}
        spline = self.interpolation == "spline"
        if spline:
            if self.mask_channels and self.mask_channels[-1] >= Cc:
                raise ValueError(f"mask_channels {self.mask_channels} for {Cc} channels")
            if self.mask_channels and seg is None:
                raise ValueError("mask_channels needs the segmentation: MaskTransform zeroes the channels where the resampled label is negative")
            # coefficients only for the planes of samples that drew a rotation or a scale; the others are cropped
            moved = [b for b in range(B) if not _is_identity(d["spatial"][b])]
            planes = np.array([b * Cc + c for b in moved for c in range(Cc)], np.int32)
            slots = np.full(B * Cc, -1, np.int32)
            slots[planes] = np.arange(len(planes), dtype=np.int32)
            n_ws = int(L.du_aug_spline_ws_elems(max(len(planes), 1), Hi, Wi))
            if n_ws < 0:
                _lib.check(n_ws, "du_aug_spline_ws_elems")
            coef = torch.empty(n_ws, dtype=torch.float64, device=dev)
            t_planes, t_slots, t_sizes = _lib.upload([planes if len(planes) else [0], slots, _lowres_sizes(d["zoom"], H, W)], np.int32, dev)
            if len(planes):
                _lib.check(L.du_aug_spline_coeffs(_p(data), B * Cc, _p(t_planes), len(planes), Hi, Wi, _p(coef), n_ws, _st()), "du_aug_spline_coeffs")
            _lib.check(L.du_aug_spatial_spline(_p(data), _p(seg), _p(t_sp), _p(coef), len(planes), _p(t_slots), _p(out), _p(sout), B, Cc, Hi, Wi,
                                               H, W, _st()), "du_aug_spatial_spline")
        else:
            _lib.check(L.du_aug_spatial(_p(data), _p(seg), _p(t_sp), _p(out), _p(sout), B, Cc, Hi, Wi, H, W, _st()), "du_aug_spatial")
        P, n = B * Cc, H * W
        tmp = torch.empty_like(out)
        stats = torch.empty((P, 4), dtype=torch.float32, device=dev)
        # GaussianNoise (before blur and brightness in the reference order; the multiplier pass comes after the blur)
        _lib.check(L.du_aug_noise_mult(_p(out), _p(t_noise), _p(t_one), P, n, d["seed"], _st()), "du_aug_noise_mult")
        if (d["blur_sigma"] > 0).any():
            _lib.check(L.du_aug_blur(_p(out), _p(tmp), _p(t_blur), P, H, W, 0, _st()), "du_aug_blur")
            _lib.check(L.du_aug_blur(_p(tmp), _p(out), _p(t_blur), P, H, W, 1, _st()), "du_aug_blur")
        _lib.check(L.du_aug_noise_mult(_p(out), _p(t_zero), _p(t_mult), P, n, 0, _st()), "du_aug_noise_mult")
        if (d["contrast"] != 1).any():
            _lib.check(L.du_aug_plane_stats(_p(out), _p(stats), P, n, _st()), "du_aug_plane_stats")
            _lib.check(L.du_aug_contrast(_p(out), _p(t_con), _p(stats), P, n, _st()), "du_aug_contrast")
        if ((d["zoom"] > 0) & (d["zoom"] < 1)).any():
            if spline:
                t_bounds = torch.empty((P, 32, 2), dtype=torch.float32, device=dev)
                t_mid = torch.empty(P * n, dtype=torch.float64, device=dev)
                _lib.check(L.du_aug_lowres_spline(_p(out), _p(tmp), _p(t_sizes), _p(t_bounds), _p(t_mid), P, H, W, _st()), "du_aug_lowres_spline")
            else:
                _lib.check(L.du_aug_lowres(_p(out), _p(tmp), _p(t_zoom), P, H, W, _st()), "du_aug_lowres")
            out, tmp = tmp, out
        keep = []                      # operands of the asynchronous launches below stay referenced until apply() returns
        for key, inv in (("gamma_inv", 1.0), ("gamma", 0.0)):
            g = d[key]
            if not (g > 0).any():
                continue
            t_g, t_inv, onv = t_gamma[key]                        # gamma, [on] * inv, [on]
            _lib.check(L.du_aug_plane_stats(_p(out), _p(stats), P, n, _st()), "du_aug_plane_stats")       # mean / std to retain, range
            before = stats.clone()
            _lib.check(L.du_aug_gamma(_p(out), _p(t_g), _p(t_inv), _p(stats), P, n, _st()), "du_aug_gamma")
            _lib.check(L.du_aug_plane_stats(_p(out), _p(stats), P, n, _st()), "du_aug_plane_stats")
            # retain_stats on the (possibly negated) image: x = (x - mean') / (std' + 1e-8) * std + mean, then negate back
            sgn = 1.0 - 2.0 * t_inv.view(-1)
            mean_b, std_b = before[:, 0] * sgn, before[:, 1]
            a = std_b / (stats[:, 1] + 1e-8)
            bb = mean_b - stats[:, 0] * a
            a = ((a * sgn) * onv + (1 - onv)).contiguous()
            bb = ((bb * sgn) * onv).contiguous()
            _lib.check(L.du_aug_affine(_p(out), _p(a), _p(bb), P, n, _st()), "du_aug_affine")
            keep += [t_g, t_inv, onv, a, bb, before]
        if spline and sout is not None:
            # MaskTransform after every intensity transform, then RemoveLabel(-1, 0): the spline path's labels may hold -1
            if self._keep_raw_labels:
                self._raw_labels = sout.clone()
            bits = sum(1 << c for c in (self.mask_channels or []))
            _lib.check(L.du_aug_mask(_p(out), _p(sout), bits, B, Cc, n, _st()), "du_aug_mask")
        return out, sout

    def __call__(self, data, seg=None):
        d = self.draw(data.shape[0], data.shape[1])
        return self.apply(data, seg, d)
