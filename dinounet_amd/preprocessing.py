"""Preprocessing on the MI355X: a raw case -> the cropped, normalised, resampled array the network is run on, and the `properties` that
export.predict_segmentation needs to bring the prediction back to the raw geometry.

Mirrors DefaultPreprocessor.run_case_npy (dinounet/preprocessing/preprocessors/default_preprocessor.py:40-118) in the reference's order:
transpose_forward, crop_to_nonzero (cropping/cropping.py:8-52, with scipy's binary_fill_holes), the five schemes of
normalization/default_normalization_schemes.py, resample_data_or_seg_to_shape (resampling/default_resampling.py:77-216) for the two
pairs the planner emits (default_experiment_planner.py:127-140): order 3 for the image, order 1 for the segmentation.

The reference's preprocessing cannot be run next to this module: it needs skimage, acvl_utils and batchgenerators, none of which the
reference vendors.  Parity is therefore against RESTATEMENTS of their published behaviour, as for augmentation and postprocessing:

    fill holes   a zero voxel is filled exactly when its 6-connected component of zero voxels touches no face of the (D, H, W) volume
                 (scipy.ndimage.binary_fill_holes, default structure).  With D <= 2 every voxel lies on a z face: nothing is filled.
    order 3      skimage.transform.resize(x, shape, 3, mode='edge', anti_aliasing=False) (skimage >= 0.19) =
                 scipy.ndimage.zoom(x, shape_out / shape_in, order=3, mode='nearest', grid_mode=True), then a clip to [min x, max x]:
                 12 edge samples of padding, the cubic B-spline prefilter (pole sqrt(3) - 2, gain 6, mirror initialisation) along every
                 resampled axis, source coordinate (i + 1/2) n_in / n_out - 1/2 NOT clamped, four B-spline taps per axis.  fp64
                 throughout, one rounding to fp32.
    order 1 seg  batchgenerators' resize_segmentation(seg, shape, 1): for every label in ascending order the one-hot map resized with
                 order 1 and mode 'edge' is painted where it is >= 0.5, later labels over earlier ones, 0 where no label reaches 0.5.
                 Evaluated in integers: the weight of a label is a sum of products of the integer tap weights of export.source_taps over
                 the denominator 4 Ho Wo, the test is 2 numerator >= denominator.

CUDA tensors run csrc/preprocess.hip; CPU tensors run the numpy / scipy restatement of the same semantics, which is
what the GPU tests compare the kernels against (tests/test_cpu_preprocessing.py checks the restatements against independent code).
On the device the only read-backs are the bounding box (it sizes the output) and, for RGBTo01Normalization, the range check.

Differences from the reference, on purpose:
  * the crop is the one cropping.py:8-52 describes: bounding box of the filled non-zero mask, `nonzero_label` outside it.  (The
    reference tree's copy sets its mask all True right after computing it, :34, which turns the crop into the identity.)  An all-zero
    case raises ValueError;
  * resampling is in-plane only: a new shape that changes the number of slices, or a separate-z axis other than 0, raises ValueError
    (the same limit export.py states);
  * the segmentation is always int16 (the reference emits int8 or int16 by the maximum label: a read-back would have to decide it);
  * ZScoreNormalization takes mean and standard deviation in fp64 (two passes) and rounds the result once; numpy's float32 recipe differs
    from that by its own summation error (DESIGN 3e has the figure);
  * the image comes out of the crop as fp32 whatever its dtype was;
  * properties['class_locations'] (:94-111) is training-set preparation with a host RNG: run_case leaves it out,
    dataloading.add_class_locations fills it from the returned segmentation."""
import math

import numpy as np
import torch

from . import _lib

ANISO_THRESHOLD = 3                 # dinounet/configuration.py
SPLINE_PAD = 12                     # scipy.ndimage.zoom pads 12 samples for mode='nearest'
_POLE = math.sqrt(3.0) - 2.0
_DTYPES = {torch.float32: 0, torch.float64: 1, torch.uint8: 2, torch.int16: 3, torch.int32: 4}
NORM_NONE, NORM_RGB, NORM_CT, NORM_RESCALE, NORM_ZSCORE = 0, 1, 2, 3, 4
_SCHEMES = {"NoNormalization": NORM_NONE, "RGBTo01Normalization": NORM_RGB, "CTNormalization": NORM_CT,
            "RescaleTo01Normalization": NORM_RESCALE, "ZScoreNormalization": NORM_ZSCORE}


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------ checks
def _check_data(data):
    if not isinstance(data, torch.Tensor) or data.ndim != 4:
        raise ValueError("data must be a (C, D, H, W) torch tensor; a 2-D case has D == 1")
    if data.numel() == 0:
        raise ValueError("empty image")
    if data.dtype in (torch.float16, torch.bfloat16):
        data = data.float()
    elif data.dtype == torch.int8:
        data = data.to(torch.int16)
    if data.dtype not in _DTYPES:
        raise ValueError(f"image dtype {data.dtype} is not supported (float16/32/64, bfloat16, uint8, int8/16/32)")
    if data[0].numel() >= (1 << 31) - 1:
        raise ValueError(f"fewer than 2^31 - 1 voxels per channel are supported, got {tuple(data.shape)}")
    return data.contiguous()


def _check_seg(seg, data):
    if seg is None:
        return None
    if not isinstance(seg, torch.Tensor) or seg.ndim != 4 or seg.shape[0] != 1 or seg.shape[1:] != data.shape[1:]:
        raise ValueError("seg must be a (1, D, H, W) torch tensor of the image's spatial shape")
    if seg.is_floating_point() or seg.dtype == torch.bool:
        raise ValueError("seg must be an integer tensor")
    if seg.device != data.device:
        raise ValueError("data and seg must be on one device")
    return seg.to(torch.int16).contiguous()


# ------------------------------------------------------------------------------------------------ the restatements (numpy / scipy)
def _fill_holes_numpy(mask):
    """scipy.ndimage.binary_fill_holes(mask) for a 3-D bool array, restated: mask | the 6-connected components of ~mask that touch no face"""
    from scipy import ndimage
    lab, k = ndimage.label(~mask, structure=ndimage.generate_binary_structure(3, 1))
    outside = np.zeros(k + 1, dtype=bool)
    outside[0] = True                                                                 # label 0: the mask itself
    for face in (lab[0], lab[-1], lab[:, 0], lab[:, -1], lab[:, :, 0], lab[:, :, -1]):
        outside[np.unique(face)] = True
    return mask | ~outside[lab]


def _bbox_numpy(mask):
    """half-open [lo, hi) per axis of the True voxels (acvl_utils' get_bbox_from_mask)"""
    bbox = []
    for ax in range(3):
        hit = np.flatnonzero(mask.any(axis=tuple(a for a in range(3) if a != ax)))
        bbox.append([int(hit[0]), int(hit[-1]) + 1])
    return bbox


def _spline_prefilter(x, axis):
    """cubic B-spline coefficients of float64 `x` along `axis` (scipy.ndimage.spline_filter1d, order 3, mode 'mirror'): gain 6, the
    causal recursion from the exact mirror sum, the anticausal one from c[n - 1] = z / (z^2 - 1) (c+[n - 1] + z c+[n - 2])"""
    z = _POLE
    c = np.moveaxis(x, axis, 0) * 6.0
    n = c.shape[0]
    assert n >= 3
    col = (-1,) + (1,) * (c.ndim - 1)
    zn1 = z ** (n - 1)
    zp = (z ** np.arange(1, n - 1)).reshape(col)
    c[0] = (c[0] + zn1 * c[n - 1] + (zp * (c[1:n - 1] + zn1 * c[n - 2:0:-1])).sum(0)) / (1.0 - zn1 * zn1)
    for i in range(1, n):
        c[i] += z * c[i - 1]
    c[n - 1] = (z / (z * z - 1.0)) * (c[n - 1] + z * c[n - 2])
    for i in range(n - 2, -1, -1):
        c[i] = z * (c[i + 1] - c[i])
    return np.moveaxis(c, 0, axis)


def _cubic_axis(x, n_out, axis):
    """float64 x resampled to n_out samples along `axis`: pad, prefilter, four taps at the unclamped source coordinate"""
    n_in = x.shape[axis]
    pad = [(0, 0)] * x.ndim
    pad[axis] = (SPLINE_PAD, SPLINE_PAD)
    c = _spline_prefilter(np.pad(x, pad, mode="edge"), axis)
    o = np.arange(n_out, dtype=np.int64)
    num, den = (2 * o + 1) * n_in - n_out, 2 * n_out
    f = num // den                                                                    # floor of the source coordinate
    t = (num - f * den) / float(den)
    u = 1.0 - t
    weights = (u * u * u / 6.0, (4.0 - 6.0 * t * t + 3.0 * t * t * t) / 6.0, (4.0 - 6.0 * u * u + 3.0 * u * u * u) / 6.0, t * t * t / 6.0)
    col = [1] * x.ndim
    col[axis] = -1
    out = 0.0
    for j, w in enumerate(weights):
        out = out + w.reshape(col) * np.take(c, f + SPLINE_PAD - 1 + j, axis=axis)
    return out


def _resize_cubic_float64(x, out_hw):
    """x (..., H, W) -> float64 (..., Ho, Wo), before the clip.  An axis that keeps its extent is not touched (there the prefilter and the
    taps at integer coordinates cancel)."""
    y = np.asarray(x, dtype=np.float64)
    if int(out_hw[1]) != y.shape[-1]:
        y = _cubic_axis(y, int(out_hw[1]), y.ndim - 1)
    if int(out_hw[0]) != y.shape[-2]:
        y = _cubic_axis(y, int(out_hw[0]), y.ndim - 2)
    return y


def _int_taps(n_in, n_out):
    """export.source_taps in integers: (lower tap, upper tap, weight of the lower, weight of the upper) over the denominator 2 n_out"""
    o = np.arange(n_out, dtype=np.int64)
    num, den = (2 * o + 1) * n_in - n_out, 2 * n_out
    f = num // den
    wb = num - f * den
    return np.clip(f, 0, n_in - 1), np.clip(f + 1, 0, n_in - 1), den - wb, wb


def _label_weights(seg, out_hw):
    """the four tap labels and their integer weights (denominator 4 Ho Wo) of every output pixel of seg (D, H, W)"""
    ya, yb, wya, wyb = _int_taps(seg.shape[1], int(out_hw[0]))
    xa, xb, wxa, wxb = _int_taps(seg.shape[2], int(out_hw[1]))
    labels = [seg[:, ys][:, :, xs].astype(np.int64) for ys in (ya, yb) for xs in (xa, xb)]
    weights = [wy[:, None] * wx[None, :] for wy in (wya, wyb) for wx in (wxa, wxb)]
    return labels, weights


def _resize_seg_numpy(seg, out_hw):
    """the integer vote: the largest label whose weight is at least half the denominator, else 0"""
    labels, weights = _label_weights(seg, out_hw)
    den = 4 * int(out_hw[0]) * int(out_hw[1])
    none = -(1 << 40)
    best = np.full(labels[0].shape, none, dtype=np.int64)
    for q in range(4):
        tot = sum(np.where(labels[r] == labels[q], weights[r][None], 0) for r in range(4))
        best = np.where((2 * tot >= den) & (labels[q] > best), labels[q], best)
    return np.where(best == none, 0, best).astype(np.int16)


def _normalize_numpy(x, mask, code, params):
    """one channel volume, float32 in place.  The four fp32 schemes are the reference's own operations in its order."""
    if code == NORM_RGB:
        x /= np.float32(255.0)
    elif code == NORM_CT:
        lo, hi, mean, den = (np.float32(v) for v in params)
        np.clip(x, lo, hi, out=x)
        x -= mean
        x /= den
    elif code == NORM_RESCALE:
        x -= x.min()
        x /= max(x.max(), np.float32(1e-8))
    elif code == NORM_ZSCORE:
        sel = x[mask].astype(np.float64) if mask is not None else x.astype(np.float64)
        if sel.size == 0:
            return
        mean = sel.sum() / sel.size
        std = math.sqrt(float(((sel - mean) ** 2).sum() / sel.size))
        res = ((sel - mean) / max(std, 1e-8)).astype(np.float32)
        if mask is not None:
            x[mask] = res
        else:
            x[...] = res


# ------------------------------------------------------------------------------------------------ crop
def _mask_and_bbox(data):
    """data (C, D, H, W) checked -> (mask uint8 (D, H, W) on data's device, bbox [[lo, hi]] * 3)"""
    C, D, H, W = (int(i) for i in data.shape)
    if not data.is_cuda:
        x = data.numpy()
        nonzero = np.zeros((D, H, W), dtype=bool)
        for c in range(C):                                                            # cropping.py:16-19
            nonzero |= x[c] != 0
        mask = _fill_holes_numpy(nonzero)
        if not mask.any():
            raise ValueError("the case is zero everywhere: there is nothing to crop to")
        return torch.from_numpy(mask.astype(np.uint8)), _bbox_numpy(mask)
    L = _lib.lib()
    mask = torch.empty((D, H, W), dtype=torch.uint8, device=data.device)
    bbox = torch.empty(6, dtype=torch.int32, device=data.device)
    ws_elems = int(L.du_pre_fill_ws_elems(D, H, W))
    ws = torch.empty(max(ws_elems, 4), dtype=torch.int32, device=data.device)
    _lib.check(L.du_pre_nonzero_mask(data.data_ptr(), _DTYPES[data.dtype], C, D, H, W, mask.data_ptr(), bbox.data_ptr(), ws.data_ptr(),
                                     ws_elems, _stream()), "du_pre_nonzero_mask")
    b = bbox.tolist()                                                                 # the read-back that sizes the output
    if b[3] == 0:
        raise ValueError("the case is zero everywhere: there is nothing to crop to")
    return mask, [[b[0], b[3]], [b[1], b[4]], [b[2], b[5]]]


def create_nonzero_mask(data):
    """cropping.py:8-21 for a (C, D, H, W) tensor: bool (D, H, W) on data's device, True where any channel is non-zero, holes filled.
    CUDA tensors run du_pre_nonzero_mask, CPU tensors the scipy restatement."""
    mask, _ = _mask_and_bbox(_check_data(data))
    return mask.bool()


def crop_to_nonzero(data, seg=None, nonzero_label=-1):
    """cropping.py:24-52: (data fp32 (C, d, h, w), seg int16 (1, d, h, w), bbox [[lo, hi], [lo, hi], [lo, hi]]) on data's device, cropped
    to the half-open bounding box of the filled non-zero mask.  With a segmentation (1, D, H, W): seg[(seg == 0) & ~mask] =
    nonzero_label; without: nonzero_label outside the mask, 0 inside.  The inputs are not modified.  ValueError for an all-zero case."""
    data = _check_data(data)
    seg = _check_seg(seg, data)
    label = int(nonzero_label)
    if not -32768 <= label <= 32767:
        raise ValueError("nonzero_label must fit int16")
    mask, bbox = _mask_and_bbox(data)
    (z0, z1), (y0, y1), (x0, x1) = bbox
    C, D, H, W = (int(i) for i in data.shape)
    d, h, w = z1 - z0, y1 - y0, x1 - x0
    if not data.is_cuda:
        sl = (slice(z0, z1), slice(y0, y1), slice(x0, x1))
        out = torch.from_numpy(data.numpy()[(slice(None), *sl)].astype(np.float32))
        m = mask.numpy()[sl] != 0
        if seg is not None:
            s = seg.numpy()[0][sl].copy()
            s[(s == 0) & ~m] = label                                                  # :46
        else:
            s = np.where(m, 0, label).astype(np.int16)                                # :48-50
        return out, torch.from_numpy(s)[None], bbox
    out = torch.empty((C, d, h, w), dtype=torch.float32, device=data.device)
    seg_out = torch.empty((1, d, h, w), dtype=torch.int16, device=data.device)
    _lib.check(_lib.lib().du_pre_crop(data.data_ptr(), _DTYPES[data.dtype], mask.data_ptr(), None if seg is None else seg.data_ptr(), C, D,
                                      H, W, z0, y0, x0, d, h, w, label, out.data_ptr(), seg_out.data_ptr(), _stream()), "du_pre_crop")
    return out, seg_out, bbox


# ------------------------------------------------------------------------------------------------ normalisation
def _check_image(data, what="data"):
    if not isinstance(data, torch.Tensor) or data.ndim != 4 or data.dtype != torch.float32 or not data.is_contiguous() or data.numel() == 0:
        raise ValueError(f"{what} must be a contiguous float32 (C, D, H, W) tensor (what crop_to_nonzero returns)")


def _plane_stats(data, seg):
    """-> plane_minmax (C D, 2) fp32, chan_stats (C, 5) fp64 on the device (du_pre_plane_stats)"""
    L = _lib.lib()
    C, D, H, W = (int(i) for i in data.shape)
    ws_elems = int(L.du_pre_stats_ws_elems(C, D, H * W))
    if ws_elems == 0:
        raise ValueError(f"at most 65535 channel slices are supported, got {C * D}")
    ws = torch.empty(ws_elems, dtype=torch.float64, device=data.device)
    planes = torch.empty((C * D, 2), dtype=torch.float32, device=data.device)
    chans = torch.empty((C, 5), dtype=torch.float64, device=data.device)
    _lib.check(L.du_pre_plane_stats(data.data_ptr(), None if seg is None else seg.data_ptr(), planes.data_ptr(), chans.data_ptr(), C, D,
                                    H * W, ws.data_ptr(), ws_elems, _stream()), "du_pre_plane_stats")
    return planes, chans, (ws, ws_elems)


def normalize(data, seg, schemes, use_mask_for_norm, intensity_properties):
    """DefaultPreprocessor._normalize (default_preprocessor.py:183-195): channel c of the contiguous fp32 (C, D, H, W) image is normalised
    IN PLACE with schemes[c] (the reference's class names) and returned.  seg (1, D, H, W) int16 as crop_to_nonzero returns it;
    use_mask_for_norm[c] restricts ZScoreNormalization to seg >= 0 and leaves every other voxel as it is; intensity_properties[str(c)]
    holds mean, std, percentile_00_5 and percentile_99_5 for CTNormalization.  NoNormalization, RGBTo01Normalization (ValueError outside
    [0, 255]), CTNormalization and RescaleTo01Normalization are the reference's fp32 operations, equal to the bit; ZScoreNormalization
    is fp32((double(x) - mean) / max(std, 1e-8)) with the population standard deviation, both moments in fp64."""
    _check_image(data)
    C, D, H, W = (int(i) for i in data.shape)
    schemes = list(schemes)
    if len(schemes) != C:
        raise ValueError(f"{len(schemes)} normalisation schemes for {C} channels")
    unknown = [s for s in schemes if s not in _SCHEMES]
    if unknown:
        raise ValueError(f"unknown normalisation scheme {unknown[0]!r}; known: {sorted(_SCHEMES)}")
    codes = [_SCHEMES[s] for s in schemes]
    use_mask = [False] * C if use_mask_for_norm is None else [bool(m) for m in use_mask_for_norm]
    if len(use_mask) != C:
        raise ValueError(f"use_mask_for_norm has {len(use_mask)} entries for {C} channels")
    masked = [codes[c] == NORM_ZSCORE and use_mask[c] for c in range(C)]
    if any(masked):
        if seg is None or seg.dtype != torch.int16 or tuple(seg.shape) != (1, D, H, W) or seg.device != data.device:
            raise ValueError("a masked ZScoreNormalization needs the int16 (1, D, H, W) segmentation of crop_to_nonzero")
        seg = seg.contiguous()
    params = []
    for c in range(C):
        if codes[c] == NORM_CT:
            ip = None if intensity_properties is None else intensity_properties.get(str(c), intensity_properties.get(c))
            if ip is None:
                raise ValueError("CTNormalization requires intensity properties")
            params.append((float(ip["percentile_00_5"]), float(ip["percentile_99_5"]), float(ip["mean"]), max(float(ip["std"]), 1e-8)))
        else:
            params.append((0.0, 0.0, 0.0, 1.0))

    if not data.is_cuda:
        x = data.numpy()
        for c in range(C):
            if codes[c] == NORM_RGB and (x[c].min() < 0 or x[c].max() > 255):
                raise ValueError("RGBTo01Normalization: pixel values outside [0, 255]; the images do not seem to be RGB images")
        for c in range(C):
            _normalize_numpy(x[c], (seg.numpy()[0] >= 0) if masked[c] else None, codes[c], params[c])
        return data

    L = _lib.lib()
    n = D * H * W
    stats = {}
    for with_mask in (False, True):                   # at most two statistics runs: channels with and without the mask
        want = [c for c in range(C) if codes[c] in (NORM_RGB, NORM_RESCALE, NORM_ZSCORE) and masked[c] == with_mask]
        if not want:
            continue
        s = seg if with_mask else None
        _, chans, (ws, ws_elems) = _plane_stats(data, s)
        if any(codes[c] == NORM_ZSCORE for c in want):
            _lib.check(L.du_pre_sq_dev(data.data_ptr(), None if s is None else s.data_ptr(), chans.data_ptr(), C, D, H * W, ws.data_ptr(),
                                       ws_elems, _stream()), "du_pre_sq_dev")
        stats[with_mask] = chans
    rgb = [c for c in range(C) if codes[c] == NORM_RGB]
    if rgb:
        lims = stats[False][:, :2].tolist()                                           # the range check raises on the host
        if any(lims[c][0] < 0 or lims[c][1] > 255 for c in rgb):
            raise ValueError("RGBTo01Normalization: pixel values outside [0, 255]; the images do not seem to be RGB images")
    spare = torch.zeros(5, dtype=torch.float64, device=data.device)
    for c in range(C):
        if codes[c] == NORM_NONE:
            continue
        chans = stats.get(masked[c])
        st = spare if chans is None else chans[c]
        _lib.check(L.du_pre_normalize(data[c].data_ptr(), seg.data_ptr() if masked[c] else None, st.data_ptr(), codes[c], *params[c], n,
                                      _stream()), "du_pre_normalize")
    return data


# ------------------------------------------------------------------------------------------------ resampling
def compute_new_shape(old_shape, old_spacing, new_spacing):
    """default_resampling.py:23-29 (Python's round: halves go to the even integer)"""
    if not len(old_shape) == len(old_spacing) == len(new_spacing):
        raise ValueError("old_shape, old_spacing and new_spacing must have one length")
    return [int(round(i / j * k)) for i, j, k in zip(old_spacing, new_spacing, old_shape)]


def _get_do_separate_z(spacing):
    return (np.max(spacing) / np.min(spacing)) > ANISO_THRESHOLD                      # :13-15


def _get_lowres_axis(spacing):
    return np.where(max(spacing) / np.array(spacing) == 1)[0]                         # :18-20


def _separate_z(current_spacing, new_spacing, force_separate_z):
    """default_resampling.py:90-116 -> (do_separate_z, axis or None)"""
    if force_separate_z is not None:
        do, axis = bool(force_separate_z), (_get_lowres_axis(current_spacing) if force_separate_z else None)
    elif _get_do_separate_z(current_spacing):
        do, axis = True, _get_lowres_axis(current_spacing)
    elif _get_do_separate_z(new_spacing):
        do, axis = True, _get_lowres_axis(new_spacing)
    else:
        do, axis = False, None
    if axis is not None and len(axis) in (2, 3):
        do = False
    return do, axis


def _resize_image(data, out_hw, per_slice):
    """data (C, D, H, W) fp32 -> (C, D, Ho, Wo) fp32: order 3 in-plane, clipped to [min, max] of the channel slice or the channel volume"""
    C, D, H, W = (int(i) for i in data.shape)
    Ho, Wo = out_hw
    if not data.is_cuda:
        x = data.numpy()
        y = _resize_cubic_float64(x, out_hw)
        axes = (2, 3) if per_slice else (1, 2, 3)
        y = np.clip(y, x.min(axis=axes, keepdims=True).astype(np.float64), x.max(axis=axes, keepdims=True).astype(np.float64))
        return torch.from_numpy(y.astype(np.float32))
    planes, chans, _ = _plane_stats(data, None)
    bounds = planes if per_slice else chans[:, None, :2].expand(C, D, 2).to(torch.float32).reshape(C * D, 2).contiguous()
    out = torch.empty((C, D, Ho, Wo), dtype=torch.float32, device=data.device)
    tmp = torch.empty((C * D, H, Wo), dtype=torch.float64, device=data.device) if (Ho != H and Wo != W) else None
    _lib.check(_lib.lib().du_pre_resize_cubic(data.data_ptr(), out.data_ptr(), bounds.data_ptr(), None if tmp is None else tmp.data_ptr(),
                                              C * D, H, W, Ho, Wo, _stream()), "du_pre_resize_cubic")
    return out


def _resize_seg(seg, out_hw):
    """seg (C, D, H, W) int16 -> (C, D, Ho, Wo) int16: the order-1 vote in-plane"""
    C, D, H, W = (int(i) for i in seg.shape)
    Ho, Wo = out_hw
    if not seg.is_cuda:
        return torch.from_numpy(np.stack([_resize_seg_numpy(s, out_hw) for s in seg.numpy()]))
    out = torch.empty((C, D, Ho, Wo), dtype=torch.int16, device=seg.device)
    _lib.check(_lib.lib().du_pre_resize_seg(seg.data_ptr(), out.data_ptr(), C * D, H, W, Ho, Wo, _stream()), "du_pre_resize_seg")
    return out


def resample_data_or_seg_to_shape(data, new_shape, current_spacing, new_spacing, is_seg=False, order=3, order_z=0, force_separate_z=None):
    """default_resampling.py:77-216 for the in-plane case.  data (C, D, H, W): fp32 with is_seg=False, order=3 (skimage's resize, see the
    module docstring) or an integer tensor with is_seg=True, order=1 (resize_segmentation; int16 out); these are the pairs the planner
    emits, any other order raises ValueError.  The clip of order 3 follows the reference's do_separate_z rule with force_separate_z (None
    = decide from the spacings against ANISO_THRESHOLD): exactly one anisotropic axis, and it is axis 0 -> resize runs per slice and
    clips per channel slice; otherwise it runs on the channel volume with z unchanged and clips per channel volume.  new_shape[0] != D
    or a separate-z axis other than 0 raises ValueError; order_z is then never used.  An unchanged shape returns `data` itself."""
    if (bool(is_seg), int(order)) not in ((False, 3), (True, 1)):
        raise ValueError(f"only order 3 for images and order 1 for segmentations are supported, got is_seg={is_seg}, order={order}")
    if not isinstance(data, torch.Tensor) or data.ndim != 4 or data.numel() == 0:
        raise ValueError("data must be a (C, D, H, W) torch tensor")
    new_shape = [int(i) for i in new_shape]
    if len(new_shape) != 3 or len(current_spacing) != 3 or len(new_spacing) != 3:
        raise ValueError("new_shape and the spacings must have three entries")
    if any(s < 1 for s in new_shape):
        raise ValueError(f"empty target shape {new_shape}")
    do_separate_z, axis = _separate_z(list(current_spacing), list(new_spacing), force_separate_z)
    shape = [int(i) for i in data.shape[1:]]
    if shape == new_shape:
        return data                                                                   # :214-216
    if new_shape[0] != shape[0]:
        raise ValueError(f"out-of-plane resampling is not supported: {shape[0]} slices would become {new_shape[0]}")
    if do_separate_z and int(axis[0]) != 0:
        raise ValueError(f"resampling separately along axis {int(axis[0])} is not supported (only in-plane resampling, axis 0 apart)")
    out_hw = (new_shape[1], new_shape[2])
    if is_seg:
        if data.is_floating_point() or data.dtype == torch.bool:
            raise ValueError("a segmentation must be an integer tensor")
        return _resize_seg(data.to(torch.int16).contiguous(), out_hw)
    if data.dtype != torch.float32:
        raise ValueError("the image must be float32")
    return _resize_image(data.contiguous(), out_hw, per_slice=bool(do_separate_z))


# ------------------------------------------------------------------------------------------------ the case
def _check_transpose(transpose_forward):
    tf = [int(i) for i in transpose_forward]
    if sorted(tf) != [0, 1, 2]:
        raise ValueError(f"transpose_forward must be a permutation of (0, 1, 2), got {transpose_forward}")
    return tf


def run_case(data, seg, properties, *, transpose_forward, spacing, normalization_schemes, use_mask_for_norm,
             foreground_intensity_properties_per_channel):
    """DefaultPreprocessor.run_case_npy (default_preprocessor.py:40-118): data (C, X, Y, Z) raw, seg (1, X, Y, Z) or None,
    properties['spacing'] = the raw spacing.  transpose_forward, then crop_to_nonzero, normalize, resample_data_or_seg_to_shape to the
    configuration's `spacing` (two entries for a 2-D configuration: the case's own slice spacing is prepended, :69-72).  Fills
    properties['shape_before_cropping'], ['bbox_used_for_cropping'] and ['shape_after_cropping_and_before_resampling'], which
    export.predict_segmentation reads.  Returns (data fp32 (C, D, H', W'), seg int16 (1, D, H', W')) on the input's device; the inputs
    are not modified.  properties['class_locations'] (:94-111: foreground sampling for training, a host RNG) is filled by
    dataloading.add_class_locations(seg, properties, ...), not here."""
    tf = _check_transpose(transpose_forward)
    if not isinstance(data, torch.Tensor) or data.ndim != 4:
        raise ValueError("data must be a (C, X, Y, Z) torch tensor")
    if seg is not None and (not isinstance(seg, torch.Tensor) or seg.shape[1:] != data.shape[1:]):
        raise ValueError("Shape mismatch between image and segmentation")             # :46
    if "spacing" not in properties or len(properties["spacing"]) != 3:
        raise ValueError("properties['spacing'] must hold the three raw spacings")
    perm = [0, *[i + 1 for i in tf]]
    data = data.permute(*perm)                                                        # :52-54
    seg = None if seg is None else seg.permute(*perm)
    original_spacing = [float(properties["spacing"][i]) for i in tf]
    shape_before_cropping = tuple(int(i) for i in data.shape[1:])
    data, seg, bbox = crop_to_nonzero(data, seg)                                      # :61
    target_spacing = [float(s) for s in spacing]
    if len(target_spacing) < 3:
        target_spacing = [original_spacing[0]] + target_spacing                       # :69-72
    new_shape = compute_new_shape(data.shape[1:], original_spacing, target_spacing)
    if new_shape[0] != data.shape[1]:
        raise ValueError(f"out-of-plane resampling is not supported: {data.shape[1]} slices would become {new_shape[0]}")
    properties["shape_before_cropping"] = shape_before_cropping                       # :59
    properties["bbox_used_for_cropping"] = bbox                                       # :62
    properties["shape_after_cropping_and_before_resampling"] = tuple(int(i) for i in data.shape[1:])      # :64
    data = normalize(data, seg, normalization_schemes, use_mask_for_norm, foreground_intensity_properties_per_channel)     # :79
    data = resample_data_or_seg_to_shape(data, new_shape, original_spacing, target_spacing, is_seg=False, order=3, order_z=0,
                                         force_separate_z=None)                       # :86
    seg = resample_data_or_seg_to_shape(seg, new_shape, original_spacing, target_spacing, is_seg=True, order=1, order_z=0,
                                        force_separate_z=None)                        # :87
    return data, seg


def _configuration(plans, name, visited=()):
    """plans_handler.py:245-267: a configuration with its `inherits_from` chain resolved"""
    if name not in plans["configurations"]:
        raise ValueError(f"the configuration {name} does not exist in the plans; there are {list(plans['configurations'])}")
    conf = dict(plans["configurations"][name])
    parent = conf.get("inherits_from")
    if parent is not None:
        if parent in visited or parent == name:
            raise ValueError(f"circular inherits_from in the plans: {(*visited, name, parent)}")
        base = _configuration(plans, parent, (*visited, name))
        base.update(conf)
        conf = base
    return conf


def _plans_arguments(plans, configuration_name):
    conf = _configuration(plans, configuration_name)
    for key, want in (("resampling_fn_data_kwargs", (False, 3)), ("resampling_fn_seg_kwargs", (True, 1))):
        kw = conf.get(key)
        if kw is not None and (bool(kw.get("is_seg", want[0])), int(kw.get("order", want[1]))) != want:
            raise ValueError(f"{key} = {kw}: only order 3 for the image and order 1 for the segmentation are supported")
        if kw is not None and kw.get("force_separate_z") is not None:
            raise ValueError(f"{key} = {kw}: only force_separate_z = None is supported")
    return dict(transpose_forward=plans["transpose_forward"], spacing=conf["spacing"], normalization_schemes=conf["normalization_schemes"],
                use_mask_for_norm=conf["use_mask_for_norm"],
                foreground_intensity_properties_per_channel=plans.get("foreground_intensity_properties_per_channel"))


def run_case_from_plans(data, seg, properties, plans, configuration_name):
    """run_case with its arguments read from the reference's plans dict (plans.json): transpose_forward and
    foreground_intensity_properties_per_channel from the top level; spacing, normalization_schemes and use_mask_for_norm from
    plans['configurations'][configuration_name], `inherits_from` resolved."""
    return run_case(data, seg, properties, **_plans_arguments(plans, configuration_name))


@torch.no_grad()
def predict_from_raw(net, data, properties, patch_size, *, transpose_forward, spacing, normalization_schemes, use_mask_for_norm,
                     foreground_intensity_properties_per_channel, list_of_parameters=None, **predict_kwargs):
    """Raw array in, label map in the raw geometry out: run_case(data, None, properties, ...), then export.predict_segmentation on the
    preprocessed image with `properties` and transpose_backward = the inverse of transpose_forward.  predict_kwargs are those of
    predict_segmentation (tile_step_size, use_gaussian, batch_size, graph, mirror_axes, regions_class_order, return_probabilities).
    Returns the uint8 label map of data's spatial shape on the network's device (with return_probabilities: and the probabilities).
    Fold ensembles: `net` may be an inference.EnsemblePredictor, or list_of_parameters holds the folds' parameter sets for `net` (a
    predictor is then built for this call; keep one yourself to predict many cases)."""
    from .export import predict_segmentation
    from .inference import EnsemblePredictor
    if list_of_parameters is not None:
        if isinstance(net, EnsemblePredictor):
            raise ValueError("list_of_parameters goes with a network, not with an EnsemblePredictor")
        net = EnsemblePredictor(net, list_of_parameters)
    for k in ("properties", "transpose_backward"):
        if k in predict_kwargs:
            raise ValueError(f"predict_from_raw derives {k} itself")
    tf = _check_transpose(transpose_forward)
    pre, _ = run_case(data, None, properties, transpose_forward=tf, spacing=spacing, normalization_schemes=normalization_schemes,
                      use_mask_for_norm=use_mask_for_norm,
                      foreground_intensity_properties_per_channel=foreground_intensity_properties_per_channel)
    transpose_backward = [tf.index(i) for i in range(3)]
    return predict_segmentation(net, pre, patch_size, properties=properties, transpose_backward=transpose_backward, **predict_kwargs)
