"""The export tail of inference on the MI355X: window sums -> label map in the case's original geometry -> per-case metrics.

Mirrors convert_predicted_logits_to_segmentation_with_correct_shape (dinounet/inference/export_prediction.py:15-68) and the counts and
ratios of compute_metrics (dinounet/evaluation/evaluate_predictions.py:152-234) for the 2D networks of this repo:

    logits (K, D, H, W)  --resample in-plane (order 1, edge clamp, half-pixel centres) to shape_after_cropping_and_before_resampling-->
    softmax + argmax | sigmoid + region paint loop (label_handling.py:128-175)  --paste at bbox_used_for_cropping into
    shape_before_cropping (:44-48)-->  transpose_backward (:52)

On the GPU all of it is ONE HIP pass (csrc/export.hip: du_export_seg) over the accumulators of the window loop: the positive factor
1 / n_predictions cannot change a label, so without resampling the raw sums are compared and the normalised logits never exist; with
resampling they exist at four taps per output pixel only.  One uint8 volume crosses to the host instead of K fp32 volumes.  The counts
are a second integer kernel (du_seg_counts).  CPU tensors take a torch restatement that interpolates in float64 with the same integer
source positions; it is what the tests compare the kernel against.

The surface metrics of that table, HD95 and ASD (compute_surface_distances, evaluate_predictions.py:97-149: medpy.metric.hd95 / asd),
are computed on the device as well (csrc/surface.hip): the border voxels of every label or region of both maps, an exact separable
Euclidean distance transform of the complement of each border set in squared fp64 distances, and its values at the other map's border
voxels compacted per region and direction.  Only two order statistics and one sum per region cross to the host.  CPU tensors take the
medpy formula written with scipy.ndimage and numpy.percentile.

Differences from the reference, on purpose: a region is predicted where logit > 0 (the reference: torch's fp32 sigmoid(x) > 0.5; they
differ only for 0 < x < ~1.2e-7); the resampling is in-plane only (shape_after_cropping_and_before_resampling[0] must
be the number of slices); label maps are uint8 (at most 254 foreground labels; the reference switches to uint16 at 255, :46); the surface
metrics need a spacing of three positive floats (the reference's "pad or trim the spacing" branches are not mirrored) and volumes of at most
1024 voxels per axis."""
import math

import torch

from . import _lib

MAX_CLASSES = 8                     # du_export_seg: K in [2, 8] (softmax) / R in [1, 8] (regions); du_seg_counts: R <= 8 per launch
EXPORT_SOFTMAX, EXPORT_REGIONS = 0, 1


def source_taps(n_src, n_dst, device="cpu"):
    """Order-1 source positions of `n_dst` output pixels over `n_src` input pixels with half-pixel centres
    (src = (dst + 0.5) * n_src / n_dst - 0.5), from integers: n = (2 dst + 1) n_src - n_dst, lower tap floor(n / (2 n_dst)), weight of the
    upper tap (n mod 2 n_dst) / (2 n_dst); taps clamped to the edge.  Returns (lower int64, upper int64, weight float64)."""
    dst = torch.arange(n_dst, dtype=torch.int64, device=device)
    n = (2 * dst + 1) * n_src - n_dst
    den = 2 * n_dst
    lo = torch.div(n, den, rounding_mode="floor")
    w = (n - lo * den).to(torch.float64) / float(den)
    return lo.clamp(0, n_src - 1), (lo + 1).clamp(0, n_src - 1), w


def resize_inplane_float64(x, size):
    """x (..., H, W) -> float64 (..., Ho, Wo): order-1 interpolation at source_taps.  What scipy.ndimage.zoom(order=1, mode='nearest',
    grid_mode=True) and skimage.transform.resize(order=1, mode='edge', anti_aliasing=False) compute."""
    x = x.to(torch.float64)
    ya, yb, wy = source_taps(x.shape[-2], int(size[0]), x.device)
    xa, xb, wx = source_taps(x.shape[-1], int(size[1]), x.device)
    left, right = x.index_select(-1, xa), x.index_select(-1, xb)
    rows = left + wx * (right - left)
    top, bot = rows.index_select(-2, ya), rows.index_select(-2, yb)
    return top + wy[:, None] * (bot - top)


def _geometry(shape, properties):
    """(D, H, W) of the logits and the reference's properties dict -> (Ho, Wo), (D0, H0, W0), (bd, by, bx); ValueError if they do not fit"""
    D, H, W = (int(i) for i in shape)
    if properties is None:
        return (H, W), (D, H, W), (0, 0, 0)
    after = [int(i) for i in properties["shape_after_cropping_and_before_resampling"]]
    before = [int(i) for i in properties["shape_before_cropping"]]
    bbox = [[int(i) for i in b] for b in properties["bbox_used_for_cropping"]]
    if len(after) != 3 or len(before) != 3 or len(bbox) != 3:
        raise ValueError("properties must describe a (D, H, W) volume")
    if after[0] != D:
        raise ValueError(f"out-of-plane resampling is not supported: shape_after_cropping_and_before_resampling[0] = {after[0]} "
                         f"but the logits have {D} slices (only the two in-plane axes are resampled)")
    if any(a <= 0 for a in after) or any(b <= 0 for b in before):
        raise ValueError("properties hold an empty shape")
    for ax in range(3):
        lo, hi = bbox[ax]
        if lo < 0 or hi > before[ax] or hi - lo != after[ax]:
            raise ValueError(f"bbox_used_for_cropping {bbox} does not fit: axis {ax} needs 0 <= lo, hi <= {before[ax]} and "
                             f"hi - lo == {after[ax]}")
    return (after[1], after[2]), tuple(before), tuple(b[0] for b in bbox)


def _check_heads(K, regions_class_order):
    if regions_class_order is None:
        if not 2 <= K <= MAX_CLASSES:
            raise ValueError(f"softmax export supports 2..{MAX_CLASSES} classes, got {K}")
        return None
    order = [int(c) for c in regions_class_order]
    if not 1 <= K <= MAX_CLASSES:
        raise ValueError(f"region export supports 1..{MAX_CLASSES} regions, got {K}")
    if len(order) != K:
        raise ValueError(f"regions_class_order has {len(order)} entries for {K} region logits")
    if any(c < 0 or c > 254 for c in order):
        raise ValueError("label maps are uint8: more than 254 labels are not supported")
    return order


def _permute(seg, probs, transpose_backward):
    if transpose_backward is not None:
        tb = [int(i) for i in transpose_backward]
        if sorted(tb) != [0, 1, 2]:
            raise ValueError(f"transpose_backward must be a permutation of (0, 1, 2), got {transpose_backward}")
        seg = seg.permute(*tb)                                                       # export_prediction.py:52
        if probs is not None:
            probs = probs.permute(0, *[i + 1 for i in tb])                           # :62-63
    return seg, probs


def _export_torch(sums, npred, window, order, out_hw, before, corner, want_probs):
    """the restatement: same semantics as du_export_seg, interpolation and probabilities in float64"""
    y0, x0, Hc, Wc = window
    x = sums[:, :, y0:y0 + Hc, x0:x0 + Wc]
    n = None if npred is None else npred[:, y0:y0 + Hc, x0:x0 + Wc]
    finite = bool(torch.isfinite(x).all()) and (n is None or bool(torch.isfinite(n).all()))
    resample = tuple(out_hw) != (Hc, Wc)
    if resample or want_probs:
        z = x.to(torch.float64) if n is None else x.to(torch.float64) / n.to(torch.float64)
        if resample:
            z = resize_inplane_float64(z, out_hw)
    dec = z if resample else x                       # no resampling: the raw sums decide (no arithmetic on them)
    if order is None:
        lab = dec.argmax(0).to(torch.uint8)
    else:
        lab = torch.zeros(dec.shape[1:], dtype=torch.uint8, device=dec.device)
        for i, c in enumerate(order):                # label_handling.py:170-171
            lab[dec[i] > 0] = c
    D, (Ho, Wo) = x.shape[1], out_hw
    sl = (slice(corner[0], corner[0] + D), slice(corner[1], corner[1] + Ho), slice(corner[2], corner[2] + Wo))
    seg = torch.zeros(before, dtype=torch.uint8, device=sums.device)
    seg[sl] = lab
    probs = None
    if want_probs:
        p = torch.softmax(z, 0) if order is None else torch.sigmoid(z)
        probs = torch.zeros((x.shape[0], *before), dtype=torch.float32, device=sums.device)
        if order is None:
            probs[0] = 1                             # label_handling.py:204-205
        probs[(slice(None), *sl)] = p.to(torch.float32)
    return seg, probs, finite


def _export_hip(sums, npred, window, order, out_hw, before, corner, want_probs, flag=None):
    """flag: a zeroed int32 element on the device that the caller reads back itself (the cases path reads a group's flags in one copy);
    None = read here"""
    K, D, Hp, Wp = sums.shape
    y0, x0, Hc, Wc = window
    dev = sums.device
    seg = torch.empty(before, dtype=torch.uint8, device=dev)
    probs = torch.empty((K, *before), dtype=torch.float32, device=dev) if want_probs else None
    deferred = flag is not None
    if not deferred:
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
    packed = 0 if order is None else _signed64(sum(c << (8 * i) for i, c in enumerate(order)))
    _lib.check(_lib.lib().du_export_seg(sums.data_ptr(), None if npred is None else npred.data_ptr(), seg.data_ptr(),
                                        None if probs is None else probs.data_ptr(), flag.data_ptr(), K, D, Hp, Wp, y0, x0, Hc, Wc,
                                        out_hw[0], out_hw[1], before[0], before[1], before[2], corner[0], corner[1], corner[2],
                                        EXPORT_SOFTMAX if order is None else EXPORT_REGIONS, packed,
                                        torch.cuda.current_stream().cuda_stream), "du_export_seg")
    return seg, probs, deferred or int(flag.item()) == 0


def _export(sums, npred, window, regions_class_order, properties, transpose_backward, return_probabilities, flag=None):
    if sums.ndim != 4:
        raise ValueError("logits must be (K, D, H, W)")
    if sums.dtype != torch.float32:
        raise ValueError("logits must be float32")
    order = _check_heads(sums.shape[0], regions_class_order)
    if npred is not None and (npred.dtype != torch.float32 or tuple(npred.shape) != tuple(sums.shape[1:]) or npred.device != sums.device):
        raise ValueError("npred must be float32 (D, H, W) next to the sums")
    D = sums.shape[1]
    out_hw, before, corner = _geometry((D, window[2], window[3]), properties)
    sums = sums.contiguous()
    npred = None if npred is None else npred.contiguous()
    if flag is not None and sums.is_cuda:
        seg, probs, finite = _export_hip(sums, npred, window, order, out_hw, before, corner, return_probabilities, flag)
    else:
        run = _export_hip if sums.is_cuda else _export_torch
        seg, probs, finite = run(sums, npred, window, order, out_hw, before, corner, return_probabilities)
    if not finite:
        raise RuntimeError("Encountered inf in predicted array")                     # predict_from_raw_data.py:612-615
    seg, probs = _permute(seg, probs, transpose_backward)
    return (seg, probs) if return_probabilities else seg


@torch.no_grad()
def logits_to_segmentation(logits_or_sums, npred=None, *, regions_class_order=None, properties=None, transpose_backward=None,
                           return_probabilities=False):
    """Functional form of convert_predicted_logits_to_segmentation_with_correct_shape (export_prediction.py:15-68).
    logits_or_sums (K, D, H, W) fp32: finished logits, or with npred (D, H, W) the un-normalised window sums (logits = sums / npred).
    regions_class_order: None = softmax heads (argmax), else the label painted for each region logit, in order (label_handling.py:170).
    properties: the reference's dict (shape_before_cropping, bbox_used_for_cropping, shape_after_cropping_and_before_resampling); None =
    no crop, no resampling.  Returns the uint8 label map on the input's device, permuted by transpose_backward; with
    return_probabilities also the fp32 probabilities (K, ...), permuted likewise.  CUDA tensors run du_export_seg, CPU tensors the
    float64 torch restatement."""
    H, W = logits_or_sums.shape[-2:]
    return _export(logits_or_sums, npred, (0, 0, int(H), int(W)), regions_class_order, properties, transpose_backward,
                   return_probabilities)


@torch.no_grad()
def predict_segmentation(net, data, patch_size, tile_step_size=0.5, use_gaussian=True, batch_size=8, graph=False, mirror_axes=None, *,
                         regions_class_order=None, properties=None, transpose_backward=None, return_probabilities=False):
    """predict_sliding_window_logits + logits_to_segmentation without the logits in between: the window loop of
    inference.predict_sliding_window_logits, then ONE pass from the accumulators (still padded, not divided) to the label map -- no
    normalise, isfinite or slice pass over the K planes."""
    from . import inference
    assert data.ndim == 4, "input_image must be a 4D tensor (c, d, y, x)"
    out = [None]
    sink = inference._segmentation_sink(out, regions_class_order, None if properties is None else [properties], transpose_backward,
                                        return_probabilities, named=False)
    inference._accumulate_cases(net, [data], patch_size, tile_step_size, use_gaussian, batch_size, graph, mirror_axes, sink)
    return out[0]


def _region_mask_bits(region_or_label):
    labels = region_or_label if isinstance(region_or_label, (tuple, list)) else (region_or_label,)
    bits = 0
    for l in labels:
        l = int(l)
        if 0 <= l < 64:                              # du_labels_to_regions convention: any other label is in no region
            bits |= 1 << l
    return bits


def _signed64(v):
    return v - (1 << 64) if v >= (1 << 63) else v


def _counts_torch(pred, ref, masks, ignore_label):
    valid = torch.ones_like(ref, dtype=torch.bool) if ignore_label is None else ref != ignore_label
    rows = []
    for bits in masks:
        labels = [l for l in range(64) if (bits >> l) & 1]
        mp, mr = torch.zeros_like(valid), torch.zeros_like(valid)
        for l in labels:                             # region_or_label_to_mask, evaluate_predictions.py:75-82
            mp |= pred == l
            mr |= ref == l
        rows.append([int((mr & mp & valid).sum()), int((~mr & mp & valid).sum()), int((mr & ~mp & valid).sum()),
                     int((~mr & ~mp & valid).sum())])
    return torch.tensor(rows, dtype=torch.int64).t().contiguous()          # (4, R)


def _counts_hip(pred, ref, masks, ignore_label):
    L = _lib.lib()
    dev, n = pred.device, pred.numel()
    st = torch.cuda.current_stream().cuda_stream
    out = []
    for i0 in range(0, len(masks), MAX_CLASSES):
        chunk = masks[i0:i0 + MAX_CLASSES]
        R = len(chunk)
        table = torch.tensor(chunk, dtype=torch.int64).to(dev)
        counts = torch.empty((4, R), dtype=torch.int64, device=dev)
        ws_elems = int(L.du_seg_counts_ws_elems(n, R))
        ws = torch.empty(max(ws_elems, 1), dtype=torch.int32, device=dev)
        _lib.check(L.du_seg_counts(pred.data_ptr(), ref.data_ptr(), table.data_ptr(), counts.data_ptr(), n, R,
                                   0 if ignore_label is None else 1, 0 if ignore_label is None else int(ignore_label), ws.data_ptr(),
                                   ws_elems, st), "du_seg_counts")
        out.append(counts)
    return torch.cat(out, 1).cpu()


def segmentation_counts(seg_pred, seg_ref, labels_or_regions, ignore_label=None):
    """(4, R) int64 on the host = tp | fp | fn | tn of every label or region over the voxels whose reference label is not the ignore label
    (compute_tp_fp_fn_tn with region_or_label_to_mask, evaluate_predictions.py:75-94, 176-186).  uint8 label maps of one shape and
    device; CUDA tensors run du_seg_counts (8 regions per launch), CPU tensors torch."""
    if seg_pred.dtype != torch.uint8 or seg_ref.dtype != torch.uint8:
        raise ValueError("label maps must be uint8")
    if seg_pred.shape != seg_ref.shape or seg_pred.device != seg_ref.device:
        raise ValueError("prediction and reference must have one shape and device")
    if seg_pred.numel() == 0 or len(labels_or_regions) == 0:
        raise ValueError("empty label map or no labels")
    masks = [_region_mask_bits(r) for r in labels_or_regions]
    if seg_pred.is_cuda:
        return _counts_hip(seg_pred.contiguous().view(-1), seg_ref.contiguous().view(-1), [_signed64(m) for m in masks], ignore_label)
    return _counts_torch(seg_pred, seg_ref, masks, ignore_label)


def case_metrics(seg_pred, seg_ref, labels_or_regions, ignore_label=None, spacing=None):
    """The `metrics` dict of compute_metrics (evaluate_predictions.py:176-234) for one case: per label or region (the key, as given; lists
    become tuples) Dice, IoU, Sensitivity, Specificity, Precision, FP, TP, FN, TN, n_pred, n_ref with the nan rules of :189-210.  The
    counts are exact integers from the device; the ratios are float64 on the host.  With `spacing` (three positive floats in the axis
    order of the (D, H, W) maps) HD95 and ASD of surface_metrics follow Precision, where the reference puts them (:225-226); the ignore
    label plays no part in them."""
    counts = segmentation_counts(seg_pred, seg_ref, labels_or_regions, ignore_label).tolist()
    surface = None if spacing is None else surface_metrics(seg_pred, seg_ref, labels_or_regions, spacing)
    nan = float("nan")
    metrics = {}
    for i, r in enumerate(labels_or_regions):
        tp, fp, fn, tn = (counts[j][i] for j in range(4))
        m = {}
        m["Dice"] = 2 * tp / (2 * tp + fp + fn) if tp + fp + fn > 0 else nan          # :189-194
        m["IoU"] = tp / (tp + fp + fn) if tp + fp + fn > 0 else nan
        m["Sensitivity"] = tp / (tp + fn) if tp + fn > 0 else nan                     # :197-200
        m["Specificity"] = tn / (tn + fp) if tn + fp > 0 else nan                     # :202-205
        m["Precision"] = tp / (tp + fp) if tp + fp > 0 else nan                       # :207-210
        if surface is not None:
            sm = surface[tuple(r) if isinstance(r, list) else r]
            m["HD95"], m["ASD"] = sm["HD95"], sm["ASD"]                                # :225-226
        m["FP"], m["TP"], m["FN"], m["TN"] = fp, tp, fn, tn                           # :229-232
        m["n_pred"], m["n_ref"] = fp + tp, fn + tp                                    # :233-234
        metrics[tuple(r) if isinstance(r, list) else r] = m
    return metrics


# ------------------------------------------------------------------------------------------------ surface metrics: HD95 / ASD
SURFACE_MAX_EXTENT = 1024           # csrc/surface.hip: indices and offsets are 10-bit fields


def _check_spacing(spacing):
    try:
        sp = tuple(float(v) for v in spacing)
    except TypeError:
        raise ValueError("spacing must be three positive floats in array-axis order") from None
    if len(sp) != 3 or not all(math.isfinite(v) and 0.0 < v < 1e100 for v in sp):
        raise ValueError(f"spacing must be three positive floats in array-axis order, got {spacing}")
    return sp


def _check_volume(seg):
    if seg.ndim != 3:
        raise ValueError("label maps must be (D, H, W); a 2-D case has D == 1")
    if seg.is_cuda and any(int(e) > SURFACE_MAX_EXTENT for e in seg.shape):
        raise ValueError(f"surface metrics on the device support at most {SURFACE_MAX_EXTENT} voxels per axis, got {tuple(seg.shape)}")


def _mask_numpy(seg, bits):
    """region_or_label_to_mask (evaluate_predictions.py:75-82) with the bit-mask convention of _region_mask_bits"""
    import numpy as np
    return np.isin(seg, [l for l in range(64) if (bits >> l) & 1])


def _border_numpy(mask):
    """medpy.metric.binary.__surface_distances: mask ^ binary_erosion(mask, generate_binary_structure(ndim, 1)) (border_value 0)"""
    from scipy import ndimage
    return mask ^ ndimage.binary_erosion(mask, structure=ndimage.generate_binary_structure(mask.ndim, 1), iterations=1)


def _dist_sq_numpy(border, spacing):
    """distance_transform_edt(~border, sampling=spacing) ** 2 without the root: the squared offsets to scipy's nearest border voxel, times
    the spacing, squared and added in axis order -- the arithmetic scipy itself does before its sqrt.  inf without a border voxel."""
    import numpy as np
    from scipy import ndimage
    if not border.any():
        return np.full(border.shape, np.inf)
    idx = ndimage.distance_transform_edt(~border, sampling=spacing, return_distances=False, return_indices=True)
    d2 = np.zeros(border.shape, dtype=np.float64)
    for ax in range(border.ndim):
        off = (idx[ax] - np.arange(border.shape[ax]).reshape([-1 if a == ax else 1 for a in range(border.ndim)])).astype(np.float64)
        off *= spacing[ax]
        d2 += off * off
    return d2


def _surface_scipy(pred, ref, bits, spacing):
    """medpy.metric.hd95(pred, ref, spacing) and medpy.metric.asd(pred, ref, spacing) for one region, restated from their published
    behaviour: hd95 = percentile(hstack((d_pr, d_rp)), 95), asd = d_pr.mean(), d_pr = the distance field of ref's border at pred's border."""
    import numpy as np
    from scipy import ndimage
    mp, mr = _mask_numpy(pred, bits), _mask_numpy(ref, bits)
    bp, br = _border_numpy(mp), _border_numpy(mr)
    out = {"HD95": float("nan"), "ASD": float("nan"), "n_surface_pred": int(bp.sum()), "n_surface_ref": int(br.sum())}
    if not mp.any() or not mr.any():                                                  # evaluate_predictions.py:117-118
        return out
    d_pr = ndimage.distance_transform_edt(~br, sampling=spacing)[bp]
    d_rp = ndimage.distance_transform_edt(~bp, sampling=spacing)[br]
    out["HD95"] = float(np.percentile(np.hstack((d_pr, d_rp)), 95))
    out["ASD"] = float(d_pr.mean())
    return out


def _lerp(a, b, t):
    """numpy's _lerp (lib/_function_base_impl.py), the interpolation of numpy.percentile(method='linear')"""
    d = b - a
    return b - d * (1 - t) if t >= 0.5 else a + d * t


def _surface_border_hip(pred, ref, chunk):
    """-> bits (D, H, W) int16 view of the uint16 border bit sets, counts (4, R) int64 on the device"""
    L = _lib.lib()
    D, H, W = (int(i) for i in pred.shape)
    dev, R = pred.device, len(chunk)
    st = torch.cuda.current_stream().cuda_stream
    table = torch.tensor([_signed64(m) for m in chunk], dtype=torch.int64).to(dev)
    bits = torch.empty((D, H, W), dtype=torch.int16, device=dev)
    counts = torch.empty((4, R), dtype=torch.int64, device=dev)
    ws_elems = int(L.du_surface_border_ws_elems(D * H * W, R))
    ws = torch.empty(max(ws_elems, 1), dtype=torch.int32, device=dev)
    _lib.check(L.du_surface_border(pred.data_ptr(), ref.data_ptr(), table.data_ptr(), bits.data_ptr(), counts.data_ptr(), D, H, W, R,
                                   ws.data_ptr(), ws_elems, st), "du_surface_border")
    return bits, counts


def _surface_ws(shape, dev):
    D, H, W = (int(i) for i in shape)
    ws_elems = int(_lib.lib().du_surface_ws_elems(D, H, W))
    return torch.empty(max(ws_elems, 1), dtype=torch.float64, device=dev), ws_elems


def _surface_hip(pred, ref, masks, spacing):
    import ctypes
    L = _lib.lib()
    D, H, W = (int(i) for i in pred.shape)
    dev = pred.device
    st = torch.cuda.current_stream().cuda_stream
    ws, ws_elems = _surface_ws(pred.shape, dev)
    out = []
    for i0 in range(0, len(masks), MAX_CLASSES):
        chunk = masks[i0:i0 + MAX_CLASSES]
        R = len(chunk)
        bits, counts = _surface_border_hip(pred, ref, chunk)
        n_pred, n_ref, nb_pred, nb_ref = counts.tolist()                              # synchronisation 1 of 2: segment sizes
        active = [r for r in range(R) if n_pred[r] > 0 and n_ref[r] > 0]
        rows = [{"HD95": float("nan"), "ASD": float("nan"), "n_surface_pred": nb_pred[r], "n_surface_ref": nb_ref[r]} for r in range(R)]
        out.extend(rows)
        if not active:
            continue
        off = [0]
        for r in range(R):
            on = r in active
            off.append(off[-1] + (nb_pred[r] if on else 0))
            off.append(off[-1] + (nb_ref[r] if on else 0))
        seg_off = (ctypes.c_int64 * (2 * R + 1))(*off)
        dist_sq = torch.empty(off[-1], dtype=torch.float64, device=dev)
        sums = torch.zeros(R, dtype=torch.float64, device=dev)
        _lib.check(L.du_surface_gather(bits.data_ptr(), D, H, W, R, sum(1 << r for r in active), spacing[0], spacing[1], spacing[2],
                                       ctypes.addressof(seg_off), dist_sq.data_ptr(), sums.data_ptr(), ws.data_ptr(), ws_elems, st),
                   "du_surface_gather")
        # the two order statistics around numpy's virtual index 0.95 (n - 1) of hstack((d_pr, d_rp)): both segments of a region are adjacent
        picks = []
        for r in active:
            n = off[2 * r + 2] - off[2 * r]
            lo = math.floor((n - 1) * 0.95)
            srt = torch.sort(dist_sq[off[2 * r]:off[2 * r + 2]]).values
            picks.append(srt[torch.tensor([lo, min(lo + 1, n - 1)], device=dev)])
        got = torch.cat(picks + [sums]).tolist()                                      # synchronisation 2 of 2
        for j, r in enumerate(active):
            n = off[2 * r + 2] - off[2 * r]
            vi = (n - 1) * 0.95
            a, b = math.sqrt(got[2 * j]), math.sqrt(got[2 * j + 1])
            rows[r]["HD95"] = float(_lerp(a, b, vi - math.floor(vi)))
            rows[r]["ASD"] = got[2 * len(active) + r] / nb_pred[r]
    return out


def _check_pair(seg_pred, seg_ref, labels_or_regions):
    if seg_pred.dtype != torch.uint8 or seg_ref.dtype != torch.uint8:
        raise ValueError("label maps must be uint8")
    if seg_pred.shape != seg_ref.shape or seg_pred.device != seg_ref.device:
        raise ValueError("prediction and reference must have one shape and device")
    if seg_pred.numel() == 0 or len(labels_or_regions) == 0:
        raise ValueError("empty label map or no labels")


def surface_metrics(seg_pred, seg_ref, labels_or_regions, spacing):
    """HD95 and ASD of compute_surface_distances (evaluate_predictions.py:97-149) for every label or region: {key: {"HD95", "ASD",
    "n_surface_pred", "n_surface_ref"}}, keys as in case_metrics.  uint8 (D, H, W) label maps of one shape and device (2-D data: D == 1,
    where every mask voxel is a border voxel, as in the reference); spacing: three positive floats in array-axis order.  Either mask empty:
    both nan (:117-118).  HD95 = numpy.percentile(hstack((d_pr, d_rp)), 95), ASD = d_pr.mean() (prediction to reference only, as
    medpy.metric.asd).  CUDA tensors run csrc/surface.hip, 8 regions per chunk and two synchronisations per chunk, at most 1024 voxels
    per axis; CPU tensors the scipy restatement."""
    _check_pair(seg_pred, seg_ref, labels_or_regions)
    _check_volume(seg_pred)
    sp = _check_spacing(spacing)
    masks = [_region_mask_bits(r) for r in labels_or_regions]
    if seg_pred.is_cuda:
        rows = _surface_hip(seg_pred.contiguous(), seg_ref.contiguous(), masks, sp)
    else:
        p, g = seg_pred.numpy(), seg_ref.numpy()
        rows = [_surface_scipy(p, g, m, sp) for m in masks]
    return {(tuple(r) if isinstance(r, list) else r): row for r, row in zip(labels_or_regions, rows)}


def border_distance_sq(seg, region_or_label, spacing):
    """(border bool (D, H, W), dist_sq float64 (D, H, W)) on seg's device: the border voxels of one label or region of a uint8 label map
    (mask voxels with a face neighbour outside the mask or the volume) and the squared Euclidean distance (dz sz)^2 + (dy sy)^2 + (dx sx)^2
    of every voxel to the nearest of them, inf if there is none."""
    if seg.dtype != torch.uint8:
        raise ValueError("label maps must be uint8")
    if seg.numel() == 0:
        raise ValueError("empty label map")
    _check_volume(seg)
    sp = _check_spacing(spacing)
    m = _region_mask_bits(region_or_label)
    if not seg.is_cuda:
        border = _border_numpy(_mask_numpy(seg.numpy(), m))
        return torch.from_numpy(border), torch.from_numpy(_dist_sq_numpy(border, sp))
    seg = seg.contiguous()
    D, H, W = (int(i) for i in seg.shape)
    bits, _ = _surface_border_hip(seg, seg, [m])
    ws, ws_elems = _surface_ws(seg.shape, seg.device)
    field = torch.empty((D, H, W), dtype=torch.float64, device=seg.device)
    _lib.check(_lib.lib().du_surface_field(bits.data_ptr(), field.data_ptr(), D, H, W, 0, sp[0], sp[1], sp[2], ws.data_ptr(), ws_elems,
                                           torch.cuda.current_stream().cuda_stream), "du_surface_field")
    return (bits & 1).bool(), field
