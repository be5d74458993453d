"""Postprocessing on the MI355X: connected components of a label map, "keep only the largest component", and the search that decides
where doing so raises the mean Dice.

Mirrors dinounet/postprocessing/remove_connected_components.py: remove_all_but_largest_component_from_segmentation (:22-34),
apply_postprocessing (:37-40) and determine_postprocessing (:53-245), the last over two lists of label maps instead of two folders (no
files, pool or reader/writer).  The reference labels through acvl_utils.morphology.morphology_helper.remove_all_but_largest_component(mask)
with connectivity=None, which reaches skimage.measure.label(connectivity=None): full connectivity, 26 neighbours on the 3-D seg[0].  Neither
package is vendored by the reference or pinned, so that published behaviour is restated here:

    mask      = union over labels_or_regions of region_or_label_to_mask (the 64-bit mask convention of export._region_mask_bits)
    component = 26-connected set of mask voxels (8 in-plane with D == 1); its id = the smallest linear index (z H + y) W + x of its voxels
    largest   = the maximum voxel count; on a tie the smallest id, i.e. the first component in raster order: what
                [ids[np.argmax(sizes)]] over skimage's raster-ordered labels keeps
    out       = background_label where a voxel is in the mask but not in the largest component, else the input

CUDA tensors run csrc/cc.hip (tile-local union-find in LDS, a global merge over tile faces, flatten, select, apply: DESIGN section 3d); the
label map never leaves the device and nothing is read back to choose the component.  CPU tensors run the restatement with
scipy.ndimage.label(mask, structure=np.ones((3, 3, 3))), np.bincount and the explicit tie rule; the GPU tests compare against that path.

Differences from the reference, on purpose: label maps are uint8 (D, H, W) torch tensors (2-D data: D == 1; no leading channel axis);
labels above 63 are in no mask; D H W < 2^31; an EMPTY mask returns a copy of the input (the reference raises from np.argmax of an empty
list); determine_postprocessing reports Dice only (the only metric the search reads), and its `report` is the dict the reference writes
to postprocessing.json, returned instead of saved."""
import warnings

import numpy as np
import torch

from . import _lib
from .export import _mask_numpy, _region_mask_bits, _signed64, segmentation_counts

MAX_VOXELS = 1 << 31                # csrc/cc.hip: voxel indices are int32


def _as_list(labels_or_regions):
    return labels_or_regions if isinstance(labels_or_regions, list) else [labels_or_regions]      # :27-28


def _mask_bits(labels_or_regions):
    """OR of the masks of every element: a Python list means "the union of these labels / regions" (:26-30)"""
    bits = 0
    for l_or_r in _as_list(labels_or_regions):
        bits |= _region_mask_bits(l_or_r)
    return bits


def _check_seg(seg, labels_or_regions):
    if not isinstance(seg, torch.Tensor) or seg.dtype != torch.uint8:
        raise ValueError("label maps must be uint8 torch tensors")
    if seg.ndim != 3:
        raise ValueError("label maps must be (D, H, W); a 2-D case has D == 1")
    if seg.numel() == 0:
        raise ValueError("empty label map")
    if seg.numel() >= MAX_VOXELS:
        raise ValueError(f"connected components support fewer than 2^31 voxels, got {tuple(seg.shape)}")
    if isinstance(labels_or_regions, (list, tuple)) and len(labels_or_regions) == 0:
        raise ValueError("labels_or_regions is empty")


def _components_numpy(mask):
    """mask bool (D, H, W) -> ids int32 (component id = smallest linear index, -1 outside), stats dict"""
    from scipy import ndimage
    lab, k = ndimage.label(mask, structure=np.ones((3, 3, 3), dtype=bool))
    ids = np.full(mask.shape, -1, dtype=np.int32)
    if k == 0:
        return ids, {"n_components": 0, "largest_size": 0, "largest_id": -1}
    flat = lab.ravel()
    pos = np.flatnonzero(flat)
    first = np.zeros(k + 1, dtype=np.int64)
    first[flat[pos][::-1]] = pos[::-1]                      # repeated index: the last assignment stays = the smallest position
    sizes = np.bincount(flat, minlength=k + 1)
    ids.ravel()[pos] = first[flat[pos]]
    largest = int(sizes[1:].max())
    best = int(first[1:][sizes[1:] == largest].min())       # most voxels, then the smallest id
    return ids, {"n_components": int(k), "largest_size": largest, "largest_id": best}


def _ws(shape, keep, dev):
    D, H, W = (int(i) for i in shape)
    ws_elems = int(_lib.lib().du_cc_ws_elems(D, H, W, keep))
    return torch.empty(max(ws_elems, 4), dtype=torch.int32, device=dev), ws_elems


def _stats_dict(stats):
    n, size, cid = stats.tolist()
    return {"n_components": n, "largest_size": size, "largest_id": cid}


def component_ids(seg, labels_or_regions):
    """Connected components (26 neighbours) of the mask `labels_or_regions` of a uint8 (D, H, W) label map: (ids int32 (D, H, W) on seg's
    device: the smallest linear index of the voxel's component, -1 outside the mask; {"n_components", "largest_size", "largest_id"},
    largest_id -1 for an empty mask).  CUDA tensors run du_cc_label, CPU tensors the scipy restatement."""
    _check_seg(seg, labels_or_regions)
    bits = _mask_bits(labels_or_regions)
    if not seg.is_cuda:
        ids, stats = _components_numpy(_mask_numpy(seg.numpy(), bits))
        return torch.from_numpy(ids), stats
    seg = seg.contiguous()
    D, H, W = (int(i) for i in seg.shape)
    ids = torch.empty((D, H, W), dtype=torch.int32, device=seg.device)
    stats = torch.empty(3, dtype=torch.int64, device=seg.device)
    ws, ws_elems = _ws(seg.shape, 0, seg.device)
    _lib.check(_lib.lib().du_cc_label(seg.data_ptr(), _signed64(bits), ids.data_ptr(), stats.data_ptr(), D, H, W, ws.data_ptr(), ws_elems,
                                      torch.cuda.current_stream().cuda_stream), "du_cc_label")
    return ids, _stats_dict(stats)


def remove_all_but_largest_component_from_segmentation(segmentation, labels_or_regions, background_label=0):
    """remove_connected_components.py:22-34 for a uint8 (D, H, W) torch tensor: a new tensor on the same device in which every voxel of the
    mask (a label, a region tuple, or a list of those = their union) outside the mask's largest 26-connected component is
    background_label; everything else, labels outside the mask included, is copied.  The input is not modified.  An empty mask gives an
    equal copy.  CUDA tensors run du_cc_keep_largest without a synchronisation, CPU tensors the scipy restatement."""
    _check_seg(segmentation, labels_or_regions)
    bg = int(background_label)
    if not 0 <= bg <= 255:
        raise ValueError(f"background_label must be in 0..255 (uint8 label maps), got {background_label}")
    bits = _mask_bits(labels_or_regions)
    if not segmentation.is_cuda:
        seg = segmentation.numpy()
        mask = _mask_numpy(seg, bits)
        ids, stats = _components_numpy(mask)
        ret = np.copy(seg)                                                            # do not modify the input (:32)
        ret[mask & (ids != stats["largest_id"])] = bg                                 # :33
        return torch.from_numpy(ret)
    seg = segmentation.contiguous()
    D, H, W = (int(i) for i in seg.shape)
    out = torch.empty((D, H, W), dtype=torch.uint8, device=seg.device)
    stats = torch.empty(3, dtype=torch.int64, device=seg.device)
    ws, ws_elems = _ws(seg.shape, 1, seg.device)
    _lib.check(_lib.lib().du_cc_keep_largest(seg.data_ptr(), _signed64(bits), bg, out.data_ptr(), stats.data_ptr(), D, H, W, ws.data_ptr(),
                                             ws_elems, torch.cuda.current_stream().cuda_stream), "du_cc_keep_largest")
    return out


def apply_postprocessing(segmentation, pp_fns, pp_fn_kwargs):
    """remove_connected_components.py:37-40"""
    for fn, kwargs in zip(pp_fns, pp_fn_kwargs):
        segmentation = fn(segmentation, **kwargs)
    return segmentation


def _key(label_or_region):
    return tuple(label_or_region) if isinstance(label_or_region, list) else label_or_region


def _summary(preds, refs, labels_or_regions, ignore_label):
    """{'mean': {key: {'Dice'}}, 'foreground_mean': {'Dice'}} as compute_metrics_on_folder aggregates (evaluate_predictions.py:278-294):
    per label np.nanmean over the cases of Dice (nan where tp + fp + fn == 0, :189-194), then np.mean over the labels other than 0"""
    dice = np.empty((len(preds), len(labels_or_regions)), dtype=np.float64)
    for c, (p, g) in enumerate(zip(preds, refs)):
        tp, fp, fn, _ = segmentation_counts(p, g, labels_or_regions, ignore_label).tolist()
        for i in range(len(labels_or_regions)):
            dice[c, i] = 2 * tp[i] / (2 * tp[i] + fp[i] + fn[i]) if tp[i] + fp[i] + fn[i] > 0 else float("nan")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                               # a label absent from every case: mean of nothing
        means = {_key(r): {"Dice": float(np.nanmean(dice[:, i]))} for i, r in enumerate(labels_or_regions)}
    values = [m["Dice"] for k, m in means.items() if not (k == 0 or k == "0")]
    return {"mean": means, "foreground_mean": {"Dice": float(np.mean(values))}}


def determine_postprocessing(preds, refs, labels_or_regions, foreground_labels, ignore_label=None):
    """The search of remove_connected_components.py:53-245 over two equal-length lists of uint8 (D, H, W) label maps (prediction and
    reference of every case, each pair of one shape and device).  labels_or_regions: what the cases are scored on (foreground labels, or
    foreground regions as tuples); foreground_labels: the labels whose union step 1 treats as one mask.
      step 1  keep only the largest component of the union of foreground_labels; adopted if foreground_mean Dice rises strictly and no
              label's mean Dice falls (:151-157)
      step 2  only with more than one label or region: for each in the given order, keep only its largest component in the current best
              maps; adopted if that label's mean Dice rises strictly (:176-216)
    A comparison with nan is false, as in the reference.  Returns (pp_fns, pp_fn_kwargs, report): the first two replay through
    apply_postprocessing; report = {'input_folder', 'postprocessed': {'foreground_mean', 'mean' (keys as str)}, 'postprocessing_fns',
    'postprocessing_kwargs'} as postprocessing.json.  With device tensors the maps stay on the device; only (4, R) count tables cross."""
    preds, refs = list(preds), list(refs)
    if len(preds) != len(refs) or len(preds) == 0:
        raise ValueError("predictions and references must be two equal-length, non-empty lists")
    labels_or_regions = list(labels_or_regions)
    if len(labels_or_regions) == 0:
        raise ValueError("labels_or_regions is empty")
    for p in preds:
        _check_seg(p, labels_or_regions)
    pp_fn = remove_all_but_largest_component_from_segmentation
    pp_fns, pp_fn_kwargs = [], []
    baseline = _summary(preds, refs, labels_or_regions, ignore_label)

    kwargs = {"labels_or_regions": list(foreground_labels)}
    cand = [pp_fn(p, **kwargs) for p in preds]
    res = _summary(cand, refs, labels_or_regions, ignore_label)
    do_this = res["foreground_mean"]["Dice"] > baseline["foreground_mean"]["Dice"]
    if do_this:
        for k in res["mean"]:
            if res["mean"][k]["Dice"] < baseline["mean"][k]["Dice"]:
                do_this = False
                break
    source, source_res = preds, baseline
    if do_this:
        source, source_res = cand, res
        pp_fns.append(pp_fn)
        pp_fn_kwargs.append(kwargs)

    if len(labels_or_regions) > 1:
        for label_or_region in labels_or_regions:
            kwargs = {"labels_or_regions": label_or_region}
            cand = [pp_fn(p, **kwargs) for p in source]
            res = _summary(cand, refs, labels_or_regions, ignore_label)
            k = _key(label_or_region)
            if res["mean"][k]["Dice"] > source_res["mean"][k]["Dice"]:
                source, source_res = cand, res
                pp_fns.append(pp_fn)
                pp_fn_kwargs.append(kwargs)

    def section(summary):
        return {"foreground_mean": dict(summary["foreground_mean"]), "mean": {str(k): dict(v) for k, v in summary["mean"].items()}}

    report = {"input_folder": section(baseline), "postprocessed": section(source_res),
              "postprocessing_fns": [f.__name__ for f in pp_fns], "postprocessing_kwargs": pp_fn_kwargs}
    return pp_fns, pp_fn_kwargs, report
