"""Generate tests/golden/export_reference.npz: label maps, probabilities and per-case metrics of the reference's export path
(convert_predicted_logits_to_segmentation_with_correct_shape, dinounet/inference/export_prediction.py:15-68; compute_metrics,
dinounet/evaluation/evaluate_predictions.py:152-234) on fixed fp32 logits.  Runs only where the reference tree exists; the tests read the
committed .npz, which holds data only.

Route.  Labels and probabilities come from the reference's own LabelManager (apply_inference_nonlin, convert_probabilities_to_segmentation,
revert_cropping_on_probabilities, utilities/label_handling/label_handling.py:128-209), the counts and ratios from its own compute_metrics
(with region_or_label_to_mask and compute_tp_fp_fn_tn, evaluate_predictions.py:75-94) fed through an in-memory reader, all imported through
oracle.refshim.  Local stubs stand in for the third-party names those modules import and the build container lacks:
acvl_utils.cropping_and_padding.bounding_boxes.bounding_box_to_slice (restated: a tuple of slice(lo, hi)), batchgenerators' file helpers
(join = os.path.join; the json / listing helpers are never called), the image reader / writer modules (SimpleITK, nibabel, tifffile) and the
plans handler (only type annotations use it).
GLUED BY HAND: the bbox paste and the transpose of export_prediction.py:44-52 and :62-63 (`reference_export` below) -- the function itself
needs a PlansManager / ConfigurationManager built from a plans file.
RESTATED: the resampling.  The reference calls resample_data_or_seg (preprocessing/resampling/default_resampling.py:125-213; order 1 per experiment_planning/experiment_planners/default_experiment_planner.py:152-159), whose
non-segmentation branch is skimage.transform.resize(order=1, mode='edge', anti_aliasing=False) per channel in float64, cast back to the
input's fp32 (:152, :213).  skimage is not installed; since 0.19 that call is scipy.ndimage.zoom(order=1, mode='nearest', grid_mode=True),
which is what runs here, per channel and slice (in-plane only: the slice axis keeps its size, as for this repo's 2D configurations).  The
boundary to skimage is therefore unpinned.

Conditions on the inputs, asserted here.  The tie band of a case is 1e-5 * max|logit| (the fp32 error of the 4-tap interpolation plus
the normalisation is about 1e-6 * max|logit|: a factor 10 of room); a voxel is in the band if its float64 top-two gap (softmax) / any
|logit| (regions) is below it; at most 0.1 % of a case's voxels may be.  Cases marked `exact` hold small integer logits with exact ties and
are either not resampled or upsampled 2x / 4x (dyadic weights): every operation on them is exact in fp32 and float64 alike, so their band
is 0 and labels must agree everywhere.  `band` is stored per case as a mask in the output geometry.

    python tools/make_golden_export.py
"""
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "export_reference.npz")
BAND_REL, BAND_CAP = 1e-5, 1e-3

# name, kind, K | R, D, (Hc, Wc), (Ho, Wo), shape_before_cropping, bbox low corner, regions_class_order, transpose_backward, exact
CASES = [
    ("softmax3_up", "softmax", 3, 2, (17, 23), (40, 31), (4, 44, 37), (1, 2, 3), None, (0, 1, 2), False),        # bbox touches no side
    ("regions1_mixed", "regions", 1, 1, (64, 64), (37, 129), (1, 37, 129), (0, 0, 0), [2], (0, 1, 2), False),    # down in y, up in x; all sides
    ("softmax8_down", "softmax", 8, 1, (20, 30), (7, 9), (2, 9, 12), (0, 1, 1), None, (0, 1, 2), False),         # bbox touches one side
    ("regions3_one_axis", "regions", 3, 2, (33, 20), (33, 47), (2, 33, 47), (0, 0, 0), [3, 1, 2], (0, 2, 1), False),
    ("regions4_plain", "regions", 4, 1, (17, 23), (17, 23), (3, 20, 27), (1, 2, 3), [4, 1, 3, 2], (0, 1, 2), False),
    ("softmax2_plain", "softmax", 2, 2, (32, 32), (32, 32), (2, 32, 32), (0, 0, 0), None, (2, 0, 1), False),
    ("softmax4_ties", "softmax", 4, 1, (16, 16), (16, 16), (1, 16, 16), (0, 0, 0), None, (0, 1, 2), True),
    ("regions3_ties", "regions", 3, 1, (16, 16), (16, 16), (2, 18, 16), (1, 2, 0), [2, 1, 3], (0, 1, 2), True),
    ("softmax3_ties_up", "softmax", 3, 1, (12, 10), (24, 40), (1, 24, 40), (0, 0, 0), None, (0, 1, 2), True),
]
# name, shape (1, z, y, x), labels present, labels_or_regions, ignore_label
METRIC_CASES = [
    ("labels", (1, 2, 17, 23), 4, [1, 2, 3, 5], None),                                  # 5 is in neither map: nan
    ("regions_ignore", (1, 1, 32, 32), 4, [(1, 2, 3), (2, 3), 3], 4),
    ("labels_ignore", (1, 3, 16, 16), 3, [0, 1, 2, 7], 3),
]
METRIC_KEYS = ["Dice", "IoU", "Sensitivity", "Specificity", "Precision", "FP", "TP", "FN", "TN", "n_pred", "n_ref"]


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def reference_modules():
    """LabelManager and the evaluation module of the reference tree (refshim import path plus the stubs of the module docstring)"""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from oracle import refshim
    refshim.install()
    for n in ("acvl_utils", "acvl_utils.cropping_and_padding", "batchgenerators", "batchgenerators.utilities"):
        _stub(n).__path__ = []
    _stub("acvl_utils.cropping_and_padding.bounding_boxes", bounding_box_to_slice=lambda bbox: tuple(slice(*i) for i in bbox))

    def _unused(*a, **k):
        raise RuntimeError("file helper stub: not available here")

    _stub("batchgenerators.utilities.file_and_folder_operations", join=os.path.join, isfile=os.path.isfile, subfiles=_unused,
          save_json=_unused, load_json=_unused, save_pickle=_unused)
    _stub("dinounet.imageio.reader_writer_registry", determine_reader_writer_from_dataset_json=_unused,
          determine_reader_writer_from_file_ending=_unused)
    _stub("dinounet.imageio.simpleitk_reader_writer", SimpleITKIO=None)
    _stub("dinounet.utilities.plans_handling.plans_handler", PlansManager=None, ConfigurationManager=None)
    from dinounet.utilities.label_handling.label_handling import LabelManager
    import io
    import contextlib
    with contextlib.redirect_stdout(io.StringIO()):                       # the module prints that medpy is absent
        from dinounet.evaluation import evaluate_predictions
    return LabelManager, evaluate_predictions


def label_manager(LabelManager, kind, C, order):
    if kind == "softmax":
        return LabelManager({"background": 0, **{f"c{i}": i for i in range(1, C)}}, None)
    top = max(order)
    # C nested regions over the labels 1..top (what they contain does not matter to the export path: only their number and the order do)
    regions = {"background": 0}
    for i in range(C):
        regions[f"r{i}"] = tuple(range(1, top + 2))[: max(2, top + 1 - i)]
    lm = LabelManager(regions, list(order))
    assert lm.has_regions and lm.num_segmentation_heads == C
    return lm


def resample_like_reference(logits32, out_hw):
    """default_resampling.py:152-213 for non-segmentation data, in-plane: float64 order-1 zoom per channel and slice, back to fp32.
    Returns (fp32 result, float64 result)"""
    from scipy.ndimage import zoom
    K, D, H, W = logits32.shape
    if (H, W) == tuple(out_hw):
        return logits32.copy(), logits32.astype(np.float64)
    z64 = np.empty((K, D, *out_hw), dtype=np.float64)
    for k in range(K):
        for d in range(D):
            z64[k, d] = zoom(logits32[k, d].astype(np.float64), (out_hw[0] / H, out_hw[1] / W), order=1, mode="nearest", grid_mode=True)
    return z64.astype(np.float32), z64


def reference_export(lm, logits32, out_hw, before, corner, tb):
    """export_prediction.py:25-65 with the paste (:44-48) and the transposes (:52, :62-63) by hand"""
    res32, res64 = resample_like_reference(logits32, out_hw)
    probs = lm.apply_inference_nonlin(res32)                                          # :36
    seg = lm.convert_probabilities_to_segmentation(probs)                             # :38
    seg = seg.cpu().numpy()
    bbox = [[c, c + s] for c, s in zip(corner, seg.shape)]
    out = np.zeros(before, dtype=np.uint8)                                            # :45-46
    out[tuple(slice(*b) for b in bbox)] = seg                                         # :47-48
    out = out.transpose(tb)                                                           # :52
    p = lm.revert_cropping_on_probabilities(probs, bbox, before).cpu().numpy()        # :55-60
    p = p.transpose([0] + [i + 1 for i in tb])                                        # :62-63
    return out, p, res64, bbox


class _MemoryReader:
    """read_seg of a BaseReaderWriter over arrays held in memory"""

    def __init__(self, arrays):
        self.arrays = arrays

    def read_seg(self, name):
        return self.arrays[name], {"spacing": (1.0, 1.0, 1.0)}


def main():
    torch.set_default_dtype(torch.float32)
    LabelManager, ev = reference_modules()
    arrays, meta = {}, {"cases": [], "metric_cases": [], "metric_keys": METRIC_KEYS, "band_rel": BAND_REL, "band_cap": BAND_CAP}
    for i, (name, kind, C, D, hw, out_hw, before, corner, order, tb, exact) in enumerate(CASES):
        g = torch.Generator().manual_seed(4200 + 10 * i)
        if exact:
            lim = 8 if hw != out_hw else 1
            logits = torch.randint(-lim, lim + 1, (C, D, *hw), generator=g).float().numpy()
        else:
            logits = (torch.randn((C, D, *hw), generator=g) * 2.0).float().numpy()
        lm = label_manager(LabelManager, kind, C, order)
        seg, probs, res64, bbox = reference_export(lm, logits, out_hw, before, corner, tb)
        if exact:
            band, inband = 0.0, np.zeros(res64.shape[1:], dtype=bool)
            assert np.array_equal(res64, res64.astype(np.float32).astype(np.float64)), name      # the resampled values are exact
        else:
            band = BAND_REL * float(np.abs(logits).max())
            if kind == "softmax":
                top2 = np.sort(res64, axis=0)[-2:]
                inband = (top2[1] - top2[0]) < band
            else:
                inband = (np.abs(res64) < band).any(0)
            assert inband.mean() <= BAND_CAP, (name, inband.sum(), inband.size)
        band_mask = np.zeros(before, dtype=np.uint8)
        band_mask[tuple(slice(*b) for b in bbox)] = inband
        arrays[f"{name}/logits"] = logits
        arrays[f"{name}/seg"] = seg
        arrays[f"{name}/probs"] = probs.astype(np.float32)
        arrays[f"{name}/band"] = band_mask.transpose(tb)
        meta["cases"].append({"name": name, "kind": kind, "C": C, "exact": exact, "band": band, "n_inband": int(inband.sum()),
                              "regions_class_order": order, "transpose_backward": list(tb),
                              "properties": {"shape_before_cropping": list(before), "bbox_used_for_cropping": bbox,
                                             "shape_after_cropping_and_before_resampling": [D, *out_hw]}})
        print(f"{name}: seg {seg.shape} labels {np.unique(seg).tolist()} band {band:.3g} in-band {int(inband.sum())} / {inband.size}")
    for i, (name, shape, top, lors, ig) in enumerate(METRIC_CASES):
        g = torch.Generator().manual_seed(5000 + 10 * i)
        ref = torch.randint(0, top, shape, generator=g)
        pred = torch.where(torch.rand(shape, generator=g) < 0.7, ref, torch.randint(0, top, shape, generator=g))
        if ig is not None:
            ref = torch.where(torch.rand(shape, generator=g) < 0.2, torch.full_like(ref, ig), ref)
        ref, pred = ref.numpy().astype(np.uint8), pred.numpy().astype(np.uint8)
        res = ev.compute_metrics("ref", "pred", _MemoryReader({"ref": ref, "pred": pred}), lors, ig)["metrics"]      # :152-235
        table = np.array([[float(res[r][k]) for k in METRIC_KEYS] for r in lors], dtype=np.float64)
        arrays[f"metrics_{name}/ref"], arrays[f"metrics_{name}/pred"], arrays[f"metrics_{name}/table"] = ref, pred, table
        meta["metric_cases"].append({"name": name, "labels_or_regions": [list(r) if isinstance(r, tuple) else r for r in lors],
                                     "ignore_label": ig})
        print(f"metrics_{name}: Dice {table[:, 0]}")
    np.savez_compressed(OUT, meta=json.dumps(meta), **arrays)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
