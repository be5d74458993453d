"""Ensembling on the MI355X: the step between export and postprocessing.  Probability volumes of several models (or folds) are averaged and
turned into one label map; the best model or pair of models is picked by foreground-mean Dice and handed to the postprocessing search.

Mirrors dinounet/ensembling/ensemble.py (average_probabilities :17-29, merge_files :32-46, ensemble_folders :49-111,
ensemble_crossvalidations :128-206) and dinounet/evaluation/find_best_configuration.py:81-211, over tensors and dicts instead of folders of
.npz files (no files, pool or reader/writer):

    mean = (((p0 + p1) + p2) + ...) / M      fp32, the members in their order, one true division: numpy's `avg += p; avg /= M` to the bit
    label map = argmax(mean)  |  regions_class_order[i] painted where mean[i] > 0.5, in order

Members are what export.logits_to_segmentation(..., return_probabilities=True) returns: fp32 (or, like the reference's .npz, fp16)
(K, D, H, W) probabilities already in the case's original geometry, the background plane 1 outside the crop.  CUDA tensors run ONE HIP pass
(csrc/ensemble.hip: du_ensemble_merge) that reads every member once and writes the uint8 label map; the mean is written only when asked
for.  CPU tensors take a torch restatement of the same arithmetic; it is what the tests compare the kernel against.

Differences from the reference, on purpose.  merge_files passes the averaged PROBABILITIES to convert_logits_to_segmentation
(ensemble.py:42), which applies the nonlinearity a second time (label_handling.py:128-141).  With softmax heads that is monotone, so the
argmax is the same wherever fp32 softmax keeps two distinct means distinct; here the argmax is taken of the mean itself (lowest index among
equal maxima).  With region heads the second sigmoid turns the threshold into sigmoid(mean) > 0.5, i.e. mean > 0, which paints nearly every
voxel; here convert_probabilities_to_segmentation's own `> 0.5` (label_handling.py:165-171) is applied to the mean.  Label maps are uint8
(export.py); at most 16 members per merge; a non-finite value raises the RuntimeError export raises."""
import torch

from . import _lib
from .export import EXPORT_REGIONS, EXPORT_SOFTMAX, MAX_CLASSES, _check_heads, _signed64

MAX_MEMBERS = 16                    # du_ensemble_merge: M in [1, 16]


def _check_members(members):
    members = list(members)
    if len(members) == 0:
        raise ValueError("at least one member must be given")                       # ensemble.py:18
    if len(members) > MAX_MEMBERS:
        raise ValueError(f"at most {MAX_MEMBERS} members can be merged at once, got {len(members)}")
    first = members[0]
    for m in members:
        if not isinstance(m, torch.Tensor) or m.ndim != 4:
            raise ValueError("members must be (K, D, H, W) tensors")
        if m.shape != first.shape or m.dtype != first.dtype or m.device != first.device:
            raise ValueError("members must have one shape, dtype and device")
    if first.dtype not in (torch.float32, torch.float16):
        raise ValueError(f"members must be float32 or float16, got {first.dtype}")
    return members


def _mean_torch(members):
    """average_probabilities (ensemble.py:17-29), line by line"""
    avg = members[0].to(torch.float32, copy=True)
    for m in members[1:]:
        avg += m                                         # an fp16 member widens exactly in the add
    avg /= float(len(members))
    return avg


def _labels_torch(mean, order):
    if order is None:
        return mean.argmax(0).to(torch.uint8)
    lab = torch.zeros(mean.shape[1:], dtype=torch.uint8, device=mean.device)
    for i, c in enumerate(order):                        # label_handling.py:170-171
        lab[mean[i] > 0.5] = c
    return lab


def _merge_hip(members, order, want_seg, want_mean):
    """members: checked CUDA tensors.  One launch per 8 planes (one launch for everything that has a label map)."""
    L = _lib.lib()
    first = members[0]
    K = int(first.shape[0])
    n = first[0].numel()
    dev = first.device
    members = [m.contiguous() for m in members]          # a contiguous view keeps its (possibly unaligned) start
    es = first.element_size()
    seg = torch.empty(first.shape[1:], dtype=torch.uint8, device=dev) if want_seg else None
    mean = torch.empty(first.shape, dtype=torch.float32, device=dev) if want_mean else None
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    packed = 0 if order is None else _signed64(sum(c << (8 * i) for i, c in enumerate(order)))
    st = torch.cuda.current_stream().cuda_stream
    for k0 in range(0, K, MAX_CLASSES):                  # more than 8 planes: only without a label map (average_probabilities)
        kc = min(MAX_CLASSES, K - k0)
        table = torch.tensor([m.data_ptr() + k0 * n * es for m in members], dtype=torch.int64).to(dev)
        _lib.check(L.du_ensemble_merge(table.data_ptr(), len(members), es, kc, n, EXPORT_SOFTMAX if order is None else EXPORT_REGIONS,
                                       packed, None if seg is None else seg.data_ptr(),
                                       None if mean is None else mean.data_ptr() + 4 * k0 * n, flag.data_ptr(), st), "du_ensemble_merge")
    return seg, mean, int(flag.item()) == 0


@torch.no_grad()
def average_probabilities(members):
    """average_probabilities (ensemble.py:17-29) over a list of (K, D, H, W) tensors of one shape, dtype (fp32 or fp16) and device: the fp32
    mean, the members added in their order and divided once.  CUDA tensors run du_ensemble_merge, CPU tensors torch."""
    members = _check_members(members)
    if members[0].numel() == 0:
        raise ValueError("empty members")
    if members[0].is_cuda:
        return _merge_hip(members, None, False, True)[1]
    return _mean_torch(members)


@torch.no_grad()
def merge_probabilities(members, *, regions_class_order=None, return_probabilities=False):
    """merge_files (ensemble.py:32-46) without the files: members (list of 1..16 (K, D, H, W) probability tensors of one shape, dtype and
    device) -> the uint8 (D, H, W) label map of their mean on the members' device, with return_probabilities also the fp32 mean.
    regions_class_order: None = softmax heads (K in 2..8, argmax of the mean), else the label painted for each of the K = R in 1..8 regions
    where its mean exceeds 0.5, in order.  See the module docstring for where this differs from the reference.  CUDA tensors run
    du_ensemble_merge, CPU tensors the torch restatement."""
    members = _check_members(members)
    order = _check_heads(int(members[0].shape[0]), regions_class_order)
    if members[0].numel() == 0:
        raise ValueError("empty members")
    if members[0].is_cuda:
        seg, mean, finite = _merge_hip(members, order, True, return_probabilities)
    else:
        mean = _mean_torch(members)
        seg, finite = _labels_torch(mean, order), bool(torch.isfinite(mean).all())
    if not finite:
        raise RuntimeError("Encountered inf in predicted array")                     # as export does (predict_from_raw_data.py:612-615)
    return (seg, mean) if return_probabilities else seg


def ensemble_cases(list_of_models, *, regions_class_order=None, return_probabilities=False):
    """ensemble_folders (ensemble.py:49-111): list_of_models = one dict case_id -> probabilities per model; returns dict case_id -> what
    merge_probabilities returns for the members of that case, in the order of the models.  Every model must hold the same cases (:87-89)."""
    list_of_models = list(list_of_models)
    if len(list_of_models) == 0:
        raise ValueError("at least one model must be given")
    cases = set()
    for model in list_of_models:
        cases.update(model.keys())
    for i, model in enumerate(list_of_models):
        missing = cases.difference(model.keys())
        if missing:
            raise AssertionError(f"Not all models contain the same cases for ensembling: model {i} misses {sorted(missing, key=str)}")
    return {c: merge_probabilities([model[c] for model in list_of_models], regions_class_order=regions_class_order,
                                   return_probabilities=return_probabilities) for c in sorted(cases, key=str)}


def ensemble_crossvalidations(list_of_models_by_fold, folds=None, *, regions_class_order=None, return_probabilities=False):
    """ensemble_crossvalidations (ensemble.py:128-206): every model is a dict fold -> dict case_id -> probabilities (the validation cases of
    that fold; models may have different splits).  folds: the folds to read, None = every fold of each model.  RuntimeError for a requested
    fold that is missing or empty (:145-151), for a model that lacks a case another model has (:156-166) and for a case that is present in
    more than one fold of one model (:175-176).  Returns dict case_id -> what merge_probabilities returns."""
    list_of_models_by_fold = list(list_of_models_by_fold)
    if len(list_of_models_by_fold) == 0:
        raise ValueError("at least one model must be given")
    mappings, unique = [], set()
    for i, model in enumerate(list_of_models_by_fold):
        mapping = {}
        for f in (list(model.keys()) if folds is None else folds):
            if f not in model or len(model[f]) == 0:
                raise RuntimeError(f"model {i} has no predictions for fold {f}: all requested folds must be present")
            for case, probs in model[f].items():
                if case in mapping:
                    raise RuntimeError(f"Duplicate detected. Case {case} is present in more than one fold of model {i}.")
                mapping[case] = probs
        mappings.append(mapping)
        unique.update(mapping.keys())
    for i, mapping in enumerate(mappings):
        missing = unique.difference(mapping.keys())
        if missing:
            raise RuntimeError(f"model {i} does not seem to contain all predictions. Missing: {sorted(missing, key=str)}")
    return {c: merge_probabilities([mapping[c] for mapping in mappings], regions_class_order=regions_class_order,
                                   return_probabilities=return_probabilities) for c in sorted(unique, key=str)}


def find_best_configuration(models, references, labels_or_regions, foreground_labels, ignore_label=None, allow_ensembling=True, *,
                            regions_class_order=None):
    """find_best_configuration (evaluation/find_best_configuration.py:81-211) over tensors.  models: ordered dict name -> dict case_id ->
    (segmentation uint8 (D, H, W), probabilities (K, D, H, W) or None); references: dict case_id -> uint8 label map.  Every model is scored by
    the foreground_mean Dice of compute_metrics_on_folder over labels_or_regions; with allow_ensembling every pair i < j as well, merged by
    merge_probabilities and named ensemble___{a}___{b} (both need probabilities).  The maximum wins, the first entry on a tie: single models
    come before ensembles (:142-146).  determine_postprocessing then runs on the winner's label maps.  Returns the fields of the reference's
    return_dict that do not name files: 'all_results' {name: Dice}, 'best_model_or_ensemble' {'result_on_crossval_pre_pp',
    'result_on_crossval_post_pp', 'selected_model_or_models' [names]}, and 'postprocessing' = (pp_fns, pp_fn_kwargs), which replay through
    postprocessing.apply_postprocessing.  With device tensors only (4, R) count tables cross to the host."""
    from .postprocessing import _summary, determine_postprocessing
    names = list(models.keys())
    if len(names) == 0:
        raise ValueError("at least one model must be given")
    cases = sorted(references.keys(), key=str)
    if len(cases) == 0:
        raise ValueError("no reference cases")
    for name in names:
        if set(models[name].keys()) != set(cases):
            raise ValueError(f"model {name!r} does not hold exactly the reference cases")
    labels_or_regions = list(labels_or_regions)
    refs = [references[c] for c in cases]
    segs, all_results = {}, {}
    for name in names:
        segs[name] = [models[name][c][0] for c in cases]
        all_results[name] = _summary(segs[name], refs, labels_or_regions, ignore_label)["foreground_mean"]["Dice"]
    members_of = {name: [name] for name in names}
    if allow_ensembling:
        for i in range(len(names)):
            for j in range(i + 1, len(names)):
                a, b = names[i], names[j]
                for name in (a, b):
                    if any(models[name][c][1] is None for c in cases):
                        raise ValueError(f"model {name!r} has no probabilities: ensembling needs them (or allow_ensembling=False)")
                key = f"ensemble___{a}___{b}"
                segs[key] = [merge_probabilities([models[a][c][1], models[b][c][1]], regions_class_order=regions_class_order) for c in cases]
                all_results[key] = _summary(segs[key], refs, labels_or_regions, ignore_label)["foreground_mean"]["Dice"]
                members_of[key] = [a, b]
    unranked = [k for k, v in all_results.items() if v != v]
    if unranked:
        raise ValueError(f"the foreground-mean Dice of {unranked} is nan (a label of labels_or_regions occurs in no case, neither "
                         f"predicted nor reference): it cannot be ranked")
    best_score = max(all_results.values())
    best_key = [k for k, v in all_results.items() if v == best_score][0]             # a tie: the first, i.e. the simpler one (:143-146)
    pp_fns, pp_fn_kwargs, report = determine_postprocessing(segs[best_key], refs, labels_or_regions, foreground_labels, ignore_label)
    return {"all_results": all_results,
            "best_model_or_ensemble": {"result_on_crossval_pre_pp": all_results[best_key],
                                       "result_on_crossval_post_pp": report["postprocessed"]["foreground_mean"]["Dice"],
                                       "selected_model_or_models": members_of[best_key]},
            "postprocessing": (pp_fns, pp_fn_kwargs)}
