"""The plain construction of the sliding-window sums, shared by tests/test_cpu_predict_cases.py and tests/test_gpu_predict_cases.py:
pad_to_patch + slicing + the reference's sequential `+=` loop in float32 (predict_from_raw_data.py:607-608), one window after the other."""
import numpy as np
import torch

from dinounet_amd import inference as INF


def plain_accumulate(logits, gauss, desc, preds, npreds):
    """in place; logits (nb, K, ph, pw), gauss (ph, pw), desc = [(case, d, y0, x0), ...], preds[case] (K, D, Hp, Wp), npreds[case] (D, Hp, Wp)"""
    ph, pw = gauss.shape
    for b, (i, d, y0, x0) in enumerate(desc):                                      # predict_from_raw_data.py:607-608, float32
        preds[i][:, d, y0:y0 + ph, x0:x0 + pw] += logits[b] * gauss
        npreds[i][d, y0:y0 + ph, x0:x0 + pw] += gauss


def plain_window_sums(forward, data, patch, step, gauss, batch_size, mirror_axes=None):
    """One case (C, D, H, W) on the forward's device -> float32 numpy (pred (K, D, Hp, Wp), npred (D, Hp, Wp), (y slice, x slice)): the padded
    copy, windows sliced from it in sliding_window_origins order and stacked batch_size at a time, INF._mirror_and_predict around `forward`,
    and every window added with plain_accumulate on the host.  gauss: float32 numpy (ph, pw)."""
    padded, slices = INF.pad_to_patch(data.float(), patch)
    D, Hp, Wp = padded.shape[1:]
    origins = INF.sliding_window_origins((D, Hp, Wp), patch, step)
    combos = INF.mirror_axes_combinations(mirror_axes, 4)
    pred = npred = None
    for i0 in range(0, len(origins), batch_size):
        chunk = origins[i0:i0 + batch_size]
        x = torch.stack([padded[:, d, y0:y0 + patch[0], x0:x0 + patch[1]] for d, y0, x0 in chunk])
        logits = INF._mirror_and_predict(forward, x, combos)[:len(chunk)].float().cpu().numpy()
        if pred is None:
            pred, npred = np.zeros((logits.shape[1], D, Hp, Wp), np.float32), np.zeros((D, Hp, Wp), np.float32)
        plain_accumulate(logits, gauss, [(0, *o) for o in chunk], [pred], [npred])
    return pred, npred, slices
