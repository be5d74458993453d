"""Generate tests/golden/val_counts_reference.npz: tp / fp / fn of the reference trainer's validation step (nnUNetTrainer.validation_step,
nnUNetTrainer.py:946-1008) and the epoch values of on_validation_epoch_end (:1010-1052) on fixed fp32 inputs.  Runs only where the
reference tree exists; the tests read the committed .npz.

Route: the counts come from the reference's own get_tp_fp_fn_tn (training/loss/dice.py:122, imported through oracle.refshim), fed the
way validation_step feeds it -- the hard prediction of :973-980, the mask / target rewrite of :982-992, axes (0, 2, 3) -- with those
twenty lines GLUED BY HAND below (`reference_validation_step`): nnUNetTrainer.validation_step itself could not be called on a stub
`self`, because the trainer module does not import here (its first imports need batchgenerators, which is absent).  The per-step loss is
the reference's own loss module (DC_and_CE_loss / DC_and_BCE_loss as _build_loss configures them) in fp64 on the fp32 logits, as in
tools/make_golden_seg_loss.py.

The fixture holds data only: per case the fp32 logits, int16 labels, the float32 counts the reference returns (all classes; the
background is dropped per :999-1006 for the epoch values) and the loss; per epoch (the cases of one label configuration, one validation
step each) the :1046-1047 values.

Conditions on the inputs, asserted here: no region logit in (0, 1e-6) (the product predicts a region where x > 0, the reference where
torch's fp32 sigmoid(x) > 0.5: they differ only for 0 < x < ~1.2e-7); every count < 2^24 (the reference sums in fp32: exact below that).

    python tools/make_golden_val_counts.py
"""
import json
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "val_counts_reference.npz")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden_seg_loss import make_labels, reference_classes, reference_loss, regions_onehot  # noqa: E402

# (name, kind, shape (B, K or R, H, W), regions, ignore_label, ties)
CASES = [
    ("softmax", "softmax", (2, 4, 32, 32), None, None, False),
    ("softmax_ignore", "softmax", (2, 3, 17, 23), None, 3, False),
    ("softmax_all_ignored", "softmax", (1, 3, 16, 16), None, 3, False),
    ("regions_ignore", "regions", (2, 3, 32, 32), [(1, 2, 3), (2, 3), (3,)], 4, False),
    ("regions_tail", "regions", (2, 2, 17, 23), [1, (1, 2)], None, False),
    ("softmax_ties", "softmax", (1, 4, 16, 16), None, None, True),
    ("regions_ties", "regions", (1, 4, 16, 16), [1, 2, 3, (1, 2, 3)], None, True),
]
# on_validation_epoch_end over the cases of one label configuration (same number of outputs), one validation step per case
EPOCHS = [
    ("epoch_softmax", ["softmax", "softmax_ties"]),
    ("epoch_softmax_ignore", ["softmax_ignore", "softmax_all_ignored"]),
    ("epoch_regions_ignore", ["regions_ignore"]),
    ("epoch_regions_tail", ["regions_tail"]),
    ("epoch_regions_ties", ["regions_ties"]),
]


def reference_validation_step(get_tp_fp_fn_tn, output, target, has_regions, ignore_label):
    """nnUNetTrainer.py:971-1006 by hand (see the module docstring): output fp32 logits, target the trainer's float target -- the label
    map (B,1,H,W), or the one-hot region planes with the ignore plane last"""
    if has_regions:
        pred = (torch.sigmoid(output) > 0.5).long()                                   # :973-974
    else:
        pred = torch.zeros_like(output).scatter_(1, output.argmax(1, keepdim=True), 1)   # :976-979
    mask = None
    if ignore_label is not None and has_regions:                                      # :987-990
        mask, target = 1 - target[:, -1:], target[:, :-1]
    elif ignore_label is not None:                                                    # :984-986
        mask = (target != ignore_label).float()
        target = torch.where(target == ignore_label, torch.zeros_like(target), target)
    tp, fp, fn, _ = get_tp_fp_fn_tn(pred, target, axes=[0, 2, 3], mask=mask)          # :994
    return tp.numpy(), fp.numpy(), fn.numpy()


def case_inputs(shape, kind, regions, ignore_label, ties, seed):
    g = torch.Generator().manual_seed(seed)
    if ties:
        logits = torch.randint(-1, 2, shape, generator=g).float()
    else:
        logits = (torch.randn(shape, generator=g) * 2.0).float()
    return logits, make_labels(shape, kind, regions, ignore_label, seed + 1)


def main():
    torch.set_default_dtype(torch.float32)
    reference_classes()                                   # installs the refshim import path
    from dinounet.training.loss.dice import get_tp_fp_fn_tn
    arrays, meta = {}, {"cases": [], "epochs": []}
    steps = {}
    for i, (name, kind, shape, regions, ig, ties) in enumerate(CASES):
        logits, lab = case_inputs(shape, kind, regions, ig, ties, 1000 + 10 * i)
        if name == "softmax_all_ignored":
            lab[:] = ig
        if kind == "regions":
            assert not bool(((logits > 0) & (logits < 1e-6)).any()), name
            tgt = regions_onehot(lab, regions, ig).float()
        else:
            tgt = lab.float()                             # the trainer's target is float (NumpyToTensor 'float', nnUNetTrainer.py:771)
        tp, fp, fn = reference_validation_step(get_tp_fp_fn_tn, logits, tgt, kind == "regions", ig)
        assert max(tp.max(), fp.max(), fn.max()) < 2 ** 24, name
        with torch.no_grad():
            loss = float(reference_loss(kind, ig)(logits.double(), tgt.double()))
        arrays[f"{name}/logits"] = logits.numpy()
        arrays[f"{name}/labels"] = lab.numpy().astype(np.int16)
        arrays[f"{name}/tp"], arrays[f"{name}/fp"], arrays[f"{name}/fn"] = tp, fp, fn
        arrays[f"{name}/loss"] = np.array(loss, dtype=np.float64)
        meta["cases"].append({"name": name, "kind": kind, "shape": list(shape), "regions": regions, "ignore_label": ig, "ties": ties})
        steps[name] = (kind, tp, fp, fn, loss)
        print(f"{name}: tp {tp} fp {fp} fn {fn} loss {loss:.8f}")
    for ename, names in EPOCHS:
        drop = 0 if steps[names[0]][0] == "regions" else 1          # :999-1006
        tp = np.sum([steps[n][1][drop:] for n in names], 0)         # :1012-1014
        fp = np.sum([steps[n][2][drop:] for n in names], 0)
        fn = np.sum([steps[n][3][drop:] for n in names], 0)
        assert tp.dtype == np.float32                               # the reference divides in fp32 (:1046); nan where 0 / 0
        with np.errstate(divide="ignore", invalid="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            dice = 2 * tp / (2 * tp + fp + fn)                      # :1046
            mean_fg_dice = np.nanmean(dice)                         # :1047
        arrays[f"{ename}/dice"] = dice.astype(np.float64)
        arrays[f"{ename}/mean_fg_dice"] = np.array(mean_fg_dice, dtype=np.float64)
        arrays[f"{ename}/val_loss"] = np.array(np.mean([steps[n][4] for n in names]), dtype=np.float64)    # :1043
        meta["epochs"].append({"name": ename, "cases": names})
        print(f"{ename}: dice {dice} mean_fg_dice {mean_fg_dice}")
    np.savez_compressed(OUT, meta=json.dumps(meta), **arrays)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
