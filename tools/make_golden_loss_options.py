"""Generate tests/golden/loss_options.json: what the reference's own loss classes (DC_and_CE_loss, DC_and_BCE_loss with
MemoryEfficientSoftDiceLoss and RobustCrossEntropyLoss; compound_losses.py, dice.py, robust_ce_loss.py) return in fp64 for a list of
option sets: weight_ce, weight_dice, batch_dice, do_bg, class weights, with and without an ignore label, softmax and regions.  The three
files are loaded by path, with stub modules for their dinounet.* imports (helpers.softmax_helper_dim1, ddp_allgather.AllGatherGrad:
ddp=False here, so the latter is never called).  Runs only where the reference tree exists; the tests read the committed json, which
holds data only: seeds, shapes, option sets, the fp64 losses and a handful of gradient entries (the inputs come from the seeds:
tests/_loss_opt_ref.golden_inputs).

    python tools/make_golden_loss_options.py
"""
import importlib.util
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.refshim import REF_ROOT as REF  # noqa: E402  (where the reference tree lives: DINOUNET_REFERENCE_ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "loss_options.json")
SMOOTH = 1e-5
N_GRAD = 6


def load_reference():
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        m.__path__ = []
        sys.modules[name] = m
        return m

    class _NoGather:
        @staticmethod
        def apply(*a):
            raise RuntimeError("AllGatherGrad must not be reached with ddp=False")

    for n in ("dinounet", "dinounet.training", "dinounet.training.loss", "dinounet.utilities"):
        stub(n)
    stub("dinounet.utilities.helpers", softmax_helper_dim1=lambda x: torch.softmax(x, 1))
    stub("dinounet.utilities.ddp_allgather", AllGatherGrad=_NoGather)
    mods = {}
    for n in ("dice", "robust_ce_loss", "compound_losses"):
        full = f"dinounet.training.loss.{n}"
        spec = importlib.util.spec_from_file_location(full, os.path.join(REF, "dinounet", "training", "loss", n + ".py"))
        m = importlib.util.module_from_spec(spec)
        sys.modules[full] = m
        spec.loader.exec_module(m)
        mods[n] = m
    return mods


def cases():
    out, seed = [], 7000

    def add(name, shape, regions=False, has_ignore=False, ignore_frac=0.0, **opt):
        nonlocal seed
        seed += 1
        o = dict(weight_ce=1.0, weight_dice=1.0, batch_dice=True, do_bg=bool(regions), class_w=None)
        o.update(opt)
        out.append(dict(name=name, shape=list(shape), regions=regions, has_ignore=has_ignore, ignore_frac=ignore_frac, seed=seed, options=o))

    for ig in (False, True):
        f, tag = (0.3, "_ign") if ig else (0.0, "")
        add("defaults" + tag, (2, 3, 5, 7), has_ignore=ig, ignore_frac=f)
        add("weights" + tag, (2, 3, 5, 7), has_ignore=ig, ignore_frac=f, weight_ce=0.5, weight_dice=2.0)
        add("per_sample" + tag, (3, 4, 6, 5), has_ignore=ig, ignore_frac=f, batch_dice=False)
        add("do_bg" + tag, (2, 3, 5, 7), has_ignore=ig, ignore_frac=f, do_bg=True)
        add("class_w" + tag, (2, 4, 5, 7), has_ignore=ig, ignore_frac=f, class_w=[0.5, 1.0, 2.0, 4.0])
        add("do_bg_per_sample" + tag, (3, 2, 4, 4), has_ignore=ig, ignore_frac=f, do_bg=True, batch_dice=False)
        add("no_ce" + tag, (2, 5, 5, 7), has_ignore=ig, ignore_frac=f, weight_ce=0.0)
        add("no_dice" + tag, (2, 8, 5, 7), has_ignore=ig, ignore_frac=f, weight_dice=0.0, class_w=[0.3 + 0.45 * k for k in range(8)])
        add("all" + tag, (3, 3, 6, 5), has_ignore=ig, ignore_frac=f, weight_ce=0.25, weight_dice=3.0, batch_dice=False, do_bg=True,
            class_w=[2.0, 0.5, 1.5])
        add("regions_weights" + tag, (2, 3, 5, 7), regions=True, has_ignore=ig, ignore_frac=f, weight_ce=0.5, weight_dice=2.0)
        add("regions_per_sample" + tag, (3, 1, 6, 5), regions=True, has_ignore=ig, ignore_frac=f, batch_dice=False)
        add("regions_no_ce" + tag, (2, 8, 4, 4), regions=True, has_ignore=ig, ignore_frac=f, weight_ce=0.0, batch_dice=False)
        add("regions_no_dice" + tag, (2, 2, 4, 4), regions=True, has_ignore=ig, ignore_frac=f, weight_dice=0.0)
    add("all_ignored", (2, 3, 4, 4), has_ignore=True, ignore_frac=2.0, batch_dice=False, class_w=[1.0, 2.0, 4.0])
    return out


def main():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _loss_opt_ref as O
    import _loss_ref as R
    mods = load_reference()
    C, D = mods["compound_losses"], mods["dice"]
    res = []
    for c in cases():
        o = c["options"]
        x32, t = O.golden_inputs(c)
        x = x32.double().requires_grad_(True)
        dice_kw = {"batch_dice": o["batch_dice"], "smooth": SMOOTH, "do_bg": o["do_bg"], "ddp": False}
        if c["regions"]:
            mod = C.DC_and_BCE_loss({}, dice_kw, weight_ce=o["weight_ce"], weight_dice=o["weight_dice"], use_ignore_label=c["has_ignore"],
                                    dice_class=D.MemoryEfficientSoftDiceLoss)
            tgt = t.double()
        else:
            ce_kw = {} if o["class_w"] is None else {"weight": torch.tensor(o["class_w"], dtype=torch.float64)}
            mod = C.DC_and_CE_loss(dice_kw, ce_kw, weight_ce=o["weight_ce"], weight_dice=o["weight_dice"],
                                   ignore_label=R.IGNORE if c["has_ignore"] else None, dice_class=D.MemoryEfficientSoftDiceLoss)
            tgt = t
        loss = mod(x, tgt)
        loss.backward()
        g = x.grad.reshape(-1)
        idx = torch.randperm(g.numel(), generator=torch.Generator().manual_seed(c["seed"] + 500))[:N_GRAD].tolist()
        c["loss"] = float(loss)
        c["grad_index"] = idx
        c["grad"] = [float(g[i]) for i in idx]
        c["grad_abs_sum"] = float(g.abs().sum())
        res.append(c)
        print(f"{c['name']}: loss {c['loss']:.12f}")
    json.dump({"smooth": SMOOTH, "ignore_label": R.IGNORE, "cases": res}, open(OUT, "w"), indent=1)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
