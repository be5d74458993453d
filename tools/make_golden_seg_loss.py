"""Generate tests/golden/seg_loss_reference.npz: the reference trainer's ignore-label and region losses (nnUNetTrainer._build_loss,
nnUNetTrainer.py:355-365) on fixed fp32 inputs, evaluated in fp64 on the CPU by the reference's own classes (DC_and_CE_loss with an
ignore label, DC_and_BCE_loss with MemoryEfficientSoftDiceLoss) imported through oracle.refshim.  Runs only where the reference tree
exists; the tests read the committed .npz.

Each case stores the fp32 logits, the labels (and the one-hot region target), the fp64 loss and d loss / d logits.  The world-2 cases
come from two gloo ranks on the CPU with ddp=True (AllGatherGrad Dice sums, ddp_allgather.py:25-48); rank 1's pixels are all ignored.

    python tools/make_golden_seg_loss.py
"""
import json
import os
import socket
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "seg_loss_reference.npz")
SMOOTH = 1e-5

# (name, kind, shape (B, K or R, H, W), regions, ignore_label)
CASES = [
    ("ce_ignore", "softmax", (2, 4, 32, 32), None, 4),
    ("ce_all_ignored", "softmax", (1, 3, 16, 16), None, 3),
    ("regions_ignore", "regions", (2, 3, 32, 32), [(1, 2, 3), (2, 3), (3,)], 4),
    ("regions_tail", "regions", (2, 2, 17, 23), [1, (1, 2)], None),
]
DDP_CASES = [
    ("ddp_ce_ignore", "softmax", (2, 3, 16, 16), None, 3),
    ("ddp_regions_ignore", "regions", (2, 2, 16, 16), [(1, 2), (2,)], 3),
]


def reference_classes():
    """DC_and_CE_loss, DC_and_BCE_loss, MemoryEfficientSoftDiceLoss of the reference tree (refshim import path)"""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from oracle import refshim
    refshim.install()
    sys.modules["dinounet.training"].__path__ = [os.path.join(refshim.REF_ROOT, "dinounet", "training")]
    from dinounet.training.loss.compound_losses import DC_and_BCE_loss, DC_and_CE_loss
    from dinounet.training.loss.dice import MemoryEfficientSoftDiceLoss
    return DC_and_CE_loss, DC_and_BCE_loss, MemoryEfficientSoftDiceLoss


def reference_loss(kind, ignore_label, ddp=False):
    """the loss module nnUNetTrainer._build_loss builds (batch_dice=True, no deep supervision)"""
    DC_and_CE_loss, DC_and_BCE_loss, MSD = reference_classes()
    if kind == "regions":
        return DC_and_BCE_loss({}, {"batch_dice": True, "do_bg": True, "smooth": SMOOTH, "ddp": ddp},
                               use_ignore_label=ignore_label is not None, dice_class=MSD)
    return DC_and_CE_loss({"batch_dice": True, "smooth": SMOOTH, "do_bg": False, "ddp": ddp}, {}, weight_ce=1, weight_dice=1,
                          ignore_label=ignore_label, dice_class=MSD)


def make_labels(shape, kind, regions, ignore_label, seed, ignored_frac=0.3):
    """(B,1,H,W) int64 labels: classes 0..K-1 (softmax) / 0..max region label (regions), about `ignored_frac` of them the ignore label"""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    top = C if kind == "softmax" else max(max((r,) if isinstance(r, int) else r) for r in regions) + 1
    lab = torch.randint(0, top, (B, 1, H, W), generator=g)
    if ignore_label is not None:
        lab = torch.where(torch.rand((B, 1, H, W), generator=g) < ignored_frac, torch.full_like(lab, ignore_label), lab)
    return lab


def regions_onehot(lab, regions, ignore_label):
    """ConvertSegmentationToRegionsTransform (region_based_training.py:23-37) with the ignore label appended as the last region"""
    planes = []
    for r in list(regions) + ([ignore_label] if ignore_label is not None else []):
        m = torch.zeros_like(lab[:, 0], dtype=torch.bool)
        for l in ((r,) if isinstance(r, int) else r):
            m |= lab[:, 0] == l
        planes.append(m)
    return torch.stack(planes, 1).to(torch.uint8)


def reference_eval(kind, logits32, lab, regions, ignore_label, ddp=False):
    """fp64 loss and d loss / d logits of the reference classes on fp32 inputs"""
    x = logits32.double().requires_grad_(True)
    if kind == "regions":
        tgt = regions_onehot(lab, regions, ignore_label).double()
    else:
        tgt = lab.double()                      # the trainer's target is float (NumpyToTensor 'float', nnUNetTrainer.py:771)
    loss = reference_loss(kind, ignore_label, ddp)(x, tgt)
    loss.backward()
    return float(loss.detach()), x.grad.numpy().copy()


def _case_inputs(shape, kind, regions, ignore_label, seed):
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(shape, generator=g) * 2.0).float()
    return logits, make_labels(shape, kind, regions, ignore_label, seed + 1)


def _ddp_worker(rank, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=2)
    out = {}
    for i, (name, kind, shape, regions, ig) in enumerate(DDP_CASES):
        logits, lab = _case_inputs(shape, kind, regions, ig, 100 + 10 * i)
        lab[1:] = ig                            # rank 1: every pixel ignored
        loss, grad = reference_eval(kind, logits[rank:rank + 1], lab[rank:rank + 1], regions, ig, ddp=True)
        out[name] = (logits.numpy(), lab.numpy(), loss, grad)
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def main():
    torch.set_default_dtype(torch.float32)
    arrays, meta = {}, {"smooth": SMOOTH, "cases": []}
    for i, (name, kind, shape, regions, ig) in enumerate(CASES):
        logits, lab = _case_inputs(shape, kind, regions, ig, 10 * i)
        if name == "ce_all_ignored":
            lab[:] = ig
        loss, grad = reference_eval(kind, logits, lab, regions, ig)
        arrays[f"{name}/logits"] = logits.numpy()
        arrays[f"{name}/labels"] = lab.numpy().astype(np.int16)
        if kind == "regions":
            arrays[f"{name}/onehot"] = regions_onehot(lab, regions, ig).numpy()
        arrays[f"{name}/loss"] = np.array(loss, dtype=np.float64)
        arrays[f"{name}/grad"] = grad
        meta["cases"].append({"name": name, "kind": kind, "shape": list(shape), "regions": regions, "ignore_label": ig, "world": 1})
        print(f"{name}: loss {loss:.10f}")
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_ddp_worker, args=(r, port, q)) for r in range(2)]
    [p.start() for p in procs]
    res = dict(q.get(timeout=300) for _ in range(2))
    [p.join(timeout=60) for p in procs]
    assert all(p.exitcode == 0 for p in procs)
    for name, kind, shape, regions, ig in DDP_CASES:
        logits, lab = res[0][name][0], res[0][name][1]
        arrays[f"{name}/logits"] = logits
        arrays[f"{name}/labels"] = lab.astype(np.int16)
        if kind == "regions":
            arrays[f"{name}/onehot"] = regions_onehot(torch.from_numpy(lab), regions, ig).numpy()
        arrays[f"{name}/loss"] = np.array([res[r][name][2] for r in range(2)], dtype=np.float64)       # per rank
        arrays[f"{name}/grad"] = np.concatenate([res[r][name][3] for r in range(2)], 0)                # rank r's slice of the batch
        meta["cases"].append({"name": name, "kind": kind, "shape": list(shape), "regions": regions, "ignore_label": ig, "world": 2})
        print(f"{name}: per-rank loss {arrays[f'{name}/loss']}")
    np.savez_compressed(OUT, meta=json.dumps(meta), **arrays)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
