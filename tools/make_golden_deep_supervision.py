"""Generate tests/golden/deep_supervision_reference.npz: the reference trainer's deep-supervision loss on fixed fp32 inputs, evaluated in
fp64 on the CPU by the reference's own classes imported through oracle.refshim -- DeepSupervisionWrapper
(training/loss/deep_supervision.py) around DC_and_CE_loss / DC_and_BCE_loss with MemoryEfficientSoftDiceLoss, the weights of
nnUNetTrainer._build_loss (nnUNetTrainer.py:373-387).  The target list is what DownsampleSegForDSTransform2 (order 0) makes of the
full-resolution labels: batchgenerators' resize_segmentation(order=0) is skimage resize(order=0, mode="edge", anti_aliasing=False), i.e.
scipy.ndimage.zoom(order=0, mode="nearest", grid_mode=True); neither skimage nor batchgenerators is needed, scipy's zoom is called here.
In region mode the labels are converted to one-hot planes first and every plane is resampled, the order the reference's transforms run in.
Runs only where the reference tree exists; the tests read the committed .npz.

Each case stores the fp32 logits of every scale, the full-resolution labels, the fp64 loss and d loss / d logits of every scale with a
non-zero weight.  The world-2 case comes from two gloo ranks on the CPU with ddp=True.  meta also holds the weights and scales the tests
compare deep_supervision_weights / deep_supervision_scales with, computed here with numpy as the trainer computes them.

    python tools/make_golden_deep_supervision.py
"""
import json
import os
import sys

import numpy as np
import torch
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_seg_loss as G  # noqa: E402  (reference_loss, make_labels, regions_onehot, _free_port)

OUT = os.path.join(ROOT, "tests", "golden", "deep_supervision_reference.npz")


def trainer_weights(n, ddp):
    w = np.array([1 / (2 ** i) for i in range(n)])
    w[-1] = 1e-6 if ddp else 0
    return w / w.sum()


def trainer_scales(pool_op_kernel_sizes):
    return [list(i) for i in 1 / np.cumprod(np.vstack(pool_op_kernel_sizes), axis=0)][:-1]


# (name, kind, logits shape of scale 0, lower-scale (h, w), regions, ignore_label, ddp weights)
CASES = [
    ("ds_plain", "softmax", (2, 3, 16, 16), [(8, 8), (4, 4)], None, None, False),
    ("ds_ce_ignore", "softmax", (2, 4, 20, 12), [(10, 6), (5, 3)], None, 4, True),
    ("ds_regions_ignore", "regions", (2, 3, 18, 10), [(9, 5), (4, 2)], [(1, 2, 3), (2, 3), (3,)], 4, True),
]
DDP_CASES = [
    ("ds_ddp_ce_ignore", "softmax", (2, 3, 16, 16), [(8, 8)], None, 3, True),
]
POOLS = [[[1, 1], [2, 2], [2, 2], [2, 2]], [[1, 1], [2, 2], [2, 2], [2, 2], [2, 2], [2, 2], [2, 2]], [[1, 1], [2, 1], [2, 2], [1, 2]]]


def zoom0(a, hw):
    """resize_segmentation(order=0) of one 2-D map"""
    H, W = a.shape
    out = ndimage.zoom(a, (hw[0] / H, hw[1] / W), order=0, mode="nearest", grid_mode=True)
    assert out.shape == tuple(hw), (out.shape, hw)
    return out


def downsample(t, hw):
    """(B,C,H,W) tensor -> (B,C,h,w), channel by channel as DownsampleSegForDSTransform2 does"""
    a = t.numpy()
    return torch.from_numpy(np.stack([np.stack([zoom0(a[b, c], hw) for c in range(a.shape[1])]) for b in range(a.shape[0])]))


def inputs(shape, lower, kind, regions, ig, seed):
    g = torch.Generator().manual_seed(seed)
    B, C = shape[:2]
    logits = [(torch.randn((B, C, h, w), generator=g) * 2.0).float() for h, w in [shape[2:]] + list(lower)]
    return logits, G.make_labels(shape, kind, regions, ig, seed + 1)


def reference_eval(kind, logits32, lab, regions, ig, weights, ddp=False):
    from dinounet.training.loss.deep_supervision import DeepSupervisionWrapper
    xs = [x.double().requires_grad_(True) for x in logits32]
    full = G.regions_onehot(lab, regions, ig) if kind == "regions" else lab
    tgts = [downsample(full, tuple(x.shape[2:])).double() for x in xs]
    assert torch.equal(tgts[0], full.double())
    loss = DeepSupervisionWrapper(G.reference_loss(kind, ig, ddp), weights)(xs, tgts)
    loss.backward()
    return float(loss.detach()), [None if x.grad is None else x.grad.numpy().copy() for x in xs]


def _ddp_worker(rank, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=2)
    G.reference_classes()
    out = {}
    for i, (name, kind, shape, lower, regions, ig, ddpw) in enumerate(DDP_CASES):
        logits, lab = inputs(shape, lower, kind, regions, ig, 300 + 10 * i)
        w = trainer_weights(1 + len(lower), ddpw)
        loss, grads = reference_eval(kind, [x[rank:rank + 1] for x in logits], lab[rank:rank + 1], regions, ig, w, ddp=True)
        out[name] = ([x.numpy() for x in logits], lab.numpy(), loss, grads)
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def main():
    torch.set_default_dtype(torch.float32)
    G.reference_classes()
    arrays, meta = {}, {"smooth": G.SMOOTH, "cases": []}
    meta["weights"] = {f"{n}/{int(d)}": [float(v) for v in trainer_weights(n, d)] for n in (2, 3, 4, 5) for d in (False, True)}
    meta["scales"] = [{"pool": p, "scales": [[float(v) for v in s] for s in trainer_scales(p)]} for p in POOLS]
    for i, (name, kind, shape, lower, regions, ig, ddpw) in enumerate(CASES):
        logits, lab = inputs(shape, lower, kind, regions, ig, 200 + 10 * i)
        w = trainer_weights(len(logits), ddpw)
        loss, grads = reference_eval(kind, logits, lab, regions, ig, w)
        for s, x in enumerate(logits):
            arrays[f"{name}/logits{s}"] = x.numpy()
            if grads[s] is not None:
                arrays[f"{name}/grad{s}"] = grads[s]
        arrays[f"{name}/labels"] = lab.numpy().astype(np.int16)
        arrays[f"{name}/loss"] = np.array(loss, dtype=np.float64)
        meta["cases"].append({"name": name, "kind": kind, "shape": list(shape), "lower": [list(l) for l in lower], "regions": regions,
                              "ignore_label": ig, "weights": [float(v) for v in w], "world": 1})
        print(f"{name}: loss {loss:.10f}, gradients for scales {[s for s, g_ in enumerate(grads) if g_ is not None]}")
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = G._free_port()
    procs = [ctx.Process(target=_ddp_worker, args=(r, port, q)) for r in range(2)]
    [p.start() for p in procs]
    res = dict(q.get(timeout=300) for _ in range(2))
    [p.join(timeout=60) for p in procs]
    assert all(p.exitcode == 0 for p in procs)
    for name, kind, shape, lower, regions, ig, ddpw in DDP_CASES:
        logits, lab = res[0][name][0], res[0][name][1]
        for s, x in enumerate(logits):
            arrays[f"{name}/logits{s}"] = x
            arrays[f"{name}/grad{s}"] = np.concatenate([res[r][name][3][s] for r in range(2)], 0)     # rank r's slice of the batch
        arrays[f"{name}/labels"] = lab.astype(np.int16)
        arrays[f"{name}/loss"] = np.array([res[r][name][2] for r in range(2)], dtype=np.float64)      # per rank
        meta["cases"].append({"name": name, "kind": kind, "shape": list(shape), "lower": [list(l) for l in lower], "regions": regions,
                              "ignore_label": ig, "weights": [float(v) for v in trainer_weights(1 + len(lower), ddpw)], "world": 2})
        print(f"{name}: per-rank loss {arrays[f'{name}/loss']}")
    np.savez_compressed(OUT, meta=json.dumps(meta), **arrays)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
