"""Generate tests/golden/topk_loss_reference.npz: the reference's top-k losses (TopKLoss, robust_ce_loss.py:19-32; DC_and_topk_loss,
compound_losses.py:102-150, with SoftDiceLoss(softmax, batch_dice=True, do_bg=False, smooth=1e-5)) on fixed fp32 inputs, evaluated in
fp64 on the CPU by the reference's own classes imported through oracle.refshim.  Runs only where the reference tree exists; the tests
read the committed .npz.

Each case stores the fp32 logits, the labels, the fp64 loss and d loss / d logits, k_vox, the fp64 threshold (the k_vox-th largest
per-voxel CE) and the gap to the next value below it.  torch.topk leaves the choice among equal values open and the package breaks ties
its own way, so whole gradients are comparable only where the threshold is isolated: the generator asserts a gap of at least 1e-3 (ten
times the kernels' per-element bound 2e-5 max(1, v) at these thresholds, < 5).  The all-ignored case is exempt: every CE is 0, the
selection is all ties, and every gradient is 0 whatever is selected.  The world-2 case comes from two gloo ranks on the CPU with ddp=True
(AllGatherGrad Dice sums, one sample per rank; the top-k is each rank's own).

    python tools/make_golden_topk_loss.py
"""
import json
import os
import socket
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "topk_loss_reference.npz")
SMOOTH = 1e-5
MIN_GAP = 1e-3

# (name, kind, shape (B, K, H, W), ignore_label, k percent, seed); kind "dc_topk" = DC_and_topk_loss, "topk" = TopKLoss alone
CASES = [
    ("plain", "dc_topk", (2, 3, 32, 32), None, 10, 0),
    ("ignore", "dc_topk", (2, 4, 32, 32), 4, 10, 10),
    ("tail", "dc_topk", (3, 4, 17, 23), None, 10, 20),
    ("k8", "dc_topk", (1, 8, 32, 32), None, 25, 30),
    ("half_ignore", "dc_topk", (1, 3, 16, 16), 3, 50, 50),
    ("all_ignored", "dc_topk", (1, 3, 16, 16), 3, 10, 60),
    ("topk_only", "topk", (2, 3, 32, 32), None, 10, 70),
]
DDP_CASES = [
    ("ddp", "dc_topk", (2, 3, 16, 16), 3, 10, 80),
]


def reference_loss(kind, ignore_label, k, ddp=False):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from oracle import refshim
    refshim.install()
    sys.modules["dinounet.training"].__path__ = [os.path.join(refshim.REF_ROOT, "dinounet", "training")]
    from dinounet.training.loss.compound_losses import DC_and_topk_loss
    from dinounet.training.loss.robust_ce_loss import TopKLoss
    if kind == "topk":
        return TopKLoss(k=k) if ignore_label is None else TopKLoss(k=k, ignore_index=ignore_label)
    return DC_and_topk_loss({"batch_dice": True, "smooth": SMOOTH, "do_bg": False, "ddp": ddp}, {"k": k}, weight_ce=1, weight_dice=1,
                            ignore_label=ignore_label)


def case_inputs(shape, ignore_label, seed):
    """one generator, in this order: logits, labels, (with an ignore label) the ignored voxels"""
    B, K, H, W = shape
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(shape, generator=g) * 2).float()
    lab = torch.randint(0, K, (B, 1, H, W), generator=g)
    if ignore_label is not None:
        lab = torch.where(torch.rand((B, 1, H, W), generator=g) < 0.3, torch.full_like(lab, ignore_label), lab)
    return logits, lab


def threshold_gap(logits32, lab, ignore_label, k):
    """k_vox, the fp64 threshold and its distance to the next smaller per-voxel CE"""
    v = torch.nn.functional.cross_entropy(logits32.double(), lab[:, 0].long(), reduction="none",
                                          ignore_index=-100 if ignore_label is None else ignore_label).reshape(-1)
    k_vox = int(np.int64(v.numel()) * k / 100)
    s = torch.sort(v, descending=True)[0]
    return k_vox, float(s[k_vox - 1]), float(s[k_vox - 1] - s[k_vox]) if k_vox < v.numel() else float("inf")


def reference_eval(kind, logits32, lab, ignore_label, k, ddp=False):
    """fp64 loss and d loss / d logits of the reference classes on fp32 inputs"""
    x = logits32.double().requires_grad_(True)
    loss = reference_loss(kind, ignore_label, k, ddp)(x, lab.clone())
    loss.backward()
    return float(loss.detach()), x.grad.numpy().copy()


def _ddp_worker(rank, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=2)
    out = {}
    for name, kind, shape, ig, k, seed in DDP_CASES:
        logits, lab = case_inputs(shape, ig, seed)
        loss, grad = reference_eval(kind, logits[rank:rank + 1], lab[rank:rank + 1], ig, k, ddp=True)
        out[name] = (logits.numpy(), lab.numpy(), loss, grad)
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def main():
    torch.set_default_dtype(torch.float32)
    arrays, meta = {}, {"smooth": SMOOTH, "cases": []}
    for name, kind, shape, ig, k, seed in CASES:
        logits, lab = case_inputs(shape, ig, seed)
        if name == "all_ignored":
            lab[:] = ig
        k_vox, thr, gap = threshold_gap(logits, lab, ig, k)
        assert name == "all_ignored" or gap >= MIN_GAP, (name, gap)
        loss, grad = reference_eval(kind, logits, lab, ig, k)
        arrays[f"{name}/logits"] = logits.numpy()
        arrays[f"{name}/labels"] = lab.numpy().astype(np.int16)
        arrays[f"{name}/loss"] = np.array(loss, dtype=np.float64)
        arrays[f"{name}/grad"] = grad
        arrays[f"{name}/k_vox"] = np.array(k_vox, dtype=np.int64)
        arrays[f"{name}/threshold"] = np.array(thr, dtype=np.float64)
        arrays[f"{name}/gap"] = np.array(gap, dtype=np.float64)
        meta["cases"].append({"name": name, "kind": kind, "shape": list(shape), "ignore_label": ig, "k": k, "seed": seed, "world": 1})
        print(f"{name}: loss {loss:.10f} k_vox {k_vox} threshold {thr:.6f} gap {gap:.3g}")
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_ddp_worker, args=(r, port, q)) for r in range(2)]
    [p.start() for p in procs]
    res = dict(q.get(timeout=300) for _ in range(2))
    [p.join(timeout=60) for p in procs]
    assert all(p.exitcode == 0 for p in procs)
    for name, kind, shape, ig, k, seed in DDP_CASES:
        logits, lab = torch.from_numpy(res[0][name][0]), torch.from_numpy(res[0][name][1])
        per_rank = [threshold_gap(logits[r:r + 1], lab[r:r + 1], ig, k) for r in range(2)]
        assert all(g >= MIN_GAP for _, _, g in per_rank), (name, per_rank)
        arrays[f"{name}/logits"] = logits.numpy()
        arrays[f"{name}/labels"] = lab.numpy().astype(np.int16)
        arrays[f"{name}/loss"] = np.array([res[r][name][2] for r in range(2)], dtype=np.float64)       # per rank
        arrays[f"{name}/grad"] = np.concatenate([res[r][name][3] for r in range(2)], 0)                # rank r's slice of the batch
        arrays[f"{name}/k_vox"] = np.array([p[0] for p in per_rank], dtype=np.int64)
        arrays[f"{name}/threshold"] = np.array([p[1] for p in per_rank], dtype=np.float64)
        arrays[f"{name}/gap"] = np.array([p[2] for p in per_rank], dtype=np.float64)
        meta["cases"].append({"name": name, "kind": kind, "shape": list(shape), "ignore_label": ig, "k": k, "seed": seed, "world": 2})
        print(f"{name}: per-rank loss {arrays[f'{name}/loss']} k_vox {per_rank[0][0]} gaps {[p[2] for p in per_rank]}")
    np.savez_compressed(OUT, meta=json.dumps(meta), **arrays)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
