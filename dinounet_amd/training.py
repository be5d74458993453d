"""Synthetic-data training-step harness replicating the reference trainer's `train_step`
(dinounet/training/nnUNetTrainer/nnUNetTrainer.py:899-929): forward -> DC+CE loss -> backward -> clip_grad_norm_(12)
-> SGD(nesterov, momentum 0.99, wd 3e-5).  On the GPU the loss is the fused Dice+CE kernel pair (csrc/loss.hip) and clip + SGD the
fused three-launch optimiser (csrc/optim.hip); the torch formula below serves the CPU / many-class path of the gloo tests.
build_loss covers the trainer's other label configurations (ignore label, regions: nnUNetTrainer.py:355-365) and, with
deep_supervision_weights, the DeepSupervisionWrapper around them (DeepSupervisionLoss: one fused multi-scale pass); ValStep / validation_counts
are the validation half of the epoch (validation_step / on_validation_epoch_end, nnUNetTrainer.py:946-1052)."""
import os
import threading

import torch
import torch.distributed as dist
import torch.nn.functional as F

from .optim import FusedClipSGD

# test configuration (ops.sync_active): the SyncBatchNorm / batch-Dice collectives issued on a one-rank group as well
_FORCE_SMALL = os.environ.get("DINOUNET_FORCE_SMALL_COLLECTIVES") == "1"


def _ddp_default(group):
    return dist.is_available() and dist.is_initialized() and (dist.get_world_size(group) > 1 or _FORCE_SMALL)


def _loss_group(ddp, group):
    """the group argument of a fused loss: the process group its Dice sums are all-reduced over, None for a local loss"""
    return (group if group is not None else dist.group.WORLD) if ddp else None


class _AllReduceSumGrad(torch.autograd.Function):
    """dinounet/utilities/ddp_allgather.py:25-48 followed by .sum(0): all-gather forward / all-reduce backward."""

    @staticmethod
    def forward(ctx, x, group):
        ctx.group = group
        y = x.clone()
        dist.all_reduce(y, group=group)
        return y

    @staticmethod
    def backward(ctx, g):
        g = g.clone()
        dist.all_reduce(g, group=ctx.group)
        return g, None


def check_loss_options(num_classes, regions=None, topk_percent=None, weight_ce=1.0, weight_dice=1.0, batch_dice=True, do_bg=None,
                       ce_class_weights=None):
    """The options of the reference's loss classes that the trainer freezes (DC_and_CE_loss / DC_and_BCE_loss weight_ce, weight_dice;
    MemoryEfficientSoftDiceLoss batch_dice, do_bg; ce_kwargs={'weight': w}), validated on the host -> (weight_ce, weight_dice,
    batch_dice, do_bg, class weights as a tuple or None, options_default).  do_bg None is the trainer's choice: False for softmax,
    True for regions.  ValueError for: both weights 0; a negative or non-finite weight; a class weight <= 0 or not finite, or not
    num_classes of them; ce_class_weights or do_bg=False together with regions; any non-default option together with topk_percent."""
    import math
    for name, v in (("weight_ce", weight_ce), ("weight_dice", weight_dice)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
            raise ValueError(f"{name} must be a finite number >= 0, got {v!r}")
    weight_ce, weight_dice = float(weight_ce), float(weight_dice)
    if weight_ce == 0.0 and weight_dice == 0.0:
        raise ValueError("weight_ce and weight_dice are both 0: no loss is left")
    if not isinstance(batch_dice, bool):
        raise ValueError(f"batch_dice must be a bool, got {batch_dice!r}")
    if do_bg is not None and not isinstance(do_bg, bool):
        raise ValueError(f"do_bg must be None or a bool, got {do_bg!r}")
    cw = None
    if ce_class_weights is not None:
        cw = tuple(float(v) for v in (ce_class_weights.tolist() if isinstance(ce_class_weights, torch.Tensor) else ce_class_weights))
        if regions is not None:
            raise ValueError("ce_class_weights with regions: BCEWithLogitsLoss has no class weights (pos_weight is out of scope)")
        if len(cw) != num_classes:
            raise ValueError(f"ce_class_weights: {len(cw)} weights for {num_classes} classes")
        if not all(math.isfinite(v) and v > 0 for v in cw):
            raise ValueError(f"ce_class_weights must be positive finite numbers, got {cw!r}")
    if regions is not None and do_bg is False:
        raise ValueError("do_bg=False with regions: every region is a foreground structure (the reference uses do_bg=True there)")
    bg = (regions is not None) if do_bg is None else do_bg
    default = (weight_ce == 1.0 and weight_dice == 1.0 and batch_dice and cw is None and bg == (regions is not None))
    if topk_percent is not None and not default:
        raise ValueError("loss options (weight_ce, weight_dice, batch_dice, do_bg, ce_class_weights) are not available together with "
                         "topk_percent: the top-k family stays at the trainer's defaults")
    return weight_ce, weight_dice, batch_dice, bg, cw, default


def _dice_term(inter, sum_pred, sum_gt, smooth, batch_dice, ddp, group):
    """MemoryEfficientSoftDiceLoss's mean Dice from per-(sample, class) sums (B, C), dice.py:106-118: batch_dice adds over the batch
    (globally under DDP), otherwise dc stays (B, C), nothing is gathered, and the mean runs over both axes"""
    if batch_dice:
        return _global_dice(inter, sum_pred, sum_gt, smooth, ddp, group)
    return ((2 * inter + smooth) / torch.clip(sum_gt + sum_pred + smooth, 1e-8)).mean()


def _dc_and_ce_opt_torch(logits, target, ignore_label, smooth, ddp, group, weight_ce, weight_dice, batch_dice, do_bg, class_w):
    """DC_and_CE_loss with every option, in torch: the CPU / many-class path and, in fp64, the oracle of csrc/loss_opt.hip.
    CE = sum_valid w_t nll / sum_valid w_t (F.cross_entropy(weight=w, ignore_index) = torch's weighted mean), exactly 0 when the
    denominator is 0, decided without a host read; a term whose weight is 0 is not computed (compound_losses.py:50-55)."""
    lab = target[:, 0].long()
    m = (lab != ignore_label) if ignore_label is not None else torch.ones_like(lab, dtype=torch.bool)
    lab0 = torch.where(m, lab, torch.zeros_like(lab))
    mf = m[:, None].to(logits.dtype)
    total = None
    if weight_ce != 0:
        nll = -torch.log_softmax(logits, 1).gather(1, lab0[:, None])
        wt = mf if class_w is None else class_w.to(logits.dtype)[lab0][:, None] * mf
        den = wt.sum()
        total = weight_ce * ((nll * wt).sum() / torch.where(den > 0, den, torch.ones_like(den)))
    if weight_dice != 0:
        c0 = 0 if do_bg else 1
        prob = torch.softmax(logits, 1)
        with torch.no_grad():
            onehot = torch.zeros(prob.shape, device=prob.device, dtype=prob.dtype).scatter_(1, lab0[:, None], 1)[:, c0:] * mf
            sum_gt = onehot.sum((2, 3))
        p = prob[:, c0:] * mf
        dc = weight_dice * _dice_term((p * onehot).sum((2, 3)), p.sum((2, 3)), sum_gt, smooth, batch_dice, ddp, group)
        total = -dc if total is None else total - dc
    return total


def _dc_and_bce_opt_torch(logits, target, u, smooth, ddp, group, weight_ce, weight_dice, batch_dice):
    """DC_and_BCE_loss with weight_ce, weight_dice and batch_dice, in torch (CPU path and fp64 oracle); target (B, R + u, H, W)"""
    R = logits.shape[1]
    y = target[:, :R].to(logits.dtype)
    mf = (1 - target[:, -1:]).bool().to(logits.dtype) if u else None
    total = None
    if weight_ce != 0:
        bce = F.binary_cross_entropy_with_logits(logits, y, reduction="none")
        total = weight_ce * ((bce * mf).sum() / torch.clip(mf.sum(), min=1e-8) if u else bce.mean())
    if weight_dice != 0:
        x = torch.sigmoid(logits)
        if u:
            y, x = y * mf, x * mf
        dc = weight_dice * _dice_term((x * y).sum((2, 3)), x.sum((2, 3)), y.sum((2, 3)), smooth, batch_dice, ddp, group)
        total = -dc if total is None else total - dc
    return total


def _class_w_tensor(ce_class_weights, device, dtype=torch.float32):
    """the class weights as a tensor: fp32 for the kernels, the logits' dtype for the torch formula"""
    if ce_class_weights is None:
        return None
    if isinstance(ce_class_weights, torch.Tensor):
        return ce_class_weights.to(device=device, dtype=dtype)
    return torch.tensor([float(v) for v in ce_class_weights], dtype=dtype, device=device)


def dc_and_ce_loss(logits, target, smooth=1e-5, ddp=None, group=None, ignore_label=None, weight_ce=1.0, weight_dice=1.0, batch_dice=True,
                   do_bg=None, ce_class_weights=None):
    """DC_and_CE_loss (compound_losses.py:8-56) with MemoryEfficientSoftDiceLoss(batch_dice=True, do_bg=False,
    smooth=1e-5) (dice.py:58-119, trainer config nnUNetTrainer.py:363-365).  target (B,1,H,W) integer labels.
    On the GPU (2..8 classes) this is the fused HIP loss (ops.dice_ce_loss); the torch formula below is the CPU / many-class path
    used by the gloo tests.  With `ignore_label` the pixels carrying it are masked out (compound_losses.py:38-53): see
    _dc_and_ce_masked.
    weight_ce, weight_dice, batch_dice, do_bg and ce_class_weights (K weights, a sequence or a tensor) are the options of the reference's
    classes (check_loss_options); at their defaults the code below runs as before, otherwise the fused option loss
    (ops.dice_ce_opt_loss, csrc/loss_opt.hip) on the GPU and _dc_and_ce_opt_torch elsewhere."""
    weight_ce, weight_dice, batch_dice, do_bg, cw, default = check_loss_options(
        logits.shape[1], None, None, weight_ce, weight_dice, batch_dice, do_bg,
        None if isinstance(ce_class_weights, torch.Tensor) else ce_class_weights)
    if isinstance(ce_class_weights, torch.Tensor):        # a prepared device tensor (SegLoss validated its values): no read-back here
        if ce_class_weights.numel() != logits.shape[1]:
            raise ValueError(f"ce_class_weights: {ce_class_weights.numel()} weights for {logits.shape[1]} classes")
        default = False
    if not default:
        K = logits.shape[1]
        if ddp is None:
            ddp = _ddp_default(group)
        if logits.is_cuda and 2 <= K <= 8:
            from . import ops
            class_w = _class_w_tensor(ce_class_weights, logits.device)
            return ops.dice_ce_opt_loss(logits, target, ignore_label, do_bg, batch_dice, weight_ce, weight_dice, class_w, smooth,
                                        _loss_group(ddp, group))
        class_w = _class_w_tensor(ce_class_weights, logits.device, logits.dtype)
        return _dc_and_ce_opt_torch(logits, target, ignore_label, smooth, ddp, group, weight_ce, weight_dice, batch_dice, do_bg, class_w)
    if ignore_label is not None:
        return _dc_and_ce_masked(logits, target, ignore_label, smooth, ddp, group)
    K = logits.shape[1]
    if logits.is_cuda and 2 <= K <= 8:
        from . import ops
        if ddp is None:
            ddp = _ddp_default(group)
        return ops.dice_ce_loss(logits, target, smooth, _loss_group(ddp, group))
    lab = target[:, 0].long()
    ce = F.cross_entropy(logits, lab)
    prob = torch.softmax(logits, 1)
    with torch.no_grad():
        onehot = torch.zeros(prob.shape, device=prob.device, dtype=torch.bool).scatter_(1, lab[:, None], 1)[:, 1:]
        sum_gt = onehot.sum((2, 3))
    p = prob[:, 1:]
    inter = (p * onehot).sum((2, 3))
    sum_pred = p.sum((2, 3))
    if ddp is None:
        ddp = _ddp_default(group)
    inter, sum_pred, sum_gt = inter.sum(0), sum_pred.sum(0), sum_gt.sum(0).to(p.dtype)
    if ddp:
        inter = _AllReduceSumGrad.apply(inter, group)
        sum_pred = _AllReduceSumGrad.apply(sum_pred, group)
        sum_gt = _AllReduceSumGrad.apply(sum_gt, group)
    dc = (2 * inter + smooth) / torch.clip(sum_gt + sum_pred + smooth, 1e-8)
    return ce - dc.mean()


def _global_dice(inter, sum_pred, sum_gt, smooth, ddp, group):
    """batch Dice from per-(sample, class) sums (B, C); under DDP the sums are global (dice.py:106-114), the rest stays local"""
    if ddp is None:
        ddp = _ddp_default(group)
    inter, sum_pred, sum_gt = inter.sum(0), sum_pred.sum(0), sum_gt.sum(0)
    if ddp:
        inter = _AllReduceSumGrad.apply(inter, group)
        sum_pred = _AllReduceSumGrad.apply(sum_pred, group)
        sum_gt = _AllReduceSumGrad.apply(sum_gt, group)
    return ((2 * inter + smooth) / torch.clip(sum_gt + sum_pred + smooth, 1e-8)).mean()


def _dc_and_ce_masked(logits, target, ignore_label, smooth=1e-5, ddp=None, group=None):
    """DC_and_CE_loss(ignore_label) (compound_losses.py:31-56, dice.py:72-119 with loss_mask, do_bg=False): m = [t != ignore];
    CE = mean of -log p_t over valid pixels, exactly 0 when there is none -- decided without a host read (the reference's `num_fg > 0`
    test, :53, is a sync no captured step can hold); Dice over classes 1..K-1 with p and the one-hot target multiplied by m.
    On the GPU (2..8 classes) the fused HIP loss (ops.dice_ce_masked_loss); the torch formula below is the CPU / many-class path."""
    K = logits.shape[1]
    if logits.is_cuda and 2 <= K <= 8:
        from . import ops
        if ddp is None:
            ddp = _ddp_default(group)
        return ops.dice_ce_masked_loss(logits, target, ignore_label, smooth, _loss_group(ddp, group))
    lab = target[:, 0].long()
    m = lab != ignore_label
    lab0 = torch.where(m, lab, torch.zeros_like(lab))
    mf = m[:, None].to(logits.dtype)
    logp = torch.log_softmax(logits, 1)
    nll = -logp.gather(1, lab0[:, None])
    ce = (nll * mf).sum() / m.sum().clamp_min(1).to(logits.dtype)       # n_valid = 0: the sum is 0, so is CE
    prob = torch.softmax(logits, 1)
    with torch.no_grad():
        onehot = torch.zeros(prob.shape, device=prob.device, dtype=prob.dtype).scatter_(1, lab0[:, None], 1)[:, 1:] * mf
        sum_gt = onehot.sum((2, 3))
    p = prob[:, 1:] * mf
    return ce - _global_dice((p * onehot).sum((2, 3)), p.sum((2, 3)), sum_gt, smooth, ddp, group)


def check_topk_percent(k):
    """ValueError unless k is a percentage in (0, 100] (any such k is valid: whether it selects a voxel depends on the shape)"""
    if isinstance(k, bool) or not isinstance(k, (int, float)) or not 0 < k <= 100:
        raise ValueError(f"top-k loss: k must be a percentage in (0, 100], got {k!r}")


def topk_voxels(n_voxels, k):
    """k_vox of TopKLoss (robust_ce_loss.py:30-31), in its arithmetic: int(np.int64(N) * k / 100), N counting ignored voxels too.
    ValueError for k outside (0, 100] and for k_vox < 1 -- the reference takes the mean of an empty topk there and returns nan."""
    import numpy as np
    check_topk_percent(k)
    k_vox = int(np.int64(n_voxels) * k / 100)
    if k_vox < 1:
        raise ValueError(f"top-k loss: k = {k} % of {n_voxels} voxels selects none (the reference returns nan here)")
    return k_vox


def _topk_ce_torch(logits, target, k, ignore_label):
    """TopKLoss (robust_ce_loss.py:19-32) in torch: the CPU / many-class path and the fp64 oracle of the fused kernels.  On the GPU it
    refuses to be captured: a hipGraph holding torch.topk faulted with an illegal memory access when it was replayed
    (tools/bench_topk_loss.py, (8, 3, 512, 512), k = 10 %; the runtime's dump named a kernel of torch.topk's sort, why it faults under
    replay is not known); TrainStep / ValStep then fall back to eager steps with a warning.  The fused route has no such limit."""
    if logits.is_cuda and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("top-k loss: the torch formula (more than 8 classes, or 2^31 voxels and more) cannot be captured into a "
                           "hipGraph; run eager steps")
    v = F.cross_entropy(logits, target[:, 0].long(), reduction="none", ignore_index=-100 if ignore_label is None else ignore_label)
    return torch.topk(v.reshape(-1), topk_voxels(v.numel(), k), sorted=False)[0].mean()


def _soft_dice_torch(logits, target, ignore_label, smooth, ddp, group):
    """SoftDiceLoss(softmax, batch_dice=True, do_bg=False, smooth) as DC_and_topk_loss calls it (compound_losses.py:131-145): with an
    ignore label the probabilities and the one-hot target are multiplied by m = [t != ignore]; 2tp + fp + fn = P_c + G_c"""
    lab = target[:, 0].long()
    prob = torch.softmax(logits, 1)
    if ignore_label is not None:
        m = lab != ignore_label
        lab = torch.where(m, lab, torch.zeros_like(lab))
        mf = m[:, None].to(logits.dtype)
    with torch.no_grad():
        onehot = torch.zeros(prob.shape, device=prob.device, dtype=prob.dtype).scatter_(1, lab[:, None], 1)[:, 1:]
        if ignore_label is not None:
            onehot = onehot * mf
        sum_gt = onehot.sum((2, 3))
    p = prob[:, 1:] if ignore_label is None else prob[:, 1:] * mf
    return _global_dice((p * onehot).sum((2, 3)), p.sum((2, 3)), sum_gt, smooth, ddp, group)


def topk_fused(is_cuda, num_classes, n_voxels):
    """the limits of the fused top-k kernels (csrc/loss_topk.hip): a GPU tensor, 2..8 classes, fewer than 2^31 voxels; beyond them the
    torch formula runs"""
    return bool(is_cuda) and 2 <= num_classes <= 8 and n_voxels < 2 ** 31


def _topk_fused(logits):
    return topk_fused(logits.is_cuda, logits.shape[1], logits.shape[0] * logits.shape[2] * logits.shape[3])


def topk_ce_loss(logits, target, k=10, ignore_label=None):
    """TopKLoss(k, ignore_index) (robust_ce_loss.py:19-32): the mean of the k_vox = int(N k / 100) largest per-voxel cross-entropies,
    N = B H W; an ignored voxel has CE 0 and counts in N.  target (B,1,H,W) integer labels.  ValueError where the reference returns nan
    (k_vox < 1) and for k outside (0, 100].  On the GPU (2..8 classes, N < 2^31) the fused HIP loss (ops.topk_ce_loss, csrc/loss_topk.hip: radix
    select on the device, ties to the lowest flat index); otherwise torch.topk."""
    if _topk_fused(logits):
        from . import ops
        return ops.topk_ce_loss(logits, target, k, ignore_label)
    return _topk_ce_torch(logits, target, k, ignore_label)


def dc_and_topk_loss(logits, target, k=10, smooth=1e-5, ddp=None, group=None, ignore_label=None):
    """DC_and_topk_loss (compound_losses.py:102-150; upstream's "Dice + TopK10"), weight_ce = weight_dice = 1: topk_ce_loss + SoftDiceLoss
    (softmax, batch_dice=True, do_bg=False, smooth; masked by the ignore label).  The reference's host-side `num_fg > 0` test needs no
    decision here: with every voxel ignored every CE is 0 and so is the top-k mean.  Under DDP the top-k is local to the rank (its own N
    and k_vox), only the Dice sums are global.  On the GPU (2..8 classes, N < 2^31) the fused HIP loss (ops.dice_topk_loss); the torch formula
    below is the CPU / many-class path and the fp64 oracle of the tests."""
    if ddp is None:
        ddp = _ddp_default(group)
    if _topk_fused(logits):
        from . import ops
        return ops.dice_topk_loss(logits, target, k, ignore_label, smooth, _loss_group(ddp, group))
    return _topk_ce_torch(logits, target, k, ignore_label) - _soft_dice_torch(logits, target, ignore_label, smooth, ddp, group)


def dc_and_bce_loss(logits, target, use_ignore_label=False, smooth=1e-5, ddp=None, group=None, weight_ce=1.0, weight_dice=1.0,
                    batch_dice=True):
    """DC_and_BCE_loss (compound_losses.py:59-99) with MemoryEfficientSoftDiceLoss(sigmoid, batch_dice=True, do_bg=True, smooth=1e-5)
    (nnUNetTrainer.py:356-361): region-based training.  logits (B,R,H,W); target the reference's one-hot form (B, R + u, H, W) in {0,1},
    u = 1 with `use_ignore_label` (ignore channel last, m = 1 - target[:, -1]).  BCE is the mean over every element without an ignore
    channel, else sum(bce m) / clip(sum m, 1e-8) with the (B,1,H,W) mask broadcast over R -- the denominator counts pixels (:95).
    On the GPU (1..8 regions) the fused HIP loss (ops.dice_bce_loss; a non-uint8 target is converted once); the torch formula below is
    the CPU path.  Soft (non-binary) targets are outside this contract.
    weight_ce, weight_dice and batch_dice are the options of the reference's classes (check_loss_options): at their defaults the code
    below runs as before, otherwise ops.dice_bce_opt_loss (csrc/loss_opt.hip) on the GPU and _dc_and_bce_opt_torch elsewhere."""
    R = logits.shape[1]
    u = 1 if use_ignore_label else 0
    if target.shape[1] != R + u:
        raise ValueError(f"dc_and_bce_loss: target has {target.shape[1]} channels, expected {R + u} ({R} regions"
                         f"{' + the ignore channel' if u else ''})")
    if ddp is None:
        ddp = _ddp_default(group)
    weight_ce, weight_dice, batch_dice, _, _, default = check_loss_options(R, (), None, weight_ce, weight_dice, batch_dice)
    if not default:
        if logits.is_cuda and 1 <= R <= 8:
            from . import ops
            tgt = target if target.dtype == torch.uint8 else target.to(torch.uint8)
            return ops.dice_bce_opt_loss(logits, tgt, u, batch_dice, weight_ce, weight_dice, smooth, _loss_group(ddp, group))
        return _dc_and_bce_opt_torch(logits, target, u, smooth, ddp, group, weight_ce, weight_dice, batch_dice)
    if logits.is_cuda and 1 <= R <= 8:
        from . import ops
        tgt = target if target.dtype == torch.uint8 else target.to(torch.uint8)
        return ops.dice_bce_loss(logits, tgt, u, smooth, _loss_group(ddp, group))
    y = target[:, :R].to(logits.dtype)
    bce = F.binary_cross_entropy_with_logits(logits, y, reduction="none")
    x = torch.sigmoid(logits)
    if u:
        mf = (1 - target[:, -1:]).bool().to(logits.dtype)
        ce = (bce * mf).sum() / torch.clip(mf.sum(), min=1e-8)
        y = y * mf
        x = x * mf
    else:
        ce = bce.mean()
    return ce - _global_dice((x * y).sum((2, 3)), x.sum((2, 3)), y.sum((2, 3)), smooth, ddp, group)


def _region_masks(regions):
    """regions (each an int or a tuple of ints, labels 0..63) -> one int64 bit mask per region (bit l = label l belongs to it)"""
    out = []
    for r in regions:
        labs = (r,) if isinstance(r, int) else tuple(r)
        v = 0
        for l in labs:
            if isinstance(l, bool) or not isinstance(l, int) or not 0 <= int(l) <= 63:
                raise ValueError(f"region label {l!r} outside 0..63")
            v |= 1 << int(l)
        out.append(v - (1 << 64) if v >= 1 << 63 else v)        # label 63 is the sign bit of the int64
    return out


def _region_table(regions, device):
    return torch.tensor(_region_masks(regions), dtype=torch.int64, device=device)


def labels_to_regions(seg, regions, ignore_label=None, table=None):
    """ConvertSegmentationToRegionsTransform (region_based_training.py:7-37; the ignore label appended as the last region,
    nnUNetTrainer.py:764-767): seg (B,1,H,W) integer labels -> uint8 (B, R + u, H, W), plane r = [seg in regions[r]], u = 1 with an
    ignore label, last plane = [seg == ignore_label].  A label outside 0..63 is in no region.  On the GPU the HIP kernel
    (du_labels_to_regions) with the regions as a device table of bit masks (`table`: a prepared one, e.g. build_loss's); on the CPU
    torch.isin."""
    if seg.is_cuda:
        from . import ops
        if table is None:
            table = _region_table(regions, seg.device)
        return ops.labels_to_regions(seg, table, ignore_label)
    s = seg[:, 0]
    planes = []
    for r in regions:
        labs = torch.tensor([r] if isinstance(r, int) else list(r), dtype=s.dtype)
        planes.append(torch.isin(s, labs))
    if ignore_label is not None:
        planes.append(s == ignore_label)
    return torch.stack(planes, 1).to(torch.uint8)


class SegLoss(torch.nn.Module):
    """What nnUNetTrainer._build_loss (nnUNetTrainer.py:355-365) returns for 2D, batch Dice, before the deep-supervision wrapper
    (DeepSupervisionLoss below adds it): DC_and_CE_loss (plain
    labels or with an ignore label) or DC_and_BCE_loss (regions, with or without an ignore label); with `topk_percent` DC_and_topk_loss
    (compound_losses.py:102-150, modes "topk" / "topk_ignore"; not with regions).  Called as loss(logits, target) with
    integer label maps (B,1,H,W) in both modes; in region mode the labels become the one-hot region target on the device inside the same
    step (labels_to_regions with the table built here, at construction, outside any capture).
    weight_ce, weight_dice, batch_dice, do_bg and ce_class_weights are the options of the reference's classes (check_loss_options has
    their meaning and the ValueErrors); `options_default` tells whether all of them are at the trainer's values, and then forward is the
    code path it has always been.  Otherwise the fused option losses of csrc/loss_opt.hip run on the GPU (the class weights live in the
    buffer `class_w`, built here).  The top-k family takes no options."""

    def __init__(self, num_classes, regions=None, ignore_label=None, smooth=1e-5, ddp=None, group=None, topk_percent=None,
                 weight_ce=1.0, weight_dice=1.0, batch_dice=True, do_bg=None, ce_class_weights=None):
        super().__init__()
        (self.weight_ce, self.weight_dice, self.batch_dice, self.do_bg, self.ce_class_weights, self.options_default) = check_loss_options(
            num_classes, regions, topk_percent, weight_ce, weight_dice, batch_dice, do_bg, ce_class_weights)
        if topk_percent is not None:
            if regions is not None:
                raise ValueError("top-k loss with regions: the reference has no such loss (DC_and_topk_loss is softmax-only)")
            check_topk_percent(topk_percent)                     # the range only: k_vox depends on the shape of each call
        self.topk_percent = topk_percent
        if ignore_label is not None:
            if isinstance(ignore_label, bool) or not isinstance(ignore_label, int):
                raise ValueError(f"ignore_label must be an int, got {ignore_label!r}")
            if ignore_label < num_classes:
                raise ValueError(f"ignore_label {ignore_label} must not be a class index (< num_classes = {num_classes})")
        self.num_classes, self.ignore_label, self.smooth, self.ddp, self.group = num_classes, ignore_label, smooth, ddp, group
        self.regions = None if regions is None else [r if isinstance(r, int) else tuple(r) for r in regions]
        if self.regions is not None:
            if not 1 <= len(self.regions) <= 8:
                raise ValueError(f"region-based loss: 1..8 regions supported, got {len(self.regions)}")
            if len(self.regions) != num_classes:
                raise ValueError(f"region-based loss: num_classes (network outputs) {num_classes} != {len(self.regions)} regions")
            masks = _region_masks(self.regions)                  # ValueError for a label outside 0..63
            if ignore_label is not None and 0 <= ignore_label <= 63 and any((m >> ignore_label) & 1 for m in masks):
                raise ValueError(f"ignore_label {ignore_label} lies inside a region")
            dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
            self.register_buffer("table", _region_table(self.regions, dev), persistent=False)
        self.mode = "regions" if self.regions is not None else ("softmax_ignore" if ignore_label is not None else "softmax")
        if topk_percent is not None:
            self.mode = "topk_ignore" if ignore_label is not None else "topk"
        if self.ce_class_weights is not None:
            dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
            self.register_buffer("class_w", _class_w_tensor(self.ce_class_weights, dev), persistent=False)

    def _forward_options(self, logits, target):
        """the loss with non-default options: the functions above with the options of this module"""
        if self.regions is None:
            cw = None
            if self.ce_class_weights is not None:
                cw = self.class_w if logits.is_cuda else self.ce_class_weights     # (the torch formula takes them in the logits' dtype)
                if logits.is_cuda and cw.device != logits.device:
                    raise RuntimeError(f"SegLoss: class weights live on {cw.device}, logits on {logits.device} (move the module with .to())")
            return dc_and_ce_loss(logits, target, self.smooth, ddp=self.ddp, group=self.group, ignore_label=self.ignore_label,
                                  weight_ce=self.weight_ce, weight_dice=self.weight_dice, batch_dice=self.batch_dice, do_bg=self.do_bg,
                                  ce_class_weights=cw)
        table = self.table if self.table.device == target.device else None
        if target.is_cuda and table is None:
            raise RuntimeError(f"SegLoss: region table lives on {self.table.device}, target on {target.device} (move the module with .to())")
        onehot = labels_to_regions(target, self.regions, self.ignore_label, table=table)
        return dc_and_bce_loss(logits, onehot, self.ignore_label is not None, self.smooth, ddp=self.ddp, group=self.group,
                               weight_ce=self.weight_ce, weight_dice=self.weight_dice, batch_dice=self.batch_dice)

    def forward(self, logits, target):
        if not self.options_default:
            return self._forward_options(logits, target)
        if self.topk_percent is not None:
            return dc_and_topk_loss(logits, target, self.topk_percent, self.smooth, ddp=self.ddp, group=self.group,
                                    ignore_label=self.ignore_label)
        if self.regions is None:
            return dc_and_ce_loss(logits, target, self.smooth, ddp=self.ddp, group=self.group, ignore_label=self.ignore_label)
        table = self.table if self.table.device == target.device else None
        if target.is_cuda and table is None:
            raise RuntimeError(f"SegLoss: region table lives on {self.table.device}, target on {target.device} (move the module with .to())")
        onehot = labels_to_regions(target, self.regions, self.ignore_label, table=table)
        return dc_and_bce_loss(logits, onehot, self.ignore_label is not None, self.smooth, ddp=self.ddp, group=self.group)


def deep_supervision_scales(pool_op_kernel_sizes):
    """nnUNetTrainer._get_deep_supervision_scales (nnUNetTrainer.py:300-306): 1 / cumprod of the pooling kernel sizes along the stages,
    the last (lowest) stage dropped -> one list of per-axis scales per deep-supervision output, largest first ([1.0, 1.0] first)."""
    out, cp = [], None
    for k in pool_op_kernel_sizes:
        k = [k] if isinstance(k, (int, float)) else list(k)
        cp = [float(v) for v in k] if cp is None else [a * float(v) for a, v in zip(cp, k)]
        out.append([1.0 / v for v in cp])
    return out[:-1]


def deep_supervision_weights(n_outputs, ddp=False):
    """the weights of nnUNetTrainer._build_loss (nnUNetTrainer.py:373-387): 1 / 2**i per output, the last set to 0 -- or to 1e-6 under
    DDP, the reference's workaround for DDP's unused-parameter check -- then divided by their sum.  Three outputs: [2/3, 1/3, 0]."""
    if isinstance(n_outputs, bool) or not isinstance(n_outputs, int) or n_outputs < 1:
        raise ValueError(f"deep_supervision_weights: n_outputs must be a positive int, got {n_outputs!r}")
    w = [1.0 / (2 ** i) for i in range(n_outputs)]
    w[-1] = 1e-6 if ddp else 0.0
    tot = sum(w)
    if tot == 0.0:
        raise ValueError("deep_supervision_weights: a single output without DDP leaves no non-zero weight")
    return [v / tot for v in w]


def ds_target_index(n_out, n_in, device=None):
    """source index of every output position of resize_segmentation(order=0) along one axis, i.e. what scipy.ndimage.zoom(order=0,
    mode="nearest", grid_mode=True) (= skimage resize(order=0, mode="edge", anti_aliasing=False)) picks:
    floor(clamp((i + 0.5) z - 0.5, 0, n_in - 1) + 0.5) with z = n_in / n_out, evaluated in float64 step by step as scipy's NI_ZoomShift
    does.  In exact arithmetic that is ((2 i + 1) n_in) div (2 n_out) (round half up); the two differ only where z is not a binary
    fraction and the exact coordinate is a tie, which scipy's rounding then decides (148 -> 18 at i = 13: 110, not 111) -- and the
    reference's targets are scipy's.  The identity for n_out == n_in."""
    z = float(n_in) / float(n_out)
    cc = (torch.arange(n_out, dtype=torch.float64, device=device) + 0.5) * z
    cc = (cc - 0.5).clamp(0.0, float(n_in - 1))
    return torch.floor(cc + 0.5).to(torch.int64)


def downsample_target(target, hw):
    """target (B,C,H,W) -> (B,C,h,w) by the index formula of ds_target_index (DownsampleSegForDSTransform2, order 0); torch indexing"""
    H, W = target.shape[-2], target.shape[-1]
    h, w = int(hw[0]), int(hw[1])
    if (h, w) == (H, W):
        return target
    return target[:, :, ds_target_index(h, H, target.device)][:, :, :, ds_target_index(w, W, target.device)]


class DeepSupervisionLoss(torch.nn.Module):
    """DeepSupervisionWrapper (training/loss/deep_supervision.py) around a SegLoss, as nnUNetTrainer._build_loss wraps it
    (nnUNetTrainer.py:373-387): loss(outs, target) = sum_s w_s base(outs[s], target_s) over the scales with w_s != 0, in scale order; a
    zero-weight output is not read and gets no gradient.  outs: the list a deep-supervision decoder returns, largest first.  target: the
    full-resolution label map (B,1,H,W) alone -- the reference's target list is DownsampleSegForDSTransform2 of its first element
    (order 0, the last transform), so target_s is resampled from it here (ds_target_index); a list raises ValueError.
    On the GPU within the class limits of the fused losses: one fused multi-scale pass (ops.ds_seg_loss, four launches whatever the
    number of scales, no target pyramid in memory).  Otherwise (CPU, more classes): the composition of the per-scale losses on indexed
    targets, which is also the fp64 oracle of the GPU tests.  mode, regions, ignore_label, smooth, ddp, group and table are the base's."""

    MAX_FUSED_SCALES = 4

    def __init__(self, base, weights):
        super().__init__()
        if not isinstance(base, SegLoss):
            raise TypeError(f"DeepSupervisionLoss wraps a SegLoss (build_loss), got {type(base).__name__}")
        weights = tuple(float(w) for w in weights)
        if not weights or not any(w != 0.0 for w in weights):
            raise ValueError("DeepSupervisionLoss: at least one weight must be != 0")
        self.base, self.weights = base, weights

    mode = property(lambda self: self.base.mode)
    regions = property(lambda self: self.base.regions)
    ignore_label = property(lambda self: self.base.ignore_label)
    smooth = property(lambda self: self.base.smooth)
    ddp = property(lambda self: self.base.ddp)
    group = property(lambda self: self.base.group)
    num_classes = property(lambda self: self.base.num_classes)
    table = property(lambda self: getattr(self.base, "table", None))

    def _check(self, outs, target):
        if isinstance(target, (list, tuple)):
            raise ValueError("DeepSupervisionLoss: pass the full-resolution target, i.e. the first element of the reference's target "
                             "list; the lower scales are resampled from it")
        if not isinstance(outs, (list, tuple)):
            raise TypeError("DeepSupervisionLoss: the network output must be a list of logits (a decoder with deep_supervision=True)")
        if len(outs) != len(self.weights):
            raise ValueError(f"DeepSupervisionLoss: {len(outs)} outputs, {len(self.weights)} weights")
        if tuple(outs[0].shape[-2:]) != tuple(target.shape[-2:]):
            raise ValueError(f"DeepSupervisionLoss: outs[0] is {tuple(outs[0].shape[-2:])}, the target {tuple(target.shape[-2:])}")

    def fused(self, outs):
        C_ = outs[0].shape[1]
        if self.mode in ("topk", "topk_ignore"):       # composed of the fused per-scale top-k losses: every scale has its own N and k_vox
            return False
        if not self.base.options_default:              # composed of the fused per-scale option losses (csrc/loss_opt.hip)
            return False
        return (all(o.is_cuda for o in outs) and len(outs) <= self.MAX_FUSED_SCALES
                and ((1 <= C_ <= 8) if self.mode == "regions" else (2 <= C_ <= 8)))

    def composed(self, outs, target):
        """the torch formula: the pyramid by integer indexing, the base loss per scale, the weighted sum"""
        self._check(outs, target)
        total = None
        for w, o in zip(self.weights, outs):
            if w == 0.0:
                continue
            l = w * self.base(o, downsample_target(target, o.shape[-2:]))
            total = l if total is None else total + l
        return total

    def forward(self, outs, target, return_scale_losses=False):
        self._check(outs, target)
        if not self.fused(outs):
            if return_scale_losses:
                raise RuntimeError("DeepSupervisionLoss: per-scale losses come from the fused pass only")
            return self.composed(outs, target)
        from . import ops
        ddp = self.ddp if self.ddp is not None else _ddp_default(self.group)
        table = None
        if self.mode == "regions":
            table = self.table
            if table.device != target.device:
                raise RuntimeError(f"DeepSupervisionLoss: region table lives on {table.device}, target on {target.device} "
                                   "(move the module with .to())")
        return ops.ds_seg_loss(outs, target, self.mode, self.weights, table=table, ignore_label=self.ignore_label, smooth=self.smooth,
                               group=_loss_group(ddp, self.group),
                               return_scale_losses=return_scale_losses)


def build_loss(num_classes, regions=None, ignore_label=None, smooth=1e-5, ddp=None, group=None, deep_supervision_weights=None,
               topk_percent=None, weight_ce=1.0, weight_dice=1.0, batch_dice=True, do_bg=None, ce_class_weights=None):
    """nnUNetTrainer._build_loss (nnUNetTrainer.py:355-387) for this package: the loss module for plain labels, labels with an ignore
    label, or regions (each an int or a tuple of ints; num_classes = number of network outputs = len(regions)).  Validated on the host:
    ValueError for an ignore label below num_classes, more than 8 regions, a region label outside 0..63 or an ignore label inside a
    region.  With `deep_supervision_weights` (one per decoder output, e.g. deep_supervision_weights(3)) the module is wrapped in a
    DeepSupervisionLoss, called as loss(outs, target) on the decoder's list.  With `topk_percent` (e.g. 10) the module is
    DC_and_topk_loss instead of DC_and_CE_loss ("Dice + TopK10"; ValueError together with regions); under deep supervision the wrapper
    then composes the fused per-scale losses on indexed targets.  Pass the result to TrainStep(loss=...).
    The options of the reference's loss classes, which its trainer variants set (all validated by check_loss_options, ValueError):
    weight_ce / weight_dice (1.0; 0 removes the term, value and gradient; not both 0), batch_dice (True; False: per-sample Dice, the mean
    over (b, c), no all-reduce under DDP), do_bg (None = the trainer's choice: False for softmax, True for regions; True gives class 0 a
    Dice term; False with regions is refused), ce_class_weights (None; K positive weights: CE = sum w_t nll / sum w_t over the valid
    pixels, exactly 0 when none is valid; softmax only).  At their defaults the module is exactly the one described above; otherwise the
    fused option losses (csrc/loss_opt.hip) run on the GPU for 2..8 classes / 1..8 regions and the wrapper composes the per-scale losses.
    The top-k family stays as it is: any non-default option together with topk_percent is a ValueError."""
    base = SegLoss(num_classes, regions=regions, ignore_label=ignore_label, smooth=smooth, ddp=ddp, group=group, topk_percent=topk_percent,
                   weight_ce=weight_ce, weight_dice=weight_dice, batch_dice=batch_dice, do_bg=do_bg, ce_class_weights=ce_class_weights)
    if deep_supervision_weights is None:
        return base
    return DeepSupervisionLoss(base, deep_supervision_weights)


class _CaptureSegments:
    """A train step recorded as SEVERAL hipGraphs with host-issued work between them (DINOUNET_COMM_OUTSIDE_GRAPH=1, or the fallback
    when the capture of a whole multi-rank step fails): graph | batch-Dice all-reduce | graph | gradient all-reduces | graph.  No RCCL
    call is recorded into a graph; everything else keeps the replay's launch path.  The graphs share one memory pool and are replayed
    in capture order, so a tensor made in one segment is alive in the next.  A cut ends the running capture, which HIP only allows from
    the thread that began it: cuts happen at main-thread points of the step (the loss forward, after backward), never inside autograd's
    device thread.  Consequence: a collective issued by a BACKWARD node (SyncBatchNorm's statistics all-reduce, i.e. the full model at
    N > 1) asks for a cut from that thread, `cut` raises, and TrainStep falls back to eager steps for that configuration."""

    def __init__(self, mode):
        self.mode = mode
        self.graphs, self.between, self.what = [], [], []
        self.pool = torch.cuda.graph_pool_handle()
        self.cur = None
        self.thread = threading.get_ident()

    def begin(self):
        self.cur = torch.cuda.CUDAGraph()
        self.cur.capture_begin(pool=self.pool, capture_error_mode=self.mode)

    def cut(self, eager_fn, what="cut"):
        if threading.get_ident() != self.thread and self.mode != "relaxed":
            # (hipStreamEndCapture from another thread than the one that began the capture is an error in the global / thread-local
            #  modes; "relaxed" lifts that, which is what a collective issued by a backward node -- autograd's device thread -- needs)
            raise RuntimeError(f"segmented capture: '{what}' asks for a cut from a thread that did not begin the capture")
        self.cur.capture_end()
        self.graphs.append(self.cur)
        self.between.append(eager_fn)
        self.what.append(what)
        self.begin()

    def end(self):
        self.cur.capture_end()
        self.graphs.append(self.cur)
        self.between.append(None)
        self.cur = None

    def abort(self):
        if self.cur is not None:
            try:
                self.cur.capture_end()
            except Exception:  # noqa: BLE001
                pass
            self.cur = None

    def replay(self):
        for g, fn in zip(self.graphs, self.between):
            g.replay()
            if fn is not None:
                fn()

    def reset(self):
        for g in self.graphs:
            g.reset()
        self.graphs, self.between, self.what = [], [], []


class TrainStep:
    """One optimiser step of the reference trainer (nnUNetTrainer.py:899-929) on static input buffers:
    zero_grad -> forward -> DC+CE -> backward [-> bucketed RCCL all-reduce] -> clip_grad_norm_(12) -> SGD step.

    With `graph=True` the whole step (a few thousand launches, most of them small) is captured once into a hipGraph
    after `warmup` eager iterations and replayed afterwards, which removes the host launch path from the critical path
    (MI355X guide: "capture launch-bound inner loops in hipGraphs").  Device-side RNG (drop-path masks, RoPE rescale) stays
    live under replay because torch registers the generator's Philox offset with the graph."""

    def __init__(self, net, optimizer, params, x_shape, tgt_shape, device, reducer=None, max_norm=12.0, graph=True, warmup=3,
                 ddp_loss=None, comm_outside_graph=None, loss=None):
        self.net, self.opt, self.params, self.reducer, self.max_norm = net, optimizer, params, reducer, max_norm
        self.ddp_loss = ddp_loss         # None: batch-Dice sums all-reduced iff world size > 1 (dice.py:58-119 with ddp=True)
        self.loss_fn = loss              # None: dc_and_ce_loss on plain labels; else a build_loss module, called as loss(logits, tgt)
        #                                  (a DeepSupervisionLoss for a network that returns the deep-supervision list)
        if comm_outside_graph is None:
            comm_outside_graph = os.environ.get("DINOUNET_COMM_OUTSIDE_GRAPH", "0") == "1"
        self.comm_outside_graph = bool(comm_outside_graph) and reducer is not None
        self.capture_mode = "eager"      # -> "whole_step" | "segments(n)" once a capture exists (bench.py reports it)
        self._segments = None
        self.x = torch.zeros(x_shape, device=device)
        self.tgt = torch.zeros(tgt_shape, dtype=torch.long, device=device)
        self.loss = None
        self.graph = None
        self.use_graph = graph
        self.warmup = warmup
        self._n = 0
        self.comm_events = None          # list -> eager steps record (start, end) events around reducer.finish()
        self._opt_generation = 0

    def _step(self):
        self.opt.zero_grad(set_to_none=True)
        logits = self.net(self.x)
        if isinstance(logits, (list, tuple)):
            # a deep-supervision decoder: the list goes to a DeepSupervisionLoss with the one full-resolution target buffer
            if not isinstance(self.loss_fn, DeepSupervisionLoss):
                raise TypeError("TrainStep: the network returns a list of logits (deep supervision) but the loss is "
                                f"{'the default dc_and_ce_loss' if self.loss_fn is None else type(self.loss_fn).__name__}; pass "
                                "loss=build_loss(..., deep_supervision_weights=deep_supervision_weights(n_outputs))")
            loss = self.loss_fn(logits, self.tgt)
            logits = logits[0]
        elif self.loss_fn is None:
            loss = dc_and_ce_loss(logits, self.tgt, ddp=self.ddp_loss)
        else:
            loss = self.loss_fn(logits, self.tgt)
        loss.backward()
        if logits.is_cuda:
            from . import ops
            ops.WGRAD.flush()          # deferred weight gradients (already flushed by the engine callback; idempotent)
        if self.reducer is not None:
            if self._segments is not None:                  # segmented capture: every bucket's all-reduce from the host, between two graphs
                self.reducer.fill_missing()
                self._segments.cut(self.reducer.reduce_deferred, "gradient_buckets")
            if self.comm_events is not None:               # bench.py: how long the step waits for the gradient all-reduce after backward
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                self.reducer.finish()
                e1.record()
                self.comm_events.append((e0, e1))
            else:
                self.reducer.finish()
        if isinstance(self.opt, FusedClipSGD):              # clip + SGD in three launches (csrc/optim.hip)
            self.opt.max_norm = self.max_norm
            self.opt.step()
        else:
            torch.nn.utils.clip_grad_norm_(self.params, self.max_norm)
            self.opt.step()
        return loss.detach()

    def _forget_failed_pass(self):
        """a capture that raised part-way through backward: re-arm the reducer's bucket counters and drop the weight-gradient products
        the dead pass queued (nobody will read them; the queue would otherwise launch them at the next backward, ops.WgradQueue._arm)"""
        if self.reducer is not None:
            self.reducer.rearm()
        if self.x.is_cuda:
            from . import ops
            ops.WGRAD._drop()
            ops.ZEROS.rec = []           # the dead pass's truncated request record must not become the next step's plan

    def _all_ranks(self, ok):
        """the capture mode is a collective decision: MIN over the ranks of 'my capture worked' (outside any capture)"""
        if self.reducer is None or not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return ok
        t = torch.tensor([1 if ok else 0], dtype=torch.int32, device=self.x.device)
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        return bool(int(t.item()))

    def _capture_in_segments(self, mode):
        import gc
        from . import ops
        seg = _CaptureSegments(mode)
        torch.cuda.synchronize()
        gc.collect()
        torch.cuda.empty_cache()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        self._segments, ops.CAPTURE_CUT, self.reducer.defer = seg, seg.cut, True
        try:
            ops.ks_scratch_prepare(s)          # du_gemm's in-launch scratch of the capture stream: created and zeroed outside any capture
            with torch.cuda.stream(s):
                seg.begin()
                self.loss = self._step()
                seg.end()
        except BaseException:
            seg.abort()
            raise
        finally:
            self._segments, ops.CAPTURE_CUT, self.reducer.defer = None, None, False
        torch.cuda.current_stream().wait_stream(s)
        return seg

    def __call__(self, x=None, tgt=None):
        if x is not None:
            self.x.copy_(x, non_blocking=True)
        if tgt is not None:
            self.tgt.copy_(tgt, non_blocking=True)
        if not self.use_graph:
            self.loss = self._step()
            return self.loss
        if self.graph is None:
            if self._n < self.warmup:                  # eager warm-up on a side stream (allocator + lazy caches settle)
                s = torch.cuda.Stream()
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):
                    self.loss = self._step()
                torch.cuda.current_stream().wait_stream(s)
                self._n += 1
                return self.loss
            torch.cuda.synchronize()
            if dist.is_available() and dist.is_initialized() and dist.get_backend() == "nccl":
                # Quiesce RCCL's watchdog before the capture.  The eager warm-up steps left Work objects in its list; it retires them by
                # polling their events every ~100 ms from its own thread.  A poll that lands while this thread is beginning the capture is
                # the one window in which round 3 saw a watchdog-thread SIGABRT (1 of 18 single-rank runs, never reproduced): after the
                # synchronize above every one of those events is complete, so waiting out a few poll periods empties the list and the
                # watchdog has nothing to query during the capture (collectives issued INSIDE a capture are not handed to it).
                import time
                time.sleep(0.35)
            # With a process group alive, ProcessGroupNCCL's watchdog thread polls its work events (hipEventQuery) while this
            # thread captures; under the default "global" capture mode that call is illegal and the watchdog aborts the process
            # ("operation not permitted when stream is capturing").  thread_local confines the capture restrictions to this thread.
            mode = "thread_local" if (dist.is_available() and dist.is_initialized()) else "global"
            err = None
            if not self.comm_outside_graph:
                try:
                    graph = torch.cuda.CUDAGraph()
                    # (ops.capture: du_gemm's in-launch scratch of the capture stream is created and zeroed BEFORE the capture -- made inside
                    #  it, the zeroing would be a graph node that never runs if this capture is discarded)
                    from . import ops
                    with ops.capture(graph, capture_error_mode=mode):
                        self.loss = self._step()
                    self.graph = graph
                    self.capture_mode = "whole_step"
                except Exception as e:  # noqa: BLE001
                    err = e
                    torch.cuda.synchronize()
                    self._forget_failed_pass()
                if not self._all_ranks(self.graph is not None) and self.graph is not None:
                    # another rank's capture failed: every rank leaves this mode together -- a rank replaying a whole-step graph issues
                    # its bucket all-reduces in hook-ready order, a segmented one in bucket-index order (mixed modes hang
                    # or sum the wrong buckets)
                    self.graph.reset()
                    self.graph = None
                    self.capture_mode = "eager"
                    err = RuntimeError("whole-step capture failed on another rank")
                    self._forget_failed_pass()
            if self.graph is None and self.reducer is not None:
                # the collectives outside the graphs: asked for, or the capture of the whole step (RCCL kernels recorded into it) failed.
                # First with the mode of the whole-step attempt (cuts from the capturing thread only); a step whose BACKWARD issues
                # collectives (SyncBatchNorm at N > 1: autograd's device thread) asks for a cut from that thread, which only a "relaxed"
                # capture may serve -- second attempt
                # (a capture that dies inside autograd's thread cannot be ended cleanly -- the graph's destructor throws and takes the
                #  process down, seen on hardware -- so the doomed thread-local attempt is not made when backward collectives are known to come)
                from . import ops as _ops
                for seg_mode in (("relaxed",) if _ops.sync_active() else (mode, "relaxed")):
                    try:
                        self.graph = self._capture_in_segments(seg_mode)
                        self.capture_mode = f"segments({len(self.graph.graphs)})" + ("" if seg_mode == mode else "/relaxed")
                        err = None
                    except Exception as e:  # noqa: BLE001
                        err = e
                        torch.cuda.synchronize()
                        self._forget_failed_pass()
                    if not self._all_ranks(self.graph is not None) and self.graph is not None:
                        self.graph.reset()
                        self.graph = None
                        self.capture_mode = "eager"
                        err = RuntimeError("segmented capture failed on another rank")
                        self._forget_failed_pass()
                    if self.graph is not None:
                        break
            if self.graph is None:     # capture is an optimisation: a step that cannot be captured still has to train
                import warnings
                warnings.warn(f"hipGraph capture of the train step failed ({err!r}); continuing with eager steps")
                self.use_graph = False
                torch.cuda.synchronize()
                self.loss = self._step()
                return self.loss
            self._opt_generation = getattr(self.opt, "generation", 0)
        if isinstance(self.opt, FusedClipSGD):
            if getattr(self.opt, "generation", 0) != self._opt_generation:
                # optimizer.load_state_dict / reallocated parameters since the capture: the recorded step points at retired tables and
                # momentum buffers -- drop it and capture again
                self.graph.reset()
                self.graph = None
                self._n = max(0, self.warmup - 1)
                return self.__call__()
            self.opt.refresh_hyper()                        # the captured step re-reads lr & co. from the pinned host buffer
        self.graph.replay()
        return self.loss


def _cpu_validation_counts(logits, target, regions=None, ignore_label=None):
    """nnUNetTrainer.validation_step, nnUNetTrainer.py:971-994 with get_tp_fp_fn_tn (dice.py:122-167), restated in integer torch ops:
    (3, C) int64 = [tp | fp | fn] over axes (0, 2, 3).  The oracle of the HIP counts (tests) and the CPU path."""
    if regions is not None:
        onehot = labels_to_regions(target, regions, ignore_label)
        R = len(regions)
        pred = torch.sigmoid(logits.float()) > 0.5                                          # :973-974
        y = onehot[:, :R].bool()
        m = (onehot[:, R:] == 0) if ignore_label is not None else torch.ones_like(y[:, :1])  # :987-990
    else:
        lab = target[:, :1].long()
        pred = torch.zeros(logits.shape, dtype=torch.bool, device=logits.device).scatter_(1, logits.argmax(1)[:, None], True)   # :976-979
        if ignore_label is not None:
            m = lab != ignore_label                                                         # :984
            lab = torch.where(m, lab, torch.zeros_like(lab))                                # :986
        else:
            m = torch.ones_like(lab, dtype=torch.bool)
        y = torch.zeros(logits.shape, dtype=torch.bool, device=logits.device).scatter_(1, lab, True)
    tp = (pred & y & m).sum((0, 2, 3))
    fp = (pred & ~y & m).sum((0, 2, 3))
    fn = (~pred & y & m).sum((0, 2, 3))
    return torch.stack([tp, fp, fn]).to(torch.int64)


def _val_loss_counts(logits, target, mode, regions, ignore_label, table, smooth, ddp, group, counts=None, accum=None):
    """validation loss (the training loss's forward value) and this step's (3, C) counts; `accum` += counts.  GPU: one fused pass
    (ops.val_dice_ce / ops.val_dice_bce); CPU, or more classes than the kernels serve: the torch formulas."""
    C_ = logits.shape[1]
    fused = logits.is_cuda and ((1 <= C_ <= 8) if mode == "regions" else (2 <= C_ <= 8))
    if ddp is None:
        ddp = _ddp_default(group)
    if fused:
        from . import ops
        g = _loss_group(ddp, group)
        if mode == "regions":
            onehot = labels_to_regions(target, regions, ignore_label, table=table)
            return ops.val_dice_bce(logits, onehot, ignore_label is not None, smooth, g, counts, accum)
        return ops.val_dice_ce(logits, target, ignore_label, smooth, g, counts, accum)
    with torch.no_grad():
        if mode == "regions":
            onehot = labels_to_regions(target, regions, ignore_label, table=table)
            loss = dc_and_bce_loss(logits, onehot, ignore_label is not None, smooth, ddp=ddp, group=group)
        else:
            loss = dc_and_ce_loss(logits, target, smooth, ddp=ddp, group=group, ignore_label=ignore_label)
        c = _cpu_validation_counts(logits, target, regions, ignore_label)
        if counts is None:
            counts = c
        else:
            counts.copy_(c)
        if accum is not None:
            accum += c
    return loss.detach(), counts


def validation_counts(logits, target, regions=None, ignore_label=None):
    """tp, fp, fn of nnUNetTrainer.validation_step (nnUNetTrainer.py:971-994): int64 tensors of length K (softmax modes: the argmax
    prediction, lowest index among equal maxima; every class, the background included) or R (regions: sigmoid(x) > 0.5).  target (B,1,H,W)
    integer labels in every mode (regions: converted by labels_to_regions, as SegLoss does); a pixel with `ignore_label` adds to no count.
    On the GPU the HIP validation pass (csrc/loss.hip, which predicts a region where x > 0: the same predicate outside 0 < x < ~1.2e-7,
    where torch's fp32 sigmoid rounds to exactly 0.5); on the CPU the plain torch restatement."""
    C_ = logits.shape[1]
    if logits.is_cuda:
        if regions is not None and len(regions) != C_:
            raise ValueError(f"validation_counts: {C_} logits planes, {len(regions)} regions")
        mode = "regions" if regions is not None else ("softmax_ignore" if ignore_label is not None else "softmax")
        _, c = _val_loss_counts(logits, target, mode, regions, ignore_label, None, 1e-5, False, None)
    else:
        c = _cpu_validation_counts(logits, target, regions, ignore_label)
    return c[0], c[1], c[2]


class ValStep:
    """One validation step of the reference trainer (nnUNetTrainer.validation_step, nnUNetTrainer.py:946-1008) on static input buffers,
    the eval-mode sibling of TrainStep:  net.eval() -> no_grad forward -> fused loss + tp / fp / fn (csrc/loss.hip, one pass over the
    logits); net.train(...) is restored on exit.  Nothing is read back per step: every step adds its counts to `counts` ((3, C) int64 =
    [tp | fp | fn], all classes), its loss to `loss_sum` (float64) -- both on the device -- and 1 to `steps`.  last() returns the
    reference's per-step dict, epoch_end() what on_validation_epoch_end (:1010-1052) logs.

    With `graph=True` the step is captured once into a hipGraph after `warmup` eager steps and replayed.  The graph reads the parameters
    and running statistics in place, so it stays valid while a TrainStep on the same `net` updates them (not if they are re-allocated:
    build a new ValStep then; inference.clear_window_cache states the same rule).  `loss`: a build_loss module or None (plain labels);
    mode, regions, ignore label, smooth, ddp and group come from it, the region table was built with it, outside any capture.  With a
    DeepSupervisionLoss and a network that returns a list, the step loss is the module's multi-scale forward value (validation_step :963)
    while the counts come from outs[0] and the full-resolution target (:966-968); with any other loss a list is reduced to outs[0].  With a
    top-k loss (build_loss(..., topk_percent=...)) the counts come from the same softmax / softmax-ignore counts pass and the step loss is
    the top-k module's forward value; a loss with non-default options (weight_ce, batch_dice, ...) is arranged the same way.  With a
    group the Dice sums are all-reduced as in the training forward (the reference's validation loss is the same module); under a
    capture that all-reduce is recorded into the graph, a capture that fails falls back to eager steps with a warning, and the multi-rank
    capture itself has been run on CPU / gloo eager steps only, not on several GPUs."""

    def __init__(self, net, x_shape, tgt_shape, device, loss=None, graph=True, warmup=2):
        self.net = net
        device = torch.device(device)
        self.mode = "softmax" if loss is None else loss.mode
        self.regions = None if loss is None else loss.regions
        self.ignore_label = None if loss is None else loss.ignore_label
        self.smooth = 1e-5 if loss is None else loss.smooth
        self.ddp = None if loss is None else loss.ddp
        self.group = None if loss is None else loss.group
        self.ds_loss = loss if isinstance(loss, DeepSupervisionLoss) else None      # step loss = its multi-scale forward value
        # a top-k loss: the counts come from the softmax / softmax-ignore counts pass, the step loss is the module's forward value
        self.topk_loss = None
        if self.mode in ("topk", "topk_ignore"):
            self.topk_loss = loss.base if isinstance(loss, DeepSupervisionLoss) else loss
        # a loss with non-default options: the same arrangement (counts from the default counts pass, step loss = the module's value)
        self.opt_loss = None
        base = loss.base if isinstance(loss, DeepSupervisionLoss) else loss
        if base is not None and not getattr(base, "options_default", True):
            self.opt_loss = base
        self.table = None
        if self.regions is not None and device.type == "cuda":
            self.table = loss.table if loss.table.device == device else _region_table(self.regions, device)
        self.x = torch.zeros(x_shape, device=device)
        self.tgt = torch.zeros(tgt_shape, dtype=torch.long, device=device)
        self.counts = None               # (3, C) int64, allocated at the first step (C = the network's output planes)
        self.loss_sum = torch.zeros((), dtype=torch.float64, device=device)
        self.steps = 0
        self.loss = None                 # this step's loss (device scalar) and counts
        self.step_counts = None
        self.graph = None
        self.use_graph = bool(graph) and device.type == "cuda"
        self.warmup = max(1, warmup)     # the first step allocates the accumulators: never inside the capture
        self._n = 0

    def _step(self):
        was_training = self.net.training
        self.net.eval()
        try:
            with torch.no_grad():
                logits = self.net(self.x)
                ds_loss = None
                if isinstance(logits, (list, tuple)):
                    if self.ds_loss is not None:     # validation_step :963: the loss module on the whole list; counts from outs[0] (:966-968)
                        ds_loss = self.ds_loss(logits, self.tgt).detach()
                    logits = logits[0]
                if self.counts is None:
                    C_ = logits.shape[1]
                    self.counts = torch.zeros((3, C_), dtype=torch.int64, device=self.x.device)
                    self.step_counts = torch.zeros((3, C_), dtype=torch.int64, device=self.x.device)
                loss, _ = _val_loss_counts(logits, self.tgt, self.mode, self.regions, self.ignore_label, self.table, self.smooth,
                                           self.ddp, self.group, counts=self.step_counts, accum=self.counts)
                if ds_loss is not None:
                    loss = ds_loss
                elif self.topk_loss is not None:
                    loss = self.topk_loss(logits, self.tgt).detach()
                elif self.opt_loss is not None:
                    loss = self.opt_loss(logits, self.tgt).detach()
                self.loss_sum += loss.double()
        finally:
            self.net.train(was_training)
        return loss

    def __call__(self, x=None, tgt=None):
        if x is not None:
            self.x.copy_(x, non_blocking=True)
        if tgt is not None:
            self.tgt.copy_(tgt, non_blocking=True)
        self.loss = self._run()
        self.steps += 1                                # counted once the step has been issued
        return self.loss

    def _run(self):
        if not self.use_graph:
            return self._step()
        if self.graph is None:
            if self._n < self.warmup:                  # eager warm-up on a side stream (allocator + lazy caches settle); real steps
                s = torch.cuda.Stream()
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):
                    loss = self._step()
                torch.cuda.current_stream().wait_stream(s)
                self._n += 1
                return loss
            torch.cuda.synchronize()
            from . import ops
            pg = dist.is_available() and dist.is_initialized()
            if pg and dist.get_backend() == "nccl":
                import time
                time.sleep(0.35)                       # RCCL's watchdog retires the warm-up steps' work before the capture (see TrainStep)
            # (thread_local: with a process group alive its watchdog thread polls events while this thread captures, see TrainStep)
            mode = "thread_local" if pg else "global"
            graph = torch.cuda.CUDAGraph()
            try:
                # a capture records, it does not run: a failure leaves the accumulators untouched
                with ops.capture(graph, capture_error_mode=mode):     # ks_scratch_prepare on the capture stream first
                    self.loss = self._step()
                self.graph = graph
            except Exception as e:  # noqa: BLE001
                # capture is an optimisation: a step that cannot be captured still has to validate.  With a Dice group the all-reduce
                # is recorded into the graph (no segmented capture here); that multi-rank capture has not been exercised on hardware
                import warnings
                warnings.warn(f"hipGraph capture of the validation step failed ({e!r}); continuing with eager steps")
                torch.cuda.synchronize()
                self.use_graph = False
                return self._step()
        self.graph.replay()
        return self.loss

    def _drop_bg(self, a):
        return a if self.mode == "regions" else a[1:]

    def last(self):
        """the reference's validation_step return value for the latest step (:996-1008; syncs): loss and tp_hard / fp_hard / fn_hard as
        numpy arrays, the background class dropped in the softmax modes"""
        c = self.step_counts.cpu().numpy()
        return {"loss": self.loss.detach().cpu().numpy(), "tp_hard": self._drop_bg(c[0]), "fp_hard": self._drop_bg(c[1]),
                "fn_hard": self._drop_bg(c[2])}

    def reset(self):
        if self.counts is not None:
            self.counts.zero_()
        self.loss_sum.zero_()
        self.steps = 0

    def absorb(self, other):
        """continue the epoch another ValStep began (another batch shape, e.g. a ragged last batch): its accumulators are added to
        this one's and zeroed.  Same device, same number of classes."""
        if other.counts is not None:
            if self.counts is None:
                self.counts = torch.zeros_like(other.counts)
                self.step_counts = torch.zeros_like(other.counts)
            self.counts += other.counts
        self.loss_sum += other.loss_sum
        self.steps += other.steps
        other.reset()

    def epoch_end(self, group=None):
        """on_validation_epoch_end (:1010-1052; syncs): with a group the counts, the loss sum and the step count are all-reduced (SUM).
        Dice = 2 tp / (2 tp + fp + fn) in float64 per foreground class / region, nan where tp = fp = fn = 0; mean_fg_dice = nanmean.
        Zeroes the accumulators."""
        import numpy as np
        if self.counts is None:
            raise RuntimeError("ValStep.epoch_end: no step has run")
        counts, tail = self.counts.clone(), torch.stack([self.loss_sum, torch.tensor(float(self.steps), dtype=torch.float64,
                                                                                    device=self.loss_sum.device)])
        if group is not None and dist.is_available() and dist.is_initialized():
            dist.all_reduce(counts, group=group)
            dist.all_reduce(tail, group=group)
        c = counts.cpu().numpy()
        tail = tail.cpu().numpy()
        steps = int(round(float(tail[1])))
        tp, fp, fn = (self._drop_bg(c[i]) for i in range(3))
        with np.errstate(divide="ignore", invalid="ignore"):
            dice = 2.0 * tp.astype(np.float64) / (2.0 * tp + fp + fn).astype(np.float64)
            mean_fg = float(np.nanmean(dice)) if np.isfinite(dice).any() else float("nan")
        self.reset()
        return {"val_loss": float(tail[0]) / steps if steps else float("nan"), "dice_per_class_or_region": [float(d) for d in dice],
                "mean_fg_dice": mean_fg, "tp": tp, "fp": fp, "fn": fn, "steps": steps}
