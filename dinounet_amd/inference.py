"""Sliding-window inference with Gaussian blending on the MI355X -- SURVEY.md 8(f) rank 2: the consumer of the forward path that
produces the segmentation the Dice metric is computed on.  Mirrors the reference predictor
(dinounet/inference/predict_from_raw_data.py:503-535 slicers, :571-621 accumulation, :680-727 padding / un-padding;
dinounet/inference/sliding_window_prediction.py:10-60 Gaussian map and step positions) for the 2D networks of this repo:

    data (C, D, H, W): every slice d is tiled with `patch_size` windows at `tile_step_size`; each window's logits are weighted with
    a Gaussian importance map (sigma = patch / 8, peak value 10, zeros replaced by the smallest non-zero value), accumulated, and the
    sum is divided by the accumulated weights.

Differences from the reference, all on purpose: windows are run through the network in batches (the reference predicts one window
per forward); the accumulators are fp32 (the reference keeps fp16 buffers and aborts on overflow, :612-615); the weighted
accumulate and the final division are two HIP kernels (csrc/elementwise.hip: du_window_accumulate, du_window_normalize) instead of
two indexed read-modify-write torch ops per window.  Test-time mirroring (predict_from_raw_data.py:537-552: the prediction is
averaged with the un-flipped predictions of every non-empty combination of the allowed mirror axes) is available through
mirror_axes=...; the in-trainer validation passes use_mirroring=False (nnUNetTrainer.py:1160), the stand-alone predictor defaults to
the checkpoint's inference_allowed_mirroring_axes.  There is no CPU path: the module needs the GPU.
What follows the logits in the reference (resampling, argmax / region paint, bbox paste, per-case metrics; export_prediction.py:15-68,
evaluate_predictions.py:152-234) is export.py: predict_segmentation runs the window loop below and goes from the accumulators straight
to the label map.
`acvl_utils.pad_nd_image` (not vendored in the reference tree) is restated from its published behaviour: centred constant padding
up to the patch size, extra pixel on the high side."""
import itertools
import math

import numpy as np
import torch

from . import _lib


def compute_gaussian(tile_size, sigma_scale=1.0 / 8, value_scaling_factor=1.0, dtype=torch.float32, device="cpu"):
    """sliding_window_prediction.py:10-31 (scipy's gaussian_filter of a centred delta, normalised to `value_scaling_factor`)."""
    from scipy.ndimage import gaussian_filter
    tmp = np.zeros(tile_size)
    tmp[tuple(i // 2 for i in tile_size)] = 1
    g = gaussian_filter(tmp, [i * sigma_scale for i in tile_size], 0, mode="constant", cval=0)
    g = torch.from_numpy(g)
    g = g / torch.max(g) * value_scaling_factor
    g = g.type(dtype).to(device)
    g[g == 0] = torch.min(g[g != 0])       # the importance map must not be 0 (division by the accumulated weights)
    return g


def compute_steps_for_sliding_window(image_size, tile_size, tile_step_size):
    """sliding_window_prediction.py:34-60: window origins per axis, evenly spread, at most tile*step apart."""
    assert all(i >= j for i, j in zip(image_size, tile_size)), "image size must be as large or larger than patch_size"
    assert 0 < tile_step_size <= 1, "step_size must be larger than 0 and smaller or equal to 1"
    target = [i * tile_step_size for i in tile_size]
    num_steps = [int(np.ceil((i - k) / j)) + 1 for i, j, k in zip(image_size, target, tile_size)]
    steps = []
    for dim in range(len(tile_size)):
        max_step = image_size[dim] - tile_size[dim]
        actual = max_step / (num_steps[dim] - 1) if num_steps[dim] > 1 else 99999999999
        steps.append([int(np.round(actual * i)) for i in range(num_steps[dim])])
    return steps


def sliding_window_origins(image_size, patch_size, tile_step_size):
    """(d, y0, x0) of every window of a (D, H, W) volume predicted slice-wise with a 2D patch -- predict_from_raw_data.py:505-522
    (same order: slices outermost, then x steps, then y steps)."""
    assert len(image_size) == 3 and len(patch_size) == 2
    steps = compute_steps_for_sliding_window(image_size[1:], patch_size, tile_step_size)
    return [(d, sy, sx) for d in range(image_size[0]) for sy in steps[0] for sx in steps[1]]


def pad_to_patch(data, patch_size):
    """pad_nd_image(data, patch_size, 'constant', {'value': 0}, return_slicer=True) for the trailing 2 axes: centred, the odd pixel
    goes to the high side.  Returns (padded, (y slice, x slice)) where the slices undo the padding."""
    H, W = data.shape[-2:]
    nh, nw = max(H, patch_size[0]), max(W, patch_size[1])
    dy, dx = nh - H, nw - W
    if dy == 0 and dx == 0:
        return data, (slice(0, H), slice(0, W))
    lo_y, lo_x = dy // 2, dx // 2
    padded = torch.nn.functional.pad(data, (lo_x, dx - lo_x, lo_y, dy - lo_y), mode="constant", value=0)
    return padded, (slice(lo_y, lo_y + H), slice(lo_x, lo_x + W))


class _WindowForward:
    """Eval-mode forward of a fixed (batch, C, ph, pw) window batch captured into a hipGraph (the forward is a few hundred small
    launches; eager it is host-bound).  A ragged last batch is padded with zero windows whose logits are never accumulated."""

    def __init__(self, net, shape, device):
        self.x = torch.zeros(shape, dtype=torch.float32, device=device)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):                      # allocator / lazy caches settle before the capture
                net(self.x)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        from . import ops
        with ops.capture(self.graph):               # (the capture stream's du_gemm scratch exists before the capture: the ViT's K-sliced units run in the graph)
            y = net(self.x)
            self.y = (y[0] if isinstance(y, (list, tuple)) else y).float().contiguous()

    def __call__(self, x):
        n = x.shape[0]
        self.x[:n].copy_(x)
        if n < self.x.shape[0]:
            self.x[n:].zero_()
        self.graph.replay()
        return self.y


def clear_window_cache(net):
    """Drop the captured window forwards of `net` (after load_state_dict with re-allocated tensors, .to(), dtype changes)."""
    net.__dict__.pop("_sw_forward_cache", None)


def mirror_axes_combinations(mirror_axes, ndim):
    """predict_from_raw_data.py:541-548: tensor dims to flip for every non-empty subset of the allowed mirror axes (axis m of the
    spatial dims = tensor dim m + 2 of the (b, c, *spatial) window batch)."""
    if mirror_axes is None or len(mirror_axes) == 0:
        return []
    assert max(mirror_axes) <= ndim - 3, "mirror_axes does not match the dimension of the input!"
    return [c for i in range(len(mirror_axes)) for c in itertools.combinations([m + 2 for m in mirror_axes], i + 1)]


def _mirror_and_predict(forward, x, combos):
    """predict_from_raw_data.py:537-552 around `forward` (which may hand back a buffer it reuses on the next call)."""
    if not combos:
        return forward(x)
    pred = forward(x).clone()
    for axes in combos:
        pred += torch.flip(forward(torch.flip(x, axes)), axes)
    pred /= (len(combos) + 1)
    return pred


@torch.no_grad()
def _accumulate_windows(net, data, patch_size, tile_step_size, use_gaussian, batch_size, graph, mirror_axes):
    """The window loop shared by predict_sliding_window_logits and export.predict_segmentation: data (C, D, H, W) -> the accumulators
    predicted_logits (K, D, Hp, Wp) and n_predictions (D, Hp, Wp) of the padded volume (predict_from_raw_data.py:607-608, not yet
    divided) and the (y, x) slices that undo the padding."""
    assert data.ndim == 4, "input_image must be a 4D tensor (c, d, y, x)"
    dev = next(net.parameters()).device
    if dev.type != "cuda":
        raise RuntimeError("sliding-window inference runs on the MI355X (no CPU fallback)")
    was_training = net.training
    net.eval()
    try:
        def eager_forward(xb):
            out = net(xb)
            if isinstance(out, (list, tuple)):
                out = out[0]
            return out.float().contiguous()

        def graph_forward(xb):
            # cached on the module: replays read the parameters / running statistics in place, so the capture stays valid
            # while they are updated (not if they are re-allocated: clear_window_cache(net) then)
            cache = net.__dict__.setdefault("_sw_forward_cache", {})
            key = (batch_size, xb.shape[1], xb.shape[2], xb.shape[3], str(dev))
            if key not in cache:
                cache[key] = _WindowForward(net, (batch_size, *xb.shape[1:]), dev)
            return cache[key](xb)

        return _window_loop(graph_forward if graph else eager_forward, dev, data, patch_size, tile_step_size, use_gaussian, batch_size,
                            mirror_axes)
    finally:
        net.train(was_training)


def _window_loop(forward, dev, data, patch_size, tile_step_size, use_gaussian, batch_size, mirror_axes):
    """The loop itself.  forward(x (b, C, ph, pw)) -> contiguous fp32 logits of at least b windows (a captured forward hands back its whole
    batch, in a buffer it reuses).  One du_window_accumulate per window batch."""
    data = data.to(dev, torch.float32)
    data, (ys, xs) = pad_to_patch(data, patch_size)
    Cc, D, H, W = data.shape
    ph, pw = int(patch_size[0]), int(patch_size[1])
    origins = sliding_window_origins((D, H, W), (ph, pw), tile_step_size)
    gauss = (compute_gaussian((ph, pw), sigma_scale=1.0 / 8, value_scaling_factor=10, dtype=torch.float32, device=dev)
             if use_gaussian else torch.ones((ph, pw), dtype=torch.float32, device=dev)).contiguous()
    pred = npred = None
    coords_all = torch.tensor(origins, dtype=torch.int32).to(dev)        # one host->device copy for the whole volume
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    combos = mirror_axes_combinations(mirror_axes, 4)
    for i0 in range(0, len(origins), batch_size):
        chunk = origins[i0:i0 + batch_size]
        x = torch.stack([data[:, d, y0:y0 + ph, x0:x0 + pw] for d, y0, x0 in chunk])           # (b, C, ph, pw)
        logits = _mirror_and_predict(forward, x, combos)
        if combos and logits.shape[0] > len(chunk):
            logits = logits[:len(chunk)].contiguous()
        K = logits.shape[1]
        if pred is None:
            pred = torch.zeros((K, D, H, W), dtype=torch.float32, device=dev)
            npred = torch.zeros((D, H, W), dtype=torch.float32, device=dev)
        coords = coords_all[i0:i0 + len(chunk)]
        _lib.check(L.du_window_accumulate(logits.data_ptr(), gauss.data_ptr(), coords.data_ptr(), pred.data_ptr(), npred.data_ptr(),
                                          len(chunk), K, ph, pw, D, H, W, st), "du_window_accumulate")
    return pred, npred, (ys, xs)


@torch.no_grad()
def predict_sliding_window_logits(net, data, patch_size, tile_step_size=0.5, use_gaussian=True, batch_size=8, graph=False,
                                  mirror_axes=None):
    """data (C, D, H, W) on the GPU (or host: moved once) -> fp32 logits (K, D, H, W) on the GPU.
    predict_from_raw_data.py:680-727 with _internal_predict_sliding_window_return_logits :571-621.  graph=True replays a captured
    forward of a full window batch (worth it from a few batches per volume on).  mirror_axes: allowed_mirroring_axes of the
    predictor (for this 2D path a subset of (0, 1) = the window's rows / columns), None = no test-time mirroring."""
    pred, npred, (ys, xs) = _accumulate_windows(net, data, patch_size, tile_step_size, use_gaussian, batch_size, graph, mirror_axes)
    K = pred.shape[0]
    _lib.check(_lib.lib().du_window_normalize(pred.data_ptr(), npred.data_ptr(), K, npred.numel(), torch.cuda.current_stream().cuda_stream),
               "du_window_normalize")
    if not math.isfinite(float(pred.abs().max())):
        raise RuntimeError("Encountered inf in predicted array")                                 # :612-615
    return pred[:, :, ys, xs]


def _training_flags(module):
    return [(m, m.training) for m in module.modules()]


def _set_training_flags(flags):
    for m, training in flags:
        m.training = training


class EnsemblePredictor:
    """Fold ensemble of one network: the predictor's loop over list_of_parameters (predict_from_raw_data.py:477-496: every window is
    predicted with every parameter set and the logits are averaged), with the frozen backbone run ONCE per window batch.

    Every fold of a Dino U-Net carries the same frozen DINOv3 backbone (checkpoint.py stores its fingerprint instead of its tensors), and the
    backbone's layers do not depend on the adapter (DINOv3_Adapter._forward launches it beside the prior module).  So per window batch and
    mirror combination: one backbone pass, the F heads (prior module, interactions, FAPM, decoder) on its layers, the logits summed over the
    folds, one du_window_accumulate.  The reference re-runs the whole network F times.

    list_of_parameters: full state dicts of `net`, or compact dicts of checkpoint.compact_state_dict (no frozen backbone entries, no
    decoder.encoder.* aliases).  Everything except the backbone is replicated F times and each set is loaded strictly into its replica
    (BatchNorm statistics are per fold); the backbone module is shared by object identity with `net`.  A full dict whose frozen backbone
    tensors differ from net's raises ValueError: a shared backbone would be wrong, and so does a backbone with a trainable parameter (it
    would belong to the folds, not to the backbone they share).  `net` itself is not modified, the training flags of the shared backbone
    included: the backbone's output depends on them (RoPE rescaling and stochastic depth in train mode), so every prediction puts it into
    eval mode for its window loop -- warm-up and capture of graph=True inside it -- and restores the flags afterwards, whatever net.train()
    / net.eval() did in between.  The captured forwards of graph=True are cached on the predictor (clear_cache() after the replicas'
    tensors were re-allocated)."""

    def __init__(self, net, list_of_parameters):
        import copy
        from . import checkpoint
        sets = list(list_of_parameters)
        if len(sets) == 0:
            raise ValueError("list_of_parameters is empty")
        self.device = next(net.parameters()).device
        if self.device.type != "cuda":
            raise RuntimeError("sliding-window inference runs on the MI355X (no CPU fallback)")
        backbone = net.encoder.dinov3_adapter.backbone
        trainable = [n for n, p in backbone.named_parameters() if p.requires_grad]
        if trainable:
            raise ValueError(f"the backbone has trainable parameters ({trainable[:3]} ...): folds cannot share it")
        full = net.state_dict()
        frozen = set(checkpoint._frozen_keys(net))
        aliases = {k for k in full if k.startswith(checkpoint.ALIAS_PREFIX)}
        compact_keys = set(full) - frozen - aliases
        self.nets = []
        modes = _training_flags(backbone)                    # rep.eval() below reaches the shared backbone
        for i, params in enumerate(sets):
            keys = set(params.keys())
            if keys != set(full) and keys != compact_keys:
                missing, unexpected = sorted((compact_keys if not (keys & frozen) else set(full)) - keys), sorted(keys - set(full))
                raise RuntimeError(f"parameter set {i} does not fit the network (strict): missing {missing[:4]}, unexpected {unexpected[:4]}")
            for k in sorted(keys & frozen):
                if not torch.equal(params[k].to(full[k].device, full[k].dtype), full[k]):
                    raise ValueError(f"parameter set {i}: frozen backbone tensor {k} differs from the network's; folds can share the "
                                     f"backbone only if it is the same")
            # a copy of everything but the backbone (and but the captured forwards cached on net, which belong to net's own tensors)
            memo = {id(backbone): backbone}
            if "_sw_forward_cache" in net.__dict__:
                memo[id(net.__dict__["_sw_forward_cache"])] = {}
            rep = copy.deepcopy(net, memo)
            assert rep.encoder.dinov3_adapter.backbone is backbone
            # the key sets were compared above, which is what strict means; the frozen entries are left out so that the shared backbone is
            # not written (for a compact dict the aliases are absent too: their tensors are loaded under their own names)
            rep.load_state_dict({k: v for k, v in params.items() if k not in frozen}, strict=False)
            self.nets.append(rep.eval())
        _set_training_flags(modes)
        self.backbone = backbone
        self._forward_cache = {}

    def clear_cache(self):
        self._forward_cache.clear()

    def _eager_forward(self, xb):
        """sum over the folds of the logits of one window batch: one backbone pass, F heads.  The heads are called below DinoUNet.forward:
        its per-step weight packing covers the process-wide table -- net's and every replica's weights -- so once per window batch is enough"""
        from . import ops
        xb = xb.float()
        ops.PACK.refresh()
        ops.ZEROS.new_step()
        layers = self.nets[0].encoder.backbone_layers(xb)
        total = None
        for rep in self.nets:
            out = rep.decoder(rep.encoder(xb, layers))
            if isinstance(out, (list, tuple)):
                out = out[0]
            out = out.float()
            total = out if total is None else total.add_(out)             # fold 0's logits are a fresh tensor nobody else holds
        return total.contiguous()

    def _forward(self, batch_size, graph):
        if not graph:
            return self._eager_forward

        def graph_forward(xb):
            key = (batch_size, xb.shape[1], xb.shape[2], xb.shape[3])
            if key not in self._forward_cache:                             # backbone + F heads: one graph per (batch, C, patch)
                self._forward_cache[key] = _WindowForward(self._eager_forward, (batch_size, *xb.shape[1:]), self.device)
            return self._forward_cache[key](xb)
        return graph_forward

    @torch.no_grad()
    def _accumulate(self, data, patch_size, tile_step_size, use_gaussian, batch_size, graph, mirror_axes):
        """_accumulate_windows of the ensemble: the accumulators hold the SUM over the folds; n_predictions is scaled by F so that
        sums / n_predictions is the mean logit (one (D, H, W) plane, instead of a pass over the K planes)"""
        assert data.ndim == 4, "input_image must be a 4D tensor (c, d, y, x)"
        modes = _training_flags(self.backbone)
        self.backbone.eval()
        try:
            pred, npred, slices = _window_loop(self._forward(batch_size, graph), self.device, data, patch_size, tile_step_size,
                                               use_gaussian, batch_size, mirror_axes)
        finally:
            _set_training_flags(modes)
        if len(self.nets) > 1:
            npred.mul_(float(len(self.nets)))
        return pred, npred, slices

    @torch.no_grad()
    def predict_logits(self, data, patch_size, tile_step_size=0.5, use_gaussian=True, batch_size=8, graph=False, mirror_axes=None):
        """predict_sliding_window_logits of the ensemble: the mean over the folds of the logits (K, D, H, W), fp32 on the GPU"""
        pred, npred, (ys, xs) = self._accumulate(data, patch_size, tile_step_size, use_gaussian, batch_size, graph, mirror_axes)
        _lib.check(_lib.lib().du_window_normalize(pred.data_ptr(), npred.data_ptr(), pred.shape[0], npred.numel(),
                                                  torch.cuda.current_stream().cuda_stream), "du_window_normalize")
        if not math.isfinite(float(pred.abs().max())):
            raise RuntimeError("Encountered inf in predicted array")                             # :612-615
        return pred[:, :, ys, xs]

    @torch.no_grad()
    def predict_segmentation(self, data, patch_size, tile_step_size=0.5, use_gaussian=True, batch_size=8, graph=False, mirror_axes=None, *,
                             regions_class_order=None, properties=None, transpose_backward=None, return_probabilities=False):
        """export.predict_segmentation of the ensemble: the window loop, then ONE pass from the accumulators to the label map.  The positive
        factor 1 / F cannot change a label, so without resampling the sums over folds and windows decide."""
        from . import export
        pred, npred, (ys, xs) = self._accumulate(data, patch_size, tile_step_size, use_gaussian, batch_size, graph, mirror_axes)
        window = (ys.start, xs.start, ys.stop - ys.start, xs.stop - xs.start)
        return export._export(pred, npred, window, regions_class_order, properties, transpose_backward, return_probabilities)

    def predict_from_raw(self, data, properties, patch_size, **kwargs):
        """preprocessing.predict_from_raw with this ensemble in place of one network: raw array in, ensemble label map out"""
        from .preprocessing import predict_from_raw
        return predict_from_raw(self, data, properties, patch_size, **kwargs)


# the export tail (label maps, probabilities, per-case metrics) lives in export.py; its names are part of this module's interface
from .export import case_metrics, logits_to_segmentation, predict_segmentation  # noqa: E402,F401
# ... and what precedes the window loop (crop, normalise, resample a raw case) in preprocessing.py: raw array in, label map out
from .preprocessing import predict_from_raw  # noqa: E402,F401
