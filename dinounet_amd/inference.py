"""Sliding-window inference with Gaussian blending on the MI355X -- SURVEY.md 8(f) rank 2: the consumer of the forward path that
produces the segmentation the Dice metric is computed on.  Mirrors the reference predictor
(dinounet/inference/predict_from_raw_data.py:503-535 slicers, :571-621 accumulation, :680-727 padding / un-padding;
dinounet/inference/sliding_window_prediction.py:10-60 Gaussian map and step positions) for the 2D networks of this repo:

    data (C, D, H, W): every slice d is tiled with `patch_size` windows at `tile_step_size`; each window's logits are weighted with
    a Gaussian importance map (sigma = patch / 8, peak value 10, zeros replaced by the smallest non-zero value), accumulated, and the
    sum is divided by the accumulated weights.

Differences from the reference, all on purpose: windows are run through the network in batches (the reference predicts one window
per forward); the accumulators are fp32 (the reference keeps fp16 buffers and aborts on overflow, :612-615); the weighted
accumulate and the final division are two HIP kernels (csrc/window.hip: du_window_accumulate_cases, csrc/elementwise.hip:
du_window_normalize) instead of two indexed read-modify-write torch ops per window.  Test-time mirroring (predict_from_raw_data.py:537-552: the prediction is
averaged with the un-flipped predictions of every non-empty combination of the allowed mirror axes) is available through
mirror_axes=...; the in-trainer validation passes use_mirroring=False (nnUNetTrainer.py:1160), the stand-alone predictor defaults to
the checkpoint's inference_allowed_mirroring_axes.  There is no CPU path: the module needs the GPU.
What follows the logits in the reference (resampling, argmax / region paint, bbox paste, per-case metrics; export_prediction.py:15-68,
evaluate_predictions.py:152-234) is export.py: predict_segmentation runs the window loop below and goes from the accumulators straight
to the label map.
A LIST of cases (predict_from_raw_data.py:330-427, predict_from_list_of_npy_arrays / predict_from_data_iterator, which loop case by case)
goes through predict_cases_logits / predict_cases_segmentation / predict_from_list_of_npy_arrays and their EnsemblePredictor methods: the
windows of consecutive cases share window batches (plan_case_batches), so a list of small 2-D cases pays ceil(windows / batch) forwards
instead of one mostly empty forward per case.  Around the `forward` two kernels of csrc/window.hip stand where torch glue and float
atomics would: du_window_gather builds a batch straight from several cases, the padding folded in, and du_window_accumulate_cases adds
the weighted logits with one owner lane per accumulator element in slot order -- the reference's sequential loop in fp32 to the bit,
reproducible, and independent of which cases share a batch.  There is ONE window loop (_window_loop_cases): the single-case functions run
it on the list of one, and a network and an EnsemblePredictor go through the same _accumulate_cases.
The importance map is the outer product of the filtered 1-D deltas (equal to filtering the patch, to the bit), memoised per
(patch, sigma_scale) as the reference memoises it (sliding_window_prediction.py:10).
`acvl_utils.pad_nd_image` (not vendored in the reference tree) is restated from its published behaviour: centred constant padding
up to the patch size, extra pixel on the high side."""
import contextlib
import itertools

import numpy as np
import torch

from . import _lib


_DELTA_CACHE = {}


def _filtered_delta(tile_size, sigma_scale):
    """float64 gaussian_filter(delta at tile // 2, sigma = tile * sigma_scale, mode='constant') without filtering the tile: the filter is
    separable and every sample but the delta is 0, so each pass multiplies the previous result by the filtered 1-D delta of its axis (all
    other terms are 0 * w) -- the outer product of the lines, taken in scipy's axis order, is the filtered tile to the bit."""
    key = (tile_size, sigma_scale)
    if key not in _DELTA_CACHE:
        from scipy.ndimage import gaussian_filter
        g = None
        for n in tile_size:
            line = np.zeros(n)
            line[n // 2] = 1
            line = gaussian_filter(line, n * sigma_scale, 0, mode="constant", cval=0)
            g = line if g is None else np.multiply.outer(g, line)
        _DELTA_CACHE[key] = g
    return _DELTA_CACHE[key]


def compute_gaussian(tile_size, sigma_scale=1.0 / 8, value_scaling_factor=1.0, dtype=torch.float32, device="cpu"):
    """sliding_window_prediction.py:10-31 (scipy's gaussian_filter of a centred delta, normalised to `value_scaling_factor`).
    The filtered delta comes from _filtered_delta: memoised per (tile_size, sigma_scale), as the reference memoises; everything after it
    makes new tensors, so the returned map is the caller's own."""
    g = torch.from_numpy(_filtered_delta(tuple(int(i) for i in tile_size), float(sigma_scale)))
    g = g / torch.max(g) * value_scaling_factor                # a new tensor: the memoised array is never written
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
        if n != self.x.shape[0] or x.data_ptr() != self.x.data_ptr():       # (the cases path gathers straight into self.x: nothing to copy)
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


class _NetPredictor:
    """A plain network in the three things in which it differs from an EnsemblePredictor for the window loop: the forward of a window batch
    (with the cache its captures live in), what is put into eval mode and restored, and the fold count."""
    folds = 1

    def __init__(self, net):
        self.net = net
        self.device = next(net.parameters()).device
        if self.device.type != "cuda":
            raise RuntimeError("sliding-window inference runs on the MI355X (no CPU fallback)")

    def _eager_forward(self, xb):
        out = self.net(xb)
        if isinstance(out, (list, tuple)):
            out = out[0]
        return out.float().contiguous()

    def _captures(self):
        # cached on the module: replays read the parameters / running statistics in place, so the capture stays valid
        # while they are updated (not if they are re-allocated: clear_window_cache(net) then)
        return self.net.__dict__.setdefault("_sw_forward_cache", {}), (str(self.device),)

    @contextlib.contextmanager
    def _eval_mode(self):
        was_training = self.net.training
        self.net.eval()
        try:
            yield
        finally:
            self.net.train(was_training)


def _window_forward(predictor, batch_size, graph):
    """the `forward` of _window_loop_cases for a predictor (in eval mode while it is called): eager, or the captured full window batch"""
    if not graph:
        return predictor._eager_forward

    def captured(C, ph, pw):
        cache, key_tail = predictor._captures()
        key = (batch_size, C, ph, pw, *key_tail)
        if key not in cache:
            cache[key] = _WindowForward(predictor._eager_forward, (batch_size, C, ph, pw), predictor.device)
        return cache[key]

    def graph_forward(xb):
        return captured(*xb.shape[1:])(xb)

    graph_forward.static_input = lambda C, ph, pw: captured(C, ph, pw).x      # _window_loop_cases gathers into it
    return graph_forward


# ------------------------------------------------------------------------------------------------ the window loop: a list of cases, windows batched across them
MAX_WINDOW_BATCH = 64               # du_window_accumulate_cases: one ballot bit per slot of a launch


def _padded_shape(shape, patch_size):
    D, H, W = (int(i) for i in shape)
    return D, max(H, int(patch_size[0])), max(W, int(patch_size[1]))


def plan_case_batches(shapes, patch_size, tile_step_size, batch_size, max_voxels_in_flight=2 ** 26):
    """Which windows share a forward when a list of cases is predicted.  shapes: (D, H, W) of every case.  Consecutive cases are grouped
    greedily: a case joins the current group unless the group is non-empty and the accumulator voxels D * Hp * Wp of the group (Hp, Wp: the
    padded frame of pad_to_patch) would exceed max_voxels_in_flight; a case larger than the budget is a group of its own.  The windows of a
    group form one list -- cases in list order, each case's windows in sliding_window_origins order -- cut into consecutive chunks of
    batch_size, so only a group's last chunk can be ragged.  Returns [(case indices, [chunk, ...]), ...] with chunk = [(case, d, y0, x0),
    ...], `case` the index into `shapes`, y0 / x0 in the padded frame.  Forwards: count_case_forwards."""
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError("batch_size must be positive")
    padded = [_padded_shape(s, patch_size) for s in shapes]
    groups, current, voxels = [], [], 0
    for i, (D, Hp, Wp) in enumerate(padded):
        if current and voxels + D * Hp * Wp > max_voxels_in_flight:
            groups.append(current)
            current, voxels = [], 0
        current.append(i)
        voxels += D * Hp * Wp
    if current:
        groups.append(current)
    plan = []
    for members in groups:
        windows = [(i, d, y0, x0) for i in members for d, y0, x0 in sliding_window_origins(padded[i], patch_size, tile_step_size)]
        plan.append((members, [windows[j:j + batch_size] for j in range(0, len(windows), batch_size)]))
    return plan


def count_case_forwards(plan, mirror_axes=None):
    """network forwards of a plan: one per chunk, times 1 + the number of mirror combinations"""
    return sum(len(chunks) for _, chunks in plan) * (1 + len(mirror_axes_combinations(mirror_axes, 4)))


def _gather_cases_numpy(cases, desc, patch_size, slots=None):
    """du_window_gather on the host: cases = float32 arrays (C, D, H, W), desc = [(case, d, y0, x0), ...] -> x (slots, C, ph, pw) float32.
    Element (y, x) of a window reads source row y0 + y - lo_y, column x0 + x - lo_x of its case; outside the image it is 0, and so are the
    slots after the last descriptor."""
    ph, pw = int(patch_size[0]), int(patch_size[1])
    C = cases[0].shape[0]
    x = np.zeros((len(desc) if slots is None else slots, C, ph, pw), dtype=np.float32)
    for s, (i, d, y0, x0) in enumerate(desc):
        H, W = cases[i].shape[2:]
        sy = y0 + np.arange(ph) - (max(H, ph) - H) // 2
        sx = x0 + np.arange(pw) - (max(W, pw) - W) // 2
        iy, ix = np.flatnonzero((sy >= 0) & (sy < H)), np.flatnonzero((sx >= 0) & (sx < W))
        x[s][:, iy[:, None], ix[None, :]] = np.asarray(cases[i], dtype=np.float32)[:, d][:, sy[iy][:, None], sx[ix][None, :]]
    return x


def _accumulate_cases_numpy(logits, gauss, desc, preds, npreds):
    """du_window_accumulate_cases on the host, float32, in place: logits (nb, K, ph, pw), gauss (ph, pw), desc = [(case, d, y0, x0), ...],
    preds[case] (K, D, Hp, Wp), npreds[case] (D, Hp, Wp).  As the kernel: slot b owns the elements of its window that no lower slot of the
    same case and slice covers; an owned element is read once, gets the rounded product logit * g (npred: g) of every covering slot added
    in slot order, and is written once."""
    logits, gauss = np.asarray(logits, dtype=np.float32), np.asarray(gauss, dtype=np.float32)
    nb, K, ph, pw = logits.shape
    yy, xx = np.mgrid[0:ph, 0:pw]

    def covers(j, Y, X):
        return (Y >= desc[j][2]) & (Y < desc[j][2] + ph) & (X >= desc[j][3]) & (X < desc[j][3] + pw)

    for b, (i, d, y0, x0) in enumerate(desc):
        Y, X = yy + y0, xx + x0
        meets = [j for j in range(nb) if j != b and desc[j][0] == i and desc[j][1] == d]
        owned = np.ones((ph, pw), dtype=bool)
        for j in meets:
            if j < b:
                owned &= ~covers(j, Y, X)
        Y, X = Y[owned], X[owned]
        acc, acc_n = preds[i][:, d, Y, X], npreds[i][d, Y, X]                       # the one read (fancy indexing copies)
        for j in [b] + [j for j in meets if j > b]:
            c = covers(j, Y, X)
            yj, xj = Y[c] - desc[j][2], X[c] - desc[j][3]
            g = gauss[yj, xj]
            acc[:, c] = acc[:, c] + logits[j][:, yj, xj] * g                        # float32: the product is rounded, then added
            acc_n[c] = acc_n[c] + g
        preds[i][:, d, Y, X], npreds[i][d, Y, X] = acc, acc_n                       # the one write


def _check_cases(list_of_data, batch_size, properties=None):
    """the ValueErrors of the cases path, before any launch; returns the cases as tensors"""
    if isinstance(list_of_data, (torch.Tensor, np.ndarray)) or len(list_of_data) == 0:
        raise ValueError("list_of_data must be a non-empty list of (C, D, H, W) arrays")
    cases = [torch.as_tensor(c) for c in list_of_data]
    for i, c in enumerate(cases):
        if c.ndim != 4 or c.numel() == 0:
            raise ValueError(f"case {i} must be a 4D tensor (c, d, y, x), got shape {tuple(c.shape)}")
        if c.shape[0] != cases[0].shape[0]:
            raise ValueError(f"case {i} has {c.shape[0]} channels, case 0 has {cases[0].shape[0]}")
    if not 1 <= int(batch_size) <= MAX_WINDOW_BATCH:
        raise ValueError(f"batch_size must be in 1..{MAX_WINDOW_BATCH} on the cases path, got {batch_size}")
    if properties is not None and (isinstance(properties, dict) or len(properties) != len(cases)):
        raise ValueError(f"properties must be a list with one entry per case ({len(cases)})")
    return cases


def _window_loop_cases(forward, dev, cases, patch_size, tile_step_size, use_gaussian, batch_size, mirror_axes, sink, full_batch=False,
                       max_voxels_in_flight=2 ** 26):
    """The window loop, for a list of (C, D, H, W) cases (a single case is the list of one): the windows of consecutive cases share window
    batches (plan_case_batches).  forward(x (b, C, ph, pw)) -> contiguous fp32 logits of at least b windows (a captured forward hands back
    its whole batch, in a buffer it reuses).  Per group the accumulators are allocated and the tables uploaded once; per chunk
    du_window_gather builds the batch straight from the cases (no padded copy), _mirror_and_predict runs the forward, and
    du_window_accumulate_cases adds the weighted logits without float atomics, in the reference's order -- a chunk above MAX_WINDOW_BATCH in
    consecutive launches of at most that many slots.  full_batch: gather all batch_size slots (zeros after the last window)
    -- the static buffer of a captured forward, which the gather then writes directly (forward.static_input) unless mirroring needs the
    un-flipped batch kept; otherwise a ragged chunk is a smaller batch.  When a group is done, sink([(case index, pred
    (K, D, Hp, Wp), npred (D, Hp, Wp), (y slice, x slice)), ...]) gets the un-normalised accumulators, which are dropped after it returns.
    A sink launches its device work and may return a callable that reads the result's non-finite flags back and raises; the loop calls it
    at once, except the last group's, which it returns: the caller restores the training flags first (host work under the device's last
    chunks) and synchronises after."""
    ph, pw = int(patch_size[0]), int(patch_size[1])
    plan = plan_case_batches([c.shape[1:] for c in cases], (ph, pw), tile_step_size, batch_size, max_voxels_in_flight)
    gauss = (compute_gaussian((ph, pw), sigma_scale=1.0 / 8, value_scaling_factor=10, dtype=torch.float32, device=dev)
             if use_gaussian else torch.ones((ph, pw), dtype=torch.float32, device=dev)).contiguous()
    combos = mirror_axes_combinations(mirror_axes, 4)
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    C = int(cases[0].shape[0])
    # a captured forward offers its static input: the gather writes the batch there and the replay copies nothing.  Not with mirroring:
    # the flipped batches go through that buffer while the un-flipped one is still needed.
    static = getattr(forward, "static_input", None) if full_batch and not combos else None
    xbuf = static(C, ph, pw) if static is not None else torch.empty((batch_size, C, ph, pw), dtype=torch.float32, device=dev)
    for members, chunks in plan:
        local = {i: j for j, i in enumerate(members)}
        vols = [cases[i].to(dev, torch.float32).contiguous() for i in members]
        n = len(vols)
        # the group's tables, one host->device copy each: source pointers, geometries, every window of the group
        src = torch.tensor([v.data_ptr() for v in vols], dtype=torch.int64).to(dev)
        geom = torch.tensor([list(v.shape[1:]) for v in vols], dtype=torch.int32).to(dev)
        desc_all = torch.tensor([[local[i], d, y0, x0] for chunk in chunks for i, d, y0, x0 in chunk], dtype=torch.int32).to(dev)
        preds = npreds = acc = None
        w0 = 0
        for chunk in chunks:
            nb = len(chunk)
            slots = batch_size if full_batch else nb
            x, desc = xbuf[:slots], desc_all[w0:w0 + nb]
            w0 += nb
            _lib.check(L.du_window_gather(src.data_ptr(), geom.data_ptr(), desc.data_ptr(), x.data_ptr(), n, nb, slots, C, ph, pw, st),
                       "du_window_gather")
            logits = _mirror_and_predict(forward, x, combos)
            if (logits.ndim != 4 or logits.shape[0] < nb or tuple(logits.shape[2:]) != (ph, pw) or logits.dtype != torch.float32
                    or not logits.is_contiguous() or logits.device != xbuf.device):
                raise RuntimeError(f"forward must return contiguous fp32 logits (>= {nb}, K, {ph}, {pw}) on the device, got "
                                   f"{tuple(logits.shape)} {logits.dtype}")
            K = int(logits.shape[1])
            if preds is None:                                              # (the number of heads is known after the first forward)
                shapes = [_padded_shape(v.shape[1:], (ph, pw)) for v in vols]
                preds = [torch.zeros((K, *s), dtype=torch.float32, device=dev) for s in shapes]
                npreds = [torch.zeros(s, dtype=torch.float32, device=dev) for s in shapes]
                # the accumulators' pointer table, written by fill launches: an upload at this point would hold the host until the first
                # forward is through, and with it what the caller does under the device's work (restoring the training flags)
                acc = torch.empty((2, n), dtype=torch.int64, device=dev)
                for j in range(n):
                    acc[0, j], acc[1, j] = preds[j].data_ptr(), npreds[j].data_ptr()
            elif K != preds[0].shape[0]:
                raise RuntimeError(f"forward returned {K} heads after {preds[0].shape[0]}")
            for s0 in range(0, nb, MAX_WINDOW_BATCH):                      # (launches of one stream are ordered, slots keep window order)
                _lib.check(L.du_window_accumulate_cases(logits[s0:].data_ptr(), gauss.data_ptr(), desc[s0:].data_ptr(), geom.data_ptr(),
                                                        acc[0].data_ptr(), acc[1].data_ptr(), n, min(nb - s0, MAX_WINDOW_BATCH), K, ph, pw, st),
                           "du_window_accumulate_cases")
        group = []
        for j, i in enumerate(members):
            H, W = (int(e) for e in vols[j].shape[2:])
            lo_y, lo_x = (max(H, ph) - H) // 2, (max(W, pw) - W) // 2
            group.append((i, preds[j], npreds[j], (slice(lo_y, lo_y + H), slice(lo_x, lo_x + W))))
        check = sink(group)
        del group, preds, npreds, vols
        if check is not None and members is not plan[-1][0]:
            check()
    return check


def _non_finite_check(group, bad, named):
    """what a sink returns: one synchronising read-back of a group's non-finite flags `bad` (device, one per case), and the reference's
    error (:612-615).  named: the message lists the cases (not for the single-case functions, which have no list)."""
    indices = [g[0] for g in group]                                                # (not the group: its accumulators are dropped)

    def check():
        raised = [i for i, f in zip(indices, bad.tolist()) if f]
        if raised:
            raise RuntimeError("Encountered inf in predicted array" + (f" (cases {raised})" if named else ""))
    return check


def _logits_sink(out, named=True):
    """sink of _window_loop_cases: normalise, un-pad, and the check of the cases' maxima together"""
    def sink(group):
        L = _lib.lib()
        st = torch.cuda.current_stream().cuda_stream
        worst = []
        for i, pred, npred, (ys, xs) in group:
            _lib.check(L.du_window_normalize(pred.data_ptr(), npred.data_ptr(), pred.shape[0], npred.numel(), st), "du_window_normalize")
            worst.append(torch.stack(torch.aminmax(pred)))                         # (no |pred| temporary; a NaN comes through both)
            out[i] = pred[:, :, ys, xs]
        return _non_finite_check(group, ~torch.isfinite(torch.stack(worst)).all(1), named)
    return sink


def _segmentation_sink(out, regions_class_order, properties, transpose_backward, return_probabilities, named=True):
    """sink of _window_loop_cases: export._export of every case from its un-normalised accumulators; the non-finite flags of a group sit in
    one tensor and are read back together.  properties: None or one dict per case."""
    from . import export

    def sink(group):
        flags = torch.zeros(len(group), dtype=torch.int32, device=group[0][1].device)
        for j, (i, pred, npred, (ys, xs)) in enumerate(group):
            window = (ys.start, xs.start, ys.stop - ys.start, xs.stop - xs.start)
            out[i] = export._export(pred, npred, window, regions_class_order, None if properties is None else properties[i],
                                    transpose_backward, return_probabilities, flag=flags[j:j + 1])
        return _non_finite_check(group, flags, named)
    return sink


@torch.no_grad()
def _accumulate_cases(net, cases, patch_size, tile_step_size, use_gaussian, batch_size, graph, mirror_axes, sink, max_voxels_in_flight=2 ** 26):
    """The predictor (a network, or an EnsemblePredictor) in eval mode around _window_loop_cases.  The accumulators hold the SUM over the
    folds; every case's n_predictions is scaled by the fold count before `sink` sees it, so that sums / n_predictions is the mean logit
    (one (D, H, W) plane, instead of a pass over the K planes)."""
    predictor = net if isinstance(net, EnsemblePredictor) else _NetPredictor(net)

    def scaled(group):
        for _, _, npred, _ in group:
            npred.mul_(float(predictor.folds))
        return sink(group)

    with predictor._eval_mode():
        check = _window_loop_cases(_window_forward(predictor, batch_size, graph), predictor.device, cases, patch_size, tile_step_size,
                                   use_gaussian, batch_size, mirror_axes, sink if predictor.folds == 1 else scaled, full_batch=graph,
                                   max_voxels_in_flight=max_voxels_in_flight)
    check()                            # the last group's read-back, after the flags: restoring them overlaps the device's last chunks


@torch.no_grad()
def predict_sliding_window_logits(net, data, patch_size, tile_step_size=0.5, use_gaussian=True, batch_size=8, graph=False,
                                  mirror_axes=None):
    """data (C, D, H, W) on the GPU (or host: moved once) -> fp32 logits (K, D, H, W) on the GPU.
    predict_from_raw_data.py:680-727 with _internal_predict_sliding_window_return_logits :571-621.  graph=True replays a captured
    forward of a full window batch (worth it from a few batches per volume on).  mirror_axes: allowed_mirroring_axes of the
    predictor (for this 2D path a subset of (0, 1) = the window's rows / columns), None = no test-time mirroring.  The case runs as the
    list of one (predict_cases_logits; any positive batch_size), so the logits are reproducible and in the reference's summation order."""
    assert data.ndim == 4, "input_image must be a 4D tensor (c, d, y, x)"
    out = [None]
    _accumulate_cases(net, [data], patch_size, tile_step_size, use_gaussian, batch_size, graph, mirror_axes, _logits_sink(out, named=False))
    return out[0]


@torch.no_grad()
def predict_cases_logits(net, list_of_data, patch_size, tile_step_size=0.5, use_gaussian=True, batch_size=8, graph=False, mirror_axes=None,
                         *, max_voxels_in_flight=2 ** 26):
    """predict_sliding_window_logits for a list of (C, D, H, W) cases of any sizes (one channel count) -> list of fp32 logits (K, D, H, W) on
    the GPU.  Windows of consecutive cases share window batches (plan_case_batches: sum over groups of ceil(windows / batch_size) forwards
    instead of one or more per case), which is what small 2-D cases need; the accumulation has no float atomics, so a case's logits are
    reproducible and do not depend on the cases it shares batches with.  batch_size <= 64.  max_voxels_in_flight bounds the accumulator
    voxels of the cases that are open at a time.  `net`: a network, or an EnsemblePredictor (whose methods call these functions)."""
    cases = _check_cases(list_of_data, batch_size)
    out = [None] * len(cases)
    _accumulate_cases(net, cases, patch_size, tile_step_size, use_gaussian, batch_size, graph, mirror_axes, _logits_sink(out),
                      max_voxels_in_flight)
    return out


@torch.no_grad()
def predict_cases_segmentation(net, list_of_data, patch_size, tile_step_size=0.5, use_gaussian=True, batch_size=8, graph=False,
                               mirror_axes=None, *, regions_class_order=None, properties=None, transpose_backward=None,
                               return_probabilities=False, max_voxels_in_flight=2 ** 26):
    """export.predict_segmentation for a list of cases: the window loop over the list (predict_cases_logits), then every case goes from its
    un-normalised accumulators to its label map in one pass.  properties: None or one dict per case.  Returns a list of uint8 label maps,
    with return_probabilities a list of (seg, probs)."""
    cases = _check_cases(list_of_data, batch_size, properties)
    out = [None] * len(cases)
    sink = _segmentation_sink(out, regions_class_order, properties, transpose_backward, return_probabilities)
    _accumulate_cases(net, cases, patch_size, tile_step_size, use_gaussian, batch_size, graph, mirror_axes, sink, max_voxels_in_flight)
    return out


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
    folds, one du_window_accumulate_cases.  The reference re-runs the whole network F times.

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

    # the three things _accumulate_cases asks of a predictor (_NetPredictor: the same of a plain network)
    folds = property(lambda self: len(self.nets))

    def _captures(self):
        return self._forward_cache, ()                                     # backbone + F heads: one graph per (batch, C, patch)

    @contextlib.contextmanager
    def _eval_mode(self):
        modes = _training_flags(self.backbone)
        self.backbone.eval()
        try:
            yield
        finally:
            _set_training_flags(modes)

    def predict_logits(self, data, patch_size, tile_step_size=0.5, use_gaussian=True, batch_size=8, graph=False, mirror_axes=None):
        """predict_sliding_window_logits of the ensemble: the mean over the folds of the logits (K, D, H, W), fp32 on the GPU"""
        return predict_sliding_window_logits(self, data, patch_size, tile_step_size, use_gaussian, batch_size, graph, mirror_axes)

    def predict_segmentation(self, data, patch_size, tile_step_size=0.5, use_gaussian=True, batch_size=8, graph=False, mirror_axes=None, *,
                             regions_class_order=None, properties=None, transpose_backward=None, return_probabilities=False):
        """export.predict_segmentation of the ensemble: the window loop, then ONE pass from the accumulators to the label map.  The positive
        factor 1 / F cannot change a label, so without resampling the sums over folds and windows decide."""
        return predict_segmentation(self, data, patch_size, tile_step_size, use_gaussian, batch_size, graph, mirror_axes,
                                    regions_class_order=regions_class_order, properties=properties, transpose_backward=transpose_backward,
                                    return_probabilities=return_probabilities)

    def predict_cases_logits(self, list_of_data, patch_size, tile_step_size=0.5, use_gaussian=True, batch_size=8, graph=False,
                             mirror_axes=None, *, max_voxels_in_flight=2 ** 26):
        """predict_cases_logits of the ensemble: per case the mean over the folds of the logits (K, D, H, W), fp32 on the GPU"""
        return predict_cases_logits(self, list_of_data, patch_size, tile_step_size, use_gaussian, batch_size, graph, mirror_axes,
                                    max_voxels_in_flight=max_voxels_in_flight)

    def predict_cases_segmentation(self, list_of_data, patch_size, tile_step_size=0.5, use_gaussian=True, batch_size=8, graph=False,
                                   mirror_axes=None, *, regions_class_order=None, properties=None, transpose_backward=None,
                                   return_probabilities=False, max_voxels_in_flight=2 ** 26):
        """predict_cases_segmentation of the ensemble: a list of label maps (or of (seg, probs))"""
        return predict_cases_segmentation(self, list_of_data, patch_size, tile_step_size, use_gaussian, batch_size, graph, mirror_axes,
                                          regions_class_order=regions_class_order, properties=properties,
                                          transpose_backward=transpose_backward, return_probabilities=return_probabilities,
                                          max_voxels_in_flight=max_voxels_in_flight)

    def predict_from_raw(self, data, properties, patch_size, **kwargs):
        """preprocessing.predict_from_raw with this ensemble in place of one network: raw array in, ensemble label map out"""
        from .preprocessing import predict_from_raw
        return predict_from_raw(self, data, properties, patch_size, **kwargs)


# the export tail (label maps, probabilities, per-case metrics) lives in export.py; its names are part of this module's interface
from .export import case_metrics, logits_to_segmentation, predict_segmentation  # noqa: E402,F401
# ... and what precedes the window loop (crop, normalise, resample a raw case) in preprocessing.py: raw array in, label map out
from .preprocessing import predict_from_raw  # noqa: E402,F401


@torch.no_grad()
def predict_from_list_of_npy_arrays(net_or_predictor, image_or_list_of_images, properties_or_list_of_properties, patch_size, *,
                                    transpose_forward, spacing, normalization_schemes, use_mask_for_norm,
                                    foreground_intensity_properties_per_channel, list_of_parameters=None, **predict_kwargs):
    """nnUNetPredictor.predict_from_list_of_npy_arrays (predict_from_raw_data.py:330-427) without files: raw (C, X, Y, Z) arrays (numpy or
    torch) and their properties dicts in, the list of uint8 label maps in the raw geometries out.  preprocessing.run_case per case (it fills
    each properties dict, as for predict_from_raw), then the cases path -- predict_cases_segmentation with every case's properties and
    transpose_backward = the inverse of transpose_forward -- so the windows of small cases share forwards.  A single array with a single
    dict is accepted (the result is still a list).  net_or_predictor: a network (optionally with list_of_parameters = the folds' parameter
    sets) or an EnsemblePredictor.  predict_kwargs: those of predict_cases_segmentation.  The list is checked as a whole before anything is
    launched; then it is preprocessed and predicted group by group (the groups of plan_case_batches under max_voxels_in_flight), so only one
    group's preprocessed cases and accumulators are on the device at a time."""
    from .preprocessing import _check_transpose, run_case
    if isinstance(image_or_list_of_images, (np.ndarray, torch.Tensor)):
        if not isinstance(properties_or_list_of_properties, dict):
            raise ValueError("a single image goes with a single properties dict")
        images, props = [image_or_list_of_images], [properties_or_list_of_properties]
    else:
        images, props = list(image_or_list_of_images), properties_or_list_of_properties
        if isinstance(props, dict) or props is None or len(props) != len(images):
            raise ValueError(f"properties must be a list with one dict per image ({len(images)})")
        props = list(props)
    for k in ("properties", "transpose_backward"):
        if k in predict_kwargs:
            raise ValueError(f"predict_from_list_of_npy_arrays derives {k} itself")
    # every ValueError of the list before anything is launched (run_case would meet a bad case only after its predecessors ran)
    images = _check_cases(images, predict_kwargs.get("batch_size", 8))
    for j, q in enumerate(props):
        if not isinstance(q, dict) or "spacing" not in q or len(q["spacing"]) != 3:
            raise ValueError(f"properties of case {j} must be a dict whose 'spacing' holds the three raw spacings")
    tf = _check_transpose(transpose_forward)
    if list_of_parameters is not None:
        if isinstance(net_or_predictor, EnsemblePredictor):
            raise ValueError("list_of_parameters goes with a network, not with an EnsemblePredictor")
        net_or_predictor = EnsemblePredictor(net_or_predictor, list_of_parameters)
    transpose_backward = [tf.index(i) for i in range(3)]
    budget = predict_kwargs.get("max_voxels_in_flight", 2 ** 26)
    out, pre, first, voxels = [], [], 0, 0

    def flush():
        return predict_cases_segmentation(net_or_predictor, pre, patch_size, properties=props[first:first + len(pre)],
                                          transpose_backward=transpose_backward, **predict_kwargs)

    # group by group, by the rule of plan_case_batches: the preprocessed cases of one group are all that is held at a time, and as window
    # batches never span groups the label maps are those of one call on the whole list
    for j, (img, q) in enumerate(zip(images, props)):
        case = run_case(img, None, q, transpose_forward=tf, spacing=spacing, normalization_schemes=normalization_schemes,
                        use_mask_for_norm=use_mask_for_norm,
                        foreground_intensity_properties_per_channel=foreground_intensity_properties_per_channel)[0]
        D, Hp, Wp = _padded_shape(case.shape[1:], patch_size)
        if pre and voxels + D * Hp * Wp > budget:
            out += flush()
            pre, first, voxels = [], j, 0
        pre.append(case)
        voxels += D * Hp * Wp
    return out + flush()
