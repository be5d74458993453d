"""The dataset fingerprint on the MI355X: the foreground intensity samples and statistics experiment planning and CTNormalization start
from.  With this module `raw dataset -> extract_fingerprint -> preprocessing.run_case -> DeviceDataset -> TrainBatches -> TrainStep` leaves
nothing but file reading on the host.

Mirrors DatasetFingerprintExtractor (dinounet/experiment_planning/dataset_fingerprint/fingerprint_extractor.py), in its order of
operations and of random draws:
    collect_foreground_intensities   :42-80   the samples and the per-case table of the voxels with seg > 0
    analyze_case                     :82-105  without the file reading: crop_to_nonzero, then the above
    extract_fingerprint              :107-194 (run) without the worker pool and the json file

CUDA tensors run csrc/fingerprint.hip (C ABI `du_fp_*`); CPU tensors run a numpy restatement of the same semantics,
which is what the GPU tests compare the kernels against (tests/test_cpu_fingerprint.py checks it against np.percentile, np.median and
RandomState.choice themselves).  The foreground voxel list `images[c][mask]` is never built on the device: order statistics come from a
radix select over the image, the samples from a select-by-rank, both at ranks the host computes.

Arithmetic, pinned to numpy 2.2: for float32 input np.percentile works in float32 throughout,
    q32 = float32(q) / float32(100);  v = float32(float32(n - 1) q32);  lo = floor(v);  hi = min(lo + 1, n - 1);  g = float32(v - lo)
    a, b = sorted[lo], sorted[hi];  d = float32(b - a);  result = b - d (1 - g) if g >= 0.5 else a + d g, every step rounded to float32
and np.median is float32(float32(sorted[(n - 1) // 2] + sorted[n // 2]) / 2).  Above n = 2^24 the virtual index v is a ROUNDED float32
(n = 10^8, q = 99.5: exactly 99 500 000).  lo, hi and g are computed on the host by this recipe, the device returns a and b, and the last
three operations are numpy float32 scalars on the host.  min, max, median, the percentiles and the samples therefore equal numpy to the bit.

Differences from the reference, on purpose:
  * `mean` is the fp64 sum in a fixed order divided by n and `std` the population standard deviation from a second fp64 pass (as for
    ZScoreNormalization); numpy's float32 pairwise recipe differs from that by its own summation error;
  * the statistics are Python floats and the samples one (C, num_samples) tensor on the input's device, (C, 0) without foreground (the
    reference: numpy scalars and a list of arrays, [] without foreground);
  * NaN among the foreground voxels raises ValueError (the reference asserts on the whole image);
  * a dataset without a single foreground sample raises ValueError (the reference fails inside numpy)."""
import math

import numpy as np
import torch

from . import _lib
from . import preprocessing

PERCENTILES = (("percentile_00_5", 0.5), ("percentile_99_5", 99.5))
RMAX = 8                            # targets du_fp_order_stats serves in one call


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------ numpy's float32 arithmetic
def virtual_index(n, q):
    """np.percentile's 'linear' virtual index for n float32 values -> (lo, hi, g): the two ranks and the float32 weight"""
    q32 = np.float32(q) / np.float32(100)
    v = np.float32(np.float32(n - 1) * q32)
    lo = min(int(np.floor(v)), n - 1)
    hi = min(lo + 1, n - 1)
    return lo, hi, np.float32(v - np.float32(lo))


def lerp(a, b, g):
    """numpy's _lerp on float32 scalars"""
    a, b, g = np.float32(a), np.float32(b), np.float32(g)
    d = np.float32(b - a)
    if g >= 0.5:
        return np.float32(b - np.float32(d * np.float32(np.float32(1) - g)))
    return np.float32(a + np.float32(d * g))


def _rank_plan(n):
    """the ranks the statistics of n members need, and what to do with the values found there"""
    ranks = [(n - 1) // 2, n // 2]
    weights = []
    for _, q in PERCENTILES:
        lo, hi, g = virtual_index(n, q)
        ranks += [lo, hi]
        weights.append(g)
    return ranks, weights


def _order_dict(values, weights):
    """values: the floats found at _rank_plan's ranks"""
    with np.errstate(over="ignore", invalid="ignore"):
        v = [np.float32(x) for x in values]
        out = {"median": float(np.float32(np.float32(v[0] + v[1]) / np.float32(2)))}
        for i, (name, _) in enumerate(PERCENTILES):
            out[name] = float(lerp(v[2 + 2 * i], v[3 + 2 * i], weights[i]))
    return out


# ------------------------------------------------------------------------------------------------ the three device operations
def _check_flat(img, seg):
    if not isinstance(img, torch.Tensor) or img.ndim != 2 or img.dtype != torch.float32 or not img.is_contiguous() or img.numel() == 0:
        raise ValueError("img must be a contiguous float32 (C, n) tensor with n >= 1")
    if seg is not None:
        if not isinstance(seg, torch.Tensor) or seg.dtype != torch.int16 or tuple(seg.shape) != (img.shape[1],) or not seg.is_contiguous():
            raise ValueError("seg must be a contiguous int16 (n) tensor")
        if seg.device != img.device:
            raise ValueError("img and seg must be on one device")


def workspace_elems(C, n):
    """int32 words the du_fp_* calls need; RuntimeError naming DU_ERR_BAD_ARG / DU_ERR_UNSUPPORTED for a shape they do not take (nothing
    is launched or allocated)"""
    w = int(_lib.lib().du_fp_ws_elems(int(C), int(n)))
    if w < 0:
        _lib.check(w, "du_fp_ws_elems")
    return w


def _workspace(img):
    C, n = (int(i) for i in img.shape)
    w = workspace_elems(C, n)
    return torch.empty(w, dtype=torch.int32, device=img.device), w


def _members_numpy(img, seg):
    x = img.numpy()
    return x if seg is None else x[:, seg.numpy() > 0]


def foreground_moments(img, seg, with_std=False, ws=None):
    """img (C, n) fp32, seg (n) int16 or None -> (C, 6) fp64 tensor on img's device: {member count, min, max, fp64 sum, count of NaN members,
    fp64 sum of (x - sum / count)^2 (0 without with_std)}; members are the elements with seg > 0, all of them without seg.  min / max are
    +inf / -inf without members."""
    _check_flat(img, seg)
    C, n = (int(i) for i in img.shape)
    if not img.is_cuda:
        m = _members_numpy(img, seg)
        out = np.zeros((C, 6), np.float64)
        for c in range(C):
            x = m[c]
            ok = x[~np.isnan(x)]
            s = float(x.astype(np.float64).sum()) if x.size else 0.0
            out[c, :5] = (x.size, ok.min() if ok.size else np.inf, ok.max() if ok.size else -np.inf, s, x.size - ok.size)
            if with_std and x.size:
                out[c, 5] = float(((x.astype(np.float64) - s / x.size) ** 2).sum())
        return torch.from_numpy(out)
    L = _lib.lib()
    ws, ws_elems = _workspace(img) if ws is None else ws
    stats = torch.empty((C, 6), dtype=torch.float64, device=img.device)
    for mode in (0, 1) if with_std else (0,):
        _lib.check(L.du_fp_moments(img.data_ptr(), None if seg is None else seg.data_ptr(), C, n, mode, stats.data_ptr(), ws.data_ptr(),
                                   ws_elems, _stream()), "du_fp_moments")
    return stats


def _check_ranks(ranks, img, width=None):
    if not isinstance(ranks, torch.Tensor) or ranks.dtype != torch.int64 or ranks.ndim != 2 or ranks.shape[0] != img.shape[0] or \
            ranks.device != img.device or ranks.shape[1] < 1:
        raise ValueError("ranks must be an int64 (C, R) tensor on img's device")
    if width is not None and ranks.shape[1] > width:
        raise ValueError(f"at most {width} ranks per channel in one call")
    return ranks.contiguous()


def foreground_order_stats(img, seg, ranks, ws=None):
    """ranks (C, R <= 8) int64 on img's device, each in [0, member count) -> fp32 (C, R) = np.sort(members of channel c)[ranks[c]].  A rank
    outside that range gives NaN."""
    _check_flat(img, seg)
    ranks = _check_ranks(ranks, img, RMAX)
    C, n = (int(i) for i in img.shape)
    R = int(ranks.shape[1])
    if not img.is_cuda:
        m = np.sort(_members_numpy(img, seg), axis=1)
        r = ranks.numpy()
        out = np.full((C, R), np.nan, np.float32)
        ok = (r >= 0) & (r < m.shape[1])
        for c in range(C):
            out[c, ok[c]] = m[c][r[c][ok[c]]]
        return torch.from_numpy(out)
    ws, ws_elems = _workspace(img) if ws is None else ws
    out = torch.empty((C, R), dtype=torch.float32, device=img.device)
    _lib.check(_lib.lib().du_fp_order_stats(img.data_ptr(), None if seg is None else seg.data_ptr(), C, n, ranks.data_ptr(), R,
                                            out.data_ptr(), ws.data_ptr(), ws_elems, _stream()), "du_fp_order_stats")
    return out


def foreground_sample(img, seg, ranks, ws=None):
    """ranks (C, m) int64 on img's device, ranks of the members in raster order, any order, repeats allowed -> fp32 (C, m) =
    img[c][seg > 0][ranks[c]].  A rank outside [0, member count) gives NaN."""
    _check_flat(img, seg)
    ranks = _check_ranks(ranks, img)
    C, n = (int(i) for i in img.shape)
    m = int(ranks.shape[1])
    if not img.is_cuda:
        mem = _members_numpy(img, seg)
        r = ranks.numpy()
        out = np.full((C, m), np.nan, np.float32)
        ok = (r >= 0) & (r < mem.shape[1])
        for c in range(C):
            out[c, ok[c]] = mem[c][r[c][ok[c]]]
        return torch.from_numpy(out)
    ws, ws_elems = _workspace(img) if ws is None else ws
    out = torch.empty((C, m), dtype=torch.float32, device=img.device)
    _lib.check(_lib.lib().du_fp_sample(img.data_ptr(), None if seg is None else seg.data_ptr(), C, n, ranks.data_ptr(), m, out.data_ptr(),
                                       ws.data_ptr(), ws_elems, _stream()), "du_fp_sample")
    return out


# ------------------------------------------------------------------------------------------------ the reference's functions
def _statistics(img, seg, with_std, what):
    """the moments read-back, then the order statistics at the host's ranks -> (member count, list of C dicts, workspace); raises for NaN"""
    ws = _workspace(img) if img.is_cuda else None
    rows = foreground_moments(img, seg, with_std=with_std, ws=ws).tolist()            # the first read-back: it sizes everything after it
    n = int(rows[0][0])
    if any(r[4] > 0 for r in rows):
        raise ValueError(f"{what} contain NaN values")
    if n == 0:
        return 0, None, ws
    ranks, weights = _rank_plan(n)
    C = int(img.shape[0])
    table = torch.tensor([ranks] * C, dtype=torch.int64).to(img.device)
    found = foreground_order_stats(img, seg, table, ws=ws).tolist()                   # the second and last read-back
    stats = []
    for c in range(C):
        d = {"mean": rows[c][3] / n, "min": rows[c][1], "max": rows[c][2]}
        d.update(_order_dict(found[c], weights))
        if with_std:
            d["std"] = math.sqrt(rows[c][5] / n)
        stats.append(d)
    return n, stats, ws


def intensity_statistics(samples):
    """the dataset-level step of extract_fingerprint: samples (C, N) fp32, every element a member -> a list of C dicts {mean, median, std,
    min, max, percentile_99_5, percentile_00_5} of Python floats.  On the device: both moment passes, one read-back of the (C, 6) row, the
    order statistics, one read-back of them."""
    n, stats, _ = _statistics(samples, None, True, "the foreground samples")
    return stats


def collect_foreground_intensities(segmentation, images, seed=1234, num_samples=10000):
    """DatasetFingerprintExtractor.collect_foreground_intensities (:42-80).  images: contiguous fp32 (C, D, H, W); segmentation: int16
    (1, D, H, W) on the same device, as crop_to_nonzero returns them.  Returns (intensities, stats): intensities a fp32 (C, num_samples)
    tensor on the input's device = for channel 0, 1, ... in turn images[c][segmentation[0] > 0][rs.randint(0, n_fg, num_samples)] with one
    RandomState(seed) (which consumes the stream exactly as rs.choice(foreground_pixels, num_samples, replace=True) does), (C, 0) without
    foreground; stats a list of C dicts {mean, median, min, max, percentile_99_5, percentile_00_5} of Python floats, NaN without
    foreground.  ValueError for NaN among the foreground voxels.

    On the device the moments row is read back first (the count sizes the draw and the virtual indices), then one (C, 6) copy of the
    order statistics; nothing else crosses to the host."""
    preprocessing._check_image(images, "images")
    if not isinstance(segmentation, torch.Tensor) or segmentation.dtype != torch.int16 or \
            tuple(segmentation.shape) != (1, *images.shape[1:]) or segmentation.device != images.device:
        raise ValueError("segmentation must be an int16 (1, D, H, W) tensor of the image's spatial shape on its device")
    num_samples = int(num_samples)
    if num_samples < 0:
        raise ValueError("num_samples must not be negative")
    C = int(images.shape[0])
    img = images.reshape(C, -1)
    seg = segmentation.contiguous().reshape(-1)
    n_fg, stats, ws = _statistics(img, seg, False, "the foreground voxels")
    if n_fg == 0:
        nan = float("nan")
        keys = ("mean", "median", "min", "max", "percentile_99_5", "percentile_00_5")
        return torch.empty((C, 0), dtype=torch.float32, device=images.device), [{k: nan for k in keys} for _ in range(C)]
    if num_samples == 0:
        return torch.empty((C, 0), dtype=torch.float32, device=images.device), stats
    rs = np.random.RandomState(seed)
    draws = np.stack([rs.randint(0, n_fg, num_samples).astype(np.int64) for _ in range(C)])
    intensities = foreground_sample(img, seg, torch.from_numpy(draws).to(images.device), ws=ws)
    return intensities, stats


def analyze_case(images, segmentation, spacing, num_samples=10000):
    """DatasetFingerprintExtractor.analyze_case (:82-105) for a case that has been read: images (C, D, H, W) of any dtype
    preprocessing.crop_to_nonzero takes, segmentation (1, D, H, W) integer.  Returns (shape_after_crop, spacing, intensities, stats,
    relative_size_after_cropping) with intensities and stats as collect_foreground_intensities returns them."""
    data, seg, _ = preprocessing.crop_to_nonzero(images, segmentation)
    intensities, stats = collect_foreground_intensities(seg, data, num_samples=num_samples)
    shape_before, shape_after = tuple(int(i) for i in images.shape[1:]), tuple(int(i) for i in data.shape[1:])
    relative = float(np.prod(shape_after) / np.prod(shape_before))
    return shape_after, spacing, intensities, stats, relative


def extract_fingerprint(cases, num_foreground_voxels=10e7):
    """DatasetFingerprintExtractor.run (:107-194) for cases = a sequence of (images, segmentation, spacing): every case keeps
    int(num_foreground_voxels // len(cases)) foreground samples per channel; the samples stay on the device, are concatenated per channel
    and their statistics computed there.  Returns {'spacings', 'shapes_after_crop', 'foreground_intensity_properties_per_channel':
    {c: {mean, median, std, min, max, percentile_99_5, percentile_00_5}} of Python floats (what preprocessing.normalize takes as
    intensity_properties), 'median_relative_size_after_cropping'}.  ValueError if no case has a foreground voxel."""
    cases = list(cases)
    if not cases:
        raise ValueError("no case given")
    num_samples = int(num_foreground_voxels // len(cases))
    results = [analyze_case(images, segmentation, spacing, num_samples) for images, segmentation, spacing in cases]
    if len({int(r[2].shape[0]) for r in results}) != 1:
        raise ValueError("every case of a dataset has the same number of channels")
    samples = torch.cat([r[2] for r in results], dim=1).contiguous()
    if samples.shape[1] == 0:
        raise ValueError("no case has a foreground voxel (or no samples were asked for): there are no intensities to describe")
    stats = intensity_statistics(samples)
    keys = ("mean", "median", "std", "min", "max", "percentile_99_5", "percentile_00_5")
    return {"spacings": [r[1] for r in results],
            "shapes_after_crop": [r[0] for r in results],
            "foreground_intensity_properties_per_channel": {c: {k: float(s[k]) for k in keys} for c, s in enumerate(stats)},
            "median_relative_size_after_cropping": float(np.median([r[4] for r in results], 0))}
