"""Training batches on the MI355X: the class-location tables of a preprocessed case, the 2-D loader that draws a batch from cases that stay
on the device, and the iterator that hands augmented batches to TrainStep.  After this module `raw case -> preprocessing.run_case ->
DeviceDataset -> DataLoader2D -> GPUAugment2D -> TrainStep` has no host array in it.

Mirrors, in the reference's order of operations and of random draws:
    sample_foreground_locations   DefaultPreprocessor._sample_foreground_locations (default_preprocessor.py:157-181)
    add_class_locations           default_preprocessor.py:94-111 (what fills properties['class_locations'])
    DataLoader2D                  nnUNetDataLoader2D.generate_train_batch (data_loader_2d.py:7-87) and nnUNetDataLoaderBase.get_bbox
                                  (base_data_loader.py:64-139)
    split_batch_for_rank          nnUNetTrainer._set_batch_size_and_oversample (nnUNetTrainer.py:308-353)
    initial_patch_size            configure_rotation_dummyDA_mirroring_and_inital_patch_size (:391-441) for two dimensions
    TrainBatches                  get_dataloaders (:601-650) without the worker processes

Random decisions are drawn on the host from a numpy RandomState the object owns, exactly as the reference draws them from numpy's global
stream (RandomState(s) and np.random.seed(s) agree draw for draw); per-voxel work runs in csrc/dataload.hip (C ABI `du_dl_*`, DESIGN
section 3f).  CPU tensors run a numpy restatement of the same semantics; the GPU tests compare the kernels against it and
tests/test_cpu_dataloading.py checks it against brute force.  `batchgenerators` and `acvl_utils` are not vendored by the reference:
what it takes from them (DataLoader.get_indices = np.random.choice(indices, batch_size, True, p); get_patch_size and rotate_coords_2d)
is restated from their published behaviour.

A class or region is an int64 bit mask over the labels 0..63 (training._region_masks): a voxel whose label is below 0 or above 63 is in
no mask, and asking for a class outside 0..63 raises ValueError."""
from collections.abc import Mapping

import numpy as np
import torch

from . import _lib
from .training import _region_masks, labels_to_regions

NUM_SAMPLES = 10000                 # default_preprocessor.py:159
MIN_PERCENT_COVERAGE = 0.01         # :160


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------ class locations
def _entry_key(c):
    """the reference's key: the int, or tuple(region)"""
    if isinstance(c, (tuple, list, np.ndarray)):
        return tuple(int(l) for l in c)
    return int(c)


def _entry_masks(classes_or_regions):
    keys = [_entry_key(c) for c in classes_or_regions]
    return keys, _region_masks(keys)                                                  # ValueError for a label outside 0..63


def _check_label_map(seg):
    """(1, D, H, W) or (D, H, W) integer tensor -> contiguous int16 (D, H, W)"""
    if not isinstance(seg, torch.Tensor) or seg.ndim not in (3, 4) or (seg.ndim == 4 and seg.shape[0] != 1):
        raise ValueError("seg must be a (1, D, H, W) or (D, H, W) torch tensor")
    if seg.is_floating_point() or seg.dtype == torch.bool:
        raise ValueError("seg must be an integer tensor")
    if seg.numel() == 0:
        raise ValueError("empty segmentation")
    if seg.ndim == 4:
        seg = seg[0]
    return seg.to(torch.int16).contiguous()


def target_num_samples(n):
    """how many of a class's n voxels the table keeps (:176-177): all of them up to 10 000, then 10 000, then 1 % once that is more"""
    return max(min(NUM_SAMPLES, n), int(np.ceil(n * MIN_PERCENT_COVERAGE)))


def workspace_elems(D, H, W, G):
    """int32 words du_dl_class_counts needs; RuntimeError naming DU_ERR_BAD_ARG / DU_ERR_UNSUPPORTED for a shape it does not take (nothing
    is launched or allocated)"""
    n = int(_lib.lib().du_dl_ws_elems(int(D), int(H), int(W), int(G)))
    if n < 0:
        _lib.check(n, "du_dl_ws_elems")
    return n


def _member_numpy(seg, bits):
    """bool array: the label is in 0..63 and its bit is set"""
    s = seg.astype(np.int64)
    ok = (s >= 0) & (s <= 63)
    return ok & (((np.uint64(bits & (2 ** 64 - 1)) >> np.where(ok, s, 0).astype(np.uint64)) & np.uint64(1)) != 0)


class ClassCounts:
    """The member counts of G masks over one label map, and what selecting members by rank needs.  `totals` is an int64 (G) tensor on
    seg's device.  CUDA: du_dl_class_counts has run on the current stream, its workspace is kept here; CPU: numpy."""

    def __init__(self, seg, classes_or_regions):
        self.seg = _check_label_map(seg)
        self.keys, self.masks = _entry_masks(classes_or_regions)
        if not self.keys:
            raise ValueError("no class or region given")
        D, H, W = (int(i) for i in self.seg.shape)
        G = len(self.keys)
        if not self.seg.is_cuda:
            s = self.seg.numpy()
            self.totals = torch.tensor([int(_member_numpy(s, b).sum()) for b in self.masks], dtype=torch.int64)
            return
        dev = self.seg.device
        self.ws_elems = workspace_elems(D, H, W, G)
        self.ws = torch.empty(self.ws_elems, dtype=torch.int32, device=dev)
        self.table = torch.tensor(self.masks, dtype=torch.int64, device=dev)
        self.totals = torch.empty(G, dtype=torch.int64, device=dev)
        _lib.check(_lib.lib().du_dl_class_counts(self.seg.data_ptr(), self.table.data_ptr(), G, D, H, W, self.ws.data_ptr(), self.ws_elems,
                                                 self.totals.data_ptr(), _stream()), "du_dl_class_counts")

    def select(self, g, ranks):
        """ranks (m) int64 on seg's device, each in [0, totals[g]), in any order -> int32 (m, 4) = np.argwhere(mask_g[None])[ranks]"""
        if ranks.dtype != torch.int64 or ranks.ndim != 1 or ranks.device != self.seg.device:
            raise ValueError("ranks must be a 1-D int64 tensor on seg's device")
        m = int(ranks.numel())
        if not self.seg.is_cuda:
            locs = np.argwhere(_member_numpy(self.seg.numpy(), self.masks[g])[None])
            return torch.from_numpy(locs[ranks.numpy()].astype(np.int32))
        D, H, W = (int(i) for i in self.seg.shape)
        ranks = ranks.contiguous()
        out = torch.empty((m, 4), dtype=torch.int32, device=self.seg.device)
        _lib.check(_lib.lib().du_dl_select(self.seg.data_ptr(), self.table.data_ptr(), len(self.keys), int(g), D, H, W, self.ws.data_ptr(),
                                           self.ws_elems, ranks.data_ptr(), m, out.data_ptr(), _stream()), "du_dl_select")
        return out


def sample_foreground_locations(seg, classes_or_regions, seed=1234):
    """DefaultPreprocessor._sample_foreground_locations (default_preprocessor.py:157-181) for seg (1, D, H, W) or (D, H, W), an integer
    tensor: for every class (int) or region (tuple / list of ints) with n voxels, m = max(min(10000, n), ceil(0.01 n)) of them, chosen as
    np.argwhere(mask)[RandomState(seed).choice(n, m, replace=False)] with one RandomState shared by the entries in order.  Returns
    (tables, mirror): two dicts keyed by the int or tuple(region); tables[k] is an int32 (m, 4) tensor of {0, z, y, x} rows on seg's device
    (an absent class: shape (0, 4)), mirror[k] the same rows as a numpy array on the host (an absent class: [], as in the reference).
    The mirror is small (16 bytes a row) and is what DataLoader2D draws from.

    On the device (csrc/dataload.hip): one pass counts all G masks, the G totals are the one read-back (they size the tables and feed
    the host draw), then one select-by-rank launch per present class; the mirrors come back in one copy of the finished tables.  The
    voxel list np.argwhere would build is never materialised."""
    counts = ClassCounts(seg, classes_or_regions)
    dev = counts.seg.device
    totals = counts.totals.tolist()                                                   # the read-back
    rndst = np.random.RandomState(seed)
    parts, spans, at = [], [], 0
    for g, n in enumerate(totals):
        if n == 0:
            spans.append(None)
            continue
        m = target_num_samples(n)
        ranks = torch.from_numpy(rndst.choice(n, m, replace=False).astype(np.int64)).to(dev)
        parts.append(counts.select(g, ranks))
        spans.append((at, at + m))
        at += m
    flat = torch.cat(parts) if parts else torch.empty((0, 4), dtype=torch.int32, device=dev)
    host = flat.cpu().numpy()
    tables, mirror = {}, {}
    for k, span in zip(counts.keys, spans):
        tables[k] = flat[0:0] if span is None else flat[span[0]:span[1]]
        mirror[k] = [] if span is None else host[span[0]:span[1]]
    return tables, mirror


def add_class_locations(seg, properties, foreground_labels_or_regions, all_labels=None):
    """default_preprocessor.py:94-111 for a case preprocessing.run_case returned: properties['class_locations'] = the host mirror of
    sample_foreground_locations(seg, foreground labels or regions): numpy arrays, the reference's type, which DataLoader2D draws from.
    With an ignore label pass all_labels (every label but the ignore label, background included): the extra key tuple(all_labels),
    from which the loader picks annotated voxels, is appended as the last entry (:103-106).  Returns properties."""
    collect = list(foreground_labels_or_regions)
    if all_labels is not None:
        collect.append(tuple(int(l) for l in all_labels))
    properties["class_locations"] = sample_foreground_locations(seg, collect)[1]
    return properties


# ------------------------------------------------------------------------------------------------ the dataset
class DeviceDataset(Mapping):
    """key -> (data (C, D, H, W) fp32, seg (1, D, H, W) int16, properties): the preprocessed cases of a training set, resident on one device
    (nnUNetDataset.load_case without the files).  properties['class_locations'] must be there (add_class_locations).  Every case has the
    same number of channels.

    Memory: the cases are never evicted, so the set takes 4 C + 2 bytes per voxel (a 3-channel case of 512 x 512 pixels: 3.7 MB; 1000 of
    them: 3.7 GB of the MI355X's 288 GB) plus, on the host, 16 bytes per row of the class-location tables (at most max(10 000, 1 %) rows per class).  A set
    that does not fit has to be sharded by the caller.  CPU tensors are accepted too: the loader then runs its numpy restatement."""

    def __init__(self, cases=None):
        self._cases = {}
        for k, (data, seg, properties) in (cases or {}).items():
            self.add(k, data, seg, properties)

    def add(self, key, data, seg, properties):
        if not isinstance(data, torch.Tensor) or data.ndim != 4 or data.dtype != torch.float32 or data.numel() == 0:
            raise ValueError("data must be a float32 (C, D, H, W) tensor")
        if not isinstance(seg, torch.Tensor) or seg.dtype != torch.int16 or tuple(seg.shape) != (1, *data.shape[1:]):
            raise ValueError("seg must be an int16 (1, D, H, W) tensor of the image's spatial shape")
        if seg.device != data.device:
            raise ValueError("data and seg must be on one device")
        if "class_locations" not in properties:
            raise ValueError("properties['class_locations'] is missing: run add_class_locations on the case first")
        if self._cases:
            d0 = next(iter(self._cases.values()))[0]
            if d0.shape[0] != data.shape[0] or d0.device != data.device:
                raise ValueError("every case of a dataset has the same number of channels and lives on the same device")
        self._cases[key] = (data.contiguous(), seg.contiguous(), properties)

    def load_case(self, key):
        return self._cases[key]

    def __getitem__(self, key):
        return self._cases[key]

    def __iter__(self):
        return iter(self._cases)

    def __len__(self):
        return len(self._cases)

    def nbytes(self):
        """bytes of image and segmentation the set keeps resident"""
        return sum(d.numel() * 4 + s.numel() * 2 for d, s, _ in self._cases.values())


# ------------------------------------------------------------------------------------------------ the loader
class DataLoader2D:
    """nnUNetDataLoader2D: batches of 2-D patches from the slices of the cases of `dataset` (a DeviceDataset), foreground oversampled.

    draw() makes every random decision of one batch on the host, with the reference's draws in the reference's order from self.rs:
      1. rs.choice(keys, batch_size, True, sampling_probabilities) (batchgenerators' get_indices; drawn here as the index into the key
         list, which consumes the stream identically and does not need keys numpy can hold);
      then per sample j
      2. force_fg = not j < round(batch_size (1 - oversample_foreground_percent)), or rs.uniform() < oversample_foreground_percent with
         probabilistic_oversampling;
      3. the class: without force_fg the annotated-classes key tuple(all_labels) under has_ignore, else none; with force_fg the classes
         with a non-empty table, minus the annotated-classes key when others exist, one of them by rs.choice(len(eligible)) (none if
         the case has no foreground);
      4. the slice: rs.choice(table[:, 1]) with a class, else rs.choice(D);
      5. get_bbox: need_to_pad = patch_size - final_patch_size, grown per axis so that need_to_pad + shape >= patch_size;
         lbs = -need_to_pad // 2, ubs = shape + need_to_pad // 2 + need_to_pad % 2 - patch_size; with a class the voxel is
         rows_in_slice[rs.choice(len(rows_in_slice))] and bbox_lb = max(lb, voxel - patch_size // 2) -- there is NO clamp against ubs, as
         in the reference: a voxel near the high edge puts the box past the image; without a class rs.randint(lb, ub + 1) per axis.
    assemble(d) uploads one (B, 8) job table and gathers the whole batch in one launch (du_dl_gather): 'data' (B, C, *patch_size) fp32,
    zero outside the image; 'seg' (B, 1, *patch_size) int16, -1 outside (fp32 with seg_float=True, what GPUAugment2D.apply takes).  A
    dataset of CPU tensors runs the numpy restatement of the same window.  next(loader) = {'data', 'seg', 'keys', 'properties'}; the
    decisions of the last batch stay in loader.last_draw.

    Departures from the reference, on purpose: under has_ignore a case with no annotated voxel (an empty annotated-classes table)
    raises ValueError where the reference would index an empty list; the tensors stay on the dataset's device."""

    def __init__(self, dataset, batch_size, patch_size, final_patch_size, all_labels, has_ignore, oversample_foreground_percent=0.33,
                 sampling_probabilities=None, probabilistic_oversampling=False, seed=None, seg_float=False):
        if len(dataset) == 0:
            raise ValueError("empty dataset")
        self.dataset = dataset
        self.batch_size = int(batch_size)
        self.patch_size = tuple(int(v) for v in patch_size)
        self.final_patch_size = tuple(int(v) for v in final_patch_size)
        if self.batch_size < 1 or len(self.patch_size) != 2 or len(self.final_patch_size) != 2 or min(self.patch_size) < 1:
            raise ValueError("batch_size >= 1 and two positive patch extents are required")
        self.need_to_pad = [p - f for p, f in zip(self.patch_size, self.final_patch_size)]        # base_data_loader.py:31
        self.oversample_foreground_percent = float(oversample_foreground_percent)
        self.sampling_probabilities = sampling_probabilities
        self.probabilistic_oversampling = bool(probabilistic_oversampling)
        self.annotated_classes_key = tuple(int(l) for l in all_labels)
        self.has_ignore = bool(has_ignore)
        self.seg_float = bool(seg_float)
        self.list_of_keys = list(dataset.keys())
        if self.has_ignore:
            for k in self.list_of_keys:
                if self.annotated_classes_key not in dataset[k][2]["class_locations"]:
                    raise ValueError(f"case {k!r}: class_locations lacks the annotated-classes key {self.annotated_classes_key} "
                                     "(add_class_locations(..., all_labels=...))")
        self.rs = np.random.RandomState(seed)
        self.last_draw = None
        self._jobs = None

    # ---- decisions (host) -----------------------------------------------------------------------------------------------------
    def _do_oversample(self, j):
        if self.probabilistic_oversampling:
            return self.rs.uniform() < self.oversample_foreground_percent              # base_data_loader.py:51-53
        return not j < round(self.batch_size * (1 - self.oversample_foreground_percent))             # :45-49

    def get_bbox(self, shape, locations):
        """base_data_loader.py:64-139 for a slice of `shape` (H, W); locations: the chosen class's rows {0, y, x} in that slice, or None
        for a random position -> (bbox_lbs, bbox_ubs)"""
        need = list(self.need_to_pad)
        for d in range(2):
            if need[d] + shape[d] < self.patch_size[d]:
                need[d] = self.patch_size[d] - shape[d]
        lbs = [-need[i] // 2 for i in range(2)]
        ubs = [shape[i] + need[i] // 2 + need[i] % 2 - self.patch_size[i] for i in range(2)]
        if locations is not None:
            voxel = locations[self.rs.choice(len(locations))]
            bbox_lbs = [max(lbs[i], int(voxel[i + 1]) - self.patch_size[i] // 2) for i in range(2)]
        else:
            bbox_lbs = [int(self.rs.randint(lbs[i], ubs[i] + 1)) for i in range(2)]
        return bbox_lbs, [bbox_lbs[i] + self.patch_size[i] for i in range(2)]

    def draw(self):
        """All random decisions of one batch -> dict (also the input of the restatement): 'keys' (the cases), 'force_fg', 'classes' (the
        class or region each patch was centred on, or None), 'slices' (B) and 'bbox_lbs' (B, 2) int64"""
        rs, B = self.rs, self.batch_size
        idx = rs.choice(len(self.list_of_keys), B, True, self.sampling_probabilities)
        keys = [self.list_of_keys[int(i)] for i in idx]
        force, classes = [], []
        slices, lbs = np.zeros(B, np.int64), np.zeros((B, 2), np.int64)
        for j, key in enumerate(keys):
            force_fg = bool(self._do_oversample(j))
            data, _, properties = self.dataset[key]
            locs = properties["class_locations"]
            if not force_fg:
                selected = self.annotated_classes_key if self.has_ignore else None
            else:
                eligible = [k for k in locs.keys() if len(locs[k]) > 0]
                hit = [k == self.annotated_classes_key if isinstance(k, tuple) else False for k in eligible]
                if any(hit) and len(eligible) > 1:
                    eligible.pop(hit.index(True))
                selected = eligible[rs.choice(len(eligible))] if len(eligible) > 0 else None
            if self.has_ignore and (selected is None or len(locs[selected]) == 0):
                raise ValueError(f"case {key!r} has an ignore label and no annotated voxel: there is nothing to sample from")
            if selected is not None:
                table = np.asarray(locs[selected])
                z = int(rs.choice(table[:, 1]))
                in_slice = table[table[:, 1] == z][:, (0, 2, 3)]
            else:
                z = int(rs.choice(int(data.shape[1])))
                in_slice = None
            bbox_lbs, _ = self.get_bbox([int(data.shape[2]), int(data.shape[3])], in_slice)
            force.append(force_fg)
            classes.append(selected)
            slices[j] = z
            lbs[j] = bbox_lbs
        return dict(keys=keys, force_fg=force, classes=classes, slices=slices, bbox_lbs=lbs)

    # ---- the batch ------------------------------------------------------------------------------------------------------------
    def assemble(self, d, seg_float=None):
        """d = draw() -> (data (B, C, ph, pw) fp32, seg (B, 1, ph, pw) int16 or fp32) on the dataset's device"""
        seg_float = self.seg_float if seg_float is None else bool(seg_float)
        ph, pw = self.patch_size
        cases = [self.dataset[k] for k in d["keys"]]
        B, C = len(cases), int(cases[0][0].shape[0])
        for j, (data, _, _) in enumerate(cases):
            if not 0 <= int(d["slices"][j]) < data.shape[1]:
                raise ValueError(f"sample {j}: slice {int(d['slices'][j])} outside the case's {int(data.shape[1])} slices")
        dev = cases[0][0].device
        if dev.type != "cuda":
            out = np.zeros((B, C, ph, pw), np.float32)
            sout = np.full((B, 1, ph, pw), -1, np.float32 if seg_float else np.int16)
            for j, (data, seg, _) in enumerate(cases):
                z, (y0, x0) = int(d["slices"][j]), (int(v) for v in d["bbox_lbs"][j])
                H, W = int(data.shape[2]), int(data.shape[3])
                ya, yb, xa, xb = max(0, y0), min(H, y0 + ph), max(0, x0), min(W, x0 + pw)        # the part of the box inside the image
                if ya < yb and xa < xb:
                    out[j, :, ya - y0:yb - y0, xa - x0:xb - x0] = data.numpy()[:, z, ya:yb, xa:xb]
                    sout[j, :, ya - y0:yb - y0, xa - x0:xb - x0] = seg.numpy()[:, z, ya:yb, xa:xb]
            return torch.from_numpy(out), torch.from_numpy(sout)
        jobs = np.zeros((B, 8), np.int64)
        for j, (data, seg, _) in enumerate(cases):
            jobs[j] = (data.data_ptr(), seg.data_ptr(), data.shape[1], data.shape[2], data.shape[3], d["slices"][j], d["bbox_lbs"][j][0],
                       d["bbox_lbs"][j][1])
        # (pinned and asynchronous: an upload from pageable memory would make the host wait for the work already queued on the stream)
        self._jobs = _lib.upload([jobs], np.int64, dev)[0]                           # stays referenced until the next batch replaces it
        out = torch.empty((B, C, ph, pw), dtype=torch.float32, device=dev)
        sout = torch.empty((B, 1, ph, pw), dtype=torch.float32 if seg_float else torch.int16, device=dev)
        _lib.check(_lib.lib().du_dl_gather(self._jobs.data_ptr(), B, C, ph, pw, out.data_ptr(), sout.data_ptr(), int(seg_float), _stream()),
                   "du_dl_gather")
        return out, sout

    def __iter__(self):
        return self

    def __next__(self):
        d = self.draw()
        data, seg = self.assemble(d)
        self.last_draw = d
        return {"data": data, "seg": seg, "keys": d["keys"], "properties": [self.dataset[k][2] for k in d["keys"]]}


# ------------------------------------------------------------------------------------------------ trainer arithmetic
def split_batch_for_rank(global_batch, oversample_percent, rank, world):
    """nnUNetTrainer._set_batch_size_and_oversample (nnUNetTrainer.py:308-353) -> (batch_size, oversample_percent) of `rank` among `world`
    ranks.  world == 1 (no DDP) returns the arguments.  The first global_batch % world ranks get one sample more; a rank whose samples all
    lie below (above) the oversampled tail of the global batch gets 0.0 (1.0), any other the share of its own samples that fall in the
    tail, where the tail is decided by the loader's rounding rule on the GLOBAL batch.  ValueError for global_batch < world."""
    global_batch, rank, world = int(global_batch), int(rank), int(world)
    if world < 1 or not 0 <= rank < world:
        raise ValueError(f"rank {rank} outside a world of {world}")
    if world == 1:
        return global_batch, oversample_percent
    if global_batch < world:
        raise ValueError("Cannot run DDP if the batch size is smaller than the number of GPUs")
    per = [global_batch // world] * world
    per = [per[i] + 1 if per[i] * world + i < global_batch else per[i] for i in range(world)]
    assert sum(per) == global_batch
    low, high = sum(per[:rank]), sum(per[:rank + 1])
    oversample = [not i < round(global_batch * (1 - oversample_percent)) for i in range(global_batch)]
    if high / global_batch < (1 - oversample_percent):
        share = 0.0
    elif low / global_batch > (1 - oversample_percent):
        share = 1.0
    else:
        share = sum(oversample[low:high]) / per[rank]
    return per[rank], share


def rotation_limit(patch_size):
    """the 2-D rotation range GPUAugment2D uses (nnUNetTrainer.py:398-412): 15 degrees for patches with aspect > 1.5, else 180, in radians"""
    return (15.0 if max(patch_size) / min(patch_size) > 1.5 else 180.0) / 360 * 2.0 * np.pi


def initial_patch_size(patch_size):
    """configure_rotation_dummyDA_mirroring_and_inital_patch_size (nnUNetTrainer.py:391-441) for a 2-D patch: the patch the loader must cut
    so that rotation and down-scaling never read outside it.  batchgenerators' get_patch_size(patch, rot_x, rot_y, rot_z, (0.85, 1.25)),
    restated: the patch vector is rotated by min(90 degrees, rotation limit), the elementwise max of |rotated| and the patch is divided
    by 0.85 and truncated.  rotate_coords_2d is restated as coords @ [[cos, -sin], [sin, cos]], i.e. (a cos + b sin, b cos - a sin);
    the reference does not vendor the package, so the convention is unpinned against it -- the transposed matrix gives
    (a cos - b sin, a sin + b cos), which differs only for non-square patches at the 15 degree limit.  (512, 512) gives (602, 602) under
    either."""
    patch = np.array([int(v) for v in patch_size])
    if patch.shape != (2,) or patch.min() < 1:
        raise ValueError("a 2-D patch size is required")
    rot = min(90 / 360 * 2.0 * np.pi, rotation_limit(patch))
    c, s = np.cos(rot), np.sin(rot)
    rotated = np.dot(patch.astype(np.float64), np.array([[c, -s], [s, c]]))
    final = np.max(np.vstack((np.abs(rotated), patch)), 0)
    final /= 0.85
    return tuple(int(v) for v in final.astype(int))


# ------------------------------------------------------------------------------------------------ batches for TrainStep
class TrainBatches:
    """An endless iterator of (x, target) for TrainStep / ValStep from a DeviceDataset (nnUNetTrainer.get_dataloaders, :601-650, without
    worker processes: nothing leaves the device, so there is nothing to overlap).

    Training (val=False): split_batch_for_rank(batch_size, oversample_foreground_percent, rank, world) sizes this rank's loader; a
    DataLoader2D cuts patches of initial_patch_size(patch_size) with the labels as fp32; GPUAugment2D(patch_size) augments them and
    crops to patch_size (its output labels are >= 0: RemoveLabel(-1, 0) is part of it).  Validation (val=True, get_validation_transforms):
    the loader's patch is patch_size itself, no augmentation, -1 -> 0.
    x is fp32 (B, C, *patch_size); target is the int64 (B, 1, *patch_size) label map TrainStep(x_shape, tgt_shape) copies into its static
    buffer, whose loss (training.build_loss, regions included) takes label maps.  With `regions` the target is instead what
    training.labels_to_regions(target, regions, ignore_label) gives, uint8 (B, R + u, *patch_size), for a loss that takes the one-hot
    region target (training.dc_and_bce_loss); leave regions=None for a TrainStep whose SegLoss converts inside the captured step.
    With ignore_label, all_labels (every label but the ignore label) names the annotated-classes table.  The loader draws from
    RandomState(seed), the augmentation from RandomState(seed + 1); last_draw = (loader decisions, augmentation decisions or None).

    Known seam against batchgenerators: the loader pads the segmentation with -1, and du_aug_spatial counts an IN-IMAGE negative label
    as weight against every label (as it does a neighbour outside its input), while batchgenerators' order-1 label interpolation counts
    such a pixel as 0 in the other labels' one-hot maps.  A pixel with bilinear weight w on label c and v on padding is c there when
    w >= 1/2 and here when w - v >= 1/2; everywhere else both give 0 after RemoveLabel(-1, 0).  The difference is confined to the
    one-pixel seam between image and padding, where a label can be one pixel narrower here.  du_aug_spatial is existing behaviour and
    is left as it is.  With interpolation="spline" the seam is absent: du_aug_spatial_spline treats -1 as a label of
    its own, as batchgenerators does.

    interpolation and use_mask_for_norm (one bool per channel, or channel indices) go to GPUAugment2D(interpolation=..., mask_channels=...):
    "spline" resamples as batchgenerators does, and the masked channels are 0 wherever the resampled segmentation is negative."""

    def __init__(self, dataset, patch_size, batch_size, oversample_foreground_percent=0.33, all_labels=None, regions=None, ignore_label=None,
                 seed=None, rank=0, world=1, val=False, sampling_probabilities=None, probabilistic_oversampling=False, interpolation="keys",
                 use_mask_for_norm=None):
        from .augment import GPUAugment2D
        self.patch_size = tuple(int(v) for v in patch_size)
        self.val = bool(val)
        self.regions = None if regions is None else [_entry_key(r) for r in regions]
        self.ignore_label = None if ignore_label is None else int(ignore_label)
        if self.ignore_label is not None and all_labels is None:
            raise ValueError("with an ignore label, all_labels (every other label, background included) is required")
        self.batch_size, self.oversample_foreground_percent = split_batch_for_rank(batch_size, oversample_foreground_percent, rank, world)
        loader_patch = self.patch_size if self.val else initial_patch_size(self.patch_size)
        self.loader = DataLoader2D(dataset, self.batch_size, loader_patch, self.patch_size, () if all_labels is None else all_labels,
                                   self.ignore_label is not None, self.oversample_foreground_percent, sampling_probabilities,
                                   probabilistic_oversampling, seed=seed, seg_float=not self.val)
        self.augment = None if self.val else GPUAugment2D(self.patch_size, seed=None if seed is None else int(seed) + 1,
                                                          interpolation=interpolation, mask_channels=use_mask_for_norm)
        dev = next(iter(dataset.values()))[0].device
        self.table = None
        if self.regions is not None and dev.type == "cuda":
            self.table = torch.tensor(_region_masks(self.regions), dtype=torch.int64, device=dev)
        self.last_draw = None

    def __iter__(self):
        return self

    def __next__(self):
        d = self.loader.draw()
        data, seg = self.loader.assemble(d)
        if self.val:
            a, x = None, data
            target = torch.where(seg == -1, torch.zeros_like(seg), seg).long()        # RemoveLabelTransform(-1, 0)
        else:
            a = self.augment.draw(data.shape[0], data.shape[1])
            x, target = self.augment.apply(data, seg, a)
            target = target.long()
        if self.regions is not None:
            target = labels_to_regions(target, self.regions, self.ignore_label, table=self.table)
        self.last_draw = (d, a)
        return x, target


def downsample_seg_for_ds(seg, shapes_or_scales):
    """DownsampleSegForDSTransform2 (data_augmentation/custom_transforms/deep_supervision_donwsampling.py, the last training transform,
    nnUNetTrainer.py:770-771; order 0): seg (B,C,H,W) integer labels -> the reference's list, one map per entry.  An entry is a shape
    (h, w) of ints, or a scale: a float or one float per axis (deep_supervision_scales), giving round(H s), round(W s) as np.round does.
    An entry that keeps the size returns `seg` itself, as the reference does.  The maps are resize_segmentation(order=0) of seg, which is
    scipy.ndimage.zoom(order=0, mode="nearest", grid_mode=True): the source indices are training.ds_target_index per axis.  On the GPU
    one launch writes up to four maps (du_downsample_seg); on the CPU torch indexing.  DeepSupervisionLoss needs none of this: it
    resamples the full-resolution target inside its kernels."""
    from .training import downsample_target
    if seg.dim() != 4:
        raise ValueError(f"downsample_seg_for_ds: seg must be (B,C,H,W), got {tuple(seg.shape)}")
    H, W = int(seg.shape[2]), int(seg.shape[3])
    shapes = []
    for e in shapes_or_scales:
        e = list(e) if isinstance(e, (tuple, list)) else [e, e]
        if len(e) != 2:
            raise ValueError(f"downsample_seg_for_ds: entry {e!r} is neither a (h, w) shape nor one scale per axis")
        if all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in e):
            h, w = int(e[0]), int(e[1])
        else:
            h, w = int(round(H * float(e[0]))), int(round(W * float(e[1])))
        if not (1 <= h <= H and 1 <= w <= W):
            raise ValueError(f"downsample_seg_for_ds: entry {e!r} gives {(h, w)}, outside 1..{(H, W)}")
        shapes.append((h, w))
    small = [s for s in shapes if s != (H, W)]
    if seg.is_cuda and small:
        from . import ops
        made = iter(o if o.dtype == seg.dtype else o.to(seg.dtype) for o in ops.downsample_seg(seg, small))   # the kernel works in int64
        return [seg if s == (H, W) else next(made) for s in shapes]
    return [downsample_target(seg, s) for s in shapes]
