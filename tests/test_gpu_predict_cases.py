"""GPU tests (-m gpu) of the window loop of inference: du_window_gather and du_window_accumulate_cases (csrc/window.hip) to the bit against
the torch construction / the host restatement, _window_loop_cases to the bit against the plain construction (tests/_window_ref.py: padded
copy, slices, the sequential `+=`), the loop with a stand-in forward (forward counts, independence of the list's order, chunks above the
64 slots of a launch), the single-case functions as the list of one, and predict_cases_segmentation / predict_from_list_of_npy_arrays
against the single-case functions on a real network.

Bounds.  Kernels: bit for bit, no tolerance (a copy; a fixed order of fp32 operations).  End to end: the label maps of two runs whose fp32
summation order differs agree outside the tie band of tests/test_gpu_export.py (float64 top-two gap below 1e-5 * max|logit|) and the
share of differing voxels is below 1e-4, that file's bound."""
from functools import partial

import numpy as np
import pytest
import torch

from dinounet_amd import _lib
from dinounet_amd import export as EX
from dinounet_amd import inference as INF
from test_gpu_ops import dev, gen
from _window_ref import plain_accumulate, plain_window_sums

pytestmark = pytest.mark.gpu

CASES = [(1, 5, 7), (2, 8, 12), (1, 13, 12), (3, 9, 31)]        # smaller than the patch | equal | taller only | wider, odd width
PATCHES = [(8, 12), (6, 10)]
LIST_A = [(1, 40, 50), (1, 64, 64), (1, 70, 100), (1, 96, 96), (3, 64, 64), (1, 130, 64)]
BAND_REL = 1e-5


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a.cpu()), bits(b.cpu()))


def padded(shape, patch):
    return (shape[0], max(shape[1], patch[0]), max(shape[2], patch[1]))


def device_tables(vols, d):
    src = torch.tensor([v.data_ptr() for v in vols], dtype=torch.int64).to(d)
    geom = torch.tensor([list(v.shape[1:]) for v in vols], dtype=torch.int32).to(d)
    return src, geom


def stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------ du_window_gather
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("patch", PATCHES)
def test_gather_exact(patch, C):
    d = dev()
    vols = [gen(C, *s, seed=3 + i).to(d) for i, s in enumerate(CASES)]
    src, geom = device_tables(vols, d)
    (_, chunks), = INF.plan_case_batches(CASES, patch, 0.5, 13)
    assert len(chunks) >= 2 and len({w[0] for w in chunks[0]}) >= 3               # windows of at least 3 cases share a launch
    assert any(w[3] % 4 for c in chunks for w in c)                                # shifted x0
    for chunk in chunks:
        nb = len(chunk)
        x = torch.full((16, C, *patch), float("nan"), device=d)
        desc = torch.tensor(chunk, dtype=torch.int32).to(d)
        rc = _lib.lib().du_window_gather(src.data_ptr(), geom.data_ptr(), desc.data_ptr(), x.data_ptr(), len(vols), nb, 16, C, patch[0], patch[1],
                                         stream())
        assert rc == 0
        want = torch.stack([INF.pad_to_patch(vols[i], patch)[0][:, dd, y0:y0 + patch[0], x0:x0 + patch[1]] for i, dd, y0, x0 in chunk])
        assert same_bits(x[:nb], want)
        assert not bits(x[nb:]).any()                                              # the tail slots: +0.0, every bit
        host = INF._gather_cases_numpy([v.cpu().numpy() for v in vols], chunk, patch, slots=16)
        assert same_bits(x, torch.from_numpy(host))


# ------------------------------------------------------------------------------------------------ du_window_accumulate_cases
def accumulate_list(shapes, logits_of, gauss, patch, step, chunk_size, K, d):
    """the accumulators of `shapes` after every chunk of the plan went through the kernel; logits_of[(case, d, y0, x0)] (K, ph, pw)"""
    pshapes = [padded(s, patch) for s in shapes]
    preds = [torch.zeros((K, *s), device=d) for s in pshapes]
    npreds = [torch.zeros(s, device=d) for s in pshapes]
    acc = torch.tensor([[p.data_ptr() for p in preds], [p.data_ptr() for p in npreds]], dtype=torch.int64).to(d)
    geom = torch.tensor([list(s) for s in shapes], dtype=torch.int32).to(d)
    (_, chunks), = INF.plan_case_batches(shapes, patch, step, chunk_size)
    for chunk in chunks:
        logits = torch.stack([logits_of[w] for w in chunk]).to(d)
        desc = torch.tensor(chunk, dtype=torch.int32).to(d)
        rc = _lib.lib().du_window_accumulate_cases(logits.data_ptr(), gauss.data_ptr(), desc.data_ptr(), geom.data_ptr(), acc[0].data_ptr(),
                                                   acc[1].data_ptr(), len(shapes), len(chunk), K, patch[0], patch[1], stream())
        assert rc == 0
    return preds, npreds, chunks


@pytest.mark.parametrize("chunk_size", [1, 5, 16])
@pytest.mark.parametrize("step", [0.5, 0.3])
@pytest.mark.parametrize("patch", PATCHES)
def test_accumulate_exact(patch, step, chunk_size):
    d, K = dev(), 3
    gauss = INF.compute_gaussian(patch, sigma_scale=1.0 / 8, value_scaling_factor=10, device=d).contiguous()
    windows = [(i, *o) for i, s in enumerate(CASES) for o in INF.sliding_window_origins(padded(s, patch), patch, step)]
    g = torch.Generator().manual_seed(11)
    logits_of = {w: torch.randn((K, *patch), generator=g) for w in windows}
    preds, npreds, chunks = accumulate_list(CASES, logits_of, gauss, patch, step, chunk_size, K, d)
    if step == 0.3:                                                                # more than 4 windows meet in an element
        cover = np.zeros(padded(CASES[3], patch)[1:], int)
        for w in windows:
            if w[0] == 3 and w[1] == 0:
                cover[w[2]:w[2] + patch[0], w[3]:w[3] + patch[1]] += 1
        assert cover.max() > 4
    # the host restatement, chunk by chunk
    pshapes = [padded(s, patch) for s in CASES]
    want_p, want_n = [np.zeros((K, *s), np.float32) for s in pshapes], [np.zeros(s, np.float32) for s in pshapes]
    for chunk in chunks:
        INF._accumulate_cases_numpy(np.stack([logits_of[w].numpy() for w in chunk]), gauss.cpu().numpy(), chunk, want_p, want_n)
    for i in range(len(CASES)):
        assert same_bits(preds[i], torch.from_numpy(want_p[i])) and same_bits(npreds[i], torch.from_numpy(want_n[i]))
    # two runs are bit-identical
    again_p, again_n, _ = accumulate_list(CASES, logits_of, gauss, patch, step, chunk_size, K, d)
    for i in range(len(CASES)):
        assert same_bits(preds[i], again_p[i]) and same_bits(npreds[i], again_n[i])
    # a case's accumulators do not depend on the cases it shares launches with, nor on where the chunks are cut
    for i, s in enumerate(CASES):
        alone = {(0, *w[1:]): v for w, v in logits_of.items() if w[0] == i}
        p1, n1, _ = accumulate_list([s], alone, gauss, patch, step, chunk_size, K, d)
        assert same_bits(preds[i], p1[0]) and same_bits(npreds[i], n1[0])


def test_error_codes():
    d = dev()
    L = _lib.lib()
    t = torch.zeros(1024, device=d)
    tab = torch.zeros(256, dtype=torch.int64, device=d)
    p, q = t.data_ptr(), tab.data_ptr()
    BAD, UNSUPPORTED = -1, -2
    assert L.du_window_gather(None, q, q, p, 1, 1, 1, 1, 4, 4, stream()) == BAD
    assert L.du_window_gather(q, None, q, p, 1, 1, 1, 1, 4, 4, stream()) == BAD
    assert L.du_window_gather(q, q, None, p, 1, 1, 1, 1, 4, 4, stream()) == BAD
    assert L.du_window_gather(q, q, q, None, 1, 1, 1, 1, 4, 4, stream()) == BAD
    for sizes in [(0, 1, 1, 1, 4, 4), (1, 0, 1, 1, 4, 4), (1, 2, 1, 1, 4, 4), (1, 1, 1, 0, 4, 4), (1, 1, 1, 1, 0, 4), (1, 1, 1, 1, 4, -4)]:
        assert L.du_window_gather(q, q, q, p, *sizes, stream()) == BAD
    assert L.du_window_accumulate_cases(None, p, q, q, q, q, 1, 1, 1, 4, 4, stream()) == BAD
    assert L.du_window_accumulate_cases(p, None, q, q, q, q, 1, 1, 1, 4, 4, stream()) == BAD
    assert L.du_window_accumulate_cases(p, p, None, q, q, q, 1, 1, 1, 4, 4, stream()) == BAD
    assert L.du_window_accumulate_cases(p, p, q, None, q, q, 1, 1, 1, 4, 4, stream()) == BAD
    assert L.du_window_accumulate_cases(p, p, q, q, None, q, 1, 1, 1, 4, 4, stream()) == BAD
    assert L.du_window_accumulate_cases(p, p, q, q, q, None, 1, 1, 1, 4, 4, stream()) == BAD
    for sizes in [(0, 1, 1, 4, 4), (1, 0, 1, 4, 4), (1, 1, 0, 4, 4), (1, 1, 1, 0, 4), (1, 1, 1, 4, -1)]:
        assert L.du_window_accumulate_cases(p, p, q, q, q, q, *sizes, stream()) == BAD
    assert L.du_window_accumulate_cases(p, p, q, q, q, q, 1, 65, 1, 4, 4, stream()) == UNSUPPORTED
    torch.cuda.synchronize()
    assert not t.any() and not tab.any()                                           # nothing ran


# ------------------------------------------------------------------------------------------------ the loop, stand-in forwards
def ramp(ph, pw, d):
    y, x = torch.meshgrid(torch.arange(ph, device=d), torch.arange(pw, device=d), indexing="ij")
    return ((3 * y + 5 * x) % 17).float()                                          # integers 0..16, not symmetric under either flip


def integer_forward(calls=None):
    """(b, C, ph, pw) -> (b, 3, ph, pw) integer-valued logits, |v| <= 64: a pointwise function of the window plus a position term"""
    def forward(x):
        if calls is not None:
            calls.append(tuple(x.shape))
        r = ramp(x.shape[2], x.shape[3], x.device)
        q = torch.round(x * 16).clamp(-48, 48)
        return torch.stack([q[:, 0] + r, -q[:, 0] + r, q[:, -1] - r], 1).contiguous()
    return forward


def pointwise_forward(x):
    """PointwiseNet's arithmetic as a function: non-integer logits that do not depend on the batch a window sits in"""
    return torch.stack([torch.tanh(x[:, 0]) * 0.75 + x[:, 1], x[:, 0] * x[:, 1] - 1.25], 1).contiguous()


def importance_map(patch, use_gaussian):
    """the loop's weights, float32 on the host"""
    return INF.compute_gaussian(patch, sigma_scale=1.0 / 8, value_scaling_factor=10) if use_gaussian else torch.ones(patch)


def loop_accumulators(forward, d, cases, patch, step, use_gaussian, batch_size, mirror=None):
    """{case index: (pred, npred, (y slice, x slice))}: what _window_loop_cases hands to its sink"""
    got = {}
    INF._window_loop_cases(forward, d, cases, patch, step, use_gaussian, batch_size, mirror, lambda group: got.update({g[0]: g[1:] for g in group}))
    assert sorted(got) == list(range(len(cases)))
    return got


@pytest.mark.parametrize("mirror", [None, (0, 1)])
def test_old_and_new_loop_agree_where_both_are_exact(mirror):
    """The loop against the plain construction (padded copy, slices, the sequential fp32 `+=`), to the bit.  use_gaussian=False and integer
    logits: every fp32 sum is exact whatever its order; with both mirror axes the averages are multiples of 1/4 below 2^8, still exact.
    The reference being the sequential loop, the order is pinned too: the Gaussian and non-integer logits, to the bit as well."""
    d, patch = dev(), (8, 12)
    cases = [gen(2, *s, seed=20 + i).to(d) for i, s in enumerate(CASES)]
    for use_gaussian, forward in ((False, integer_forward()), (True, pointwise_forward)):
        got = loop_accumulators(forward, d, cases, patch, 0.5, use_gaussian, 5, mirror)
        gauss = importance_map(patch, use_gaussian).numpy()
        for i, c in enumerate(cases):
            pred, npred, (ys, xs) = plain_window_sums(forward, c, patch, 0.5, gauss, 5, mirror)
            assert same_bits(got[i][0], torch.from_numpy(pred)) and same_bits(got[i][1], torch.from_numpy(npred)) and got[i][2] == (ys, xs)
        if not use_gaussian:
            assert float(got[3][1].max()) >= 4.0                                   # windows do meet: the counts are the weights here


class PointwiseNet(torch.nn.Module):
    """a stand-in network: 2 heads, a pointwise function of the window, so a window's logits do not depend on its batch"""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor([0.75, -1.25]))
        self.calls = []

    def forward(self, x):
        self.calls.append(x.shape[0])
        return torch.stack([torch.tanh(x[:, 0]) * self.w[0] + x[:, 1], x[:, 0] * x[:, 1] + self.w[1]], 1)


def test_loop_with_a_stand_in_forward():
    d = dev()
    net = PointwiseNet().to(d)
    cases = [gen(2, *s, seed=40 + i).to(d) for i, s in enumerate(LIST_A)]
    kw = dict(tile_step_size=0.5, use_gaussian=True, batch_size=8)
    out = INF.predict_cases_logits(net, cases, (64, 64), **kw)
    assert net.calls == [8, 8, 3]                                                  # ceil(19 / 8) forwards, only the last one ragged
    assert [tuple(o.shape) for o in out] == [(2, *s) for s in LIST_A] and all(o.is_cuda and o.dtype == torch.float32 for o in out)
    net.calls.clear()
    mirrored = INF.predict_cases_logits(net, cases, (64, 64), mirror_axes=(0, 1), **kw)
    assert len(net.calls) == 12
    assert all(float((a - b).abs().max()) < 1e-5 * float(b.abs().max()) for a, b in zip(mirrored, out))   # a pointwise net: mirroring is a no-op
    rev = INF.predict_cases_logits(net, cases[::-1], (64, 64), **kw)[::-1]
    net.calls.clear()
    for i, c in enumerate(cases):
        one, = INF.predict_cases_logits(net, [c], (64, 64), **kw)
        assert same_bits(out[i], rev[i]) and same_bits(out[i], one)
    assert len(net.calls) == 6                                                     # what the per-case loop pays
    # ... and the values are those of the single-case function
    for i in (2, 5):
        assert same_bits(out[i], INF.predict_sliding_window_logits(net, cases[i], (64, 64), **kw))
    # a small budget: more groups, the same bits
    split = INF.predict_cases_logits(net, cases, (64, 64), max_voxels_in_flight=22000, **kw)
    assert all(same_bits(a, b) for a, b in zip(split, out))


class OverflowNet(PointwiseNet):
    def forward(self, x):
        return super().forward(x) * 1e30                                           # a marker of 1e20 in the input overflows fp32


def test_non_finite_names_the_cases():
    d = dev()
    net = OverflowNet().to(d)
    cases = [gen(2, *s, seed=50 + i).to(d) for i, s in enumerate(LIST_A[:4])]
    cases[2][1, 0, 3, 4] = 1e20
    with pytest.raises(RuntimeError, match=r"Encountered inf in predicted array \(cases \[2\]\)"):
        INF.predict_cases_logits(net, cases, (64, 64), batch_size=8)
    with pytest.raises(RuntimeError, match=r"Encountered inf in predicted array \(cases \[2\]\)"):
        INF.predict_cases_segmentation(net, cases, (64, 64), batch_size=8)
    cases[2][1, 0, 3, 4] = 0.0
    assert len(INF.predict_cases_segmentation(net, cases, (64, 64), batch_size=8)) == 4


def test_non_finite_single_case_has_no_case_list():
    d = dev()
    net = OverflowNet().to(d)
    data = gen(2, *LIST_A[2], seed=52).to(d)
    data[1, 0, 3, 4] = 1e20
    for predict in (INF.predict_sliding_window_logits, INF.predict_segmentation):
        with pytest.raises(RuntimeError, match=r"^Encountered inf in predicted array$"):
            predict(net, data, (64, 64), batch_size=8)


class RaisingNet(PointwiseNet):
    def forward(self, x):
        raise ValueError("the forward failed")


def test_training_flag_restored_when_the_forward_raises():
    d = dev()
    net = RaisingNet().to(d)
    data = gen(2, *LIST_A[0], seed=53).to(d)
    calls = [lambda: INF.predict_sliding_window_logits(net, data, (64, 64)), lambda: INF.predict_segmentation(net, data, (64, 64)),
             lambda: INF.predict_cases_logits(net, [data], (64, 64)), lambda: INF.predict_cases_segmentation(net, [data], (64, 64))]
    for training in (True, False):
        net.train(training)
        for call in calls:
            with pytest.raises(ValueError, match="the forward failed"):
                call()
            assert net.training is training


# ------------------------------------------------------------------------------------------------ chunks above the 64 slots of an accumulate launch
def normalized(pred, npred, d):
    """host sums -> logits on the device by the package's own normalisation (du_window_normalize: the accumulation is what is compared)"""
    p, n = torch.from_numpy(pred).to(d), torch.from_numpy(npred).to(d)
    assert _lib.lib().du_window_normalize(p.data_ptr(), n.data_ptr(), p.shape[0], n.numel(), stream()) == 0
    return p


def test_single_case_window_batch_above_the_launch_limit():
    """batch_size=128 on a case of 72 windows: one forward, the accumulate in launches of 64 + 8 slots"""
    d, patch = dev(), (6, 10)
    net = PointwiseNet().to(d)
    data = gen(2, *CASES[3], seed=70).to(d)
    assert [[len(c) for c in chunks] for _, chunks in INF.plan_case_batches([CASES[3]], patch, 0.3, 128)] == [[72]]
    big = INF.predict_sliding_window_logits(net, data, patch, tile_step_size=0.3, batch_size=128)
    assert net.calls == [72]
    assert same_bits(big, INF.predict_sliding_window_logits(net, data, patch, tile_step_size=0.3, batch_size=5))
    with torch.no_grad():
        pred, npred, (ys, xs) = plain_window_sums(net, data, patch, 0.3, importance_map(patch, True).numpy(), 72)
    assert same_bits(big, normalized(pred, npred, d)[:, :, ys, xs])


def test_loop_chunk_above_the_launch_limit():
    """one chunk of 95 windows of four cases: launches of 64 + 31 slots, against the host restatement applied to the same split and against
    the plain loop over all 95"""
    d, patch = dev(), (6, 10)
    cases = [gen(2, *s, seed=80 + i).to(d) for i, s in enumerate(CASES)]
    (_, (chunk,)), = INF.plan_case_batches(CASES, patch, 0.3, 100)
    assert len(chunk) == 95
    got = loop_accumulators(pointwise_forward, d, cases, patch, 0.3, True, 100)
    gauss = importance_map(patch, True).numpy()
    x = torch.stack([INF.pad_to_patch(cases[i], patch)[0][:, dd, y0:y0 + patch[0], x0:x0 + patch[1]] for i, dd, y0, x0 in chunk])
    logits = pointwise_forward(x).cpu().numpy()
    pshapes = [padded(s, patch) for s in CASES]
    split = [np.zeros((2, *s), np.float32) for s in pshapes], [np.zeros(s, np.float32) for s in pshapes]
    plain = [np.zeros((2, *s), np.float32) for s in pshapes], [np.zeros(s, np.float32) for s in pshapes]
    for s0 in range(0, len(chunk), INF.MAX_WINDOW_BATCH):
        INF._accumulate_cases_numpy(logits[s0:s0 + INF.MAX_WINDOW_BATCH], gauss, chunk[s0:s0 + INF.MAX_WINDOW_BATCH], *split)
    plain_accumulate(logits, gauss, chunk, *plain)
    for i in range(len(CASES)):
        for want_p, want_n in (split, plain):
            assert same_bits(got[i][0], torch.from_numpy(want_p[i])) and same_bits(got[i][1], torch.from_numpy(want_n[i]))


# ------------------------------------------------------------------------------------------------ end to end with the network
_E2E = {}
E2E_SHAPES = [(3, 1, 100, 128), (3, 1, 130, 150), (3, 2, 160, 200), (3, 1, 90, 70)]
E2E_KW = dict(tile_step_size=0.5, use_gaussian=True, batch_size=5)


def e2e_net():
    """the recipe of tests/test_gpu_export.py::e2e_net: dinounet_s, fp32, the oracle's seeded state dict"""
    if "net" not in _E2E:
        from oracle import weights
        from dinounet_amd.network_architecture import DinoUNet
        from dinounet_amd.plans import PLANS_2D
        net = DinoUNet.from_config(PLANS_2D, 3, 3, dinov3_pretrained_path=None, dinov3_model_name="dinounet_s", precision="fp32")
        ks = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
        net.load_state_dict(weights.make_state_dict(ks, seed=0), strict=True)
        _E2E["net"] = net.to(dev()).eval()
    return _E2E["net"]


def e2e_predictor():
    """an EnsemblePredictor of two parameter sets: the network's own and one with seeded noise on the trainable tensors"""
    if "predictor" not in _E2E:
        net = e2e_net()
        trainable = {n for n, p in net.named_parameters() if p.requires_grad}
        g = torch.Generator().manual_seed(1)
        noisy = {k: v.detach().clone() for k, v in net.state_dict().items()}
        for k in sorted(trainable):
            noisy[k] += 0.05 * float(noisy[k].abs().mean()) * torch.randn(noisy[k].shape, generator=g).to(noisy[k].device)
        for k in noisy:
            if k.startswith("decoder.encoder."):
                noisy[k] = noisy["encoder." + k[len("decoder.encoder."):]]
        _E2E["predictor"] = INF.EnsemblePredictor(net, [net.state_dict(), noisy])
    return _E2E["predictor"]


def e2e_data():
    return [gen(*s, seed=60 + i) for i, s in enumerate(E2E_SHAPES)]


def e2e_props(shape):
    D, H, W = shape[1:]
    Ho, Wo = (3 * H) // 2, (3 * W) // 2
    return {"shape_before_cropping": [D + 1, Ho + 7, Wo + 5], "bbox_used_for_cropping": [[1, D + 1], [4, Ho + 4], [5, Wo + 5]],
            "shape_after_cropping_and_before_resampling": [D, Ho, Wo]}


def in_band(z64):
    """the tie band of float64 logits (K, ...): top-two gap below 1e-5 * max|logit| (tests/test_gpu_export.py)"""
    top = z64.topk(2, dim=0).values
    return (top[0] - top[1]) < BAND_REL * float(z64.abs().max())


def assert_same_up_to_band(got, want, band):
    diff = got.cpu() != want.cpu()
    share = float(diff.float().mean())
    print(f"differing voxels {int(diff.sum())} of {diff.numel()}, in band {int(band.sum())}")
    assert got.shape == want.shape and not (diff & ~band).any() and share < 1e-4, (int(diff.sum()), int((diff & ~band).sum()), share)


def e2e_reference(who, resample):
    """per case: the single-case label map and the tie band of the single-case logits, once per (network | ensemble, properties)"""
    key = ("ref", who, resample)
    if key not in _E2E:
        single = e2e_net() if who == "net" else e2e_predictor()
        rows = []
        for data, shape in zip(e2e_data(), E2E_SHAPES):
            if who == "net":
                logits = INF.predict_sliding_window_logits(single, data, (128, 128), **E2E_KW)
                seg = lambda **k: INF.predict_segmentation(single, data, (128, 128), **E2E_KW, **k)          # noqa: E731
            else:
                logits = single.predict_logits(data, (128, 128), **E2E_KW)
                seg = lambda **k: single.predict_segmentation(data, (128, 128), **E2E_KW, **k)                # noqa: E731
            if not resample:
                rows.append((seg(), in_band(logits.double().cpu())))
            else:
                props = e2e_props(shape)
                D, Ho, Wo = props["shape_after_cropping_and_before_resampling"]
                band = torch.zeros(tuple(props["shape_before_cropping"]), dtype=torch.bool)
                band[1:, 4:Ho + 4, 5:Wo + 5] = in_band(EX.resize_inplane_float64(logits.cpu(), (Ho, Wo)))
                rows.append((seg(properties=props, transpose_backward=(0, 2, 1)), band.permute(0, 2, 1)))
        _E2E[key] = rows
    return _E2E[key]


@pytest.mark.parametrize("resample", [False, True], ids=["plain", "resample"])
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("who", ["net", "ensemble"])
def test_predict_cases_segmentation_end_to_end(who, graph, resample):
    net = e2e_net()
    run = (lambda *a, **k: INF.predict_cases_segmentation(net, *a, **k)) if who == "net" else e2e_predictor().predict_cases_segmentation
    want = e2e_reference(who, resample)
    kw = dict(properties=[e2e_props(s) for s in E2E_SHAPES], transpose_backward=(0, 2, 1)) if resample else {}
    segs = run(e2e_data(), (128, 128), graph=graph, **E2E_KW, **kw)
    assert len(segs) == len(E2E_SHAPES)
    for seg, shape, (ref, band) in zip(segs, E2E_SHAPES, want):
        assert seg.dtype == torch.uint8 and seg.is_cuda
        if not resample:
            assert tuple(seg.shape) == shape[1:]
        assert_same_up_to_band(seg, ref, band)
    assert net.training is False
    if who == "net" and not graph and not resample:                                # the training flag is restored, probabilities come along
        net.train()
        try:
            pairs = INF.predict_cases_segmentation(net, e2e_data()[:1], (128, 128), return_probabilities=True, **E2E_KW)
            assert net.training is True
        finally:
            net.eval()
        (seg, probs), = pairs
        assert tuple(probs.shape) == (3, *E2E_SHAPES[0][1:])
        assert_same_up_to_band(seg, want[0][0], want[0][1])                        # (another batch composition: the forward's own round-off)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("who", ["stand-in", "ensemble"])
def test_single_case_is_the_list_of_one(who, graph):
    """predict_sliding_window_logits / predict_segmentation (EnsemblePredictor: predict_logits / predict_segmentation) equal element 0 of the
    predict_cases_* call on [data], to the bit"""
    if who == "stand-in":
        net = PointwiseNet().to(dev())
        data, patch, kw = gen(2, *LIST_A[2], seed=90), (64, 64), dict(tile_step_size=0.5, use_gaussian=True, batch_size=4)   # 6 windows: 4 + 2
        one_logits, one_seg = partial(INF.predict_sliding_window_logits, net), partial(INF.predict_segmentation, net)
        list_logits, list_seg = partial(INF.predict_cases_logits, net), partial(INF.predict_cases_segmentation, net)
    else:
        p = e2e_predictor()
        data, patch, kw = e2e_data()[0], (128, 128), E2E_KW
        one_logits, one_seg, list_logits, list_seg = p.predict_logits, p.predict_segmentation, p.predict_cases_logits, p.predict_cases_segmentation
    logits = one_logits(data, patch, graph=graph, **kw)
    assert logits.is_cuda and logits.dtype == torch.float32 and tuple(logits.shape[1:]) == tuple(data.shape[1:])
    assert same_bits(logits, list_logits([data], patch, graph=graph, **kw)[0])
    seg = one_seg(data, patch, graph=graph, **kw)
    assert seg.dtype == torch.uint8 and torch.equal(seg, list_seg([data], patch, graph=graph, **kw)[0])


# ------------------------------------------------------------------------------------------------ raw in, labels out
def raw_image(shape, frame, seed):
    """(3, 1, H, W) float32 raw image: positive intensities inside `frame` = (y0, y1, x0, x1), zeros around (crop_to_nonzero removes them)"""
    rng = np.random.default_rng(seed)
    img = np.zeros((3, *shape), np.float32)
    y0, y1, x0, x1 = frame
    img[:, :, y0:y1, x0:x1] = rng.uniform(1.0, 200.0, (3, shape[0], y1 - y0, x1 - x0)).astype(np.float32)
    return img


def test_predict_from_list_of_npy_arrays():
    from dinounet_amd import preprocessing as P
    d, net = dev(), e2e_net()
    kw = dict(transpose_forward=(0, 2, 1), spacing=[0.9375, 0.9375], normalization_schemes=["ZScoreNormalization"] * 3,
              use_mask_for_norm=[False] * 3, foreground_intensity_properties_per_channel=None)
    pk = dict(tile_step_size=0.5, use_gaussian=True)
    raws = [raw_image((1, 76, 110), (8, 68, 10, 100), 5), raw_image((1, 90, 70), (5, 80, 3, 66), 6)]
    props = [{"spacing": (999.0, 1.0, 1.0)}, {"spacing": (999.0, 1.0, 1.0)}]
    segs = INF.predict_from_list_of_npy_arrays(net, [torch.from_numpy(r).to(d) for r in raws], props, (64, 64), batch_size=4, **kw, **pk)
    assert len(segs) == 2
    bands = []
    for raw, prop, seg in zip(raws, props, segs):
        t = torch.from_numpy(raw).to(d)
        own = {"spacing": (999.0, 1.0, 1.0)}
        want = INF.predict_from_raw(net, t, own, (64, 64), batch_size=1, **kw, **pk)
        assert own == prop                                                          # run_case filled the caller's dicts
        assert seg.dtype == torch.uint8 and tuple(seg.shape) == raw.shape[1:] and seg.is_cuda
        pre, _ = P.run_case(t, None, dict(own), **kw)
        logits = INF.predict_sliding_window_logits(net, pre, (64, 64), batch_size=1, **pk)
        Dn, Ho, Wo = own["shape_after_cropping_and_before_resampling"]
        (b0, _), (by, _), (bx, _) = own["bbox_used_for_cropping"]
        band = torch.zeros(tuple(own["shape_before_cropping"]), dtype=torch.bool)
        band[b0:b0 + Dn, by:by + Ho, bx:bx + Wo] = in_band(EX.resize_inplane_float64(logits.cpu(), (Ho, Wo)))
        bands.append(band.permute(0, 2, 1))                                         # transpose_backward = the inverse of (0, 2, 1)
        assert_same_up_to_band(seg, want, bands[-1])
    # a budget of one voxel: every case is preprocessed and predicted as a group of its own, the label maps stay
    apart = INF.predict_from_list_of_npy_arrays(net, [torch.from_numpy(r).to(d) for r in raws], [dict(own), dict(own)], (64, 64), batch_size=4,
                                                max_voxels_in_flight=1, **kw, **pk)
    for a, b, band in zip(apart, segs, bands):
        assert_same_up_to_band(a, b, band)
    # a single array with a single dict: still a list
    one = INF.predict_from_list_of_npy_arrays(net, torch.from_numpy(raws[0]).to(d), {"spacing": (999.0, 1.0, 1.0)}, (64, 64), batch_size=4, **kw, **pk)
    assert isinstance(one, list) and len(one) == 1
    assert_same_up_to_band(one[0], segs[0], bands[0])
