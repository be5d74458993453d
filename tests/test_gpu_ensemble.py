"""GPU tests (-m gpu) of ensembling: du_ensemble_merge (csrc/ensemble.hip) through dinounet_amd.ensemble against numpy's own
`avg += p; avg /= M` -- bit for bit, for grid inputs and for softmax / sigmoid of random logits alike: the kernel adds the members in their
order and divides once, correctly rounded, so there is no tolerance -- and inference.EnsemblePredictor (folds that share one backbone pass)
against the mean of per-fold sliding-window predictions.

Bounds of the fold tests.  Both sides run the same kernels per fold and differ only in the order of fp32 additions (sum over folds before
or after the weighted accumulation and the division), the situation of test_gpu_export's end-to-end tests, whose bounds are applied as
they stand: logits rel < 2e-5 (test_gpu_ops.rel), labels equal outside the tie band 1e-5 * max|logit| of the float64 logits, and the share
of differing voxels below 1e-4.  Measured (printed by the tests): logits rel 3.1e-07 for three folds, eager and captured, with net in eval
or in train mode; 1.4e-07 .. 1.9e-07 for one fold; captured against eager 2.0e-07; no differing voxel of 64 000; [A, B] against [A, A]
moves the logits by 0.20 of their maximum."""
import copy

import numpy as np
import pytest
import torch

from dinounet_amd import ensemble as ENS
from test_cpu_ensemble import (ORDERS, SHAPES, as_np, check_find_best, grid_members, np_argmax, np_average, np_regions, random_members,
                               same_bits)
from test_gpu_export import assert_same_up_to_band, e2e_net, in_band
from test_gpu_ops import dev, gen, rel

pytestmark = pytest.mark.gpu


def on(members, d):
    return [m.to(d) for m in members]


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("M", [1, 2, 3, 5, 16])
def test_merge_matches_numpy_bit_for_bit(M, dtype):
    d = dev()
    for shape in SHAPES:                                 # n = 70 (tail, no multiple of 4) | 1024 (aligned) | 25929 (several workgroups + tail)
        for K in (2, 3, 8):
            for kind, members in (("grid", grid_members(M, K, shape, 7 * M + K, dtype)), ("random", random_members(M, K, shape, 9 * M + K, dtype))):
                want = np_average(as_np(members))
                seg, mean = ENS.merge_probabilities(on(members, d), return_probabilities=True)
                assert seg.is_cuda and seg.dtype == torch.uint8 and tuple(seg.shape) == shape and mean.dtype == torch.float32
                assert same_bits(mean.cpu().numpy(), want), (kind, K, shape)
                assert np.array_equal(seg.cpu().numpy(), np_argmax(want)), (kind, K, shape)
                assert torch.equal(ENS.merge_probabilities(on(members, d)), seg)                  # the mean not written: same labels
                assert same_bits(ENS.average_probabilities(on(members, d)).cpu().numpy(), want)
        for R in (1, 3):
            for kind, members in (("grid", grid_members(M, R, shape, 11 * M + R, dtype)),
                                  ("random", random_members(M, R, shape, 13 * M + R, dtype, regions=True))):
                want = np_average(as_np(members))
                seg, mean = ENS.merge_probabilities(on(members, d), regions_class_order=ORDERS[R], return_probabilities=True)
                assert same_bits(mean.cpu().numpy(), want), (kind, R, shape)
                assert np.array_equal(seg.cpu().numpy(), np_regions(want, ORDERS[R])), (kind, R, shape)
                assert torch.equal(ENS.merge_probabilities(on(members, d), regions_class_order=ORDERS[R]), seg)


def test_grid_ties_are_present_and_resolved_to_the_lowest_index():
    d = dev()
    members = grid_members(3, 8, (3, 67, 129), 5)
    mean = np_average(as_np(members))
    top = np.sort(mean, axis=0)
    assert int((top[-1] == top[-2]).sum()) > 100
    assert np.array_equal(ENS.merge_probabilities(on(members, d)).cpu().numpy(), np_argmax(mean))
    p = torch.tensor([0.25, 0.5, 0.5, 0.125]).view(4, 1, 1, 1).expand(4, 2, 5, 7).contiguous()
    q = torch.tensor([0.5, 0.25, 0.25, 0.5]).view(4, 1, 1, 1).expand(4, 2, 5, 7).contiguous()
    assert bool((ENS.merge_probabilities([p.to(d), q.to(d)]) == 0).all())            # means 0.375 0.375 0.375 0.3125
    assert bool((ENS.merge_probabilities([p.to(d)]) == 1).all())
    assert bool((ENS.merge_probabilities([p.half().to(d), q.half().to(d)]) == 0).all())


def test_region_threshold_and_paint_order():
    d = dev()
    # two regions, four kinds of voxel: means (0.5, 0.5) | (0.625, 0.5) | (0.625, 0.625) | (0.375, 0.75); 1024 voxels and 70 voxels
    for shape in ((1, 16, 64), (2, 5, 7)):
        a = torch.tensor([[0.25, 0.5, 0.5, 0.25], [0.25, 0.25, 0.5, 0.75]])
        b = torch.tensor([[0.75, 0.75, 0.75, 0.5], [0.75, 0.75, 0.75, 0.75]])
        n = shape[0] * shape[1] * shape[2]
        a, b = (t.repeat(1, n // 4 + 1)[:, :n].reshape(2, *shape).contiguous() for t in (a, b))
        want = torch.tensor([0, 3, 1, 1], dtype=torch.uint8).repeat(n // 4 + 1)[:n].reshape(shape)
        for dt in (torch.float32, torch.float16):
            seg = ENS.merge_probabilities([a.to(dt).to(d), b.to(dt).to(d)], regions_class_order=[3, 1])
            assert torch.equal(seg.cpu(), want), (shape, dt)      # 0.5 is not painted; the later region overwrites the earlier one


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_views_one_element_into_their_storage_take_the_scalar_path(dtype):
    d = dev()
    for shape in SHAPES[1:]:
        K, n = 3, shape[0] * shape[1] * shape[2]
        members = random_members(3, K, shape, 17, dtype)
        want_seg, want_mean = ENS.merge_probabilities(on(members, d), return_probabilities=True)
        for which in ((0, 1, 2), (1,)):                  # every member shifted / one of them only
            shifted = []
            for i, m in enumerate(members):
                if i in which:
                    store = torch.zeros(K * n + 1, dtype=dtype, device=d)
                    view = store[1:].view(K, *shape)
                    view.copy_(m)
                    assert view.is_contiguous() and view.data_ptr() % 16 == store.element_size()
                    shifted.append(view)
                else:
                    shifted.append(m.to(d))
            seg, mean = ENS.merge_probabilities(shifted, return_probabilities=True)
            assert torch.equal(seg, want_seg) and torch.equal(mean, want_mean), (shape, which)


def raw_merge(table, M, es, K, n, seg_ptr, mean_ptr, mode=0, order=0):
    from dinounet_amd import _lib
    flag = torch.zeros(1, dtype=torch.int32, device=table.device)
    rc = _lib.lib().du_ensemble_merge(table.data_ptr(), M, es, K, n, mode, order, seg_ptr, mean_ptr, flag.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, int(flag.item())


def test_writes_stay_inside_the_outputs():
    """seg and mean pre-filled with guards around them, at aligned and unaligned addresses (word and byte stores)"""
    d = dev()
    K = 3
    for shape in SHAPES[:2]:
        n = shape[0] * shape[1] * shape[2]
        for dtype in (torch.float32, torch.float16):
            members = on(random_members(2, K, shape, 23, dtype), d)
            table = torch.tensor([m.data_ptr() for m in members], dtype=torch.int64).to(d)
            want_seg, want_mean = ENS.merge_probabilities(members, return_probabilities=True)
            for guard in (64, 67):
                seg_buf = torch.full((n + 2 * guard,), 255, dtype=torch.uint8, device=d)
                mean_buf = torch.full((K * n + 2 * guard,), -7.0, dtype=torch.float32, device=d)
                rc, flag = raw_merge(table, 2, members[0].element_size(), K, n, seg_buf.data_ptr() + guard, mean_buf.data_ptr() + 4 * guard)
                assert rc == 0 and flag == 0
                assert bool((seg_buf[:guard] == 255).all()) and bool((seg_buf[guard + n:] == 255).all()), (shape, dtype, guard)
                assert bool((mean_buf[:guard] == -7.0).all()) and bool((mean_buf[guard + K * n:] == -7.0).all()), (shape, dtype, guard)
                assert torch.equal(seg_buf[guard:guard + n].view(shape), want_seg)
                assert torch.equal(mean_buf[guard:guard + K * n].view(K, *shape), want_mean)


def test_non_finite_raises():
    d = dev()
    for dtype in (torch.float32, torch.float16):
        for bad in (float("nan"), float("inf")):
            for shape, at in ((SHAPES[0], (1, 1, 4, 6)), (SHAPES[1], (2, 0, 9, 33))):       # scalar path (the last voxel) and vector path
                members = grid_members(3, 3, shape, 3, dtype)
                members[1][at] = bad
                with pytest.raises(RuntimeError, match="Encountered inf in predicted array"):
                    ENS.merge_probabilities(on(members, d))
                with pytest.raises(RuntimeError, match="Encountered inf in predicted array"):
                    ENS.merge_probabilities(on(members, d), regions_class_order=[1, 2, 3])


def test_error_codes_and_value_errors():
    d = dev()
    members = on(grid_members(2, 3, (1, 4, 4), 0), d)
    table = torch.tensor([m.data_ptr() for m in members] + [members[0].data_ptr()] * 15, dtype=torch.int64).to(d)
    seg = torch.zeros(16, dtype=torch.uint8, device=d)
    assert raw_merge(table, 2, 4, 3, 16, seg.data_ptr(), None)[0] == 0
    assert raw_merge(table, 0, 4, 3, 16, seg.data_ptr(), None)[0] == -2                  # M = 0
    assert raw_merge(table, 17, 4, 3, 16, seg.data_ptr(), None)[0] == -2                 # M = 17
    big = torch.zeros((9, 1, 4, 4), device=d)
    assert raw_merge(torch.tensor([big.data_ptr()], dtype=torch.int64).to(d), 1, 4, 9, 16, seg.data_ptr(), None)[0] == -2      # K = 9
    assert raw_merge(table, 2, 4, 3, -1, seg.data_ptr(), None)[0] == -2                  # n < 0
    assert raw_merge(table, 2, 8, 3, 16, seg.data_ptr(), None)[0] == -2                  # neither fp32 nor fp16
    assert raw_merge(table, 2, 4, 1, 16, seg.data_ptr(), None)[0] == -2                  # one class has no argmax
    assert raw_merge(table, 2, 4, 1, 16, seg.data_ptr(), None, mode=1, order=3)[0] == 0
    assert raw_merge(table, 2, 4, 3, 16, None, None)[0] == -1                            # nothing to write
    with pytest.raises(ValueError, match="one shape, dtype and device"):
        ENS.merge_probabilities([members[0], members[1].cpu()])
    with pytest.raises(ValueError, match="at most 16"):
        ENS.merge_probabilities(on(grid_members(17, 2, (1, 2, 2), 0), d))
    with pytest.raises(ValueError, match="2..8 classes"):
        ENS.merge_probabilities([big])


def test_gpu_and_cpu_paths_agree():
    d = dev()
    for dtype in (torch.float32, torch.float16):
        members = random_members(5, 4, (3, 67, 129), 41, dtype)
        seg_c, mean_c = ENS.merge_probabilities(members, return_probabilities=True)
        seg_g, mean_g = ENS.merge_probabilities(on(members, d), return_probabilities=True)
        assert torch.equal(seg_g.cpu(), seg_c) and torch.equal(mean_g.cpu(), mean_c)
        regions = random_members(5, 4, (3, 67, 129), 43, dtype, regions=True)
        seg_c, mean_c = ENS.merge_probabilities(regions, regions_class_order=[4, 1, 3, 2], return_probabilities=True)
        seg_g, mean_g = ENS.merge_probabilities(on(regions, d), regions_class_order=[4, 1, 3, 2], return_probabilities=True)
        assert torch.equal(seg_g.cpu(), seg_c) and torch.equal(mean_g.cpu(), mean_c)
    many = random_members(3, 11, (2, 5, 7), 47)                                          # the mean alone: planes in chunks of 8
    assert same_bits(ENS.average_probabilities(on(many, d)).cpu().numpy(), np_average(as_np(many)))
    sliced = [m[:, :, ::2] for m in on(members, d)]                                      # non-contiguous members are copied first
    assert torch.equal(ENS.merge_probabilities(sliced).cpu(), ENS.merge_probabilities([m[:, :, ::2] for m in members]))


def test_find_best_configuration_on_the_device():
    check_find_best(dev())


# ------------------------------------------------------------------------------------------------ folds
SHAPE, BS, PATCH = (3, 2, 160, 200), 5, (128, 128)
KW = dict(tile_step_size=0.5, use_gaussian=True, batch_size=BS)
_FOLDS = {}


def fold_sets():
    """three full state dicts of e2e_net() whose trainable tensors carry seeded noise (the frozen backbone untouched)"""
    if "sets" not in _FOLDS:
        net = e2e_net()
        trainable = {n for n, p in net.named_parameters() if p.requires_grad}
        sets = []
        for seed in (1, 2, 3):
            g = torch.Generator().manual_seed(seed)
            sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
            for k in sorted(trainable):
                noise = torch.randn(sd[k].shape, generator=g).to(sd[k].device)
                sd[k] += 0.05 * float(sd[k].abs().mean()) * noise
            for k in sd:
                if k.startswith("decoder.encoder."):
                    sd[k] = sd["encoder." + k[len("decoder.encoder."):]]
            sets.append(sd)
        _FOLDS["sets"] = sets
    return _FOLDS["sets"]


def loaded_copy(i):
    """a copy of the network (its own backbone included) loaded with set i"""
    if "copy" not in _FOLDS:
        net = e2e_net()
        cache = net.__dict__.get("_sw_forward_cache")                 # captured forwards of other tests stay with their network
        _FOLDS["copy"] = copy.deepcopy(net, {} if cache is None else {id(cache): {}})
    _FOLDS["copy"].load_state_dict(fold_sets()[i], strict=True)
    return _FOLDS["copy"].eval()


def fold_logits(i):
    """predict_sliding_window_logits of that copy, once per set"""
    if ("logits", i) not in _FOLDS:
        from dinounet_amd import inference as INF
        _FOLDS[("logits", i)] = INF.predict_sliding_window_logits(loaded_copy(i), gen(*SHAPE, seed=7), PATCH, **KW)
    return _FOLDS[("logits", i)]


def predictor(which=(0, 1, 2)):
    if ("pred", which) not in _FOLDS:
        from dinounet_amd import inference as INF
        _FOLDS[("pred", which)] = INF.EnsemblePredictor(e2e_net(), [fold_sets()[i] for i in which])
    return _FOLDS[("pred", which)]


def check_against(pred, want, **kw):
    data = gen(*SHAPE, seed=7)
    got = pred.predict_logits(data, PATCH, **KW, **kw)
    fig = rel(got, want)
    print(f"logits rel {fig:.3e}")
    assert got.shape == want.shape and fig < 2e-5
    seg = pred.predict_segmentation(data, PATCH, **KW, **kw)
    assert seg.dtype == torch.uint8 and tuple(seg.shape) == SHAPE[1:] and seg.is_cuda
    assert_same_up_to_band(seg, want.argmax(0).to(torch.uint8), in_band(want.double().cpu()))
    return got


def test_fold_ensemble_matches_the_mean_of_the_folds():
    net = e2e_net()
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    net.train()
    try:
        pred = predictor()
        want = (fold_logits(0) + fold_logits(1) + fold_logits(2)) / 3.0
        check_against(pred, want)
        assert net.training is True                                    # the mode of net is left as it was,
        assert all(m.training for m in net.modules())                  # the shared backbone's flags included
    finally:
        net.eval()
    after = net.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    # the backbone is shared by identity, everything else is per fold
    bb = net.encoder.dinov3_adapter.backbone
    assert all(r.encoder.dinov3_adapter.backbone is bb and r.decoder.encoder is r.encoder and r.training is False for r in pred.nets)
    w = [r.decoder.seg_layers[-1].weight for r in pred.nets]
    assert w[0].data_ptr() != w[1].data_ptr() and not torch.equal(w[0], w[1]) and torch.equal(w[2], fold_sets()[2]["decoder.seg_layers.2.weight"])
    assert "_sw_forward_cache" not in pred.nets[0].__dict__ or pred.nets[0].__dict__["_sw_forward_cache"] == {}


def test_one_fold_equals_predict_segmentation():
    from dinounet_amd import inference as INF
    want = fold_logits(0)
    check_against(predictor((0,)), want)
    data = gen(*SHAPE, seed=7)
    seg = predictor((0,)).predict_segmentation(data, PATCH, **KW)
    assert_same_up_to_band(seg, INF.predict_segmentation(loaded_copy(0), data, PATCH, **KW), in_band(want.double().cpu()))


def test_the_sets_are_used_and_compact_dicts_load():
    from dinounet_amd import checkpoint as CK
    from dinounet_amd import inference as INF
    net = e2e_net()
    data = gen(*SHAPE, seed=7)
    ab = predictor((0, 1)).predict_logits(data, PATCH, **KW)
    aa = predictor((0, 0)).predict_logits(data, PATCH, **KW)
    assert rel(aa, fold_logits(0)) < 2e-5
    moved = float((ab - aa).abs().max() / aa.abs().max())
    print(f"[A, B] against [A, A]: {moved:.3e}")
    assert moved > 1e-3
    # the compact form of checkpoint.py: no frozen backbone entries, no decoder.encoder.* aliases
    frozen = set(CK._frozen_keys(net))
    compact = [{k: v for k, v in fold_sets()[i].items() if k not in frozen and not k.startswith(CK.ALIAS_PREFIX)} for i in (0, 1)]
    assert 0 < len(compact[0]) < len(fold_sets()[0]) - len(frozen)
    assert rel(INF.EnsemblePredictor(net, compact).predict_logits(data, PATCH, **KW), ab) < 2e-5
    with pytest.raises(RuntimeError, match="strict"):
        INF.EnsemblePredictor(net, [{k: v for k, v in compact[0].items() if k != "decoder.seg_layers.2.bias"}])
    with pytest.raises(RuntimeError, match="strict"):
        INF.EnsemblePredictor(net, [dict(compact[0], stray=torch.zeros(1))])
    with pytest.raises(ValueError, match="empty"):
        INF.EnsemblePredictor(net, [])


def test_backbone_runs_once_per_window_batch_and_mirror_combination(monkeypatch):
    net = e2e_net()
    bb = net.encoder.dinov3_adapter.backbone
    calls = []
    inner = bb.begin_intermediate_layers

    def counted(x, **kw):
        calls.append(int(x.shape[0]))
        return inner(x, **kw)
    monkeypatch.setattr(bb, "begin_intermediate_layers", counted)
    data = gen(3, 1, 160, 200, seed=9)                   # 6 windows in batches of 4: 2 window batches
    counts = {}
    for which in ((0,), (0, 1, 2)):
        del calls[:]
        predictor(which).predict_logits(data, PATCH, tile_step_size=0.5, use_gaussian=True, batch_size=4, mirror_axes=(0, 1))
        counts[which] = len(calls)
    assert counts[(0,)] == counts[(0, 1, 2)] == 2 * (1 + 3)
    del calls[:]
    predictor().predict_segmentation(data, PATCH, tile_step_size=0.5, use_gaussian=True, batch_size=4)
    assert len(calls) == 2


def test_construction_and_prediction_leave_the_backbone_mode_alone():
    """The backbone is shared with net, its training flags too, and in train mode it draws RoPE rescale factors and drops paths: a
    predictor must neither change the flags nor predict with them set, whatever net.train() / net.eval() did since it was built."""
    from dinounet_amd import inference as INF
    net = e2e_net()
    bb = net.encoder.dinov3_adapter.backbone
    data = gen(*SHAPE, seed=7)
    want = (fold_logits(0) + fold_logits(1) + fold_logits(2)) / 3.0
    built_in_eval = INF.EnsemblePredictor(net, fold_sets())
    assert not any(m.training for m in net.modules())
    net.train()
    try:
        # the train-mode backbone really is another function: the precondition of this test
        x = gen(2, 3, 128, 128, seed=3).to(dev())
        with torch.no_grad():
            a = net.backbone_layers(x)[-1][0].float()
            bb.eval()
            b = net.backbone_layers(x)[-1][0].float()
            bb.train()
        assert float((a - b).abs().max() / b.abs().max()) > 1e-3
        built_in_train = INF.EnsemblePredictor(net, fold_sets())
        assert all(m.training for m in net.modules())
        for pred in (built_in_eval, built_in_train):
            for graph in (False, True):                   # graph=True: warm-up and capture happen here, under net.train()
                got = pred.predict_logits(data, PATCH, **KW, graph=graph)
                fig = rel(got, want)
                print(f"net in train mode, graph={graph}: logits rel {fig:.3e}")
                assert fig < 2e-5
                assert all(m.training for m in net.modules())
        seg = built_in_eval.predict_segmentation(data, PATCH, **KW)
        assert_same_up_to_band(seg, want.argmax(0).to(torch.uint8), in_band(want.double().cpu()))
        assert all(m.training for m in net.modules())
    finally:
        net.eval()
    assert all(r.training is False and not any(m.training for m in r.decoder.modules()) for r in built_in_train.nets)


def test_a_trainable_backbone_is_refused():
    from dinounet_amd import inference as INF
    net = e2e_net()
    p = net.encoder.dinov3_adapter.backbone.cls_token
    p.requires_grad_(True)
    try:
        with pytest.raises(ValueError, match="trainable"):
            INF.EnsemblePredictor(net, [fold_sets()[0]])
    finally:
        p.requires_grad_(False)


def test_forward_takes_the_backbone_layers():
    """DinoUNet.forward(x, vit_layers=backbone_layers(x)): the same kernels on the same inputs as forward(x); without the argument nothing
    changed (every other test of the suite).  1- and 2-channel inputs go through the encoder's channel handling on both sides."""
    net = e2e_net()
    for C in (3, 1, 2):
        x = gen(2, C, 128, 128, seed=20 + C).to(dev())
        with torch.no_grad():
            want = net(x)
            layers = net.backbone_layers(x)
            got = net(x, vit_layers=layers)
            other = predictor().nets[1](x, vit_layers=layers)          # another fold's head on the same layers
        assert rel(got, want) < 2e-5, C
        assert rel(other, want) > 1e-3, C


def test_captured_fold_forward_matches_eager():
    pred = predictor()
    want = (fold_logits(0) + fold_logits(1) + fold_logits(2)) / 3.0
    captured = check_against(pred, want, graph=True)
    # ... and against the eager run itself, under the same bounds
    data = gen(*SHAPE, seed=7)
    eager = pred.predict_logits(data, PATCH, **KW, graph=False)
    fig = rel(captured, eager)
    print(f"captured against eager: logits rel {fig:.3e}")
    assert fig < 2e-5
    assert_same_up_to_band(pred.predict_segmentation(data, PATCH, **KW, graph=True), pred.predict_segmentation(data, PATCH, **KW, graph=False),
                           in_band(eager.double().cpu()))
    assert list(pred._forward_cache) == [(BS, 3, 128, 128)]                                  # the cache is the predictor's
    assert all("_sw_forward_cache" not in r.__dict__ or not r.__dict__["_sw_forward_cache"] for r in pred.nets)


def test_a_different_backbone_is_refused():
    from dinounet_amd import inference as INF
    net = e2e_net()
    bad = dict(fold_sets()[1])
    key = "encoder.dinov3_adapter.backbone.cls_token"
    bad[key] = bad[key] + 1
    with pytest.raises(ValueError, match="frozen backbone tensor"):
        INF.EnsemblePredictor(net, [fold_sets()[0], bad])


def test_predict_from_raw_with_folds():
    """raw array in, ensemble label map out (one window per launch: launches are ordered, so two runs agree to the bit)"""
    from dinounet_amd import inference as INF
    from dinounet_amd import preprocessing as P
    from test_gpu_preprocessing import raw_case
    net = e2e_net()
    img, _ = raw_case((1, 76, 110), (0, 8, 10), channels=3, seed=5)
    kw = dict(transpose_forward=(0, 1, 2), spacing=[0.9375, 0.9375], normalization_schemes=["ZScoreNormalization"] * 3,
              use_mask_for_norm=[False] * 3, foreground_intensity_properties_per_channel=None)
    pk = dict(tile_step_size=0.5, use_gaussian=True, batch_size=1)
    raw = torch.from_numpy(img).to(dev())
    props = {"spacing": (999.0, 1.0, 1.0)}
    seg = INF.predict_from_raw(net, raw, props, (64, 64), list_of_parameters=[fold_sets()[0], fold_sets()[1]], **kw, **pk)
    assert seg.dtype == torch.uint8 and tuple(seg.shape) == (1, 76, 110) and seg.is_cuda
    props2 = {"spacing": (999.0, 1.0, 1.0)}
    pre, _ = P.run_case(raw, None, props2, **kw)
    want = predictor((0, 1)).predict_segmentation(pre, (64, 64), properties=props2, transpose_backward=[0, 1, 2], **pk)
    assert torch.equal(seg, want)
    assert torch.equal(predictor((0, 1)).predict_from_raw(raw, {"spacing": (999.0, 1.0, 1.0)}, (64, 64), **kw, **pk), want)
    single = INF.predict_from_raw(net, raw, {"spacing": (999.0, 1.0, 1.0)}, (64, 64), **kw, **pk)
    assert not torch.equal(seg, single)
