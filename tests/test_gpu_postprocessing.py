"""GPU tests (-m gpu) of csrc/cc.hip through dinounet_amd.postprocessing: component ids, statistics, the keep-largest map and the search,
against the scipy restatement that CPU tensors run (tests/test_cpu_postprocessing.py checks that restatement against a brute-force flood
fill).  Everything is integer: every comparison is equality.

The shapes cross the 4 x 8 x 64 tile of the kernels in every axis, hit exact multiples of it, and degenerate; (8, 256, 256) has 256 tiles,
so many workgroups merge at once.  The reference of a (pattern, shape) pair is computed once."""
import functools

import numpy as np
import pytest
import torch

from dinounet_amd import _lib
from dinounet_amd import postprocessing as PP
from test_cpu_postprocessing import PATTERNS, REMOVE, hand_case, label_map, make_mask, run_search, same_report
from test_gpu_ops import dev

pytestmark = pytest.mark.gpu

SHAPES = [(1, 70, 150), (5, 37, 131), (3, 64, 128), (17, 9, 67), (1, 1, 300), (2, 2, 2), (1, 1, 1), (8, 256, 256)]


@functools.lru_cache(maxsize=None)
def reference(pattern, shape):
    """(seg uint8 CPU, ids, stats, kept map) from the restatement"""
    seg = torch.from_numpy(make_mask(pattern, shape).astype(np.uint8))
    ids, stats = PP.component_ids(seg, 1)
    return seg, ids, stats, REMOVE(seg, 1)


def check(seg, want_ids, want_stats, want_out, lor=1, **kw):
    d = seg.to(dev())
    ids, stats = PP.component_ids(d, lor)
    out = REMOVE(d, lor, **kw)
    print(f"{tuple(seg.shape)}: stats {stats} (restatement {want_stats}); ids differ at {int((ids.cpu() != want_ids).sum())} voxels, "
          f"maps at {int((out.cpu() != want_out).sum())}")
    assert ids.dtype == torch.int32 and ids.device == d.device and out.dtype == torch.uint8 and out.device == d.device
    assert stats == want_stats
    assert torch.equal(ids.cpu(), want_ids)
    assert torch.equal(out.cpu(), want_out)
    assert torch.equal(d.cpu(), seg), "the input was modified"
    assert out.data_ptr() != d.data_ptr()


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_patterns(pattern, shape):
    check(*reference(pattern, shape))


def test_two_serpentines_of_equal_size_keep_the_first():
    seg, ids, stats, out = reference("two_serpentines", (3, 40, 130))
    assert stats == {"n_components": 2, "largest_size": 2620, "largest_id": 0}
    check(seg, ids, stats, out)
    assert torch.equal(out[0], seg[0]) and int(out[1:].sum()) == 0


def test_serpentine_is_one_component():
    for shape in [(5, 37, 131), (8, 256, 256)]:
        assert reference("serpentine", shape)[2]["n_components"] == 1


@pytest.mark.parametrize("shape", [(5, 37, 131), (1, 70, 150), (8, 256, 256)], ids=str)
@pytest.mark.parametrize("lor,bg", [([1, (2, 3)], 0), ([1, (2, 3)], 7), (5, 7), ((2, 3), 255), (200, 7), ([1, 200], 3), ([(5, 200), 2], 0)])
def test_labels_and_regions(lor, bg, shape):
    seg = label_map(shape, seed=11)
    assert (seg == 200).any()
    ids, stats = PP.component_ids(seg, lor)
    check(seg, ids, stats, REMOVE(seg, lor, background_label=bg), lor=lor, background_label=bg)
    if lor == 200:
        assert stats["n_components"] == 0 and stats["largest_id"] == -1


def test_unaligned_views_and_non_contiguous_input():
    base = label_map((6, 40, 139), seed=12)
    d = base.to(dev())
    for cut in (lambda t: t[1:], lambda t: t[:, 3:, :], lambda t: t[:, :, 1:], lambda t: t.permute(0, 2, 1), lambda t: t.reshape(-1)[7:7 + 5 * 40 * 139].view(5, 40, 139)):
        view = cut(base)
        ids, stats = PP.component_ids(view, [1, 2])
        want = REMOVE(view, [1, 2])
        check(view.contiguous(), ids, stats, want, lor=[1, 2])
        assert torch.equal(REMOVE(cut(d), [1, 2]).cpu(), want)                         # the last view starts 7 bytes into the allocation
        assert torch.equal(PP.component_ids(cut(d), [1, 2])[0].cpu(), ids)


def test_two_runs_give_the_same_bytes():
    for pattern in ("random0.25", "random0.6", "serpentine"):
        d = reference(pattern, (8, 256, 256))[0].to(dev())
        ids_a, stats_a = PP.component_ids(d, 1)
        ids_b, stats_b = PP.component_ids(d, 1)
        out_a, out_b = REMOVE(d, 1), REMOVE(d, 1)
        assert stats_a == stats_b and torch.equal(ids_a, ids_b) and torch.equal(out_a, out_b)


@pytest.mark.parametrize("name", ["i", "ii", "iii"])
def test_determine_postprocessing_on_the_device(name):
    case = hand_case(name)
    fns_c, kwargs_c, report_c, final_c = run_search(case)
    fns_d, kwargs_d, report_d, final_d = run_search(case, dev())
    assert kwargs_d == kwargs_c == case["kwargs"] and fns_d == fns_c
    assert same_report(report_d, report_c), (report_d, report_c)
    assert all(f.device.type == "cuda" and torch.equal(f.cpu(), w) for f, w in zip(final_d, final_c))
    assert all(torch.equal(f, w) for f, w in zip(final_c, case["final"]))


def test_too_many_voxels_is_a_value_error_without_a_launch():
    big = torch.zeros(1, dtype=torch.uint8, device=dev()).expand(2048, 1024, 1024)      # 2^31 voxels, one byte of memory
    with pytest.raises(ValueError):
        REMOVE(big, 1)
    with pytest.raises(ValueError):
        PP.component_ids(big, 1)


def test_c_abi_argument_checks():
    L = _lib.lib()
    BAD_ARG, UNSUPPORTED = -1, -2
    D, H, W = 3, 9, 70
    n = D * H * W
    assert L.du_cc_ws_elems(D, H, W, 0) == 4 + 2 * ((n + 3) // 4 * 4) and L.du_cc_ws_elems(D, H, W, 1) == 4 + 3 * ((n + 3) // 4 * 4)
    assert L.du_cc_ws_elems(0, H, W, 0) == 0 and L.du_cc_ws_elems(2048, 1024, 1024, 1) == 0
    seg = torch.zeros((D, H, W), dtype=torch.uint8, device=dev())
    out = torch.full((D, H, W), 9, dtype=torch.uint8, device=dev())
    ids = torch.full((D, H, W), 9, dtype=torch.int32, device=dev())
    stats = torch.full((3,), 9, dtype=torch.int64, device=dev())
    st = torch.cuda.current_stream().cuda_stream
    for keep in (0, 1):
        we = int(L.du_cc_ws_elems(D, H, W, keep))
        ws = torch.zeros(we, dtype=torch.int32, device=dev())

        def call(seg_p=seg.data_ptr(), dst_p=None, stats_p=stats.data_ptr(), shape=(D, H, W), ws_p=ws.data_ptr(), ws_elems=we, bg=0):
            if keep:
                return L.du_cc_keep_largest(seg_p, 2, bg, out.data_ptr() if dst_p is None else dst_p, stats_p, *shape, ws_p, ws_elems, st)
            return L.du_cc_label(seg_p, 2, ids.data_ptr() if dst_p is None else dst_p, stats_p, *shape, ws_p, ws_elems, st)

        assert call(ws_elems=we - 1) == BAD_ARG                                        # a short workspace
        with pytest.raises(RuntimeError, match="DU_ERR_BAD_ARG"):
            _lib.check(call(ws_elems=we - 1), "du_cc")
        assert call(seg_p=None) == BAD_ARG and call(dst_p=0) == BAD_ARG and call(stats_p=None) == BAD_ARG and call(ws_p=None) == BAD_ARG
        assert call(shape=(0, H, W)) == BAD_ARG and call(shape=(D, -1, W)) == BAD_ARG and call(shape=(D, H, 0)) == BAD_ARG
        assert call(shape=(2048, 1024, 1024)) == UNSUPPORTED and call(shape=(65536, 65536, 65536)) == UNSUPPORTED
        assert call(ws_p=ws.data_ptr() + 4) == BAD_ARG                                 # workspace not 16-byte aligned
        if keep:
            assert call(dst_p=seg.data_ptr()) == BAD_ARG and call(dst_p=seg.data_ptr() + 16) == BAD_ARG     # out overlaps seg
            assert call(bg=256) == BAD_ARG and call(bg=-1) == BAD_ARG
    torch.cuda.synchronize()
    assert int((out != 9).sum()) == 0 and int((ids != 9).sum()) == 0 and int((stats != 9).sum()) == 0, "a refused call wrote"
