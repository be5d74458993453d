"""CPU tests of dinounet_amd.ensemble: the torch restatement of average_probabilities / merge_files against numpy's own two lines
(`avg += p; avg /= M`), bit for bit; the label rules; every ValueError; the case and fold bookkeeping; find_best_configuration on hand-made
cases.  The numpy restatement of the reference and the input generators live here and are shared with tests/test_gpu_ensemble.py.

Inputs "on the grid" are multiples of 1/256 in [0, 1]: exact in fp16 and fp32, their sums over up to 16 members are exact in fp32, and two
distinct means differ by at least 1 / (256 M) -- far above the ~6e-8 resolution of an fp32 softmax of values in [0, 1], so
argmax(softmax(mean)) (what the reference computes, the nonlinearity applied a second time) and argmax(mean) (what we compute) must agree
everywhere, exact ties included."""
import numpy as np
import pytest
import torch

from dinounet_amd import ensemble as ENS
from dinounet_amd import export as EX
from dinounet_amd import postprocessing as PP


# ------------------------------------------------------------------------------------------------ the reference, in numpy
def np_average(members):
    """average_probabilities (ensembling/ensemble.py:17-29) over arrays instead of files"""
    avg = None
    for p in members:
        if avg is None:
            avg = np.array(p, copy=True)
            if avg.dtype != np.float32:
                avg = avg.astype(np.float32)
        else:
            avg += p
    avg /= len(members)
    return avg


def np_argmax(mean):
    return mean.argmax(0).astype(np.uint8)


def np_softmax_argmax(mean):
    """what merge_files does with the mean: convert_logits_to_segmentation = torch.softmax, then argmax (label_handling.py:128-163)"""
    return torch.softmax(torch.from_numpy(mean).float(), 0).argmax(0).numpy().astype(np.uint8)


def np_regions(mean, order):
    lab = np.zeros(mean.shape[1:], dtype=np.uint8)
    for i, c in enumerate(order):
        lab[mean[i] > 0.5] = c
    return lab


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == np.float32 and b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------------------ inputs
def grid_members(M, K, shape, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randint(0, 257, (K, *shape), generator=g).float() / 256.0).to(dtype) for _ in range(M)]


def random_members(M, K, shape, seed, dtype=torch.float32, regions=False):
    """softmax / sigmoid of seeded random logits: what export hands to an ensemble"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(M):
        z = torch.randn((K, *shape), generator=g) * 3.0
        out.append((torch.sigmoid(z) if regions else torch.softmax(z, 0)).to(dtype))
    return out


def as_np(members):
    return [m.numpy() for m in members]


ORDERS = {1: [5], 3: [2, 7, 1], 8: [3, 7, 1, 8, 2, 6, 4, 5]}
SHAPES = [(2, 5, 7), (1, 16, 64), (3, 67, 129)]


# ------------------------------------------------------------------------------------------------ the mean and the labels
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("M", [1, 2, 3, 5, 16])
def test_restatement_matches_numpy_bit_for_bit(M, dtype):
    for K, shape in [(2, SHAPES[0]), (3, SHAPES[1]), (8, SHAPES[0])]:
        for members in (grid_members(M, K, shape, 10 * M + K, dtype), random_members(M, K, shape, 20 * M + K, dtype)):
            want = np_average(as_np(members))
            got = ENS.average_probabilities(members)
            assert got.dtype == torch.float32 and same_bits(got.numpy(), want), (M, K, shape)
            seg, mean = ENS.merge_probabilities(members, return_probabilities=True)
            assert seg.dtype == torch.uint8 and tuple(seg.shape) == shape
            assert same_bits(mean.numpy(), want)
            assert np.array_equal(seg.numpy(), np_argmax(want))
            assert torch.equal(ENS.merge_probabilities(members), seg)
    for R in (1, 3):
        members = random_members(M, R, SHAPES[0], 30 * M + R, dtype, regions=True)
        want = np_average(as_np(members))
        seg, mean = ENS.merge_probabilities(members, regions_class_order=ORDERS[R], return_probabilities=True)
        assert same_bits(mean.numpy(), want) and np.array_equal(seg.numpy(), np_regions(want, ORDERS[R]))


def test_inputs_are_not_modified():
    members = grid_members(3, 2, (1, 4, 4), 1)
    before = [m.clone() for m in members]
    ENS.average_probabilities(members)
    ENS.merge_probabilities(members)
    assert all(torch.equal(a, b) for a, b in zip(members, before))


@pytest.mark.parametrize("M", [2, 3, 5, 16])
@pytest.mark.parametrize("K", [2, 3, 8])
def test_grid_inputs_argmax_of_mean_equals_the_reference_argmax(M, K):
    members = grid_members(M, K, (3, 67, 129), 100 * M + K)
    mean = np_average(as_np(members))
    a, b = np_argmax(mean), np_softmax_argmax(mean)
    assert np.array_equal(a, b)                                        # the precondition: the two numpy formulas agree on the grid
    top = np.sort(mean, axis=0)
    assert int((top[-1] == top[-2]).sum()) > 0                         # exact ties are among the voxels
    assert np.array_equal(ENS.merge_probabilities(members).numpy(), a)


def test_exact_ties_give_the_lowest_index():
    p = torch.tensor([0.25, 0.5, 0.5, 0.125]).view(4, 1, 1, 1).expand(4, 1, 2, 3).contiguous()
    q = torch.tensor([0.5, 0.25, 0.25, 0.5]).view(4, 1, 1, 1).expand(4, 1, 2, 3).contiguous()
    assert bool((ENS.merge_probabilities([p, q]) == 0).all())         # means 0.375 0.375 0.375 0.3125
    assert bool((ENS.merge_probabilities([p]) == 1).all())


def test_region_threshold_and_paint_order():
    # two regions, four voxels: means (0.5, 0.5) | (0.625, 0.5) | (0.625, 0.625) | (0.375, 0.75)
    a = torch.tensor([[0.25, 0.5, 0.5, 0.25], [0.25, 0.25, 0.5, 0.75]]).view(2, 1, 1, 4)
    b = torch.tensor([[0.75, 0.75, 0.75, 0.5], [0.75, 0.75, 0.75, 0.75]]).view(2, 1, 1, 4)
    seg, mean = ENS.merge_probabilities([a, b], regions_class_order=[3, 1], return_probabilities=True)
    assert mean.view(2, 4).tolist() == [[0.5, 0.625, 0.625, 0.375], [0.5, 0.5, 0.625, 0.75]]
    assert seg.view(4).tolist() == [0, 3, 1, 1]                        # 0.5 is not painted; a later region overwrites an earlier one
    assert ENS.merge_probabilities([a, b], regions_class_order=[1, 3]).view(4).tolist() == [0, 1, 3, 3]
    # the reference's double sigmoid would paint all four: sigmoid(mean) > 0.5 wherever mean > 0
    assert bool((torch.sigmoid(mean) > 0.5).all())


def test_non_finite_raises():
    for bad in (float("nan"), float("inf")):
        members = grid_members(2, 3, (1, 4, 4), 3)
        members[1][2, 0, 1, 1] = bad
        with pytest.raises(RuntimeError, match="Encountered inf in predicted array"):
            ENS.merge_probabilities(members)


def test_value_errors():
    ok = grid_members(2, 3, (1, 4, 4), 0)
    with pytest.raises(ValueError, match="at least one"):
        ENS.merge_probabilities([])
    with pytest.raises(ValueError, match="at least one"):
        ENS.average_probabilities([])
    with pytest.raises(ValueError, match="at most 16"):
        ENS.merge_probabilities(grid_members(17, 2, (1, 2, 2), 0))
    with pytest.raises(ValueError, match="at most 16"):
        ENS.average_probabilities(grid_members(17, 2, (1, 2, 2), 0))
    with pytest.raises(ValueError, match="one shape, dtype and device"):
        ENS.merge_probabilities([ok[0], ok[1][:, :, :3]])
    with pytest.raises(ValueError, match="one shape, dtype and device"):
        ENS.merge_probabilities([ok[0], ok[1].half()])
    with pytest.raises(ValueError, match="float32 or float16"):
        ENS.merge_probabilities([m.double() for m in ok])
    with pytest.raises(ValueError, match="float32 or float16"):
        ENS.average_probabilities([m.to(torch.bfloat16) for m in ok])
    with pytest.raises(ValueError, match=r"\(K, D, H, W\)"):
        ENS.merge_probabilities([m[0] for m in ok])
    with pytest.raises(ValueError, match="2..8 classes"):
        ENS.merge_probabilities(grid_members(2, 9, (1, 2, 2), 0))
    with pytest.raises(ValueError, match="2..8 classes"):
        ENS.merge_probabilities(grid_members(2, 1, (1, 2, 2), 0))
    with pytest.raises(ValueError, match="1..8 regions"):
        ENS.merge_probabilities(grid_members(2, 9, (1, 2, 2), 0), regions_class_order=list(range(1, 10)))
    with pytest.raises(ValueError, match="regions_class_order has"):
        ENS.merge_probabilities(ok, regions_class_order=[1, 2])
    assert ENS.merge_probabilities(grid_members(2, 1, (1, 2, 2), 0), regions_class_order=[4]).shape == (1, 2, 2)
    assert ENS.average_probabilities(grid_members(2, 11, (1, 2, 2), 0)).shape == (11, 1, 2, 2)       # the mean alone has no head limit


# ------------------------------------------------------------------------------------------------ cases and folds
def test_ensemble_cases():
    m1 = {f"case{i}": grid_members(1, 3, (1, 4, 5), i)[0] for i in range(3)}
    m2 = {f"case{i}": grid_members(1, 3, (1, 4, 5), 10 + i)[0] for i in range(3)}
    out = ENS.ensemble_cases([m1, m2])
    assert list(out) == ["case0", "case1", "case2"]
    for c in out:
        assert torch.equal(out[c], ENS.merge_probabilities([m1[c], m2[c]]))
    seg, mean = ENS.ensemble_cases([m1, m2], return_probabilities=True)["case1"]
    assert same_bits(mean.numpy(), np_average([m1["case1"].numpy(), m2["case1"].numpy()]))
    short = {k: v for k, v in m2.items() if k != "case1"}
    with pytest.raises(AssertionError, match="same cases"):
        ENS.ensemble_cases([m1, short])
    with pytest.raises(AssertionError, match="same cases"):
        ENS.ensemble_cases([short, m1])


def test_ensemble_crossvalidations():
    probs = {i: grid_members(2, 2, (1, 3, 4), 50 + i) for i in range(4)}                  # case i -> [model a, model b]
    a = {0: {"c0": probs[0][0], "c1": probs[1][0]}, 1: {"c2": probs[2][0], "c3": probs[3][0]}}
    b = {0: {"c3": probs[3][1]}, 1: {"c0": probs[0][1], "c1": probs[1][1], "c2": probs[2][1]}}      # another split of the same cases
    out = ENS.ensemble_crossvalidations([a, b])
    assert list(out) == ["c0", "c1", "c2", "c3"]
    for i in range(4):
        assert torch.equal(out[f"c{i}"], ENS.merge_probabilities(probs[i]))
    assert list(ENS.ensemble_crossvalidations([a, b], folds=(0, 1))) == ["c0", "c1", "c2", "c3"]
    missing = {0: dict(b[0]), 1: {k: v for k, v in b[1].items() if k != "c1"}}
    with pytest.raises(RuntimeError, match="Missing"):
        ENS.ensemble_crossvalidations([a, missing])
    dup = {0: dict(b[0], c0=probs[0][1]), 1: dict(b[1])}
    with pytest.raises(RuntimeError, match="Duplicate"):
        ENS.ensemble_crossvalidations([a, dup])
    with pytest.raises(RuntimeError, match="fold 2"):
        ENS.ensemble_crossvalidations([a, b], folds=(0, 1, 2))
    with pytest.raises(RuntimeError, match="fold 1"):
        ENS.ensemble_crossvalidations([a, {0: b[0], 1: {}}])


# ------------------------------------------------------------------------------------------------ find_best_configuration
def fb_cases(device="cpu"):
    """Three cases (1, 12, 12), label 1 = a 6 x 6 square.  `left` is sure (0.875) of the square's left half and doubtful (0.375) of its right
    half, `right` the other way round: their mean is 0.625 on the whole square.  Both, and so their mean, see a false voxel far away
    (0.625).  `poor` predicts one row of the square only."""
    refs, left, right, poor = {}, {}, {}, {}
    for i, (y, x) in enumerate([(0, 0), (1, 2), (3, 1)]):
        ref = torch.zeros((1, 12, 12), dtype=torch.uint8)
        ref[0, y:y + 6, x:x + 6] = 1
        pl, pr, pp = torch.zeros((1, 12, 12)), torch.zeros((1, 12, 12)), torch.zeros((1, 12, 12))
        pl[0, y:y + 6, x:x + 3], pl[0, y:y + 6, x + 3:x + 6] = 0.875, 0.375
        pr[0, y:y + 6, x:x + 3], pr[0, y:y + 6, x + 3:x + 6] = 0.375, 0.875
        pl[0, 11, 11] = pr[0, 11, 11] = 0.625
        pp[0, y, x:x + 6] = 0.75
        name = f"case{i}"
        refs[name] = ref.to(device)
        for table, p1 in ((left, pl), (right, pr), (poor, pp)):
            probs = torch.stack([1.0 - p1, p1]).to(device)
            table[name] = (ENS.merge_probabilities([probs]), probs)
    return refs, left, right, poor


def dice_of(segs, refs):
    vals = []
    for c in refs:
        tp, fp, fn, _ = EX.segmentation_counts(segs[c], refs[c], [1]).tolist()
        vals.append(2 * tp[0] / (2 * tp[0] + fp[0] + fn[0]))
    return float(np.mean(vals))


def check_find_best(device="cpu"):
    refs, left, right, poor = fb_cases(device)
    models = {"left": left, "right": right, "poor": poor}
    res = ENS.find_best_configuration(models, refs, [1], [1])
    # single models first, then the pairs i < j
    assert list(res["all_results"]) == ["left", "right", "poor", "ensemble___left___right", "ensemble___left___poor", "ensemble___right___poor"]
    half = 2 * 18 / (2 * 18 + 1 + 18)
    assert res["all_results"]["left"] == pytest.approx(half, abs=1e-12) and res["all_results"]["right"] == res["all_results"]["left"]
    assert res["all_results"]["poor"] == pytest.approx(2 * 6 / (2 * 6 + 30), abs=1e-12)
    # the ensemble beats both of its members and is selected
    best = res["best_model_or_ensemble"]
    assert best["selected_model_or_models"] == ["left", "right"]
    assert best["result_on_crossval_pre_pp"] == res["all_results"]["ensemble___left___right"] == pytest.approx(72 / 73, abs=1e-12)
    assert best["result_on_crossval_pre_pp"] > max(res["all_results"]["left"], res["all_results"]["right"])
    # the hand-off to determine_postprocessing: the false voxel goes, and the result replays through apply_postprocessing
    pp_fns, pp_fn_kwargs = res["postprocessing"]
    assert [f.__name__ for f in pp_fns] == ["remove_all_but_largest_component_from_segmentation"] and pp_fn_kwargs == [{"labels_or_regions": [1]}]
    assert best["result_on_crossval_post_pp"] == 1.0
    merged = {c: ENS.merge_probabilities([left[c][1], right[c][1]]) for c in refs}
    replayed = {c: PP.apply_postprocessing(merged[c], pp_fns, pp_fn_kwargs) for c in refs}
    assert all(torch.equal(replayed[c], refs[c]) for c in refs)
    assert dice_of(merged, refs) == pytest.approx(best["result_on_crossval_pre_pp"], abs=1e-12)
    # an exact tie picks the first entry, whatever the order
    for names in (("left", "right"), ("right", "left")):
        tie = ENS.find_best_configuration({n: models[n] for n in names}, refs, [1], [1], allow_ensembling=False)
        assert list(tie["all_results"]) == list(names) and tie["all_results"][names[0]] == tie["all_results"][names[1]]
        assert tie["best_model_or_ensemble"]["selected_model_or_models"] == [names[0]]
    # ... and a single model wins a tie against an ensemble: two copies of one model, their ensemble predicts the same maps
    twin = ENS.find_best_configuration({"a": left, "b": left}, refs, [1], [1])
    assert len(set(twin["all_results"].values())) == 1 and list(twin["all_results"])[-1] == "ensemble___a___b"
    assert twin["best_model_or_ensemble"]["selected_model_or_models"] == ["a"]
    # without probabilities there is nothing to merge
    no_probs = {c: (s, None) for c, (s, _) in right.items()}
    with pytest.raises(ValueError, match="no probabilities"):
        ENS.find_best_configuration({"left": left, "right": no_probs}, refs, [1], [1])
    alone = ENS.find_best_configuration({"left": left, "right": no_probs}, refs, [1], [1], allow_ensembling=False)
    assert alone["best_model_or_ensemble"]["selected_model_or_models"] == ["left"]
    with pytest.raises(ValueError, match="reference cases"):
        ENS.find_best_configuration({"left": {c: v for c, v in left.items() if c != "case1"}}, refs, [1], [1])
    # label 2 occurs nowhere: its Dice is nan in every case, so is every foreground mean, and nothing can be ranked
    with pytest.raises(ValueError, match="nan"):
        ENS.find_best_configuration(models, refs, [1, 2], [1, 2])


def test_find_best_configuration():
    check_find_best("cpu")
