"""GPU tests (-m gpu) of what the shared per-pixel bodies of the fused losses (csrc/loss_common.h) make structural: kernels that run the
same body over the same grid in the same reduction order give the same bits.

 * the deep-supervision loss with ONE scale of weight 1 at full resolution is the single-scale loss: loss and gradient bits of
   dice_ce_masked_loss (softmax with an ignore label) and of dice_bce_loss on labels_to_regions planes (regions, with and without an
   ignore label);
 * its plain-label mode is the masked loss with an ignore value no label takes;
 * the values pass of the top-k loss adds the Dice sums of the masked loss: sums[1:] of du_topk_loss_fwd and du_dice_ce_masked_sums.

(2, 3, 5, 7): the guarded scalar path with a partial last quad; (2, 3, 48, 48): the vector path, three partial rows."""
import pytest
import torch

from test_gpu_ops import dev

pytestmark = pytest.mark.gpu

SHAPES = [(2, 3, 5, 7), (2, 3, 48, 48)]
IGNORE = 3
GO = 1.7


def _inputs(shape, ignore, odd=False, seed=0):
    """logits and (B,1,H,W) labels in [0, C) with ~20 % `ignore` (None: none); odd: a few -1 and 70, which belong to no region"""
    B, C_, H, W = shape
    g = torch.Generator().manual_seed(seed + H)
    x = torch.randn(shape, generator=g) * 3.0
    t = torch.randint(0, C_, (B, 1, H, W), generator=g)
    u = torch.rand((B, 1, H, W), generator=g)
    if ignore is not None:
        t[u < 0.2] = ignore
    if odd:
        t[(u > 0.2) & (u < 0.23)] = -1
        t[(u > 0.23) & (u < 0.26)] = 70
    d = dev()
    return x.to(d), t.to(d)


def _loss_and_grad(fn, x):
    x = x.clone().requires_grad_(True)
    loss = fn(x)
    (loss * GO).backward()
    torch.cuda.synchronize()
    return loss.detach(), x.grad


def _assert_same_bits(a, b, what):
    (la, ga), (lb, gb) = a, b
    assert torch.equal(la, lb), f"{what}: loss {float(la)!r} vs {float(lb)!r}"
    assert bool(torch.isfinite(ga).all()) and float(ga.abs().max()) > 0
    assert torch.equal(ga, gb), f"{what}: {int((ga != gb).sum())} gradient elements differ, max {float((ga - gb).abs().max()):.3e}"


@pytest.mark.parametrize("shape", SHAPES)
def test_one_scale_softmax_ignore_is_the_masked_loss(shape):
    from dinounet_amd import ops
    x, t = _inputs(shape, IGNORE)
    ds = _loss_and_grad(lambda v: ops.ds_seg_loss([v], t, "softmax_ignore", (1.0,), ignore_label=IGNORE), x)
    one = _loss_and_grad(lambda v: ops.dice_ce_masked_loss(v, t, IGNORE), x)
    _assert_same_bits(ds, one, f"softmax_ignore {shape}")


@pytest.mark.parametrize("ignore", [None, 7])
@pytest.mark.parametrize("shape", SHAPES)
def test_one_scale_regions_is_the_region_loss(shape, ignore):
    from dinounet_amd import ops
    x, t = _inputs(shape, ignore, odd=True)
    table = torch.tensor([0b1110, 0b1100, 0b1000], dtype=torch.int64, device=x.device)      # regions (1, 2, 3), (2, 3), (3,)
    planes = ops.labels_to_regions(t, table, ignore)
    ds = _loss_and_grad(lambda v: ops.ds_seg_loss([v], t, "regions", (1.0,), table=table, ignore_label=ignore), x)
    one = _loss_and_grad(lambda v: ops.dice_bce_loss(v, planes, ignore is not None), x)
    _assert_same_bits(ds, one, f"regions {shape} ignore {ignore}")


@pytest.mark.parametrize("shape", SHAPES)
def test_one_scale_plain_labels_is_the_masked_loss_with_an_unused_ignore_value(shape):
    from dinounet_amd import ops
    x, t = _inputs(shape, None)
    ds = _loss_and_grad(lambda v: ops.ds_seg_loss([v], t, "softmax", (1.0,)), x)
    one = _loss_and_grad(lambda v: ops.dice_ce_masked_loss(v, t, -1), x)
    _assert_same_bits(ds, one, f"softmax {shape}")


@pytest.mark.parametrize("has_ignore", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_topk_values_pass_adds_the_dice_sums_of_the_masked_loss(shape, has_ignore):
    from dinounet_amd import _lib
    from dinounet_amd.ops import _p, _st
    L = _lib.lib()
    x, t = _inputs(shape, IGNORE if has_ignore else None)
    B, K, H, W = shape
    HW = H * W
    t = t.reshape(B, HW).contiguous()
    d = x.device
    ignore = IGNORE if has_ignore else -(2 ** 63)                 # what du_topk_loss_fwd masks with when there is no ignore label
    n = int(L.du_dice_ce_masked_ws_elems(B, K, HW))
    ws = torch.empty(n, dtype=torch.float32, device=d)
    sums_m = torch.empty(2 + 3 * (K - 1), dtype=torch.float32, device=d)
    _lib.check(L.du_dice_ce_masked_sums(_p(x), _p(t), _p(sums_m), B, K, HW, ignore, _p(ws), n, _st()), "du_dice_ce_masked_sums")
    n = int(L.du_topk_loss_ws_elems(B, K, HW))
    ws = torch.empty(n, dtype=torch.int32, device=d)
    values = torch.empty((B, HW), dtype=torch.float32, device=d)
    sums_t = torch.empty(2 + 3 * (K - 1), dtype=torch.float32, device=d)
    _lib.check(L.du_topk_loss_fwd(_p(x), _p(t), _p(values), _p(sums_t), B, K, HW, has_ignore, IGNORE, max(1, B * HW // 10), _p(ws), n,
                                  _st()), "du_topk_loss_fwd")
    torch.cuda.synchronize()
    assert float(sums_t[1]) > 0 and bool((sums_t[2:] > 0).all())
    assert torch.equal(sums_t[1:], sums_m[1:]), (sums_t.tolist(), sums_m.tolist())
