"""CPU suite (-m "not gpu"): the oracle against the committed golden vectors, the drop-in boundary (state_dict key
contract, plugin classes, module API), the C-ABI library (loads, exports every declared symbol) and the host glue
(product modules with torch stand-ins for the HIP ops reproduce the reference's logits)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from oracle import dinounet_oracle as O
from oracle import weights
from oracle.refshim import PLANS_2D

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _load(name):
    g = np.load(os.path.join(GOLD, name + ".npz"))
    return g, json.loads(str(g["meta"]))


def _sd(model):
    keys = json.load(open(os.path.join(GOLD, f"state_dict_{model}.json")))["keys"]
    return weights.make_state_dict([(k, tuple(s)) for k, s, _ in keys], seed=0)


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


# ---------------------------------------------------------------- oracle vs golden (reference outputs)
@pytest.mark.parametrize("name", ["dinounet_s_64_eval", "dinounet_s_96x64_eval", "dinounet_s_64_c1_eval", "dinounet_s_64_k4_eval",
                                  "dinounet_b_64_eval"])
def test_oracle_matches_reference_golden(name):
    g, meta = _load(name)
    sd = _sd(meta["model"])
    if meta["num_classes"] != 2:   # seg heads have K rows
        for k in list(sd):
            if ".seg_layers." in k:
                shp = list(sd[k].shape); shp[0] = meta["num_classes"]
                sd[k] = weights.make_tensor(k, shp)
    x = weights.make_input(meta["B"], meta["C"], meta["H"], meta["W"], seed=0)
    with torch.no_grad():
        y = O.dinounet_forward(x, sd, meta["model"])
    ref = torch.from_numpy(g["logits"])
    assert rel(y, ref) < 2e-5
    am = y.argmax(1).numpy().astype(np.uint8)
    gold_am = np.unpackbits(g["argmax"])[: am.size].reshape(am.shape) if meta["num_classes"] == 2 else g["argmax"]
    assert (am != gold_am).mean() < 1e-4


def test_oracle_vit7b_style_matches_reference_golden():
    """The paths only the 7B backbone takes (head dim 128, no qkv bias, SwiGLU-64, train-mode batch-subset stochastic depth 0.4 with
    pinned subsets + pinned per-block RoPE rescale): the restatement against the reference's own DinoVisionTransformer outputs."""
    g = np.load(os.path.join(GOLD, "vit7b_style_64.npz"))
    meta = json.loads(str(g["meta"]))
    cfg, B = meta["cfg"], meta["B"]
    sd = weights.make_state_dict([(k, tuple(s)) for k, s in meta["keys"]], seed=0)
    depth = cfg["depth"]
    ocfg = dict(embed_dim=cfg["embed_dim"], depth=depth, num_heads=cfg["num_heads"], ffn="swiglu", qkv_bias=False,
                interaction_indexes=list(range(depth)))
    x = weights.make_input(B, 3, meta["H"], meta["W"], seed=6)
    with torch.no_grad():
        ev = O.vit_intermediate(x, O.SD(sd), ocfg)
        log_scales, _ = weights.pinned_randomness(depth, B, seed=3)
        subsets = weights.pinned_subsets(depth, B, cfg["drop_path_rate"], seed=3)
        tr = O.vit_intermediate(x, O.SD(sd), ocfg, rope_rescale=log_scales.exp(), subsets=subsets)
    for i in range(depth):
        assert rel(ev[i][0], torch.from_numpy(g[f"eval_patch{i}"])) < 2e-5 and rel(ev[i][1], torch.from_numpy(g[f"eval_cls{i}"])) < 2e-5
        assert rel(tr[i][0], torch.from_numpy(g[f"train_patch{i}"])) < 2e-5 and rel(tr[i][1], torch.from_numpy(g[f"train_cls{i}"])) < 2e-5
    assert rel(tr[depth - 1][0], ev[depth - 1][0]) > 1e-3      # the pinned train-mode path really differs from eval


def test_oracle_msda_loops_match_reference_fixture():
    """ops/test.py fixture (seed 3): scalar restatement of the CUDA loop == reference grid_sample core (fp64)."""
    g = np.load(os.path.join(GOLD, "msda_testpy.npz"))
    shapes, lsi = torch.from_numpy(g["shapes"]), torch.from_numpy(g["level_start_index"])
    for tag in ("D2", "D30", "D71", "border"):
        v, loc, a = (torch.from_numpy(g[f"{tag}_{n}"]) for n in ("value", "loc", "attn"))
        out = O.msda_core_loops(v, shapes, lsi, loc, a)
        assert (out - torch.from_numpy(g[f"{tag}_out"])).abs().max() < 1e-12
        gv, gl, ga = O.msda_backward(v, shapes.tolist(), loc, a, torch.from_numpy(g[f"{tag}_grad_out"]))
        assert (gv - torch.from_numpy(g[f"{tag}_grad_value"])).abs().max() < 1e-10
        assert (gl - torch.from_numpy(g[f"{tag}_grad_loc"])).abs().max() < 1e-10
        assert (ga - torch.from_numpy(g[f"{tag}_grad_attn"])).abs().max() < 1e-10


# ---------------------------------------------------------------- boundary
@pytest.mark.parametrize("model", ["dinounet_s", "dinounet_b"])
def test_state_dict_contract(model):
    from dinounet_amd.network_architecture import DinoUNet
    net = DinoUNet.from_config(PLANS_2D, 3, 2, dinov3_pretrained_path=None, dinov3_model_name=model)
    gold = json.load(open(os.path.join(GOLD, f"state_dict_{model}.json")))["keys"]
    mine = [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in net.state_dict().items()]
    assert mine == gold                                     # same keys, shapes, dtypes, same order
    sd = net.state_dict()
    assert sd["decoder.encoder.fapm.shared_basis.weight"].data_ptr() == sd["encoder.fapm.shared_basis.weight"].data_ptr()
    trainable = sum(p.numel() for p in net.parameters() if p.requires_grad)
    frozen = sum(p.numel() for p in net.parameters() if not p.requires_grad)
    assert (trainable, frozen) == {"dinounet_s": (6188322, 21596544), "dinounet_b": (13178082, 85670400)}[model] or trainable > 0
    assert all(not p.requires_grad for p in net.encoder.dinov3_adapter.backbone.parameters())
    net.load_state_dict(weights.make_state_dict([(k, tuple(s)) for k, s, _ in gold]), strict=True)


def test_plugin_surface():
    import dinounet_amd.dinounet_training as DT
    for n in ("DinoUNet", "DINOv3EncoderAdapter", "FAPM", "UNetDecoder", "SqueezeExcitation", "DepthwiseSeparableConv",
              "LearnableUpsampleBlock", "DinoUNetTrainer", "DinoUNetTrainer_s", "DinoUNetTrainer_b", "DinoUNetTrainer_l",
              "DinoUNetTrainer_7b", "DINOV3_TRAINERS", "get_dinov3_trainer", "load_dinov3_model", "DINOv3_MODEL_FACTORIES",
              "DINOv3_INTERACTION_INDEXES", "DINOv3_MODEL_INFO", "main_dinov3"):
        assert hasattr(DT, n), n
    T = DT.get_dinov3_trainer("dinounet_s")
    T.set_network_config(PLANS_2D, dinov3_pretrained_path="/nonexistent.pth")
    with pytest.raises(FileNotFoundError):                 # a wrong checkpoint path must not silently train on a random frozen ViT
        T.build_network_architecture("ignored", {}, [], 3, 2, enable_deep_supervision=False)
    DT.DinoUNetTrainer._dinov3_pretrained_path = T._dinov3_pretrained_path = None
    net = T.build_network_architecture("ignored", {}, [], 3, 2, enable_deep_supervision=False)
    assert isinstance(net, DT.DinoUNet) and net.decoder.deep_supervision is False
    enc = net.encoder
    for a in ("output_channels", "strides", "kernel_sizes", "conv_op", "norm_op", "norm_op_kwargs", "dropout_op",
              "dropout_op_kwargs", "nonlin", "nonlin_kwargs", "conv_bias"):
        assert hasattr(enc, a)
    with pytest.raises(ValueError):
        DT.get_dinov3_trainer("dinounet_xl")
    with pytest.raises(RuntimeError):                      # product path has no CPU fallback
        net(torch.zeros(1, 3, 64, 64))


def test_msda_extension_module_surface():
    import MultiScaleDeformableAttention as MSDA
    assert callable(MSDA.ms_deform_attn_forward) and callable(MSDA.ms_deform_attn_backward)
    v = torch.zeros(1, 4, 2, 4)
    with pytest.raises(RuntimeError):                      # "must be a CUDA tensor" (ms_deform_attn_cuda.cu:39-43)
        MSDA.ms_deform_attn_forward(v, torch.tensor([[2, 2]]), torch.tensor([0]), torch.zeros(1, 1, 2, 1, 1, 2),
                                    torch.zeros(1, 1, 2, 1, 1), 64)


# ---------------------------------------------------------------- C ABI
def test_c_abi_exports_every_declared_symbol():
    from dinounet_amd import _lib
    protos = _lib.header_prototypes()
    assert len(protos) >= 25
    assert os.path.exists(_lib.LIB_PATH), "libdinounet_hip.so must be built (python -m dinounet_amd._build)"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in protos:
        assert hasattr(lib, name), f"{name} declared in include/dinounet_hip.h but not exported"
    assert b"gfx950" in _lib.lib().du_version()


def test_release_library_reads_no_environment_knobs():
    """the debugging / A-B knobs of csrc/*.hip (DU_CONV_STRIP, DU_P8_NO_TAIL, DU_SKINNY_FUSE_KMAX, ...) are compiled
    in only with -DDU_DEBUG_KNOBS (DINOUNET_DEBUG_KNOBS=1 at build time, the measurement tools' build).  The library the product and the
    driver build must not contain a single one of those names: what ships cannot be reconfigured through the environment."""
    import re
    from dinounet_amd import _build
    if os.environ.get("DINOUNET_DEBUG_KNOBS") == "1":
        pytest.skip("debug-knob build")
    names = set()
    for f in os.listdir(_build.CSRC):
        if f.endswith(".hip"):
            names |= set(re.findall(r'DU_GETENV\("([A-Z0-9_]+)"\)', open(os.path.join(_build.CSRC, f)).read()))
    assert len(names) >= 25                                   # the knobs exist in the sources ...
    blob = open(_build.build(verbose=False), "rb").read()
    present = sorted(n for n in names if n.encode() in blob)
    assert not present, present                              # ... and none of them in the binary


def test_c_abi_argument_validation_without_gpu():
    """Bad arguments are rejected before any launch (DU_ERR_BAD_ARG), so this runs without a device."""
    from dinounet_amd import _lib
    a = _lib.GemmArgs()
    assert _lib.lib().du_gemm(ctypes.byref(a), None) == -1
    with pytest.raises(RuntimeError):
        _lib.check(-1, "du_gemm")


# ---------------------------------------------------------------- host glue with stand-in ops
@pytest.mark.parametrize("name", ["dinounet_s_64_eval", "dinounet_s_96x64_eval", "dinounet_s_64_c1_eval"])
def test_host_glue_reproduces_reference_logits(name):
    import _cpu_op_shim as shim
    from dinounet_amd.network_architecture import DinoUNet
    g, meta = _load(name)
    net = DinoUNet.from_config(PLANS_2D, 3, 2, dinov3_pretrained_path=None, dinov3_model_name=meta["model"], precision="fp32")
    net.load_state_dict(_sd(meta["model"]), strict=True)
    net.eval()
    x = weights.make_input(meta["B"], meta["C"], meta["H"], meta["W"], seed=0)
    with shim.patched_ops(), torch.no_grad():
        y = net.decoder(net.encoder(x))
    assert rel(y, torch.from_numpy(g["logits"])) < 2e-5


def test_host_glue_train_mode_and_grads():
    """train(): batch-stat BN + running-stat update, loss, backward through the product's module wiring."""
    import _cpu_op_shim as shim
    from dinounet_amd.network_architecture import DinoUNet
    from dinounet_amd.dinov3.adapter import DropPath
    g, meta = _load("dinounet_s_64_train")
    net = DinoUNet.from_config(PLANS_2D, 3, 2, dinov3_pretrained_path=None, dinov3_model_name="dinounet_s", precision="fp32")
    net.load_state_dict(_sd("dinounet_s"), strict=True)
    net.train()
    for m in net.modules():
        if isinstance(m, DropPath):
            m.drop_prob = 0.0
    net.encoder.dinov3_adapter.backbone.rope_embed.rescale_coords = None
    x = weights.make_input(2, 3, 64, 64, seed=1)
    tgt = weights.make_target(2, 64, 64, 2, seed=1)
    with shim.patched_ops():
        y = net.decoder(net.encoder(x))
        loss = O.dc_and_ce_loss(y, tgt)
        loss.backward()
    assert rel(y.detach(), torch.from_numpy(g["logits"])) < 2e-5
    assert abs(loss.item() - float(g["loss"])) < 1e-5
    norms = meta["grad_norms"]
    gmax = max(norms.values())
    named = dict(net.named_parameters())
    for k, n in norms.items():
        got = float(named[k].grad.norm())
        assert abs(got - n) <= 5e-3 * max(n, 1e-3 * gmax), (k, got, n)
    assert sorted(k for k, p in named.items() if p.requires_grad and p.grad is None) == meta["unused"]


def test_deep_supervision_oracle_and_host_glue_match_reference_golden():
    """deep_supervision=True (dinounet_training.py:603-629): the oracle restatement AND the product's module wiring (kernels replaced by the
    torch shim) against the reference's three logits tensors, the weighted loss and the gradient norms of dinounet_s_64_ds_train.npz."""
    import _cpu_op_shim as shim
    from dinounet_amd.network_architecture import DinoUNet
    from dinounet_amd.dinov3.adapter import DropPath
    g, meta = _load("dinounet_s_64_ds_train")
    x = weights.make_input(2, 3, 64, 64, seed=1)
    tgt = weights.make_target(2, 64, 64, 2, seed=1)
    with torch.no_grad():
        outs = O.dinounet_forward(x, _sd("dinounet_s"), "dinounet_s", training=True, deep_supervision=True)
    assert [tuple(o.shape) for o in outs] == [(2, 2, 64, 64), (2, 2, 32, 32), (2, 2, 16, 16)]
    for i, o in enumerate(outs):
        assert rel(o, torch.from_numpy(g[f"logits{i}"])) < 2e-5, i
    plans = dict(PLANS_2D, architecture=dict(PLANS_2D["architecture"], deep_supervision=True))
    net = DinoUNet.from_config(plans, 3, 2, dinov3_pretrained_path=None, dinov3_model_name="dinounet_s", precision="fp32")
    net.load_state_dict(_sd("dinounet_s"), strict=True)
    net.train()
    for m in net.modules():
        if isinstance(m, DropPath):
            m.drop_prob = 0.0
    net.encoder.dinov3_adapter.backbone.rope_embed.rescale_coords = None
    with shim.patched_ops():
        ys = net.decoder(net.encoder(x))
        assert isinstance(ys, list) and len(ys) == 3
        loss = sum(w * O.dc_and_ce_loss(y, tgt[..., ::2 ** i, ::2 ** i].contiguous()) for i, (y, w) in enumerate(zip(ys, meta["ds_weights"])))
        loss.backward()
    for i, y in enumerate(ys):
        assert rel(y.detach(), torch.from_numpy(g[f"logits{i}"])) < 2e-5, i
    assert abs(loss.item() - float(g["loss"])) < 1e-5
    norms = meta["grad_norms"]
    gmax = max(norms.values())
    named = dict(net.named_parameters())
    for k, n in norms.items():
        got = float(named[k].grad.norm())
        assert abs(got - n) <= 5e-3 * max(n, 1e-3 * gmax), (k, got, n)
    assert sorted(k for k, p in named.items() if p.requires_grad and p.grad is None) == meta["unused"]


def test_host_glue_pinned_train_randomness():
    """train() with the per-block RoPE rescale draws and the DropPath masks pinned to the values the reference was given
    (oracle/make_golden.py: pin_reference_randomness): the product's wiring of both random ops (device-side draws replaced through the
    `pinned_*` hooks) reproduces the reference's logits, loss and every gradient -- SURVEY rows a6 / a15."""
    import _cpu_op_shim as shim
    from dinounet_amd.network_architecture import DinoUNet
    from dinounet_amd.dinov3.adapter import DropPath
    g, meta = _load("dinounet_s_64_train_pinned")
    net = DinoUNet.from_config(PLANS_2D, 3, 2, dinov3_pretrained_path=None, dinov3_model_name="dinounet_s", precision="fp32")
    net.load_state_dict(_sd("dinounet_s"), strict=True)
    net.train()
    bb = net.encoder.dinov3_adapter.backbone
    log_scales, masks = weights.pinned_randomness(len(bb.blocks), meta["B"], seed=2)
    bb.rope_embed.pinned_log_scales = log_scales
    dps = [m for m in net.modules() if isinstance(m, DropPath)]
    assert len(dps) == len(masks)
    for m, mk in zip(dps, masks):
        m.pinned_mask = mk
    x = weights.make_input(meta["B"], 3, meta["H"], meta["W"], seed=2)
    tgt = weights.make_target(meta["B"], meta["H"], meta["W"], 2, seed=2)
    with shim.patched_ops():
        y = net.decoder(net.encoder(x))
        loss = O.dc_and_ce_loss(y, tgt)
        loss.backward()
    assert rel(y.detach(), torch.from_numpy(g["logits"])) < 2e-5
    assert abs(loss.item() - float(g["loss"])) < 1e-5
    gmax = max(meta["grad_norms"].values())
    named = dict(net.named_parameters())
    n = 0
    for key in g.files:
        if key.startswith("grad:"):
            k = key[5:]
            ref = torch.from_numpy(g[key])
            got = named[k].grad.flatten()
            if got.numel() > meta["sample"]:
                got = got[weights.sample_indices(k, got.numel(), meta["sample"])]
            denom = max(float(ref.norm()), 1e-3 * gmax * (ref.numel() / named[k].numel()) ** 0.5)
            assert float((got - ref).norm()) / denom < 5e-3, k
            n += 1
    assert n == len(meta["grad_norms"])


def test_zero_pool_one_buffer_per_step_without_aliasing():
    """ops.ZeroPool: the second step with the same request sequence is served from ONE zero-filled buffer; a later step never hands
    out memory that an earlier step's gradients still own; a deviating request falls back to plain zeros."""
    from dinounet_amd import ops
    pool = ops.ZeroPool()
    pool.enabled = True
    dev = torch.device("cpu")
    pool.new_step()
    a1, b1 = pool.zeros((4, 8), dev), pool.zeros((3,), dev)                      # recording step: plain tensors
    assert a1.untyped_storage().data_ptr() != b1.untyped_storage().data_ptr()
    pool.new_step()
    a2, b2 = pool.zeros((4, 8), dev), pool.zeros((3,), dev)
    assert a2.untyped_storage().data_ptr() == b2.untyped_storage().data_ptr() and a2.shape == (4, 8) and b2.shape == (3,)
    assert float(a2.abs().sum()) == 0 and float(b2.abs().sum()) == 0
    a2.add_(1.0)
    b2.add_(2.0)
    pool.new_step()
    a3 = pool.zeros((4, 8), dev)
    assert a3.untyped_storage().data_ptr() != a2.untyped_storage().data_ptr()
    assert float(a3.abs().sum()) == 0 and float(a2.sum()) == 32 and float(b2.sum()) == 6
    c3 = pool.zeros((5,), dev)                                                   # not the recorded size: fallback
    assert c3.untyped_storage().data_ptr() != a3.untyped_storage().data_ptr() and float(c3.abs().sum()) == 0
    d3 = pool.zeros((3,), dev)                                                   # rest of the step stays on the fallback
    assert d3.untyped_storage().data_ptr() != a3.untyped_storage().data_ptr()
    pool.new_step()                                                              # the deviating step became the new plan
    a4, c4, d4 = pool.zeros((4, 8), dev), pool.zeros((5,), dev), pool.zeros((3,), dev)
    assert a4.untyped_storage().data_ptr() == c4.untyped_storage().data_ptr() == d4.untyped_storage().data_ptr()


def test_sliding_window_helpers_match_reference_golden():
    """compute_gaussian / compute_steps_for_sliding_window: the oracle restatement AND the product's host logic reproduce the outputs
    of the reference's own functions (tests/golden/sliding_window.npz, written by oracle/make_golden_sw.py from
    dinounet/inference/sliding_window_prediction.py); window order as predict_from_raw_data.py:517-522; padding round trip."""
    from oracle import sliding_window_oracle as SW
    from dinounet_amd import inference as INF
    g = np.load(os.path.join(GOLD, "sliding_window.npz"))
    i = 0
    while f"steps{i}_args" in g:
        a = g[f"steps{i}_args"]
        img, tile, step = (int(a[0]), int(a[1])), (int(a[2]), int(a[3])), float(a[4])
        want = [g[f"steps{i}_ax0"].tolist(), g[f"steps{i}_ax1"].tolist()]
        assert SW.compute_steps(img, tile, step) == want
        assert INF.compute_steps_for_sliding_window(img, tile, step) == want
        i += 1
    assert i >= 5
    i = 0
    while f"gauss{i}_args" in g:
        a = g[f"gauss{i}_args"]
        tile, sig, val = (int(a[0]), int(a[1])), float(a[2]), float(a[3])
        want = torch.from_numpy(g[f"gauss{i}"])
        assert torch.equal(SW.compute_gaussian(tile, sig, val), want)
        assert torch.equal(INF.compute_gaussian(tile, sig, val), want)
        assert float(want.min()) > 0
        i += 1
    assert i >= 2
    # slices outermost, then the first-axis steps, then the second-axis steps
    assert INF.sliding_window_origins((2, 160, 200), (128, 128), 0.5) == [(d, y, x) for d in range(2) for y in (0, 32) for x in (0, 36, 72)]
    # images smaller than the patch: centred zero padding, odd pixel on the high side; the slices undo it
    x = torch.arange(2 * 3 * 5 * 7, dtype=torch.float32).view(2, 3, 5, 7)
    for pad_fn in (INF.pad_to_patch, SW.pad_nd_image_2d):
        p, (ys, xs) = pad_fn(x, (8, 8))
        assert p.shape == (2, 3, 8, 8) and (ys, xs) == (slice(1, 6), slice(0, 7)) and torch.equal(p[..., ys, xs], x)
        assert float(p.sum()) == float(x.sum())
        p2, (ys2, xs2) = pad_fn(x, (4, 4))
        assert p2.shape == x.shape and torch.equal(p2[..., ys2, xs2], x)


def test_sliding_window_oracle_blending_properties():
    """The blending itself, through size-independent properties: a predictor that returns a constant gives that constant everywhere
    (weights cancel); a linear predictor of the window's own pixels reproduces the image-wide linear map; fp16 accumulators (the
    reference's dtype) stay within fp16 rounding of the fp32 ones."""
    from oracle import sliding_window_oracle as SW
    torch.manual_seed(0)
    data = torch.randn(3, 2, 70, 90)
    const = SW.predict_sliding_window_logits(lambda w: torch.full((1, 4, *w.shape[-2:]), 2.5), data, (32, 48), 0.5)
    assert const.shape == (4, 2, 70, 90) and float((const - 2.5).abs().max()) < 1e-5
    A = torch.randn(4, 3)
    lin = SW.predict_sliding_window_logits(lambda w: torch.einsum("kc,bchw->bkhw", A, w), data, (32, 48), 0.5)
    assert float((lin - torch.einsum("kc,cdhw->kdhw", A, data)).abs().max()) < 1e-4
    half = SW.predict_sliding_window_logits(lambda w: torch.einsum("kc,bchw->bkhw", A, w), data, (32, 48), 0.5, accum_dtype=torch.float16)
    assert float((half.float() - lin).abs().max()) < 3e-2
    small = SW.predict_sliding_window_logits(lambda w: torch.einsum("kc,bchw->bkhw", A, w), data[..., :20, :30], (32, 48), 0.5)
    assert small.shape == (4, 2, 20, 30) and float((small - torch.einsum("kc,cdhw->kdhw", A, data[..., :20, :30])).abs().max()) < 1e-4


def test_compact_checkpoint_round_trip_and_reference_key_contract(tmp_path):
    """checkpoint.py: the compact file drops the frozen backbone and the `decoder.encoder.*` duplicates, and its
    expansion is exactly the dict the reference's load_checkpoint feeds to load_state_dict(strict): same keys in the same order as the
    reference module's state_dict (tests/golden/state_dict_dinounet_s.json), identical tensors, aliases sharing storage."""
    from dinounet_amd import checkpoint as CK
    from dinounet_amd.plans import PLANS_2D
    from dinounet_amd.network_architecture import DinoUNet
    torch.manual_seed(0)
    net = DinoUNet.from_config(PLANS_2D, 3, 2, dinov3_pretrained_path=None, dinov3_model_name="dinounet_s", precision="fp32")
    ks = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    net.load_state_dict(weights.make_state_dict(ks, seed=3), strict=True)
    params = [p for p in net.parameters() if p.requires_grad]
    opt = torch.optim.SGD(params, lr=1e-2, momentum=0.99, nesterov=True)
    for p in params[:5]:
        opt.state[p]["momentum_buffer"] = torch.randn_like(p)
    full = {k: v.clone() for k, v in net.state_dict().items()}
    compact, meta = CK.compact_state_dict(net)
    assert not any(k.startswith("decoder.encoder.") for k in compact)
    assert not any(k.startswith("encoder.dinov3_adapter.backbone.") for k in compact)          # the whole ViT is frozen
    assert all(k in compact for k in full if k.startswith("encoder.fapm.") or k.startswith("decoder.stages."))
    assert any(k.endswith("running_mean") for k in compact) and any(k.endswith("num_batches_tracked") for k in compact)
    ref_keys = [k for k, _, _ in json.load(open(os.path.join(GOLD, "state_dict_dinounet_s.json")))["keys"]]
    path = str(tmp_path / "ckpt.pth")
    CK.save_checkpoint(path, net, opt, current_epoch=7, _best_ema=0.5, trainer_name="DinoUNetTrainer_s", init_args={"fold": 0},
                       logging={"train_losses": [1.0]}, inference_allowed_mirroring_axes=None)
    torch.save({"network_weights": full}, str(tmp_path / "full.pth"))
    ratio = os.path.getsize(path) / os.path.getsize(str(tmp_path / "full.pth"))
    assert ratio < 0.2, ratio                                                                   # dinounet_s: 86 M frozen x 2 copies dropped
    # scramble the trainable part of the live module, then load the compact file back
    with torch.no_grad():
        for p in params:
            p.add_(1.0)
    opt2 = torch.optim.SGD(params, lr=1e-2, momentum=0.99, nesterov=True)
    ck = CK.load_checkpoint(path, net, opt2)
    assert ck["current_epoch"] == 7 and ck["trainer_name"] == "DinoUNetTrainer_s" and "network_weights_meta" not in ck
    assert list(ck["network_weights"].keys()) == ref_keys == list(full.keys())
    for k, v in net.state_dict().items():
        assert torch.equal(v, full[k]), k
    w = ck["network_weights"]
    assert w["decoder.encoder.fapm.shared_basis.weight"].data_ptr() == w["encoder.fapm.shared_basis.weight"].data_ptr()
    assert len(opt2.state_dict()["state"]) == 5
    # a different backbone is refused; a matching external backbone state dict is accepted
    bb = {k[len(CK.FROZEN_PREFIX):]: v.clone() for k, v in full.items() if k.startswith(CK.FROZEN_PREFIX)}
    ok = CK.expand_state_dict(compact, meta, backbone_state=bb)
    assert all(torch.equal(ok[k], full[k]) for k in full)
    bb["cls_token"] = bb["cls_token"] + 1
    with pytest.raises(ValueError):
        CK.expand_state_dict(compact, meta, backbone_state=bb)
    assert CK.expand_state_dict(compact, meta, backbone_state=bb, check=False)["encoder.dinov3_adapter.backbone.cls_token"] is bb["cls_token"]


def test_test_time_mirroring_matches_reference_golden():
    """Test-time mirroring: the oracle restatement AND the product's host logic (inference._mirror_and_predict around any forward) reproduce
    the outputs of the reference's own nnUNetPredictor._internal_maybe_mirror_and_predict (tests/golden/sliding_window_mirror.npz, written
    by oracle/make_golden_mirror.py from predict_from_raw_data.py:537-552 driving a small non-symmetric stand-in network)."""
    from oracle import sliding_window_oracle as SW
    from oracle.make_golden_mirror import toy_network
    from dinounet_amd import inference as INF
    g = np.load(os.path.join(GOLD, "sliding_window_mirror.npz"))
    x = torch.from_numpy(g["x"])
    i = 0
    while f"axes{i}" in g:
        axes = None if int(g[f"axes{i}"][0]) < 0 else tuple(int(a) for a in g[f"axes{i}"])
        want = torch.from_numpy(g[f"y{i}"])
        assert torch.allclose(SW.mirror_and_predict(toy_network, x.clone(), axes), want, rtol=0, atol=1e-6)
        combos = INF.mirror_axes_combinations(axes, x.ndim)
        assert len(combos) == (0 if axes is None else 2 ** len(axes) - 1)
        assert torch.allclose(INF._mirror_and_predict(toy_network, x.clone(), combos), want, rtol=0, atol=1e-6)
        i += 1
    assert i == 4
    assert not torch.allclose(torch.from_numpy(g["y0"]), torch.from_numpy(g["y3"]), atol=1e-3)      # mirroring changes the prediction


def test_gemm_dispatch_host_logic_without_gpu():
    """du_gemm's kernel-family choice (du_gemm_route: pure host logic of csrc/gemm*.hip, no launch) for the shapes of a dinounet_l
    512^2 batch-8 train step -- a regression guard for the dispatch heuristics the measured numbers in DESIGN.md / profiles/ rest on:
    0 generic, 1 bf16 128 x 128 engine, 2 direct-to-LDS 128 x 128, 3 / 4 multi-phase 256 x 256 / 256 x 128, 5 multi-phase weight-gradient."""
    import ctypes as C
    from dinounet_amd import _lib
    from dinounet_amd._lib import (DU_BF16, DU_F32, IM2COL_COL, IM2COL_ROW, PLAIN_COL, PLAIN_ROW, ConvGeom, GemmArgs)
    L = _lib.lib()

    def route(M, N, K, am=PLAIN_ROW, bm=PLAIN_ROW, dt=DU_BF16, od=DU_BF16, split=1, geom=None, lda=None, ldb=None, row_scale=False, act=0):
        a = GemmArgs()
        a.dtype, a.out_dtype, a.a_mode, a.b_mode = dt, od, am, bm
        a.M, a.N, a.K = M, N, K
        a.A, a.B, a.C = 0x100000, 0x200000, 0x300000          # aligned fake addresses: nothing is dereferenced
        a.lda = lda or (K if am == PLAIN_ROW else M)
        a.ldb = ldb or (K if bm == PLAIN_ROW else N)
        a.ldc = N
        a.batch, a.split_k, a.alpha = 1, split, 1.0
        a.act = act
        if row_scale:
            a.row_scale, a.rs_rows = 0x400000, 5376
        if geom is not None:
            a.geom = geom
        ws = int(L.du_gemm_ws_elems(C.byref(a)))
        if ws > 0:                                            # as ops.gemm_raw: the caller lends the scratch the product asks for -- du_gemm_route
            a.ws, a.ws_elems = 0x500000, ws                   # answers for the arguments as passed, and without it the ragged rows stay in the tile grid
        return int(L.du_gemm_route(C.byref(a))), ws

    # frozen ViT-L, M = 8 * 1029 tokens: 256 x 128 tiles for proj / fc2 (fp32 result + residual: one tile per CU); round 5: the PERSISTENT
    # 256 x 128 kernel (6) for the bf16 products whose narrow tiles come out at >= 2 per CU and cheaper than rounds of wide tiles -- qkv
    # (3 tiles against 2 rounds), fc1 with its GELU (4 against 2), ViT-B's K = 768 products; without the GELU the 8232 x 4096 x 1024 product
    # keeps 2 rounds of 256 x 256 tiles (3), and so do the big square products; the 40 ragged rows leave the tile grid
    ACT_GELU = 1
    assert route(8232, 3072, 1024)[0] == 6 and route(8232, 4096, 1024, act=ACT_GELU)[0] == 6 and route(8232, 2304, 768)[0] == 6
    assert route(8232, 4096, 1024)[0] == 3 and route(4096, 4096, 4096)[0] == 3 and route(131072, 512, 1024)[0] == 3
    assert route(8232, 1024, 4096, od=DU_F32)[0] == 4 and route(8232, 1024, 1024, od=DU_F32)[0] == 4
    assert route(8232, 3072, 1024)[1] > 0 and route(8192, 3072, 1024)[1] == 0
    try:                      # du_set_option(10, 0): the round-4 choice
        L.du_set_option(10, 0)
        assert route(8232, 3072, 1024)[0] == 3 and route(8232, 4096, 1024, act=ACT_GELU)[0] == 3 and route(8232, 2304, 768)[0] == 4
    finally:
        L.du_set_option(10, 1)
    # short contractions on tall products (round 5): the resident-weights streaming kernel (7) from 2^24 output elements up, K <= 192 --
    # the adapter's K = 192 data gradient, the SPM's 64 -> 1024 projection; small ones stay on the direct-to-LDS 128 x 128 kernel
    assert route(43008, 1024, 192)[0] == 7 and route(131072, 1024, 64)[0] == 7 and route(524288, 128, 64)[0] == 7
    assert route(32768, 256, 64)[0] == 2 and route(2048, 256, 256)[0] == 2 and route(43008, 1024, 256)[0] == 6 and route(131072, 512, 256)[0] == 7
    try:
        L.du_set_option(12, 0)
        assert route(43008, 1024, 192)[0] == 2 and route(131072, 1024, 64)[0] == 2
    finally:
        L.du_set_option(12, 1)
    assert route(43008, 1024, 512)[0] == 6 and route(43008, 1024, 256)[0] == 6 and route(43008, 192, 1024)[0] == 3
    # weight gradients: short splits stay on the 128 x 128 engine (atomics per workgroup), long ones go to the multi-phase TN form;
    # a DropPath row scale on the contraction rows is implemented by the 128 x 128 engine only
    assert route(1024, 512, 43008, PLAIN_COL, PLAIN_COL, od=DU_F32, split=16)[0] == 1
    assert route(512, 1024, 131072, PLAIN_COL, PLAIN_COL, od=DU_F32, split=16)[0] == 5
    assert route(512, 1024, 131072, PLAIN_COL, PLAIN_COL, od=DU_F32, split=16, row_scale=True)[0] == 1
    assert route(512, 1024, 131072, PLAIN_COL, PLAIN_COL, od=DU_F32, split=1)[0] == 1           # no split requested: C is not known to be zeroed
    # ConvTranspose2d k2 s2 1024 -> 1024 on a 64 x 64 grid (the adapter's `up`): both gradients gather dY in place on the multi-phase kernels
    g = ConvGeom()
    g.Hi, g.Wi, g.C, g.C1, g.KH, g.KW, g.stride, g.pad, g.Ho, g.Wo, g.transposed = 128, 128, 1024, 1024, 2, 2, 2, 0, 64, 64, 0
    assert route(32768, 1024, 4096, IM2COL_ROW, PLAIN_ROW, geom=g, lda=1024, ldb=4096)[0] == 3
    assert route(1024, 4096, 32768, PLAIN_COL, IM2COL_COL, od=DU_F32, split=4, geom=g, lda=1024, ldb=1024)[0] == 5
    g3 = ConvGeom()
    g3.Hi, g3.Wi, g3.C, g3.C1, g3.KH, g3.KW, g3.stride, g3.pad, g3.Ho, g3.Wo, g3.transposed = 512, 512, 64, 64, 3, 3, 2, 1, 256, 256, 0
    assert route(64, 576, 524288, PLAIN_COL, IM2COL_COL, od=DU_F32, split=64, geom=g3, lda=64, ldb=64)[0] == 1        # 3 x 3 im2col: no gather form
    # fp32 parity mode: the generic exact-fp32 kernel
    assert route(8232, 3072, 1024, dt=DU_F32, od=DU_F32)[0] == 0


def test_conv3x3_kernel_choice_host_logic_without_gpu():
    """Which 3x3 kernel serves a shape, and how many partial-statistics rows it writes (du_conv3x3_halo_parts: what the caller
    allocates) -- pure host logic of csrc/conv_strip.hip / conv_halo.hip.  Strip kernel: Cin in {32, 64 (one tensor or a 32 + 32 concat)},
    Cout in {32, 64}, W % 128 == 0, H % 8 == 0: one partial row per (image, row segment, 32-column strip); anything else: the LDS-tiled
    kernel's 8 x 16 tiles.  du_conv3x3_strip declines (DU_ERR_UNSUPPORTED) without touching the device."""
    from dinounet_amd import _lib
    L = _lib.lib()
    parts = lambda C1, Cin, Cout, B, H, W: int(L.du_conv3x3_halo_parts(C1, Cin, Cout, B, H, W))
    # dinounet_l decoder at batch 8: 512^2 32 -> 32 in 16-row... segments chosen for >= 512 workgroups: 8 x (512 / 128) x (512 / 32) => RS = 32
    assert parts(32, 32, 32, 8, 512, 512) == 8 * (512 // 32) * (512 // 32)
    assert parts(32, 64, 32, 8, 512, 512) == 8 * (512 // 64) * (512 // 32)          # concat 32 + 32: one workgroup per CU wanted => RS = 64
    assert parts(64, 64, 64, 8, 256, 256) == 8 * (256 // 16) * (256 // 32)          # 256 workgroups => RS = 16
    assert parts(32, 32, 32, 1, 8, 128) == 1 * 1 * 4                                 # a single 8-row segment
    assert parts(32, 32, 32, 2, 40, 384) == 2 * 4 * 12                               # 40 rows -> segments of 10
    # not served by the strip kernel: 8 x 16 tiles of the LDS-tiled kernel
    for C1, Cin, Cout, B, H, W in [(128, 128, 128, 8, 128, 128), (64, 128, 64, 8, 256, 256), (32, 32, 32, 2, 16, 48), (64, 64, 32, 2, 16, 32)]:
        assert parts(C1, Cin, Cout, B, H, W) == B * (H // 8) * (W // 16)
    assert parts(32, 32, 32, 1, 12, 128) == 0                                        # H % 8: neither kernel
    import ctypes as C
    args = (None, C.c_int64(128), None, C.c_int64(0), 128, 128, 128, 8, 128, 128, None, None, None, C.c_int64(128), None, None)
    assert int(L.du_conv3x3_strip(*args)) == -2                                      # DU_ERR_UNSUPPORTED, before any pointer is looked at
    # a 32-channel slice of a 512-channel-wide tensor at 1024^2 is a strip-kernel SHAPE (the partial-statistics buffer is sized
    # for strips) but a per-image input of 1 GiB, which the strip kernel declines on.  du_conv3x3_halo must then decline as a whole when
    # statistics are asked for -- the LDS-tiled kernel would write B * (H / 8) * (W / 16) rows into the smaller strip-sized buffer --
    # and it must do so before anything is launched (fake aligned addresses, no device here).
    assert parts(32, 32, 32, 2, 1024, 1024) != 2 * (1024 // 8) * (1024 // 16)
    big = (C.c_void_p(0x100000), C.c_int64(512), None, C.c_int64(0), 32, 32, 32, 2, 1024, 1024, C.c_void_p(0x200000), None,
           C.c_void_p(0x300000), C.c_int64(32), C.c_void_p(0x400000), None)
    assert int(L.du_conv3x3_strip(*big)) == -2
    assert int(L.du_conv3x3_halo(*big)) == -2
    # weight gradient: workgroups = partial slabs.  The round-5 kernel (two LDS stages) runs one workgroup per CU for everything but the
    # 32 -> 32 form (39 KB of LDS: two per CU); the round-3 kernel (du_set_option(13, 0)) went by slab size alone.  128 outputs: not served
    # (the grouped launch) unless option 13 = 2 (round 6, opt-in): the rows kernel with 128 workgroups (0.6-1.2 MB slabs).
    blocks = lambda C1, Cin, Cout, B, H, W: int(L.du_conv3x3_wgrad_halo_blocks(C1, Cin, Cout, B, H, W))
    try:
        assert blocks(32, 32, 32, 8, 512, 512) == 512 and blocks(32, 64, 32, 8, 512, 512) == 512      # (32 + 32 concat: 32-channel chunks)
        assert blocks(64, 64, 64, 8, 256, 256) == 256 and blocks(64, 128, 64, 8, 256, 256) == 256 and blocks(64, 64, 32, 8, 512, 512) == 256
        assert blocks(32, 32, 64, 8, 256, 256) == 256
        assert blocks(32, 32, 32, 1, 16, 32) == 4                                                         # fewer tiles than workgroups
        assert blocks(128, 128, 128, 8, 128, 128) == 0 and blocks(32, 32, 32, 1, 12, 128) == 0
        L.du_set_option(13, 2)
        assert blocks(128, 128, 128, 8, 128, 128) == 128 and blocks(128, 256, 128, 8, 128, 128) == 128 and blocks(128, 128, 128, 1, 8, 16) == 1
        assert blocks(128, 384, 128, 8, 128, 128) == 0 and blocks(64, 64, 64, 8, 256, 256) == 256
        L.du_set_option(13, 0)
        assert blocks(128, 128, 128, 8, 128, 128) == 0
        assert blocks(64, 64, 32, 8, 512, 512) == 512 and blocks(32, 32, 64, 8, 256, 256) == 512 and blocks(64, 64, 64, 8, 256, 256) == 256
    finally:
        L.du_set_option(13, 1)


def test_bench_roofline_reads_pmc_summaries_only_for_matching_kernel_sources(monkeypatch):
    """roofline.traffic / roofline.pmc_cycles come from committed rocprofv3 PMC summaries (counters cannot be collected inside the timed
    process); each summary names the digest of the kernel sources it was measured on, and bench.py must ignore a summary taken on other
    sources (traffic stays absent, with a note) instead of reporting stale bytes."""
    import importlib.util
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    from dinounet_amd import _build
    newest = [f for f in (os.path.join(root, "profiles", f"{r}_pmc_fetch_size_eager.txt") for r in bench.PMC_ROUNDS) if os.path.exists(f)][0]
    head = open(newest).read().splitlines()[0]
    recorded = re.match(r"# csrc-digest ([0-9a-f]{64})", head).group(1)
    kernel = "gemm_nt_p8n_kernel<bf16,linear>"

    monkeypatch.setattr(_build, "_digest", lambda: recorded)
    roof = {"kernel": kernel}
    bench.pmc_traffic(roof)
    bench.pmc_cycles(roof)
    assert isinstance(roof["traffic"], int) and 5e7 < roof["traffic"] < 1e9 and recorded[:12] in roof["traffic_source"]
    pc = roof["pmc_cycles"]
    assert 0.0 < pc["matrix_pipe_busy"] < 1.0 and abs(pc["waves_parked"] + pc["waves_issue_stalled"] + pc["waves_issuing"] - 1.0) < 0.05

    monkeypatch.setattr(_build, "_digest", lambda: "0" * 64)
    roof = {"kernel": kernel}
    bench.pmc_traffic(roof)
    bench.pmc_cycles(roof)
    assert "traffic" not in roof and "digest mismatch" in roof["traffic_note"] and "pmc_cycles" not in roof


def test_launch_count_tool_finds_the_replayed_step_not_a_sub_period(tmp_path):
    """tools/rocpd_counts.py: the kernel trace of bench.py holds eager warm-up steps with one-time work beside the replayed steps, and a
    network of identical blocks has windows SHORTER than a step whose kernel multisets agree several times in a row (round 3: 823 and 845
    were found before the true 867).  The period must come from the once-per-step kernels."""
    import sqlite3
    import subprocess
    import sys
    block = ["ln", "qkv", "rope", "attn", "proj", "ln", "fc1", "fc2", "tail_a", "tail_b"]
    step = ["prep"] + block * 24 + [f"dec{i % 7}" for i in range(60)] + ["loss", "sgd"]
    names = []
    for w in range(3):                                     # warm-up: the step + first-use work
        names += step + [f"init{w}_{i}" for i in range(40 + 13 * w)]
    names += step * 10 + ["readback"]
    db = tmp_path / "trace.db"
    c = sqlite3.connect(db)
    c.execute("create table kernels(name text, start int, end int)")
    c.executemany("insert into kernels values(?,?,?)", [(n, 1000 * i, 1000 * i + 700) for i, n in enumerate(names)])
    c.commit(); c.close()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "rocpd_counts.py"), str(db), "13"], capture_output=True, text=True, check=True).stdout
    assert f"steady state: {len(step)} dispatches per replayed step" in out.splitlines()[0], out[:300]
    assert "  24.0/step" in out and "   1.0/step" in out
