"""The "f16" inference arithmetic of the ResNet encoder (bev_native.set_conv_arith("f16")): fp16 weights and fp16
activations from layer to layer on the fp16 matrix cores, fp32 accumulation -- what the reference's validation
forward computes in eval() under autocast(float16) (train.py:285-286), with the stem kept fp32-class.

Rounding points (the ones the CPU restatement R64 below reproduces): the BN-folded weights once (the pack); the
operand of every trunk conv (the fp32 stem + max-pool output is rounded as layer1 reads it; everything after is stored
in fp16); every trunk conv's output once, after bias + residual + ReLU; the proj reads the fp16 trunk output with
fp16 weights and writes fp32.

(e) the mode switch and that panels do not leak between modes;
(f) the trunk output is BITWISE the test's own composition of the fp32-output fp16 kernel (conv2d_h16_any) per layer
    with .half() after each, in the plain block order -- with 1 and 2 stream groups, even and odd image sizes;
(g) end to end against float64: the native error is within 1.5x (relative L2) / 2x (max) of the error R64 itself has
    against the exact float64 forward -- the margins cover fp32 summation-order flips of roundings, nothing more
    (on the CPU, an fp32-accumulating restatement measured 0.99-1.00x and 0.86-1.25x);
(h) one BEVNet forward in the mode.
"""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(2, 3, 96, 160), (3, 3, 70, 118)]
_ENC, _REF = {}, {}


def _encoder(name):
    """One CNNEncoder per backbone (BN statistics randomised, proj materialised), shared by the tests."""
    if name not in _ENC:
        from models.encoders.cnn_encoder import CNNEncoder
        torch.manual_seed(11)
        enc = CNNEncoder(out_channels=64, backbone=name, pretrained=False, out_index=2)
        g = torch.Generator().manual_seed(5)
        for m in enc.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.uniform_(-0.2, 0.2, generator=g)
                m.running_var.uniform_(0.5, 1.5, generator=g)
                m.weight.data.uniform_(0.5, 1.5, generator=g)
                m.bias.data.uniform_(-0.2, 0.2, generator=g)
        enc = enc.eval().to(DEV)
        with torch.no_grad():
            enc(_images(SIZES[0]))  # the lazy proj
        _ENC[name] = enc
    return _ENC[name]


def _images(size):
    return torch.randn(*size, generator=torch.Generator().manual_seed(size[2])).to(DEV)


def _fold(conv, bn, dtype, device):
    """conv + eval BN -> (w OIHW, b) in `dtype` (fp32: the operation order of the package's fold)."""
    w = conv.weight.detach().to(device=device, dtype=dtype)
    b = (conv.bias.detach().to(device=device, dtype=dtype) if conv.bias is not None
         else torch.zeros(w.shape[0], device=device, dtype=dtype))
    if bn is not None:
        scale = bn.weight.detach().to(device, dtype) / torch.sqrt(bn.running_var.detach().to(device, dtype) + bn.eps)
        w = w * scale.view(-1, 1, 1, 1)
        b = bn.bias.detach().to(device, dtype) + (b - bn.running_mean.detach().to(device, dtype)) * scale
    return w, b


def _blocks(rn):
    return [blk for layer in (rn.layer1, rn.layer2) for blk in layer]


def _compose_native(rn, x):
    """The trunk in the f16 arithmetic from the fp32-output kernel: .half() after every conv, plain block order."""
    import bev_native as nat
    with torch.no_grad():
        y = rn.forward_features_nhwc(x, 0)  # the stem (default arithmetic, fp32)
        y = nat.maxpool_nhwc(y, 3, 2, 1)

        def conv(conv_m, bn, t, relu, residual=None):
            w, b = _fold(conv_m, bn, torch.float32, DEV)
            z = nat.conv2d_h16_any(t, nat.pack_conv_weight_h16(w.contiguous()), w.shape[0], w.shape[2], w.shape[3],
                                   conv_m.stride[0], conv_m.padding[0], bias=b.contiguous(),
                                   residual=None if residual is None else residual.float())
            return (torch.relu(z) if relu else z).half()

        for blk in _blocks(rn):
            sc = conv(blk.downsample[0], blk.downsample[1], y, False) if blk.downsample is not None else y.half()
            h = y
            chain = blk.convs()
            for idx, (c, bn, relu) in enumerate(chain):
                h = conv(c, bn, h, relu, residual=sc if idx == len(chain) - 1 else None)
            y = h
    return y


def _forward64(enc, x, rounded):
    """float64 forward of the folded encoder on the CPU.  rounded = False: exact.  True: R64 -- fp16-rounded folded
    weights (folded in fp32 first, as the pack sees them), conv operands and conv outputs rounded to fp16 at the
    points listed in the module docstring, float64 sums, the stem unrounded."""
    rn = enc.backbone
    h16 = (lambda t: t.half().double()) if rounded else (lambda t: t)

    def conv(conv_m, bn, t, relu, residual=None, round_out=True):
        if rounded:
            w, b = _fold(conv_m, bn, torch.float32, "cpu")
            w, b = w.half().double(), b.double()
        else:
            w, b = _fold(conv_m, bn, torch.float64, "cpu")
        z = F.conv2d(h16(t), w, b, conv_m.stride, conv_m.padding)
        if residual is not None:
            z = z + residual
        if relu:
            z = z.clamp_min(0)
        return h16(z) if round_out else z

    with torch.no_grad():
        w, b = _fold(rn.conv1, rn.bn1, torch.float64, "cpu")
        y = F.conv2d(x.double().cpu(), w, b, 2, 3).clamp_min(0)
        y = F.max_pool2d(y, 3, 2, 1)
        for blk in _blocks(rn):
            sc = conv(blk.downsample[0], blk.downsample[1], y, False) if blk.downsample is not None else h16(y)
            h = y
            chain = blk.convs()
            for idx, (c, bn, relu) in enumerate(chain):
                h = conv(c, bn, h, relu, residual=sc if idx == len(chain) - 1 else None)
            y = h
        y = conv(enc.proj, None, y, False, round_out=False)
    return y  # NCHW float64


def _refs(name, si):
    k = (name, si)
    if k not in _REF:
        enc = _encoder(name)
        x = _images(SIZES[si])
        exact, r64 = _forward64(enc, x, False), _forward64(enc, x, True)
        _REF[k] = dict(x=x, exact=exact, r64=r64, composed=_compose_native(enc.backbone, x))
    return _REF[k]


def test_f16_mode_switch_and_default_output_unchanged():
    import bev_native as nat
    assert "f16" in nat.CONV_ARITHS and nat.conv_arith() == "bf16x6"
    with pytest.raises(ValueError):
        nat.set_conv_arith("f8")
    prev = nat.set_conv_arith("f16")
    assert prev == "bf16x6" and nat.conv_arith() == "f16"
    assert nat.set_conv_arith(prev) == "f16"
    with nat.conv_arith_mode("f32"):
        with nat.conv_arith_mode("f16"):
            assert nat.conv_arith() == "f16"
        assert nat.conv_arith() == "f32"
    assert nat.conv_arith() == "bf16x6"
    enc, x = _encoder("resnet50"), _images(SIZES[0])
    with torch.no_grad():
        before = enc(x).clone()
        with nat.conv_arith_mode("f16"):
            half = enc(x).clone()
        after = enc(x).clone()
    assert before.dtype == half.dtype == torch.float32 and before.shape == half.shape
    assert torch.equal(before, after)  # the f16 panels did not replace the default mode's
    assert not torch.equal(before, half)


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("si", [0, 1], ids=["96x160", "70x118"])
@pytest.mark.parametrize("name", ["resnet50", "resnet18"])
def test_f16_trunk_is_bitwise_the_per_layer_composition(name, si, groups):
    import bev_native as nat
    ref = _refs(name, si)
    rn = _encoder(name).backbone
    old = rn.stream_groups
    rn.stream_groups = groups
    try:
        with torch.no_grad(), nat.conv_arith_mode("f16"):
            y = rn.forward_features_nhwc(ref["x"], 2)
        torch.cuda.synchronize()
    finally:
        rn.stream_groups = old
    assert y.dtype == torch.float16 and y.shape == ref["composed"].shape
    assert torch.equal(y, ref["composed"]), int((y != ref["composed"]).sum())


def _rel_l2(a, b):
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("si", [0, 1], ids=["96x160", "70x118"])
@pytest.mark.parametrize("name", ["resnet50", "resnet18"])
def test_f16_encoder_error_within_the_float64_restatement(name, si):
    import bev_native as nat
    ref = _refs(name, si)
    enc = _encoder(name)
    with torch.no_grad(), nat.conv_arith_mode("f16"):
        y = enc(ref["x"])  # [1, N, C, Hf, Wf] fp32
    assert y.dtype == torch.float32
    got = y[0].double().cpu()
    exact, r64 = ref["exact"], ref["r64"]
    assert got.shape == exact.shape
    l2n, l2r = _rel_l2(got, exact), _rel_l2(r64, exact)
    mxn, mxr = float((got - exact).abs().max()), float((r64 - exact).abs().max())
    print(f"{name} {SIZES[si]}: relL2 native {l2n:.3e} R64 {l2r:.3e} ratio {l2n / l2r:.3f}; "
          f"max native {mxn:.3e} R64 {mxr:.3e} ratio {mxn / mxr:.3f}")
    assert l2r > 1e-5  # the restatement does round
    assert l2n <= 1.5 * l2r
    assert mxn <= 2.0 * mxr


def test_f16_bevnet_forward():
    """One BEVNet eval forward (the bevnet_small fixture's geometry and images, native ResNet-18 encoder) in the f16
    arithmetic: finite, same shapes, and the heatmap follows the default-mode forward.

    Derived bound: between the two modes the heatmap's only input that changes is the encoder feature tensor, by
    d = feats_f16 - feats_default.  (g) bounds the f16 features' error at 1.5x (relative L2) and 2x (max) of what the
    fp16 roundings alone cause; so the heatmap may move by 1.5x (relative L2) / 2x (max) of what a perturbation of
    the features with the size of d moves it.  That reference movement is measured here by running everything after
    the encoder on feats_default + white noise of d's RMS (fixed seed)."""
    import bev_native as nat
    from models.model_wrapper import BEVNet
    d = np.load(os.path.join(GOLDEN, "bevnet_small.npz"))
    cfg = json.loads(str(d["cfg"]))
    cfg["MODEL"]["BACKBONE_IMPL"] = "native"
    torch.manual_seed(3)
    net = BEVNet(cfg).to(DEV).eval()
    batch = {"images": torch.from_numpy(d["images"]).to(DEV),
             "calib": {"intrinsic": torch.from_numpy(d["K"]).to(DEV), "extrinsic": torch.from_numpy(d["Rt"]).to(DEV)}}
    with torch.no_grad():
        net(batch)  # lazy proj / detector
        base = net(batch)
        feats = net.encoder(batch["images"]).clone()
        with nat.conv_arith_mode("f16"):
            half = net(batch)
            feats16 = net.encoder(batch["images"]).clone()
        delta = feats16 - feats
        noise = torch.randn(feats.shape, generator=torch.Generator().manual_seed(1)).to(DEV) * delta.pow(2).mean().sqrt()
        # in the encoder's layout: a channels-last view of an NHWC buffer
        noisy = (feats.permute(0, 1, 3, 4, 2).contiguous() + noise.permute(0, 1, 3, 4, 2)).permute(0, 1, 4, 2, 3)
        enc_forward = net.encoder.forward
        net.encoder.forward = lambda images: noisy
        try:
            pert = net(batch)
        finally:
            net.encoder.forward = enc_forward
    for k in ("heatmap", "heatmap_logits", "offset", "size", "bev_feat"):
        assert half[k].shape == base[k].shape and bool(torch.isfinite(half[k]).all()), k
    assert float(delta.abs().max()) > 0
    hb, hh, hp = base["heatmap"].double(), half["heatmap"].double(), pert["heatmap"].double()
    l2h, l2p = _rel_l2(hh, hb), _rel_l2(hp, hb)
    mxh, mxp = float((hh - hb).abs().max()), float((hp - hb).abs().max())
    print(f"features relL2 {_rel_l2(feats16.double(), feats.double()):.3e}; heatmap relL2 f16 {l2h:.3e} noise {l2p:.3e} "
          f"ratio {l2h / l2p:.3f}; max f16 {mxh:.3e} noise {mxp:.3e} ratio {mxh / mxp:.3f}")
    assert l2h <= 1.5 * l2p
    assert mxh <= 2.0 * mxp
