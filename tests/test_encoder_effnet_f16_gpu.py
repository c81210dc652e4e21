"""The "f16" inference arithmetic of the EfficientNet encoder (bev_native.conv_arith_mode("f16"), efficientnet_b0 /
b3, out_index 2): fp16 storage from the stem to the trunk output -- what the reference's validation forward computes
in eval() under autocast(float16) on its shipped backbone (configs/wildtrack.yaml, train.py:285-286).

Rounding points (the ones the float64 restatement R64 below reproduces): the BN-folded weights of the expansion,
depthwise, projection and proj convs once (folded in fp32 first); the stem's fp32 result after SiLU; the expanded
tensor after SiLU; the depthwise output after SiLU; the projection's operand f16(y * gate) with the gate computed in
fp32-class arithmetic from the means of the STORED depthwise output; the projection's output after bias + skip; the
encoder proj reads the fp16 trunk output with fp16 weights and writes fp32, unrounded.

(i)   the fp16 trunk output is BITWISE the test's own per-layer composition through the public wrappers
      (conv2d_stem3_h16, dwconv2d_nhwc_h16, ir_expand_dw_h16, se_gate, conv2d_pw_h16): gate, skip and partial-count wiring;
(ii)  end to end against float64: the native error is within 1.5x (relative L2) / 2x (max) of the error R64 itself has
      against the exact float64 forward (on the CPU, an fp32-accumulating restatement of the whole b0 / b3 encoder with
      a 64-channel proj measured L2 ratios 0.997-1.005 and max ratios 0.888-1.009 at these sizes; R64's own relative L2
      2.6-2.8e-4);
(iii) the default mode's output is bitwise the same before and after a forward in "f16";
(iv)  out_index 3 under "f16" is the default arithmetic: fp32, equal to the default output;
(v)   one BEVNet forward in the mode, with the noise-referenced heatmap bound of test_encoder_f16_gpu.py.
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
NAMES = ["efficientnet_b0", "efficientnet_b3"]
_ENC, _REF = {}, {}


def _randomise_bn(module, seed):
    g = torch.Generator().manual_seed(seed)
    for m in module.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.uniform_(-0.2, 0.2, generator=g)
            m.running_var.uniform_(0.5, 1.5, generator=g)
            m.weight.data.uniform_(0.5, 1.5, generator=g)
            m.bias.data.uniform_(-0.2, 0.2, generator=g)


def _encoder(name, out_index=2):
    """One CNNEncoder per backbone and index (BN statistics randomised, proj materialised), shared by the tests."""
    k = (name, out_index)
    if k not in _ENC:
        from models.encoders.cnn_encoder import CNNEncoder
        torch.manual_seed(11)
        enc = CNNEncoder(out_channels=64, backbone=name, pretrained=False, out_index=out_index)
        _randomise_bn(enc, 5)
        enc = enc.eval().to(DEV)
        with torch.no_grad():
            enc(_images(SIZES[0]))  # the lazy proj
        _ENC[k] = enc
    return _ENC[k]


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


def _blocks(bb, out_index=2):
    from models.encoders.efficientnet import FEATURE_STAGE
    return [blk for si in range(FEATURE_STAGE[out_index] + 1) for blk in bb.blocks[si]]


def _parts(blk):
    """(expansion conv, bn) or None, (depthwise conv, bn), (projection conv, bn) of a block."""
    from models.encoders.efficientnet import DepthwiseSeparableConv
    if isinstance(blk, DepthwiseSeparableConv):
        return None, (blk.conv_dw, blk.bn1), (blk.conv_pw, blk.bn2)
    return (blk.conv_pw, blk.bn1), (blk.conv_dw, blk.bn2), (blk.conv_pwl, blk.bn3)


def _compose_native(bb, x):
    """The trunk in the f16 arithmetic, layer by layer through the public wrappers, with the test's own folding."""
    import bev_native as nat
    with torch.no_grad():
        w, b = _fold(bb.conv_stem, bb.bn1, torch.float32, DEV)
        y = nat.conv2d_stem3_h16(x, w.permute(1, 2, 3, 0).reshape(27, -1).contiguous(), b.contiguous(), nat.ACT_SILU)
        for blk in _blocks(bb):
            exp, (dw, bnd), (pw, bnp) = _parts(blk)
            K, S = dw.kernel_size[0], dw.stride[0]
            wd, bd = _fold(dw, bnd, torch.float32, DEV)
            wd16 = wd.reshape(wd.shape[0], K * K).t().half().contiguous()
            if exp is None:
                z, ps = nat.dwconv2d_nhwc_h16(y, wd16, bd.contiguous(), K, S, K // 2, nat.ACT_SILU, want_psum=True)
            else:
                we, be = _fold(exp[0], exp[1], torch.float32, DEV)
                z, ps = nat.ir_expand_dw_h16(y, we.reshape(we.shape[0], -1).half().contiguous(), be.contiguous(), wd16,
                                             bd.contiguous(), K, S)
            se = blk.se
            gate = nat.se_gate(ps, z.shape[1] * z.shape[2], se.conv_reduce.weight.detach().reshape(se.conv_reduce.out_channels, -1),
                               se.conv_reduce.bias.detach(), se.conv_expand.weight.detach().reshape(se.conv_expand.out_channels, -1),
                               se.conv_expand.bias.detach())
            wp, bp = _fold(pw, bnp, torch.float32, DEV)
            y = nat.conv2d_pw_h16(z, wp.reshape(wp.shape[0], -1).half().contiguous(), bp.contiguous(), gate=gate,
                                  residual=y if blk.has_skip else None)
    return y


def _silu(z):
    return z * torch.sigmoid(z)


def _forward64(enc, x, rounded):
    """float64 forward of the folded encoder on the CPU.  rounded = False: exact.  True: R64 -- the rounding points of
    the module docstring, float64 sums."""
    bb = enc.backbone
    h16 = (lambda t: t.half().double()) if rounded else (lambda t: t)

    def folded(conv, bn):
        if rounded:
            w, b = _fold(conv, bn, torch.float32, "cpu")
            return w.half().double(), b.double()
        return _fold(conv, bn, torch.float64, "cpu")

    with torch.no_grad():
        w, b = _fold(bb.conv_stem, bb.bn1, torch.float64, "cpu")  # the stem's arithmetic is fp32: weights unrounded
        y = h16(_silu(F.conv2d(x.double().cpu(), w, b, 2, 1)))
        for blk in _blocks(bb):
            exp, (dw, bnd), (pw, bnp) = _parts(blk)
            z = y
            if exp is not None:
                z = h16(_silu(F.conv2d(z, *folded(*exp))))
            wd, bd = folded(dw, bnd)
            z = h16(_silu(F.conv2d(z, wd, bd, dw.stride, dw.padding, groups=dw.groups)))
            se = blk.se
            r = _silu(F.conv2d(z.mean((2, 3), keepdim=True), se.conv_reduce.weight.detach().double().cpu(),
                               se.conv_reduce.bias.detach().double().cpu()))
            gate = torch.sigmoid(F.conv2d(r, se.conv_expand.weight.detach().double().cpu(),
                                          se.conv_expand.bias.detach().double().cpu()))
            if rounded:
                gate = gate.float().double()  # the gate is stored in fp32
            out = F.conv2d(h16(z * gate), *folded(pw, bnp))
            y = h16(out + y if blk.has_skip else out)
        if rounded:
            wp, bp = enc.proj.weight.detach().cpu().half().double(), enc.proj.bias.detach().cpu().double()
        else:
            wp, bp = enc.proj.weight.detach().cpu().double(), enc.proj.bias.detach().cpu().double()
        y = F.conv2d(y, wp, bp)
    return y  # NCHW float64


def _refs(name, si):
    k = (name, si)
    if k not in _REF:
        enc = _encoder(name)
        x = _images(SIZES[si])
        _REF[k] = dict(x=x, exact=_forward64(enc, x, False), r64=_forward64(enc, x, True),
                       composed=_compose_native(enc.backbone, x))
    return _REF[k]


@pytest.mark.parametrize("si", [0, 1], ids=["96x160", "70x118"])
@pytest.mark.parametrize("name", NAMES)
def test_f16_trunk_is_bitwise_the_per_layer_composition(name, si):
    import bev_native as nat
    ref = _refs(name, si)
    bb = _encoder(name).backbone
    assert bb.f16_applies(2)
    with torch.no_grad(), nat.conv_arith_mode("f16"):
        y = bb.forward_features_nhwc(ref["x"], 2)
    torch.cuda.synchronize()
    assert y.dtype == torch.float16 and y.shape == ref["composed"].shape
    assert bool(torch.isfinite(y).all())
    assert torch.equal(y, ref["composed"]), int((y != ref["composed"]).sum())


def _rel_l2(a, b):
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("si", [0, 1], ids=["96x160", "70x118"])
@pytest.mark.parametrize("name", NAMES)
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


@pytest.mark.parametrize("name", NAMES)
def test_default_output_unchanged_by_a_forward_in_f16(name):
    import bev_native as nat
    enc, x = _encoder(name), _images(SIZES[0])
    with torch.no_grad():
        before = enc(x).clone()
        with nat.conv_arith_mode("f16"):
            half = enc(x).clone()
            trunk16 = enc.backbone.forward_features_nhwc(x, 2)
        after = enc(x).clone()
        trunk32 = enc.backbone.forward_features_nhwc(x, 2)
    assert before.dtype == half.dtype == torch.float32 and before.shape == half.shape
    assert trunk16.dtype == torch.float16 and trunk32.dtype == torch.float32
    assert torch.equal(before, after)  # the fp16 weights did not replace the default mode's
    assert not torch.equal(before, half)


def test_out_index_3_keeps_the_default_arithmetic():
    import bev_native as nat
    enc, x = _encoder("efficientnet_b0", 3), _images(SIZES[0])
    assert not enc.backbone.f16_applies(3)
    with torch.no_grad():
        base = enc(x).clone()
        with nat.conv_arith_mode("f16"):
            trunk = enc.backbone.forward_features_nhwc(x, 3)
            half = enc(x).clone()
    assert trunk.dtype == torch.float32 and half.dtype == torch.float32
    assert torch.equal(base, half)


def test_f16_bevnet_forward_efficientnet_b0():
    """One BEVNet eval forward (the bevnet_small fixture's geometry and images, native efficientnet_b0 encoder) in the
    f16 arithmetic: finite, same shapes, and the heatmap follows the default-mode forward within the noise-referenced
    bound of test_encoder_f16_gpu.py::test_f16_bevnet_forward: the heatmap may move by 1.5x (relative L2) / 2x (max)
    of what white noise of the feature difference's RMS, added to the default features, moves it."""
    import bev_native as nat
    from models.model_wrapper import BEVNet
    d = np.load(os.path.join(GOLDEN, "bevnet_small.npz"))
    cfg = json.loads(str(d["cfg"]))
    cfg["MODEL"]["BACKBONE_IMPL"] = "native"
    cfg["MODEL"]["BACKBONE"] = "efficientnet_b0"
    cfg["MODEL"]["OUT_INDEX"] = 2
    torch.manual_seed(3)
    net = BEVNet(cfg)
    _randomise_bn(net, 9)
    net = net.to(DEV).eval()
    batch = {"images": torch.from_numpy(d["images"]).to(DEV),
             "calib": {"intrinsic": torch.from_numpy(d["K"]).to(DEV), "extrinsic": torch.from_numpy(d["Rt"]).to(DEV)}}
    with torch.no_grad():
        net(batch)  # lazy proj / detector
        base = net(batch)
        feats = net.encoder(batch["images"]).clone()
        with nat.conv_arith_mode("f16"):
            assert net.encoder.backbone.forward_features_nhwc(batch["images"][0], 2).dtype == torch.float16
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
