"""The "f16" inference arithmetic of the BEV detection head (bev_native.head_arith_mode("f16")) -- what the reference's
validation forward computes for BEVDetector in eval() under autocast(float16) (train.py:285-286).

With W1..W3 the stem convs (dilation 1, 2, 1), Wh / bh the concatenated 128 -> 5 conv and x the fp32 NHWC operand:

    z_i = f16( sum f16(a_{i-1}) f16(W_i) )                       fp32 accumulation; a_0 = x, rounded while staging
    (scale_i, shift_i) = GroupNorm(32) affine of the STORED fp16 z_i (double sums, biased variance, fp32 results)
    a_i = f16( max( float(z_i) scale_i + shift_i, 0 ) )          one fp32 multiply, one fp32 add; formed in the NEXT
                                                                 conv's operand loader, never written
    y   = sum a_3 f16(Wh) + bh                                   fp32, not rounded

(a) the conv with the affine in its loader == the same conv on the materialised groupnorm_apply_half operand, bitwise,
    with the buffer-load and the pointer staging (CONV_H16_BUF 1 / 0 -- CONV_H16_KERNEL selects tile widths, not the
    staging form), fp16 and fp32 output;
(b) GroupNorm statistics of an fp16-stored map == those of the upcast map, bitwise;
(c) the f16 head == its composition from the AMP training primitives, bitwise;
(d) against float64: the native error is within 1.5x (relative L2) / 2x (max) of the error the restatement R64 of the
    arithmetic above (float64 sums, the roundings listed) has against the exact float64 head -- the encoder test's
    margins, which cover fp32 summation order flipping a rounding and nothing more (an fp32-accumulating CPU stand-in
    measured 0.993-1.012 and 0.96-1.25 on these shapes);
(e) the switch: panels do not leak between modes, the trunk's switch does not touch the head;
(f) one BEVNet eval forward in the mode.
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
GROUPS = 32


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- (a) ---------------------------------------------------------------------------------------------------------------
#        N  H   W   Ci   Co  dil  what
CASES = [(5, 5, 7, 64, 128, 1),    # Ho Wo = 35: a 128-row tile spans four images; ragged last tile
         (2, 9, 13, 512, 128, 2),  # the channel offset wraps per tap (8 K steps each); border taps at distance 2
         (3, 6, 10, 128, 5, 1),    # fp32 output in an 8-wide buffer; the 64-column tile
         (1, 1, 1, 128, 64, 1),    # every tap but the centre is padding
         (2, 4, 5, 1024, 8, 1)]    # Ci above the kernel's constant table: every row reads its constants from memory
IDS = ["5x5x7_c64", "2x9x13_c512_d2", "3x6x10_co5", "1x1x1", "2x4x5_c1024"]


def _affine_case(case, seed):
    N, H, W, Ci, Co, dil = case
    g = _gen(seed)
    x16 = torch.randn(N, H, W, Ci, generator=g).half().to(DEV)
    scale = torch.randn(N, Ci, generator=g).to(DEV)                  # both signs
    shift = (torch.randn(N, Ci, generator=g) * 0.5 + 0.5).to(DEV)    # positive for most channels: relu(shift) > 0
    w = (torch.randn(Co, Ci, 3, 3, generator=g) * 0.05).to(DEV)
    bias = torch.randn(Co, generator=g).to(DEV)
    return x16, scale, shift, w, bias


@pytest.mark.parametrize("buf", [1, 0], ids=["buffer", "pointer"])
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_affine_loader_is_bitwise_the_materialised_operand(ci, buf):
    import bev_native as nat
    case = CASES[ci]
    N, H, W, Ci, Co, dil = case
    x16, scale, shift, w, bias = _affine_case(case, 100 + ci)
    packed = nat.pack_conv_weight_h16(w)
    for relu in ((True, False) if ci == 0 else (True,)):
        a16 = nat.groupnorm_apply_half(x16.float(), scale, shift, relu)
        assert float(a16[:, 0, 0].float().abs().max()) > 0
        for y_half in ((True, False) if Co % 8 == 0 else (False,)):
            ldy = Co if y_half else (Co + 7) // 8 * 8 + (0 if Co % 8 else 8)
            dt = torch.float16 if y_half else torch.float32
            with nat.tuned(CONV_H16_BUF=buf):
                out = torch.full((N, H, W, ldy), 7.0, device=DEV, dtype=dt)
                got = nat.conv2d_h16_affine(x16, packed, bias, Co, 3, dil, dil, in_scale=scale, in_shift=shift,
                                            in_relu=relu, y_half=y_half, out=out)
                ref = nat.conv2d_h16_affine(a16, packed, bias, Co, 3, dil, dil, y_half=y_half)
            torch.cuda.synchronize()
            assert got.dtype == dt and bool(torch.isfinite(got.float()).all())
            assert torch.equal(got[..., :Co], ref), (relu, y_half, int((got[..., :Co] != ref).sum()))
            assert bool((got[..., Co:] == 7.0).all())  # the channels past Co of a wider buffer are not written
            if y_half:  # ... and the fp16 output is the fp32 output rounded once
                assert torch.equal(ref, nat.conv2d_h16_any(a16, packed, Co, 3, 3, 1, dil, bias=bias,
                                                           dilation=dil).half())


def test_affine_conv_tile_widths_agree():
    """CONV_H16_KERNEL 2 / 3 (128- / 64-column tiles always) give the default's bits with the affine too."""
    import bev_native as nat
    case = CASES[0]
    x16, scale, shift, w, bias = _affine_case(case, 7)
    packed = nat.pack_conv_weight_h16(w)
    outs = []
    for kern in (0, 2, 3):
        with nat.tuned(CONV_H16_KERNEL=kern):
            outs.append(nat.conv2d_h16_affine(x16, packed, bias, case[4], 3, 1, 1, in_scale=scale, in_shift=shift,
                                              in_relu=True, y_half=True))
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_affine_conv_refuses_what_it_cannot_take():
    import bev_native as nat
    x16, scale, shift, w, bias = _affine_case(CASES[0], 1)
    packed = nat.pack_conv_weight_h16(w)
    with pytest.raises(nat.HipError):  # the affine needs the fp16-stored operand
        nat.conv2d_h16_affine(x16.float(), packed, bias, 128, 3, 1, 1, in_scale=scale, in_shift=shift)
    with pytest.raises(nat.HipError):
        nat.conv2d_h16_affine(x16, packed, bias, 128, 3, 1, 1, in_scale=scale)
    with pytest.raises(nat.HipError):  # Ci % 64
        nat.conv2d_h16_affine(x16[..., :32].contiguous(), packed, bias, 128, 3, 1, 1)


# ---- (b) ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(23, 31), (5, 7)], ids=["23x31", "5x7"])
@pytest.mark.parametrize("C", [512, 128])
def test_groupnorm_statistics_of_an_fp16_map_are_bitwise_those_of_the_upcast_map(C, hw):
    import bev_native as nat
    g = _gen(C + hw[0])
    z16 = (torch.randn(2, hw[0], hw[1], C, generator=g) * 1.7 + 0.3).half().to(DEV)
    gamma = torch.rand(C, generator=g).add(0.5).to(DEV)
    beta = torch.randn(C, generator=g).to(DEV)
    got = nat.groupnorm_fwd(z16, GROUPS, gamma, beta, 1e-5)
    ref = nat.groupnorm_fwd(z16.float(), GROUPS, gamma, beta, 1e-5)
    for name, a, b in zip(("mean", "rstd", "scale", "shift"), got, ref):
        assert a.dtype == torch.float32 and a.shape == b.shape, name
        assert torch.equal(a, b), name
    # and they are the statistics: against float64 on the host
    zd = z16.double().cpu().view(2, -1, GROUPS, C // GROUPS)
    mu = zd.mean(dim=(1, 3))
    assert torch.allclose(got[0].double().cpu(), mu, rtol=1e-6, atol=1e-7)


# ---- (c), (d) ------------------------------------------------------------------------------------------------------------
HEADS = [(130, 23, 31), (130, 24, 40), (18, 23, 31), (18, 24, 40)]
HEAD_IDS = ["c130_23x31", "c130_24x40", "c18_23x31", "c18_24x40"]
_HEAD = {}


def _head(hi):
    """A BEVDetector with every parameter randomised (the CenterNet init zeroes the offset head), its fp32 NHWC
    operand (B = 2, input_channels_padded wide, the pad zero), and the references -- built once per shape."""
    if hi in _HEAD:
        return _HEAD[hi]
    from models.heads.detector import BEVDetector
    cin, H, W = HEADS[hi]
    torch.manual_seed(40 + hi)
    det = BEVDetector(in_channels=cin, bev_size=(H, W)).eval()
    g = _gen(60 + hi)
    with torch.no_grad():
        for m in det.modules():
            if isinstance(m, torch.nn.GroupNorm):
                m.weight.uniform_(0.5, 1.5, generator=g)
                m.bias.uniform_(-0.3, 0.3, generator=g)
        for h in (det.heatmap_head, det.offset_head, det.size_head):
            h.weight.normal_(0.0, 0.05, generator=g)
            h.bias.uniform_(-1.0, 1.0, generator=g)
    x = torch.zeros(2, H, W, det.input_channels_padded)
    x[..., :cin] = torch.randn(2, H, W, cin, generator=g)
    exact, r64 = _forward64(det, x, False), _forward64(det, x, True)
    det = det.to(DEV)
    x = x.to(DEV)
    _HEAD[hi] = dict(det=det, x=x, exact=exact, r64=r64, composed=_compose_native(det, x))
    return _HEAD[hi]


def _head_wb(det, dtype):
    w, b = det._head_params()
    return w.detach().to(dtype), b.detach().to(dtype)


def _compose_native(det, x):
    """The f16 head from the AMP training primitives: the fp32-output fp16 conv, .half(), GroupNorm statistics of the
    upcast map, the materialised fp16 GroupNorm + ReLU output."""
    import bev_native as nat
    convs, gns = det._convs()
    with torch.no_grad():
        a = F.pad(x, (0, (-x.shape[-1]) % 64)).contiguous()
        for conv, gn in zip(convs, gns):
            d = conv.dilation[0]
            w = F.pad(conv.weight.detach().float(), (0, 0, 0, 0, 0, a.shape[-1] - conv.weight.shape[1])).contiguous()
            z = nat.conv2d_h16_any(a, nat.pack_conv_weight_h16(w), w.shape[0], 3, 3, 1, d, dilation=d).half()
            _, _, scale, shift = nat.groupnorm_fwd(z.float(), GROUPS, gn.weight, gn.bias, gn.eps)
            a = nat.groupnorm_apply_half(z.float(), scale, shift, True)
        w, b = _head_wb(det, torch.float32)
        return nat.conv2d_h16_any(a, nat.pack_conv_weight_h16(w.contiguous()), 5, 3, 3, 1, 1, bias=b.contiguous())


def _forward64(det, x, rounded):
    """The eval head on the CPU in float64 -> y [B, H, W, 5].  rounded = False: exact, no rounding anywhere.
    True: R64, the module docstring's arithmetic -- float64 conv sums of fp16-rounded operands and weights, z stored
    in fp16, the GroupNorm affine of the stored values (double sums; rstd, scale, shift in fp32 as the finalize
    kernel forms them), a = f16(max(float(z) scale + shift, 0)) in fp32, the last conv unrounded."""
    convs, gns = det._convs()
    h16 = (lambda t: t.half().double()) if rounded else (lambda t: t)
    with torch.no_grad():
        a = x[..., :det.in_channels].double().permute(0, 3, 1, 2)
        for conv, gn in zip(convs, gns):
            d = conv.dilation[0]
            z = F.conv2d(h16(a), h16(conv.weight.detach().double()), None, 1, d, d)
            if not rounded:
                a = F.group_norm(z, GROUPS, gn.weight.detach().double(), gn.bias.detach().double(), gn.eps).clamp_min(0)
                continue
            z = z.half()
            B, C = z.shape[:2]
            zg = z.double().contiguous().view(B, GROUPS, -1)
            mu = zg.mean(dim=2)
            var = ((zg * zg).mean(dim=2) - mu * mu).clamp_min(0)
            rstd = (1.0 / torch.sqrt(var + float(gn.eps))).float()
            cpg = C // GROUPS
            scale = rstd.repeat_interleave(cpg, dim=1) * gn.weight.detach().float()       # [B, C] fp32
            shift = gn.bias.detach().float() - mu.float().repeat_interleave(cpg, dim=1) * scale
            t = z.float() * scale.view(B, C, 1, 1)
            a = (t + shift.view(B, C, 1, 1)).clamp_min(0).half().double()
        w, b = _head_wb(det, torch.float64)
        y = F.conv2d(a, h16(w), b, 1, 1)
    return y.permute(0, 2, 3, 1).contiguous()


def _y(out):
    """The 5-channel conv output [B, H, W, 5] back from the head's dict."""
    return torch.cat([out["heatmap_logits"], out["offset_raw"], out["size_raw"]], dim=1).permute(0, 2, 3, 1)


@pytest.mark.parametrize("hi", range(len(HEADS)), ids=HEAD_IDS)
def test_f16_head_is_bitwise_its_composition(hi):
    import bev_native as nat
    ref = _head(hi)
    det, x = ref["det"], ref["x"]
    with torch.no_grad(), nat.head_arith_mode("f16"):
        assert det.operand_channels() == (HEADS[hi][0] + 63) // 64 * 64
        narrow = det.forward_nhwc(x)                                          # input_channels_padded wide: padded by a copy
        wide = det.forward_nhwc(F.pad(x, (0, det.operand_channels() - x.shape[-1])).contiguous())
        nchw = det(x[..., :HEADS[hi][0]].permute(0, 3, 1, 2))                 # BEVDetector.forward pads itself
    torch.cuda.synchronize()
    assert det.operand_channels() == det.input_channels_padded
    for out in (narrow, wide, nchw):
        y = _y(out)
        assert y.dtype == torch.float32 and y.shape == ref["composed"].shape
        assert torch.equal(y, ref["composed"]), int((y != ref["composed"]).sum())
        assert torch.equal(out["heatmap"], torch.sigmoid(out["heatmap_logits"]))
        assert torch.equal(out["size"], torch.exp(out["size_raw"]))
    assert float(ref["composed"][..., 1:3].abs().max()) > 0  # the offset head is not the zero of its init


def _rel_l2(a, b):
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("hi", range(len(HEADS)), ids=HEAD_IDS)
def test_f16_head_error_within_the_float64_restatement(hi):
    import bev_native as nat
    ref = _head(hi)
    with torch.no_grad(), nat.head_arith_mode("f16"):
        got = _y(ref["det"].forward_nhwc(ref["x"])).double().cpu()
    exact, r64 = ref["exact"], ref["r64"]
    assert got.shape == exact.shape
    l2n, l2r = _rel_l2(got, exact), _rel_l2(r64, exact)
    mxn, mxr = float((got - exact).abs().max()), float((r64 - exact).abs().max())
    print(f"{HEAD_IDS[hi]}: relL2 native {l2n:.3e} R64 {l2r:.3e} ratio {l2n / l2r:.3f}; "
          f"max native {mxn:.3e} R64 {mxr:.3e} ratio {mxn / mxr:.3f}")
    assert l2r > 1e-5  # the restatement does round
    assert l2n <= 1.5 * l2r
    assert mxn <= 2.0 * mxr


# ---- (e) ---------------------------------------------------------------------------------------------------------------
def test_head_switch_hygiene():
    import bev_native as nat
    ref = _head(2)
    det, x = ref["det"], ref["x"]
    assert nat.head_arith() == "f32"
    with torch.no_grad():
        before = _y(det.forward_nhwc(x)).clone()
        with nat.head_arith_mode("f16"):
            half = _y(det.forward_nhwc(x)).clone()
        after = _y(det.forward_nhwc(x)).clone()
        with nat.conv_arith_mode("f16"):  # the trunk's switch does not touch the head
            trunk16 = _y(det.forward_nhwc(x)).clone()
        with nat.head_arith_mode("f16"):
            again = _y(det.forward_nhwc(x)).clone()
    assert before.dtype == half.dtype == torch.float32 and before.shape == half.shape
    assert torch.equal(before, after)      # the fp16 panels did not replace the default mode's
    assert not torch.equal(before, half)
    assert torch.equal(before, trunk16)
    assert torch.equal(half, again)


def test_f16_head_follows_a_parameter_update():
    """The fp16 panels are keyed like the fp32 ones: an in-place update of a weight rebuilds them."""
    import bev_native as nat
    from models.heads.detector import BEVDetector
    torch.manual_seed(2)
    det = BEVDetector(in_channels=18, bev_size=(6, 9)).to(DEV).eval()
    x = torch.zeros(1, 6, 9, 32, device=DEV)
    x[..., :18] = torch.randn(1, 6, 9, 18, generator=_gen(3)).to(DEV)
    with torch.no_grad(), nat.head_arith_mode("f16"):
        y0 = _y(det.forward_nhwc(x)).clone()
        det.size_head.bias.add_(1.0)
        y1 = _y(det.forward_nhwc(x)).clone()
        det.stem[0].weight.mul_(1.5)
        y2 = _y(det.forward_nhwc(x)).clone()
    # the bias is added in fp32 after the sum: (s + (b + 1)) against (s + b) + 1, values of order 1 to 10
    assert torch.equal(y1[..., :3], y0[..., :3])
    assert torch.allclose(y1[..., 3:], y0[..., 3:] + 1.0, rtol=1e-6, atol=1e-5)
    assert not torch.equal(y2, y1)


# ---- (f) ---------------------------------------------------------------------------------------------------------------
def test_f16_head_bevnet_forward():
    """One BEVNet eval forward (the bevnet_small fixture) with the head in the f16 arithmetic: the default forward's
    keys, shapes and fp32 dtypes, finite values, and bev_feat -- the operand's view, assembled 64-wide here -- equal
    to the default forward's."""
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
        with nat.head_arith_mode("f16"):
            half = net(batch)
    assert set(half) == set(base)
    for k in ("heatmap", "heatmap_logits", "offset", "offset_raw", "size", "size_raw", "bev_feat"):
        assert half[k].shape == base[k].shape and half[k].dtype == base[k].dtype == torch.float32, k
        assert bool(torch.isfinite(half[k]).all()), k
    assert torch.equal(half["bev_feat"], base["bev_feat"])
    assert not torch.equal(half["heatmap_logits"], base["heatmap_logits"])
    assert len(half["boxes"]) == len(base["boxes"]) and len(half["scores"]) == len(base["scores"])
