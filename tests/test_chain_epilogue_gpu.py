"""The chained bottleneck kernels' epilogue (x6_chain_epilogue, csrc/bev_conv_x6.hip): conv3's W3 panel staged
through LDS once per workgroup, counted vmcnt waits, compile-time activations.

The reference is always the SEPARATE launches, whose epilogue is another function: conv2d_nhwc_x6 (conv2) then
conv2d_nhwc_x6 with the residual (identity chains) or conv2d_dual_nhwc (dual chains) -- never the other chain
kernel.  Every comparison is torch.equal: the chain must sum every output element in the separate launches' order.
"""
import functools

import pytest
import torch

import bev_native as nat

pytestmark = pytest.mark.gpu

DEV = "cuda"

SHAPES = [(2, 25, 37), (1, 31, 20)]  # ragged last tile for the 128- and the 64-row tile
CHANS = [(64, 64, 128), (64, 64, 256), (128, 128, 512), (128, 128, 128)]  # one / several blocks, both tiles


@functools.lru_cache(maxsize=None)
def _identity_case(shape, chans, stride):
    """Operands, panels and the separate launches' conv2 output of one identity chain; built once."""
    N, H, W = shape
    Ci, Co, Co2 = chans
    g = torch.Generator().manual_seed(1000 * H + 10 * Co2 + Ci + stride)
    x = torch.randn(N, H, W, Ci, generator=g).to(DEV)
    w2 = (torch.randn(Co, Ci, 3, 3, generator=g) / (9 * Ci) ** 0.5).to(DEV)
    w3 = (torch.randn(Co2, Co, 1, 1, generator=g) / Co ** 0.5).to(DEV)
    b2, b3 = (torch.randn(Co, generator=g) * 0.1).to(DEV), (torch.randn(Co2, generator=g) * 0.1).to(DEV)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    res = torch.randn(N, Ho, Wo, Co2, generator=g).to(DEV)
    p2, p3 = nat.pack_conv_weight_x6(w2), nat.pack_conv_weight_x6(w3)
    h2 = nat.conv2d_nhwc_x6(x, p2, b2, Co, 3, 3, stride, 1, 1, 1)
    return dict(x=x, xs=nat.split3(x), p2=p2, p3=p3, b2=b2, b3=b3, res=res, h2=h2)


@functools.lru_cache(maxsize=None)
def _identity_ref(shape, chans, stride, with_res, act2):
    c = _identity_case(shape, chans, stride)
    ref = nat.conv2d_nhwc_x6(c["h2"], c["p3"], c["b3"], chans[2], 1, 1, 1, 0, 1, act2,
                             residual=c["res"] if with_res else None)
    torch.cuda.synchronize()
    return ref


def _identity_chain(c, chans, stride, split, with_res, act2):
    return nat.conv2d_chain_nhwc(c["xs"] if split else c["x"], c["p2"], c["b2"], chans[1], 3, 3, stride, 1, 1,
                                 c["p3"], c["b3"], chans[2], act2, residual=c["res"] if with_res else None)


@pytest.mark.parametrize("act2", [1, 0], ids=["relu", "noact"])
@pytest.mark.parametrize("with_res", [True, False], ids=["res", "nores"])
@pytest.mark.parametrize("split", [False, True], ids=["fp32", "presplit"])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("chans", CHANS, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_chain_epilogue_equals_separate_launches(shape, chans, stride, split, with_res, act2):
    c = _identity_case(shape, chans, stride)
    ref = _identity_ref(shape, chans, stride, with_res, act2)
    got = _identity_chain(c, chans, stride, split, with_res, act2)
    torch.cuda.synchronize()
    assert torch.equal(got, ref)


@functools.lru_cache(maxsize=None)
def _dual_case(shape):
    """The layer1.0 dual: Ci 64, shortcut 64 channels, Co2 256; reference = conv2 launch + dual tail launch."""
    N, H, W = shape
    Ci, Co, Co2 = 64, 64, 256
    g = torch.Generator().manual_seed(17 + H)
    x = torch.randn(N, H, W, Ci, generator=g).to(DEV)
    xb = torch.randn(N, H, W, 64, generator=g).to(DEV)
    w2 = (torch.randn(Co, Ci, 3, 3, generator=g) / (9 * Ci) ** 0.5).to(DEV)
    w3 = (torch.randn(Co2, Co + 64, 1, 1, generator=g) / (Co + 64) ** 0.5).to(DEV)
    b2, b3 = (torch.randn(Co, generator=g) * 0.1).to(DEV), (torch.randn(Co2, generator=g) * 0.1).to(DEV)
    p2, p3 = nat.pack_conv_weight_x6(w2), nat.pack_conv_weight_x6(w3)
    h2 = nat.conv2d_nhwc_x6(x, p2, b2, Co, 3, 3, 1, 1, 1, 1)
    ref = nat.conv2d_dual_nhwc(h2, xb, 1, p3, b3, Co2, relu=True)
    torch.cuda.synchronize()
    return dict(x=x, xs=nat.split3(x), xb=xb, p2=p2, p3=p3, b2=b2, b3=b3, ref=ref)


def _dual_chain(c, split):
    return nat.conv2d_chain_dual_nhwc(c["xs"] if split else c["x"], c["p2"], c["b2"], 64, 3, 3, 1, 1, 1, c["xb"], 1,
                                      c["p3"], c["b3"], 256, 1)


@pytest.mark.parametrize("split", [False, True], ids=["fp32", "presplit"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_chain_dual_epilogue_equals_separate_launches(shape, split):
    c = _dual_case(shape)
    got = _dual_chain(c, split)
    torch.cuda.synchronize()
    assert torch.equal(got, c["ref"])


# More workgroups than resident slots (2 per CU): a workgroup's W3 stages are rewritten while its neighbours run, and
# a missing barrier between a stage's last read and the DMA that overwrites it would show as a run-to-run difference.
@pytest.mark.parametrize("split", [False, True], ids=["fp32", "presplit"])
@pytest.mark.parametrize("shape,chans", [((1, 288, 480), (64, 64, 256)), ((1, 144, 240), (128, 128, 512))],
                         ids=["1080tiles-64x64x256", "540tiles-128x128x512"])
def test_chain_epilogue_many_workgroups_repeatable(shape, chans, split):
    c = _identity_case(shape, chans, 1)
    ref = _identity_ref(shape, chans, 1, True, 1)
    one = _identity_chain(c, chans, 1, split, True, 1)
    two = _identity_chain(c, chans, 1, split, True, 1)
    torch.cuda.synchronize()
    assert torch.equal(one, two)
    assert torch.equal(one, ref)


@pytest.mark.parametrize("split", [False, True], ids=["fp32", "presplit"])
def test_chain_dual_epilogue_many_workgroups_repeatable(split):
    c = _dual_case((1, 288, 480))
    one = _dual_chain(c, split)
    two = _dual_chain(c, split)
    torch.cuda.synchronize()
    assert torch.equal(one, two)
    assert torch.equal(one, c["ref"])
