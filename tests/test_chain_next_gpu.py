"""The layer1 chain that also runs the next block's 1x1 conv1 in its epilogue (bev_conv2d_chain_conv1_x6_f32,
k_conv_x6s<4, 1, 1, 2, 3, true>; csrc/bev_conv_x6.hip x6_chain_epilogue NXT).

Reference: the same library's chain launch (bev_conv2d_chain_x6_f32 on the same pre-split operand) followed by the
separate conv2d_nhwc_x6(y, ..., split_out=True).  The fused launch must give the same y and the same three planes of
h', bit for bit -- compared on integer views, so NaNs compare too.  Shapes are the smallest at which the kernel can
go wrong (ragged tiles, image borders inside a tile, W = 1 / 2, the bench's width), Co2 walks the column-block loop
through 1, 2, an odd number of pairs, and 4 pairs of blocks.
"""
import functools

import pytest
import torch

import bev_native as nat

pytestmark = pytest.mark.gpu

DEV = "cuda"
CO3 = 64


@functools.lru_cache(maxsize=None)
def _weights(Co2, seed=0):
    """Panels and biases of conv2 (3x3, 64 -> 64), conv3 (1x1, 64 -> Co2) and the next conv1 (1x1, Co2 -> 64)."""
    g = torch.Generator(device=DEV).manual_seed(1000 + Co2 + seed)
    r = lambda *s: torch.nan_to_num(torch.randn(*s, generator=g, device=DEV))
    w2, w3, wn = r(64, 64, 3, 3) / 24.0, r(Co2, 64, 1, 1) / 8.0, r(CO3, Co2, 1, 1) / Co2 ** 0.5
    return (nat.pack_conv_weight_x6(w2), r(64) * 0.1, nat.pack_conv_weight_x6(w3), r(Co2) * 0.1,
            nat.pack_conv_weight_x6(wn), r(CO3) * 0.1)


def _operands(N, H, W, Co2, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.nan_to_num(torch.randn(N, H, W, 64, generator=g, device=DEV))
    res = torch.nan_to_num(torch.randn(N, H, W, Co2, generator=g, device=DEV))
    return x, res


def _both(xs, Co2, res, bias2=True, bias3=True, act2=1, act3=1):
    """(fused y, fused h' planes, reference y, reference h' planes)"""
    p2, b2, p3, b3, pn, bn = _weights(Co2)
    b3 = b3 if bias2 else None
    bn = bn if bias3 else None
    y_ref = nat.conv2d_chain_nhwc(xs, p2, b2, 64, 3, 3, 1, 1, 1, p3, b3, Co2, act2, residual=res)
    h_ref = nat.conv2d_nhwc_x6(y_ref, pn, bn, CO3, 1, 1, 1, 0, 1, act3, split_out=True)
    y, h = nat.conv2d_chain_conv1_x6(xs, p2, b2, 64, 3, 3, 1, 1, 1, p3, b3, Co2, act2, pn, bn, CO3, act3,
                                     residual=res)
    torch.cuda.synchronize()
    return y, h.planes, y_ref, h_ref.planes


def _same_bits(y, h, y_ref, h_ref):
    assert y.shape == y_ref.shape and h.shape == h_ref.shape
    assert torch.equal(y.view(torch.int32), y_ref.view(torch.int32))
    for p in range(3):
        assert torch.equal(h[p].view(torch.int16), h_ref[p].view(torch.int16)), f"plane {p}"


SHAPES = [(1, 1, 1), (1, 8, 16), (1, 9, 15), (3, 5, 7), (2, 5, 1), (2, 5, 2), (1, 2, 480)]


@pytest.mark.parametrize("N,H,W", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_chain_conv1_bit_identical_shapes(N, H, W):
    """One ragged tile with every tap row outside, exactly one tile, a tile of 7 rows, tiles crossing image borders,
    the strip's edge selects (W = 1, 2), 7.5 tiles of the bench's width; Co2 = 64 (the look-ahead on empty
    descriptors from the start), 128, 192 (an odd number of block pairs), 256."""
    for Co2 in (64, 128, 192, 256):
        x, res = _operands(N, H, W, Co2, 7 * N + H + W + Co2)
        _same_bits(*_both(nat.split3(x), Co2, res))


@pytest.mark.parametrize("with_res", [True, False], ids=["res", "nores"])
def test_chain_conv1_operand_forms(with_res):
    """With and without the residual, bias2, bias3; act2 and act3 each none and ReLU."""
    N, H, W, Co2 = 3, 5, 7, 128
    x, res = _operands(N, H, W, Co2, 99)
    xs = nat.split3(x)
    for bias2 in (True, False):
        for bias3 in (True, False):
            for act2 in (0, 1):
                for act3 in (0, 1):
                    _same_bits(*_both(xs, Co2, res if with_res else None, bias2, bias3, act2, act3))


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("where", ["res", "h1_first", "h1_last"])
def test_chain_conv1_non_finite(where, bad):
    """One non-finite element in the residual, or in h1 at the first / last pixel of a tile (tile 1 of 8): the bits,
    and so the non-finite pixels of h', are those of the separate launches."""
    N, H, W, Co2 = 1, 2, 480, 128
    x, res = _operands(N, H, W, Co2, 5)
    if where == "res":
        res.view(-1, Co2)[300, 37] = bad
    else:
        x.view(-1, 64)[128 if where == "h1_first" else 255, 11] = bad
    y, h, y_ref, h_ref = _both(nat.split3(x), Co2, res)
    _same_bits(y, h, y_ref, h_ref)
    fin = lambda pl: torch.isfinite(pl.float()).all(0).all(-1).view(-1)  # per pixel: every plane, every channel
    assert torch.equal(fin(h), fin(h_ref))
    assert not fin(h).all() and fin(h).any()


def test_chain_conv1_repeatable_at_size():
    """1,000 tiles, two launches: equal to each other and to the separate launches."""
    N, H, W, Co2 = 2, 250, 256, 256
    x, res = _operands(N, H, W, Co2, 17)
    xs = nat.split3(x)
    y1, h1, y_ref, h_ref = _both(xs, Co2, res)
    y1, h1 = y1.clone(), h1.clone()
    y2, h2, _, _ = _both(xs, Co2, res)
    assert torch.equal(y1, y2) and torch.equal(h1.view(torch.int16), h2.view(torch.int16))
    _same_bits(y1, h1, y_ref, h_ref)


@pytest.mark.parametrize("groups", [1, 2])
def test_resnet50_plan_bit_identical(groups, monkeypatch):
    """ResNet-50 to layer2 with the plan on == with it off, and the plan does run the fused launch: once per image
    group (layer1.1's chain runs layer1.2's conv1)."""
    from models.encoders import resnet
    torch.manual_seed(3)
    net = resnet.resnet50().eval().to(DEV)
    net.stream_groups = groups
    imgs = torch.randn(2, 3, 64, 96, device=DEV)
    calls = []
    fused = nat.conv2d_chain_conv1_x6
    monkeypatch.setattr(nat, "conv2d_chain_conv1_x6", lambda *a, **k: (calls.append(1), fused(*a, **k))[1])
    with torch.no_grad(), nat.conv_arith_mode("bf16x6"):
        monkeypatch.setattr(resnet, "CHAIN_CONV1", False)
        ref = net.forward_features_nhwc(imgs, 2).clone()
        assert not calls
        monkeypatch.setattr(resnet, "CHAIN_CONV1", True)
        got = net.forward_features_nhwc(imgs, 2).clone()
    torch.cuda.synchronize()
    assert len(calls) == groups
    assert torch.equal(got, ref)


_ORDER = ("x xs N H W Ci packed bias Co KH KW stride pad act packed2 bias2 Co2 residual act2 y packed3 bias3 Co3 act3 "
          "ys3 Ho Wo stream").split()
_BASE = dict(x=None, xs=0x60000, N=0, H=8, W=8, Ci=64, packed=0x20000, bias=None, Co=64, KH=3, KW=3, stride=1, pad=1,
             act=1, packed2=0x50000, bias2=None, Co2=256, residual=None, act2=1, y=0x30000, packed3=0x70000,
             bias3=None, Co3=64, act3=1, ys3=0x90000, Ho=8, Wo=8, stream=None)
_REFUSED = [
    dict(x=0x10000), dict(x=0x10000, xs=None), dict(xs=None), dict(xs=0x60008), dict(N=-1), dict(H=0), dict(W=0),
    dict(Ci=32), dict(Ci=128), dict(Co=32), dict(Co=128), dict(packed=None), dict(packed=0x20008),
    dict(KH=1, KW=1, pad=0), dict(KH=1, pad=0, Ho=8), dict(KH=5, KW=5, pad=2), dict(stride=2, Ho=4, Wo=4),
    dict(pad=0, Ho=6, Wo=6), dict(pad=2, Ho=10, Wo=10), dict(act=-1), dict(act=3), dict(packed2=None),
    dict(packed2=0x50008), dict(Co2=0), dict(Co2=96), dict(Co2=-64), dict(act2=-1), dict(act2=3), dict(y=None),
    dict(packed3=None), dict(packed3=0x70008), dict(Co3=0), dict(Co3=32), dict(Co3=128), dict(act3=-1), dict(act3=3),
    dict(ys3=None), dict(ys3=0x90008), dict(Ho=7), dict(Wo=9),
]


def test_chain_conv1_argument_rules():
    """The accepted set answers 0 (N = 0: before any HIP call); every set with one rule broken answers BEV_ERR_ARGS
    -- with N = 0 as well, so nothing can reach a kernel and a rule checked only behind the empty call's answer
    would show as 0."""
    fn = nat.lib().bev_conv2d_chain_conv1_x6_f32
    call = lambda ch: fn(*[dict(_BASE, **ch)[k] for k in _ORDER])
    assert call({}) == 0
    assert call(dict(residual=0x80000, bias=0xA0000, bias2=0xA0100, bias3=0xA0200, act=0, act2=0, act3=0)) == 0
    bad = [(ch, got) for ch in _REFUSED for got in [call(ch)] if got != -1]
    assert not bad, bad
