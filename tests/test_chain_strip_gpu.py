"""The strip-staged mainloop of the layer1 chain kernels (k_conv_x6s<4,1,1,2,CHAIN,true>, csrc/bev_conv_x6.hip;
BEV_TUNE_CONV_X6_STRIP): conv2's pre-split operand is staged once per tap row, a strip of 130 pixels serving the
taps kx = 0, 1, 2, with the horizontal image edges zeroed at the fragment read.

Two references, both independent of the strip code: the SEPARATE launches (conv2d_nhwc_x6 on the fp32 operand, then
conv3 with the residual, or conv2d_dual_nhwc for the dual), and the same chain call with the knob at 0 (one staging
per tap).  Every comparison is bitwise: the strip changes where A fragments come from, not one product or its order.
"""
import functools

import pytest
import torch

import bev_native as nat

pytestmark = pytest.mark.gpu

DEV = "cuda"
CI, CO, CO2 = 64, 64, 256

SHAPES = [
    (1, 1, 1),    # both edge masks on one pixel
    (2, 3, 2),
    (2, 5, 37),   # several image rows per 128-pixel tile
    (3, 2, 128),  # a tile is exactly one row; the image changes every two tiles
    (1, 2, 129),  # a tile boundary one pixel past a row start
    (1, 3, 130),  # ... and two
    (1, 2, 480),  # the benchmark's width
]
IDS = ["x".join(map(str, s)) for s in SHAPES]


def _same_bits(got, ref):
    gn, rn = torch.isnan(got), torch.isnan(ref)
    assert torch.equal(gn, rn)
    assert torch.equal(got[~gn].view(torch.int32), ref[~rn].view(torch.int32))


def _operands(shape, nan_at=()):
    N, H, W = shape
    g = torch.Generator().manual_seed(7919 * N + 101 * H + W)
    x = torch.randn(N, H, W, CI, generator=g)
    for n, y, xx in nan_at:
        x[n, y, xx, (n + y + xx) % CI] = float("nan")  # one channel is enough: every product of the pixel's slice
    xb = torch.randn(N, H, W, 64, generator=g).to(DEV)
    w2 = (torch.randn(CO, CI, 3, 3, generator=g) / (9 * CI) ** 0.5).to(DEV)
    w3 = (torch.randn(CO2, CO, 1, 1, generator=g) / CO ** 0.5).to(DEV)
    w3d = (torch.randn(CO2, CO + 64, 1, 1, generator=g) / (CO + 64) ** 0.5).to(DEV)
    b2, b3 = (torch.randn(CO, generator=g) * 0.1).to(DEV), (torch.randn(CO2, generator=g) * 0.1).to(DEV)
    res = torch.randn(N, H, W, CO2, generator=g).to(DEV)
    x = x.to(DEV)
    return dict(x=x, xs=nat.split3(x), xb=xb, b2=b2, b3=b3, res=res, p2=nat.pack_conv_weight_x6(w2),
                p3=nat.pack_conv_weight_x6(w3), p3d=nat.pack_conv_weight_x6(w3d))


def _separate(c):
    """The separate launches: (identity with residual, identity without, dual)."""
    h2 = nat.conv2d_nhwc_x6(c["x"], c["p2"], c["b2"], CO, 3, 3, 1, 1, 1, 1)
    ref_res = nat.conv2d_nhwc_x6(h2, c["p3"], c["b3"], CO2, 1, 1, 1, 0, 1, 1, residual=c["res"])
    ref_nores = nat.conv2d_nhwc_x6(h2, c["p3"], c["b3"], CO2, 1, 1, 1, 0, 1, 1)
    ref_dual = nat.conv2d_dual_nhwc(h2, c["xb"], 1, c["p3d"], c["b3"], CO2, relu=True)
    torch.cuda.synchronize()
    return ref_res, ref_nores, ref_dual


@functools.lru_cache(maxsize=None)
def _case(shape):
    c = _operands(shape)
    c["ref_res"], c["ref_nores"], c["ref_dual"] = _separate(c)
    return c


def _identity(c, with_res, strip):
    with nat.tuned(CONV_X6_STRIP=strip):
        y = nat.conv2d_chain_nhwc(c["xs"], c["p2"], c["b2"], CO, 3, 3, 1, 1, 1, c["p3"], c["b3"], CO2, 1,
                                  residual=c["res"] if with_res else None)
    torch.cuda.synchronize()
    return y


def _dual(c, strip):
    with nat.tuned(CONV_X6_STRIP=strip):
        y = nat.conv2d_chain_dual_nhwc(c["xs"], c["p2"], c["b2"], 64, 3, 3, 1, 1, 1, c["xb"], 1, c["p3d"], c["b3"],
                                       CO2, 1)
    torch.cuda.synchronize()
    return y


def test_strip_knob_is_on_by_default_and_restores():
    assert nat.tune(nat.TUNE_CONV_X6_STRIP, 0) == 1
    assert nat.tune(nat.TUNE_CONV_X6_STRIP, 1) == 0
    with pytest.raises(ValueError):
        nat.tune(nat.TUNE_CONV_X6_STRIP, 2)
    assert nat.tune(nat.TUNE_CONV_X6_STRIP, 1) == 1


@pytest.mark.parametrize("with_res", [True, False], ids=["res", "nores"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_strip_identity_chain_bitwise(shape, with_res):
    c = _case(shape)
    got = _identity(c, with_res, 1)
    _same_bits(got, c["ref_res" if with_res else "ref_nores"])
    _same_bits(got, _identity(c, with_res, 0))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_strip_dual_chain_bitwise(shape):
    c = _case(shape)
    got = _dual(c, 1)
    _same_bits(got, c["ref_dual"])
    _same_bits(got, _dual(c, 0))


def test_strip_non_finite_stays_in_its_receptive_field():
    """NaN at the last pixel of a row and the first of the next, and in the last row of image 0 and the first row of
    image 1: the strip holds those pixels next to outputs they do not belong to (the previous / next row's edge, the
    other image).  Outputs outside the pixels' true 3x3 fields are finite and bit-equal to both references."""
    shape = N, H, W = (2, 5, 37)
    nan_at = [(0, 1, W - 1), (0, 2, 0), (0, H - 1, W - 1), (0, H - 1, 5), (1, 0, 0), (1, 0, 7)]
    c = _operands(shape, tuple(nan_at))
    field = torch.zeros(N, H, W, dtype=torch.bool)
    for n, y, x in nan_at:
        field[n, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = True
    field = field.to(DEV)
    refs = _separate(c)
    for got, ref, got0 in ((_identity(c, True, 1), refs[0], _identity(c, True, 0)),
                           (_identity(c, False, 1), refs[1], _identity(c, False, 0)),
                           (_dual(c, 1), refs[2], _dual(c, 0))):
        assert torch.isfinite(got[~field]).all()
        assert torch.isnan(got[field]).all()
        _same_bits(got, ref)
        _same_bits(got, got0)
