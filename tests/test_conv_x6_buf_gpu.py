"""Buffer-load operand staging of the split-bf16 convs on an fp32 operand (k_conv_x6 / k_conv_x6b BUFA,
BEV_TUNE_CONV_X6_BUF; csrc/bev_conv_x6.hip) and the pairwise operand split (split3x2).

The buffer form addresses an operand row by a 32-bit offset from a per-workgroup base (the first image the tile
touches), carries tap and channel offset in the scalar offset, and masks a lane by sending its offset out of range.
Every case is run

  * against the same call with the knob at 0 (the 64-bit pointer form), torch.equal;
  * for two 1x1 cases and one 3x3 case against the pre-split route (bev_split3_f32 + k_conv_x6s, whose addressing is
    another one), torch.equal;
  * against float64 torch on the fp32 operands with the bar of tests/test_conv_x6_gpu.py: 1e-5 of the output scale.

Guard band: every fp32 operand (x, and x2 of the dual form) is a slice of a larger allocation filled with NaN, at
least one 128-pixel tile of NaN on each side, and every weight is nonzero: an address outside the tensor, or a masked
lane that loaded, makes an output non-finite.  Shapes are the smallest at which the addressing can go wrong: one pixel,
ragged tiles, a tile over five images, a row longer than a tile, strides, dilation, both tiles, both kernels.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bev_native as nat

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _guarded(t):
    """t on the device as a slice of a NaN-filled allocation: >= 128 pixels of NaN (one tile's rows) on each side,
    the slice 16-byte aligned."""
    g = 128 * t.shape[-1] + 64
    buf = torch.full((2 * g + t.numel(),), float("nan"), device=DEV, dtype=torch.float32)
    v = buf[g:g + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 0 and v.is_contiguous()
    return v


def _nonzero(w):
    return torch.where(w == 0, torch.ones_like(w), w)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _out_hw(H, W, K, s, p, d):
    return (H + 2 * p - d * (K - 1) - 1) // s + 1, (W + 2 * p - d * (K - 1) - 1) // s + 1


@functools.lru_cache(maxsize=None)
def _single(N, H, W, Ci, Co, K, s, p, d):
    """Operands (x guarded), panel, residual and the float64 references of one conv; built once, never modified."""
    g = torch.Generator().manual_seed(1000 * H + 10 * W + Ci + Co + K + s)
    x = torch.randn(N, H, W, Ci, generator=g)
    w = _nonzero(torch.randn(Co, Ci, K, K, generator=g) / (Ci * K * K) ** 0.5)
    b = torch.randn(Co, generator=g) * 0.1
    Ho, Wo = _out_hw(H, W, K, s, p, d)
    res = torch.randn(N, Ho, Wo, Co, generator=g)
    z = _nhwc(F.conv2d(_nchw(x).double(), w.double(), None, stride=s, padding=p, dilation=d))
    return dict(x=_guarded(x), p6=nat.pack_conv_weight_x6(w.to(DEV)), b=b.to(DEV), res=res.to(DEV), z=z,
                b64=b.double(), res64=res.double())


MODES = ["nobias", "bias", "res-relu", "split-out"]


def _run_single(c, geom, mode, x=None):
    N, H, W, Ci, Co, K, s, p, d = geom
    x = c["x"] if x is None else x
    bias = None if mode == "nobias" else c["b"]
    if mode == "res-relu":
        return nat.conv2d_nhwc_x6(x, c["p6"], bias, Co, K, K, s, p, d, 1, residual=c["res"])
    if mode == "split-out":
        return nat.conv2d_nhwc_x6(x, c["p6"], bias, Co, K, K, s, p, d, 0, split_out=True)
    return nat.conv2d_nhwc_x6(x, c["p6"], bias, Co, K, K, s, p, d, 0)


def _ref64(c, mode):
    z = c["z"]
    if mode != "nobias":
        z = z + c["b64"]
    if mode == "res-relu":
        z = torch.relu(z + c["res64"])
    return z


def _check_single(geom, mode, knobs=None, presplit=False):
    c = _single(*geom)
    with nat.tuned(**(knobs or {})):
        with nat.tuned(CONV_X6_BUF=1):
            got = _run_single(c, geom, mode)
        with nat.tuned(CONV_X6_BUF=0):
            ptr = _run_single(c, geom, mode)
        pre = _run_single(c, geom, mode, nat.split3(c["x"])) if presplit else None
    torch.cuda.synchronize()
    if mode == "split-out":
        assert torch.equal(got.planes.view(torch.int16), ptr.planes.view(torch.int16))
        if pre is not None:
            assert torch.equal(got.planes.view(torch.int16), pre.planes.view(torch.int16))
        got = got.to_float()
    else:
        assert torch.equal(got.view(torch.int32), ptr.view(torch.int32))
        if pre is not None:
            assert torch.equal(got.view(torch.int32), pre.view(torch.int32))
    assert torch.isfinite(got).all()
    ref = _ref64(c, mode)
    scale = ref.abs().max().item()
    err = (got.cpu().double() - ref).abs().max().item()
    assert err <= 1e-5 * scale, (err, scale)


# 1x1 / stride 1 / pad 0: N, H, W, Ci, Co, knobs, also against the pre-split route
PW = [
    ("one-pixel", (1, 1, 1, 32, 64), {}, False),
    ("m135-ragged-second-tile", (1, 9, 15, 64, 64), {}, True),
    ("m105-one-tile-five-images", (5, 3, 7, 256, 64), {}, False),
    ("128x128-tile", (3, 7, 19, 256, 128), {}, True),
    ("proj-nt-exact-tiles", (2, 8, 16, 512, 64), dict(CONV_X6_NT=1), False),
]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", PW, ids=[c[0] for c in PW])
def test_buf_pointwise(case, mode):
    _, (N, H, W, Ci, Co), knobs, presplit = case
    _check_single((N, H, W, Ci, Co, 1, 1, 0, 1), mode, knobs, presplit)


# the other conv forms: N, H, W, Ci, Co, K, stride, pad, dilation
FORMS = [
    ("1x1-s2", (2, 9, 15, 256, 128, 1, 2, 0, 1), False),
    ("3x3-s1-p1", (2, 5, 7, 32, 64, 3, 1, 1, 1), True),
    ("3x3-s1-p1-row-longer-than-a-tile", (1, 3, 130, 64, 128, 3, 1, 1, 1), False),
    ("3x3-s2-p1", (2, 9, 15, 128, 128, 3, 2, 1, 1), False),
    ("3x3-dil2-p2", (1, 11, 13, 32, 64, 3, 1, 2, 2), False),
    ("16deep-3x3-ci48", (2, 5, 7, 48, 64, 3, 1, 1, 1), False),
    ("16deep-1x1-ci48", (2, 5, 7, 48, 96, 1, 1, 0, 1), False),
]


@pytest.mark.parametrize("mode", ["bias", "res-relu"])
@pytest.mark.parametrize("case", FORMS, ids=[c[0] for c in FORMS])
def test_buf_conv_forms(case, mode):
    _, geom, presplit = case
    _check_single(geom, mode, None, presplit)


@pytest.mark.parametrize("case", [FORMS[1], FORMS[3]], ids=[FORMS[1][0], FORMS[3][0]])
def test_buf_16deep_kernel_forced(case):
    """The 16-deep kernel's buffer form on 32-channel-multiple shapes too (BEV_TUNE_CONV_X6_KERNEL = 1)."""
    _check_single(case[1], "bias", dict(CONV_X6_KERNEL=1))


@functools.lru_cache(maxsize=None)
def _dual(N, Ho, Wo, Ci, H2, W2, Ci2, s2, Co):
    g = torch.Generator().manual_seed(Ci + Ci2 + Co + s2)
    x = torch.randn(N, Ho, Wo, Ci, generator=g)
    x2 = torch.randn(N, H2, W2, Ci2, generator=g)
    w1 = _nonzero(torch.randn(Co, Ci, 1, 1, generator=g) / Ci ** 0.5)
    w2 = _nonzero(torch.randn(Co, Ci2, 1, 1, generator=g) / Ci2 ** 0.5)
    b = torch.randn(Co, generator=g) * 0.1
    ref = _nhwc(torch.relu(F.conv2d(_nchw(x).double(), w1.double(), b.double()) +
                           F.conv2d(_nchw(x2).double(), w2.double(), stride=s2)))
    wcat = torch.cat([w1.reshape(Co, -1), w2.reshape(Co, -1)], 1).reshape(Co, Ci + Ci2, 1, 1).contiguous()
    return dict(x=_guarded(x), x2=_guarded(x2), p6=nat.pack_conv_weight_x6(wcat.to(DEV)), b=b.to(DEV), ref=ref)


DUALS = [
    ("s2-co512", (2, 5, 7, 128, 10, 14, 256, 2, 512)),
    ("s1-co64", (2, 5, 7, 32, 5, 7, 64, 1, 64)),
]


@pytest.mark.parametrize("kernel", [0, 1], ids=["32deep", "16deep"])
@pytest.mark.parametrize("case", DUALS, ids=[c[0] for c in DUALS])
def test_buf_dual(case, kernel):
    """The dual form: a second descriptor for x2 (both operands guarded), the K step picking one by a scalar test."""
    geom = case[1]
    c = _dual(*geom)
    s2, Co = geom[7], geom[8]
    with nat.tuned(CONV_X6_KERNEL=kernel):
        with nat.tuned(CONV_X6_BUF=1):
            got = nat.conv2d_dual_nhwc(c["x"], c["x2"], s2, c["p6"], c["b"], Co, relu=True)
        with nat.tuned(CONV_X6_BUF=0):
            ptr = nat.conv2d_dual_nhwc(c["x"], c["x2"], s2, c["p6"], c["b"], Co, relu=True)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), ptr.view(torch.int32))
    assert torch.isfinite(got).all()
    scale = c["ref"].abs().max().item()
    err = (got.cpu().double() - c["ref"]).abs().max().item()
    assert err <= 1e-5 * scale, (err, scale)


# 3x3 cases whose tiles cross the boundary between two images
@pytest.mark.parametrize("case", [FORMS[1], FORMS[3]], ids=[FORMS[1][0], FORMS[3][0]])
@pytest.mark.parametrize("poisoned", [0, 1], ids=["last-row-of-image-0", "first-row-of-image-1"])
def test_buf_neighbouring_images_do_not_leak(case, poisoned):
    """NaN in the last row of image 0 (the first row of image 1): the other image's outputs, border rows included,
    stay finite and keep their bits -- a padded tap never reads the neighbouring image."""
    geom = case[1]
    N, H, W, Ci, Co, K, s, p, d = geom
    c = _single(*geom)
    clean = _run_single(c, geom, "bias")
    x = _guarded(c["x"])
    if poisoned == 0:
        x[0, H - 1] = float("nan")
    else:
        x[1, 0] = float("nan")
    got = _run_single(c, geom, "bias", x)
    with nat.tuned(CONV_X6_BUF=0):
        ptr = _run_single(c, geom, "bias", x)
    torch.cuda.synchronize()
    other = 1 - poisoned
    assert torch.isfinite(got[other]).all()
    assert torch.equal(got[other].view(torch.int32), clean[other].view(torch.int32))
    assert not torch.isfinite(got[poisoned]).all()  # the poison is seen where it belongs
    assert torch.equal(torch.isfinite(got), torch.isfinite(ptr))
    assert torch.equal(torch.nan_to_num(got).view(torch.int32), torch.nan_to_num(ptr).view(torch.int32))


def test_buf_knob():
    assert nat.tune(nat.TUNE_CONV_X6_BUF, 0) == 1
    assert nat.tune(nat.TUNE_CONV_X6_BUF, 1) == 0
    with pytest.raises(ValueError):
        nat.tune(nat.TUNE_CONV_X6_BUF, 2)
    assert nat.tune(nat.TUNE_CONV_X6_BUF, 1) == 1


# ---------------------------------------------------------------------------
# the split
# ---------------------------------------------------------------------------
def _bf16_rne(bits):
    """fp32 bit patterns (uint32) -> bf16 bit patterns by round-to-nearest-even; a NaN keeps its sign and top payload
    bits and is made quiet (v_cvt_pk_bf16_f32)."""
    bits = bits.astype(np.uint64)
    nan = ((bits & 0x7F800000) == 0x7F800000) & ((bits & 0x007FFFFF) != 0)
    r = ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16).astype(np.uint32)
    return np.where(nan, ((bits >> 16) | 0x40).astype(np.uint32), r).astype(np.uint16)


def _split3_numpy(v):
    """split3 of csrc/bev_conv_x6.hip restated: h = bf16(v), r = v - h, m = bf16(r), l = bf16(r - m), the differences
    in fp32.  A NaN made by Inf - Inf is 0xFFC00000, the default quiet NaN of the GPU's fp32 adder (what the
    per-element split3 of the parent commit's library returns for +-Inf and for |v| >= 0x7F7F8000); a NaN operand is
    passed on quiet."""
    def up(h):
        return (h.astype(np.uint32) << 16).view(np.float32)

    def sub(a, b):
        with np.errstate(invalid="ignore"):
            d = (a - b).astype(np.float32)
        abits, dbits = a.view(np.uint32), d.view(np.uint32).copy()
        made = np.isnan(d) & ~np.isnan(a) & ~np.isnan(b)
        dbits[made] = 0xFFC00000
        passed = np.isnan(a)
        dbits[passed] = abits[passed] | 0x00400000
        return dbits.view(np.float32)

    h = _bf16_rne(v.view(np.uint32))
    r = sub(v, up(h))
    m = _bf16_rne(r.view(np.uint32))
    l = _bf16_rne(sub(r, up(m)).view(np.uint32))
    return np.stack([h, m, l])


def test_split3_bit_equal_to_numpy_restatement():
    """k_split3 (two elements per thread through split3x2) on 4,099 values -- an odd count, so the last thread holds
    one -- normal, subnormal, +-0, +-Inf, NaN, 0x7F7F8000 (the smallest value that rounds to a bf16 Inf) and its
    neighbours: every plane bit-equal to the per-element split."""
    rng = np.random.default_rng(7)
    special = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F7F8000, 0x7F7F7FFF,
                        0x7F7F8001, 0xFF7F8000, 0xFF7F7FFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x00000001, 0x807FFFFF, 0x00800000,
                        0x3F800000, 0x3F808000, 0x3F818000, 0x3F80FFFF, 0x7F800001, 0xFFA00000, 0x7FFFFFFF],
                       dtype=np.uint32)
    n = 4099
    normal = rng.standard_normal(3000).astype(np.float32) * np.exp2(rng.integers(-60, 60, 3000)).astype(np.float32)
    subn = rng.integers(1, 0x00800000, 500, dtype=np.uint32) | (rng.integers(0, 2, 500, dtype=np.uint32) << 31)
    edge = (0x7F7F0000 + rng.integers(0, 0x10000, n - 3500 - special.size, dtype=np.uint32)).astype(np.uint32)
    bits = np.concatenate([special, normal.view(np.uint32), subn, edge]).astype(np.uint32)
    assert bits.size == n
    x = torch.from_numpy(bits.view(np.float32).copy()).reshape(1, 1, 1, n).to(DEV)
    got = nat.split3(x).planes.view(torch.int16).cpu().numpy().view(np.uint16).reshape(3, n)
    ref = _split3_numpy(bits.view(np.float32))
    for p in range(3):
        bad = np.nonzero(got[p] != ref[p])[0]
        assert bad.size == 0, (p, [(hex(bits[i]), hex(got[p][i]), hex(ref[p][i])) for i in bad[:8]])


# The smallest shape of tests/test_chain_epilogue_gpu.py, (1, 31, 20) with 64 -> 64 -> 128 channels, and its
# 128-channel-h2 and dual neighbours: the chain's h2 split (two accumulator rows per split3x2) and the chains'
# buffer-form mainloops on an fp32 operand, against the separate launches.
@pytest.mark.parametrize("split", [False, True], ids=["fp32", "presplit"])
@pytest.mark.parametrize("chans", [(64, 64, 128), (128, 128, 128)], ids=["64x64x128", "128x128x128"])
def test_chain_equals_separate_launches(chans, split):
    N, H, W = 1, 31, 20
    Ci, Co, Co2 = chans
    g = torch.Generator().manual_seed(31 + Co2 + Ci)
    x = _guarded(torch.randn(N, H, W, Ci, generator=g))
    w2 = _nonzero(torch.randn(Co, Ci, 3, 3, generator=g) / (9 * Ci) ** 0.5).to(DEV)
    w3 = _nonzero(torch.randn(Co2, Co, 1, 1, generator=g) / Co ** 0.5).to(DEV)
    b2, b3 = (torch.randn(Co, generator=g) * 0.1).to(DEV), (torch.randn(Co2, generator=g) * 0.1).to(DEV)
    res = torch.randn(N, H, W, Co2, generator=g).to(DEV)
    p2, p3 = nat.pack_conv_weight_x6(w2), nat.pack_conv_weight_x6(w3)
    with nat.tuned(CONV_X6_BUF=0):
        h2 = nat.conv2d_nhwc_x6(x, p2, b2, Co, 3, 3, 1, 1, 1, 1)
        ref = nat.conv2d_nhwc_x6(h2, p3, b3, Co2, 1, 1, 1, 0, 1, 1, residual=res)
        ptr = nat.conv2d_chain_nhwc(x, p2, b2, Co, 3, 3, 1, 1, 1, p3, b3, Co2, 1, residual=res)
    got = nat.conv2d_chain_nhwc(nat.split3(x) if split else x, p2, b2, Co, 3, 3, 1, 1, 1, p3, b3, Co2, 1, residual=res)
    torch.cuda.synchronize()
    assert torch.isfinite(got).all()
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))
    assert torch.equal(ptr.view(torch.int32), ref.view(torch.int32))


def test_chain_dual_equals_separate_launches():
    N, H, W, Ci, Co, Co2 = 1, 31, 20, 64, 64, 256
    g = torch.Generator().manual_seed(48)
    x = _guarded(torch.randn(N, H, W, Ci, generator=g))
    xb = _guarded(torch.randn(N, H, W, 64, generator=g))
    w2 = _nonzero(torch.randn(Co, Ci, 3, 3, generator=g) / (9 * Ci) ** 0.5).to(DEV)
    w3 = _nonzero(torch.randn(Co2, Co + 64, 1, 1, generator=g) / (Co + 64) ** 0.5).to(DEV)
    b2, b3 = (torch.randn(Co, generator=g) * 0.1).to(DEV), (torch.randn(Co2, generator=g) * 0.1).to(DEV)
    p2, p3 = nat.pack_conv_weight_x6(w2), nat.pack_conv_weight_x6(w3)
    with nat.tuned(CONV_X6_BUF=0):
        h2 = nat.conv2d_nhwc_x6(x, p2, b2, Co, 3, 3, 1, 1, 1, 1)
        ref = nat.conv2d_dual_nhwc(h2, xb, 1, p3, b3, Co2, relu=True)
        ptr = nat.conv2d_chain_dual_nhwc(x, p2, b2, Co, 3, 3, 1, 1, 1, xb, 1, p3, b3, Co2, 1)
    got = nat.conv2d_chain_dual_nhwc(x, p2, b2, Co, 3, 3, 1, 1, 1, xb, 1, p3, b3, Co2, 1)
    torch.cuda.synchronize()
    assert torch.isfinite(got).all()
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))
    assert torch.equal(ptr.view(torch.int32), ref.view(torch.int32))
