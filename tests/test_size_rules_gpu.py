"""The 32-bit-offset size rules at their limits, and operands past 2 GiB.

Every hot kernel has a form with 32-bit offsets (raw buffer loads, one descriptor per workgroup) and a 64-bit pointer
form; the host code picks by comparing byte sizes against 2^31 or 2^32.  Each rule is run one pixel column (one pixel,
one row) inside and one outside its limit: the case restates the rule's left-hand side from the .hip source and asserts
on which side the shape lies and that its neighbour lies on the other.  The pointer forms and the streaming passes run
on tensors whose byte offsets cross 2^31, 2^32 and 2^33 and whose element indices cross 2^31.

  * Operands are torch.randn of a seeded device generator; nothing large crosses to the host; weights are nonzero.
  * Guard bands: every large operand is a slice of a NaN-filled allocation (>= one 128-row tile, for convs with taps
    two image rows, of NaN on each side); the whole output is asserted finite on the device.
  * Reference: float64 torch.nn.functional on the CPU on bands -- the first and last rows, the rows on both sides of
    every crossing of an input or output, with the input halo of the taps; reductions over all of M (statistics,
    column sums) against float64 torch on the device, accumulated in chunks.
  * Dispatch knobs (CONV_X6_BUF, CONV_H16_BUF): knob 1 against knob 0, torch.equal over the whole output, or, where
    two outputs would not fit, one int64 checksum per 2^20-element block of the first kept while the second runs.
  * Bars are those of the small-shape tests of the same kernel: 1e-5 of the output scale (tests/test_conv_x6_gpu.py),
    the fp32 summation bound of tests/test_conv_h16_gpu.py / test_conv_h16_half_gpu.py, exact for the passes that only
    move or select values.
  * Memory: no test holds more than 32 GiB (asserted from torch.cuda.max_memory_allocated), each frees its tensors and
    empties the cache, nothing is cached across tests, and a test skips when the device has less free than it needs.
  * test_which_form_ran: a kernel trace of the below-cap and above-cap calls in a child process -- the buffer instance
    below, the pointer instance above; without it a rule that always chose the pointer form would pass the rest.
"""
import csv
import glob
import os
import shutil
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import bev_native as nat
import size_rules_helper as S
from conftest import PKG, REPO

pytestmark = pytest.mark.gpu
DEV = S.DEV
X6_BUF_MAX = (1 << 31) - 16  # csrc/bev_conv_x6.hip


# ---------------------------------------------------------------------------
# the split-bf16 convs on an fp32 operand (k_conv_x6 / k_conv_x6b): conv_x6()'s `buf`
# ---------------------------------------------------------------------------
def x6_lhs(N, H, W, Ci, K, s, p, d):
    """conv_x6(): span H W Ci 4 + pad (W + 1) Ci 4, span = min(N, 128 / (Ho Wo) + 2); the buffer form runs while this
    is below X6_BUF_MAX."""
    Ho, Wo = S.out_hw(H, W, K, s, p, d)
    span = min(N, 128 // (Ho * Wo) + 2)
    return span * H * W * Ci * 4 + p * (W + 1) * Ci * 4


def x6_side(geom):
    """'buf' / 'ptr' by the restated rule, asserting the shape is within one pixel column of the limit."""
    N, H, W, Ci, Co, K, s, p, d = geom
    here = x6_lhs(N, H, W, Ci, K, s, p, d)
    if here < X6_BUF_MAX:
        assert x6_lhs(N, H, W + 1, Ci, K, s, p, d) >= X6_BUF_MAX, "not within one column of the limit"
        return "buf"
    assert x6_lhs(N, H, W - 1, Ci, K, s, p, d) < X6_BUF_MAX, "not within one column of the limit"
    return "ptr"


def x6_operands(geom, seed, residual):
    N, H, W, Ci, Co, K, s, p, d = geom
    g = S.gen(seed)
    Ho, Wo = S.out_hw(H, W, K, s, p, d)
    x = S.guarded((N, H, W, Ci), g, guard_pixels=max(128, 2 * W + 2))
    w = S.nonzero(torch.randn(Co, Ci, K, K, generator=g, device=DEV) / (Ci * K * K) ** 0.5)
    b = torch.randn(Co, generator=g, device=DEV) * 0.1
    res = S.guarded((N, Ho, Wo, Co), g) if residual else None
    return x, w, b, res


def x6_check_bands(y, x, w, b, res, geom, relu, meter):
    """y (fp32 [N, Ho, Wo, Co]) against float64 on the bands; 1e-5 of the output scale."""
    N, H, W, Ci, Co, K, s, p, d = geom
    w64, b64 = w.cpu().double(), b.cpu().double()
    worst, scale, rows = 0.0, 0.0, 0
    for band in S.conv_bands(N, H, W, Ci, Co, K, s, p, d):
        n, o0, o1 = band
        ref = S.conv_band_ref(x, w64, band, K, s, p, d)[0] + b64
        if res is not None:
            ref = ref + res[n, o0:o1].cpu().double()
        if relu:
            ref = torch.relu(ref)
        got = y[n, o0:o1].cpu().double()
        worst = max(worst, (got - ref).abs().max().item())
        scale = max(scale, ref.abs().max().item())
        rows += o1 - o0
    meter.note(f"{rows} band rows, max err {worst:.3e}, bar {1e-5 * scale:.3e}")
    assert worst <= 1e-5 * scale, (worst, scale)


# N, H, W, Ci, Co, K, stride, pad, dilation: one image (span 1) one pixel column inside / outside the cap
X6_CAP = [
    ("3x3-s1-w8190-inside", (1, 4096, 8190, 16, 16, 3, 1, 1, 1), "buf"),
    ("3x3-s1-w8191-outside", (1, 4096, 8191, 16, 16, 3, 1, 1, 1), "ptr"),
    ("3x3-s2-d2-w8188-inside", (1, 4096, 8188, 16, 16, 3, 2, 2, 2), "buf"),
    ("3x3-s2-d2-w8189-outside", (1, 4096, 8189, 16, 16, 3, 2, 2, 2), "ptr"),
    ("32deep-3x3-s1-w8188-inside", (1, 2048, 8188, 32, 16, 3, 1, 1, 1), "buf"),
    ("32deep-3x3-s1-w8189-outside", (1, 2048, 8189, 32, 16, 3, 1, 1, 1), "ptr"),
]


def test_x6_cap_arithmetic():
    """Case 1 of the issue by hand: 4096 x 8190 x 16 channels is 48 bytes under the cap."""
    assert x6_lhs(1, 4096, 8190, 16, 3, 1, 1, 1) == 2_147_483_584 == X6_BUF_MAX - 48
    assert [x6_side(c[1]) for c in X6_CAP] == [c[2] for c in X6_CAP]


@pytest.mark.parametrize("mode", ["bias", "res-relu"])
@pytest.mark.parametrize("case", X6_CAP, ids=[c[0] for c in X6_CAP])
def test_x6_one_image_at_the_cap(case, mode):
    name, geom, side = case
    assert x6_side(geom) == side
    N, H, W, Ci, Co, K, s, p, d = geom
    Ho, Wo = S.out_hw(H, W, K, s, p, d)
    ybytes = N * Ho * Wo * Co * 4
    S.need(N * H * W * Ci * 4 + 3 * ybytes + S.GIB)
    with S.Meter(f"x6-cap[{name}-{mode}]") as meter:
        x, w, b, res = x6_operands(geom, 11, mode == "res-relu")
        p6 = nat.pack_conv_weight_x6(w)
        act = 1 if mode == "res-relu" else 0
        y = nat.conv2d_nhwc_x6(x, p6, b, Co, K, K, s, p, d, act, residual=res)
        assert S.all_finite(y)
        if side == "buf":  # the pointer form of the same call
            with nat.tuned(CONV_X6_BUF=0):
                y0 = nat.conv2d_nhwc_x6(x, p6, b, Co, K, K, s, p, d, act, residual=res)
            assert torch.equal(y.view(torch.int32), y0.view(torch.int32))
            del y0
        x6_check_bands(y, x, w, b, res, geom, act == 1, meter)
        del x, y, res


def test_x6_many_images_past_4gib():
    """Five images, each just under half the cap (span 2): the per-workgroup base n_first * img crosses 2^31 and 2^32
    bytes, the last image's descriptor ends with the tensor."""
    geom = (5, 4096, 4095, 16, 16, 3, 2, 1, 1)
    N, H, W, Ci, Co, K, s, p, d = geom
    Ho, Wo = S.out_hw(H, W, K, s, p, d)
    assert min(N, 128 // (Ho * Wo) + 2) == 2 and x6_side(geom) == "buf"
    img = H * W * Ci * 4
    assert 2 * img < (1 << 31) < 3 * img and 4 * img < (1 << 32) < 5 * img  # both crossings inside the tensor
    S.need(N * img + 3 * N * Ho * Wo * Co * 4 + S.GIB)
    with S.Meter("x6-five-images") as meter:
        x, w, b, _ = x6_operands(geom, 12, False)
        p6 = nat.pack_conv_weight_x6(w)
        y = nat.conv2d_nhwc_x6(x, p6, b, Co, K, K, s, p, d, 0)
        with nat.tuned(CONV_X6_BUF=0):
            y0 = nat.conv2d_nhwc_x6(x, p6, b, Co, K, K, s, p, d, 0)
        assert S.all_finite(y)
        assert torch.equal(y.view(torch.int32), y0.view(torch.int32))
        del y0
        bands = S.conv_bands(N, H, W, Ci, Co, K, s, p, d)
        assert {n for n, _, _ in bands} >= {0, 2, 4}  # first rows, the 2^31 crossing (image 2), 2^32 and last (image 4)
        x6_check_bands(y, x, w, b, None, geom, False, meter)
        del x, y


# 1x1 / stride 1 / pad 0 (the linear form): three images of 3345 x 3345 pixels, M = 33,567,075 = 2^25 + 12,643
PW_GEOM = (3, 3345, 3345, 16)


def pw_check(y_rows, x2d, w, b, Co, meter, what):
    """y_rows(m0, m1) -> fp32 [m1 - m0, Co] of the output; x2d [M, Ci]."""
    M, Ci = x2d.shape
    w64, b64 = w.reshape(Co, Ci).cpu().double(), b.cpu().double()
    worst, scale, rows = 0.0, 0.0, 0
    for m0, m1 in S.row_bands(M, [(Ci, 4), (Co, 4), (Co, 2)], S.plane_crossing_rows(Co, 2, M, 3)):  # split planes too
        ref = x2d[m0:m1].cpu().double() @ w64.t() + b64
        worst = max(worst, (y_rows(m0, m1).cpu().double() - ref).abs().max().item())
        scale = max(scale, ref.abs().max().item())
        rows += m1 - m0
    meter.note(f"{what}: {rows} band rows, max err {worst:.3e}, bar {1e-5 * scale:.3e}")
    assert worst <= 1e-5 * scale, (what, worst, scale)


@pytest.mark.parametrize("Co,split", [(64, False), (128, False), (64, True)], ids=["co64", "co128", "co64-split-out"])
def test_x6_pointwise_large_output(Co, split):
    """x crosses 2^31 bytes; y crosses 2^31 elements and 2^32 and 2^33 bytes (Co = 128: 2^32 elements and 2^34 bytes
    too); split output: the plane stride yps is past 2^31 elements."""
    N, H, W, Ci = PW_GEOM
    M = N * H * W
    assert M > 1 << 25 and M % 128 != 0 and x6_lhs(N, H, W, Ci, 1, 1, 0, 1) < X6_BUF_MAX
    assert M * Ci * 4 > 1 << 31 and M * Co > 1 << 31 and M * Co * 4 > 1 << 33
    ybytes = M * Co * (6 if split else 4)
    S.need(M * Ci * 4 + ybytes + S.GIB)
    with S.Meter(f"x6-pointwise[co{Co}{'-split' if split else ''}]") as meter:
        g = S.gen(13 + Co)
        x = S.guarded((N, H, W, Ci), g)
        w = S.nonzero(torch.randn(Co, Ci, 1, 1, generator=g, device=DEV) / Ci ** 0.5)
        b = torch.randn(Co, generator=g, device=DEV) * 0.1
        p6 = nat.pack_conv_weight_x6(w)

        def run():
            return nat.conv2d_nhwc_x6(x, p6, b, Co, 1, 1, 1, 0, 1, 0, split_out=split)

        with nat.tuned(CONV_X6_BUF=0):
            y0 = run()
            sums0 = S.checksums(y0.planes if split else y0)
            del y0
        y = run()
        data = y.planes if split else y
        assert S.all_finite(data)
        assert torch.equal(S.checksums(data), sums0)
        if split:
            assert M * Co > 1 << 31  # yps
            planes = data.view(3, M, Co)

            def rows(m0, m1):
                q = planes[:, m0:m1].float()
                return (q[0] + q[1]) + q[2]
        else:
            flat = data.view(M, Co)

            def rows(m0, m1):
                return flat[m0:m1]
        pw_check(rows, x.view(M, Ci), w, b, Co, meter, "y")
        del x, y, data


DUAL = [("w2-8191-inside", 8191, "buf"), ("w2-8192-outside", 8192, "ptr")]


@pytest.mark.parametrize("case", DUAL, ids=[c[0] for c in DUAL])
def test_x6_dual_second_operand_at_its_limit(case):
    """conv_x6(): span H2 W2 Ci2 4 < X6_BUF_MAX for x2 (no padding bias), one pixel column inside and outside."""
    _, W2, side = case
    N, H2, Ci, Ci2, Co, s2 = 1, 4096, 16, 16, 64, 2
    Ho, Wo = (H2 - 1) // s2 + 1, (W2 - 1) // s2 + 1

    def lhs2(w2):
        return min(N, 128 // (Ho * Wo) + 2) * H2 * w2 * Ci2 * 4

    assert (lhs2(W2) < X6_BUF_MAX) == (side == "buf")
    assert lhs2(W2 + 1) >= X6_BUF_MAX and lhs2(W2 - 1) < X6_BUF_MAX
    assert x6_lhs(N, Ho, Wo, Ci, 1, 1, 0, 1) < X6_BUF_MAX  # x itself is far inside
    S.need(H2 * W2 * Ci2 * 4 + Ho * Wo * (Ci + 2 * Co) * 4 + S.GIB)
    with S.Meter(f"x6-dual[{case[0]}]") as meter:
        g = S.gen(14)
        x = S.guarded((N, Ho, Wo, Ci), g)
        x2 = S.guarded((N, H2, W2, Ci2), g, guard_pixels=2 * W2 + 2)
        w1 = S.nonzero(torch.randn(Co, Ci, generator=g, device=DEV) / Ci ** 0.5)
        w2 = S.nonzero(torch.randn(Co, Ci2, generator=g, device=DEV) / Ci2 ** 0.5)
        b = torch.randn(Co, generator=g, device=DEV) * 0.1
        p6 = nat.pack_conv_weight_x6(torch.cat([w1, w2], 1).reshape(Co, Ci + Ci2, 1, 1).contiguous())
        y = nat.conv2d_dual_nhwc(x, x2, s2, p6, b, Co, relu=True)
        assert S.all_finite(y)
        if side == "buf":
            with nat.tuned(CONV_X6_BUF=0):
                y0 = nat.conv2d_dual_nhwc(x, x2, s2, p6, b, Co, relu=True)
            assert torch.equal(y.view(torch.int32), y0.view(torch.int32))
            del y0
        w1d, w2d, bd = w1.cpu().double(), w2.cpu().double(), b.cpu().double()
        worst, scale = 0.0, 0.0
        rows = {0, Ho - 1} | {min(Ho - 1, r // s2) for r in S.crossing_rows(W2 * Ci2, 4, H2)}
        for o0, o1 in S.merge(rows, Ho):
            a = x[0, o0:o1].cpu().double()
            c = x2[0, o0 * s2:(o1 - 1) * s2 + 1:s2, ::s2].cpu().double()
            ref = torch.relu(a @ w1d.t() + c @ w2d.t() + bd)
            worst = max(worst, (y[0, o0:o1].cpu().double() - ref).abs().max().item())
            scale = max(scale, ref.abs().max().item())
        meter.note(f"max err {worst:.3e}, bar {1e-5 * scale:.3e}")
        assert worst <= 1e-5 * scale, (worst, scale)
        del x, x2, y


# ---------------------------------------------------------------------------
# the fp16 convs (k_conv_h16b): conv_h16()'s `buf`
# ---------------------------------------------------------------------------
H16_BUF_MAX = (1 << 31) - 16  # csrc/bev_conv_h16.hip


def h16_side(N, H, W, Ci):
    """conv_h16(): an fp16 operand is staged by buffer loads while N H W Ci 2 < 2^31 - 16; within one pixel."""
    here = N * H * W * Ci * 2
    if here < H16_BUF_MAX:
        assert here + Ci * 2 >= H16_BUF_MAX, "not within one pixel of the limit"
        return "buf"
    assert here - Ci * 2 < H16_BUF_MAX, "not within one pixel of the limit"
    return "ptr"


# The fp16-operand entries take Ci % 64 == 0 (one 64-deep K step), so the pixel is 128 bytes: M = 2^24 - 1 = 4095 x 4097
# pixels is one pixel under the limit, M = 2^24 one pixel at it.
H16_UNDER, H16_AT = (1, 4095, 4097, 64), (1, 4096, 4096, 64)


def test_h16_cap_arithmetic():
    assert 4095 * 4097 == (1 << 24) - 1
    assert h16_side(*H16_UNDER) == "buf" and h16_side(*H16_AT) == "ptr"


def h16_bands_check(y, x, w, b, geom, K, pad, out_half, meter):
    """The bars of tests/test_conv_h16_gpu.py (fp32 out) and tests/test_conv_h16_half_gpu.py (fp16 out): float64 conv
    of the fp16-rounded operands, worst-case fp32 summation bound Kt 2^-24 sum |terms| per output."""
    N, H, W, Ci = geom
    Co = w.shape[0]
    wh, b64 = w.half().cpu().double(), b.cpu().double()
    Kt = Ci * K * K
    worst = 0.0
    for band in S.conv_bands(N, H, W, Ci, Co, K, 1, pad, 1, x_esize=x.element_size(), y_esize=y.element_size()):
        n, o0, o1 = band
        z, mag = S.conv_band_ref(x, wh, band, K, 1, pad, 1, round_x=torch.float16)
        ref = z + b64
        err = (y[n, o0:o1].cpu().double() - ref).abs()
        if out_half:
            bound = 2.0 ** -11 * ref.abs() + (Kt + 2) * 2.0 ** -24 * (mag + b64.abs()) + 2.0 ** -24
        else:
            bound = Kt * 2.0 ** -24 * (mag + b64.abs()) + 1e-6
            assert float((err / (mag + 1e-3)).max()) < 2e-6
        assert bool((err <= bound).all()), float((err - bound).max())
        worst = max(worst, float((err / bound).max()))
    meter.note(f"max err / bound {worst:.3f}")


H16_CASES = [
    ("1x1-under-f32out", H16_UNDER, 1, "f32"),
    ("1x1-at-f32out", H16_AT, 1, "f32"),
    ("1x1-under-f16out", H16_UNDER, 1, "f16"),
    ("1x1-at-f16out", H16_AT, 1, "f16"),
    ("3x3-under-f32out", H16_UNDER, 3, "f32"),
    ("3x3-at-f32out", H16_AT, 3, "f32"),
    ("3x3-under-f16out", H16_UNDER, 3, "f16"),
    ("1x1-under-stats", H16_UNDER, 1, "stats"),
    ("1x1-at-stats", H16_AT, 1, "stats"),
]


@pytest.mark.parametrize("case", H16_CASES, ids=[c[0] for c in H16_CASES])
def test_h16_operand_at_the_cap(case):
    name, geom, K, out = case
    N, H, W, Ci = geom
    side = h16_side(*geom)
    assert side == ("buf" if geom == H16_UNDER else "ptr")
    Co, pad, M = 8, K // 2, N * H * W
    S.need(M * Ci * 2 + 2 * M * Co * 4 + S.GIB)
    with S.Meter(f"h16-cap[{name}]") as meter:
        g = S.gen(21 + K)
        x = S.guarded((N, H, W, Ci), g, dtype=torch.float16, guard_pixels=max(128, 2 * W + 2))
        w = S.nonzero(torch.randn(Co, Ci, K, K, generator=g, device=DEV) / (Ci * K * K) ** 0.5)
        b = torch.randn(Co, generator=g, device=DEV)
        ph = nat.pack_conv_weight_h16(w)

        def run():
            if out == "f16":
                return nat.conv2d_h16_half(x, ph, b, Co, K, K, 1, pad), None
            if out == "stats":
                return nat.conv2d_h16_any(x, ph, Co, K, K, 1, pad, stats=True)
            return nat.conv2d_h16_any(x, ph, Co, K, K, 1, pad, bias=b), None

        y, tiles = run()
        assert S.all_finite(y)
        if side == "buf":
            with nat.tuned(CONV_H16_BUF=0):
                y0, tiles0 = run()
            assert torch.equal(y, y0)
            assert tiles is None or torch.equal(tiles, tiles0)
            del y0, tiles0
        zero = torch.zeros_like(b)
        h16_bands_check(y, x, w, zero if out == "stats" else b, geom, K, pad, out == "f16", meter)
        if out == "stats":
            # the tile partials (sum, sum of squared deviations from the tile mean, per 128 rows) against float64 torch
            # of the kernel's own output, on the device: every tile, first to last
            nt = (M + 127) // 128
            assert tiles.shape == (Co, nt, 2) and S.all_finite(tiles)
            z = y.view(M, Co)
            full = M // 128
            zt = z[:full * 128].view(full, 128, Co).double()
            s1 = zt.sum(1)
            m2 = ((zt - s1[:, None] / 128) ** 2).sum(1)
            if full < nt:
                tail = z[full * 128:].double()
                s1 = torch.cat([s1, tail.sum(0, keepdim=True)])
                m2 = torch.cat([m2, ((tail - tail.mean(0)) ** 2).sum(0, keepdim=True)])
            del zt
            zmax = z.abs().max().item()
            e1 = (tiles[:, :, 0].t() - s1).abs()
            e2 = (tiles[:, :, 1].t() - m2).abs()
            # fp32 arithmetic over a tile's 128 rows.  Sum: 128 additions, each 2^-24 of a partial sum <= 128 max |z|.
            # M2: a deviation d carries 2^-23 (|z| + |mean|) <= 2^-22 max |z|, so sum d^2 carries
            # 2^-21 max |z| sum |d| <= 2^-21 max |z| sqrt(128 M2), plus 129 roundings of the accumulation.
            b1 = 128 * 2.0 ** -24 * 128 * zmax
            b2 = 2.0 ** -21 * zmax * (128 * m2).sqrt() + 129 * 2.0 ** -24 * m2 + 1e-30
            meter.note(f"tile sums: max err {e1.max().item():.3e}, bar {b1:.3e}; M2 max err / bar "
                       f"{(e2 / b2).max().item():.3f}")
            assert e1.max().item() <= b1 and bool((e2 <= b2).all())
        del x, y, tiles


def test_h16_fp32_operand_of_the_same_size():
    """An fp32 operand has no buffer form: the pointer form on 4 GiB, byte offsets crossing 2^31 and 2^32."""
    N, H, W, Ci = H16_AT
    Co, M = 8, N * H * W
    assert M * Ci * 4 == 1 << 32
    geom = (1, H + 1, W, Ci)  # one row more: the 2^32 crossing lies inside
    M = (H + 1) * W
    S.need(M * Ci * 4 + M * Co * 4 + S.GIB)
    with S.Meter("h16-fp32-operand") as meter:
        g = S.gen(23)
        x = S.guarded(geom, g, guard_pixels=2 * W + 2)
        w = S.nonzero(torch.randn(Co, Ci, 3, 3, generator=g, device=DEV) / (Ci * 9) ** 0.5)
        b = torch.randn(Co, generator=g, device=DEV)
        ph = nat.pack_conv_weight_h16(w)
        y = nat.conv2d_h16_any(x, ph, Co, 3, 3, 1, 1, bias=b)
        assert S.all_finite(y)
        h16_bands_check(y, x, w, b, geom, 3, 1, False, meter)
        del x, y


# ---------------------------------------------------------------------------
# the fp16 weight gradient: k_wgrad_h16c (32-bit offsets) inside its two rules, k_wgrad_h16b outside
# ---------------------------------------------------------------------------
WMS2 = 64  # csrc/bev_conv_h16.hip: pixel rows per step


def wgrad_rules(M, Ci, Co):
    """bev_conv_wgrad_h16_ex_f32 (1x1 / stride 1, so N H W = M): k_wgrad_h16c runs while M Co < 2^31 - WMS2 Co and
    N H W Ci < 2^31."""
    return M * Co < (1 << 31) - WMS2 * Co, M * Ci < (1 << 31)


def product64(a, b, rows=1 << 18):
    """a^T b over all rows in float64 and, from the same operands in the same chunks, in plain fp32 torch -- the
    measure of what fp32 accumulation costs on this product."""
    M = a.shape[0]
    r64 = torch.zeros(a.shape[1], b.shape[1], dtype=torch.float64, device=DEV)
    r32 = torch.zeros(a.shape[1], b.shape[1], dtype=torch.float32, device=DEV)
    for m0 in range(0, M, rows):
        ac, bc = a[m0:m0 + rows], b[m0:m0 + rows]
        r64 += ac.double().t() @ bc.double()
        r32 += ac.float().t() @ bc.float()
    return r64, r32


def wgrad_check(dw, r64, r32, meter, what):
    """The bar is measured: four times the error of the plain fp32 product against float64, relative to the output
    scale (the kernel's summation order is unspecified; a misaddressed row costs an order of magnitude more)."""
    scale = r64.abs().max().item()
    e32 = (r32.double() - r64).abs().max().item() / scale
    ek = (dw.double() - r64).abs().max().item() / scale
    meter.note(f"{what}: kernel err {ek:.3e}, plain fp32 torch err {e32:.3e}, bar {4 * e32:.3e} (of the output scale)")
    assert bool(torch.isfinite(dw).all())
    assert ek <= 4 * e32, (what, ek, e32)


WGRAD = [
    ("co512-m-inside", (1 << 22) - WMS2 - 1, 8, 512, True),
    ("co512-m-outside", (1 << 22) - WMS2, 8, 512, False),
    ("ci512-m-inside", (1 << 22) - 1, 512, 8, True),
    ("ci512-m-outside", 1 << 22, 512, 8, False),
]


@pytest.mark.parametrize("case", WGRAD, ids=[c[0] for c in WGRAD])
def test_wgrad_h16_rules(case):
    name, M, Ci, Co, inside = case
    assert all(wgrad_rules(M, Ci, Co)) == inside
    if inside:  # one pixel more leaves the 32-bit kernel
        assert not all(wgrad_rules(M + 1, Ci, Co))
    else:
        assert all(wgrad_rules(M - 1, Ci, Co))
    S.need(M * (Ci + Co) * 2 + 4 * S.GIB)
    with S.Meter(f"wgrad-h16[{name}]") as meter:
        g = S.gen(51)
        x = S.guarded((1, 1, M, Ci), g, dtype=torch.float16)
        dz = S.guarded((1, 1, M, Co), g, dtype=torch.float16)
        dw = nat.conv_wgrad_h16_any(x, dz, 1, 1, 1, 0)
        assert dw.shape == (Co, Ci, 1, 1)
        r64, r32 = product64(dz.view(M, Co), x.view(M, Ci))
        wgrad_check(dw.view(Co, Ci), r64, r32, meter, name)
        del x, dz


def test_wgrad_f32_past_2_31_elements():
    """The fp32 weight gradient (k_wgrad_nat, the default): dz [M, 512] with M Co = 2^31 + 512 * 4099 elements."""
    M, Ci, Co = (1 << 22) + 4099, 8, 512
    assert M * Co > 1 << 31
    S.need(M * (Ci + Co) * 4 + 4 * S.GIB)
    with S.Meter("wgrad-f32") as meter:
        g = S.gen(52)
        x = S.guarded((1, 1, M, Ci), g)
        dz = S.guarded((1, 1, M, Co), g)
        dw = nat.conv_wgrad(x, dz, 1, 1, 1, 0)
        r64, r32 = product64(dz.view(M, Co), x.view(M, Ci))
        wgrad_check(dw.reshape(Co, Ci), r64, r32, meter, "k_wgrad_nat")
        del x, dz


# ---------------------------------------------------------------------------
# the pre-split operand (k_conv_x6s): plane stride xps past 2^31 elements; conv_x6() has no size rule for it
# ---------------------------------------------------------------------------
def test_x6s_presplit_plane_stride_past_2_31():
    """3x3 / 1 / 1 over a Split3 of [1, 8193, 8193, 32]: xps = 2^31 + 2^19 + 32 elements, plane 1 starts past 4 GiB.
    k_conv_x6s addresses by 64-bit pointers (LDS-DMA sources): read, nothing to fix.  The reference runs on the fp32
    values the planes hold (h + m + l is exact)."""
    geom = (1, 8193, 8193, 32, 16, 3, 1, 1, 1)
    N, H, W, Ci, Co, K, s, p, d = geom
    xps = N * H * W * Ci
    assert xps > 1 << 31
    S.need(xps * 4 + xps * 6 + S.GIB)
    with S.Meter("x6s-presplit") as meter:
        g = S.gen(61)
        x = S.guarded((N, H, W, Ci), g, guard_pixels=2 * W + 2)
        w = S.nonzero(torch.randn(Co, Ci, K, K, generator=g, device=DEV) / (Ci * K * K) ** 0.5)
        b = torch.randn(Co, generator=g, device=DEV) * 0.1
        xs = nat.split3(x)
        # crossings of y and of the three bf16 planes, counted from the planes' allocation (plane 1 starts past 4 GiB)
        bands = S.conv_bands(N, H, W, Ci, Co, K, s, p, d, x_esize=2, x_rows=S.plane_crossing_rows(W * Ci, 2, H, 3))
        keep = {}
        for n, o0, o1 in bands:  # the fp32 rows the bands need, then x goes
            lo, hi = max(0, o0 - 1), min(H, o1 + 1)
            keep[(n, o0, o1)] = (lo, x[n, lo:hi].cpu())
            q = xs.planes[:, n, lo:hi].float()
            assert torch.equal(((q[0] + q[1]) + q[2]).cpu(), keep[(n, o0, o1)][1])
        del x
        y = nat.conv2d_nhwc_x6(xs, nat.pack_conv_weight_x6(w), b, Co, K, K, s, p, d, 0)
        assert S.all_finite(y)
        w64, b64 = w.cpu().double(), b.cpu().double()
        worst, scale = 0.0, 0.0
        for band in bands:
            n, o0, o1 = band
            lo, rows = keep[band]
            ref = band_ref_rows(rows, lo, H, w64, band, K, s, p, d) + b64
            worst = max(worst, (y[n, o0:o1].cpu().double() - ref).abs().max().item())
            scale = max(scale, ref.abs().max().item())
        meter.note(f"max err {worst:.3e}, bar {1e-5 * scale:.3e}")
        assert worst <= 1e-5 * scale, (worst, scale)
        del xs, y


def band_ref_rows(rows, lo, H, w64, band, K, s, p, d):
    """S.conv_band_ref for input rows kept on the host: rows = x[n, lo:lo + len(rows)]."""
    n, oy0, oy1 = band
    iy0, iy1 = oy0 * s - p, (oy1 - 1) * s - p + d * (K - 1) + 1
    a, b = max(iy0, 0), min(iy1, H)
    xs = rows[a - lo:b - lo].double().permute(2, 0, 1)[None]
    xs = F.pad(xs, (p, p, a - iy0, iy1 - b))
    return F.conv2d(xs, w64, None, stride=s, dilation=d)[0].permute(1, 2, 0)


def test_x6s_layer1_chain_plane_stride_past_2_31():
    """The layer1 chain on a pre-split operand (the strip kernel: 3x3 / 1 / 1 over 64 channels, then 1x1 to 64, ReLU
    after each) on [1, 5793, 5793, 64]: xps = 2^31 + 282,688 elements.  Against float64 of the two convs on bands,
    1e-5 of the output scale."""
    N, H, W, Ci, Co, Co2 = 1, 5793, 5793, 64, 64, 64
    xps = N * H * W * Ci
    assert xps == (1 << 31) + 282_688
    S.need(xps * 4 + xps * 6 + S.GIB)
    with S.Meter("x6s-chain") as meter:
        g = S.gen(62)
        x = S.guarded((N, H, W, Ci), g, guard_pixels=2 * W + 2)
        w2 = S.nonzero(torch.randn(Co, Ci, 3, 3, generator=g, device=DEV) / (9 * Ci) ** 0.5)
        w3 = S.nonzero(torch.randn(Co2, Co, 1, 1, generator=g, device=DEV) / Co ** 0.5)
        b2 = torch.randn(Co, generator=g, device=DEV) * 0.1
        b3 = torch.randn(Co2, generator=g, device=DEV) * 0.1
        xs = nat.split3(x)
        bands = S.conv_bands(N, H, W, Ci, Co2, 3, 1, 1, 1, x_esize=2, x_rows=S.plane_crossing_rows(W * Ci, 2, H, 3))
        keep = {bd: (max(0, bd[1] - 1), x[bd[0], max(0, bd[1] - 1):min(H, bd[2] + 1)].cpu()) for bd in bands}
        del x
        y = nat.conv2d_chain_nhwc(xs, nat.pack_conv_weight_x6(w2), b2, Co, 3, 3, 1, 1, 1,
                                  nat.pack_conv_weight_x6(w3), b3, Co2, 1)
        assert y.shape == (N, H, W, Co2) and S.all_finite(y)
        w2d, w3d = w2.cpu().double(), w3.reshape(Co2, Co).cpu().double()
        worst, scale = 0.0, 0.0
        for band in bands:
            n, o0, o1 = band
            lo, rows = keep[band]
            h2 = torch.relu(band_ref_rows(rows, lo, H, w2d, band, 3, 1, 1, 1) + b2.cpu().double())
            ref = torch.relu(h2 @ w3d.t() + b3.cpu().double())
            worst = max(worst, (y[n, o0:o1].cpu().double() - ref).abs().max().item())
            scale = max(scale, ref.abs().max().item())
        meter.note(f"max err {worst:.3e}, bar {1e-5 * scale:.3e}")  # the x6 bar of tests/test_conv_x6_gpu.py, unchanged
        assert worst <= 1e-5 * scale, (worst, scale)
        del xs, y


# ---------------------------------------------------------------------------
# EfficientNet expansion + depthwise (k_irdw, k_irdw_h16): per-image 32-bit offsets, refused past them
# ---------------------------------------------------------------------------
def ir_rules(H, W, Ci, Cm, K, s):
    """bev_ir_expand_dw_f32 / _h16: H W Ci >= 2^31 or Ho Wo Cm >= 2^31 is BEV_ERR_ARGS."""
    Ho, Wo = S.out_hw(H, W, K, s, K // 2, 1)
    return H * W * Ci < 1 << 31, Ho * Wo * Cm < 1 << 31


# H, W, Ci, Cm, K, stride.  Cm is a multiple of 48, so Ho Wo Cm cannot equal 2^31: the first row count past it
IR_CASES = [
    ("input-at-2^31", (16384, 8192, 16, 48, 3, 2), False),
    ("input-one-row-less", (16383, 8192, 16, 48, 3, 2), True),
    ("output-past-2^31", (5462, 8192, 16, 48, 3, 1), False),
    ("output-one-row-less", (5461, 8192, 16, 48, 3, 1), True),
]


def silu64(z):
    return z * torch.sigmoid(z)


def ir_band_ref(x, we, be, wd, bd, band, geom, rounded):
    """float64 1x1 -> SiLU -> depthwise -> SiLU of the output rows of `band` (the depthwise pads the expanded tensor
    with zeros); rounded: with the fp16 kernel's rounding points (fp16 weights, h and y rounded to fp16)."""
    H, W, Ci, Cm, K, s = geom
    r = (lambda t: t.half().double()) if rounded else (lambda t: t.double())
    _, o0, o1 = band
    p = K // 2
    iy0, iy1 = o0 * s - p, (o1 - 1) * s - p + K
    lo, hi = max(iy0, 0), min(iy1, H)
    xs = x[0, lo:hi].cpu().double()
    h = r(silu64(xs @ r(we.cpu()).t() + be.cpu().double())).permute(2, 0, 1)[None]
    h = F.pad(h, (p, p, lo - iy0, iy1 - hi))
    w64 = r(wd.cpu()).t().reshape(Cm, 1, K, K)
    return r(silu64(F.conv2d(h, w64, bd.cpu().double(), s, 0, groups=Cm)))[0].permute(1, 2, 0)


@pytest.mark.parametrize("half", [False, True], ids=["f32", "h16"])
@pytest.mark.parametrize("case", IR_CASES, ids=[c[0] for c in IR_CASES])
def test_effnet_per_image_rules(case, half):
    name, geom, runs = case
    H, W, Ci, Cm, K, s = geom
    assert all(ir_rules(*geom)) == runs
    assert all(ir_rules(H - 1, W, Ci, Cm, K, s)) and not all(ir_rules(H + 1, W, Ci, Cm, K, s))  # within one row
    Ho, Wo = S.out_hw(H, W, K, s, K // 2, 1)
    es = 2 if half else 4
    dt = torch.float16 if half else torch.float32
    S.need((H * W * Ci + Ho * Wo * Cm) * es + 2 * S.GIB)
    with S.Meter(f"effnet[{name}-{'h16' if half else 'f32'}]") as meter:
        g = S.gen(71)
        x = S.guarded((1, H, W, Ci), g, dtype=dt, guard_pixels=2 * W + 2)
        we = torch.randn(Cm, Ci, generator=g, device=DEV) / Ci ** 0.5
        be = 0.2 * torch.randn(Cm, generator=g, device=DEV)
        wd = 0.3 * torch.randn(K * K, Cm, generator=g, device=DEV)
        bd = 0.2 * torch.randn(Cm, generator=g, device=DEV)
        wek, wdk = (we.half(), wd.half()) if half else (we, wd)  # the references round the fp32 weights themselves
        if not runs:  # the C entry itself, on real allocations: refused, the output's fill untouched
            nb = nat.lib().bev_ir_expand_dw_blocks(Ho, Wo, K, s)
            y = S.filled((1, Ho, Wo, Cm), dt)
            ps = S.filled((1, nb, Cm))
            fn = nat.lib().bev_ir_expand_dw_h16 if half else nat.lib().bev_ir_expand_dw_f32
            rc = fn(nat._ptr(x), 1, H, W, Ci, nat._ptr(wek), nat._ptr(be), Cm, nat._ptr(wdk), nat._ptr(bd), K, s,
                    nat._ptr(y), Ho, Wo, nat._ptr(ps), nat._stream(x))
            torch.cuda.synchronize()
            assert rc == nat.BEV_ERR_ARGS
            assert S.all_nan(y) and S.all_nan(ps)
            del x, y
            return
        y, ps = (nat.ir_expand_dw_h16 if half else nat.ir_expand_dw)(x, wek, be, wdk, bd, K, s)
        assert S.all_finite(y) and S.all_finite(ps)
        # the SE partial sums [1, nb, Cm] add up to the channel sums of the returned y (float64 on the device, in
        # chunks): 1e-5 max(1, max |sum|), the bar of test_irdw_instances / test_irdw_h16_instances
        y2 = y.view(Ho * Wo, Cm)
        sums = sum(y2[m0:m0 + (1 << 20)].double().sum(0) for m0 in range(0, Ho * Wo, 1 << 20))
        perr = (ps.double().sum(1)[0] - sums).abs().max().item()
        meter.note(f"partial sums err {perr:.3e}, bar {1e-5 * max(1.0, sums.abs().max().item()):.3e}")
        assert perr <= 1e-5 * max(1.0, sums.abs().max().item()), perr
        bands = S.conv_bands(1, H, W, Ci, Cm, K, s, K // 2, 1, x_esize=es, y_esize=es)
        if not half:  # tests/test_kernel_instances_gpu.py test_irdw_instances: 1e-5 of the output scale
            worst, scale = 0.0, 0.0
            for band in bands:
                ref = ir_band_ref(x, we, be, wd, bd, band, geom, False)
                worst = max(worst, (y[0, band[1]:band[2]].cpu().double() - ref).abs().max().item())
                scale = max(scale, ref.abs().max().item())
            meter.note(f"max err {worst:.3e}, bar {1e-5 * scale:.3e}")
            assert worst <= 1e-5 * scale, (worst, scale)
        else:  # tests/test_effnet_h16_kernels_gpu.py: against the exact forward no worse than 1.5 x (L2) / 2 x (max)
            # the float64 sums with the kernel's rounding points, and at most 1 % of the outputs off their fp16 rounding
            got = torch.cat([y[0, b[1]:b[2]].cpu().reshape(-1) for b in bands])
            exact = torch.cat([ir_band_ref(x, we, be, wd, bd, b, geom, False).reshape(-1) for b in bands])
            r64 = torch.cat([ir_band_ref(x, we, be, wd, bd, b, geom, True).reshape(-1) for b in bands])
            l2 = float((got.double() - exact).norm() / (r64 - exact).norm())
            mx = float((got.double() - exact).abs().max() / (r64 - exact).abs().max())
            off = float((got != r64.half()).double().mean())
            meter.note(f"L2 ratio {l2:.3f}, max ratio {mx:.3f}, off f16(R64) {100 * off:.3f} %")
            assert l2 <= 1.5 and mx <= 2.0 and off <= 0.01
        del x, y


# ---------------------------------------------------------------------------
# the fused warp: warp_fuse_impl()'s dma_ok and the two output-layout rules
# ---------------------------------------------------------------------------
BOUNDS = (-24.0, 24.0, -7.2, 7.2)


def warp_setup(V, C, Hf, Wf, Hb, Wb, seed, strides=None):
    """Channels-last features (guarded), homographies of the synthetic rig, BEV axes, image size.  strides = (sH, sW):
    one view whose rows / pixels lie that many elements apart inside a NaN-filled allocation."""
    from bev_rig import rig
    from models.fusion.geometry import GeometryTransformer
    img = (8 * Hf, 8 * Wf)
    K, Rt = rig(V, img[0], img[1], 1)
    g = GeometryTransformer(Hb, Wb, BOUNDS)
    H = g.homographies(torch.from_numpy(K).to(DEV), torch.from_numpy(Rt).to(DEV), 1, V, torch.device(DEV))
    xs, ys = (a.to(DEV) for a in g._axes_cpu)
    if strides is not None:
        assert V == 1
        sH, sW = strides
        ext = (Hf - 1) * sH + (Wf - 1) * sW + C
        base = S.filled((ext + 8192,))
        feats = base.as_strided((1, 1, C, Hf, Wf), (ext, ext, 1, sH, sW), 4096)
        feats.copy_(torch.randn(1, 1, C, Hf, Wf, generator=S.gen(seed), device=DEV))
        assert feats.data_ptr() % 16 == 0
        return feats, H, xs, ys, img
    f = S.guarded((1, V, Hf, Wf, C), S.gen(seed), guard_pixels=2 * Wf + 2)
    return f.permute(0, 1, 4, 2, 3), H, xs, ys, img


def warp_band_ref(oracle, feats, H, xs, ys, img, mode, r0, r1):
    """The reference the warp tests use (the CPU oracle, bit for bit) on BEV rows [r0, r1): [C, rows, Wb]."""
    per = oracle.warp(feats[0].contiguous().cpu().numpy(), H.cpu().numpy(), xs.cpu().numpy(),
                      ys[r0:r1].cpu().numpy(), img)
    return torch.from_numpy(oracle.fuse(per[None], mode)[0])


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


WARP_DMA = [("c64-under", 64, 4095, "dma"), ("c128-under", 128, 4095, "dma"), ("c64-over", 64, 4096, "ck")]


@pytest.mark.parametrize("case", WARP_DMA, ids=[c[0] for c in WARP_DMA])
def test_warp_output_planes_at_4gib(case, oracle):
    """dma_ok: Hb Wb 64 4 < 2^32 -- the LDS-DMA kernel one BEV row under it (4095 x 4096 cells), the register-staged
    kernel (launch_fuse_ck) at it.  NCHW output of 4 / 8 GiB, bit-identical to the oracle on bands of BEV rows: first,
    last, and the rows in which the output's byte offset crosses 2^31 and 2^32."""
    name, C, Hb, side = case
    V, Hf, Wf, Wb = 2, 16, 28, 4096
    lhs = Hb * Wb * 64 * 4
    assert (lhs < 1 << 32) == (side == "dma") and (Hb - 1) * Wb * 256 < 1 << 32 <= (Hb + 1) * Wb * 256
    S.need(C * Hb * Wb * 4 + S.GIB)
    with S.Meter(f"warp-planes[{name}]") as meter:
        feats, H, xs, ys, img = warp_setup(V, C, Hf, Wf, Hb, Wb, 81)
        out = nat.warp_fuse(feats, H, xs, ys, img, "mean")
        assert out.shape == (1, C, Hb, Wb) and S.all_finite(out)
        plane = Hb * Wb * 4
        rows = {0, Hb - 1} | {(lim % plane) // (Wb * 4) for lim in S.LIMITS if lim < C * plane}
        nz = 0
        for r0, r1 in S.merge(rows, Hb):
            ref = warp_band_ref(oracle, feats, H, xs, ys, img, "mean", r0, r1)
            assert same_bits(out[0, :, r0:r1].cpu(), ref), (r0, r1)
            nz += int((ref != 0).sum())
        meter.note(f"{nz} nonzero reference values on the bands")
        assert nz > 0
        del feats, out


# name, Hf, Wf, sH, sW: a view with rows 2^27 elements apart, and a column-major one with pixels 2^26 apart
WARP_STRIDE = [
    ("row-stride-under", 16, 28, (1 << 27) - 4, 64, "dma"),
    ("row-stride-at", 16, 28, 1 << 27, 64, "ck"),
    ("pixel-stride-under", 16, 32, 64, (1 << 26) - 4, "dma"),
    ("pixel-stride-at", 16, 32, 64, 1 << 26, "ck"),
]


def warp_stride_rule(Hf, Wf, sH, sW):
    """dma_ok: Hf sH < 2^31 and Wf sW < 2^31 (32-bit element offsets inside a map)."""
    return Hf * sH < 1 << 31 and Wf * sW < 1 << 31


@pytest.mark.parametrize("case", WARP_STRIDE, ids=[c[0] for c in WARP_STRIDE])
def test_warp_map_stride_rules(case, oracle):
    """The two stride clauses of dma_ok on a strided feature view (8 GiB of NaN around 16 x 28 live pixels), one
    stride step (4 elements: strides are multiples of 4) inside and at the limit; bit-identical to the oracle."""
    name, Hf, Wf, sH, sW, side = case
    assert warp_stride_rule(Hf, Wf, sH, sW) == (side == "dma")
    if side == "dma":
        assert not warp_stride_rule(Hf, Wf, sH + 4, sW) or not warp_stride_rule(Hf, Wf, sH, sW + 4)
    else:
        assert warp_stride_rule(Hf, Wf, sH - 4, sW) or warp_stride_rule(Hf, Wf, sH, sW - 4)
    Hb, Wb, C = 60, 180, 64
    S.need(((Hf - 1) * sH + (Wf - 1) * sW) * 4 + S.GIB)
    with S.Meter(f"warp-stride[{name}]") as meter:
        feats, H, xs, ys, img = warp_setup(1, C, Hf, Wf, Hb, Wb, 85, strides=(sH, sW))
        out = nat.warp_fuse(feats, H, xs, ys, img, "sum")
        assert S.all_finite(out)
        ref = warp_band_ref(oracle, feats, H, xs, ys, img, "sum", 0, Hb)
        nz = int((ref != 0).sum())
        meter.note(f"{nz} nonzero reference values")
        assert nz > 0 and same_bits(out[0].cpu(), ref)
        del feats, out


def warp_raw(entry, feats, H, xs, ys, img, mode, out, rpr=None):
    """The C entry itself (the Python wrappers answer BEV_ERR_ARGS with another route)."""
    B, V, C, Hf, Wf = feats.shape
    Hb, Wb = ys.numel(), xs.numel()
    sx, sy = nat._scales(Hf, Wf, img)
    s = feats.stride()
    nws = nat.lib().bev_ipm_warp_fuse_workspace_bytes(B, V, Hb, Wb)
    ws = torch.empty(max(nws, 8), device=DEV, dtype=torch.uint8)
    args = [nat._ptr(feats), s[1], s[2], s[3], s[4], nat._ptr(H), nat._ptr(xs), nat._ptr(ys), B, V, C, Hf, Wf, sx, sy,
            Hb, Wb, nat.FUSE_MODES[mode]]
    if rpr is not None:
        args.append(rpr)
    rc = getattr(nat.lib(), entry)(*args, nat._ptr(out), nat._ptr(ws), nws, 0, nat._stream(feats))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("Hb", [4095, 4096], ids=["under-2gib", "at-2gib"])
def test_warp_channels_last_frame_rule(Hb, oracle):
    """Channels-last output: a frame Hb Wb C 4 below 2 GiB runs (bit-identical to the oracle on bands), at 2 GiB the
    entry returns BEV_ERR_ARGS and leaves the output's NaN fill untouched."""
    V, C, Hf, Wf, Wb = 2, 64, 16, 28, 2048
    runs = Hb * Wb * C * 4 < 1 << 31
    assert runs == (Hb == 4095) and (Hb - 1) * Wb * C * 4 < 1 << 31 <= (Hb + 1) * Wb * C * 4
    S.need(Hb * Wb * C * 4 + S.GIB)
    with S.Meter(f"warp-nhwc[{Hb}]"):
        feats, H, xs, ys, img = warp_setup(V, C, Hf, Wf, Hb, Wb, 82)
        store = S.filled((1, Hb, Wb, C))
        rc = warp_raw("bev_ipm_warp_fuse_nhwc_f32", feats, H, xs, ys, img, "max", store)
        if not runs:
            assert rc == nat.BEV_ERR_ARGS and S.all_nan(store)
            return
        assert rc == 0 and S.all_finite(store)
        for r0, r1 in S.merge({0, Hb // 2, Hb - 1}, Hb):
            ref = warp_band_ref(oracle, feats, H, xs, ys, img, "max", r0, r1)
            assert same_bits(store[0, r0:r1].permute(2, 0, 1).cpu(), ref), (r0, r1)
        del feats, store


@pytest.mark.parametrize("Hb", [4095, 4096], ids=["under-2gib", "past-2gib"])
def test_warp_chunked_output_rule(Hb, oracle):
    """Rank-chunk-major output [ceil(Hb / rpr)][B][C][rpr][Wb]: the whole output (padding rows included) below 2 GiB
    runs, else BEV_ERR_ARGS with the fill untouched.  rpr = 45 divides 4095: one BEV row more adds a chunk."""
    V, C, Hf, Wf, Wb, rpr = 2, 64, 16, 28, 2048, 45
    nck = -(-Hb // rpr)
    runs = nck * rpr * 1 * C * Wb * 4 < 1 << 31
    assert runs == (Hb == 4095) and 4095 % rpr == 0
    S.need(nck * rpr * C * Wb * 4 + S.GIB)
    with S.Meter(f"warp-chunked[{Hb}]"):
        feats, H, xs, ys, img = warp_setup(V, C, Hf, Wf, Hb, Wb, 83)
        out = S.filled((nck, 1, C, rpr, Wb))
        rc = warp_raw("bev_ipm_warp_fuse_chunked_f32", feats, H, xs, ys, img, "sum", out, rpr)
        if not runs:
            assert rc == nat.BEV_ERR_ARGS and S.all_nan(out)
            return
        assert rc == 0 and S.all_finite(out)
        for ck in (0, nck // 2, nck - 1):  # whole chunks: the first, a middle one, the last
            ref = warp_band_ref(oracle, feats, H, xs, ys, img, "sum", ck * rpr, (ck + 1) * rpr)
            assert same_bits(out[ck, 0].cpu(), ref), ck
        del feats, out


@pytest.mark.parametrize("Hf", [2047, 2048], ids=["under-2^22", "at-2^22"])
def test_warp_feature_map_size_rule(Hf, oracle):
    """Hf Wf >= 2^22 (the footprint index's fast division) is BEV_ERR_ARGS; one feature row less runs.  The 2 GiB of
    features stay on the device: the reference gathers the four taps of every cell (the oracle's taps, which need no
    features) and blends them in float64 -- a bilinear sample and a sum over two views, so 2^-21 sum |w f|."""
    V, C, Wf, Hb, Wb = 2, 64, 2048, 24, 40
    runs = Hf * Wf < 1 << 22
    assert runs == (Hf == 2047) and (Hf - 1) * Wf < 1 << 22 <= (Hf + 1) * Wf
    S.need(V * Hf * Wf * C * 4 + S.GIB)
    with S.Meter(f"warp-feature-size[{Hf}]"):
        feats, H, xs, ys, img = warp_setup(V, C, Hf, Wf, Hb, Wb, 84)
        out = S.filled((1, C, Hb, Wb))
        nws = nat.lib().bev_ipm_warp_fuse_workspace_bytes(1, V, Hb, Wb)
        ws = torch.empty(max(nws, 8), device=DEV, dtype=torch.uint8)
        sx, sy = nat._scales(Hf, Wf, img)
        s = feats.stride()
        rc = nat.lib().bev_ipm_warp_fuse_ws_f32(nat._ptr(feats), s[1], s[2], s[3], s[4], nat._ptr(H), nat._ptr(xs),
                                                nat._ptr(ys), 1, V, C, Hf, Wf, sx, sy, Hb, Wb, nat.FUSE_MODES["sum"],
                                                nat._ptr(out), nat._ptr(ws), nws, nat._stream(feats))
        torch.cuda.synchronize()
        if not runs:
            assert rc == nat.BEV_ERR_ARGS and S.all_nan(out)
            return
        assert rc == 0 and S.all_finite(out)
        x0y0, wts, valid = oracle.taps(H.cpu().numpy(), xs.cpu().numpy(), ys.cpu().numpy(), Hf, Wf, img)
        ref = torch.zeros(Hb, Wb, C, dtype=torch.float64)
        mag = torch.zeros(Hb, Wb, C, dtype=torch.float64)
        fl = feats[0].permute(0, 2, 3, 1)  # [V, Hf, Wf, C] as stored
        for v in range(V):
            x0 = torch.from_numpy(x0y0[v, ..., 0].astype("int64"))
            y0 = torch.from_numpy(x0y0[v, ..., 1].astype("int64"))
            vb = torch.from_numpy(valid[v].astype("int64"))  # bit q: tap q lies inside the map
            for q, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
                yy, xx = y0 + dy, x0 + dx
                inside = ((vb >> q) & 1).bool()
                assert bool(((yy >= 0) & (yy < Hf) & (xx >= 0) & (xx < Wf))[inside].all())
                tap = fl[v, yy.clamp(0, Hf - 1).to(DEV), xx.clamp(0, Wf - 1).to(DEV)].cpu().double()
                w = torch.from_numpy(wts[v, ..., q]).double() * inside
                ref += w[..., None] * tap
                mag += (w[..., None] * tap).abs()
        err = (out[0].permute(1, 2, 0).cpu().double() - ref).abs()
        assert bool((mag > 0).any()) and bool((err <= 2.0 ** -21 * mag).all()), float(err.max())
        del feats, out


# ---------------------------------------------------------------------------
# streaming passes past 2^31 elements: no size rule, int64 indices throughout
# ---------------------------------------------------------------------------
SH, SW, SC = 4099, 8191, 64  # one image of 4099 x 8191 pixels x 64 channels
SM = SH * SW                 # 33,574,909 rows = 2^25 + 20,477; M C = 2^31 + a ragged tail of 1,310,528 elements
ROWS = 1 << 20               # rows per pass of the float64 reductions on the device
EPS, MOM = 1e-5, 0.1


def test_streaming_shape():
    assert SM > 1 << 25 and SM % 256 != 0 and SM * SC > 1 << 31 and SM * SC * 4 > 1 << 33


def chan_sums64(M, fn):
    """sum over all rows of fn(m0, m1) -> [rows, C] float64 on the device, accumulated in chunks."""
    acc = None
    for m0 in range(0, M, ROWS):
        s = fn(m0, min(M, m0 + ROWS)).sum(0)
        acc = s if acc is None else acc + s
    return acc


def chan_stats64(z2d):
    M = z2d.shape[0]
    mean = chan_sums64(M, lambda a, b: z2d[a:b].double()) / M
    var = chan_sums64(M, lambda a, b: (z2d[a:b].double() - mean) ** 2) / M
    return mean, var


def stream_bands(M, C=SC):
    return S.row_bands(M, [(C, 4), (C, 2)])


def rel_ok(what, got, ref, bar, meter):
    err = ((got.double() - ref).abs() / ref.abs().clamp_min(1e-300)).max().item()
    meter.note(f"{what} max rel err {err:.2e} (bar {bar:.0e})")
    assert bool(((got.double() - ref).abs() <= bar * ref.abs()).all()), (what, err)


def test_bn_train_forward_statistics():
    """batchnorm_train_fwd over M C = 2^31 + tail against float64 statistics accumulated on the device; the bars of
    tests/test_grad_value_domain_gpu.py (A1): mean, rstd 1e-6, scale 2e-6, shift 2^-22 (|mean scale| + |beta|),
    running statistics 1e-5."""
    S.need(SM * SC * 4 + 4 * S.GIB)
    with S.Meter("bn-train-fwd") as meter:
        g = S.gen(31)
        z = S.guarded((1, SH, SW, SC), g, scale=1.5, shift=2.0)
        gamma = torch.rand(SC, generator=g, device=DEV) + 0.5
        beta = torch.randn(SC, generator=g, device=DEV)
        rm, rv = torch.zeros(SC, device=DEV), torch.ones(SC, device=DEV)
        mean, rstd, scale, shift = nat.batchnorm_train_fwd(z, gamma, beta, rm, rv, EPS, MOM)
        mu, var = chan_stats64(z.view(SM, SC))
        r64 = (var + EPS).rsqrt()
        s64 = gamma.double() * r64
        rel_ok("mean", mean, mu, 1e-6, meter)
        rel_ok("rstd", rstd, r64, 1e-6, meter)
        rel_ok("scale", scale, s64, 2e-6, meter)
        h64 = beta.double() - mu * s64
        assert bool(((shift.double() - h64).abs() <= 2.0 ** -22 * ((mu * s64).abs() + beta.double().abs())).all())
        rel_ok("running_mean", rm, MOM * mu, 1e-5, meter)
        rel_ok("running_var", rv, (1 - MOM) + MOM * var * SM / (SM - 1), 1e-5, meter)
        del z


# C = 64 takes the row-block kernels (256 % (C / 4) == 0: k_bn_apply_q, k_bn_bwd_apply_q); C = 96 the flat grid-stride
# kernels with the 32-bit quad index (k_bn_apply<uint32_t, ..>, k_bn_bwd_apply<uint32_t, ..>), past 2^31 elements too
FLAT = (4099, 5461, 96)  # 22,384,639 rows x 96 channels = 2^31 + 1,441,696 elements
BN_APPLY = ["f32", "f32-res-relu", "f16-relu", "mask-res", "flat-f32-res-relu", "flat-f16-relu"]


def bn_shape(flat):
    H, W, C = FLAT if flat else (SH, SW, SC)
    assert H * W * C > 1 << 31 and (256 % (C // 4) != 0) == flat
    return (1, H, W, C), H * W, C


@pytest.mark.parametrize("form", BN_APPLY)
def test_bn_apply(form):
    """batchnorm_apply (fp32 out, with and without residual), batchnorm_apply_half, batchnorm_apply_mask on bands: per
    element 2^-22 (|z scale| + |shift| + |res|) + 1e-5 |ref| (A1's bar), plus half an fp16 ulp for the fp16 store."""
    with_res = "res" in form
    shp, M_, C_ = bn_shape(form.startswith("flat"))
    form = form.replace("flat-", "")
    S.need(M_ * C_ * 4 * (3 if with_res else 2) + 2 * S.GIB)
    with S.Meter(f"bn-apply[{'flat-' if C_ == 96 else ''}{form}]") as meter:
        g = S.gen(32)
        z = S.guarded(shp, g)
        res = S.guarded(shp, g) if with_res else None
        scale = torch.rand(C_, generator=g, device=DEV) + 0.5
        shift = torch.randn(C_, generator=g, device=DEV)
        mask = None
        if form == "f32":
            y, act = nat.batchnorm_apply(z, scale, shift, None, 0), 0
        elif form == "f32-res-relu":
            y, act = nat.batchnorm_apply(z, scale, shift, res, 1), 1
        elif form == "f16-relu":
            y, act = nat.batchnorm_apply_half(z, scale, shift, act=1), 1
        else:
            (y, mask), act = nat.batchnorm_apply_mask(z, scale, shift, res), 1
        assert S.all_finite(y)
        z2, y2 = z.view(M_, C_), y.view(M_, C_)
        s64, h64 = scale.cpu().double(), shift.cpu().double()
        worst = 0.0
        for m0, m1 in stream_bands(M_, C_):
            zs = z2[m0:m1].cpu().double() * s64
            r = res.view(M_, C_)[m0:m1].cpu().double() if with_res else torch.zeros_like(zs)
            u = zs + h64 + r
            ref = u.clamp_min(0) if act else u
            bound = 2.0 ** -22 * (zs.abs() + h64.abs() + r.abs()) + 1e-5 * ref.abs()
            if y.dtype == torch.float16:
                bound = bound + 2.0 ** -11 * ref.abs() + 2.0 ** -25
            got = y2[m0:m1].cpu()
            err = (got.double() - ref).abs()
            assert bool((err <= bound).all()), (m0, float((err - bound).max()))
            worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
            if mask is not None:  # bit u of byte k: y[4 k + u] > 0
                mb = mask[m0 * C_ // 4:m1 * C_ // 4].cpu().int()
                bits = ((mb[:, None] >> torch.arange(4)) & 1).bool().reshape(m1 - m0, C_)
                assert torch.equal(bits, got > 0)
        meter.note(f"max err / bound {worst:.3f}")
        del z, res, y, mask


@pytest.mark.parametrize("flat", [False, True], ids=["rows-c64", "flat-c96"])
def test_bn_bwd_half_relu_from_z(flat):
    """batchnorm_bwd_half (fp16 dz: the case fits the cap), ACT_RELU_FROM_Z, from the test's own fp32 statistics
    against the closed formula in float64: dgamma, dbeta and the batch means over all of M accumulated on the device,
    dz on bands.  A1's bars: dz, dgamma 1e-4 of the channel's max |ref|, dbeta 1e-5; dz is stored in fp16, half an
    fp16 ulp more.  The ReLU decision is the forward's: fp32 z scale + shift > 0, two roundings, evaluated in fp32."""
    shp, M_, C_ = bn_shape(flat)
    S.need(M_ * C_ * 10 + 5 * S.GIB)
    with S.Meter(f"bn-bwd-half[{'flat-c96' if flat else 'rows-c64'}]") as meter:
        g = S.gen(33)
        z = S.guarded(shp, g, scale=1.5, shift=0.25)
        dy = S.guarded(shp, g, shift=0.5)
        gamma = torch.rand(C_, generator=g, device=DEV) + 0.5
        beta = torch.randn(C_, generator=g, device=DEV) * 0.5
        z2, dy2 = z.view(M_, C_), dy.view(M_, C_)
        mu, var = chan_stats64(z2)
        mean32, rstd32 = mu.float(), (var + EPS).rsqrt().float()
        scale32 = (gamma.double() * rstd32.double()).float()
        shift32 = (beta.double() - mean32.double() * scale32.double()).float()
        dz, dres, dg, db = nat.batchnorm_bwd_half(dy, None, z, mean32, rstd32, gamma, False, nat.ACT_RELU_FROM_Z,
                                                  scale32, shift32)
        assert dres is None and dz.dtype == torch.float16 and S.all_finite(dz)
        m64, r64 = mean32.double(), rstd32.double()

        def grads(a, b, dev_):
            zz, dd = z2[a:b].to(dev_), dy2[a:b].to(dev_)
            open_ = (zz * scale32.to(dev_) + shift32.to(dev_)) > 0
            gg = torch.where(open_, dd.double(), torch.zeros((), dtype=torch.float64, device=dev_))
            return gg, (zz.double() - m64.to(dev_)) * r64.to(dev_)

        sg = chan_sums64(M_, lambda a, b: grads(a, b, DEV)[0])
        sgx = chan_sums64(M_, lambda a, b: torch.mul(*grads(a, b, DEV)))
        rel_ok("dbeta", db, sg, 1e-5, meter)
        rel_ok("dgamma", dg, sgx, 1e-4, meter)
        k1, k2, gr = (sg / M_).cpu(), (sgx / M_).cpu(), (gamma.double() * r64).cpu()
        err, scl, refs = torch.zeros(C_, dtype=torch.float64), torch.zeros(C_, dtype=torch.float64), []
        dz2 = dz.view(M_, C_)
        for m0, m1 in stream_bands(M_, C_):
            gg, xh = grads(m0, m1, "cpu")
            ref = gr * (gg - k1 - xh * k2)
            e = (dz2[m0:m1].cpu().double() - ref).abs() - 2.0 ** -11 * ref.abs()
            err, scl = torch.maximum(err, e.amax(0)), torch.maximum(scl, ref.abs().amax(0))
        meter.note(f"dz worst err / max|ref| {(err / scl).max().item():.2e} (bar 1e-4)")
        assert bool((err <= 1e-4 * scl).all()), (err / scl).max().item()
        del z, dy, dz


def test_relu_bwd_whole_tensor():
    """k_relu_bwd: a select, so every element of the 2^31 + tail is compared on the device, chunk by chunk."""
    n = SM * SC
    S.need(3 * n * 4 + 2 * S.GIB)
    with S.Meter("relu-bwd"):
        g = S.gen(34)
        dy, y = S.guarded((SM, SC), g), S.guarded((SM, SC), g)
        dz = nat.relu_bwd(dy, y)
        a, b, c = dy.view(-1), y.view(-1), dz.view(-1)
        for i in range(0, n, S.CHUNK):
            ref = torch.where(b[i:i + S.CHUNK] > 0, a[i:i + S.CHUNK], torch.zeros((), device=DEV))
            assert torch.equal(c[i:i + S.CHUNK], ref), i
        del dy, y, dz


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_dilate_large_output(dtype):
    """k_dilate: the zero-inserted map [1, 4099, 8191, 64] past 2^31 elements, exact on bands of output rows."""
    s, top, left = 2, 1, 1
    Ho, Wo = 2049, 4095
    assert top + s * (Ho - 1) < SH and left + s * (Wo - 1) < SW
    es = 4 if dtype == torch.float32 else 2
    S.need(SM * SC * es + Ho * Wo * SC * es + S.GIB)
    with S.Meter(f"dilate[{'f32' if es == 4 else 'f16'}]"):
        dz = S.guarded((1, Ho, Wo, SC), S.gen(35), dtype=dtype)
        fn = nat.dilate_nhwc if es == 4 else nat.dilate_nhwc_any
        out = fn(dz, s, top, left, SH, SW)
        assert out.dtype == dtype and S.all_finite(out)
        rows = {0, SH - 1} | set(S.crossing_rows(SW * SC, es, SH))
        for r0, r1 in S.merge(rows, SH):
            ref = torch.zeros(r1 - r0, SW, SC, dtype=dtype)
            for r in range(r0, r1):
                yy = r - top
                if yy >= 0 and yy % s == 0 and yy // s < Ho:
                    ref[r - r0, left:left + s * Wo:s] = dz[0, yy // s].cpu()
            assert torch.equal(out[0, r0:r1].cpu(), ref), (r0, r1)
        # nothing but the placed values: the sums of |.| agree (float64 on the device, in chunks)
        tot = sum(float(out.view(-1)[i:i + S.CHUNK].abs().sum(dtype=torch.float64)) for i in range(0, SM * SC, S.CHUNK))
        src = float(dz.abs().sum(dtype=torch.float64))
        assert abs(tot - src) <= 1e-9 * src
        del dz, out


def test_place_strided_large_output():
    """k_place_strided with a residual: out [1, 4099, 8191, 64] = residual + y at (2 oy, 2 ox); one fp32 addition, so
    2^-24 |ref| against float64 on bands."""
    s, Ho, Wo = 2, 2050, 4096
    assert s * (Ho - 1) < SH and s * (Wo - 1) < SW
    S.need(2 * SM * SC * 4 + Ho * Wo * SC * 4 + S.GIB)
    with S.Meter("place-strided"):
        g = S.gen(36)
        y = S.guarded((1, Ho, Wo, SC), g)
        res = S.guarded((1, SH, SW, SC), g)
        out = nat.place_strided(y, s, SH, SW, res)
        assert S.all_finite(out)
        rows = {0, SH - 1} | set(S.crossing_rows(SW * SC, 4, SH))
        for r0, r1 in S.merge(rows, SH):
            ref = res[0, r0:r1].cpu().double()
            for r in range(r0, r1):
                if r % s == 0 and r // s < Ho:
                    ref[r - r0, 0:s * Wo:s] += y[0, r // s].cpu().double()
            err = (out[0, r0:r1].cpu().double() - ref).abs()
            assert bool((err <= 2.0 ** -24 * ref.abs()).all()), (r0, float(err.max()))
        del y, res, out


def test_colsum_all_rows():
    """k_colsum_v4 over 2^25 + 20,477 rows against float64 on the device: 1e-5 sum |x| per column
    (tests/test_grad_value_domain_gpu.py A4)."""
    S.need(SM * SC * 4 + 3 * S.GIB)
    with S.Meter("colsum") as meter:
        dz = S.guarded((SM, SC), S.gen(37), shift=0.25)
        db = nat.colsum(dz)
        ref = chan_sums64(SM, lambda a, b: dz[a:b].double())
        mag = chan_sums64(SM, lambda a, b: dz[a:b].double().abs())
        err = (db.double() - ref).abs()
        meter.note(f"max err / sum|x| {(err / mag).max().item():.2e} (bar 1e-5)")
        assert bool((err <= 1e-5 * mag).all())
        del dz


def test_maxpool_forward_and_backward():
    """maxpool_fwd_arg_nhwc (3x3 / 2 / 1) over an input past 2^31 elements and maxpool_bwd_arg_nhwc into a gradient of
    that size, against torch's float64 max_pool2d and its autograd on bands with their window halo."""
    k, s, p = 3, 2, 1
    Ho, Wo = S.out_hw(SH, SW, k, s, p, 1)
    S.need(2 * SM * SC * 4 + 2 * Ho * Wo * SC * 4 + Ho * Wo * SC + S.GIB)
    with S.Meter("maxpool"):
        g = S.gen(38)
        x = S.guarded((1, SH, SW, SC), g, guard_pixels=2 * SW + 2)
        y, arg = nat.maxpool_fwd_arg_nhwc(x, k, s, p)
        dy = S.guarded((1, Ho, Wo, SC), g)
        dx = nat.maxpool_bwd_arg_nhwc(arg, dy, SH, SW, k, s, p)
        assert S.all_finite(y) and S.all_finite(dx)
        rows = {0, SH - 1} | set(S.crossing_rows(SW * SC, 4, SH))
        ninf = float("-inf")
        for i0, i1 in S.merge(rows, SH):
            o0, o1 = max(0, i0 // 2), min(Ho - 1, i1 // 2)  # the windows that hold input rows [i0, i1)
            a, b = max(0, 2 * o0 - 1), min(SH, 2 * o1 + 2)
            xb = x[0, a:b].cpu().double().permute(2, 0, 1)[None].requires_grad_(True)
            xp = F.pad(xb, (0, 0, a - (2 * o0 - 1), (2 * o1 + 2) - b), value=ninf)
            yb = F.max_pool2d(xp, k, s, padding=(0, p))
            assert yb.shape[2] == o1 + 1 - o0
            assert torch.equal(y[0, o0:o1 + 1].cpu().double(), yb[0].permute(1, 2, 0).detach())
            d = dy[0, o0:o1 + 1].cpu().double().permute(2, 0, 1)[None]
            yb.backward(d, retain_graph=True)
            ref = xb.grad[0].permute(1, 2, 0)[i0 - a:i1 - a].clone()
            xb.grad = None
            yb.backward(d.abs())
            mag = xb.grad[0].permute(1, 2, 0)[i0 - a:i1 - a]
            err = (dx[0, i0:i1].cpu().double() - ref).abs()
            assert bool((err <= 2.0 ** -22 * mag).all()), (i0, float(err.max()))  # up to four fp32 additions
        del x, y, arg, dy, dx


FM = 3 * (1 << 28) + 4099  # elements per view: with V = 3 the views' element offsets cross 2^31 (2^32, 2^33 bytes)


@pytest.mark.parametrize("mode", ["sum", "mean", "max"])
def test_view_fuse_whole_tensor(mode):
    """bev_view_fuse_f32 over [1, 3, M], 3 M past 2^31 elements: every output against float64 on the device.  sum /
    mean: three fp32 roundings (two additions, the division), each half an ulp of at most sum |x|; max: exact."""
    V = 3
    assert V * FM > 1 << 31 and V * FM * 4 > 1 << 33
    S.need((V + 1) * FM * 4 + 4 * S.GIB)
    with S.Meter(f"view-fuse[{mode}]"):
        x = S.guarded((1, V, FM), S.gen(39), guard_elems=1 << 16)
        out = nat.view_fuse(x, mode)
        assert out.shape == (1, FM)
        step = 1 << 26
        for i in range(0, FM, step):
            xs = x[0, :, i:i + step].double()
            got = out[0, i:i + step].double()
            if mode == "max":
                assert torch.equal(got, xs.amax(0)), i
            else:
                ref = xs.sum(0) / (V if mode == "mean" else 1)
                assert bool(((got - ref).abs() <= 3 * 2.0 ** -24 * xs.abs().sum(0)).all()), i
        del x, out


def test_view_max_bwd_whole_tensor():
    """bev_view_max_bwd_f32 over [1, 3, M]: the gradient goes to the first maximal view, every other view gets 0 --
    every element compared on the device."""
    V = 3
    S.need((2 * V + 1) * FM * 4 + 3 * S.GIB)
    with S.Meter("view-max-bwd"):
        g = S.gen(40)
        x = S.guarded((1, V, FM), g, guard_elems=1 << 16)
        gout = S.guarded((1, FM), g, guard_elems=1 << 16)
        gx = nat.view_max_bwd(x, gout)
        step = 1 << 26
        for i in range(0, FM, step):
            xs = x[0, :, i:i + step]
            best, arg = xs[0], torch.zeros(xs.shape[1], dtype=torch.int64, device=DEV)
            for v in range(1, V):
                up = xs[v] > best
                best, arg = torch.where(up, xs[v], best), torch.where(up, v, arg)
            for v in range(V):
                ref = torch.where(arg == v, gout[0, i:i + step], torch.zeros((), device=DEV))
                assert torch.equal(gx[0, v, i:i + step], ref), (v, i)
        del x, gout, gx


def test_channel_affine_past_2_31_elements():
    """bev_channel_affine_f32 on [2, 4099, 4096, 64] (2^31 + 2^19 elements; the 32-bit quad index form): 2^-23 (|x a|
    + |b|) on bands.  Its own rule, total quads < 2^32 - 65536 * 256, needs a 64 GiB operand: untested."""
    N, H, W = 2, 4099, 4096
    M = N * H * W
    assert M * SC > 1 << 31 and M * SC // 4 < (1 << 32) - 65536 * 256
    S.need(2 * M * SC * 4 + S.GIB)
    with S.Meter("channel-affine"):
        g = S.gen(41)
        x = S.guarded((N, H, W, SC), g)
        a = torch.randn(N, SC, generator=g, device=DEV)
        b = torch.randn(N, SC, generator=g, device=DEV)
        y = nat.channel_affine(x, a, b)
        assert S.all_finite(y)
        x2, y2 = x.view(M, SC), y.view(M, SC)
        marks = stream_bands(M) + [(H * W - 256, H * W + 256)]  # and the boundary between the two images
        for m0, m1 in marks:
            n = torch.arange(m0, m1) // (H * W)
            xa = x2[m0:m1].cpu().double() * a.cpu().double()[n]
            bb = b.cpu().double()[n]
            err = (y2[m0:m1].cpu().double() - (xa + bb)).abs()
            assert bool((err <= 2.0 ** -23 * (xa.abs() + bb.abs())).all()), (m0, float(err.max()))
        del x, y


# ---------------------------------------------------------------------------
# which form ran
# ---------------------------------------------------------------------------
TRACE_SCRIPT = """
import sys
sys.path.insert(0, {pkg!r})
sys.path.insert(0, {tests!r})
import torch
import bev_native as nat
dev = "cuda:0"


def z(*shape, dtype=torch.float32):
    return torch.zeros(*shape, device=dev, dtype=dtype)


def done(y):  # the operands are zeros: only the launch matters here
    torch.cuda.synchronize()


# every pair: the below-cap shape, then the above-cap shape of the same case
for N, H, W, Ci, Co, K, s, p, d in {x6!r}:
    done(nat.conv2d_nhwc_x6(z(N, H, W, Ci), nat.pack_conv_weight_x6(torch.ones(Co, Ci, K, K, device=dev)), None, Co,
                            K, K, s, p, d, 0))
for Co, split in ((64, False), (128, False), (64, True)):
    for N, H, W, Ci in {pw!r}:
        done(nat.conv2d_nhwc_x6(z(N, H, W, Ci), nat.pack_conv_weight_x6(torch.ones(Co, Ci, 1, 1, device=dev)), None, Co,
                                1, 1, 1, 0, 1, 0, split_out=split))
for W2 in {dual!r}:
    done(nat.conv2d_dual_nhwc(z(1, 2048, 4096, 16), z(1, 4096, W2, 16), 2,
                              nat.pack_conv_weight_x6(torch.ones(64, 32, 1, 1, device=dev)), None, 64, relu=True))
for K, out in ((1, "f32"), (3, "f32"), (1, "f16"), (1, "stats")):
    for N, H, W, Ci in {h16!r}:
        x = z(N, H, W, Ci, dtype=torch.float16)
        ph = nat.pack_conv_weight_h16(torch.ones(8, Ci, K, K, device=dev))
        if out == "f16":
            done(nat.conv2d_h16_half(x, ph, z(8), 8, K, K, 1, K // 2))
        else:
            y = nat.conv2d_h16_any(x, ph, 8, K, K, 1, K // 2, stats=out == "stats")
            done(y[0] if out == "stats" else y)
        del x
import test_size_rules_gpu as T
for C, Hb in ((64, 4095), (64, 4096)):
    feats, H, xs, ys, img = T.warp_setup(2, C, 16, 28, Hb, 4096, 81)
    nat.warp_fuse(feats, H, xs, ys, img, "mean")
    torch.cuda.synchronize()
for _, Hf, Wf, sH, sW, _ in T.WARP_STRIDE:
    feats, H, xs, ys, img = T.warp_setup(1, 64, Hf, Wf, 60, 180, 85, strides=(sH, sW))
    nat.warp_fuse(feats, H, xs, ys, img, "sum")
    torch.cuda.synchronize()
    del feats
"""

# (N, H, W, Ci) below and above conv_x6()'s cap for the 1x1 linear form: three images (span 2) / one image past it
PW_TRACE = [PW_GEOM, (1, 5793, 5793, 16)]
X6 = r"k_conv_x6<4, 1, 1, 2, false, {}>"
H16 = r"k_conv_h16b<true, 64, {}, false, false>"
# one pattern per traced case, in launch order; {} is BUFA / BUF: true below the cap, false above it
TRACE_EXPECT = [X6, X6, r"k_conv_x6b<4, 1, 1, 2, false, (\w+, )*{}>", X6,      # X6_CAP's three, five images
                X6, r"k_conv_x6<2, 2, 2, 2, false, {}>", X6,                            # 1x1: Co 64, 128, split output
                r"k_conv_x6<4, 1, 1, 2, true, {}>",                                     # dual
                H16, H16, r"k_conv_h16b<true, 64, {}, true, false>", H16]               # 1x1, 3x3, fp16 out, statistics
TRACE_WARP = 1 + len(WARP_STRIDE) // 2  # output planes, then the two stride clauses: k_warp_fuse_v2, k_warp_fuse each


def test_which_form_ran(tmp_path):
    """One below-cap and one above-cap call of every x6, h16 and warp dispatch case of this file in a child process
    under a kernel trace (the pattern of tests/test_mod_metrics_gpu.py, names through tools/kernel_coverage.py), in
    launch order: the BUFA / BUF = true instance below the cap and the false one above it; k_warp_fuse_v2 inside
    dma_ok and k_warp_fuse outside.  Without this a rule that always chose the pointer form would pass the rest."""
    import re
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import kernel_coverage as kc
    assert x6_lhs(*PW_TRACE[0], 1, 1, 0, 1) < X6_BUF_MAX <= x6_lhs(*PW_TRACE[1], 1, 1, 0, 1)
    five = [(5, 4096, 4095, 16, 16, 3, 2, 1, 1), (5, 4096, 4096, 16, 16, 3, 2, 1, 1)]
    assert [x6_side(g) for g in five] == ["buf", "ptr"]
    S.need(20 * S.GIB)
    prof = os.path.join(kc.ROCM, "bin", "rocprofv3")
    prof = prof if os.path.exists(prof) else shutil.which("rocprofv3")
    assert prof, "rocprofv3 not found"
    script = tmp_path / "forms.py"
    script.write_text(TRACE_SCRIPT.format(pkg=PKG, tests=os.path.join(REPO, "tests"), x6=[c[1] for c in X6_CAP] + five,
                                          pw=PW_TRACE, dual=[c[1] for c in DUAL], h16=[H16_UNDER, H16_AT]))
    run = subprocess.run([prof, "--kernel-trace", "--output-format", "csv", "-d", str(tmp_path / "kt"), "-o", "run",
                          "--", sys.executable, str(script)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    traces = glob.glob(str(tmp_path / "kt" / "**" / "*kernel_trace.csv"), recursive=True)
    assert traces, os.listdir(tmp_path / "kt")
    with open(traces[0], newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    raw = [r["Kernel_Name"].strip().strip("'\"") for r in rows]
    raw = [n[:-3] if n.endswith(".kd") else n for n in raw]
    mangled = sorted({n for n in raw if n.startswith("_Z")})
    dem = dict(zip(mangled, kc.demangle(mangled)))
    names = [kc.short(kc.normalize(dem.get(n, n))) for n in raw]
    convs = [n for n in names if n.startswith(("k_conv_x6<", "k_conv_x6b<", "k_conv_h16b<"))]
    want = [pat.replace("<", r"\<").format(flag) for pat in TRACE_EXPECT for flag in ("true", "false")]
    assert len(convs) == len(want), convs
    for got, pat in zip(convs, want):
        assert re.fullmatch(pat, got), (got, pat, convs)
    warps = [n.split("<")[0] for n in names if n.startswith(("k_warp_fuse_v2<", "k_warp_fuse<"))]
    assert warps == ["k_warp_fuse_v2", "k_warp_fuse"] * TRACE_WARP, warps
