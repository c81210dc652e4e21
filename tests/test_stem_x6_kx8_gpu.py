"""The split-arithmetic ResNet stem's in-kernel K order k' = (ky, ci, kx8) (csrc/bev_conv_x6.hip, k_stem_x6).

The kernel takes the generic split panel (k = (ky, kx, ci), 147 taps padded to 160) and permutes it, while copying
it into LDS, into 21 runs (ky, ci) of 8 slots -- slots 0..6 = kx, slot 7 padding -- plus a padded 22nd run; an A
fragment is then 8 contiguous bf16 of one patch row.  What can go wrong, and what these tests pin down:
  1. the permutation (a tap's weight meeting another tap's input)          -> one-hot weights, exact;
  2. tile edges (ragged rows / columns, the second M tile, Co < 64)         -> float64, the suite's x6 bars;
  3. the padding slots (slot 7 = input column 2 ox + 4, outside the 7x7 field; the 22nd run) leaking a NaN / Inf
     into an output whose receptive field does not hold it                -> exact non-finite sets;
  4. the fused max-pool form on the same main loop                          -> bit-identical to stem + max-pool.
The expectations of 1 and 3 are integer / indexing arithmetic on the CPU (checked there against float64
F.conv2d); only the kernel launches need the GPU.
"""
import itertools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _ref64(x, w, b, relu):
    y = F.conv2d(x.double(), w.double(), b.double(), stride=2, padding=3)
    return (torch.relu(y) if relu else y).permute(0, 2, 3, 1).contiguous()


# ----------------------------------------------------------------------------------------------------------------------
# 1. every tap lands where it should
# ----------------------------------------------------------------------------------------------------------------------
def onehot_weights(i):
    """[64, 3, 7, 7]: output channel co has weight 1.0 at tap co + 64 i (the OIHW-flattened (ci, ky, kx) index) and
    zero elsewhere; taps >= 147 do not exist (those channels stay all-zero)."""
    w = torch.zeros(64, 147)
    for co in range(64):
        if co + 64 * i < 147:
            w[co, co + 64 * i] = 1.0
    return w.reshape(64, 3, 7, 7)


def onehot_expect(x, i):
    """y[n, oy, ox, co] = x[n, ci, 2 oy + ky - 3, 2 ox + kx - 3] (0 outside the image) for tap co + 64 i = (ci, ky, kx),
    by indexing alone."""
    N, _, H, W = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = F.pad(x, (3, 3, 3, 3))
    y = torch.zeros(N, Ho, Wo, 64)
    for co in range(64):
        tap = co + 64 * i
        if tap < 147:
            ci, ky, kx = tap // 49, (tap // 7) % 7, tap % 7
            y[:, :, :, co] = xp[:, ci, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2]
    return y


@pytest.mark.parametrize("i", [0, 1, 2])
def test_stem_x6_one_hot_taps_exact(i):
    """With a weight of exactly 1.0 (h = 1, m = l = 0) the six products reduce to x_h + x_m + x_l = x, exactly: the
    output is the input value under that tap, bit for bit.  Three launches cover all 147 taps."""
    import bev_native as nat
    x = torch.randn(1, 3, 20, 24, generator=torch.Generator().manual_seed(700 + i))
    want = onehot_expect(x, i)
    got = nat.conv2d_stem_x6(x.to(DEV), nat.pack_conv_weight_x6(onehot_weights(i).to(DEV)),
                             torch.zeros(64, device=DEV), 64, False).cpu()
    assert got.shape == want.shape
    bad = (got.view(torch.int32) != want.view(torch.int32)).nonzero()
    assert bad.numel() == 0, (bad[:8].tolist(), int(bad.shape[0]))


# ----------------------------------------------------------------------------------------------------------------------
# 2. / 4. tile edges: Ho in {8, 9, 17} (one tile row, one row past it, three rows), Wo in {64, 65, 128, 129}
# ----------------------------------------------------------------------------------------------------------------------
EDGE_HW = [(16, 128), (18, 130), (15, 255), (33, 258)]


def _edge_case(H, W, Co):
    g = torch.Generator().manual_seed(9000 + H + W + Co)
    x = torch.randn(2, 3, H, W, generator=g)
    w = torch.randn(Co, 3, 7, 7, generator=g) / 147 ** 0.5
    b = torch.randn(Co, generator=g) * 0.1
    return x, w, b


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "norelu"])
@pytest.mark.parametrize("Co", [64, 40])
@pytest.mark.parametrize("H,W", EDGE_HW)
def test_stem_x6_tile_edges_vs_float64(H, W, Co, relu):
    """test_conv_x6_gpu.py's stem bars (max error <= 1e-5 max|ref| against float64; no worse than 4x the exact-f32
    stem + 1e-7 scale) at the tile edges."""
    import bev_native as nat
    x, w, b = _edge_case(H, W, Co)
    ref = _ref64(x, w, b, relu)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    y6 = nat.conv2d_stem_x6(xd, nat.pack_conv_weight_x6(wd), bd, Co, relu)
    yf = nat.conv2d_nhwc(xd, nat.pack_conv_weight(wd), bd, Co, 7, 7, 2, 3, relu, in_nchw=True)
    torch.cuda.synchronize()
    scale = ref.abs().max().item()
    e6, ef = (y6.cpu().double() - ref).abs().max().item(), (yf.cpu().double() - ref).abs().max().item()
    print(f"[stem kx8] {H}x{W} Co {Co} relu {relu}: x6 err {e6:.3e} f32 err {ef:.3e} scale {scale:.3e}")
    assert y6.shape == ref.shape and torch.isfinite(y6).all()
    assert e6 <= 1e-5 * scale, (e6, scale)
    assert e6 <= 4 * ef + 1e-7 * scale, (e6, ef)


@pytest.mark.parametrize("H,W", EDGE_HW)
def test_stem_pool_x6_tile_edges_bit_identical(H, W):
    """conv2d_stem_pool_x6 == maxpool_nhwc(conv2d_stem_x6(relu)) bit for bit: seams, corners and a ragged last tile on
    both axes."""
    import bev_native as nat
    x, w, b = _edge_case(H, W, 64)
    xd, bd = x.to(DEV), b.to(DEV)
    packed = nat.pack_conv_weight_x6(w.to(DEV))
    ref = nat.maxpool_nhwc(nat.conv2d_stem_x6(xd, packed, bd, 64, True), 3, 2, 1)
    got = nat.conv2d_stem_pool_x6(xd, packed, bd)
    torch.cuda.synchronize()
    assert got.shape == ref.shape
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), (got - ref).abs().max().item()


# ----------------------------------------------------------------------------------------------------------------------
# 3. slot 7 and the padded run do not leak
# ----------------------------------------------------------------------------------------------------------------------
PH, PW = 24, 140                                      # Ho x Wo = 12 x 70: two tile rows, two tile columns
POISON_X = [0, 1, 4, 5, 124, 125, 129, 130, 131, 139]  # even / odd slot-7 columns (x = 2 ox + 4) on both sides of
POISON_Y = [0, 12, 13, 23]                             # the 64-column tile boundary; first / last; the 8-row boundary


def field(y, x, H=PH, W=PW):
    """The outputs (oy0, oy1, ox0, ox1), inclusive, whose 7x7 / s2 / p3 window holds input pixel (y, x):
    2 o - 3 <= p <= 2 o + 3."""
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    lo = lambda p: max(0, -((3 - p) // 2))      # ceil((p - 3) / 2)
    hi = lambda p, n: min(n - 1, (p + 3) // 2)  # floor((p + 3) / 2)
    return lo(y), hi(y, Ho), lo(x), hi(x, Wo)


def overlap(a, b):
    return a[0] <= b[1] and b[0] <= a[1] and a[2] <= b[3] and b[2] <= a[3]


def pack_positions():
    """The 40 (y, x) positions packed greedily into image slots so that no two fields in one image share an output;
    two slots = one 2-image launch.  (x = 0, 1, 4, 5 share output columns and y = 12, 13 output rows: those eight
    positions need eight images, so a (value, channel) takes four launches, not one.)"""
    slots = []
    for pos in itertools.product(POISON_Y, POISON_X):
        for s in slots:
            if not any(overlap(field(*pos), field(*q)) for q in s):
                s.append(pos)
                break
        else:
            slots.append([pos])
    if len(slots) % 2:
        slots.append([])
    return [(slots[i], slots[i + 1]) for i in range(0, len(slots), 2)]


def field_mask(launch, H=PH, W=PW):
    """[2, Ho, Wo] bool: the union of the fields of a launch's positions, per image."""
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    m = torch.zeros(2, Ho, Wo, dtype=torch.bool)
    for n, slot in enumerate(launch):
        for pos in slot:
            oy0, oy1, ox0, ox1 = field(*pos)
            m[n, oy0:oy1 + 1, ox0:ox1 + 1] = True
    return m


_POISON_OPS = {}


def _poison_ops(Co):
    """Operands and the unpoisoned output, computed once per Co."""
    import bev_native as nat
    if Co not in _POISON_OPS:
        g = torch.Generator().manual_seed(7300 + Co)
        x = torch.randn(2, 3, PH, PW, generator=g)
        w = torch.randn(Co, 3, 7, 7, generator=g) / 147 ** 0.5
        b = torch.randn(Co, generator=g) * 0.1
        assert bool((w != 0).all()) and bool(torch.isfinite(x).all())
        p, bd = nat.pack_conv_weight_x6(w.to(DEV)), b.to(DEV)
        clean = nat.conv2d_stem_x6(x.to(DEV), p, bd, Co, False).cpu()
        assert bool(torch.isfinite(clean).all())
        _POISON_OPS[Co] = (x, p, bd, clean)
    return _POISON_OPS[Co]


@pytest.mark.parametrize("ci", [0, 1, 2])
@pytest.mark.parametrize("poison", ["nan", "inf"])
@pytest.mark.parametrize("Co", [64, 40])
def test_stem_x6_padding_slots_do_not_leak(Co, poison, ci):
    """One NaN / +Inf pixel per position: the non-finite outputs are exactly the (oy, ox) whose window holds it, in
    every channel < Co, and every other output equals the unpoisoned run bit for bit."""
    import bev_native as nat
    x, p, bd, clean = _poison_ops(Co)
    val = float("nan") if poison == "nan" else float("inf")
    launches = pack_positions()
    assert sorted(q for l in launches for s in l for q in s) == sorted(itertools.product(POISON_Y, POISON_X))
    for launch in launches:
        xp = x.clone()
        for n, slot in enumerate(launch):
            for a, b in itertools.combinations(slot, 2):
                assert not overlap(field(*a), field(*b)), (a, b)
            for (py, px) in slot:
                xp[n, ci, py, px] = val
        got = nat.conv2d_stem_x6(xp.to(DEV), p, bd, Co, False).cpu()
        want = field_mask(launch)[..., None].expand(-1, -1, -1, Co)
        nonfin = ~torch.isfinite(got)
        extra, missing = (nonfin & ~want).nonzero(), (want & ~nonfin).nonzero()
        assert extra.numel() == 0 and missing.numel() == 0, (launch, extra[:6].tolist(), missing[:6].tolist())
        same = got.view(torch.int32) == clean.view(torch.int32)
        assert bool((same | want).all()), (launch, (~(same | want)).nonzero()[:6].tolist())
