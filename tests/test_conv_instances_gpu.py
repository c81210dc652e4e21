"""One case per conv-kernel instantiation that shape-driven dispatch only reaches at workload size or through a
bev_tune knob (csrc/bev_conv.hip, bev_conv_x6.hip, bev_conv_h16.hip, k_stem3 of bev_effnet.hip): each case forces the
instance through the public wrappers and nat.tuned(...), and its id names it.  tools/kernel_coverage.py lists which
compiled kernels the suite launches (profiles/r11a_kernel_coverage_*.txt).

The reference is always torch.nn.functional.conv2d in float64 on the CPU over the operands as the kernel sees them
(fp32 values, or their fp16 roundings for the fp16 family; an operand affine / channel scale applied with the kernel's
fp32 roundings first), bias, residual and ReLU / SiLU in float64 -- never another kernel.  Bounds, all the project's:

 1. the family's float64 bar: split-bf16 and exact-f32 kernels max|err| <= 1e-5 max|ref| and finite
    (test_conv_x6_gpu.py); k_stem3 2e-6 max|ref| (test_effnet.py); fp16 kernels the per-element bounds derived in
    test_conv_h16_gpu.py (fp32 output: K 2^-24 (sum|x||w| + |b| + |r|) + 1e-6) and test_conv_h16_half_gpu.py (fp16
    output: 2^-11 |ref| + (K + 2) 2^-24 (sum|x||w| + |b| + |r|) + 2^-24), x 1.2 for SiLU.
 2. no less accurate than the pinned default: max / mean error <= 4 x the error of the family's default-dispatch
    instance on the same operands + 1e-7 / 1e-9 max|ref| (test_x6_conv_fp32_accuracy_vs_float64's criterion, which
    catches a lost low-order split plane).  For the split-bf16 family the pinned instance of that test, the exact-f32
    MFMA kernel on the same operands, is held to as well: a dual case whose default dispatch IS the forced instance
    (Ci % 32 != 0) would otherwise be compared with itself.
 3. torch.equal against the default instance where include/bev_mi355x.h promises the same bits: CONV_DMA,
    CONV_X6_KERNEL, CONV_X6_TILE, CONV_X6_NT, CONV_H16_KERNEL (convs), CONV_H16_BUF, STEM3_STAGE.
 4. CONV_XCD and CONV_NBUF: torch.equal too.  By reading k_conv / k_conv_dma: a.xcd only permutes which (m0, n0) tile
    a workgroup takes (bid -> (x < r ? x (q + 1) : r (q + 1) + (x - r) q) + bid / 8 is a bijection of [0, gridDim.x));
    NBUF only selects the LDS staging buffer a K step is written to and read from and adds a barrier.  Neither touches
    the order in which an accumulator receives its k (step by step, MFMA slot h of half `half`, p: k = 32 step + 16 h +
    8 half + p), so every output's sum is the same sequence of operations.

Shapes: M = 270 or 782 rows (three / seven 128-row tiles, five / thirteen 64-row ones, the last ragged, tiles that
straddle the two images), Co = 200 / 72 / 40 (ragged against 128- and 64-column tiles), >= 2 K steps of the instance's
depth, padded 3x3 taps, one stride-2 case per family, dual cases with stride2 = 2 and Ci != Ci2.  The CONV_XCD grids
(N = 2, 17 x 23, Co = 200: 14 / 28 / 26 / 52 workgroups) have more than 8 workgroups and no multiple of 8.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_CACHE = {}


def _cached(key, make):
    """Operands and float64 references are made once per shape and shared (never modified)."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _act64(z, act):
    if act == 1:
        return z.clamp_min(0)
    if act == 2:
        return z * torch.sigmoid(z)
    return z


def _errs(y, ref):
    e = (y.detach().cpu().double() - ref).abs()
    return e.max().item(), e.mean().item()


def _check12(tag, y, pinned, ref, bar=1e-5):
    """Bounds 1 and 2; `pinned`: dict name -> output of a pinned instance on the same operands."""
    scale = ref.abs().max().item()
    assert bool(torch.isfinite(y).all()), tag
    em, ea = _errs(y, ref)
    assert em <= bar * scale, (tag, em, scale)
    for name, y0 in pinned.items():
        dm, da = _errs(y0, ref)
        print(f"[instance] {tag}: max err {em:.3e} = {em / scale:.2e} max|ref|; vs {name}: "
              f"max {em / max(dm, 1e-300):.3f}x mean {ea / max(da, 1e-300):.3f}x")
        assert em <= 4 * dm + 1e-7 * scale, (tag, name, em, dm)
        assert ea <= 4 * da + 1e-9 * scale, (tag, name, ea, da)


def _rand(g, *shape):
    return torch.randn(*shape, generator=g)


# ======================================================================================================================
# exact-f32 MFMA convs (bev_conv.hip): k_conv<tile, LOADER, NBUF>, k_conv_dma<tile>
# ======================================================================================================================
CO = 200
F32_TILES = [("128x128", dict(CONV_TILE=1)), ("128x64-nbuf1", dict(CONV_TILE=2, CONV_NBUF=1)),
             ("128x64-nbuf2", dict(CONV_TILE=2, CONV_NBUF=2)), ("64x128-nbuf1", dict(CONV_TILE=3, CONV_NBUF=1)),
             ("64x128-nbuf2", dict(CONV_TILE=3, CONV_NBUF=2)), ("64x64", dict(CONV_TILE=4))]
F32_LOADERS = ["generic", "fast", "fast-s2", "stem-nchw", "dual", "contig", "affine-dil2", "chscale"]


def _f32_op(loader):
    """-> (run() -> y [2, 9, 15, >= CO] on the device, float64 NHWC reference) for one operand form."""
    import bev_native as nat

    def make():
        g = torch.Generator().manual_seed(1000 + F32_LOADERS.index(loader))
        N, Ho, Wo = 2, 9, 15
        b = _rand(g, CO) * 0.1
        bd = b.to(DEV)
        res = _rand(g, N, Ho, Wo, CO)

        def wgt(Ci, K):
            return _rand(g, CO, Ci, K, K) / (Ci * K * K) ** 0.5

        if loader == "generic":  # LOADER 0: Ci = 6 NHWC, 3x3 / p1, K = 54 -> two 32-deep steps
            x, w = _rand(g, N, Ho, Wo, 6), wgt(6, 3)
            ref = _act64(_nhwc(F.conv2d(_nchw(x).double(), w.double(), b.double(), 1, 1)) + res.double(), 1)
            xd, p, rd = x.to(DEV), nat.pack_conv_weight(w.to(DEV)), res.to(DEV)
            return (lambda: nat.conv2d_nhwc(xd, p, bd, CO, 3, 3, 1, 1, True, residual=rd)), ref
        if loader in ("fast", "fast-s2"):  # LOADER 1 (k_conv_dma with CONV_DMA): Ci = 32, 3x3 / p1, nine steps
            s = 2 if loader == "fast-s2" else 1
            x, w = _rand(g, N, 17 if s == 2 else Ho, 29 if s == 2 else Wo, 32), wgt(32, 3)
            ref = _act64(_nhwc(F.conv2d(_nchw(x).double(), w.double(), b.double(), s, 1)) + res.double(), 1)
            xd, p, rd = x.to(DEV), nat.pack_conv_weight(w.to(DEV)), res.to(DEV)
            return (lambda: nat.conv2d_nhwc(xd, p, bd, CO, 3, 3, s, 1, True, residual=rd)), ref
        if loader == "stem-nchw":  # LOADER 2: NCHW Ci = 3, 7x7 / s2 / p3, K = 147 -> five steps
            x, w = _rand(g, N, 3, 17, 29), wgt(3, 7)
            ref = _act64(_nhwc(F.conv2d(x.double(), w.double(), b.double(), 2, 3)), 1)
            xd, p = x.to(DEV), nat.pack_conv_weight(w.to(DEV))
            return (lambda: nat.conv2d_nhwc(xd, p, bd, CO, 7, 7, 2, 3, True, in_nchw=True)), ref
        if loader == "dual":  # LOADER 3: K = [32 of x | 64 of x2 at stride 2] -> three steps
            x, x2, w1, w2 = _rand(g, N, Ho, Wo, 32), _rand(g, N, 17, 29, 64), wgt(32, 1), wgt(64, 1)
            ref = _act64(_nhwc(F.conv2d(_nchw(x).double(), w1.double(), b.double())
                               + F.conv2d(_nchw(x2).double(), w2.double(), None, 2)), 1)
            p = nat.pack_conv_weight(torch.cat([w1, w2], 1).contiguous().to(DEV))
            xd, x2d = x.to(DEV), x2.to(DEV)
            return (lambda: nat.conv2d_dual_nhwc(xd, x2d, 2, p, bd, CO, relu=True)), ref
        if loader == "contig":  # LOADER 4: 1x1 over Ci = 72 (% 4, not % 32) -> three steps, the last K-padded; SiLU
            x, w = _rand(g, N, Ho, Wo, 72), wgt(72, 1)
            ref = _act64(_nhwc(F.conv2d(_nchw(x).double(), w.double(), b.double())) + res.double(), 2)
            xd, p, rd = x.to(DEV), nat.pack_conv_weight(w.to(DEV)), res.to(DEV)
            return (lambda: nat.conv2d_nhwc(xd, p, bd, CO, 1, 1, 1, 0, nat.ACT_SILU, residual=rd)), ref
        if loader == "affine-dil2":  # LOADER 5: relu(x scale + shift) in the loader, 3x3 / p2 / dilation 2, ldy > Co
            x, w = _rand(g, N, Ho, Wo, 32), wgt(32, 3)
            sc, sh = _rand(g, N, 32), _rand(g, N, 32) * 0.5 + 0.5
            op = (x * sc[:, None, None, :] + sh[:, None, None, :]).clamp_min(0)  # fp32: one multiply, one add
            ref = _act64(_nhwc(F.conv2d(_nchw(op).double(), w.double(), b.double(), 1, 2, 2)), 1)
            xd, p, scd, shd = x.to(DEV), nat.pack_conv_weight(w.to(DEV)), sc.to(DEV), sh.to(DEV)

            def run():
                out = torch.full((N, Ho, Wo, CO + 8), 7.0, device=DEV)
                nat.conv2d_nhwc_ex(xd, p, bd, CO, 3, 2, 2, in_scale=scd, in_shift=shd, in_relu=True, out=out,
                                   relu=True)
                assert bool((out[..., CO:] == 7.0).all()), "columns past Co written"
                return out[..., :CO].contiguous()
            return run, ref
        assert loader == "chscale"  # LOADER 6: x gate[n][ci] in the loader (tiles that straddle the two images)
        x, w, gate = _rand(g, N, Ho, Wo, 32), wgt(32, 3), torch.rand(N, 32, generator=g) + 0.25
        op = x * gate[:, None, None, :]
        ref = _act64(_nhwc(F.conv2d(_nchw(op).double(), w.double(), b.double(), 1, 1)) + res.double(), 1)
        xd, p, rd, gd = x.to(DEV), nat.pack_conv_weight(w.to(DEV)), res.to(DEV), gate.to(DEV)
        return (lambda: nat.conv2d_nhwc(xd, p, bd, CO, 3, 3, 1, 1, True, residual=rd, ascale=gd)), ref

    return _cached(("f32", loader), make)


def _f32_default(loader):
    """The default-dispatch instance's output (knobs untouched), once per operand form."""
    run, _ = _f32_op(loader)
    return _cached(("f32-default", loader), run)


@pytest.mark.parametrize("tile", F32_TILES, ids=[t[0] for t in F32_TILES])
@pytest.mark.parametrize("loader", F32_LOADERS)
def test_f32_conv_tile_loader_nbuf_instances(loader, tile, request):
    """k_conv<tile, LOADER, NBUF> for every loader on every tile and staging depth (register staging: CONV_DMA 0)."""
    import bev_native as nat
    run, ref = _f32_op(loader)
    y0 = _f32_default(loader)
    knobs = dict(tile[1], CONV_DMA=0)
    with nat.tuned(**knobs):
        y = run()
    torch.cuda.synchronize()
    _check12(request.node.callspec.id, y, {"default": y0}, ref)
    if "CONV_NBUF" in knobs:  # bound 4: the staging depth against the tile's automatic one
        with nat.tuned(CONV_TILE=knobs["CONV_TILE"], CONV_DMA=0):
            assert torch.equal(y, run())
        assert torch.equal(y, y0)  # ... and every tile sums in the same K order (see the module docstring)


@pytest.mark.parametrize("tile", [1, 2, 3, 4], ids=["128x128", "128x64", "64x128", "64x64"])
@pytest.mark.parametrize("loader", ["fast", "fast-s2"])
def test_f32_conv_dma_every_tile(loader, tile, request):
    """k_conv_dma<tile> (CONV_DMA 2: LDS-DMA staging on every tile) == register staging (CONV_DMA 0), bit for bit."""
    import bev_native as nat
    run, ref = _f32_op(loader)
    with nat.tuned(CONV_TILE=tile, CONV_DMA=2):
        y = run()
    with nat.tuned(CONV_TILE=tile, CONV_DMA=0):
        yr = run()
    torch.cuda.synchronize()
    _check12(request.node.callspec.id, y, {"default": _f32_default(loader)}, ref)
    assert torch.equal(y, yr)
    assert torch.equal(y, _f32_default(loader))


@pytest.mark.parametrize("dma", [0, 2], ids=["regs", "dma"])
@pytest.mark.parametrize("tile", [1, 2, 3, 4], ids=["128x128", "128x64", "64x128", "64x64"])
def test_f32_conv_xcd_order_off(tile, dma, request):
    """CONV_XCD 0 (plain block order) == CONV_XCD 1 (default), bit for bit, on grids of 14 / 28 / 26 / 52 workgroups
    (more than 8, no multiple of 8: the remainder branch of the XCD permutation), k_conv and k_conv_dma."""
    import bev_native as nat

    def make():
        g = torch.Generator().manual_seed(77)
        x, w, b = _rand(g, 2, 17, 23, 64), _rand(g, CO, 64, 1, 1) / 8, _rand(g, CO) * 0.1
        ref = _act64(_nhwc(F.conv2d(_nchw(x).double(), w.double(), b.double())), 1)
        xd, p, bd = x.to(DEV), nat.pack_conv_weight(w.to(DEV)), b.to(DEV)
        run = lambda: nat.conv2d_nhwc(xd, p, bd, CO, 1, 1, 1, 0, True)  # noqa: E731
        return run, ref, run()
    run, ref, y0 = _cached("f32-xcd", make)
    with nat.tuned(CONV_TILE=tile, CONV_DMA=dma, CONV_XCD=0):
        y = run()
    with nat.tuned(CONV_TILE=tile, CONV_DMA=dma, CONV_XCD=1):
        y1 = run()
    torch.cuda.synchronize()
    _check12(request.node.callspec.id, y, {"default": y0}, ref)
    assert torch.equal(y, y1)
    assert torch.equal(y, y0)


@pytest.mark.parametrize("N,H,W,C", [(2, 9, 15, 6), (65536, 2, 2, 4)], ids=["scalar-c6", "flat-vec-n65536"])
def test_maxpool_flat_kernels(N, H, W, C):
    """k_maxpool<false> (C % 4 != 0) and k_maxpool<true> (float4 channels, taken past 65535 images where the
    (row piece, output row, image) grid of k_maxpool_rows does not apply): exactly torch's max_pool2d(3, 2, 1)."""
    import bev_native as nat
    x = _rand(torch.Generator().manual_seed(C), N, H, W, C)
    ref = _nhwc(F.max_pool2d(_nchw(x).double(), 3, 2, 1))
    y = nat.maxpool_nhwc(x.to(DEV), 3, 2, 1)
    torch.cuda.synchronize()
    assert torch.equal(y.cpu().double(), ref)


# ======================================================================================================================
# split-bf16 convs (bev_conv_x6.hip): dispatch_x6<DUAL>
# ======================================================================================================================
def _x6_dual_op(Ci, Ci2, s2, Co):
    import bev_native as nat

    def make():
        g = torch.Generator().manual_seed(Ci + 3 * Ci2 + Co + s2)
        N, Ho, Wo = 2, 9, 15
        H2, W2 = (17, 29) if s2 == 2 else (Ho, Wo)
        x, x2 = _rand(g, N, Ho, Wo, Ci), _rand(g, N, H2, W2, Ci2)
        w1, w2, b = _rand(g, Co, Ci, 1, 1) / Ci ** 0.5, _rand(g, Co, Ci2, 1, 1) / Ci2 ** 0.5, _rand(g, Co) * 0.1
        ref = _act64(_nhwc(F.conv2d(_nchw(x).double(), w1.double(), b.double())
                           + F.conv2d(_nchw(x2).double(), w2.double(), None, s2)), 1)
        wcat = torch.cat([w1, w2], 1).contiguous().to(DEV)
        xd, x2d, bd, p6 = x.to(DEV), x2.to(DEV), b.to(DEV), nat.pack_conv_weight_x6(wcat)
        run = lambda: nat.conv2d_dual_nhwc(xd, x2d, s2, p6, bd, Co, relu=True)  # noqa: E731
        # the exact-f32 MFMA kernel on the same operands: one 1x1 conv over [x | x2 at the strided pixels]
        xcat = torch.cat([xd, x2d[:, ::s2, ::s2]], 3).contiguous()
        yf = nat.conv2d_nhwc(xcat, nat.pack_conv_weight(wcat), bd, Co, 1, 1, 1, 0, True)
        return run, ref, {"x6 default": run(), "exact-f32": yf}
    return _cached(("x6-dual", Ci, Ci2, s2, Co), make)


X6_DUAL = [
    # id, Ci, Ci2, stride2, Co, knobs, same bits as the default dispatch
    ("x6-dual-16deep-128x128", 48, 80, 2, 200, {}, False),             # Ci, Ci2 % 32 != 0, Co > 64
    ("x6-dual-16deep-128x64", 48, 80, 2, 40, {}, False),               # Co <= 64
    ("x6-dual-16deep-128x64-tile2", 48, 80, 2, 200, dict(CONV_X6_TILE=2), True),
    ("x6-dual-16deep-128x128-tile1", 48, 80, 2, 40, dict(CONV_X6_TILE=1), True),
    ("x6-dual-16deep-128x128-s1", 48, 16, 1, 72, {}, False),           # stride2 = 1
    ("x6-dual-16deep-128x128-kernel1", 32, 64, 2, 200, dict(CONV_X6_KERNEL=1), True),
    ("x6-dual-16deep-128x64-kernel1", 32, 64, 2, 200, dict(CONV_X6_KERNEL=1, CONV_X6_TILE=2), True),
    ("x6-dual-16deep-128x64-kernel1-co40", 32, 64, 2, 40, dict(CONV_X6_KERNEL=1), True),
    ("x6-dual-32deep-128x64", 32, 64, 2, 40, {}, False),
    ("x6-dual-32deep-128x64-tile2", 32, 64, 2, 200, dict(CONV_X6_TILE=2), True),
    ("x6-dual-32deep-128x128-tile1", 32, 64, 2, 40, dict(CONV_X6_TILE=1), True),
    ("x6-dual-32deep-128x128", 32, 64, 2, 200, {}, False),
    ("x6-dual-32deep-nt-ignored", 32, 64, 2, 40, dict(CONV_X6_NT=1), True),   # the dual form has no NT instance
]


@pytest.mark.parametrize("case", X6_DUAL, ids=[c[0] for c in X6_DUAL])
def test_x6_dual_instances(case):
    """dispatch_x6<true>: k_conv_x6<.., true> (16-deep steps) and k_conv_x6b<.., true> (32-deep) on both tiles."""
    import bev_native as nat
    tag, Ci, Ci2, s2, Co, knobs, same_bits = case
    run, ref, pinned = _x6_dual_op(Ci, Ci2, s2, Co)
    with nat.tuned(**knobs):
        y = run()
    torch.cuda.synchronize()
    _check12(tag, y, pinned, ref)
    if same_bits:
        assert torch.equal(y, pinned["x6 default"])


def _x6_single_op(Ci, K, s, Co, act):
    import bev_native as nat

    def make():
        g = torch.Generator().manual_seed(Ci + 5 * K + Co + s)
        N, Ho, Wo = 2, 9, 15
        H, W = (17, 29) if s == 2 else (Ho, Wo)
        x, w, b = _rand(g, N, H, W, Ci), _rand(g, Co, Ci, K, K) / (Ci * K * K) ** 0.5, _rand(g, Co) * 0.1
        res = _rand(g, N, Ho, Wo, Co)
        ref = _act64(_nhwc(F.conv2d(_nchw(x).double(), w.double(), b.double(), s, K // 2)) + res.double(), act)
        xd, bd, rd, wd = x.to(DEV), b.to(DEV), res.to(DEV), w.to(DEV)
        p6 = nat.pack_conv_weight_x6(wd)
        run = lambda: nat.conv2d_nhwc_x6(xd, p6, bd, Co, K, K, s, K // 2, 1, act, residual=rd)  # noqa: E731
        yf = nat.conv2d_nhwc(xd, nat.pack_conv_weight(wd), bd, Co, K, K, s, K // 2, act, residual=rd)
        return run, ref, {"x6 default": run(), "exact-f32": yf}
    return _cached(("x6-single", Ci, K, s, Co, act), make)


X6_SINGLE = [
    # id, Ci, K, stride, Co, act, knobs, same bits as the default dispatch
    ("x6-16deep-128x128", 48, 3, 1, 200, 1, {}, False),
    ("x6-16deep-128x64", 48, 3, 1, 40, 2, {}, False),
    ("x6-16deep-128x64-tile2-s2", 16, 3, 2, 200, 1, dict(CONV_X6_TILE=2), True),
    ("x6-16deep-128x128-kernel1", 64, 3, 1, 200, 1, dict(CONV_X6_KERNEL=1), True),
    ("x6-16deep-128x64-kernel1", 64, 3, 1, 72, 1, dict(CONV_X6_KERNEL=1, CONV_X6_TILE=2), True),
    ("x6-32deep-nt-128x64", 64, 3, 1, 40, 1, dict(CONV_X6_NT=1), True),
    ("x6-32deep-nt-128x64-tile2", 64, 3, 1, 72, 1, dict(CONV_X6_NT=1, CONV_X6_TILE=2), True),
    ("x6-32deep-128x64-tile2", 64, 3, 1, 200, 1, dict(CONV_X6_TILE=2), True),
    ("x6-32deep-128x128-tile1-s2", 32, 3, 2, 40, 1, dict(CONV_X6_TILE=1), True),
]


@pytest.mark.parametrize("case", X6_SINGLE, ids=[c[0] for c in X6_SINGLE])
def test_x6_single_instances(case):
    """dispatch_x6<false>: k_conv_x6<.., false>, k_conv_x6b<.., false> and its non-temporal-load instance."""
    import bev_native as nat
    tag, Ci, K, s, Co, act, knobs, same_bits = case
    run, ref, pinned = _x6_single_op(Ci, K, s, Co, act)
    with nat.tuned(**knobs):
        y = run()
    torch.cuda.synchronize()
    _check12(tag, y, pinned, ref)
    if same_bits:
        assert torch.equal(y, pinned["x6 default"])


# ======================================================================================================================
# fp16 convs (bev_conv_h16.hip): k_conv_h16 and k_conv_h16b<HIN, BN, BUF, HOUT, AFF> (+ the BN-statistics epilogue)
# ======================================================================================================================
H16_CI = 128  # two 64-deep (four 32-deep) K steps per tap


def _h16_op(Co, stride, aff):
    import bev_native as nat

    def make():
        g = torch.Generator().manual_seed(Co + 7 * stride + int(aff))
        N, Ho, Wo, Ci = 2, 9, 15, H16_CI
        H, W = (17, 29) if stride == 2 else (Ho, Wo)
        x = _rand(g, N, H, W, Ci)
        w, b = _rand(g, Co, Ci, 3, 3) / (Ci * 9) ** 0.5, _rand(g, Co)
        res = _rand(g, N, Ho, Wo, Co).half()
        sc, sh = _rand(g, N, Ci), _rand(g, N, Ci) * 0.5 + 0.5
        x16 = x.half()
        # the operand as the kernel sees it: f16(x), or f16(max(float(f16 x) scale + shift, 0)) (fp32 mul, fp32 add)
        op = (x16.float() * sc[:, None, None, :] + sh[:, None, None, :]).clamp_min(0).half() if aff else x16
        opd, wd = _nchw(op.double()), w.half().double()
        z = _nhwc(F.conv2d(opd, wd, None, stride, 1))
        mag = _nhwc(F.conv2d(opd.abs(), wd.abs(), None, stride, 1))
        return dict(N=N, Ho=Ho, Wo=Wo, Co=Co, stride=stride, z=z, mag=mag, b=b, res=res, x=x.to(DEV),
                    x16=x16.to(DEV), bd=b.to(DEV), res16=res.to(DEV), res32=res.float().to(DEV), sc=sc.to(DEV),
                    sh=sh.to(DEV), packed=nat.pack_conv_weight_h16(w.to(DEV)))
    return _cached(("h16", Co, stride, aff), make)


def _h16_bound(c, y_half, act, with_res):
    """-> (float64 reference, per-element bound): bound 1 of the fp16 family (see the module docstring)."""
    Kt = H16_CI * 9
    ref = c["z"] + c["b"].double()
    mag = c["mag"] + c["b"].double().abs()
    if with_res:
        ref, mag = ref + c["res"].double(), mag + c["res"].double().abs()
    ref = _act64(ref, act)
    if y_half:
        bound = 2.0 ** -11 * ref.abs() + (Kt + 2) * 2.0 ** -24 * mag + 2.0 ** -24
        return ref, bound * 1.2 if act == 2 else bound
    bound = Kt * 2.0 ** -24 * mag + 1e-6
    return ref, bound * 1.2 + 1e-6 if act == 2 else bound


def _h16_check(tag, y, y0, ref, bound):
    err = (y.cpu().double() - ref).abs()
    print(f"[instance] {tag}: max err {float(err.max()):.3e}, max err / bound {float((err / bound).max()):.3f}")
    assert bool(torch.isfinite(y.float()).all()), tag
    assert bool((err <= bound).all()), (tag, float((err - bound).max()))
    _check12(tag, y.float(), {"default": y0.float()}, ref, bar=float("inf"))  # bound 2 (bound 1 is the line above)
    assert torch.equal(y, y0), (tag, int((y != y0).sum()))  # bound 3: CONV_H16_KERNEL / CONV_H16_BUF keep the bits


H16_KERN = {0: "k0", 1: "k1-32deep", 2: "k2-bn128", 3: "k3-bn64"}


def _h16_ids(entry):
    out = []
    for Co in (200, 40):
        for kern in (0, 1, 2, 3):
            for xh, buf in ((0, 1), (1, 1), (1, 0)):
                if entry == "aff" and not xh:
                    continue
                for flag in (0, 1):  # f32out: the statistics epilogue; f16out: -; aff: fp16 / fp32 output
                    if entry == "f16out" and flag:
                        continue
                    out.append((Co, kern, xh, buf, flag))
    return out


def _h16_id(entry, p):
    Co, kern, xh, buf, flag = p
    bn = 64 if (kern == 3 or (Co <= 64 and kern != 2)) else 128
    if entry == "f32out" and kern == 1 and not xh and not flag:
        name = "h16-32deep"
    else:
        name = f"h16b-bn{bn}"
    tail = {"f32out": "-stats" if flag else "", "f16out": "", "aff": "-f16out" if flag else "-f32out"}[entry]
    return (f"{name}-{'xf16' if xh else 'xf32'}{('-buf' if buf else '-ptr') if xh else ''}-{entry}{tail}"
            f"-co{Co}-{H16_KERN[kern]}")


@pytest.mark.parametrize("p", _h16_ids("f32out"), ids=[_h16_id("f32out", p) for p in _h16_ids("f32out")])
def test_h16_f32_output_instances(p):
    """bev_conv2d_h16_ex_f32: k_conv_h16 and k_conv_h16b<HIN, BN, BUF> with bias + residual + ReLU, or with the
    BatchNorm statistics epilogue (raw conv output; mean / rstd against float64 statistics of z at
    test_conv_h16_epilogue_batchnorm_stats's tolerances)."""
    import bev_native as nat
    Co, kern, xh, buf, stats = p
    c = _h16_op(Co, 1, False)
    x = c["x16"] if xh else c["x"]

    def run():
        if stats:
            return nat.conv2d_h16_any(x, c["packed"], Co, 3, 3, 1, 1, stats=True)
        return nat.conv2d_h16_any(x, c["packed"], Co, 3, 3, 1, 1, residual=c["res32"], bias=c["bd"], act=1), None
    y0, _ = _cached(("h16-f32out-default", Co, xh, stats), run)
    with nat.tuned(CONV_H16_KERNEL=kern, CONV_H16_BUF=buf):
        y, tiles = run()
    torch.cuda.synchronize()
    if stats:
        ref, bound = c["z"], H16_CI * 9 * 2.0 ** -24 * c["mag"] + 1e-6
    else:
        ref, bound = _h16_bound(c, False, 1, True)
    _h16_check(_h16_id("f32out", p), y, y0, ref, bound)
    if stats:
        M = c["N"] * c["Ho"] * c["Wo"]
        assert tiles.shape == (Co, (M + 127) // 128, 2)
        ones, zeros = torch.ones(Co, device=DEV), torch.zeros(Co, device=DEV)
        mean, rstd = nat.batchnorm_finalize_tiles(tiles, M, ones, zeros, zeros.clone(), ones.clone(), 1e-5, 0.1)[:2]
        zd = y.double().reshape(M, Co)
        torch.testing.assert_close(mean.double(), zd.mean(0), rtol=1e-6, atol=1e-7)
        torch.testing.assert_close(rstd.double(), 1 / torch.sqrt(zd.var(0, unbiased=False) + 1e-5), rtol=1e-6, atol=0)


@pytest.mark.parametrize("p", _h16_ids("f16out"), ids=[_h16_id("f16out", p) for p in _h16_ids("f16out")])
def test_h16_f16_output_instances(p):
    """bev_conv2d_h16_h16: k_conv_h16b<HIN, BN, BUF, HOUT = true> with bias + fp16 residual + SiLU."""
    import bev_native as nat
    Co, kern, xh, buf, _ = p
    c = _h16_op(Co, 1, False)
    x = c["x16"] if xh else c["x"]
    run = lambda: nat.conv2d_h16_half(x, c["packed"], c["bd"], Co, 3, 3, 1, 1, 1, 2, residual=c["res16"])  # noqa: E731
    y0 = _cached(("h16-f16out-default", Co, xh), run)
    with nat.tuned(CONV_H16_KERNEL=kern, CONV_H16_BUF=buf):
        y = run()
    torch.cuda.synchronize()
    _h16_check(_h16_id("f16out", p), y, y0, *_h16_bound(c, True, 2, True))


@pytest.mark.parametrize("p", _h16_ids("aff"), ids=[_h16_id("aff", p) for p in _h16_ids("aff")])
def test_h16_affine_operand_instances(p):
    """bev_conv2d_h16_affine with the GroupNorm affine + ReLU in the loader: k_conv_h16b<true, BN, BUF, HOUT, true>,
    fp16 and fp32 (wider buffer) output, bias + ReLU."""
    import bev_native as nat
    Co, kern, _, buf, y_half = p
    c = _h16_op(Co, 1, True)

    def run():
        out = None if y_half else torch.full((c["N"], c["Ho"], c["Wo"], Co + 8), 7.0, device=DEV)
        y = nat.conv2d_h16_affine(c["x16"], c["packed"], c["bd"], Co, 3, 1, 1, in_scale=c["sc"], in_shift=c["sh"],
                                  in_relu=True, y_half=bool(y_half), out=out, act=1)
        if out is not None:
            assert bool((out[..., Co:] == 7.0).all()), "columns past Co written"
            y = out[..., :Co].contiguous()
        return y
    y0 = _cached(("h16-aff-default", Co, y_half), run)
    with nat.tuned(CONV_H16_KERNEL=kern, CONV_H16_BUF=buf):
        y = run()
    torch.cuda.synchronize()
    _h16_check(_h16_id("aff", p), y, y0, *_h16_bound(c, bool(y_half), 1, False))


H16_S2 = [("h16-32deep-xf32-s2", 1, 0, 1, False), ("h16b-bn128-xf32-s2", 0, 0, 1, False),
          ("h16b-bn64-xf16-ptr-s2", 3, 1, 0, False), ("h16b-bn128-xf16-buf-f16out-s2", 2, 1, 1, True)]


@pytest.mark.parametrize("case", H16_S2, ids=[c[0] for c in H16_S2])
def test_h16_stride2_instances(case):
    """The family's stride-2 cases (3x3 / s2 / p1 over 17 x 29): border taps on every side at stride 2."""
    import bev_native as nat
    tag, kern, xh, buf, y_half = case
    Co = 200
    c = _h16_op(Co, 2, False)
    x = c["x16"] if xh else c["x"]

    def run():
        if y_half:
            return nat.conv2d_h16_half(x, c["packed"], c["bd"], Co, 3, 3, 2, 1, 1, 1, residual=c["res16"])
        return nat.conv2d_h16_any(x, c["packed"], Co, 3, 3, 2, 1, residual=c["res32"], bias=c["bd"], act=1)
    y0 = _cached(("h16-s2-default", xh, y_half), run)
    with nat.tuned(CONV_H16_KERNEL=kern, CONV_H16_BUF=buf):
        y = run()
    torch.cuda.synchronize()
    _h16_check(tag, y, y0, *_h16_bound(c, y_half, 1, True))


@pytest.mark.parametrize("dz_half", [False, True], ids=["dzf32", "dzf16"])
@pytest.mark.parametrize("x_half", [False, True], ids=["xf32", "xf16"])
def test_wgrad_h16b_operand_forms(x_half, dz_half):
    """k_wgrad_h16b<XH, DH> (the register-transpose weight gradient, taken where Co % 8 != 0) for every storage form
    of its operands -- fp16 x with an fp32 gradient is a form no other test passes; against the float64 weight
    gradient of the fp16-rounded operands, relative to sum |terms| < 2e-6 (test_wgrad_h16_fp16_gradient_vs_float64)."""
    import bev_native as nat

    def make():
        g = torch.Generator().manual_seed(36)
        x, dz = _rand(g, 2, 9, 15, 64), _rand(g, 2, 9, 15, 36) * 1e-3
        xh, dh = _nchw(x.half().double()), _nchw(dz.half().double())
        ref = torch.nn.grad.conv2d_weight(xh, (36, 64, 3, 3), dh, 1, 1, 1)
        mag = torch.nn.grad.conv2d_weight(xh.abs(), (36, 64, 3, 3), dh.abs(), 1, 1, 1)
        return x.to(DEV), dz.to(DEV), ref, mag
    x, dz, ref, mag = _cached("wgrad-h16b", make)
    dw = nat.conv_wgrad_h16_any(x.half() if x_half else x, dz.half() if dz_half else dz, 3, 3, 1, 1)
    torch.cuda.synchronize()
    assert dw.shape == (36, 64, 3, 3) and bool(torch.isfinite(dw).all())
    assert float(((dw.cpu().double() - ref).abs() / (mag + 1e-12)).max()) < 2e-6


# ======================================================================================================================
# k_stem3<CO, SP> (bev_effnet.hip): BEV_TUNE_STEM3_STAGE
# ======================================================================================================================
@pytest.mark.parametrize("stage", [0, 1, 2], ids=["stage0-registers", "stage1-64px", "stage2-32px"])
@pytest.mark.parametrize("Co", [32, 40, 48, 64])
def test_stem3_stage_instances(Co, stage, request):
    """k_stem3<Co, 0 / 64 / 32>: 3x3 / s2 / p1 over NCHW [2, 3, 17, 131] -> 9 x 66 outputs (two ragged 8 x 64 tiles
    each way), SiLU; within test_stem3_vs_float64_and_generic_conv's 2e-6 max|ref| and the default stage's bits."""
    import bev_native as nat

    def make():
        g = torch.Generator().manual_seed(Co)
        x, w, b = _rand(g, 2, 3, 17, 131), _rand(g, Co, 3, 3, 3) / 27 ** 0.5, _rand(g, Co) * 0.1
        ref = _act64(_nhwc(F.conv2d(x.double(), w.double(), b.double(), 2, 1)), 2)
        xd, wt, bd = x.to(DEV), w.permute(1, 2, 3, 0).reshape(27, Co).contiguous().to(DEV), b.to(DEV)
        run = lambda: nat.conv2d_stem3(xd, wt, bd, nat.ACT_SILU)  # noqa: E731
        return run, ref, run()
    run, ref, y0 = _cached(("stem3", Co), make)
    with nat.tuned(STEM3_STAGE=stage):
        y = run()
    torch.cuda.synchronize()
    assert y.shape == ref.shape
    _check12(request.node.callspec.id, y, {"default": y0}, ref, bar=2e-6)
    assert torch.equal(y, y0)
