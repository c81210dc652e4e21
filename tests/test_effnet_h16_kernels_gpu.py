"""The fp16-storage kernels of the EfficientNet "f16" inference arithmetic (bev_effnet_h16.hip, k_stem3's fp16 store),
each through its public wrapper, against float64 torch on the CPU over the operands as the kernel sees them.

 conv2d_pw_h16      the operand a = f16(float(y16) * gate) is computed on the host in torch fp32 (the kernel's exact
                    operation), then |y - ref| <= 2^-11 |ref| + (Ci + 2) 2^-24 (sum |a||w| + |b| + |r|) + 2^-24, the
                    bound of tests/test_conv_h16_half_gpu.py (a); for the fp32 output without the first term.  The
                    output is written into the middle of a sentinel-filled buffer, at ldy = Co and ldy = Co + 8:
                    nothing outside [M][Co] changes.  M = 2 x 11 x 19 = 418 is ragged against the 32-pixel wave and
                    the 128-pixel workgroup.  test_pw_h16_every_instance runs every compiled instance (operand size
                    x output type) under the same bound.
 dwconv2d_nhwc_h16  the same bound with K K products, x 1.2 for SiLU (the hardware exp2 / rcp form); the SE partials
                    sum to the channel sums of the RETURNED fp16 tensor within 1e-5 max(1, |sums|).
 ir_expand_dw_h16   the 20 (K, S, Ci) cases and shapes of test_kernel_instances_gpu.py::test_irdw_instances.  A rounding
                    of h that flips carries through a depthwise weight into y, so no elementwise ulp bound holds
                    (on the CPU outputs near zero moved by up to ~140 fp16 ulps).  Instead, with exact = the float64
                    forward of the unrounded operands on the fp16-rounded input and R64 = float64 sums with the
                    kernel's rounding points (fp16 weights, h = f16(SiLU), y = f16(SiLU)): relative L2 error against
                    exact <= 1.5 x R64's, max error <= 2 x R64's (the bars of test_encoder_f16_gpu.py), and at most
                    1 % of the outputs differ from f16(R64).
                    CPU check of these inputs (an fp32-accumulating torch restatement of the same rounding points in
                    place of the kernel, all 20 cases): L2 ratio 0.999-1.001, max ratio 1.000-1.000, 0.035-0.127 %
                    of the elements differ from f16(R64).
 conv2d_stem3_h16   bitwise conv2d_stem3(...).half().
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


def _silu64(z):
    return z * torch.sigmoid(z)


# ---- pointwise -------------------------------------------------------------------------------------------------------
PW_N, PW_H, PW_W = 2, 11, 19
PW = [  # Ci, Co, gate, residual, fp32 output
    (24, 24, True, True, False), (32, 16, False, False, False), (40, 72, False, False, True),
    (96, 24, True, False, False), (144, 40, True, True, False), (240, 40, True, False, False),
    (288, 48, True, True, False)]
PW_IDS = [f"{ci}to{co}{'g' if g else ''}{'r' if r else ''}{'_f32' if f else ''}" for ci, co, g, r, f in PW]


def _pw_case(i):
    def make():
        Ci, Co, has_gate, has_res, f32 = PW[i]
        g = torch.Generator().manual_seed(300 + i)
        y16 = torch.randn(PW_N, PW_H, PW_W, Ci, generator=g).half()
        gate = torch.sigmoid(torch.randn(PW_N, Ci, generator=g)) if has_gate else None
        w16 = (torch.randn(Co, Ci, generator=g) / Ci ** 0.5).half()
        b = torch.randn(Co, generator=g)
        r16 = torch.randn(PW_N, PW_H, PW_W, Co, generator=g).half() if has_res else None
        a16 = (y16.float() * gate.view(PW_N, 1, 1, Ci)).half() if has_gate else y16  # the kernel's own operation
        ref = a16.double() @ w16.double().t() + b.double()
        mag = a16.double().abs() @ w16.double().abs().t() + b.double().abs()
        if has_res:
            ref, mag = ref + r16.double(), mag + r16.double().abs()
        dev = lambda t: None if t is None else t.to(DEV)
        return dict(Ci=Ci, Co=Co, f32=f32, y16=dev(y16), gate=dev(gate), w16=dev(w16), b=dev(b), r16=dev(r16), ref=ref,
                    mag=mag)
    return _cached(("pw", i), make)


@pytest.mark.parametrize("pad_cols", [0, 8], ids=["dense", "ldy+8"])
@pytest.mark.parametrize("i", range(len(PW)), ids=PW_IDS)
def test_pw_h16_vs_float64_and_writes_nothing_outside(i, pad_cols):
    import bev_native as nat
    c = _pw_case(i)
    Co, ldy, M = c["Co"], c["Co"] + pad_cols, PW_N * PW_H * PW_W
    odt = torch.float32 if c["f32"] else torch.float16
    SENT, GUARD = 777.0, 40  # guard rows before and after the output
    buf = torch.full((M + 2 * GUARD, ldy), SENT, dtype=odt, device=DEV)
    out = buf[GUARD:GUARD + M].view(PW_N, PW_H, PW_W, ldy)
    got = nat.conv2d_pw_h16(c["y16"], c["w16"], c["b"], gate=c["gate"], residual=c["r16"], f32_out=c["f32"], out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and got.dtype == odt
    host = buf.cpu()
    assert bool((host[:GUARD] == SENT).all()) and bool((host[GUARD + M:] == SENT).all())
    assert bool((host[GUARD:GUARD + M, Co:] == SENT).all())
    y = host[GUARD:GUARD + M, :Co].double().view(PW_N, PW_H, PW_W, Co)
    ref = c["ref"]
    bound = (c["Ci"] + 2) * 2.0 ** -24 * c["mag"] + 2.0 ** -24
    if not c["f32"]:
        bound = bound + 2.0 ** -11 * ref.abs()
    err = (y - ref).abs()
    print(f"{PW_IDS[i]}: max err {float(err.max()):.3e}  max err/bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), float((err - bound).max())
    if pad_cols == 0:  # the wrapper's own allocation gives the same values
        y2 = nat.conv2d_pw_h16(c["y16"], c["w16"], c["b"], gate=c["gate"], residual=c["r16"], f32_out=c["f32"])
        assert y2.dtype == odt and torch.equal(y2.cpu().view(M, Co), host[GUARD:GUARD + M, :Co])


# every k_pw_h16<NS, F32OUT> instance (NS = the operand's 16-channel register pieces: 2, 3, 6, 9, 12, 15, 18 for the
# trunk's widths, 32 for anything up to Ci 512), fp16 and fp32 output, and two widths that run in the next size up
# (Ci 64 in NS 6, Ci 320 in NS 32: the pieces past Ci are zero).  M = 5 x 9 = 45: two waves, the second ragged.
PW_INST = [(Ci, f32) for f32 in (False, True) for Ci in (32, 48, 64, 96, 144, 192, 240, 288, 320, 512)]


@pytest.mark.parametrize("Ci,f32", PW_INST, ids=[f"ci{Ci}{'_f32' if f else ''}" for Ci, f in PW_INST])
def test_pw_h16_every_instance(Ci, f32):
    import bev_native as nat
    N, H, W, Co = 1, 5, 9, 40
    g = torch.Generator().manual_seed(500 + Ci)
    y16 = torch.randn(N, H, W, Ci, generator=g).half()
    gate = torch.sigmoid(torch.randn(N, Ci, generator=g))
    w16 = (torch.randn(Co, Ci, generator=g) / Ci ** 0.5).half()
    b = torch.randn(Co, generator=g)
    r16 = torch.randn(N, H, W, Co, generator=g).half()
    a16 = (y16.float() * gate.view(N, 1, 1, Ci)).half()
    ref = a16.double() @ w16.double().t() + b.double() + r16.double()
    mag = a16.double().abs() @ w16.double().abs().t() + b.double().abs() + r16.double().abs()
    y = nat.conv2d_pw_h16(y16.to(DEV), w16.to(DEV), b.to(DEV), gate=gate.to(DEV), residual=r16.to(DEV), f32_out=f32)
    torch.cuda.synchronize()
    assert y.dtype == (torch.float32 if f32 else torch.float16) and tuple(y.shape) == (N, H, W, Co)
    bound = (Ci + 2) * 2.0 ** -24 * mag + 2.0 ** -24
    if not f32:
        bound = bound + 2.0 ** -11 * ref.abs()
    err = (y.cpu().double() - ref).abs()
    print(f"Ci {Ci}{' f32' if f32 else ''}: max err {float(err.max()):.3e}  max err/bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), float((err - bound).max())


# ---- depthwise -------------------------------------------------------------------------------------------------------
DW_HO, DW_WO = 11, 19
DW = [(C, K, S, act) for C in (24, 32, 40) for K, S in ((3, 1), (3, 2), (5, 1), (5, 2)) for act in (2, 0)]


@pytest.mark.parametrize("C,K,S,act", DW, ids=[f"c{C}k{K}s{S}a{a}" for C, K, S, a in DW])
def test_dwconv_h16_vs_float64_and_partials(C, K, S, act):
    import bev_native as nat
    H, W = (DW_HO, DW_WO) if S == 1 else (2 * DW_HO - 1, 2 * DW_WO - 1)

    def make():
        g = torch.Generator().manual_seed(1000 * C + 10 * K + S)
        x16 = torch.randn(2, H, W, C, generator=g).half()
        wd16 = (0.3 * torch.randn(K * K, C, generator=g)).half()
        b = 0.5 * torch.randn(C, generator=g)
        w64 = wd16.double().t().reshape(C, 1, K, K)
        xd = x16.double().permute(0, 3, 1, 2)
        pre = F.conv2d(xd, w64, b.double(), S, K // 2, groups=C).permute(0, 2, 3, 1)
        mag = F.conv2d(xd.abs(), w64.abs(), b.double().abs(), S, K // 2, groups=C).permute(0, 2, 3, 1)
        return dict(x16=x16.to(DEV), wd16=wd16.to(DEV), b=b.to(DEV), pre=pre, mag=mag)
    c = _cached(("dw", C, K, S), make)
    y, ps = nat.dwconv2d_nhwc_h16(c["x16"], c["wd16"], c["b"], K, S, K // 2, act, want_psum=True)
    torch.cuda.synchronize()
    assert y.dtype == torch.float16 and tuple(y.shape) == (2, DW_HO, DW_WO, C)
    nb = nat.lib().bev_dwconv_h16_psum_blocks(DW_HO, DW_WO, C, S)
    assert ps.dtype == torch.float32 and tuple(ps.shape) == (2, nb, C)
    ref = _silu64(c["pre"]) if act == 2 else c["pre"]
    bound = 2.0 ** -11 * ref.abs() + (K * K + 2) * 2.0 ** -24 * c["mag"] + 2.0 ** -24
    if act == 2:
        bound = bound * 1.2
    yd = y.cpu().double()
    err = (yd - ref).abs()
    print(f"max err {float(err.max()):.3e}  max err/bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), float((err - bound).max())
    sums = yd.sum(dim=(1, 2))  # of the returned (rounded) tensor
    perr = float((ps.double().sum(1).cpu() - sums).abs().max())
    assert perr <= 1e-5 * max(1.0, float(sums.abs().max())), perr
    y0, none = nat.dwconv2d_nhwc_h16(c["x16"], c["wd16"], c["b"], K, S, K // 2, act)  # without partials: same y
    assert none is None and torch.equal(y0, y)


# ---- fused expansion + depthwise -------------------------------------------------------------------------------------
IRDW = [(K, S, Ci) for K, S in ((3, 1), (3, 2), (5, 1), (5, 2)) for Ci in (16, 24, 32, 40, 48)]
IR_CM, IR_HO = 96, 19


def ir_case(K, S, Ci):
    """Inputs (CPU) and the two float64 references of one case: x ~ N(0, 1), we ~ N(0, 1 / Ci), wd ~ 0.3 N(0, 1)."""
    def make():
        tc = (32 - K) // S + 1
        Ho, Wo, Cm = IR_HO, tc + 3, IR_CM
        H, W = (Ho, Wo) if S == 1 else (2 * Ho - 1, 2 * Wo - 1)
        g = torch.Generator().manual_seed(7000 + 100 * K + 10 * S + Ci)
        x16 = torch.randn(2, H, W, Ci, generator=g).half()
        we = torch.randn(Cm, Ci, generator=g) / Ci ** 0.5
        be = 0.2 * torch.randn(Cm, generator=g)
        wd = 0.3 * torch.randn(K * K, Cm, generator=g)
        bd = 0.2 * torch.randn(Cm, generator=g)
        xd = x16.double().permute(0, 3, 1, 2)

        def fwd(rounded):
            r = (lambda t: t.half().double()) if rounded else (lambda t: t)
            h = r(_silu64(F.conv2d(xd, r(we).double().view(Cm, Ci, 1, 1), be.double())))
            w64 = r(wd).double().t().reshape(Cm, 1, K, K)
            return r(_silu64(F.conv2d(h, w64, bd.double(), S, K // 2, groups=Cm))).permute(0, 2, 3, 1)
        return dict(Ho=Ho, Wo=Wo, x16=x16, we16=we.half(), be=be, wd16=wd.half(), bd=bd, exact=fwd(False), r64=fwd(True))
    return _cached(("ir", K, S, Ci), make)


def ir_report(tag, y16, c):
    """(L2 ratio, max ratio, fraction of elements off f16(R64)) of a result y16 (CPU fp16) for case c."""
    yd, exact, r64 = y16.double(), c["exact"], c["r64"]
    l2n, l2r = float((yd - exact).norm() / exact.norm()), float((r64 - exact).norm() / exact.norm())
    mxn, mxr = float((yd - exact).abs().max()), float((r64 - exact).abs().max())
    off = float((y16 != r64.half()).double().mean())
    print(f"{tag}: relL2 native {l2n:.3e} R64 {l2r:.3e} ratio {l2n / l2r:.3f}; max native {mxn:.3e} R64 {mxr:.3e} "
          f"ratio {mxn / mxr:.3f}; off f16(R64) {100 * off:.3f} %")
    return l2n / l2r, mxn / mxr, off


@pytest.mark.parametrize("K,S,Ci", IRDW, ids=[f"k_irdw_h16<{K},{S},{Ci}>" for K, S, Ci in IRDW])
def test_irdw_h16_instances(K, S, Ci):
    import bev_native as nat
    c = ir_case(K, S, Ci)
    y, ps = nat.ir_expand_dw_h16(*(c[k].to(DEV) for k in ("x16", "we16", "be", "wd16", "bd")), K, S)
    torch.cuda.synchronize()
    assert y.dtype == torch.float16 and tuple(y.shape) == (2, c["Ho"], c["Wo"], IR_CM) and tuple(ps.shape) == (2, 4, IR_CM)
    yc = y.cpu()
    assert bool(torch.isfinite(yc).all())
    l2, mx, off = ir_report(f"k_irdw_h16<{K},{S},{Ci}>", yc, c)
    assert l2 <= 1.5 and mx <= 2.0 and off <= 0.01
    sums = yc.double().sum(dim=(1, 2))  # of the returned (rounded) tensor
    perr = float((ps.double().sum(1).cpu() - sums).abs().max())
    assert perr <= 1e-5 * max(1.0, float(sums.abs().max())), perr


# ---- stem ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Co", [32, 40, 48, 64])
def test_stem3_h16_is_the_fp32_stem_rounded_once(Co):
    import bev_native as nat
    g = torch.Generator().manual_seed(Co)
    x = torch.randn(2, 3, 37, 71, generator=g).to(DEV)
    wt = (torch.randn(27, Co, generator=g) / 27 ** 0.5).to(DEV)
    b = (0.5 * torch.randn(Co, generator=g)).to(DEV)
    y16 = nat.conv2d_stem3_h16(x, wt, b, nat.ACT_SILU)
    y32 = nat.conv2d_stem3(x, wt, b, nat.ACT_SILU)
    torch.cuda.synchronize()
    assert y16.dtype == torch.float16 and tuple(y16.shape) == (2, 19, 36, Co)
    assert torch.equal(y16, y32.half()), int((y16 != y32.half()).sum())
