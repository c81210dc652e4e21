"""What the conv / depthwise / normalisation kernels do with operand VALUES the other modules never feed them: NaN,
Inf, -0, magnitudes at both ends of the fp32 / fp16 range, fp16 subnormals.  (Every other conv test draws randn at unit
scale and judges max|err| against max|ref|.)

The reference is always float64 torch on the CPU (F.conv2d, elementwise ops) over the operands as the kernel sees them
(fp32 values, or their fp16 roundings for the fp16 families; an operand affine / gate applied with the kernel's fp32
roundings first), bias, residual and activation in float64 -- never another kernel.  Shapes are those of
test_conv_instances_gpu.py: N = 2, 9 x 15 outputs (17 x 29 inputs at stride 2), M = 270 rows (ragged 128- and 64-row
tiles, tiles that straddle the two images), Co = 200 / 40, Ci = 6 / 32 / 48 / 64 / 72 by loader.

A1  Poison locality.  One operand element is NaN, or +Inf, at
      a  the last channel of the last pixel of image 0 (next to image 1 in memory, in a tile straddling both), Co 200
      b  channel 0 of pixel (0, 0) of image 1 (every padding tap in play), Co 40
      c  an interior pixel of image 0, channel Ci // 2, Co 200
      d  (dual / chain-dual forms) an interior pixel of image 1 of the SECOND operand, Co 40
    (Co follows the position so that both widths run without doubling the case count; the chain entries have their
    own fixed widths.)  Then ~isfinite(y) == ~isfinite(ref) elementwise -- the reference's set is exactly the poisoned
    element's receptive field, so a loader that over-read a neighbour against a zero weight (0 * NaN = NaN) or dropped
    a tap fails -- and the finite elements meet the family's float64 bar, max|ref| taken over the finite elements.
    For the exact-f32 and fp16 families also isnan(y) == isnan(ref) and every Inf has the reference's sign.
    Split-bf16 family: split3 computes h = bf16(v), r = v - h, so v = Inf gives h = Inf, r = NaN and the output is NaN
    where the reference has +-Inf.  Only the non-finite SETS are compared there, and with an Inf poison the set is that
    of the reference's pre-activation value (the receptive field): relu(-Inf) = 0 is finite in the reference, while
    the kernel's relu(NaN) stays NaN.  Non-finite in, non-finite out; never a finite wrong number.
    Where a wrapper takes out=, the buffer is filled with NaN before the call; where it may be wider than Co
    (ldy > Co) the columns past Co must still hold the prefill's bits.
A2  The other users of the ReLU epilogue (BatchNorm / GroupNorm apply; the head's ReLU is k_gn_apply, reached through
    groupnorm_apply / groupnorm_apply_half) with one NaN and one -0.0 in the input.
A3  Scale equivariance, bit for bit: y(2^a x, 2^b w, 2^(a+b) bias, 2^(a+b) res) == 2^(a+b) y(x, w, bias, res).
    Derived, not measured: scaling by a power of two commutes with every rounding while no intermediate leaves the
    normal range.  Operands have a full 24-bit significand and magnitudes in [2^-6, 2^6]; for |a|, |b| <= 30 the
    smallest non-zero split piece is >= 2^-29 2^-30, the smallest kept partial product >= 2^-95 with its lowest bit
    >= 2^-111, outputs < 2^80.  fp16 family: a, b in {-4, 0, 4} over operands pre-rounded to fp16 normals.
A4  The ends of the range: a = b = -50 / +50 (relative float64 bar), FLT_MAX through both fp32 arithmetics, fp16
    stores that overflow to Inf (not saturate) or round to 65504, fp16-subnormal operands of the fp16 MFMA kernels.
"""
import types

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_CACHE = {}
N, HO, WO = 2, 9, 15
H2, W2 = 17, 29  # the stride-2 input of a 9 x 15 output
NAN, INF = float("nan"), float("inf")
FLT_MAX = 3.4028234663852886e38
POISON = {"nan": NAN, "inf": INF}
CO_AT = {"a": 200, "b": 40, "c": 200, "d": 40}


def _cached(key, make):
    """Unpoisoned operands and packed panels are made once per entry and shared (never modified)."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _act64(z, act):
    if act == 1:
        return z.clamp_min(0)  # propagates NaN, as torch.relu does
    if act == 2:
        return z * torch.sigmoid(z)
    return z


def _rand(g, *shape):
    return torch.randn(*shape, generator=g)


def _conv64(op, w, stride=1, pad=0, dil=1, nchw=False, groups=1):
    """float64 conv of an NHWC (or NCHW) operand with OIHW weights -> NHWC, no bias."""
    xin = op.double() if nchw else _nchw(op.double())
    return _nhwc(F.conv2d(xin, w.double(), None, stride, pad, dil, groups))


def _poison(t, pos, val, nchw=False):
    """A copy of t with one element set to val at position a / b / c (d: the interior pixel of image 1)."""
    t = t.clone()
    if nchw:
        _, C, H, W = t.shape
    else:
        _, H, W, C = t.shape
    n, h, w, c = {"a": (0, H - 1, W - 1, C - 1), "b": (1, 0, 0, 0), "c": (0, H // 2, W // 2, C // 2),
                  "d": (1, H // 2, W // 2, C // 2)}[pos]
    if nchw:
        t[n, c, h, w] = val
    else:
        t[n, h, w, c] = val
    return t


def _nanbuf(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, device=DEV, dtype=dtype)


def _take(out, Co):
    """The first Co columns of a NaN-prefilled (maybe wider) output; the columns past Co still hold the prefill."""
    if out.shape[-1] > Co:
        tail = out[..., Co:].contiguous()
        bits = torch.int16 if out.dtype == torch.float16 else torch.int32
        assert torch.equal(tail.view(bits), torch.full_like(tail, NAN).view(bits)), "columns past Co written"
    return out[..., :Co].contiguous()


def _check(tag, y, z, act, family, bar=None, bound=None, inf_poison=False):
    """A1's assertions.  z: the float64 pre-activation reference, ref = act(z).  family "x6": sets only."""
    ref = _act64(z, act)
    yd = y.detach().cpu().double()
    assert yd.shape == ref.shape, (tag, yd.shape, ref.shape)
    # split-bf16 with an Inf poison: the set of the pre-activation reference (see the module docstring)
    nf = ~torch.isfinite(z) if (family == "x6" and inf_poison) else ~torch.isfinite(ref)
    got = ~torch.isfinite(yd)
    field = ~torch.isfinite(z)  # (relu(-Inf) = 0 may leave no non-finite output: a depthwise corner with negative taps)
    assert bool(field.any()) and not bool(field.all()), (tag, "the poison is not in play")
    assert torch.equal(got, nf), (tag, "non-finite set", int(got.sum()), int(nf.sum()), int((got != nf).sum()),
                                  (got != nf).nonzero()[:4].tolist())
    if family != "x6":
        assert torch.equal(torch.isnan(yd), torch.isnan(ref)), (tag, "NaN set")
        inf = torch.isinf(ref)
        assert torch.equal(yd[inf], ref[inf]), (tag, "sign of Inf")
    fin = ~nf
    err = (yd - ref).abs()[fin]
    if bound is not None:
        b = bound[fin]
        print(f"[value] {tag}: {int(nf.sum())} non-finite, max err / bound {float((err / b).max()):.3f}")
        assert bool((err <= b).all()), (tag, float((err - b).max()))
    else:
        scale = float(ref[fin].abs().max())
        print(f"[value] {tag}: {int(nf.sum())} non-finite, max err {float(err.max()):.3e} = "
              f"{float(err.max()) / scale:.2e} max|ref| (bar {bar:.0e})")
        assert float(err.max()) <= bar * scale, (tag, float(err.max()), scale)


# ======================================================================================================================
# A1: the entries.  Each takes (position, poison value, act) and returns dict(y, z, family, bar | bound).
# ======================================================================================================================
F32_LOADERS = ["generic", "fast", "fast-s2", "stem-nchw", "dual", "contig", "affine-dil2", "chscale"]


def _e_f32(loader, pos, val, act):
    """conv2d_nhwc / conv2d_dual_nhwc / conv2d_nhwc_ex on the exact-f32 panels, one operand form per loader."""
    import bev_native as nat
    Co = CO_AT[pos]
    geo = {"generic": (6, 3, 1, 1, 1), "fast": (32, 3, 1, 1, 1), "fast-s2": (32, 3, 2, 1, 1),
           "stem-nchw": (3, 7, 2, 3, 1), "dual": (32, 1, 1, 0, 1), "contig": (72, 1, 1, 0, 1),
           "affine-dil2": (32, 3, 1, 2, 2), "chscale": (32, 3, 1, 1, 1)}[loader]
    Ci, K, s, pad, dil = geo
    nchw = loader == "stem-nchw"

    def make():
        g = torch.Generator().manual_seed(4000 + 10 * F32_LOADERS.index(loader) + Co)
        c = types.SimpleNamespace()
        H, W = (H2, W2) if s == 2 else (HO, WO)
        c.x = _rand(g, N, Ci, H, W) if nchw else _rand(g, N, H, W, Ci)
        c.w = _rand(g, Co, Ci, K, K) / (Ci * K * K) ** 0.5
        c.b, c.res = _rand(g, Co) * 0.1, _rand(g, N, HO, WO, Co)
        c.bd, c.rd = c.b.to(DEV), c.res.to(DEV)
        wd = c.w.to(DEV)
        if loader == "dual":
            c.x2, c.w2 = _rand(g, N, H2, W2, 64), _rand(g, Co, 64, 1, 1) / 8
            wd = torch.cat([c.w, c.w2], 1).contiguous().to(DEV)
        if loader == "affine-dil2":  # a positive scale, so that an Inf poison reaches the operand ReLU as +Inf
            c.sc, c.sh = torch.rand(N, Ci, generator=g) + 0.5, _rand(g, N, Ci) * 0.5
            c.scd, c.shd = c.sc.to(DEV), c.sh.to(DEV)
        if loader == "chscale":
            c.gate = torch.rand(N, Ci, generator=g) + 0.25
            c.gd = c.gate.to(DEV)
        c.p = nat.pack_conv_weight(wd)
        return c
    c = _cached(("f32", loader, Co), make)
    x = c.x if pos == "d" else _poison(c.x, pos, val, nchw)
    xd = x.to(DEV)
    if loader == "dual":
        x2 = _poison(c.x2, "d", val) if pos == "d" else c.x2
        z = _conv64(x, c.w) + _conv64(x2, c.w2, 2) + c.b.double()
        y = nat.conv2d_dual_nhwc(xd, x2.to(DEV), 2, c.p, c.bd, Co, relu=act, out=_nanbuf(N, HO, WO, Co))
    elif loader == "affine-dil2":  # the operand the loader forms: relu(x scale + shift), fp32 multiply then add
        op = (x * c.sc[:, None, None, :] + c.sh[:, None, None, :]).clamp_min(0)
        z = _conv64(op, c.w, 1, pad, dil) + c.b.double()
        out = _nanbuf(N, HO, WO, Co + 8)
        nat.conv2d_nhwc_ex(xd, c.p, c.bd, Co, K, pad, dil, in_scale=c.scd, in_shift=c.shd, in_relu=True, out=out,
                           relu=bool(act))
        y = _take(out, Co)
    elif loader == "stem-nchw":  # Co 40: k_stem (slot 147 re-reads tap 146 against a zero weight); 200: LOADER 2
        z = _conv64(x, c.w, s, pad, nchw=True) + c.b.double()
        y = nat.conv2d_nhwc(xd, c.p, c.bd, Co, K, K, s, pad, act, in_nchw=True, out=_nanbuf(N, HO, WO, Co))
    else:
        op = x * c.gate[:, None, None, :] if loader == "chscale" else x
        z = _conv64(op, c.w, s, pad) + c.b.double() + c.res.double()
        y = nat.conv2d_nhwc(xd, c.p, c.bd, Co, K, K, s, pad, act, residual=c.rd, out=_nanbuf(N, HO, WO, Co),
                            ascale=c.gd if loader == "chscale" else None)
    return dict(y=y, z=z, family="f32", bar=1e-5)


def _e_x6(form, pos, val, act):
    """conv2d_nhwc_x6 with an fp32 operand (Ci 48: 16-deep steps; bias + residual, dense out) and with a pre-split
    operand (Ci 64; bias, ldy = Co + 8); conv2d_dual_nhwc under the split arithmetic."""
    import bev_native as nat
    Co = CO_AT[pos]
    Ci = {"fp32": 48, "split": 64, "dual": 32}[form]
    K = 1 if form == "dual" else 3

    def make():
        g = torch.Generator().manual_seed(4200 + Ci + Co)
        c = types.SimpleNamespace()
        c.x, c.w = _rand(g, N, HO, WO, Ci), _rand(g, Co, Ci, K, K) / (Ci * K * K) ** 0.5
        c.b, c.res = _rand(g, Co) * 0.1, _rand(g, N, HO, WO, Co)
        c.bd, c.rd = c.b.to(DEV), c.res.to(DEV)
        wd = c.w.to(DEV)
        if form == "dual":
            c.x2, c.w2 = _rand(g, N, H2, W2, 64), _rand(g, Co, 64, 1, 1) / 8
            wd = torch.cat([c.w, c.w2], 1).contiguous().to(DEV)
        c.p = nat.pack_conv_weight_x6(wd)
        return c
    c = _cached(("x6", form, Co), make)
    x = c.x if pos == "d" else _poison(c.x, pos, val)
    xd = x.to(DEV)
    if form == "dual":
        x2 = _poison(c.x2, "d", val) if pos == "d" else c.x2
        z = _conv64(x, c.w) + _conv64(x2, c.w2, 2) + c.b.double()
        y = nat.conv2d_dual_nhwc(xd, x2.to(DEV), 2, c.p, c.bd, Co, relu=act, out=_nanbuf(N, HO, WO, Co))
    elif form == "split":
        z = _conv64(x, c.w, 1, 1) + c.b.double()
        out = _nanbuf(N, HO, WO, Co + 8)
        nat.conv2d_nhwc_x6(nat.split3(xd), c.p, c.bd, Co, 3, 3, 1, 1, 1, act, out=out)
        y = _take(out, Co)
    else:
        z = _conv64(x, c.w, 1, 1) + c.b.double() + c.res.double()
        y = nat.conv2d_nhwc_x6(xd, c.p, c.bd, Co, 3, 3, 1, 1, 1, act, residual=c.rd, out=_nanbuf(N, HO, WO, Co))
    return dict(y=y, z=z, family="x6", bar=1e-5)


def _e_chain(arith, dual, pos, val, act):
    """conv2d_chain_nhwc (3x3 Ci 32 -> 64, ReLU, 1x1 -> 128 + residual) and conv2d_chain_dual_nhwc (conv3's K
    continued over a 64-channel second operand), exact-f32 and split-bf16 panels; `act` is the outer activation."""
    import bev_native as nat
    Ci, Cm, Co2 = 32, 64, 128

    def make():
        g = torch.Generator().manual_seed(4300 + int(dual))
        c = types.SimpleNamespace()
        c.x, c.w1, c.b1 = _rand(g, N, HO, WO, Ci), _rand(g, Cm, Ci, 3, 3) / (Ci * 9) ** 0.5, _rand(g, Cm) * 0.1
        K2 = Cm + (64 if dual else 0)
        c.w2, c.b2 = _rand(g, Co2, K2, 1, 1) / K2 ** 0.5, _rand(g, Co2) * 0.1
        c.res, c.x2 = _rand(g, N, HO, WO, Co2), _rand(g, N, HO, WO, 64)
        pack = nat.pack_conv_weight if arith == "f32" else nat.pack_conv_weight_x6
        c.p1, c.p2 = pack(c.w1.to(DEV)), pack(c.w2.to(DEV))
        c.b1d, c.b2d, c.rd = c.b1.to(DEV), c.b2.to(DEV), c.res.to(DEV)
        return c
    c = _cached(("chain", arith, dual), make)
    x = c.x if pos == "d" else _poison(c.x, pos, val)
    h = _act64(_conv64(x, c.w1, 1, 1) + c.b1.double(), 1)
    if dual:
        x2 = _poison(c.x2, "d", val) if pos == "d" else c.x2
        z = _conv64(torch.cat([h, x2.double()], 3), c.w2) + c.b2.double()
        y = nat.conv2d_chain_dual_nhwc(x.to(DEV), c.p1, c.b1d, Cm, 3, 3, 1, 1, 1, x2.to(DEV), 1, c.p2, c.b2d, Co2, act,
                                       out=_nanbuf(N, HO, WO, Co2))
    else:
        z = _conv64(h, c.w2) + c.b2.double() + c.res.double()
        y = nat.conv2d_chain_nhwc(x.to(DEV), c.p1, c.b1d, Cm, 3, 3, 1, 1, 1, c.p2, c.b2d, Co2, act, residual=c.rd,
                                  out=_nanbuf(N, HO, WO, Co2))
    return dict(y=y, z=z, family=arith, bar=1e-5)


def _stem_ops(Co, W=W2):
    import bev_native as nat

    def make():
        g = torch.Generator().manual_seed(4400 + Co + W)
        c = types.SimpleNamespace()
        c.x, c.w, c.b = _rand(g, N, 3, H2, W), _rand(g, Co, 3, 7, 7) / 147 ** 0.5, _rand(g, Co) * 0.1
        c.p, c.bd = nat.pack_conv_weight_x6(c.w.to(DEV)), c.b.to(DEV)
        return c
    return _cached(("stem-x6", Co, W), make)


def _e_stem_x6(pos, val, act):
    """conv2d_stem_x6 (7x7 / s2 / p3 over NCHW; stem6::koff sends k >= 147 to tap 0 against a zero weight)."""
    import bev_native as nat
    Co = {"a": 64, "b": 40, "c": 64}[pos]
    c = _stem_ops(Co)
    x = _poison(c.x, pos, val, nchw=True)
    z = _conv64(x, c.w, 2, 3, nchw=True) + c.b.double()
    y = nat.conv2d_stem_x6(x.to(DEV), c.p, c.bd, Co, bool(act), out=_nanbuf(N, HO, WO, Co))
    return dict(y=y, z=z, family="x6", bar=1e-5)


def _h16_bound(z_mag, ref, Kt, y_half):
    """The fp16 family's per-element bounds (test_conv_h16_gpu.py / test_conv_h16_half_gpu.py), ReLU or no act."""
    if y_half:
        return 2.0 ** -11 * ref.abs() + (Kt + 2) * 2.0 ** -24 * z_mag + 2.0 ** -24
    return Kt * 2.0 ** -24 * z_mag + 1e-6


def _e_h16(entry, pos, val, act):
    """conv2d_nhwc_h16 (fp32 x, Ci 32, fp32 out: + residual dense, or ldy = Co + 8 at position b), conv2d_h16_half
    (fp16 x, Ci 64, fp16 residual and output), conv2d_h16_affine (fp16 x, GroupNorm affine + ReLU in the loader; fp32
    output at ldy = Co + 8, fp16 output at position b)."""
    import bev_native as nat
    Co = CO_AT[pos]
    Ci = 32 if entry == "f32out" else 64
    Kt = Ci * 9

    def make():
        g = torch.Generator().manual_seed(4500 + Ci + Co + len(entry))
        c = types.SimpleNamespace()
        c.x, c.w = _rand(g, N, HO, WO, Ci), _rand(g, Co, Ci, 3, 3) / Kt ** 0.5
        c.b, c.res = _rand(g, Co), _rand(g, N, HO, WO, Co).half()
        c.sc, c.sh = torch.rand(N, Ci, generator=g) + 0.5, _rand(g, N, Ci) * 0.5
        c.p, c.bd = nat.pack_conv_weight_h16(c.w.to(DEV)), c.b.to(DEV)
        c.r16, c.r32, c.scd, c.shd = c.res.to(DEV), c.res.float().to(DEV), c.sc.to(DEV), c.sh.to(DEV)
        return c
    c = _cached(("h16", entry, Co), make)
    x = _poison(c.x, pos, val)
    x16 = x.half()
    op = x16
    if entry == "affine":  # f16(max(float(f16 x) scale + shift, 0)): fp32 multiply, fp32 add
        op = (x16.float() * c.sc[:, None, None, :] + c.sh[:, None, None, :]).clamp_min(0).half()
    w64 = c.w.half().double()
    z, mag = _conv64(op, w64, 1, 1) + c.b.double(), _conv64(op.abs(), w64.abs(), 1, 1) + c.b.double().abs()
    with_res = entry == "f16out" or (entry == "f32out" and pos != "b")
    if with_res:
        z, mag = z + c.res.double(), mag + c.res.double().abs()
    if entry == "f32out":
        if with_res:
            y = nat.conv2d_nhwc_h16(x.to(DEV), c.p, c.bd, Co, 3, 3, 1, 1, 1, act, residual=c.r32,
                                    out=_nanbuf(N, HO, WO, Co))
        else:
            y = _take(nat.conv2d_nhwc_h16(x.to(DEV), c.p, c.bd, Co, 3, 3, 1, 1, 1, act,
                                          out=_nanbuf(N, HO, WO, Co + 8)), Co)
        y_half = False
    elif entry == "f16out":
        y = nat.conv2d_h16_half(x16.to(DEV), c.p, c.bd, Co, 3, 3, 1, 1, 1, act, residual=c.r16,
                                out=_nanbuf(N, HO, WO, Co, dtype=torch.float16))
        y_half = True
    else:
        y_half = pos == "b"
        out = _nanbuf(N, HO, WO, Co, dtype=torch.float16) if y_half else _nanbuf(N, HO, WO, Co + 8)
        y = _take(nat.conv2d_h16_affine(x16.to(DEV), c.p, c.bd, Co, 3, 1, 1, in_scale=c.scd, in_shift=c.shd,
                                        in_relu=True, y_half=y_half, out=out, act=act), Co)
    return dict(y=y, z=z, family="h16", bound=_h16_bound(mag, _act64(z, act), Kt, y_half))


def _e_stem3(half, pos, val, act):
    """conv2d_stem3 / conv2d_stem3_h16 (3x3 / s2 / p1 over NCHW, Co 40)."""
    import bev_native as nat
    Co = 40

    def make():
        g = torch.Generator().manual_seed(4600)
        c = types.SimpleNamespace()
        c.x, c.w, c.b = _rand(g, N, 3, H2, W2), _rand(g, Co, 3, 3, 3) / 27 ** 0.5, _rand(g, Co) * 0.1
        c.wt, c.bd = c.w.permute(1, 2, 3, 0).reshape(27, Co).contiguous().to(DEV), c.b.to(DEV)
        return c
    c = _cached("stem3", make)
    x = _poison(c.x, pos, val, nchw=True)
    z = _conv64(x, c.w, 2, 1, nchw=True) + c.b.double()
    y = (nat.conv2d_stem3_h16 if half else nat.conv2d_stem3)(x.to(DEV), c.wt, c.bd, act)
    if not half:
        return dict(y=y, z=z, family="f32", bar=2e-6)  # test_effnet.py's bar for k_stem3
    ref = _act64(z, act)
    fin = torch.isfinite(ref)
    bound = 2.0 ** -11 * ref.abs() + 2.0 ** -25 + 2e-6 * float(ref[fin].abs().max())  # the same, rounded once to fp16
    return dict(y=y, z=z, family="h16", bound=bound)


DW_GEO = {3: (1, HO, WO), 5: (2, H2, W2)}  # K -> stride, input size


def _e_dw(half, K, pos, val, act):
    """dwconv2d_nhwc / dwconv2d_nhwc_h16: K = 3 at stride 1, K = 5 at stride 2, C = 48."""
    import bev_native as nat
    C = 48
    S, H, W = DW_GEO[K]

    def make():
        g = torch.Generator().manual_seed(4700 + K)
        c = types.SimpleNamespace()
        c.x, c.w, c.b = _rand(g, N, H, W, C), _rand(g, C, 1, K, K) * 0.3, _rand(g, C) * 0.1
        c.wt, c.bd = c.w.reshape(C, K * K).t().contiguous().to(DEV), c.b.to(DEV)
        return c
    c = _cached(("dw", K), make)
    x = _poison(c.x, pos, val)
    if not half:
        z = _conv64(x, c.w, S, K // 2, groups=C) + c.b.double()
        y, _ = nat.dwconv2d_nhwc(x.to(DEV), c.wt, c.bd, K, S, K // 2, act)
        return dict(y=y, z=z, family="f32", bar=1e-5)
    x16, w64 = x.half(), c.w.half().double()
    z = _conv64(x16, w64, S, K // 2, groups=C) + c.b.double()
    mag = _conv64(x16.abs(), w64.abs(), S, K // 2, groups=C) + c.b.double().abs()
    y, _ = nat.dwconv2d_nhwc_h16(x16.to(DEV), c.wt.half(), c.bd, K, S, K // 2, act)
    return dict(y=y, z=z, family="h16", bound=_h16_bound(mag, _act64(z, act), K * K, True))


def _silu64(z):
    return z * torch.sigmoid(z)


def _e_ir(half, K, pos, val):
    """ir_expand_dw / ir_expand_dw_h16 at the smallest legal Cin and one 48-channel group: 1x1 16 -> 48, SiLU,
    depthwise K (3 at stride 1, 5 at stride 2), SiLU.  -> (y, float64 forward, float64 forward with the fp16 kernel's
    rounding points or None)."""
    import bev_native as nat
    Ci, Cm = 16, 48
    S, H, W = DW_GEO[K]

    def make():
        g = torch.Generator().manual_seed(4800 + K)
        c = types.SimpleNamespace()
        c.x = _rand(g, N, H, W, Ci)
        c.we, c.be = _rand(g, Cm, Ci) / Ci ** 0.5, 0.2 * _rand(g, Cm)
        c.wd, c.bd = 0.3 * _rand(g, K * K, Cm), 0.2 * _rand(g, Cm)
        c.dev = [t.to(DEV) for t in (c.we, c.be, c.wd, c.bd)]
        return c
    c = _cached(("ir", K), make)
    x = _poison(c.x, pos, val)
    if half:
        x = x.half()

    def fwd(rounded):
        r = (lambda t: t.half().double()) if rounded else (lambda t: t.double())
        h = r(_silu64(_conv64(x, r(c.we).view(Cm, Ci, 1, 1)) + c.be.double()))
        return r(_silu64(_conv64(h, r(c.wd).t().reshape(Cm, 1, K, K), S, K // 2, groups=Cm) + c.bd.double()))
    we, be, wd, bd = c.dev
    if not half:
        y, _ = nat.ir_expand_dw(x.to(DEV), we, be, wd, bd, K, S)
        return y, fwd(False), None
    y, _ = nat.ir_expand_dw_h16(x.to(DEV), we.half(), be, wd.half(), bd, K, S)
    return y, fwd(False), fwd(True)


def _e_pw(pos, val):
    """conv2d_pw_h16: Ci 40 (the operand's pieces past Ci are zero), gate, fp16 residual; fp32 output at ldy = Co + 8
    (positions a, c), fp16 output dense (b)."""
    import bev_native as nat
    Co, Ci = CO_AT[pos], 40
    f32 = pos != "b"

    def make():
        g = torch.Generator().manual_seed(4900 + Co)
        c = types.SimpleNamespace()
        c.x, c.gate = _rand(g, N, HO, WO, Ci).half(), torch.sigmoid(_rand(g, N, Ci))
        c.w, c.b, c.res = (_rand(g, Co, Ci) / Ci ** 0.5).half(), _rand(g, Co), _rand(g, N, HO, WO, Co).half()
        c.dev = [t.to(DEV) for t in (c.w, c.b, c.gate, c.res)]
        return c
    c = _cached(("pw", Co), make)
    x = _poison(c.x, pos, val)
    a16 = (x.float() * c.gate.view(N, 1, 1, Ci)).half()  # the kernel's own operation
    z = a16.double() @ c.w.double().t() + c.b.double() + c.res.double()
    mag = a16.double().abs() @ c.w.double().abs().t() + c.b.double().abs() + c.res.double().abs()
    w, b, gate, res = c.dev
    out = _nanbuf(N, HO, WO, Co + 8) if f32 else _nanbuf(N, HO, WO, Co, dtype=torch.float16)
    y = _take(nat.conv2d_pw_h16(x.to(DEV), w, b, gate=gate, residual=res, f32_out=f32, out=out), Co)
    bound = (Ci + 2) * 2.0 ** -24 * mag + 2.0 ** -24
    return dict(y=y, z=z, family="h16", bound=bound if f32 else bound + 2.0 ** -11 * z.abs())


ENTRIES = {}
for _l in F32_LOADERS:
    ENTRIES["f32-" + _l] = (lambda pos, val, act, _l=_l: _e_f32(_l, pos, val, act), "abcd" if _l == "dual" else "abc")
for _f in ("fp32", "split", "dual"):
    ENTRIES["x6-" + _f] = (lambda pos, val, act, _f=_f: _e_x6(_f, pos, val, act), "abcd" if _f == "dual" else "abc")
for _a in ("f32", "x6"):
    ENTRIES[f"chain-{_a}"] = (lambda pos, val, act, _a=_a: _e_chain(_a, False, pos, val, act), "abc")
    ENTRIES[f"chain-dual-{_a}"] = (lambda pos, val, act, _a=_a: _e_chain(_a, True, pos, val, act), "abcd")
ENTRIES["stem-x6"] = (_e_stem_x6, "abc")
for _e in ("f32out", "f16out", "affine"):
    ENTRIES["h16-" + _e] = (lambda pos, val, act, _e=_e: _e_h16(_e, pos, val, act), "abc")
for _h in (False, True):
    _s = "-h16" if _h else ""
    ENTRIES["stem3" + _s] = (lambda pos, val, act, _h=_h: _e_stem3(_h, pos, val, act), "abc")
    for _k in (3, 5):
        ENTRIES[f"dw{_k}{_s}"] = (lambda pos, val, act, _h=_h, _k=_k: _e_dw(_h, _k, pos, val, act), "abc")
A1_CASES = [(name, pos, poison, act) for name, (_, where) in ENTRIES.items() for pos in where
            for poison in ("nan", "inf") for act in (0, 1)]


@pytest.mark.parametrize("name,pos,poison,act", A1_CASES,
                         ids=[f"{n}-{p}-{v}-{'relu' if a else 'none'}" for n, p, v, a in A1_CASES])
def test_poison_locality(name, pos, poison, act, request):
    r = ENTRIES[name][0](pos, POISON[poison], act)
    torch.cuda.synchronize()
    _check(request.node.callspec.id, r["y"], r["z"], act, r["family"], r.get("bar"), r.get("bound"), poison == "inf")


@pytest.mark.parametrize("poison", ["nan", "inf"])
@pytest.mark.parametrize("pos", ["a", "b", "c"])
def test_poison_locality_pw_h16(pos, poison, request):
    """conv2d_pw_h16 has no activation."""
    r = _e_pw(pos, POISON[poison])
    torch.cuda.synchronize()
    _check(request.node.callspec.id, r["y"], r["z"], 0, "h16", bound=r["bound"])


@pytest.mark.parametrize("poison", ["nan", "inf"])
@pytest.mark.parametrize("pos", ["a", "b", "c"])
@pytest.mark.parametrize("K", [3, 5])
@pytest.mark.parametrize("half", [False, True], ids=["f32", "h16"])
def test_poison_locality_ir_expand_dw(half, K, pos, poison, request):
    """The fused expansion + depthwise (SiLU twice, no ReLU): the poisoned pixel's 48 expanded channels are non-finite,
    so is the depthwise window around it and nothing else.  Finite elements: fp32 1e-5 max|ref|
    (test_kernel_instances_gpu.py); fp16 the bars of test_effnet_h16_kernels_gpu.py (relative L2 <= 1.5 x, max error
    <= 2 x those of the float64 forward with the kernel's rounding points, <= 1 % of the elements off its rounding)."""
    tag = request.node.callspec.id
    y, exact, r64 = _e_ir(half, K, pos, POISON[poison])
    torch.cuda.synchronize()
    yd = y.cpu().double()
    nf = ~torch.isfinite(exact)
    assert bool(nf.any()) and not bool(nf.all())
    assert torch.equal(~torch.isfinite(yd), nf), (tag, int((~torch.isfinite(yd)).sum()), int(nf.sum()))
    assert torch.equal(torch.isnan(yd), torch.isnan(exact)), tag
    assert torch.equal(yd[torch.isinf(exact)], exact[torch.isinf(exact)]), tag
    fin = ~nf
    if not half:
        err, scale = float((yd - exact)[fin].abs().max()), float(exact[fin].abs().max())
        print(f"[value] {tag}: {int(nf.sum())} non-finite, max err {err / scale:.2e} max|ref|")
        assert err <= 1e-5 * scale, (tag, err, scale)
        return
    assert torch.equal(~torch.isfinite(r64), nf), tag  # the rounded restatement has the same set
    e, r, g = exact[fin], r64[fin], yd[fin]
    l2 = float((g - e).norm() / (r - e).norm())
    mx = float((g - e).abs().max() / (r - e).abs().max())
    off = float((y.cpu()[fin] != r64.half()[fin]).double().mean())
    print(f"[value] {tag}: {int(nf.sum())} non-finite, L2 ratio {l2:.3f} max ratio {mx:.3f} off {100 * off:.3f} %")
    assert l2 <= 1.5 and mx <= 2.0 and off <= 0.01, (tag, l2, mx, off)


@pytest.mark.parametrize("poison", ["nan", "inf"])
@pytest.mark.parametrize("pos", ["a", "b", "c", "seam"])
def test_stem_pool_x6_poison_equals_stem_then_maxpool(pos, poison):
    """conv2d_stem_pool_x6 == maxpool_nhwc(conv2d_stem_x6(relu)) bit for bit on poisoned images (NaN masks equal, the
    rest equal under nan_to_num, as test_backbone_gpu.py compares max-pools), and its NaN set is that of float64
    max_pool2d(relu(conv)), which propagates NaN.  17 x 131 images: 9 x 66 stem outputs = 2 x 2 tiles of 8 x 64, so
    the pooled seam row, seam column and their corner exist; `seam` poisons input (15, 127), whose receptive field
    (stem rows 6..8, columns 62..65) covers all four tiles."""
    import bev_native as nat
    c = _stem_ops(64, 131)
    val = POISON[poison]
    x = _poison(c.x, pos, val, nchw=True) if pos != "seam" else c.x.clone()
    if pos == "seam":
        x[1, 1, 15, 127] = val
    xd = x.to(DEV)
    got = nat.conv2d_stem_pool_x6(xd, c.p, c.bd, 64)
    two = nat.maxpool_nhwc(nat.conv2d_stem_x6(xd, c.p, c.bd, 64, True), 3, 2, 1)
    torch.cuda.synchronize()
    assert torch.equal(torch.isnan(got), torch.isnan(two)), (int(torch.isnan(got).sum()), int(torch.isnan(two).sum()))
    assert torch.equal(torch.nan_to_num(got), torch.nan_to_num(two))
    z = _conv64(x, c.w, 2, 3, nchw=True) + c.b.double()
    # split-bf16: an Inf operand comes out as NaN, so the set is the pooled receptive field (pre-activation non-finite)
    field = F.max_pool2d(_nchw((~torch.isfinite(z)).double()), 3, 2, 1) > 0
    ref = _nhwc(F.max_pool2d(_nchw(_act64(z, 1)), 3, 2, 1))
    nf = _nhwc(field)
    assert bool(nf.any()) and torch.equal(~torch.isfinite(got.cpu()), nf)
    if poison == "nan":
        assert torch.equal(nf, torch.isnan(ref))
    fin = ~nf
    err = (got.cpu().double() - ref)[fin].abs().max()
    assert float(err) <= 1e-5 * float(ref[fin].abs().max())


@pytest.mark.parametrize("family", ["f32", "x6", "h16"])
def test_weight_poison_one_output_column(family):
    """One NaN weight of a 1x1 / pad 0 conv: exactly output column co is NaN, every other column meets the bar."""
    import bev_native as nat
    Ci, Co, co = 64, 40, 17
    g = torch.Generator().manual_seed(5000)
    x, w, b = _rand(g, N, HO, WO, Ci), _rand(g, Co, Ci, 1, 1) / 8, _rand(g, Co) * 0.1
    w[co, 5] = NAN
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    if family == "f32":
        y = nat.conv2d_nhwc(xd, nat.pack_conv_weight(wd), bd, Co, 1, 1, 1, 0, 0)
        z = _conv64(x, w) + b.double()
    elif family == "x6":
        y = nat.conv2d_nhwc_x6(xd, nat.pack_conv_weight_x6(wd), bd, Co, 1, 1, 1, 0, 1, 0)
        z = _conv64(x, w) + b.double()
    else:
        y = nat.conv2d_nhwc_h16(xd, nat.pack_conv_weight_h16(wd), bd, Co, 1, 1, 1, 0, 1, 0)
        z = _conv64(x.half(), w.half()) + b.double()
    torch.cuda.synchronize()
    col = torch.zeros(N, HO, WO, Co, dtype=torch.bool)
    col[..., co] = True
    assert torch.equal(torch.isnan(z), col)
    yd = y.cpu().double()
    assert torch.equal(torch.isnan(yd), col) and torch.equal(~torch.isfinite(yd), col)
    err, scale = float((yd - z)[~col].abs().max()), float(z[~col].abs().max())
    if family == "h16":
        mag = _conv64(x.half().abs(), torch.nan_to_num(w).half().abs()) + b.double().abs()
        assert bool(((yd - z).abs()[~col] <= (Ci * 2.0 ** -24 * mag + 1e-6)[~col]).all())
    else:
        assert err <= 1e-5 * scale, (err, scale)


# ======================================================================================================================
# A2: BatchNorm / GroupNorm apply with ReLU: a NaN stays a NaN, -0 behaves as 0
# ======================================================================================================================
def _norm_input(C, per_image):
    """z [2, 9, 15, C] with one NaN and one -0.0; scale / shift [C] (or [2, C]); the -0.0 element's channel has shift
    -0.0, so that the value reaching the ReLU is -0 (-0 scale + -0)."""
    g = torch.Generator().manual_seed(5100 + C)
    z = _rand(g, N, HO, WO, C)
    lead = (N, C) if per_image else (C,)
    scale, shift = torch.rand(*lead, generator=g) + 0.5, _rand(g, *lead) * 0.5
    shift[..., 3] = -0.0
    z[0, HO - 1, WO - 1, C - 1] = NAN
    z[1, 4, 7, 3] = -0.0
    bc = (lambda t: t[:, None, None, :]) if per_image else (lambda t: t)
    pre = z.double() * bc(scale).double() + bc(shift).double()
    return z, scale, shift, pre


def _norm_check(tag, y, ref, half, rtol, atol_frac):
    yd = y.cpu().double()
    nan = torch.isnan(ref)
    assert int(nan.sum()) == 1 and torch.equal(torch.isnan(yd), nan), (tag, int(torch.isnan(yd).sum()))
    assert torch.equal(~torch.isfinite(yd), nan), tag
    fin = ~nan
    scale = float(ref[fin].abs().max())
    bound = rtol * ref.abs() + atol_frac * scale + (2.0 ** -11 * ref.abs() + 2.0 ** -25 if half else 0.0)
    err = (yd - ref).abs()
    print(f"[value] {tag}: max err / bound {float((err[fin] / bound[fin]).max()):.3f}")
    assert bool((err[fin] <= bound[fin]).all()), (tag, float((err - bound)[fin].max()))
    assert float(yd[1, 4, 7, 3]) == 0.0, tag


BN_CASES = [("apply", 64), ("apply", 24), ("apply_half", 64), ("apply_half", 24), ("apply_mask", 64)]


@pytest.mark.parametrize("entry,C", BN_CASES,
                         ids=[f"{e}-{'row-block' if c == 64 else 'flat'}-c{c}" for e, c in BN_CASES])
def test_batchnorm_apply_relu_keeps_nan(entry, C):
    """batchnorm_apply(act = 1, with a residual), batchnorm_apply_half, batchnorm_apply_mask on k_bn_apply_q (C 64) and
    the flat k_bn_apply (C 24; the mask form has the row-block kernel only): NaN mask equal to float64 torch's, finite
    elements within test_kernel_instances_gpu.py's bars (fp32: 1e-5 max|ref|; fp16: 2^-11 |ref| + 2^-25 + 1e-5
    max|ref|).  The mask byte's bit of the NaN element stays "not positive", so the backward sends 0 there."""
    import bev_native as nat
    z, scale, shift, pre = _norm_input(C, False)
    zd, sd, hd = z.to(DEV), scale.to(DEV), shift.to(DEV)
    if entry == "apply":
        res = _rand(torch.Generator().manual_seed(C), N, HO, WO, C)
        res[1, 4, 7, 3] = -0.0  # the value reaching the ReLU stays -0
        y, ref = nat.batchnorm_apply(zd, sd, hd, residual=res.to(DEV), act=1), (pre + res.double()).clamp_min(0)
    elif entry == "apply_half":
        y, ref = nat.batchnorm_apply_half(zd, sd, hd, act=1), pre.clamp_min(0)
    else:
        (y, mask), ref = nat.batchnorm_apply_mask(zd, sd, hd), pre.clamp_min(0)
    torch.cuda.synchronize()
    _norm_check(f"batchnorm_{entry}-c{C}", y, ref, entry == "apply_half", 0.0, 1e-5)
    if entry == "apply_mask":
        bits = ((mask.cpu().int()[:, None] >> torch.arange(4)) & 1).bool().reshape(N, HO, WO, C)
        assert torch.equal(bits, y.cpu() > 0)  # NaN > 0 is false: the NaN element's bit is 0
        assert not bool(bits[0, HO - 1, WO - 1, C - 1])


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_groupnorm_apply_relu_keeps_nan(half):
    """groupnorm_apply(relu=True) / groupnorm_apply_half: k_gn_apply, the BEV head's ReLU.  Bars of test_head_gpu.py
    (|err| <= 1e-4 |ref| + 1e-5 max|ref|), for the fp16 store plus its rounding 2^-11 |ref| + 2^-25."""
    import bev_native as nat
    z, scale, shift, pre = _norm_input(64, True)
    fn = nat.groupnorm_apply_half if half else nat.groupnorm_apply
    y = fn(z.to(DEV), scale.to(DEV), shift.to(DEV), True)
    torch.cuda.synchronize()
    _norm_check(f"groupnorm_apply{'_half' if half else ''}", y, pre.clamp_min(0), half, 1e-4, 1e-5)


# ======================================================================================================================
# A3 / A4: scale equivariance and the ends of the range
# ======================================================================================================================
def _wide(g, *shape, fp16=False):
    """Random sign, magnitude log-uniform in [2^-6, 2^6), a full 24-bit (fp16: 11-bit) significand."""
    bits = 10 if fp16 else 23
    mant = 1.0 + torch.randint(0, 2 ** bits, shape, generator=g).double() / 2 ** bits
    expo = torch.randint(-6, 6, shape, generator=g).double()
    sign = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    v = (sign * mant * 2.0 ** expo).float()
    assert torch.equal(v.double(), sign * mant * 2.0 ** expo)
    return v


EQ_FAMILIES = ["f32", "x6", "x6-dual", "chain-f32", "chain-x6", "stem-x6", "h16"]


def _eq_ops(family):
    """-> (run(a, b, act) -> y on the device, ref(act) -> float64 reference at a = b = 0)."""
    import bev_native as nat

    def make():
        g = torch.Generator().manual_seed(5200 + EQ_FAMILIES.index(family))
        h16 = family == "h16"
        Co = 64 if family == "stem-x6" else 128 if family.startswith("chain") else 40
        if family == "stem-x6":
            x, w = _wide(g, N, 3, H2, W2), _wide(g, Co, 3, 7, 7)
        else:
            x, w = _wide(g, N, HO, WO, 32, fp16=h16), _wide(g, 64 if family.startswith("chain") else Co, 32, 3, 3,
                                                            fp16=h16)
        b, res = _wide(g, Co), _wide(g, N, HO, WO, Co)
        x2, w2 = _wide(g, N, H2, W2, 64), _wide(g, Co, 64, 1, 1)           # x6-dual's second operand
        b1, w3 = _wide(g, 64), _wide(g, Co, 64, 1, 1)                      # the chain's inner bias and conv3
        if family == "x6-dual":
            w = _wide(g, Co, 32, 1, 1)
        pack = {"f32": nat.pack_conv_weight, "chain-f32": nat.pack_conv_weight, "h16": nat.pack_conv_weight_h16}.get(
            family, nat.pack_conv_weight_x6)
        p3 = pack(w3.to(DEV)) if family.startswith("chain") else None
        dev = {k: v.to(DEV) for k, v in dict(x=x, w=w, b=b, res=res, x2=x2, w2=w2, b1=b1).items()}

        def run(a, bb, act):
            sx, sw, sy = 2.0 ** a, 2.0 ** bb, 2.0 ** (a + bb)
            xd, bd, rd = dev["x"] * sx, dev["b"] * sy, dev["res"] * sy
            if family == "x6-dual":
                p = pack(torch.cat([dev["w"], dev["w2"]], 1).contiguous() * sw)
                return nat.conv2d_dual_nhwc(xd, dev["x2"] * sx, 2, p, bd, Co, relu=act)
            p = pack(dev["w"] * sw)
            if family == "f32":
                return nat.conv2d_nhwc(xd, p, bd, Co, 3, 3, 1, 1, act, residual=rd)
            if family == "x6":
                return nat.conv2d_nhwc_x6(xd, p, bd, Co, 3, 3, 1, 1, 1, act, residual=rd)
            if family == "h16":
                return nat.conv2d_nhwc_h16(xd, p, bd, Co, 3, 3, 1, 1, 1, act, residual=rd)
            if family == "stem-x6":
                return nat.conv2d_stem_x6(xd, p, bd, Co, bool(act))
            return nat.conv2d_chain_nhwc(xd, p, dev["b1"] * sy, 64, 3, 3, 1, 1, 1, p3, bd, Co, act, residual=rd)

        def ref(act):
            if family == "x6-dual":
                return _act64(_conv64(x, w) + _conv64(x2, w2, 2) + b.double(), act)
            if family == "stem-x6":
                return _act64(_conv64(x, w, 2, 3, nchw=True) + b.double(), act)
            if family.startswith("chain"):
                h = _act64(_conv64(x, w, 1, 1) + b1.double(), 1)
                return _act64(_conv64(h, w3) + b.double() + res.double(), act)
            return _act64(_conv64(x, w, 1, 1) + b.double() + res.double(), act)
        mag = _conv64(x.abs(), w.abs(), 1, 1) + b.double().abs() + res.double().abs() if h16 else None
        return run, ref, mag
    return _cached(("eq", family), make)


@pytest.mark.parametrize("act", [0, 1], ids=["none", "relu"])
@pytest.mark.parametrize("family", EQ_FAMILIES)
def test_scale_equivariance_bit_for_bit(family, act):
    """y(2^a x, 2^b w, 2^(a+b) bias, 2^(a+b) res) == 2^(a+b) y(x, w, bias, res) under torch.equal for the nine (a, b)
    of {-30, 0, 30}^2 ({-4, 0, 4}^2 for the fp16 kernel, operands fp16 normals), and y at a = b = 0 meets the family's
    float64 bar.  (The chain scales conv2's operands and inner bias; conv3's weights stay, its bias and the residual
    scale with the output.  The stem entry has no residual.)"""
    run, ref, mag = _eq_ops(family)
    steps = (-4, 0, 4) if family == "h16" else (-30, 0, 30)
    y0 = run(0, 0, act)
    r = ref(act)
    err = (y0.cpu().double() - r).abs()
    assert bool(torch.isfinite(y0).all())
    if family == "h16":
        assert bool((err <= 288 * 2.0 ** -24 * mag + 1e-6).all()), float(err.max())
    else:
        print(f"[value] scale {family}: max err {float(err.max()) / float(r.abs().max()):.2e} max|ref|")
        assert float(err.max()) <= 1e-5 * float(r.abs().max())
    for a in steps:
        for b in steps:
            y = run(a, b, act)
            assert torch.equal(y, y0 * 2.0 ** (a + b)), (family, a, b, int((y != y0 * 2.0 ** (a + b)).sum()))


WIDE_EXP = 50  # |a| = |b| of the wide sweep; the bar held here on the MI355X: not narrowed


@pytest.mark.parametrize("sign", [-1, 1], ids=["2^-100", "2^+100"])
@pytest.mark.parametrize("family", ["f32", "x6"])
def test_wide_dynamic_range(family, sign):
    """The A3 operands at a = b = -50 and +50: outputs around 2^-100 / 2^+100 (below 2^128: 2^112 products, 288 terms);
    at 2^-100 the low split planes' products are fp32-subnormal.  Relative float64 bar 1e-5 max|ref|."""
    run, ref, _ = _eq_ops(family)
    e = sign * WIDE_EXP
    y = run(e, e, 1)
    r = ref(1) * 2.0 ** (2 * e)
    assert bool(torch.isfinite(y).all())
    err, scale = float((y.cpu().double() - r).abs().max()), float(r.abs().max())
    print(f"[value] wide {family} 2^{2 * e}: max err {err / scale:.3e} max|ref|")
    assert err <= 1e-5 * scale, (family, e, err / scale)


def test_flt_max_operand():
    """One element of x is FLT_MAX in a 1x1 conv with weights +-2^-10: the float64 reference is finite (~3.3e35).
    The exact-f32 kernel meets its bar; in the split arithmetic bf16(FLT_MAX) = Inf (every |v| >= 0x7F7F8000 rounds
    up to it), so that pixel's outputs are non-finite -- all of them, none a wrong finite number -- and every other
    pixel meets the bar (taken against max|ref| of the other pixels, not the 3.3e35)."""
    import bev_native as nat
    Ci, Co = 64, 40
    g = torch.Generator().manual_seed(5300)
    x = _rand(g, N, HO, WO, Ci)
    w = (torch.randint(0, 2, (Co, Ci, 1, 1), generator=g).float() * 2 - 1) * 2.0 ** -10
    b = _rand(g, Co) * 0.1
    x[0, 4, 7, 9] = FLT_MAX
    ref = _conv64(x, w) + b.double()
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(ref.float()).all())
    pix = torch.zeros(N, HO, WO, Co, dtype=torch.bool)
    pix[0, 4, 7] = True
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    yf = nat.conv2d_nhwc(xd, nat.pack_conv_weight(wd), bd, Co, 1, 1, 1, 0, 0).cpu().double()
    y6 = nat.conv2d_nhwc_x6(xd, nat.pack_conv_weight_x6(wd), bd, Co, 1, 1, 1, 0, 1, 0).cpu().double()
    rest = float(ref[~pix].abs().max())
    assert bool(torch.isfinite(yf).all())
    assert float((yf - ref)[pix].abs().max()) <= 1e-5 * float(ref[pix].abs().max())
    assert float((yf - ref)[~pix].abs().max()) <= 1e-5 * rest
    assert torch.equal(~torch.isfinite(y6), pix), int((~torch.isfinite(y6)).sum())
    assert float((y6 - ref)[~pix].abs().max()) <= 1e-5 * rest


OVERFLOW = ["conv2d_h16_half", "conv2d_pw_h16", "dwconv2d_nhwc_h16", "batchnorm_apply_half"]


@pytest.mark.parametrize("entry", OVERFLOW)
def test_fp16_store_overflows_like_tensor_half(entry):
    """fp16 stores round to nearest even and overflow to Inf, as tensor.half() does: channels whose bias (shift) puts
    the float64 result above 65520 must store +Inf, between 65504 and 65520 must store 65504, below -65520 -Inf.  A
    saturating or round-toward-zero store fails.  The conv part of each result is |.| < 4, and elements within 1 of a
    band edge are left out (the fp32 sum's own error at 65504 is ~ 0.01)."""
    import bev_native as nat
    g = torch.Generator().manual_seed(5400)
    C = 48
    band = torch.tensor([70000.0, 65512.0, -70000.0, 65530.0, 65506.0, -65530.0, 0.5, 60000.0])
    b = band.repeat(C // 8)
    if entry == "conv2d_h16_half":
        x, w = (_rand(g, N, HO, WO, 64) * 0.25).half(), (_rand(g, C, 64, 3, 3) / 24).half()
        ref = _conv64(x, w, 1, 1) + b.double()
        y = nat.conv2d_h16_half(x.to(DEV), nat.pack_conv_weight_h16(w.float().to(DEV)), b.to(DEV), C, 3, 3, 1, 1)
    elif entry == "conv2d_pw_h16":
        x, w = (_rand(g, N, HO, WO, 40) * 0.25).half(), (_rand(g, C, 40) / 40 ** 0.5).half()
        ref = x.double() @ w.double().t() + b.double()
        y = nat.conv2d_pw_h16(x.to(DEV), w.to(DEV), b.to(DEV), f32_out=False)
    elif entry == "dwconv2d_nhwc_h16":
        x, w = (_rand(g, N, HO, WO, C) * 0.25).half(), (_rand(g, C, 1, 3, 3) * 0.3).half()
        ref = _conv64(x, w, 1, 1, groups=C) + b.double()
        y, _ = nat.dwconv2d_nhwc_h16(x.to(DEV), w.reshape(C, 9).t().contiguous().to(DEV), b.to(DEV), 3, 1, 1, 0)
    else:
        z, scale = _rand(g, N, HO, WO, C) * 0.25, torch.rand(C, generator=g) + 0.5
        ref = z.double() * scale.double() + b.double()
        y = nat.batchnorm_apply_half(z.to(DEV), scale.to(DEV), b.to(DEV), act=0)
    torch.cuda.synchronize()
    assert float((ref - b.double()).abs().max()) < 4.0
    yc, want = y.cpu(), ref.half()
    hi, mid, lo = ref > 65521, (ref > 65505) & (ref < 65519), ref < -65521
    assert int(hi.sum()) > 500 and int(mid.sum()) > 500 and int(lo.sum()) > 500
    assert bool((want[hi] == INF).all()) and bool((want[mid] == 65504).all()) and bool((want[lo] == -INF).all())
    for name, m in (("above 65520", hi), ("65504..65520", mid), ("below -65520", lo)):
        assert torch.equal(yc[m], want[m]), (entry, name, yc[m][yc[m] != want[m]][:4].tolist())
    rest = ~(hi | mid | lo) & (ref.abs() < 65000)
    assert bool(torch.isfinite(yc[rest]).all())


def _subnormal_case(which):
    """One operand entirely fp16-subnormal (k 2^-24, k in [1, 511]: [2^-24, 2^-15)), the other with magnitudes in
    [2^3, 2^15) (< 65504).  -> x, w (fp32 tensors holding fp16 values)."""
    g = torch.Generator().manual_seed(5500)

    def sub(*shape):
        k = torch.randint(1, 512, shape, generator=g).float()
        return k * 2.0 ** -24 * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)

    def big(*shape):
        return _wide(g, *shape, fp16=True) * 2.0 ** 9  # 2^3 .. 2^15

    if which == "x":
        return sub(N, HO, WO, 32), big(40, 32, 3, 3)
    return big(N, HO, WO, 32), sub(40, 32, 3, 3)


@pytest.mark.parametrize("which", ["x", "w"], ids=["x-subnormal", "w-subnormal"])
def test_h16_conv_subnormal_operand(which):
    """conv2d_nhwc_h16 (3x3, Ci 32) with one operand in the fp16 subnormal range: float64 over the fp16 values, the
    per-element bound of test_conv_h16_gpu.py unchanged (K 2^-24 sum|x||w| + 1e-6).  The scales make its absolute 1e-6
    at most 1/32 of the median bound (asserted), so the case cannot pass by that slack."""
    import bev_native as nat
    x, w = _subnormal_case(which)
    assert torch.equal(x.half().float(), x) and torch.equal(w.half().float(), w)
    s = x if which == "x" else w
    assert float(s.abs().max()) < 2.0 ** -15 and float(s.abs().min()) >= 2.0 ** -24
    ref, mag = _conv64(x, w, 1, 1), _conv64(x.abs(), w.abs(), 1, 1)
    bound = 288 * 2.0 ** -24 * mag + 1e-6
    assert 1e-6 <= float(bound.median()) / 32, float(bound.median())
    y = nat.conv2d_nhwc_h16(x.to(DEV), nat.pack_conv_weight_h16(w.to(DEV)), None, 40, 3, 3, 1, 1)
    torch.cuda.synchronize()
    err = (y.cpu().double() - ref).abs()
    print(f"[value] h16 conv {which}-subnormal: max err / bound {float((err / bound).max()):.3e}, "
          f"|y| max {float(y.abs().max()):.3e}, |ref| max {float(ref.abs().max()):.3e}")
    assert bool((err <= bound).all()), float((err - bound).max())


@pytest.mark.parametrize("stored", ["f32", "f16"])
@pytest.mark.parametrize("which", ["x", "dz"], ids=["x-subnormal", "dz-subnormal"])
def test_h16_wgrad_subnormal_operand(which, stored):
    """conv_wgrad_h16_any, operands stored in fp32 and in fp16: x or the gradient dz (GradScaler-scaled gradients of
    the first layers are fp16-subnormal) entirely subnormal.  Same bound, K = the 270 pixels summed per weight."""
    import bev_native as nat
    g = torch.Generator().manual_seed(5600)
    Ci, Co = 64, 36

    def sub(*shape):
        k = torch.randint(1, 512, shape, generator=g).float()
        return k * 2.0 ** -24 * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)

    def big(*shape):
        return _wide(g, *shape, fp16=True) * 2.0 ** 8  # 2^2 .. 2^14
    x, dz = (sub(N, HO, WO, Ci), big(N, HO, WO, Co)) if which == "x" else (big(N, HO, WO, Ci), sub(N, HO, WO, Co))
    assert torch.equal(x.half().float(), x) and torch.equal(dz.half().float(), dz)
    xn, dn = _nchw(x.double()), _nchw(dz.double())
    ref = torch.nn.grad.conv2d_weight(xn, (Co, Ci, 3, 3), dn, 1, 1, 1)
    mag = torch.nn.grad.conv2d_weight(xn.abs(), (Co, Ci, 3, 3), dn.abs(), 1, 1, 1)
    bound = N * HO * WO * 2.0 ** -24 * mag + 1e-6
    assert 1e-6 <= float(bound.median()) / 32, float(bound.median())
    cast = (lambda t: t.half()) if stored == "f16" else (lambda t: t)
    dw = nat.conv_wgrad_h16_any(cast(x).to(DEV), cast(dz).to(DEV), 3, 3, 1, 1)
    torch.cuda.synchronize()
    err = (dw.cpu().double() - ref).abs()
    print(f"[value] h16 wgrad {which}-subnormal {stored}: max err / bound {float((err / bound).max()):.3e}")
    assert bool((err <= bound).all()), float((err - bound).max())
