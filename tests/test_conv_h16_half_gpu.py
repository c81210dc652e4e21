"""bev_conv2d_h16_h16 (bev_native.conv2d_h16_half): the "f16" inference convolution -- fp16 operands on the fp16
matrix cores, fp32 accumulation, fp16 residual, fp16 output rounded once after bias + residual + act.

(a) against a float64 convolution of the fp16-rounded operands, independent of the other kernels:
        |y - ref| <= 2^-11 |ref| + (K + 2) 2^-24 (sum |x||w| + |b| + |r|) + 2^-24
    = half an fp16 ulp of the result + the worst-case fp32 summation bound of tests/test_conv_h16_gpu.py (K products,
    the bias and the residual add) + the fp16 subnormal step; x 1.2 for SiLU (the hardware exp2 / rcp form), as there.
(b) bit-exactness: every output is the fp32-output kernel's (bev_conv2d_h16_ex_f32, conv2d_h16_any) value with act
    applied in fp32, rounded once to fp16 -- for x stored in fp32 and in fp16, and for each tile form
    (CONV_H16_KERNEL 0 / 2 / 3).  ReLU is applied by torch on the fp32 tensor; SiLU by the fp32-output kernel itself
    (its hardware form is not torch's to the bit).
(c) nothing outside [N][Ho][Wo][Co] is written (rows past M in the last tile, columns past Co).
(d) refusals.

The shapes are the smallest that reach each tail of the K pipeline (1, 2, 3 and 9+ steps), both tile widths, a ragged
last row tile, Co that is no multiple of the tile and every conv form of the ResNet trunk.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = [
    # 1x1 64 -> 64: M = 117 < 128, one K step, the 64-column tile
    dict(N=1, H=9, W=13, Ci=64, Co=64, K=1, stride=1, pad=0, act=1, res=False),
    # ragged M = 286, two K steps, fp16 residual + ReLU
    dict(N=2, H=11, W=13, Ci=128, Co=256, K=1, stride=1, pad=0, act=1, res=True),
    # three K steps, Co % 64 != 0, no act
    dict(N=1, H=12, W=12, Ci=192, Co=72, K=1, stride=1, pad=0, act=0, res=False),
    # a 128-column tile plus an 8-column tail, residual
    dict(N=1, H=12, W=12, Ci=256, Co=136, K=1, stride=1, pad=0, act=0, res=True),
    # padding taps across image boundaries
    dict(N=2, H=10, W=12, Ci=64, Co=64, K=3, stride=1, pad=1, act=1, res=False),
    # stride 2
    dict(N=1, H=17, W=33, Ci=128, Co=128, K=3, stride=2, pad=1, act=1, res=True),
    # the downsample form
    dict(N=1, H=15, W=21, Ci=256, Co=512, K=1, stride=2, pad=0, act=0, res=False),
    # SiLU
    dict(N=1, H=8, W=8, Ci=64, Co=40, K=3, stride=1, pad=1, act=2, res=False),
]
IDS = [f"{d['Ci']}to{d['Co']}k{d['K']}s{d['stride']}a{d['act']}{'r' if d['res'] else ''}" for d in SHAPES]
_CACHE = {}


def _case(i):
    """Inputs of shape i (host + device) and the float64 references, computed once and shared (never modified)."""
    if i in _CACHE:
        return _CACHE[i]
    import bev_native as nat
    d = SHAPES[i]
    N, H, W, Ci, Co, K, st, pad, act = (d[k] for k in ("N", "H", "W", "Ci", "Co", "K", "stride", "pad", "act"))
    g = torch.Generator().manual_seed(100 + i)
    x = torch.randn(N, H, W, Ci, generator=g)
    w = torch.randn(Co, Ci, K, K, generator=g) / (Ci * K * K) ** 0.5
    b = torch.randn(Co, generator=g)
    Ho, Wo = (H + 2 * pad - K) // st + 1, (W + 2 * pad - K) // st + 1
    r16 = torch.randn(N, Ho, Wo, Co, generator=g).half() if d["res"] else None

    def ref64(xd, wd):
        z = F.conv2d(xd.permute(0, 3, 1, 2), wd, None, st, pad).permute(0, 2, 3, 1) + b.double()
        if r16 is not None:
            z = z + r16.double()
        if act == 1:
            z = z.clamp_min(0)
        elif act == 2:
            z = z * torch.sigmoid(z)
        return z

    xh, wh = x.half().double(), w.half().double()
    mag = F.conv2d(xh.abs().permute(0, 3, 1, 2), wh.abs(), None, st, pad).permute(0, 2, 3, 1) + b.double().abs()
    if r16 is not None:
        mag = mag + r16.double().abs()
    c = dict(d, Ho=Ho, Wo=Wo, x=x.to(DEV), xh=x.half().to(DEV), b=b.to(DEV),
             r16=None if r16 is None else r16.to(DEV), packed=nat.pack_conv_weight_h16(w.to(DEV)),
             ref=ref64(xh, wh), ref_raw=ref64(x.double(), w.double()), mag=mag)
    _CACHE[i] = c
    return c


def _run(c, x, out=None):
    import bev_native as nat
    return nat.conv2d_h16_half(x, c["packed"], c["b"], c["Co"], c["K"], c["K"], c["stride"], c["pad"], 1, c["act"],
                               residual=c["r16"], out=out)


@pytest.mark.parametrize("x_half", [False, True], ids=["xf32", "xf16"])
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_h16_half_vs_float64_of_rounded_operands(i, x_half):
    c = _case(i)
    y = _run(c, c["xh"] if x_half else c["x"])
    torch.cuda.synchronize()
    assert y.dtype == torch.float16 and tuple(y.shape) == (c["N"], c["Ho"], c["Wo"], c["Co"])
    yd, ref = y.cpu().double(), c["ref"]
    Kt = c["Ci"] * c["K"] * c["K"]
    bound = 2.0 ** -11 * ref.abs() + (Kt + 2) * 2.0 ** -24 * c["mag"] + 2.0 ** -24
    if c["act"] == 2:
        bound = bound * 1.2
    err = (yd - ref).abs()
    print(f"max err {float(err.max()):.3e}  max err/bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), float((err - bound).max())
    # and it is the arithmetic of the fp16-rounded operands: the result of the unrounded ones, rounded the same way,
    # differs in many more elements
    miss = int((y.cpu() != ref.half()).sum())
    miss_raw = int((y.cpu() != c["ref_raw"].half()).sum())
    print(f"elements off the rounded-operand result {miss}, off the unrounded-operand result {miss_raw}")
    assert miss_raw > 0 and miss < miss_raw


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_h16_half_is_the_f32_output_kernel_rounded_once(i):
    import bev_native as nat
    c = _case(i)
    r32 = None if c["r16"] is None else c["r16"].float()
    z = nat.conv2d_h16_any(c["x"], c["packed"], c["Co"], c["K"], c["K"], c["stride"], c["pad"], residual=r32,
                           bias=c["b"], act=2 if c["act"] == 2 else 0)
    if c["act"] == 1:
        z = torch.relu(z)
    want = z.half()
    for x in (c["x"], c["xh"]):
        for kern in (0, 2, 3):
            with nat.tuned(CONV_H16_KERNEL=kern):
                y = _run(c, x)
            assert torch.equal(y, want), (str(x.dtype), kern, int((y != want).sum()))


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_h16_half_writes_only_its_output(i):
    import bev_native as nat
    c = _case(i)
    n = c["N"] * c["Ho"] * c["Wo"] * c["Co"]
    pad = 128 * 136  # more than one tile row block past either end
    for kern in (0, 2, 3):
        buf = torch.full((pad + n + pad,), 1234.0, device=DEV, dtype=torch.float16)
        out = buf[pad:pad + n].view(c["N"], c["Ho"], c["Wo"], c["Co"])
        with nat.tuned(CONV_H16_KERNEL=kern):
            y = _run(c, c["xh"], out=out)
        assert y.data_ptr() == out.data_ptr()
        assert bool((buf[:pad] == 1234.0).all()) and bool((buf[pad + n:] == 1234.0).all()), kern
        assert torch.equal(out, _run(c, c["xh"]))


def test_h16_half_refusals():
    import bev_native as nat
    z = lambda *s, dt=torch.float32: torch.zeros(*s, device=DEV, dtype=dt)  # noqa: E731
    p64 = nat.pack_conv_weight_h16(z(64, 64, 1, 1))
    b64 = z(64)
    with pytest.raises(nat.HipError):  # Ci = 96: no whole 64-channel K steps
        nat.conv2d_h16_half(z(1, 4, 4, 96), nat.pack_conv_weight_h16(z(64, 96, 1, 1)), b64, 64, 1, 1, 1, 0)
    with pytest.raises(nat.HipError):  # Co = 20: no 16-B groups of 8 output channels
        nat.conv2d_h16_half(z(1, 4, 4, 64), nat.pack_conv_weight_h16(z(20, 64, 1, 1)), z(20), 20, 1, 1, 1, 0)
    x = z(1, 4, 4, 64)
    buf = z(16 * 64 + 8, dt=torch.float16)
    with pytest.raises(nat.HipError):  # y 8 B past a 16-B boundary
        nat.conv2d_h16_half(x, p64, b64, 64, 1, 1, 1, 0, out=buf[4:4 + 16 * 64].view(1, 4, 4, 64))
    r = z(1, 4, 4, 64, dt=torch.float16)
    with pytest.raises(nat.HipError):  # the residual is the output
        nat.conv2d_h16_half(x, p64, b64, 64, 1, 1, 1, 0, residual=r, out=r)
    with pytest.raises(nat.HipError):  # ... or overlaps it
        nat.conv2d_h16_half(x, p64, b64, 64, 1, 1, 1, 0, residual=buf[8:8 + 16 * 64].view(1, 4, 4, 64),
                            out=buf[:16 * 64].view(1, 4, 4, 64))
    with pytest.raises(nat.HipError):  # an fp32 panel
        nat.conv2d_h16_half(x, p64.float(), b64, 64, 1, 1, 1, 0)
    with pytest.raises(nat.HipError):  # act out of range
        nat.conv2d_h16_half(x, p64, b64, 64, 1, 1, 1, 0, act=3)
    y = nat.conv2d_h16_half(x, p64, b64, 64, 1, 1, 1, 0, residual=r)  # and the well-formed call runs
    torch.cuda.synchronize()
    assert y.dtype == torch.float16 and not bool(y.any())
