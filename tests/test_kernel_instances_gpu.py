"""One case per kernel instantiation outside the conv sources that no other test launches (tools/kernel_coverage.py,
profiles/r11a_kernel_coverage_after.txt): the fp16-store and SiLU + residual / mask-byte forms of bev_bn.hip, the
scalar weight gradient k_wgrad of bev_train.hip, the per-pixel depthwise kernel on a width the row runs do not take and
every k_irdw of bev_effnet.hip, the register-staged fused warp k_warp_fuse and the span-staged channels-last k_warp_fuse_v2 of
bev_warp.hip.  Each case forces its instance through the public wrappers, nat.lib() and nat.tuned(...), and its id
names it (with the siblings of its family, so that a whole family is compared under one set of bounds).

The reference is always float64 torch on the CPU over the operands as the kernel sees them (for the warp: the CPU
oracle, bit for bit) -- never another kernel.  Bounds, all the project's:

 BatchNorm  fp32 outputs: test_batchnorm_train_kernels_vs_torch's bars, 1e-5 max|ref| for y, dres, dbeta and 1e-4
            max|ref| for dz, dgamma.  fp16 outputs, per element: |got - ref| <= 2^-11 |ref| + 2^-25 + bar32 (round to
            nearest of a normal, half the subnormal spacing, the fp32 bar of the same quantity), and
            torch.equal(out16, out32.half()): bev_bn.hip's st4 is RNE of the same per-element arithmetic.  Gradients
            through ReLU only after asserting that no ReLU decision differs from the reference's.
 k_wgrad    1e-4 max|dW_ref| (float atomics change the summation order), against float64 autograd of F.conv2d and
            against the padded float4 / MFMA path (conv_wgrad_ex) within the same bar.
 depthwise  y within 1e-5 max|ref|; the SE partials summed over blocks within 1e-5 max(1, max|sums|) of the float64
            channel sums of the reference, their count bev_dwconv_psum_blocks'; torch.equal(y + 0.0, y_0 + 0.0) against
            BEV_TUNE_DW_RUN 0 (the header: same y up to the sign of an exact zero).  k_irdw: the first two.
 warp       bit-identical to oracle.fused_stream; span staging also to the same launch with BEV_TUNE_WARP_SPAN 0 and
            to the NCHW output.

Shapes: BatchNorm M = 2 x 13 x 17 = 442 rows (no multiple of BNQ_ROWS = 256 nor of BN_U x nph: the unrolled loop and
the tail both run), C = 64 / 4 / 1024 (row-block kernels: 16 / 256 / 1 row phases) and 24 / 144 (flat grid-stride
kernels), one flat case of M = 350001 rows (total4 > 8192 x 256: the grid-stride loop iterates twice); weight gradient
N = 2 on 13 x 17 outputs (28 m-chunks of 16 rows, the last of 10); depthwise 11 x 19 outputs (209 pixels: 27 workgroups
of 8, the last of 1); k_irdw 19 output rows (two IR_RSEG = 16 segments) x tc + 3 columns (two strips, the last of 3), Cm = 96
(two 48-channel groups); the warp on the small fixture geometries.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_CACHE = {}


def _cached(key, make):
    """Operands and float64 references are made once per shape and shared (never modified)."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _act64(z, act):
    if act == 1:
        return z.clamp_min(0)
    if act == 2:
        return z * torch.sigmoid(z)
    return z


def _tf(b):
    return "true" if b else "false"


# ======================================================================================================================
# BatchNorm store forms (bev_bn.hip): k_bn_apply<IT, OT>, k_bn_apply_q<OT, ACT, RES>, k_bn_bwd_apply<IT, OT>,
# k_bn_bwd_apply_q<OT, ACT>
# ======================================================================================================================
BN_M = 2 * 13 * 17
BN_Q_C = (64, 4, 1024)   # 256 % (C / 4) == 0: the row-block kernels
BN_FLAT_C = (24, 144)    # every other width: the flat grid-stride kernels


def _bn_op(C, M=BN_M):
    """test_batchnorm_train_kernels_vs_torch's operand generators as rows [M][C]; statistics from the library."""
    import bev_native as nat

    def make():
        g = torch.Generator().manual_seed(C + M)
        z = torch.randn(M, C, generator=g) * 2 + 0.5
        gamma = torch.rand(C, generator=g) + 0.5
        beta = torch.randn(C, generator=g) * 0.3
        r = torch.randn(M, C, generator=g)
        dy = torch.randn(M, C, generator=g)
        zg, gg = z.to(DEV), gamma.to(DEV)
        mean, rstd, scale, shift = nat.batchnorm_train_fwd(zg, gg, beta.to(DEV), None, None, 1e-5, 0.1)
        return dict(z=z, gamma=gamma, beta=beta, r=r, dy=dy, zg=zg, gg=gg, rg=r.to(DEV), dyg=dy.to(DEV), mean=mean,
                    rstd=rstd, scale=scale, shift=shift)
    return _cached(("bn-op", C, M), make)


def _bn_ref(C, act, res, M=BN_M, grads=True):
    """float64 F.batch_norm (batch statistics) -> + residual -> ReLU / SiLU, and its autograd under dy.  `dres` is the
    gradient reaching the pre-activation (what the kernel calls d(residual), with or without a residual)."""
    c = _bn_op(C, M)

    def make():
        zd = c["z"].double().requires_grad_(grads)
        gd, bd = c["gamma"].double().requires_grad_(grads), c["beta"].double().requires_grad_(grads)
        pre = F.batch_norm(zd, None, None, gd, bd, True, 0.1, 1e-5)
        if res:
            pre = pre + c["r"].double()
        if not grads:
            return dict(y=_act64(pre, act).detach())
        pre.retain_grad()
        y = torch.relu(pre) if act == 1 else F.silu(pre) if act == 2 else pre * 1.0
        y.backward(c["dy"].double())
        return dict(y=y.detach(), dz=zd.grad, dres=pre.grad, dgamma=gd.grad, dbeta=bd.grad)
    return _cached(("bn-ref", C, act, res, M, grads), make)


def _bn_apply(c, res, act, half):
    """bev_batchnorm_apply_ex_f32 (the product's fp16-store wrapper takes no residual)."""
    import bev_native as nat
    z = c["zg"]
    M, C = z.shape
    y = torch.empty(M, C, device=DEV, dtype=torch.float16 if half else torch.float32)
    rc = nat.lib().bev_batchnorm_apply_ex_f32(nat._ptr(z), M, C, nat._ptr(c["scale"]), nat._ptr(c["shift"]),
                                              nat._ptr(c["rg"]) if res else None, int(act), nat._ptr(y), int(half),
                                              nat._stream(z))
    assert rc == 0, rc
    return y


def _bn_bwd(c, yarg, act, half):
    """bev_batchnorm_bwd_ex_f32 with dres requested -> (dz, dres, dgamma, dbeta)."""
    import bev_native as nat
    z = c["zg"]
    M, C = z.shape
    dz = torch.empty(M, C, device=DEV, dtype=torch.float16 if half else torch.float32)
    dres, dg, db = torch.empty(M, C, device=DEV), torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    ws = nat._bn_workspace(M, C, z.device)
    rc = nat.lib().bev_batchnorm_bwd_ex_f32(nat._ptr(c["dyg"]), nat._ptr(yarg), nat._ptr(z), M, C, nat._ptr(c["mean"]),
                                            nat._ptr(c["rstd"]), nat._ptr(c["gg"]), nat._ptr(c["scale"]),
                                            nat._ptr(c["shift"]), int(act), 0, nat._ptr(dz), int(half), nat._ptr(dres),
                                            nat._ptr(dg), nat._ptr(db), nat._ptr(ws), nat._stream(z))
    assert rc == 0, rc
    return dz, dres, dg, db


def _chk32(tag, what, got, ref, tol):
    assert got.dtype == torch.float32 and bool(torch.isfinite(got).all()), (tag, what)
    err, scale = (got.double().cpu() - ref).abs().max().item(), ref.abs().max().item()
    print(f"[instance] {tag} {what}: max err {err:.3e} = {err / max(scale, 1e-300):.2e} max|ref| (bar {tol:.0e})")
    assert err <= tol * scale, (tag, what, err, scale)


def _chk16(tag, what, got, ref, tol32):
    assert got.dtype == torch.float16 and bool(torch.isfinite(got).all()), (tag, what)
    err = (got.double().cpu() - ref).abs()
    bound = 2.0 ** -11 * ref.abs() + 2.0 ** -25 + tol32 * ref.abs().max().item()
    print(f"[instance] {tag} {what} (fp16): max err {err.max().item():.3e}, max err / bound "
          f"{(err / bound).max().item():.3f}")
    assert bool((err <= bound).all()), (tag, what, (err - bound).max().item())


def _bn_fwd16_cases():
    out = []
    for C in BN_Q_C + BN_FLAT_C:
        for act in (0, 1, 2):
            for res in (False, True):
                if C in BN_Q_C:
                    out.append((f"k_bn_apply_q<_Float16,{act},{_tf(res)}>-c{C}", C, act, res))
                else:
                    out.append((f"k_bn_apply<unsigned,_Float16>-act{act}-res{int(res)}-c{C}", C, act, res))
    return out


@pytest.mark.parametrize("case", _bn_fwd16_cases(), ids=[c[0] for c in _bn_fwd16_cases()])
def test_bn_apply_fp16_store(case):
    """bev_batchnorm_apply_ex_f32 with y_half = 1, act none / ReLU / SiLU, with and without residual, on the row-block
    and the flat kernel: against float64 BatchNorm, and RNE of the fp32-store call's y bit for bit."""
    tag, C, act, res = case
    c, ref = _bn_op(C), _bn_ref(C, act, res)["y"]
    y32 = _cached(("bn-y32", C, act, res), lambda: _bn_apply(c, res, act, False))
    y16 = _bn_apply(c, res, act, True)
    torch.cuda.synchronize()
    _chk32(tag, "y32", y32, ref, 1e-5)
    _chk16(tag, "y", y16, ref, 1e-5)
    assert torch.equal(y16, y32.half()), (tag, int((y16 != y32.half()).sum()))


@pytest.mark.parametrize("C", BN_Q_C, ids=[f"k_bn_apply_q<float,2,true>-c{C}" for C in BN_Q_C])
def test_bn_apply_silu_residual_fp32(C):
    """fp32 SiLU + residual on the row-block kernel (EfficientNet's act with a ResNet shortcut: no trunk has it)."""
    c, ref = _bn_op(C), _bn_ref(C, 2, True)["y"]
    y32 = _cached(("bn-y32", C, 2, True), lambda: _bn_apply(c, True, 2, False))
    torch.cuda.synchronize()
    _chk32(f"k_bn_apply_q<float,2,true>-c{C}", "y", y32, ref, 1e-5)


BN_BWD = [
    # id, C, act of the backward call, residual in the forward, dz stored in fp16
    ("k_bn_bwd_apply_q<_Float16,0>-c64", 64, 0, True, True),
    ("k_bn_bwd_apply_q<_Float16,0>-c4", 4, 0, True, True),
    ("k_bn_bwd_apply_q<_Float16,2>-c64", 64, 2, False, True),   # the backward's SiLU argument is z scale + shift:
    ("k_bn_bwd_apply_q<_Float16,2>-c1024", 1024, 2, False, True),  # a layer without residual
    ("k_bn_bwd_apply<unsigned,_Float16>-act1-c24", 24, 1, True, True),
    ("k_bn_bwd_apply<unsigned,_Float16>-act2-c144", 144, 2, False, True),
    ("k_bn_bwd_apply_q<float,4>-c64", 64, 4, True, False),
    ("k_bn_bwd_apply_q<float,4>-c1024", 1024, 4, True, False),
]


@pytest.mark.parametrize("case", BN_BWD, ids=[c[0] for c in BN_BWD])
def test_bn_bwd_store_forms(case):
    """bev_batchnorm_bwd_ex_f32 with dz_half = 1 (act 0, 2 on the row-block kernel, act 1 / 2 on the flat one) and
    act 4 (batchnorm_apply_mask's bytes) with fp32 dz: dz, dres, dgamma, dbeta against float64 autograd; the fp16 dz
    is RNE of the fp32-store call's, act 4 has act 1's bits."""
    import bev_native as nat
    tag, C, act, res, half = case
    fact = 1 if act == 4 else act
    c, ref = _bn_op(C), _bn_ref(C, fact, res)
    yarg = None
    if act == 4:
        y, yarg = nat.batchnorm_apply_mask(c["zg"], c["scale"], c["shift"], c["rg"])
    elif act == 1:
        y = yarg = _bn_apply(c, res, 1, False)
    if fact == 1:  # gradient checks need the same ReLU decisions as the reference
        assert int(((y.cpu() > 0) != (ref["y"] > 0)).sum()) == 0
    dz, dres, dg, db = _bn_bwd(c, yarg, act, half)
    if half:
        dz32, dres32, dg32, db32 = _bn_bwd(c, yarg, act, False)
    if act == 4:
        like1 = _bn_bwd(c, y, 1, False)
    torch.cuda.synchronize()
    if half:
        _chk16(tag, "dz", dz, ref["dz"], 1e-4)
        _chk32(tag, "dz32", dz32, ref["dz"], 1e-4)
        assert torch.equal(dz, dz32.half()), (tag, int((dz != dz32.half()).sum()))
        assert torch.equal(dres, dres32) and torch.equal(dg, dg32) and torch.equal(db, db32)
    else:
        _chk32(tag, "dz", dz, ref["dz"], 1e-4)
    _chk32(tag, "dres", dres, ref["dres"], 1e-5)
    _chk32(tag, "dgamma", dg, ref["dgamma"], 1e-4)
    _chk32(tag, "dbeta", db, ref["dbeta"], 1e-5)
    if act == 4:  # include/bev_mi355x.h: act 4 is bit-identical to act 1
        for u, v in zip((dz, dres, dg, db), like1):
            assert torch.equal(u, v)


BN_BIG_M = 350001  # x 24 / 4 = 2,100,006 float4 > 8192 x 256: stream_blocks' cap, a second grid-stride iteration


@pytest.mark.parametrize("half", [False, True], ids=["k_bn_apply<unsigned,float>-gridstride-m350001-c24",
                                                     "k_bn_apply<unsigned,_Float16>-gridstride-m350001-c24"])
def test_bn_apply_flat_grid_stride(half):
    """The flat kernel on more float4 than its capped grid has threads (SiLU + residual), fp32 and fp16 store."""
    C, act, res = 24, 2, True
    c, ref = _bn_op(C, BN_BIG_M), _bn_ref(C, act, res, BN_BIG_M, grads=False)["y"]
    assert BN_BIG_M * C // 4 > 8192 * 256
    y32 = _cached(("bn-y32", C, act, res, BN_BIG_M), lambda: _bn_apply(c, res, act, False))
    tag = f"k_bn_apply-gridstride-{'f16' if half else 'f32'}"
    if half:
        y16 = _bn_apply(c, res, act, True)
        torch.cuda.synchronize()
        _chk16(tag, "y", y16, ref, 1e-5)
        assert torch.equal(y16, y32.half()), int((y16 != y32.half()).sum())
    else:
        torch.cuda.synchronize()
        _chk32(tag, "y", y32, ref, 1e-5)


# ======================================================================================================================
# k_wgrad (bev_train.hip): the scalar weight gradient bev_conv_wgrad_ex_f32 runs when Ci % 4 != 0 or Co % 4 != 0
# ======================================================================================================================
WGRAD = [
    # id, Ci, Co, KH, KW, stride, pad, dilation, H, W (N = 2; outputs 13 x 17, 13 x 15 for 3x5)
    ("k_wgrad-ci3-co5-3x3", 3, 5, 3, 3, 1, 1, 1, 13, 17),
    ("k_wgrad-ci6-co8-3x3", 6, 8, 3, 3, 1, 1, 1, 13, 17),
    ("k_wgrad-ci8-co6-3x3", 8, 6, 3, 3, 1, 1, 1, 13, 17),
    ("k_wgrad-ci3-co72-7x7-s2-stem", 3, 72, 7, 7, 2, 3, 1, 26, 33),   # K = 147: three k blocks, two co blocks
    ("k_wgrad-ci6-co8-3x3-dil2", 6, 8, 3, 3, 1, 2, 2, 13, 17),
    ("k_wgrad-ci3-co5-3x5", 3, 5, 3, 5, 1, 1, 1, 13, 17),
]


@pytest.mark.parametrize("case", WGRAD, ids=[c[0] for c in WGRAD])
def test_wgrad_scalar_kernel(case):
    """bev_conv_wgrad_ex_f32 on unpadded operands (dW [Co, KH, KW, Ci]) against float64 autograd of F.conv2d, and
    against conv_wgrad_ex (channels zero-padded to multiples of 4: the float4 / MFMA kernels)."""
    import bev_native as nat
    tag, Ci, Co, KH, KW, s, p, dil, H, W = case
    N = 2
    g = torch.Generator().manual_seed(Ci + 10 * Co + KH * KW + dil)
    x = torch.randn(N, Ci, H, W, generator=g)
    w = torch.zeros(Co, Ci, KH, KW, dtype=torch.float64, requires_grad=True)
    out = F.conv2d(x.double(), w, None, s, p, dil)
    _, _, Ho, Wo = out.shape
    dz = torch.randn(N, Co, Ho, Wo, generator=g)
    out.backward(dz.double())
    ref = w.grad
    assert Ci % 4 != 0 or Co % 4 != 0  # else bev_conv_wgrad_ex_f32 takes k_wgrad_v4 / the MFMA kernels
    xd, dzd = x.permute(0, 2, 3, 1).contiguous().to(DEV), dz.permute(0, 2, 3, 1).contiguous().to(DEV)
    dW = torch.empty(Co, KH, KW, Ci, device=DEV)
    rc = nat.lib().bev_conv_wgrad_ex_f32(nat._ptr(xd), N, H, W, Ci, nat._ptr(dzd), Ho, Wo, Co, KH, KW, s, p, dil,
                                         nat._ptr(dW), nat._stream(xd))
    assert rc == 0, rc
    padded = nat.conv_wgrad_ex(xd, dzd, KH, p, dil, stride=s, KW=KW)
    torch.cuda.synchronize()
    got = dW.permute(0, 3, 1, 2)
    scale = ref.abs().max().item()
    _chk32(tag, "dW", got.contiguous(), ref, 1e-4)
    _chk32(tag, "dW (padded path)", padded, ref, 1e-4)
    assert (got - padded).abs().max().item() <= 1e-4 * scale


# ======================================================================================================================
# k_dwconv<K> (bev_effnet.hip) at the defaults: channel counts that the row runs cannot chunk
# ======================================================================================================================
DW_HO, DW_WO = 11, 19


def _dw_op(C, K, S):
    def make():
        g = torch.Generator().manual_seed(C + 7 * K + S)
        H, W = (DW_HO, DW_WO) if S == 1 else (2 * DW_HO - 1, 2 * DW_WO - 1)
        x = torch.randn(2, C, H, W, generator=g)
        w, b = torch.randn(C, 1, K, K, generator=g) * 0.3, torch.randn(C, generator=g) * 0.1
        z = F.conv2d(x.double(), w.double(), b.double(), S, K // 2, groups=C).permute(0, 2, 3, 1)
        assert z.shape[1:3] == (DW_HO, DW_WO)
        return dict(z=z, x=x.permute(0, 2, 3, 1).contiguous().to(DEV), wt=w.reshape(C, K * K).t().contiguous().to(DEV),
                    b=b.to(DEV))
    return _cached(("dw", C, K, S), make)


def _dw_check(tag, C, K, S, nb):
    import bev_native as nat
    c = _dw_op(C, K, S)
    assert nat.lib().bev_dwconv_psum_blocks(DW_HO, DW_WO, C, S) == nb, tag  # the count worked out in the case
    for act in (0, 2):
        ref = _act64(c["z"], act)
        y, ps = nat.dwconv2d_nhwc(c["x"], c["wt"], c["b"], K, S, K // 2, act, want_psum=True)
        with nat.tuned(DW_RUN=0):
            y0, _ = nat.dwconv2d_nhwc(c["x"], c["wt"], c["b"], K, S, K // 2, act, want_psum=True)
        torch.cuda.synchronize()
        assert y.shape == ref.shape and ps.shape == (2, nb, C), (tag, ps.shape)  # one SE partial per workgroup
        _chk32(tag, f"y act {act}", y, ref, 1e-5)
        sums = ref.sum(dim=(1, 2))
        err = (ps.double().sum(1).cpu() - sums).abs().max().item()
        assert err <= 1e-5 * max(1.0, sums.abs().max().item()), (tag, act, err)
        assert torch.equal(y + 0.0, y0 + 0.0), (tag, act)


@pytest.mark.parametrize("K,S", [(3, 1), (5, 2)], ids=["k_dwconv<3>-c536-s1", "k_dwconv<5>-c536-s2"])
def test_dwconv_unchunkable_width_runs_per_pixel(K, S):
    """C = 536: 134 channel quads, which the row runs cannot split into equal chunks of at most 64 and whose even
    count the LDS tile (last tree e891532) used to take at the defaults.  Now the per-pixel k_dwconv: 11 x 19
    outputs, one pixel per step (256 // 134) -> 8 pixels per workgroup, 27 SE partials, the last workgroup ragged."""
    ppb = 8 * (256 // (536 // 4))  # DW_STEPS pixel steps of 256 // (C / 4) pixels
    _dw_check(f"k_dwconv<{K}> C 536 stride {S}", 536, K, S, -(-DW_HO * DW_WO // ppb))


# ======================================================================================================================
# k_irdw<K, S, Ci> (bev_effnet.hip): every instance through ir_expand_dw
# ======================================================================================================================
IRDW = [(K, S, Ci) for K, S in ((3, 1), (3, 2), (5, 1), (5, 2)) for Ci in (16, 24, 32, 40, 48)]
IR_CM, IR_HO = 96, 19


@pytest.mark.parametrize("K,S,Ci", IRDW, ids=[f"k_irdw<{K},{S},{Ci}>" for K, S, Ci in IRDW])
def test_irdw_instances(K, S, Ci):
    """Expansion + depthwise in one pass: operands folded as test_ir_expand_dw_fused_vs_float64_and_separate folds them
    (FoldedConv / FoldedDW); float64 conv_pw -> SiLU -> conv_dw -> SiLU over the folded fp32 operands.  Two row
    segments (16 + 3 rows), two strips (tc + 3 columns), two 48-channel groups, two images."""
    import bev_native as nat
    from models.encoders.efficientnet import FoldedDW
    from models.encoders.resnet import FoldedConv
    tag = f"k_irdw<{K},{S},{Ci}>"
    tc = (32 - K) // S + 1
    Ho, Wo, Cm = IR_HO, tc + 3, IR_CM
    H, W = (Ho, Wo) if S == 1 else (2 * Ho - 1, 2 * Wo - 1)
    torch.manual_seed(Ci + K + S + H)
    pw, bn1 = torch.nn.Conv2d(Ci, Cm, 1, bias=False), torch.nn.BatchNorm2d(Cm)
    dw, bn2 = torch.nn.Conv2d(Cm, Cm, K, S, K // 2, groups=Cm, bias=False), torch.nn.BatchNorm2d(Cm)
    with torch.no_grad():
        for bn in (bn1, bn2):
            bn.weight.uniform_(0.5, 1.5), bn.bias.uniform_(-0.5, 0.5)
            bn.running_mean.uniform_(-0.2, 0.2), bn.running_var.uniform_(0.5, 2.0)
    for m in (bn1, bn2):
        m.eval()
    x = torch.randn(2, Ci, H, W, generator=torch.Generator().manual_seed(Ci + H))
    fc = FoldedConv(pw.to(DEV), bn1.to(DEV))
    fdw = FoldedDW(dw.to(DEV), bn2.to(DEV))
    fdw.prepare(DEV)
    we, be = fc.folded(DEV)
    we = we.reshape(Cm, Ci).contiguous()
    xn = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    y, ps = nat.ir_expand_dw(xn, we, be, fdw.wt, fdw.bias, K, S)
    torch.cuda.synchronize()
    wd64 = fdw.wt.double().cpu().t().reshape(Cm, 1, K, K)
    h = F.silu(F.conv2d(x.double(), we.double().cpu().reshape(Cm, Ci, 1, 1), be.double().cpu()))
    ref = F.silu(F.conv2d(h, wd64, fdw.bias.double().cpu(), S, K // 2, groups=Cm)).permute(0, 2, 3, 1)
    assert y.shape == ref.shape == (2, Ho, Wo, Cm) and ps.shape == (2, 4, Cm), (tag, y.shape, ps.shape)
    _chk32(tag, "y", y, ref, 1e-5)
    sums = ref.sum(dim=(1, 2))
    err = (ps.double().sum(1).cpu() - sums).abs().max().item()
    assert err <= 1e-5 * max(1.0, sums.abs().max().item()), (tag, err)


# ======================================================================================================================
# k_warp_fuse<CK, MODE, VEC> (bev_warp.hip): the register-staged fused warp of every feature map with C % 64 != 0
# ======================================================================================================================
WARP_SMALL = ("warp_w2_b2_small", "warp_w4_odd", "warp_w6_degenerate", "warp_w7_tiny")
WARP_CK = {4: (4,), 16: (12, 16), 32: (20, 32)}  # channel counts that take k_warp_fuse<CK, ..>
MODES = ("sum", "mean", "max")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _warp_fixture(name, oracle):
    """Fixture geometry with seeded 32-channel features and the oracle's fused outputs (a C-channel case takes the
    first C channels of both: the warp treats every channel alike)."""
    def make():
        from models.fusion.geometry import GeometryTransformer
        d = np.load(os.path.join(GOLDEN, name + ".npz"))
        B, V, Hf, Wf = (int(d[k]) for k in ("B", "V", "Hf", "Wf"))
        g = GeometryTransformer(int(d["bev_h"]), int(d["bev_w"]), tuple(float(v) for v in d["bounds"]))
        img = (int(d["img_h"]), int(d["img_w"]))
        feats = np.random.default_rng(200 + int(d["seed"])).standard_normal(size=(B, V, 32, Hf, Wf), dtype=np.float32)
        refs = oracle.fused_stream(feats, d["K"], d["Rt"], img, g.bev_h, g.bev_w, g.bounds)
        return g, img, feats, torch.from_numpy(d["K"]).to(DEV), torch.from_numpy(d["Rt"]).to(DEV), refs
    return _cached(("warp", name), make)


WARP_REG = [(ck, m, vec) for ck in (4, 16, 32) for m in (0, 1, 2) for vec in (True, False)]


@pytest.mark.parametrize("ck,m,vec", WARP_REG, ids=[f"k_warp_fuse<{ck},{m},{_tf(vec)}>" for ck, m, vec in WARP_REG])
def test_warp_fuse_register_staged_instances(ck, m, vec, oracle):
    """forward_fused on C = 4 / 12, 16 / 20, 32 channels, channels-last storage (the float4 path, VEC) and plain NCHW
    (the scalar path), sum / mean / max, on the small fixture geometries (B = 2, the odd 97 x 301 map, degenerate
    regions, 1-pixel maps): bit-identical to the oracle."""
    mode = MODES[m]
    for name in WARP_SMALL:
        g, img, feats, K, Rt, refs = _warp_fixture(name, oracle)
        for C in WARP_CK[ck]:
            f = torch.from_numpy(np.ascontiguousarray(feats[:, :, :C])).to(DEV)
            if vec:
                f = f.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)  # channels-last storage
            assert (f.stride(2) == 1) == vec
            got = g.forward_fused(f, K, Rt, img, mode).cpu().numpy()
            ref = refs[mode][:, :C]
            assert got.shape == ref.shape
            assert np.array_equal(_bits(got), _bits(ref)), (name, C, mode, int((_bits(got) != _bits(ref)).sum()))


# ======================================================================================================================
# k_warp_fuse_v2<MODE, 16, false, true, true> (bev_warp.hip): span staging with the channels-last store
# ======================================================================================================================
# The bench rig's cameras (7 views, one frame) over 34 x 60 feature maps and a ragged 61 x 183 map (3 + 11 whole 16 x 16
# tiles and a partial one each way): k_warp_boxes flags 156 / 13 span-staged views of 1344 at BEV_TUNE_WARP_SPAN 100 /
# 50 with a 40 KiB pool and 75 / 20 with 12 KiB: small, and span-staged views at every setting the cases use.
SPAN_BEV, SPAN_FEAT = (61, 183), (34, 60)


def _span_case(oracle):
    def make():
        from bev_rig import rig
        from models.fusion.geometry import GeometryTransformer
        g = GeometryTransformer(SPAN_BEV[0], SPAN_BEV[1], (-24.0, 24.0, -7.2, 7.2))
        K, Rt = rig(7, 1080, 1920, 1)
        feats = np.random.default_rng(47).standard_normal(size=(1, 7, 64) + SPAN_FEAT, dtype=np.float32)
        refs = oracle.fused_stream(feats, K, Rt, (1080, 1920), g.bev_h, g.bev_w, g.bounds)
        f = torch.from_numpy(feats).to(DEV).permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
        Hm, xs, ys, hw = g._sampling(f, torch.from_numpy(K).to(DEV), torch.from_numpy(Rt).to(DEV), (1080, 1920))
        return g, f, Hm, xs, ys, hw, refs
    return _cached("warp-span", make)


def _warp_nhwc_entry(f, Hm, xs, ys, hw, mode, boxes):
    """bev_ipm_warp_fuse_nhwc_f32 itself (warp_fuse(channels_last=True) falls back to the NCHW launch and a copy where
    the entry refuses the pool) -> (rc, out [B, C, Hb, Wb] in channels-last storage)."""
    import bev_native as nat
    B, V, C, Hf, Wf = f.shape
    Hb, Wb = ys.numel(), xs.numel()
    sx, sy = nat._scales(Hf, Wf, hw)
    out = torch.empty(B, Hb, Wb, C, device=DEV).permute(0, 3, 1, 2)
    s = f.stride()
    rc = nat.lib().bev_ipm_warp_fuse_nhwc_f32(nat._ptr(f), s[1], s[2], s[3], s[4], nat._ptr(Hm), nat._ptr(xs),
                                              nat._ptr(ys), B, V, C, Hf, Wf, sx, sy, Hb, Wb, nat.FUSE_MODES[mode],
                                              nat._ptr(out), nat._ptr(boxes), boxes.numel(), 1, nat._stream(f))
    return rc, out


SPAN_CASES = [(m, pool, pct) for m in (0, 1, 2) for pool in (40, 12) for pct in (100, 50)]


@pytest.mark.parametrize("m,pool,pct", SPAN_CASES,
                         ids=[f"k_warp_fuse_v2<{m},16,false,true,true>-pool{p}-span{s}" for m, p, s in SPAN_CASES])
def test_warp_span_staging_channels_last(m, pool, pct, oracle):
    """Span staging (BEV_TUNE_WARP_SPAN 100 / 50) with the channels-last store, C = 64, on a box workspace that flags
    span-staged views (box word bit 30): bit-identical to the oracle, to the same launch with span staging off and to
    the NCHW output.  The NHWC entry keeps its 36 KiB parking area inside the LDS pool (warp_fuse_impl), so it takes
    a 40 KiB pool and refuses the 12 KiB one, where warp_fuse(channels_last=True) runs the NCHW launch and copies --
    that path is held to the same three comparisons."""
    import bev_native as nat
    mode = MODES[m]
    g, f, Hm, xs, ys, hw, refs = _span_case(oracle)
    B, V, C, Hf, Wf = f.shape
    ref = refs[mode]
    nwords = 8 * B * ((g.bev_h + 15) // 16) * ((g.bev_w + 15) // 16) * V
    with nat.tuned(WARP_POOL_KB=pool, WARP_SPAN=pct):
        boxes = nat.warp_fuse_boxes(Hm, xs, ys, B, V, Hf, Wf, hw, mode)
        words = boxes[16:16 + nwords].cpu().numpy().view(np.uint32)
        flagged = int(((words[0::2] >> 30) & 3 == 1).sum())
        rc, cl = _warp_nhwc_entry(f, Hm, xs, ys, hw, mode, boxes)
        if rc != 0:
            cl = nat.warp_fuse(f, Hm, xs, ys, hw, mode, boxes=boxes, channels_last=True)
        nchw = nat.warp_fuse(f, Hm, xs, ys, hw, mode, boxes=boxes)
    with nat.tuned(WARP_POOL_KB=pool, WARP_SPAN=0):
        boxes0 = nat.warp_fuse_boxes(Hm, xs, ys, B, V, Hf, Wf, hw, mode)
        rc0, cl0 = _warp_nhwc_entry(f, Hm, xs, ys, hw, mode, boxes0)
        if rc0 != 0:
            cl0 = nat.warp_fuse(f, Hm, xs, ys, hw, mode, boxes=boxes0, channels_last=True)
    torch.cuda.synchronize()
    print(f"[instance] span staging {mode} pool {pool} KiB span {pct}: {flagged} span-staged views, entry rc {rc}")
    assert flagged > 0, (mode, pool, pct)
    assert rc == rc0 == (0 if pool * 1024 >= 4 * 64 * 36 * 4 else nat.BEV_ERR_ARGS), (rc, rc0)
    assert cl.shape == nchw.shape == ref.shape and cl.is_contiguous(memory_format=torch.channels_last)
    got = cl.cpu().numpy()
    assert np.array_equal(_bits(got), _bits(ref)), (mode, pool, pct, int((_bits(got) != _bits(ref)).sum()))
    assert torch.equal(cl.view(torch.int32), cl0.view(torch.int32))
    assert torch.equal(cl.view(torch.int32), nchw.view(torch.int32))
