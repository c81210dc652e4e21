"""What the training path -- the backward kernels, the BatchNorm / GroupNorm statistics and the reductions -- does with
VALUES the other modules never feed it: channels whose mean is large against their spread, non-finite incoming
gradients, gradients 2^40 / 2^16 / 2^-40 times their unit scale.  (test_train.py, test_head_gpu.py, test_warp_gpu.py
and test_targets.py draw randn at unit scale and judge max|err| against max|ref| over the whole tensor, so one bad
channel hides behind a large one.)  The sibling of test_conv_value_domain_gpu.py, which does the same for the forward.

The reference is always float64 torch on the CPU, never another kernel: autograd of the same operation, or, where
stated, the closed formula evaluated in float64.  Every comparison against a tolerance is per channel (or per group):
never a maximum taken over channels of different scale.

A   Statistics and normalisation off unit scale.
    A1  batchnorm_train_fwd / batchnorm_apply / batchnorm_bwd (+ batchnorm_bwd_half) on [2, 13, 17, 64] (M = 442: one
        row block of 1024), [2, 29, 37, 8] (M = 2146: three row blocks, the last ragged) and [2, 13, 17, 264] (a
        second channel slice past 256).  Channel c has (mean, std) taken cyclically from PAIRS -- up to mean / std =
        4096, std 2^-7 about 8, variance 1e-6 < eps -- plus a channel that is exactly 1000 and one that is 1000 but
        for a single 1001.  Values are drawn in float64 and rounded to fp32 once; the reference is computed from those
        fp32 values.  mean, rstd: rel 1e-6 (test_conv_h16_epilogue_batchnorm_stats' bars at unit scale); scale: rel
        2e-6; shift: 2^-22 (|mean scale| + |beta|); running statistics: rel 1e-5 after one momentum update.
        y, per element: 2^-22 (|z scale| + |shift| + |res|) + 1e-5 |ref| -- five roundings of half an ulp on terms of
        that size, the relative term carries rstd's 1e-6 with room to spare.
        Backward: the test rounds the float64 statistics to fp32 itself (mean32, rstd32, scale32, shift32) and hands
        those to the kernel -- the C ABI takes fp32 statistics, so their rounding belongs to the input -- and the
        reference is the closed formula in float64 from the same values: xhat = (z - mean32) rstd32, u = z scale32 +
        shift32 (+ res), g = dy act'(u), dz = gamma rstd32 (g - mean(g) - xhat mean(g xhat)).  dz, dgamma: 1e-4 of the
        channel's max|ref|; dbeta, dres: 1e-5; batchnorm_bwd_half == the fp32 result rounded to fp16, bit for bit.
        SiLU: act' is evaluated (in float64) at the pre-activation the forward computed, u32 = fp32(fp32(z scale32) +
        shift32) -- the value a SiLU backward reads back (torch saves it in fp32 too); its two roundings, 2^-24 (|z
        scale| + |u|), belong to the forward and are bounded by the y test.  (At a float64 u the constant channel,
        z scale = 1.6e5, is off by 5e-4 of max|dz| and the 4096 / 1 channels by 1e-4: not the backward's error.)
        ReLU decisions: z is built so that no float64 pre-activation (with or without the residual) lies within
        2^-20 (|z scale| + |shift| + |res|) of 0 (nudged before the data is frozen; the two constant channels get
        |beta| = 1.5, gamma 0.5 instead), the kernel's mask is asserted equal to the reference's on every element, and
        no element is excluded from any comparison.  ACT_RELU_MASK needs 256 % (C / 4) == 0, so it is not run at C 264.
    A2  conv2d_nhwc_h16_bnstats + batchnorm_finalize_tiles (per-tile M2, Chan) and batchnorm_train_fwd on the same z:
        x = 8 + randn / 32, positive weights, no padding (a zero border would widen the spread), so mean / std of z
        is in the thousands (asserted > 256 on at least half the channels).  Float64 statistics of the returned z, A1's
        bars.
    A3  groupnorm_fwd / groupnorm_apply / groupnorm_bwd (+ _half) on [2, 9, 15, C], C 128 and 512, 32 groups: group g
        of image n takes PAIRS[(g + n) % 8], one group is constant.  A1's bars; dx 1e-4 per (image, group), dgamma /
        dbeta 1e-4 per channel, the closed formula of bev_head.hip's header comment.
    A4  colsum, channel_sums(x), channel_sums(x, x2), channel_affine: columns randn + mean, M 442 / 4097, C 24 (generic
        kernel) / 128 (v4): test_colsum_sizes' bar 1e-5 sum|x|, per column.
B   Where a non-finite gradient goes.  One element of the incoming gradient is NaN or +Inf, at
      a  the last channel of the last pixel of image 0     b  channel 0 of pixel (0, 0) of image 1
      c  an interior pixel
    (test_conv_instances_gpu.py's small shapes: N 2, 9 x 15 outputs, 17 x 29 inputs at stride 2).  Then
    ~isfinite(got) == ~isfinite(ref) elementwise, the finite elements meet the entry's unit-scale bar taken over the
    finite reference elements, and the reference's set is neither empty nor everything unless the case says so.  The
    torch rules at stake: a ReLU mask is a select (y > 0 ? g : 0), never a multiply (0 * Inf = NaN); max-pool routes to
    the argmax alone.  Weight gradients: the poisoned output channel's dW row is non-finite on every tap whose input
    pixel is inside the image and every other row is finite; taps that fall in the padding for the poisoned pixel are
    NOT asserted either way, because a zero-filled stage may form 0 * Inf -- position c has no such tap, position b
    exercises the exemption.
    Entries: relu_bwd; batchnorm_bwd / _half (batch and frozen statistics, the poison under a closed mask);
    groupnorm_bwd / _half; the three max-pool backward forms; trunk_grad._dgrad's branches and _dgrad_h16; the depthwise
    input gradient; conv_wgrad (WGRAD_MFMA 2 / 1 / 0), conv_wgrad_ex, the scalar weight gradient, conv_wgrad_h16_any,
    dwconv_wgrad, colsum; warp_bwd / warp_fuse_bwd (WARP_BWD_POOL 0 / 96 / 3) and the max-fused backward; view_max_bwd;
    head_operand_bwd / _bias; Proj1x1; the focal loss (also finite extreme logits) and the L1 losses.
C   An overflowing step is skipped: bev_dist.train_step + GradScaler on the small BEVNet of
    test_bevnet_amp_step_matches_reference_fp32_gradients -- scale 2^60 with fp16 convs (skipped, every parameter and
    optimizer state tensor keeps its bits), the same scale in fp32 (taken; unscaled gradients as at scale 1), one +Inf
    in the fused BEV map's gradient at scale 1 (skipped in both modes).
D   Gradient magnitude.  The B entries without poison, the incoming gradient times 2^40, 2^16, 2^-40: the
    deterministic kernels return exactly that power of two times their unit-scale result (torch.equal) -- derived, not
    measured: a power of two commutes with every rounding while nothing leaves the normal range; the kernels that add
    with float atomics (weight gradients, colsum, the warp and max-fused backward, Proj1x1's dW / db, the head
    operand's bias gradient) meet their unit-scale bar relative to the scaled reference.  The losses' backward takes
    the factor through grad_loss, where GradScaler's scale enters the native path.  conv_wgrad_h16_any and _dgrad_h16:
    2^4 and 2^-4 on an fp32-stored gradient.
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
EPS, MOM = 1e-5, 0.1
PAIRS = [(0.0, 1.0), (16.0, 1.0), (256.0, 1.0), (1024.0, 1.0), (4096.0, 1.0), (-1024.0, 1.0), (8.0, 2.0 ** -7),
         (1.0, 1e-3)]
PAIR_IDS = ["0/1", "16/1", "256/1", "1024/1", "4096/1", "-1024/1", "8/2^-7", "1/1e-3", "const", "const+1"]


def _cached(key, make):
    """Inputs and references are made once and shared (never modified)."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _d(t):
    return t.detach().cpu().double()


def _pos(shape, pos):
    """Index (n, h, w, c) of poison position a / b / c in an NHWC shape."""
    _, H, W, C = shape
    return {"a": (0, H - 1, W - 1, C - 1), "b": (1, 0, 0, 0), "c": (0, H // 2, W // 2, C // 2)}[pos]


def _rel(tag, what, got, ref, bar, groups=None):
    """|got - ref| <= bar |ref| elementwise (a per-channel quantity); prints the worst ratio, per PAIRS entry if the
    channels' entries are given."""
    got, ref = _d(got), _d(ref)
    err = (got - ref).abs() / ref.abs().clamp_min(1e-300)
    if groups is not None:
        worst = {PAIR_IDS[k]: float(err.reshape(-1)[groups.reshape(-1) == k].max()) for k in groups.unique().tolist()}
        print(f"[grad] {tag} {what}: worst rel err per offset " + ", ".join(f"{k}: {v:.1e}" for k, v in worst.items()))
    else:
        print(f"[grad] {tag} {what}: worst rel err {float(err.max()):.2e} (bar {bar:.0e})")
    assert bool(((got - ref).abs() <= bar * ref.abs()).all()), (tag, what, float(err.max()), int(err.argmax()))


def _bound(tag, what, got, ref, bound, groups=None):
    got, ref = _d(got), _d(ref)
    assert got.shape == ref.shape, (tag, what, got.shape, ref.shape)
    err = (got - ref).abs()
    assert bool(torch.isfinite(got).all()), (tag, what, "non-finite")
    ratio = err / bound.clamp_min(1e-300)
    if groups is not None:
        worst = {PAIR_IDS[k]: float(ratio.reshape(-1)[groups.reshape(-1) == k].max()) for k in groups.unique().tolist()}
        print(f"[grad] {tag} {what}: max err / bound per offset "
              + ", ".join(f"{k}: {v:.3f}" for k, v in worst.items()))
    print(f"[grad] {tag} {what}: max err / bound {float(ratio.max()):.3f}")
    assert bool((err <= bound).all()), (tag, what, float(ratio.max()), int(ratio.argmax()))


def _per(tag, what, got, ref, bar, dims, groups=None):
    """max over `dims` of |got - ref| <= bar max over `dims` of |ref|: one comparison per channel (or group)."""
    got, ref = _d(got), _d(ref)
    assert got.shape == ref.shape, (tag, what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), (tag, what, "non-finite")
    err, scale = (got - ref).abs(), ref.abs()
    if dims:
        err, scale = err.amax(dims), scale.amax(dims)
    ratio = err / scale.clamp_min(1e-300)
    ratio[(scale == 0) & (err == 0)] = 0.0
    if groups is not None:
        worst = {PAIR_IDS[k]: float(ratio.reshape(-1)[groups.reshape(-1) == k].max()) for k in groups.unique().tolist()}
        print(f"[grad] {tag} {what} (bar {bar:.0e}): worst per offset " + ", ".join(f"{k}: {v:.1e}"
                                                                                      for k, v in worst.items()))
    else:
        print(f"[grad] {tag} {what}: worst err / max|ref| {float(ratio.max()):.2e} (bar {bar:.0e})")
    assert bool((err <= bar * scale).all()), (tag, what, float(ratio.max()), int(ratio.argmax()))
    return float(ratio.max())


def _act64(u, act):
    if act == 1:
        return u.clamp_min(0)
    if act == 2:
        return u * torch.sigmoid(u)
    return u


def _dact64(u, act):
    """act'(u) as the factor of the incoming gradient (ReLU: a 0 / 1 mask, applied as a select by the callers)."""
    if act == 2:
        s = torch.sigmoid(u)
        return s * (1 + u * (1 - s))
    return torch.ones_like(u)


# ======================================================================================================================
# A1: BatchNorm off unit scale
# ======================================================================================================================
BN_SHAPES = {"m442-c64": ((2, 13, 17, 64), 0), "m2146-c8": ((2, 29, 37, 8), 2), "m442-c264": ((2, 13, 17, 264), 0)}


def _stats64(zd, gamma, beta, dims):
    """float64 (mean, biased var, rstd, scale, shift) over `dims`, kept broadcastable against zd."""
    mean = zd.mean(dims, keepdim=True)
    var = ((zd - mean) ** 2).mean(dims, keepdim=True)
    rstd = 1 / torch.sqrt(var + EPS)
    scale = gamma.double() * rstd
    return mean, var, rstd, scale, beta.double() - mean * scale


def _nudge(z64, res, gamma, beta, dims, free):
    """Move the elements of z64 (where `free`) until no float64 pre-activation -- z scale + shift and the same plus
    res, with the float64 statistics and with their fp32 roundings -- lies within 2^-20 (|z scale| + |shift| + |res|)
    of 0.  -> the fp32 tensor."""
    for _ in range(40):
        z = z64.float()
        zd = z.double()
        _, _, _, sc, sh = _stats64(zd, gamma, beta, dims)
        sc32, sh32 = sc.float().double(), sh.float().double()
        margin = 2.0 ** -20 * ((zd * sc).abs() + sh.abs() + res.double().abs())
        pre = [zd * sc + sh, zd * sc32 + sh32]
        pre += [p + res.double() for p in pre]
        bad = torch.zeros_like(zd, dtype=torch.bool)
        move = torch.zeros_like(zd)
        for p in pre:
            b = (p.abs() < margin) & ~bad
            sign = torch.where(p < 0, -1.0, 1.0).double()
            move = torch.where(b, (sign * 4 * margin - p) / sc, move)
            bad |= b
        if not bool(bad.any()):
            return z
        assert not bool((bad & ~free).any()), "a fixed element sits on the ReLU kink"
        z64 = zd + move
    raise AssertionError("the ReLU nudge did not converge")


def _bn_case(key):
    def make():
        (n, h, w, C), off = BN_SHAPES[key]
        M = n * h * w
        g = _gen(6000 + C + M)
        c = types.SimpleNamespace(shape=(n, h, w, C), M=M, C=C)
        pair = torch.tensor([(k + off) % 8 for k in range(C - 2)] + [8, 9])
        m = torch.tensor([PAIRS[k][0] for k in pair[:-2].tolist()] + [1000.0, 1000.0], dtype=torch.float64)
        s = torch.tensor([PAIRS[k][1] for k in pair[:-2].tolist()] + [0.0, 0.0], dtype=torch.float64)
        z64 = m + s * torch.randn(M, C, generator=g, dtype=torch.float64)
        z64[M // 3, C - 1] = 1001.0
        c.gamma, c.beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.5
        c.gamma[C - 2:] = 0.5
        c.beta[C - 2], c.beta[C - 1] = 1.5, -1.5
        c.res = torch.randn(M, C, generator=g)
        c.res[:, C - 2:] = c.res[:, C - 2:].clamp(-0.9, 0.9)  # |beta + res| >= 0.6: twice the constant channel's margin
        free = torch.ones(M, C, dtype=torch.bool)
        free[:, C - 2:] = False
        c.z = _nudge(z64, c.res, c.gamma, c.beta, (0,), free)
        assert bool((c.z[:, C - 2] == 1000).all()) and int((c.z[:, C - 1] != 1000).sum()) == 1
        c.pair = pair
        c.zd = c.z.double()
        c.mean, c.var, c.rstd, c.scale, c.shift = (t.reshape(C) for t in _stats64(c.zd, c.gamma, c.beta, (0,)))
        ratio = c.mean.abs() / c.var.sqrt().clamp_min(1e-30)
        for k, want in ((2, 256), (3, 1024), (4, 4096)):
            if bool((pair == k).any()):
                assert float(ratio[pair == k].min()) > 0.9 * want
        c.dy = torch.randn(M, C, generator=g)
        c.rm0, c.rv0 = torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) + 0.5
        c.dev = types.SimpleNamespace(**{k: getattr(c, k).to(DEV) for k in ("gamma", "beta", "res", "dy")})
        c.dev.z = c.z.reshape(n, h, w, C).to(DEV)
        c.dev.res, c.dev.dy = c.dev.res.reshape(n, h, w, C), c.dev.dy.reshape(n, h, w, C)
        # the statistics the test hands to the backward: fp32 roundings of the float64 values
        c.mean32, c.rstd32, c.scale32, c.shift32 = (t.float() for t in (c.mean, c.rstd, c.scale, c.shift))
        for k in ("mean32", "rstd32", "scale32", "shift32"):
            setattr(c.dev, k, getattr(c, k).to(DEV))
        return c
    return _cached(("bn", key), make)


def _bn_kernel_stats(key):
    """batchnorm_train_fwd's outputs for a case, computed once."""
    import bev_native as nat

    def make():
        c = _bn_case(key)
        rm, rv = c.rm0.to(DEV), c.rv0.to(DEV)
        out = nat.batchnorm_train_fwd(c.dev.z, c.dev.gamma, c.dev.beta, rm, rv, EPS, MOM)
        torch.cuda.synchronize()
        return out + (rm, rv)
    return _cached(("bn-stats", key), make)


def _check_stats(tag, c, got, M, pair=None):
    """A1's bars on (mean, rstd, scale, shift, running_mean, running_var) against the float64 statistics in c."""
    mean, rstd, scale, shift, rm, rv = got
    _rel(tag, "mean", mean, c.mean, 1e-6, pair)
    _rel(tag, "rstd", rstd, c.rstd, 1e-6, pair)
    _rel(tag, "scale", scale, c.scale, 2e-6, pair)
    _bound(tag, "shift", shift, c.shift, 2.0 ** -22 * ((c.mean * c.scale).abs() + c.beta.double().abs()))
    _rel(tag, "running_mean", rm, (1 - MOM) * c.rm0.double() + MOM * c.mean, 1e-5)
    _rel(tag, "running_var", rv, (1 - MOM) * c.rv0.double() + MOM * c.var * M / (M - 1), 1e-5)


@pytest.mark.parametrize("key", list(BN_SHAPES))
def test_batchnorm_statistics_off_unit_scale(key):
    """batchnorm_train_fwd: A1's bars per channel; the constant channel's rstd is 1 / sqrt(eps)."""
    c = _bn_case(key)
    got = _bn_kernel_stats(key)
    _check_stats(f"bn-stats-{key}", c, got, c.M, c.pair)
    const = float(got[1][c.C - 2])
    assert abs(const - EPS ** -0.5) <= 1e-6 * EPS ** -0.5, const


@pytest.mark.parametrize("res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("act", [0, 1, 2], ids=["none", "relu", "silu"])
@pytest.mark.parametrize("key", list(BN_SHAPES))
def test_batchnorm_apply_off_unit_scale(key, act, res):
    """batchnorm_apply over batchnorm_train_fwd's own scale / shift against float64 act(z scale + shift (+ res)) from
    the float64 statistics, per element; ReLU: the kernel's mask equals the reference's everywhere; the constant
    channel gives act(beta (+ res))."""
    import bev_native as nat
    c = _bn_case(key)
    _, _, scale, shift, _, _ = _bn_kernel_stats(key)
    y = nat.batchnorm_apply(c.dev.z, scale, shift, c.dev.res if res else None, act)
    torch.cuda.synchronize()
    r = c.res.double() if res else torch.zeros_like(c.zd)
    u = c.zd * c.scale + c.shift + r
    ref = _act64(u, act)
    bound = 2.0 ** -22 * ((c.zd * c.scale).abs() + c.shift.abs() + r.abs()) + 1e-5 * ref.abs()
    yd = _d(y).reshape(c.M, c.C)
    if act == 1:
        assert torch.equal(yd > 0, u > 0), int(((yd > 0) != (u > 0)).sum())
    _bound(f"bn-apply-{key}-act{act}-res{int(res)}", "y", yd, ref, bound, c.pair.expand(c.M, c.C))
    want = _act64(c.beta[c.C - 2].double() + r[:, c.C - 2], act)
    assert bool(((yd[:, c.C - 2] - want).abs() <= bound[:, c.C - 2]).all())


BN_BWD = {"none-res": (0, True, False), "relu-res": (1, True, False), "silu": (2, False, False),
          "relu-from-z": (3, False, False), "relu-mask-res": (4, True, False), "relu-res-frozen": (1, True, True),
          "silu-frozen": (2, False, True), "none-frozen": (0, False, True)}
BN_BWD_CASES = [(k, m) for k in BN_SHAPES for m in BN_BWD if not (m == "relu-mask-res" and k == "m442-c264")]


def _bn_bwd_ref(zd, dy, res, mean, rstd, scale, shift, gamma, act, frozen, dims=(0,)):
    """The closed formula in float64 -> (dz, dres (= g), dgamma, dbeta, mask or None)."""
    u = zd * scale + shift + (res if res is not None else 0.0)
    mask = None
    if act in (1, 3, 4):
        mask = u > 0
        g = torch.where(mask, dy, torch.zeros_like(dy))  # a select: a closed mask stops NaN / Inf
    else:
        u32 = ((zd.float() * scale.float()) + shift.float()).double() if act == 2 else u  # two fp32 roundings, no fma
        g = dy * _dact64(u32, act)
    xh = (zd - mean) * rstd
    k1 = torch.zeros_like(mean) if frozen else g.mean(dims, keepdim=True)
    k2 = torch.zeros_like(mean) if frozen else (g * xh).mean(dims, keepdim=True)
    dz = gamma * rstd * (g - k1 - xh * k2)
    return dz, g, (g * xh).sum(dims), g.sum(dims), mask


def _bn_bwd_run(nat, dy, z, res, mean32, rstd32, scale32, shift32, gamma, act, frozen, half):
    """The native backward as the trunk calls it -> (dz, dres, dgamma, dbeta, the forward's ReLU mask or None)."""
    yarg, mask = None, None
    if act in (1, 3):
        y = nat.batchnorm_apply(z, scale32, shift32, res, 1)
        mask = y > 0
        yarg = y if act == 1 else None  # act 3 recomputes the mask with batchnorm_apply's own expression
    elif act == 4:
        y, yarg = nat.batchnorm_apply_mask(z, scale32, shift32, res)
        mask = ((yarg.int()[:, None] >> torch.arange(4, device=DEV)) & 1).bool().reshape(z.shape)
        assert torch.equal(mask, y > 0)
    if act == 4 and not half:  # the mask bytes are read by the fp16-storing entry only; bit-identical to act 1
        yarg, act = y, 1
    fn = nat.batchnorm_bwd_half if half else nat.batchnorm_bwd
    out = fn(dy, yarg, z, mean32, rstd32, gamma, res is not None, act, scale32, shift32, frozen)
    torch.cuda.synchronize()
    return out + (mask,)


@pytest.mark.parametrize("key,mode", BN_BWD_CASES, ids=[f"{k}-{m}" for k, m in BN_BWD_CASES])
def test_batchnorm_bwd_off_unit_scale(key, mode):
    """batchnorm_bwd / batchnorm_bwd_half from the test's own fp32 statistics against the closed formula in float64;
    per-channel bars; the constant channel's dz is finite; frozen: the statistics are constants.  ACT_RELU_MASK is
    taken by batchnorm_bwd_half alone (the fp32 wrapper takes y): its fp16 dz must be the rounding of the fp32 dz of
    ACT_RELU over the same mask, its dres / dgamma / dbeta meet the bars themselves."""
    import bev_native as nat
    act, with_res, frozen = BN_BWD[mode]
    c = _bn_case(key)
    tag = f"bn-bwd-{key}-{mode}"
    d = c.dev
    res = d.res if with_res else None
    dz, dres, dg, db, mask = _bn_bwd_run(nat, d.dy, d.z, res, d.mean32, d.rstd32, d.scale32, d.shift32, d.gamma, act,
                                         frozen, False)
    h = _bn_bwd_run(nat, d.dy, d.z, res, d.mean32, d.rstd32, d.scale32, d.shift32, d.gamma, act, frozen, True)
    dz16 = h[0]
    if act == 4:  # the mask-byte form's own residual gradient, dgamma and dbeta are the ones judged
        dres, dg, db = h[1:4]
    rdz, rg, rdg, rdb, rmask = _bn_bwd_ref(c.zd, c.dy.double(), c.res.double() if with_res else None,
                                           c.mean32.double(), c.rstd32.double(), c.scale32.double(),
                                           c.shift32.double(), c.gamma.double(), act, frozen)
    if rmask is not None:
        assert torch.equal(mask.cpu().reshape(c.M, c.C), rmask), int((mask.cpu().reshape(c.M, c.C) != rmask).sum())
    pair = c.pair
    _per(tag, "dz", dz.reshape(c.M, c.C), rdz, 1e-4, (0,), pair)
    _per(tag, "dgamma", dg, rdg, 1e-4, None, pair)
    _per(tag, "dbeta", db, rdb, 1e-5, None, pair)
    if with_res:
        _per(tag, "dres", dres.reshape(c.M, c.C), rg, 1e-5, (0,), pair)
    assert bool(torch.isfinite(dz[..., c.C - 2]).all())
    assert torch.equal(dz16.view(torch.int16), dz.half().view(torch.int16)), int((dz16 != dz.half()).sum())


# ======================================================================================================================
# A2: the conv epilogue's tile statistics
# ======================================================================================================================
@pytest.mark.parametrize("stride", [1, 2])
def test_batchnorm_finalize_tiles_off_unit_scale(stride):
    """conv2d_nhwc_h16_bnstats + batchnorm_finalize_tiles, and batchnorm_train_fwd on the same z, against the float64
    statistics of the returned z (mean / std in the thousands): A1's bars for both."""
    import bev_native as nat
    g = _gen(6100 + stride)
    Ci, Co = 64, 128
    x = 8 + torch.randn(N, 17, 26, Ci, generator=g) / 32
    w = (torch.rand(Co, 1, 1, 1, generator=g) * 0.75 + 0.25 + 0.1 * torch.randn(Co, Ci, 3, 3, generator=g)) / 24
    c = types.SimpleNamespace()
    c.gamma, c.beta = torch.rand(Co, generator=g) + 0.5, torch.randn(Co, generator=g) * 0.5
    c.rm0, c.rv0 = torch.rand(Co, generator=g) + 0.5, torch.rand(Co, generator=g) + 0.5
    z, tiles = nat.conv2d_nhwc_h16_bnstats(x.to(DEV), nat.pack_conv_weight_h16(w.to(DEV)), Co, 3, 3, stride, 0)
    M = z.numel() // Co
    assert tiles.shape[1] > 1 and M % 128 != 0  # several tiles, the last ragged
    zd = _d(z).reshape(M, Co)
    c.mean, c.var, c.rstd, c.scale, c.shift = (t.reshape(Co) for t in _stats64(zd, c.gamma, c.beta, (0,)))
    ratio = c.mean.abs() / c.var.sqrt()
    print(f"[grad] bn-tiles-s{stride}: mean / std of z in [{float(ratio.min()):.0f}, {float(ratio.max()):.0f}]")
    assert int((ratio > 256).sum()) >= Co // 2
    gd, bd = c.gamma.to(DEV), c.beta.to(DEV)
    for name in ("tiles", "train_fwd"):
        rm, rv = c.rm0.to(DEV), c.rv0.to(DEV)
        if name == "tiles":
            out = nat.batchnorm_finalize_tiles(tiles, M, gd, bd, rm, rv, EPS, MOM)
        else:
            out = nat.batchnorm_train_fwd(z, gd, bd, rm, rv, EPS, MOM)
        torch.cuda.synchronize()
        _check_stats(f"bn-{name}-s{stride}", c, out + (rm, rv), M)


# ======================================================================================================================
# A3: GroupNorm off unit scale
# ======================================================================================================================
GN_G = 32  # the head's group count


def _gn_case(C):
    def make():
        g = _gen(6200 + C)
        P, cpg = HO * WO, C // GN_G
        c = types.SimpleNamespace(C=C, P=P, cpg=cpg)
        pair = torch.tensor([[(k + n) % 8 for k in range(GN_G)] for n in range(N)])
        pair[0, 5] = 8  # the constant group
        c.pair = pair
        m = torch.tensor([[PAIRS[k][0] if k < 8 else 1000.0 for k in row] for row in pair.tolist()],
                         dtype=torch.float64)
        s = torch.tensor([[PAIRS[k][1] if k < 8 else 0.0 for k in row] for row in pair.tolist()], dtype=torch.float64)
        x64 = m[:, None, :, None] + s[:, None, :, None] * torch.randn(N, P, GN_G, cpg, generator=g,
                                                                         dtype=torch.float64)
        c.gamma, c.beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.5
        lo, hi = 5 * cpg, 6 * cpg  # the constant group's channels (image 1 has a random group there)
        c.gamma[lo:hi] = 0.5
        c.beta[lo:hi] = torch.tensor([1.5, -1.5] * (cpg // 2))
        c.res = torch.zeros(N, P, GN_G, cpg)
        free = torch.ones(N, P, GN_G, cpg, dtype=torch.bool)
        free[0, :, 5] = False
        ga, be = c.gamma.reshape(GN_G, cpg), c.beta.reshape(GN_G, cpg)
        c.x = _nudge(x64, c.res, ga, be, (1, 3), free)
        assert bool((c.x[0, :, 5] == 1000).all())
        c.xd = c.x.double()
        c.mean, c.var, c.rstd, c.scale, c.shift = _stats64(c.xd, ga, be, (1, 3))
        c.dy = torch.randn(N, P, GN_G, cpg, generator=g)
        c.mean32, c.rstd32, c.scale32, c.shift32 = (t.float() for t in (c.mean, c.rstd, c.scale, c.shift))
        c.dev = types.SimpleNamespace(
            x=c.x.reshape(N, HO, WO, C).to(DEV), dy=c.dy.reshape(N, HO, WO, C).to(DEV), gamma=c.gamma.to(DEV),
            beta=c.beta.to(DEV), mean32=c.mean32.reshape(N, GN_G).to(DEV), rstd32=c.rstd32.reshape(N, GN_G).to(DEV),
            scale32=c.scale32.reshape(N, C).to(DEV), shift32=c.shift32.reshape(N, C).to(DEV))
        return c
    return _cached(("gn", C), make)


@pytest.mark.parametrize("C", [128, 512])
def test_groupnorm_fwd_off_unit_scale(C):
    """groupnorm_fwd's (mean, rstd, scale, shift) and groupnorm_apply (with and without ReLU) over them: A1's bars."""
    import bev_native as nat
    c = _gn_case(C)
    tag = f"gn-fwd-c{C}"
    mean, rstd, scale, shift = nat.groupnorm_fwd(c.dev.x, GN_G, c.dev.gamma, c.dev.beta, EPS)
    torch.cuda.synchronize()
    _rel(tag, "mean", mean, c.mean.reshape(N, GN_G), 1e-6, c.pair)
    _rel(tag, "rstd", rstd, c.rstd.reshape(N, GN_G), 1e-6, c.pair)
    _rel(tag, "scale", scale, c.scale.reshape(N, C), 2e-6)
    _bound(tag, "shift", shift, c.shift.reshape(N, C),
           2.0 ** -22 * ((c.mean * c.scale).abs() + c.beta.reshape(GN_G, c.cpg).double().abs()).reshape(N, C))
    assert abs(float(rstd[0, 5]) - EPS ** -0.5) <= 1e-6 * EPS ** -0.5
    u = c.xd * c.scale + c.shift
    for relu in (False, True):
        y = _d(nat.groupnorm_apply(c.dev.x, scale, shift, relu)).reshape(u.shape)
        ref = u.clamp_min(0) if relu else u
        if relu:
            assert torch.equal(y > 0, u > 0), int(((y > 0) != (u > 0)).sum())
        bound = 2.0 ** -22 * ((c.xd * c.scale).abs() + c.shift.abs()) + 1e-5 * ref.abs()
        _bound(tag, f"y relu={int(relu)}", y, ref, bound, c.pair[:, None, :, None].expand(u.shape))


def _gn_bwd_ref(xd, dy, mean, rstd, scale, shift, gamma, relu):
    """bev_head.hip's header formula in float64 on [N, P, G, cpg] -> (dx, dgamma [G, cpg], dbeta [G, cpg])."""
    u = xd * scale + shift
    g = torch.where(u > 0, dy, torch.zeros_like(dy)) if relu else dy
    xh = (xd - mean) * rstd
    gg = g * gamma
    dx = rstd * (gg - gg.mean((1, 3), keepdim=True) - xh * (gg * xh).mean((1, 3), keepdim=True))
    return dx, (g * xh).sum((0, 1)), g.sum((0, 1))


@pytest.mark.parametrize("relu", [False, True], ids=["none", "relu"])
@pytest.mark.parametrize("C", [128, 512])
def test_groupnorm_bwd_off_unit_scale(C, relu):
    """groupnorm_bwd / groupnorm_bwd_half from the test's own fp32 statistics: dx 1e-4 per (image, group), dgamma /
    dbeta 1e-4 per channel; the fp16 form is the fp32 result rounded."""
    import bev_native as nat
    c = _gn_case(C)
    d = c.dev
    tag = f"gn-bwd-c{C}-relu{int(relu)}"
    dx, dg, db = nat.groupnorm_bwd(d.x, d.dy, GN_G, d.mean32, d.rstd32, d.gamma, d.scale32, d.shift32, relu)
    dx16 = nat.groupnorm_bwd_half(d.x, d.dy, GN_G, d.mean32, d.rstd32, d.gamma, d.scale32, d.shift32, relu)[0]
    torch.cuda.synchronize()
    rdx, rdg, rdb = _gn_bwd_ref(c.xd, c.dy.double(), c.mean32.double(), c.rstd32.double(), c.scale32.double(),
                                c.shift32.double(), c.gamma.reshape(GN_G, c.cpg).double(), relu)
    _per(tag, "dx", dx.reshape(rdx.shape), rdx, 1e-4, (1, 3), c.pair)
    _per(tag, "dgamma", dg.reshape(GN_G, c.cpg), rdg, 1e-4, None)
    _per(tag, "dbeta", db.reshape(GN_G, c.cpg), rdb, 1e-4, None)
    assert torch.equal(dx16.view(torch.int16), dx.half().view(torch.int16)), int((dx16 != dx.half()).sum())


# ======================================================================================================================
# A4: the reductions
# ======================================================================================================================
@pytest.mark.parametrize("C", [24, 128], ids=["c24-generic", "c128-v4"])
@pytest.mark.parametrize("M", [442, 4097])
def test_reductions_off_unit_scale(M, C):
    """colsum, channel_sums(x), channel_sums(x, x2), channel_affine(x, a[, b]) on columns randn + PAIRS mean: 1e-5 of
    the column's own sum of |terms|; channel_affine per element within 2^-23 (|x a| + |b|) (two roundings)."""
    import bev_native as nat
    g = _gen(6300 + M + C)
    m = torch.tensor([PAIRS[k % 8][0] for k in range(C)])
    x = torch.randn(M, C, generator=g) + m
    x2 = torch.randn(M, C, generator=g) + m.roll(3)
    a, b = torch.randn(1, C, generator=g) + 2, torch.randn(1, C, generator=g) * 100
    xd, x2d = x.to(DEV), x2.to(DEV)
    x4, x24 = xd.reshape(1, M, 1, C), x2d.reshape(1, M, 1, C)
    tag = f"reduce-m{M}-c{C}"
    _bound(tag, "colsum", nat.colsum(xd), x.double().sum(0), 1e-5 * x.double().abs().sum(0))
    _bound(tag, "channel_sums", nat.channel_sums(x4)[0], x.double().sum(0), 1e-5 * x.double().abs().sum(0))
    prod = x.double() * x2.double()
    _bound(tag, "channel_sums x2", nat.channel_sums(x4, x24)[0], prod.sum(0), 1e-5 * prod.abs().sum(0))
    xa = x.double() * a.double()
    _bound(tag, "channel_affine", nat.channel_affine(x4, a.to(DEV)).reshape(M, C), xa, 2.0 ** -23 * xa.abs())
    _bound(tag, "channel_affine b", nat.channel_affine(x4, a.to(DEV), b.to(DEV)).reshape(M, C), xa + b.double(),
           2.0 ** -23 * (xa.abs() + b.double().abs()))


# ======================================================================================================================
# B: where a non-finite gradient goes.  Each entry: run(dy on the device) -> tuple of outputs, ref(dy float64 CPU) ->
# tuple of float64 references; dy is the incoming gradient [N, h, w, C] (NHWC), poisoned by the caller.
# ======================================================================================================================
def _sets(tag, what, got, ref, bar, expect="some", bound=None):
    """B's assertions on one output: equal non-finite sets, the finite elements within bar max|finite ref| (or the
    per-element bound).  expect "some": the reference's set is neither empty nor everything; "none": it is empty."""
    got = _d(got)
    assert got.shape == ref.shape, (tag, what, got.shape, ref.shape)
    nf, g = ~torch.isfinite(ref), ~torch.isfinite(got)
    if expect == "none":
        assert not bool(nf.any()), (tag, what, "the reference is not finite")
    elif expect == "some":
        assert bool(nf.any()) and not bool(nf.all()), (tag, what, "the poison is not in play", int(nf.sum()))
    assert torch.equal(g, nf), (tag, what, "non-finite set", int(g.sum()), int(nf.sum()),
                                (g != nf).nonzero()[:4].tolist())
    fin = ~nf
    err = (got - ref).abs()
    if bound is not None:
        worst = float((err[fin] / bound[fin].clamp_min(1e-300)).max())
        assert bool((err[fin] <= bound[fin]).all()), (tag, what, worst)
    else:
        scale = float(ref[fin].abs().max())
        worst = float(err[fin].max()) / max(scale, 1e-300)
        assert float(err[fin].max()) <= bar * scale, (tag, what, worst)
    print(f"[grad] {tag} {what}: {int(nf.sum())} non-finite, finite err {worst:.2e} of the bar's scale")
    return nf


def _poisoned(dy, pos, val):
    dy = dy.clone()
    dy[_pos(dy.shape, pos)] = val
    return dy


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ---- relu_bwd ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", ["nan", "inf"])
@pytest.mark.parametrize("pos", ["a", "b", "c"])
@pytest.mark.parametrize("gate", ["open", "closed"])
def test_relu_bwd_poison(gate, pos, poison):
    """relu_bwd: the poison where y > 0 comes out on exactly that element; where y == 0 everything is finite and
    that element is exactly 0 (a select, not dy * mask).  Exact (bar 0)."""
    import bev_native as nat
    g = _gen(7000)
    y = torch.randn(N, HO, WO, 64, generator=g).clamp_min(0)
    dy = _poisoned(torch.randn(N, HO, WO, 64, generator=g), pos, POISON[poison])
    y[_pos(y.shape, pos)] = 1.0 if gate == "open" else 0.0
    got = nat.relu_bwd(dy.to(DEV), y.to(DEV))
    torch.cuda.synchronize()
    ref = torch.where(y > 0, dy, torch.zeros_like(dy)).double()
    nf = _sets(f"relu_bwd-{gate}-{pos}-{poison}", "dz", got, ref, 0.0, "some" if gate == "open" else "none")
    assert int(nf.sum()) == (1 if gate == "open" else 0)
    if gate == "closed":
        assert float(got[_pos(y.shape, pos)]) == 0.0


# ---- batchnorm_bwd -------------------------------------------------------------------------------------------------
def _bnb_case(pos, gate):
    """Unit-scale BatchNorm operands [2, 9, 15, 64] whose element at `pos` has pre-activation > 0 (open) or < 0."""
    def make():
        g = _gen(7100)
        C, M = 64, N * HO * WO
        c = types.SimpleNamespace(C=C, M=M, shape=(N, HO, WO, C))
        z64 = (2 * torch.randn(N, HO, WO, C, generator=g) + 0.5).double()
        c.gamma, c.beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
        c.res = torch.randn(N, HO, WO, C, generator=g)
        at = _pos(z64.shape, pos)
        z64[at] = 8.0 if gate == "open" else -8.0
        c.res[at] = 0.0
        free = torch.ones_like(z64, dtype=torch.bool)
        free[at] = False
        c.z = _nudge(z64.reshape(M, C), c.res.reshape(M, C), c.gamma, c.beta, (0,), free.reshape(M, C))
        c.zd = c.z.double()
        st = [t.reshape(C) for t in _stats64(c.zd, c.gamma, c.beta, (0,))]
        c.mean32, c.rstd32, c.scale32, c.shift32 = st[0].float(), st[2].float(), st[3].float(), st[4].float()
        c.dy = torch.randn(N, HO, WO, C, generator=g)
        c.dev = types.SimpleNamespace(z=c.z.reshape(c.shape).to(DEV), res=c.res.to(DEV), gamma=c.gamma.to(DEV),
                                      **{k: getattr(c, k).to(DEV) for k in ("mean32", "rstd32", "scale32", "shift32")})
        return c
    return _cached(("bnb", pos, gate), make)


def _bnb_run(c, dy, act, with_res, frozen, half):
    import bev_native as nat
    d = c.dev
    return _bn_bwd_run(nat, dy.to(DEV), d.z, d.res if with_res else None, d.mean32, d.rstd32, d.scale32, d.shift32,
                       d.gamma, act, frozen, half)


def _bnb_ref(c, dy, act, with_res, frozen):
    return _bn_bwd_ref(c.zd, dy.double().reshape(c.M, c.C), c.res.double().reshape(c.M, c.C) if with_res else None,
                       c.mean32.double(), c.rstd32.double(), c.scale32.double(), c.shift32.double(), c.gamma.double(),
                       act, frozen)


BNB_ACTS = {"none": (0, True), "relu": (1, True), "silu": (2, False), "relu-from-z": (3, False),
            "relu-mask": (4, True)}


def _bnb_check(tag, c, dy, act, with_res, frozen, expect):
    dz, dres, dg, db, _ = _bnb_run(c, dy, act, with_res, frozen, False)
    h = _bnb_run(c, dy, act, with_res, frozen, True)
    if act == 4:
        dres, dg, db = h[1:4]
    rdz, rg, rdg, rdb, _ = _bnb_ref(c, dy, act, with_res, frozen)
    sets = {"dz": _sets(tag, "dz", dz.reshape(c.M, c.C), rdz, 1e-4, expect),
            "dgamma": _sets(tag, "dgamma", dg, rdg, 1e-4, expect), "dbeta": _sets(tag, "dbeta", db, rdb, 1e-5, expect)}
    if with_res:
        sets["dres"] = _sets(tag, "dres", dres.reshape(c.M, c.C), rg, 1e-5, expect)
    dz16, want = h[0].reshape(c.M, c.C).cpu(), dz.half().reshape(c.M, c.C).cpu()
    assert torch.equal(~torch.isfinite(dz16), sets["dz"]), (tag, "fp16 dz: non-finite set")
    assert torch.equal(dz16[~sets["dz"]], want[~sets["dz"]]), (tag, "fp16 dz != the fp32 dz rounded")
    return sets


@pytest.mark.parametrize("poison", ["nan", "inf"])
@pytest.mark.parametrize("pos", ["a", "b", "c"])
@pytest.mark.parametrize("act", list(BNB_ACTS))
def test_batchnorm_bwd_poison(act, pos, poison):
    """batchnorm_bwd / _half with batch statistics, the poison under an open mask: the poisoned channel's dz, dgamma
    and dbeta are non-finite throughout, every other channel is finite, dres is non-finite on the one element."""
    a, with_res = BNB_ACTS[act]
    c = _bnb_case(pos, "open")
    ch = _pos(c.shape, pos)[3]
    sets = _bnb_check(f"bn-bwd-{act}-{pos}-{poison}", c, _poisoned(c.dy, pos, POISON[poison]), a, with_res, False,
                      "some")
    col = torch.zeros(c.M, c.C, dtype=torch.bool)
    col[:, ch] = True
    assert torch.equal(sets["dz"], col)
    assert torch.equal(sets["dgamma"], col[0]) and torch.equal(sets["dbeta"], col[0])
    if with_res:
        assert int(sets["dres"].sum()) == 1


@pytest.mark.parametrize("poison", ["nan", "inf"])
@pytest.mark.parametrize("pos", ["a", "b", "c"])
@pytest.mark.parametrize("act", ["none", "relu", "silu"])
def test_batchnorm_bwd_frozen_poison(act, pos, poison):
    """Frozen statistics: only the element, its channel's dgamma and its channel's dbeta are non-finite."""
    a, with_res = BNB_ACTS[act]
    c = _bnb_case(pos, "open")
    sets = _bnb_check(f"bn-bwd-frozen-{act}-{pos}-{poison}", c, _poisoned(c.dy, pos, POISON[poison]), a, with_res, True,
                      "some")
    assert int(sets["dz"].sum()) == 1 and int(sets["dgamma"].sum()) == 1 and int(sets["dbeta"].sum()) == 1


@pytest.mark.parametrize("poison", ["nan", "inf"])
@pytest.mark.parametrize("pos", ["a", "b", "c"])
@pytest.mark.parametrize("act", ["relu", "relu-from-z", "relu-mask"])
def test_batchnorm_bwd_poison_under_closed_mask(act, pos, poison):
    """The poison under a closed ReLU mask (from y, recomputed from z, from the mask bytes): everything is finite."""
    a, with_res = BNB_ACTS[act]
    c = _bnb_case(pos, "closed")
    _bnb_check(f"bn-bwd-closed-{act}-{pos}-{poison}", c, _poisoned(c.dy, pos, POISON[poison]), a, with_res, False,
               "none")


# ---- groupnorm_bwd -------------------------------------------------------------------------------------------------
def _gnb_case(pos):
    def make():
        g = _gen(7200)
        C, P, cpg = 128, HO * WO, 128 // GN_G
        c = types.SimpleNamespace(C=C, P=P, cpg=cpg)
        x64 = (torch.randn(N, HO, WO, C, generator=g) * 3 + 1).double()
        at = _pos(x64.shape, pos)
        x64[at] = 30.0  # an open ReLU at the poisoned element
        free = torch.ones_like(x64, dtype=torch.bool)
        free[at] = False
        c.gamma, c.beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
        ga, be = c.gamma.reshape(GN_G, cpg), c.beta.reshape(GN_G, cpg)
        v = (N, P, GN_G, cpg)
        c.x = _nudge(x64.reshape(v), torch.zeros(v), ga, be, (1, 3), free.reshape(v))
        c.xd = c.x.double()
        mean, _, rstd, scale, shift = _stats64(c.xd, ga, be, (1, 3))
        c.mean32, c.rstd32, c.scale32, c.shift32 = (t.float() for t in (mean, rstd, scale, shift))
        c.dy = torch.randn(N, HO, WO, C, generator=g)
        c.dev = types.SimpleNamespace(
            x=c.x.reshape(N, HO, WO, C).to(DEV), gamma=c.gamma.to(DEV), mean32=c.mean32.reshape(N, GN_G).to(DEV),
            rstd32=c.rstd32.reshape(N, GN_G).to(DEV), scale32=c.scale32.reshape(N, C).to(DEV),
            shift32=c.shift32.reshape(N, C).to(DEV))
        return c
    return _cached(("gnb", pos), make)


def _gnb_run(c, dy, relu, half):
    import bev_native as nat
    d = c.dev
    fn = nat.groupnorm_bwd_half if half else nat.groupnorm_bwd
    out = fn(d.x, dy.to(DEV), GN_G, d.mean32, d.rstd32, d.gamma, d.scale32, d.shift32, relu)
    torch.cuda.synchronize()
    return out


def _gnb_ref(c, dy, relu):
    return _gn_bwd_ref(c.xd, dy.double().reshape(c.xd.shape), c.mean32.double(), c.rstd32.double(), c.scale32.double(),
                       c.shift32.double(), c.gamma.reshape(GN_G, c.cpg).double(), relu)


@pytest.mark.parametrize("poison", ["nan", "inf"])
@pytest.mark.parametrize("pos", ["a", "b", "c"])
@pytest.mark.parametrize("relu", [False, True], ids=["none", "relu"])
def test_groupnorm_bwd_poison(relu, pos, poison):
    """groupnorm_bwd / _half: the poisoned (image, group) is non-finite throughout dx, the other image and the other
    groups are finite; dgamma and dbeta are non-finite on that channel only."""
    c = _gnb_case(pos)
    tag = f"gn-bwd-{'relu' if relu else 'none'}-{pos}-{poison}"
    dy = _poisoned(c.dy, pos, POISON[poison])
    dx, dg, db = _gnb_run(c, dy, relu, False)
    dx16 = _gnb_run(c, dy, relu, True)[0]
    rdx, rdg, rdb = _gnb_ref(c, dy, relu)
    nf = _sets(tag, "dx", dx.reshape(rdx.shape), rdx, 1e-4)
    n, _, _, ch = _pos((N, HO, WO, c.C), pos)
    want = torch.zeros_like(nf)
    want[n, :, ch // c.cpg] = True
    assert torch.equal(nf, want)
    chan = torch.zeros(c.C, dtype=torch.bool)
    chan[ch] = True
    assert torch.equal(_sets(tag, "dgamma", dg.reshape(rdg.shape), rdg, 1e-4).reshape(-1), chan)
    assert torch.equal(_sets(tag, "dbeta", db.reshape(rdb.shape), rdb, 1e-4).reshape(-1), chan)
    d16, w16 = dx16.reshape(rdx.shape).cpu(), dx.half().reshape(rdx.shape).cpu()
    assert torch.equal(~torch.isfinite(d16), nf) and torch.equal(d16[~nf], w16[~nf])


# ---- max-pool backward ---------------------------------------------------------------------------------------------
def _pool_run(form, x, dy):
    import bev_native as nat
    xd, dyd = x.to(DEV), dy.to(DEV)
    n, H, W, C = x.shape
    if form == "arg-c8":
        _, arg = nat.maxpool_fwd_arg_nhwc(xd, 3, 2, 1)
        out = nat.maxpool_bwd_arg_nhwc(arg, dyd, H, W, 3, 2, 1)
    else:  # the single-pass entry: C 6 the scalar kernel, C 8 the float4 one
        out = torch.full_like(xd, NAN)
        rc = nat.lib().bev_maxpool2d_bwd_nhwc_f32(nat._ptr(xd), nat._ptr(dyd), n, H, W, C, 3, 2, 1, dy.shape[1],
                                                  dy.shape[2], nat._ptr(out), nat._stream(xd))
        assert rc == 0, rc
    torch.cuda.synchronize()
    return out


def _pool_case(form):
    def make():
        C = 6 if form == "scalar-c6" else 8
        g = _gen(7300 + C)
        x = torch.randint(-3, 4, (N, H2, W2, C), generator=g).float()
        x[0, 7:10, 13:16, C // 2] = 3.0  # position c's window (rows 7..9, columns 13..15): a nine-way tie
        return x, torch.randn(N, HO, WO, C, generator=g)
    return _cached(("pool", form), make)


def _pool_ref(x, dy):
    xr = _nchw(x.double()).clone().requires_grad_(True)
    F.max_pool2d(xr, 3, 2, 1).backward(_nchw(dy.double()))
    return _nhwc(xr.grad)


POOL_FORMS = ["scalar-c6", "v4-c8", "arg-c8"]


@pytest.mark.parametrize("poison", ["nan", "inf"])
@pytest.mark.parametrize("pos", ["a", "b", "c"])
@pytest.mark.parametrize("form", POOL_FORMS)
def test_maxpool_bwd_poison(form, pos, poison):
    """3 / 2 / 1 max-pool over 17 x 29 (integer inputs: tied windows everywhere): exactly the window's argmax input is
    non-finite, the first maximum in scan order; position c's window is a nine-way tie, its first tap is (7, 13)."""
    x, dy = _pool_case(form)
    dy = _poisoned(dy, pos, POISON[poison])
    ref = _pool_ref(x, dy)
    got = _pool_run(form, x, dy)
    nf = _sets(f"maxpool-{form}-{pos}-{poison}", "dx", got, ref, 0.0,
               bound=1e-6 + 1e-6 * torch.nan_to_num(ref, 0.0, 0.0, 0.0).abs())
    assert int(nf.sum()) == 1
    if pos == "c":
        assert bool(nf[0, 7, 13, x.shape[3] // 2])


# ---- conv input gradients ------------------------------------------------------------------------------------------
DGRAD = {  # id: (K, stride, pad, H, W, residual)
    "3x3s1-res": (3, 1, 1, HO, WO, True), "1x1s2": (1, 2, 0, H2, W2, False), "1x1s2-res": (1, 2, 0, H2, W2, True),
    "3x3s2-ryrx": (3, 2, 1, 18, 30, False), "3x3s2-res": (3, 2, 1, H2, W2, True)}


def _dgrad_case(name, Co=40, Ci=32, fp16=False):
    def make():
        K, s, p, H, W, with_res = DGRAD[name]
        g = _gen(7400 + list(DGRAD).index(name) + Co)
        c = types.SimpleNamespace(K=K, s=s, p=p, H=H, W=W)
        c.w = torch.randn(Co, Ci, K, K, generator=g) / (Co * K * K) ** 0.5
        c.dy = torch.randn(N, HO, WO, Co, generator=g)
        c.res = torch.randn(N, H, W, Ci, generator=g) if with_res else None
        if fp16:
            c.w = c.w.half().float()
        assert ((H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1) == (HO, WO)
        c.wd, c.rd = c.w.to(DEV), c.res.to(DEV) if with_res else None
        return c
    return _cached(("dgrad", name, Co, Ci, fp16), make)


def _dgrad_ref(c, dy, absolute=False):
    """float64 autograd of F.conv2d (+ the residual); absolute: the same sum over |terms|."""
    w, dyd = (c.w.double().abs(), dy.double().abs()) if absolute else (c.w.double(), dy.double())
    x = torch.zeros(N, c.w.shape[1], c.H, c.W, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w, None, c.s, c.p).backward(_nchw(dyd))
    out = _nhwc(x.grad)
    if c.res is not None:
        out = out + (c.res.double().abs() if absolute else c.res.double())
    return out


def _dgrad_field(c, pos):
    """The poison's transposed receptive field: input pixels (iy, ix) = s (oy, ox) - p + (ky, kx), every channel."""
    n, oy, ox, _ = _pos((N, HO, WO, 1), pos)
    want = torch.zeros(N, c.H, c.W, c.w.shape[1], dtype=torch.bool)
    for ky in range(c.K):
        for kx in range(c.K):
            iy, ix = c.s * oy - c.p + ky, c.s * ox - c.p + kx
            if 0 <= iy < c.H and 0 <= ix < c.W:
                want[n, iy, ix] = True
    return want


@pytest.mark.parametrize("poison", ["nan", "inf"])
@pytest.mark.parametrize("pos", ["a", "b", "c"])
@pytest.mark.parametrize("arith", ["f32", "bf16x6"])
@pytest.mark.parametrize("name", list(DGRAD))
def test_dgrad_poison(name, arith, pos, poison):
    """trunk_grad._dgrad's four branches (stride 1 + residual; 1x1 stride 2 through place_strided, with and without a
    residual; 3x3 stride 2 through dilate_nhwc with both remainders ry = rx = 1, and with a residual) under both trunk
    arithmetics: the non-finite set is the poison's transposed receptive field; sets only (Inf - Inf may be NaN)."""
    import bev_native as nat
    from models.encoders import trunk_grad as tg
    c = _dgrad_case(name)
    dy = _poisoned(c.dy, pos, POISON[poison])
    with nat.conv_arith_mode(arith):
        got = tg._dgrad(dy.to(DEV), c.wd, c.H, c.W, c.s, c.p, c.rd)
    torch.cuda.synchronize()
    nf = _sets(f"dgrad-{name}-{arith}-{pos}-{poison}", "dx", got, _dgrad_ref(c, dy), 1e-5)
    assert torch.equal(nf, _dgrad_field(c, pos))


@pytest.mark.parametrize("poison", ["nan", "inf"])
@pytest.mark.parametrize("pos", ["a", "b", "c"])
@pytest.mark.parametrize("stored", ["f32", "f16"])
@pytest.mark.parametrize("name", ["3x3s1-res", "3x3s2-ryrx"])
def test_dgrad_h16_poison(name, stored, pos, poison):
    """trunk_grad._dgrad_h16 (the autocast input gradient) with dz stored in fp32 and in fp16: the same set; finite
    elements within the fp16 family's bound K 2^-24 sum|terms| + 1e-6 over the fp16-rounded operands."""
    import bev_native as nat
    from models.encoders import trunk_grad as tg
    c = _dgrad_case(name, Co=64, fp16=True)
    dy = _poisoned(c.dy.half().float(), pos, POISON[poison])
    dyd = dy.to(DEV).half() if stored == "f16" else dy.to(DEV)
    with nat._half_mode(True):
        got = tg._dgrad_h16(dyd, c.wd, c.H, c.W, c.s, c.p, c.rd)
    torch.cuda.synchronize()
    clean = torch.nan_to_num(dy, 0.0, 0.0, 0.0)
    bound = 64 * c.K * c.K * 2.0 ** -24 * _dgrad_ref(c, clean, absolute=True) + 1e-6
    nf = _sets(f"dgrad-h16-{name}-{stored}-{pos}-{poison}", "dx", got, _dgrad_ref(c, dy), None, bound=bound)
    assert torch.equal(nf, _dgrad_field(c, pos))


DW_CASES = [(3, 1), (3, 2), (5, 1), (5, 2)]  # (K, stride): EfficientNet runs all four; stride 2 reads 17 x 29
DW_IDS = [f"k{k}s{s}" for k, s in DW_CASES]


def _dw_dgrad(nat, dz, wt, K, st, p, H, W):
    """DWConvBNTrain.backward's input-gradient calls."""
    C = dz.shape[-1]
    wf = wt.view(K, K, C).flip(0, 1).reshape(K * K, C).contiguous()
    zero = torch.zeros(C, device=dz.device)
    q = K - 1 - p
    if st == 1:
        return nat.dwconv2d_nhwc(dz, wf, zero, K, 1, q, nat.ACT_NONE)[0]
    Ho, Wo = dz.shape[1], dz.shape[2]
    ry, rx = (H + 2 * p - K) % st, (W + 2 * p - K) % st
    Hd, Wd = st * (Ho - 1) + 1 + 2 * q + ry, st * (Wo - 1) + 1 + 2 * q + rx
    return nat.dwconv2d_nhwc(nat.dilate_nhwc(dz, st, q, q, Hd, Wd), wf, zero, K, 1, 0, nat.ACT_NONE)[0]


def _dw_case(K, s):
    def make():
        g = _gen(7500 + 10 * K + s)
        C = 48
        H, W = (HO, WO) if s == 1 else (H2, W2)
        assert ((H + 2 * (K // 2) - K) // s + 1, (W + 2 * (K // 2) - K) // s + 1) == (HO, WO)
        c = types.SimpleNamespace(K=K, s=s, p=K // 2, H=H, W=W, C=C)
        c.w = torch.randn(C, 1, K, K, generator=g) * 0.3
        c.wt = c.w.reshape(C, K * K).t().contiguous().to(DEV)
        c.x, c.dy = torch.randn(N, H, W, C, generator=g), torch.randn(N, HO, WO, C, generator=g)
        return c
    return _cached(("dw", K, s), make)


def _dw_dgrad_ref(c, dy):
    x = torch.zeros(N, c.C, c.H, c.W, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, c.w.double(), None, c.s, c.p, 1, c.C).backward(_nchw(dy.double()))
    return _nhwc(x.grad)


@pytest.mark.parametrize("poison", ["nan", "inf"])
@pytest.mark.parametrize("pos", ["a", "b", "c"])
@pytest.mark.parametrize("K,s", DW_CASES, ids=DW_IDS)
def test_dwconv_dgrad_poison(K, s, pos, poison):
    """DWConvBNTrain's depthwise input gradient (K 3 and 5; stride 1 directly, stride 2 through dilate_nhwc), through
    the calls its backward makes: the poisoned channel's transposed window and nothing else."""
    import bev_native as nat
    c = _dw_case(K, s)
    dy = _poisoned(c.dy, pos, POISON[poison])
    got = _dw_dgrad(nat, dy.to(DEV), c.wt, K, c.s, c.p, c.H, c.W)
    torch.cuda.synchronize()
    nf = _sets(f"dw-dgrad-k{K}s{s}-{pos}-{poison}", "dx", got, _dw_dgrad_ref(c, dy), 1e-5)
    n, oy, ox, ch = _pos(dy.shape, pos)
    want = torch.zeros_like(nf)
    for ky in range(K):
        for kx in range(K):
            iy, ix = c.s * oy - c.p + ky, c.s * ox - c.p + kx
            if 0 <= iy < c.H and 0 <= ix < c.W:
                want[n, iy, ix, ch] = True
    assert torch.equal(nf, want)


# ---- weight gradients ----------------------------------------------------------------------------------------------
WGRAD = {  # id: (Ci, Co, K, stride, pad, dilation, H, W)
    "mfma-nat": (32, 40, 3, 2, 1, 1, H2, W2), "mfma-transposed": (32, 40, 3, 2, 1, 1, H2, W2),
    "valu": (32, 40, 3, 2, 1, 1, H2, W2), "ex-dil2": (32, 40, 3, 1, 2, 2, HO, WO),
    "scalar-ci6-co5": (6, 5, 3, 1, 1, 1, HO, WO),
    "h16-any": (64, 36, 3, 1, 1, 1, HO, WO)}
WGRAD_MFMA = {"mfma-nat": 2, "mfma-transposed": 1, "valu": 0}


def _wgrad_case(name):
    def make():
        Ci, Co, K, s, p, dil, H, W = WGRAD[name]
        g = _gen(7600 + Ci + Co + dil)
        c = types.SimpleNamespace(Ci=Ci, Co=Co, K=K, s=s, p=p, dil=dil, H=H, W=W)
        c.x, c.dy = torch.randn(N, H, W, Ci, generator=g), torch.randn(N, HO, WO, Co, generator=g)
        if name == "h16-any":
            c.x, c.dy = c.x.half().float(), c.dy.half().float()
        c.xd = c.x.to(DEV)
        return c
    return _cached(("wgrad", name), make)


def _wgrad_run(name, c, dy):
    import bev_native as nat
    dyd = dy.to(DEV)
    if name in WGRAD_MFMA:
        with nat.tuned(WGRAD_MFMA=WGRAD_MFMA[name]):
            out = nat.conv_wgrad(c.xd, dyd, c.K, c.K, c.s, c.p)
    elif name == "ex-dil2":
        out = nat.conv_wgrad_ex(c.xd, dyd, c.K, c.p, c.dil)
    elif name == "h16-any":
        out = nat.conv_wgrad_h16_any(c.xd, dyd, c.K, c.K, c.s, c.p)
    else:  # unpadded operands through the C entry: the scalar kernel (Ci % 4 != 0)
        dW = torch.full((c.Co, c.K, c.K, c.Ci), NAN, device=DEV)
        rc = nat.lib().bev_conv_wgrad_ex_f32(nat._ptr(c.xd), N, c.H, c.W, c.Ci, nat._ptr(dyd), HO, WO, c.Co, c.K, c.K,
                                             c.s, c.p, c.dil, nat._ptr(dW), nat._stream(dyd))
        assert rc == 0, rc
        out = dW.permute(0, 3, 1, 2)
    torch.cuda.synchronize()
    return out


def _wgrad_ref(c, dy, absolute=False):
    x, d = (c.x.double().abs(), dy.double().abs()) if absolute else (c.x.double(), dy.double())
    return torch.nn.grad.conv2d_weight(_nchw(x), (c.Co, c.Ci, c.K, c.K), _nchw(d), c.s, c.p, c.dil)


def _wgrad_check(tag, c, got, dy, pos, name):
    """The poisoned row is non-finite on every tap whose input pixel is inside the image, every other row is finite
    and meets the bar against the clean reference (the poison touches no other row); the poisoned row's taps in the
    padding are not asserted either way."""
    n, oy, ox, co = _pos(dy.shape, pos)
    got = _d(got)
    ref = _wgrad_ref(c, torch.nan_to_num(dy, 0.0, 0.0, 0.0))
    inside = torch.zeros(c.K, c.K, dtype=torch.bool)
    for ky in range(c.K):
        for kx in range(c.K):
            iy, ix = c.s * oy - c.p + ky * c.dil, c.s * ox - c.p + kx * c.dil
            inside[ky, kx] = 0 <= iy < c.H and 0 <= ix < c.W
    assert bool(inside.any()) and (pos != "c" or bool(inside.all())) and (pos != "b" or not bool(inside.all()))
    assert not bool(torch.isfinite(got[co][:, inside]).any()), (tag, "a tap of the poisoned row is finite")
    rows = torch.ones(c.Co, dtype=torch.bool)
    rows[co] = False
    assert bool(torch.isfinite(got[rows]).all()), (tag, "the poison reached another row")
    err = (got[rows] - ref[rows]).abs()
    if name == "h16-any":  # test_wgrad_h16_fp16_gradient_vs_float64's bar: 2e-6 of sum |terms|
        mag = _wgrad_ref(c, torch.nan_to_num(dy, 0.0, 0.0, 0.0), absolute=True)[rows]
        worst = float((err / (mag + 1e-12)).max()) / 2e-6
    else:
        worst = float(err.max()) / (1e-4 * float(ref[rows].abs().max()))
    print(f"[grad] {tag}: finite rows' err / bar {worst:.3f}")
    assert worst <= 1.0, (tag, worst)


@pytest.mark.parametrize("poison", ["nan", "inf"])
@pytest.mark.parametrize("pos", ["a", "b", "c"])
@pytest.mark.parametrize("name", list(WGRAD))
def test_conv_wgrad_poison(name, pos, poison):
    """conv_wgrad under WGRAD_MFMA 2 / 1 / 0 (3x3 stride 2), conv_wgrad_ex (dilation 2), the scalar kernel (Ci 6, Co 5,
    through the C entry), conv_wgrad_h16_any."""
    c = _wgrad_case(name)
    dy = _poisoned(c.dy, pos, POISON[poison])
    _wgrad_check(f"wgrad-{name}-{pos}-{poison}", c, _wgrad_run(name, c, dy), dy, pos, name)


@pytest.mark.parametrize("poison", ["nan", "inf"])
@pytest.mark.parametrize("pos", ["a", "b", "c"])
@pytest.mark.parametrize("K,s", DW_CASES, ids=DW_IDS)
def test_dwconv_wgrad_poison(K, s, pos, poison):
    """dwconv_wgrad (dW [K K, C]): the poisoned channel's column is non-finite on the taps inside the image, every
    other channel is finite and within 1e-4 max|ref| (test_dwconv_wgrad_and_channel_ops_vs_torch's bar)."""
    import bev_native as nat
    c = _dw_case(K, s)
    dy = _poisoned(c.dy, pos, POISON[poison])
    got = _d(nat.dwconv_wgrad(c.x.to(DEV), dy.to(DEV), K, c.s, c.p)).t().reshape(c.C, K, K)
    w = torch.zeros(c.C, 1, K, K, dtype=torch.float64, requires_grad=True)
    clean = torch.nan_to_num(dy, 0.0, 0.0, 0.0)
    F.conv2d(_nchw(c.x.double()), w, None, c.s, c.p, 1, c.C).backward(_nchw(clean.double()))
    ref = w.grad[:, 0]
    n, oy, ox, ch = _pos(dy.shape, pos)
    inside = torch.zeros(K, K, dtype=torch.bool)
    for ky in range(K):
        for kx in range(K):
            inside[ky, kx] = 0 <= c.s * oy - c.p + ky < c.H and 0 <= c.s * ox - c.p + kx < c.W
    assert bool(inside.any()) and (pos != "c" or bool(inside.all())) and (pos != "b" or not bool(inside.all()))
    assert not bool(torch.isfinite(got[ch][inside]).any())
    rows = torch.ones(c.C, dtype=torch.bool)
    rows[ch] = False
    assert bool(torch.isfinite(got[rows]).all())
    assert float((got[rows] - ref[rows]).abs().max()) <= 1e-4 * float(ref[rows].abs().max())


@pytest.mark.parametrize("poison", ["nan", "inf"])
@pytest.mark.parametrize("pos", ["a", "b", "c"])
@pytest.mark.parametrize("C", [24, 128], ids=["c24-generic", "c128-v4"])
def test_colsum_poison(C, pos, poison):
    """colsum: that column only; the others within test_colsum_sizes' 1e-5 sum|x| (per column)."""
    import bev_native as nat
    dy = _poisoned(torch.randn(N, HO, WO, C, generator=_gen(7700 + C)), pos, POISON[poison])
    ref = dy.double().sum((0, 1, 2))
    nf = _sets(f"colsum-c{C}-{pos}-{poison}", "db", nat.colsum(dy.to(DEV)), ref, None,
               bound=1e-5 * torch.nan_to_num(dy, 0.0, 0.0, 0.0).double().abs().sum((0, 1, 2)))
    assert int(nf.sum()) == 1 and bool(nf[_pos(dy.shape, pos)[3]])


# ---- view max, head operand ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", ["nan", "inf"])
@pytest.mark.parametrize("pos", ["a", "b", "c"])
def test_view_max_bwd_poison(pos, poison):
    """view_max_bwd: only the winning view's element is non-finite (integer inputs: ties go to torch's index)."""
    import bev_native as nat
    g = _gen(7800)
    V = 5
    x = torch.randint(-2, 3, (N, V, HO, WO, 8), generator=g).float()
    dy = _poisoned(torch.randn(N, HO, WO, 8, generator=g), pos, POISON[poison])
    xr = x.double().requires_grad_(True)
    xr.max(1).values.backward(dy.double())
    nf = _sets(f"view_max_bwd-{pos}-{poison}", "gx", nat.view_max_bwd(x.to(DEV), dy.to(DEV)), xr.grad, 0.0)
    assert int(nf.sum()) == 1


@pytest.mark.parametrize("poison", ["nan", "inf"])
@pytest.mark.parametrize("where", ["a", "b", "c", "pad"])
@pytest.mark.parametrize("Wb", [16, 15], ids=["v4", "scalar"])
def test_head_operand_bwd_poison(Wb, where, poison):
    """head_operand_bwd / head_operand_bwd_bias (gs = gx[..., :P] in NCHW, gbias its sum) against float64: the poison
    in a projected channel reaches one element of gs and that channel's bias gradient; in the positional / padding
    channels past P it reaches nothing.  Exact copies; the bias within 1e-5 sum|terms|."""
    import bev_native as nat
    P, cp = 18, 24
    gx = torch.randn(N, HO, Wb, cp, generator=_gen(7900 + Wb))
    if where == "pad":
        gx[0, 4, 7, P + 1] = POISON[poison]
    else:
        n, h, w, _ = _pos(gx.shape, where)
        gx[n, h, w, {"a": P - 1, "b": 0, "c": P // 2}[where]] = POISON[poison]
    ref = gx[..., :P].permute(0, 3, 1, 2).double()
    tag = f"head_operand_bwd-{Wb}-{where}-{poison}"
    expect = "none" if where == "pad" else "some"
    gs = nat.head_operand_bwd(gx.to(DEV), P)
    gs2, gb = nat.head_operand_bwd_bias(gx.to(DEV), P)
    torch.cuda.synchronize()
    assert int(_sets(tag, "gs", gs, ref, 0.0, expect).sum()) == (0 if where == "pad" else 1)
    _sets(tag, "gs (bias form)", gs2, ref, 0.0, expect)
    assert (gb is None) == (Wb % 4 != 0)
    if gb is not None:
        mag = torch.nan_to_num(gx[..., :P], 0.0, 0.0, 0.0).double().abs().sum((0, 1, 2))
        assert int(_sets(tag, "gbias", gb, ref.sum((0, 2, 3)), None, expect, bound=1e-5 * mag).sum()) == (
            0 if where == "pad" else 1)


# ---- the losses ----------------------------------------------------------------------------------------------------
def _focal64(x, gt, alpha, beta):
    """model_wrapper's torch composition of the CenterNet focal loss, in float64."""
    p = torch.sigmoid(x).clamp(1e-4, 1 - 1e-4)
    peak = gt == 1.0
    pos = torch.where(peak, p.log() * (1 - p).pow(alpha), torch.zeros_like(p))
    neg = torch.where(gt < 1.0, (1 - p).log() * p.pow(alpha) * (1 - gt).pow(beta), torch.zeros_like(p))
    return -(pos.sum() + neg.sum()) / peak.sum().double().clamp(min=1.0)


def _focal_case():
    def make():
        g = _gen(8000)
        gt = torch.rand(N, 1, 12, 20, generator=g) * 0.9
        gt.view(-1)[::37] = 1.0
        return torch.randn(N, 1, 12, 20, generator=g) * 3, gt
    return _cached("focal", make)


def _focal_both(x, gt, alpha=2.0, beta=4.0, gl=1.7):
    import bev_native as nat
    xd, gd = x.to(DEV), gt.to(DEV)
    loss, inv = nat.focal_loss(xd, gd, alpha, beta)
    dx = nat.focal_loss_bwd(xd, gd, alpha, beta, torch.tensor(gl, device=DEV), inv)
    torch.cuda.synchronize()
    xr = x.double().requires_grad_(True)
    lr = _focal64(xr, gt.double(), alpha, beta)
    (gr,) = torch.autograd.grad(lr * gl, xr)
    return float(loss), _d(dx), float(lr.detach()), gr


FOCAL_CELLS = {"peak": 0, "neg": 1}  # flat indices: gt == 1 (every 37th cell) and gt < 1


@pytest.mark.parametrize("cell", list(FOCAL_CELLS))
@pytest.mark.parametrize("value", ["nan", "inf", "-inf"])
def test_focal_loss_non_finite_logit(value, cell):
    """One logit NaN / +Inf / -Inf: the loss and that cell's gradient follow the float64 torch composition (NaN
    propagates through sigmoid and clamp; +-Inf saturates into the clamp, where the gradient is 0), and every other
    cell's gradient is finite and within the existing bars (1e-5 on the loss, rtol 1e-4 + 1e-5 max|ref|)."""
    x, gt = _focal_case()
    x = x.clone()
    i = FOCAL_CELLS[cell]
    assert (float(gt.view(-1)[i]) == 1.0) == (cell == "peak")
    x.view(-1)[i] = {"nan": NAN, "inf": INF, "-inf": -INF}[value]
    loss, dx, lr, gr = _focal_both(x, gt)
    tag = f"focal-{value}-{cell}"
    print(f"[grad] {tag}: loss {loss} (float64 {lr}), d cell {float(dx.view(-1)[i])} ({float(gr.view(-1)[i])})")
    if torch.isfinite(torch.tensor(lr)):
        assert abs(loss - lr) <= 1e-5 * abs(lr), (tag, loss, lr)
    else:
        assert not torch.isfinite(torch.tensor(loss)), (tag, loss, lr)
    nf = ~torch.isfinite(gr)
    assert torch.equal(~torch.isfinite(dx), nf), (tag, int((~torch.isfinite(dx)).sum()), int(nf.sum()))
    assert int(nf.sum()) <= 1 and (not bool(nf.any()) or bool(nf.view(-1)[i]))
    scale = float(gr[~nf].abs().max())
    assert bool(((dx - gr).abs()[~nf] <= 1e-4 * gr.abs()[~nf] + 1e-5 * scale).all()), tag


@pytest.mark.parametrize("cell", list(FOCAL_CELLS))
@pytest.mark.parametrize("value", [90.0, -90.0, 1e4, -1e4, FLT_MAX, -FLT_MAX])
def test_focal_loss_extreme_logit(value, cell):
    """Finite extreme logits (exp overflows in fp32 on one side of each; the existing test stops at +-20): the loss is
    finite and within 1e-5, the gradient is that of the torch composition."""
    x, gt = _focal_case()
    x = x.clone()
    i = FOCAL_CELLS[cell]
    x.view(-1)[i] = value
    loss, dx, lr, gr = _focal_both(x, gt)
    tag = f"focal-{value:g}-{cell}"
    assert torch.isfinite(torch.tensor(loss)) and abs(loss - lr) <= 1e-5 * abs(lr), (tag, loss, lr)
    assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(gr).all()), tag
    assert float(dx.view(-1)[i]) == float(gr.view(-1)[i]) == 0.0, (tag, float(dx.view(-1)[i]), float(gr.view(-1)[i]))
    assert bool(((dx - gr).abs() <= 1e-4 * gr.abs() + 1e-5 * float(gr.abs().max())).all()), tag


def _l1_case():
    """(offset, size [2, 2, 12, 20], indices, mask [2, 6], offset / size targets [2, 6, 2]): two objects share cell 5 of
    image 0, two slots of image 0 and four of image 1 are empty."""
    def make():
        g = _gen(8100)
        B, M, H, W = 2, 6, 12, 20
        off, size = torch.rand(B, 2, H, W, generator=g), torch.randn(B, 2, H, W, generator=g)
        idx = torch.tensor([[5, 5, 77, 130, 0, 0], [200, 31, 0, 0, 0, 0]])
        mask = torch.tensor([[1.0, 1, 1, 1, 0, 0], [1, 1, 0, 0, 0, 0]])
        return off, size, idx, mask, torch.rand(B, M, 2, generator=g), torch.randn(B, M, 2, generator=g)
    return _cached("l1", make)


@pytest.mark.parametrize("cell", ["object", "empty"])
def test_l1_losses_nan_in_offset_map(cell):
    """A NaN in the offset map at a cell that holds an object: that loss is NaN, and the gradients are those of the
    float64 torch composition -- every one finite, the cell's own 0, because torch's abs backward is g sign(x) and
    sign(NaN) = 0 (asserted on the reference; the kernel's comparisons give the same 0).  So a NaN in this map shows
    in the loss alone.  At a cell that holds no object everything is finite (the gather never reads it).  Bars of
    test_native_l1_losses_vs_float64_torch (1e-5; rtol 1e-5 + 1e-7)."""
    import bev_native as nat
    off, size, idx, mask, off_t, size_t = (t.clone() for t in _l1_case())
    B, M = idx.shape
    flat = 77 if cell == "object" else 78
    off.view(B, 2, -1)[0, 1, flat] = NAN
    dev = [t.to(DEV) for t in (off, size, idx, mask, off_t, size_t)]
    out = nat.l1_losses(*dev)
    gl = torch.tensor([1.3, 0.7], device=DEV)
    d_off, d_sz = nat.l1_losses_bwd(*dev, gl, out)
    torch.cuda.synchronize()
    o, s = off.double().requires_grad_(True), size.double().requires_grad_(True)
    m = mask.double().unsqueeze(-1)
    n = m.sum() + 1e-4
    gather = lambda t: t.view(B, 2, -1).gather(2, idx.unsqueeze(1).expand(B, 2, M)).permute(0, 2, 1)  # noqa: E731
    lo = (gather(o) - off_t.double()).mul(m).abs().sum() / n
    ls = (gather(s) - size_t.double()).mul(m).abs().sum() / n
    go, gs = torch.autograd.grad(1.3 * lo + 0.7 * ls, (o, s))
    tag = f"l1-{cell}"
    print(f"[grad] {tag}: losses {out[:2].tolist()} (float64 {float(lo.detach())}, {float(ls.detach())})")
    lo, ls = lo.detach(), ls.detach()
    assert bool(torch.isfinite(lo)) == (cell == "empty")
    assert bool(torch.isfinite(out[0])) == bool(torch.isfinite(lo))
    if cell == "empty":
        assert abs(float(out[0]) - float(lo)) <= 1e-5 * float(lo)
    assert abs(float(out[1]) - float(ls)) <= 1e-5 * float(ls)
    assert bool(torch.isfinite(go).all()) and float(go.view(B, 2, -1)[0, 1, flat]) == 0.0  # sign(NaN) = 0
    _sets(tag, "d offset", d_off, go, None, "none", bound=1e-5 * go.abs() + 1e-7)
    assert float(d_off.view(B, 2, -1)[0, 1, flat]) == 0.0
    _sets(tag, "d size", d_sz, gs, None, "none", bound=1e-5 * gs.abs() + 1e-7)


# ======================================================================================================================
# B, the warp backward, the max-fused backward and the 1x1 projection (float64 grid_sample autograd over the oracle's
# grid cast to double)
# ======================================================================================================================
def _warp_case(name):
    def make():
        import os

        import numpy as np

        import oracle as O
        from conftest import GOLDEN
        d = np.load(os.path.join(GOLDEN, name + ".npz"))
        c = types.SimpleNamespace(**{k: int(d[k]) for k in ("V", "C", "Hf", "Wf", "bev_h", "bev_w")})
        c.img = (int(d["img_h"]), int(d["img_w"]))
        H = d["H"].reshape(-1, 9)
        c.grid = torch.from_numpy(O.Oracle().grid(H, d["xs"], d["ys"], c.Hf, c.Wf, c.img)).double()  # [V, Hb, Wb, 2]
        c.Hd, c.xs, c.ys = (torch.from_numpy(np.ascontiguousarray(t)).float().to(DEV) for t in (H, d["xs"], d["ys"]))
        c.K, c.Rt = torch.from_numpy(d["K"]).to(DEV), torch.from_numpy(d["Rt"]).to(DEV)
        c.bounds = tuple(float(x) for x in d["bounds"])
        # a tap of the bilinear footprint is inside the map iff -1 < pixel coordinate < size (align_corners=False)
        px, py = ((c.grid[..., 0] + 1) * c.Wf - 1) / 2, ((c.grid[..., 1] + 1) * c.Hf - 1) / 2
        inside = (px > 0.25) & (px < c.Wf - 1.25) & (py > 0.25) & (py < c.Hf - 1.25)
        outside = ~((px > -1.5) & (px < c.Wf + 0.5) & (py > -1.5) & (py < c.Hf + 0.5)) | ~torch.isfinite(px + py)
        seen = inside.any(0).nonzero()
        assert len(seen) > 0, "no BEV cell samples inside a view"
        # neither fixture has a cell outside EVERY view, so the unseen case runs over the views that do not see the
        # cell: the cell outside the most views, and those views (all V stay in the per-view form)
        count = outside.sum(0)
        unseen = (count == count.max()).nonzero()
        assert int(count.max()) > 0, "no BEV cell outside a view"
        c.cell = {"seen": tuple(seen[len(seen) // 2].tolist()), "unseen": tuple(unseen[len(unseen) // 2].tolist())}
        c.views = {"seen": list(range(c.V)), "unseen": outside[:, c.cell["unseen"][0], c.cell["unseen"][1]].nonzero()
                   .reshape(-1).tolist()}
        c.view = {"seen": int(inside[:, c.cell["seen"][0], c.cell["seen"][1]].nonzero()[0]),
                  "unseen": c.views["unseen"][0]}
        g = _gen(8200 + c.V)
        c.go = torch.randn(c.V, c.C, c.bev_h, c.bev_w, generator=g)
        return c
    return _cached(("warp", name), make)


def _warp_ref(c, gout, mode, vs=None):
    vs = list(range(c.V)) if vs is None else vs
    fc = torch.zeros(1, len(vs), c.C, c.Hf, c.Wf, dtype=torch.float64, requires_grad=True)
    r = torch.stack([F.grid_sample(fc[0, i][None], c.grid[v][None], mode="bilinear", padding_mode="zeros",
                                   align_corners=False)[0] for i, v in enumerate(vs)])
    r = r.mean(0) if mode == "mean" else r.sum(0) if mode == "sum" else r
    r.backward(gout.double())
    return fc.grad[0]


def _warp_run(c, gout, mode, pool, vs=None):
    import bev_native as nat
    vs = list(range(c.V)) if vs is None else vs
    Hd = c.Hd[vs].contiguous()
    with nat.tuned(WARP_BWD_POOL=pool):
        if mode == "views":
            out = nat.warp_bwd(gout.to(DEV), Hd, c.xs, c.ys, c.Hf, c.Wf, c.img)
        else:
            out = nat.warp_fuse_bwd(gout[None].to(DEV), Hd, c.xs, c.ys, len(vs), c.Hf, c.Wf, c.img, mode)[0]
    torch.cuda.synchronize()
    return out


def _warp_gout(c, mode, cell, val, k=0):
    y, x = c.cell[cell] if cell else (0, 0)
    go = (c.go if mode == "views" else c.go[0]).clone() * 2.0 ** k
    if cell:
        go[(c.view[cell], c.C // 2, y, x) if mode == "views" else (c.C // 2, y, x)] = val
    return go


@pytest.mark.parametrize("poison", ["nan", "inf"])
@pytest.mark.parametrize("cell", ["seen", "unseen"])
@pytest.mark.parametrize("pool", [0, 96, 3])
@pytest.mark.parametrize("mode", ["views", "sum", "mean"])
@pytest.mark.parametrize("name", ["warp_w3_v3", "warp_w7_tiny"])
def test_warp_bwd_poison(name, mode, pool, cell, poison):
    """warp_bwd and warp_fuse_bwd (sum, mean) under WARP_BWD_POOL 0 / 96 / 3 (LDS footprint images, one-pixel images,
    none): a poison in a BEV cell that samples inside a view reaches that cell's bilinear taps of the poisoned channel
    (of every view that sees it, for the fused forms) and nothing else -- an LDS image flushed with 0 * Inf would
    smear it; in a cell that no view sees it reaches nothing.  (Every cell of both fixtures is inside some view, so
    "unseen" takes the cell outside the most views: the per-view form poisons the gradient of one of those views, the
    fused forms run over those views alone.)  Finite elements: rtol 1e-4 + atol 5e-5."""
    c = _warp_case(name)
    go = _warp_gout(c, mode, cell, POISON[poison])
    vs = None if mode == "views" else c.views[cell]
    ref = _warp_ref(c, go, None if mode == "views" else mode, vs)
    got = _warp_run(c, go, mode, pool, vs)
    nf = _sets(f"warp-{name}-{mode}-pool{pool}-{cell}-{poison}", "d feats", got, ref, None,
               "some" if cell == "seen" else "none", bound=1e-4 * torch.nan_to_num(ref, 0.0, 0.0, 0.0).abs() + 5e-5)
    assert 0 < int(nf.sum()) <= 4 * c.V if cell == "seen" else not bool(nf.any())


@pytest.mark.parametrize("poison", ["nan", "inf"])
def test_fused_max_bwd_poison(poison):
    """GeometryTransformer.forward_fused(..., 'max') backward on the warp_w3_v3 geometry (C = 8, channels-last): only
    the winning view's taps of the poisoned channel are non-finite.  The float64 reference routes each element to the
    view that wins among the fp32 samples (torch CPU grid_sample in fp32, asserted bit-identical to the native
    forward, as test_fused_max_backward_vs_torch_autograd has it): two views within an fp32 rounding of each other
    may swap in float64, and the element then carries its whole gradient on the other view -- the routing is pinned by
    the forward's own test, the gradient values are what is compared here."""
    c = _warp_case("warp_w3_v3")
    gm = _fused_max_gm(c).clone()
    y, x = c.cell["seen"]
    gm[0, gm.shape[1] // 2, y, x] = POISON[poison]
    got, ref = _fused_max_both(c, gm)
    nf = _sets(f"fused-max-bwd-{poison}", "d feats", got, ref, None,
               bound=1e-4 * torch.nan_to_num(ref, 0.0, 0.0, 0.0).abs() + 5e-5)
    views = nf.reshape(c.V, -1).any(1)
    assert int(views.sum()) == 1 and 0 < int(nf.sum()) <= 4


def _fused_max_gm(c):
    return _cached("fused-max-gm", lambda: torch.randn(1, 8, c.bev_h, c.bev_w, generator=_gen(8301)))


def _fused_max_both(c, gm):
    """-> (native d feats, float64 d feats) of forward_fused(..., 'max') for the upstream gradient gm."""
    from models.fusion.geometry import GeometryTransformer
    feats = _cached("fused-max-feats", lambda: torch.randn(1, c.V, 8, c.Hf, c.Wf, generator=_gen(8300)))
    fc = feats.double().requires_grad_(True)
    r32 = torch.stack([F.grid_sample(feats[0, v][None], c.grid[v][None].float(), mode="bilinear", padding_mode="zeros",
                                     align_corners=False)[0] for v in range(c.V)]).max(dim=0)
    r = torch.stack([F.grid_sample(fc[0, v][None], c.grid[v][None], mode="bilinear", padding_mode="zeros",
                                   align_corners=False)[0] for v in range(c.V)]).gather(0, r32.indices[None])
    r.backward(gm.double())
    fl = feats.permute(0, 1, 3, 4, 2).contiguous().to(DEV).permute(0, 1, 4, 2, 3).requires_grad_(True)
    geo = GeometryTransformer(c.bev_h, c.bev_w, c.bounds)
    out = geo.forward_fused(fl, c.K, c.Rt, c.img, "max")
    assert torch.equal(out.detach().cpu()[0].view(torch.int32), r32.values.view(torch.int32))
    out.backward(gm.to(DEV))
    torch.cuda.synchronize()
    return fl.grad, fc.grad


@pytest.mark.parametrize("poison", ["nan", "inf"])
@pytest.mark.parametrize("pos", ["a", "b", "c"])
def test_proj1x1_bwd_poison(pos, poison):
    """models/encoders/proj.py's Proj1x1 (the encoder / BEV 1x1 projection) backward against autograd of the float64
    composition: d feat is non-finite on the poisoned pixel (every input channel), dW on the poisoned output
    channel's row, db on that channel; test_train.py's bar for the finite rest (1e-4 of the gradient's scale)."""
    Ci, Co = PROJ
    gy = _poisoned(_proj_case()[3], pos, POISON[poison])
    got, ref = _proj_both(gy)
    tag = f"proj1x1-{pos}-{poison}"
    n, h, wx, co = _pos(gy.shape, pos)
    nf = _sets(tag, "d feat", got[0], ref[0], 1e-4)
    want = torch.zeros_like(nf)
    want[n, h, wx] = True
    assert torch.equal(nf, want)
    nf = _sets(tag, "dW", got[1], ref[1], 1e-4)
    assert torch.equal(nf.reshape(Co, Ci).all(1), torch.arange(Co) == co) and int(nf.sum()) == Ci
    nf = _sets(tag, "db", got[2], ref[2], 1e-4)
    assert torch.equal(nf, torch.arange(Co) == co)


PROJ = (64, 40)  # Ci, Co


def _proj_case():
    def make():
        g = _gen(8400)
        Ci, Co = PROJ
        return (torch.randn(N, HO, WO, Ci, generator=g), torch.randn(Co, Ci, 1, 1, generator=g) / 8,
                torch.randn(Co, generator=g), torch.randn(N, HO, WO, Co, generator=g))
    return _cached("proj", make)


def _proj_both(gy):
    """-> ((d feat NHWC, dW, db) of Proj1x1 on the device, the same from float64 autograd of F.conv2d)."""
    from models.encoders.proj import Proj1x1
    feat, w, b, _ = _proj_case()
    leaves = [t.to(DEV).requires_grad_(True) for t in (feat, w, b)]
    Proj1x1.apply(*leaves).backward(gy.to(DEV))
    torch.cuda.synchronize()
    ref = [t.double().requires_grad_(True) for t in (_nchw(feat), w, b)]
    F.conv2d(*ref).backward(_nchw(gy.double()))
    return [t.grad for t in leaves], [_nhwc(ref[0].grad), ref[1].grad, ref[2].grad]


# ======================================================================================================================
# C: an overflowing step is skipped (bev_dist.train_step + GradScaler on the small BEVNet of
# test_bevnet_amp_step_matches_reference_fp32_gradients)
# ======================================================================================================================
def _small_net(monkeypatch, half):
    import numpy as np

    import bev_native as nat
    from test_bevnet_gpu import PATH, build, targets_of
    monkeypatch.setattr(nat, "AMP_HALF_CONVS", half)
    d = np.load(PATH)
    net, batch, cfg = build(d)
    net.train()
    return net, batch, targets_of(d), cfg["LOSS"]


def _snapshot(net, opt):
    state = [t.detach().clone() for s in opt.state.values() for t in s.values() if torch.is_tensor(t)]
    return [p.detach().clone() for p in net.parameters()], state


def _same_bits(a, b):
    return len(a) == len(b) and all(torch.equal(x.view(torch.uint8) if x.dim() else x.reshape(1).view(torch.uint8),
                                                y.view(torch.uint8) if y.dim() else y.reshape(1).view(torch.uint8))
                                    for x, y in zip(a, b))


def _skipped_step(net, batch, targets, loss_cfg, scaler, scale_after, arm=None):
    """One ordinary step first (so Adam holds state), then the step under test: every parameter and every optimizer
    state tensor keeps its bits, the scale is halved, a parameter gradient is non-finite."""
    import bev_dist
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    bev_dist.train_step(net, batch, targets, opt, loss_cfg, torch.amp.GradScaler("cuda"))
    params, state = _snapshot(net, opt)
    assert len(state) >= 2 * 15
    if arm is not None:
        arm()
    bev_dist.train_step(net, batch, targets, opt, loss_cfg, scaler)
    params2, state2 = _snapshot(net, opt)
    assert _same_bits(params, params2), "a parameter moved in a step that had to be skipped"
    assert _same_bits(state, state2), "optimizer state changed in a step that had to be skipped"
    assert scaler.get_scale() == scale_after, scaler.get_scale()
    bad = [n for n, p in net.named_parameters() if p.grad is not None and not bool(torch.isfinite(p.grad).all())]
    print(f"[grad] skipped step: {len(bad)} parameters with a non-finite gradient")
    assert bad


def test_overflowing_step_is_skipped_fp16_convs(monkeypatch):
    """GradScaler(init_scale = 2^60) with the fp16 convs: the scaled gradients overflow their fp16 storage, so the
    step is skipped and the scale comes down to 2^59."""
    net, batch, targets, loss_cfg = _small_net(monkeypatch, True)
    _skipped_step(net, batch, targets, loss_cfg, torch.amp.GradScaler("cuda", init_scale=2.0 ** 60), 2.0 ** 59)


def _unscaled_grads(monkeypatch, scale):
    net, batch, targets, loss_cfg = _small_net(monkeypatch, False)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    scaler = torch.amp.GradScaler("cuda", init_scale=scale)
    with torch.autocast("cuda", dtype=torch.float16):
        loss = net.loss(net(batch), targets, loss_cfg)["total_loss"]
    scaler.scale(loss).backward()
    scaler.unscale_(opt)
    return {n: p.grad.detach().cpu().numpy() for n, p in net.named_parameters() if p.grad is not None}


def test_step_at_scale_2_60_is_taken_in_fp32(monkeypatch):
    """The same scale with AMP_HALF_CONVS = False: nothing overflows in fp32 -- the step is taken and the scale kept --
    and the unscaled gradients (a separate backward + scaler.unscale_) equal those of a run at scale 1 within the
    fp32 bar of test_bevnet_amp_step_matches_reference_fp32_gradients (rtol 1e-3, atol 1e-3 max|ref|)."""
    import bev_dist
    from test_bevnet_gpu import close
    g1, g60 = _unscaled_grads(monkeypatch, 1.0), _unscaled_grads(monkeypatch, 2.0 ** 60)
    assert g1.keys() == g60.keys() and len(g1) >= 15
    for n in g1:
        close(g60[n], g1[n], 1e-3, 1e-3, "unscaled grad " + n)
    net, batch, targets, loss_cfg = _small_net(monkeypatch, False)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 60)
    before, _ = _snapshot(net, opt)
    bev_dist.train_step(net, batch, targets, opt, loss_cfg, scaler)
    assert scaler.get_scale() == 2.0 ** 60
    after, _ = _snapshot(net, opt)
    assert sum(int(not torch.equal(a, b)) for a, b in zip(before, after)) >= 15
    assert all(bool(torch.isfinite(p).all()) for p in after)
    assert all(bool(torch.isfinite(p.grad).all()) for p in net.parameters() if p.grad is not None)


@pytest.mark.parametrize("half", [False, True], ids=["fp32-kernels", "fp16-convs"])
def test_inf_in_the_bev_gradient_skips_the_step(half, monkeypatch):
    """Scale 1, and a backward hook on the fused BEV map that sets one element of its incoming gradient to +Inf: the
    native warp / projection / trunk backward carry it to the parameters, so the step is skipped in both modes."""
    net, batch, targets, loss_cfg = _small_net(monkeypatch, half)
    inner, armed = net._bev_main, []

    def hooked(*a, **kw):
        out = inner(*a, **kw)
        main = out[0] if isinstance(out, tuple) else out
        if armed and main.requires_grad:
            def poison(g):
                g = g.clone()
                g.view(-1)[g.numel() // 2 + 7] = INF
                return g
            main.register_hook(poison)
        return out
    monkeypatch.setattr(net, "_bev_main", hooked)
    _skipped_step(net, batch, targets, loss_cfg, torch.amp.GradScaler("cuda", init_scale=1.0), 0.5,
                  arm=lambda: armed.append(True))
    assert armed


# ======================================================================================================================
# D: gradient magnitude
# ======================================================================================================================
SCALES = [40, 16, -40]


def _exact_entries():
    """name -> run(k): the entry's outputs with every incoming-gradient operand times 2^k (tuple of device tensors)."""
    import bev_native as nat
    from models.encoders import trunk_grad as tg
    e = {}
    g = _gen(9000)
    y = torch.randn(N, HO, WO, 64, generator=g).clamp_min(0).to(DEV)
    dy64 = torch.randn(N, HO, WO, 64, generator=g).to(DEV)
    e["relu_bwd"] = lambda k: (nat.relu_bwd(dy64 * 2.0 ** k, y),)
    cb = _bnb_case("c", "open")
    for name, (a, with_res) in BNB_ACTS.items():
        for frozen in (False, True):
            e[f"batchnorm_bwd-{name}{'-frozen' if frozen else ''}"] = (
                lambda k, a=a, r=with_res, f=frozen: tuple(t for t in _bnb_run(cb, cb.dy * 2.0 ** k, a, r, f, False)[:4]
                                                           if t is not None))
    cg = _gnb_case("c")
    for relu in (False, True):
        e[f"groupnorm_bwd-{'relu' if relu else 'none'}"] = lambda k, r=relu: _gnb_run(cg, cg.dy * 2.0 ** k, r, False)
    for form in POOL_FORMS:
        x, dy = _pool_case(form)
        e[f"maxpool-{form}"] = lambda k, f=form, x=x, dy=dy: (_pool_run(f, x, dy * 2.0 ** k),)
    dz = torch.randn(N, HO, WO, 32, generator=g).to(DEV)
    res = torch.randn(N, H2, W2, 32, generator=g).to(DEV)
    e["dilate_nhwc"] = lambda k: (nat.dilate_nhwc(dz * 2.0 ** k, 2, 1, 1, 20, 32),)
    e["place_strided"] = lambda k: (nat.place_strided(dz * 2.0 ** k, 2, H2, W2),)
    e["place_strided-res"] = lambda k: (nat.place_strided(dz * 2.0 ** k, 2, H2, W2, res * 2.0 ** k),)
    for name in DGRAD:
        for arith in ("f32", "bf16x6"):
            c = _dgrad_case(name)

            def run(k, c=c, arith=arith):
                with nat.conv_arith_mode(arith):
                    r = c.rd * 2.0 ** k if c.rd is not None else None
                    return (tg._dgrad(c.dy.to(DEV) * 2.0 ** k, c.wd, c.H, c.W, c.s, c.p, r),)
            e[f"dgrad-{name}-{arith}"] = run
    for K, s in DW_CASES:
        c = _dw_case(K, s)
        e[f"dw-dgrad-k{K}s{s}"] = lambda k, c=c, K=K: (_dw_dgrad(nat, c.dy.to(DEV) * 2.0 ** k, c.wt, K, c.s, c.p, c.H,
                                                                 c.W),)
    xa = torch.randn(N, HO, WO, 64, generator=g).to(DEV)
    a, b = torch.randn(N, 64, generator=g).to(DEV), torch.randn(N, 64, generator=g).to(DEV)
    e["channel_affine"] = lambda k: (nat.channel_affine(xa * 2.0 ** k, a),)
    e["channel_affine-b"] = lambda k: (nat.channel_affine(xa * 2.0 ** k, a, b * 2.0 ** k),)
    xv = torch.randint(-2, 3, (N, 5, HO, WO, 8), generator=g).float().to(DEV)
    gv = torch.randn(N, HO, WO, 8, generator=g).to(DEV)
    e["view_max_bwd"] = lambda k: (nat.view_max_bwd(xv, gv * 2.0 ** k),)
    return e


EXACT = (["relu_bwd"] + [f"batchnorm_bwd-{n}{f}" for n in BNB_ACTS for f in ("", "-frozen")]
         + ["groupnorm_bwd-none", "groupnorm_bwd-relu"] + [f"maxpool-{f}" for f in POOL_FORMS]
         + ["dilate_nhwc", "place_strided", "place_strided-res"]
         + [f"dgrad-{n}-{a}" for n in DGRAD for a in ("f32", "bf16x6")]
         + [f"dw-dgrad-{i}" for i in DW_IDS] + ["channel_affine", "channel_affine-b", "view_max_bwd"])


@pytest.mark.parametrize("name", EXACT)
def test_gradient_scale_bit_for_bit(name):
    """The deterministic backward kernels on a gradient 2^40, 2^16 and 2^-40 times the unit-scale one return exactly
    that power of two times their unit-scale result (every output: dz, dres, dgamma, dbeta ...).  Derived: a power of
    two commutes with every rounding -- fp32 products and sums, the double partial sums, the final conversions --
    while nothing leaves the normal range (unit-scale magnitudes lie in [1e-9, 1e3]: 2^-40 of them is above 1e-21,
    2^40 below 1e15).  The residual of a fused epilogue is a gradient too and scales with it."""
    entries = _cached("exact-entries", _exact_entries)
    assert sorted(entries) == sorted(EXACT)
    run = entries[name]
    base = run(0)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in base)
    assert any(bool((t != 0).any()) for t in base)
    for k in SCALES:
        out = run(k)
        torch.cuda.synchronize()
        assert len(out) == len(base)
        for i, (t, t0) in enumerate(zip(out, base)):
            assert torch.equal(t, t0 * 2.0 ** k), (name, k, i, int((t != t0 * 2.0 ** k).sum()))


@pytest.mark.parametrize("k", SCALES, ids=["2^40", "2^16", "2^-40"])
@pytest.mark.parametrize("name", [n for n in WGRAD if n != "h16-any"] + [f"dwconv-{i}" for i in DW_IDS] + ["colsum"])
def test_gradient_scale_atomic_kernels(name, k):
    """The kernels that add with float atomics (weight gradients, colsum) on the scaled gradient: their unit-scale
    bar, relative to the scaled float64 reference (1e-4 max|ref|; colsum 1e-5 sum|x| per column)."""
    import bev_native as nat
    if name == "colsum":
        dy = torch.randn(N, HO, WO, 128, generator=_gen(9100)) * 2.0 ** k
        _bound(f"scale-colsum-{k}", "db", nat.colsum(dy.to(DEV)), dy.double().sum((0, 1, 2)),
               1e-5 * dy.double().abs().sum((0, 1, 2)))
        return
    if name.startswith("dwconv"):
        K, st = int(name[-3]), int(name[-1])
        c = _dw_case(K, st)
        dy = c.dy * 2.0 ** k
        got = _d(nat.dwconv_wgrad(c.x.to(DEV), dy.to(DEV), K, c.s, c.p)).t().reshape(c.C, 1, K, K)
        w = torch.zeros(c.C, 1, K, K, dtype=torch.float64, requires_grad=True)
        F.conv2d(_nchw(c.x.double()), w, None, c.s, c.p, 1, c.C).backward(_nchw(dy.double()))
        ref = w.grad
    else:
        c = _wgrad_case(name)
        dy = c.dy * 2.0 ** k
        got, ref = _d(_wgrad_run(name, c, dy)), _wgrad_ref(c, dy)
    _per(f"scale-wgrad-{name}-{k}", "dW", got, ref, 1e-4, tuple(range(ref.dim())))


@pytest.mark.parametrize("k", [4, -4], ids=["2^4", "2^-4"])
def test_gradient_scale_h16(k):
    """conv_wgrad_h16_any and _dgrad_h16 on an fp32-stored gradient times 2^4 / 2^-4: nothing leaves the fp16 range
    (max |dz| 2^4 < 65504, asserted; at 2^-4 the smallest elements become fp16-subnormal, which the kernel's own
    rounding of the stored fp32 value keeps -- the reference takes that rounding).  The fp16 family's bounds relative
    to the scaled reference."""
    import bev_native as nat
    from models.encoders import trunk_grad as tg
    c = _wgrad_case("h16-any")
    dy = c.dy * 2.0 ** k
    assert float(dy.abs().max()) < 65504
    got = _d(_wgrad_run("h16-any", c, dy))
    dy = dy.half().float()
    _bound(f"scale-wgrad-h16-{k}", "dW", got, _wgrad_ref(c, dy), 2e-6 * (_wgrad_ref(c, dy, absolute=True) + 1e-12))
    for name in ("3x3s1-res", "3x3s2-ryrx"):
        d = _dgrad_case(name, Co=64, fp16=True)
        dz = d.dy * 2.0 ** k
        assert float(dz.abs().max()) < 65504
        res = d.res * 2.0 ** k if d.res is not None else None
        with nat._half_mode(True):
            out = tg._dgrad_h16(dz.to(DEV), d.wd, d.H, d.W, d.s, d.p, res.to(DEV) if res is not None else None)
        torch.cuda.synchronize()
        dd = types.SimpleNamespace(**vars(d))
        dd.res = res
        dz = dz.half().float()
        _bound(f"scale-dgrad-h16-{name}-{k}", "dx", out, _dgrad_ref(dd, dz),
               64 * d.K * d.K * 2.0 ** -24 * _dgrad_ref(dd, dz, absolute=True) + 1e-6 * 2.0 ** k)


@pytest.mark.parametrize("k", SCALES, ids=["2^40", "2^16", "2^-40"])
@pytest.mark.parametrize("mode", ["views", "sum", "mean"])
def test_gradient_scale_warp_bwd(mode, k):
    """The warp backward (float atomics) on a scaled gradient: its bar relative to the scaled reference."""
    c = _warp_case("warp_w3_v3")
    go = _warp_gout(c, mode, None, 0.0, k)
    ref = _warp_ref(c, go, None if mode == "views" else mode)
    _bound(f"scale-warp-{mode}-{k}", "d feats", _warp_run(c, go, mode, 0), ref, 1e-4 * ref.abs() + 5e-5 * 2.0 ** k)


@pytest.mark.parametrize("k", SCALES, ids=["2^40", "2^16", "2^-40"])
def test_gradient_scale_head_operand_and_losses(k):
    """The remaining deterministic entries, bit for bit: head_operand_bwd's copy (both forms), focal_loss_bwd and
    l1_losses_bwd with the incoming loss gradient -- where GradScaler's factor enters the native path -- times 2^k
    (l1's atomic adds meet at most two addends per cell, and a + b = b + a).  The bias gradient of
    head_operand_bwd_bias (block partials) meets 1e-5 sum|terms| of the scaled float64 sum."""
    import bev_native as nat
    f = 2.0 ** k
    P = 18
    gx = torch.randn(N, HO, 16, 24, generator=_gen(9200))
    gs0, (gs1, gb0) = nat.head_operand_bwd(gx.to(DEV), P), nat.head_operand_bwd_bias(gx.to(DEV), P)
    gs, (gs2, gb) = nat.head_operand_bwd((gx * f).to(DEV), P), nat.head_operand_bwd_bias((gx * f).to(DEV), P)
    assert torch.equal(gs, gs0 * f) and torch.equal(gs2, gs1 * f) and torch.equal(gs, gs2) and bool((gs0 != 0).any())
    ref = (gx * f)[..., :P].double()
    _bound(f"scale-head_operand_bwd_bias-{k}", "gbias", gb, ref.sum((0, 1, 2)), 1e-5 * ref.abs().sum((0, 1, 2)))
    x, gt = _focal_case()
    xd, gd = x.to(DEV), gt.to(DEV)
    _, inv = nat.focal_loss(xd, gd, 2.0, 4.0)
    dx0 = nat.focal_loss_bwd(xd, gd, 2.0, 4.0, torch.tensor(1.7, device=DEV), inv)
    dx = nat.focal_loss_bwd(xd, gd, 2.0, 4.0, torch.tensor(1.7, device=DEV) * f, inv)
    assert float(dx0.abs()[dx0 != 0].min()) * 2.0 ** -40 > 1e-30  # nothing leaves the normal range
    assert torch.equal(dx, dx0 * f) and bool((dx0 != 0).any())
    ops = [t.to(DEV) for t in _l1_case()]
    out = nat.l1_losses(*ops)
    gl = torch.tensor([1.3, 0.7], device=DEV)
    d0, d1 = nat.l1_losses_bwd(*ops, gl, out), nat.l1_losses_bwd(*ops, gl * f, out)
    torch.cuda.synchronize()
    for a, b in zip(d0, d1):
        assert torch.equal(b, a * f) and bool((a != 0).any())


@pytest.mark.parametrize("k", SCALES, ids=["2^40", "2^16", "2^-40"])
def test_gradient_scale_proj1x1_and_fused_max(k):
    """Proj1x1's backward and the max-fused warp backward on a scaled gradient: d feat of the projection (a
    deterministic conv) bit for bit; its dW / db (float atomics) and the max-fused scatter within their unit-scale
    bars against the scaled float64 reference."""
    f = 2.0 ** k
    gy = _proj_case()[3]
    got0, _ = _proj_both(gy)
    got, ref = _proj_both(gy * f)
    assert torch.equal(got[0], got0[0] * f)
    _per(f"scale-proj1x1-{k}", "dW", got[1], ref[1], 1e-4, (0, 1, 2, 3))
    _per(f"scale-proj1x1-{k}", "db", got[2], ref[2], 1e-4, (0,))
    c = _warp_case("warp_w3_v3")
    got, ref = _fused_max_both(c, _fused_max_gm(c) * f)
    _bound(f"scale-fused-max-{k}", "d feats", got, ref, 1e-4 * ref.abs() + 5e-5 * f)
