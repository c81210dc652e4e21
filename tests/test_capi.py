"""C ABI of libbev_mi355x.so (include/bev_mi355x.h): loads, exports every declared
entry point, validates arguments on the host.  No GPU compute is launched here."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, PKG, REPO

HEADER = os.path.join(REPO, "include", "bev_mi355x.h")
LIB = os.path.join(PKG, "libbev_mi355x.so")


def declared_symbols():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(bev_[a-z0-9_]+)\s*\(", txt)))


@pytest.fixture(scope="module")
def lib():
    import bev_native
    if not os.path.exists(LIB):
        bev_native.build()
    return bev_native.lib()


def test_every_declared_symbol_is_exported(lib):
    syms = declared_symbols()
    assert len(syms) >= 15, syms
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    missing = [s for s in syms if s not in exported]
    assert not missing, missing
    for s in syms:
        assert hasattr(lib, s)


def test_ctypes_signatures_cover_header(lib):
    import bev_native
    assert sorted(bev_native.SIGNATURES) == declared_symbols()


def test_abi_version(lib):
    import bev_native
    assert lib.bev_abi_version() == bev_native.ABI_VERSION == 18


def test_abi_16_retired_the_fused_next_chain(lib):
    """ABI 16 removed the pre-split chain that also ran the next block's conv1: the library no longer exports the
    entry point (its name is spelled in two halves so the tree stays free of it), at 16 or any later number
    (test_abi_version pins the current one)."""
    gone = "bev_conv2d_chain_" + "next_x6_f32"
    assert lib.bev_abi_version() >= 16
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    assert gone not in {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert gone not in declared_symbols()


def test_linspace_host_entry_bit_exact(lib):
    """bev_linspace_f32 (host) == torch.linspace CPU as the reference calls it (geometry.py:26-27)."""
    import bev_native
    d = np.load(os.path.join(GOLDEN, "linspace_cases.npz"))
    pos = 0
    for lo, hi, n in zip(d["lo"], d["hi"], d["n"]):
        ref = d["out"][pos:pos + n]
        pos += n
        got = bev_native.linspace(float(lo), float(hi), int(n)).numpy()
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (lo, hi, n)


def test_argument_validation_without_gpu(lib):
    """Bad shapes are rejected on the host with BEV_ERR_ARGS (-1) before any launch."""
    null = None
    assert lib.bev_ipm_warp_f32(null, 0, 0, 0, 0, null, null, null, -1, 1, 1, 1, 1.0, 1.0, 1, 1, null, null) == -1
    assert lib.bev_ipm_warp_f32(null, 0, 0, 0, 0, null, null, null, 1, 1, 0, 1, 1.0, 1.0, 1, 1, null, null) == -1
    assert lib.bev_ipm_warp_fuse_f32(null, 0, 0, 0, 0, null, null, null, 1, 0, 1, 1, 1, 1.0, 1.0, 1, 1, 1, null,
                                     null) == -1
    assert lib.bev_ipm_warp_fuse_f32(null, 0, 0, 0, 0, null, null, null, 1, 1, 1, 1, 1, 1.0, 1.0, 1, 1, 7, null,
                                     null) == -1  # bad mode
    assert lib.bev_view_fuse_f32(null, 1, 0, 10, 0, null, null) == -1
    assert lib.bev_ipm_warp_fuse_bwd_f32(null, null, null, null, 1, 1, 1, 1, 1, 1.0, 1.0, 1, 1, 2, null, null) == -1
    # conv: output size inconsistent with the geometry, null pointers
    assert lib.bev_conv2d_f32(null, 0, 1, 8, 8, 16, null, null, null, 16, 3, 3, 1, 1, 0, null, 8, 8, null) == -1
    assert lib.bev_conv_packed_size(64, 64, 3, 3) > 0
    assert lib.bev_conv_packed_size(0, 64, 3, 3) == 0
    assert lib.bev_maxpool2d_nhwc_f32(null, 1, 8, 8, 4, 3, 2, 1, null, 4, 4, null) == -1
    # empty work is a successful no-op
    assert lib.bev_homography_f32(null, null, 0, null, null) == 0


# Argument order of the five fp16 forward conv entry points (include/bev_mi355x.h) and one accepted argument set.
# N = 0 in every row: the library answers (0 or BEV_ERR_ARGS) before any HIP call, so the made-up addresses are
# never handed to a kernel.
_H16_ORDER = {
    "bev_conv2d_h16_f32": "x N H W Ci packed bias residual Co KH KW stride pad dilation act y ldy Ho Wo stream",
    "bev_conv2d_h16_bnstats_f32": "x N H W Ci packed bias Co KH KW stride pad dilation y Ho Wo tile_stats stream",
    "bev_conv2d_h16_ex_f32": "x x_half N H W Ci packed bias residual Co KH KW stride pad dilation act y ldy Ho Wo "
                             "tile_stats stream",
    "bev_conv2d_h16_h16": "x x_half N H W Ci packed bias residual Co KH KW stride pad dilation act y Ho Wo stream",
    "bev_conv2d_h16_affine": "x x_half N H W Ci in_scale in_shift in_relu packed bias Co KH KW stride pad dilation act "
                             "y y_half ldy Ho Wo stream",
}
_H16_BASE = dict(x=0x10000, x_half=1, N=0, H=8, W=8, Ci=64, packed=0x20000, bias=None, residual=None, Co=64, KH=3, KW=3,
                 stride=1, pad=1, dilation=1, act=0, y=0x30000, y_half=1, ldy=64, Ho=8, Wo=8, tile_stats=None,
                 in_scale=None, in_shift=None, in_relu=0, stream=None)
_H16_F32 = ("bev_conv2d_h16_f32", "bev_conv2d_h16_bnstats_f32", "bev_conv2d_h16_ex_f32")
_H16_COMMON = [  # one rule violated -> -1 from every entry that has the argument
    dict(x=None), dict(packed=None), dict(y=None), dict(N=-1), dict(H=0), dict(W=0), dict(Ci=0), dict(Co=0), dict(KH=0),
    dict(KW=0), dict(stride=0), dict(dilation=0), dict(pad=-1), dict(act=-1), dict(act=3),
    dict(Ho=7), dict(Wo=9), dict(stride=2),          # Ho / Wo inconsistent with the geometry
    dict(H=1, pad=0, Ho=-1, Wo=6),                   # consistent, but no output row
    dict(x=0x10008), dict(packed=0x20008),           # 8 mod 16
]
_H16_ROWS = (
    [(e, {}, 0) for e in _H16_ORDER]
    + [(e, v, -1) for e in _H16_ORDER for v in _H16_COMMON if set(v) <= set(_H16_ORDER[e].split())]
    # fp32-output entries: 32-channel K steps, ldy >= Co, a residual needs dense rows, y alignment is not checked
    + [(e, dict(Ci=96, x_half=0), 0) for e in ("bev_conv2d_h16_f32", "bev_conv2d_h16_ex_f32")]
    + [(e, dict(Ci=48, x_half=0), -1) for e in _H16_F32]
    + [(e, dict(y=0x30002), 0) for e in _H16_F32]
    + [(e, dict(ldy=63), -1) for e in ("bev_conv2d_h16_f32", "bev_conv2d_h16_ex_f32")]
    + [(e, dict(ldy=128), 0) for e in ("bev_conv2d_h16_f32", "bev_conv2d_h16_ex_f32")]
    + [(e, dict(ldy=128, residual=0x40000), -1) for e in ("bev_conv2d_h16_f32", "bev_conv2d_h16_ex_f32")]
    + [(e, dict(residual=0x30000), 0) for e in ("bev_conv2d_h16_f32", "bev_conv2d_h16_ex_f32")]  # y may alias it
    + [("bev_conv2d_h16_bnstats_f32", dict(tile_stats=None), -1),
       ("bev_conv2d_h16_bnstats_f32", dict(Ci=96), -1),                            # statistics: k_conv_h16b only
       ("bev_conv2d_h16_ex_f32", dict(tile_stats=0x40000), 0),
       ("bev_conv2d_h16_ex_f32", dict(tile_stats=0x40000, act=1), -1),
       ("bev_conv2d_h16_ex_f32", dict(tile_stats=0x40000, residual=0x50000), -1),
       ("bev_conv2d_h16_ex_f32", dict(tile_stats=0x40000, Ci=96, x_half=0), -1),   # statistics: k_conv_h16b only
       ("bev_conv2d_h16_ex_f32", dict(x_half=1, Ci=96), -1),                       # fp16 operand: k_conv_h16b only
       # fp16 in, fp16 out: 64-channel K steps, 8-channel output groups, everything 16-B aligned, no aliasing
       ("bev_conv2d_h16_h16", dict(x_half=0), 0),
       ("bev_conv2d_h16_h16", dict(residual=0x40000), 0),
       ("bev_conv2d_h16_h16", dict(Ci=96), -1),
       ("bev_conv2d_h16_h16", dict(Co=60), -1),
       ("bev_conv2d_h16_h16", dict(y=0x30008), -1),
       ("bev_conv2d_h16_h16", dict(residual=0x40008), -1),
       ("bev_conv2d_h16_h16", dict(residual=0x30000), -1),                         # y == residual, even with M = 0
       # operand affine
       ("bev_conv2d_h16_affine", dict(in_scale=0x50000, in_shift=0x60000, in_relu=1), 0),
       ("bev_conv2d_h16_affine", dict(x_half=0), 0),
       ("bev_conv2d_h16_affine", dict(y_half=0, y=0x30004, ldy=128), 0),
       ("bev_conv2d_h16_affine", dict(y_half=0, Co=60, ldy=60), 0),
       ("bev_conv2d_h16_affine", dict(ldy=63), -1),
       ("bev_conv2d_h16_affine", dict(Ci=96), -1),
       ("bev_conv2d_h16_affine", dict(in_scale=0x50000), -1),
       ("bev_conv2d_h16_affine", dict(in_shift=0x60000), -1),
       ("bev_conv2d_h16_affine", dict(in_scale=0x50000, in_shift=0x60000, x_half=0), -1),
       ("bev_conv2d_h16_affine", dict(Co=60, ldy=60), -1),
       ("bev_conv2d_h16_affine", dict(ldy=128), -1),
       ("bev_conv2d_h16_affine", dict(in_scale=0x50008, in_shift=0x60000), -1),
       ("bev_conv2d_h16_affine", dict(in_scale=0x50000, in_shift=0x60008), -1),
       ("bev_conv2d_h16_affine", dict(y=0x30008), -1),                             # fp16 y: 16 bytes
       ("bev_conv2d_h16_affine", dict(y_half=0, y=0x30002), -1)]                   # fp32 y: 4 bytes
)


def _h16_call(lib, entry, changes):
    args = dict(_H16_BASE, tile_stats=0x40000 if entry == "bev_conv2d_h16_bnstats_f32" else None)
    args.update(changes)
    assert args["N"] <= 0, "only empty or rejected calls: nothing may reach a kernel"
    return getattr(lib, entry)(*[args[k] for k in _H16_ORDER[entry].split()])


def test_conv_h16_argument_rules_without_gpu(lib):
    """The fp16 forward convs' per-entry argument rules: every row is an accepted argument set (-> 0) or that set with
    one rule broken (-> BEV_ERR_ARGS), with N = 0 so that either answer comes before any HIP call.  No answer depends
    on BEV_TUNE_CONV_H16_KERNEL: 1 selects the 32-deep kernel for fp32 operands without statistics only, and the
    fp16-output and affine entries never run it."""
    import bev_native as nat
    assert len(_H16_ROWS) > 100 and {e for e, _, _ in _H16_ROWS} == set(_H16_ORDER)
    bad = [(e, c, want, got) for e, c, want in _H16_ROWS for got in [_h16_call(lib, e, c)] if got != want]
    assert not bad, bad
    for kern in (1, 2, 3):
        with nat.tuned(CONV_H16_KERNEL=kern):
            bad = [(kern, e, c, want, got) for e, c, want in _H16_ROWS for got in [_h16_call(lib, e, c)] if got != want]
        assert not bad, bad


# Argument order of the six split-bf16 (x6) conv entry points (include/bev_mi355x.h).  The four tensor entries get one
# accepted argument set each, with N = 0 so that the answer comes before any HIP call; the two stem entries reject
# N = 0, so their base set (N = 1) would launch and only rows with one rule broken are called.
_X6_ORDER = {
    "bev_conv2d_x6_f32": "x xs N H W Ci packed bias residual Co KH KW stride pad dilation act y ys ldy Ho Wo stream",
    "bev_conv2d_dual_x6_f32": "x N Ho Wo Ci x2 H2 W2 Ci2 stride2 packed bias Co act y stream",
    "bev_conv2d_chain_x6_f32": "x xs N H W Ci packed bias Co KH KW stride pad act packed2 bias2 Co2 residual act2 y Ho Wo "
                               "stream",
    "bev_conv2d_chain_dual_x6_f32": "x xs N H W Ci packed bias Co KH KW stride pad act x2 H2 W2 Ci2 stride2 packed2 bias2 "
                                    "Co2 act2 y Ho Wo stream",
    "bev_conv2d_stem_x6_f32": "x N H W packed bias Co relu y Ho Wo stream",
    "bev_conv2d_stem_pool_x6_f32": "x N H W packed bias Co y Hp Wp workspace workspace_bytes stream",
}
_X6_PLAIN, _X6_DUAL, _X6_CHAIN, _X6_CDUAL, _X6_STEM, _X6_SPOOL = _X6_ORDER
_X6_TENSOR = (_X6_PLAIN, _X6_DUAL, _X6_CHAIN, _X6_CDUAL)
_X6_BASE = dict(x=0x10000, xs=None, N=0, H=8, W=8, Ci=64, packed=0x20000, bias=None, residual=None, Co=64, KH=3, KW=3,
                stride=1, pad=1, dilation=1, act=0, y=0x30000, ys=None, ldy=64, Ho=8, Wo=8, stream=None,
                x2=0x40000, H2=8, W2=8, Ci2=64, stride2=1, packed2=0x50000, bias2=None, Co2=256, act2=1)
_X6_STEM_BASE = {  # 16 x 16 image -> 8 x 8 stem output; 32 x 32 -> 16 x 16 -> 8 x 8 pooled
    _X6_STEM: dict(x=0x10000, N=1, H=16, W=16, packed=0x20000, bias=0x70000, Co=64, relu=1, y=0x30000, Ho=8, Wo=8,
                   stream=None),
    _X6_SPOOL: dict(x=0x10000, N=1, H=32, W=32, packed=0x20000, bias=0x70000, Co=64, y=0x30000, Hp=8, Wp=8,
                    workspace=0xA0000, workspace_bytes=1 << 30, stream=None),
}
_X6_COMMON = [  # one rule violated -> -1 from every tensor entry that has the argument
    dict(x=None), dict(xs=0x60000),                  # exactly one of x / xs
    dict(packed=None), dict(packed2=None), dict(x2=None), dict(y=None), dict(N=-1), dict(H=0), dict(W=0), dict(Co=0),
    dict(KH=0), dict(KW=0), dict(stride=0), dict(pad=-1), dict(act=-1), dict(act=3), dict(act2=-1), dict(act2=3),
    dict(H2=0), dict(W2=0), dict(stride2=0), dict(Co2=0), dict(Co2=-64), dict(Co2=96),
    dict(Ho=7), dict(Wo=9), dict(stride=2), dict(stride2=2),  # Ho / Wo inconsistent with the geometry
    dict(H=1, pad=0, Ho=-1, Wo=6),                   # consistent, but no output row
    dict(x=0x10008), dict(x=None, xs=0x60008), dict(packed=0x20008), dict(packed2=0x50008),  # 8 mod 16
    dict(Ci=40),                                     # no whole K step in any entry
]
_X6_ROWS = (
    [(e, {}, 0) for e in _X6_TENSOR]
    + [(e, v, -1) for e in _X6_TENSOR for v in _X6_COMMON if set(v) <= set(_X6_ORDER[e].split())]
    # never checked by any entry: the alignment of y, bias, bias2 and the residual
    + [(e, v, 0) for e in _X6_TENSOR for v in (dict(y=0x30004), dict(bias=0x70004), dict(bias2=0x70004),
                                               dict(residual=0x80004), dict(residual=0x30000))
       if set(v) <= set(_X6_ORDER[e].split())]
    # a pre-split operand in place of x (K steps of 32 channels)
    + [(e, dict(x=None, xs=0x60000), 0) for e in (_X6_PLAIN, _X6_CHAIN, _X6_CDUAL)]
    + [(e, dict(x=None, xs=0x60000, Ci=96), 0) for e in (_X6_PLAIN, _X6_CHAIN, _X6_CDUAL)]
    + [(_X6_PLAIN, dict(Ci=48), 0), (_X6_PLAIN, dict(x=None, xs=0x60000, Ci=48), -1),  # fp32 x: 16-channel K steps
       (_X6_PLAIN, dict(Ci=0), -1),
       # only the plain entry has (and checks) a dilation and an output row pitch; ldy >= Co, dense rows for a
       # residual and for split output
       (_X6_PLAIN, dict(dilation=0), -1), (_X6_PLAIN, dict(dilation=2), -1),
       (_X6_PLAIN, dict(dilation=2, Ho=6, Wo=6), 0),
       (_X6_PLAIN, dict(ldy=63), -1), (_X6_PLAIN, dict(ldy=128), 0),
       (_X6_PLAIN, dict(residual=0x80000), 0), (_X6_PLAIN, dict(residual=0x80000, ldy=128), -1),
       # exactly one of y / ys; split output: ldy == Co, Co % 4 == 0, 8-byte aligned
       (_X6_PLAIN, dict(ys=0x90000), -1), (_X6_PLAIN, dict(y=None, ys=0x90000), 0),
       (_X6_PLAIN, dict(y=None, ys=0x90008), 0), (_X6_PLAIN, dict(y=None, ys=0x90004), -1),
       (_X6_PLAIN, dict(y=None, ys=0x90000, ldy=128), -1), (_X6_PLAIN, dict(y=None, ys=0x90000, Co=62, ldy=62), -1),
       (_X6_PLAIN, dict(Co=62, ldy=62), 0), (_X6_PLAIN, dict(y=None, ys=0x90000, residual=0x80000), 0),
       # dual: both K parts in 16-channel steps, the shortcut operand aligned, geometry from (H2, W2, stride2)
       (_X6_DUAL, dict(Ci=48), 0), (_X6_DUAL, dict(Ci2=48), 0), (_X6_DUAL, dict(Ci2=40), -1),
       (_X6_DUAL, dict(Ci=0), -1), (_X6_DUAL, dict(Ci2=0), -1), (_X6_DUAL, dict(Ho=0), -1), (_X6_DUAL, dict(Wo=0), -1),
       (_X6_DUAL, dict(x2=0x40008), -1), (_X6_DUAL, dict(stride2=2, Ho=4, Wo=4), 0), (_X6_DUAL, dict(Co=60), 0),
       # chain: 32-channel K steps; h2 of 64 or 128 channels; Co2 in 64s
       (_X6_CHAIN, dict(Ci=48), -1), (_X6_CHAIN, dict(Ci=96), 0), (_X6_CHAIN, dict(Co=32), -1),
       (_X6_CHAIN, dict(Co=256), -1), (_X6_CHAIN, dict(Co=128), 0), (_X6_CHAIN, dict(Co2=64), 0),
       (_X6_CHAIN, dict(residual=0x80000), 0), (_X6_CHAIN, dict(bias=0x70000, bias2=0x70100), 0),
       # QUIRK: Co = 128 needs Co2 % 128 == 0 (two waves share a 32-row band), but that is checked after the N == 0
       # return, so the empty call answers 0
       (_X6_CHAIN, dict(Co=128, Co2=64), 0),
       # QUIRK: the chain entries check Ci % 32 only, not its sign: with N = 0 a zero Ci is accepted
       (_X6_CHAIN, dict(Ci=0), 0), (_X6_CDUAL, dict(Ci=0), 0),
       # chain + shortcut: the layer1 block-0 shape only (Co 64, Ci2 64); x2 aligned; both geometries give Ho, Wo
       (_X6_CDUAL, dict(Ci=48), -1), (_X6_CDUAL, dict(Ci=96), 0), (_X6_CDUAL, dict(Co=128), -1),
       (_X6_CDUAL, dict(Co=32), -1), (_X6_CDUAL, dict(Ci2=128), -1), (_X6_CDUAL, dict(Ci2=32), -1),
       (_X6_CDUAL, dict(Co2=64), 0), (_X6_CDUAL, dict(x2=0x40008), -1), (_X6_CDUAL, dict(H2=16), -1),
       (_X6_CDUAL, dict(W2=16), -1), (_X6_CDUAL, dict(H2=16, W2=16, stride2=2), 0)]
    # QUIRK: the stem entries reject N == 0, where the tensor entries answer 0
    + [(e, v, -1) for e in (_X6_STEM, _X6_SPOOL) for v in (
        dict(N=0), dict(N=-1), dict(x=None), dict(packed=None), dict(bias=None), dict(y=None), dict(H=0), dict(W=0),
        dict(packed=0x20008))]
    + [(_X6_STEM, v, -1) for v in (dict(Co=0), dict(Co=65), dict(Ho=7), dict(Wo=9), dict(H=18), dict(W=18))]
    + [(_X6_SPOOL, v, -1) for v in (dict(Co=32), dict(Co=0), dict(Hp=7), dict(Wp=9), dict(H=36), dict(W=36),
                                    dict(workspace=None), dict(workspace=0xA0008), dict(y=0x30008),
                                    dict(workspace_bytes=0), dict(workspace_bytes=37 * 64 * 4 - 1))]
)


def _x6_call(lib, entry, changes, want):
    args = dict(_X6_STEM_BASE.get(entry, _X6_BASE))
    assert set(changes) <= set(_X6_ORDER[entry].split()), (entry, changes)
    args.update(changes)
    # only empty or rejected calls: nothing may reach a kernel
    assert args["N"] <= 0 if entry in _X6_TENSOR else (want == -1 and changes), (entry, changes)
    return getattr(lib, entry)(*[args[k] for k in _X6_ORDER[entry].split()])


def test_conv_x6_argument_rules_without_gpu(lib):
    """The split-bf16 convs' per-entry argument rules: every row is an accepted argument set (-> 0) or that set with
    one rule broken (-> BEV_ERR_ARGS), answered before any HIP call (N = 0, or a rejected stem call).  The rows marked
    QUIRK pin answers that are what they are, not what one would design.  No answer depends on the knobs that choose
    among the k_conv_x6 / x6b / x6s instances."""
    import bev_native as nat
    assert len(_X6_ROWS) >= 80 and {e for e, _, _ in _X6_ROWS} == set(_X6_ORDER)
    for knobs in ({}, dict(CONV_X6_TILE=1), dict(CONV_X6_TILE=2), dict(CONV_X6_KERNEL=1), dict(CONV_X6_NT=1)):
        with nat.tuned(**knobs):
            bad = [(knobs, e, c, want, got) for e, c, want in _X6_ROWS for got in [_x6_call(lib, e, c, want)]
                   if got != want]
        assert not bad, bad


def test_tune_knobs_host_only(lib):
    """bev_tune: every knob returns its previous value, rejects out-of-range values and unknown knobs;
    no GPU involved (knobs are read at launch)."""
    import bev_native as nat
    assert lib.bev_tune(99, 0) == -1
    for knob, good, bad in ((nat.TUNE_CONV_TILE, 3, 5), (nat.TUNE_WARP_POOL_KB, 16, 151), (nat.TUNE_WARP_KERNEL, 1, 5),
                            (nat.TUNE_WARP_BWD_POOL, 96, 1 << 20),
                            (nat.TUNE_CONV_XCD, 0, 2), (nat.TUNE_CONV_NBUF, 1, 3), (nat.TUNE_CONV_DMA, 2, 3),
                            (nat.TUNE_WGRAD_MFMA, 0, 3), (nat.TUNE_CONV_X6_TILE, 2, 3),
                            (nat.TUNE_CONV_X6_KERNEL, 1, 3), (nat.TUNE_CONV_H16_KERNEL, 1, 4),
                            (nat.TUNE_CONV_PW_SMALL, 0, 5),
                            (nat.TUNE_DW_RUN, 0, 4), (nat.TUNE_CONV_X6_NT, 1, 2),
                            (nat.TUNE_STEM3_STAGE, 1, 3),
                            (nat.TUNE_WARP_SPAN, 50, 101), (nat.TUNE_WARP_TILE_BAND, 4, 65)):
        old = lib.bev_tune(knob, good)
        assert old >= 0
        assert lib.bev_tune(knob, bad) == -1
        assert lib.bev_tune(knob, old) == good
    with nat.tuned(WARP_KERNEL=1, WARP_POOL_KB=8):
        assert lib.bev_tune(nat.TUNE_WARP_KERNEL, 1) == 1
    assert lib.bev_tune(nat.TUNE_WARP_KERNEL, 0) == 0  # the default kernel stays selected
    # the round-6 warp knobs' defaults: span staging off, automatic tile bands
    assert lib.bev_tune(nat.TUNE_WARP_SPAN, 0) == 0
    assert lib.bev_tune(nat.TUNE_WARP_TILE_BAND, 0) == 0
    # removed with ABI 14: the persistent kernel's knob (18, not reused)
    assert lib.bev_tune(18, 0) == -1
    # removed with ABI 17: the values that selected retired depthwise kernels, and an alias
    for knob, value in ((nat.TUNE_DW_RUN, 1), (nat.TUNE_DW_RUN, 2), (nat.TUNE_CONV_X6_KERNEL, 2)):
        assert lib.bev_tune(knob, value) == -1
    # ... and the default reads back unchanged
    assert lib.bev_tune(nat.TUNE_DW_RUN, 3) == 3


def test_no_environment_knobs_in_library():
    """The shipped library reads no environment variables (performance knobs are bev_tune only)."""
    import glob
    for src in glob.glob(os.path.join(PKG, "csrc", "*.hip")) + glob.glob(os.path.join(PKG, "csrc", "*.h")):
        assert "getenv" not in open(src).read(), src
