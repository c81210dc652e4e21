"""Host side of the EfficientNet "f16" inference arithmetic: where it applies, the four new C entry points and their
argument rules.  No GPU: every call below has N = 0 or is rejected, so the library answers before any HIP call and the
made-up addresses are never handed to a kernel (the style of test_capi.py's fp16 conv rows)."""
import os
import re
import subprocess

import pytest

from conftest import PKG, REPO

HEADER = os.path.join(REPO, "include", "bev_mi355x.h")
LIB = os.path.join(PKG, "libbev_mi355x.so")
ENTRIES = ("bev_conv2d_stem3_h16", "bev_dwconv2d_h16", "bev_ir_expand_dw_h16", "bev_conv2d_pw_h16")


@pytest.fixture(scope="module")
def lib():
    import bev_native
    if not os.path.exists(LIB):
        bev_native.build()
    return bev_native.lib()


@pytest.mark.parametrize("name", ["efficientnet_b0", "efficientnet_b1", "efficientnet_b2", "efficientnet_b3"])
def test_f16_applies_up_to_index_2(name):
    from models.encoders.efficientnet import EFFICIENTNETS
    net = EFFICIENTNETS[name]()
    assert [net.f16_applies(i) for i in range(5)] == [True, True, True, False, False]
    assert not net.f16_applies(5)
    net.ir_fuse = False  # without the fused kernel the inverted residuals have no fp16 form
    assert [net.f16_applies(i) for i in range(5)] == [True, False, False, False, False]


def test_header_declares_and_library_exports_the_entry_points(lib):
    import bev_native
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for e in ENTRIES + ("bev_dwconv_h16_psum_blocks",):
        assert re.search(r"\bint\s+" + e + r"\s*\(", txt), e
        assert e in exported and e in bev_native.SIGNATURES, e
    assert lib.bev_abi_version() == 18  # entry points were added, no signature of theirs changed (17: retired tuning-knob
    # values; 18: the BatchNorm tile partials became double)


_ORDER = {
    "bev_conv2d_stem3_h16": "x N H W wt bias Co act y Ho Wo stream",
    "bev_dwconv2d_h16": "x N H W C wt bias K stride pad act y Ho Wo psum stream",
    "bev_ir_expand_dw_h16": "x N H W Ci we be Cm wd bd K stride y Ho Wo psum stream",
    "bev_conv2d_pw_h16": "x N H W Ci w bias gate residual Co y y_half ldy stream",
}
_BASE = {
    "bev_conv2d_stem3_h16": dict(x=0x10000, N=0, H=16, W=24, wt=0x20000, bias=0x30000, Co=32, act=2, y=0x40000, Ho=8,
                                 Wo=12, stream=None),
    "bev_dwconv2d_h16": dict(x=0x10000, N=0, H=8, W=8, C=32, wt=0x20000, bias=0x30000, K=3, stride=1, pad=1, act=2,
                             y=0x40000, Ho=8, Wo=8, psum=0x50000, stream=None),
    "bev_ir_expand_dw_h16": dict(x=0x10000, N=0, H=8, W=8, Ci=24, we=0x20000, be=0x30000, Cm=144, wd=0x60000,
                                 bd=0x70000, K=3, stride=1, y=0x40000, Ho=8, Wo=8, psum=0x50000, stream=None),
    "bev_conv2d_pw_h16": dict(x=0x10000, N=0, H=8, W=8, Ci=144, w=0x20000, bias=0x30000, gate=0x50000, residual=0x60000,
                              Co=24, y=0x40000, y_half=1, ldy=24, stream=None),
}
_ROWS = (
    [(e, {}, 0) for e in _ORDER]
    # a null pointer is refused (with N > 0 too: the check comes before the empty-batch return)
    + [(e, {k: None}, -1) for e in _ORDER for k in ("x", "y")]
    + [(e, {k: None, "N": n}, -1) for e in _ORDER for k in ("x", "y") for n in (1, 2)]
    + [("bev_conv2d_stem3_h16", {k: None}, -1) for k in ("wt", "bias")]
    + [("bev_dwconv2d_h16", {k: None}, -1) for k in ("wt", "bias")]
    + [("bev_ir_expand_dw_h16", {k: None}, -1) for k in ("we", "be", "wd", "bd", "psum")]
    + [("bev_conv2d_pw_h16", {"w": None}, -1)]
    # optional pointers
    + [("bev_dwconv2d_h16", {"psum": None}, 0)]
    + [("bev_conv2d_pw_h16", {k: None}, 0) for k in ("bias", "gate", "residual")]
    + [(e, {"N": -1}, -1) for e in _ORDER] + [(e, {"H": 0}, -1) for e in _ORDER] + [(e, {"W": 0}, -1) for e in _ORDER]
    # misaligned pointers (8 mod 16)
    + [("bev_conv2d_stem3_h16", {"y": 0x40008}, -1)]
    + [("bev_dwconv2d_h16", {k: _BASE["bev_dwconv2d_h16"][k] + 8}, -1) for k in ("x", "wt", "bias", "y", "psum")]
    + [("bev_ir_expand_dw_h16", {k: _BASE["bev_ir_expand_dw_h16"][k] + 8}, -1) for k in ("x", "we", "be", "bd", "y", "psum")]
    + [("bev_ir_expand_dw_h16", {"wd": 0x60001}, -1), ("bev_ir_expand_dw_h16", {"wd": 0x60002}, 0)]
    + [("bev_conv2d_pw_h16", {k: _BASE["bev_conv2d_pw_h16"][k] + 8}, -1) for k in ("x", "w", "bias", "gate", "residual", "y")]
    # widths, kernel sizes, strides
    + [("bev_conv2d_stem3_h16", {"Co": c}, 0 if c in (32, 40, 48, 64) else -1) for c in (0, 16, 24, 32, 40, 48, 56, 64, 72)]
    + [("bev_conv2d_stem3_h16", {"act": 3}, -1), ("bev_conv2d_stem3_h16", {"Ho": 9}, -1),
       ("bev_conv2d_stem3_h16", {"Wo": 11}, -1)]
    + [("bev_dwconv2d_h16", {"C": c}, 0 if c in (8, 24, 40, 256) else -1) for c in (0, 4, 8, 12, 24, 36, 40, 256, 264, 288)]
    + [("bev_dwconv2d_h16", {"K": k, "pad": k // 2}, 0 if k in (3, 5) else -1) for k in (1, 2, 3, 4, 5, 7)]
    + [("bev_dwconv2d_h16", {"stride": s, "Ho": (8 - 1) // max(s, 1) + 1, "Wo": (8 - 1) // max(s, 1) + 1},
        0 if s in (1, 2) else -1) for s in (0, 1, 2, 3)]
    + [("bev_dwconv2d_h16", d, -1) for d in (dict(act=-1), dict(act=3), dict(pad=-1), dict(Ho=7), dict(Wo=9),
                                             dict(pad=0), dict(y=0x10000))]
    + [("bev_ir_expand_dw_h16", {"Ci": c}, 0 if c in (16, 24, 32, 40, 48) else -1) for c in (0, 8, 16, 20, 24, 32, 40, 48, 56, 64)]
    + [("bev_ir_expand_dw_h16", {"Cm": c}, 0 if c in (48, 96, 288) else -1) for c in (0, 24, 48, 64, 96, 100, 288)]
    + [("bev_ir_expand_dw_h16", {"K": k}, 0 if k in (3, 5) else -1) for k in (1, 3, 4, 5, 7)]
    + [("bev_ir_expand_dw_h16", {"stride": 2, "Ho": 4, "Wo": 4}, 0), ("bev_ir_expand_dw_h16", {"stride": 2}, -1),
       ("bev_ir_expand_dw_h16", {"stride": 0}, -1), ("bev_ir_expand_dw_h16", {"stride": 3, "Ho": 3, "Wo": 3}, -1),
       ("bev_ir_expand_dw_h16", {"Ho": 7}, -1), ("bev_ir_expand_dw_h16", {"y": 0x10000}, -1)]
    + [("bev_conv2d_pw_h16", {"Ci": c}, 0 if c in (8, 24, 40, 288, 512) else -1) for c in (0, 4, 8, 12, 24, 40, 288, 512, 520)]
    + [("bev_conv2d_pw_h16", {"Co": c, "ldy": max(c, 8)}, 0 if c in (8, 16, 72, 1280) else -1)
       for c in (0, 4, 8, 12, 16, 20, 72, 1280)]
    + [("bev_conv2d_pw_h16", d, 0) for d in (dict(ldy=32), dict(y_half=0), dict(y_half=0, ldy=64))]
    + [("bev_conv2d_pw_h16", d, -1) for d in (dict(ldy=16), dict(ldy=28), dict(y_half=2), dict(y_half=-1),
                                              dict(y=0x10000), dict(y=0x60000))]  # an output aliases an input
)


def _call(lib, entry, changes):
    args = dict(_BASE[entry])
    args.update(changes)
    rejected_or_empty = args["N"] <= 0 or any(args[k] is None for k in ("x", "y"))
    assert rejected_or_empty, "only empty or rejected calls: nothing may reach a kernel"
    return getattr(lib, entry)(*[args[k] for k in _ORDER[entry].split()])


def test_entry_point_argument_rules_without_gpu(lib):
    assert len(_ROWS) > 120 and {e for e, _, _ in _ROWS} == set(ENTRIES)
    bad = [(e, c, want, got) for e, c, want in _ROWS for got in [_call(lib, e, c)] if got != want]
    assert not bad, bad


def test_partial_count_queries(lib):
    # the depthwise row runs: 8 (stride 1) / 4 (stride 2) outputs per run, 256 / (C / 4) runs per workgroup
    assert lib.bev_dwconv_h16_psum_blocks(11, 19, 32, 1) == (11 * 3 + 31) // 32
    assert lib.bev_dwconv_h16_psum_blocks(11, 19, 40, 2) == (11 * 5 + 24) // 25
    for bad in ((0, 19, 32, 1), (11, 0, 32, 1), (11, 19, 36, 1), (11, 19, 264, 1), (11, 19, 32, 3)):
        assert lib.bev_dwconv_h16_psum_blocks(*bad) == -1, bad


def test_wrappers_refuse_cpu_tensors():
    import torch
    import bev_native as nat
    h, f = torch.zeros(1, 8, 8, 24, dtype=torch.float16), torch.zeros(24)
    with pytest.raises(nat.HipError):
        nat.conv2d_stem3_h16(torch.zeros(1, 3, 8, 8), torch.zeros(27, 32), torch.zeros(32), nat.ACT_SILU)
    with pytest.raises(nat.HipError):
        nat.dwconv2d_nhwc_h16(h, torch.zeros(9, 24, dtype=torch.float16), f, 3, 1, 1, nat.ACT_SILU)
    with pytest.raises(nat.HipError):
        nat.ir_expand_dw_h16(h, torch.zeros(144, 24, dtype=torch.float16), torch.zeros(144),
                             torch.zeros(9, 144, dtype=torch.float16), torch.zeros(144), 3, 1)
    with pytest.raises(nat.HipError):
        nat.conv2d_pw_h16(h, torch.zeros(24, 24, dtype=torch.float16), f)
