"""Host-side contract of the "f16" inference arithmetic of the BEV head: the switch (separate from the trunk's), the
two C entries behind it in the header and the binding, and their argument checks.  No GPU."""
import ctypes
import os
import re

import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "bev_mi355x.h")


def test_head_arith_switch():
    import bev_native as nat
    assert nat.HEAD_ARITHS == ("f32", "f16")
    assert nat.head_arith() == "f32"  # the default
    with pytest.raises(ValueError):
        nat.set_head_arith("f8")
    assert nat.head_arith() == "f32"
    prev = nat.set_head_arith("f16")
    assert prev == "f32" and nat.head_arith() == "f16"
    assert nat.set_head_arith(prev) == "f16" and nat.head_arith() == "f32"


def test_head_arith_context_manager_nests_and_restores():
    import bev_native as nat
    with nat.head_arith_mode("f16"):
        assert nat.head_arith() == "f16"
        with nat.head_arith_mode("f32"):
            assert nat.head_arith() == "f32"
            with nat.head_arith_mode("f16"):
                assert nat.head_arith() == "f16"
            assert nat.head_arith() == "f32"
        assert nat.head_arith() == "f16"
    assert nat.head_arith() == "f32"
    with pytest.raises(RuntimeError):
        with nat.head_arith_mode("f16"):
            raise RuntimeError("restored on the way out")
    assert nat.head_arith() == "f32"


def test_head_switch_and_trunk_switch_are_independent():
    import bev_native as nat
    trunk = nat.conv_arith()
    with nat.head_arith_mode("f16"):
        assert nat.conv_arith() == trunk
    with nat.conv_arith_mode("f16"):
        assert nat.head_arith() == "f32"
    assert nat.conv_arith() == trunk


def _params(name):
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", txt)
    assert m, f"{name} is not declared"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_declares_the_head_entries_as_the_binding_has_them():
    import bev_native as nat
    p = _params("bev_conv2d_h16_affine")
    assert len(p) == 24 and p[0] == "const void *x" and p[1] == "int x_half" and p[-1] == "void *stream"
    assert p[6:9] == ["const float *in_scale", "const float *in_shift", "int in_relu"]
    assert p[18:21] == ["void *y", "int y_half", "int ldy"]
    assert len(nat.SIGNATURES["bev_conv2d_h16_affine"][1]) == len(p)
    g = _params("bev_groupnorm_fwd_ex_f32")
    assert g[:2] == ["const void *x", "int x_half"]
    assert g[2:] == _params("bev_groupnorm_fwd_f32")[1:]  # otherwise bev_groupnorm_fwd_f32's arguments
    assert len(nat.SIGNATURES["bev_groupnorm_fwd_ex_f32"][1]) == len(g)
    assert callable(nat.conv2d_h16_affine)


def test_affine_conv_argument_validation_without_gpu():
    """BEV_ERR_ARGS (-1) before any launch: null pointers, Ci % 64, an fp16 output of Co % 8 != 0 or ldy != Co, an
    affine on an fp32-stored operand, half an affine; N == 0 with good arguments is a no-op."""
    import bev_native as nat
    L = nat.lib()
    buf = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(buf) + 255) & ~255  # 256-B aligned host addresses: checked, never dereferenced
    x, w, y, sc, sh = (ctypes.c_void_p(base + 512 * i) for i in range(5))

    def call(x=x, x_half=1, N=1, Ci=128, scale=sc, shift=sh, w=w, Co=128, y=y, y_half=1, ldy=None, HW=8, Ho=8):
        return L.bev_conv2d_h16_affine(x, x_half, N, HW, HW, Ci, scale, shift, 1, w, None, Co, 3, 3, 1, 1, 1, 0, y,
                                       y_half, Co if ldy is None else ldy, Ho, Ho, None)

    assert call(x=None, w=None, y=None, scale=None, shift=None) == -1
    assert call(N=0) == 0                          # the arguments below differ from this accepted call in one thing
    assert call(N=0, scale=None, shift=None, x_half=0) == 0
    assert call(N=0, y_half=0, Co=5, ldy=8) == 0
    assert call(N=0, Ci=96) == -1                  # the K step is 64 channels
    assert call(N=0, Co=20) == -1                  # fp16 output: 16-B groups of 8 channels
    assert call(N=0, ldy=136) == -1                # fp16 output is dense
    assert call(N=0, x_half=0) == -1               # the affine needs the fp16-stored operand
    assert call(N=0, shift=None) == -1             # both or neither
    assert call(N=0, y_half=0, Co=5, ldy=4) == -1  # pitch below Co
    assert call(N=0, Ho=7) == -1                   # output size inconsistent with the geometry
    assert call(N=0, x=ctypes.c_void_p(base + 8)) == -1  # 16-B alignment
    assert call(N=-1) == -1


def test_groupnorm_ex_argument_validation_without_gpu():
    import bev_native as nat
    L = nat.lib()
    assert L.bev_groupnorm_fwd_ex_f32(None, 1, 1, 64, 128, 32, 1e-5, None, None, None, None, None, None, None,
                                      None) == -1
