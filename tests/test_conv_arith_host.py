"""Host-side contract of the "f16" inference arithmetic: the mode is offered, the C header declares the fp16-output
conv, and the ABI number of the binding is the one the header states.  No GPU."""
import os
import re

from conftest import PKG, REPO

HEADER = os.path.join(REPO, "include", "bev_mi355x.h")


def test_f16_is_a_conv_arithmetic():
    import bev_native as nat
    assert "f16" in nat.CONV_ARITHS
    assert nat.CONV_ARITHS[:2] == ("f32", "bf16x6") and nat.conv_arith() == "bf16x6"  # the default stays


def test_header_declares_the_fp16_output_conv():
    import bev_native as nat
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+bev_conv2d_h16_h16\s*\(([^;]*)\)\s*;", txt)
    assert m, "bev_conv2d_h16_h16 is not declared"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 20 and params[1] == "int x_half" and params[-1] == "void *stream"
    assert "uint16_t *y" in params and "const uint16_t *residual" in params
    restype, argtypes = nat.SIGNATURES["bev_conv2d_h16_h16"]
    assert len(argtypes) == len(params)
    assert callable(nat.conv2d_h16_half)


def test_abi_version_matches_header_and_library_source():
    import bev_native as nat
    m = re.search(r"ABI version[^*]*?:\s*(\d+)\.\s*\*/\s*int bev_abi_version", open(HEADER).read())
    assert m, "the header comment above bev_abi_version states the number"
    assert int(m.group(1)) == nat.ABI_VERSION
    src = open(os.path.join(PKG, "csrc", "bev_warp.hip")).read()
    assert re.search(r"int bev_abi_version\(void\) \{ return (\d+); \}", src).group(1) == str(nat.ABI_VERSION)
