"""tools/kernel_coverage.py: matching launched kernel names (rocprofv3 --kernel-trace CSV rows) to compiled ones
(code-object metadata symbols).  No GPU, no profiler: the inputs are written out here."""
import io
import os
import sys

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tools"))
import kernel_coverage as kc  # noqa: E402

# metadata symbols (.symbol of amdhsa.kernels, mangled, with their .kd)
CONV_SYMBOLS = [
    "_ZN12_GLOBAL__N_16k_convILi2ELi2ELi2ELi2ELi1ELi2ELi0EEEvNS_8ConvArgsE.kd",  # templated, anonymous namespace
    "_ZN12_GLOBAL__N_16k_convILi4ELi1ELi1ELi2ELi1ELi1ELi0EEEvNS_8ConvArgsE.kd",  # compiled, never launched
    "_ZN12_GLOBAL__N_16k_stemENS_8StemArgsE.kd",
]
X6_SYMBOLS = ["_ZN12_GLOBAL__N_19k_pack_x6EPKfiiiillPDF16b.kd"]

TRACE = '''"Kind","Agent_Id","Queue_Id","Kernel_Id","Kernel_Name","Correlation_Id","Start_Timestamp","End_Timestamp"
"KERNEL_DISPATCH","Agent 4",1,11,"void (anonymous namespace)::k_conv<2, 2, 2, 2, 1, 2, 0>((anonymous namespace)::ConvArgs)",1,100,200
"KERNEL_DISPATCH","Agent 4",1,11,"_ZN12_GLOBAL__N_16k_convILi2ELi2ELi2ELi2ELi1ELi2ELi0EEEvNS_8ConvArgsE.kd",2,300,400
"KERNEL_DISPATCH","Agent 4",1,12,"(anonymous namespace)::k_stem((anonymous namespace)::StemArgs)",3,500,600
"KERNEL_DISPATCH","Agent 4",1,12,"_ZN12_GLOBAL__N_16k_stemENS_8StemArgsE.kd",4,500,600
"KERNEL_DISPATCH","Agent 4",1,13,"void at::native::vectorized_elementwise_kernel<4, at::native::FillFunctor<float>, std::array<char*, 1ul> >(int, at::native::FillFunctor<float>, std::array<char*, 1ul>)",5,700,800
"KERNEL_DISPATCH","Agent 4",1,14,"(anonymous namespace)::k_pack_x6(float const*, int, int, int, int, long, long, a_bf16_spelling*)",6,900,950
"KERNEL_DISPATCH","Agent 4",1,15,"k_conv.kd",7,960,970
'''


def test_kernel_coverage_name_matching():
    compiled = (kc.kernels_from_symbols("bev_conv.hip", CONV_SYMBOLS)
                + kc.kernels_from_symbols("bev_conv_x6.hip", X6_SYMBOLS))
    assert [n for _, n in compiled[:3]] == [
        "k_conv<2, 2, 2, 2, 1, 2, 0>(ConvArgs)", "k_conv<4, 1, 1, 2, 1, 1, 0>(ConvArgs)", "k_stem(StemArgs)"]
    pack = compiled[3][1]  # its last parameter is __bf16*, which demanglers spell differently
    assert pack.startswith("k_pack_x6(float const*, int, int, int, int, long, long, ")
    launched = kc.read_launches(io.StringIO(TRACE))
    rows = {n: (src, c, sh) for src, n, c, sh in kc.match(compiled, launched)}
    # demangled and mangled + ".kd" rows of one templated kernel in the anonymous namespace add up
    assert rows["k_conv<2, 2, 2, 2, 1, 2, 0>(ConvArgs)"] == ("bev_conv.hip", 2, 1)
    # a compiled kernel nothing launched stays in the listing with zero; the bare "k_conv" row names two
    # instances, so it is counted for neither
    assert rows["k_conv<4, 1, 1, 2, 1, 1, 0>(ConvArgs)"] == ("bev_conv.hip", 0, 1)
    # a ".kd" suffix on a mangled name
    assert rows["k_stem(StemArgs)"] == ("bev_conv.hip", 2, 1)
    # another demangler's spelling of a parameter type: matched by name when only one compiled kernel has it
    assert rows[pack] == ("bev_conv_x6.hip", 1, 1)
    # torch's kernel is nobody's: ignored
    assert len(rows) == 4 and not any("at::native" in n for n in rows)
    # the aggregate form (Kernel_Name, Launches) reads back to the same counts
    agg = io.StringIO('"Kernel_Name","Launches"\n"_ZN12_GLOBAL__N_16k_stemENS_8StemArgsE.kd","7"\n')
    assert kc.read_launches(agg) == {"k_stem(StemArgs)": 7}
    # the listing: never-launched kernels first, a count per source at the end
    out = io.StringIO()
    kc.write_report(kc.match(compiled, launched), out, "abc1234", ["tests/test_x.py"],
                    [("k_conv<4,", "example reason")])
    lines = out.getvalue().splitlines()
    body = [ln for ln in lines if not ln.startswith("#")]
    assert body[0].startswith("bev_conv.hip\t0\tk_conv<4, 1, 1, 2, 1, 1, 0>(ConvArgs)") and "example reason" in body[0]
    assert "abc1234" in lines[0] and any("tests/test_x.py" in ln for ln in lines[:4])
    assert "# bev_conv.hip\t3\t1\t0" in lines and "# bev_conv_x6.hip\t1\t0\t0" in lines
