"""Instruction mix of a kernel's MFMA loops, from a gfx950 assembly listing.
usage: python tools/loop_listing.py <file.s> [name filter]
    hipcc --offload-arch=gfx950 <the Makefile's flags> --cuda-device-only -S -o file.s csrc/<source>.hip

For every kernel whose (demangled-ish) name matches the filter, every innermost loop (a label and the last backward
branch to it, no other loop inside) that holds MFMAs is printed as one line: MFMAs, vector-ALU instructions (v_*
without the MFMAs), the conversions and packed adds among them, 64-bit / multiply address arithmetic, vector-memory
loads, LDS operations, scalar loads, s_getpc, exec-masked regions, waits on lgkmcnt(0), barriers and branches."""
import re
import sys

ADDR = ("v_mad_u64_u32", "v_mad_i64_i32", "v_mul_lo_u32", "v_mul_hi_u32", "v_lshl_add_u64", "v_mul_u32_u24",
        "v_mad_u32_u24", "v_lshlrev_b64", "v_add_co_u32", "v_addc_co_u32", "v_ashrrev_i64")


def kernels(lines):
    name, body = None, []
    for ln in lines:
        m = re.match(r"^(_Z\w+|\w+):\s*(;.*)?$", ln)
        if m and not ln.startswith(".L"):
            if name:
                yield name, body
            name, body = m.group(1), []
        elif name is not None:
            body.append(ln)
            if ln.strip().startswith("s_endpgm"):
                yield name, body
                name, body = None, []


def loops(body):
    pos = {}
    for i, ln in enumerate(body):
        m = re.match(r"^(\.LBB\w+):", ln)
        if m:
            pos[m.group(1)] = i
    found = {}
    for i, ln in enumerate(body):
        m = re.match(r"\s+s_cbranch_\w+\s+(\.LBB\w+)|\s+s_branch\s+(\.LBB\w+)", ln)
        if m:
            tgt = m.group(1) or m.group(2)
            if tgt in pos and pos[tgt] < i:
                found[tgt] = max(found.get(tgt, 0), i)
    spans = sorted((pos[t], e) for t, e in found.items())
    inner = [(s, e) for s, e in spans if not any(s < s2 and e2 < e for s2, e2 in spans)]  # innermost only
    keep = []  # a rotated loop shows up as two overlapping spans: the first stands for both
    for s, e in inner:
        if not keep or s > keep[-1][1]:
            keep.append((s, e))
    return keep


def mix(block):
    ops = [ln.split()[0] for ln in block if ln.startswith("\t") and not ln.strip().startswith((";", "."))]
    text = [ln for ln in block if ln.startswith("\t")]
    c = lambda f: sum(1 for o in ops if f(o))
    return {
        "mfma": c(lambda o: o.startswith("v_mfma")),
        "valu": c(lambda o: o.startswith("v_") and not o.startswith("v_mfma")),
        "cvt_pk_bf16": c(lambda o: o == "v_cvt_pk_bf16_f32"),
        "pk_add_f32": c(lambda o: o == "v_pk_add_f32"),
        "sub_f32": c(lambda o: o.startswith("v_sub_f32")),
        "addr64_mul": c(lambda o: o.startswith(ADDR)),
        "cndmask": c(lambda o: o.startswith("v_cndmask")),
        "readfirstlane": c(lambda o: o.startswith("v_readfirstlane")),
        "global_load": c(lambda o: o.startswith("global_load")),
        "buffer_load": c(lambda o: o.startswith("buffer_load")),
        "nt": sum(1 for ln in text if re.search(r"_load\w*\s.*\bnt\b", ln)),
        "ds": c(lambda o: o.startswith("ds_")),
        "s_load": c(lambda o: o.startswith("s_load")),
        "s_getpc": c(lambda o: o.startswith("s_getpc")),
        "saveexec": c(lambda o: "saveexec" in o),
        "lgkmcnt0": sum(1 for ln in text if "s_waitcnt" in ln and "lgkmcnt(0)" in ln),
        "barrier": c(lambda o: o == "s_barrier"),
        "branch": c(lambda o: o.startswith(("s_cbranch", "s_branch"))),
    }


def main():
    lines = open(sys.argv[1]).read().split("\n")
    filt = re.compile(sys.argv[2] if len(sys.argv) > 2 else ".")
    for name, body in kernels(lines):
        if not filt.search(name):
            continue
        for s, e in loops(body):
            m = mix(body[s:e + 1])
            if m["mfma"] == 0:
                continue
            print(name)
            print("    lines %d-%d: " % (s, e) + " ".join("%s=%d" % kv for kv in m.items() if kv[1] or kv[0] in (
                "s_load", "s_getpc", "saveexec", "lgkmcnt0", "addr64_mul")))


if __name__ == "__main__":
    main()
