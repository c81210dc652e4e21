"""Which compiled kernels do the GPU tests launch?

Two inputs, one output:

  compiled  every __global__ kernel of every HIP source of the library (csrc/*.hip as the Makefile's SRCS lists
            them), from the code-object metadata (.symbol of amdhsa.kernels) of a
            `hipcc --offload-arch=gfx950 -save-temps` compile with the Makefile's flags, demangled with the ROCm
            toolchain's llvm-cxxfilt (an install without one: llvm-cxxfilt / c++filt from PATH).  No GPU needed.
  launched  kernel names and launch counts from the CSV files of `rocprofv3 --kernel-trace` runs (one row per
            dispatch, column Kernel_Name), or from this tool's own aggregate of them (columns Kernel_Name, Launches).
            Names may be mangled or demangled, may end in ".kd" and may carry the anonymous-namespace prefix; names
            that are not the library's (torch's own kernels) are ignored.

  python tools/kernel_coverage.py aggregate -o counts.csv run1_kernel_trace.csv run2_kernel_trace.csv ...
  python tools/kernel_coverage.py report --commit "$(git rev-parse --short HEAD)" --traced tests/test_a.py,... \
         [--note NAME=REASON ...] -o listing.txt counts.csv [more.csv ...]

`aggregate` shrinks traces where they were taken (a trace has one row per dispatch); `report` compiles, matches and
writes one line per compiled kernel -- source, launch count, demangled name -- never-launched kernels first, then a
count per source.  A --note marks a never-launched kernel whose name contains NAME with the reason it stays untested.

Kernels in anonymous namespaces of different sources can share one signature; a launch of such a name is counted
for each source that compiles it and the line is marked "(name shared by N sources)".
"""
import argparse
import collections
import concurrent.futures
import csv
import os
import re
import shutil
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "vision-based-spatio-temporal-analysis_amd")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
HIPCC = os.path.join(ROCM, "bin", "hipcc")


def cxxfilt_path() -> str:
    for sub in (("llvm", "bin"), ("lib", "llvm", "bin")):
        p = os.path.join(ROCM, *sub, "llvm-cxxfilt")
        if os.path.exists(p):
            return p
    for tool in ("llvm-cxxfilt", "c++filt"):  # a ROCm install without it: the same Itanium demangling from PATH
        p = shutil.which(tool)
        if p:
            return p
    raise FileNotFoundError("no llvm-cxxfilt under " + ROCM + " and no llvm-cxxfilt / c++filt on PATH")


def demangle(names):
    """Mangled names -> demangled, in order (one llvm-cxxfilt process)."""
    names = list(names)
    if not names:
        return []
    out = subprocess.run([cxxfilt_path()], input="\n".join(names) + "\n", capture_output=True, text=True, check=True)
    res = out.stdout.split("\n")[:len(names)]
    assert len(res) == len(names)
    # a demangler older than the _Float16 mangling (DF16_) hands such names back untouched: spell the type as the
    # IEEE half it knows (Dh; neither is a substitution candidate, so the rest of the name is unchanged) and rename it
    retry = [i for i, (n, r) in enumerate(zip(names, res)) if r == n and n.startswith("_Z") and "DF16_" in n]
    if retry:
        again = subprocess.run([cxxfilt_path()], input="\n".join(names[i].replace("DF16_", "Dh") for i in retry) + "\n",
                               capture_output=True, text=True, check=True).stdout.split("\n")
        for i, r in zip(retry, again):
            if not r.startswith("_Z"):
                res[i] = re.sub(r"\bhalf\b", "_Float16", r)
    return res


_ANON = re.compile(r"\(anonymous namespace\)::")
_WS = re.compile(r"\s+")


def normalize(name: str, demangler=demangle) -> str:
    """The form names are matched in: demangled, no ".kd", no anonymous-namespace prefix, no return type, single
    spaces.  `_ZN12_GLOBAL__N_16k_convILi2E...EEvNS_8ConvArgsE.kd` and
    `void (anonymous namespace)::k_conv<2, ...>((anonymous namespace)::ConvArgs)` give the same string."""
    name = name.strip().strip("'\"")
    if name.endswith(".kd"):
        name = name[:-3]
    if name.startswith("_Z"):
        name = demangler([name])[0]
    name = _ANON.sub("", name)
    name = _WS.sub(" ", name).strip()
    # the return type of a template instance ("void k<...>(...)"): everything before the function name
    depth, cut = 0, 0
    for i, ch in enumerate(name):
        if ch in "<(":
            if depth == 0 and ch == "(":
                break
            depth += 1
        elif ch in ">)":
            depth -= 1
        elif ch == " " and depth == 0:
            cut = i + 1
    return name[cut:]


def short(norm: str) -> str:
    """A normalised name without its parameter list (what a trace with truncated kernel names holds)."""
    depth = 0
    for i, ch in enumerate(norm):
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            return norm[:i]
    return norm


def read_launches(lines, demangler=demangle) -> collections.Counter:
    """CSV lines (an iterable of str, header first) -> Counter of normalised name -> launches.  A `Launches` (or the
    stats file's `Calls`) column is a count; without one every row is one dispatch."""
    rd = csv.DictReader(lines)
    key = "Kernel_Name" if "Kernel_Name" in (rd.fieldnames or []) else "Name"
    if key not in (rd.fieldnames or []):
        raise ValueError(f"no Kernel_Name column in {rd.fieldnames}")
    cnt = "Launches" if "Launches" in rd.fieldnames else "Calls" if "Calls" in rd.fieldnames else None
    raw = collections.Counter()
    for row in rd:
        raw[row[key]] += int(row[cnt]) if cnt else 1
    names = list(raw)
    mangled = [n.strip().strip("'\"") for n in names]
    mangled = [n[:-3] if n.endswith(".kd") else n for n in mangled]
    idx = [i for i, n in enumerate(mangled) if n.startswith("_Z")]
    dem = dict(zip((mangled[i] for i in idx), demangler([mangled[i] for i in idx])))
    out = collections.Counter()
    for n, m in zip(names, mangled):
        out[normalize(dem.get(m, m), demangler)] += raw[n]
    return out


def match(compiled, launched):
    """compiled: list of (source, normalised name); launched: Counter of normalised names ->
    list of (source, name, launches, sources sharing the name).  Launched names that no source compiles are dropped;
    a launched name whose parameter list is absent or spelled differently matches by name and template arguments
    when exactly one compiled kernel has them."""
    full = {n for _, n in compiled}
    shorts = collections.defaultdict(set)
    for n in full:
        shorts[short(n)].add(n)
    count = collections.Counter()
    for n, c in launched.items():
        if n in full:
            count[n] += c
        elif len(shorts.get(short(n), ())) == 1:
            # no parameter list (truncated names), or one that another demangler spells differently (rocprofv3
            # writes __bf16 as "bool _Accum"): the name and template arguments of exactly one compiled kernel
            count[next(iter(shorts[short(n)]))] += c
    share = collections.Counter(n for _, n in compiled)
    return [(src, n, count[n], share[n]) for src, n in compiled]


def unmatched(compiled, launched):
    """Launched names that look like the library's (a compiled kernel's function name) but matched no compiled
    kernel -- a spelling the matching does not bridge; the listing would under-count."""
    ident = re.compile(r"[A-Za-z_]\w*")
    base = {ident.match(short(n)).group(0) for _, n in compiled if ident.match(short(n))}
    full = {n for _, n in compiled}
    shorts = collections.Counter(short(n) for n in full)
    return sorted(n for n in launched
                  if n not in full and shorts.get(short(n), 0) != 1 and ident.match(short(n))
                  and ident.match(short(n)).group(0) in base)


def sources():
    """The library's HIP sources: the Makefile's SRCS."""
    with open(os.path.join(PKG, "Makefile")) as f:
        for line in f:
            if line.startswith("SRCS"):
                return [os.path.join(PKG, s) for s in line.split("=", 1)[1].split()]
    raise RuntimeError("no SRCS line in the Makefile")


def compiled_symbols(src: str):
    """Mangled kernel symbols of one source (its code-object metadata), in file order."""
    with tempfile.TemporaryDirectory() as d:
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-c",
                        "-save-temps", "-o", "k.o", src], cwd=d, check=True, capture_output=True)
        asm = [f for f in os.listdir(d) if "gfx950" in f and f.endswith(".s")]
        if len(asm) != 1:
            raise RuntimeError(f"{src}: expected one gfx950 assembly file, got {asm}")
        syms = []
        with open(os.path.join(d, asm[0])) as f:
            for line in f:
                m = re.match(r"\s+\.symbol:\s+'?([^'\s]+)\.kd'?\s*$", line)
                if m:
                    syms.append(m.group(1))
    return syms


def compiled_kernels(jobs: int = 8):
    srcs = sources()
    with concurrent.futures.ThreadPoolExecutor(max_workers=jobs) as ex:
        syms = list(ex.map(compiled_symbols, srcs))
    out = []
    for s, names in zip(srcs, syms):
        out += kernels_from_symbols(os.path.basename(s), names)
    return out


def kernels_from_symbols(source: str, symbols):
    """Metadata symbols of one source -> [(source, normalised name)]."""
    return [(source, normalize(n)) for n in demangle(s[:-3] if s.endswith(".kd") else s for s in symbols)]


def write_report(rows, out, commit, traced, notes):
    rows = sorted(rows, key=lambda r: (r[2] != 0, r[0], r[1]))
    print(f"# kernel coverage of the GPU tests: commit {commit}", file=out)
    print("# launches: rocprofv3 --kernel-trace, one run per test file; compiled: hipcc --offload-arch=gfx950 "
          "-save-temps metadata", file=out)
    print("# traced test files: " + (", ".join(traced) if traced else "(none given)"), file=out)
    print("# source\tlaunches\tkernel", file=out)
    for src, n, c, sh in rows:
        tail = f"\t(name shared by {sh} sources)" if sh > 1 else ""
        if c == 0:
            for key, why in notes:
                if key in n:
                    tail += f"\t[untested: {why}]"
                    break
        print(f"{src}\t{c}\t{n}{tail}", file=out)
    print("#\n# per source: kernels, never launched, never launched without a stated reason", file=out)
    per = collections.OrderedDict()
    for src, n, c, _ in sorted(rows, key=lambda r: r[0]):
        t = per.setdefault(src, [0, 0, 0])
        t[0] += 1
        if c == 0:
            t[1] += 1
            t[2] += not any(key in n for key, _ in notes)
    for src, (k, z, u) in per.items():
        print(f"# {src}\t{k}\t{z}\t{u}", file=out)
    print(f"# total\t{sum(t[0] for t in per.values())}\t{sum(t[1] for t in per.values())}\t"
          f"{sum(t[2] for t in per.values())}", file=out)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    a = sub.add_parser("aggregate", help="kernel-trace CSVs -> one small Kernel_Name,Launches CSV (names untouched)")
    a.add_argument("-o", "--out", required=True)
    a.add_argument("csv", nargs="+")
    r = sub.add_parser("report", help="compile, match, write the listing")
    r.add_argument("-o", "--out", default="-")
    r.add_argument("--commit", default="(unknown)")
    r.add_argument("--traced", default="", help="comma-separated test files the traces come from (for the header)")
    r.add_argument("--note", action="append", default=[], metavar="NAME=REASON")
    r.add_argument("--jobs", type=int, default=8)
    r.add_argument("csv", nargs="*")
    args = ap.parse_args(argv)
    if args.cmd == "aggregate":
        raw = collections.Counter()
        for p in args.csv:
            with open(p, newline="") as f:
                rd = csv.DictReader(f)
                cnt = "Launches" if "Launches" in (rd.fieldnames or []) else None
                for row in rd:
                    raw[row["Kernel_Name"]] += int(row[cnt]) if cnt else 1
        with open(args.out, "w", newline="") as f:
            w = csv.writer(f, quoting=csv.QUOTE_ALL)
            w.writerow(["Kernel_Name", "Launches"])
            for n in sorted(raw):
                w.writerow([n, raw[n]])
        return 0
    launched = collections.Counter()
    for p in args.csv:
        with open(p, newline="") as f:
            launched.update(read_launches(f))
    notes = [tuple(n.split("=", 1)) for n in args.note]
    compiled = compiled_kernels(args.jobs)
    rows = match(compiled, launched)
    for n in unmatched(compiled, launched):
        print(f"warning: launched {n!r} matches no compiled kernel by name", file=sys.stderr)
    out = sys.stdout if args.out == "-" else open(args.out, "w")
    write_report(rows, out, args.commit, [t for t in args.traced.split(",") if t], notes)
    if out is not sys.stdout:
        out.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
