#!/usr/bin/env python3
"""Is the device code of two source trees the same?  No GPU needed.

    tools/compare_device_code.py CSRC_A CSRC_B [--jobs N] [--check-reproducible] [--keep DIR]

CSRC_A / CSRC_B: two directories with the library's Makefile and sources (oceananigans.jl_amd/csrc of two checkouts).  For every object of
a Makefile (`make -n -B`) the gfx950 code object is built with that object's own flags (--cuda-device-only), taken out of its offload
bundle where the compiler wrote one, and compared.  One line per object:

    identical                       the two code objects are the same bytes
    kernels -N: <names>             B lacks N kernels of A (or has +N more); every kernel both have disassembles to the same text
    kernels renamed N: <names>      N kernels have another symbol (the types of their arguments were renamed, or their template argument
                                    list grew at its end); all disassemble to the same text.  With -N / +N for the kernels left unpaired
    DIFFERENT: ...                  anything else

Whole code objects and the disassembly text of whole kernels are compared; nothing looks for particular instructions.
--check-reproducible builds A a second time first and requires the same bytes (otherwise a difference would mean nothing).
The exit status is 0 unless an object is DIFFERENT (or A is not reproducible)."""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def compile_commands(src):
    """{object name: its compile command} from the Makefile in src"""
    out = subprocess.run(["make", "-n", "-B", "-C", src], check=True, capture_output=True, text=True).stdout
    cmds = {}
    for line in out.splitlines():
        m = re.search(r" -c (\S+) -o build/(\S+)\.o$", line.strip())
        if m:
            cmds[m.group(2)] = line.strip()
    return cmds


def build_one(src, cmd, name, outdir):
    """the gfx950 code object of one Makefile object"""
    raw, co = os.path.join(outdir, name + ".device"), os.path.join(outdir, name + ".co")
    # (-cuid: the compilation-unit id, otherwise a hash of the source's path and of this command line, names one symbol of the code object)
    cmd = re.sub(r" -c (\S+) -o build/\S+\.o$", r" --cuda-device-only -cuid=" + name + r" -c \1 -o " + raw, cmd)
    subprocess.run(cmd, shell=True, check=True, cwd=src, capture_output=True)
    with open(raw, "rb") as f:
        bundled = f.read(len(BUNDLE_MAGIC)) == BUNDLE_MAGIC
    if bundled:
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=" + TARGET, "--input=" + raw, "--output=" + co,
                        "--unbundle"], check=True, capture_output=True)
        os.remove(raw)
    else:
        os.rename(raw, co)
    return co


def build_all(src, outdir, jobs):
    os.makedirs(outdir, exist_ok=True)
    cmds = compile_commands(src)
    with ThreadPoolExecutor(jobs) as pool:
        futures = {name: pool.submit(build_one, src, cmd, name, outdir) for name, cmd in cmds.items()}
        return {name: f.result() for name, f in futures.items()}


def kernels(co):
    """{kernel symbol: its disassembly text without addresses}"""
    syms = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-s", "--wide", co], check=True, capture_output=True, text=True).stdout
    names = set()
    for line in syms.splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] == "FUNC" and f[4] in ("GLOBAL", "WEAK") and f[6] != "UND":
            names.add(f[7])
    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", co], check=True, capture_output=True, text=True).stdout
    text, current = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-fA-F]+ <(\S+)>:$", line)
        if m:
            current = m.group(1)
            text[current] = []
        elif current is not None and line.strip() not in ("", "..."):  # (not the padding between two kernels)
            text[current].append(re.sub(r"// [0-9A-Fa-f]+:", "//", line))  # (where the kernel lies in the object is not part of it)
    return {n: "\n".join(text.get(n, [])) for n in names}


def demangle(names):
    tool = shutil.which("llvm-cxxfilt", path=LLVM) or shutil.which("c++filt")
    if not names or not tool:
        return list(names)
    out = subprocess.run([tool] + list(names), check=True, capture_output=True, text=True).stdout
    return [without_parameters(n) for n in out.splitlines()]


def without_parameters(name):
    """a demangled function name without its parameter list: the text before the parenthesis that the last one closes"""
    if not name.endswith(")"):
        return name
    depth = 0
    for at in range(len(name) - 1, -1, -1):
        depth += {")": 1, "(": -1}.get(name[at], 0)
        if depth == 0:
            return name[:at]
    return name


def same_kernel(da, db):
    """demangled names without parameters: equal, or b is a with further trailing template arguments"""
    return da == db or (da.endswith(">") and db.endswith(">") and db.startswith(da[:-1] + ", "))


def compare(a, b):
    with open(a, "rb") as fa, open(b, "rb") as fb:
        if fa.read() == fb.read():
            return True, "identical"
    ka, kb = kernels(a), kernels(b)
    changed = sorted(n for n in ka.keys() & kb.keys() if ka[n] != kb[n])
    if changed:
        return False, f"DIFFERENT: the disassembly of {len(changed)} kernels differs: " + ", ".join(demangle(changed)[:4])
    gone, new = sorted(ka.keys() - kb.keys()), sorted(kb.keys() - ka.keys())
    # a kernel whose argument types were renamed (a struct moved to another namespace) or whose template argument list grew at its end has
    # another symbol: pair such kernels by their demangled name without the parameter list (the equal name before the longer one) and
    # compare their text with the kernel's own symbol taken out
    named_gone, named_new = list(zip(gone, demangle(gone))), list(zip(new, demangle(new)))
    renamed = {}
    for exact in (True, False):
        for n, dn in named_gone:
            free = [m for m, dm in named_new if m not in renamed.values() and (dn == dm if exact else same_kernel(dn, dm))]
            if free and n not in renamed:
                renamed[n] = free[0]
    if renamed:
        changed = sorted(n for n, m in renamed.items() if ka[n].replace(n, "") != kb[m].replace(m, ""))
        if changed:
            return False, f"DIFFERENT: {len(renamed)} kernels renamed, the disassembly of {len(changed)} differs: " + ", ".join(demangle(changed)[:4])
        line = f"kernels renamed {len(renamed)}: " + ", ".join(demangle(sorted(renamed)))
        gone, new = [n for n in gone if n not in renamed], [m for m in new if m not in renamed.values()]
        for sign, rest in (("-", gone), ("+", new)):
            if rest:
                line += f"; kernels {sign}{len(rest)}: " + ", ".join(demangle(rest))
        return True, line + f"; all {len(ka) - len(gone)} kernels both have disassemble to the same text"
    if not gone and not new:
        return False, "DIFFERENT: same kernels with the same disassembly, other bytes (data, metadata)"
    parts = ([f"kernels -{len(gone)}: " + ", ".join(demangle(gone))] if gone else []) + ([f"kernels +{len(new)}: " + ", ".join(demangle(new))] if new else [])
    return True, "; ".join(parts) + f"; the {len(ka.keys() & kb.keys())} kernels both have disassemble to the same text"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("csrc_a")
    ap.add_argument("csrc_b")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--check-reproducible", action="store_true")
    ap.add_argument("--keep", help="keep the code objects in this directory")
    args = ap.parse_args()
    work = args.keep or tempfile.mkdtemp(prefix="ocn_device_code_")
    a = build_all(os.path.abspath(args.csrc_a), os.path.join(work, "a"), args.jobs)
    ok = True
    if args.check_reproducible:
        a2 = build_all(os.path.abspath(args.csrc_a), os.path.join(work, "a2"), args.jobs)
        same = all(open(a[n], "rb").read() == open(a2[n], "rb").read() for n in a)
        print("A built twice:", "the same bytes for every object" if same else "NOT REPRODUCIBLE")
        ok = ok and same
    b = build_all(os.path.abspath(args.csrc_b), os.path.join(work, "b"), args.jobs)
    for name in sorted(a.keys() | b.keys()):
        if name not in a or name not in b:
            print(f"{name}: DIFFERENT: only in {'A' if name in a else 'B'}")
            ok = False
            continue
        good, line = compare(a[name], b[name])
        print(f"{name}: {line}")
        ok = ok and good
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
