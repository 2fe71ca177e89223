"""Instruction classes of the plane loop of one kernel in a gfx950 assembly listing (hipcc -S --cuda-device-only), per thread and plane,
plus the kernel's register resources.  The plane loop is the largest backward branch whose body holds an s_barrier.
Usage: python tools/isa_loop.py file.s REGEX [...]      (REGEX is matched against the mangled kernel names)
Example: hipcc --offload-arch=gfx950 -O3 -std=c++17 -DOCN_STRICT=0 -ffp-contract=fast -S --cuda-device-only \\
             oceananigans.jl_amd/csrc/tendencies.hip -o t.s && python tools/isa_loop.py t.s 'momentum_tendencies_pc32'"""
import re
import sys
from collections import Counter

F64 = ("v_mul_f64", "v_fmac_f64", "v_add_f64", "v_fma_f64", "v_rcp_f64")
MOVE = ("v_mov_b", "v_cndmask", "v_readlane", "v_writelane", "v_readfirstlane", "v_accvgpr")


def kernels(txt):
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end", txt, re.S | re.M):
        yield m.group(1), m.group(2)


def metadata(txt, name):
    m = re.search(r"\.name:\s+" + re.escape(name) + r"\n", txt)
    if not m:
        return {}
    s = txt.rfind("\n  - ", 0, m.start())
    e = txt.find("\n  - ", m.end())
    body = txt[s:e if e > 0 else len(txt)]
    out = {}
    for k in ("sgpr_count", "sgpr_spill_count", "vgpr_count", "vgpr_spill_count", "private_segment_fixed_size"):
        mm = re.search(r"\." + k + r":\s+(\d+)", body)
        if mm:
            out[k] = int(mm.group(1))
    return out


def plane_loop(body):
    lines = [l.strip() for l in body.splitlines()]
    labels = {}
    for n, l in enumerate(lines):
        if re.match(r"^\.LBB\w+:", l):
            labels[l.split(":")[0]] = n
    best = None
    for n, l in enumerate(lines):
        m = re.match(r"^s_(?:cbranch_\w+|branch)\s+(\.LBB\w+)", l)
        if m and m.group(1) in labels and labels[m.group(1)] < n:
            a = labels[m.group(1)]
            seg = lines[a:n + 1]
            if any(x.startswith("s_barrier") for x in seg) and (best is None or n - a > best[1] - best[0]):
                best = (a, n)
    if best is None:
        return []
    return [l.split()[0] for l in lines[best[0]:best[1] + 1] if l and not l.startswith((";", ".")) and not l.endswith(":")]


def classes(ins):
    c = Counter()
    for i in ins:
        if i.startswith("v_"):
            c["valu"] += 1
            if any(i.startswith(p) for p in F64) or ("f64" in i and i.startswith("v_cmp")):
                c["valu_f64"] += 1
            elif any(i.startswith(p) for p in MOVE):
                c["valu_move_select"] += 1
            else:
                c["valu_int_addr"] += 1
            if i.startswith("v_lshl_add_u64"):
                c["v_lshl_add_u64"] += 1
            if i.startswith(("v_readlane", "v_writelane")):
                c["v_readlane/writelane"] += 1
        elif i.startswith("ds_"):
            c["lds"] += 1
        elif i.startswith(("global_load", "buffer_load", "flat_load")):
            c["vmem_load"] += 1
        elif i.startswith(("global_store", "buffer_store", "flat_store")):
            c["vmem_store"] += 1
        elif i.startswith("s_waitcnt"):
            c["s_waitcnt"] += 1
        elif i.startswith("scratch_"):
            c["scratch"] += 1
        elif i.startswith("s_"):
            c["salu_other"] += 1
    return c


def main():
    txt = open(sys.argv[1]).read()
    pats = sys.argv[2:] or ["tiled|pc32"]
    for name, body in kernels(txt):
        if not any(re.search(p, name) for p in pats):
            continue
        c = classes(plane_loop(body))
        md = metadata(txt, name)
        print(name)
        print("  resources: " + ", ".join("%s %d" % kv for kv in md.items()))
        print("  plane loop: " + ", ".join("%s %d" % (k, c[k]) for k in ("valu", "valu_f64", "valu_int_addr", "valu_move_select",
                                                                           "v_lshl_add_u64", "v_readlane/writelane", "lds", "vmem_load",
                                                                           "vmem_store", "s_waitcnt", "salu_other", "scratch")))


if __name__ == "__main__":
    main()
