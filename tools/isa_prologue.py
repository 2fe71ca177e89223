"""How a kernel of a gfx950 assembly listing (hipcc -S --cuda-device-only) starts: what it asks memory for, and in which order, before
its first data arrive -- the static record of the transform kernels' prologues (profiles/r06a_fft_prologue.md).
Per kernel whose mangled name a REGEX matches:
  loads before the first wait    VMEM loads issued before the first `s_waitcnt vmcnt`
  vmcnt(0) before the data       `s_waitcnt vmcnt(0)` (a full drain: one memory round trip each) in front of the first data load
  first data load at VALU        number of VALU instructions from the kernel's entry to the first data load
  after the first barrier        VMEM loads / v_div_scale_f64 behind the first s_barrier (the fused z pass: between its two transforms)
  resources                      VGPRs, spills, scratch bytes, static LDS bytes from the listing's metadata
The DATA loads are told from the table loads by their shape: the longest run of VMEM loads with one addressing form (scalar base, or
64-bit vector address `off`) and no vmcnt wait between them -- the 8 or 16 `global_load_dwordx4 ..., off` of a thread's column or row
elements, the velocity loads of the source kernel's first group -- against one to five loads per table, mostly off a scalar base.  More
than GAP VALU instructions between two loads (the address arithmetic between the tables and the data) end a run as well.  (A table load
with a vector address right in front of the data is still counted into the run: rowfft_c2r_kernel's second twN load.)
Usage: python tools/isa_prologue.py file.s REGEX [...]
Example: hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only oceananigans.jl_amd/csrc/colfft.hip -o c.s && \\
             python tools/isa_prologue.py c.s 'colfft_kernelILi512ELi8ELi[012]E'"""
import re
import sys

from isa_loop import kernels

LOAD = ("global_load", "buffer_load", "flat_load")
GAP = 32


def instructions(body):
    for l in body.splitlines():
        l = l.strip()
        if l and not l.startswith((";", ".")) and not l.endswith(":"):
            yield l


def metadata(txt, name):
    m = re.search(r"\.name:\s+" + re.escape(name) + r"\n", txt)
    if not m:
        return {}
    s = txt.rfind("\n  - ", 0, m.start())
    e = txt.find("\n  - ", m.end())
    body = txt[s:e if e > 0 else len(txt)]
    out = {}
    for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"):
        mm = re.search(r"\." + k + r":\s+(\d+)", body)
        if mm:
            out[k] = int(mm.group(1))
    return out


def prologue(body):
    ins = list(instructions(body))
    valu = 0
    events = []  # (kind, index into ins, VALU instructions before it, detail)
    for n, l in enumerate(ins):
        op = l.split()[0]
        if op.startswith("v_"):
            valu += 1
        elif op.startswith(LOAD):
            form = "off" if re.search(r",\s*off\b", l) else "sbase"
            events.append(("load", n, valu, form))
        elif op == "s_waitcnt" and "vmcnt" in l:
            events.append(("wait", n, valu, int(re.search(r"vmcnt\((\d+)\)", l).group(1))))
        elif op == "s_barrier":
            events.append(("barrier", n, valu, None))
    # the data burst: the longest run of loads of one shape with no vmcnt wait between them
    best, run = [], []
    for e in events:
        if e[0] == "load" and run and run[-1][3] == e[3] and e[2] - run[-1][2] <= GAP:
            run.append(e)
        elif e[0] == "load":
            run = [e]
        elif e[0] == "wait":
            run = []
        if len(run) > len(best):
            best = list(run)
    first_data = best[0] if best else None
    first_wait = next((e for e in events if e[0] == "wait"), None)
    first_barrier = next((e for e in events if e[0] == "barrier"), None)
    out = {
        "loads_before_first_wait": sum(1 for e in events if e[0] == "load" and (first_wait is None or e[1] < first_wait[1])),
        "drains_before_data": sum(1 for e in events if e[0] == "wait" and e[3] == 0 and first_data and e[1] < first_data[1]),
        "first_data_valu": first_data[2] if first_data else None,
        "data_burst": "%d loads, %s" % (len(best), best[0][3]) if best else "-",
        "first_barrier_valu": first_barrier[2] if first_barrier else None,
    }
    if first_barrier:
        tail = ins[first_barrier[1]:]
        out["loads_after_barrier"] = sum(1 for l in tail if l.split()[0].startswith(LOAD))
        out["div_scale_after_barrier"] = sum(1 for l in tail if l.startswith("v_div_scale_f64"))
    return out


def main():
    txt = open(sys.argv[1]).read()
    pats = sys.argv[2:]
    if not pats:
        sys.exit(__doc__)
    for name, body in kernels(txt):
        if not any(re.search(p, name) for p in pats):
            continue
        p, md = prologue(body), metadata(txt, name)
        print(name)
        print("  loads before the first wait %d, vmcnt(0) before the data %d, first data load at VALU %s [%s], first barrier at VALU %s"
              % (p["loads_before_first_wait"], p["drains_before_data"], p["first_data_valu"], p["data_burst"], p["first_barrier_valu"]))
        print("  after the first barrier: VMEM loads %s, v_div_scale_f64 %s" % (p.get("loads_after_barrier"), p.get("div_scale_after_barrier")))
        print("  resources: VGPRs %s, VGPR spills %s, SGPR spills %s, scratch bytes %s, static LDS bytes %s"
              % tuple(md.get(k) for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
                                          "group_segment_fixed_size")))


if __name__ == "__main__":
    main()
