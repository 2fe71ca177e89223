#!/usr/bin/env python3
"""Bitwise record of solve_for_pressure!: per shape the SHA-256 of the interior pressure bytes and a few sampled values, for seeded
random velocities.  A change that only reorders the memory requests of the transform kernels (csrc/colfft.hip, rowfft.hip) must
reproduce every digest; a mismatch is an indexing bug, not a rounding question.

The shapes are the smallest that reach each path of the kernels (tests/test_gpu_poisson_bitwise.py lists what each one is for).  They
run one after the other in THIS process, each solver gone before the next is made: rocFFT's real plans (the x / y transforms of the
16 x 12 x N cases) are chosen at creation and can depend on which other plans are alive (tests/test_gpu_poisson_pipelines.py), so the
test recomputes in a fresh process of the same script, and the record holds each solver's info() next to its digest.

Usage: python tools/record_poisson_digests.py OUT.json [--commit ID]
       (OCN_LIB_PATH selects the library; tests/golden/poisson_digests.json was written by a library built from the commit it names)"""
import gc
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TOPOLOGY = {"P": "Periodic", "B": "Bounded"}
# (id, topology, size)
CASES = [
    ("PPP-128x64x64", "PPP", (128, 64, 64)),
    ("PPP-128x64x512", "PPP", (128, 64, 512)),
    ("PPP-16x12x64", "PPP", (16, 12, 64)),
    ("PPP-16x12x128", "PPP", (16, 12, 128)),
    ("PPP-16x12x256", "PPP", (16, 12, 256)),
    ("PPP-16x12x512", "PPP", (16, 12, 512)),
    ("PPB-128x64x64", "PPB", (128, 64, 64)),
    ("BBB-64x64x64", "BBB", (64, 64, 64)),
]
DT = 0.37
N_SAMPLES = 6


def solve_case(ocn, case, seed):
    """(info, interior pressure as a contiguous [k, j, i] array) of one case"""
    import numpy as np
    import torch
    _, topo, size = case
    grid = ocn.RectilinearGrid(ocn.GPU(), size=size, x=(0, 1), y=(0, 2.5), z=(0, 4), topology=tuple(TOPOLOGY[t] for t in topo),
                               halo=(3, 3, 3))
    rng = np.random.default_rng(seed)
    U = []
    for loc in (1, 2, 4):
        f = ocn.Field(loc, grid)
        f.data.copy_(torch.from_numpy(rng.uniform(-1, 1, tuple(f.data.shape))))  # (halos included: some pipelines read them)
        U.append(f)
    solver = ocn.nonhydrostatic_pressure_solver(grid)
    p = ocn.CenterField(grid)
    ocn.solve_for_pressure(p, solver, DT, U)
    ocn.sync_device()
    i = solver.info()
    return [i["kind"], int(i["r2c"]), i["direct_out"]], np.ascontiguousarray(p.interior_view().cpu().numpy())


def record(ocn):
    import numpy as np
    out = {}
    for n, case in enumerate(CASES):
        info, p = solve_case(ocn, case, 1234 + n)
        flat = p.reshape(-1)
        where = [int(w) for w in np.linspace(0, flat.size - 1, N_SAMPLES).astype(np.int64)]
        out[case[0]] = {"topology": case[1], "size": list(case[2]), "info": info, "sha256": hashlib.sha256(p.tobytes()).hexdigest(),
                        "samples": [[w, float(flat[w]).hex()] for w in where]}
        gc.collect()
    return out


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    commit = sys.argv[sys.argv.index("--commit") + 1] if "--commit" in sys.argv else None
    import oceananigans_jl_amd
    doc = {"commit": commit, "dt": DT, "cases": record(oceananigans_jl_amd)}
    with open(sys.argv[1], "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
