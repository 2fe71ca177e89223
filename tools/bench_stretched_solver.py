#!/usr/bin/env python3
"""Times solve_for_pressure! with HIP events on an N³ box stretched in x (Bounded, Periodic, Periodic), in y (Periodic, Bounded, Periodic)
and in z (Periodic, Periodic, Bounded: the same problem with its axes permuted), and the batched Thomas sweeps along x and along z on
the same N³ complex array (the x sweep against the z sweep, which does the same work with naturally coalesced lanes).
Usage: bench_stretched_solver.py [N] [repeats]"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import oceananigans_jl_amd as ocn  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
P, B = "Periodic", "Bounded"
faces = np.cumsum(np.r_[0.0, 1 + 0.5 * np.cos(np.linspace(0, 3 * np.pi, n))])


def timed(fn):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


out = {"N": n}
for name, d in (("stretched_x", 0), ("stretched_y", 1), ("stretched_z", 2)):
    topo, ext = [P, P, P], [(0, float(n)), (0, float(n)), (0, float(n))]
    topo[d], ext[d] = B, faces
    g = ocn.RectilinearGrid(ocn.GPU(), size=(n, n, n), topology=tuple(topo), x=ext[0], y=ext[1], z=ext[2])
    U = [ocn.Field(loc, g) for loc in (1, 2, 4)]
    for f in U:
        f.data.copy_(torch.rand(f.data.shape, device="cuda", dtype=torch.float64))
    p = ocn.CenterField(g)
    s = ocn.nonhydrostatic_pressure_solver(g)
    out[name + "_ms"] = round(timed(lambda: ocn.solve_for_pressure(p, s, 1.0, U)), 4)
    out[name + "_kind"] = s.info()["kind"]
    del s, p, U, g
    torch.cuda.empty_cache()

# the two sweeps alone on one N³ complex array
a = torch.rand(n - 1, device="cuda", dtype=torch.float64)
b = 3 + torch.rand(n ** 3, device="cuda", dtype=torch.float64)
f = torch.rand(2 * n ** 3, device="cuda", dtype=torch.float64)
t = torch.zeros(n ** 3, device="cuda", dtype=torch.float64)
phi = torch.zeros(2 * n ** 3, device="cuda", dtype=torch.float64)
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
for name in ("x", "y", "z"):
    out[f"sweep_{name}_ms"] = round(timed(lambda: ocn._lib.call(f"ocn_batched_tridiagonal_solve_{name}", n, n, n, a.data_ptr(), b.data_ptr(),
                                                               a.data_ptr(), f.data_ptr(), t.data_ptr(), phi.data_ptr(), stream)), 4)
out["sweep_x_over_z"] = round(out["sweep_x_ms"] / out["sweep_z_ms"], 3)
print(json.dumps(out))
