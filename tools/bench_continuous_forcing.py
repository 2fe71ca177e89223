#!/usr/bin/env python3
"""Time of the forcing programs (oceananigans.jl_amd/forcing_programs.py) on (Periodic, Periodic, Bounded) grids of 256^3 and 512 x 512 x 256.

1. ms per ocn_op_accumulate of  -mu u  on u,  the plankton term (mu0 exp(z / lam) - m) P  on a tracer  and a term with three
   interpolated dependencies (u, v, w at a tracer's location), each next to its yardstick taken in the same run: ocn_op_compute of the
   SAME program into a scratch field, which is existing code.  The accumulate launch moves 8 B per cell more (it reads G), so it should
   take at most  compute time x (bytes of accumulate / bytes of compute) x 1.10; the achieved bytes/s of both are printed.
   Bytes = the distinct field parents the program reads + the cells written (+ the cells of G read).
2. ms per time_step of a model whose u is forced by a function of x and t: as Forcing(func) (sampled by NumPy and uploaded at every
   tendency evaluation: a whole field per stage) and as ContinuousForcing(func) (traced: a patched constant and an Nx-long vector).

  tools/bench_continuous_forcing.py [reps] [steps] [--small]
Device work is timed with a host clock around a window that ends in a synchronise, after a warm-up; ten launches per window for the
kernels (one is tens of microseconds at the small size).  Median [min, max] of `reps` windows; `steps` time steps per model."""
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import oceananigans_jl_amd as ocn
from oceananigans_jl_amd.forcings import validate_forcing

args = [a for a in sys.argv[1:] if not a.startswith("--")]
reps = int(args[0]) if len(args) > 0 else 20
steps = int(args[1]) if len(args) > 1 else 5
sizes = [(64, 64, 32)] if "--small" in sys.argv else [(256, 256, 256), (512, 512, 256)]
INNER = 10
PLANKTON = dict(mu0=1 / 86400, lam=5.0, m=0.1 / 86400)


def timed(fn, n):
    out = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return statistics.median(out), min(out), max(out)


def forcing_function(x, y, z, t):
    return 1e-3 * np.sin(2.0 * t) * np.cos(6.0 * x)


def kernels(N):
    grid = ocn.RectilinearGrid(ocn.GPU(), size=N, x=(0, 1), y=(0, 1), z=(-64, 0), topology=("Periodic", "Periodic", "Bounded"))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    f = dict(u=ocn.XFaceField(grid), v=ocn.YFaceField(grid), w=ocn.ZFaceField(grid), P=ocn.CenterField(grid))
    for x in f.values():
        x.data.copy_(torch.rand(x.data.shape, generator=gen, device="cuda", dtype=torch.float64) * 2 - 1)
    ocn.fill_halo_regions(tuple(f.values()), fill_boundary_normal_velocities=False)
    cases = [
        ("-mu u  on u", "u", ocn.ContinuousForcing(lambda x, y, z, t, u, mu: -mu * u, field_dependencies="u", parameters=0.375)),
        ("plankton  on P", "P", ocn.ContinuousForcing(lambda x, y, z, t, P, p: (p["mu0"] * ocn.exp(z / p["lam"]) - p["m"]) * P,
                                                      field_dependencies="P", parameters=PLANKTON)),
        ("u v + w P, three interpolated", "P", ocn.ContinuousForcing(lambda x, y, z, t, u, v, w, P: u * v + w * P,
                                                                     field_dependencies=("u", "v", "w", "P"))),
    ]
    for name, forced, term in cases:
        pf = ocn.ProgramForcing(validate_forcing({forced: term}, grid, tuple(f))[forced], grid, forced, f)
        G, scratch = ocn.Field(f[forced].loc, grid), ocn.Field(f[forced].loc, grid)
        c = pf._c
        cells = int(np.prod(pf.program.interior_size()))
        read = sum(x.data.numel() * 8 for x in pf.program.fields if isinstance(x, ocn.Field))
        bytes_compute, bytes_accumulate = read + 8 * cells, read + 16 * cells

        def accumulate():
            for _ in range(INNER):
                pf.accumulate(G, 0.0)

        def compute():  # (on these grids the tendency cells of u and of a tracer ARE the interior ocn_op_compute runs over)
            for _ in range(INNER):
                ocn._lib.call("ocn_op_compute", grid.cref, C.byref(c), scratch.ptr, ocn.architectures.stream_ptr())
        for _ in range(3):
            accumulate()
            compute()
        ta, tc = [], []
        for _ in range(2):  # alternating
            ta.append(timed(accumulate, reps))
            tc.append(timed(compute, reps))
        a, c_ = min(t[0] for t in ta) / INNER, min(t[0] for t in tc) / INNER
        bound = c_ * bytes_accumulate / bytes_compute * 1.10
        print(f"  {name:32s} {len(pf.program.instructions):2d} instructions, {pf.program.n_registers} registers | accumulate {a * 1e3:7.3f} ms "
              f"{bytes_accumulate / a / 1e9:7.1f} GB/s | compute {c_ * 1e3:7.3f} ms {bytes_compute / c_ / 1e9:7.1f} GB/s | bound "
              f"{bound * 1e3:7.3f} ms: {'within' if a <= bound else 'MISSED'}", flush=True)


def time_steps(N):
    dt = 1e-3
    out = {}
    for kind, make in (("Forcing(func), sampled", ocn.Forcing), ("ContinuousForcing(func), traced", ocn.ContinuousForcing)):
        grid = ocn.RectilinearGrid(ocn.GPU(), size=N, x=(0, 1), y=(0, 1), z=(-1, 0), topology=("Periodic", "Periodic", "Bounded"))
        model = ocn.NonhydrostaticModel(grid, advection=ocn.WENO(), forcing={"u": make(forcing_function)})
        rng = np.random.default_rng(0)
        ocn.set(model, u=lambda x, y, z: 0.1 * np.sin(2 * np.pi * x) * np.cos(2 * np.pi * y) + 0 * z,
                v=lambda x, y, z: -0.1 * np.cos(2 * np.pi * x) * np.sin(2 * np.pi * y) + 0 * z)
        ocn.time_step(model, dt)
        t = timed(lambda: ocn.time_step(model, dt), steps)
        ocn.flush_tendencies(model)
        out[kind] = (t, model.u.interior())
        print(f"  time_step, {kind:34s} {t[0] * 1e3:9.2f} ms [{t[1] * 1e3:.2f}, {t[2] * 1e3:.2f}]", flush=True)
        del model
        torch.cuda.empty_cache()
    (ts, us), (tt, ut) = out.values()
    print(f"  sampled / traced = {ts[0] / tt[0]:.2f}; max |u_sampled - u_traced| = {float(np.max(np.abs(us - ut))):.2e} (max |u| = {float(np.max(np.abs(us))):.2e})")


for N in sizes:
    print(f"grid {N[0]} x {N[1]} x {N[2]}, halo 3, {reps} windows of {INNER} launches (best median of two alternating runs); {steps} time steps")
    kernels(N)
    time_steps(N)
