#!/usr/bin/env python3
"""Baroclinic adjustment (the reference's examples/baroclinic_adjustment.jl, its parameters): a front in a stratified channel on a
β-plane goes baroclinically unstable.  A (Periodic, Bounded, Bounded) channel of 1000 km x 1000 km x 1 km with 48 x 48 x 8 cells,
HydrostaticFreeSurfaceModel with flux-form WENO() momentum and tracer advection, BetaPlane(latitude = -45), BuoyancyTracer and the default
ImplicitFreeSurface (FFT solver: Fourier in x, cosine transform between the walls in y).

    b(x, y, z, t = 0) = N² z + Δb ramp(y, Δy) + ϵb randn(),   N² = 1e-5 s⁻², M² = 1e-7 s⁻², Δy = 100 km, Δb = Δy M², ϵb = 1e-2 Δb

Δt starts at 20 minutes; the time-step wizard (cfl = 0.2, max_Δt = 20 minutes) is consulted every 20 iterations.  Progress is printed
every 100 iterations: max |u|, |v|, |w| and the next Δt, as the reference's print_progress does.  The meridional velocity on the two
walls stays exactly zero.

    python examples/baroclinic_adjustment.py [--n 48] [--nz 8] [--days 20]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import oceananigans_jl_amd as ocn

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=48)
ap.add_argument("--nz", type=int, default=8)
ap.add_argument("--days", type=float, default=20.0)
a = ap.parse_args()

kilometers, minutes, days = 1e3, 60.0, 86400.0
Lx, Ly, Lz = 1000 * kilometers, 1000 * kilometers, 1 * kilometers
grid = ocn.RectilinearGrid(ocn.GPU(), size=(a.n, a.n, a.nz), x=(0, Lx), y=(-Ly / 2, Ly / 2), z=(-Lz, 0),
                           topology=("Periodic", "Bounded", "Bounded"))
model = ocn.HydrostaticFreeSurfaceModel(grid, coriolis=ocn.BetaPlane(latitude=-45), buoyancy=ocn.BuoyancyTracer(), tracers=("b",),
                                        momentum_advection=ocn.WENO(), tracer_advection=ocn.WENO())

N2, M2, dy_front = 1e-5, 1e-7, 100 * kilometers
db = dy_front * M2
eps_b = 1e-2 * db
rng = np.random.default_rng(1)


def ramp(y, width):
    """linear ramp from 0 to 1 between -width / 2 and +width / 2"""
    return np.minimum(np.maximum(0.0, y / width + 0.5), 1.0)


model.set(b=lambda x, y, z: N2 * z + db * ramp(y, dy_front) + eps_b * rng.standard_normal(np.broadcast(x, y, z).shape))

wizard = ocn.TimeStepWizard(cfl=0.2, max_dt=20 * minutes)
dt, stop_time = 20 * minutes, a.days * days
t0 = time.perf_counter()
while model.clock.time < stop_time:
    it = model.clock.iteration
    if it % 20 == 0 and it > 0:
        dt = wizard(model, dt)
    if it % 100 == 0:
        u, v, w = (float(f.interior_view().abs().max()) for f in model.velocities)
        print("[%05.2f%%] i: %d, t: %.2f days, wall time: %.1f s, max(u): (%6.3e, %6.3e, %6.3e) m/s, next Δt: %.1f minutes" % (
            100 * model.clock.time / stop_time, it, model.clock.time / days, time.perf_counter() - t0, u, v, w, dt / minutes), flush=True)
    model.time_step(min(dt, stop_time - model.clock.time))
ocn.sync_device()
v = model.v.parent()
b = model.field("b").interior()
print("done: %d iterations in %.1f s; max |v| on the south / north wall faces: %g / %g; b in [%.3e, %.3e]; zonal-mean surface b, south to north:" % (
    model.clock.iteration, time.perf_counter() - t0, np.abs(v[:, grid.Hy, :]).max(), np.abs(v[:, grid.Hy + grid.Ny, :]).max(), b.min(), b.max()))
print(np.array2string(b[:, :, -1].mean(axis=0)[::max(1, a.n // 8)], precision=3))
if not np.isfinite(b).all():
    sys.exit("the buoyancy is not finite")
