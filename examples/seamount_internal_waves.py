#!/usr/bin/env python3
"""Internal waves over a seamount: the geometry and the stratification of the reference's examples/internal_tide.jl on
ImmersedBoundaryGrid(grid, GridFittedBottom(h)).  A Gaussian hill of 250 m (width 20 km) in 2 km of water, N² = 1e-4 s⁻², an f-plane at
45° S, and an initial barotropic flow U = ε ω₂ σ (the reference's tidal velocity for an excursion parameter of 0.1) that adjusts over the
hill and radiates internal waves (and turns inertially: nothing balances it).

It is NOT the reference example; it stays within what the model takes on an immersed grid:
  * a thin periodic y (4 cells) where the reference has a Flat y;
  * GridFittedBottom (full cells, a staircase) where the reference has PartialCellBottom;
  * VectorInvariant() momentum and Centered() tracers, second order, where the reference has WENO();
  * no forcing: the flow is started and left alone, where the reference drives it with the M₂ tide.

    python examples/seamount_internal_waves.py [--nx 250] [--nz 125] [--hours 12]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import oceananigans_jl_amd as ocn

ap = argparse.ArgumentParser()
ap.add_argument("--nx", type=int, default=250)
ap.add_argument("--nz", type=int, default=125)
ap.add_argument("--hours", type=float, default=12.0)
a = ap.parse_args()

kilometers, minutes, hours = 1e3, 60.0, 3600.0
H, Lx, Ny = 2 * kilometers, 2000 * kilometers, 4
underlying_grid = ocn.RectilinearGrid(ocn.GPU(), size=(a.nx, Ny, a.nz), x=(-Lx / 2, Lx / 2), y=(0, Ny * Lx / a.nx), z=(-H, 0),
                                      topology=("Periodic", "Periodic", "Bounded"), halo=(4, 4, 4))
h0, width = 250.0, 20 * kilometers
grid = ocn.ImmersedBoundaryGrid(underlying_grid, ocn.GridFittedBottom(lambda x, y: -H + h0 * np.exp(-x ** 2 / (2 * width ** 2)) + 0 * y))
kbot = grid.kbot[:, 0]
print("bathymetry: %d of %d columns rise above the floor, the summit immerses %d of %d cells (bottom height %.0f m)" % (
    (kbot > 0).sum(), a.nx, kbot.max(), a.nz, grid.immersed_boundary.bottom_height.max()))

f = 2 * 7.292115e-5 * np.sin(np.deg2rad(-45.0))
omega2 = 2 * np.pi / (12.421 * hours)
U_tidal = 0.1 * omega2 * width
N2 = 1e-4
model = ocn.HydrostaticFreeSurfaceModel(grid, coriolis=ocn.FPlane(f=f), buoyancy=ocn.BuoyancyTracer(), tracers=("b",))
print("free surface: SplitExplicitFreeSurface(grid, cfl = 0.7), the default on an immersed grid; halo %s" % ((model.grid.Hx, model.grid.Hy, model.grid.Hz),))
model.set(u=U_tidal, b=lambda x, y, z: N2 * z + 0 * x + 0 * y)

immersed = ocn.immersed_cell(model.grid)
u_masked = ocn.immersed_peripheral_node(model.grid, 1)   # the u faces next to an immersed cell: held at 0
dt, stop_time = 5 * minutes, a.hours * hours
t0 = time.perf_counter()
while model.clock.time < stop_time:
    it = model.clock.iteration
    if it % 24 == 0:
        u, w = model.u.interior(), model.w.interior()
        print("i: %4d, t: %5.2f hours, wall time: %5.1f s, max |u - U|: %.3e m/s, max |w|: %.3e m/s" % (
            it, model.clock.time / hours, time.perf_counter() - t0, np.abs(np.where(u_masked, 0.0, u - U_tidal)).max(), np.abs(w).max()), flush=True)
    model.time_step(min(dt, stop_time - model.clock.time))
ocn.sync_device()
u, b = model.u.interior(), model.field("b").interior()
print("done: %d iterations in %.1f s; u is exactly 0 on %d faces next to the bottom, b on %d immersed cells" % (
    model.clock.iteration, time.perf_counter() - t0, int((u[u_masked] == 0).sum()), int((b[immersed] == 0).sum())))
if not (np.isfinite(u).all() and np.isfinite(b).all()):
    sys.exit("the fields are not finite")
