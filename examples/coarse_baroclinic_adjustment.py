#!/usr/bin/env python3
"""Coarse baroclinic adjustment (the reference's validation/mesoscale_turbulence/coarse_baroclinic_adjustment.jl, its parameters): a front on
a grid of 50 km cells, too coarse to resolve the baroclinic eddies that would flatten it, slumps through the Gent-McWilliams eddy velocities of
IsopycnalSkewSymmetricDiffusivity(κ_skew = 1e3, κ_symmetric = 1e3, slope_limiter = FluxTapering(1e-2)), while a passive tracer spreads along the
isopycnals.  Here the domain is doubly periodic (the closure's kernels wrap x and y): 2000 km x 1000 km x 1 km with 40 x 20 x 20 cells, the
reference's front in x at -Lx / 4 and its mirror image at +Lx / 4, so that b is periodic.  HydrostaticFreeSurfaceModel with flux-form WENO()
momentum and tracer advection, FPlane(latitude = -45), BuoyancyTracer, the default ImplicitFreeSurface and the closure pair
(HorizontalScalarBiharmonicDiffusivity(ν = κ = Δy⁴ / 10 days), IsopycnalSkewSymmetricDiffusivity); the reference's third closure, a
VerticalScalarDiffusivity, has no place in a pair yet.

    b(x, y, z, t = 0) = N² z + Δb (ramp(x + Lx / 4) - ramp(x - Lx / 4)),   N² = 4e-6 s⁻², M² = 8e-8 s⁻², Δ = 100 km, Δb = Δ M²
    c(x, y, z, t = 0) = exp(-y² / 2Δc²) exp(-(z + Lz / 4)² / 2Δz²),        Δc = 200 km, Δz = 100 m

Δt is 20 minutes.  Progress is printed every 100 iterations: max |u|, |v|, |w|, max |uₑ| and the available potential energy of the front,
-Σ (b - <b>_xy) z V, which the eddy velocities release.

    python examples/coarse_baroclinic_adjustment.py [--n 20] [--nz 20] [--days 30] [--no-closure]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import oceananigans_jl_amd as ocn

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=20)
ap.add_argument("--nz", type=int, default=20)
ap.add_argument("--days", type=float, default=30.0)
ap.add_argument("--no-closure", action="store_true", help="the biharmonic closure alone: the front stays")
a = ap.parse_args()

kilometers, minutes, days = 1e3, 60.0, 86400.0
Ly, Lz = 1000 * kilometers, 1 * kilometers
Lx = 2 * Ly
grid = ocn.RectilinearGrid(ocn.GPU(), size=(2 * a.n, a.n, a.nz), x=(-Lx / 2, Lx / 2), y=(-Ly / 2, Ly / 2), z=(-Lz, 0),
                           topology=("Periodic", "Periodic", "Bounded"), halo=(3, 3, 3))
dy = Ly / a.n
horizontal_closure = ocn.HorizontalScalarBiharmonicDiffusivity(ν=dy ** 4 / (10 * days), κ=dy ** 4 / (10 * days))
gent_mcwilliams_diffusivity = ocn.IsopycnalSkewSymmetricDiffusivity(κ_skew=1e3, κ_symmetric=1e3, slope_limiter=ocn.FluxTapering(1e-2))
closure = horizontal_closure if a.no_closure else (horizontal_closure, gent_mcwilliams_diffusivity)
model = ocn.HydrostaticFreeSurfaceModel(grid, coriolis=ocn.FPlane(latitude=-45), buoyancy=ocn.BuoyancyTracer(), tracers=("b", "c"),
                                        closure=closure, momentum_advection=ocn.WENO(), tracer_advection=ocn.WENO())
print(gent_mcwilliams_diffusivity.summary() if not a.no_closure else repr(horizontal_closure))

N2, M2, width = 4e-6, 8e-8, 100 * kilometers
dz_c, dc, db = 100.0, 2 * width, width * M2


def ramp(x, width):
    """linear ramp from 0 to 1 between -width / 2 and +width / 2"""
    return np.minimum(np.maximum(0.0, x / width + 0.5), 1.0)


model.set(b=lambda x, y, z: N2 * z + db * (ramp(x + Lx / 4, width) - ramp(x - Lx / 4, width)) + 0 * y,
          c=lambda x, y, z: np.exp(-y ** 2 / (2 * dc ** 2)) * np.exp(-(z + Lz / 4) ** 2 / (2 * dz_c ** 2)) + 0 * x)

zc = np.asarray(grid.nodes_1d(2, False), dtype=np.float64).reshape(1, 1, -1)
volume = grid.dx * grid.dy * (Lz / a.nz)


def available_potential_energy():
    b = model.field("b").interior()
    return float(-np.sum((b - b.mean(axis=(0, 1), keepdims=True)) * zc) * volume)


dt, stop_time = 20 * minutes, a.days * days
c0 = float(np.sum(model.field("c").interior()))
ape0 = available_potential_energy()
t0 = time.perf_counter()
while model.clock.time < stop_time:
    it = model.clock.iteration
    if it % 100 == 0:
        u, v, w = (float(f.interior_view().abs().max()) for f in model.velocities)
        ue = 0.0 if a.no_closure else float(model.diffusivity_fields["u"].interior_view().abs().max())
        print("[%05.2f%%] i: %d, t: %.2f days, wall time: %.1f s, max(u): (%6.3e, %6.3e, %6.3e) m/s, max(uₑ): %6.3e m/s, APE / APE₀: %.4f" % (
            100 * model.clock.time / stop_time, it, model.clock.time / days, time.perf_counter() - t0, u, v, w, ue,
            available_potential_energy() / ape0), flush=True)
    model.time_step(min(dt, stop_time - model.clock.time))
ocn.sync_device()
b, c = model.field("b").interior(), model.field("c").interior()
print("done: %d iterations in %.1f s; APE / APE₀ = %.4f; Σc / Σc₀ - 1 = %.2e; surface b along x at y = 0:" % (
    model.clock.iteration, time.perf_counter() - t0, available_potential_energy() / ape0, float(np.sum(c)) / c0 - 1))
print(np.array2string(b[::max(1, a.n // 5), a.n // 2, -1], precision=3))
if not (np.isfinite(b).all() and np.isfinite(c).all()):
    sys.exit("a tracer is not finite")
