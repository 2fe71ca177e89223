#!/usr/bin/env python3
"""Convective deepening of a mixed layer in a hydrostatic box: a (Periodic, Periodic, Bounded) HydrostaticFreeSurfaceModel whose linearly
stratified temperature, T = T₀ + Γ z, is cooled through the top by a FluxBoundaryCondition.  A hydrostatic model cannot overturn, so the
cold water stays on top unless a closure mixes it: ConvectiveAdjustmentVerticalDiffusivity(convective_κz = 1) sets κ = 1 m² s⁻¹ on every
face where ∂z b < 0 and the background value elsewhere, vertically implicit by default -- the explicit limit Δz² / 2κ would be 2 s here,
the step is a minute.  Non-penetrative convection erodes the stratification to the depth h(t) = √(2 J t / Γ) (the heat lost, J t, is the
triangle Γ h² / 2 cut from the profile); the script prints the depth of the deepest unstable face next to it as it deepens.

    python examples/convective_adjustment.py [--n 16] [--nz 50] [--hours 24] [--dt 60]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import oceananigans_jl_amd as ocn

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=16)
ap.add_argument("--nz", type=int, default=50)
ap.add_argument("--hours", type=float, default=24.0)
ap.add_argument("--dt", type=float, default=60.0)
a = ap.parse_args()

L, H = 1000.0, 100.0
T0, Gamma = 20.0, 0.01            # surface temperature and stratification ∂z T [K m⁻¹]
Q, rho, cp = 200.0, 1026.0, 3991.0
J = Q / (rho * cp)                # temperature flux out of the top [K m s⁻¹]
grid = ocn.RectilinearGrid(ocn.GPU(), size=(a.n, a.n, a.nz), x=(0, L), y=(0, L), z=(-H, 0), topology=("Periodic", "Periodic", "Bounded"))
closure = ocn.ConvectiveAdjustmentVerticalDiffusivity(convective_κz=1.0, background_κz=1e-5, convective_νz=0.1, background_νz=1e-4)
model = ocn.HydrostaticFreeSurfaceModel(grid, tracers=("T", "S"), buoyancy=ocn.SeawaterBuoyancy(), coriolis=ocn.FPlane(f=1e-4), closure=closure,
                                        boundary_conditions={"T": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(J))})
rng = np.random.default_rng(1)
model.set(T=lambda x, y, z: T0 + Gamma * z + 1e-6 * rng.standard_normal(np.broadcast(x, y, z).shape), S=35.0)
print(closure)
print(f"Δz = {H / a.nz:g} m, Δt = {a.dt:g} s: diffusion number Δt convective_κz / Δz² = {a.dt * 1.0 / (H / a.nz) ** 2:g}; J = {J:.3e} K m s⁻¹")
z_faces = np.asarray(grid.nodes_1d(2, True))[:a.nz]   # faces k = 1..Nz


def mixed_layer_depth():
    """the depth of the deepest face that the last update_state found unstable, the median over the columns"""
    unstable = model.diffusivity_fields["kappa_c"].interior()[:, :, :a.nz] == closure.convective_κz
    deepest = np.where(unstable.any(axis=2), -z_faces[np.argmax(unstable, axis=2)], 0.0)
    return float(np.median(deepest))


t0, every = time.perf_counter(), max(1, int(round(2 * 3600 / a.dt)))
depths = []
while model.clock.time < a.hours * 3600:
    if model.clock.iteration % every == 0:
        h = mixed_layer_depth()
        depths.append(h)
        print("Iter: %5d, t = %5.1f h, wall %5.1f s | mixed-layer depth %6.2f m, non-penetrative estimate %6.2f m, surface T %.4f" % (
            model.clock.iteration, model.clock.time / 3600, time.perf_counter() - t0, h, np.sqrt(2 * J * model.clock.time / Gamma),
            float(model.field("T").interior()[:, :, -1].mean())), flush=True)
    model.time_step(a.dt)
ocn.sync_device()
h, estimate = mixed_layer_depth(), np.sqrt(2 * J * model.clock.time / Gamma)
print(f"after {model.clock.time / 3600:.1f} h: mixed-layer depth {h:.2f} m, non-penetrative estimate {estimate:.2f} m")
T = model.field("T").interior()
assert np.isfinite(T).all() and h > depths[0]
assert abs(h - estimate) <= 3 * H / a.nz  # the layer has deepened to the estimate, within three cells
