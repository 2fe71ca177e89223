#!/usr/bin/env python3
"""The reference's examples/convecting_plankton.jl on the MI355X backend: same grid, physics, boundary conditions, forcing, initial
condition and time-step wizard; plotting / JLD2 output left out.

    python examples/convecting_plankton.py [--size 64 64] [--stop-hours 24] [--steps N]

The plankton "dynamics" is a forcing function of the plankton tracer itself, (μ₀ exp(z / λ) - m) P: a ContinuousForcing with
field_dependencies, traced once and evaluated on the device.  The host folds exp(z / λ) -- and with it μ₀ exp(z / λ) - m -- into one
vector on the z nodes; the device multiplies it with P.  The top buoyancy flux is a function of the time that the host samples.
--steps N stops after N time steps (the tests run three on a small grid).
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import oceananigans_jl_amd as ocn

minutes, hour, hours, day = 60.0, 3600.0, 3600.0, 86400.0
ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, nargs=2, default=(64, 64), metavar=("NX", "NZ"))
ap.add_argument("--stop-hours", type=float, default=24.0)
ap.add_argument("--steps", type=int, default=None)
ap.add_argument("--math", choices=("fast", "strict"), default="fast")
a = ap.parse_args()
ocn.set_math_mode(ocn.MATH_FAST if a.math == "fast" else ocn.MATH_STRICT)

Nx, Nz = a.size
grid = ocn.RectilinearGrid(ocn.GPU(), size=(Nx, Nz), x=(0, 64), z=(-64, 0), halo=(3, 3), topology=("Periodic", "Flat", "Bounded"))


def buoyancy_flux(x, t, params):
    return params["initial_buoyancy_flux"] * np.exp(-t ** 4 / (24 * params["shut_off_time"] ** 4))


buoyancy_flux_parameters = dict(initial_buoyancy_flux=1e-8,  # m² s⁻³
                                shut_off_time=2 * hours)
buoyancy_flux_bc = ocn.FluxBoundaryCondition(buoyancy_flux, parameters=buoyancy_flux_parameters)
N2 = 1e-4  # s⁻²
buoyancy_bcs = ocn.FieldBoundaryConditions(top=buoyancy_flux_bc, bottom=ocn.GradientBoundaryCondition(N2))


def growing_and_grazing(x, z, t, P, params):
    return (params["mu0"] * ocn.exp(z / params["lam"]) - params["m"]) * P


plankton_dynamics_parameters = dict(mu0=1 / day,   # surface growth rate
                                    lam=5,         # sunlight attenuation length scale (m)
                                    m=0.1 / day)   # mortality rate due to virus and zooplankton grazing
plankton_dynamics = ocn.ContinuousForcing(growing_and_grazing, field_dependencies="P", parameters=plankton_dynamics_parameters)

model = ocn.NonhydrostaticModel(grid, advection=ocn.UpwindBiased(order=5), closure=ocn.ScalarDiffusivity(nu=1e-4, kappa=1e-4),
                                coriolis=ocn.FPlane(f=1e-4), tracers=("b", "P"),  # P for Plankton
                                buoyancy=ocn.BuoyancyTracer(), forcing={"P": plankton_dynamics}, boundary_conditions={"b": buoyancy_bcs})

mixed_layer_depth = 32  # m
rng = np.random.default_rng(0)
stratification = lambda z: np.where(z < -mixed_layer_depth, N2 * z, -N2 * mixed_layer_depth)
noise = lambda z: 1e-4 * N2 * grid.Lz * rng.standard_normal((Nx, 1, np.shape(z)[-1])) * np.exp(z / 4)
ocn.set(model, b=lambda x, y, z: stratification(z) + noise(z), P=1.0)
P_initial = model.field("P").interior()

dt, stop_time = 2 * minutes, a.stop_hours * hours
wizard = ocn.TimeStepWizard(cfl=1.0, max_dt=2 * minutes)
t0 = time.perf_counter()
while model.clock.time < stop_time and (a.steps is None or model.clock.iteration < a.steps):
    if model.clock.iteration % 10 == 0:
        dt = wizard(model, dt)
    if model.clock.iteration % 100 == 0:
        print(f"Iteration: {model.clock.iteration}, time: {model.clock.time / hour:.3f} hours, Δt: {dt:.1f} s", flush=True)
    ocn.time_step(model, min(dt, stop_time - model.clock.time))
ocn.flush_tendencies(model)
ocn.sync_device()
fields = {n: model.field(n).interior() for n in ("u", "v", "w", "b", "P")}
P = fields["P"]
avg_P = P.mean(axis=(0, 1))
print(f"done: {model.clock.iteration} iterations, {time.perf_counter() - t0:.1f} s; max(|w|) = {np.abs(fields['w']).max():.2e} m s⁻¹, "
      f"P in [{P.min():.6f}, {P.max():.6f}], horizontal mean of P at the surface {avg_P[-1]:.6f}, at the bottom {avg_P[0]:.6f}")
print(f"finite fields: {all(bool(np.all(np.isfinite(f))) for f in fields.values())}")
print(f"P changed: {not np.array_equal(P, P_initial)}")
