#!/usr/bin/env python3
"""Lagrangian particles in free convection: a 64³ (Periodic, Periodic, Bounded) box cooled from above (a buoyancy tracer with a surface
flux, WENO advection, ScalarDiffusivity, RungeKutta3) that carries a few thousand LagrangianParticles released on one level.  The
particles track the buoyancy and the vertical velocity they feel; the script prints how their depths spread as the convection sets in.

    python examples/lagrangian_particles.py [--n 64] [--particles 4096] [--stop-time 40] [--restitution 1.0]

The particles are advected on the device (csrc/particles.hip) after the update_state! of every RK3 stage, with the pressure-corrected
velocities of that stage, as step_lagrangian_particles! of the reference does (src/TimeSteppers/runge_kutta_3.jl:111, 127, 148)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import oceananigans_jl_amd as ocn

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=64)
ap.add_argument("--particles", type=int, default=4096)
ap.add_argument("--stop-time", type=float, default=40.0)
ap.add_argument("--restitution", type=float, default=1.0)
ap.add_argument("--max-iterations", type=int, default=0, help="stop after this many iterations (0 = run to stop-time)")
a = ap.parse_args()

L, H, Qb, N2, nu = 2.0, 1.0, 1e-2, 1e-1, 2e-4
grid = ocn.RectilinearGrid(ocn.GPU(), size=(a.n, a.n, a.n), x=(0, L), y=(0, L), z=(-H, 0), topology=("Periodic", "Periodic", "Bounded"))
rng = np.random.default_rng(1)
P = a.particles
particles = ocn.LagrangianParticles(x=rng.uniform(0, L, P), y=rng.uniform(0, L, P), z=np.full(P, -0.25 * H), restitution=a.restitution,
                                    tracked_fields={"b": "b", "w": "w"}, properties={"b": np.zeros(P), "w": np.zeros(P)})
b_bcs = ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(Qb))  # a positive upward buoyancy flux: cooling
model = ocn.NonhydrostaticModel(grid, advection=ocn.WENO(), timestepper="RungeKutta3", tracers=("b",), buoyancy=ocn.BuoyancyTracer(),
                                closure=ocn.ScalarDiffusivity(ν=nu, κ=nu), boundary_conditions={"b": b_bcs}, particles=particles)
print(model.particles)
ocn.set(model, b=lambda x, y, z: N2 * z + 1e-4 * rng.standard_normal(np.broadcast(x, y, z).shape))
wizard = ocn.TimeStepWizard(cfl=0.5, max_dt=0.2)


def report():
    z, b, w = (model.particles.properties[k].cpu().numpy() for k in "zbw")
    print("Iter: %5d, t = %7.3f, wall %6.1f s, dt = %.4f | particle depth: mean %.4f, std %.4f, min %.4f, max %.4f | tracked b: mean %+.3e, "
          "w: rms %.3e" % (model.clock.iteration, model.clock.time, time.perf_counter() - t0, dt, z.mean(), z.std(), z.min(), z.max(), b.mean(),
                           np.sqrt((w ** 2).mean())), flush=True)
    return z


dt, t0 = 0.05, time.perf_counter()
while model.clock.time < a.stop_time and not (a.max_iterations and model.clock.iteration >= a.max_iterations):
    if model.clock.iteration % 50 == 0:
        dt = wizard(model, dt)
        report()
    ocn.time_step(model, min(dt, a.stop_time - model.clock.time))
ocn.flush_tendencies(model)
ocn.sync_device()
z = report()
assert len(model.particles) == P and np.all(np.isfinite(z)) and z.min() >= -H and z.max() <= 0.0  # the walls keep every particle inside
