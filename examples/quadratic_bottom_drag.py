#!/usr/bin/env python3
"""Spin-down by quadratic bottom drag: a (Periodic, Periodic, Bounded) box whose uniform flow, with a little noise, is decelerated from
below by the drag law of the reference's tilted-bottom-boundary-layer example (examples/tilted_bottom_boundary_layer.jl:110-126),

    drag_u(x, y, t, u, v, p) = -cᴰ √(u² + v²) u,    drag_v = -cᴰ √(u² + v²) v,    cᴰ = (κ / log(z₁ / z₀))²

passed as FluxBoundaryCondition(drag_u, field_dependencies=("u", "v"), parameters=...).  The functions are called ONCE, with symbolic
operands, when the model is built; the expression they return is evaluated on the device at every tendency evaluation.
The script prints the domain-mean speed, an ocn.Average computed on the device.

    python examples/quadratic_bottom_drag.py [--n 64] [--nz 32] [--stop-time 200] [--max-iterations 0]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import oceananigans_jl_amd as ocn

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=64)
ap.add_argument("--nz", type=int, default=32)
ap.add_argument("--stop-time", type=float, default=200.0)
ap.add_argument("--max-iterations", type=int, default=0, help="stop after this many iterations (0 = run to stop-time)")
a = ap.parse_args()

L, H, U0, nu = 100.0, 20.0, 0.1, 1e-3
grid = ocn.RectilinearGrid(ocn.GPU(), size=(a.n, a.n, a.nz), x=(0, L), y=(0, L), z=(-H, 0), topology=("Periodic", "Periodic", "Bounded"))

kappa, z0 = 0.4, 0.1                                   # von Kármán constant, roughness length
z1 = grid.nodes_1d(2, False)[0] + H                    # height of the lowest cell centre above the bottom
cd = (kappa / np.log(z1 / z0)) ** 2


def drag_u(x, y, t, u, v, p):
    return -p["cᴰ"] * ocn.sqrt(u ** 2 + v ** 2) * u


def drag_v(x, y, t, u, v, p):
    return -p["cᴰ"] * ocn.sqrt(u ** 2 + v ** 2) * v


drag = lambda f: ocn.FluxBoundaryCondition(f, field_dependencies=("u", "v"), parameters={"cᴰ": cd})
model = ocn.NonhydrostaticModel(grid, advection=ocn.WENO(), timestepper="RungeKutta3", closure=ocn.ScalarDiffusivity(ν=nu),
                                boundary_conditions={"u": ocn.FieldBoundaryConditions(bottom=drag(drag_u)),
                                                     "v": ocn.FieldBoundaryConditions(bottom=drag(drag_v))})
rng = np.random.default_rng(1)
noise = lambda x, y, z: 1e-3 * rng.standard_normal(np.broadcast(x, y, z).shape)
ocn.set(model, u=lambda x, y, z: U0 + noise(x, y, z), v=noise, w=noise)
speed = ocn.ComputedField(ocn.Average(ocn.sqrt(model.u * model.u + model.v * model.v)))
wizard = ocn.TimeStepWizard(cfl=0.5, max_dt=5.0)
print(f"cᴰ = {cd:.4e} (z₁ = {z1:.4f}, z₀ = {z0}); a column of depth {H} loses momentum at the rate cᴰ |U| / H = {cd * U0 / H:.3e} per unit time")


def report():
    s = float(speed.compute().interior_view().item())
    print("Iter: %5d, t = %8.3f, wall %6.1f s, dt = %.4f | domain-mean speed %.6e" % (model.clock.iteration, model.clock.time,
                                                                                      time.perf_counter() - t0, dt, s), flush=True)
    return s


dt, t0 = 1.0, time.perf_counter()
first = None
while model.clock.time < a.stop_time and not (a.max_iterations and model.clock.iteration >= a.max_iterations):
    if model.clock.iteration % 20 == 0:
        dt = wizard(model, dt)
        s = report()
        first = s if first is None else first
    ocn.time_step(model, min(dt, a.stop_time - model.clock.time))
ocn.flush_tendencies(model)
ocn.sync_device()
last = report()
assert np.isfinite(last) and last < first  # the drag only ever takes momentum out
