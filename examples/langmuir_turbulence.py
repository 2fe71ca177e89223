#!/usr/bin/env python3
"""The reference's examples/langmuir_turbulence.jl on the MI355X backend: same grid (32^3, extent (128, 128, 64)), wave parameters, Stokes
drift, boundary conditions, Coriolis, closure, initial condition, time-step wizard and progress message; JLD2 output and plotting left out.

    python examples/langmuir_turbulence.py [--stop-hours 4] [--max-steps N] [--math fast|strict] [--host] [--averages]

The whole RK3 step runs behind one C call (ocn.ModelRK3Driver) unless --host asks for the Python host.  --max-steps (or the environment
variable LANGMUIR_MAX_STEPS) caps the number of time steps: the test suite runs 20.  --averages builds the reference example's horizontal
averages U, V, B, wu, wv (langmuir_turbulence.jl:221-225) once, computes them on the device at every progress message and prints them.
"""
import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import oceananigans_jl_amd as ocn

minute, hour = 60.0, 3600.0
g_Earth = 9.80665


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--stop-hours", type=float, default=4.0)
    ap.add_argument("--max-steps", type=int, default=int(os.environ.get("LANGMUIR_MAX_STEPS", "0")), help="0: no cap")
    ap.add_argument("--math", choices=("fast", "strict"), default="fast")
    ap.add_argument("--host", action="store_true", help="time_step(model, dt) from Python instead of ModelRK3Driver")
    ap.add_argument("--averages", action="store_true", help="print the horizontal averages U, V, B, wu, wv with every progress message")
    a = ap.parse_args(argv)
    ocn.set_math_mode(ocn.MATH_FAST if a.math == "fast" else ocn.MATH_STRICT)

    Nx = Ny = Nz = 32
    grid = ocn.RectilinearGrid(ocn.GPU(), size=(Nx, Ny, Nz), x=(0, 128), y=(0, 128), z=(-64, 0),
                               topology=("Periodic", "Periodic", "Bounded"), halo=(3, 3, 3))

    # The Stokes drift profile of a deep-water surface wave
    amplitude = 0.8                                  # m
    wavelength = 60.0                                # m
    wavenumber = 2 * math.pi / wavelength            # m⁻¹
    frequency = math.sqrt(g_Earth * wavenumber)      # s⁻¹
    vertical_scale = wavelength / (4 * math.pi)      # the vertical scale over which the Stokes drift decays
    Us = amplitude ** 2 * wavenumber * frequency     # m s⁻¹, Stokes drift velocity at the surface

    def dz_us(z, t):  # ∂z_uˢ(z, t)
        return 1 / vertical_scale * Us * np.exp(z / vertical_scale)

    # (the profile does not depend on t: sampled once, which is what ModelRK3Driver takes)
    stokes_drift = ocn.UniformStokesDrift(dz_us=dz_us, steady=True)

    tau_x = -3.72e-5   # m² s⁻², surface kinematic momentum flux
    Jb = 2.307e-8      # m² s⁻³, surface buoyancy flux
    N2 = 1.936e-5      # s⁻², initial and bottom buoyancy gradient
    u_bcs = ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(tau_x))
    b_bcs = ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(Jb), bottom=ocn.GradientBoundaryCondition(N2))

    model = ocn.NonhydrostaticModel(grid, coriolis=ocn.FPlane(f=1e-4), advection=ocn.WENO(), timestepper="RungeKutta3", tracers=("b",),
                                    buoyancy=ocn.BuoyancyTracer(), closure=ocn.AnisotropicMinimumDissipation(), stokes_drift=stokes_drift,
                                    boundary_conditions={"u": u_bcs, "b": b_bcs})
    print(model.stokes_drift)

    rng = np.random.default_rng(0)
    Xi = lambda z: rng.standard_normal(np.broadcast_shapes(np.shape(z), (Nx, Ny, 1))) * np.exp(z / 4)  # noise, decaying with depth
    initial_mixed_layer_depth = 33.0  # m
    stratification = lambda z: np.where(z < -initial_mixed_layer_depth, N2 * z, N2 * (-initial_mixed_layer_depth))
    u_star = math.sqrt(abs(tau_x))
    ocn.set(model, u=lambda x, y, z: u_star * 1e-1 * Xi(z), w=lambda x, y, z: u_star * 1e-1 * Xi(z),
            b=lambda x, y, z: stratification(z) + 1e-1 * Xi(z) * N2 * grid.Lz)

    dt, stop_time = 45.0, a.stop_hours * hour
    wizard = ocn.TimeStepWizard(cfl=1.0, max_dt=1 * minute)
    driver = None if a.host else ocn.ModelRK3Driver(model)

    averages = {}
    if a.averages:  # built once: lowering, validation and allocation happen here, compute() only enqueues kernels
        u, v, w, b = model.u, model.v, model.w, model.field("b")
        averages = {name: ocn.ComputedField(ocn.Average(op, dims=(1, 2))) for name, op in
                    (("U", u), ("V", v), ("B", b), ("wu", w * u), ("wv", w * v))}

    def flush():
        if driver is not None:
            driver.flush()

    t0 = time.perf_counter()
    while model.clock.time < stop_time and not (a.max_steps and model.clock.iteration >= a.max_steps):
        it = model.clock.iteration
        if it % 10 == 0 or it % 20 == 0:
            flush()  # the wizard and the progress message read the model's own arrays
        if it % 10 == 0:
            dt = wizard(model, dt)
        if it % 20 == 0:
            umax = [float(f.data.abs().max()) for f in model.velocities]
            print(f"i: {it:04d}, t: {model.clock.time / minute:7.3f} min, Δt: {dt:6.2f} s, umax = ({umax[0]:.1e}, {umax[1]:.1e}, {umax[2]:.1e}) ms⁻¹, "
                  f"wall time: {time.perf_counter() - t0:.1f} s", flush=True)
            for name, avg in averages.items():
                profile = avg.compute().interior()[0, 0, :]
                print(f"    {name:>2s}(z): " + " ".join(f"{x: .2e}" for x in profile[::max(1, len(profile) // 8)]), flush=True)
        step = min(dt, stop_time - model.clock.time)
        if driver is not None:
            driver.time_step(step)
        else:
            ocn.time_step(model, step)
    flush()
    ocn.sync_device()
    nan = ocn.hasnan(model)
    print(f"done: {model.clock.iteration} iterations to t = {model.clock.time / minute:.2f} min in {time.perf_counter() - t0:.1f} s; "
          f"Δt = {dt:.3f} s, max(|w|) = {float(model.w.data.abs().max()):.2e} m s⁻¹, NaN: {nan}")
    return model, dt


if __name__ == "__main__":
    main()
