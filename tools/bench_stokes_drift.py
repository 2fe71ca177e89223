#!/usr/bin/env python3
"""Cost of stokes_drift = UniformStokesDrift on config 4's grid and term set (tools/bench_config4.py with physics = 2: 512 x 512 x 256
(Periodic, Periodic, Bounded), stretched z, WENO5, RK3, T / S SeawaterBuoyancy, FPlane, AnisotropicMinimumDissipation, flux conditions):
two models with the same initial state, one with a steady UniformStokesDrift(dz_us=...), timed alternately in the same process.

  tools/bench_stokes_drift.py [Nx] [Nz] [steps] [rounds] [only: both|off|on]
Prints ms/step of every round for both models."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import oceananigans_jl_amd as ocn

Nx = int(sys.argv[1]) if len(sys.argv) > 1 else 512
Nz = int(sys.argv[2]) if len(sys.argv) > 2 else 256
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 3
only = sys.argv[5] if len(sys.argv) > 5 else "both"
Lz, refinement, stretching = 32.0, 1.2, 12.0
h = lambda k: (k - 1) / Nz
zeta0 = lambda k: 1 + (h(k) - 1) / refinement
Sigma = lambda k: (1 - np.exp(-stretching * h(k))) / (1 - np.exp(-stretching))
z_faces = np.array([Lz * (zeta0(k) * Sigma(k) - 1) for k in range(1, Nz + 2)])
ocn.set_math_mode(ocn.MATH_FAST)
Q, rho, cp, dTdz = 200.0, 1026.0, 3991.0, 0.01
taux = -1.225 / rho * 2.5e-3 * 10 * 10


def build(stokes):
    g = ocn.RectilinearGrid(ocn.GPU(), size=(Nx, Nx, Nz), x=(0, 64), y=(0, 64), z=z_faces, topology=("Periodic", "Periodic", "Bounded"), halo=(3, 3, 3))
    bcs = {"u": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(taux)),
           "T": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(Q / (rho * cp)), bottom=ocn.GradientBoundaryCondition(dTdz)),
           "S": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(0.0, coeff=-1e-3 / 3600))}
    sd = ocn.UniformStokesDrift(dz_us=lambda z, t: 0.0681 / 4.77 * np.exp(z / 4.77), steady=True) if stokes else None
    m = ocn.NonhydrostaticModel(g, advection=ocn.WENO(), tracers=("T", "S"), coriolis=ocn.FPlane(f=1e-4), closure=ocn.AnisotropicMinimumDissipation(),
                                buoyancy=ocn.SeawaterBuoyancy(equation_of_state=ocn.LinearEquationOfState(2e-4, 8e-4)), boundary_conditions=bcs,
                                stokes_drift=sd)
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    zc = 0.5 * (z_faces[1:] + z_faces[:-1])
    T = m.field("T").interior_view()
    T.copy_(torch.from_numpy(20 + dTdz * zc)[:, None, None].to("cuda") + 1e-6 * torch.rand(T.shape, generator=gen, device="cuda", dtype=torch.float64))
    m.field("S").interior_view().fill_(35.0)
    for f in m.velocities:
        iv = f.interior_view(); iv.copy_(1e-2 * (torch.rand(iv.shape, generator=gen, device="cuda", dtype=torch.float64) * 2 - 1))
    ocn.set(m)
    return m


models = {name: build(name == "on") for name in (("off", "on") if only == "both" else (only,))}
m0 = next(iter(models.values()))
umax = float(torch.stack([f.interior_view().abs().max() for f in m0.velocities]).max())
dt = 0.1 * min(m0.grid.dx, float(np.diff(z_faces).min())) / umax
for m in models.values():
    for _ in range(2): ocn.time_step(m, dt)
    ocn.flush_tendencies(m)
torch.cuda.synchronize()
for r in range(rounds):
    for name, m in models.items():
        t0 = time.perf_counter()
        for _ in range(steps): ocn.time_step(m, dt)
        ocn.flush_tendencies(m); torch.cuda.synchronize()
        print(f"round {r + 1} stokes_drift {name}: {(time.perf_counter() - t0) / steps * 1e3:.3f} ms/step", flush=True)
print("finite:", all(bool(torch.isfinite(f.data).all()) for m in models.values() for f in m.prognostic_fields()))
