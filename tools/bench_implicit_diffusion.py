#!/usr/bin/env python3
"""ScalarDiffusivity(VerticallyImplicitTimeDiscretization(), ...) at config 4's grid (512 x 512 x 256, stretched z):

  tools/bench_implicit_diffusion.py [Nx] [Nz] [steps]

1. kernel times (device events around repeated launches): ONE implicit step over u, v, w, T, S, and the explicit-part kernels (momentum + two
   tracers), each with its achieved bytes/s against the kernel's own minimum traffic:
     implicit step    32 B per cell and field: the forward sweep reads and writes the field, the backward sweep reads and writes it again
     explicit part    72 B per cell for momentum (u, v, w read; Gu, Gv, Gw read and written), 24 B per cell and tracer (c read; Gc read and written)
2. step times of the config-4-like model (tools/bench_config4.py physics = 1: SeawaterBuoyancy, T and S, FPlane, wind stress, heat flux)
   with the vertically implicit closure and with the explicit one (whose kernels and host path this feature does not touch), RK3, same Δt.
Prints one line per figure."""
import ctypes as C
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import oceananigans_jl_amd as ocn

Nx = int(sys.argv[1]) if len(sys.argv) > 1 else 512
Nz = int(sys.argv[2]) if len(sys.argv) > 2 else 256
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
Lz, refinement, stretching = 32.0, 1.2, 12.0
h = lambda k: (k - 1) / Nz
zeta0 = lambda k: 1 + (h(k) - 1) / refinement
Sigma = lambda k: (1 - np.exp(-stretching * h(k))) / (1 - np.exp(-stretching))
z_faces = np.array([Lz * (zeta0(k) * Sigma(k) - 1) for k in range(1, Nz + 2)])
ocn.set_math_mode(ocn.MATH_FAST)
g = ocn.RectilinearGrid(ocn.GPU(), size=(Nx, Nx, Nz), x=(0, 64), y=(0, 64), z=z_faces, topology=("Periodic", "Periodic", "Bounded"), halo=(3, 3, 3))
cells = Nx * Nx * Nz
L = ocn._lib


def device_ms(call, repeats=10):
    call(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(repeats):
        call()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / repeats


def model(closure):
    Q, rho, cp, dTdz = 200.0, 1026.0, 3991.0, 0.01
    taux = -1.225 / rho * 2.5e-3 * 10 * 10
    bcs = {"u": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(taux)),
           "T": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(Q / (rho * cp)), bottom=ocn.GradientBoundaryCondition(dTdz)),
           "S": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(0.0, coeff=-1e-3 / 3600))}
    m = ocn.NonhydrostaticModel(g, advection=ocn.WENO(), tracers=("T", "S"), coriolis=ocn.FPlane(f=1e-4), closure=closure,
                                buoyancy=ocn.SeawaterBuoyancy(equation_of_state=ocn.LinearEquationOfState(2e-4, 8e-4)), boundary_conditions=bcs)
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    zc = 0.5 * (z_faces[1:] + z_faces[:-1])
    T = m.field("T").interior_view()
    T.copy_(torch.from_numpy(20 + dTdz * zc)[:, None, None].to("cuda") + 1e-6 * torch.rand(T.shape, generator=gen, device="cuda", dtype=torch.float64))
    m.field("S").interior_view().fill_(35.0)
    for f in m.velocities:
        iv = f.interior_view(); iv.copy_(1e-2 * (torch.rand(iv.shape, generator=gen, device="cuda", dtype=torch.float64) * 2 - 1))
    ocn.set(m)
    return m


def step_ms(m, dt):
    for _ in range(2):
        ocn.time_step(m, dt)
    ocn.flush_tendencies(m); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        ocn.time_step(m, dt)
    ocn.flush_tendencies(m); torch.cuda.synchronize()
    ok = bool(all(torch.isfinite(f.data).all() for f in m.prognostic_fields()))
    return (time.perf_counter() - t0) / steps * 1e3, ok


nu = kappa = 1e-4
m = model(ocn.ScalarDiffusivity(ocn.VerticallyImplicitTimeDiscretization(), ν=nu, κ=kappa))
umax = float(torch.stack([f.interior_view().abs().max() for f in m.velocities]).max())
dzmin = float(np.diff(z_faces).min())
dt = 0.1 * min(g.dx, dzmin) / umax
# ---- kernels
prog = m.prognostic_fields()
scratch = [torch.clone(f.data) for f in prog]  # the solves run on copies: repeated in-place solves would drive the fields to their column means
ptrs = L.ptr_array([s.data_ptr() for s in scratch])
locs = L.i32_array([f.loc for f in prog])
kap = (C.c_double * len(prog))(*([nu] * 3 + [kappa] * 2))
ms = device_ms(lambda: L.call("ocn_implicit_vertical_diffusion_step", g.cref, len(prog), ptrs, locs, kap, dt, 0))
print(f"implicit step, {len(prog)} fields {Nx}x{Nx}x{Nz}: {ms:.3f} ms per launch, {32 * cells * len(prog) / ms / 1e9:.3f} TB/s of its 32 B/cell/field "
      f"(diffusion number {dt * kappa / dzmin ** 2:.3g})", flush=True)
Gs = [torch.zeros_like(f.data) for f in prog]
call = lambda: L.call("ocn_add_vertically_implicit_explicit_fluxes", g.cref, nu, m.u.ptr, m.v.ptr, m.w.ptr, Gs[0].data_ptr(), Gs[1].data_ptr(),
                      Gs[2].data_ptr(), 2, (C.c_double * 2)(kappa, kappa), L.ptr_array([c.ptr for c in m.tracers]),
                      L.ptr_array([G.data_ptr() for G in Gs[3:]]), None, 0)
ms = device_ms(call)
print(f"explicit part, momentum + 2 tracers: {ms:.3f} ms per call (3 launches), {(72 + 2 * 24) * cells / ms / 1e9:.3f} TB/s of its 120 B/cell", flush=True)
call_m = lambda: L.call("ocn_add_vertically_implicit_explicit_fluxes", g.cref, nu, m.u.ptr, m.v.ptr, m.w.ptr, Gs[0].data_ptr(), Gs[1].data_ptr(),
                        Gs[2].data_ptr(), 0, None, None, None, None, 0)
ms = device_ms(call_m)
print(f"explicit part, momentum alone: {ms:.3f} ms per launch, {72 * cells / ms / 1e9:.3f} TB/s of its 72 B/cell", flush=True)
del scratch, Gs
# ---- steps (each model built, warmed up and timed on its own).  The first model a process times runs about 20 ms per step slower than the
# same model timed later (one-time costs beyond the two warm-up steps; the kernel trace of the step shows no such time), so the implicit
# model is timed first AND last: quote the last
del m
torch.cuda.empty_cache()


def timed(label, closure, fuse="1"):
    os.environ["OCN_FUSE_GENERAL"] = fuse
    mm = model(closure)
    ms, ok = step_ms(mm, dt)
    print(f"config-4-like step, {label}: {ms:.2f} ms/step (finite={ok}, fused stage boundaries={mm.fuse_stage_boundaries})", flush=True)
    del mm
    torch.cuda.empty_cache()


implicit = lambda: ocn.ScalarDiffusivity(ocn.VerticallyImplicitTimeDiscretization(), ν=nu, κ=kappa)
timed("vertically implicit closure, FIRST model of the process (one-time costs included: not the figure to quote)", implicit())
timed("explicit closure", ocn.ScalarDiffusivity(ν=nu, κ=kappa))
timed("explicit closure, OCN_FUSE_GENERAL=0", ocn.ScalarDiffusivity(ν=nu, κ=kappa), fuse="0")
timed("vertically implicit closure", implicit())
