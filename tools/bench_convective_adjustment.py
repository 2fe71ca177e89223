#!/usr/bin/env python3
"""ConvectiveAdjustmentVerticalDiffusivity at config 5's grid (1024 x 1024 x 128, regular z), one GPU, one process:

  tools/bench_convective_adjustment.py [Nx] [Nz] [steps]

1. kernel times (device events around repeated launches after a warm-up launch), each with its achieved bytes/s against the kernel's own
   minimum traffic per cell:
     diffusivities             32 B: T and S read, κᶜ and κᵘ written
     field-valued step         24 B per distinct matrix (κ read, the multipliers t written and read) + 32 B per field (read and written in
                               each sweep): u 56, v 56, T and S together 88 -- 200 B for the four; a single tracer 56
     constant-κ step           32 B per field (ocn_implicit_vertical_diffusion_step over the same four fields: 128 B), alternating with the
                               field-valued one in the same loop
     closure term, explicit    120 B: u, v, κᵘ read, Gu, Gv read and written (56); per tracer c and κᶜ read, Gc read and written (32)
     closure term, boundary    the same per cell of the planes k = 1 and k = Nz, the only ones launched
2. step times of the config-5 model (bench.py --workload config5: VectorInvariant, WENO tracers, SplitExplicitFreeSurface(substeps = 30),
   FPlane, SeawaterBuoyancy, QAB2) with ConvectiveAdjustmentVerticalDiffusivity (vertically implicit), with
   ScalarDiffusivity(VerticallyImplicitTimeDiscretization()), with the explicit ScalarDiffusivity at fused = False, and with the latter's
   default fused step.  The surface is cooled and the top fifth of the column starts unstable, so both coefficient values are in play.
Prints one line per figure."""
import ctypes as C
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import oceananigans_jl_amd as ocn

Nx = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
Nz = int(sys.argv[2]) if len(sys.argv) > 2 else 128
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 6
H, Lx, substeps = 1000.0, 1.0e6 * Nx / 1024.0, 30
ocn.set_math_mode(ocn.MATH_FAST)  # (bench.py's default; the kernels of this closure have one strict build)
g = ocn.RectilinearGrid(ocn.GPU(), size=(Nx, Nx, Nz), x=(0, Lx), y=(0, Lx), z=(-H, 0.0), topology=("Periodic", "Periodic", "Bounded"), halo=(3, 3, 3))
cells = Nx * Nx * Nz
L = ocn._lib
dt = 2.0 * g.dx / np.sqrt(9.80665 * H)  # bench.py's config-5 step: baroclinic gravity-wave CFL 2


def device_ms(call, repeats=10):
    call(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(repeats):
        call()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / repeats


def model(closure, fused=None):
    bcs = {"T": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(200.0 / (1026.0 * 3991.0)))}  # 200 W m⁻² of cooling
    m = ocn.HydrostaticFreeSurfaceModel(g, momentum_advection=ocn.VectorInvariant(), tracer_advection=ocn.WENO(), tracers=("T", "S"),
                                        free_surface=ocn.SplitExplicitFreeSurface(substeps=substeps), coriolis=ocn.FPlane(f=1e-4), closure=closure,
                                        buoyancy=ocn.SeawaterBuoyancy(equation_of_state=ocn.LinearEquationOfState(2e-4, 8e-4)),
                                        boundary_conditions=bcs, fused=fused)
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    zc = torch.linspace(-H + H / (2 * Nz), -H / (2 * Nz), Nz, device="cuda", dtype=torch.float64)
    profile = 20 + 0.01 * zc - 0.02 * torch.clamp(zc + 0.2 * H, min=0.0)  # stable below -H / 5, unstable above
    T = m.field("T").interior_view()
    T.copy_(profile[:, None, None] + 1e-4 * torch.rand(T.shape, generator=gen, device="cuda", dtype=torch.float64))
    m.field("S").interior_view().fill_(35.0)
    for f in (m.u, m.v):
        iv = f.interior_view(); iv.copy_(1e-2 * (torch.rand(iv.shape, generator=gen, device="cuda", dtype=torch.float64) * 2 - 1))
    m.update_state(compute_tendencies=False)
    return m


def step_ms(m):
    for _ in range(2):
        m.time_step(dt)
    m.flush_tendencies(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        m.time_step(dt)
    m.flush_tendencies(); torch.cuda.synchronize()
    ok = bool(all(torch.isfinite(f.data).all() for f in (m.u, m.v) + tuple(m.tracers)))
    return (time.perf_counter() - t0) / steps * 1e3, ok


cavd = lambda: ocn.ConvectiveAdjustmentVerticalDiffusivity(convective_κz=1.0, background_κz=1e-3, convective_νz=0.1, background_νz=1e-2)
m = model(cavd())
d = m.diffusivity_fields
kc, ku = d["kappa_c"], d["kappa_u"]
unstable = float((kc.interior_view()[:Nz] == 1.0).double().mean())
print(f"grid {Nx}x{Nx}x{Nz}, dt = {dt:.4g} s (diffusion number dt convective_κz / Δz² = {dt * 1.0 / g.dz ** 2:.3g}), {100 * unstable:.1f} % of the faces unstable", flush=True)
# ---- kernels
nh = m._nh
cl = m._closure.struct
ms = device_ms(lambda: L.call("ocn_compute_convective_adjustment_diffusivities", g.cref, C.byref(nh._terms), C.byref(cl), kc.ptr, ku.ptr, 0))
print(f"diffusivities: {ms:.3f} ms per launch, {32 * cells / ms / 1e9:.3f} TB/s of its 32 B/cell", flush=True)
fields = [m.u, m.v] + list(m.tracers)
work = [torch.clone(f.data) for f in fields]  # the solves run on copies: repeated in-place solves drive the fields to their column means
tscr = m._closure.ivd_scratch
locs = [f.loc for f in fields]


def fields_step(idx):
    kappas = [ku.ptr if locs[q] != 0 else kc.ptr for q in idx]
    scratch = [tscr[min(q, 2)].data_ptr() for q in idx]
    n = len(idx)
    return lambda: L.call("ocn_implicit_vertical_diffusion_step_fields", g.cref, n, L.ptr_array([work[q].data_ptr() for q in idx]),
                          L.i32_array([locs[q] for q in idx]), L.ptr_array(kappas), L.ptr_array(scratch), dt, 0)


def constant_step(idx):
    n = len(idx)
    return lambda: L.call("ocn_implicit_vertical_diffusion_step", g.cref, n, L.ptr_array([work[q].data_ptr() for q in idx]),
                          L.i32_array([locs[q] for q in idx]), (C.c_double * n)(*([1e-2] * n)), dt, 0)


new4, old4 = fields_step([0, 1, 2, 3]), constant_step([0, 1, 2, 3])
for rep in range(2):  # the two alternate in the same call
    a, b = device_ms(new4), device_ms(old4)
    print(f"[{rep}] field-valued step, u v T S: {a:.3f} ms per call (2 launches), {200 * cells / a / 1e9:.3f} TB/s of its 200 B/cell | "
          f"constant-κ step, same four fields: {b:.3f} ms per launch, {128 * cells / b / 1e9:.3f} TB/s of its 128 B/cell", flush=True)
for label, idx, nbytes in (("u alone", [0], 56), ("v alone", [1], 56), ("T alone", [2], 56), ("T and S together", [2, 3], 88)):
    a = device_ms(fields_step(idx))
    print(f"field-valued step, {label}: {a:.3f} ms per launch, {nbytes * cells / a / 1e9:.3f} TB/s of its {nbytes} B/cell", flush=True)
b = device_ms(constant_step([2]))
print(f"constant-κ step, T alone: {b:.3f} ms per launch, {32 * cells / b / 1e9:.3f} TB/s of its 32 B/cell", flush=True)
Gs = [torch.zeros_like(f.data) for f in fields]
for boundary_only, label, ncells in ((0, "explicit", cells), (1, "boundary_only (planes k = 1 and k = Nz)", 2 * Nx * Nx)):
    call = lambda: L.call("ocn_add_vertical_diffusivity_fluxes", g.cref, ku.ptr, m.u.ptr, m.v.ptr, Gs[0].data_ptr(), Gs[1].data_ptr(), 2,
                          L.ptr_array([kc.ptr, kc.ptr]), L.ptr_array([c.ptr for c in m.tracers]), L.ptr_array([G.data_ptr() for G in Gs[2:]]),
                          boundary_only, None, 0)
    ms = device_ms(call)
    print(f"closure term, {label}, momentum + 2 tracers: {ms:.4f} ms per call, {120 * ncells / ms / 1e9:.3f} TB/s of its 120 B/cell", flush=True)
del work, Gs, m, d, kc, ku, nh, tscr
torch.cuda.empty_cache()


# ---- steps (each model built, warmed up and timed on its own; the first model a process times carries one-time costs: it is timed again last)
def timed(label, closure, fused=None):
    mm = model(closure, fused)
    ms, ok = step_ms(mm)
    extra = ""
    if mm.diffusivity_fields is not None:
        k = mm.diffusivity_fields["kappa_c"].interior_view()[:Nz]
        extra = f", {100 * float((k == 1.0).double().mean()):.1f} % of the faces unstable at the end"
    print(f"config-5 step, {label}: {ms:.2f} ms/step (finite={ok}, fused={mm.fused}{extra})", flush=True)
    del mm
    torch.cuda.empty_cache()


VI = ocn.VerticallyImplicitTimeDiscretization
timed("ConvectiveAdjustmentVerticalDiffusivity, FIRST model of the process (one-time costs included: not the figure to quote)", cavd())
timed("ScalarDiffusivity(VerticallyImplicitTimeDiscretization(), ν=1e-2, κ=1e-3)", ocn.ScalarDiffusivity(VI(), ν=1e-2, κ=1e-3))
timed("explicit ScalarDiffusivity(ν=1e-2, κ=1e-3), fused = False", ocn.ScalarDiffusivity(ν=1e-2, κ=1e-3), fused=False)
timed("explicit ScalarDiffusivity(ν=1e-2, κ=1e-3), default (fused)", ocn.ScalarDiffusivity(ν=1e-2, κ=1e-3))
timed("ConvectiveAdjustmentVerticalDiffusivity (vertically implicit)", cavd())
