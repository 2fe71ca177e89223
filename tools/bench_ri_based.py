#!/usr/bin/env python3
"""RiBasedVerticalDiffusivity at config 5's grid (1024 x 1024 x 128, regular z), one GPU, one process:

  tools/bench_ri_based.py [Nx] [Nz] [steps]

1. kernel times (device events around repeated launches after a warm-up launch), each with its achieved bytes/s against the kernel's own
   minimum traffic per cell, the CAVD diffusivity kernel alternating with them in the same loop:
     one launch, no filter     72 B: u, v, T, S read, κᶜ and κᵘ read and written, Ri written
     Ri alone                  40 B: u, v, T, S read, Ri written
     diffusivities from Ri     56 B: T, S, Ri read (the 3 x 3 stencil of the filter from the same lines), κᶜ and κᵘ read and written
     filtered pass             96 B = 40 + 56, plus the halo fill of Ri between the two launches
     CAVD diffusivities        32 B: T and S read, κᶜ and κᵘ written
2. step times of the config-5 model (bench.py --workload config5: VectorInvariant, WENO tracers, SplitExplicitFreeSurface(substeps = 30),
   FPlane, SeawaterBuoyancy, QAB2) with RiBasedVerticalDiffusivity (vertically implicit; unfiltered and filtered) next to
   ConvectiveAdjustmentVerticalDiffusivity in the same call.  The surface is cooled and the top fifth of the column starts unstable.
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
ocn.set_math_mode(ocn.MATH_FAST)  # (bench.py's default; the kernels of these closures have one strict build)
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


ri_based = lambda **kw: ocn.RiBasedVerticalDiffusivity(warning=False, **kw)
cavd = lambda: ocn.ConvectiveAdjustmentVerticalDiffusivity(convective_κz=1.0, background_κz=1e-3, convective_νz=0.1, background_νz=1e-2)
m = model(ri_based())
d = m.diffusivity_fields
kc, ku, ri = d["kappa_c"], d["kappa_u"], d["Ri"]
r = ri.interior_view()[:Nz]
print(f"grid {Nx}x{Nx}x{Nz}, dt = {dt:.4g} s; Ri: {100 * float((r == 0).double().mean()):.1f} % zero, {100 * float(torch.isinf(r).double().mean()):.1f} % "
      f"infinite; max κᶜ {float(kc.interior_view().max()):.3g}", flush=True)
# ---- kernels
nh = m._nh
terms = C.byref(nh._terms)
plain, filtered = ri_based().c_struct(), ri_based(horizontal_Ri_filter=ocn.FivePointHorizontalFilter()).c_struct()
cacl = cavd().c_struct()
tops = m._closure.top_conditions(nh)
fused_call = lambda: L.call("ocn_compute_ri_based_diffusivities_fused", g.cref, terms, C.byref(plain), *tops, m.u.ptr, m.v.ptr, ri.ptr, kc.ptr, ku.ptr, 0)
ri_call = lambda: L.call("ocn_compute_ri_number", g.cref, terms, m.u.ptr, m.v.ptr, ri.ptr, 0)
dif_call = lambda cl: (lambda: L.call("ocn_compute_ri_based_diffusivities", g.cref, terms, C.byref(cl), *tops, ri.ptr, kc.ptr, ku.ptr, 0))
fill_call = lambda: ocn.fill_halo_regions((ri,), fill_boundary_normal_velocities=False)


def filtered_pass():
    ri_call(); fill_call(); dif_call(filtered)()


work_c, work_u = torch.zeros_like(kc.data), torch.zeros_like(ku.data)
cavd_call = lambda: L.call("ocn_compute_convective_adjustment_diffusivities", g.cref, terms, C.byref(cacl), work_c.data_ptr(), work_u.data_ptr(), 0)
for rep in range(2):  # all of them alternate in the same call
    a, b, c, e, f, h, k = (device_ms(x) for x in (fused_call, ri_call, dif_call(plain), dif_call(filtered), fill_call, filtered_pass, cavd_call))
    print(f"[{rep}] one launch, no filter: {a:.3f} ms, {72 * cells / a / 1e9:.3f} TB/s of its 72 B/cell | Ri alone: {b:.3f} ms, "
          f"{40 * cells / b / 1e9:.3f} TB/s of 40 B | diffusivities from Ri: {c:.3f} ms, {56 * cells / c / 1e9:.3f} TB/s of 56 B; filtered {e:.3f} ms, "
          f"{56 * cells / e / 1e9:.3f} TB/s | halo fill of Ri: {f:.3f} ms | filtered pass (3 launches): {h:.3f} ms, {96 * cells / h / 1e9:.3f} TB/s of "
          f"96 B | CAVD diffusivities: {k:.3f} ms, {32 * cells / k / 1e9:.3f} TB/s of 32 B | one launch / CAVD = {a / k:.2f} (bytes 72 / 32 = 2.25)",
          flush=True)
del m, d, kc, ku, ri, r, nh, work_c, work_u, tops
torch.cuda.empty_cache()


# ---- steps (each model built, warmed up and timed on its own; the first model a process times carries one-time costs: it is timed again last)
def timed(label, closure, fused=None):
    mm = model(closure, fused)
    ms, ok = step_ms(mm)
    k = mm.diffusivity_fields["kappa_c"].interior_view()[:Nz]
    print(f"config-5 step, {label}: {ms:.2f} ms/step (finite={ok}, fused={mm.fused}, mean κᶜ {float(k.mean()):.3g}, max {float(k.max()):.3g})", flush=True)
    del mm
    torch.cuda.empty_cache()


timed("RiBasedVerticalDiffusivity, FIRST model of the process (one-time costs included: not the figure to quote)", ri_based())
timed("ConvectiveAdjustmentVerticalDiffusivity (vertically implicit)", cavd())
timed("RiBasedVerticalDiffusivity (vertically implicit)", ri_based())
timed("RiBasedVerticalDiffusivity, FivePointHorizontalFilter", ri_based(horizontal_Ri_filter=ocn.FivePointHorizontalFilter()))
timed("ConvectiveAdjustmentVerticalDiffusivity (vertically implicit), again", cavd())
