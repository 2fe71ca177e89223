#!/usr/bin/env python3
"""WENOVectorInvariant(order=5) at config 5's grid (1024 x 1024 x 128, regular z), one GPU, one process:

  tools/bench_vector_invariant_weno.py [Nx] [Nz] [steps]

1. kernel times (a device-event pair around every launch after a warm-up; the median, the minimum and the maximum of the repeats), on the
   same arrays in the same process, alternating:
     ocn_compute_vector_invariant_weno_momentum_tendencies   the new launch: WENO(order=5) vorticity (VelocityStencil), divergence / vertical
                                                              and kinetic-energy-gradient schemes; also the other scheme combinations
     yardstick 1: ocn_compute_vector_invariant_momentum_tendencies   the default VectorInvariant() launch (second order, no reconstruction)
     yardstick 2: ocn_compute_momentum_tendencies_terms, strict       the flux-form WENO(order=5) momentum launch (Gu, Gv, Gw): 9 biased
                                                              reconstructions for its three tendencies, 6 of them for Gu and Gv, against
                                                              8 here plus the smoothness measured on other quantities
2. step times of the config-5 model (bench.py --workload config5: WENO tracers, SplitExplicitFreeSurface(substeps = 30), FPlane,
   SeawaterBuoyancy, QAB2) at fused = False with momentum_advection = VectorInvariant() and = WENOVectorInvariant(order=5).
Prints one line per figure."""
import os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as C
import numpy as np, torch
import oceananigans_jl_amd as ocn

Nx = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
Nz = int(sys.argv[2]) if len(sys.argv) > 2 else 128
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 6
H, Lx, substeps = 1000.0, 1.0e6 * Nx / 1024.0, 30
P, B = "Periodic", "Bounded"
L = ocn._lib
cells = Nx * Nx * Nz


def grid(mode):
    g = ocn.RectilinearGrid(ocn.GPU(), size=(Nx, Nx, Nz), x=(0, Lx), y=(0, Lx), z=(-H, 0.0), topology=(P, P, B), halo=(4, 4, 3))
    return g.with_math_mode(mode)


def device_ms(call, repeats=11):
    call(); torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record(); torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times), max(times)


# ---- kernels: random u and v of both signs, w from continuity (both vertical biases occur), the same arrays for every launch
gs, gf = grid(ocn.MATH_STRICT), grid(ocn.MATH_FAST)
dt = 2.0 * gs.dx / np.sqrt(9.80665 * H)  # bench.py's config-5 step: baroclinic gravity-wave CFL 2
print(f"grid {Nx}x{Nx}x{Nz}, halo (4, 4, 3), dt = {dt:.4g} s", flush=True)
gen = torch.Generator(device="cuda"); gen.manual_seed(1)
u, v, w = ocn.Field(1, gs), ocn.Field(2, gs), ocn.Field(4, gs)
for f in (u, v):
    f.data.copy_(1e-1 * (torch.rand(f.data.shape, generator=gen, device="cuda", dtype=torch.float64) * 2 - 1))
ocn.fill_halo_regions((u, v), fill_boundary_normal_velocities=False)
L.call("ocn_compute_w_from_continuity", gs.cref, u.ptr, v.ptr, w.ptr, 0)
Gu, Gv, Gw = (torch.zeros_like(f.data) for f in (u, v, w))
flux_form = L.CModelTerms()
flux_form.advection = L.ADVECTION_WENO5
new = lambda flags, g=gs: (lambda: L.call("ocn_compute_vector_invariant_weno_momentum_tendencies", g.cref, flags, u.ptr, v.ptr, w.ptr, Gu.data_ptr(),
                                          Gv.data_ptr(), None, 9.80665, 0))
calls = {
    "new: WENO vorticity (VelocityStencil) + vertical + KE gradient [flags 7]": new(7),
    "yardstick 1: default VectorInvariant() launch": lambda: L.call("ocn_compute_vector_invariant_momentum_tendencies", gs.cref, u.ptr, v.ptr, w.ptr,
                                                                    Gu.data_ptr(), Gv.data_ptr(), None, 9.80665, 0),
    "yardstick 2: flux-form WENO(order=5) momentum launch, strict": lambda: L.call("ocn_compute_momentum_tendencies_terms", gs.cref, C.byref(flux_form),
                                                                                   u.ptr, v.ptr, w.ptr, Gu.data_ptr(), Gv.data_ptr(), Gw.data_ptr(), None, 0),
    "    (flux-form WENO(order=5) momentum launch, fast math)": lambda: L.call("ocn_compute_momentum_tendencies_terms", gf.cref, C.byref(flux_form),
                                                                               u.ptr, v.ptr, w.ptr, Gu.data_ptr(), Gv.data_ptr(), Gw.data_ptr(), None, 0),
    "new: the same with the DefaultStencil [flags 15]": new(15),
    "new: WENO vorticity + vertical, conserving KE gradient [flags 3]": new(3),
    "new: WENO vorticity alone [flags 1]": new(1),
    "new: WENO vertical + KE gradient, conserving vorticity [flags 6]": new(6),
}
medians = {}
for rep in range(2):  # the new launches and the yardsticks alternate in the same process
    for label, call in calls.items():
        med, lo, hi = device_ms(call)
        medians.setdefault(label, []).append(med)
        print(f"[{rep}] {label}: {med:.3f} ms (min {lo:.3f}, max {hi:.3f} of 11), {cells / med / 1e6:.2f} Gcell/s", flush=True)
labels = list(calls)
best = {k: min(x) for k, x in medians.items()}
print(f"ratios (lower median of the two rounds): new / default = {best[labels[0]] / best[labels[1]]:.2f}, "
      f"new / flux-form strict = {best[labels[0]] / best[labels[2]]:.2f}", flush=True)
del u, v, w, Gu, Gv, Gw, calls
torch.cuda.empty_cache()


# ---- steps (each model built, warmed up and timed on its own; the first model a process times carries one-time costs: it is timed again)
def model(advection):
    g = ocn.RectilinearGrid(ocn.GPU(), size=(Nx, Nx, Nz), x=(0, Lx), y=(0, Lx), z=(-H, 0.0), topology=(P, P, B), halo=(4, 4, 3))
    bcs = {"T": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(200.0 / (1026.0 * 3991.0)))}  # 200 W m⁻² of cooling
    m = ocn.HydrostaticFreeSurfaceModel(g, momentum_advection=advection, tracer_advection=ocn.WENO(), tracers=("T", "S"),
                                        free_surface=ocn.SplitExplicitFreeSurface(substeps=substeps), coriolis=ocn.FPlane(f=1e-4),
                                        buoyancy=ocn.SeawaterBuoyancy(equation_of_state=ocn.LinearEquationOfState(2e-4, 8e-4)),
                                        boundary_conditions=bcs, fused=False, math_mode=ocn.MATH_FAST)
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    zc = torch.linspace(-H + H / (2 * Nz), -H / (2 * Nz), Nz, device="cuda", dtype=torch.float64)
    T = m.field("T").interior_view()
    T.copy_((20 + 0.01 * zc)[:, None, None] + 1e-4 * torch.rand(T.shape, generator=gen, device="cuda", dtype=torch.float64))
    m.field("S").interior_view().fill_(35.0)
    for f in (m.u, m.v):
        iv = f.interior_view(); iv.copy_(1e-2 * (torch.rand(iv.shape, generator=gen, device="cuda", dtype=torch.float64) * 2 - 1))
    m.update_state(compute_tendencies=False)
    return m


def timed(label, advection):
    m = model(advection)
    for _ in range(2):
        m.time_step(dt)
    m.flush_tendencies(); torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        t0 = time.perf_counter()
        m.time_step(dt)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    ok = bool(all(torch.isfinite(f.data).all() for f in (m.u, m.v) + tuple(m.tracers)))
    print(f"config-5 step, fused = False, {label}: {statistics.median(times):.2f} ms/step (min {min(times):.2f}, max {max(times):.2f} of {steps}, "
          f"finite={ok})", flush=True)
    del m
    torch.cuda.empty_cache()


timed("VectorInvariant(), FIRST model of the process (one-time costs included: not the figure to quote)", ocn.VectorInvariant())
for rep in range(2):
    timed(f"[{rep}] VectorInvariant()", ocn.VectorInvariant())
    timed(f"[{rep}] WENOVectorInvariant(order=5)", ocn.WENOVectorInvariant(order=5))
