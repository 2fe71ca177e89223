#!/usr/bin/env python3
"""IsopycnalSkewSymmetricDiffusivity at config 5's grid (1024 x 1024 x 128, regular z, T and S) and at 256 x 256 x 64, one GPU, one process:

  tools/bench_isopycnal.py [Nx] [Nz] [steps]        (no arguments: both grids)

1. kernel times (a device-event pair around every launch after a warm-up; the median of the repeats), each with its achieved bytes/s
   against the algorithmic traffic per cell:
     diffusivity launch (ϵ_R₃₃, κz, uₑ, vₑ, wₑ)    56 B: T and S read once, five arrays written
     ... without eddy velocities                  32 B
     total velocities                             72 B: three sums of two arrays
     flux divergence, T and S (one launch)        48 B: T and S read once, two tendencies read and written
     flux divergence, one tracer                  32 B
   and, as the yardstick for a 3-D stencil of this size, HorizontalScalarBiharmonicDiffusivity's tracer launch (24 B) on the same arrays in
   the same process, alternating with the new launches.
2. step times of the config-5 model (bench.py --workload config5: VectorInvariant, WENO tracers, SplitExplicitFreeSurface(substeps = 30),
   FPlane, SeawaterBuoyancy, QAB2) at fused = False: without closure, with the closure, and with the pair (biharmonic, isopycnal).
Prints one line per figure."""
import os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as C
import numpy as np, torch
import oceananigans_jl_amd as ocn

steps = int(sys.argv[3]) if len(sys.argv) > 3 else 6
GRIDS = [(int(sys.argv[1]), int(sys.argv[2]) if len(sys.argv) > 2 else 128)] if len(sys.argv) > 1 else [(1024, 128), (256, 64)]
H, substeps = 1000.0, 30
KAPPA_SKEW = KAPPA_SYMMETRIC = 1.0e3
ocn.set_math_mode(ocn.MATH_FAST)  # (bench.py's default; the kernels of this closure have one strict build)
L = ocn._lib


def device_ms(call, repeats=11):
    call(); torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record(); torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times)


def run(Nx, Nz):
    Lx = 1.0e6 * Nx / 1024.0
    g = ocn.RectilinearGrid(ocn.GPU(), size=(Nx, Nx, Nz), x=(0, Lx), y=(0, Lx), z=(-H, 0.0), topology=("Periodic", "Periodic", "Bounded"), halo=(3, 3, 3))
    cells = Nx * Nx * Nz
    dt = 2.0 * g.dx / np.sqrt(9.80665 * H)  # bench.py's config-5 step: baroclinic gravity-wave CFL 2
    NU = KAPPA = 0.02 / (dt * (8 / g.dx ** 2) ** 2)

    def model(closure):
        bcs = {"T": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(200.0 / (1026.0 * 3991.0)))}  # 200 W m⁻² of cooling
        m = ocn.HydrostaticFreeSurfaceModel(g, momentum_advection=ocn.VectorInvariant(), tracer_advection=ocn.WENO(), tracers=("T", "S"),
                                            free_surface=ocn.SplitExplicitFreeSurface(substeps=substeps), coriolis=ocn.FPlane(f=1e-4), closure=closure,
                                            buoyancy=ocn.SeawaterBuoyancy(equation_of_state=ocn.LinearEquationOfState(2e-4, 8e-4)),
                                            boundary_conditions=bcs, fused=False)
        gen = torch.Generator(device="cuda"); gen.manual_seed(1)
        zc = torch.linspace(-H + H / (2 * Nz), -H / (2 * Nz), Nz, device="cuda", dtype=torch.float64)
        xc = torch.linspace(0.5 / Nx, 1 - 0.5 / Nx, Nx, device="cuda", dtype=torch.float64)
        profile = 20 + 0.01 * zc - 0.02 * torch.clamp(zc + 0.2 * H, min=0.0)  # stable below -H / 5, unstable above
        front = 2.0 * torch.cos(2 * np.pi * xc)  # slopes of up to 2π 2 K / Lx / 0.01 K/m: about 1e-3 at Nx = 1024, tapered at 256
        T = m.field("T").interior_view()
        T.copy_(profile[:, None, None] + front[None, None, :] + 1e-3 * torch.rand(T.shape, generator=gen, device="cuda", dtype=torch.float64))
        m.field("S").interior_view().fill_(35.0)
        for f in (m.u, m.v):
            iv = f.interior_view(); iv.copy_(1e-2 * (torch.rand(iv.shape, generator=gen, device="cuda", dtype=torch.float64) * 2 - 1))
        m.update_state(compute_tendencies=False)
        return m

    def step_ms(m):
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
        return statistics.median(times), ok

    issd = lambda: ocn.IsopycnalSkewSymmetricDiffusivity(κ_skew=KAPPA_SKEW, κ_symmetric=KAPPA_SYMMETRIC)
    bih = lambda: ocn.HorizontalScalarBiharmonicDiffusivity(ν=NU, κ=KAPPA)
    print(f"grid {Nx}x{Nx}x{Nz}, dt = {dt:.4g} s, κ_skew = κ_symmetric = {KAPPA_SKEW:g} m²/s", flush=True)
    # ---- kernels, on the arrays of a model with the closure
    m = model(issd())
    nh, cl, d = m._nh, m._closure, m.diffusivity_fields
    terms, struct = C.byref(nh._terms), C.byref(cl.struct)
    kz = list(cl.kz.values())
    pa = L.ptr_array
    Gs = [torch.zeros_like(c.data) for c in m.tracers]
    two = (C.c_double * 2)(KAPPA_SYMMETRIC, KAPPA_SYMMETRIC)
    zero2 = (C.c_double * 2)(0.0, 0.0)
    eddy = [d[n].ptr for n in "uvw"]
    calls = {
        "diffusivity launch (eps_R33, kz, eddy velocities)": (56, lambda: L.call(
            "ocn_compute_isopycnal_diffusivities", g.cref, terms, struct, KAPPA_SKEW, d["eps_R33"].ptr, *eddy, 1, (C.c_double * 1)(KAPPA_SYMMETRIC),
            pa([kz[0].ptr]), 0)),
        "diffusivity launch without eddy velocities": (32, lambda: L.call(
            "ocn_compute_isopycnal_diffusivities", g.cref, terms, struct, 0.0, d["eps_R33"].ptr, None, None, None, 1, (C.c_double * 1)(KAPPA_SYMMETRIC),
            pa([kz[0].ptr]), 0)),
        "total velocities (one launch)": (72, lambda: L.call(
            "ocn_sum_velocities", g.cref, pa([m.u.ptr, m.v.ptr, m.w.ptr]), pa(eddy), pa([f.ptr for f in cl.total]), 0)),
        "flux divergence, T and S (one launch)": (48, lambda: L.call(
            "ocn_add_isopycnal_fluxes", g.cref, terms, struct, 2, two, zero2, pa([c.ptr for c in m.tracers]), pa([G.data_ptr() for G in Gs]), 0)),
        "flux divergence, one tracer": (32, lambda: L.call(
            "ocn_add_isopycnal_fluxes", g.cref, terms, struct, 1, two, zero2, pa([m.tracers[0].ptr]), pa([Gs[0].data_ptr()]), 0)),
        "yardstick: biharmonic term, one tracer": (24, lambda: L.call(
            "ocn_add_biharmonic_fluxes", g.cref, 0.0, None, None, None, None, 1, (C.c_double * 1)(KAPPA), pa([m.tracers[0].ptr]),
            pa([Gs[0].data_ptr()]), None, None, None, 0)),
    }
    for rep in range(2):  # the new launches and the yardstick alternate in the same process
        for label, (nbytes, call) in calls.items():
            ms = device_ms(call)
            print(f"[{rep}] {label}: {ms:.3f} ms, {nbytes * cells / ms / 1e9:.3f} TB/s of its {nbytes} B/cell", flush=True)
    del Gs, m, nh, cl, d, kz, calls, eddy
    torch.cuda.empty_cache()

    # ---- steps (each model built, warmed up and timed on its own; the first model a process times carries one-time costs)
    def timed(label, closure):
        mm = model(closure)
        ms, ok = step_ms(mm)
        print(f"config-5 step at {Nx}x{Nx}x{Nz}, fused = False, {label}: {ms:.2f} ms/step (median of {steps}, finite={ok})", flush=True)
        del mm
        torch.cuda.empty_cache()

    timed("no closure, FIRST model of the process (one-time costs included: not the figure to quote)", None)
    for rep in range(2):
        timed(f"[{rep}] no closure", None)
        timed(f"[{rep}] IsopycnalSkewSymmetricDiffusivity", issd())
        timed(f"[{rep}] (HorizontalScalarBiharmonicDiffusivity, IsopycnalSkewSymmetricDiffusivity)", (bih(), issd()))


for Nx, Nz in GRIDS:
    run(Nx, Nz)
