#!/usr/bin/env python3
"""HorizontalScalarBiharmonicDiffusivity at config 5's grid (1024 x 1024 x 128, regular z, two tracers), one GPU, one process:

  tools/bench_biharmonic.py [Nx] [Nz] [steps]

1. kernel times (a device-event pair around every launch after a warm-up; the median of the repeats), each with its achieved bytes/s
   against the algorithmic traffic per cell:
     biharmonic term, momentum      48 B: u and v read once, Gu and Gv read and written
     biharmonic term, one tracer    24 B: c read, Gc read and written
     ... with neg_other arrays      +16 B / +8 B: the tuple route reads minus the other closure's term as well
   and, as the yardstick, ocn_add_vertical_diffusivity_fluxes (explicit) on the same arrays in the same process, alternating with the new
   launches: an existing add-on kernel with the same read-modify-write pattern (56 B momentum, 32 B per tracer).
2. step times of the config-5 model (bench.py --workload config5: VectorInvariant, WENO tracers, SplitExplicitFreeSurface(substeps = 30),
   FPlane, SeawaterBuoyancy, QAB2) at fused = False: without closure, with the biharmonic closure, with
   ConvectiveAdjustmentVerticalDiffusivity, and with the tuple of the two.
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
ocn.set_math_mode(ocn.MATH_FAST)  # (bench.py's default; the kernels of this closure have one strict build)
g = ocn.RectilinearGrid(ocn.GPU(), size=(Nx, Nx, Nz), x=(0, Lx), y=(0, Lx), z=(-H, 0.0), topology=("Periodic", "Periodic", "Bounded"), halo=(3, 3, 3))
cells = Nx * Nx * Nz
L = ocn._lib
dt = 2.0 * g.dx / np.sqrt(9.80665 * H)  # bench.py's config-5 step: baroclinic gravity-wave CFL 2
NU = KAPPA = 0.02 / (dt * (8 / g.dx ** 2) ** 2)  # the grid-scale mode decays by 2 % per step


def device_ms(call, repeats=11):
    call(); torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record(); torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times)


def model(closure):
    bcs = {"T": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(200.0 / (1026.0 * 3991.0)))}  # 200 W m⁻² of cooling
    m = ocn.HydrostaticFreeSurfaceModel(g, momentum_advection=ocn.VectorInvariant(), tracer_advection=ocn.WENO(), tracers=("T", "S"),
                                        free_surface=ocn.SplitExplicitFreeSurface(substeps=substeps), coriolis=ocn.FPlane(f=1e-4), closure=closure,
                                        buoyancy=ocn.SeawaterBuoyancy(equation_of_state=ocn.LinearEquationOfState(2e-4, 8e-4)),
                                        boundary_conditions=bcs, fused=False)
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
    times = []
    for _ in range(steps):
        t0 = time.perf_counter()
        m.time_step(dt)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    ok = bool(all(torch.isfinite(f.data).all() for f in (m.u, m.v) + tuple(m.tracers)))
    return statistics.median(times), ok


bih = lambda: ocn.HorizontalScalarBiharmonicDiffusivity(ν=NU, κ=KAPPA)
cavd = lambda: ocn.ConvectiveAdjustmentVerticalDiffusivity(convective_κz=1.0, background_κz=1e-3, convective_νz=0.1, background_νz=1e-2)
print(f"grid {Nx}x{Nx}x{Nz}, dt = {dt:.4g} s, ν = κ = {NU:.3g} m⁴/s", flush=True)
# ---- kernels, on the arrays of a model with the tuple
m = model((bih(), cavd()))
d = m.diffusivity_fields
kc, ku = d["kappa_c"], d["kappa_u"]
fields = [m.u, m.v] + list(m.tracers)
Gs = [torch.zeros_like(f.data) for f in fields]
Ss = [torch.zeros_like(f.data) for f in fields]
pa = L.ptr_array
one = lambda x: (C.c_double * 1)(x)
calls = {
    "biharmonic term, momentum": (48, lambda: L.call("ocn_add_biharmonic_fluxes", g.cref, NU, m.u.ptr, m.v.ptr, Gs[0].data_ptr(), Gs[1].data_ptr(), 0,
                                                      None, None, None, None, None, None, 0)),
    "biharmonic term, one tracer": (24, lambda: L.call("ocn_add_biharmonic_fluxes", g.cref, 0.0, None, None, None, None, 1, one(KAPPA),
                                                        pa([fields[2].ptr]), pa([Gs[2].data_ptr()]), None, None, None, 0)),
    "biharmonic term, momentum + 2 tracers (3 launches)": (96, lambda: L.call(
        "ocn_add_biharmonic_fluxes", g.cref, NU, m.u.ptr, m.v.ptr, Gs[0].data_ptr(), Gs[1].data_ptr(), 2, (C.c_double * 2)(KAPPA, KAPPA),
        pa([c.ptr for c in m.tracers]), pa([G.data_ptr() for G in Gs[2:]]), None, None, None, 0)),
    "biharmonic term, momentum, with neg_other": (64, lambda: L.call("ocn_add_biharmonic_fluxes", g.cref, NU, m.u.ptr, m.v.ptr, Gs[0].data_ptr(),
                                                                      Gs[1].data_ptr(), 0, None, None, None, Ss[0].data_ptr(), Ss[1].data_ptr(), None, 0)),
    "biharmonic term, one tracer, with neg_other": (32, lambda: L.call("ocn_add_biharmonic_fluxes", g.cref, 0.0, None, None, None, None, 1, one(KAPPA),
                                                                        pa([fields[2].ptr]), pa([Gs[2].data_ptr()]), None, None,
                                                                        pa([Ss[2].data_ptr()]), 0)),
    "yardstick: vertical closure term (explicit), momentum": (56, lambda: L.call(
        "ocn_add_vertical_diffusivity_fluxes", g.cref, ku.ptr, m.u.ptr, m.v.ptr, Gs[0].data_ptr(), Gs[1].data_ptr(), 0, None, None, None, 0, None, 0)),
    "yardstick: vertical closure term (explicit), one tracer": (32, lambda: L.call(
        "ocn_add_vertical_diffusivity_fluxes", g.cref, None, None, None, None, None, 1, pa([kc.ptr]), pa([fields[2].ptr]), pa([Gs[2].data_ptr()]), 0, None, 0)),
    "yardstick: vertical closure term (explicit), momentum + 2 tracers (3 launches)": (120, lambda: L.call(
        "ocn_add_vertical_diffusivity_fluxes", g.cref, ku.ptr, m.u.ptr, m.v.ptr, Gs[0].data_ptr(), Gs[1].data_ptr(), 2, pa([kc.ptr, kc.ptr]),
        pa([c.ptr for c in m.tracers]), pa([G.data_ptr() for G in Gs[2:]]), 0, None, 0)),
}
for rep in range(2):  # the new launches and the yardstick alternate in the same process
    for label, (nbytes, call) in calls.items():
        ms = device_ms(call)
        print(f"[{rep}] {label}: {ms:.3f} ms, {nbytes * cells / ms / 1e9:.3f} TB/s of its {nbytes} B/cell", flush=True)
del Gs, Ss, m, d, kc, ku, fields, calls
torch.cuda.empty_cache()


# ---- steps (each model built, warmed up and timed on its own; the first model a process times carries one-time costs: it is timed again last)
def timed(label, closure):
    mm = model(closure)
    ms, ok = step_ms(mm)
    print(f"config-5 step, fused = False, {label}: {ms:.2f} ms/step (median of {steps}, finite={ok})", flush=True)
    del mm
    torch.cuda.empty_cache()


timed("no closure, FIRST model of the process (one-time costs included: not the figure to quote)", None)
for rep in range(2):
    timed(f"[{rep}] no closure", None)
    timed(f"[{rep}] HorizontalScalarBiharmonicDiffusivity", bih())
    timed(f"[{rep}] ConvectiveAdjustmentVerticalDiffusivity", cavd())
    timed(f"[{rep}] (HorizontalScalarBiharmonicDiffusivity, ConvectiveAdjustmentVerticalDiffusivity)", (bih(), cavd()))
