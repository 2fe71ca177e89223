#!/usr/bin/env python3
"""CATKEVerticalDiffusivity at config 5's grid (1024 x 1024 x 128, regular z), one GPU, one process:

  tools/bench_catke.py [Nx] [Nz] [steps]

1. kernel times (device events around 10 launches after a warm-up launch, 5 such samples alternating between the kernels: median and the
   range are printed), each with its achieved bytes/s against the kernel's own minimum traffic per cell:
     diffusivities              64 B: u, v, T, S, e read, κᵘ, κᶜ, κᵉ written
     substep + solve           152 B: u⁺, v⁺, uⁿ, vⁿ, T, S, e, κᵘ, κᶜ, Gⁿe, G⁻e read (88), κᵉ, Le, G⁻e, e and the multipliers written (40), the
                                      multipliers and e read and e written by the backward sweep (24)
     substep alone             120 B: the same without the multipliers and the backward sweep
     Jᵇ and the top flux of e   planes: two layers of u, v, three of T, S, one of e per column; ms only
2. step times of the config-5 model (bench.py --workload config5: VectorInvariant, WENO tracers, SplitExplicitFreeSurface(substeps = 30),
   FPlane, SeawaterBuoyancy, QAB2) with CATKEVerticalDiffusivity, with RiBasedVerticalDiffusivity and with closure = None, each model
   built, warmed up (2 steps) and timed `steps` steps three times; the ratio of the medians to the Ri-based step is printed.  The surface is
   cooled, the wind blows, and the top fifth of the column starts unstable.
Prints one line per figure."""
import ctypes as C
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import oceananigans_jl_amd as ocn
from oceananigans_jl_amd.hydrostatic_closures import top_condition

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


def model(closure, tracers=("T", "S")):
    bcs = {"T": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(200.0 / (1026.0 * 3991.0))),  # 200 W m⁻² of cooling
           "u": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(-1e-4))}
    m = ocn.HydrostaticFreeSurfaceModel(g, momentum_advection=ocn.VectorInvariant(), tracer_advection=ocn.WENO(), tracers=tracers,
                                        free_surface=ocn.SplitExplicitFreeSurface(substeps=substeps), coriolis=ocn.FPlane(f=1e-4), closure=closure,
                                        buoyancy=ocn.SeawaterBuoyancy(equation_of_state=ocn.LinearEquationOfState(2e-4, 8e-4)),
                                        boundary_conditions=bcs)
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    zc = torch.linspace(-H + H / (2 * Nz), -H / (2 * Nz), Nz, device="cuda", dtype=torch.float64)
    profile = 20 + 0.01 * zc - 0.02 * torch.clamp(zc + 0.2 * H, min=0.0)  # stable below -H / 5, unstable above
    T = m.field("T").interior_view()
    T.copy_(profile[:, None, None] + 1e-4 * torch.rand(T.shape, generator=gen, device="cuda", dtype=torch.float64))
    m.field("S").interior_view().fill_(35.0)
    if "e" in tracers:
        m.field("e").interior_view().fill_(1e-6)
    for f in (m.u, m.v):
        iv = f.interior_view(); iv.copy_(1e-2 * (torch.rand(iv.shape, generator=gen, device="cuda", dtype=torch.float64) * 2 - 1))
    m.update_state(compute_tendencies=False)
    return m


def step_ms(m):
    for _ in range(2):
        m.time_step(dt)
    m.flush_tendencies(); torch.cuda.synchronize()
    samples = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(steps):
            m.time_step(dt)
        m.flush_tendencies(); torch.cuda.synchronize()
        samples.append((time.perf_counter() - t0) / steps * 1e3)
    ok = bool(all(torch.isfinite(f.data).all() for f in (m.u, m.v) + tuple(m.tracers)))
    return samples, ok


# ---- kernels
m = model(ocn.CATKEVerticalDiffusivity(), ("T", "S", "e"))
for _ in range(2):  # a state with turbulence in it
    m.time_step(dt)
torch.cuda.synchronize()
cf, nh = m._closure, m._nh
d = cf.fields
terms, cl, (zf, zc_) = C.byref(nh._terms), C.byref(cf.struct), cf.znodes
tops = cf.top_conditions(nh)
e = nh.field("e")
Gn, Gm = cf._tendencies(nh, "e")
e_work, Gm_work, Jb_work = torch.zeros_like(e.data), torch.zeros_like(Gm.data), torch.zeros_like(d["Jb"])
ku_w, kc_w, ke_w, Le_w = (torch.zeros_like(d[n].data) for n in ("kappa_u", "kappa_c", "kappa_e", "Le"))
print(f"grid {Nx}x{Nx}x{Nz}, dt = {dt:.4g} s; max e {float(e.interior_view().max()):.3g}, max κᶜ {float(d['kappa_c'].interior_view().max()):.3g}, "
      f"mean Jᵇ {float(d['Jb'].mean()):.3g}", flush=True)
dif_call = lambda: L.call("ocn_compute_catke_diffusivities", g.cref, terms, cl, zf.data_ptr(), zc_.data_ptr(), m.u.ptr, m.v.ptr, e.ptr,
                          d["Jb"].data_ptr(), ku_w.data_ptr(), kc_w.data_ptr(), ke_w.data_ptr(), 0)


def substep_call(solve):
    def call():  # (e and G⁻e are stepped in place: work copies, refreshed outside the timed region by the warm-up launch only)
        L.call("ocn_catke_substep_tke", g.cref, terms, cl, zf.data_ptr(), zc_.data_ptr(), m.u.ptr, m.v.ptr, cf.u_prev.ptr, cf.v_prev.ptr,
               e_work.data_ptr(), d["Jb"].data_ptr(), d["kappa_u"].ptr, d["kappa_c"].ptr, ke_w.data_ptr(), Le_w.data_ptr(), Gn.ptr,
               Gm_work.data_ptr(), cf.ivd_scratch[3].data_ptr(), float(dt), 0.1, solve, 0)
    return call


jb_call = lambda: L.call("ocn_compute_catke_surface_buoyancy_flux", g.cref, terms, cl, *tops, zf.data_ptr(), zc_.data_ptr(), m.u.ptr, m.v.ptr, e.ptr,
                         Jb_work.data_ptr(), float(dt), 0)
top_call = lambda: L.call("ocn_compute_catke_top_tke_flux", g.cref, terms, cl, top_condition(nh, nh.u), top_condition(nh, nh.v), *tops, m.u.ptr, m.v.ptr,
                          cf.top_e._device_values.data_ptr(), 0)
calls = [("diffusivities", dif_call, 64), ("substep + solve", substep_call(1), 152), ("substep alone", substep_call(0), 120),
         ("surface buoyancy flux (plane)", jb_call, 0), ("top flux of e (plane)", top_call, 0)]
samples = {name: [] for name, _, _ in calls}
for rep in range(5):  # the kernels alternate
    e_work.copy_(e.data); Gm_work.copy_(Gm.data); Jb_work.copy_(d["Jb"])
    for name, call, _ in calls:
        samples[name].append(device_ms(call))
for name, _, nbytes in calls:
    s = sorted(samples[name])
    rate = f", {nbytes * cells / s[2] / 1e9:.3f} TB/s of its {nbytes} B/cell" if nbytes else ""
    print(f"{name}: median {s[2]:.3f} ms (min {s[0]:.3f}, max {s[-1]:.3f}; 5 samples of 10 launches){rate}", flush=True)
del m, cf, nh, d, e, Gn, Gm, e_work, Gm_work, Jb_work, ku_w, kc_w, ke_w, Le_w, tops
torch.cuda.empty_cache()


# ---- steps (each model built, warmed up and timed on its own; the first model a process times carries one-time costs: it is timed again last)
def timed(label, closure, tracers=("T", "S")):
    mm = model(closure, tracers)
    s, ok = step_ms(mm)
    print(f"config-5 step, {label}: median {sorted(s)[1]:.2f} ms/step (samples {', '.join(f'{x:.2f}' for x in s)}; finite={ok}, fused={mm.fused})", flush=True)
    del mm
    torch.cuda.empty_cache()
    return sorted(s)[1]


timed("CATKEVerticalDiffusivity, FIRST model of the process (one-time costs included: not the figure to quote)", ocn.CATKEVerticalDiffusivity(),
      ("T", "S", "e"))
ri = timed("RiBasedVerticalDiffusivity (vertically implicit)", ocn.RiBasedVerticalDiffusivity(warning=False))
none = timed("closure = None", None)
catke = timed("CATKEVerticalDiffusivity", ocn.CATKEVerticalDiffusivity(), ("T", "S", "e"))
print(f"CATKE / Ri-based = {catke / ri:.2f}; CATKE / no closure = {catke / none:.2f}; Ri-based / no closure = {ri / none:.2f}", flush=True)
