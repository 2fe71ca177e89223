#!/usr/bin/env python3
"""TKEDissipationVerticalDiffusivity (k-ϵ) at config 5's grid (1024 x 1024 x 128, regular z), one GPU, one process:

  tools/bench_tke_dissipation.py [Nx] [Nz] [steps]

1. kernel times (device events around 10 launches after a warm-up launch, 5 such samples alternating between the kernels: median and the
   range are printed), each with its achieved bytes/s against the kernel's own minimum traffic per cell:
     k-ϵ diffusivities            80 B: u, v, T, S, e, ϵ read, κᵘ, κᶜ, κᵉ, κᵋ written
     k-ϵ substep + two solves    240 B: u⁺, v⁺, uⁿ, vⁿ, T, S, e, ϵ, κᵘ, κᶜ, Gⁿe, G⁻e, Gⁿϵ, G⁻ϵ read (112), κᵉ, κᵋ, Le, Lϵ, G⁻e, G⁻ϵ, e, ϵ and the two
                                        multipliers written (80), the multipliers, e and ϵ read and e, ϵ written by the backward sweeps (48)
     k-ϵ substep alone           176 B: the same without the multipliers and the backward sweeps
     k-ϵ top fluxes               planes: one layer of u, v, e per column; ms only
   and, alternating with them in the same loop as the yardstick, CATKE's two column launches with their own minima (tools/bench_catke.py):
     CATKE diffusivities          64 B
     CATKE substep + solve       152 B
2. step times of the config-5 model (bench.py --workload config5: VectorInvariant, WENO tracers, SplitExplicitFreeSurface(substeps = 30),
   FPlane, SeawaterBuoyancy, QAB2) with TKEDissipationVerticalDiffusivity, with CATKEVerticalDiffusivity and with closure = None, each model
   built, warmed up (2 steps) and timed `steps` steps three times; the ratios of the medians are printed.  The surface is cooled, the wind
   blows, and the top fifth of the column starts unstable.
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
KEPS, CATKE = ("T", "S", "e", "epsilon"), ("T", "S", "e")


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
    if "epsilon" in tracers:
        m.field("epsilon").interior_view().fill_(1e-9)
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


# ---- kernels: a k-ϵ model and a CATKE model, each with turbulence in its state
def turbulent(closure, tracers):
    m = model(closure, tracers)
    for _ in range(2):
        m.time_step(dt)
    torch.cuda.synchronize()
    return m


mk, mc = turbulent(ocn.TKEDissipationVerticalDiffusivity(), KEPS), turbulent(ocn.CATKEVerticalDiffusivity(), CATKE)
kf, kn, cf, cn = mk._closure, mk._nh, mc._closure, mc._nh
kd, cd = kf.fields, cf.fields
e, p = kn.field("e"), kn.field("epsilon")
(Gn_e, Gm_e), (Gn_p, Gm_p) = kf._tendencies(kn, "e"), kf._tendencies(kn, "epsilon")
work = {name: torch.zeros_like(t.data) for name, t in (("e", e), ("eps", p), ("Gm_e", Gm_e), ("Gm_eps", Gm_p), ("Le", kd["Le"]), ("Leps", kd["Leps"]))}
kw = [torch.zeros_like(kd[n].data) for n in ("kappa_u", "kappa_c", "kappa_e", "kappa_eps")]
Qw = [torch.zeros_like(kf.tops["e"]._device_values) for _ in range(2)]
print(f"grid {Nx}x{Nx}x{Nz}, dt = {dt:.4g} s; k-ϵ: max e {float(e.interior_view().max()):.3g}, max ϵ {float(p.interior_view().max()):.3g}, "
      f"max κᶜ {float(kd['kappa_c'].interior_view().max()):.3g}; CATKE: max e {float(cn.field('e').interior_view().max()):.3g}", flush=True)
k_terms, k_cl = C.byref(kn._terms), C.byref(kf.struct)
k_dif = lambda: L.call("ocn_compute_tke_dissipation_diffusivities", g.cref, k_terms, k_cl, mk.u.ptr, mk.v.ptr, e.ptr, p.ptr, *[t.data_ptr() for t in kw], 0)


def k_substep(solve):
    def call():  # (e, ϵ and G⁻ are stepped in place: work copies, refreshed outside the timed region)
        L.call("ocn_tke_dissipation_substep", g.cref, k_terms, k_cl, mk.u.ptr, mk.v.ptr, kf.u_prev.ptr, kf.v_prev.ptr, work["e"].data_ptr(),
               work["eps"].data_ptr(), kd["kappa_u"].ptr, kd["kappa_c"].ptr, kw[2].data_ptr(), kw[3].data_ptr(), work["Le"].data_ptr(),
               work["Leps"].data_ptr(), Gn_e.ptr, work["Gm_e"].data_ptr(), Gn_p.ptr, work["Gm_eps"].data_ptr(), kf.ivd_scratch[3].data_ptr(),
               float(dt), 0.1, solve, 0)
    return call


k_top = lambda: L.call("ocn_compute_tke_dissipation_top_fluxes", g.cref, k_cl, top_condition(kn, kn.u), top_condition(kn, kn.v), kf.zc.data_ptr(), mk.u.ptr, mk.v.ptr,
                       e.ptr, Qw[0].data_ptr(), Qw[1].data_ptr(), 0)
# the yardstick
c_terms, c_cl, (zf, zc_) = C.byref(cn._terms), C.byref(cf.struct), cf.znodes
ce = cn.field("e")
cGn, cGm = cf._tendencies(cn, "e")
c_work = {"e": torch.zeros_like(ce.data), "Gm": torch.zeros_like(cGm.data), "Le": torch.zeros_like(cd["Le"].data)}
cw = [torch.zeros_like(cd[n].data) for n in ("kappa_u", "kappa_c", "kappa_e")]
c_dif = lambda: L.call("ocn_compute_catke_diffusivities", g.cref, c_terms, c_cl, zf.data_ptr(), zc_.data_ptr(), mc.u.ptr, mc.v.ptr, ce.ptr,
                       cd["Jb"].data_ptr(), *[t.data_ptr() for t in cw], 0)
c_sub = lambda: L.call("ocn_catke_substep_tke", g.cref, c_terms, c_cl, zf.data_ptr(), zc_.data_ptr(), mc.u.ptr, mc.v.ptr, cf.u_prev.ptr, cf.v_prev.ptr,
                       c_work["e"].data_ptr(), cd["Jb"].data_ptr(), cd["kappa_u"].ptr, cd["kappa_c"].ptr, cw[2].data_ptr(), c_work["Le"].data_ptr(),
                       cGn.ptr, c_work["Gm"].data_ptr(), cf.ivd_scratch[3].data_ptr(), float(dt), 0.1, 1, 0)
calls = [("k-ϵ diffusivities", k_dif, 80), ("CATKE diffusivities (yardstick)", c_dif, 64), ("k-ϵ substep + two solves", k_substep(1), 240),
         ("CATKE substep + solve (yardstick)", c_sub, 152), ("k-ϵ substep alone", k_substep(0), 176), ("k-ϵ top fluxes (plane)", k_top, 0)]
samples = {name: [] for name, _, _ in calls}
for rep in range(5):  # the kernels alternate
    for name, t in (("e", e), ("eps", p), ("Gm_e", Gm_e), ("Gm_eps", Gm_p)):
        work[name].copy_(t.data)
    c_work["e"].copy_(ce.data); c_work["Gm"].copy_(cGm.data)
    for name, call, _ in calls:
        samples[name].append(device_ms(call))
for name, _, nbytes in calls:
    s = sorted(samples[name])
    rate = f", {nbytes * cells / s[2] / 1e9:.3f} TB/s of its {nbytes} B/cell" if nbytes else ""
    print(f"{name}: median {s[2]:.3f} ms (min {s[0]:.3f}, max {s[-1]:.3f}; 5 samples of 10 launches){rate}", flush=True)
del mk, mc, kf, kn, cf, cn, kd, cd, e, p, ce, Gn_e, Gm_e, Gn_p, Gm_p, cGn, cGm, work, c_work, kw, cw, Qw
torch.cuda.empty_cache()


# ---- steps (each model built, warmed up and timed on its own; the first model a process times carries one-time costs: it is timed again last)
def timed(label, closure, tracers=("T", "S")):
    mm = model(closure, tracers)
    s, ok = step_ms(mm)
    print(f"config-5 step, {label}: median {sorted(s)[1]:.2f} ms/step (samples {', '.join(f'{x:.2f}' for x in s)}; finite={ok}, fused={mm.fused})", flush=True)
    del mm
    torch.cuda.empty_cache()
    return sorted(s)[1]


timed("TKEDissipationVerticalDiffusivity, FIRST model of the process (one-time costs included: not the figure to quote)",
      ocn.TKEDissipationVerticalDiffusivity(), KEPS)
catke = timed("CATKEVerticalDiffusivity", ocn.CATKEVerticalDiffusivity(), CATKE)
none = timed("closure = None", None)
keps = timed("TKEDissipationVerticalDiffusivity", ocn.TKEDissipationVerticalDiffusivity(), KEPS)
print(f"k-ϵ / CATKE = {keps / catke:.2f}; k-ϵ / no closure = {keps / none:.2f}; CATKE / no closure = {catke / none:.2f}", flush=True)
