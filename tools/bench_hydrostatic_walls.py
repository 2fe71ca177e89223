#!/usr/bin/env python3
"""HydrostaticFreeSurfaceModel on grids with walls against the doubly periodic grid, config 5's term set (VectorInvariant() momentum, WENO
tracers T and S, SplitExplicitFreeSurface(substeps = 30), FPlane, SeawaterBuoyancy, ScalarDiffusivity, QAB2) at 1024 x 1024 x 128, one GPU,
one process, the three topologies alternating:

  tools/bench_hydrostatic_walls.py [Nx] [Nz] [steps]

1. the unfused step (fused = False: the reference's launch sequence, the only one on wall grids) on (Periodic, Periodic, Bounded) -- the
   yardstick: the <false, false> instantiation of the same kernels (csrc/hydrostatic_surface.hip) --, (Periodic, Bounded, Bounded) and (Bounded, Bounded, Bounded);
2. every hydrostatic-specific entry point alone on each topology (a device-event pair around each launch after a warm-up);
3. the tendency entry points shared with NonhydrostaticModel, which are known to cost more on wall grids, reported apart.
Two rounds of repeats; per round the median (minimum to maximum).  Prints one line per figure and topology."""
import os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as C
import numpy as np, torch
import oceananigans_jl_amd as ocn

Nx = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
Nz = int(sys.argv[2]) if len(sys.argv) > 2 else 128
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
H, Lx, substeps, grav = 1000.0, 1.0e6 * Nx / 1024.0, 30, 9.80665
TOPOLOGIES = {"PPB": ("Periodic", "Periodic", "Bounded"), "PBB": ("Periodic", "Bounded", "Bounded"), "BBB": ("Bounded", "Bounded", "Bounded")}
L = ocn._lib
ocn.set_math_mode(ocn.MATH_FAST)  # bench.py's config-5 mode (the hydrostatic-specific kernels have one arithmetic variant)


def device_ms(call, repeats):
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record(); torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return times


def show(label, topo, rounds):
    txt = "; ".join("round %d: %.3f (%.3f to %.3f) ms" % (n + 1, statistics.median(t), min(t), max(t)) for n, t in enumerate(rounds))
    print(f"{label:<52s} {topo}  {txt}", flush=True)
    return [statistics.median(t) for t in rounds]


def make_model(topo):
    g = ocn.RectilinearGrid(ocn.GPU(), size=(Nx, Nx, Nz), x=(0, Lx), y=(0, Lx), z=(-H, 0.0), topology=TOPOLOGIES[topo], halo=(3, 3, 3))
    m = ocn.HydrostaticFreeSurfaceModel(g, momentum_advection=ocn.VectorInvariant(), tracer_advection=ocn.WENO(), tracers=("T", "S"),
                                        free_surface=ocn.SplitExplicitFreeSurface(substeps=substeps), coriolis=ocn.FPlane(f=1e-4),
                                        closure=ocn.ScalarDiffusivity(ν=1e-2, κ=1e-3),
                                        buoyancy=ocn.SeawaterBuoyancy(equation_of_state=ocn.LinearEquationOfState(2e-4, 8e-4)), fused=False)
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    rnd = lambda t, amp: amp * (torch.rand(t.shape, generator=gen, device="cuda", dtype=torch.float64) * 2 - 1)
    m.u.interior_view().copy_(rnd(m.u.interior_view(), 1e-2)); m.v.interior_view().copy_(rnd(m.v.interior_view(), 1e-2))
    m.field("T").interior_view().copy_(20 + rnd(m.field("T").interior_view(), 1e-2)); m.field("S").interior_view().fill_(35.0)
    m.eta_interior().copy_(rnd(m.eta_interior(), 1e-2))
    m.update_state(compute_tendencies=False)
    return m


def kernels(m):
    g, nh = m.grid, m._nh
    Gn, Gm = nh.timestepper._Gn, nh.timestepper._Gm
    w = (C.c_double * substeps)(*([1.0 / substeps] * substeps))
    dtau = 0.5 * g.dx / np.sqrt(grav * H)
    Qu, Qv = torch.zeros_like(m.U), torch.zeros_like(m.V)
    rhs = torch.zeros((g.Ny, g.Nx), dtype=torch.float64, device="cuda")
    e, U, V, eb, Ub, Vb, GU, GV = (t.data_ptr() for t in (m.eta, m.U, m.V, m._etab, m._Ub, m._Vb, m._GU, m._GV))
    u, v, ww = m.u.ptr, m.v.ptr, m.w.ptr
    own = {
        "ocn_compute_w_from_continuity": lambda: L.call("ocn_compute_w_from_continuity", g.cref, u, v, ww, 0),
        "ocn_fill_free_surface_halos": lambda: L.call("ocn_fill_free_surface_halos", g.cref, e, 0),
        "ocn_compute_vector_invariant_momentum_tendencies": lambda: L.call("ocn_compute_vector_invariant_momentum_tendencies", g.cref, u, v, ww,
                                                                          Gn[0].ptr, Gn[1].ptr, None, grav, 0),
        "... with eta": lambda: L.call("ocn_compute_vector_invariant_momentum_tendencies", g.cref, u, v, ww, Gn[0].ptr, Gn[1].ptr, e, grav, 0),
        "ocn_add_barotropic_pressure_gradient": lambda: L.call("ocn_add_barotropic_pressure_gradient", g.cref, grav, e, Gn[0].ptr, Gn[1].ptr, 0),
        "ocn_compute_barotropic_mode": lambda: L.call("ocn_compute_barotropic_mode", g.cref, u, v, Ub, Vb, 0),
        "ocn_split_explicit_forcing": lambda: L.call("ocn_split_explicit_forcing", g.cref, Gn[0].ptr, Gm[0].ptr, Gn[1].ptr, Gm[1].ptr, 0.1, GU, GV, 0),
        f"ocn_split_explicit_substeps (n = {substeps})": lambda: L.call("ocn_split_explicit_substeps", g.cref, substeps, w, float(dtau), grav, H, e, U, V,
                                                                      eb, Ub, Vb, GU, GV, 0),
        "ocn_barotropic_split_explicit_corrector": lambda: L.call("ocn_barotropic_split_explicit_corrector", g.cref, u, v, U, V, Ub, Vb, H, 0),
        "ocn_explicit_free_surface_ab2_step": lambda: L.call("ocn_explicit_free_surface_ab2_step", g.cref, ww, e, m._Geta.data_ptr(),
                                                             m._Geta_m.data_ptr(), 1e-6, 0.1, 0),
        "ocn_implicit_free_surface_rhs": lambda: L.call("ocn_implicit_free_surface_rhs", g.cref, u, v, e, grav, 100.0, Qu.data_ptr(), Qv.data_ptr(),
                                                        rhs.data_ptr(), 0),
        "ocn_barotropic_pressure_correction": lambda: L.call("ocn_barotropic_pressure_correction", g.cref, u, v, e, grav, 1e-6, 0),
    }
    terms = C.byref(nh._terms)
    T = m.field("T")
    shared = {
        "ocn_add_momentum_terms (shared)": lambda: L.call("ocn_add_momentum_terms", g.cref, terms, u, v, ww, Gn[0].ptr, Gn[1].ptr, Gn[2].ptr, None, 0),
        "ocn_compute_tracer_tendency_terms (shared)": lambda: L.call("ocn_compute_tracer_tendency_terms", g.cref, terms, 1e-3, None, u, v, ww, T.ptr,
                                                                    Gn[3].ptr, None, 0),
        "fill_halo_regions of u, v, T, S (shared)": lambda: ocn.fill_halo_regions((m.u, m.v) + tuple(m.tracers), fill_boundary_normal_velocities=False),
    }
    return own, shared


models = {t: make_model(t) for t in TOPOLOGIES}
dt = 2.0 * models["PPB"].grid.dx / np.sqrt(grav * H)  # bench.py's config-5 step
print(f"grid {Nx}x{Nx}x{Nz}, halo (3, 3, 3), dt = {dt:.4g} s, fast math, {steps} steps and 11 kernel repeats per round", flush=True)
for m in models.values():  # warm-up: two steps each
    m.time_step(dt); m.time_step(dt)
torch.cuda.synchronize()
step_rounds = {t: [[], []] for t in TOPOLOGIES}
for r in range(2):
    for _ in range(steps):
        for t, m in models.items():  # alternating
            step_rounds[t][r] += device_ms(lambda: m.time_step(dt), 1)
medians = {t: show("unfused QAB2 step", t, step_rounds[t]) for t in TOPOLOGIES}
for t in ("PBB", "BBB"):
    print(f"step ratio {t} / PPB: " + ", ".join("%.3f" % (a / b) for a, b in zip(medians[t], medians["PPB"])), flush=True)
finite = all(bool(torch.isfinite(f.data).all()) for m in models.values() for f in (m.u, m.v, m.w) + tuple(m.tracers))
print("finite after the steps:", finite, flush=True)
sets = {t: kernels(m) for t, m in models.items()}
for which in (0, 1):
    for name in sets["PPB"][which]:
        rounds = {t: [[], []] for t in TOPOLOGIES}
        for t in TOPOLOGIES:
            sets[t][which][name](); torch.cuda.synchronize()
        for r in range(2):
            for _ in range(11):
                for t in TOPOLOGIES:
                    rounds[t][r] += device_ms(sets[t][which][name], 1)
        med = {t: show(name, t, rounds[t]) for t in TOPOLOGIES}
        spread = abs(med["PPB"][0] - med["PPB"][1]) / min(med["PPB"])
        print("    ratios to PPB: " + "; ".join(f"{t} " + ", ".join("%.3f" % (a / b) for a, b in zip(med[t], med["PPB"])) for t in ("PBB", "BBB"))
              + "; PPB round-to-round spread %.3f" % spread, flush=True)
sys.exit(0 if finite else 1)
