#!/usr/bin/env python3
"""HydrostaticFreeSurfaceModel over bathymetry (ImmersedBoundaryGrid(grid, GridFittedBottom(h)), csrc/immersed.hip) against the plain grid,
at 1024 x 1024 x 128, one GPU, one process, strict math (the immersed kernels have one arithmetic variant):

  tools/bench_immersed.py [Nx] [Nz] [steps]

VectorInvariant() momentum, Centered() tracers b and c, BuoyancyTracer, FPlane, SplitExplicitFreeSurface(substeps = 20), ScalarDiffusivity, QAB2.
1. the model step, three models alternating: over a Gaussian seamount (250 m in 2 km of water, as in the reference's internal_tide.jl), over
   a flat bottom on an ImmersedBoundaryGrid (the cost of the predicates alone) and on the plain grid with fused = False (the yardstick: the
   reference's launch sequence on the kernels that existed before);
2. every new entry point alone (a device-event pair around each launch after a warm-up), over the seamount and over the flat bottom, next
   to the plain launch it stands in for, with the bytes each must move per cell (every array it reads or writes, once) and the rate that gives.
Two rounds of repeats; per round the median (minimum to maximum).  Prints one line per figure."""
import os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as C
import numpy as np, torch
import oceananigans_jl_amd as ocn

Nx = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
Nz = int(sys.argv[2]) if len(sys.argv) > 2 else 128
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
H, Lx, substeps, grav = 2000.0, 2.0e6 * Nx / 1024.0, 20, 9.80665
L = ocn._lib
ocn.set_math_mode(ocn.MATH_STRICT)


def device_ms(call, repeats):
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record(); torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return times


def show(label, which, rounds, bytes_per_cell=None):
    txt = "; ".join("round %d: %.3f (%.3f to %.3f) ms" % (n + 1, statistics.median(t), min(t), max(t)) for n, t in enumerate(rounds))
    med = [statistics.median(t) for t in rounds]
    rate = ""
    if bytes_per_cell:
        rate = "  %d B/cell, %.2f TB/s" % (bytes_per_cell, bytes_per_cell * Nx * Nx * Nz / (min(med) * 1e-3) / 1e12)
    print(f"{label:<58s} {which:<9s} {txt}{rate}", flush=True)
    return med


def seamount(x, y):
    return -H + 250.0 * np.exp(-((x - Lx / 2) ** 2 + (y - Lx / 2) ** 2) / (2 * (Lx / 20) ** 2))


def make_model(which):
    g = ocn.RectilinearGrid(ocn.GPU(), size=(Nx, Nx, Nz), x=(0, Lx), y=(0, Lx), z=(-H, 0.0), topology=("Periodic", "Periodic", "Bounded"),
                            halo=(3, 3, 3))
    if which != "plain":
        g = ocn.ImmersedBoundaryGrid(g, ocn.GridFittedBottom(seamount if which == "seamount" else -2 * H))
    m = ocn.HydrostaticFreeSurfaceModel(g, tracers=("b", "c"), free_surface=ocn.SplitExplicitFreeSurface(substeps=substeps),
                                        coriolis=ocn.FPlane(f=1e-4), closure=ocn.ScalarDiffusivity(ν=1e-2, κ=1e-3), buoyancy=ocn.BuoyancyTracer(),
                                        fused=False if which == "plain" else None)
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    rnd = lambda t, amp: amp * (torch.rand(t.shape, generator=gen, device="cuda", dtype=torch.float64) * 2 - 1)
    m.u.interior_view().copy_(rnd(m.u.interior_view(), 1e-2)); m.v.interior_view().copy_(rnd(m.v.interior_view(), 1e-2))
    m.field("b").interior_view().copy_(rnd(m.field("b").interior_view(), 1e-4)); m.field("c").interior_view().copy_(1 + rnd(m.field("c").interior_view(), 0.5))
    m.eta_interior().copy_(rnd(m.eta_interior(), 1e-2))
    m.update_state(compute_tendencies=False)
    return m


def kernels(m, immersed):
    """{label: (call, bytes per cell)}; the plain model gets the launches the immersed ones stand in for, under the same labels"""
    g, nh = m.grid, m._nh
    Gn, Gm = nh.timestepper._Gn, nh.timestepper._Gm
    w = (C.c_double * substeps)(*([1.0 / substeps] * substeps))
    dtau = 0.5 * g.dx / np.sqrt(grav * H)
    e, U, V, eb, Ub, Vb, GU, GV = (t.data_ptr() for t in (m.eta, m.U, m.V, m._etab, m._Ub, m._Vb, m._GU, m._GV))
    u, v, ww, c = m.u.ptr, m.v.ptr, m.w.ptr, m.field("c").ptr
    if immersed:
        kb, Hfc, Hcf = g.plane_ptr("kbot"), g.plane_ptr("Hfc"), g.plane_ptr("Hcf")
        fields = [m.u, m.v] + list(m.tracers)
        pa, ia = L.ptr_array([f.ptr for f in fields]), L.i32_array([f.loc for f in fields])
        return {
            "mask of u, v, b, c, eta, U, V (writes masked nodes only)": (lambda: L.call("ocn_immersed_mask_fields", g.cref, kb, 4, pa, ia, 0.0, e, U, V, 0), None),
            "vector-invariant momentum tendencies": (lambda: L.call("ocn_immersed_vector_invariant_momentum_tendencies", g.cref, kb, u, v, ww, Gn[0].ptr,
                                                                    Gn[1].ptr, None, grav, 0), 40),
            "viscous terms of u, v": (lambda: L.call("ocn_immersed_add_viscous_terms", g.cref, kb, 1e-2, u, v, ww, Gn[0].ptr, Gn[1].ptr, 0), 56),
            "tracer tendency, Centered + ScalarDiffusivity": (lambda: L.call("ocn_immersed_tracer_tendency", g.cref, kb, 1, 1e-3, u, v, ww, c, Gn[4].ptr, 0), 40),
            "split-explicit forcing": (lambda: L.call("ocn_immersed_split_explicit_forcing", g.cref, kb, Gn[0].ptr, Gm[0].ptr, Gn[1].ptr, Gm[1].ptr, 0.1,
                                                      GU, GV, 0), 32),
            f"split-explicit substeps (n = {substeps}; planes only)": (lambda: L.call("ocn_immersed_split_explicit_substeps", g.cref, kb, Hfc, Hcf, substeps, w,
                                                                                  float(dtau), grav, e, U, V, eb, Ub, Vb, GU, GV, 0), None),
            "barotropic mode + corrector": (lambda: L.call("ocn_immersed_barotropic_corrector", g.cref, Hfc, Hcf, u, v, U, V, Ub, Vb, 0), 48),
        }
    only_closure = L.CModelTerms.from_buffer_copy(nh._terms)
    only_closure.coriolis, only_closure.buoyancy, only_closure.pHY = 0, 0, None
    return {
        "vector-invariant momentum tendencies": (lambda: L.call("ocn_compute_vector_invariant_momentum_tendencies", g.cref, u, v, ww, Gn[0].ptr, Gn[1].ptr,
                                                                None, grav, 0), 40),
        # (the plain launch also adds the closure term of w: three components, 3 + 6 arrays)
        "viscous terms of u, v": (lambda: L.call("ocn_add_momentum_terms", g.cref, C.byref(only_closure), u, v, ww, Gn[0].ptr, Gn[1].ptr, Gn[2].ptr, None, 0), 72),
        # (two launches: advection writes G, diffusion reads c and updates G)
        "tracer tendency, Centered + ScalarDiffusivity": (lambda: L.call("ocn_compute_tracer_tendency_terms", g.cref, C.byref(nh._terms), 1e-3, None, u, v, ww,
                                                                         c, Gn[4].ptr, None, 0), 64),
        "split-explicit forcing": (lambda: L.call("ocn_split_explicit_forcing", g.cref, Gn[0].ptr, Gm[0].ptr, Gn[1].ptr, Gm[1].ptr, 0.1, GU, GV, 0), 32),
        f"split-explicit substeps (n = {substeps}; planes only)": (lambda: L.call("ocn_split_explicit_substeps", g.cref, substeps, w, float(dtau), grav, H, e, U,
                                                                              V, eb, Ub, Vb, GU, GV, 0), None),
        "barotropic mode + corrector": (lambda: L.call("ocn_barotropic_split_explicit_corrector", g.cref, u, v, U, V, Ub, Vb, H, 0), 48),
    }


WHICH = ("seamount", "flat", "plain")
models = {t: make_model(t) for t in WHICH}
kb = models["seamount"].grid.kbot
dt = 2.0 * models["plain"].grid.dx / np.sqrt(grav * H)
print(f"grid {Nx}x{Nx}x{Nz}, halo (3, 3, 3), dt = {dt:.4g} s, strict math, {steps} steps and 11 kernel repeats per round; seamount: up to "
      f"{int(kb.max())} immersed cells per column, {float((kb > 0).mean()) * 100:.1f} % of the columns touched, "
      f"{float(kb.sum()) / (Nx * Nx * Nz) * 100:.2f} % of the cells immersed", flush=True)
for m in models.values():  # warm-up: two steps each
    m.time_step(dt); m.time_step(dt)
torch.cuda.synchronize()
step_rounds = {t: [[], []] for t in WHICH}
for r in range(2):
    for _ in range(steps):
        for t, m in models.items():  # alternating
            step_rounds[t][r] += device_ms(lambda: m.time_step(dt), 1)
medians = {t: show("QAB2 step (reference launch sequence)", t, step_rounds[t]) for t in WHICH}
for t in ("seamount", "flat"):
    print(f"step ratio {t} / plain: " + ", ".join("%.3f" % (a / b) for a, b in zip(medians[t], medians["plain"])), flush=True)
finite = all(bool(torch.isfinite(f.interior_view()).all()) for m in models.values() for f in (m.u, m.v, m.w) + tuple(m.tracers))
print("finite interiors after the steps:", finite, flush=True)
sets = {t: kernels(m, t != "plain") for t, m in models.items()}
for name in sets["seamount"]:
    have = [t for t in WHICH if name in sets[t]]
    rounds = {t: [[], []] for t in have}
    for t in have:
        sets[t][name][0](); torch.cuda.synchronize()
    for r in range(2):
        for _ in range(11):
            for t in have:
                rounds[t][r] += device_ms(sets[t][name][0], 1)
    med = {t: show(name, t, rounds[t], sets[t][name][1]) for t in have}
    if "plain" in med:
        print("    ratios to the plain launch: " + "; ".join(f"{t} " + ", ".join("%.3f" % (a / b) for a, b in zip(med[t], med["plain"]))
                                                             for t in ("seamount", "flat")), flush=True)
sys.exit(0 if finite else 1)
