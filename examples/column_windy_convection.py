#!/usr/bin/env python3
"""A wind- and cooling-forced column, after the reference's validation/vertical_mixing_closures/column_windy_convection.jl: linearly
stratified buoyancy b = N² z under a destabilising surface buoyancy flux Jᵇ and a wind stress τˣ on an f-plane, mixed by
RiBasedVerticalDiffusivity (vertically implicit: Δt is far above Δz² / 2κ).  The reference's column is (Flat, Flat, Bounded); here it is a
small horizontally periodic box of identical columns, since this package's closure needs a non-Flat x and y.  The mixed layer deepens by
convective adjustment (κᶜᵃ where N² < 0), by entrainment at its base (Cᵉⁿ Jᵇ / N² under a convecting face) and by shear mixing where
Ri = N² / S² is small (κ₀, ν₀ times the taper); the script prints its depth -- the shallowest face whose N² is still at least half the
initial one -- next to the non-penetrative estimate √(2 Jᵇ t / N²).  --closure catke mixes with CATKEVerticalDiffusivity instead: a second
tracer e, the turbulent kinetic energy, which the closure steps itself; the script then prints max e as well.  As in the reference e is
stepped after the halo fill of update_state!, so its columns differ at rounding level; on 25 m cells the cooled, unstably stratified layer
turns that into resolved hydrostatic convection between the columns, which a (Flat, Flat, Bounded) column does not have.  The CATKE box
is therefore 400 km wide by default (--width), where no horizontal mode is resolved.  --closure k_epsilon mixes with
TKEDissipationVerticalDiffusivity, the third closure of the reference's script: two tracers that the closure steps itself, e and its
dissipation epsilon; the same wide box, and max e and max ϵ are printed.

    python examples/column_windy_convection.py [--closure ri|cavd|catke|k_epsilon] [--nz 128] [--hours 24] [--dt 60] [--taper tanh|exp|linear] [--filter] [--width W]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import oceananigans_jl_amd as ocn

ap = argparse.ArgumentParser()
ap.add_argument("--closure", choices=("ri", "cavd", "catke", "k_epsilon"), default="ri")
ap.add_argument("--nz", type=int, default=128)
ap.add_argument("--hours", type=float, default=24.0)
ap.add_argument("--dt", type=float, default=60.0)
ap.add_argument("--taper", choices=("tanh", "exp", "linear"), default="tanh")
ap.add_argument("--filter", action="store_true", help="horizontal_Ri_filter = FivePointHorizontalFilter()")
ap.add_argument("--width", type=float, default=None, help="extent of the box in x and y [m]: 100 by default, 4e5 with --closure catke or k_epsilon")
a = ap.parse_args()

Lz = 256.0        # extent of the vertical domain [m] (Δz = 2 m at the default Nz)
f0 = 1e-4         # Coriolis parameter [s⁻¹]
N2 = 1e-5         # buoyancy gradient [s⁻²]
Jb = 1e-7         # surface buoyancy flux [m² s⁻³], positive: destabilising
tau_x = -1e-4     # surface kinematic momentum flux [m² s⁻²]
n = 4             # columns per side
width = a.width if a.width is not None else (4e5 if a.closure in ("catke", "k_epsilon") else 100.0)
grid = ocn.RectilinearGrid(ocn.GPU(), size=(n, n, a.nz), x=(0, width), y=(0, width), z=(-Lz, 0), topology=("Periodic", "Periodic", "Bounded"))
if a.closure == "ri":
    taper = {"tanh": ocn.HyperbolicTangentRiDependentTapering, "exp": ocn.ExponentialRiDependentTapering,
             "linear": ocn.PiecewiseLinearRiDependentTapering}[a.taper]()
    closure = ocn.RiBasedVerticalDiffusivity(Ri_dependent_tapering=taper, horizontal_Ri_filter=ocn.FivePointHorizontalFilter() if a.filter else None)
elif a.closure == "catke":
    closure = ocn.CATKEVerticalDiffusivity()
elif a.closure == "k_epsilon":
    closure = ocn.TKEDissipationVerticalDiffusivity()
else:
    closure = ocn.ConvectiveAdjustmentVerticalDiffusivity(convective_κz=1.0, background_κz=1e-5, convective_νz=0.1, background_νz=1e-4)
bcs = {"b": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(Jb)), "u": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(tau_x))}
tracers = {"catke": ("b", "e"), "k_epsilon": ("b", "e", "epsilon")}.get(a.closure, ("b",))
model = ocn.HydrostaticFreeSurfaceModel(grid, tracers=tracers, buoyancy=ocn.BuoyancyTracer(), coriolis=ocn.FPlane(f=f0), closure=closure,
                                        boundary_conditions=bcs)
model.set(b=lambda x, y, z: N2 * z + 0 * x + 0 * y)
print(closure)
dz = Lz / a.nz
print(f"Δz = {dz:g} m, Δt = {a.dt:g} s, Jᵇ = {Jb:g} m² s⁻³, τˣ = {tau_x:g} m² s⁻², N² = {N2:g} s⁻²")
z_faces = np.asarray(grid.nodes_1d(2, True))[:a.nz + 1]


def mixed_layer_depth():
    """the depth of the shallowest interior face whose N² is at least half the initial stratification (column 1, 1)"""
    b = model.field("b").interior()[0, 0, :]
    stratified = (b[1:] - b[:-1]) / dz >= 0.5 * N2          # faces 2..Nz
    k = np.nonzero(stratified)[0]
    return float(-z_faces[1 + k.max()]) if k.size else Lz


t0, every = time.perf_counter(), max(1, int(round(2 * 3600 / a.dt)))
depths = []
while model.clock.time < a.hours * 3600:
    if model.clock.iteration % every == 0:
        h = mixed_layer_depth()
        depths.append(h)
        kc = model.diffusivity_fields["kappa_c"].interior()[0, 0, :a.nz]
        tke = ", max(e) %.3g" % float(model.field("e").interior().max()) if "e" in tracers else ""
        print("Iter: %5d, t = %5.1f h, wall %5.1f s | mixed-layer depth %6.1f m, non-penetrative estimate %6.1f m, max(κc) %.3g, max(u) %.3g%s" % (
            model.clock.iteration, model.clock.time / 3600, time.perf_counter() - t0, h, np.sqrt(2 * Jb * model.clock.time / N2), kc.max(),
            float(np.abs(model.u.interior()).max()), tke), flush=True)
    model.time_step(a.dt)
ocn.sync_device()
h, estimate = mixed_layer_depth(), np.sqrt(2 * Jb * model.clock.time / N2)
print(f"after {model.clock.time / 3600:.1f} h: mixed-layer depth {h:.1f} m, non-penetrative estimate {estimate:.1f} m")
if "e" in tracers:
    print(f"max e {float(model.field('e').interior().max()):.3g} m² s⁻²")
if "epsilon" in tracers:
    print(f"max ϵ {float(model.field('epsilon').interior().max()):.3g} m² s⁻³")
b = model.field("b").interior()
print(f"largest difference between the columns: {np.abs(b - b[:1, :1]).max():.3g}")
assert np.isfinite(b).all() and h > depths[0]
