#!/usr/bin/env python3
"""Record of what HydrostaticFreeSurfaceModel does with its closure: per case the ordered names of the library calls of the construction
plus `set` and of each of three `time_step(DT)`, and after the third step (and `flush_tendencies` where the step is fused) the SHA-256 of
the parent bytes of u, v, w, the tracers, η, every Gⁿ and every diffusivity field.  A change to the Python host that sequences the
launches (hydrostatic.py, hydrostatic_closures.py, models.py) must reproduce every list and every digest; a mismatch is a launch that
moved, went missing, or received another argument.

Only the public API and a replacement of `_lib.call` are used, so the same file runs on any commit; the cases run in order in THIS
process.  The settings are those of tests/test_gpu_biharmonic.py (`_model_grid`, `_initial`: 13 x 6 x 4, stretched z, T and S,
SeawaterBuoyancy, an FPlane, a top flux on T, strict math, an unstable upper half so that both values of κᶜ and κᵘ occur).

Usage: python tools/record_hydrostatic_steps.py OUT.json [--commit ID]
       (tests/golden/hydrostatic_steps.json was written from a checkout of the commit it names, with a library built from it)"""
import hashlib
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

STEPS = 3
SCALAR = dict(ν=0.02, κ={"T": 0.01, "S": 0.03})  # (κ Δt / min Δz² = 0.13 with the explicit discretization)
# id -> (closure, keywords of the model other than the shared ones); fs: the free surface kinds of test_gpu_biharmonic._free_surface
CASES = {
    "none-defaults": (lambda o, T: None, dict(fs="split", tracer_advection=None)),
    "scalar-fused": (lambda o, T: o.ScalarDiffusivity(**SCALAR), dict(fs="split", fused=True)),
    "scalar-unfused-explicit_fs": (lambda o, T: o.ScalarDiffusivity(**SCALAR), dict(fs="explicit", fused=False)),
    "implicit_scalar": (lambda o, T: o.ScalarDiffusivity(o.VerticallyImplicitTimeDiscretization(), **SCALAR), dict(fs="split")),
    "implicit_scalar-flux_form": (lambda o, T: o.ScalarDiffusivity(o.VerticallyImplicitTimeDiscretization(), **SCALAR),
                                  dict(fs="split", momentum_advection="WENO")),
    "cavd-implicit_fs": (lambda o, T: o.ConvectiveAdjustmentVerticalDiffusivity(**T.CAVD_COEFFS), dict(fs="implicit")),
    "cavd_explicit": (lambda o, T: o.ConvectiveAdjustmentVerticalDiffusivity("Explicit", **T.CAVD_COEFFS), dict(fs="split")),
    "ri_based": (lambda o, T: o.RiBasedVerticalDiffusivity(), dict(fs="split")),
    "ri_based-filter-explicit_fs": (lambda o, T: o.RiBasedVerticalDiffusivity(horizontal_Ri_filter=o.FivePointHorizontalFilter()),
                                    dict(fs="explicit")),
    "biharmonic": (lambda o, T: o.HorizontalScalarBiharmonicDiffusivity(**T.BIH), dict(fs="split")),
    "biharmonic-split_rk3": (lambda o, T: o.HorizontalScalarBiharmonicDiffusivity(**T.BIH), dict(fs="split", timestepper="SplitRungeKutta3")),
    "biharmonic+cavd": (lambda o, T: (o.HorizontalScalarBiharmonicDiffusivity(**T.BIH), o.ConvectiveAdjustmentVerticalDiffusivity(**T.CAVD_COEFFS)),
                        dict(fs="split")),
    "biharmonic+cavd_explicit": (lambda o, T: (o.HorizontalScalarBiharmonicDiffusivity(**T.BIH),
                                               o.ConvectiveAdjustmentVerticalDiffusivity("Explicit", **T.CAVD_COEFFS)), dict(fs="split")),
    "ri_based+biharmonic": (lambda o, T: (o.RiBasedVerticalDiffusivity(), o.HorizontalScalarBiharmonicDiffusivity(**T.BIH)), dict(fs="split")),
}


def run_case(ocn, T, closure, fs, **kw):
    """the record of one case: {"construction": names, "steps": [names] * 3, "sha256": {field: digest}}"""
    L, names = ocn._lib, []
    real_call = L.call

    def call(name, *args):
        names.append(name[4:] if name.startswith("ocn_") else name)
        return real_call(name, *args)

    def taken():
        out = " ".join(names)
        names.clear()
        return out

    for key in ("momentum_advection", "tracer_advection"):
        kw[key] = ocn.WENO() if kw.get(key, "WENO" if key == "tracer_advection" else None) == "WENO" else None
    L.call = call
    try:
        m = ocn.HydrostaticFreeSurfaceModel(T._model_grid(ocn), closure=closure(ocn, T), tracers=("T", "S"), buoyancy=ocn.SeawaterBuoyancy(),
                                            coriolis=ocn.FPlane(f=1e-4), math_mode=ocn.MATH_STRICT, free_surface=T._free_surface(ocn, fs),
                                            boundary_conditions={"T": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(1e-3))}, **kw)
        m.set(**T._initial())
        out = {"fused": bool(m.fused), "construction": taken(), "steps": []}
        for _ in range(STEPS):
            m.time_step(T.DT)
            out["steps"].append(taken())
        m.flush_tendencies()
        out["flush"] = taken()
    finally:
        L.call = real_call
    ocn.sync_device()
    fields = {n: m.field(n).parent() for n in ("u", "v", "w") + tuple(m.tracer_names)}
    fields["η"] = m.eta.cpu().numpy()
    fields.update({f"Gⁿ[{q}]": G.parent() for q, G in enumerate(m._nh.timestepper._Gn)})
    fields.update({f"diffusivity_fields/{n}": f.parent() for n, f in (m.diffusivity_fields or {}).items()})
    out["sha256"] = {n: hashlib.sha256(a.tobytes()).hexdigest() for n, a in fields.items()}
    return out


def record(ocn):
    import test_gpu_biharmonic as T
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)  # (RiBasedVerticalDiffusivity says that it is experimental)
        return {name: run_case(ocn, T, closure, **kw) for name, (closure, kw) in CASES.items()}


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    commit = sys.argv[sys.argv.index("--commit") + 1] if "--commit" in sys.argv else None
    import oceananigans_jl_amd
    doc = {"commit": commit, "cases": record(oceananigans_jl_amd)}
    with open(sys.argv[1], "w") as f:
        json.dump(doc, f, indent=1, ensure_ascii=False)
        f.write("\n")
