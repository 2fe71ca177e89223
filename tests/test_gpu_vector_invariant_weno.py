"""The upwinding vector-invariant momentum advection on the GPU (csrc/vector_invariant_weno.hip):
ocn_compute_vector_invariant_weno_momentum_tendencies against the NumPy restatement of the reference
(tests/vector_invariant_weno_numpy.py, pinned without a GPU in tests/test_host_vector_invariant_weno.py) bit for bit on whole parent
arrays, its refusals, the tendencies of a HydrostaticFreeSurfaceModel with WENOVectorInvariant(order=5), the reference's own time-stepping
test with every free surface, SplitRungeKutta3 and a closure tuple, and the unchanged default VectorInvariant().

The kernel works on 32 x 8 tiles of the xy plane and marches eight planes per workgroup: 5 x 6 x 4 is smaller than a tile and has every
vertical face order-reduced; 67 x 13 x 9 has ragged tile edges in x and y, two marches, and faces 4 .. 7 of full order on a stretched z;
130 x 9 x 7 has five tiles in x, unequal halos wider than the reach, and a march that ends early."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import pytest

import implicit_diffusion_numpy as IDN
import vector_invariant_weno_numpy as VIN
from helpers import from_dev, stretched_faces, to_dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

P, B = "Periodic", "Bounded"
CC, CCF = 0, 4  # location masks (Periodic x and y: u, v and the tendencies share the parent shape of a centre field)
GRAV = 9.80665
# size, halo, z
SHAPES = [((5, 6, 4), (3, 3, 3), (-1.0, 0.0)), ((67, 13, 9), (4, 4, 3), "stretched"), ((130, 9, 7), (5, 6, 4), (-2.0, 0.0))]
SHAPE_IDS = ["below_a_tile", "ragged_stretched", "five_tiles_wide_halos"]
VARIANTS = [(name, stencil) for name, s in VIN.SCHEMES.items() for stencil in (("velocity", "default") if s.vorticity == VIN.W else ("velocity",))]
VARIANT_IDS = [f"{n}-{st}" for n, st in VARIANTS]


def _grid(ocn, size, halo, z, topo=(P, P, B)):
    zz = stretched_faces(size[2]) if isinstance(z, str) else z
    return ocn.RectilinearGrid(ocn.GPU(), size=size, x=(0, size[0] / 16), y=(0, size[1] / 12), z=zz, topology=topo, halo=halo)


def _poison(g, a, reach_xy, faces):
    """a copy with NaN wherever the kernel may not read: beyond `reach_xy` cells from the interior in x and y, and beyond one plane from the
    interior in z (the order reduction keeps the z stencils inside; `faces`: the field has the face Nz + 1 of its own)"""
    p = np.full(a.shape, np.nan)
    keep = (slice(g.Hx - reach_xy, g.Hx + g.Nx + reach_xy), slice(g.Hy - reach_xy, g.Hy + g.Ny + reach_xy),
            slice(g.Hz, g.Hz + g.Nz + 1) if faces else slice(g.Hz - 1, g.Hz + g.Nz + 1))
    p[keep] = a[keep]
    return p


def random_inputs(g, seed):
    """random parents of u, v, w (both signs everywhere; w is not from continuity, so both vertical biases occur on every face), each with
    a patch of exact zeros (the `> 0` tie of the bias, and stencils of zeros); random tendencies and η"""
    rng = np.random.default_rng(seed)
    shape = (g.Nx + 2 * g.Hx, g.Ny + 2 * g.Hy, g.Nz + 2 * g.Hz)
    f = dict(u=rng.uniform(-1, 1, shape), v=rng.uniform(-1, 1, shape), w=rng.uniform(-1, 1, shape[:2] + (shape[2] + 1,)))
    for n, (name, a) in enumerate(f.items()):
        i, j = g.Hx + (n * 2) % max(g.Nx - 2, 1), g.Hy + n % max(g.Ny - 2, 1)
        a[i:i + 4, j:j + 3, g.Hz:g.Hz + 3] = 0.0
    G = dict(u=rng.uniform(-1, 1, shape), v=rng.uniform(-1, 1, shape))
    eta = rng.uniform(-1, 1, shape[:2])
    return f, G, eta


_cases = {}


def _case(ocn, n):
    if n not in _cases:
        pg = _grid(ocn, *SHAPES[n])
        g = IDN.describe(pg)
        f, G, eta = random_inputs(g, 4100 + n)
        _cases[n] = dict(pg=pg, g=g, f=f, G=G, eta=eta, want={})
    return _cases[n]


def _want(c, name, stencil, with_eta):
    key = (name, stencil, with_eta)
    if key not in c["want"]:
        s = VIN.SCHEMES[name]._replace(stencil=stencil)
        c["want"][key] = VIN.tendencies(c["g"], s, c["f"]["u"], c["f"]["v"], c["f"]["w"], c["eta"] if with_eta else None, GRAV)
    return c["want"][key]


def _eta_dev(ocn, pg, eta):
    import torch
    return torch.from_numpy(np.ascontiguousarray(eta.T)).to(ocn.Field(CC, pg).data.device)


# ---- 1. the entry point, bit for bit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,stencil", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("n", range(len(SHAPES)), ids=SHAPE_IDS)
def test_entry_point_equals_the_restatement_bit_for_bit(ocn, n, name, stencil):
    """Gu and Gv over the interior equal the restatement's (np.array_equal on whole parents: the halos of G keep their random values),
    without and with η.  The device reads fields that hold NaN beyond the reach stated in include/ocn_hip.h (3 cells in x and y for u and
    v, 2 for w, one plane in z), the restatement the clean ones."""
    c = _case(ocn, n)
    pg, g, f = c["pg"], c["g"], c["f"]
    s = VIN.SCHEMES[name]._replace(stencil=stencil)
    du, dv = (to_dev(ocn, pg, CC, _poison(g, f[q], 3, False)) for q in "uv")
    dw = to_dev(ocn, pg, CCF, _poison(g, f["w"], 2, True))
    deta = _eta_dev(ocn, pg, c["eta"])
    for with_eta in (False, True):
        dGu, dGv = to_dev(ocn, pg, CC, c["G"]["u"]), to_dev(ocn, pg, CC, c["G"]["v"])
        ocn._lib.call("ocn_compute_vector_invariant_weno_momentum_tendencies", pg.cref, VIN.flags(s), du.ptr, dv.ptr, dw.ptr, dGu.ptr, dGv.ptr,
                      deta.data_ptr() if with_eta else None, GRAV, 0)
        ocn.sync_device()
        want = _want(c, name, stencil, with_eta)
        for q, dG, wq in (("u", dGu, want[0]), ("v", dGv, want[1])):
            got, full = from_dev(dG), VIN.into_parent(g, c["G"][q], wq)
            assert np.isfinite(got).all(), q
            assert np.abs(wq).max() > 0.1
            assert np.array_equal(got, full), f"G{q} (eta: {with_eta}): max difference {np.abs(got - full).max():.3e}"
    assert not np.array_equal(_want(c, name, stencil, False)[0], _want(c, name, stencil, True)[0])
    if n == 0 and s.vertical == VIN.W:  # every face of this column is order-reduced: faces 1, 2, 4, 5 of order 1, face 3 of order 3
        assert g.Nz == 4


# ---- 2. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_return_an_error_and_launch_nothing(ocn):
    fn = ocn._lib.lib().ocn_compute_vector_invariant_weno_momentum_tendencies
    rng = np.random.default_rng(5)

    def attempt(pg, flags_, null=None):
        g = IDN.describe(pg)
        shape = (g.Nx + 2 * g.Hx, g.Ny + 2 * g.Hy, g.Nz + 2 * g.Hz)
        host = {q: rng.uniform(-1, 1, shape[:2] + (shape[2] + (q == "w"),)) for q in ("u", "v", "w", "Gu", "Gv")}
        dev = {q: to_dev(ocn, pg, CCF if q == "w" else CC, a) for q, a in host.items()}
        ptr = {q: (None if q == null else C.c_void_p(d.ptr if isinstance(d.ptr, int) else d.ptr.value)) for q, d in dev.items()}
        st = fn(pg.cref, flags_, ptr["u"], ptr["v"], ptr["w"], ptr["Gu"], ptr["Gv"], None, GRAV, None)
        ocn.sync_device()
        assert st < 0 and ocn._lib.lib().ocn_last_error()
        for q in ("Gu", "Gv"):
            assert np.array_equal(from_dev(dev[q]), host[q])

    size, z = (8, 8, 6), (-1.0, 0.0)
    attempt(_grid(ocn, size, (2, 3, 3), z), 7)                      # a halo below the reach
    attempt(_grid(ocn, size, (3, 3, 3), z, topo=(P, B, B)), 7)      # a Bounded y
    attempt(_grid(ocn, size, (3, 3, 3), z), 0)                      # all conserving: the other entry point's case
    attempt(_grid(ocn, size, (3, 3, 3), z), 7, null="v")            # a null pointer
    attempt(_grid(ocn, size, (3, 3, 3), z), 7, null="Gu")


# ---- 3. the model's tendencies --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,mode", [("split", "strict"), ("explicit", "strict"), ("split", "fast")])
def test_model_tendencies_equal_the_restatement(ocn, kind, mode):
    """HydrostaticFreeSurfaceModel(16 x 12 x 8, momentum_advection = WENOVectorInvariant(order=5)) with no other term: after `set` and
    update_state, Gⁿ[0] and Gⁿ[1] are the restatement applied to the model's own u, v and w -- with - g ∇η for the ExplicitFreeSurface.
    A MATH_FAST model calls the same kernel."""
    pg = ocn.RectilinearGrid(ocn.GPU(), size=(16, 12, 8), x=(0, 1), y=(0, 1), z=stretched_faces(8), topology=(P, P, B), halo=(3, 3, 3))
    fs = ocn.SplitExplicitFreeSurface(substeps=10) if kind == "split" else ocn.ExplicitFreeSurface()
    m = ocn.HydrostaticFreeSurfaceModel(pg, momentum_advection=ocn.WENOVectorInvariant(order=5), free_surface=fs,
                                        math_mode=ocn.MATH_STRICT if mode == "strict" else ocn.MATH_FAST)
    assert m.fused is False and (m.grid.Hx, m.grid.Hy, m.grid.Hz) == (4, 4, 3)
    rng = np.random.default_rng(77)
    m.set(u=rng.uniform(-1, 1, (16, 12, 8)), v=rng.uniform(-1, 1, (16, 12, 8)), eta=0.1 * rng.uniform(-1, 1, (16, 12)))
    m.update_state()
    ocn.sync_device()
    g = IDN.describe(m.grid)
    u, v, w = m.u.parent(), m.v.parent(), m.w.parent()
    assert np.abs(w).max() > 0
    eta = m.eta.cpu().numpy().T if kind == "explicit" else None
    Gu, Gv = VIN.tendencies(g, VIN.SCHEMES["WWW"], u, v, w, eta, m.free_surface.gravitational_acceleration)
    Gn = m._nh.timestepper._Gn
    assert np.abs(Gu).max() > 0.1
    assert np.array_equal(g_interior(g, Gn[0].parent()), Gu) and np.array_equal(g_interior(g, Gn[1].parent()), Gv)
    if kind == "explicit":
        plain = VIN.tendencies(g, VIN.SCHEMES["WWW"], u, v, w)
        assert not np.array_equal(plain[0], Gu)


def g_interior(g, a):
    return a[g.Hx:g.Hx + g.Nx, g.Hy:g.Hy + g.Ny, g.Hz:g.Hz + g.Nz]


# ---- 4. the reference's own test ------------------------------------------------------------------------------------------------------
def _digests(m):
    fields = {n: m.field(n).parent() for n in ("u", "v", "w") + tuple(m.tracer_names)}
    fields["η"] = m.eta.cpu().numpy()
    fields.update({f"Gⁿ[{q}]": G.parent() for q, G in enumerate(m._nh.timestepper._Gn)})
    assert all(np.isfinite(a).all() for a in fields.values())
    return {n: hashlib.sha256(a.tobytes()).hexdigest() for n, a in fields.items()}


@pytest.mark.parametrize("setting", ["explicit", "split", "implicit", "split_rk3", "closure_tuple"])
@pytest.mark.parametrize("scheme", ["WENOVectorInvariant", "VectorInvariant_WENO"])
def test_time_step_hydrostatic_model_works(ocn, scheme, setting):
    """time_step_hydrostatic_model_works (test_hydrostatic_free_surface_models.jl:10-30; the reference steps both spellings at :249-281):
    one step, finite fields, with T and S, SeawaterBuoyancy, an FPlane and WENO() tracers on 13 x 6 x 4 with a stretched z.  Two identical
    runs end in identical bits; the model is unfused and its halo (4, 4, 3)."""
    import test_gpu_biharmonic as T

    def run():
        adv = ocn.WENOVectorInvariant(order=5) if scheme == "WENOVectorInvariant" else ocn.VectorInvariant(vorticity_scheme=ocn.WENO(), vertical_scheme=ocn.WENO())
        closure = None
        if setting == "closure_tuple":
            closure = (ocn.HorizontalScalarBiharmonicDiffusivity(**T.BIH), ocn.ConvectiveAdjustmentVerticalDiffusivity(**T.CAVD_COEFFS))
        m = ocn.HydrostaticFreeSurfaceModel(T._model_grid(ocn), momentum_advection=adv, tracer_advection=ocn.WENO(), tracers=("T", "S"),
                                            buoyancy=ocn.SeawaterBuoyancy(), coriolis=ocn.FPlane(f=1e-4), closure=closure,
                                            free_surface=T._free_surface(ocn, setting if setting in ("explicit", "implicit") else "split"),
                                            timestepper="SplitRungeKutta3" if setting == "split_rk3" else "QuasiAdamsBashforth2",
                                            math_mode=ocn.MATH_STRICT)
        assert m.fused is False and (m.grid.Hx, m.grid.Hy, m.grid.Hz) == (4, 4, 3)
        assert m.momentum_advection.scheme_flags == 7
        m.set(**T._initial())
        m.time_step(T.DT)
        m.flush_tendencies()
        ocn.sync_device()
        assert m.clock.iteration == 1 and np.abs(m.u.interior()).max() > 0 and np.abs(m.eta.cpu().numpy()).max() > 0
        return _digests(m)

    assert run() == run()


# ---- 5. the default is what it was ---------------------------------------------------------------------------------------------------
def test_default_vector_invariant_is_unchanged(ocn):
    """Three steps of the `none-defaults` case of tests/golden/hydrostatic_steps.json (VectorInvariant() momentum, Centered() tracers, split-
    explicit free surface, fused by default) with the scheme spelled out through the new keywords: the digests of that record, which
    tests/test_gpu_hydrostatic_steps.py holds momentum_advection = None to."""
    import json
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import record_hydrostatic_steps as R
    import test_gpu_biharmonic as T
    with open(os.path.join(ROOT, "tests", "golden", "hydrostatic_steps.json")) as f:
        golden = json.load(f)["cases"]["none-defaults"]
    adv = ocn.VectorInvariant(vorticity_scheme=ocn.EnstrophyConserving(), vorticity_stencil=ocn.VelocityStencil(), vertical_scheme=ocn.EnergyConserving(),
                              upwinding=ocn.OnlySelfUpwinding())
    assert adv.scheme_flags == 0 and not adv.upwinds
    m = ocn.HydrostaticFreeSurfaceModel(T._model_grid(ocn), momentum_advection=adv, closure=None, tracers=("T", "S"), buoyancy=ocn.SeawaterBuoyancy(),
                                        coriolis=ocn.FPlane(f=1e-4), math_mode=ocn.MATH_STRICT, free_surface=T._free_surface(ocn, "split"),
                                        boundary_conditions={"T": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(1e-3))})
    assert m.fused is True and golden["fused"] is True
    assert (m.grid.Hx, m.grid.Hy, m.grid.Hz) == (3, 3, 3)
    m.set(**T._initial())
    for _ in range(R.STEPS):
        m.time_step(T.DT)
    m.flush_tendencies()
    ocn.sync_device()
    assert _digests(m) == {n: d for n, d in golden["sha256"].items() if not n.startswith("diffusivity_fields/")}
