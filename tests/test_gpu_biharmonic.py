"""HorizontalScalarBiharmonicDiffusivity on the GPU (csrc/biharmonic.hip): ocn_add_biharmonic_fluxes against the NumPy restatement of the
reference (tests/biharmonic_numpy.py, pinned without a GPU in tests/test_host_biharmonic.py) bit for bit on whole parent arrays -- alone and
as one half of a two-closure tuple --, steps of the hydrostatic model against a twin whose tendencies receive the restatement's term, and the
decay of a grid-scale mode on the device.

The kernel works on 64 x 8 tiles of the xy plane and marches eight planes per workgroup: 13 x 6 is a partial tile, 65 x 9 is one cell more
than a tile in x and in y (four workgroups, three of them nearly empty), Nz = 12 takes one full and one partial march, and on 4 x 3 x 1 with
halos (2, 2, 1) the stencil meets the periodic images of its own cell."""
import ctypes as C
import warnings

import numpy as np
import pytest

import biharmonic_numpy as BHN
import convective_adjustment_numpy as CAN
import implicit_diffusion_numpy as IDN
from helpers import from_dev, stretched_faces, to_dev

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
P, B = "Periodic", "Bounded"
U, V, CC, CCF = 1, 2, 0, 4  # location masks
SEAWATER = ("SeawaterBuoyancy", 9.80665, 1.67e-4, 7.80e-4)
# size, z ("stretched" or an interval), halo (a halo is at most the size)
CASES = [((13, 6, 12), "stretched", (3, 3, 3)),
         ((13, 6, 3), (-1.0, 0.0), (2, 2, 2)),
         ((13, 6, 12), "stretched", (4, 3, 5)),
         ((4, 3, 1), (-1.0, 0.0), (2, 2, 1)),
         ((65, 9, 2), "stretched", (2, 2, 2))]
IDS = ["stretched", "minimal_halo", "halo435", "own_images", "tile_plus_one"]
NAMES = ("u", "v", "c", "c2")
NU, KAPPAS = 1.0e-6, (2.0e-6, 5.0e-7)  # (Δx = 1 / 13, Δy = 1 / 12: ν (4 / Δx² + 4 / Δy²)² = 1.6, the term is of the size of G)
TUPLE_SEED = 4242  # test 7: chosen on the CPU so that the restatement tells G - (a + b) from (G - a) - b (asserted there)


def _grid(ocn, size, z, halo, arch="gpu"):
    zz = stretched_faces(size[2]) if isinstance(z, str) else z
    return ocn.RectilinearGrid(ocn.GPU() if arch == "gpu" else None, size=size, x=(0, size[0] / 13), y=(0, size[1] / 12), z=zz,
                               topology=(P, P, B), halo=halo)


def random_inputs(g, seed):
    """random parents (halos included) of u, v, two tracers and their tendencies, and copies of the fields whose cells further than two
    from the interior in x or y, and every plane outside k = 1..Nz, hold NaN: the kernel may not read them"""
    rng = np.random.default_rng(seed)
    shape = (g.Nx + 2 * g.Hx, g.Ny + 2 * g.Hy, g.Nz + 2 * g.Hz)  # Periodic x and y: the three locations share it
    f = {name: rng.uniform(-1, 1, shape) for name in NAMES}
    G = {name: rng.uniform(-1, 1, shape) for name in NAMES}
    poisoned = {}
    for name, a in f.items():
        p = np.full(shape, np.nan)
        keep = (slice(g.Hx - 2, g.Hx + g.Nx + 2), slice(g.Hy - 2, g.Hy + g.Ny + 2), slice(g.Hz, g.Hz + g.Nz))
        p[keep] = a[keep]
        poisoned[name] = p
    return f, G, poisoned


_inputs = {}


def _case(ocn, n):
    if n not in _inputs:
        pg = _grid(ocn, *CASES[n])
        g = IDN.describe(pg)
        f, G, poisoned = random_inputs(g, 991 + n)
        a_u, a_v, a_c = BHN.terms(g, NU, f["u"], f["v"], KAPPAS, [f["c"], f["c2"]])
        _inputs[n] = dict(pg=pg, g=g, f=f, G=G, poisoned=poisoned, a=dict(u=a_u, v=a_v, c=a_c[0], c2=a_c[1]))
    return _inputs[n]


def _call(ocn, pg, nu, momentum, kappas, tracers, neg_momentum=(None, None), neg_tracers=None):
    """momentum: (u, v, Gu, Gv) device fields or None; tracers: [(c, Gc), ...]"""
    L = ocn._lib
    ptr = lambda x: None if x is None else x.ptr
    nt = len(tracers)
    L.call("ocn_add_biharmonic_fluxes", pg.cref, float(nu), *([ptr(x) for x in momentum] if momentum else [None] * 4), nt,
           (C.c_double * max(nt, 1))(*kappas) if nt else None, L.ptr_array([c.ptr for c, _ in tracers]) if nt else None,
           L.ptr_array([G.ptr for _, G in tracers]) if nt else None, ptr(neg_momentum[0]), ptr(neg_momentum[1]),
           L.ptr_array([ptr(x) for x in neg_tracers]) if neg_tracers else None, 0)
    ocn.sync_device()


# ---- 6. the entry point, bit for bit -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["momentum", "tracers", "both", "nu0"])
@pytest.mark.parametrize("n", range(len(CASES)), ids=IDS)
def test_entry_point_equals_the_restatement_bit_for_bit(ocn, n, variant):
    """G - (closure term) for u, v and two tracers with different κ, whole parent arrays compared (np.array_equal, strict build): the halos
    of G and the tendencies a variant leaves out keep their random values.  The device reads fields whose cells beyond two from the
    interior (and every z halo plane) are NaN, the restatement the clean ones: the read radius.  Variants: momentum only (n_tracers = 0),
    tracers only (u == NULL), both, and ν = 0 with κ != 0 (the momentum launch is skipped: G - 0 ν-free)."""
    c = _case(ocn, n)
    pg, g = c["pg"], c["g"]
    df = {name: to_dev(ocn, pg, CC, c["poisoned"][name]) for name in NAMES}
    dG = {name: to_dev(ocn, pg, CC, c["G"][name]) for name in NAMES}
    momentum = (df["u"], df["v"], dG["u"], dG["v"]) if variant != "tracers" else None
    tracers = [(df["c"], dG["c"]), (df["c2"], dG["c2"])] if variant != "momentum" else []
    nu = 0.0 if variant == "nu0" else NU
    _call(ocn, pg, nu, momentum, KAPPAS, tracers)
    touched = {"momentum": ("u", "v"), "tracers": ("c", "c2"), "both": NAMES, "nu0": NAMES}[variant]
    for name in NAMES:
        got = from_dev(dG[name])
        if name not in touched:
            want = c["G"][name]
        elif variant == "nu0" and name in ("u", "v"):
            a0 = BHN.momentum_terms(g, 0.0, c["f"]["u"], c["f"]["v"])[name == "v"]
            assert np.all(a0 == 0)
            want = BHN.subtract(g, c["G"][name], a0)
        else:
            want = BHN.subtract(g, c["G"][name], c["a"][name])
            assert not np.array_equal(want, c["G"][name]) and np.abs(c["a"][name]).max() > 1e-3
        assert np.isfinite(got).all(), name
        assert np.array_equal(got, want), f"{name}: max difference {np.abs(got - want).max():.3e}"
    for name in NAMES:  # the fields themselves are read only
        assert np.array_equal(from_dev(df[name]), c["poisoned"][name], equal_nan=True)


# ---- 7. the tuple path ---------------------------------------------------------------------------------------------------------------------
def tuple_inputs(g, seed):
    """test 7's inputs from a grid description alone (so that the seed can be chosen without a GPU): the random fields, and κ fields of
    ConvectiveAdjustmentVerticalDiffusivity from CAN.plateau_inputs (κᶜ: 0 / 1, κᵘ: 1e-2 / 0.5), x / y halos filled"""
    f, G, _ = random_inputs(g, seed)
    T, S = CAN.plateau_inputs(g, seed + 1)
    zeros = np.zeros(CAN.ccf_shape(g))
    kc, ku = CAN.diffusivities(g, SEAWATER, T, S, 1.0, 0.5, 0.0, 1e-2, zeros, zeros)
    return f, G, CAN.fill_xy_halos(g, kc), CAN.fill_xy_halos(g, ku)


@pytest.mark.parametrize("boundary_only", [0, 1], ids=["explicit", "boundary_only"])
def test_tuple_path_subtracts_the_sum_of_both_terms(ocn, boundary_only):
    """closure = (biharmonic, V): ocn_add_vertical_diffusivity_fluxes on zeroed scratch arrays leaves exactly 0 - b there, and
    ocn_add_biharmonic_fluxes with them as neg_other_* gives the restatement's G - (a + b) bit for bit -- which differs from (G - a) - b in
    the inputs chosen (asserted), so the test tells the two orders apart."""
    pg = _grid(ocn, *CASES[0])
    g, L = IDN.describe(pg), ocn._lib
    f, G, kc, ku = tuple_inputs(g, TUPLE_SEED)
    a_u, a_v, a_c = BHN.terms(g, NU, f["u"], f["v"], KAPPAS, [f["c"], f["c2"]])
    b_u, b_v, b_c = CAN.vertical_fluxes(g, ku, f["u"], f["v"], [kc, kc], [f["c"], f["c2"]], boundary_only)
    a = dict(u=a_u, v=a_v, c=a_c[0], c2=a_c[1])
    b = dict(u=b_u, v=b_v, c=b_c[0], c2=b_c[1])
    sl = BHN.interior(g)
    for name in NAMES:
        Gi = G[name][sl]
        assert np.any(Gi - (a[name] + b[name]) != (Gi - a[name]) - b[name]), name
        assert np.abs(b[name]).max() > 0
    df = {name: to_dev(ocn, pg, CC, f[name]) for name in NAMES}
    dG = {name: to_dev(ocn, pg, CC, G[name]) for name in NAMES}
    dS = {name: ocn.Field(CC, pg) for name in NAMES}
    dku, dkc = to_dev(ocn, pg, CCF, ku), to_dev(ocn, pg, CCF, kc)
    for S in dS.values():
        assert not S.data.any()
    L.call("ocn_add_vertical_diffusivity_fluxes", pg.cref, dku.ptr, df["u"].ptr, df["v"].ptr, dS["u"].ptr, dS["v"].ptr, 2,
           L.ptr_array([dkc.ptr, dkc.ptr]), L.ptr_array([df["c"].ptr, df["c2"].ptr]), L.ptr_array([dS["c"].ptr, dS["c2"].ptr]),
           int(boundary_only), None, 0)
    ocn.sync_device()
    zeros = np.zeros_like(G["u"])
    for name in NAMES:  # the scratch holds exactly -b
        assert np.array_equal(from_dev(dS[name]), BHN.subtract(g, zeros, b[name])), name
    _call(ocn, pg, NU, (df["u"], df["v"], dG["u"], dG["v"]), KAPPAS, [(df["c"], dG["c"]), (df["c2"], dG["c2"])], (dS["u"], dS["v"]),
          [dS["c"], dS["c2"]])
    for name in NAMES:
        got, want = from_dev(dG[name]), BHN.subtract(g, G[name], a[name], b[name])
        assert np.isfinite(got).all()
        assert np.array_equal(got, want), f"{name}: max difference {np.abs(got - want).max():.3e}"
        assert not np.array_equal(want, BHN.subtract(g, BHN.subtract(g, G[name], a[name]), b[name]))


# ---- 8. models against a twin ----------------------------------------------------------------------------------------------------------------
BIH = dict(ν=0.05, κ={"T": 0.02, "S": 0.04})
CAVD_COEFFS = dict(convective_κz=0.05, background_κz=1e-3, convective_νz=0.02, background_νz=1e-3)
DT = 0.05  # ν (4 / Δx² + 4 / Δy²)² Δt = 0.16; gravity waves: sqrt(g Lz) Δt / Δx = 0.16; convective_κz Δt / min Δz² = 0.21


def _model_grid(ocn, halo=(3, 3, 3)):
    return ocn.RectilinearGrid(ocn.GPU(), size=(13, 6, 4), x=(0, 13), y=(0, 6), z=stretched_faces(4), topology=(P, P, B), halo=halo)


def _free_surface(ocn, kind):
    return {"explicit": lambda: ocn.ExplicitFreeSurface(), "split": lambda: ocn.SplitExplicitFreeSurface(substeps=10),
            "implicit": lambda: ocn.ImplicitFreeSurface()}[kind]()


def _initial():
    """noise on everything, T falling towards the surface in the upper half (unstable there)"""
    rng = np.random.default_rng(9)
    zc = -1.0 + (np.arange(4) + 0.5) / 4
    T = 20 + np.where(zc < -0.5, 2.0 * (zc + 0.5), -1.5 * (zc + 0.5))
    init = {n: 0.1 * rng.uniform(-1, 1, (13, 6, 4)) for n in "uv"}
    init["T"] = np.broadcast_to(T, (13, 6, 4)) + 0.05 * rng.uniform(-1, 1, (13, 6, 4))
    init["S"] = 35 + 0.01 * rng.uniform(-1, 1, (13, 6, 4))
    return init


def _upload(field, a):
    import torch
    field.data.copy_(torch.from_numpy(np.ascontiguousarray(a.T)))


def _restate_closure_term(ocn, r, bih, vertical):
    """replace r.compute_tendencies (r: a model without the biharmonic closure, fused = False) by: the model's own launches -- without the
    add of its vertical closure V, if it has one --, then G - a, or G - (a + b), from the restatements on the host, then the boundary
    contributions, as hydrostatic.py orders them"""
    from oceananigans_jl_amd import models
    L, g, original = ocn._lib, IDN.describe(r.grid), r.compute_tendencies
    seen = dict(a=0.0, b=0.0, calls=0)

    def compute_tendencies(boundary_contributions=True):
        real_call = L.call
        L.call = lambda name, *args: None if name == "ocn_add_vertical_diffusivity_fluxes" else real_call(name, *args)
        try:
            original(boundary_contributions=False)
        finally:
            L.call = real_call
        Gn = r._nh.timestepper._Gn
        u, v, tracers = r.u.parent(), r.v.parent(), [c.parent() for c in r.tracers]
        a_u, a_v, a_c = BHN.terms(g, bih.nu, u, v, [bih.kappa_of(n) for n in r.tracer_names], tracers)
        bs = [None] * (2 + len(tracers))
        if vertical:
            d = r.diffusivity_fields
            b_u, b_v, b_c = CAN.vertical_fluxes(g, d["kappa_u"].parent(), u, v, [d["kappa_c"].parent()] * len(tracers), tracers, int(r._closure.implicit))
            bs = [b_u, b_v] + b_c
            seen["b"] = max(seen["b"], max(np.abs(x).max() for x in bs))
        for q, a, b in zip([0, 1] + [3 + n for n in range(len(tracers))], [a_u, a_v] + a_c, bs):
            _upload(Gn[q], BHN.subtract(g, Gn[q].parent(), a, b))
        seen["a"] = max(seen["a"], np.abs(a_u).max())
        seen["calls"] += 1
        if boundary_contributions:
            models.compute_boundary_tendency_contributions(r._nh)
    r.compute_tendencies = compute_tendencies
    return seen


def _run_against_twin(ocn, kind, vertical=None, timestepper="QuasiAdamsBashforth2", momentum_advection=None, tracer_advection="WENO",
                      halo=(3, 3, 3), order=0):
    """three steps of the model with the biharmonic closure (alone, or in a tuple with `vertical` in the given order) and of its twin"""
    bih = ocn.HorizontalScalarBiharmonicDiffusivity(**BIH)
    closure = bih if vertical is None else ((bih, vertical), (vertical, bih))[order]
    tracer_advection = ocn.WENO() if tracer_advection == "WENO" else tracer_advection
    bcs = lambda: {"T": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(1e-3))}
    kw = dict(tracers=("T", "S"), buoyancy=ocn.SeawaterBuoyancy(), coriolis=ocn.FPlane(f=1e-4), math_mode=ocn.MATH_STRICT,
              momentum_advection=momentum_advection, tracer_advection=tracer_advection, timestepper=timestepper)
    m = ocn.HydrostaticFreeSurfaceModel(_model_grid(ocn, halo), closure=closure, boundary_conditions=bcs(), free_surface=_free_surface(ocn, kind), **kw)
    assert m.fused is False and min(m.grid.Hx, m.grid.Hy, m.grid.Hz) >= 2
    assert m._nh._terms.closure == 0  # the container keeps the closure out of the terms
    if vertical is None:
        assert m.diffusivity_fields is None
    else:
        assert {"kappa_c", "kappa_u"} <= set(m.diffusivity_fields)  # V's dict
    r = ocn.HydrostaticFreeSurfaceModel(_model_grid(ocn, (m.grid.Hx, m.grid.Hy, m.grid.Hz)), closure=vertical, boundary_conditions=bcs(),
                                        free_surface=_free_surface(ocn, kind), fused=False, **kw)
    seen = _restate_closure_term(ocn, r, bih, vertical is not None)
    init = _initial()
    m.set(**init)
    r.set(**init)
    for step in range(3):
        m.time_step(DT)
        r.time_step(DT)
    ocn.sync_device()
    # (a vertically implicit V keeps only the fluxes through the bottom and the top in the tendencies, which the default conditions make 0)
    assert seen["calls"] >= 3 and seen["a"] > 1e-3 and (vertical is None or r._closure.implicit or seen["b"] > 1e-3)
    for name in ("u", "v", "w", "T", "S"):
        a, b = m.field(name).parent(), r.field(name).parent()
        assert np.isfinite(a).all(), name
        assert np.array_equal(a, b), f"{name}: max difference {np.abs(a - b).max():.3e}"
    assert np.array_equal(m.eta.cpu().numpy(), r.eta.cpu().numpy())
    for Gm_, Gr_ in zip(m._nh.timestepper._Gn, r._nh.timestepper._Gn):
        assert np.array_equal(Gm_.parent(), Gr_.parent())
    assert np.abs(m.u.interior()).max() > 0 and np.abs(m.eta.cpu().numpy()).max() > 0
    if vertical is not None:
        for name, field in m.diffusivity_fields.items():
            assert np.array_equal(field.parent(), r.diffusivity_fields[name].parent()), name
    return m


@pytest.mark.parametrize("kind", ["explicit", "split", "implicit"])
def test_hydrostatic_model_steps_equal_the_twin_with_the_restated_term(ocn, kind):
    """Three QAB2 steps on 13 x 6 x 4 with a stretched z, T and S, SeawaterBuoyancy, an FPlane, VectorInvariant() momentum and WENO() tracers
    with each free surface: u, v, w, η, the tracers and the tendencies bit for bit against closure = None plus G - a from the restatement
    at every compute_tendencies."""
    _run_against_twin(ocn, kind)


def test_hydrostatic_model_with_split_runge_kutta_3_equals_the_twin(ocn):
    _run_against_twin(ocn, "split", timestepper="SplitRungeKutta3")


def test_hydrostatic_model_with_flux_form_momentum_equals_the_twin(ocn):
    _run_against_twin(ocn, "explicit", momentum_advection=ocn.WENO())


def test_halo_is_inflated_to_two_from_a_halo_of_one(ocn):
    """Centered() tracers and VectorInvariant() momentum need a halo of 1: the closure's required_halo_size of 2 decides, in x, y and z"""
    m = _run_against_twin(ocn, "explicit", tracer_advection=None, halo=(1, 1, 1))
    assert (m.grid.Hx, m.grid.Hy, m.grid.Hz) == (2, 2, 2)


@pytest.mark.parametrize("order", [0, 1], ids=["biharmonic_first", "biharmonic_last"])
@pytest.mark.parametrize("which", ["cavd_implicit", "cavd_explicit", "ri_based"])
def test_closure_tuple_steps_equal_the_twin_with_the_restated_sum(ocn, which, order):
    """closure = (biharmonic, V) and (V, biharmonic): three QAB2 steps against the twin with V alone whose own add is replaced by the
    restatement's G - (a + b); V's diffusivity fields (computed on the device in both) agree as well"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)  # (RiBasedVerticalDiffusivity says that it is experimental)
        V_ = {"cavd_implicit": lambda: ocn.ConvectiveAdjustmentVerticalDiffusivity(**CAVD_COEFFS),
              "cavd_explicit": lambda: ocn.ConvectiveAdjustmentVerticalDiffusivity("Explicit", **CAVD_COEFFS),
              "ri_based": lambda: ocn.RiBasedVerticalDiffusivity()}[which]()
        m = _run_against_twin(ocn, "split", vertical=V_, order=order)
    assert m.closure[order] is not V_ and m.closure[1 - order] is V_
    assert m._closure.implicit == (which != "cavd_explicit")


# ---- 9. a property of the device result ------------------------------------------------------------------------------------------------------
def test_grid_scale_modes_decay_at_the_rate_of_their_eigenvalue(ocn):
    """Ten QAB2 steps with nothing but the closure at work: no buoyancy, no Coriolis, v = 0 and u = u(y) (no divergence: w and η stay 0
    exactly) at an amplitude of 2^-100, so that the quadratic terms of the momentum equations and the advection of T fall far below the
    rounding of the closure term (floating point is scale-free).  u holds a grid-scale wave in y plus the gravest one, T a checkerboard in
    x and y plus the gravest wave in x on a background of 20.  Every mode must follow the forward-Euler / AB2 recursion of its eigenvalue
    ν λ²: the grid-scale ones fall to less than 0.55, the smooth ones keep more than 0.99.  Tolerance per mode: 10 steps of (1.5 + χ) +
    (0.5 + χ) times Δt times BHN.bound for the term, 5 eps for the arithmetic of a step, and Nx Ny eps for the projection's sum.  The
    horizontal sum of T stays to BHN.OPERATIONS eps Σ|T|."""
    Nx, Ny, Nz, steps, dt = 16, 12, 3, 10, 0.1
    pg = ocn.RectilinearGrid(ocn.GPU(), size=(Nx, Ny, Nz), x=(0, Nx), y=(0, Ny), z=(-1, 0), topology=(P, P, B), halo=(3, 3, 3))
    nu, kappa = 4.0e-2, 2.0e-2
    m = ocn.HydrostaticFreeSurfaceModel(pg, closure=ocn.HorizontalScalarBiharmonicDiffusivity(ν=nu, κ=kappa), tracers=("T",),
                                        free_surface=ocn.ExplicitFreeSurface(), math_mode=ocn.MATH_STRICT)
    g = IDN.describe(m.grid)
    i, j = np.arange(Nx)[:, None, None], np.arange(Ny)[None, :, None]
    one = np.ones((Nx, Ny, Nz))
    A = 2.0 ** -100
    modes_u = {"grid": ((-1.0) ** j * one, BHN.eigenvalue(g, 0, Ny // 2)), "smooth": (np.cos(2 * np.pi * (j + 0.5) / Ny) * one, BHN.eigenvalue(g, 0, 1))}
    modes_T = {"grid": ((-1.0) ** (i + j) * one, BHN.eigenvalue(g, Nx // 2, Ny // 2)),
               "smooth": (np.cos(2 * np.pi * (i + 0.5) / Nx) * one, BHN.eigenvalue(g, 1, 0))}
    u0 = A * (modes_u["grid"][0] + 0.5 * modes_u["smooth"][0])
    T0 = 20.0 + modes_T["grid"][0] + 0.5 * modes_T["smooth"][0]
    m.set(u=u0, T=T0)
    for _ in range(steps):
        m.time_step(dt)
    ocn.sync_device()
    # what the quadratic terms left in v, w and η is of the order of A², far below the rounding of u
    for other in (m.v.parent(), m.w.parent(), m.eta.cpu().numpy()):
        assert np.abs(other).max() <= A * EPS
    chi = m._nh.timestepper.chi

    def recursion(mu):
        a = [1.0, 1.0 - dt * mu]
        for _ in range(steps - 1):
            a.append(a[-1] - dt * mu * ((1.5 + chi) * a[-1] - (0.5 + chi) * a[-2]))
        return a[-1]

    for field, modes, coefficient, start, scale in ((m.u.interior()[:, :, :Nz], modes_u, nu, u0, A), (m.field("T").interior(), modes_T, kappa, T0, 1.0)):
        assert np.isfinite(field).all()
        tol = steps * (((1.5 + chi) + (0.5 + chi)) * dt * BHN.bound(g, coefficient, np.abs(start).max()) + 5 * EPS * np.abs(start).max()) \
            + Nx * Ny * EPS * np.abs(start).max()
        for name, (mode, lam) in modes.items():
            amplitude = lambda a: (a * mode).sum() / (mode * mode).sum()
            want = recursion(coefficient * lam ** 2) * amplitude(start)
            got = amplitude(field)
            print(f"{name}: eigenvalue {coefficient * lam ** 2:.3e}, amplitude / initial {got / amplitude(start):.6f}, error {abs(got - want) / scale:.2e}, "
                  f"tolerance {tol / scale:.2e}")
            assert abs(got - want) <= tol, name
            assert (got / amplitude(start) < 0.55) if name == "grid" else (got / amplitude(start) > 0.99)
    T = m.field("T").interior()
    for k in range(Nz):
        assert abs(T[:, :, k].sum() - T0[:, :, k].sum()) <= BHN.OPERATIONS * EPS * np.abs(T0[:, :, k]).sum()
