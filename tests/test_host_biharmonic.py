"""HorizontalScalarBiharmonicDiffusivity without a GPU: the constructor and the refusals (before any allocation), the argument checks of
ocn_add_biharmonic_fluxes (no device is touched), and the NumPy restatement (tests/biharmonic_numpy.py) pinned independently of its author:
against the closed form of the operator on Fourier modes, and against the properties of a flux divergence that dissipates."""
import ctypes as C

import numpy as np
import pytest

import biharmonic_numpy as BHN
import implicit_diffusion_numpy as IDN
from helpers import stretched_faces

P, B, F = "Periodic", "Bounded", "Flat"
INVALID = -1  # OCN_ERR_INVALID_ARGUMENT (include/ocn_hip.h)
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def pkg():
    import oceananigans_jl_amd as ocn
    return ocn


def _grid(pkg, topo=(P, P, B), size=(4, 5, 6), z=(-1, 0), halo=None):
    return pkg.RectilinearGrid(None, size=size, x=(0, 1), y=(0, 1), z=z, topology=topo, halo=halo or (3, 3, min(3, size[2])))


def _no_alloc(monkeypatch):
    import oceananigans_jl_amd.fields as fields

    def no_alloc(*a, **k):
        raise AssertionError("a field was allocated before the refusal")
    monkeypatch.setattr(fields.Field, "__init__", no_alloc)


# ---- 1. constructor ------------------------------------------------------------------------------------------------------------------------
def test_constructor_mirrors_the_reference(pkg):
    SBD, HSBD, HF = pkg.ScalarBiharmonicDiffusivity, pkg.HorizontalScalarBiharmonicDiffusivity, pkg.HorizontalFormulation
    c = HSBD(ν=2.5, κ=1e-3)
    assert isinstance(c, SBD) and isinstance(c.formulation, HF)
    assert c == SBD(HF(), ν=2.5, κ=1e-3) == SBD("Horizontal", nu=2.5, kappa=1e-3) == SBD(formulation=HF, ν=2.5, kappa=1e-3)
    assert c != HSBD(ν=2.5, κ=2e-3)
    assert (c.nu, c.ν, c.kappa, c.κ) == (2.5, 2.5, 1e-3, 1e-3) and c.kappa_of("T") == 1e-3 and c.kappa_of("anything") == 1e-3
    assert (HSBD().nu, HSBD().kappa_of("T")) == (0.0, 0.0)  # the reference's defaults
    assert c.required_halo_size == 2
    assert isinstance(c.time_discretization, pkg.ExplicitTimeDiscretization)  # always (abstract_scalar_biharmonic_diffusivity_closure.jl:8)
    from oceananigans_jl_amd.physics import has_diffusivity_fields, is_vertically_implicit, owns_eddy_fields
    assert not is_vertically_implicit(c) and not owns_eddy_fields(c) and not has_diffusivity_fields(c)
    d = HSBD(ν=1, κ={"T": 1e-3, "S": np.float64(2e-3)})
    assert d.kappa_of("T") == 1e-3 and d.kappa_of("S") == 2e-3
    with pytest.raises(ValueError, match="no diffusivity κ given for tracer b"):
        d.kappa_of("b")
    # the reference's summary
    assert repr(c) == "ScalarBiharmonicDiffusivity{HorizontalFormulation}(ν=2.5, κ=0.001)"
    assert repr(HSBD(ν=1e10)) == "ScalarBiharmonicDiffusivity{HorizontalFormulation}(ν=1.0e10, κ=0.0)"
    assert repr(d) == "ScalarBiharmonicDiffusivity{HorizontalFormulation}(ν=1.0, κ=(T=0.001, S=0.002))"
    assert repr(HF()) == "HorizontalFormulation()"


def test_what_is_not_implemented_says_so(pkg):
    SBD, HSBD = pkg.ScalarBiharmonicDiffusivity, pkg.HorizontalScalarBiharmonicDiffusivity
    with pytest.raises(NotImplementedError, match="ThreeDimensionalFormulation"):
        SBD(ν=1)  # the reference's default formulation
    for formulation, name in ((pkg.ThreeDimensionalFormulation(), "ThreeDimensionalFormulation"), ("Vertical", "VerticalFormulation"),
                              (pkg.VerticalFormulation, "VerticalFormulation"),
                              (pkg.HorizontalDivergenceFormulation(), "HorizontalDivergenceFormulation"),
                              ("HorizontalDivergence", "HorizontalDivergenceFormulation")):
        with pytest.raises(NotImplementedError, match="the " + name):
            SBD(formulation, ν=1)
    with pytest.raises(ValueError, match="formulation must be"):
        SBD("Diagonal")
    for bad in (lambda x, y, z, t: 1.0, np.ones(3), np.ones((2, 2, 2)), "1", True):
        for name in ("ν", "nu", "κ", "kappa"):
            with pytest.raises(NotImplementedError, match="must be a number"):
                HSBD(**{name: bad})
    with pytest.raises(NotImplementedError, match="must be a number"):
        HSBD(κ={"T": lambda x, y, z, t: 1.0})
    with pytest.raises(NotImplementedError, match="discrete_form"):
        HSBD(ν=1, discrete_form=True)
    with pytest.raises(NotImplementedError, match="loc"):
        HSBD(ν=1, loc=(pkg.Center, pkg.Center, pkg.Center))
    with pytest.raises(NotImplementedError, match="parameters"):
        HSBD(ν=1, parameters={"a": 1})
    with pytest.raises(NotImplementedError, match="required_halo_size"):
        HSBD(ν=1, required_halo_size=3)
    HSBD(ν=1, discrete_form=False, loc=(None, None, None), parameters=None, required_halo_size=2)  # the defaults, spelled out
    with pytest.raises(TypeError, match="twice"):
        HSBD(ν=1, nu=1)
    with pytest.raises(TypeError, match="unexpected"):
        HSBD(viscosity=1)
    # ScalarDiffusivity keeps refusing a formulation
    with pytest.raises(NotImplementedError, match="ThreeDimensionalFormulation"):
        pkg.ScalarDiffusivity(ν=1, formulation="Horizontal")


# ---- 2. models -----------------------------------------------------------------------------------------------------------------------------
class _FakeDistributed:  # what the models ask of a Distributed architecture
    partition = object()
    communicates = True


def test_model_refusals_come_before_any_allocation_and_the_tuples_pass_validation(pkg, monkeypatch):
    _no_alloc(monkeypatch)
    HSBD, CAVD, RI = pkg.HorizontalScalarBiharmonicDiffusivity, pkg.ConvectiveAdjustmentVerticalDiffusivity, pkg.RiBasedVerticalDiffusivity
    g = _grid(pkg)
    bih = HSBD(ν=1e-3, κ=1e-4)
    hydro = lambda closure, **kw: pkg.HydrostaticFreeSurfaceModel(g, closure=closure, **{"free_surface": pkg.ExplicitFreeSurface(), **kw})
    with pytest.raises(NotImplementedError, match="ScalarBiharmonicDiffusivity on NonhydrostaticModel"):
        pkg.NonhydrostaticModel(g, advection=pkg.WENO(), closure=bih)
    with pytest.raises(NotImplementedError, match=r"runs the reference's launch sequence \(fused = False\)"):
        hydro(bih, fused=True)
    gs = _grid(pkg)
    gs.architecture = _FakeDistributed()
    gs.topology = (pkg.FullyConnected, P, B)
    with pytest.raises(NotImplementedError, match="Distributed"):
        pkg.HydrostaticFreeSurfaceModel(gs, closure=bih, free_surface=pkg.SplitExplicitFreeSurface(substeps=10))
    vertical = (CAVD(convective_κz=1), CAVD("Explicit", convective_κz=1), RI(), RI("Explicit"))
    refused = [(bih,), [bih], (bih, pkg.ScalarDiffusivity(ν=1e-2)), (pkg.ScalarDiffusivity(ν=1e-2), bih), (bih, pkg.AnisotropicMinimumDissipation()),
               (bih, pkg.SmagorinskyLilly()), (bih, vertical[0], vertical[2]), (bih, vertical[0], pkg.ScalarDiffusivity(ν=1)), (bih, HSBD(κ=1)),
               (vertical[0], vertical[2]), (vertical[0],), ()]
    for closure in refused:
        with pytest.raises(NotImplementedError, match="closure tuples"):
            hydro(closure)
        with pytest.raises(NotImplementedError):
            pkg.NonhydrostaticModel(g, advection=pkg.WENO(), closure=closure)
    # what is accepted gets as far as allocating its fields
    accepted = [bih] + [(bih, V) for V in vertical] + [(V, bih) for V in vertical] + [[bih, vertical[0]]]
    for closure in accepted:
        with pytest.raises(AssertionError, match="a field was allocated"):
            hydro(closure, tracers=("T", "S"), buoyancy=pkg.SeawaterBuoyancy())
        with pytest.raises(NotImplementedError):
            pkg.NonhydrostaticModel(g, advection=pkg.WENO(), closure=closure)
    for fs in (pkg.SplitExplicitFreeSurface(substeps=10), pkg.ImplicitFreeSurface()):
        with pytest.raises(AssertionError, match="a field was allocated"):
            hydro(bih, free_surface=fs)
    with pytest.raises(AssertionError, match="a field was allocated"):
        hydro(bih, free_surface=pkg.SplitExplicitFreeSurface(substeps=10), timestepper="SplitRungeKutta3")
    # the constraints of the vertical closure apply to the tuple
    for V in vertical:
        with pytest.raises(NotImplementedError, match="fused = False"):
            hydro((bih, V), fused=True)
        with pytest.raises(NotImplementedError, match="SplitRungeKutta3"):
            hydro((V, bih), free_surface=pkg.SplitExplicitFreeSurface(substeps=10), timestepper="SplitRungeKutta3")


# ---- 3. C ABI: argument checks before any HIP call ---------------------------------------------------------------------------------------------
def test_c_abi_argument_checks_touch_no_device(pkg):
    lib, L = pkg._lib.lib(), pkg._lib
    fn = lib.ocn_add_biharmonic_fluxes
    g = _grid(pkg, size=(16, 16, 8))
    p = [C.c_void_p(8 * q) for q in range(1, 12)]  # never dereferenced
    u, v, Gu, Gv, c1, c2, G1, G2, Su, Sv, S1 = p
    kap = (C.c_double * 5)(1.0, 2.0, 0.0, 0.0, 0.0)
    cs, Gs = L.ptr_array([c1, c2]), L.ptr_array([G1, G2])
    ok_momentum = (1.0, u, v, Gu, Gv)
    ok_tracers = (2, kap, cs, Gs)
    none3 = (None, None, None, None)

    def refused(grid, *args, say=None):
        assert fn(grid.cref if grid is not None else None, *args) == INVALID
        if say is not None:
            assert say in lib.ocn_last_error(), lib.ocn_last_error()

    refused(None, *ok_momentum, *ok_tracers, *none3)
    for topo in ((B, P, B), (P, B, B)):
        refused(_grid(pkg, topo=topo, size=(16, 16, 8)), *ok_momentum, *ok_tracers, *none3, say=b"must be Periodic")
    refused(pkg.RectilinearGrid(None, size=(16, 8), x=(0, 1), z=(-1, 0), topology=(P, F, B), halo=(3, 3)), *ok_momentum, *ok_tracers, *none3,
            say=b"must be Periodic")
    refused(_grid(pkg, size=(16, 16, 8), halo=(1, 3, 3)), *ok_momentum, *ok_tracers, *none3, say=b"halo >= 2")
    refused(_grid(pkg, size=(16, 16, 8), halo=(2, 1, 3)), *ok_momentum, *ok_tracers, *none3, say=b"halo >= 2")
    refused(g, 1.0, u, v, None, Gv, *ok_tracers, *none3, say=b"null field pointer")
    refused(g, 1.0, u, None, Gu, Gv, *ok_tracers, *none3, say=b"null field pointer")
    refused(g, 1.0, None, v, Gu, Gv, *ok_tracers, *none3, say=b"u is NULL")
    refused(g, 1.0, None, None, None, None, 2, kap, cs, Gs, Su, None, None, None, say=b"u is NULL")
    refused(g, 1.0, None, None, None, None, 0, None, None, None, *none3, say=b"nothing to do")
    refused(g, *ok_momentum, 5, kap, cs, Gs, *none3, say=b"number of tracers")  # OCN_MODEL_MAX_TRACERS + 1
    refused(g, *ok_momentum, -1, kap, cs, Gs, *none3, say=b"number of tracers")
    refused(g, *ok_momentum, 2, None, cs, Gs, *none3, say=b"null tracer array")
    refused(g, *ok_momentum, 2, kap, L.ptr_array([c1, None]), Gs, *none3, say=b"tracer 1: null pointer")
    refused(g, -1.0, u, v, Gu, Gv, *ok_tracers, *none3, say=b"nu =")
    refused(g, float("nan"), u, v, Gu, Gv, *ok_tracers, *none3, say=b"nu =")
    refused(g, *ok_momentum, 2, (C.c_double * 2)(1.0, float("inf")), cs, Gs, *none3, say=b"kappa =")
    # aliases
    refused(g, 1.0, u, u, Gu, Gv, *ok_tracers, *none3, say=b"u and v are the same")
    refused(g, 1.0, u, v, Gu, Gu, *ok_tracers, *none3, say=b"same array")
    refused(g, 1.0, u, v, u, Gv, *ok_tracers, *none3, say=b"is u or v")
    refused(g, *ok_momentum, 2, kap, cs, L.ptr_array([G1, c1]), *none3, say=b"is tracer 0")
    refused(g, *ok_momentum, 2, kap, cs, L.ptr_array([G1, G1]), *none3, say=b"same array")
    refused(g, *ok_momentum, *ok_tracers, Gu, Sv, None, None, say=b"same array")
    refused(g, *ok_momentum, *ok_tracers, Su, Sv, L.ptr_array([S1, Su]), None, say=b"same array")
    refused(g, *ok_momentum, *ok_tracers, Su, Sv, L.ptr_array([S1, c2]), None, say=b"is tracer 1")


# ---- 4. the restatement against closed forms ---------------------------------------------------------------------------------------------------
def _mode_grid(pkg, z):
    return pkg.RectilinearGrid(None, size=(16, 12, 3), x=(0, 2.0), y=(0, 3.0), z=z, topology=(P, P, B), halo=(3, 3, 3))


def _mode(g, m, n, face_x=False, face_y=False):
    """cos(2π m x / Lx) cos(2π n y / Ly) on the parent array of a field whose x / y nodes are faces or centres, the same on every plane"""
    i = np.arange(-g.Hx, g.Nx + g.Hx) + (0.0 if face_x else 0.5)
    j = np.arange(-g.Hy, g.Ny + g.Hy) + (0.0 if face_y else 0.5)
    plane = np.cos(2 * np.pi * m * i / g.Nx)[:, None] * np.cos(2 * np.pi * n * j / g.Ny)[None, :]
    return np.repeat(plane[:, :, None], g.Nz + 2 * g.Hz, axis=2)


@pytest.mark.parametrize("z", ["uniform", "stretched"])
@pytest.mark.parametrize("m,n", [(1, 0), (0, 1), (2, 3), (8, 6), (8, 0), (5, 6)])
def test_restatement_gives_the_closed_form_on_fourier_modes(pkg, z, m, n):
    """u = cos(2π m x / Lx) cos(2π n y / Ly) with v = 0 gives a_u = ν λ² u, λ = 4 / Δx² sin²(π m / Nx) + 4 / Δy² sin²(π n / Ny) (and a_v = ν times
    a cross term that vanishes: ∂x ∂y of δ★ and ζ★ cancel); alike for v with u = 0 and for a tracer with κ.  Bound: BHN.bound, 32 eps ν
    (4 / Δx² + 4 / Δy²)² max|u| -- 25 rounded operations counted in tests/biharmonic_numpy.py plus 7 for the rounded inputs and closed form; on
    the stretched z every plane meets the same bound (Δz cancels up to rounding, which the count includes: the metric roundings)."""
    g = IDN.describe(_mode_grid(pkg, (-1, 0) if z == "uniform" else stretched_faces(3)))
    nu, kappa = 3.0e-3, 7.0e-4
    lam = BHN.eigenvalue(g, m, n)
    sl = BHN.interior(g)
    zero = np.zeros((g.Nx + 2 * g.Hx, g.Ny + 2 * g.Hy, g.Nz + 2 * g.Hz))
    u = _mode(g, m, n, face_x=True)
    a_u, a_v = BHN.momentum_terms(g, nu, u, zero)
    tol = BHN.bound(g, nu, 1.0)
    assert np.abs(a_u - nu * lam ** 2 * u[sl]).max() <= tol and np.abs(a_v).max() <= tol
    if (m, n) == (8, 0):  # a grid-scale wave in x (±1 at the u nodes): the x half of the operator norm
        assert np.abs(a_u).max() > 0.99 * nu * (4 / g.dx ** 2) ** 2
    v = _mode(g, m, n, face_y=True)
    a_u, a_v = BHN.momentum_terms(g, nu, zero, v)
    assert np.abs(a_v - nu * lam ** 2 * v[sl]).max() <= tol and np.abs(a_u).max() <= tol
    c = _mode(g, m, n)
    a_c = BHN.tracer_term(g, kappa, c)
    assert np.abs(a_c - kappa * lam ** 2 * c[sl]).max() <= BHN.bound(g, kappa, 1.0)


# ---- 5. properties of the restatement on random inputs -------------------------------------------------------------------------------------
@pytest.mark.parametrize("z", ["uniform", "stretched"])
def test_restatement_is_a_flux_divergence_that_dissipates(pkg, z):
    """On random periodic fields: Σ V a vanishes for a_c, a_u and a_v to OPERATIONS eps Σ|V a| (a flux divergence on a periodic plane
    telescopes), and Σ V (u a_u + v a_v) >= 0, Σ V c a_c >= 0 (ν ∇²h ∇²h is positive semi-definite)."""
    pg = pkg.RectilinearGrid(None, size=(13, 6, 4), x=(0, 1.3), y=(0, 0.9), z=(-1, 0) if z == "uniform" else stretched_faces(4),
                             topology=(P, P, B), halo=(2, 2, 2))
    g = IDN.describe(pg)
    rng = np.random.default_rng(11)
    pad = lambda a: np.pad(np.pad(a, ((g.Hx, g.Hx), (g.Hy, g.Hy), (0, 0)), mode="wrap"), ((0, 0), (0, 0), (g.Hz, g.Hz)), constant_values=np.nan)
    u, v, c = (pad(rng.uniform(-1, 1, (g.Nx, g.Ny, g.Nz))) for _ in range(3))  # (NaN above and below: no plane but its own is read)
    a_u, a_v, (a_c,) = BHN.terms(g, 2.0e-5, u, v, [3.0e-5], [c])
    V, sl = BHN.volumes(g), BHN.interior(g)
    for a in (a_u, a_v, a_c):
        assert np.isfinite(a).all() and np.abs(a).max() > 0
        for k in range(g.Nz):  # plane by plane: the term is horizontal
            assert abs((V * a)[:, :, k].sum()) <= BHN.OPERATIONS * EPS * np.abs(V * a)[:, :, k].sum()
    assert (V * (u[sl] * a_u + v[sl] * a_v)).sum() > 0 and (V * c[sl] * a_c).sum() > 0
    # ... and the order of a tuple's sum matters in floating point: G - (a + b) is not (G - a) - b everywhere
    G, b = rng.uniform(-1, 1, a_c.shape), rng.uniform(-1, 1, a_c.shape)
    assert np.any(G - (a_c + b) != (G - a_c) - b)
