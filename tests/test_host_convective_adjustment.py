"""ConvectiveAdjustmentVerticalDiffusivity without a GPU: the constructor and the refusals (before any allocation), the argument checks of the
three C entry points (no device is touched), and the NumPy restatement (tests/convective_adjustment_numpy.py) pinned independently of its
author: its variable-coefficient solve against numpy.linalg.solve of the dense matrix it assembles, its rows against conservation, its
matrix against the constant-κ one of tests/implicit_diffusion_numpy.py, and its classification of stable, unstable and neutral faces."""
import ctypes as C

import numpy as np
import pytest

import convective_adjustment_numpy as CAN
import implicit_diffusion_numpy as IDN
from helpers import stretched_faces

P, B, F = "Periodic", "Bounded", "Flat"
INVALID = -1  # OCN_ERR_INVALID_ARGUMENT (include/ocn_hip.h)
SEAWATER = ("SeawaterBuoyancy", 9.80665, 1.67e-4, 7.80e-4)


@pytest.fixture(scope="module")
def pkg():
    import oceananigans_jl_amd as ocn
    return ocn


def _grid(pkg, topo=(P, P, B), size=(4, 5, 6), z=(-1, 0)):
    # (a halo is at most the size: Nz = 1, 2 take Hz = Nz)
    return pkg.RectilinearGrid(None, size=size, x=(0, 1), y=(0, 1), z=z, topology=topo, halo=(3, 3, min(3, size[2])))


def _no_alloc(monkeypatch):
    import oceananigans_jl_amd.fields as fields

    def no_alloc(*a, **k):
        raise AssertionError("a field was allocated before the refusal")
    monkeypatch.setattr(fields.Field, "__init__", no_alloc)


# ---- constructor -------------------------------------------------------------------------------------------------------------------------
def test_constructor_mirrors_the_reference(pkg):
    VI, EX = pkg.VerticallyImplicitTimeDiscretization, pkg.ExplicitTimeDiscretization
    CAVD = pkg.ConvectiveAdjustmentVerticalDiffusivity
    c = CAVD()
    assert isinstance(c.time_discretization, VI)  # the reference's default (convective_adjustment_vertical_diffusivity.jl:62)
    assert (c.convective_kappa_z, c.convective_nu_z, c.background_kappa_z, c.background_nu_z) == (0.0, 0.0, 0.0, 0.0)
    for c in (CAVD(convective_κz=1, convective_νz=0.5, background_κz=1e-3, background_νz=1e-2),
              CAVD(VI(), convective_kappa_z=1, convective_nu_z=0.5, background_kappa_z=1e-3, background_nu_z=1e-2),
              CAVD("VerticallyImplicit", convective_κz=1, convective_nu_z=0.5, background_κz=1e-3, background_nu_z=1e-2),
              CAVD(time_discretization=VI, convective_κz=np.float64(1), convective_νz=0.5, background_κz=1e-3, background_νz=1e-2)):
        assert isinstance(c.time_discretization, VI)
        assert (c.convective_κz, c.convective_νz, c.background_κz, c.background_νz) == (1.0, 0.5, 1e-3, 1e-2)
        s = c.c_struct()
        assert (s.convective_kappa_z, s.convective_nu_z, s.background_kappa_z, s.background_nu_z) == (1.0, 0.5, 1e-3, 1e-2)
    for c in (CAVD(EX(), convective_κz=1), CAVD("Explicit", convective_κz=1), CAVD(time_discretization=EX(), convective_κz=1)):
        assert isinstance(c.time_discretization, EX) and c.convective_kappa_z == 1.0
    from oceananigans_jl_amd.physics import is_vertically_implicit, owns_eddy_fields
    assert is_vertically_implicit(CAVD()) and not is_vertically_implicit(CAVD(EX()))
    assert not owns_eddy_fields(CAVD())
    # the reference's summary (its docstring example: an integer prints as it was given)
    assert repr(CAVD(convective_κz=1)) == ("ConvectiveAdjustmentVerticalDiffusivity{VerticallyImplicitTimeDiscretization}"
                                           "(background_κz=0.0 convective_κz=1 background_νz=0.0 convective_νz=0.0)")
    assert repr(CAVD(EX())).startswith("ConvectiveAdjustmentVerticalDiffusivity{ExplicitTimeDiscretization}(")


def test_what_is_not_implemented_says_so(pkg):
    CAVD, VI = pkg.ConvectiveAdjustmentVerticalDiffusivity, pkg.VerticallyImplicitTimeDiscretization
    for bad in (lambda x, y, z, t: 1.0, np.ones(3), (1.0, 2.0), {"T": 1.0}, "1"):
        for name in ("convective_κz", "convective_nu_z", "background_kappa_z", "background_νz"):
            with pytest.raises(NotImplementedError, match="must be a number"):
                CAVD(**{name: bad})
    with pytest.raises(TypeError, match="twice"):
        CAVD(VI(), time_discretization=VI())
    with pytest.raises(TypeError, match="twice"):
        CAVD(convective_κz=1, convective_kappa_z=1)
    with pytest.raises(TypeError, match="unexpected"):
        CAVD(kappa=1)
    with pytest.raises(TypeError, match="one positional"):
        CAVD(VI(), 1.0)
    with pytest.raises(ValueError, match="time_discretization"):
        CAVD("Implicit")


def test_model_refusals_come_before_any_allocation(pkg, monkeypatch):
    _no_alloc(monkeypatch)
    CAVD = pkg.ConvectiveAdjustmentVerticalDiffusivity
    g = _grid(pkg)
    for closure in (CAVD(convective_κz=1), CAVD("Explicit", convective_κz=1)):
        with pytest.raises(NotImplementedError, match="ConvectiveAdjustmentVerticalDiffusivity on NonhydrostaticModel"):
            pkg.NonhydrostaticModel(g, advection=pkg.WENO(), tracers=("b",), buoyancy=pkg.BuoyancyTracer(), closure=closure)
        with pytest.raises(NotImplementedError, match="fused = False"):
            pkg.HydrostaticFreeSurfaceModel(g, closure=closure, free_surface=pkg.ExplicitFreeSurface(), fused=True)
        with pytest.raises(NotImplementedError, match="SplitRungeKutta3"):
            pkg.HydrostaticFreeSurfaceModel(g, closure=closure, free_surface=pkg.SplitExplicitFreeSurface(substeps=10), timestepper="SplitRungeKutta3")
        with pytest.raises(NotImplementedError, match="closure tuples"):
            pkg.HydrostaticFreeSurfaceModel(g, closure=(closure, pkg.ScalarDiffusivity(ν=1e-2)), free_surface=pkg.ExplicitFreeSurface())
        with pytest.raises(NotImplementedError):
            pkg.NonhydrostaticModel(g, advection=pkg.WENO(), closure=(closure,))

        class FakeDistributed:  # what the models ask of a Distributed architecture
            partition = object()
            communicates = True
        gs = _grid(pkg)
        gs.architecture = FakeDistributed()
        gs.topology = (pkg.FullyConnected, P, B)
        with pytest.raises(NotImplementedError, match="Distributed"):
            pkg.HydrostaticFreeSurfaceModel(gs, closure=closure, free_surface=pkg.SplitExplicitFreeSurface(substeps=10))


# ---- C ABI: argument checks before any HIP call ------------------------------------------------------------------------------------------
def test_c_abi_argument_checks_touch_no_device(pkg):
    lib, L = pkg._lib.lib(), pkg._lib
    g = _grid(pkg, size=(16, 16, 8))
    one, two, three = C.c_void_p(8), C.c_void_p(16), C.c_void_p(24)  # never dereferenced
    bad_grids = (_grid(pkg, topo=(P, P, P)), pkg.RectilinearGrid(None, size=(16, 16), x=(0, 1), y=(0, 1), topology=(P, P, F), halo=(3, 3)))
    thin = pkg.RectilinearGrid(None, size=(16, 16, 8), x=(0, 1), y=(0, 1), z=(-1, 0), topology=(P, P, B), halo=(3, 3, 0))
    slice_xz = pkg.RectilinearGrid(None, size=(16, 8), x=(0, 1), z=(-1, 0), topology=(P, F, B), halo=(3, 3))

    # (a) the diffusivities
    compute = lib.ocn_compute_convective_adjustment_diffusivities
    terms = L.CModelTerms()
    cl = L.CConvectiveAdjustment(1.0, 0.5, 1e-3, 1e-2)
    for bad in bad_grids:
        assert compute(bad.cref, C.byref(terms), C.byref(cl), one, two, None) == INVALID
        assert b"Bounded in the z-direction" in lib.ocn_last_error()
    assert compute(thin.cref, C.byref(terms), C.byref(cl), one, two, None) == INVALID and b"halo" in lib.ocn_last_error()
    assert compute(slice_xz.cref, C.byref(terms), C.byref(cl), one, two, None) == INVALID and b"Flat x or y" in lib.ocn_last_error()
    assert compute(None, C.byref(terms), C.byref(cl), one, two, None) == INVALID
    assert compute(g.cref, None, C.byref(cl), one, two, None) == INVALID and b"null terms" in lib.ocn_last_error()
    assert compute(g.cref, C.byref(terms), None, one, two, None) == INVALID
    assert compute(g.cref, C.byref(terms), C.byref(cl), None, two, None) == INVALID and b"null field pointer" in lib.ocn_last_error()
    assert compute(g.cref, C.byref(terms), C.byref(cl), one, None, None) == INVALID
    assert compute(g.cref, C.byref(terms), C.byref(cl), one, one, None) == INVALID and b"same array" in lib.ocn_last_error()
    for kind, wording in ((L.BUOYANCY_TRACER, b"T (or b) tracer is NULL"), (L.BUOYANCY_SEAWATER_TS, b"tracer is NULL"),
                          (L.BUOYANCY_SEAWATER_S, b"S tracer is NULL"), (9, b"unknown buoyancy")):
        t = L.CModelTerms()
        t.buoyancy = kind
        assert compute(g.cref, C.byref(t), C.byref(cl), one, two, None) == INVALID and wording in lib.ocn_last_error()
    for bad in (float("nan"), float("inf")):
        assert compute(g.cref, C.byref(terms), C.byref(L.CConvectiveAdjustment(1.0, bad, 0.0, 0.0)), one, two, None) == INVALID
        assert b"finite" in lib.ocn_last_error()

    # (b) the implicit step
    step = lib.ocn_implicit_vertical_diffusion_step_fields
    ok = (1, L.ptr_array([8]), L.i32_array([L.LOC_CCC]), L.ptr_array([16]), L.ptr_array([24]), 0.1, None)
    for bad in bad_grids:
        assert step(bad.cref, *ok) == INVALID and b"Bounded in the z-direction" in lib.ocn_last_error()
    assert step(thin.cref, *ok) == INVALID and b"halo" in lib.ocn_last_error()
    assert step(None, *ok) == INVALID
    assert step(g.cref, 0, *ok[1:]) == INVALID and b"number of fields" in lib.ocn_last_error()
    assert step(g.cref, 9, *ok[1:]) == INVALID
    for q in (1, 2, 3, 4):  # fields, locs, kappa, scratch
        args = list(ok)
        args[q] = None
        assert step(g.cref, *args) == INVALID and b"null tuple pointer" in lib.ocn_last_error()
    assert step(g.cref, 1, L.ptr_array([None]), *ok[2:]) == INVALID and b"null pointer" in lib.ocn_last_error()
    assert step(g.cref, 1, ok[1], ok[2], L.ptr_array([None]), *ok[4:]) == INVALID and b"null pointer" in lib.ocn_last_error()
    assert step(g.cref, 1, ok[1], ok[2], ok[3], L.ptr_array([None]), 0.1, None) == INVALID and b"scratch array is NULL" in lib.ocn_last_error()
    for loc in (L.LOC_CCF, 3, 5, 7):  # w has no implicit step here; corners are no locations of prognostic fields
        assert step(g.cref, 1, ok[1], L.i32_array([loc]), *ok[3:]) == INVALID and b"location" in lib.ocn_last_error()
    for bad in (-1.0, float("nan"), float("inf")):
        assert step(g.cref, *ok[:5], bad, None) == INVALID and b"dt" in lib.ocn_last_error()
    assert step(g.cref, 2, L.ptr_array([8, 8]), L.i32_array([0, 0]), L.ptr_array([16, 16]), L.ptr_array([24, 24]), 0.1, None) == INVALID
    assert b"same array" in lib.ocn_last_error()
    # two matrices (different κ arrays; the same κ array at different locations) must not share a scratch array
    assert step(g.cref, 2, L.ptr_array([8, 32]), L.i32_array([0, 0]), L.ptr_array([16, 48]), L.ptr_array([24, 24]), 0.1, None) == INVALID
    assert b"same scratch array" in lib.ocn_last_error()
    assert step(g.cref, 2, L.ptr_array([8, 32]), L.i32_array([L.LOC_FCC, L.LOC_CFC]), L.ptr_array([16, 16]), L.ptr_array([24, 24]), 0.1, None) == INVALID
    assert b"same scratch array" in lib.ocn_last_error()

    # (c) the closure term
    add = lib.ocn_add_vertical_diffusivity_fluxes
    mom = (three, one, one, two, two)  # kappa_u, u, v, Gu, Gv
    tr = (1, L.ptr_array([24]), L.ptr_array([8]), L.ptr_array([16]))
    for bad in bad_grids:
        assert add(bad.cref, *mom, *tr, 1, None, None) == INVALID and b"Bounded in the z-direction" in lib.ocn_last_error()
    assert add(thin.cref, *mom, *tr, 1, None, None) == INVALID and b"halo" in lib.ocn_last_error()
    assert add(None, *mom, *tr, 1, None, None) == INVALID
    for q in (0, 2, 3, 4):
        args = list(mom)
        args[q] = None
        assert add(g.cref, *args, *tr, 0, None, None) == INVALID and b"null field pointer" in lib.ocn_last_error()
    assert add(g.cref, three, None, one, None, None, *tr, 0, None, None) == INVALID and b"u is NULL" in lib.ocn_last_error()
    assert add(g.cref, *(None,) * 5, 0, None, None, None, 0, None, None) == INVALID and b"nothing to do" in lib.ocn_last_error()
    assert add(g.cref, *mom, 9, *tr[1:], 0, None, None) == INVALID and b"number of tracers" in lib.ocn_last_error()
    assert add(g.cref, *mom, -1, *tr[1:], 0, None, None) == INVALID
    for q in (1, 2, 3):
        args = list(tr)
        args[q] = None
        assert add(g.cref, *mom, *args, 0, None, None) == INVALID and b"null tracer array" in lib.ocn_last_error()
        args[q] = L.ptr_array([None])
        assert add(g.cref, *mom, *args, 0, None, None) == INVALID and b"null pointer" in lib.ocn_last_error()
    for rng in ([0, 16, 1, 16, 1, 8], [1, 17, 1, 16, 1, 8], [1, 16, 1, 16, 1, 9], [1, 16, 0, 16, 1, 8]):
        for boundary_only in (0, 1):
            assert add(g.cref, *mom, *tr, boundary_only, L.i32_array(rng), None) == INVALID
            assert b"outside the interior" in lib.ocn_last_error()


# ---- the restatement, pinned independently of its author --------------------------------------------------------------------------------
def _case(pkg, Nz, stretched, seed):
    """a (4, 4, Nz) grid, random T and S in [-1, 1] with default (no-flux) halos, and the κ fields ConvectiveAdjustmentVerticalDiffusivity
    (background 0, convective 1) makes of them, x / y halos filled"""
    z = stretched_faces(Nz, Lz=2.0) if stretched else (-2.0, 0.0)
    g = IDN.describe(_grid(pkg, size=(4, 4, Nz), z=z))
    rng = np.random.default_rng(seed)
    T, S = (CAN.no_flux_parent(g, rng.uniform(-1, 1, (g.Nx, g.Ny, g.Nz))) for _ in range(2))
    zeros = np.zeros(CAN.ccf_shape(g))
    kc, ku = CAN.diffusivities(g, SEAWATER, T, S, 1.0, 1.0, 0.0, 0.0, zeros, zeros)
    return g, T, S, CAN.fill_xy_halos(g, kc)


def _columns(g, kappa):
    """every κz column of the case, at the three locations of u, v and the tracers"""
    return [CAN.kappa_z_column(g, kappa, loc, i, j) for loc in (0, 1, 2) for i in range(1, g.Nx + 1) for j in range(1, g.Ny + 1)]


@pytest.mark.parametrize("stretched", [False, True], ids=["uniform", "stretched"])
@pytest.mark.parametrize("Nz", [1, 2, 3, 12])
@pytest.mark.parametrize("number", [0.1, 100.0])
def test_variable_coefficient_solve_equals_the_dense_solve_and_conserves(pkg, Nz, stretched, number):
    """Every κz column of a random case (κ switches between 0 and 1 from face to face; 0.5 where u and v average a stable and an unstable
    column) at diffusion numbers Δt κ_max / min Δz² of 0.1 and 100: the restatement's elimination against numpy.linalg.solve of the dense
    matrix it assembles, tolerance 10 cond(A) ε relative to max |x| (both solvers are backward stable: each is within a few cond ε of the
    exact solution); and Σ Δz φ kept by A and by the solve to the same bound relative to Σ Δz |φ| (no flux through the boundaries is
    implicit, and the entries of rows k and k + 1 that face k + 1 contributes are -Δt κ / (Δzᶜ Δzᶠ) with the same κ and Δzᶠ)."""
    g, _, _, kappa = _case(pkg, Nz, stretched, 300 + 10 * Nz + stretched)
    dz = g.dzc[g.Hz:g.Hz + Nz]
    dt = number * float(np.min(dz)) ** 2 / 1.0
    rng = np.random.default_rng(17 + Nz)
    worst, seen = 0.0, set()
    for column in _columns(g, kappa):
        seen.update(np.unique(column[1:Nz]).tolist())
        a, b, c = CAN.diagonals_fields(g, dt, column)
        A = IDN.dense_matrix(a, b, c)
        tol = 10 * np.linalg.cond(A) * IDN.EPS
        f = rng.uniform(-1, 1, (3, Nz))
        x = IDN.thomas(a, b, c, f)
        ref = np.linalg.solve(A, f.T).T
        err = np.abs(x - ref).max() / np.abs(ref).max()
        worst = max(worst, err / tol)
        assert err <= tol
        scale = (dz * np.abs(f)).sum(axis=-1)
        total = (dz * f).sum(axis=-1)
        assert np.all(np.abs((dz * IDN.apply_matrix(a, b, c, f)).sum(axis=-1) - total) <= tol * scale)
        assert np.all(np.abs((dz * x).sum(axis=-1) - total) <= tol * scale)
    print(f"Nz={Nz} stretched={stretched} number={number}: worst error {worst:.3g} of the tolerance; κz values {sorted(seen)}")
    if Nz == 12:
        assert seen == {0.0, 0.5, 1.0}  # the matrices are not those of one constant


@pytest.mark.parametrize("stretched", [False, True], ids=["uniform", "stretched"])
@pytest.mark.parametrize("Nz", [1, 2, 3, 12])
def test_constant_column_gives_the_constant_kappa_matrix_bit_for_bit(pkg, Nz, stretched):
    z = stretched_faces(Nz, Lz=2.0) if stretched else (-2.0, 0.0)
    g = IDN.describe(_grid(pkg, size=(4, 4, Nz), z=z))
    for kappa, dt in ((0.7, 0.3), (1.0, 1e3), (0.0, 0.3)):
        new = CAN.diagonals_fields(g, dt, np.full(Nz + 1, kappa))
        old = IDN.diagonals(g, False, dt, kappa)
        for n, o in zip(new, old):
            assert np.array_equal(n, o)


@pytest.mark.parametrize("seed", range(4))
def test_classification_has_unstable_stable_and_neutral_faces_and_the_tie_is_stable(pkg, seed):
    g = IDN.describe(_grid(pkg, size=(4, 4, 12), z=stretched_faces(12, Lz=2.0)))
    T, S = CAN.plateau_inputs(g, seed)
    N2 = CAN.dz_b(g, SEAWATER, T, S)
    assert (N2 < 0).sum() >= 1 and (N2 > 0).sum() >= 1 and (N2 == 0).sum() >= 2 * g.Nx * g.Ny + g.Ny
    sentinel = np.full(CAN.ccf_shape(g), -7.0)
    kc, ku = CAN.diffusivities(g, SEAWATER, T, S, 1.0, 0.5, 1e-3, 1e-2, sentinel, sentinel)
    sl = (slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny), slice(g.Hz, g.Hz + g.Nz))
    assert np.all(kc[sl][N2 == 0] == 1e-3) and np.all(ku[sl][N2 == 0] == 1e-2)    # the tie comes out stable
    assert np.all(kc[sl][N2 > 0] == 1e-3) and np.all(kc[sl][N2 < 0] == 1.0)
    assert np.all(ku[sl][N2 > 0] == 1e-2) and np.all(ku[sl][N2 < 0] == 0.5)
    # only faces 1..Nz of the interior are written: face Nz + 1 and every halo keep what they held
    mask = np.ones(kc.shape, dtype=bool)
    mask[sl] = False
    assert np.all(kc[mask] == -7.0) and np.all(ku[mask] == -7.0)
    assert np.all(kc[g.Hx:g.Hx + g.Nx, g.Hy:g.Hy + g.Ny, g.Hz + g.Nz] == -7.0)
    # the other buoyancy formulations: b itself, and none (every face stable)
    kb, _ = CAN.diffusivities(g, "BuoyancyTracer", T, None, 1.0, 0.5, 1e-3, 1e-2, sentinel, sentinel)
    dT = CAN.dz_b(g, "BuoyancyTracer", T)
    assert np.array_equal(kb[sl] == 1.0, dT < 0) and (dT == 0).sum() >= 2 * g.Nx * g.Ny + g.Ny
    kn, un = CAN.diffusivities(g, None, None, None, 1.0, 0.5, 1e-3, 1e-2, sentinel, sentinel)
    assert np.all(kn[sl] == 1e-3) and np.all(un[sl] == 1e-2)


def test_full_fluxes_are_boundary_fluxes_plus_the_implicit_operator(pkg):
    """The splitting the time discretizations rest on, with the restatement alone: for u, v and a tracer the ExplicitTimeDiscretization term
    equals the vertically implicit term (fluxes through the two boundaries) plus (φ - A φ) / Δt, A assembled column by column -- to 1e-12 of
    the largest term (the cancellation in φ - A φ at Δt = 0.1 min Δz² / κ, divided by Δt)."""
    g, T, S, kappa = _case(pkg, 12, True, 41)
    rng = np.random.default_rng(5)
    shape = (g.Nx + 2 * g.Hx, g.Ny + 2 * g.Hy, g.Nz + 2 * g.Hz)
    u, v, c = (rng.uniform(-1, 1, shape) for _ in range(3))
    dt = 0.1 * float(np.min(g.dzc[g.Hz:g.Hz + g.Nz])) ** 2
    full = CAN.vertical_fluxes(g, kappa, u, v, [kappa], [c], False)
    edge = CAN.vertical_fluxes(g, kappa, u, v, [kappa], [c], True)
    sl = (slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny), slice(g.Hz, g.Hz + g.Nz))
    for name, field, loc, Df, De in (("u", u, 1, full[0], edge[0]), ("v", v, 2, full[1], edge[1]), ("c", c, 0, full[2][0], edge[2][0])):
        implicit = np.zeros_like(Df)
        for i in range(1, g.Nx + 1):
            for j in range(1, g.Ny + 1):
                a, b, cc = CAN.diagonals_fields(g, dt, CAN.kappa_z_column(g, kappa, loc, i, j))
                phi = field[sl][i - 1, j - 1]
                implicit[i - 1, j - 1] = (phi - IDN.apply_matrix(a, b, cc, phi)) / dt
        scale = np.abs(Df).max()
        assert np.abs(-Df - (-De + implicit)).max() <= 1e-12 * scale
        assert np.abs(implicit).max() > 0.1 * scale
