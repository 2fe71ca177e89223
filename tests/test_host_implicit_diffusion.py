"""ScalarDiffusivity(VerticallyImplicitTimeDiscretization(), ...) without a GPU: constructors and refusals, the argument checks of the two
C entry points (no device is touched), and the NumPy restatement (tests/implicit_diffusion_numpy.py) pinned independently of its author:
its Thomas solve against numpy.linalg.solve of the dense matrix it assembles, and its Center rows against conservation."""
import ctypes as C

import numpy as np
import pytest

import implicit_diffusion_numpy as IDN
from helpers import stretched_faces

P, B, F = "Periodic", "Bounded", "Flat"
INVALID = -1  # OCN_ERR_INVALID_ARGUMENT (include/ocn_hip.h)


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


# ---- constructors ------------------------------------------------------------------------------------------------------------------------
def test_constructors_mirror_the_reference(pkg):
    VI, EX = pkg.VerticallyImplicitTimeDiscretization, pkg.ExplicitTimeDiscretization
    c = pkg.ScalarDiffusivity(VI(), ν=1e-2, κ=1e-3)
    assert isinstance(c.time_discretization, VI) and c.nu == 1e-2 and c.kappa_of("T") == 1e-3
    for c in (pkg.ScalarDiffusivity(ν=1, κ=2, time_discretization=VI()), pkg.ScalarDiffusivity(nu=1, kappa=2, time_discretization="VerticallyImplicit"),
              pkg.ScalarDiffusivity(VI(), 1, 2), pkg.ScalarDiffusivity(VI, ν=1, κ=2)):
        assert isinstance(c.time_discretization, VI) and c.nu == 1.0 and c.kappa_of("c") == 2.0
    for c in (pkg.ScalarDiffusivity(ν=1, κ=2), pkg.ScalarDiffusivity(EX(), ν=1, κ=2), pkg.ScalarDiffusivity(1, 2),
              pkg.ScalarDiffusivity(ν=1, κ=2, time_discretization="Explicit"), pkg.ScalarDiffusivity(1, 2, EX())):
        assert isinstance(c.time_discretization, EX) and c.nu == 1.0 and c.kappa_of("c") == 2.0
    d = pkg.ScalarDiffusivity(VI(), ν=1e-2, κ={"T": 1e-3, "S": 2e-3})
    assert d.kappa_of("S") == 2e-3
    with pytest.raises(ValueError, match="tracer c"):
        d.kappa_of("c")
    from oceananigans_jl_amd.physics import is_vertically_implicit
    assert is_vertically_implicit(d) and not is_vertically_implicit(pkg.ScalarDiffusivity(ν=1)) and not is_vertically_implicit(None)


def test_what_is_not_implemented_says_so(pkg):
    VI = pkg.VerticallyImplicitTimeDiscretization
    with pytest.raises(ValueError, match="time_discretization"):
        pkg.ScalarDiffusivity(ν=1, time_discretization="Implicit")
    with pytest.raises(TypeError, match="twice"):
        pkg.ScalarDiffusivity(VI(), ν=1, time_discretization=VI())
    with pytest.raises(NotImplementedError, match="ThreeDimensional"):
        pkg.ScalarDiffusivity(VI(), ν=1, formulation="Vertical")
    with pytest.raises(NotImplementedError, match="constant"):
        pkg.ScalarDiffusivity(VI(), ν=lambda x, y, z, t: 1.0)
    # the eddy-viscosity closures keep refusing a vertically implicit discretization
    for td in (VI(), "VerticallyImplicit"):
        with pytest.raises(NotImplementedError):
            pkg.Smagorinsky(time_discretization=td)
        with pytest.raises(NotImplementedError):
            pkg.SmagorinskyLilly(time_discretization=td)
        with pytest.raises((NotImplementedError, TypeError)):
            pkg.AnisotropicMinimumDissipation(time_discretization=td)
    assert pkg.Smagorinsky(time_discretization=pkg.ExplicitTimeDiscretization()).C == 0.16


def test_model_refusals_come_before_any_allocation(pkg, monkeypatch):
    _no_alloc(monkeypatch)
    closure = pkg.ScalarDiffusivity(pkg.VerticallyImplicitTimeDiscretization(), ν=1e-2, κ=1e-3)
    wording = "VerticallyImplicitTimeDiscretization can only be specified on grids that are Bounded in the z-direction."
    with pytest.raises(ValueError, match=wording):
        pkg.NonhydrostaticModel(_grid(pkg, topo=(P, P, P)), advection=pkg.WENO(), closure=closure)
    with pytest.raises(ValueError, match=wording):
        pkg.NonhydrostaticModel(pkg.RectilinearGrid(None, size=(8, 8), x=(0, 1), y=(0, 1), topology=(P, P, F), halo=(3, 3)),
                                advection=pkg.WENO(), closure=closure)

    class FakeDistributed:  # what models.py asks of a Distributed architecture: a `partition`
        partition = object()
        communicates = True
    gd = _grid(pkg)
    gd.architecture = FakeDistributed()
    with pytest.raises(NotImplementedError, match="Distributed"):
        pkg.NonhydrostaticModel(gd, advection=pkg.WENO(), closure=closure)
    # HydrostaticFreeSurfaceModel: fused = True, SplitRungeKutta3 and slab ranks
    g = _grid(pkg)
    with pytest.raises(NotImplementedError, match="fused = False"):
        pkg.HydrostaticFreeSurfaceModel(g, closure=closure, free_surface=pkg.ExplicitFreeSurface(), fused=True)
    with pytest.raises(NotImplementedError, match="SplitRungeKutta3"):
        pkg.HydrostaticFreeSurfaceModel(g, closure=closure, free_surface=pkg.SplitExplicitFreeSurface(substeps=10), timestepper="SplitRungeKutta3")
    gs = _grid(pkg)
    gs.architecture = FakeDistributed()
    gs.topology = (pkg.FullyConnected, P, B)
    with pytest.raises(NotImplementedError, match="slab-partitioned"):
        pkg.HydrostaticFreeSurfaceModel(gs, closure=closure, free_surface=pkg.SplitExplicitFreeSurface(substeps=10))


def test_drivers_name_the_python_host(pkg):
    """(the drivers look at the model before anything else; the GPU suite repeats this with real models)"""
    from types import SimpleNamespace
    m = SimpleNamespace(grid=_grid(pkg), _implicit=True, particles=None)
    for driver in (pkg.RK3Driver, pkg.ModelRK3Driver):
        with pytest.raises(NotImplementedError, match="Python host"):
            driver(m)


# ---- C ABI: argument checks before any HIP call ------------------------------------------------------------------------------------------
def test_c_abi_argument_checks_touch_no_device(pkg):
    lib, L = pkg._lib.lib(), pkg._lib
    g = _grid(pkg, size=(16, 16, 8))
    one, two = C.c_void_p(8), C.c_void_p(16)  # never dereferenced
    step = lib.ocn_implicit_vertical_diffusion_step
    dbl = lambda *v: (C.c_double * len(v))(*v)
    ok = (1, L.ptr_array([8]), L.i32_array([L.LOC_CCC]), dbl(1.0), 0.1, None)
    wording = b"can only be specified on grids that are Bounded in the z-direction"
    for bad_grid in (_grid(pkg, topo=(P, P, P)), pkg.RectilinearGrid(None, size=(16, 16), x=(0, 1), y=(0, 1), topology=(P, P, F), halo=(3, 3))):
        assert step(bad_grid.cref, *ok) == INVALID
        assert wording in lib.ocn_last_error()
    assert step(None, *ok) == INVALID
    assert step(g.cref, 0, *ok[1:]) == INVALID and b"number of fields" in lib.ocn_last_error()
    assert step(g.cref, 9, *ok[1:]) == INVALID
    assert step(g.cref, 1, None, *ok[2:]) == INVALID and b"null tuple pointer" in lib.ocn_last_error()
    assert step(g.cref, 1, ok[1], None, *ok[3:]) == INVALID
    assert step(g.cref, 1, ok[1], ok[2], None, 0.1, None) == INVALID
    assert step(g.cref, 1, L.ptr_array([None]), *ok[2:]) == INVALID and b"null pointer" in lib.ocn_last_error()
    assert step(g.cref, 1, ok[1], L.i32_array([3]), *ok[3:]) == INVALID and b"location" in lib.ocn_last_error()
    for bad in (-1.0, float("nan"), float("inf")):
        assert step(g.cref, 1, ok[1], ok[2], dbl(bad), 0.1, None) == INVALID and b"kappa" in lib.ocn_last_error()
        assert step(g.cref, 1, ok[1], ok[2], ok[3], bad, None) == INVALID and b"dt" in lib.ocn_last_error()
    assert step(g.cref, 2, L.ptr_array([8, 8]), L.i32_array([0, 0]), dbl(1.0, 1.0), 0.1, None) == INVALID
    assert b"same array" in lib.ocn_last_error()
    tall = pkg.RectilinearGrid(None, size=(4, 4, 2049), x=(0, 1), y=(0, 1), z=(-1, 0), topology=(P, P, B), halo=(3, 3, 3))
    assert step(tall.cref, *ok) == INVALID and b"2048" in lib.ocn_last_error()
    thin = pkg.RectilinearGrid(None, size=(16, 16, 8), x=(0, 1), y=(0, 1), z=(-1, 0), topology=(P, P, B), halo=(3, 3, 0))
    assert step(thin.cref, *ok) == INVALID and b"halo" in lib.ocn_last_error()

    add = lib.ocn_add_vertically_implicit_explicit_fluxes
    mom = (one, one, one, two, two, two)
    none6 = (None,) * 6
    tr = (1, dbl(1.0), L.ptr_array([8]), L.ptr_array([16]))
    for bad_grid in (_grid(pkg, topo=(P, P, P)), pkg.RectilinearGrid(None, size=(16, 16), x=(0, 1), y=(0, 1), topology=(P, P, F), halo=(3, 3))):
        assert add(bad_grid.cref, 1.0, *mom, *tr, None, None) == INVALID
        assert wording in lib.ocn_last_error()
    assert add(None, 1.0, *mom, *tr, None, None) == INVALID
    assert add(g.cref, 1.0, one, None, one, two, two, two, *tr, None, None) == INVALID and b"null field pointer" in lib.ocn_last_error()
    assert add(g.cref, 1.0, one, one, one, two, None, two, *tr, None, None) == INVALID
    assert add(g.cref, 1.0, None, one, None, None, None, None, *tr, None, None) == INVALID and b"u is NULL" in lib.ocn_last_error()
    assert add(g.cref, 1.0, *none6, 0, None, None, None, None, None) == INVALID and b"nothing to do" in lib.ocn_last_error()
    for bad in (-1.0, float("nan")):
        assert add(g.cref, bad, *mom, *tr, None, None) == INVALID and b"nu" in lib.ocn_last_error()
        assert add(g.cref, 1.0, *mom, 1, dbl(bad), tr[2], tr[3], None, None) == INVALID and b"kappa" in lib.ocn_last_error()
    assert add(g.cref, 1.0, *mom, 9, *tr[1:], None, None) == INVALID and b"number of tracers" in lib.ocn_last_error()
    assert add(g.cref, 1.0, *mom, -1, *tr[1:], None, None) == INVALID
    assert add(g.cref, 1.0, *mom, 1, None, tr[2], tr[3], None, None) == INVALID and b"null tracer array" in lib.ocn_last_error()
    assert add(g.cref, 1.0, *mom, 1, tr[1], L.ptr_array([None]), tr[3], None, None) == INVALID
    assert add(g.cref, 1.0, *mom, 1, tr[1], tr[2], L.ptr_array([None]), None, None) == INVALID
    for rng in ([0, 16, 1, 16, 1, 8], [1, 17, 1, 16, 1, 8], [1, 16, 1, 16, 1, 9], [1, 16, 0, 16, 1, 8]):
        assert add(g.cref, 1.0, *mom, *tr, L.i32_array(rng), None) == INVALID and b"outside the interior" in lib.ocn_last_error()


# ---- the restatement, pinned independently of its author --------------------------------------------------------------------------------
def _column(pkg, Nz, stretched):
    """the vertical spacings of a package grid (halos as the grid extends them)"""
    z = stretched_faces(Nz, Lz=2.0) if stretched else (-2.0, 0.0)
    return IDN.describe(_grid(pkg, size=(4, 4, Nz), z=z))


@pytest.mark.parametrize("zface", [False, True], ids=["Center", "Face"])
@pytest.mark.parametrize("stretched", [False, True], ids=["uniform", "stretched"])
@pytest.mark.parametrize("Nz", [1, 2, 3, 12])
@pytest.mark.parametrize("number", [0.1, 100.0])
def test_thomas_solve_equals_the_dense_solve(pkg, Nz, stretched, zface, number):
    """The restatement's elimination against numpy.linalg.solve of the dense matrix it assembles, at diffusion numbers Δt κ / min Δz² of
    0.1 and 100.  Tolerance 10 cond(A) ε relative to max |x| (both solvers are backward stable: each is within a few cond ε of the exact
    solution), cond computed here from the matrix."""
    g = _column(pkg, Nz, stretched)
    kappa = 0.7
    dt = number * float(np.min(g.dzc[g.Hz:g.Hz + Nz])) ** 2 / kappa
    a, b, c = IDN.diagonals(g, zface, dt, kappa)
    A = IDN.dense_matrix(a, b, c)
    assert A.shape == (Nz, Nz)
    rng = np.random.default_rng(100 * Nz + 10 * stretched + zface)
    f = rng.uniform(-1, 1, (5, 3, Nz))
    x = IDN.thomas(a, b, c, f)
    ref = np.linalg.solve(A, f.reshape(-1, Nz).T).T.reshape(f.shape)
    tol = 10 * np.linalg.cond(A) * IDN.EPS
    err = np.abs(x - ref).max() / np.abs(ref).max()
    print(f"Nz={Nz} stretched={stretched} zface={zface} number={number}: cond={np.linalg.cond(A):.3g} err={err:.3g} tol={tol:.3g}")
    assert err <= tol
    # ... and the matrix is what apply_matrix applies
    np.testing.assert_allclose(IDN.apply_matrix(a, b, c, f), f @ A.T, rtol=0, atol=8 * IDN.EPS * np.abs(A).sum(axis=1).max())


@pytest.mark.parametrize("stretched", [False, True], ids=["uniform", "stretched"])
@pytest.mark.parametrize("Nz", [1, 2, 3, 12])
@pytest.mark.parametrize("number", [0.1, 100.0])
def test_center_rows_conserve_the_column_integral(pkg, Nz, stretched, number):
    """Σ_k Δz_k (A φ)_k = Σ_k Δz_k φ_k for the Center rows (no flux through the two boundaries is implicit), to 10 cond(A) ε relative to
    Σ Δz |φ| -- and the same for the solve: Σ Δz (A⁻¹ f) = Σ Δz f."""
    g = _column(pkg, Nz, stretched)
    kappa = 0.7
    dz = g.dzc[g.Hz:g.Hz + Nz]
    dt = number * float(np.min(dz)) ** 2 / kappa
    a, b, c = IDN.diagonals(g, False, dt, kappa)
    A = IDN.dense_matrix(a, b, c)
    tol = 10 * np.linalg.cond(A) * IDN.EPS
    rng = np.random.default_rng(7 + Nz)
    phi = rng.uniform(-1, 1, (6, Nz))
    scale = (dz * np.abs(phi)).sum(axis=-1)
    lhs = (dz * IDN.apply_matrix(a, b, c, phi)).sum(axis=-1)
    rhs = (dz * phi).sum(axis=-1)
    assert np.all(np.abs(lhs - rhs) <= tol * scale)
    sol = IDN.thomas(a, b, c, phi)
    assert np.all(np.abs((dz * sol).sum(axis=-1) - rhs) <= tol * scale)
    # the column sums of Δz-weighted A are Δz itself: Σ_k Δz_k A[k, l] = Δz_l
    np.testing.assert_allclose(dz @ A, dz, rtol=tol)


def test_face_rows_are_the_reference_s_as_written(pkg):
    """The Face-in-z rows transcribed, not repaired (vertically_implicit_diffusion_solver.jl:88-104): the wall-face row 1 has the diagonal
    1 - upper(1) and a nonzero entry above the diagonal, and the entry below the diagonal of row k + 1 is built from Δzᶜ(k + 2) Δzᶠ(k + 1).
    On a uniform grid the interior rows are the second-difference operator."""
    g = _column(pkg, 6, True)
    dt, nu = 0.3, 0.5
    a, b, c = IDN.diagonals(g, True, dt, nu)
    dzc, dzf = (lambda k: g.dzc[k + g.Hz - 1]), (lambda k: g.dzf[k + g.Hz - 1])
    for k in range(1, 7):
        assert c[k - 1] == -dt * nu / (dzc(k) * dzf(k))
    for k in range(1, 6):
        assert a[k - 1] == -dt * nu / (dzc(k + 2) * dzf(k + 1))
    assert b[0] == 1.0 - c[0] and c[0] != 0.0
    for k in range(2, 7):
        assert b[k - 1] == (1.0 - c[k - 1]) - a[k - 2]
    gu = _column(pkg, 6, False)
    a, b, c = IDN.diagonals(gu, True, dt, nu)
    r = dt * nu / float(gu.dzc[gu.Hz]) ** 2
    np.testing.assert_allclose(a[:-1], -r, rtol=4 * IDN.EPS)
    np.testing.assert_allclose(c, -r, rtol=4 * IDN.EPS)
    np.testing.assert_allclose(b[1:], 1 + 2 * r, rtol=4 * IDN.EPS)
