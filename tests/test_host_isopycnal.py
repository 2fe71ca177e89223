"""IsopycnalSkewSymmetricDiffusivity without a GPU: the constructor, its strings and its refusals (before any allocation), the closure
tuples, and the NumPy restatement (tests/isopycnal_numpy.py) pinned by properties of the scheme that do not depend on its author: flat
isopycnals give horizontal diffusion, a tracer that is the buoyancy has no flux along its own isopycnals, the eddy velocities do not diverge,
and a tapered flux is the untapered one times max_slope² / slope².  The shared input of the GPU tests is checked here for branch coverage."""
import numpy as np
import pytest

import implicit_diffusion_numpy as IDN
import isopycnal_numpy as ISN

P, B = "Periodic", "Bounded"
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def pkg():
    import oceananigans_jl_amd as ocn
    return ocn


def _grid(pkg, topo=(P, P, B), size=(4, 5, 6), halo=(3, 3, 3)):
    return pkg.RectilinearGrid(None, size=size, x=(0, 1), y=(0, 1), z=(-1, 0), topology=topo, halo=halo)


def _no_alloc(monkeypatch):
    import oceananigans_jl_amd.fields as fields

    def no_alloc(*a, **k):
        raise AssertionError("a field was allocated before the refusal")
    monkeypatch.setattr(fields.Field, "__init__", no_alloc)


# ---- 1. the constructor ---------------------------------------------------------------------------------------------------------------------
def test_defaults_strings_and_keyword_spellings(pkg):
    ISSD = pkg.IsopycnalSkewSymmetricDiffusivity
    d = ISSD()
    assert d.κ_skew is None and d.κ_symmetric is None and d.kappa_skew is None and d.kappa_symmetric is None
    assert isinstance(d.skew_flux_formulation, pkg.AdvectiveFormulation) and isinstance(d.isopycnal_tensor, pkg.SmallSlopeIsopycnalTensor)
    assert d.isopycnal_tensor.minimum_bz == 0.0 and isinstance(d.slope_limiter, pkg.FluxTapering) and d.slope_limiter.max_slope == 1e-2
    assert d.required_halo_size == 1 and isinstance(d.time_discretization, pkg.VerticallyImplicitTimeDiscretization)
    from oceananigans_jl_amd.physics import has_diffusivity_fields, is_vertically_implicit, owns_eddy_fields
    assert is_vertically_implicit(d) and not owns_eddy_fields(d) and not has_diffusivity_fields(d)
    assert d.summary() == "IsopycnalSkewSymmetricDiffusivity(κ_skew=Nothing, κ_symmetric=Nothing)"
    assert repr(d) == ("IsopycnalSkewSymmetricDiffusivity: (κ_symmetric=nothing, κ_skew=nothing, "
                       "(isopycnal_tensor=SmallSlopeIsopycnalTensor{Float64}(0.0), slope_limiter=FluxTapering{Float64}(0.01))")
    c = ISSD(κ_skew=1e3, κ_symmetric=900)
    assert (c.κ_skew, c.κ_symmetric) == (1000.0, 900.0) and isinstance(c.κ_symmetric, float)
    assert c.summary() == "IsopycnalSkewSymmetricDiffusivity(κ_skew=1000.0, κ_symmetric=900.0)"
    assert repr(c).startswith("IsopycnalSkewSymmetricDiffusivity: (κ_symmetric=900.0, κ_skew=1000.0, (isopycnal_tensor=")
    a = ISSD(kappa_skew=1e3, kappa_symmetric=900)
    assert (a.κ_skew, a.κ_symmetric) == (c.κ_skew, c.κ_symmetric) and repr(a) == repr(c)
    assert ISSD(pkg.VerticallyImplicitTimeDiscretization(), κ_skew=1).κ_skew == 1.0
    assert ISSD(time_discretization="VerticallyImplicit", κ_skew=1).κ_skew == 1.0
    # the coefficients inside the fluxes (get_tracer_κ, skew_diffusivity)
    assert c.kappa_symmetric_of("b") == 900.0 and c.kappa_skew_of("b") == 0.0  # (advective: the skew part is in the eddy velocities)
    f = ISSD(κ_skew={"b": 1e3, "c": 0}, κ_symmetric={"b": 2e3, "c": 123456789.0}, skew_flux_formulation=pkg.DiffusiveFormulation())
    assert f.kappa_skew_of("b") == 1000.0 and f.kappa_skew_of("c") == 0.0 and f.kappa_symmetric_of("c") == 123456789.0
    assert f.summary() == "IsopycnalSkewSymmetricDiffusivity(κ_skew=(b=1000.0, c=0.0), κ_symmetric=(b=2000.0, c=1.23457e8))"
    assert "(κ_symmetric=(b = 2000.0, c = 1.23456789e8), κ_skew=(b = 1000.0, c = 0.0), " in repr(f)
    with pytest.raises(ValueError, match="no diffusivity κ given for tracer T"):
        f.kappa_symmetric_of("T")
    assert d.kappa_symmetric_of("b") == 0.0 and ISSD(skew_flux_formulation=pkg.DiffusiveFormulation).kappa_skew_of("b") == 0.0
    t = ISSD(isopycnal_tensor=pkg.SmallSlopeIsopycnalTensor(minimum_bz=1e-10), slope_limiter=pkg.FluxTapering(5e-3), required_halo_size=2)
    assert repr(t).endswith("(isopycnal_tensor=SmallSlopeIsopycnalTensor{Float64}(1.0e-10), slope_limiter=FluxTapering{Float64}(0.005))")
    assert t.required_halo_size == 2
    s = t.c_struct()
    assert (s.max_slope, s.minimum_bz) == (5e-3, 1e-10)
    assert repr(pkg.AdvectiveFormulation()) == "AdvectiveFormulation()" and repr(pkg.DiffusiveFormulation()) == "DiffusiveFormulation()"


def test_the_constructor_checks_of_the_reference_and_what_is_not_implemented(pkg):
    ISSD = pkg.IsopycnalSkewSymmetricDiffusivity
    with pytest.raises(ValueError, match="Only one skew coefficient for all tracers is currently supported with the AdvectiveFormulation."):
        ISSD(κ_skew={"b": 1.0})
    with pytest.raises(NotImplementedError, match=r"Only isopycnal_tensor=SmallSlopeIsopycnalTensor\(\) is currently supported."):
        ISSD(κ_skew=1.0, isopycnal_tensor=pkg.IsopycnalTensor(0.0))
    for td in ("Explicit", pkg.ExplicitTimeDiscretization(), pkg.ExplicitTimeDiscretization):
        with pytest.raises(NotImplementedError, match="explicit_κ_∂z_c.*:308.*:316"):
            ISSD(td, κ_skew=1.0)
    with pytest.raises(NotImplementedError, match="explicit_κ_∂z_c"):
        ISSD(time_discretization="Explicit")
    for bad in (lambda x, y, z, t: 1.0, np.ones(3), np.ones((2, 2, 2)), "1", True):
        for name in ("κ_skew", "kappa_skew", "κ_symmetric", "kappa_symmetric"):
            with pytest.raises(NotImplementedError, match="must be a number"):
                ISSD(**{name: bad})
    with pytest.raises(NotImplementedError, match="must be a number"):
        ISSD(κ_symmetric={"b": lambda x, y, z, t: 1.0})
    with pytest.raises(NotImplementedError, match="slope_limiter"):
        ISSD(slope_limiter=1e-2)
    with pytest.raises(TypeError, match="twice"):
        ISSD(κ_skew=1, kappa_skew=1)
    with pytest.raises(TypeError, match="unexpected"):
        ISSD(kappa=1)
    with pytest.raises(TypeError, match="skew_flux_formulation"):
        ISSD(skew_flux_formulation="Advective")
    with pytest.raises(ValueError, match="required_halo_size"):
        ISSD(required_halo_size=0)


# ---- 2. models ------------------------------------------------------------------------------------------------------------------------------
class _FakeDistributed:  # what the models ask of a Distributed architecture
    partition = object()
    communicates = True


def test_model_refusals_come_before_any_allocation_and_the_tuples_pass_validation(pkg, monkeypatch):
    _no_alloc(monkeypatch)
    ISSD, HSBD, CAVD, RI = (pkg.IsopycnalSkewSymmetricDiffusivity, pkg.HorizontalScalarBiharmonicDiffusivity,
                            pkg.ConvectiveAdjustmentVerticalDiffusivity, pkg.RiBasedVerticalDiffusivity)
    g = _grid(pkg)
    issd, bih = ISSD(κ_skew=1e3, κ_symmetric=1e3), HSBD(ν=1e-3, κ=1e-4)
    kw = dict(tracers=("b", "c"), buoyancy=pkg.BuoyancyTracer())
    hydro = lambda closure, grid=g, **k: pkg.HydrostaticFreeSurfaceModel(grid, closure=closure, **{"free_surface": pkg.ExplicitFreeSurface(), **kw, **k})
    with pytest.raises(NotImplementedError, match="IsopycnalSkewSymmetricDiffusivity on NonhydrostaticModel"):
        pkg.NonhydrostaticModel(g, advection=pkg.WENO(), closure=issd, **kw)
    with pytest.raises(NotImplementedError, match=r"IsopycnalSkewSymmetricDiffusivity runs the reference's launch sequence \(fused = False\)"):
        hydro(issd, fused=True)
    with pytest.raises(NotImplementedError, match="IsopycnalSkewSymmetricDiffusivity with SplitRungeKutta3"):
        hydro(issd, timestepper="SplitRungeKutta3", free_surface=pkg.SplitExplicitFreeSurface(substeps=10))
    gs = _grid(pkg)
    gs.architecture = _FakeDistributed()
    gs.topology = (pkg.FullyConnected, P, B)
    with pytest.raises(NotImplementedError, match="Distributed"):
        hydro(issd, grid=gs, free_surface=pkg.SplitExplicitFreeSurface(substeps=10))
    for topo in ((P, B, B), (B, B, B)):
        with pytest.raises(NotImplementedError, match="walls in x or y"):
            hydro(issd, grid=_grid(pkg, topo))
    with pytest.raises(NotImplementedError, match="arrays of closures"):
        hydro(np.array([issd, issd], dtype=object))
    with pytest.raises(ValueError, match="no diffusivity κ given for tracer c"):
        hydro(ISSD(κ_symmetric={"b": 1.0}))
    vertical = (CAVD(convective_κz=1), RI(warning=False), pkg.CATKEVerticalDiffusivity())
    refused = [(issd,), [issd], (issd, issd), (issd, pkg.ScalarDiffusivity(ν=1e-2)), (pkg.ScalarDiffusivity(ν=1e-2), issd),
               (issd, pkg.SmagorinskyLilly()), (bih, issd, vertical[0]), (issd, bih, bih)]
    refused += [(issd, V) for V in vertical] + [(V, issd) for V in vertical]
    for closure in refused:
        with pytest.raises(NotImplementedError, match="closure tuples are not implemented, except"):
            hydro(closure)
        with pytest.raises(NotImplementedError):
            pkg.NonhydrostaticModel(g, advection=pkg.WENO(), closure=closure, **kw)
    # what is accepted gets as far as allocating its fields
    for closure in (issd, ISSD(), ISSD(κ_symmetric={"b": 1.0, "c": 2.0}), (bih, issd), (issd, bih), [bih, issd]):
        with pytest.raises(AssertionError, match="a field was allocated"):
            hydro(closure)
        if isinstance(closure, ISSD) and isinstance(closure.κ_symmetric, dict):
            continue  # (its κ are named for b and c)
        with pytest.raises(AssertionError, match="a field was allocated"):
            hydro(closure, tracers=("T", "S"), buoyancy=pkg.SeawaterBuoyancy(), free_surface=pkg.SplitExplicitFreeSurface(substeps=10))


def test_the_closure_object_of_the_model(pkg):
    """resolve_closure allocates nothing: what it answers for the closure alone and in the pair"""
    from oceananigans_jl_amd.hydrostatic_closures import Biharmonic, IsopycnalFields, resolve_closure
    ISSD, bih = pkg.IsopycnalSkewSymmetricDiffusivity, pkg.HorizontalScalarBiharmonicDiffusivity(κ=1.0)
    resolve = lambda c: resolve_closure(c, None, False, False, False, pkg.BuoyancyTracer(), None, ("b", "c"))
    o = resolve(ISSD(κ_skew=1e3, κ_symmetric=1e3, required_halo_size=3))
    assert isinstance(o, IsopycnalFields) and o.unfused and o.halo == 3 and o.implicit and o.eddy and not o.no_diffusion
    assert o.container_closure is None and o.state_fields == () and o.self_stepped == ()
    assert o.kappa_of_tracer("c") == (1000.0, 0.0)
    n = resolve(ISSD(κ_skew=1e3))
    assert n.eddy and n.no_diffusion and not n.implicit          # NoDiffusionISSD
    s = resolve(ISSD(κ_symmetric=1e3))
    assert not s.eddy and not s.no_diffusion and s.implicit      # NoSkewAdvectionISSD
    d = resolve(ISSD(κ_skew={"b": 1.0, "c": 2.0}, κ_symmetric=5.0, skew_flux_formulation=pkg.DiffusiveFormulation()))
    assert not d.eddy and d.kappa_of_tracer("c") == (5.0, 2.0)
    for pair in ((bih, ISSD(κ_skew=1e3, κ_symmetric=1e3)), (ISSD(κ_skew=1e3, κ_symmetric=1e3), bih)):
        p = resolve(pair)
        assert isinstance(p, Biharmonic) and isinstance(p.other, IsopycnalFields) and p.halo == 2 and p.implicit and p.unfused
        assert p.advecting_velocities == p.other.advecting_velocities
    assert resolve((bih, ISSD(required_halo_size=4))).halo == 4


# ---- 3. properties of the restatement -----------------------------------------------------------------------------------------------------
def _describe(pkg, name):
    return IDN.describe(pkg.RectilinearGrid(None, **ISN.case_grid_arguments(name)))


def _parents(g, f):
    """a function of (x index, y index, z) evaluated on the whole parent of a centre field"""
    nx, ny, nz = ISN.parent_shape(g)
    zc = np.cumsum(np.asarray(g.dzf[:nz], dtype=np.float64))
    return f((np.arange(nx) - g.Hx)[:, None, None] * g.dx, (np.arange(ny) - g.Hy)[None, :, None] * g.dy, zc[None, None, :])


@pytest.mark.parametrize("name", ["reference_333", "tile_plus_partial"])
def test_flat_isopycnals_give_horizontal_diffusion_and_no_eddy_velocities(pkg, name):
    """b = N² z: R₁₃ = R₂₃ = R₃₁ = R₃₂ = 0 and ϵ = 1 exactly, so the x and y fluxes are those of a Laplacian diffusion with κ_symmetric,
    -(κ ∂x c) and -(κ ∂y c), bit for bit, the z flux is 0 and so are uₑ, vₑ, wₑ"""
    g, cl = _describe(pkg, name), ISN.closure()
    b = _parents(g, lambda x, y, z: 1e-5 * z + 0 * x + 0 * y)
    c = np.random.default_rng(3).uniform(-1, 1, b.shape)
    ks = 750.0
    for kw in (0.0, 300.0):
        fx, fy, fz = ISN.fluxes(g, ISN.TRACER, b, None, cl, ks, kw, c)
        cx, cy, _ = ISN.derivatives(g, c)
        for shift in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
            assert np.array_equal(fx(*shift), -(ks * cx(*shift))) and np.array_equal(fy(*shift), -(ks * cy(*shift)))
            assert np.all(fz(*shift) == 0)
        assert np.abs(fx(0, 0, 0)).max() > 0
    for q in ISN.eddy_velocities(g, ISN.TRACER, b, None, cl, 1e3):
        assert np.all(q == 0)
    assert np.all(ISN.tapered_R33(g, ISN.TRACER, b, None, cl) == 0)


def test_the_buoyancy_itself_is_not_diffused_along_its_isopycnals(pkg):
    """c = b with constant gradients, slope 0.6 max_slope (ϵ = 1), κ_skew = nothing: the x flux is -(κ bx + (κ R₁₃) ∂z b) with R₁₃ = -bx / bz
    and ∂z b = bz the same bits.  κ R₁₃ bz = -κ bx (1 + δ)³ (the division, two products), the sum adds one rounding: |flux| <= 4 eps κ |bx|;
    8 eps κ max|∇b| allows for the interpolations of gradients that are constant only up to their own rounding."""
    g, cl = _describe(pkg, "tile_plus_partial"), ISN.closure()
    N2, Sx, Sy = 1e-5, 0.6e-2 * 0.8, 0.6e-2 * 0.6
    b = _parents(g, lambda x, y, z: N2 * z + N2 * Sx * x + N2 * Sy * y)
    ks = 1e3
    fx, fy, fz = ISN.fluxes(g, ISN.TRACER, b, None, cl, ks, 0.0, b)
    G = ISN.face_gradients(g, ISN.TRACER, b, None)
    for kind in G:  # the premise: every face is untapered
        assert np.all(ISN.calc_tapering(cl, *(f(0, 0, 0) for f in G[kind])) == 1)
    bound = 8 * EPS * ks * N2 * max(Sx, Sy)
    unrotated = ks * N2 * Sx
    print(f"max |flux x| {np.abs(fx(0, 0, 0)).max():.3e}, max |flux y| {np.abs(fy(0, 0, 0)).max():.3e}, bound {bound:.3e}, κ bx {unrotated:.3e}")
    assert np.abs(fx(0, 0, 0)).max() <= bound and np.abs(fy(0, 0, 0)).max() <= bound
    assert bound < 1e-14 * unrotated
    # the z flux is the diapycnal remainder of the small-slope tensor: -κ (R₃₁ bx + R₃₂ by) = κ slope² bz, not small
    assert np.allclose(fz(0, 0, 0), ks * (Sx ** 2 + Sy ** 2) * N2, rtol=1e-6)


@pytest.mark.parametrize("buoyancy", [ISN.TRACER, ISN.SEAWATER], ids=["b", "TS"])
@pytest.mark.parametrize("name", list(ISN.CASES))
def test_the_eddy_velocities_do_not_diverge(pkg, name, buoyancy):
    """δx(Ax uₑ) + δy(Ay vₑ) + δz(Az wₑ) = 0 in every interior cell: uₑ, vₑ, wₑ are the curl of (-κ Sy, κ Sx, 0).  Each product of an area and
    a difference quotient carries four roundings (the difference, the quotient, the area, their product), wₑ adds its two quotients (one
    more) and the divergence adds six numbers (three levels): 8 eps times the sum of the magnitudes of the eight products, the two parts of
    wₑ counted apart (they may cancel)"""
    g, cl = _describe(pkg, name), ISN.closure()
    T, S, _ = ISN.case_inputs(g, buoyancy)
    ue, ve, we = ISN.eddy_velocity_functions(g, buoyancy, T, S, cl, 1e3)
    Sx, Sy = ISN.tapered_slopes(g, buoyancy, T, S, cl)
    wx = lambda c: (1e3 * Sx(1, 0, c) - 1e3 * Sx(0, 0, c)) / g.dx
    wy = lambda c: (1e3 * Sy(0, 1, c) - 1e3 * Sy(0, 0, c)) / g.dy
    assert np.array_equal(we(0, 0, 0), wx(0) + wy(0)) and np.array_equal(we(0, 0, 1), wx(1) + wy(1))
    dz = IDN._dzC(g, 0)
    Ax, Ay, Az = g.dy * dz, g.dx * dz, g.dx * g.dy
    terms = [Ax * ue(1, 0, 0), Ax * ue(0, 0, 0), Ay * ve(0, 1, 0), Ay * ve(0, 0, 0), Az * we(0, 0, 1), Az * we(0, 0, 0)]
    div = ((terms[0] - terms[1]) + (terms[2] - terms[3])) + (terms[4] - terms[5])
    scale = sum(np.abs(t) for t in terms[:4]) + Az * (np.abs(wx(0)) + np.abs(wy(0)) + np.abs(wx(1)) + np.abs(wy(1)))
    assert np.isfinite(div).all() and scale.max() > 0
    print(f"{name}: max |div| {np.abs(div).max():.3e}, max allowed {8 * EPS * scale.max():.3e}, max |div| / scale {np.nanmax(np.abs(div) / np.where(scale > 0, scale, np.nan)) / EPS:.2f} eps")
    assert np.all(np.abs(div) <= 8 * EPS * scale)
    assert np.all(we(0, 0, 0)[:, :, 0] == 0) and np.all(we(0, 0, 1)[:, :, -1] == 0)  # no flow through the bottom and the top


@pytest.mark.parametrize("name", list(ISN.CASES))
def test_a_tapered_flux_is_the_untapered_one_times_the_ratio_of_squared_slopes(pkg, name):
    """where slope² > max_slope² (and bz > 0) every flux is exactly max_slope² / slope² times the flux of a closure that never tapers
    (max_slope = 1e300: ϵ = min(1, inf) = 1): -ϵ (…) with the same bracket"""
    g, cl, never = _describe(pkg, name), ISN.closure(), ISN.closure(max_slope=1e300)
    b, _, c = ISN.case_inputs(g, ISN.TRACER)
    G = ISN.face_gradients(g, ISN.TRACER, b, None)
    tapered, free = ISN.fluxes(g, ISN.TRACER, b, None, cl, 900.0, 400.0, c), ISN.fluxes(g, ISN.TRACER, b, None, never, 900.0, 400.0, c)
    for kind, ft, ff in zip(("fcc", "cfc", "ccf"), tapered, free):
        bx, by, bz = (f(0, 0, 0) for f in G[kind])
        with np.errstate(divide="ignore", invalid="ignore"):
            slope2 = (-bx / bz) * (-bx / bz) + (-by / bz) * (-by / bz)
            where = (bz > 0) & (slope2 > cl.max_slope ** 2)
            ratio = cl.max_slope * cl.max_slope / slope2
        assert where.mean() >= 0.05, kind
        assert np.array_equal(ft(0, 0, 0)[where], (ratio * ff(0, 0, 0))[where]), kind
        assert np.all(ratio[where] < 1) and np.abs(ff(0, 0, 0)[where]).max() > 0
        assert np.array_equal(ft(0, 0, 0)[(bz > 0) & ~where], ff(0, 0, 0)[(bz > 0) & ~where]), kind


# ---- 4. the shared input of the GPU tests ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("buoyancy", [ISN.TRACER, ISN.SEAWATER], ids=["b", "TS"])
@pytest.mark.parametrize("name", list(ISN.CASES))
def test_shared_input_covers_every_branch_and_the_restatement_has_no_nan(pkg, name, buoyancy):
    """at least 5 % of the x faces, of the y faces and of the z faces that the flux kernel evaluates lie in each branch -- untapered, tapered,
    ∂z b < 0, ∂z b == 0 (where ∂x b = ∂y b = 0 too: 0 / 0) -- and every output of the restatement is finite"""
    g, cl = _describe(pkg, name), ISN.closure()
    T, S, c = ISN.case_inputs(g, buoyancy)
    fractions = ISN.branch_fractions(g, buoyancy, T, S, cl)
    print(name, {kind: {k: round(float(v), 3) for k, v in f.items()} for kind, f in fractions.items()})
    for kind, f in fractions.items():
        for branch, fraction in f.items():
            assert fraction >= 0.05, (kind, branch, fraction)
    # the 0 / 0: x faces where ∂x b and ∂z b vanish exactly, and, where the block is three columns wide, all three gradients
    bx, by, bz = (f(0, 0, 0) for f in ISN.face_gradients(g, buoyancy, T, S)["fcc"])
    assert np.any((bx == 0) & (bz == 0))
    if name == "tile_plus_partial":
        for kind, G in ISN.face_gradients(g, buoyancy, T, S).items():
            bx, by, bz = (f(0, 0, 0) for f in G)
            assert np.mean((bx == 0) & (by == 0) & (bz == 0)) >= 0.05, kind
    zeros = {n: np.zeros(ISN.parent_shape(g, n in ("eps_R33", "w"))) for n in ("eps_R33", "u", "v", "w")}
    d = ISN.diffusivity_parents(g, buoyancy, T, S, cl, 1e3, zeros)
    outputs = list(d.values()) + [ISN.kz(g, d["eps_R33"], 900.0, zeros["eps_R33"])]
    outputs += [ISN.tracer_term(g, buoyancy, T, S, cl, 900.0, kw, f) for kw in (0.0, 400.0) for f in (T, c)]
    for a in outputs:
        assert np.isfinite(a).all()
    assert np.abs(d["u"]).max() > 0 and np.abs(d["w"]).max() > 0 and d["eps_R33"].max() > 0 and np.all(d["eps_R33"] >= 0)
    # ϵ R₃₃ = min(slope², max_slope²) where the water is stratified
    assert d["eps_R33"].max() <= cl.max_slope ** 2 * (1 + 4 * EPS)
