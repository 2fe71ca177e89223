"""RiBasedVerticalDiffusivity without a GPU: the constructor (every spelling of every keyword, the warning, repr) and the refusals (before any
allocation); the hand-written tapering functions through ocn_ri_taper_host (the inline functions the kernels call, run on the CPU) against
their NumPy restatement bit for bit and against an np.longdouble oracle within 4 x the rounding error of the Float64 reference formulas
(the criterion of DESIGN §6.1); the restatement itself (tests/ri_based_numpy.py) on hand-computed faces, the filter's weights and the
convergence of the time average; and the argument checks of the C entry points, which touch no device."""
import ctypes as C
import warnings

import numpy as np
import pytest

import implicit_diffusion_numpy as IDN
import ri_based_numpy as RBN

P, B, F = "Periodic", "Bounded", "Flat"
INVALID = -1  # OCN_ERR_INVALID_ARGUMENT (include/ocn_hip.h)
U53 = 2.0 ** -53


@pytest.fixture(scope="module")
def pkg():
    import oceananigans_jl_amd as ocn
    return ocn


def _grid(pkg, topo=(P, P, B), size=(4, 5, 6), z=(-1, 0)):
    return pkg.RectilinearGrid(None, size=size, x=(0, 1), y=(0, 1), z=z, topology=topo, halo=(3, 3, min(3, size[2])))


def _no_alloc(monkeypatch):
    import oceananigans_jl_amd.fields as fields

    def no_alloc(*a, **k):
        raise AssertionError("a field was allocated before the refusal")
    monkeypatch.setattr(fields.Field, "__init__", no_alloc)


def _quiet(pkg, *a, **k):
    return pkg.RiBasedVerticalDiffusivity(*a, warning=False, **k)


# ---- constructor -------------------------------------------------------------------------------------------------------------------------
GREEK = {"nu_0": "ν₀", "kappa_0": "κ₀", "kappa_ca": "κᶜᵃ", "C_en": "Cᵉⁿ", "C_av": "Cᵃᵛ", "Ri_0": "Ri₀", "Ri_delta": "Riᵟ"}


def test_defaults_are_the_reference_s(pkg):
    """ri_based_vertical_diffusivity.jl:125-139"""
    c = _quiet(pkg)
    assert isinstance(c.time_discretization, pkg.VerticallyImplicitTimeDiscretization)
    assert isinstance(c.Ri_dependent_tapering, pkg.HyperbolicTangentRiDependentTapering) and c.horizontal_Ri_filter is None
    assert (c.nu_0, c.kappa_0, c.kappa_ca, c.C_en, c.C_av, c.Ri_0, c.Ri_delta) == (0.7, 0.5, 1.7, 0.1, 0.6, 0.1, 0.4)
    assert (c.minimum_entrainment_buoyancy_gradient, c.maximum_diffusivity, c.maximum_viscosity) == (1e-10, np.inf, np.inf)
    s = c.c_struct()
    assert (s.nu0, s.kappa0, s.kappa_ca, s.C_en, s.C_av, s.Ri0, s.Ri_delta) == (0.7, 0.5, 1.7, 0.1, 0.6, 0.1, 0.4)
    assert (s.minimum_entrainment_buoyancy_gradient, s.maximum_diffusivity, s.maximum_viscosity) == (1e-10, np.inf, np.inf)
    assert (s.tapering, s.horizontal_filter) == (pkg._lib.RI_TAPER_TANH, pkg._lib.RI_FILTER_NONE)
    from oceananigans_jl_amd.physics import has_diffusivity_fields, is_vertically_implicit, owns_eddy_fields
    assert is_vertically_implicit(c) and has_diffusivity_fields(c) and not owns_eddy_fields(c)
    assert not is_vertically_implicit(_quiet(pkg, pkg.ExplicitTimeDiscretization()))


def test_every_spelling_of_every_keyword(pkg):
    import unicodedata
    VI, EX = pkg.VerticallyImplicitTimeDiscretization, pkg.ExplicitTimeDiscretization
    for n, (ascii_name, greek) in enumerate(GREEK.items()):
        value = 0.25 + n
        spellings = {ascii_name, greek, unicodedata.normalize("NFKC", greek)}  # (the last is what Python makes of the identifier in source)
        for name in spellings:
            c = _quiet(pkg, **{name: value})
            assert getattr(c, ascii_name) == value
            assert getattr(c, greek) == value  # the reference's field names read back too
            others = [k for k in GREEK if k != ascii_name]
            assert all(getattr(c, k) == pkg.RiBasedVerticalDiffusivity.DEFAULTS[k] for k in others)
        with pytest.raises(TypeError, match="twice"):
            _quiet(pkg, **{ascii_name: 1.0, greek: 1.0})
    # the four that Python accepts in source, as written
    c = _quiet(pkg, κᶜᵃ=2, Cᵉⁿ=0.2, Cᵃᵛ=0.3, Riᵟ=np.float64(0.5))
    assert (c.kappa_ca, c.C_en, c.C_av, c.Ri_delta) == (2.0, 0.2, 0.3, 0.5) and c.κᶜᵃ == 2.0 and c.Riᵟ == 0.5
    c = _quiet(pkg, minimum_entrainment_buoyancy_gradient=1e-8, maximum_diffusivity=10, maximum_viscosity=5)
    assert (c.minimum_entrainment_buoyancy_gradient, c.maximum_diffusivity, c.maximum_viscosity) == (1e-8, 10.0, 5.0)
    for c in (_quiet(pkg, EX()), _quiet(pkg, "Explicit"), _quiet(pkg, time_discretization=EX)):
        assert isinstance(c.time_discretization, EX)
    assert isinstance(_quiet(pkg, VI()).time_discretization, VI)
    L = pkg._lib
    for cls, code in ((pkg.PiecewiseLinearRiDependentTapering, L.RI_TAPER_LINEAR), (pkg.ExponentialRiDependentTapering, L.RI_TAPER_EXP),
                      (pkg.HyperbolicTangentRiDependentTapering, L.RI_TAPER_TANH)):
        for given in (cls, cls()):
            c = _quiet(pkg, Ri_dependent_tapering=given)
            assert type(c.Ri_dependent_tapering) is cls and c.c_struct().tapering == code
    for given in (pkg.FivePointHorizontalFilter, pkg.FivePointHorizontalFilter()):
        c = _quiet(pkg, horizontal_Ri_filter=given)
        assert isinstance(c.horizontal_Ri_filter, pkg.FivePointHorizontalFilter) and c.c_struct().horizontal_filter == L.RI_FILTER_FIVE_POINT


def test_warning_and_repr(pkg):
    with pytest.warns(UserWarning, match="experimental turbulence closure"):
        pkg.RiBasedVerticalDiffusivity()
    with pytest.warns(UserWarning, match="Use with caution and report bugs"):
        pkg.RiBasedVerticalDiffusivity(warning=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        pkg.RiBasedVerticalDiffusivity(warning=False)
    # Base.show (ri_based_vertical_diffusivity.jl:347-361), numbers as prettysummary(::AbstractFloat) prints them
    assert repr(_quiet(pkg)) == "\n".join([
        "RiBasedVerticalDiffusivity{VerticallyImplicitTimeDiscretization}",
        "├── Ri_dependent_tapering: HyperbolicTangentRiDependentTapering",
        "├── κ₀: 0.5", "├── ν₀: 0.7", "├── κᶜᵃ: 1.7", "├── Cᵉⁿ: 0.1", "├── Cᵃᵛ: 0.6", "├── Ri₀: 0.1", "├── Riᵟ: 0.4",
        "├── maximum_diffusivity: Inf", "└── maximum_viscosity: Inf"])
    r = repr(_quiet(pkg, "Explicit", Ri_dependent_tapering=pkg.ExponentialRiDependentTapering(), kappa_0=1, nu_0=1e-5, maximum_diffusivity=1234567.0,
                    C_en=1 / 3, maximum_viscosity=100))
    assert r.startswith("RiBasedVerticalDiffusivity{ExplicitTimeDiscretization}\n├── Ri_dependent_tapering: ExponentialRiDependentTapering\n")
    for line in ("├── κ₀: 1.0", "├── ν₀: 1.0e-5", "├── Cᵉⁿ: 0.333333", "├── maximum_diffusivity: 1.23457e6", "└── maximum_viscosity: 100.0"):
        assert line in r.split("\n")


def test_what_is_not_implemented_says_so(pkg):
    for bad in (lambda x, y, z, t: 1.0, np.ones(3), (1.0, 2.0), {"T": 1.0}, "1", True):
        for name in ("ν₀", "kappa_0", "κᶜᵃ", "C_en", "Cᵃᵛ", "Ri_0", "Riᵟ", "maximum_diffusivity", "minimum_entrainment_buoyancy_gradient"):
            with pytest.raises(NotImplementedError, match="must be a number"):
                _quiet(pkg, **{name: bad})
    VI = pkg.VerticallyImplicitTimeDiscretization
    with pytest.raises(TypeError, match="twice"):
        _quiet(pkg, VI(), time_discretization=VI())
    with pytest.raises(TypeError, match="unexpected"):
        _quiet(pkg, kappa=1)
    with pytest.raises(TypeError, match="one positional"):
        _quiet(pkg, VI(), 1.0)
    with pytest.raises(ValueError, match="time_discretization"):
        _quiet(pkg, "Implicit")
    with pytest.raises(TypeError, match="Ri_dependent_tapering"):
        _quiet(pkg, Ri_dependent_tapering="tanh")
    with pytest.raises(TypeError, match="horizontal_Ri_filter"):
        _quiet(pkg, horizontal_Ri_filter=5)


def test_model_refusals_come_before_any_allocation(pkg, monkeypatch):
    _no_alloc(monkeypatch)
    g = _grid(pkg)
    FBC, Hy = pkg.FieldBoundaryConditions, pkg.HydrostaticFreeSurfaceModel
    for closure in (_quiet(pkg), _quiet(pkg, "Explicit", horizontal_Ri_filter=pkg.FivePointHorizontalFilter())):
        with pytest.raises(NotImplementedError, match="RiBasedVerticalDiffusivity on NonhydrostaticModel"):
            pkg.NonhydrostaticModel(g, advection=pkg.WENO(), tracers=("b",), buoyancy=pkg.BuoyancyTracer(), closure=closure)
        with pytest.raises(NotImplementedError, match="RiBasedVerticalDiffusivity runs the reference's launch sequence \\(fused = False\\)"):
            Hy(g, closure=closure, free_surface=pkg.ExplicitFreeSurface(), fused=True)
        with pytest.raises(NotImplementedError, match="RiBasedVerticalDiffusivity with SplitRungeKutta3"):
            Hy(g, closure=closure, free_surface=pkg.SplitExplicitFreeSurface(substeps=10), timestepper="SplitRungeKutta3")
        with pytest.raises(NotImplementedError, match="closure tuples"):
            Hy(g, closure=(closure, pkg.ScalarDiffusivity(ν=1e-2)), free_surface=pkg.ExplicitFreeSurface())
        with pytest.raises(NotImplementedError):
            pkg.NonhydrostaticModel(g, advection=pkg.WENO(), closure=(closure,))

        class FakeDistributed:  # what the models ask of a Distributed architecture
            partition = object()
            communicates = True
        gs = _grid(pkg)
        gs.architecture = FakeDistributed()
        gs.topology = (pkg.FullyConnected, P, B)
        with pytest.raises(NotImplementedError, match="RiBasedVerticalDiffusivity on a slab-partitioned \\(Distributed\\)"):
            Hy(gs, closure=closure, free_surface=pkg.SplitExplicitFreeSurface(substeps=10))
        # a Flat x or y
        for flat in (pkg.RectilinearGrid(None, size=(8, 6), x=(0, 1), z=(-1, 0), topology=(P, F, B), halo=(3, 3)),
                     pkg.RectilinearGrid(None, size=(8, 6), y=(0, 1), z=(-1, 0), topology=(F, P, B), halo=(3, 3))):
            with pytest.raises(NotImplementedError):
                Hy(flat, closure=closure, free_surface=pkg.ExplicitFreeSurface(), tracers=("b",), buoyancy=pkg.BuoyancyTracer())
        # a top Value or Gradient condition on a buoyancy tracer is no buoyancy flux
        for make in (pkg.ValueBoundaryCondition, pkg.GradientBoundaryCondition):
            for tracers, buoyancy, name in ((("T", "S"), pkg.SeawaterBuoyancy(), "T"), (("T", "S"), pkg.SeawaterBuoyancy(), "S"),
                                            (("b",), pkg.BuoyancyTracer(), "b")):
                with pytest.raises(NotImplementedError, match=f"top boundary condition of {name} must be a FluxBoundaryCondition"):
                    Hy(g, closure=closure, tracers=tracers, buoyancy=buoyancy, boundary_conditions={name: FBC(top=make(1.0))})


# ---- the tapering functions ------------------------------------------------------------------------------------------------------------------
PARAMETERS = [(0.0, 1.0), (0.1, 0.4)]  # (x₀, δ): the argument itself, and the reference's defaults Ri₀, Riᵟ
KINDS = [(RBN.LINEAR, "Linear"), (RBN.EXP, "Exp"), (RBN.TANH, "Tanh")]
_samples = {}


def _sample(x0, delta):
    """the fixed seeded sample: 2 10⁶ points uniform in (x - x₀) / δ over [-25, 25], 10⁶ over [-1, 1], 2 10⁵ over [-10⁻³, 10⁻³] and 5 10⁵ over
    [-5, 60] (the Exp taper's range; the others take it too)"""
    if (x0, delta) not in _samples:
        rng = np.random.default_rng(20260119)
        q = np.concatenate([rng.uniform(-25, 25, 2_000_000), rng.uniform(-1, 1, 1_000_000), rng.uniform(-1e-3, 1e-3, 200_000),
                            rng.uniform(-5, 60, 500_000)])
        _samples[(x0, delta)] = x0 + delta * q
    return _samples[(x0, delta)]


def _host(pkg, kind, x, x0, delta):
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.full(x.shape, -7.0)
    pkg._lib.call("ocn_ri_taper_host", kind, x.size, x.ctypes.data, float(x0), float(delta), out.ctypes.data)
    return out


def _specials(x0, delta):
    """±inf, NaN, ±0, the break points of the Linear taper and their neighbours, the thresholds of the hand-written exp / tanh"""
    pts = [np.inf, -np.inf, np.nan, 0.0, -0.0, x0, x0 + delta, np.nextafter(x0, -np.inf), np.nextafter(x0, np.inf),
           np.nextafter(x0 + delta, -np.inf), np.nextafter(x0 + delta, np.inf), 1e300, -1e300, 5e-324, -5e-324]
    pts += [x0 + delta * q for q in (20.0, np.nextafter(20.0, 30.0), -20.0, 19.5, 700.0, 708.0, 709.5, 740.0, 745.0, 745.2, 746.0, 746.5, 800.0,
                                     0.5 * np.log(2.0), np.log(2.0), 1.5 * np.log(2.0), 10.0, -10.0)]
    return np.array(pts)


@pytest.mark.parametrize("x0,delta", PARAMETERS)
@pytest.mark.parametrize("kind,name", KINDS)
def test_host_entry_equals_the_restatement_bit_for_bit(pkg, kind, name, x0, delta):
    x = np.concatenate([_sample(x0, delta), _specials(x0, delta)])
    got, want = _host(pkg, kind, x, x0, delta), RBN.taper(kind, x, x0, delta)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got).sum() == 1  # the NaN comes back, nothing else turns into one
    assert np.array_equal(got, want, equal_nan=True)
    assert np.all((got[~np.isnan(got)] >= 0) & (got[~np.isnan(got)] <= 1))
    # the limits: an Ri of +inf occurs wherever the water is at rest and stably stratified
    lim = _host(pkg, kind, np.array([np.inf, -np.inf, 1e300, -1e300]), x0, delta)
    assert np.array_equal(lim, [0.0, 1.0, 0.0, 1.0])
    assert np.isnan(_host(pkg, kind, np.array([np.nan]), x0, delta)[0])
    if kind == RBN.LINEAR:  # equal to NumPy's own formula exactly, break points included
        assert np.array_equal(got, RBN.taper_reference(kind, x, x0, delta), equal_nan=True)
        assert _host(pkg, kind, np.array([x0, x0 + delta]), x0, delta).tolist() == [1.0, 0.0]


@pytest.mark.parametrize("x0,delta", PARAMETERS)
@pytest.mark.parametrize("kind,name", KINDS[1:])
def test_tapers_meet_the_accuracy_bound(pkg, kind, name, x0, delta):
    """DESIGN §6.1's criterion: max |τ - τ_LD| <= 4 E_ref, E_ref = max |τ₆₄ - τ_LD| with τ₆₄ the reference formula in NumPy Float64 and τ_LD the
    same formula in np.longdouble (a 63-bit mantissa), both computed here from the formulas alone.  Measured (x₀ = 0, δ = 1):
    Exp E_ref = 0.70 2⁻⁵³, E = 1.00 2⁻⁵³; Tanh E_ref = 0.93 2⁻⁵³, E = 1.26 2⁻⁵³; with the reference's defaults (0.1, 0.4): Exp 1.10 / 1.11,
    Tanh 1.19 / 1.52."""
    assert np.finfo(np.longdouble).nmant >= 63
    x = _sample(x0, delta)
    oracle = RBN.taper_reference(kind, x, x0, delta, np.longdouble)
    E_ref = float(np.abs(RBN.taper_reference(kind, x, x0, delta, np.float64) - oracle).max())
    E = float(np.abs(_host(pkg, kind, x, x0, delta).astype(np.longdouble) - oracle).max())
    print(f"{name} x0={x0} delta={delta}: E_ref = {E_ref / U53:.3f} 2^-53, E = {E / U53:.3f} 2^-53, ratio {E / E_ref:.3f}")
    assert 0.4 * U53 < E_ref < 2 * U53  # (the yardstick itself is what a rounded Float64 evaluation gives)
    assert E <= 4 * E_ref


def test_hand_written_exp_and_tanh_alone():
    """The two functions the tapers are made of, on their whole domain, against np.longdouble.  Bounds from the rounding analysis of
    csrc/ocn_taper.h, not from its output:
      exp_nonpositive = 2^k p, p = 1 + r p₁ in [0.707, 1.414]: r carries half an ulp of its own (<= 2⁻⁵⁵, times p), p₁ its own rounding plus
      what Horner's rule passes up (<= 1.2 2⁻⁵³, times |r| <= 0.35), the product r p₁ half an ulp (2⁻⁵⁵), the last sum half an ulp of p.  For
      p < 1 (ulp 2⁻⁵³) that adds up to (0.25 + 0.25 + 0.25 + 0.5) 2⁻⁵³ = 1.25 ulp, for p >= 1 (ulp 2⁻⁵²) to 2.0 2⁻⁵³ = 1.0 ulp: bound 1.5 ulp
      down to the smallest normal number (the scaling is exact there); monotone into the subnormal range.
      tanh_absolute = (1 - e) / (1 + e): with δe <= 1.5 ulp(e) <= 3 e 2⁻⁵³, half an ulp on numerator (2⁻⁵⁴), denominator (2⁻⁵³) and quotient
      (2⁻⁵⁴), |δt| <= ((3 e + 0.5) + t (3 e + 1)) / (1 + e) 2⁻⁵³ + 0.5 2⁻⁵³, at most 2.4 2⁻⁵³ over e in [0, 1]: bound 2.5 2⁻⁵³, absolutely."""
    rng = np.random.default_rng(3)
    x = -np.concatenate([rng.uniform(0, 1, 200_000), rng.uniform(0, 708, 400_000), 10.0 ** rng.uniform(-300, 0, 100_000)])
    e = RBN.exp_nonpositive(x)
    ref = np.exp(x.astype(np.longdouble))
    worst = float((np.abs(e - ref) / np.spacing(ref.astype(np.float64))).max())
    print(f"exp_nonpositive: worst error {worst:.3f} ulp")
    assert worst <= 1.5
    tail = np.linspace(-746.5, -700.0, 20_001)
    et = RBN.exp_nonpositive(tail)
    assert np.all(np.diff(et) >= 0) and et[0] == 0.0 and et[-1] > 0 and RBN.exp_nonpositive(np.array([-745.0]))[0] == 5e-324
    assert RBN.exp_nonpositive(np.array([0.0, -0.0, -np.inf])).tolist() == [1.0, 1.0, 0.0]
    y = np.concatenate([rng.uniform(-25, 25, 400_000), rng.uniform(-1e-3, 1e-3, 100_000)])
    t = RBN.tanh_absolute(y)
    assert np.array_equal(t, -RBN.tanh_absolute(-y))
    worst = float(np.abs(t - np.tanh(y.astype(np.longdouble))).max())
    print(f"tanh_absolute: worst error {worst / U53:.3f} 2^-53")
    assert worst <= 2.5 * U53
    assert RBN.tanh_absolute(np.array([np.inf, -np.inf, 0.0])).tolist() == [1.0, -1.0, 0.0]


# ---- the restatement itself ------------------------------------------------------------------------------------------------------------------
def _column_case(pkg):
    """a (4, 4, 4) grid with Δz = 1, a buoyancy tracer b = (0, 2, 2.5, 1.5) and u = (0, 1, 1, 1) in every column, v = 0, no-flux halos"""
    g = IDN.describe(_grid(pkg, size=(4, 4, 4), z=(-4, 0)))
    shape = (g.Nx + 2 * g.Hx, g.Ny + 2 * g.Hy, g.Nz + 2 * g.Hz)
    b, u, v = np.zeros(shape), np.zeros(shape), np.zeros(shape)
    b[:, :, g.Hz - 1:g.Hz + 5] = [0.0, 0.0, 2.0, 2.5, 1.5, 1.5]
    u[:, :, g.Hz - 1:g.Hz + 5] = [0.0, 0.0, 1.0, 1.0, 1.0, 1.0]
    return g, b, u, v


def test_hand_computed_stable_convecting_and_entraining_faces(pkg):
    """Linear taper, Ri₀ = 0, Riᵟ = 4, Jᵇ = 0.25, the other parameters the defaults:
      face 1: the periphery, κ⁺ = 0 whatever is there
      face 2: N² = 2, S² = 0.5 (1 + 1) + 0 = 1, Ri = 2, τ = 1 - 2 / 4 = 0.5                 -> κᶜ⁺ = 0.5 κ₀ = 0.25, κᵘ⁺ = 0.5 ν₀ = 0.35   (stable)
      face 3: N² = 0.5 > 1e-10, N²(4) = -1 < 0, Jᵇ > 0; S² = 0, Ri = +inf, τ = 0            -> κᶜ⁺ = Cᵉⁿ Jᵇ / N² = 0.05, κᵘ⁺ = 0          (entraining)
      face 4: N² = -1 < 0, Ri = 0, τ = 1                                                  -> κᶜ⁺ = κᶜᵃ + κ₀ = 2.2, κᵘ⁺ = ν₀ = 0.7       (convecting)"""
    g, b, u, v = _column_case(pkg)
    cl = RBN.closure_dict(tapering=RBN.LINEAR, Ri0=0.0, Ri_delta=4.0)
    sentinel = np.full(RBN.ccf_shape(g), -7.0)
    Ri = RBN.ri_number(g, "BuoyancyTracer", u, v, b, None, sentinel)
    col = Ri[g.Hx + 1, g.Hy + 2, g.Hz:g.Hz + 5]
    assert col.tolist() == [0.0, 2.0, np.inf, 0.0, -7.0]  # (face 1: N² = 0 over the no-flux bottom; face Nz + 1 is not written)
    kc, ku, br = RBN.new_diffusivities(g, "BuoyancyTracer", cl, b, None, 0.25, None, Ri)
    assert kc[1, 2].tolist() == [0.0, 0.5 * 0.5, 0.1 * 0.25 / 0.5, 1.7 + 0.0 + 0.5 * 1.0]
    assert ku[1, 2].tolist() == [0.0, 0.7 * 0.5, 0.0, 0.7]
    assert br["convecting"][1, 2].tolist() == [False, False, False, True] and br["entraining"][1, 2].tolist() == [False, False, True, False]
    # no entrainment without a positive flux, below the minimum gradient, or with Cᵉⁿ = 0
    for top, kw in ((0.0, {}), (-0.25, {}), (None, {}), (0.25, dict(minimum_entrainment_buoyancy_gradient=0.5)), (0.25, dict(C_en=0.0))):
        k2, _, _ = RBN.new_diffusivities(g, "BuoyancyTracer", dict(cl, **kw), b, None, top, None, Ri)
        assert k2[1, 2, 2] == 0.0
    # the flux as an array and as value + coeff b[i, j, Nz] give the same
    for top in (np.full((g.Nx, g.Ny), 0.25), (0.1, 0.1)):
        k2, _, _ = RBN.new_diffusivities(g, "BuoyancyTracer", cl, b, None, top, None, Ri)
        assert k2[1, 2, 2] == 0.1 * (0.25 if not isinstance(top, tuple) else 0.1 + 0.1 * 1.5) / 0.5
    # SeawaterBuoyancy: Jᵇ = g (α J_T - β J_S), ∂z b = g (α ∂z T - β ∂z S): T alone with g α = 1 is the same column
    sea = ("SeawaterBuoyancy", 2.0, 0.5, 0.25)
    k3, _, _ = RBN.new_diffusivities(g, sea, cl, b, np.zeros_like(b), 0.25, 0.0, Ri)
    assert np.array_equal(k3, kc)
    k4, _, _ = RBN.new_diffusivities(g, sea, cl, b, np.zeros_like(b), 0.25, 0.5, Ri)  # Jᵇ = 2 (0.125 - 0.125) = 0: not entraining
    assert k4[1, 2, 2] == 0.0
    # the maxima clip, the time average starts from what the fields hold
    kc5, ku5, br5 = RBN.new_diffusivities(g, "BuoyancyTracer", dict(cl, maximum_diffusivity=1.0, maximum_viscosity=0.5), b, None, 0.25, None, Ri)
    assert kc5[1, 2].tolist() == [0.0, 0.25, 0.05, 1.0] and ku5[1, 2].tolist() == [0.0, 0.35, 0.0, 0.5]
    assert br5["clipped_c"][1, 2].tolist() == [False, False, False, True]
    old = np.full(RBN.ccf_shape(g), 1.0)
    a, c2 = RBN.diffusivities(g, "BuoyancyTracer", cl, b, None, 0.25, None, Ri, old, old)
    assert a[g.Hx + 1, g.Hy + 2, g.Hz:g.Hz + 5].tolist() == [(0.6 * 1.0 + x) / (1 + 0.6) for x in kc[1, 2].tolist()] + [1.0]
    mask = np.ones(a.shape, dtype=bool)
    mask[g.Hx:g.Hx + g.Nx, g.Hy:g.Hy + g.Ny, g.Hz:g.Hz + g.Nz] = False
    assert np.all(a[mask] == 1.0) and np.all(c2[mask] == 1.0)  # the halos and face Nz + 1 keep what they held


def test_filter_keeps_constants_and_its_weights_sum_to_one(pkg):
    w = RBN.filter_weights()
    assert w.tolist() == [[1 / 16, 1 / 8, 1 / 16], [1 / 8, 1 / 4, 1 / 8], [1 / 16, 1 / 8, 1 / 16]] and w.sum() == 1.0
    g = IDN.describe(_grid(pkg, size=(5, 4, 3)))
    for value in (0.3, 1e300, np.inf, 0.0):
        out = RBN.five_point_filter(g, np.full(RBN.ccf_shape(g), value))
        assert np.all(out == value)
    rng = np.random.default_rng(5)
    Ri = RBN.fill_xy_halos(g, rng.uniform(0, 2, RBN.ccf_shape(g)))
    out = RBN.five_point_filter(g, Ri)
    inner = Ri[g.Hx:g.Hx + g.Nx, g.Hy:g.Hy + g.Ny, g.Hz:g.Hz + g.Nz]
    assert abs(out.sum() - inner.sum()) < 1e-12 * inner.sum() and out.std() < inner.std()  # periodic: the mean is kept, the noise is damped
    assert np.isnan(RBN.five_point_filter(g, np.full(RBN.ccf_shape(g), np.nan))).all()


@pytest.mark.parametrize("C_av", [0.6, 0.0, 3.0])
def test_time_average_converges_with_ratio_cav_over_one_plus_cav(pkg, C_av):
    """with a frozen state κ⁺ is the same at every call, so κ - κ⁺ shrinks by Cᵃᵛ / (1 + Cᵃᵛ) per call (to rounding)"""
    g, b, u, v = _column_case(pkg)
    cl = RBN.closure_dict(tapering=RBN.LINEAR, Ri0=0.0, Ri_delta=4.0, C_av=C_av)
    Ri = RBN.ri_number(g, "BuoyancyTracer", u, v, b, None, np.zeros(RBN.ccf_shape(g)))
    target, _, _ = RBN.new_diffusivities(g, "BuoyancyTracer", cl, b, None, 0.25, None, Ri)
    kc = ku = np.zeros(RBN.ccf_shape(g))
    sl = (slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny), slice(g.Hz, g.Hz + g.Nz))
    ratio = C_av / (1 + C_av)
    for n in range(1, 9):
        kc, ku = RBN.diffusivities(g, "BuoyancyTracer", cl, b, None, 0.25, None, Ri, kc, ku)
        assert np.allclose(kc[sl] - target, -target * ratio ** n, rtol=0, atol=1e-14)
    assert np.all(np.abs(kc[sl] - target) <= max(ratio ** 8, 1e-15) * target.max() + 1e-14)


# ---- C ABI: argument checks before any HIP call ------------------------------------------------------------------------------------------
def test_c_abi_argument_checks_touch_no_device(pkg):
    lib, L = pkg._lib.lib(), pkg._lib
    g = _grid(pkg, size=(16, 16, 8))
    p = [C.c_void_p(8 * n) for n in range(1, 7)]  # never dereferenced
    bad_z = (_grid(pkg, topo=(P, P, P)), pkg.RectilinearGrid(None, size=(16, 16), x=(0, 1), y=(0, 1), topology=(P, P, F), halo=(3, 3)))
    thin = pkg.RectilinearGrid(None, size=(16, 16, 8), x=(0, 1), y=(0, 1), z=(-1, 0), topology=(P, P, B), halo=(3, 3, 0))
    slice_xz = pkg.RectilinearGrid(None, size=(16, 8), x=(0, 1), z=(-1, 0), topology=(P, F, B), halo=(3, 3))
    terms = L.CModelTerms()
    cl = _quiet(pkg).c_struct()
    none = C.POINTER(L.CBc)()
    ri = lambda grid, t=terms: lib.ocn_compute_ri_number(grid, C.byref(t), p[0], p[1], p[2], None)
    dif = lambda grid, t=terms, c=cl, tops=(none, none), f=(p[2], p[3], p[4]): lib.ocn_compute_ri_based_diffusivities(
        grid, C.byref(t), C.byref(c), *tops, *f, None)
    fus = lambda grid, t=terms, c=cl, tops=(none, none), f=(p[2], p[3], p[4]): lib.ocn_compute_ri_based_diffusivities_fused(
        grid, C.byref(t), C.byref(c), *tops, p[0], p[1], *f, None)
    for call in (ri, dif, fus):
        for bad in bad_z:
            assert call(bad.cref) == INVALID and b"Bounded in the z-direction" in lib.ocn_last_error()
        assert call(thin.cref) == INVALID and b"halo" in lib.ocn_last_error()
        assert call(slice_xz.cref) == INVALID and b"Flat x or y" in lib.ocn_last_error()
        assert call(None) == INVALID
        # a NULL tracer for the buoyancy kind
        for kind, wording in ((L.BUOYANCY_TRACER, b"T (or b) tracer is NULL"), (L.BUOYANCY_SEAWATER_TS, b"tracer is NULL"),
                              (L.BUOYANCY_SEAWATER_T, b"T (or b) tracer is NULL"), (L.BUOYANCY_SEAWATER_S, b"S tracer is NULL"),
                              (9, b"unknown buoyancy")):
            t = L.CModelTerms()
            t.buoyancy = kind
            assert call(g.cref, t) == INVALID and wording in lib.ocn_last_error()
    assert lib.ocn_compute_ri_number(g.cref, None, p[0], p[1], p[2], None) == INVALID and b"null terms" in lib.ocn_last_error()
    for q in range(3):
        args = [p[0], p[1], p[2]]
        args[q] = None
        assert lib.ocn_compute_ri_number(g.cref, C.byref(terms), *args, None) == INVALID and b"null field pointer" in lib.ocn_last_error()
    for call in (dif, fus):
        # aliased output arrays
        for f in ((p[2], p[3], p[3]), (p[2], p[2], p[4]), (p[2], p[3], p[2])):
            assert call(g.cref, f=f) == INVALID and b"three different arrays" in lib.ocn_last_error()
        for q in range(3):
            f = [p[2], p[3], p[4]]
            f[q] = None
            assert call(g.cref, f=tuple(f)) == INVALID and b"null field pointer" in lib.ocn_last_error()
        # an unknown tapering / filter code
        for code in (-1, 3, 7):
            c = _quiet(pkg).c_struct()
            c.tapering = code
            assert call(g.cref, c=c) == INVALID and b"unknown tapering code" in lib.ocn_last_error()
        for code in (-1, 2):
            c = _quiet(pkg).c_struct()
            c.horizontal_filter = code
            assert call(g.cref, c=c) == INVALID and b"unknown horizontal filter code" in lib.ocn_last_error()
        # coefficients: finite, the maxima no NaN (+inf is their default)
        for name in ("nu0", "kappa0", "kappa_ca", "C_en", "C_av", "Ri0", "Ri_delta", "minimum_entrainment_buoyancy_gradient"):
            for bad in (float("nan"), float("inf")):
                c = _quiet(pkg).c_struct()
                setattr(c, name, bad)
                assert call(g.cref, c=c) == INVALID and b"finite" in lib.ocn_last_error()
        for name in ("maximum_diffusivity", "maximum_viscosity"):
            c = _quiet(pkg).c_struct()
            setattr(c, name, float("nan"))
            assert call(g.cref, c=c) == INVALID and b"NaN" in lib.ocn_last_error()
        # a Value / Gradient top condition is no flux
        for kind in (L.BC_VALUE, L.BC_GRADIENT, L.BC_OPEN, 9):
            bc = L.CBc(kind, 0, 1.0, 0.0, None)
            assert call(g.cref, tops=(C.pointer(bc), none)) == INVALID and b"T (or b) tracer has kind" in lib.ocn_last_error()
            assert call(g.cref, tops=(none, C.pointer(bc))) == INVALID and b"S tracer has kind" in lib.ocn_last_error()
        assert lib.ocn_last_error() is not None
    assert lib.ocn_compute_ri_based_diffusivities(g.cref, C.byref(terms), None, none, none, p[2], p[3], p[4], None) == INVALID
    assert b"null closure" in lib.ocn_last_error()
    # the one-launch entry takes no filter
    c = _quiet(pkg, horizontal_Ri_filter=pkg.FivePointHorizontalFilter()).c_struct()
    assert fus(g.cref, c=c) == INVALID and b"horizontal filter reads the neighbours" in lib.ocn_last_error()
    for q in (0, 1):
        uv = [p[0], p[1]]
        uv[q] = None
        assert lib.ocn_compute_ri_based_diffusivities_fused(g.cref, C.byref(terms), C.byref(cl), none, none, *uv, p[2], p[3], p[4], None) == INVALID
        assert b"null field pointer" in lib.ocn_last_error()
    # the host entry
    x = np.zeros(4)
    out = np.zeros(4)
    assert lib.ocn_ri_taper_host(3, 4, x.ctypes.data, 0.0, 1.0, out.ctypes.data) == INVALID and b"unknown tapering code" in lib.ocn_last_error()
    assert lib.ocn_ri_taper_host(0, 4, None, 0.0, 1.0, out.ctypes.data) == INVALID
    assert lib.ocn_ri_taper_host(0, -1, x.ctypes.data, 0.0, 1.0, out.ctypes.data) == INVALID
    assert lib.ocn_ri_taper_host(0, 0, None, 0.0, 1.0, None) == 0
    assert "ocn_compute_ri_number" in L.EXPORTED_SYMBOLS and "ocn_ri_taper_host" in L.EXPORTED_SYMBOLS
