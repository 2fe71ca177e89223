"""Smagorinsky / SmagorinskyLilly without a GPU: constructors and refusals, a closed form that pins the NumPy restatement
(tests/smagorinsky_numpy.py) independently of its author, the branch coverage of the random inputs the GPU tests use, and the argument
checks of the C entry points (no device is touched)."""
import ctypes as C

import numpy as np
import pytest

import smagorinsky_numpy as SN

P, B, F = "Periodic", "Bounded", "Flat"
INVALID = -1  # OCN_ERR_INVALID_ARGUMENT (include/ocn_hip.h)


@pytest.fixture(scope="module")
def pkg():
    import oceananigans_jl_amd as ocn
    return ocn


def _grid(pkg, topo=(P, P, B), size=(4, 5, 6), arch=None):
    return pkg.RectilinearGrid(arch, size=size, x=(0, 1), y=(0, 1), z=(-1, 0), topology=topo, halo=(3, 3, 3))


def test_constructors_mirror_the_reference(pkg):
    s = pkg.Smagorinsky()
    assert s.coefficient == 0.16 and s.Pr == 1.0 and not s.lilly and s.C == 0.16 and s.Cb == 0.0
    c = pkg.LillyCoefficient()
    assert c.smagorinsky == 0.16 and c.reduction_factor == 1.0
    sl = pkg.SmagorinskyLilly()
    assert isinstance(sl, pkg.Smagorinsky) and sl.lilly and sl.C == 0.16 and sl.Cb == 1.0 and sl.Pr == 1.0
    same = pkg.Smagorinsky(coefficient=pkg.LillyCoefficient(smagorinsky=0.23, reduction_factor=0.5), Pr=2)
    sl2 = pkg.SmagorinskyLilly(C=0.23, Cb=0.5, Pr=2)
    assert (same.C, same.Cb, same.Pr, same.lilly) == (sl2.C, sl2.Cb, sl2.Pr, sl2.lilly) == (0.23, 0.5, 2.0, True)
    d = pkg.SmagorinskyLilly(Pr={"T": 1, "S": 0.5})
    assert d.Pr_of("T") == 1.0 and d.Pr_of("S") == 0.5
    with pytest.raises(ValueError, match="c"):
        d.Pr_of("c")
    cs = d.c_struct(("T", "S"))
    assert (cs.C, cs.Cb, cs.lilly, cs.n_tracers, cs.Pr[0], cs.Pr[1]) == (0.16, 1.0, 1, 2, 1.0, 0.5)
    n = pkg.Smagorinsky(coefficient=0.2).c_struct(())
    assert (n.C, n.Cb, n.lilly, n.n_tracers) == (0.2, 0.0, 0, 0)


def test_what_is_not_implemented_says_so(pkg):
    with pytest.raises(NotImplementedError):
        pkg.DynamicCoefficient(averaging=1)
    with pytest.raises(NotImplementedError):
        pkg.Smagorinsky(coefficient=pkg.DynamicCoefficient)
    with pytest.raises(NotImplementedError):
        pkg.DynamicSmagorinsky()
    with pytest.raises(NotImplementedError):
        pkg.Smagorinsky(time_discretization="VerticallyImplicit")
    with pytest.raises(NotImplementedError):
        pkg.SmagorinskyLilly(time_discretization="VerticallyImplicit")


def test_model_refusals_come_before_any_allocation(pkg, monkeypatch):
    import oceananigans_jl_amd.fields as fields

    def no_alloc(*a, **k):
        raise AssertionError("a field was allocated before the refusal")
    monkeypatch.setattr(fields.Field, "__init__", no_alloc)
    g = _grid(pkg)
    zero_flux = pkg.FieldBoundaryConditions(top=pkg.FluxBoundaryCondition(0.0))
    with pytest.raises(ValueError, match="κₑ"):
        pkg.NonhydrostaticModel(g, advection=pkg.WENO(), tracers=("T",), closure=pkg.SmagorinskyLilly(),
                                boundary_conditions={"κₑ": {"T": zero_flux}})
    with pytest.raises(ValueError, match="κₑ"):
        pkg.NonhydrostaticModel(g, advection=pkg.WENO(), tracers=("T",), closure=pkg.Smagorinsky(), boundary_conditions={"kappa_e": {"T": zero_flux}})
    with pytest.raises(ValueError, match="Pr given for tracer S"):
        pkg.NonhydrostaticModel(g, advection=pkg.WENO(), tracers=("T", "S"), closure=pkg.SmagorinskyLilly(Pr={"T": 1}))
    with pytest.raises(NotImplementedError, match="νₑ boundary condition"):
        pkg.NonhydrostaticModel(g, advection=pkg.WENO(), tracers=("T",), closure=pkg.SmagorinskyLilly(Pr=2),
                                boundary_conditions={"νₑ": pkg.FieldBoundaryConditions(top=pkg.ValueBoundaryCondition(0.0))})

    class FakeDistributed:  # what models.py asks of a Distributed architecture: a `partition`
        partition = object()
    gd = _grid(pkg)
    gd.architecture = FakeDistributed()
    with pytest.raises(NotImplementedError, match=r"Distributed architecture is not implemented \(see DESIGN.md\)"):
        pkg.NonhydrostaticModel(gd, advection=pkg.WENO(), closure=pkg.SmagorinskyLilly())
    with pytest.raises(NotImplementedError, match="non-Flat z"):
        pkg.NonhydrostaticModel(pkg.RectilinearGrid(None, size=(8, 8), x=(0, 1), y=(0, 1), topology=(P, P, F), halo=(3, 3)),
                                advection=pkg.WENO(), closure=pkg.Smagorinsky())


# ---- closed form ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shear,N2,Cb", [(1.5, -0.7, 1.0),   # N² < 0: ς = 1
                                         (1.5, 0.6, 1.0),    # 0 < Cb N² < S² / 2
                                         (1.5, 2.0, 0.75)])  # Cb N² > S² / 2: νₑ exactly 0
def test_closed_form_of_a_sheared_stratified_column(oracle, shear, N2, Cb):
    """u = S z at u's nodes, v = w = 0, b = N² z on (8, 8, 16), (Periodic, Periodic, Bounded), unit box: away from the walls
    Σ² = S² / 2 and νₑ = ς (C Δᶠ)² |S| with ς = sqrt(1 - min(1, Cb N² / (S² / 2))).  The only error is the rounding of differences of O(1)
    values over Δz = 1 / 16 (a few tens of ε): 1e-12 relative."""
    O = oracle
    og = O.Grid((8, 8, 16), x=(0, 1), y=(0, 1), z=(0, 1), topology="PPB", halo=(3, 3, 3))
    zc = og.nodes(2, False)
    u, v, w, b = og.zeros(1), og.zeros(2), og.zeros(4), og.zeros(0)
    og.interior(u)[...] = shear * zc[None, None, :]
    og.interior(b)[...] = N2 * zc[None, None, :]
    for a, loc in ((u, 1), (v, 2), (w, 4), (b, 0)):
        O.fill_halo_regions(og, a, loc)
    Cs = 0.16
    nu, S2, N2_, sig = SN.smagorinsky_viscosity(og, u, v, w, Cs, lilly=True, Cb=Cb, buoyancy="BuoyancyTracer", T=b, parts=True)
    core = (slice(None), slice(None), slice(1, og.Nz - 1))  # k = 2 .. Nz - 1
    Df = (1 / 8 * 1 / 8 * 1 / 16) ** (1 / 3)
    ratio = Cb * max(N2, 0.0) / (shear * shear / 2)
    expected_sig = np.sqrt(1 - min(1.0, ratio))
    expected = expected_sig * (Cs * Df) ** 2 * abs(shear)
    np.testing.assert_allclose(S2[core], shear * shear / 2, rtol=1e-12)
    np.testing.assert_allclose(N2_[core], N2, rtol=1e-12)
    if expected == 0:
        assert np.all(nu[core] == 0.0)
    else:
        np.testing.assert_allclose(nu[core], expected, rtol=1e-12)
    # the number coefficient: no stability function
    nu0 = SN.smagorinsky_viscosity(og, u, v, w, Cs)
    np.testing.assert_allclose(nu0[core], (Cs * Df) ** 2 * abs(shear), rtol=1e-12)


# ---- the random inputs of the GPU tests reach every branch -----------------------------------------------------------------------------
@pytest.mark.parametrize("setting", SN.SETTINGS[1:] + [SN.HALF_CB], ids=lambda s: s[0])
@pytest.mark.parametrize("size,topo,z,halo", SN.CASES)
def test_random_inputs_reach_every_branch(oracle, size, topo, z, halo, setting):
    O = oracle
    _, lilly, Cs, Cb, buoyancy = setting
    og = O.Grid(size, x=(0, 2 * np.pi), y=(0, 2 * np.pi), z=SN.case_z(size, z), topology=topo, halo=halo)
    f = SN.random_inputs(og, buoyancy)
    nu, S2, N2, sig = SN.smagorinsky_viscosity(og, f["u"], f["v"], f["w"], Cs, lilly=lilly, Cb=Cb, buoyancy=buoyancy, T=f["T"], S=f["S"],
                                               parts=True)
    assert np.isfinite(nu).all() and (nu >= 0).all()
    assert np.count_nonzero(S2 == 0) >= 1, "no cell with Σ² == 0"
    assert np.all(nu[S2 == 0] == 0.0)
    assert np.count_nonzero(N2 < 0) >= 1, "no cell with N² < 0"
    assert np.count_nonzero((sig > 0) & (sig < 1)) >= 1, "no cell with 0 < ς < 1"
    assert np.count_nonzero((sig == 0) & (S2 > 0)) >= 1, "no cell with ς == 0 and Σ² > 0"
    assert np.count_nonzero((sig == 1) & (S2 > 0)) >= 1


def test_a_constant_temperature_or_salinity_has_no_gradient(oracle):
    """SeawaterBuoyancy(constant_salinity = ...) / (constant_temperature = ...): ∂z of the constant is 0 (seawater_buoyancy.jl:219-224)"""
    O = oracle
    og = O.Grid((6, 6, 8), x=(0, 1), y=(0, 1), z=(-1, 0), topology="PPB", halo=(3, 3, 3))
    f = SN.random_inputs(og, SN.SEAWATER)
    g, alpha, beta = SN.SEAWATER[1:]
    both = SN.buoyancy_frequency(og, SN.SEAWATER, f["T"], f["S"])
    onlyT = SN.buoyancy_frequency(og, SN.SEAWATER, f["T"], None)
    onlyS = SN.buoyancy_frequency(og, SN.SEAWATER, None, f["S"])
    np.testing.assert_allclose(onlyT + onlyS, both, rtol=0, atol=1e-12 * np.abs(both).max())
    assert np.abs(onlyT).max() > 0 and np.abs(onlyS).max() > 0


# ---- C ABI: argument checks before any HIP call ------------------------------------------------------------------------------------------
def test_c_abi_argument_checks_touch_no_device(pkg):
    lib, L = pkg._lib.lib(), pkg._lib
    g = _grid(pkg, size=(16, 16, 8))
    one = C.c_void_p(8)  # never dereferenced
    f = lib.ocn_compute_smagorinsky_diffusivities

    def closure(lilly=0, n=0, Pr=()):
        s = L.CSmagorinsky()
        s.C, s.Cb, s.lilly, s.n_tracers = 0.16, float(lilly), lilly, n
        for q, p in enumerate(Pr):
            s.Pr[q] = p
        return s
    terms = L.CModelTerms()
    # a Flat z
    gf = pkg.RectilinearGrid(None, size=(16, 16), x=(0, 1), y=(0, 1), topology=(P, P, F), halo=(3, 3))
    assert f(gf.cref, C.byref(terms), C.byref(closure()), one, one, one, one, None, None) == INVALID
    assert b"non-Flat z" in lib.ocn_last_error()
    # null pointers
    assert f(g.cref, C.byref(terms), C.byref(closure()), one, one, one, None, None, None) == INVALID
    assert b"null field pointer" in lib.ocn_last_error()
    assert f(g.cref, None, C.byref(closure()), one, one, one, one, None, None) == INVALID
    assert f(g.cref, C.byref(terms), None, one, one, one, one, None, None) == INVALID
    # lilly with a buoyancy kind whose tracer pointer is NULL
    for kind, T, S in ((L.BUOYANCY_TRACER, None, None), (L.BUOYANCY_SEAWATER_TS, 8, None), (L.BUOYANCY_SEAWATER_TS, None, 8),
                       (L.BUOYANCY_SEAWATER_T, None, 8), (L.BUOYANCY_SEAWATER_S, 8, None)):
        t = L.CModelTerms()
        t.buoyancy, t.T, t.S = kind, T, S
        assert f(g.cref, C.byref(t), C.byref(closure(lilly=1)), one, one, one, one, None, None) == INVALID
        assert b"tracer is NULL" in lib.ocn_last_error()
    # Pr <= 0
    kap = L.ptr_array([8, 8])
    for bad in (0.0, -1.0):
        assert f(g.cref, C.byref(terms), C.byref(closure(n=2, Pr=(1.0, bad))), one, one, one, one, kap, None) == INVALID
        assert b"must be positive" in lib.ocn_last_error()
    # a NULL kappa_e[n] where Pr[n] != 1 (the whole array or one entry)
    assert f(g.cref, C.byref(terms), C.byref(closure(n=1, Pr=(2.0,))), one, one, one, one, None, None) == INVALID
    assert b"needs a kappa_e field" in lib.ocn_last_error()
    assert f(g.cref, C.byref(terms), C.byref(closure(n=2, Pr=(1.0, 0.5))), one, one, one, one, L.ptr_array([None, None]), None) == INVALID
    assert b"needs a kappa_e field" in lib.ocn_last_error()
    # ... and it cannot be the nu_e array
    assert f(g.cref, C.byref(terms), C.byref(closure(n=1, Pr=(2.0,))), one, one, one, one, L.ptr_array([8]), None) == INVALID
    # n_tracers outside 0..4, lilly neither 0 nor 1
    assert f(g.cref, C.byref(terms), C.byref(closure(n=5)), one, one, one, one, None, None) == INVALID
    assert f(g.cref, C.byref(terms), C.byref(closure(lilly=2)), one, one, one, one, None, None) == INVALID
    # the driver's setter
    assert lib.ocn_model_driver_set_smagorinsky(None, C.byref(closure())) == INVALID
    assert b"null driver" in lib.ocn_last_error()
