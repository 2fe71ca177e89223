"""CATKEVerticalDiffusivity without a GPU: the NumPy restatement of the reference (tests/catke_numpy.py) against what is certain independently
of its author -- break points, closed forms of special columns, a library cube root --, the constructors in every spelling, every refusal
before any allocation, the argument checks of the C entry points (no device is touched) and the host cube root of the library against the
restatement bit for bit."""
import ctypes as C
import math

import numpy as np
import pytest

import catke_numpy as CK
import implicit_diffusion_numpy as IDN
from helpers import stretched_faces

P, B, F = "Periodic", "Bounded", "Flat"
INVALID = -1  # OCN_ERR_INVALID_ARGUMENT (include/ocn_hip.h)
EPS = np.finfo(np.float64).eps
SEAWATER = ("SeawaterBuoyancy", 9.80665, 1.67e-4, 7.80e-4)


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


def _state(pkg, size=(3, 2, 8), z=(-64.0, 0.0), cl=None, b=None, e=1e-4, Jb=0.0, u=None, v=None, halo=(1, 1, 1)):
    """a column state with a buoyancy tracer b(z) (a function of the centre heights, or None: unstratified), uniform or given e, u, v"""
    pg = _grid(pkg, size=size, z=z, halo=halo)
    g = IDN.describe(pg)
    zf, zc = pg.nodes_1d(2, True), pg.nodes_1d(2, False)
    zc_all = pg.nodes_1d(2, False, with_halos=True)
    shape = pg.parent_shape(0)
    T = np.zeros(shape) + (b(zc_all) if b is not None else 0.0)
    full = lambda x, loc: np.zeros(pg.parent_shape(loc)) + (0.0 if x is None else x)
    e = np.zeros(shape) + e
    s = CK.State(g, zf, zc, pg.Lz, "BuoyancyTracer", cl or CK.closure_dict(), full(u, 1), full(v, 2), T, None, e, np.zeros((g.Nx, g.Ny)) + Jb)
    return pg, g, s


# ---- scalar functions -----------------------------------------------------------------------------------------------------------------------
def test_step_and_scale_at_their_break_points():
    c, w = 0.254, 1.02
    assert CK.step(c, c, w) == 0.0 and CK.step(np.nextafter(c, -1), c, w) == 0.0 and CK.step(-np.inf, c, w) == 0.0
    assert CK.step(c + w, c, w) <= 1.0 and CK.step(c + 2 * w, c, w) == 1.0 and CK.step(np.inf, c, w) == 1.0
    assert CK.step(c + w / 2, c, w) == pytest.approx(0.5, abs=2 * EPS) and np.isnan(CK.step(np.nan, c, w))
    un, lo, hi = 0.37, 0.361, 0.242
    assert CK.scale(-1e-300, un, lo, hi, c, w) == un and CK.scale(-np.inf, un, lo, hi, c, w) == un  # Ri < 0: σ⁻, whatever σ⁺ is
    assert CK.scale(0.0, un, lo, hi, c, w) == lo and CK.scale(c, un, lo, hi, c, w) == lo           # 0 <= Ri <= CRi⁰: σ⁰
    assert CK.scale(np.inf, un, lo, hi, c, w) == lo + (hi - lo) * 1.0                               # S² = 0 over a stable N²: σ∞
    assert CK.scale(c + w / 2, un, lo, hi, c, w) == pytest.approx(0.5 * (lo + hi), abs=4 * EPS)
    # Julia's max / min order the zeros and propagate a NaN; a false Bool is a strong zero
    assert not np.signbit(CK.jmax(0.0, -0.0)) and np.signbit(CK.jmin(0.0, -0.0)) and np.isnan(CK.jmax(0.0, np.nan)) and np.isnan(CK.jmin(np.nan, 1.0))
    assert CK.bmul(np.inf, False) == 0.0 and np.signbit(CK.bmul(-np.inf, False)) and CK.bmul(3.0, True) == 3.0 and CK.bmul(np.nan, False) == 0.0


def _ulps(a, b):
    ia, ib = np.asarray(a).view(np.int64), np.asarray(b).view(np.int64)
    return np.abs(ia - ib)


def _cbrt_sample():
    rng = np.random.default_rng(20261020)
    x = 10.0 ** rng.uniform(-30, 30, 2_000_000)
    x[::2] *= -1
    n = np.arange(1, 200_001, dtype=np.float64)
    return x, n


def test_hand_written_cbrt_against_numpy_s():
    """2 10⁶ seeded points of both signs, log-uniform over 1e-30 ... 1e30, and the exact cubes n³, n = 1 ... 2 10⁵.  Largest distance found to
    np.cbrt (glibc's, itself within 1 ulp of the cube root): 1 ulp, on 29.15 % of the sample; the exact cubes give n exactly.  Asserted: at most
    twice that."""
    x, n = _cbrt_sample()
    got = CK.cbrt(x)
    d = _ulps(got, np.cbrt(x))
    print(f"cbrt: max {d.max()} ulp, {100 * (d > 0).mean():.2f} % differ")
    assert d.max() <= 2
    cubes = CK.cbrt(n * n * n)
    dc = _ulps(cubes, n)
    print(f"cbrt of exact cubes: max {dc.max()} ulp")
    assert dc.max() <= 2
    s = np.array([0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 2.2250738585072014e-308, 1.7976931348623157e308])
    r = CK.cbrt(s)
    assert r[0] == 0 and not np.signbit(r[0]) and r[1] == 0 and np.signbit(r[1]) and r[2] == np.inf and r[3] == -np.inf
    assert _ulps(r[4:], np.cbrt(s[4:])).max() <= 2 and np.isnan(CK.cbrt(np.nan))


def test_host_cbrt_of_the_library_equals_the_restatement_bit_for_bit(pkg):
    x, n = _cbrt_sample()
    x = np.ascontiguousarray(np.concatenate([x, n * n * n, [0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 1e-310, 2.2250738585072014e-308,
                                                            1.7976931348623157e308, 8.0, 1.0]]))
    out = np.full(x.shape, -7.0)
    pkg._lib.call("ocn_catke_host_cbrt", x.size, x.ctypes.data, out.ctypes.data)
    assert np.array_equal(out, CK.cbrt(x)) and np.array_equal(np.signbit(out), np.signbit(CK.cbrt(x)))
    nan = np.array([np.nan])
    pkg._lib.call("ocn_catke_host_cbrt", 1, nan.ctypes.data, out.ctypes.data)
    assert np.isnan(out[0])


# ---- closed forms ---------------------------------------------------------------------------------------------------------------------------
def test_stably_stratified_column_at_rest_has_the_closed_form_kappa_c(pkg):
    """uniform e, no shear, N² > 0 uniform, no surface flux: Ri = +inf, σ = Cʰⁱc, no convective length:
    κc = Cʰⁱc min(Cˢ d, Cᵇ h, w★ / N) w★ on the interior faces, exactly 0 on faces 1 and Nz + 1"""
    N2 = 2e-6
    pg, g, s = _state(pkg, b=lambda z: N2 * z, e=3e-4)
    cl, w = s.cl, math.sqrt(3e-4)
    seen = set()
    for k in range(2, g.Nz + 1):
        n2 = float(CK.dz_b(s, k)[0, 0])  # (the difference quotient of N² z: N² to rounding)
        assert n2 == pytest.approx(N2, rel=1e-12)
        d, h = s.zf[g.Nz] - s.zf[k - 1], s.zf[k - 1] - s.zf[0]
        candidates = (cl["C_s"] * d, cl["C_b"] * h, w / math.sqrt(n2))
        seen.add(int(np.argmin(candidates)))
        want = cl["C_hi_c"] * min(candidates) * w
        # (σ = Cˡᵒ + (Cʰⁱ - Cˡᵒ) 1 is Cʰⁱ to an ulp, and so is the product)
        assert np.allclose(CK.kappa_ccf(s, k, "c"), want, rtol=4 * EPS, atol=0), k
    assert seen == {0, 1, 2}  # each of the three lengths limits somewhere
    for k in (1, g.Nz + 1):
        for which in "uce":
            assert np.all(CK.kappa_ccf(s, k, which) == 0.0) and not np.signbit(CK.kappa_ccf(s, k, which)).any()
    ku, kc, ke = CK.diffusivities(s, *(np.full(CK.ccf_shape(g), -7.0) for _ in range(3)))
    for a in (ku, kc, ke):
        assert np.all(a[g.Hx:-g.Hx, g.Hy:-g.Hy, g.Hz] == 0.0) and np.all(a[:, :, g.Hz + g.Nz:] == -7.0) and np.all(a[:g.Hx] == -7.0)
        assert np.all(a[g.Hx:-g.Hx, g.Hy:-g.Hy, g.Hz + 1:g.Hz + g.Nz] > 0)


def test_convecting_column_has_the_deardorff_length(pkg):
    """N² < 0, a surface flux Jᵇ > Jᵇᵋ and no shear (the sheared-convection factor is 1): ℓᶜ = Cᶜ w★³ / (Jᵇ + Jᵇᵋ); with Jᵇ <= Jᵇᵋ: 0"""
    Jb = 2e-8
    pg, g, s = _state(pkg, b=lambda z: -1e-6 * z, e=2e-4, Jb=Jb)
    w = math.sqrt(2e-4)
    w3 = 0.5 * (w * w * w + w * w * w)
    for k in range(2, g.Nz + 1):
        for which in "uce":
            Cc = s.cl[f"C_c_{which}"]
            l, convecting, entraining = CK.convective_length_ccf(s, k, Cc, s.cl[f"C_e_{which}"], with_branches=True)
            assert convecting.all() and not entraining.any()
            assert np.all(l == Cc * w3 / (Jb + 1e-11))
    s.Jb = np.zeros_like(s.Jb) + 1e-11  # not above the minimum
    assert np.all(CK.convective_length_ccf(s, 3, 4.793, 0.112) == 0.0)
    # the entrainment face: stable below an unstable face, ℓᵉ = Cᵉ Jᵇ / (w★ N² + Jᵇᵋ)
    pg, g, s = _state(pkg, b=lambda z: np.where(z < -30, 1e-5 * (z + 30), -1e-6 * (z + 30)), e=2e-4, Jb=Jb)
    found = 0
    for k in range(2, g.Nz):
        l, convecting, entraining = CK.convective_length_ccf(s, k, 4.793, 0.112, with_branches=True)
        if entraining.all():
            found += 1
            n2 = CK.dz_b(s, k)
            assert np.all(n2 > 0) and np.all(CK.dz_b(s, k + 1) < 0) and np.all(l == 0.112 * Jb / (w * n2 + 1e-11))
    assert found == 1


def test_uniform_e_decays_and_negative_e_relaxes(pkg):
    """no shear, no stratification (P = wb = 0), κᵉ clipped to 0: the substep and the solve give e / (1 + Δτ ω) with ω = √e / ℓᴰ away from the
    bottom cell, whose diagonal also holds Cᵂϵ √e / Δz; e < 0 relaxes with 1 / negative_tke_damping_time_scale; G⁻e becomes the slow tendency"""
    cl = CK.closure_dict(maximum_tke_diffusivity=0.0)
    for e0 in (1e-4, -1e-5):
        pg, g, s = _state(pkg, cl=cl, e=e0)
        zero_f, zero_c = np.zeros(CK.ccf_shape(g)), np.zeros(pg.parent_shape(0))
        dtau = 30.0
        e1, ke, Le, Gm, terms = CK.substep(s, s.u, s.v, zero_f, zero_f, zero_f, zero_c, zero_c, zero_c, dtau, 0.1, with_terms=True)
        assert np.all(terms["P"] == 0) and np.all(terms["wb"] == 0) and np.all(ke == 0) and np.array_equal(e1, s.e) and np.all(Gm == 0)
        e2 = CK.implicit_step_e(g, e1, ke, Le, dtau)
        sl = (slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny), slice(g.Hz, g.Hz + g.Nz))
        omega = terms["omega"]
        if e0 < 0:
            assert np.all(omega == 1 / 60.0)
            want = e0 / (1 + dtau / 60.0)
            assert np.allclose(e2[sl], want, rtol=4 * EPS, atol=0) and np.all(e2[sl] > e0)
        else:
            lD = np.stack([CK.dissipation_length(s, k) for k in range(1, g.Nz + 1)], axis=-1)
            assert np.array_equal(omega, math.sqrt(e0) / lD)
            want = e0 / (1 + dtau * omega)
            assert np.allclose(e2[sl][:, :, 1:], want[:, :, 1:], rtol=4 * EPS, atol=0)
            bottom = e0 / (1 + dtau * (omega[:, :, 0] + cl["C_W_eps"] * math.sqrt(e0) / s.dzC(1)))
            assert np.allclose(e2[sl][:, :, 0], bottom, rtol=4 * EPS, atol=0) and np.all(e2[sl][:, :, 0] < want[:, :, 0])
        assert np.array_equal(e2[:, :, :g.Hz], s.e[:, :, :g.Hz])  # halos untouched


def test_maxima_clip(pkg):
    pg, g, s = _state(pkg, b=lambda z: -1e-6 * z, e=2e-4, Jb=2e-8)
    free = {which: CK.kappa_ccf(s, 4, which) for which in "uce"}
    assert all(np.all(v > 1e-3) for v in free.values())
    s.cl = CK.closure_dict(maximum_viscosity=1e-3, maximum_tracer_diffusivity=2e-3, maximum_tke_diffusivity=3e-3)
    for which, m in zip("uce", (1e-3, 2e-3, 3e-3)):
        assert np.all(CK.kappa_ccf(s, 4, which) == m)


def test_substeps_open_with_an_euler_step(pkg):
    """tke_time_step = Δt / 3: M = 3 substeps of Δt / 3 with χ = -1/2, χ, χ; None: one substep with χ"""
    pg, g, s = _state(pkg, b=lambda z: 1e-5 * z, e=1e-4, u=0.0)
    rng = np.random.default_rng(3)
    s.u = s.u + 0.01 * rng.uniform(-1, 1, s.u.shape)
    zero_f, zero_c = np.zeros(CK.ccf_shape(g)), np.zeros(pg.parent_shape(0))
    ku = zero_f + 1e-3
    G = zero_c + 1e-9
    e3, ke, Le, Gm, chis = CK.time_step_tke(s, 0.5 * s.u, s.v, ku, zero_f, zero_f, zero_c, G, zero_c, 3.0, 1.0, 0.1)
    assert chis == [-0.5, 0.1, 0.1]
    e1, _, _, _, chis1 = CK.time_step_tke(s, 0.5 * s.u, s.v, ku, zero_f, zero_f, zero_c, G, zero_c, 3.0, None, 0.1)
    assert chis1 == [0.1] and not np.array_equal(e1, e3)
    # by hand: three substeps of 1.0
    e, Gm_h = s.e, zero_c
    for chi in (-0.5, 0.1, 0.1):
        sm = CK.State(s.g, s.zf, s.zc, s.Lz, s.buoyancy, s.cl, s.u, s.v, s.T, s.S, e, s.Jb)
        e, ke_h, Le_h, Gm_h = CK.substep(sm, 0.5 * s.u, s.v, ku, zero_f, zero_f, zero_c, G, Gm_h, 1.0, chi)
        e = CK.implicit_step_e(g, e, ke_h, Le_h, 1.0)
    assert np.array_equal(e, e3) and np.array_equal(Gm_h, Gm)
    assert CK.time_step_tke(s, s.u, s.v, ku, zero_f, zero_f, zero_c, G, zero_c, 3.0, 0.9, 0.1)[4] == [-0.5, 0.1, 0.1, 0.1]  # ceil


def test_implicit_step_of_e_solves_its_system(pkg):
    """(1 - Δτ ∂z κᵉ ∂z - Δτ Le) e⁺ = e: the residual of the restatement's solve against a dense matrix built from the formulas"""
    pg = _grid(pkg, size=(2, 2, 7), z=stretched_faces(7), halo=(1, 1, 2))
    g = IDN.describe(pg)
    rng = np.random.default_rng(11)
    e = rng.uniform(0, 1, pg.parent_shape(0))
    ke = rng.uniform(0.1, 1, CK.ccf_shape(g))
    ke[:, :, g.Hz] = 0
    ke[:, :, g.Hz + g.Nz] = 0
    Le = -rng.uniform(0, 2, pg.parent_shape(0))
    dt = 0.3
    out = CK.implicit_step_e(g, e, ke, Le, dt)
    i, j = g.Hx, g.Hy + 1
    A = np.zeros((g.Nz, g.Nz))
    for k in range(1, g.Nz + 1):
        dzc = g.dzc[g.Hz + k - 1]
        lo = dt * ke[i, j, g.Hz + k - 1] / (dzc * g.dzf[g.Hz + k - 1])
        up = dt * ke[i, j, g.Hz + k] / (dzc * g.dzf[g.Hz + k])
        A[k - 1, k - 1] = 1 - dt * Le[i, j, g.Hz + k - 1] + lo + up
        if k > 1:
            A[k - 1, k - 2] = -lo
        if k < g.Nz:
            A[k - 1, k] = -up
    col = slice(g.Hz, g.Hz + g.Nz)
    assert np.allclose(A @ out[i, j, col], e[i, j, col], rtol=0, atol=64 * EPS)


# ---- constructors ---------------------------------------------------------------------------------------------------------------------------
def test_constructor_defaults_and_spellings(pkg):
    c = pkg.CATKEVerticalDiffusivity()
    assert isinstance(c.time_discretization, pkg.VerticallyImplicitTimeDiscretization) and c.tke_time_step is None
    assert (c.maximum_tracer_diffusivity, c.maximum_tke_diffusivity, c.maximum_viscosity) == (math.inf,) * 3
    assert (c.minimum_tke, c.minimum_convective_buoyancy_flux, c.negative_tke_damping_time_scale) == (1e-9, 1e-11, 60.0)
    st = c.c_struct()
    for name, value in CK.closure_dict().items():
        assert getattr(st, name) == value, name
    assert repr(c) == "CATKEVerticalDiffusivity{VerticallyImplicitTimeDiscretization}"
    assert isinstance(pkg.CATKEVerticalDiffusivity(pkg.VerticallyImplicitTimeDiscretization()).mixing_length, pkg.CATKEMixingLength)
    # the reference's spellings: as identifiers where Python takes them (NFKC-normalised by Python itself), through ** otherwise
    ml = pkg.CATKEMixingLength(Cˢ=2.0, Cᵇ=0.3, Cˢᵖ=0.6, CRiᵟ=1.5, Cʰⁱu=0.25, Cˡᵒc=0.4, Cᵘⁿe=1.5, Cᶜc=5.0, Cᵉe=0.01, **{"CRi⁰": 0.3})
    assert (ml.C_s, ml.C_b, ml.C_sp, ml.CRi_delta, ml.C_hi_u, ml.C_lo_c, ml.C_un_e, ml.C_c_c, ml.C_e_e, ml.CRi_0) == \
        (2.0, 0.3, 0.6, 1.5, 0.25, 0.4, 1.5, 5.0, 0.01, 0.3)
    assert getattr(ml, "Cˢ") == 2.0 and getattr(ml, "CRi⁰") == 0.3 and ml.C_hi_c == 0.098
    for ascii_name, spelling in list(pkg.CATKEMixingLength.SPELLINGS.items()) + list(pkg.CATKEEquation.SPELLINGS.items()):
        cls = pkg.CATKEMixingLength if ascii_name in pkg.CATKEMixingLength.DEFAULTS else pkg.CATKEEquation
        assert getattr(cls(**{spelling: 0.123}), ascii_name) == 0.123 and getattr(cls(**{ascii_name: 0.321}), spelling) == 0.321
        with pytest.raises(TypeError, match="given twice"):
            cls(**{spelling: 1.0, ascii_name: 1.0})
    eq = pkg.CATKEEquation(CʰⁱD=0.6, **{"Cᵂu★": 3.0, "CᵂwΔ": 0.4, "Cᵂϵ": 2.0})
    assert (eq.C_hi_D, eq.C_W_ustar, eq.C_W_wdelta, eq.C_W_eps, eq.C_lo_D) == (0.6, 3.0, 0.4, 2.0, 1.604)
    full = pkg.CATKEVerticalDiffusivity(mixing_length=ml, turbulent_kinetic_energy_equation=eq, maximum_viscosity=1.0, minimum_tke=1e-6,
                                        tke_time_step=30).c_struct()
    assert (full.C_s, full.C_W_eps, full.maximum_viscosity, full.minimum_tke) == (2.0, 2.0, 1.0, 1e-6)
    with pytest.raises(TypeError, match="unexpected"):
        pkg.CATKEMixingLength(C_x=1.0)
    with pytest.raises(TypeError, match="unexpected"):
        pkg.CATKEVerticalDiffusivity(maximum_diffusivity=1.0)
    with pytest.raises(NotImplementedError, match="ExplicitTimeDiscretization"):
        pkg.CATKEVerticalDiffusivity(pkg.ExplicitTimeDiscretization())
    with pytest.raises(NotImplementedError, match="ExplicitTimeDiscretization"):
        pkg.CATKEVerticalDiffusivity(time_discretization="Explicit")
    # coefficients that are no numbers
    for bad in (np.ones(3), lambda x: x, "1", [1.0]):
        with pytest.raises(NotImplementedError, match="must be a number"):
            pkg.CATKEMixingLength(C_s=bad)
        with pytest.raises(NotImplementedError, match="must be a number"):
            pkg.CATKEEquation(**{"Cᵂϵ": bad})
        with pytest.raises(NotImplementedError, match="must be a number"):
            pkg.CATKEVerticalDiffusivity(minimum_tke=bad)
    for bad in (1.0, "CATKEMixingLength", pkg.CATKEEquation()):
        with pytest.raises(TypeError, match="mixing_length must be"):
            pkg.CATKEVerticalDiffusivity(mixing_length=bad)
    for bad in (1.0, pkg.CATKEMixingLength()):
        with pytest.raises(TypeError, match="turbulent_kinetic_energy_equation must be"):
            pkg.CATKEVerticalDiffusivity(turbulent_kinetic_energy_equation=bad)
    with pytest.raises(ValueError, match="tke_time_step"):
        pkg.CATKEVerticalDiffusivity(tke_time_step=0.0)


def test_model_refusals_come_before_any_allocation(pkg, monkeypatch):
    _no_alloc(monkeypatch)
    g = _grid(pkg)
    FBC, Hy = pkg.FieldBoundaryConditions, pkg.HydrostaticFreeSurfaceModel
    closure = pkg.CATKEVerticalDiffusivity()
    kw = dict(tracers=("T", "S", "e"), buoyancy=pkg.SeawaterBuoyancy())
    with pytest.raises(ValueError, match="Tracers must contain :e to represent turbulent kinetic energy for `CATKEVerticalDiffusivity`."):
        Hy(g, closure=closure, tracers=("T", "S"), buoyancy=pkg.SeawaterBuoyancy())
    with pytest.raises(ValueError, match="Tracers must contain :e"):
        Hy(g, closure=(closure, pkg.HorizontalScalarBiharmonicDiffusivity(ν=1.0)), tracers=("b",), buoyancy=pkg.BuoyancyTracer())
    with pytest.raises(NotImplementedError, match="CATKEVerticalDiffusivity on NonhydrostaticModel"):
        pkg.NonhydrostaticModel(g, advection=pkg.WENO(), tracers=("b", "e"), buoyancy=pkg.BuoyancyTracer(), closure=closure)
    with pytest.raises(NotImplementedError, match="CATKEVerticalDiffusivity runs the reference's launch sequence \\(fused = False\\)"):
        Hy(g, closure=closure, free_surface=pkg.ExplicitFreeSurface(), fused=True, **kw)
    with pytest.raises(NotImplementedError, match="CATKEVerticalDiffusivity with SplitRungeKutta3"):
        Hy(g, closure=closure, free_surface=pkg.SplitExplicitFreeSurface(substeps=10), timestepper="SplitRungeKutta3", **kw)
    for other in (pkg.ScalarDiffusivity(ν=1e-2), pkg.CATKEVerticalDiffusivity(), pkg.ConvectiveAdjustmentVerticalDiffusivity()):
        with pytest.raises(NotImplementedError, match="closure tuples"):
            Hy(g, closure=(closure, other), free_surface=pkg.ExplicitFreeSurface(), **kw)
    with pytest.raises(NotImplementedError, match="closure tuples"):
        Hy(g, closure=(closure, pkg.HorizontalScalarBiharmonicDiffusivity(ν=1.0), pkg.ScalarDiffusivity(ν=1e-2)), **kw)
    with pytest.raises(NotImplementedError, match="ensembles"):
        Hy(g, closure=np.array([closure, closure], dtype=object), **kw)

    class FakeDistributed:  # what the models ask of a Distributed architecture
        partition = object()
        communicates = True
    gs = _grid(pkg)
    gs.architecture = FakeDistributed()
    gs.topology = (pkg.FullyConnected, P, B)
    with pytest.raises(NotImplementedError, match="CATKEVerticalDiffusivity on a slab-partitioned \\(Distributed\\)"):
        Hy(gs, closure=closure, free_surface=pkg.SplitExplicitFreeSurface(substeps=10), **kw)
    # walls: the existing closure check of those topologies
    for topo in ((P, B, B), (B, B, B)):
        with pytest.raises(NotImplementedError, match="closure must be None or an explicit ScalarDiffusivity"):
            Hy(_grid(pkg, topo=topo), closure=closure, **kw)
    # the top conditions that make up the fluxes must be fluxes
    for make in (pkg.ValueBoundaryCondition, pkg.GradientBoundaryCondition):
        for name in ("T", "S", "u", "v"):
            with pytest.raises(NotImplementedError, match=f"CATKEVerticalDiffusivity: the top boundary condition of {name} must be a FluxBoundaryCondition"):
                Hy(g, closure=closure, boundary_conditions={name: FBC(top=make(1.0))}, **kw)
        with pytest.raises(NotImplementedError, match="top boundary condition of b must be a FluxBoundaryCondition"):
            Hy(g, closure=closure, tracers=("b", "e"), buoyancy=pkg.BuoyancyTracer(), boundary_conditions={"b": FBC(top=make(1.0))})


# ---- C ABI: argument checks before any HIP call ------------------------------------------------------------------------------------------
def test_c_abi_argument_checks_touch_no_device(pkg):
    lib, L = pkg._lib.lib(), pkg._lib
    g = _grid(pkg, size=(16, 16, 8))
    p = [C.c_void_p(8 * n) for n in range(1, 20)]  # never dereferenced
    terms = L.CModelTerms()
    cl = pkg.CATKEVerticalDiffusivity().c_struct()
    none = C.POINTER(L.CBc)()
    jb = lambda grid, t=terms, c=cl, tops=(none, none), f=tuple(p[:6]), dt=1.0: lib.ocn_compute_catke_surface_buoyancy_flux(
        grid, C.byref(t) if t is not None else None, C.byref(c) if c is not None else None, *tops, *f, dt, None)
    top = lambda grid, t=terms, c=cl, tops=(none,) * 4, f=tuple(p[:3]): lib.ocn_compute_catke_top_tke_flux(
        grid, C.byref(t) if t is not None else None, C.byref(c) if c is not None else None, *tops, *f, None)
    dif = lambda grid, t=terms, c=cl, f=tuple(p[:9]): lib.ocn_compute_catke_diffusivities(
        grid, C.byref(t) if t is not None else None, C.byref(c) if c is not None else None, *f, None)
    sub = lambda grid, t=terms, c=cl, f=tuple(p[:15]), dtau=1.0, chi=0.1, solve=1: lib.ocn_catke_substep_tke(
        grid, C.byref(t) if t is not None else None, C.byref(c) if c is not None else None, *f, dtau, chi, solve, None)
    calls = (jb, top, dif, sub)
    bad_grids = [(_grid(pkg, topo=(P, P, P)), b"(Periodic, Periodic, Bounded)"), (_grid(pkg, topo=(P, B, B)), b"(Periodic, Periodic, Bounded)"),
                 (_grid(pkg, topo=(B, P, B)), b"(Periodic, Periodic, Bounded)"),
                 (pkg.RectilinearGrid(None, size=(16, 8), x=(0, 1), z=(-1, 0), topology=(P, F, B), halo=(3, 3)), b"(Periodic, Periodic, Bounded)"),
                 (pkg.RectilinearGrid(None, size=(16, 16, 8), x=(0, 1), y=(0, 1), z=(-1, 0), topology=(P, P, B), halo=(3, 3, 0)), b"halo"),
                 (_grid(pkg, size=(8, 8, 1)), b"two layers")]
    for call in calls:
        for bad, wording in bad_grids:
            assert call(bad.cref) == INVALID and wording in lib.ocn_last_error(), lib.ocn_last_error()
        assert call(None) == INVALID
        assert call(g.cref, t=None) == INVALID and b"null terms" in lib.ocn_last_error()
        assert call(g.cref, c=None) == INVALID and b"null closure" in lib.ocn_last_error()
        for kind, wording in ((L.BUOYANCY_TRACER, b"T (or b) tracer is NULL"), (L.BUOYANCY_SEAWATER_TS, b"tracer is NULL"),
                              (L.BUOYANCY_SEAWATER_S, b"S tracer is NULL"), (9, b"unknown buoyancy")):
            t = L.CModelTerms()
            t.buoyancy = kind
            assert call(g.cref, t=t) == INVALID and wording in lib.ocn_last_error()
        for name in L.CATKE_FIELDS:
            for bad in (float("nan"), float("inf")):
                c = pkg.CATKEVerticalDiffusivity().c_struct()
                setattr(c, name, bad)
                ok_inf = name.startswith("maximum") and bad == float("inf")
                if not ok_inf:
                    assert call(g.cref, c=c) == INVALID and (b"finite" in lib.ocn_last_error() or b"NaN" in lib.ocn_last_error()), name
        n = {jb: 6, top: 3, dif: 9, sub: 15}[call]
        for q in range(n):
            f = list(p[:n])
            f[q] = None
            if call is sub and q == 14:  # (the scratch array: needed with solve != 0 only, checked below)
                continue
            assert call(g.cref, f=tuple(f)) == INVALID and b"null pointer" in lib.ocn_last_error(), (n, q)
    # Value / Gradient top conditions are no fluxes
    for kind in (L.BC_VALUE, L.BC_GRADIENT):
        bc = C.pointer(L.CBc(kind, 0, 1.0, 0.0, None))
        assert jb(g.cref, tops=(bc, none)) == INVALID and b"only a Flux" in lib.ocn_last_error()
        assert jb(g.cref, tops=(none, bc)) == INVALID and b"only a Flux" in lib.ocn_last_error()
        for q in range(4):
            tops = [none] * 4
            tops[q] = bc
            assert top(g.cref, tops=tuple(tops)) == INVALID and b"only a Flux" in lib.ocn_last_error()
    for dt in (-1.0, float("nan"), float("inf")):
        assert jb(g.cref, dt=dt) == INVALID and b"dt" in lib.ocn_last_error()
        assert sub(g.cref, dtau=dt) == INVALID and b"dtau" in lib.ocn_last_error()
    assert sub(g.cref, chi=float("nan")) == INVALID and b"chi" in lib.ocn_last_error()
    # aliases
    for f in ((6, 7), (6, 8), (7, 8)):
        args = list(p[:9])
        args[f[1]] = args[f[0]]
        assert dif(g.cref, f=tuple(args)) == INVALID and b"three different arrays" in lib.ocn_last_error()
    # (zf, zc, u⁺, v⁺, uⁿ, vⁿ, e, Jb, κu, κc, κe, Le, Gⁿe, G⁻e, scratch)
    for a, b_, wording in ((10, 8, b"kappa_e is written"), (10, 9, b"kappa_e is written"), (11, 6, b"different arrays"), (12, 6, b"different arrays"),
                           (13, 6, b"different arrays"), (12, 11, b"different arrays"), (13, 11, b"different arrays"), (13, 12, b"different arrays"),
                           (14, 6, b"different arrays")):
        args = list(p[:15])
        args[a] = args[b_]
        assert sub(g.cref, f=tuple(args)) == INVALID and wording in lib.ocn_last_error(), (a, b_)
    args = list(p[:15])
    args[14] = None
    assert sub(g.cref, f=tuple(args), solve=1) == INVALID and b"scratch" in lib.ocn_last_error()
    t = L.CModelTerms()
    t.buoyancy, t.T = L.BUOYANCY_TRACER, p[6]
    assert sub(g.cref, t=t) == INVALID and b"buoyancy tracer" in lib.ocn_last_error()
    x = np.ones(2)
    assert lib.ocn_catke_host_cbrt(-1, x.ctypes.data, x.ctypes.data) == INVALID and lib.ocn_catke_host_cbrt(2, None, x.ctypes.data) == INVALID
    assert lib.ocn_catke_host_cbrt(0, None, None) == 0
