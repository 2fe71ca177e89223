"""TKEDissipationVerticalDiffusivity (k-ϵ) without a GPU: the NumPy restatement of the reference (tests/tke_dissipation_numpy.py) against what is
certain independently of its author -- the quadratics behind the derived constants, break points of the clamps, closed forms of uniform
columns, a dense matrix solve --, the constructors in every spelling, every refusal before any allocation, the argument checks of the C entry
points (no device is touched), and the branch shares of the seeded inputs of tests/test_gpu_tke_dissipation.py at every shape."""
import ctypes as C
import math

import numpy as np
import pytest

import catke_numpy as CK
import implicit_diffusion_numpy as IDN
import tke_dissipation_numpy as TD
from helpers import stretched_faces

P, B, F = "Periodic", "Bounded", "Flat"
INVALID = -1  # OCN_ERR_INVALID_ARGUMENT (include/ocn_hip.h)
EPS = np.finfo(np.float64).eps
NON_DEFAULT = dict(Cu0=0.12, Cu1=0.02, Cu2=-0.0002, Cc0=0.1, Cc1=0.004, Cc2=0.001, Cd0=1.1, Cd1=0.25, Cd2=0.03, Cd3=0.006, Cd4=0.007, Cd5=-0.0004,
                   C_sigma_eps=1.3)


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


def _state(pkg, size=(3, 2, 8), z=(-64.0, 0.0), cl=None, b=None, e=1e-4, eps=1e-7, u=None, v=None, halo=(1, 1, 1)):
    """a column state with a buoyancy tracer b(z) (a function of the centre heights, or None: unstratified), uniform or given e, ϵ, u, v"""
    pg = _grid(pkg, size=size, z=z, halo=halo)
    g = IDN.describe(pg)
    zc_all = pg.nodes_1d(2, False, with_halos=True)
    shape = pg.parent_shape(0)
    T = np.zeros(shape) + (b(zc_all) if b is not None else 0.0)
    full = lambda x, loc: np.zeros(pg.parent_shape(loc)) + (0.0 if x is None else x)
    s = TD.State(g, pg.nodes_1d(2, True), pg.nodes_1d(2, False), pg.Lz, "BuoyancyTracer", cl or TD.closure_dict(), full(u, 1), full(v, 2), T, None,
                 np.zeros(shape) + e, np.zeros(shape) + eps)
    return pg, g, s


def _inner(g):
    return (slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny), slice(g.Hz, g.Hz + g.Nz))


def _zeros(pg, g):
    return np.zeros(TD.ccf_shape(g)), np.zeros(pg.parent_shape(0))


# ---- constants and clamps -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coefficients", [dict(), NON_DEFAULT], ids=["defaults", "non_default"])
def test_derived_constants_solve_their_quadratics(pkg, coefficients):
    """𝕊u₀⁴ is a root of c y² + b y + a = 0 (a = Cd₅ - Cu₂, b = Cd₂ - Cu₀, c = Cd₀); minimum_stratification_number / safety factor is a root of
    a x² + b x + c = 0 (a = Cd₄ + Cc₁, b = Cd₁ + Cc₀, c = Cd₀); maximum_shear_number is the ratio of its two polynomials.  The package's struct
    holds the bits of the restatement's formulas."""
    cl = TD.closure_dict(minimum_stratification_number_safety_factor=0.8 if coefficients else 0.73, **coefficients)
    sf = pkg.VariableStabilityFunctions(**coefficients)
    closure = pkg.TKEDissipationVerticalDiffusivity(stability_functions=sf, minimum_stratification_number_safety_factor=0.8 if coefficients else 0.73)
    st = closure.c_struct()
    a, b, c = cl["Cd5"] - cl["Cu2"], cl["Cd2"] - cl["Cu0"], cl["Cd0"]
    S = (2 * a / (-b - math.sqrt(b * b - 4 * a * c))) ** (1 / 4)
    assert sf.Su0 == S == st.Su0 == cl["Su0"] and abs(S - 0.53) < 0.03
    y = S ** 4
    assert abs(c * y * y + b * y + a) <= 8 * EPS * max(abs(c * y * y), abs(b * y), abs(a))
    assert st.Su0_cubed == S * S * S == cl["Su0_cubed"] and st.Su0_fourth_over_sigma_eps == (S * S) * (S * S) / cl["C_sigma_eps"]
    assert abs(st.Su0_fourth_over_sigma_eps * cl["C_sigma_eps"] - y) <= 4 * EPS * y
    a, b, c = cl["Cd4"] + cl["Cc1"], cl["Cd1"] + cl["Cc0"], cl["Cd0"]
    x = (-b + math.sqrt(b * b - 4 * a * c)) / (2 * a)
    assert abs(a * x * x + b * x + c) <= 16 * EPS * max(abs(a * x * x), abs(b * x), abs(c)) and x < 0
    factor = cl["minimum_stratification_number_safety_factor"]
    assert st.minimum_stratification_number == x * factor == cl["minimum_stratification_number"]
    n0, n1, d0, d1, d2, d3, d4 = (cl[n] for n in ("Cu0", "Cu1", "Cd0", "Cd1", "Cd2", "Cd3", "Cd4"))
    num = np.polynomial.Polynomial([d0 * n0, d0 * n1 + d1 * n0, d1 * n1 + d4 * n0, d4 * n1])
    den = np.polynomial.Polynomial([d2 * n0, d2 * n1 + d3 * n0, d3 * n1])
    aN = np.array([cl["minimum_stratification_number"], -1.0, 0.0, 0.5, 3.0, 1e3, 1e10])
    assert np.allclose(TD.maximum_shear_number(cl, aN), num(aN) / den(aN), rtol=16 * EPS, atol=0)
    assert TD.maximum_shear_number(cl, 0.0) == (d0 * n0) / (d2 * n0)
    # the struct of ConstantStabilityFunctions: the coefficients it does not have are 0, the minimum is not read
    k = pkg.TKEDissipationVerticalDiffusivity(stability_functions=pkg.ConstantStabilityFunctions()).c_struct()
    assert (k.stability_functions, k.Cu0, k.Cc0, k.Su0, k.Cu1, k.Cd0, k.minimum_stratification_number) == (1, 0.53, 0.53, 0.53, 0.0, 0.0, 0.0)
    assert st.stability_functions == 0


def test_both_clamps_at_their_break_points(pkg):
    """clamp(x, lo, hi) just inside, on and just outside lo and hi, a NaN x and a NaN bound; then the two numbers of a face: αᴺ within
    [αᴺmin, 1e10], αᴹ within [0, maximum_shear_number(αᴺ)], by a column whose e² / ϵ² is 1 (Cᴺ so large that Lz bounds the floor of ϵ below 1) so that αᴺ = N² and αᴹ = S²"""
    lo, hi = -2.25, 7.5
    below, above = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
    x = np.array([below, lo, np.nextafter(lo, np.inf), 0.0, np.nextafter(hi, -np.inf), hi, above, np.nan, -np.inf, np.inf])
    want = np.array([lo, lo, np.nextafter(lo, np.inf), 0.0, np.nextafter(hi, -np.inf), hi, hi, np.nan, lo, hi])
    assert np.array_equal(TD.clamp(x, lo, hi), want, equal_nan=True)
    assert np.array_equal(TD.clamp(np.array([-1.0, 9.0]), lo, np.nan), [-1.0, 9.0])  # a NaN bound never binds
    cl = TD.closure_dict(minimum_tke=1e-12, C_N=1e12)
    aN_min = cl["minimum_stratification_number"]
    for N2, expect in ((np.nextafter(aN_min, -np.inf), aN_min), (aN_min, aN_min), (np.nextafter(aN_min, np.inf), np.nextafter(aN_min, np.inf)),
                       (1e10, 1e10), (np.nextafter(1e10, np.inf), 1e10), (3e10, 1e10)):
        pg, g, s = _state(pkg, cl=cl, e=1.0, eps=1.0, size=(2, 2, 4), z=(-4.0, 0.0))
        s.T[:, :, g.Hz + 2:] += N2  # one step of N2 across face 3 (Δz = 1)
        aN, aM, aN_raw, aM_raw, aM_max = TD.clamped_numbers(s, 3, with_raw=True)
        assert np.all(aN_raw == N2) and np.all(aN == expect) and np.all(aM == 0.0), (N2, aN_raw, aN)
    aM_max = float(TD.maximum_shear_number(cl, 0.0))
    for S2, expect in ((0.0, 0.0), (np.nextafter(aM_max, -np.inf), np.nextafter(aM_max, -np.inf)), (aM_max, aM_max), (np.nextafter(aM_max, np.inf), aM_max),
                       (3 * aM_max, aM_max)):
        pg, g, s = _state(pkg, cl=cl, e=1.0, eps=1.0, size=(2, 2, 4), z=(-4.0, 0.0))
        s.u[:, :, g.Hz + 2:] += math.sqrt(S2)  # ∂z u = sqrt(S2) on face 3 at every i
        aN, aM, aN_raw, aM_raw, _ = TD.clamped_numbers(s, 3, with_raw=True)
        assert np.allclose(aM_raw, S2, rtol=4 * EPS, atol=0)
        raw = float(aM_raw[0, 0])
        assert np.all(aN == 0.0) and np.all(aM == (aM_max if raw > aM_max else raw)) and (raw > aM_max) == (expect == aM_max and S2 > aM_max), (S2, raw)


# ---- closed forms on uniform columns -------------------------------------------------------------------------------------------------------
def test_uniform_column_at_rest_has_kappa_C_e2_over_eps_and_the_maxima_clip(pkg):
    """unstratified, at rest, ConstantStabilityFunctions, ϵ above its floor: κ = C e² / ϵ on faces 2..Nz with C = Cu₀, Cc₀, Cu₀ / Cσe, Cu₀ / Cσϵ,
    exactly 0 on face 1, face Nz + 1 not written; each maximum clips its κ"""
    e, eps = 2e-4, 3e-7
    cl = TD.closure_dict(constant=True, Cu0=0.5, Cc0=0.4, C_sigma_e=1.1)
    pg, g, s = _state(pkg, cl=cl, e=e, eps=eps)
    assert np.all(TD.minimum_dissipation(s, 3) < eps)
    sentinel = np.full(TD.ccf_shape(g), -7.0)
    out = TD.diffusivities(s, sentinel, sentinel, sentinel, sentinel)
    C_of = {"u": 0.5, "c": 0.4, "e": 0.5 / 1.1, "eps": 0.5 / 1.2}
    for which, a in zip(("u", "c", "e", "eps"), out):
        col = a[g.Hx:g.Hx + g.Nx, g.Hy:g.Hy + g.Ny]
        assert np.all(col[:, :, g.Hz] == 0) and np.all(col[:, :, g.Hz + 1:g.Hz + g.Nz] == C_of[which] * (e * e) / eps) and np.all(col[:, :, g.Hz + g.Nz:] == -7.0)
        assert np.all(a[:g.Hx] == -7.0) and np.all(a[:, :g.Hy] == -7.0) and np.all(a[:, :, :g.Hz] == -7.0)
    free = {which: TD.kappa_ccf(s, 4, which) for which in C_of}
    maxima = dict(maximum_viscosity=1e-3, maximum_tracer_diffusivity=2e-3, maximum_tke_diffusivity=3e-3, maximum_dissipation_diffusivity=4e-3)
    assert all(np.all(v > 4e-3) for v in free.values())
    s.cl = TD.closure_dict(constant=True, **maxima)
    for which, m in zip(("u", "c", "e", "eps"), (1e-3, 2e-3, 3e-3, 4e-3)):
        assert np.all(TD.kappa_ccf(s, 4, which) == m)


def test_dissipation_floor_has_its_closed_form(pkg):
    """a uniformly stratified column with ϵ = 0: ϵ★ = 𝕊u₀³ sqrt(e★)³ / min(Lz, Cᴺ sqrt(e★ / N²)).  Strong stratification: the displacement scale
    binds; weak: Lz binds; unstable: N²⁺ is the 1e-14 floor and Lz binds; a tiny e★ (minimum_tke = 1e-8): the 1e-12 floor, under either length"""
    Lz, S3 = 64.0, TD.closure_dict()["Su0_cubed"]
    for N2, e, emin, branch, floored in ((1e-4, 1e-4, 1e-6, "stratified", False), (1e-12, 1e-4, 1e-6, "Lz", False), (-1e-5, 1e-4, 1e-6, "Lz", False),
                                         (1e-4, 0.0, 1e-6, "stratified", False), (1e-9, -1.0, 1e-8, "stratified", True), (-1e-9, 0.0, 1e-8, "Lz", True)):
        cl = TD.closure_dict(minimum_tke=emin)
        pg, g, s = _state(pkg, cl=cl, b=lambda z: N2 * z, e=e, eps=0.0)
        e_star = max(emin, e)
        for k in (1, 4, 8):
            n2 = CK.bz(s, lambda kk: np.maximum(1e-14, CK.dz_b(s, kk)), k)
            assert np.allclose(n2, max(N2, 1e-14), rtol=1e-12, atol=0)
            l_st = 0.75 * np.sqrt(e_star / n2)
            assert np.all(l_st < Lz) == (branch == "stratified") and np.all(l_st > Lz) == (branch != "stratified")
            w = math.sqrt(e_star)
            floor = S3 * (w * w * w) / (l_st if branch == "stratified" else Lz)
            want = np.maximum(1e-12, floor)
            assert np.all((floor < 1e-12) == floored)
            got = TD.dissipation(s, k)
            assert np.array_equal(got, want + 0 * got) and np.array_equal(TD.minimum_dissipation(s, k), got)
        # ϵ above the floor is kept, infinity included
        s.eps = s.eps + 1.0
        assert np.all(TD.dissipation(s, 4) == 1.0)
        s.eps = s.eps + np.inf
        assert np.all(TD.dissipation(s, 4) == np.inf)


def test_homogeneous_decay_and_negative_e(pkg):
    """no shear, no stratification (P = wb = 0), κᵉ = κᵋ clipped to 0, one Euler substep (χ = -1/2) and the two solves: e / (1 + Δτ ϵ / e) and
    ϵ / (1 + Δτ Cᵋϵ ϵ / e); e < 0 is damped with the rate negative_tke_damping_time_scale ITSELF (60, not 1 / 60), as the reference has it"""
    cl = TD.closure_dict(maximum_tke_diffusivity=0.0, maximum_dissipation_diffusivity=0.0)
    dtau = 30.0
    for e0, p0 in ((1e-4, 2e-7), (-1e-5, 2e-7)):
        pg, g, s = _state(pkg, cl=cl, e=e0, eps=p0)
        zf, zc = _zeros(pg, g)
        e1, p1, ke, kp, Le, Lp, Gme, Gmp, terms = TD.substep(s, s.u, s.v, zf, zf, zf, zf, zc, zc, zc, zc, zc, zc, dtau, -0.5, with_terms=True)
        assert np.all(terms["P"] == 0) and np.all(terms["wb"] == 0) and np.all(ke == 0) and np.all(kp == 0)
        assert np.array_equal(e1, s.e) and np.array_equal(p1, s.eps) and np.all(Gme == 0) and np.all(Gmp == 0)
        e2, p2 = TD.implicit_step(g, e1, ke, Le, dtau), TD.implicit_step(g, p1, kp, Lp, dtau)
        sl = _inner(g)
        e_star = max(1e-6, e0)
        assert np.all(terms["eps_star"] == p0)  # (above its floor)
        if e0 < 0:
            assert np.all(terms["omega_e"] == 60.0) and np.all(Le[sl] == -60.0)
            assert np.allclose(e2[sl], e0 / (1 + dtau * 60.0), rtol=4 * EPS, atol=0)
        else:
            assert np.all(terms["omega_e"] == p0 / e0)
            assert np.allclose(e2[sl], e0 / (1 + dtau * p0 / e0), rtol=4 * EPS, atol=0)
        assert np.allclose(p2[sl], p0 / (1 + dtau * 1.92 * p0 / e_star), rtol=4 * EPS, atol=0)
        assert np.array_equal(e2[:, :, :g.Hz], s.e[:, :, :g.Hz]) and np.array_equal(p2[:, :, :g.Hz], s.eps[:, :, :g.Hz])  # halos untouched


# ---- the pieces of the substep -------------------------------------------------------------------------------------------------------------
def test_patankar_split_switch_and_buoyancy_coefficient(pkg):
    """at rest (P = 0), κᶜ given: wb = -κᶜ N².  Stable (wb < 0): wb goes to Le = wb / e - ω while e > eᵐⁱⁿ, and is dropped from Le when
    e <= eᵐⁱⁿ; Cᵇϵ⁺ multiplies it.  Unstable (wb > 0): wb is the explicit source of e, and Cᵇϵ⁻ multiplies it.  The sign of Cᵇϵ wb decides
    between Lϵ (negative) and the explicit source of ϵ (positive)."""
    kc, dtau = 1e-3, 10.0
    for N2 in (2e-5, -2e-5):
        for Cp, Cm in ((0.5, -0.7), (-0.5, 0.7)):
            for e0 in (1e-4, 1e-6, 5e-7):
                cl = TD.closure_dict(C_b_eps_plus=Cp, C_b_eps_minus=Cm, maximum_tke_diffusivity=0.0, maximum_dissipation_diffusivity=0.0)
                pg, g, s = _state(pkg, cl=cl, b=lambda z: N2 * z, e=e0, eps=1e-6)
                zf, zc = _zeros(pg, g)
                out = TD.substep(s, s.u, s.v, zf, zf + kc, zf, zf, zc, zc, zc, zc, zc, zc, dtau, 0.1, with_terms=True)
                e1, p1, ke, kp, Le, Lp, Gme, Gmp, terms = out
                sl = _inner(g)
                wb = terms["wb"]
                assert np.allclose(wb, -kc * N2, rtol=1e-12, atol=0) and np.all(terms["P"] == 0)
                assert np.all((terms["N2"] >= 0) == (N2 > 0))
                e_star, omega, omega_eps = max(1e-6, e0), terms["eps_star"] / max(1e-6, e0), 1e-6 / max(1e-6, e0)
                Cb = Cp if N2 > 0 else Cm
                if N2 > 0:  # wb < 0
                    assert np.all(Gme[sl] == 0)
                    assert np.array_equal(Le[sl], (wb / e0 if e0 > 1e-6 else 0.0) - omega)
                else:
                    assert np.array_equal(Gme[sl], wb) and np.array_equal(Le[sl], -omega)
                    assert np.array_equal(e1[sl], e0 + dtau * (1.6 * wb))
                if Cb * (-N2) < 0:
                    assert np.array_equal(Lp[sl], Cb * wb / e_star - 1.92 * omega_eps) and np.all(Gmp[sl] == 0)
                else:
                    assert np.array_equal(Lp[sl], 0 * wb - 1.92 * omega_eps) and np.array_equal(Gmp[sl], omega_eps * (1.44 * 0.0 + Cb * wb))


def _sheared(pkg, cl=None):
    pg, g, s = _state(pkg, cl=cl, b=lambda z: 1e-5 * z, e=1e-4, eps=1e-7, u=0.0)
    rng = np.random.default_rng(3)
    s.u = s.u + 0.01 * rng.uniform(-1, 1, s.u.shape)
    return pg, g, s


def test_substeps_open_with_an_euler_step(pkg):
    """tke_dissipation_time_step = Δt / 3: M = 3 substeps of Δt / 3 with χ = -1/2, χ, χ; None: one substep with χ; ceil(Δt / Δτ)"""
    pg, g, s = _sheared(pkg)
    zf, zc = _zeros(pg, g)
    d = dict(kappa_u=zf + 1e-3, kappa_c=zf + 1e-4, kappa_e=zf, kappa_eps=zf, Le=zc, Leps=zc, u_prev=0.5 * s.u, v_prev=s.v)
    Ge, Gp = zc + 1e-9, zc + 1e-12
    r3 = TD.time_step(s, d, Ge, zc, Gp, zc, 3.0, 1.0, 0.1)
    assert r3[-1] == [-0.5, 0.1, 0.1]
    r1 = TD.time_step(s, d, Ge, zc, Gp, zc, 3.0, None, 0.1)
    assert r1[-1] == [0.1] and not np.array_equal(r1[0], r3[0]) and not np.array_equal(r1[1], r3[1])
    e, p, ke, kp, Le, Lp, Gme, Gmp = s.e, s.eps, zf, zf, zc, zc, zc, zc
    for chi in (-0.5, 0.1, 0.1):  # by hand: three substeps of 1.0
        e, p, ke, kp, Le, Lp, Gme, Gmp = TD.substep(s.with_tracers(e, p), d["u_prev"], d["v_prev"], d["kappa_u"], d["kappa_c"], ke, kp, Le, Lp, Ge, Gme,
                                                    Gp, Gmp, 1.0, chi)
        e, p = TD.implicit_step(g, e, ke, Le, 1.0), TD.implicit_step(g, p, kp, Lp, 1.0)
    assert np.array_equal(e, r3[0]) and np.array_equal(p, r3[1]) and np.array_equal(Gme, r3[6]) and np.array_equal(Gmp, r3[7])
    assert TD.time_step(s, d, Ge, zc, Gp, zc, 3.0, 0.9, 0.1)[-1] == [-0.5, 0.1, 0.1, 0.1]
    # the AB2 weights: α = 3/2 + χ on the total tendency, β = 1/2 + χ on G⁻
    a = TD.substep(s, d["u_prev"], d["v_prev"], d["kappa_u"], d["kappa_c"], zf, zf, zc, zc, Ge, zc + 2e-9, Gp, zc + 3e-12, 2.0, 0.1)
    sl = _inner(g)
    assert np.array_equal(a[0][sl], s.e[sl] + 2.0 * (1.6 * a[6][sl] - 0.6 * 2e-9)) and np.array_equal(a[1][sl], s.eps[sl] + 2.0 * (1.6 * a[7][sl] - 0.6 * 3e-12))


def test_both_implicit_steps_equal_a_dense_solve(pkg):
    """(1 - Δτ ∂z κ ∂z - Δτ L) c⁺ = c for e (κᵉ, Le) and ϵ (κᵋ, Lϵ): the restatement's elimination against numpy.linalg.solve of its dense form, and
    that dense form against a matrix written from the formulas"""
    pg = _grid(pkg, size=(2, 2, 7), z=stretched_faces(7), halo=(1, 1, 2))
    g = IDN.describe(pg)
    rng = np.random.default_rng(11)
    dt = 0.3
    for seed_scale in (1.0, 3.0):  # e's system, ϵ's system
        c = rng.uniform(0, 1, pg.parent_shape(0))
        kappa = seed_scale * rng.uniform(0.1, 1, TD.ccf_shape(g))
        kappa[:, :, g.Hz] = 0
        kappa[:, :, g.Hz + g.Nz] = 0
        L = -seed_scale * rng.uniform(0, 2, pg.parent_shape(0))
        out = TD.implicit_step(g, c, kappa, L, dt)
        col = slice(g.Hz, g.Hz + g.Nz)
        for i, j in ((0, 0), (1, 1), (0, 1)):
            A = TD.implicit_matrix(g, kappa, L, dt, i, j)
            I, J = g.Hx + i, g.Hy + j
            assert np.allclose(out[I, J, col], np.linalg.solve(A, c[I, J, col]), rtol=64 * EPS, atol=0)
            W = np.zeros((g.Nz, g.Nz))
            for k in range(1, g.Nz + 1):
                dzc = g.dzc[g.Hz + k - 1]
                lo = dt * kappa[I, J, g.Hz + k - 1] / (dzc * g.dzf[g.Hz + k - 1])
                up = dt * kappa[I, J, g.Hz + k] / (dzc * g.dzf[g.Hz + k])
                W[k - 1, k - 1] = 1 - dt * L[I, J, g.Hz + k - 1] + lo + up
                if k > 1:
                    W[k - 1, k - 2] = -lo
                if k < g.Nz:
                    W[k - 1, k] = -up
            assert np.allclose(A, W, rtol=4 * EPS, atol=0)
        assert np.array_equal(out[:, :, :g.Hz], c[:, :, :g.Hz]) and np.array_equal(out[:, :, g.Hz + g.Nz:], c[:, :, g.Hz + g.Nz:])


def test_top_fluxes_have_their_closed_forms(pkg):
    """Qe = -Cᵂu★ u★³ and Qϵ = -𝕊u₀⁴ / Cσϵ e★² / (d + ℓᵣ), u★ = (τx² + τy²)^(1/4), d = Δz / 2, ℓᵣ = max(1e-4, Cᵂα u★² / g): the Charnock length
    below the minimum (a weak stress) and above it (a strong one); e below minimum_tke enters as minimum_tke"""
    cl = TD.closure_dict(C_W_ustar=2.0)
    S4 = cl["Su0"] ** 4
    for tau_x, tau_y, charnock in ((1e-4, 0.0, False), (0.03, -0.04, True)):
        for e0 in (3e-4, 1e-7):
            pg, g, s = _state(pkg, cl=cl, e=e0)
            Qe, Qp = TD.top_fluxes(s, tau_x, tau_y)
            u_star = math.hypot(tau_x, tau_y) ** 0.5
            l_ch = 0.11 * u_star ** 2 / 9.8065
            assert (l_ch > 1e-4) == charnock
            l_r = max(1e-4, l_ch)
            e_star = max(1e-6, e0)
            assert np.allclose(Qe, -2.0 * u_star ** 3, rtol=8 * EPS, atol=0) and np.allclose(Qp, -S4 / 1.2 * e_star ** 2 / (4.0 + l_r), rtol=8 * EPS, atol=0)
    pg, g, s = _state(pkg, e=1e-4)
    Qe, Qp = TD.top_fluxes(s, None, (1e-4, 0.5))  # no flux on u; a linear drag on v (v = 0)
    assert np.all(Qe == 0) and np.signbit(Qe).all() and np.all(Qp < 0)


# ---- constructors ---------------------------------------------------------------------------------------------------------------------------
def test_constructor_defaults_and_spellings(pkg):
    c = pkg.TKEDissipationVerticalDiffusivity()
    assert isinstance(c.time_discretization, pkg.VerticallyImplicitTimeDiscretization) and c.tke_dissipation_time_step is None
    assert (c.maximum_tracer_diffusivity, c.maximum_tke_diffusivity, c.maximum_dissipation_diffusivity, c.maximum_viscosity) == (math.inf,) * 4
    assert (c.minimum_tke, c.minimum_stratification_number_safety_factor, c.negative_tke_damping_time_scale) == (1e-6, 0.73, 60.0)
    assert isinstance(c.tke_dissipation_equations, pkg.TKEDissipationEquations) and isinstance(c.stability_functions, pkg.VariableStabilityFunctions)
    assert isinstance(c.minimum_length_scale, pkg.StratifiedDisplacementScale)
    st, cl = c.c_struct(), TD.closure_dict()
    for name in pkg._lib.TKE_DISSIPATION_FIELDS:
        assert getattr(st, name) == cl[name], name
    assert set(pkg._lib.TKE_DISSIPATION_FIELDS) == set(cl) - {"constant", "minimum_stratification_number_safety_factor"}
    assert repr(c) == "TKEDissipationVerticalDiffusivity{VerticallyImplicitTimeDiscretization}"
    for name, value in TD.CONSTANT.items():
        assert getattr(pkg.ConstantStabilityFunctions(), name) == value
    # the reference's spellings: as identifiers where Python takes them (NFKC-normalised by Python itself), through ** otherwise
    eq = pkg.TKEDissipationEquations(Cᵋϵ=2.0, Cᴾϵ=1.5, Cᵂα=0.2, gravitational_acceleration=9.8, minimum_roughness_length=1e-3,
                                     **{"Cᵇϵ⁺": -0.1, "Cᵇϵ⁻": -0.2, "Cᵂu★": 3.0, "CᵂwΔ": 0.4})
    assert (eq.C_eps_eps, eq.C_P_eps, eq.C_W_alpha, eq.gravitational_acceleration, eq.minimum_roughness_length, eq.C_b_eps_plus, eq.C_b_eps_minus,
            eq.C_W_ustar, eq.C_W_wdelta) == (2.0, 1.5, 0.2, 9.8, 1e-3, -0.1, -0.2, 3.0, 0.4)
    assert getattr(eq, "Cᵇϵ⁺") == -0.1 and getattr(eq, "Cᵇϵ⁻") == -0.2 and getattr(eq, "Cᵋϵ") == 2.0
    sf = pkg.VariableStabilityFunctions(Cσe=1.1, Cσϵ=1.3, **{"Cu₀": 0.11, "Cd₅": -0.0003, "𝕊u₀": 0.5})
    assert (sf.C_sigma_e, sf.C_sigma_eps, sf.Cu0, sf.Cd5, sf.Su0, sf.Cu1) == (1.1, 1.3, 0.11, -0.0003, 0.5, 0.0173)
    assert pkg.VariableStabilityFunctions(Su0=None).Su0 == TD.closure_dict()["Su0"] and pkg.VariableStabilityFunctions(**{"𝕊u₀": None}).Su0 == sf.Su0 * 0 + TD.closure_dict()["Su0"]
    ls = pkg.StratifiedDisplacementScale(Cᴺ=0.5, minimum_buoyancy_frequency=1e-12)
    assert (ls.C_N, ls.minimum_buoyancy_frequency, getattr(ls, "Cᴺ")) == (0.5, 1e-12, 0.5)
    classes = (pkg.TKEDissipationEquations, pkg.VariableStabilityFunctions, pkg.ConstantStabilityFunctions, pkg.StratifiedDisplacementScale)
    for cls in classes:
        assert set(cls.SPELLINGS) == set(cls.DEFAULTS)
        for ascii_name, spelling in cls.SPELLINGS.items():
            # (a given 𝕊u₀ keeps VariableStabilityFunctions from taking the root of a negative discriminant, a DomainError in the reference too)
            more = {"Su0": 0.5} if cls is pkg.VariableStabilityFunctions and ascii_name != "Su0" else {}
            assert getattr(cls(**{spelling: 0.123}, **more), ascii_name) == 0.123 and getattr(cls(**{ascii_name: 0.321}, **more), spelling) == 0.321
            if spelling != ascii_name:
                with pytest.raises(TypeError, match="given twice"):
                    cls(**{spelling: 1.0, ascii_name: 1.0})
        with pytest.raises(TypeError, match="unexpected"):
            cls(C_x=1.0)
        for bad in (np.ones(3), lambda x: x, "1", [1.0]):
            with pytest.raises(NotImplementedError, match="must be a number"):
                cls(**{next(iter(cls.DEFAULTS)): bad})
    full = pkg.TKEDissipationVerticalDiffusivity(tke_dissipation_equations=eq, stability_functions=sf, minimum_length_scale=ls, maximum_viscosity=1.0,
                                                 maximum_dissipation_diffusivity=2.0, minimum_tke=1e-7, tke_dissipation_time_step=30).c_struct()
    assert (full.C_eps_eps, full.C_sigma_eps, full.C_N, full.maximum_viscosity, full.maximum_dissipation_diffusivity, full.minimum_tke, full.Su0) == \
        (2.0, 1.3, 0.5, 1.0, 2.0, 1e-7, 0.5)
    assert full.Su0_fourth_over_sigma_eps == (0.5 * 0.5) * (0.5 * 0.5) / 1.3
    with pytest.raises(TypeError, match="unexpected"):
        pkg.TKEDissipationVerticalDiffusivity(maximum_diffusivity=1.0)
    for how in (lambda: pkg.TKEDissipationVerticalDiffusivity(pkg.ExplicitTimeDiscretization()),
                lambda: pkg.TKEDissipationVerticalDiffusivity(time_discretization="Explicit")):
        with pytest.raises(NotImplementedError, match="TKEDissipationVerticalDiffusivity with ExplicitTimeDiscretization"):
            how()
    for bad in (np.ones(3), lambda x: x, "1", [1.0]):
        with pytest.raises(NotImplementedError, match="must be a number"):
            pkg.TKEDissipationVerticalDiffusivity(minimum_tke=bad)
    for key, bad in (("tke_dissipation_equations", pkg.StratifiedDisplacementScale()), ("stability_functions", 1.0),
                     ("minimum_length_scale", pkg.TKEDissipationEquations())):
        with pytest.raises(TypeError, match=f"{key} must be"):
            pkg.TKEDissipationVerticalDiffusivity(**{key: bad})
    with pytest.raises(ValueError, match="tke_dissipation_time_step"):
        pkg.TKEDissipationVerticalDiffusivity(tke_dissipation_time_step=0.0)


def test_model_refusals_come_before_any_allocation(pkg, monkeypatch):
    _no_alloc(monkeypatch)
    g = _grid(pkg)
    FBC, Hy = pkg.FieldBoundaryConditions, pkg.HydrostaticFreeSurfaceModel
    closure = pkg.TKEDissipationVerticalDiffusivity()
    kw = dict(tracers=("T", "S", "e", "epsilon"), buoyancy=pkg.SeawaterBuoyancy())
    message = "Tracers must contain :e and :ϵ to represent turbulent kinetic energy for `TKEDissipationVerticalDiffusivity`."
    for tracers in (("T", "S"), ("T", "S", "e"), ("T", "S", "epsilon"), ("T", "S", "ϵ"), ("T", "S", "e", "eps")):
        with pytest.raises(ValueError, match=message):
            Hy(g, closure=closure, tracers=tracers, buoyancy=pkg.SeawaterBuoyancy())
    with pytest.raises(ValueError, match="Tracers must contain :e and :ϵ"):
        Hy(g, closure=(closure, pkg.HorizontalScalarBiharmonicDiffusivity(ν=1.0)), tracers=("b",), buoyancy=pkg.BuoyancyTracer())
    with pytest.raises(NotImplementedError, match="TKEDissipationVerticalDiffusivity on NonhydrostaticModel"):
        pkg.NonhydrostaticModel(g, advection=pkg.WENO(), tracers=("b", "e", "epsilon"), buoyancy=pkg.BuoyancyTracer(), closure=closure)
    with pytest.raises(NotImplementedError, match="TKEDissipationVerticalDiffusivity runs the reference's launch sequence \\(fused = False\\)"):
        Hy(g, closure=closure, free_surface=pkg.ExplicitFreeSurface(), fused=True, **kw)
    with pytest.raises(NotImplementedError, match="TKEDissipationVerticalDiffusivity with SplitRungeKutta3"):
        Hy(g, closure=closure, free_surface=pkg.SplitExplicitFreeSurface(substeps=10), timestepper="SplitRungeKutta3", **kw)
    for other in (pkg.ScalarDiffusivity(ν=1e-2), pkg.TKEDissipationVerticalDiffusivity(), pkg.CATKEVerticalDiffusivity(),
                  pkg.ConvectiveAdjustmentVerticalDiffusivity()):
        with pytest.raises(NotImplementedError, match="closure tuples are not implemented, except .* TKEDissipationVerticalDiffusivity"):
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
    with pytest.raises(NotImplementedError, match="TKEDissipationVerticalDiffusivity on a slab-partitioned \\(Distributed\\)"):
        Hy(gs, closure=closure, free_surface=pkg.SplitExplicitFreeSurface(substeps=10), **kw)
    # walls: the existing closure check of those topologies
    for topo in ((P, B, B), (B, B, B)):
        with pytest.raises(NotImplementedError, match="closure must be None or an explicit ScalarDiffusivity"):
            Hy(_grid(pkg, topo=topo), closure=closure, **kw)
    # the top conditions that make up the fluxes must be fluxes
    for make in (pkg.ValueBoundaryCondition, pkg.GradientBoundaryCondition):
        for name in ("T", "S", "u", "v"):
            with pytest.raises(NotImplementedError,
                               match=f"TKEDissipationVerticalDiffusivity: the top boundary condition of {name} must be a FluxBoundaryCondition"):
                Hy(g, closure=closure, boundary_conditions={name: FBC(top=make(1.0))}, **kw)
        with pytest.raises(NotImplementedError, match="top boundary condition of b must be a FluxBoundaryCondition"):
            Hy(g, closure=closure, tracers=("b", "e", "ϵ"), buoyancy=pkg.BuoyancyTracer(), boundary_conditions={"b": FBC(top=make(1.0))})


# ---- C ABI: argument checks before any HIP call ------------------------------------------------------------------------------------------
def test_c_abi_argument_checks_touch_no_device(pkg):
    lib, L = pkg._lib.lib(), pkg._lib
    g = _grid(pkg, size=(16, 16, 8))
    p = [C.c_void_p(8 * n) for n in range(1, 24)]  # never dereferenced
    terms = L.CModelTerms()
    cl = pkg.TKEDissipationVerticalDiffusivity().c_struct()
    none = C.POINTER(L.CBc)()
    ref = lambda x: C.byref(x) if x is not None else None
    top = lambda grid, t=None, c=cl, tops=(none, none), f=tuple(p[:6]): lib.ocn_compute_tke_dissipation_top_fluxes(grid, ref(c), *tops, *f, None)
    dif = lambda grid, t=terms, c=cl, f=tuple(p[:8]): lib.ocn_compute_tke_dissipation_diffusivities(grid, ref(t), ref(c), *f, None)
    sub = lambda grid, t=terms, c=cl, f=tuple(p[:17]), dtau=1.0, chi=0.1, solve=1: lib.ocn_tke_dissipation_substep(grid, ref(t), ref(c), *f, dtau, chi,
                                                                                                              solve, None)
    bad_grids = [(_grid(pkg, topo=(P, P, P)), b"(Periodic, Periodic, Bounded)"), (_grid(pkg, topo=(P, B, B)), b"(Periodic, Periodic, Bounded)"),
                 (_grid(pkg, topo=(B, P, B)), b"(Periodic, Periodic, Bounded)"),
                 (pkg.RectilinearGrid(None, size=(16, 8), x=(0, 1), z=(-1, 0), topology=(P, F, B), halo=(3, 3)), b"(Periodic, Periodic, Bounded)"),
                 (pkg.RectilinearGrid(None, size=(16, 16, 8), x=(0, 1), y=(0, 1), z=(-1, 0), topology=(P, P, B), halo=(3, 3, 0)), b"halo"),
                 (_grid(pkg, size=(8, 8, 1)), b"two layers")]
    for call in (top, dif, sub):
        for bad, wording in bad_grids:
            assert call(bad.cref) == INVALID and wording in lib.ocn_last_error(), lib.ocn_last_error()
        assert call(None) == INVALID
        assert call(g.cref, c=None) == INVALID and b"null closure" in lib.ocn_last_error()
        if call is not top:
            assert call(g.cref, t=None) == INVALID and b"null terms" in lib.ocn_last_error()
            for kind, wording in ((L.BUOYANCY_TRACER, b"T (or b) tracer is NULL"), (L.BUOYANCY_SEAWATER_TS, b"tracer is NULL"),
                                  (L.BUOYANCY_SEAWATER_S, b"S tracer is NULL"), (9, b"unknown buoyancy")):
                t = L.CModelTerms()
                t.buoyancy = kind
                assert call(g.cref, t=t) == INVALID and wording in lib.ocn_last_error()
        for name in L.TKE_DISSIPATION_FIELDS:
            for bad in (float("nan"), float("inf")):
                c = pkg.TKEDissipationVerticalDiffusivity().c_struct()
                setattr(c, name, bad)
                if not (name.startswith("maximum") and bad == float("inf")):
                    assert call(g.cref, c=c) == INVALID and (b"finite" in lib.ocn_last_error() or b"NaN" in lib.ocn_last_error()), name
        c = pkg.TKEDissipationVerticalDiffusivity().c_struct()
        c.stability_functions = 2
        assert call(g.cref, c=c) == INVALID and b"unknown stability functions" in lib.ocn_last_error()
        n = {top: 6, dif: 8, sub: 17}[call]
        for q in range(n):
            f = list(p[:n])
            f[q] = None
            if call is sub and q == 16:  # (the scratch array: needed with solve != 0 only, checked below)
                continue
            assert call(g.cref, f=tuple(f)) == INVALID and b"null pointer" in lib.ocn_last_error(), (n, q)
    # Value / Gradient top conditions are no fluxes
    for kind in (L.BC_VALUE, L.BC_GRADIENT):
        bc = C.pointer(L.CBc(kind, 0, 1.0, 0.0, None))
        assert top(g.cref, tops=(bc, none)) == INVALID and b"only a Flux" in lib.ocn_last_error()
        assert top(g.cref, tops=(none, bc)) == INVALID and b"only a Flux" in lib.ocn_last_error()
    args = list(p[:6])  # (zc, u, v, e, Qe, Qϵ)
    args[5] = args[4]
    assert top(g.cref, f=tuple(args)) == INVALID and b"two different planes" in lib.ocn_last_error()
    for dt in (-1.0, float("nan"), float("inf")):
        assert sub(g.cref, dtau=dt) == INVALID and b"dtau" in lib.ocn_last_error()
    assert sub(g.cref, chi=float("nan")) == INVALID and b"chi" in lib.ocn_last_error()
    # aliases.  The diffusivities: (u, v, e, ϵ, κu, κc, κe, κϵ)
    for a in range(4, 8):
        for b_ in range(a + 1, 8):
            args = list(p[:8])
            args[b_] = args[a]
            assert dif(g.cref, f=tuple(args)) == INVALID and b"four different arrays" in lib.ocn_last_error()
    args = list(p[:8])
    args[3] = args[2]
    assert dif(g.cref, f=tuple(args)) == INVALID and b"e and eps" in lib.ocn_last_error()
    # the substep: (u⁺, v⁺, uⁿ, vⁿ, e, ϵ, κu, κc, κe, κϵ, Le, Lϵ, Gⁿe, G⁻e, Gⁿϵ, G⁻ϵ, scratch)
    for a, b_ in ((8, 6), (8, 7), (9, 6), (9, 7), (9, 8)):
        args = list(p[:17])
        args[a] = args[b_]
        assert sub(g.cref, f=tuple(args)) == INVALID and b"kappa_e and kappa_eps are written" in lib.ocn_last_error(), (a, b_)
    cells = (4, 5, 10, 11, 12, 13, 14, 15, 16)
    for n_, a in enumerate(cells):
        for b_ in cells[n_ + 1:]:
            args = list(p[:17])
            args[b_] = args[a]
            assert sub(g.cref, f=tuple(args)) == INVALID and b"different arrays" in lib.ocn_last_error(), (a, b_)
    args = list(p[:17])
    args[16] = None
    assert sub(g.cref, f=tuple(args), solve=1) == INVALID and b"scratch" in lib.ocn_last_error()
    for q in (4, 5):
        t = L.CModelTerms()
        t.buoyancy, t.T = L.BUOYANCY_TRACER, p[q]
        assert sub(g.cref, t=t) == INVALID and b"buoyancy tracer" in lib.ocn_last_error()


# ---- the seeded inputs of the GPU tests -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("buoyancy", ["SeawaterBuoyancy", "BuoyancyTracer"])
@pytest.mark.parametrize("n", range(len(TD.CASES)), ids=TD.IDS)
def test_seeded_inputs_take_every_branch_in_some_cells_and_not_in_all(pkg, n, buoyancy):
    """what tests/test_gpu_tke_dissipation.py asserts first, on the restatement alone, so that a share cannot fail first on the GPU: ϵ clamped up
    to its floor, αᴺ at its minimum, αᴹ at its maximum, e < 0, e <= eᵐⁱⁿ, wb > 0, wb < 0, N² < 0, N² >= 0 and each of the four κ maxima, each in
    at least one cell or face and not in all; the restatement's results are finite"""
    pg = TD.make_grid(pkg, None, n)
    c = TD.make_inputs(pg, n)
    sh = TD.shares_of_case(pg, c, buoyancy)
    assert len(sh) == 13 and all(0 < v < 1 for v in sh.values()), sh
