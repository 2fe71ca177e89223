"""The extended-precision build of the oracle (oracle/extended.py: ocn_oracle.c with long double arithmetic) against the Float64 build,
without a GPU: exact agreement where both are exact, agreement within a bound derived from the operation count elsewhere, and the
properties of the structured inputs (tests/fast_math_cases.py) that the GPU accuracy tests rely on."""
import numpy as np
import pytest

import fast_math_cases as FC
import smagorinsky_numpy as SN
from helpers import stretched_faces
from oracle import extended as X
from oracle import oracle as O

LD = np.longdouble
LOCS = (1, 2, 4, 0)
NAMES = ("u", "v", "w", "c")


def test_long_double_is_wider_than_float64():
    assert np.finfo(LD).nmant >= 63
    a = X.widen(np.array([[[1.0]]]))
    assert a.dtype == LD and (a + LD(2.0) ** -60)[0, 0, 0] != 1  # arithmetic really carries the extra bits


def _integer_fields(og, rng):
    f = {}
    for n, l in zip(NAMES, LOCS):
        a = og.zeros(l)
        a[...] = rng.integers(-4, 5, a.shape).astype(np.float64)
        O.fill_halo_regions(og, a, l)
        f[n] = a
    return f


@pytest.mark.parametrize("topo,halo", [("PPP", (1, 1, 1)), ("PPB", (3, 3, 3)), ("BBB", (2, 2, 2))])
def test_builds_agree_exactly_where_both_are_exact(topo, halo):
    """Small-integer fields on a grid with power-of-two spacings (1/2, 1/4, 1/8): every Centered(2) flux, every difference quotient,
    every product with an area and with 1 / V is a dyadic rational of a few bits, so both builds compute the exact result.  Also pins
    the layout of the long double structures (a wrong offset of dx .. dzf, f .. yf would not survive this)."""
    og = O.Grid((8, 8, 16), x=(0, 4), y=(0, 2), z=(0, 2), topology=topo, halo=halo)
    assert (og.dx, og.dy, og.dz) == (0.5, 0.25, 0.125)
    f = _integer_fields(og, np.random.default_rng(3))
    u, v, w, c = (f[n] for n in NAMES)
    G = [og.zeros(l) for l in LOCS]
    O.momentum_tendencies(og, u, v, w, *G[:3], scheme=O.ADV_CENTERED2)
    O.tracer_tendency(og, u, v, w, c, G[3], scheme=O.ADV_CENTERED2)
    Gx = X.momentum_tendencies(og, u, v, w, scheme=O.ADV_CENTERED2) + [X.tracer_tendency(og, u, v, w, c, scheme=O.ADV_CENTERED2)]
    for a, b, n in zip(G, Gx, NAMES):
        assert b.dtype == LD and np.abs(a).max() > 0
        np.testing.assert_array_equal(b, a.astype(LD), err_msg=f"Centered2 G{n}")
    np.testing.assert_array_equal(X.divergence(og, u, v, w), O.divergence(og, u, v, w).astype(LD))
    Gc = og.zeros(0)
    O.tracer_diffusion(og, 0.375, c, Gc)
    np.testing.assert_array_equal(X.tracer_diffusion(og, 0.375, c, og.zeros(0)), Gc.astype(LD))
    ph = O.Physics(f=0.5, nu=0.25, buoyancy="BuoyancyTracer")
    G2 = [a.copy(order="F") for a in G[:3]]
    O.momentum_extra_tendencies(og, ph, u, v, w, c, None, None, *G2)
    for a, b, n in zip(G2, X.momentum_extra_tendencies(og, ph, u, v, w, c, None, None, *G[:3]), "uvw"):
        np.testing.assert_array_equal(b, a.astype(LD), err_msg=f"extra terms G{n}")
    # halo fills are copies
    for n, l in zip(NAMES, LOCS):
        d = f[n].copy(order="F")
        d[:og.Hx], d[:, -og.Hy:], d[:, :, :og.Hz] = -1, -2, -3
        a = X.widen(d)
        O.fill_halo_regions(og, d, l)
        X.fill_halo_regions(og, a, l)
        np.testing.assert_array_equal(a, d.astype(LD), err_msg=f"halo fill of {n}")


def _grid(case):
    size, topo, z = case
    return O.Grid(size, x=(0, 2 * np.pi), y=(0, 2 * np.pi), z=stretched_faces(size[2]) if z == "stretched" else z, topology=topo,
                  halo=(3, 3, 3))


CASES = [((16, 12, 10), "PPB", "stretched"), ((12, 10, 9), "PBB", (-1.0, 0.0))]
# Operations on the path to one tendency value, each contributing at most one rounding of relative size ε/2 to a partial result
# that is itself bounded by the local magnitude s (products of values, areas and reciprocal volumes: no cancellation amplifies a
# LINEAR scheme's error beyond s):
#   Centered2     per flux 3 (interpolation) + 3 (second one) + 2 (area, product) = 8;    6 fluxes + 3 differences + 2 sums + 2 = 55
#   UpwindBiased5 per flux 11 (Centered4 of area * velocity: 4 + 4 + 3) + 9 (5-point stencil) + 1 = 21;   6 x 21 + 7 = 133
#   WENO5         per flux 11 + 75 (3 x 11 smoothness, 2 tau, 6 ratios, 9 alphas, 2 + 3 weights, 15 candidates, 5 combination) + 1 = 87;
#                 6 x 87 + 7 = 529.  The count bounds the error only while the nonlinear weights are well conditioned.  They are ratios
#                 tau / (beta + eps) of sums of squares formed from VALUES, squared: on a small perturbation of a large mean (mean_*) the
#                 betas lose their digits to cancellation, and at a front (front_*) the ratios reach 1e8 .. 1e16 on the quiet side and the
#                 weights hang on differences of rounded betas -- no operation count bounds that (measured here: 289 eps s in Gv of
#                 front_x).  Those regimes are measured per cell, as E_64, in tests/test_gpu_fast_math_accuracy.py and left out here.
#   diffusion     per flux 1 + 1 + 1 + 1 (difference, quotient, κ, area) = 4;   6 x 4 + 3 + 2 + 2 = 31 on top of the advective operations
#   extra terms   Coriolis 8, pressure gradient 3, viscous divergence 6 fluxes x 9 + 7 = 61: 72 on top of the advective operations
OPS = {O.ADV_CENTERED2: 55, O.ADV_UPWIND5: 133, O.ADV_WENO5: 529}
LINEAR_INPUTS = ("noise", "smooth", "mean_T", "mean_S", "front_x", "front_z", "aspect", "rest_one", "patchy", "scale_1e-30", "scale_1e+20")
WENO_INPUTS = ("noise", "smooth", "aspect", "rest_one", "patchy", "scale_1e-30", "scale_1e+20")


@pytest.mark.parametrize("case", CASES, ids=["PPB-stretched", "PBB"])
@pytest.mark.parametrize("scheme", [O.ADV_CENTERED2, O.ADV_UPWIND5, O.ADV_WENO5], ids=["Centered2", "UpwindBiased5", "WENO5"])
def test_builds_agree_within_the_operation_count(case, scheme):
    og = _grid(case)
    for inp in (WENO_INPUTS if scheme == O.ADV_WENO5 else LINEAR_INPUTS):
        f = FC.make(og, inp)
        u, v, w, c = (f[n] for n in NAMES)
        G = [og.zeros(l) for l in LOCS]
        O.momentum_tendencies(og, u, v, w, *G[:3], scheme=scheme)
        O.tracer_tendency(og, u, v, w, c, G[3], scheme=scheme)
        Gx = X.momentum_tendencies(og, u, v, w, scheme=scheme) + [X.tracer_tendency(og, u, v, w, c, scheme=scheme)]
        for a, b, n in zip(G, Gx, NAMES):
            s = FC.advective_scale(og, u, v, w, f[n])
            E, at, exact0 = FC.error_in_eps(og.interior_N(a), og.interior_N(b), s)
            print(f"scheme {scheme} {inp:12s} G{n}: {E:8.2f} eps s (bound {OPS[scheme] / 2})")
            assert exact0 and E <= OPS[scheme] / 2, f"{inp} G{n}: {E} at {at}"
        assert any(np.abs(og.interior_N(b)).max() > 0 for b in Gx)


@pytest.mark.parametrize("case", CASES, ids=["PPB-stretched", "PBB"])
def test_diffusion_and_extra_terms_agree_within_the_operation_count(case):
    og = _grid(case)
    nu, kappa, fc = 1e-1, 0.2, 0.3
    for inp in LINEAR_INPUTS:
        f = FC.make(og, inp)
        u, v, w, c = (f[n] for n in NAMES)
        ph = O.Physics(f=fc, nu=nu, buoyancy="BuoyancyTracer")
        pHY = og.zeros(0)
        O.update_hydrostatic_pressure(og, ph, c, None, pHY)
        G = [og.zeros(l) for l in LOCS]
        O.momentum_tendencies(og, u, v, w, *G[:3], scheme=O.ADV_CENTERED2)
        O.tracer_tendency(og, u, v, w, c, G[3], scheme=O.ADV_CENTERED2)
        Gx = X.momentum_tendencies(og, u, v, w, scheme=O.ADV_CENTERED2) + [X.tracer_tendency(og, u, v, w, c, scheme=O.ADV_CENTERED2)]
        Gx = X.momentum_extra_tendencies(og, ph, u, v, w, c, None, pHY, *Gx[:3]) + [X.tracer_diffusion(og, kappa, c, Gx[3])]
        O.momentum_extra_tendencies(og, ph, u, v, w, c, None, pHY, *G[:3])
        O.tracer_diffusion(og, kappa, c, G[3])
        h = FC.smallest_spacing(og)
        dU = np.maximum(np.maximum(FC.local_max_difference(og, u, 2), FC.local_max_difference(og, v, 2)), FC.local_max_difference(og, w, 2))
        hor = LD(nu) * dU / (h * h) + LD(fc) * np.maximum(FC.local_max(og, u, 2), FC.local_max(og, v, 2)) + FC.local_max_difference(og, pHY, 2) / h
        extra = [hor, hor, LD(nu) * dU / (h * h), FC.diffusive_scale(og, kappa, c)]
        for a, b, n, e, ops in zip(G, Gx, NAMES, extra, (72, 72, 72, 31)):
            s = FC.advective_scale(og, u, v, w, f[n]) + e
            E, at, exact0 = FC.error_in_eps(og.interior_N(a), og.interior_N(b), s)
            print(f"{inp:12s} G{n}: {E:8.2f} eps s (bound {(55 + ops) / 2})")
            assert exact0 and E <= (55 + ops) / 2, f"{inp} G{n}: {E} at {at}"


def test_amd_builds_agree_and_reach_both_sides_of_the_guards():
    """νₑ, κₑ: ratios of sums of products of three normalised gradients; the numerator r is a sum of ~30 signed terms of size |∇u|³ that
    may cancel, so the error is bounded relative to C Δ² max|δu| / Δ only through the ratio (terms) / q <= 1 per term: 30 terms x ~10
    operations each.  patchy and rest_one put q == 0 / σ == 0 cells next to cells of the general path."""
    og = _grid(CASES[0])
    dzc = og.dzc[og.Hz:og.Hz + og.Nz].astype(LD)
    d2 = (3 / (1 / LD(2 * og.dx) ** 2 + 1 / LD(2 * og.dy) ** 2 + 1 / (2 * dzc) ** 2)).reshape(1, 1, -1)
    for inp in ("noise", "smooth", "patchy", "rest_one", "aspect", "scale_1e-30"):
        f = FC.make(og, inp)
        u, v, w, c = (f[n] for n in NAMES)
        nu, ka = og.zeros(0), og.zeros(0)
        O.amd_viscosity(og, 1 / 12, u, v, w, nu)
        O.amd_diffusivity(og, 1 / 7, u, v, w, c, ka)
        for a, b, C_ in ((nu, X.amd_viscosity(og, 1 / 12, u, v, w), 1 / 12), (ka, X.amd_diffusivity(og, 1 / 7, u, v, w, c), 1 / 7)):
            E, at, exact0 = FC.error_in_eps(og.interior_N(a), og.interior_N(b), FC.eddy_scale(og, LD(C_) * d2, u, v, w))
            print(f"AMD {inp:12s}: {E:8.2f} eps s")
            assert exact0 and E <= 300, f"{inp}: {E} at {at}"
        if inp in ("patchy", "rest_one"):
            q = og.interior_N(nu)
            assert np.count_nonzero(q == 0) > 0 and (inp == "rest_one" or np.count_nonzero(q > 0) > 0)


def test_smagorinsky_restatement_is_dtype_generic():
    og = _grid(CASES[0])
    f = FC.make(og, "smooth")
    u, v, w = (f[n] for n in "uvw")
    kw = dict(lilly=True, Cb=1.0, buoyancy="BuoyancyTracer")
    nu = SN.smagorinsky_viscosity(og, u, v, w, 0.23, T=f["c"], **kw)
    nux = SN.smagorinsky_viscosity(og, X.widen(u), X.widen(v), X.widen(w), 0.23, T=X.widen(f["c"]), **kw)
    assert nu.dtype == np.float64 and nux.dtype == LD
    rel = np.abs(nu - nux).max() / nux.max()
    assert 0 < rel <= 64 * FC.EPS  # the Float64 result rounds; the extended one is not merely its copy


def test_structured_inputs_have_the_documented_structure():
    og = _grid(CASES[0])
    for name in FC.NAMES:
        f = FC.make(og, name)
        g = FC.make(og, name)
        for n, l in zip(NAMES, LOCS):
            assert f[n].dtype == np.float64 and f[n].shape == og.shape(l) and np.isfinite(f[n]).all()
            np.testing.assert_array_equal(f[n], g[n])  # seeded
            filled = f[n].copy(order="F")
            O.fill_halo_regions(og, filled, l)
            np.testing.assert_array_equal(filled, f[n])  # halos filled
    rest = FC.make(og, "rest")
    assert all(not rest[n].any() for n in NAMES)
    one = FC.make(og, "rest_one")
    assert all(np.count_nonzero(og.interior_N(one[n])) == 1 for n in NAMES)
    p = FC.make(og, "patchy")
    for n in NAMES:
        a = og.interior_N(p[n])
        assert not a[:og.Nx // 2, :og.Ny // 2, :og.Nz // 2].any() and np.count_nonzero(a) > a.size // 2
    m = FC.make(og, "mean_S")
    assert abs(og.interior_N(m["c"]) - 35).max() <= 1e-6 and abs(og.interior_N(m["u"]) - 10).max() <= 1e-3
    fr = FC.make(og, "front_x")["c"]
    assert np.abs(og.interior_N(fr)[:og.Nx // 2 - 4]).max() < 1e-3 and og.interior_N(fr)[og.Nx // 2 + 4:].min() > 0.49
    a = FC.make(og, "aspect")
    assert np.abs(a["w"]).max() <= 1e-6 < 0.5 < np.abs(a["u"]).max()
    sm = og.interior_N(FC.make(og, "smooth")["c"])
    assert 0.5 < np.abs(sm).max() <= 1.0
    for d in range(3):  # at least 8 cells per wavelength: neighbouring values differ by at most 2 sin(pi / 8) of the amplitude
        assert np.abs(np.diff(sm, axis=d)).max() <= 2 * np.sin(np.pi / 8) + 1e-12
    for s in FC.SCALES:
        q = FC.make(og, f"scale_{s:g}")["u"]
        assert 0.5 * s < np.abs(q).max() <= s


def test_local_magnitudes():
    og = _grid(CASES[0])
    one = FC.make(og, "rest_one")
    s = FC.advective_scale(og, one["u"], one["v"], one["w"], one["c"])
    assert s.dtype == LD and s.shape == (og.Nx, og.Ny, og.Nz)
    assert np.count_nonzero(s) > 0 and np.count_nonzero(s == 0) > 0  # zero away from the nonzero cells (beyond the stencil's reach)
    Gc = X.tracer_tendency(og, one["u"], one["v"], one["w"], one["c"])
    assert not og.interior_N(Gc)[s == 0].any()  # ... and the tendency vanishes there
    tiny = FC.make(og, "scale_1e-160")
    st = FC.advective_scale(og, tiny["u"], tiny["v"], tiny["w"], tiny["u"])
    assert st.min() > 0 and st.max() < 1e-300  # no underflow in the long double product
