"""Per-cell accuracy of the fast-math build (OCN_STRICT=0 of tendencies.hip, physics.hip, amd.hip, smagorinsky.hip, general.hip) on
structured inputs (tests/fast_math_cases.py), against the extended-precision oracle (oracle/extended.py).

For every kernel family x shape x input there are three results: G_fast (GPU, MATH_FAST), G_64 (the Float64 oracle) and G_ext (the same
oracle source in long double).  Differences are divided, cell by cell, by ε s with ε = 2^-52 and the LOCAL magnitude s of the cell
(fast_math_cases.py; np.longdouble so that products of tiny fields do not underflow), never by a global maximum:

  advective tendencies   s = (largest |u|, |v|, |w| in the (2H+1)³ neighbourhood) x (largest |advected field| there)
                             / (smallest spacing of the cell: Δx, Δy, Δzᶜ, Δzᶠ of its level, Flat directions left out)
  extra momentum terms   s = the advective s
                           + |f| (largest |u|, |v| there) + (largest |b| there, when w feels the buoyancy directly)
                           + (largest |difference of neighbouring pHY′| in the 5³ neighbourhood) / (smallest spacing)
                           + (largest ν) x (largest |difference of neighbouring u, v, w| in the 5³ neighbourhood) / (smallest spacing)²
  tracer diffusion       s = the advective s + (largest κ) x (largest |difference of neighbouring c| in 5³) / (smallest spacing)²
  νₑ, κₑ (AMD)           s = C Δ² x (largest |difference of neighbouring u, v, w| in 5³) / (smallest spacing),
                             Δ² = 3 / (1/Δᶠx² + 1/Δᶠy² + 1/Δᶠz²), Δᶠ = 2 Δ (Flat directions: Δ = 1, as the closure takes them)
  νₑ (Smagorinsky)       the same with C Δ² = C² (Δx Δy Δz)^(2/3); κₑ = νₑ / Pr: s / Pr

Where s = 0 the result must equal G_ext exactly.  Assertions, per family, shape and input:

  * G_fast is finite everywhere (every input is inside the documented range of the fast build);
  * E_fast <= 4 max(E_64, 1), E_x = max over cells of |G_x - G_ext| / (ε s).  E_64 is the reference formulation's own rounding error,
    computed on the CPU.  The factor 4: a reciprocal-multiply costs at most about three half-ulps where the strict division costs one;
    FMA contraction never adds a rounding; the reorderings (factored metrics, difference form) are linear.  Both figures are printed;
  * the strict build equals G_64 bit for bit (signed zeros included) on the same inputs.

Kernel selection (launch_momentum_tendencies / launch_tracer_tendency_t in csrc/tendencies.hip; ocn_momentum_tendencies_plan reports the
momentum launch's, and tests/test_gpu_tendency_variants.py asserts it case by case): momentum takes
17 x 15 patches where narrow_tile() prefers them (ranges at least 16 x 14) and 32 x 8 patches otherwise, for ranges of at least
16 x 8 x 4 on a non-Flat z, the per-cell kernel below that; the tracer kernel always 32 x 8 patches; the z chunk is halved from Nz while
longer than 16 (Nz = 40: 10, Nz = 20: 10).  Grids with walls in x / y go through csrc/general.hip.  On a failure the worst cell is
reported with its indices modulo the cells a patch owns (16 x 14 and 31 x 7) and the z chunk: a seam shows as a plane of outliers.
"""
import ctypes as C

import numpy as np
import pytest

import fast_math_cases as FC
import smagorinsky_numpy as SN
from helpers import from_dev, make_pair, stretched_faces, to_dev

pytestmark = pytest.mark.gpu

LD = np.longdouble
NAMES4 = ("u", "v", "w", "c")
LOCS4 = (1, 2, 4, 0)
FACTOR = 4.0
LARGE_INPUTS = ("noise", "smooth", "front_x", "front_z", "patchy", "mean_T")

# (size, topology, z): z = "stretched" -> helpers.stretched_faces, None -> Flat, else the extent
S16 = ((16, 12, 10), "PPB", "stretched")
WENO_SHAPES = [(((16, 16, 16), "PPP", (0, 2 * np.pi)), FC.NAMES),            # tiled, one z chunk
               (((32, 28, 40), "PPP", (0, 2.0)), LARGE_INPUTS),              # 2 x 2 patches of 17 x 15, four z chunks
               (((32, 28, 40), "PPB", "stretched"), LARGE_INPUTS),
               (((70, 9, 20), "PPP", (0, 3.0)), LARGE_INPUTS),               # 32 x 8 patches, two z chunks
               (S16, FC.NAMES),                                              # 32 x 8, walls in z, per-level metrics
               (((13, 17, 19), "PPP", (0, 1.0)), FC.NAMES),                  # per-cell kernel
               (((24, 16, 1), "PPF", None), FC.NAMES),                       # per-cell kernel, Flat z
               (((30, 18, 8), "BBB", (-1.0, 0.0)), FC.NAMES),                # general.hip: tiled interior box + per-cell rim
               (((12, 10, 9), "PBB", (-1.0, 0.0)), FC.NAMES)]                # general.hip: per-cell only


def _params(shapes):
    out, ids = [], []
    for shape, inputs in shapes:
        for name in inputs:
            out.append((shape, name))
            ids.append(f"{'x'.join(map(str, shape[0]))}-{shape[1]}{'-stretched' if isinstance(shape[2], str) else ''}-{name}")
    return dict(argnames="shape,inp", argvalues=out, ids=ids)


_cache = {}


def _setup(oracle, ocn, shape, inp):
    """grids and the input fields of one (shape, input): built once, shared, never modified"""
    key = (shape[0], shape[1], str(shape[2]), inp)
    if key not in _cache:
        size, topo, z = shape
        if isinstance(z, str):
            z = stretched_faces(size[2])
        og, pg = make_pair(oracle, ocn, size, topo, z=z)
        _cache[key] = (og, pg, FC.make(og, inp), {})
    return _cache[key]


def _on_device(ocn, pg, f, mode, run):
    """upload u, v, w, c, run(dev fields) in the given math mode, return the parent arrays of what it returns"""
    ocn.set_math_mode(mode)
    try:
        dev = {n: to_dev(ocn, pg, l, f[n]) for n, l in zip(NAMES4, LOCS4)}
        out = run(dev)
        ocn.sync_device()
    finally:
        ocn.set_math_mode(ocn.MATH_STRICT)
    return [np.asfortranarray(from_dev(a)) for a in out]


def _chunk(og):
    """the z chunk of the momentum launch on this grid, from the launcher's own decision (ocn_momentum_tendencies_plan; 1 for the per-cell
    kernel and where the query does not apply: walls in x / y)"""
    import oceananigans_jl_amd as ocn
    g = ocn._lib.CGrid(og.Nx, og.Ny, og.Nz, og.Hx, og.Hy, og.Hz, og.tx, og.ty, og.tz, 0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, None, None)
    st, plan = ocn._lib.momentum_tendencies_plan(g)
    return plan["KZ"] if st == 0 and plan["KZ"] > 0 else 1


def _check_fast(og, label, names, got, G64, Gext, scales):
    """finite; exact where s == 0; E_fast <= FACTOR max(E_64, 1)"""
    failures = []
    for n, a, b, x, s in zip(names, got, G64, Gext, scales):
        a, b, x = (og.interior_N(q) for q in (a, b, x))
        assert np.isfinite(a).all(), f"{label} {n}: {np.count_nonzero(~np.isfinite(a))} non-finite values in the fast build's result"
        Ef, at, exact_f = FC.error_in_eps(a, x, s)
        E64, _, exact_64 = FC.error_in_eps(b, x, s)
        print(f"{label:58s} {n:8s} E_fast {Ef:10.3f}  E_64 {E64:10.3f}  cells with s = 0: {np.count_nonzero(s == 0)}")
        assert exact_64, f"{label} {n}: the Float64 oracle differs from the extended one where the local magnitude is 0"
        if not exact_f:
            failures.append(f"{n}: differs from the extended oracle where the local magnitude is 0")
        if Ef > FACTOR * max(E64, 1.0):
            i, j, k = at
            failures.append(f"{n}: E_fast = {Ef:.2f} > {FACTOR:g} max(E_64 = {E64:.2f}, 1) at (i, j, k) = {at}; mod 16 x 14 patches "
                            f"({(i - 1) % 16}, {(j - 1) % 14}), mod 31 x 7 patches ({(i - 1) % 31}, {(j - 1) % 7}), "
                            f"mod the z chunk {(k - 1) % _chunk(og)}")
    assert not failures, f"{label}: " + "; ".join(failures)


def _check_strict(og, label, names, got, G64):
    for n, a, b in zip(names, got, G64):
        a, b = og.interior_N(a), og.interior_N(b)
        same = (a == b) & (np.signbit(a) == np.signbit(b))
        assert same.all(), (f"{label} {n}: the strict build differs from the oracle in {np.count_nonzero(~same)} cells, first at "
                            f"{tuple(int(q) + 1 for q in np.argwhere(~same)[0])}")


# ------------------------------------------------------------------------------------------------------------------------------
# advection
# ------------------------------------------------------------------------------------------------------------------------------
def _advection_reference(oracle, X, og, f, store, scheme):
    if ("adv", scheme) not in store:
        O = oracle
        G64 = [og.zeros(l) for l in LOCS4]
        O.momentum_tendencies(og, f["u"], f["v"], f["w"], *G64[:3], scheme=scheme)
        O.tracer_tendency(og, f["u"], f["v"], f["w"], f["c"], G64[3], scheme=scheme)
        Gext = X.momentum_tendencies(og, f["u"], f["v"], f["w"], scheme=scheme) + [X.tracer_tendency(og, f["u"], f["v"], f["w"], f["c"], scheme=scheme)]
        s = [FC.advective_scale(og, f["u"], f["v"], f["w"], f[n]) for n in NAMES4]
        store[("adv", scheme)] = (G64, Gext, s)
    return store[("adv", scheme)]


def _run_advection(ocn, pg, scheme):
    """scheme 0 through the plain WENO entry points (the flagship path), 1 / 2 through the model-terms ones"""
    def run(d):
        G = [ocn.Field(l, pg) for l in LOCS4]
        if scheme == 0:
            ocn._lib.call("ocn_compute_momentum_tendencies", pg.cref, d["u"].ptr, d["v"].ptr, d["w"].ptr, G[0].ptr, G[1].ptr, G[2].ptr, None, 0)
            ocn._lib.call("ocn_compute_tracer_tendency", pg.cref, d["u"].ptr, d["v"].ptr, d["w"].ptr, d["c"].ptr, G[3].ptr, None, 0)
        else:
            t = ocn._lib.CModelTerms()
            t.advection = scheme
            ocn._lib.call("ocn_compute_momentum_tendencies_terms", pg.cref, C.byref(t), d["u"].ptr, d["v"].ptr, d["w"].ptr, G[0].ptr, G[1].ptr,
                          G[2].ptr, None, 0)
            ocn._lib.call("ocn_compute_tracer_tendency_terms", pg.cref, C.byref(t), 0.0, None, d["u"].ptr, d["v"].ptr, d["w"].ptr, d["c"].ptr,
                          G[3].ptr, None, 0)
        return G
    return run


@pytest.fixture(scope="module")
def X(oracle):
    from oracle import extended
    extended.lib()
    return extended


@pytest.mark.parametrize(**_params(WENO_SHAPES))
def test_weno5_fast_error_per_cell(oracle, X, ocn, shape, inp):
    og, pg, f, store = _setup(oracle, ocn, shape, inp)
    G64, Gext, s = _advection_reference(oracle, X, og, f, store, 0)
    got = _on_device(ocn, pg, f, ocn.MATH_FAST, _run_advection(ocn, pg, 0))
    _check_fast(og, f"WENO5 {shape[0]} {shape[1]} {inp}", ("Gu", "Gv", "Gw", "Gc"), got, G64, Gext, s)


@pytest.mark.parametrize(**_params(WENO_SHAPES))
def test_weno5_strict_bitwise_on_structured_inputs(oracle, X, ocn, shape, inp):
    og, pg, f, store = _setup(oracle, ocn, shape, inp)
    G64, _, _ = _advection_reference(oracle, X, og, f, store, 0)
    got = _on_device(ocn, pg, f, ocn.MATH_STRICT, _run_advection(ocn, pg, 0))
    _check_strict(og, f"WENO5 {shape[0]} {shape[1]} {inp}", ("Gu", "Gv", "Gw", "Gc"), got, G64)


@pytest.mark.parametrize("scheme", [1, 2], ids=["Centered2", "UpwindBiased5"])
@pytest.mark.parametrize(**_params([(S16, FC.NAMES)]))
def test_linear_schemes_fast_error_per_cell(oracle, X, ocn, shape, inp, scheme):
    og, pg, f, store = _setup(oracle, ocn, shape, inp)
    G64, Gext, s = _advection_reference(oracle, X, og, f, store, scheme)
    got = _on_device(ocn, pg, f, ocn.MATH_FAST, _run_advection(ocn, pg, scheme))
    _check_fast(og, f"scheme {scheme} {shape[0]} {shape[1]} {inp}", ("Gu", "Gv", "Gw", "Gc"), got, G64, Gext, s)


@pytest.mark.parametrize("scheme", [1, 2], ids=["Centered2", "UpwindBiased5"])
@pytest.mark.parametrize(**_params([(S16, FC.NAMES)]))
def test_linear_schemes_strict_bitwise_on_structured_inputs(oracle, X, ocn, shape, inp, scheme):
    og, pg, f, store = _setup(oracle, ocn, shape, inp)
    G64, _, _ = _advection_reference(oracle, X, og, f, store, scheme)
    got = _on_device(ocn, pg, f, ocn.MATH_STRICT, _run_advection(ocn, pg, scheme))
    _check_strict(og, f"scheme {scheme} {shape[0]} {shape[1]} {inp}", ("Gu", "Gv", "Gw", "Gc"), got, G64)


# ------------------------------------------------------------------------------------------------------------------------------
# physics.hip: Coriolis, buoyancy, hydrostatic pressure gradient, ∇·ν∇ (a number, or the νₑ / κₑ fields of an eddy closure), tracer
# diffusion, on top of Centered2 advection
# ------------------------------------------------------------------------------------------------------------------------------
PHYSICS_SHAPES = [(S16, FC.NAMES), (((70, 9, 8), "PPB", (-1.0, 0.0)), FC.NAMES)]
F_COR, NU, KAPPA = 0.3, 1e-1, 0.2


def _physics_reference(oracle, X, og, f, store, fields):
    """fields False: constant ν, κ, f-plane, BuoyancyTracer c with its hydrostatic pressure; True: νₑ, κₑ arrays, nothing else"""
    if ("phys", fields) not in store:
        O = oracle
        u, v, w, c = (f[n] for n in NAMES4)
        G64, Gext, s = _advection_reference(oracle, X, og, f, store, 1)
        G64 = [a.copy(order="F") for a in G64]
        h = FC.smallest_spacing(og)
        dU = np.maximum(np.maximum(FC.local_max_difference(og, u, 2), FC.local_max_difference(og, v, 2)), FC.local_max_difference(og, w, 2))
        if fields:
            rng = np.random.default_rng(FC.SEED + 1)
            amp = max(float(np.abs(a).max()) for a in (u, v, w))  # (a viscosity of the fields' own magnitude: no term drowns the other)
            nu_e, ka_e = (og.zeros(0) for _ in range(2))
            for a in (nu_e, ka_e):
                a[...] = min(amp, 1.0) * rng.uniform(0.0, 1e-2, a.shape)
                O.fill_halo_regions(og, a, 0)
            ph = O.Physics(nu=0.0)
            O.momentum_extra_tendencies(og, ph, u, v, w, None, None, None, *G64[:3], nu_e=nu_e)
            O.tracer_diffusion(og, 0.0, c, G64[3], kappa_e=ka_e)
            Gext = X.momentum_extra_tendencies(og, ph, u, v, w, None, None, None, *Gext[:3], nu_e=nu_e) + [
                X.tracer_diffusion(og, 0.0, c, Gext[3], kappa_e=ka_e)]
            visc = FC.local_max(og, nu_e, 2) * dU / (h * h)
            s = [s[0] + visc, s[1] + visc, s[2] + visc, s[3] + FC.diffusive_scale(og, ka_e, c)]
            extra = {"nu_e": nu_e, "kappa_e": ka_e}
        else:
            ph = O.Physics(f=F_COR, nu=NU, buoyancy="BuoyancyTracer")
            pHY = og.zeros(0)
            O.update_hydrostatic_pressure(og, ph, c, None, pHY)
            O.momentum_extra_tendencies(og, ph, u, v, w, c, None, pHY, *G64[:3])
            O.tracer_diffusion(og, KAPPA, c, G64[3])
            Gext = X.momentum_extra_tendencies(og, ph, u, v, w, c, None, pHY, *Gext[:3]) + [X.tracer_diffusion(og, KAPPA, c, Gext[3])]
            visc = LD(NU) * dU / (h * h)
            cor = LD(F_COR) * np.maximum(FC.local_max(og, u, 2), FC.local_max(og, v, 2))
            dp = FC.local_max_difference(og, pHY, 2) / h
            s = [s[0] + visc + cor + dp, s[1] + visc + cor + dp, s[2] + visc, s[3] + FC.diffusive_scale(og, KAPPA, c)]
            extra = {"pHY": pHY}
        store[("phys", fields)] = (G64, Gext, s, extra)
    return store[("phys", fields)]


def _run_physics(ocn, pg, fields, extra):
    def run(d):
        G = [ocn.Field(l, pg) for l in LOCS4]
        t = ocn._lib.CModelTerms()
        t.advection = 1
        keep = [to_dev(ocn, pg, 0, a) for a in extra.values()]
        if fields:
            t.closure, t.nu_e = 2, keep[0].ptr
            kappa, kfield = 0.0, keep[1].ptr
        else:
            t.coriolis, t.f = 1, F_COR
            t.closure, t.nu = 1, NU
            t.buoyancy, t.T, t.pHY = 1, d["c"].ptr, keep[0].ptr
            kappa, kfield = KAPPA, None
        ocn._lib.call("ocn_compute_momentum_tendencies_terms", pg.cref, C.byref(t), d["u"].ptr, d["v"].ptr, d["w"].ptr, G[0].ptr, G[1].ptr,
                      G[2].ptr, None, 0)
        ocn._lib.call("ocn_compute_tracer_tendency_terms", pg.cref, C.byref(t), kappa, kfield, d["u"].ptr, d["v"].ptr, d["w"].ptr, d["c"].ptr,
                      G[3].ptr, None, 0)
        ocn.sync_device()  # (the uploaded νₑ / κₑ / pHY′ fields stay alive until here)
        return G
    return run


@pytest.mark.parametrize("fields", [False, True], ids=["constants", "eddy_fields"])
@pytest.mark.parametrize(**_params(PHYSICS_SHAPES))
def test_extra_terms_fast_error_per_cell(oracle, X, ocn, shape, inp, fields):
    og, pg, f, store = _setup(oracle, ocn, shape, inp)
    G64, Gext, s, extra = _physics_reference(oracle, X, og, f, store, fields)
    got = _on_device(ocn, pg, f, ocn.MATH_FAST, _run_physics(ocn, pg, fields, extra))
    _check_fast(og, f"terms({'fields' if fields else 'constants'}) {shape[0]} {shape[1]} {inp}", ("Gu", "Gv", "Gw", "Gc"), got, G64, Gext, s)


@pytest.mark.parametrize("fields", [False, True], ids=["constants", "eddy_fields"])
@pytest.mark.parametrize(**_params(PHYSICS_SHAPES))
def test_extra_terms_strict_bitwise_on_structured_inputs(oracle, X, ocn, shape, inp, fields):
    og, pg, f, store = _setup(oracle, ocn, shape, inp)
    G64, _, _, extra = _physics_reference(oracle, X, og, f, store, fields)
    got = _on_device(ocn, pg, f, ocn.MATH_STRICT, _run_physics(ocn, pg, fields, extra))
    _check_strict(og, f"terms({'fields' if fields else 'constants'}) {shape[0]} {shape[1]} {inp}", ("Gu", "Gv", "Gw", "Gc"), got, G64)


# ------------------------------------------------------------------------------------------------------------------------------
# AnisotropicMinimumDissipation νₑ, κₑ
# ------------------------------------------------------------------------------------------------------------------------------
AMD_SHAPES = [(S16, FC.NAMES), (((34, 17, 20), "BBB", (-1.0, 0.0)), FC.NAMES)]
CNU, CK = 1 / 12, 1 / 7


def _amd_delta2(og):
    """3 / (1/Δᶠx² + 1/Δᶠy² + 1/Δᶠz²) per level, Δᶠ = 2 Δ (Δ = 1 along a Flat direction), shape (1, 1, Nz)"""
    dzc = np.full(og.Nz, og.dz) if og.dzc is None else og.dzc[og.Hz:og.Hz + og.Nz]
    Fx, Fy, Fz = 2 * LD(og.dx), 2 * LD(og.dy), 2 * dzc.astype(LD)
    return (3 / (1 / (Fx * Fx) + 1 / (Fy * Fy) + 1 / (Fz * Fz))).reshape(1, 1, -1)


def _amd_reference(oracle, X, og, f, store):
    if "amd" not in store:
        O = oracle
        u, v, w, c = (f[n] for n in NAMES4)
        nu, ka = og.zeros(0), og.zeros(0)
        O.amd_viscosity(og, CNU, u, v, w, nu)
        O.amd_diffusivity(og, CK, u, v, w, c, ka)
        ext = [X.amd_viscosity(og, CNU, u, v, w), X.amd_diffusivity(og, CK, u, v, w, c)]
        d2 = _amd_delta2(og)
        s = [FC.eddy_scale(og, LD(CNU) * d2, u, v, w), FC.eddy_scale(og, LD(CK) * d2, u, v, w)]
        s[1] = np.where(FC.local_max_difference(og, c, 2) > 0, s[1], LD(0))  # (no tracer gradient in reach: σ == 0, κₑ = 0)
        store["amd"] = ([nu, ka], ext, s)
    return store["amd"]


def _run_amd(ocn, pg):
    def run(d):
        nu, ka = ocn.Field(0, pg), ocn.Field(0, pg)
        Ck = (C.c_double * 1)(CK)
        ocn._lib.call("ocn_compute_amd_diffusivities", pg.cref, CNU, d["u"].ptr, d["v"].ptr, d["w"].ptr, nu.ptr, 1, Ck,
                      ocn._lib.ptr_array([d["c"].ptr]), ocn._lib.ptr_array([ka.ptr]), 0)
        return [nu, ka]
    return run


@pytest.mark.parametrize(**_params(AMD_SHAPES))
def test_amd_fast_error_per_cell(oracle, X, ocn, shape, inp):
    og, pg, f, store = _setup(oracle, ocn, shape, inp)
    G64, Gext, s = _amd_reference(oracle, X, og, f, store)
    got = _on_device(ocn, pg, f, ocn.MATH_FAST, _run_amd(ocn, pg))
    _check_fast(og, f"AMD {shape[0]} {shape[1]} {inp}", ("nu_e", "kappa_e"), got, G64, Gext, s)


@pytest.mark.parametrize(**_params(AMD_SHAPES))
def test_amd_strict_bitwise_on_structured_inputs(oracle, X, ocn, shape, inp):
    og, pg, f, store = _setup(oracle, ocn, shape, inp)
    G64, _, _ = _amd_reference(oracle, X, og, f, store)
    got = _on_device(ocn, pg, f, ocn.MATH_STRICT, _run_amd(ocn, pg))
    _check_strict(og, f"AMD {shape[0]} {shape[1]} {inp}", ("nu_e", "kappa_e"), got, G64)


# ------------------------------------------------------------------------------------------------------------------------------
# SmagorinskyLilly with buoyancy, Pr != 1
# ------------------------------------------------------------------------------------------------------------------------------
SMAG_C, SMAG_CB, SMAG_PR = 0.23, 1.0, 0.5


def _smag_reference(oracle, X, og, f, store):
    """BuoyancyTracer c scaled so that Cb N² lies on both sides of Σ² (N² ~ δc / Δz against Σ² ~ (δu / Δ)²: c times max|u|² / Δz);
    reference: tests/smagorinsky_numpy.py in Float64 and in np.longdouble"""
    if "smag" not in store:
        u, v, w = (f[n] for n in "uvw")
        amp = max(float(np.abs(a).max()) for a in (u, v, w))
        dzmin = float(FC.smallest_spacing(og).min())
        b = np.asfortranarray(f["c"] * ((amp * amp / dzmin) / max(float(np.abs(f["c"]).max()), 1e-300)))
        kw = dict(lilly=True, Cb=SMAG_CB, buoyancy="BuoyancyTracer", S=None)
        nu = np.array(SN.smagorinsky_viscosity(og, u, v, w, SMAG_C, T=b, **kw))
        nux = np.array(SN.smagorinsky_viscosity(og, X.widen(u), X.widen(v), X.widen(w), SMAG_C, T=X.widen(b), **kw))
        assert nux.dtype == LD
        dzc = np.full(og.Nz, og.dz) if og.dzc is None else og.dzc[og.Hz:og.Hz + og.Nz]
        Df = np.cbrt((LD(og.dx) * LD(og.dy)) * dzc.astype(LD)).reshape(1, 1, -1)
        s = FC.eddy_scale(og, LD(SMAG_C * SMAG_C) * Df * Df, u, v, w)
        store["smag"] = ([nu, nu / SMAG_PR], [nux, nux / LD(SMAG_PR)], [s, s / LD(SMAG_PR)], b)
    return store["smag"]


def _run_smag(ocn, pg, b):
    def run(d):
        L = ocn._lib
        db = to_dev(ocn, pg, 0, b)
        t = L.CModelTerms()
        t.buoyancy, t.T = L.BUOYANCY_TRACER, db.ptr
        cs = L.CSmagorinsky()
        cs.C, cs.Cb, cs.lilly, cs.n_tracers = SMAG_C, SMAG_CB, 1, 1
        cs.Pr[0] = SMAG_PR
        nu, ka = ocn.Field(0, pg), ocn.Field(0, pg)
        L.call("ocn_compute_smagorinsky_diffusivities", pg.cref, C.byref(t), C.byref(cs), d["u"].ptr, d["v"].ptr, d["w"].ptr, nu.ptr,
               L.ptr_array([ka.ptr]), 0)
        ocn.sync_device()
        return [nu, ka]
    return run


def _interior(og, arrays):
    """the restatement returns interior arrays; the device ones are parents"""
    return [np.array(og.interior_N(a)) for a in arrays]


@pytest.mark.parametrize(**_params([(S16, FC.NAMES)]))
def test_smagorinsky_lilly_fast_error_per_cell(oracle, X, ocn, shape, inp):
    og, pg, f, store = _setup(oracle, ocn, shape, inp)
    G64, Gext, s, b = _smag_reference(oracle, X, og, f, store)
    got = _interior(og, _on_device(ocn, pg, f, ocn.MATH_FAST, _run_smag(ocn, pg, b)))
    failures = []
    for n, a, r64, x, sc in zip(("nu_e", "kappa_e"), got, G64, Gext, s):
        assert np.isfinite(a).all(), f"{n}: non-finite values in the fast build's result"
        Ef, at, exact_f = FC.error_in_eps(a, x, sc)
        E64, _, _ = FC.error_in_eps(r64, x, sc)
        print(f"{'Smagorinsky ' + str(shape[0]) + ' ' + inp:58s} {n:8s} E_fast {Ef:10.3f}  E_64 {E64:10.3f}  cells with s = 0: {np.count_nonzero(sc == 0)}")
        if not exact_f:
            failures.append(f"{n}: differs from the extended restatement where the local magnitude is 0")
        if Ef > FACTOR * max(E64, 1.0):
            failures.append(f"{n}: E_fast = {Ef:.2f} > {FACTOR:g} max(E_64 = {E64:.2f}, 1) at {at}")
    assert not failures, "; ".join(failures)


@pytest.mark.parametrize(**_params([(S16, FC.NAMES)]))
def test_smagorinsky_lilly_strict_on_structured_inputs(oracle, X, ocn, shape, inp):
    """bit for bit against the Float64 restatement, signed zeros included"""
    og, pg, f, store = _setup(oracle, ocn, shape, inp)
    G64, _, _, b = _smag_reference(oracle, X, og, f, store)
    got = _interior(og, _on_device(ocn, pg, f, ocn.MATH_STRICT, _run_smag(ocn, pg, b)))
    for n, a, r in zip(("nu_e", "kappa_e"), got, G64):
        same = (a == r) & (np.signbit(a) == np.signbit(r))
        rel = np.abs(a - r).max() / max(float(np.abs(r).max()), 1e-300)
        print(f"Smagorinsky strict {inp} {n}: {np.count_nonzero(~same)} cells differ, max difference {rel / FC.EPS:.2f} eps of max")
        assert same.all(), f"{n}: the strict build differs from the restatement in {np.count_nonzero(~same)} cells"
