"""ScalarDiffusivity(VerticallyImplicitTimeDiscretization(), ν, κ) on the GPU (csrc/implicit_diffusion.hip): the two kernels against the
NumPy restatement of the reference (tests/implicit_diffusion_numpy.py, pinned without a GPU in tests/test_host_implicit_diffusion.py) bit
for bit, the splitting of the explicit closure's term with the existing kernels as yardstick, the exact decay of a cosine mode, and five
steps of both models against the same sequence composed from the public stage functions plus the restatement.

Grids are at most 13 x 6 x 12: Nx = 13 leaves most of the one wave of a block row idle (and is no multiple of the wave width), Ny = 6 needs
two blocks of four rows, Nz = 12 takes two batches of the column sweeps' eight-plane load batches (one full, one partial)."""
import ctypes as C

import numpy as np
import pytest

import implicit_diffusion_numpy as IDN
from helpers import from_dev, stretched_faces, to_dev

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
P, B, F = "Periodic", "Bounded", "Flat"
LOCS = {"u": 1, "v": 2, "w": 4, "c": 0}
# size, topology, z ("stretched" or an interval), halo (a halo is at most the size: Nz = 1, 2 take Hz = Nz)
CASES = [((13, 6, 12), (P, P, B), "stretched", (3, 3, 3)),
         ((13, 6, 12), (B, B, B), "stretched", (3, 3, 3)),
         ((13, 1, 12), (P, F, B), (-1.0, 0.0), (3, 0, 3)),
         ((13, 6, 1), (P, P, B), (-1.0, 0.0), (3, 3, 1)),
         ((13, 6, 2), (P, P, B), "stretched", (3, 3, 2)),
         ((13, 6, 12), (P, P, B), "stretched", (4, 3, 5))]
IDS = ["PPB", "BBB", "PFB", "Nz1", "Nz2", "halo435"]
NUMBERS = [0.1, 100.0]  # diffusion numbers Δt κ / min Δz²


def _grid(ocn, size, topo, z, halo):
    keep = [d for d in range(3) if topo[d] != F]
    zz = stretched_faces(size[2]) if isinstance(z, str) else z
    return ocn.RectilinearGrid(ocn.GPU(), size=tuple(size[d] for d in keep), x=(0, 1), y=(0, 0.5), z=zz, topology=topo,
                               halo=tuple(halo[d] for d in keep))


def _random_parent(pg, loc, rng):
    return rng.uniform(-1, 1, pg.parent_shape(loc))


_inputs = {}


def _case(ocn, n):
    """grid, its description and random parent arrays (halos included) of u, v, w, c, d and of five tendencies; shared, never modified"""
    if n not in _inputs:
        pg = _grid(ocn, *CASES[n])
        g = IDN.describe(pg)
        rng = np.random.default_rng(2024 + n)
        f = {name: _random_parent(pg, LOCS[name[0]], rng) for name in ("u", "v", "w", "c", "c2")}
        G = {name: _random_parent(pg, LOCS[name[0]], rng) for name in ("u", "v", "w", "c", "c2")}
        _inputs[n] = (pg, g, f, G)
    return _inputs[n]


def _dzmin(g):
    return float(np.min(g.dzc[g.Hz:g.Hz + g.Nz]))


# ---- 1. the kernels against the restatement, bit for bit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("number", NUMBERS)
@pytest.mark.parametrize("n", range(len(CASES)), ids=IDS)
def test_implicit_step_equals_the_restatement_bit_for_bit(ocn, n, number):
    """all four locations in ONE launch, each with its own κ; the whole parent arrays are compared (halos, the east / north wall faces and
    w's face Nz + 1 are not written).  The library's build of this file has no FMA contraction and IEEE division: no tolerance."""
    pg, g, f, _ = _case(ocn, n)
    names, kappas = ("u", "v", "w", "c"), (0.7, 0.9, 1.1, 1.3)
    dt = number * _dzmin(g) ** 2 / max(kappas)
    dev = [to_dev(ocn, pg, LOCS[name], f[name]) for name in names]
    ocn._lib.call("ocn_implicit_vertical_diffusion_step", pg.cref, 4, ocn._lib.ptr_array([d.ptr for d in dev]),
                  ocn._lib.i32_array([LOCS[name] for name in names]), (C.c_double * 4)(*kappas), dt, 0)
    ocn.sync_device()
    for name, d, kappa in zip(names, dev, kappas):
        want = IDN.implicit_step(g, f[name], LOCS[name], kappa, dt)
        got = from_dev(d)
        assert np.isfinite(got).all()
        assert np.array_equal(got, want), f"{name}: max difference {np.abs(got - want).max():.3e}"
        if g.Nz > 1 or name == "w":  # (the Center rows of a single layer are the identity: nothing to diffuse against)
            assert not np.array_equal(got, f[name])


def _explicit_part_expected(g, f, G, nu, kappas, ranged=None):
    Du, Dv, Dw = IDN.momentum_explicit_part(g, nu, f["u"], f["v"], f["w"])
    D = {"u": Du, "v": Dv, "w": Dw, "c": IDN.tracer_explicit_part(g, kappas[0], f["c"]), "c2": IDN.tracer_explicit_part(g, kappas[1], f["c2"])}
    ou, ov, ow = IDN.written_offsets(g, ranged is not None)
    i0, i1, j0, j1, k0, k1 = ranged if ranged is not None else (1, g.Nx, 1, g.Ny, 1, g.Nz)
    first = {"u": (ou, 1, 1), "v": (1, ov, 1), "w": (1, 1, ow), "c": (1, 1, 1), "c2": (1, 1, 1)}
    out = {}
    for name, Dn in D.items():
        a = np.array(G[name])
        lo = [max(q, r) for q, r in zip(first[name], (i0, j0, k0))]
        sl = tuple(slice(l - 1, h) for l, h in zip(lo, (i1, j1, k1)))
        psl = tuple(slice(H + s.start, H + s.stop) for H, s in zip((g.Hx, g.Hy, g.Hz), sl))
        a[psl] = a[psl] - Dn[sl]
        out[name] = a
    return out


def _explicit_part_device(ocn, pg, f, G, nu, kappas, ranged=None, with_w=True):
    names = ("u", "v", "w", "c", "c2")
    df = {name: to_dev(ocn, pg, LOCS[name[0]], f[name]) for name in names}
    dG = {name: to_dev(ocn, pg, LOCS[name[0]], G[name]) for name in names}
    L = ocn._lib
    L.call("ocn_add_vertically_implicit_explicit_fluxes", pg.cref, nu, df["u"].ptr, df["v"].ptr, df["w"].ptr, dG["u"].ptr, dG["v"].ptr,
           dG["w"].ptr if with_w else None, 2, (C.c_double * 2)(*kappas), L.ptr_array([df["c"].ptr, df["c2"].ptr]),
           L.ptr_array([dG["c"].ptr, dG["c2"].ptr]), None if ranged is None else L.i32_array(list(ranged)), 0)
    ocn.sync_device()
    return {name: from_dev(dG[name]) for name in names}


@pytest.mark.parametrize("n", range(len(CASES)), ids=IDS)
def test_explicit_part_equals_the_restatement_bit_for_bit(ocn, n):
    """G - (explicit part of the closure term) for u, v, w and two tracers with their own κ, whole parent arrays compared: the excluded
    peripheries of the Face fields, the halos and everything outside a range keep their values.  No tolerance (strict build)."""
    pg, g, f, G = _case(ocn, n)
    nu, kappas = 0.6, (0.8, 1.2)
    want = _explicit_part_expected(g, f, G, nu, kappas)
    got = _explicit_part_device(ocn, pg, f, G, nu, kappas)
    for name in want:
        assert np.isfinite(got[name]).all()
        assert np.array_equal(got[name], want[name]), f"{name}: max difference {np.abs(got[name] - want[name]).max():.3e}"
        assert not np.array_equal(got[name], G[name])
    # a range (KernelParameters: no periphery excluded), and the u, v-only form of the hydrostatic model
    rng = (2, g.Nx - 1, 1, max(1, g.Ny - 1), 1, g.Nz)
    want = _explicit_part_expected(g, f, G, nu, kappas, ranged=rng)
    got = _explicit_part_device(ocn, pg, f, G, nu, kappas, ranged=rng, with_w=False)
    want["w"] = G["w"]
    for name in want:
        assert np.array_equal(got[name], want[name]), f"ranged {name}: max difference {np.abs(got[name] - want[name]).max():.3e}"


# ---- 2. the splitting identity, existing kernels as yardstick --------------------------------------------------------------------------------
@pytest.mark.parametrize("z", ["stretched", (-1.0, 0.0)], ids=["stretched", "uniform"])
def test_explicit_closure_term_is_explicit_part_plus_implicit_operator(ocn, z):
    """For u, v and a tracer: the tendency of the EXISTING explicit closure (closure = 1: ocn_add_momentum_terms on G = 0, and
    ocn_compute_tracer_tendency_terms with a fluid at rest, whose advective part is exactly zero) equals the new explicit part plus
    (φ - A φ) / Δt, A assembled by the restatement: what the tendencies lose, the implicit step gives back.
    w is not part of this identity: the explicit closure's z flux of w is -2 ν ∂z w while the reference's implicit operator for w is ν ∂z²
    (the other half lives in the x / y fluxes of w through continuity), and its Face rows are transcribed as written.
    Bound: the same identity evaluated with the restatement alone on the CPU (all-explicit restatement against restated explicit part +
    (φ - A φ) / Δt) is off by at most 7.8e-12 (stretched, terms up to 6.9e3) / 5.7e-13 (uniform, terms up to 1.4e3) over u, v, c for these
    inputs -- about 1e-15 of the largest term: the cancellation in φ - A φ at Δt = 0.1 min Δz² / κ, divided by Δt -- and the test allows 10
    times the value it measures that way for each field."""
    pg = _grid(ocn, (13, 6, 12), (P, P, B), z, (3, 3, 3))
    g = IDN.describe(pg)
    rng = np.random.default_rng(99)
    f = {name: _random_parent(pg, LOCS[name[0]], rng) for name in ("u", "v", "w", "c")}
    nu, kappa = 0.6, 0.8
    dt = 0.1 * _dzmin(g) ** 2 / kappa
    sl = (slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny), slice(g.Hz, g.Hz + g.Nz))
    L = ocn._lib
    # the existing kernels
    du, dv, dw, dc = (to_dev(ocn, pg, LOCS[name], f[name]) for name in ("u", "v", "w", "c"))
    Gu, Gv, Gw, Gc = (ocn.Field(LOCS[name], pg) for name in ("u", "v", "w", "c"))
    terms = L.CModelTerms()
    terms.closure, terms.nu = 1, nu
    L.call("ocn_add_momentum_terms", pg.cref, C.byref(terms), du.ptr, dv.ptr, dw.ptr, Gu.ptr, Gv.ptr, Gw.ptr, None, 0)
    rest = [ocn.Field(LOCS[name], pg) for name in ("u", "v", "w")]
    L.call("ocn_compute_tracer_tendency_terms", pg.cref, C.byref(terms), kappa, None, rest[0].ptr, rest[1].ptr, rest[2].ptr, dc.ptr, Gc.ptr, None, 0)
    existing = {"u": from_dev(Gu)[sl], "v": from_dev(Gv)[sl], "c": from_dev(Gc)[sl]}
    # the new explicit part on G = 0
    zeros = {name: np.zeros(pg.parent_shape(LOCS[name[0]])) for name in ("u", "v", "w", "c", "c2")}
    ff = dict(f, c2=f["c"])
    new = _explicit_part_device(ocn, pg, ff, zeros, nu, (kappa, kappa))
    # restatement alone
    Du, Dv, _ = IDN.momentum_explicit_part(g, nu, f["u"], f["v"], f["w"])
    Fu, Fv, _ = IDN.momentum_explicit_part(g, nu, f["u"], f["v"], f["w"], all_explicit=True)
    D = {"u": Du, "v": Dv, "c": IDN.tracer_explicit_part(g, kappa, f["c"])}
    Full = {"u": Fu, "v": Fv, "c": IDN.tracer_explicit_part(g, kappa, f["c"], all_explicit=True)}
    for name, k in (("u", nu), ("v", nu), ("c", kappa)):
        a, b, c = IDN.diagonals(g, False, dt, k)
        phi = f[name][sl]
        implicit = (phi - IDN.apply_matrix(a, b, c, phi)) / dt
        cpu = np.abs(-Full[name] - (-D[name] + implicit)).max()
        gpu = np.abs(existing[name] - (new[name][sl] + implicit)).max()
        scale = np.abs(existing[name]).max()
        print(f"{name}: restatement alone {cpu:.3e}, GPU {gpu:.3e}, max |term| {scale:.3e}")
        assert cpu <= 1e-12 * scale, "the restatement itself does not split the explicit closure's term"
        assert gpu <= 10 * cpu
        assert np.abs(implicit).max() > 0.1 * scale  # (the implicit operator carries most of the term: the identity is not vacuous)


# ---- 3. exact decay of a cosine mode ---------------------------------------------------------------------------------------------------------
def _decay_setup(ocn, timestepper, closure, field):
    Nz, m = 12, 2
    pg = ocn.RectilinearGrid(ocn.GPU(), size=(13, 6, Nz), x=(0, 1), y=(0, 0.5), z=(-1.0, 0.0), topology=(P, P, B), halo=(3, 3, 3))
    model = ocn.NonhydrostaticModel(pg, advection=ocn.WENO(), tracers=("c",), timestepper=timestepper, closure=closure)
    k = np.arange(1, Nz + 1)
    mode = np.cos(np.pi * m * (k - 0.5) / Nz)
    ocn.set(model, **{field: np.broadcast_to(mode, (13, 6, Nz)).copy()})
    dz = 1.0 / Nz
    lam = 2 * (1 - np.cos(np.pi * m / Nz)) / dz ** 2
    return model, mode, dz, lam


@pytest.mark.parametrize("field", ["c", "u"])
@pytest.mark.parametrize("timestepper", ["QuasiAdamsBashforth2", "RungeKutta3"])
def test_cosine_mode_decays_by_the_backward_euler_factor(ocn, timestepper, field):
    """Uniform z, fluid at rest apart from the mode itself, φ = cos(π m (k - ½) / Nz) uniform in x and y, default conditions: the mode is
    an eigenvector of the no-flux second difference with λ_m = 2 (1 - cos(π m / Nz)) / Δz², the explicit part of the closure term
    vanishes (no horizontal gradient, no flux through the boundaries), so after one QAB2 step (Euler: G⁻ does not enter) the interior is
    φ⁰ / (1 + Δt κ λ_m), and after one RK3 step the product of the three stage factors with stage Δt = 8/15, 2/15, 1/3 Δt.
    Diffusion number Δt κ / Δz² = 50; tolerance 10 (1 + Δt κ λ_max) ε, λ_max = 4 / Δz² (the condition number of the stage matrix is at
    most 1 + Δt κ λ_max), relative to max |φ| of the expected field.
    m = 2: the initial condition is the cosine ROUNDED to double, and its rounding error (ε relative to 1) has components on the modes that
    hardly decay (the column mean not at all), so relative to a result damped by the factor F the error is at least about ε / F whatever
    the solver does.  The bound (2010 ε) therefore needs F well above 5e-4: m = 2 has F = 1.3e-1 (QAB2) and 8.1e-3 (RK3).  With m = 5
    (F = 8.8e-5 after the three RK3 stages) the restatement alone, on the CPU, is already off by 1.06e-12 -- the same figure, to every
    digit, as the model on the GPU."""
    kappa = 1.0
    closure = ocn.ScalarDiffusivity(ocn.VerticallyImplicitTimeDiscretization(), ν=kappa, κ=kappa)
    model, mode, dz, lam = _decay_setup(ocn, timestepper, closure, field)
    dt = 50 * dz ** 2 / kappa
    ocn.time_step(model, dt)
    ocn.flush_tendencies(model)
    ocn.sync_device()
    if timestepper == "RungeKutta3":
        factor = 1.0
        for s in (8 / 15, 5 / 12 - 17 / 60, 3 / 4 - 5 / 12):
            factor /= 1 + s * dt * kappa * lam
    else:
        factor = 1 / (1 + dt * kappa * lam)
    got = model.field(field).interior()
    want = np.broadcast_to(mode * factor, got.shape)
    tol = 10 * (1 + dt * kappa * 4 / dz ** 2) * EPS
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"{timestepper} {field}: factor {factor:.6e}, relative error {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol
    for other in "uvwc":
        if other != field:
            assert np.abs(model.field(other).interior()).max() <= tol


def test_explicit_closure_blows_up_at_the_same_step(ocn):
    """the same mode, the same Δt (diffusion number 50) with the ExplicitTimeDiscretization closure: |1 - Δt κ λ_m| = 12 per Euler step for
    the mode itself and up to 199 for the rounding noise on the shortest one"""
    kappa = 1.0
    model, mode, dz, lam = _decay_setup(ocn, "QuasiAdamsBashforth2", ocn.ScalarDiffusivity(ν=kappa, κ=kappa), "c")
    dt = 50 * dz ** 2 / kappa
    for _ in range(4):
        ocn.time_step(model, dt)
    ocn.sync_device()
    c = model.field("c").interior()
    assert (not np.isfinite(c).all()) or np.abs(c).max() > 1e3


# ---- 4. model steps against the composed sequence ---------------------------------------------------------------------------------------------
NU, KAPPA = 1e-2, {"b": 8e-3, "c": 2e-3}
B_FLUX, B_TOP = 3e-6, 2e-5


def _model_grid(ocn):
    """z refined towards the BOTTOM (Δz from 0.019 to 0.13).  The reference keeps the fluxes through the two boundaries explicit, so a Value
    condition is stable only while κ Δt / Δz² of ITS boundary cell stays below about 1, whatever the implicit step does for the interior
    (with the refinement at the top, the total of b alternates in sign and grows twelvefold per step at diffusion number 20 -- in the model
    and in the composed sequence alike).  The Value condition therefore sits on the coarse side (κ Δt / Δz² = 0.33 there), the Flux condition,
    which does not depend on the state, on the fine side, and the diffusion number 20 is that of the finest cell.
    Δx = Δy = 1: the horizontal diffusion stays explicit, and ν Δt / Δx² = 7e-3 at this Δt (on a box as deep as wide it would be 1.2: unstable)."""
    faces = -1.0 + np.linspace(0.0, 1.0, 13) ** 1.6
    return ocn.RectilinearGrid(ocn.GPU(), size=(13, 6, 12), x=(0, 13), y=(0, 6), z=faces, topology=(P, P, B), halo=(3, 3, 3))


def _bcs(ocn):
    return {"b": ocn.FieldBoundaryConditions(top=ocn.ValueBoundaryCondition(B_TOP), bottom=ocn.FluxBoundaryCondition(B_FLUX))}


def _initial(seed=5):
    rng = np.random.default_rng(seed)
    init = {n: 1e-3 * rng.uniform(-1, 1, (13, 6, 13 if n == "w" else 12)) for n in "uvw"}
    init["b"] = 1e-4 * rng.uniform(-1, 1, (13, 6, 12))  # (N² ~ 5e-3: Δt N ~ 0.05, the internal waves are resolved at diffusion number 20)
    init["c"] = rng.uniform(0, 1, (13, 6, 12))
    return init


def _upload(field, a):
    import torch
    field.data.copy_(torch.from_numpy(np.ascontiguousarray(a.T)))


def _add_restated_explicit_part(g, nh, hydrostatic=False):
    """Gⁿ <- Gⁿ - (explicit part of the closure term), by the restatement, where the kernel writes"""
    Gn = nh.timestepper._Gn
    u, v, w = (f.parent() for f in nh.velocities)
    D = dict(zip("uvw", IDN.momentum_explicit_part(g, NU, u, v, w)))
    for name, c in zip(nh.tracer_names, nh.tracers):
        D[name] = IDN.tracer_explicit_part(g, KAPPA[name], c.parent())
    ow = 2  # w's first written face (x and y are Periodic)
    for q, name in enumerate(("u", "v", "w") + tuple(nh.tracer_names)):
        if hydrostatic and name == "w":
            continue
        a = Gn[q].parent()
        k0 = ow - 1 if name == "w" else 0
        psl = (slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny), slice(g.Hz + k0, g.Hz + g.Nz))
        a[psl] = a[psl] - D[name][:, :, k0:]
        _upload(Gn[q], a)


def _restated_implicit_step(g, fields, kappas, dt):
    for f, kappa in zip(fields, kappas):
        _upload(f, IDN.implicit_step(g, f.parent(), f.loc, kappa, dt))


def _composed_update_state(ocn, g, r):
    """update_state!(model): halos and auxiliaries, the closure-free interior tendencies of the existing kernels, the restated explicit
    part, then the boundary contributions -- the order of the reference's sum"""
    from oceananigans_jl_amd import models
    ocn.update_state(r, compute_tendencies=False)
    models.compute_tendencies_(r, boundary_contributions=False)
    _add_restated_explicit_part(g, r)
    models.compute_boundary_tendency_contributions(r)


def _composed_nonhydrostatic_step(ocn, g, r, dt):
    ts, clock = r.timestepper, r.clock
    kappas = [NU] * 3 + [KAPPA[n] for n in r.tracer_names]
    prog = r.prognostic_fields()
    if clock.iteration == 0:
        _composed_update_state(ocn, g, r)
    if isinstance(ts, ocn.RungeKutta3TimeStepper):
        stages = ((ts.g1, None), (ts.g2, ts.z2), (ts.g3, ts.z3))
        for n, (gam, zet) in enumerate(stages):
            stage_dt = dt * gam if zet is None else dt * (gam + zet)
            ocn.rk3_substep(r, dt, gam, zet)
            _restated_implicit_step(g, prog, kappas, stage_dt)
            ocn.calculate_pressure_correction(r, stage_dt)
            ocn.pressure_correct_velocities(r, stage_dt)
            if n < 2:
                ocn.cache_previous_tendencies(r)
            _composed_update_state(ocn, g, r)
    else:
        chi = -0.5 if dt != clock.last_dt else ts.chi
        ocn.ab2_step(r, dt, chi)
        _restated_implicit_step(g, prog, kappas, dt)
        ocn.calculate_pressure_correction(r, dt)
        ocn.pressure_correct_velocities(r, dt)
        ocn.cache_previous_tendencies(r)
        _composed_update_state(ocn, g, r)
    clock.iteration += 1
    clock.last_dt = dt


def _tracer_total(g, a):
    dz = g.dzc[g.Hz:g.Hz + g.Nz].reshape(1, 1, -1)
    inner = a[g.Hx:g.Hx + g.Nx, g.Hy:g.Hy + g.Ny, g.Hz:g.Hz + g.Nz]
    return float((inner * (g.dx * g.dy * dz)).sum()), float((np.abs(inner) * (g.dx * g.dy * dz)).sum())


def _boundary_rate(g, state, name):
    """d/dt of Σ φ ΔV from the fluxes through the two boundaries.  b: the bottom Flux condition enters as + J Az, the top Value condition
    through the explicit diffusive flux at face Nz + 1 computed from the filled halo.  Both tracers: the advective flux (Az w) φᴿ through
    the top face, where w = ∂t η of the linear free surface does not vanish in the hydrostatic model (it is 0 in the nonhydrostatic one)
    and the upwind-biased reconstruction next to the wall is the first-order one: φ[Nz] for w > 0, the halo value otherwise."""
    top = g.Hz + g.Nz
    inner = (slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny))
    a, w = state[name], state["w"]
    Az = g.dx * g.dy
    w_top = w[inner + (top,)]
    rate = -((Az * w_top) * np.where(w_top > 0, a[inner + (top - 1,)], a[inner + (top,)])).sum()
    if name == "b":
        q_top = -(KAPPA["b"] * ((a[inner + (top,)] - a[inner + (top - 1,)]) / g.dzf[top]))
        rate += B_FLUX * Az * g.Nx * g.Ny - (Az * q_top).sum()
    return float(rate)


def _check_totals(g, label, history, dt, chi0, kappa_dt):
    """Each tracer's total changes by the QAB2 combination of the boundary rates (_boundary_rate) of the states the tendencies were computed
    from -- by nothing for c in the nonhydrostatic model.  Tolerance 10 cond(A) ε relative to Σ |φ| ΔV per step, A the tracer's matrix at this Δt."""
    for name in ("b", "c"):
        a, bb, cc = IDN.diagonals(g, False, kappa_dt, KAPPA[name])
        tol = 10 * np.linalg.cond(IDN.dense_matrix(a, bb, cc)) * EPS
        prev_rate = 0.0
        for n in range(len(history) - 1):
            t0, s0 = _tracer_total(g, history[n][name])
            t1, _ = _tracer_total(g, history[n + 1][name])
            chi = -0.5 if n == 0 else chi0
            rate = _boundary_rate(g, history[n], name)
            change = dt * ((1.5 + chi) * rate - (0.5 + chi) * prev_rate)
            prev_rate = rate
            err = abs((t1 - t0) - change) / s0
            print(f"{label} {name} step {n}: total {t0:.12e} -> {t1:.12e}, boundary {change:.3e}, error {err:.3e}, tolerance {tol:.3e}")
            assert err <= tol


@pytest.mark.parametrize("timestepper", ["RungeKutta3", "QuasiAdamsBashforth2"])
def test_nonhydrostatic_model_steps_equal_the_composed_sequence(ocn, timestepper):
    """Five steps at diffusion number Δt max(ν, κ) / min Δz² = 20 on a stretched z with buoyancy, two tracers with their own κ, a Value
    condition at the top and a Flux condition at the bottom of b.  The twin is a model WITHOUT closure stepped through the public stage
    functions, with the two new pieces (explicit part of the closure term, implicit step) done by the restatement on the host: every
    prognostic field and tendency must agree bit for bit (strict math).  Totals: see _check_totals (QAB2 predicts b's change from the boundary rates; with RK3 only the
    conserved tracer c is checked, the stage states not being kept)."""
    pg = _model_grid(ocn)
    closure = ocn.ScalarDiffusivity(ocn.VerticallyImplicitTimeDiscretization(), ν=NU, κ=KAPPA)
    kw = dict(advection=ocn.WENO(), tracers=("b", "c"), timestepper=timestepper, buoyancy=ocn.BuoyancyTracer(), coriolis=ocn.FPlane(f=1e-4))
    m = ocn.NonhydrostaticModel(pg, closure=closure, boundary_conditions=_bcs(ocn), **kw)
    r = ocn.NonhydrostaticModel(pg, closure=None, boundary_conditions=_bcs(ocn), **kw)
    assert not m.fuse_stage_boundaries and not m.defer_final_tendencies
    g = IDN.describe(m.grid)
    init = _initial()
    ocn.set(m, **init)
    ocn.set(r, **init)
    dt = 20 * _dzmin(g) ** 2 / max(NU, max(KAPPA.values()))
    history = [{n: m.field(n).parent() for n in ("b", "c", "w")}]
    for step in range(5):
        ocn.time_step(m, dt)
        _composed_nonhydrostatic_step(ocn, g, r, dt)
        history.append({n: m.field(n).parent() for n in ("b", "c", "w")})
    ocn.sync_device()
    for fm, fr, name in zip(m.prognostic_fields(), r.prognostic_fields(), ("u", "v", "w", "b", "c")):
        a, b = fm.parent(), fr.parent()
        print(f"{timestepper} {name}: max |value| {np.abs(init[name]).max():.3e} -> {np.abs(a).max():.3e}")
        assert np.isfinite(a).all(), name
        assert np.array_equal(a, b), f"{name}: max difference {np.abs(a - b).max():.3e}"
    for Gm_, Gr_ in zip(m.timestepper.Gn, r.timestepper._Gn):
        assert np.array_equal(Gm_.parent(), Gr_.parent())
    assert np.abs(m.u.interior()).max() > 0
    if timestepper == "QuasiAdamsBashforth2":
        _check_totals(g, timestepper, history, dt, m.timestepper.chi, dt)
    else:
        a, bb, cc = IDN.diagonals(g, False, dt * 8 / 15, KAPPA["c"])
        tol = 10 * np.linalg.cond(IDN.dense_matrix(a, bb, cc)) * EPS
        for n in range(5):
            t0, s0 = _tracer_total(g, history[n]["c"])
            t1, _ = _tracer_total(g, history[n + 1]["c"])
            print(f"RK3 c step {n}: error {abs(t1 - t0) / s0:.3e}, tolerance {tol:.3e}")
            assert abs(t1 - t0) <= tol * s0


def _free_surface(ocn):
    """(g = 1e-2: the barotropic substeps Δt / 10 of a step at diffusion number 20 stay below the gravity-wave CFL limit on Δx = 1 / 13)"""
    return ocn.SplitExplicitFreeSurface(substeps=10, gravitational_acceleration=1e-2)


def _composed_hydrostatic_update_state(ocn, g, r):
    from oceananigans_jl_amd import models
    r.update_state(compute_tendencies=False)
    r.compute_tendencies(boundary_contributions=False)
    _add_restated_explicit_part(g, r._nh, hydrostatic=True)
    models.compute_boundary_tendency_contributions(r._nh)


def _composed_hydrostatic_step(ocn, g, r, dt):
    """time_step!(model::HydrostaticFreeSurfaceModel, Δt) with QAB2 and a SplitExplicitFreeSurface, the reference's launch sequence
    (hydrostatic.py time_step, fused = False) with the restatement in place of the two new kernels"""
    L, nh, clock, s = ocn._lib, r._nh, r.clock, 0
    pg = r.grid
    if clock.iteration == 0:
        if not r._initialized:
            L.call("ocn_compute_barotropic_mode", pg.cref, r.u.ptr, r.v.ptr, r.U.data_ptr(), r.V.data_ptr(), s)
            r._initialized = True
        _composed_hydrostatic_update_state(ocn, g, r)
    chi = -0.5 if dt != clock.last_dt else nh.timestepper.chi
    Gn, Gm = nh.timestepper._Gn, nh.timestepper._Gm
    idx = [0, 1] + [3 + n for n in range(len(r.tracers))]
    fields = [r.u, r.v] + list(r.tracers)
    L.call("ocn_ab2_step", pg.cref, len(idx), L.ptr_array([f.ptr for f in fields]), L.ptr_array([Gn[q].ptr for q in idx]),
           L.ptr_array([Gm[q].ptr for q in idx]), L.i32_array([f.loc for f in fields]), float(dt), float(chi), s)
    _restated_implicit_step(g, fields, [NU, NU] + [KAPPA[n] for n in r.tracer_names], dt)
    L.call("ocn_split_explicit_forcing", pg.cref, Gn[0].ptr, Gm[0].ptr, Gn[1].ptr, Gm[1].ptr, float(chi), r._GU.data_ptr(), r._GV.data_ptr(), s)
    r._substep_free_surface(dt, s)
    L.call("ocn_barotropic_split_explicit_corrector", pg.cref, r.u.ptr, r.v.ptr, r.U.data_ptr(), r.V.data_ptr(), r._Ub.data_ptr(),
           r._Vb.data_ptr(), float(pg.Lz), s)
    clock.time += dt
    clock.iteration += 1
    clock.last_dt = dt
    clock.last_stage_dt = dt
    nh.timestepper._Gn, nh.timestepper._Gm = Gm, Gn
    r._Geta, r._Geta_m = r._Geta_m, r._Geta
    _composed_hydrostatic_update_state(ocn, g, r)


def test_hydrostatic_model_steps_equal_the_composed_sequence(ocn):
    """HydrostaticFreeSurfaceModel with SplitExplicitFreeSurface(substeps = 10), QAB2, fused = False by default for such a closure: five
    steps at diffusion number 20 against the twin without closure (see the nonhydrostatic test): u, v, w, η and the tracers bit for bit."""
    pg = _model_grid(ocn)
    closure = ocn.ScalarDiffusivity(ocn.VerticallyImplicitTimeDiscretization(), ν=NU, κ=KAPPA)
    kw = dict(tracers=("b", "c"), buoyancy=ocn.BuoyancyTracer(), coriolis=ocn.FPlane(f=1e-4), tracer_advection=ocn.WENO())
    m = ocn.HydrostaticFreeSurfaceModel(pg, closure=closure, boundary_conditions=_bcs(ocn), free_surface=_free_surface(ocn), **kw)
    r = ocn.HydrostaticFreeSurfaceModel(pg, closure=None, boundary_conditions=_bcs(ocn), free_surface=_free_surface(ocn), fused=False, **kw)
    assert m.fused is False
    g = IDN.describe(m.grid)
    init = _initial(seed=6)
    del init["w"]
    m.set(**init)
    r.set(**init)
    dt = 20 * _dzmin(g) ** 2 / max(NU, max(KAPPA.values()))
    history = [{n: m.field(n).parent() for n in ("b", "c", "w")}]
    for step in range(5):
        m.time_step(dt)
        _composed_hydrostatic_step(ocn, g, r, dt)
        history.append({n: m.field(n).parent() for n in ("b", "c", "w")})
    ocn.sync_device()
    for name in ("u", "v", "w", "b", "c"):
        a, b = m.field(name).parent(), r.field(name).parent()
        print(f"hydrostatic {name}: max |value| after five steps {np.abs(a).max():.3e}")
        assert np.isfinite(a).all(), name
        assert np.array_equal(a, b), f"{name}: max difference {np.abs(a - b).max():.3e}"
    assert np.array_equal(m.eta.cpu().numpy(), r.eta.cpu().numpy())
    assert np.abs(m.u.interior()).max() > 0 and np.abs(m.eta.cpu().numpy()).max() > 0
    _check_totals(g, "hydrostatic", history, dt, m._nh.timestepper.chi, dt)


def test_readme_example_steps_both_models(ocn):
    closure = ocn.ScalarDiffusivity(ocn.VerticallyImplicitTimeDiscretization(), ν=1e-2, κ=1e-3)
    pg = _model_grid(ocn)
    m = ocn.NonhydrostaticModel(pg, advection=ocn.WENO(), tracers=("T",), closure=closure)
    ocn.set(m, T=lambda x, y, z: np.exp(z) + 0 * x + 0 * y)
    ocn.time_step(m, 0.1)
    h = ocn.HydrostaticFreeSurfaceModel(pg, tracers=("T",), closure=closure)
    h.set(T=lambda x, y, z: np.exp(z) + 0 * x + 0 * y)
    h.time_step(0.1)
    ocn.sync_device()
    for f in m.prognostic_fields() + h._nh.prognostic_fields():
        assert np.isfinite(f.interior()).all()


# ---- 5. the fused hosts refuse such a model ---------------------------------------------------------------------------------------------------
def test_drivers_and_fused_steps_refuse_the_closure(ocn):
    closure = ocn.ScalarDiffusivity(ocn.VerticallyImplicitTimeDiscretization(), ν=1e-2, κ=1e-3)
    pg = _model_grid(ocn)
    m = ocn.NonhydrostaticModel(pg, advection=ocn.WENO(), tracers=("T",), closure=closure)
    for driver in (ocn.RK3Driver, ocn.ModelRK3Driver):
        with pytest.raises(NotImplementedError, match="Python host"):
            driver(m)
    with pytest.raises(NotImplementedError, match="fused = False"):
        ocn.HydrostaticFreeSurfaceModel(pg, closure=closure, fused=True, free_surface=ocn.SplitExplicitFreeSurface(substeps=10))
    with pytest.raises(NotImplementedError, match="SplitRungeKutta3"):
        ocn.HydrostaticFreeSurfaceModel(pg, closure=closure, timestepper="SplitRungeKutta3", free_surface=ocn.SplitExplicitFreeSurface(substeps=10))
