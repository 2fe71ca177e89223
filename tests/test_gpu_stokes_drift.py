"""stokes_drift = UniformStokesDrift on the GPU.

The CPU oracle does not know the Stokes terms, and does not need to: they are the LAST terms of the reference's sum
(nonhydrostatic_tendency_kernel_functions.jl:73-74, 135-136, 197-198), so the reference result is (G0 + X) + T with G0 what the same entry
point returns without Stokes drift (pinned to the oracle bit for bit by test_gpu_kernels / test_gpu_physics / test_gpu_general), X the curl
term and T the time derivative, restated below in NumPy in the reference's operand order:
    ℑxzᶠᵃᶜ(w) = 0.5 (ℑx(k) + ℑx(k+1)),  ℑx(k) = 0.5 (w[i-1, k] + w[i, k])        (interpolation_operators.jl:9, 14, 50; a Flat x / y: the value)
    Gu += ℑxzᶠᵃᶜ(w) ∂z_uˢ(zc[k]) + ∂t_uˢ(zc[k]);  Gv likewise with ℑyzᵃᶠᶜ;  Gw += (-ℑxzᶜᵃᶠ(u) ∂z_uˢ(zf[k]) - ℑyzᵃᶜᶠ(v) ∂z_vˢ(zf[k])) + 0
"""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from helpers import from_dev, stretched_faces

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
NAME = {"P": "Periodic", "B": "Bounded", "F": "Flat"}


def _grid(ocn, size, topo, z):
    nonflat = [d for d in range(3) if topo[d] != "F"]
    ext = {"x": (0, 2.0), "y": (0, 3.0), "z": z}
    kw = {n: (None if topo[d] == "F" else ext[n]) for d, n in enumerate("xyz")}
    return ocn.RectilinearGrid(ocn.GPU(), size=tuple(size[d] for d in nonflat), topology=tuple(NAME[t] for t in topo),
                               halo=tuple(3 for _ in nonflat), **kw)


def _random_field(ocn, pg, loc, rng, scale=1.0):
    import torch
    f = ocn.Field(loc, pg)
    f.data.copy_(torch.from_numpy(scale * rng.uniform(-1, 1, tuple(f.data.shape))))
    return f


def _stokes_reference(pg, topo, u, v, w, prof):
    """X + T of the three components on the index ranges the kernels write, as (slices, X, T) per component; u, v, w: parent arrays [i, j, k].
    prof: the six host vectors (element 0 <-> k = 1)."""
    Nx, Ny, Nz, Hx, Hy, Hz = pg.Nx, pg.Ny, pg.Nz, pg.Hx, pg.Hy, pg.Hz
    fx, fy = topo[0] == "F", topo[1] == "F"

    def win(a, i0, i1, j0, j1, k0, k1, di=0, dj=0, dk=0):  # a[i0+di .. i1+di, ...] in 1-based interior indices
        return a[Hx + i0 - 1 + di:Hx + i1 + di, Hy + j0 - 1 + dj:Hy + j1 + dj, Hz + k0 - 1 + dk:Hz + k1 + dk]

    out = []
    # Gu: i from 2 next to a west wall
    r = (2 if topo[0] == "B" else 1, Nx, 1, Ny, 1, Nz)
    ix = lambda dk: win(w, *r, dk=dk) if fx else 0.5 * (win(w, *r, di=-1, dk=dk) + win(w, *r, dk=dk))
    X = (0.5 * (ix(0) + ix(1))) * prof["dz_us_center"][None, None, r[4] - 1:r[5]]
    out.append((r, X, np.broadcast_to(prof["dt_us"][None, None, r[4] - 1:r[5]], X.shape)))
    # Gv: j from 2 next to a south wall
    r = (1, Nx, 2 if topo[1] == "B" else 1, Ny, 1, Nz)
    iy = lambda dk: win(w, *r, dk=dk) if fy else 0.5 * (win(w, *r, dj=-1, dk=dk) + win(w, *r, dk=dk))
    X = (0.5 * (iy(0) + iy(1))) * prof["dz_vs_center"][None, None, r[4] - 1:r[5]]
    out.append((r, X, np.broadcast_to(prof["dt_vs"][None, None, r[4] - 1:r[5]], X.shape)))
    # Gw: k from 2 above the bottom wall
    r = (1, Nx, 1, Ny, 2 if topo[2] == "B" else 1, Nz)
    ixu = lambda dk: win(u, *r, dk=dk) if fx else 0.5 * (win(u, *r, dk=dk) + win(u, *r, di=1, dk=dk))
    iyv = lambda dk: win(v, *r, dk=dk) if fy else 0.5 * (win(v, *r, dk=dk) + win(v, *r, dj=1, dk=dk))
    ui, vi = 0.5 * (ixu(-1) + ixu(0)), 0.5 * (iyv(-1) + iyv(0))
    X = -(ui * prof["dz_us_face"][None, None, r[4] - 1:r[5]]) - vi * prof["dz_vs_face"][None, None, r[4] - 1:r[5]]
    out.append((r, X, np.zeros(X.shape)))
    return out, win


CASES = [((37, 21, 11), "PPP", (-4.0, 0.0)),         # tiled path; not multiples of the 32 x 8 patches
         ((40, 19, 10), "PPB", "stretched"),         # tiled path, stretched z
         ((41, 29, 9), "BBB", "stretched"),          # general path: tiled interior box + wall frames
         ((24, 1, 10), "PFB", (-2.0, 0.0)),          # general path, per-cell kernel on a slice
         ((40, 22, 6), "PBP", (-4.0, 0.0)),          # interior box 40 x 16 (a partial tile in x, two in y) with a Periodic z
         ((13, 19, 5), "PPP", (-4.0, 0.0)),          # narrower than 16: the direct kernel, Periodic z
         ((13, 19, 5), "PPB", "stretched")]          # ... and Bounded z


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("others", [False, True], ids=["stokes_only", "stokes_last_of_many"])
@pytest.mark.parametrize("size,topo,z", CASES, ids=[c[1] + "_" + "x".join(map(str, c[0])) for c in CASES])
def test_tendencies_equal_the_unforced_ones_plus_the_stokes_terms(ocn, size, topo, z, others, mode):
    """Strict: Gu, Gv, Gw bitwise equal to (G0 + X) + T.  Fast: within the per-launch bound 1e-12 max|G| of test_gpu_kernels."""
    import torch
    rng = np.random.default_rng(20261016)
    if isinstance(z, str):
        z = stretched_faces(size[2], 5.0)
    pg = _grid(ocn, size, topo, z)
    ocn.set_math_mode(ocn.MATH_STRICT if mode == "strict" else ocn.MATH_FAST)
    L = ocn._lib
    u, v, w = (_random_field(ocn, pg, loc, rng) for loc in (1, 2, 4))
    b = _random_field(ocn, pg, 0, rng, 1e-2)
    terms = L.CModelTerms()
    terms.advection = L.ADVECTION_WENO5
    if others:  # Coriolis + closure + buoyancy (no separate pHY′: w receives z_dot_g_b)
        terms.coriolis, terms.f = 1, 0.7
        terms.closure, terms.nu = 1, 3e-2
        terms.buoyancy, terms.T = L.BUOYANCY_TRACER, b.ptr
    from oceananigans_jl_amd.stokes import z_nodes, FIELDS
    zc, zf = z_nodes(pg)
    prof = {"dz_us_center": 0.3 * np.exp(zc / 2.0), "dz_us_face": 0.3 * np.exp(zf / 2.0),
            "dz_vs_center": -0.2 * np.exp(zc / 1.5), "dz_vs_face": -0.2 * np.exp(zf / 1.5),
            "dt_us": 0.05 * np.cos(zc), "dt_vs": 0.04 * np.sin(zc)}
    dev = {n: torch.from_numpy(np.ascontiguousarray(prof[n])).cuda() for n in FIELDS}
    sd = L.CStokesDrift(*[dev[n].data_ptr() for n in FIELDS])
    G0 = [ocn.Field(loc, pg) for loc in (1, 2, 4)]
    G1 = [ocn.Field(loc, pg) for loc in (1, 2, 4)]
    L.call("ocn_compute_momentum_tendencies_terms", pg.cref, C.byref(terms), u.ptr, v.ptr, w.ptr, G0[0].ptr, G0[1].ptr, G0[2].ptr, None, 0)
    L.call("ocn_compute_momentum_tendencies_terms_stokes", pg.cref, C.byref(terms), C.byref(sd), u.ptr, v.ptr, w.ptr, G1[0].ptr, G1[1].ptr,
           G1[2].ptr, None, 0)
    ocn.sync_device()
    ref, win = _stokes_reference(pg, topo, from_dev(u), from_dev(v), from_dev(w), prof)
    for (r, X, T), g0, g1, name in zip(ref, G0, G1, "uvw"):
        a0, a1 = from_dev(g0), from_dev(g1)
        expected = a0.copy()
        win(expected, *r)[...] = (win(a0, *r) + X) + T
        scale = np.abs(expected).max()
        err = np.abs(a1 - expected).max()
        print(f"{topo} {size} {mode} others={others} G{name}: max|G| = {scale:.3e}, max|X| = {np.abs(X).max():.3e}, max err = {err:.3e}")
        assert np.abs(X).max() > 0
        if mode == "strict":
            assert a1.tobytes() == expected.tobytes(), f"G{name} differs bitwise from (G0 + X) + T (max err {err:.3e})"
        else:
            assert err <= 1e-12 * scale, f"G{name}: {err:.3e} > 1e-12 * {scale:.3e}"


# ---------------------------------------------------------------------------------------------------------------------------
# closed forms, whole model
# ---------------------------------------------------------------------------------------------------------------------------
def test_constant_w_gives_w_times_the_shear_exactly(ocn):
    """u = v = 0, w = W on a triply periodic grid without other terms: Gu == W ∂z_uˢ(z centre) exactly (the four-point average of a constant
    is exact, the advective tendency of u = 0 is zero)."""
    ocn.set_math_mode(ocn.MATH_STRICT)
    g = ocn.RectilinearGrid(ocn.GPU(), size=(20, 12, 10), x=(0, 1), y=(0, 1), z=(-5, 0), topology=("Periodic",) * 3, halo=(3, 3, 3))
    shear = lambda z, t: 0.01 * np.exp(z / 2.0)
    m = ocn.NonhydrostaticModel(g, advection=ocn.WENO(), stokes_drift=ocn.UniformStokesDrift(dz_us=shear))
    W = 0.375
    ocn.set(m, w=W, enforce_incompressibility=False)
    ocn.update_state(m, compute_tendencies=True)
    ocn.sync_device()
    Gu = m.timestepper.Gn[0].interior()
    expected = np.broadcast_to((W * shear(g.nodes_1d(2, False), 0.0))[None, None, :], Gu.shape)
    assert np.array_equal(np.asarray(Gu), expected)
    assert np.all(np.asarray(m.timestepper.Gn[1].interior()) == 0) and np.all(np.asarray(m.timestepper.Gn[2].interior()) == 0)


def test_a_state_at_rest_stays_at_rest(ocn):
    """FPlane + Stokes drift without ∂t terms: the Lagrangian-mean formulation has no source for a fluid at rest -- exactly zero after 10 steps"""
    ocn.set_math_mode(ocn.MATH_STRICT)
    g = ocn.RectilinearGrid(ocn.GPU(), size=(32, 16, 12), x=(0, 64), y=(0, 64), z=(-32, 0), topology=("Periodic", "Periodic", "Bounded"))
    m = ocn.NonhydrostaticModel(g, advection=ocn.WENO(), coriolis=ocn.FPlane(f=1e-4),
                                stokes_drift=ocn.UniformStokesDrift(dz_us=lambda z, t: 0.02 * np.exp(z / 5.0), dz_vs=lambda z, t: 0.01 * np.exp(z / 3.0)))
    for _ in range(10):
        ocn.time_step(m, 5.0)
    ocn.flush_tendencies(m)
    ocn.sync_device()
    for f in m.velocities:
        assert np.all(np.asarray(f.interior()) == 0.0)


G1, G2, G3, Z2, Z3 = 8 / 15, 5 / 12, 3 / 4, -17 / 60, -5 / 12


def _numpy_rk3(a, b, dt, nsteps, shift=0):
    """du/dt = a + b t with the model's RK3 (runge_kutta_3.jl:77-151); shift = 1: every tendency evaluated one stage late in time (the stage
    time a broken time plumbing would pass)"""
    u, t = np.zeros_like(a), 0.0
    times = lambda t: (t, t + G1 * dt, t + (G1 + G2 + Z2) * dt)
    prev_last = 0.0
    for _ in range(nsteps):
        t1, t2, t3 = times(t)
        if shift:
            t1, t2, t3 = prev_last, t1, t2
        Ga = a + b * t1
        u = u + dt * G1 * Ga
        Gb = a + b * t2
        u = u + dt * (G2 * Gb + Z2 * Ga)
        Gc = a + b * t3
        u = u + dt * (G3 * Gc + Z3 * Gb)
        prev_last = times(t)[2]
        t += dt
    return u


@pytest.mark.parametrize("stepper,with_b", [("RungeKutta3", True), ("QuasiAdamsBashforth2", False)])
def test_time_dependent_profile_is_sampled_at_the_stage_times(ocn, stepper, with_b):
    """u = v = w = 0, ∂t_uˢ(z, t) = a(z) + b(z) t and nothing else: u(z) stays horizontally uniform (divergence-free), so after 10 steps
    u = a t + b t² / 2 -- RK3 integrates a right-hand side linear in t exactly (QAB2: only b = 0).  Bound: rounding alone,
    16 eps n_stages max|u| with n_stages = 30.  A stage time off by one stage misses by O(b Δt²): checked below (NumPy) to be >= 1e6 bounds."""
    ocn.set_math_mode(ocn.MATH_STRICT)
    g = ocn.RectilinearGrid(ocn.GPU(), size=(16, 8, 12), x=(0, 10), y=(0, 10), z=(-30, 0), topology=("Periodic",) * 3, halo=(3, 3, 3))
    a = lambda z: 1e-3 * np.exp(z / 10.0)
    b = (lambda z: 2e-5 * np.exp(z / 7.0)) if with_b else (lambda z: 0.0 * z)
    dt, n = 3.0, 10
    zc = g.nodes_1d(2, False)
    t_end = n * dt
    exact = a(zc) * t_end + b(zc) * t_end ** 2 / 2
    bound = 16 * EPS * 30 * np.abs(exact).max()
    if with_b:  # the test's own power: a one-stage shift of the sampling time must be far outside the bound
        assert np.abs(_numpy_rk3(a(zc), b(zc), dt, n) - exact).max() <= bound
        assert np.abs(_numpy_rk3(a(zc), b(zc), dt, n, shift=1) - exact).max() >= 1e6 * bound
    sd = ocn.UniformStokesDrift(dt_us=lambda z, t: a(z) + b(z) * t)
    assert not sd.steady
    m = ocn.NonhydrostaticModel(g, advection=ocn.WENO(), timestepper=stepper, stokes_drift=sd)
    for _ in range(n):
        ocn.time_step(m, dt)
    ocn.flush_tendencies(m)
    ocn.sync_device()
    u = np.asarray(m.u.interior())
    err = np.abs(u - exact[None, None, :]).max()
    print(f"{stepper}: max|u| = {np.abs(u).max():.6e}, max|u - exact| = {err:.3e}, bound = {bound:.3e}")
    assert err <= bound, f"{stepper}: |u - (a t + b t²/2)| = {err:.3e} > {bound:.3e}"
    assert np.all(np.asarray(m.v.interior()) == 0) and np.all(np.asarray(m.w.interior()) == 0)


# ---------------------------------------------------------------------------------------------------------------------------
# ModelRK3Driver
# ---------------------------------------------------------------------------------------------------------------------------
def _langmuir(ocn, steady=True):
    g = ocn.RectilinearGrid(ocn.GPU(), size=(32, 32, 32), x=(0, 128), y=(0, 128), z=(-64, 0), topology=("Periodic", "Periodic", "Bounded"))
    shear = (lambda z, t: 0.0681 / 4.77 * np.exp(z / 4.77)) if steady else (lambda z, t: 0.0681 / 4.77 * np.exp(z / 4.77) * (1 + 1e-3 * t))
    bcs = {"u": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(-3.72e-5)),
           "b": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(2.307e-8), bottom=ocn.GradientBoundaryCondition(1.936e-5))}
    return ocn.NonhydrostaticModel(g, coriolis=ocn.FPlane(f=1e-4), advection=ocn.WENO(), tracers=("b",), buoyancy=ocn.BuoyancyTracer(),
                                   closure=ocn.AnisotropicMinimumDissipation(), boundary_conditions=bcs,
                                   stokes_drift=ocn.UniformStokesDrift(dz_us=shear, steady=True if steady else None))


def _closed_box(ocn):
    g = ocn.RectilinearGrid(ocn.GPU(), size=(64, 64, 9), x=(0, 64), y=(0, 64), z=stretched_faces(9, 32.0), topology=("Bounded",) * 3)
    return ocn.NonhydrostaticModel(g, advection=ocn.WENO(), tracers=("b",), buoyancy=ocn.BuoyancyTracer(), coriolis=ocn.FPlane(f=1e-4),
                                   closure=ocn.ScalarDiffusivity(ν=1e-3, κ=2e-3),
                                   stokes_drift=ocn.UniformStokesDrift(dz_us=lambda z, t: 5e-3 * np.exp(z / 6.0), dz_vs=lambda z, t: 2e-3 * np.exp(z / 9.0),
                                                                       dt_us=lambda z, t: 1e-6 * np.exp(z / 6.0), steady=True))


@pytest.mark.parametrize("build", [_langmuir, _closed_box], ids=["langmuir_32", "closed_box"])
def test_model_driver_with_a_steady_drift_equals_the_python_host(ocn, build):
    """5 steps behind ocn_model_driver_time_step == 5 x time_step(model, dt), bit for bit (strict math)"""
    ocn.set_math_mode(ocn.MATH_STRICT)
    rng = np.random.default_rng(7)
    models = [build(ocn), build(ocn)]
    g = models[0].grid
    walls = g.topology[0] == "Bounded"
    init = {"u": 1e-2 * rng.uniform(-1, 1, (g.Nx + walls, g.Ny, g.Nz)), "v": 1e-2 * rng.uniform(-1, 1, (g.Nx, g.Ny + walls, g.Nz)),
            "b": 1e-4 * rng.uniform(-1, 1, (g.Nx, g.Ny, g.Nz))}
    for m in models:
        ocn.set(m, **init)
    ref, m = models
    for _ in range(5):
        ocn.time_step(ref, 2.0)
    Gref = [f.parent() for f in ref.timestepper.Gn]
    drv = ocn.ModelRK3Driver(m)
    for _ in range(5):
        drv.time_step(2.0)
    drv.flush()
    ocn.sync_device()
    assert m.clock.time == ref.clock.time and m.clock.iteration == 5
    for name, fa, fb in zip(("u", "v", "w", "b"), ref.prognostic_fields(), m.prognostic_fields()):
        assert np.abs(fa.parent()).max() > 0 or name == "w"
        assert fa.parent().tobytes() == fb.parent().tobytes(), f"{name} differs between the driver and the Python host"
    for name, Ga, fb in zip(("Gu", "Gv", "Gw", "Gb"), Gref, m.timestepper.Gn):
        assert np.asarray(Ga).tobytes() == fb.parent().tobytes(), f"{name} differs"


def test_model_driver_refuses_a_time_dependent_drift(ocn):
    m = _langmuir(ocn, steady=False)
    with pytest.raises(NotImplementedError, match="Python host"):
        ocn.ModelRK3Driver(m)
    # ... and so does the C entry point itself
    ok = _langmuir(ocn)
    drv = ocn.ModelRK3Driver(ok)
    with pytest.raises(ocn.OcnError, match="Python host"):
        ocn._lib.call("ocn_model_driver_set_stokes_drift", drv._h, C.byref(ok._stokes.c), 1)


# ---------------------------------------------------------------------------------------------------------------------------
# the example
# ---------------------------------------------------------------------------------------------------------------------------
def test_langmuir_example_runs_20_steps(ocn):
    spec = importlib.util.spec_from_file_location("langmuir_turbulence_example", os.path.join(ROOT, "examples", "langmuir_turbulence.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    try:
        model, dt = mod.main(["--max-steps", "20"])
    finally:
        ocn.set_math_mode(ocn.MATH_STRICT)
    assert model.clock.iteration == 20
    assert not ocn.hasnan(model) and not any(ocn.hasnan(f) for f in model.prognostic_fields())
    assert np.isfinite(dt) and dt > 0
    assert float(model.w.data.abs().max()) > 0
