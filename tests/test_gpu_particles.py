"""LagrangianParticles on the GPU: the kernel of csrc/particles.hip against its NumPy restatement (tests/particles_numpy.py), bit for bit
(no FMA contraction, the same operand order), and the particles inside NonhydrostaticModel time steps: they are stepped where the
reference steps them, with the velocities it sees there, and they do not change the flow by a bit."""
import numpy as np
import pytest

import particles_numpy as PN

pytestmark = pytest.mark.gpu

P, B, F = "Periodic", "Bounded", "Flat"
STRETCHED = [-1, -0.5, 0.0, 0.4, 0.7, 1]
RTOL = np.sqrt(np.finfo(np.float64).eps)  # the reference's `≈`
TOPOLOGIES = {"PPB": (P, P, B), "PFB": (P, F, B), "BBB": (B, B, B), "PPP": (P, P, P)}
KERNEL_CASES = [(t, z) for t in TOPOLOGIES for z in ("regular", "stretched") if not (z == "stretched" and TOPOLOGIES[t][2] != B)]
SEED = 2024
NP = 257  # one past a 256-thread block


def small_grid(ocn, topo, z="regular", arch="gpu"):
    kw = dict(x=(-1, 1), y=(-1, 1), z=(-1, 1) if z == "regular" else STRETCHED)
    for n, t in zip("xyz", topo):
        if t == F:
            kw[n] = None
    return ocn.RectilinearGrid(ocn.GPU() if arch == "gpu" else None, size=tuple(5 for t in topo if t != F), topology=topo, **kw)


def positions(grid, rng, n=NP):
    """random positions in the domain plus hand-placed ones: 16 each exactly on the left and on the right face of every direction, on
    cell centres, and in the half cell below the first / above the last centre of every direction"""
    lo = [grid.domain(a)[0] if grid.topology[a] != F else -1.0 for a in range(3)]
    hi = [grid.domain(a)[1] if grid.topology[a] != F else 1.0 for a in range(3)]
    X = [rng.uniform(lo[a], hi[a], n) for a in range(3)]
    q = 0
    for a in range(3):
        if grid.topology[a] == F:
            continue
        X[a][q:q + 16] = lo[a]
        X[a][q + 16:q + 32] = hi[a]
        q += 32
    for a in range(3):
        if grid.topology[a] != F:
            c = grid.nodes_1d(a, False)
            X[a][q:q + 16] = c[rng.integers(0, len(c), 16)]
    q += 16
    for a in range(3):
        if grid.topology[a] == F:
            continue
        c = grid.nodes_1d(a, False)
        X[a][q:q + 16] = lo[a] + rng.uniform(0, 1, 16) * (c[0] - lo[a])
        X[a][q + 16:q + 32] = c[-1] + rng.uniform(0, 1, 16) * (hi[a] - c[-1])
        q += 32
    assert q <= n
    return X


def random_fields(ocn, grid, rng):
    """u, v, w and a Center field with random interiors (wall faces included) and filled halos"""
    fields = (ocn.XFaceField(grid), ocn.YFaceField(grid), ocn.ZFaceField(grid), ocn.CenterField(grid))
    for f in fields:
        f.set(rng.uniform(-1, 1, tuple(reversed(f.interior_view().shape))))
    ocn.fill_halo_regions(fields, fill_boundary_normal_velocities=False)
    return fields


def make_particles(ocn, X, n, restitution, fields):
    u, v, w, c = fields
    return ocn.LagrangianParticles(x=X[0][:n].copy(), y=X[1][:n].copy(), z=X[2][:n].copy(), restitution=restitution,
                                   tracked_fields={"u": u, "v": v, "w": w, "c": c}, properties={k: np.zeros(n) for k in "uvwc"})


def host(particles, names=("x", "y", "z")):
    return [particles.properties[k].cpu().numpy() for k in names]


@pytest.mark.parametrize("topo,z", KERNEL_CASES, ids=[f"{t}-{z}" for t, z in KERNEL_CASES])
def test_kernel_equals_the_restatement_bit_for_bit(ocn, topo, z):
    rng = np.random.default_rng(SEED)
    grid = small_grid(ocn, TOPOLOGIES[topo], z)
    geom = PN.Geometry(grid)
    fields = random_fields(ocn, grid, rng)
    parents = [f.parent() for f in fields]
    X = positions(grid, rng)
    dt = 0.3
    # the inputs exercise every wrap / bounce branch: by the restatement alone, before anything is compared
    _, raw = PN.advect(geom, *X, *parents[:3], dt, 1.0, unbounded=True)
    for a, (left, right) in enumerate(PN.crossings(geom, raw)):
        assert grid.topology[a] == F or (left and right), f"no particle crosses both sides of direction {a}"
    for n, Cr in ((NP, 1.0), (NP, 0.5), (1, 1.0), (0, 1.0)):
        x0 = [c[:n] for c in X]
        want_tracked = [PN.interpolate(geom, parents[q], f.loc, *x0) for q, f in enumerate(fields)]
        want = PN.advect(geom, *x0, *parents[:3], dt, Cr)
        got = {}
        for mode in (ocn.MATH_STRICT, ocn.MATH_FAST):
            p = make_particles(ocn, X, n, Cr, fields)
            ocn.advect_lagrangian_particles(p, grid.with_math_mode(mode), fields[:3], dt, update_properties=True)  # ONE launch
            ocn.sync_device()
            got[mode] = host(p, "xyzuvwc")
        for a, b in zip(got[ocn.MATH_STRICT], got[ocn.MATH_FAST]):
            assert np.array_equal(a, b)
        for k, a, b in zip("xyzuvwc", got[ocn.MATH_STRICT], list(want) + want_tracked):
            assert a.shape == (n,) and np.array_equal(a, b), f"{k} differs for n = {n}, restitution {Cr}"
        # the sampling kernel alone gives the same bits and moves nothing
        p = make_particles(ocn, X, n, Cr, fields)
        ocn.update_lagrangian_particle_properties(p, grid)
        ocn.sync_device()
        for k, a, b in zip("xyzuvwc", host(p, "xyzuvwc"), x0 + want_tracked):
            assert np.array_equal(a, b), f"sampling only: {k} differs for n = {n}"


def test_positions_the_reference_would_read_out_of_bounds_stay_inside(ocn):
    """NaN and far-away positions: the clamped indices (checked against the array extents by the restatement) give the restatement's bits"""
    rng = np.random.default_rng(SEED + 1)
    grid = small_grid(ocn, TOPOLOGIES["PPB"], "stretched")
    geom = PN.Geometry(grid)
    fields = random_fields(ocn, grid, rng)
    parents = [f.parent() for f in fields]
    bad = np.array([np.nan, 1e300, -1e300, np.inf, -np.inf, 37.5, -41.25, 0.3])
    ok = np.zeros_like(bad)
    for X in ((bad, ok, ok), (ok, bad, ok), (ok, ok, bad), (bad, bad, bad)):
        p = make_particles(ocn, X, len(bad), 1.0, fields)
        ocn.advect_lagrangian_particles(p, grid, fields[:3], 0.3, update_properties=True)
        ocn.sync_device()
        want = list(PN.advect(geom, *X, *parents[:3], 0.3, 1.0)) + [PN.interpolate(geom, parents[q], f.loc, *X) for q, f in enumerate(fields)]
        for k, a, b in zip("xyzuvwc", host(p, "xyzuvwc"), want):
            assert np.array_equal(a, b, equal_nan=True), k


@pytest.mark.parametrize("z", ["regular", "stretched"])
def test_reference_restitution_case_and_zero_particles(ocn, z):
    """test_lagrangian_particle_tracking.jl:79-98 with prescribed velocities, and :330-345 (0 particles), through the public functions"""
    grid = small_grid(ocn, TOPOLOGIES["PPB"], z)
    Nz = grid.Nz
    z0, top = float(grid.nodes_1d(2, False)[Nz - 2]), float(grid.nodes_1d(2, True)[Nz])
    dt = 0.01
    u, v, w = ocn.XFaceField(grid), ocn.YFaceField(grid), ocn.ZFaceField(grid)
    wi = np.zeros((grid.Nx, grid.Ny, Nz + 1))
    wi[:, :, Nz - 1] = (0.1 + top - z0) / dt
    wi[:, :, Nz - 2] = (0.2 + top - z0) / dt
    w.set(wi)
    ocn.fill_halo_regions((u, v, w), fill_boundary_normal_velocities=False)
    p = ocn.LagrangianParticles(x=np.array([0.0]), y=np.array([0.0]), z=np.array([z0]))
    ocn.advect_lagrangian_particles(p, grid, (u, v, w), dt)
    ocn.sync_device()
    np.testing.assert_allclose(p.z.cpu().numpy(), top - 0.15, rtol=RTOL, atol=0)
    empty = ocn.LagrangianParticles(x=np.zeros(0), y=np.zeros(0), z=np.zeros(0))
    ocn.advect_lagrangian_particles(empty, grid, (u, v, w), dt)
    ocn.update_lagrangian_particle_properties(empty, grid)
    model = ocn.NonhydrostaticModel(grid, advection=ocn.WENO(), particles=empty)
    ocn.time_step(model, 1e-3)
    ocn.sync_device()
    assert isinstance(model.particles, ocn.LagrangianParticles) and len(model.particles) == 0


# ---- inside the model ---------------------------------------------------------------------------------------------------------------
def _model_grid(ocn, name):
    if name == "box":      # the shape that would otherwise take the pressure correction on load
        return ocn.RectilinearGrid(ocn.GPU(), size=(16, 8, 8), x=(-1, 1), y=(-1, 1), z=(-1, 1), topology=(P, P, P))
    topo = (P, P, B) if name == "general" else (B, B, B)
    return ocn.RectilinearGrid(ocn.GPU(), size=(8, 8, 8), x=(-1, 1), y=(-1, 1), z=(-1, 1), topology=topo)


def _build(ocn, name, ts, particles=None):
    kw = dict(advection=ocn.WENO(), timestepper=ts, math_mode=ocn.MATH_STRICT)
    if name == "general":
        kw.update(tracers=("T",), closure=ocn.ScalarDiffusivity(nu=1e-3, kappa=1e-3))
    if particles is not None:
        kw["particles"] = particles
    return ocn.NonhydrostaticModel(_model_grid(ocn, name), **kw)


def _step_twin_unfused(ocn, m, dt, first, record):
    """one time step through the unfused public sequence; the velocities are recorded after every update_state!"""
    ts = m.timestepper
    snap = lambda: record.append([f.parent() for f in m.velocities])
    if first:
        ocn.update_state(m)
    if isinstance(ts, ocn.RungeKutta3TimeStepper):
        for gamma, zeta, cache in ((ts.g1, None, True), (ts.g2, ts.z2, True), (ts.g3, ts.z3, False)):
            stage_dt = (gamma + (zeta or 0.0)) * dt
            ocn.rk3_substep(m, dt, gamma, zeta)
            ocn.calculate_pressure_correction(m, stage_dt)
            ocn.pressure_correct_velocities(m, stage_dt)
            if cache:
                ocn.cache_previous_tendencies(m)
            ocn.update_state(m)
            snap()
    else:
        ocn.ab2_step(m, dt, -0.5 if first else ts.chi)
        ocn.calculate_pressure_correction(m, dt)
        ocn.pressure_correct_velocities(m, dt)
        ocn.cache_previous_tendencies(m)
        ocn.update_state(m)
        snap()


@pytest.mark.parametrize("ts", ["RungeKutta3", "QuasiAdamsBashforth2"])
@pytest.mark.parametrize("name", ["box", "general", "BBB"])
def test_particles_in_the_model_follow_the_reference_sequence(ocn, name, ts):
    rng = np.random.default_rng(SEED + 7)
    n, dt, steps = 64, 0.01, 2
    records = []

    def dynamics(particles, model, stage_dt):
        records.append(dict(dt=stage_dt, pos=host(particles), vel=[f.parent() for f in model.velocities], tracked=host(particles, "s")))

    X = [rng.uniform(-1, 1, n) for _ in range(3)]
    particles = ocn.LagrangianParticles(x=X[0], y=X[1], z=X[2], restitution=0.7, dynamics=dynamics, tracked_fields={"s": "u"},
                                        properties={"s": np.zeros(n)})
    m = _build(ocn, name, ts, particles)
    twin = _build(ocn, name, ts)
    if name == "box" and ts == "RungeKutta3":
        assert twin.correct_on_load and not m.correct_on_load
    assert m.fuse_stage_boundaries == twin.fuse_stage_boundaries
    twin.fuse_stage_boundaries = twin.defer_final_tendencies = twin.correct_on_load = False
    init = {k: rng.uniform(-1, 1, tuple(reversed(f.interior_view().shape))) for k, f in zip("uvw", m.velocities)}
    if name == "general":
        init["T"] = rng.uniform(-1, 1, (8, 8, 8))
    ocn.set(m, **init)
    ocn.set(twin, **init)
    twin_vel = []
    for s in range(steps):
        ocn.time_step(m, dt)
        _step_twin_unfused(ocn, twin, dt, s == 0, twin_vel)
    ocn.sync_device()
    tsr = m.timestepper
    stage_dts = [tsr.g1 * dt, (tsr.g2 + tsr.z2) * dt, (tsr.g3 + tsr.z3) * dt] if ts == "RungeKutta3" else [dt]
    assert [r["dt"] for r in records] == stage_dts * steps
    geom = PN.Geometry(m.grid)
    final = host(m.particles)
    for q, r in enumerate(records):
        # the particles were moved with exactly the velocities the callback saw ...
        nxt = records[q + 1]["pos"] if q + 1 < len(records) else final
        for a, b in zip(PN.advect(geom, *r["pos"], *r["vel"], r["dt"], 0.7), nxt):
            assert np.array_equal(a, b), f"stage {q}"
        # ... the tracked field was sampled before the callback, at the position before the move ...
        assert np.array_equal(r["tracked"][0], PN.interpolate(geom, r["vel"][0], 1, *r["pos"]))
        # ... and those are the velocities after update_state! of the unfused sequence
        for a, b in zip(r["vel"], twin_vel[q]):
            assert np.array_equal(a, b), f"stage {q}: velocities differ from the particle-free unfused twin"
    # particles are passive
    for a, b in zip(m.prognostic_fields(), twin.prognostic_fields()):
        assert np.array_equal(a.parent(), b.parent())


@pytest.mark.parametrize("ts", ["RungeKutta3", "QuasiAdamsBashforth2"])
def test_reference_end_to_end_check_and_checkpoint(ocn, ts, tmp_path):
    """test_lagrangian_particle_tracking.jl:104-278: uniform u = v = 1, ten particles with tracked u, v, w, one step of 1e-2"""
    grid = small_grid(ocn, TOPOLOGIES["PPB"])
    n = 10

    def build():
        p = ocn.LagrangianParticles(x=np.zeros(n), y=np.zeros(n), z=0.5 * np.ones(n), tracked_fields={"u": "u", "v": "v", "w": "w"},
                                    properties={k: np.zeros(n) for k in "uvw"})
        return ocn.NonhydrostaticModel(grid, advection=ocn.WENO(), timestepper=ts, particles=p)
    m = build()
    ocn.set(m, u=1, v=1)
    ocn.time_step(m, 1e-2)
    ocn.sync_device()
    x, y, z, u, v, w = host(m.particles, "xyzuvw")
    for a, value in ((x, 0.01), (y, 0.01), (z, 0.5), (u, 1.0), (v, 1.0)):
        assert a.shape == (n,)
        np.testing.assert_allclose(a, value, rtol=RTOL, atol=0)
    assert np.all(w == 0.0)  # `w .≈ 0` with a relative tolerance only holds for an exact zero
    path = ocn.write_checkpoint(m, str(tmp_path / "particles_checkpoint.npz"))
    saved = host(m.particles, "xyzuvw")
    for a in m.particles.properties.values():
        a.zero_()
    ocn.set_from_checkpoint(m, path)
    for a, b in zip(host(m.particles, "xyzuvw"), saved):
        assert np.array_equal(a, b)
    other = ocn.NonhydrostaticModel(grid, advection=ocn.WENO(), timestepper=ts,
                                    particles=ocn.LagrangianParticles(x=np.zeros(3), y=np.zeros(3), z=np.zeros(3)))
    with pytest.raises(ValueError, match="holds 10 particles, the model has 3"):
        ocn.set_from_checkpoint(other, path)


def test_drivers_refuse_a_model_with_particles(ocn):
    p = ocn.LagrangianParticles(x=np.zeros(4), y=np.zeros(4), z=np.zeros(4))
    m = ocn.NonhydrostaticModel(_model_grid(ocn, "box"), advection=ocn.WENO(), particles=p)
    with pytest.raises(NotImplementedError, match="particles"):
        ocn.RK3Driver(m)
    with pytest.raises(NotImplementedError, match="particles"):
        ocn.ModelRK3Driver(m)
