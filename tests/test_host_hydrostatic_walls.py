"""HydrostaticFreeSurfaceModel on channels (Periodic, Bounded, Bounded) and closed basins (Bounded, Bounded, Bounded), host side: the CPU
restatement tests/hydrostatic_walls_numpy.py against an anchor that shares none of its new code (the periodic oracle on the mirrored
domain), its invariants, and what the product's constructor accepts and refuses (no GPU: the refusals come before any allocation)."""
from types import SimpleNamespace

import numpy as np
import pytest

import hydrostatic_walls_numpy as HW
from helpers import stretched_faces

EPS = np.finfo(np.float64).eps
G_EARTH = 9.80665
SURFACES = {"explicit": {}, "split": dict(split_explicit_substeps=12), "implicit": dict(implicit_free_surface=True)}
TOPOS = {"channel": "PBB", "basin": "BBB"}


def _grid(O, size, topo, Lx=2.0e3, Ly=1.5e3, halo=(3, 3, 3)):
    return O.Grid(size, x=(0, Lx), y=(0, Ly), z=stretched_faces(size[2], 40.0), topology=topo, halo=halo)


def _random_state(og, rng, amplitude=1e-2, tracer=None):
    """random interiors in the shapes of the fields' interiors (N + 1 faces along Bounded directions; the wall faces are reset by set)"""
    bx, by = int(og.tx == 1), int(og.ty == 1)
    N = (og.Nx, og.Ny, og.Nz)
    init = dict(u=amplitude * rng.uniform(-1, 1, (N[0] + bx, N[1], N[2])), v=amplitude * rng.uniform(-1, 1, (N[0], N[1] + by, N[2])),
                eta=amplitude * rng.uniform(-1, 1, N[:2]))
    if tracer:
        init[tracer] = rng.uniform(-1, 1, N)
    return init


# ---- 1. the mirror anchor -----------------------------------------------------------------------------------------------------------
def _mirror(a, axis, parity, face):
    """the even (parity = +1) or odd (-1) extension of the interior array `a` along `axis` onto the periodic domain of twice the length.
    Centres: cells 1 .. N then N .. 1.  Faces (N + 1 of them, both wall faces 0): faces 1 .. N then N + 1 .. 2 N, where face N + 1 + m
    is parity x face N + 1 - m."""
    a = np.moveaxis(a, axis, 0)
    if face:
        N = a.shape[0] - 1
        out = np.concatenate([a[:N + 1], parity * a[1:N][::-1]], axis=0)
    else:
        out = np.concatenate([a, parity * a[::-1]], axis=0)
    return np.moveaxis(out, 0, axis)


@pytest.mark.parametrize("surface", list(SURFACES))
@pytest.mark.parametrize("shape", ["channel", "basin"])
def test_walls_equal_the_mirrored_periodic_domain(oracle, surface, shape):
    """A channel with impenetrable no-flux walls IS the y-even extension on the doubly periodic grid of 2 Ny rows (u, b, η even, v odd), for
    second-order schemes without Coriolis; a basin is that in x as well (u odd, v even there).  The periodic side is oracle/hydrostatic.py,
    untouched by the wall code.  Three steps; rows 1 .. Ny (columns 1 .. Nx) agree to the project's bounds for the same arithmetic with a
    different transform (test_implicit_free_surface_model_matches_oracle): 1e-12 of the maximum for η, 1e-11 for u, v, w, 1e-13 for tracers."""
    from oracle import hydrostatic as Hy
    O = oracle
    Nx, Ny, Nz = 16, 6, 4
    basin = shape == "basin"
    gw = _grid(O, (Nx, Ny, Nz), TOPOS[shape])
    gp = _grid(O, (2 * Nx if basin else Nx, 2 * Ny, Nz), "PPB", Lx=4.0e3 if basin else 2.0e3, Ly=3.0e3)
    assert gp.dx == gw.dx and gp.dy == gw.dy
    rng = np.random.default_rng(7)
    init = _random_state(gw, rng, tracer="b")
    init["v"][:, 0] = init["v"][:, -1] = 0.0
    if basin:
        init["u"][0] = init["u"][-1] = 0.0
    kw = dict(tracers=("b",), momentum_advection="VectorInvariant", tracer_advection="Centered2", closure=(1e-2, 2e-3),
              buoyancy="BuoyancyTracer", **SURFACES[surface])
    walls = HW.HydrostaticFreeSurfaceModel(gw, **kw)
    walls.set(**init)
    mirrored = {}
    for name, a in init.items():
        parity_y = -1 if name == "v" else 1
        m = _mirror(a, 1, parity_y, face=name == "v")
        if basin:
            m = _mirror(m, 0, -1 if name == "u" else 1, face=name == "u")
        elif name == "u":
            pass
        mirrored[name] = m
    periodic = Hy.HydrostaticFreeSurfaceModel(gp, **kw)
    periodic.set(**mirrored)
    dt = 5 * gw.dx / np.sqrt(G_EARTH * 40.0) if surface == "implicit" else (20.0 if surface == "split" else 2.0)
    for _ in range(3):
        walls.time_step(dt)
        periodic.time_step(dt)

    def close(name, got, want, tol):
        assert np.abs(want).max() > 0, name
        err = np.abs(got - want).max() / np.abs(want).max()
        assert err <= tol, (name, err)

    H = (gw.Hx, gw.Hy, gw.Hz)
    bx = int(basin)
    ii, jj = slice(H[0], H[0] + Nx), slice(H[1], H[1] + Ny)
    close("eta", walls.eta[ii, jj], periodic.eta[ii, jj], 1e-12)
    close("u", walls.u[H[0]:H[0] + Nx + bx, jj, H[2]:H[2] + Nz], periodic.u[H[0]:H[0] + Nx + bx, jj, H[2]:H[2] + Nz], 1e-11)
    close("v", walls.v[ii, H[1]:H[1] + Ny + 1, H[2]:H[2] + Nz], periodic.v[ii, H[1]:H[1] + Ny + 1, H[2]:H[2] + Nz], 1e-11)
    close("w", walls.w[ii, jj, H[2]:H[2] + Nz + 1], periodic.w[ii, jj, H[2]:H[2] + Nz + 1], 1e-11)
    close("b", walls.tracers[0][ii, jj, H[2]:H[2] + Nz], periodic.tracers[0][ii, jj, H[2]:H[2] + Nz], 1e-13)


# ---- 2. wall faces, continuity, volume ----------------------------------------------------------------------------------------------
def _physics_model(O, og, surface, momentum="VectorInvariant", seed=3):
    kw = dict(tracers=("T", "S"), momentum_advection=momentum, coriolis_f=1e-4, closure=(1e-2, 2e-3),
              buoyancy=("SeawaterBuoyancy", G_EARTH, 2e-4, 8e-4),
              boundary_conditions={"u": {"top": O.FluxBoundaryCondition(-1e-4)}, "T": {"top": O.FluxBoundaryCondition(5e-5)}}, **SURFACES[surface])
    m = HW.HydrostaticFreeSurfaceModel(og, **kw)
    rng = np.random.default_rng(seed)
    init = _random_state(og, rng)
    N = (og.Nx, og.Ny, og.Nz)
    init["T"], init["S"] = 20 + 1e-2 * rng.uniform(-1, 1, N), 35 + 1e-2 * rng.uniform(-1, 1, N)
    m.set(**init)
    return m


def _wall_faces(og, m):
    faces = [m.v[:, og.Hy, :], m.v[:, og.Hy + og.Ny, :]]
    if og.tx == 1:
        faces += [m.u[og.Hx, :, :], m.u[og.Hx + og.Nx, :, :]]
    return faces


@pytest.mark.parametrize("momentum", ["VectorInvariant", "WENO5"])
@pytest.mark.parametrize("surface", list(SURFACES))
@pytest.mark.parametrize("shape", ["channel", "basin"])
def test_wall_faces_are_exactly_zero_and_w_closes_continuity(oracle, shape, surface, momentum):
    """after set and after every step the wall-normal velocity is 0.0 on the wall faces (not small: the halo fill of update_state!
    writes it), and w at the top face is minus the divergence of the barotropic transport Σₖ Δz (u, v).  The two sides add the same
    4 Nz products per column in a different association (w: level by level, each level divided by Az; the transport: u and v summed
    apart): each is within (Nz + 3) eps of the exact sum of absolute values S, so they differ by at most 2 (Nz + 3) eps S."""
    O = oracle
    og = _grid(O, (9, 6, 4), TOPOS[shape])
    m = _physics_model(O, og, surface, momentum)
    dt = {"explicit": 2.0, "split": 20.0, "implicit": 40.0}[surface]
    Hx, Hy, Hz, Nx, Ny, Nz = og.Hx, og.Hy, og.Hz, og.Nx, og.Ny, og.Nz
    dz = np.asarray(og.dzc[Hz:Hz + Nz])
    for step in range(4):
        if step:
            m.time_step(dt)
        for f in _wall_faces(og, m):
            assert np.all(f == 0.0)
        ue, uw = m.u[Hx + 1:Hx + Nx + 1, Hy:Hy + Ny, Hz:Hz + Nz], m.u[Hx:Hx + Nx, Hy:Hy + Ny, Hz:Hz + Nz]
        vn, vs = m.v[Hx:Hx + Nx, Hy + 1:Hy + Ny + 1, Hz:Hz + Nz], m.v[Hx:Hx + Nx, Hy:Hy + Ny, Hz:Hz + Nz]
        div = ((og.dy * dz * (ue - uw)).sum(2) + (og.dx * dz * (vn - vs)).sum(2)) / (og.dx * og.dy)
        S = ((og.dy * dz * (abs(ue) + abs(uw))).sum(2) + (og.dx * dz * (abs(vn) + abs(vs))).sum(2)) / (og.dx * og.dy)
        w_top = m.w[Hx:Hx + Nx, Hy:Hy + Ny, Hz + Nz]
        assert np.all(np.abs(w_top + div) <= 2 * (Nz + 3) * EPS * S)
        assert np.abs(w_top).max() > 0


@pytest.mark.parametrize("surface", ["explicit", "split"])
@pytest.mark.parametrize("shape", ["channel", "basin"])
def test_volume_is_conserved_to_rounding(oracle, shape, surface):
    """Ση over the interior stays what it was: no volume crosses a wall (the wall faces are 0; the topology-aware differences of the
    substeps ignore them).  Every update of η -- one per step (explicit), one per substep (split-explicit) -- adds increments whose exact
    sum telescopes to 0.  Its computed sum does not, by: the rounding of the Nx Ny additions η += Δη (eps |η| each, eps Σ|η| together); the
    increments themselves, sums of 4 Nz products (Nz + 3 roundings deep) of magnitude at most 2 max|η| in this regime -- asserted below
    from the data, it is a statement about the inputs -- so 2 (Nz + 3) eps Σ|η|; and the pairwise summation that takes the total,
    log2(Nx Ny) eps Σ|η|.  With Nz = 4, Nx Ny = 54: 1 + 14 + 6 = 21 eps Σ|η| per update; the filtered average of the substeps is a convex
    combination of such states (weights normalised to 1 within eps per substep, one more eps Σ|η| each).  Bound: 24 eps Σ|η| x updates."""
    O = oracle
    og = _grid(O, (9, 6, 4), TOPOS[shape])
    m = _physics_model(O, og, surface)
    ii, jj = slice(og.Hx, og.Hx + og.Nx), slice(og.Hy, og.Hy + og.Ny)
    total0, scale = m.eta[ii, jj].sum(), np.abs(m.eta[ii, jj]).sum()
    dt = {"explicit": 2.0, "split": 20.0}[surface]
    updates_per_step = 1 if surface == "explicit" else len(m.weights)
    steps = 3
    for _ in range(steps):
        before = m.eta[ii, jj].copy()
        m.time_step(dt)
        assert np.abs(m.eta[ii, jj] - before).max() <= 2 * np.abs(before).max() * updates_per_step   # the regime the multiple assumes
        scale = max(scale, np.abs(m.eta[ii, jj]).sum())
    drift = abs(m.eta[ii, jj].sum() - total0)
    assert drift <= 24 * EPS * scale * steps * updates_per_step, (drift, 24 * EPS * scale * steps * updates_per_step)
    assert np.abs(m.eta[ii, jj] - before).max() > 0


# ---- 3. rest -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("momentum", ["VectorInvariant", "WENO5"])
@pytest.mark.parametrize("surface", list(SURFACES))
@pytest.mark.parametrize("shape", ["channel", "basin"])
def test_a_resting_stratified_state_stays_at_rest(oracle, shape, surface, momentum):
    """T(z) alone: pHY′ has no horizontal gradient, every horizontal difference is exactly 0, so u, v, w and η stay exactly 0 while T
    diffuses vertically"""
    O = oracle
    og = _grid(O, (8, 6, 5), TOPOS[shape])
    m = HW.HydrostaticFreeSurfaceModel(og, tracers=("T", "S"), momentum_advection=momentum, coriolis_f=1e-4, closure=(1e-2, 2e-3),
                                       buoyancy=("SeawaterBuoyancy", G_EARTH, 2e-4, 8e-4), **SURFACES[surface])
    zc = og.nodes(2, face=False)
    T0 = np.broadcast_to(20 + 0.1 * zc, (og.Nx, og.Ny, og.Nz)).copy()
    m.set(T=T0, S=np.full((og.Nx, og.Ny, og.Nz), 35.0))
    for _ in range(3):
        m.time_step(30.0)
    for f in (m.u, m.v, m.w, m.eta):
        assert np.all(f == 0.0)
    assert np.abs(og.interior_N(m.tracers[0]) - T0).max() > 0


# ---- 3b. without walls the restatement is the periodic oracle ----------------------------------------------------------------------
@pytest.mark.parametrize("size, halo", [((16, 12, 7), (3, 3, 3)), ((67, 6, 3), (4, 5, 3))])
def test_the_restatement_on_a_periodic_grid_is_the_oracle(oracle, size, halo):
    """On (Periodic, Periodic, Bounded) the per-direction restatement functions must return the bits of what oracle/hydrostatic.py itself
    computes with: the GPU entry-point tests on PPB (test_gpu_hydrostatic_walls.py) compare against the restatement, and through this test
    against the oracle.  A split-explicit model two steps in supplies fields with filled halos and both tendency levels."""
    from oracle import hydrostatic as Hy
    O = oracle
    g = _grid(O, size, "PPB", halo=halo)
    m = Hy.HydrostaticFreeSurfaceModel(g, tracers=("T", "S"), momentum_advection="VectorInvariant", coriolis_f=1e-4, closure=(1e-2, 2e-3),
                                       buoyancy=("SeawaterBuoyancy", G_EARTH, 2e-4, 8e-4), split_explicit_substeps=5)
    rng = np.random.default_rng(11)
    init = _random_state(g, rng)
    init["T"], init["S"] = 20 + 1e-2 * rng.uniform(-1, 1, size), 35 + 1e-2 * rng.uniform(-1, 1, size)
    m.set(**init)
    for _ in range(2):
        m.time_step(20.0)
    same = np.testing.assert_array_equal
    # the η fill: NaN halos, so a cell the fill does not reach would show
    e = np.full_like(m.eta, np.nan)
    ii, jj = slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny)
    e[ii, jj] = rng.uniform(-1, 1, (g.Nx, g.Ny))
    mine, m.eta = e.copy(), e
    HW.fill_eta(g, mine)
    m._fill_eta()
    same(mine, m.eta)
    assert np.isfinite(mine).all()
    # w from continuity (the oracle also zeroes the bottom face of the last parent row / column, which has no neighbour)
    w_mine, w_oracle = (np.full_like(m.w, 777.0) for _ in range(2))
    HW.compute_w_from_continuity(g, m.u, m.v, w_mine)
    Hy.compute_w_from_continuity(g, m.u, m.v, w_oracle)
    same(w_mine[:-1, :-1], w_oracle[:-1, :-1])
    # the barotropic mode and the forcing sums, AB2 and Euler coefficients
    same(HW.barotropic_mode(g, m.u), m._barotropic_mode(m.u))
    same(HW.barotropic_mode(g, m.v), m._barotropic_mode(m.v))
    for chi in (0.1, -0.5):
        m._split_explicit_step(20.0, chi)
        same(HW.split_explicit_forcing(g, m.Gn[0], m.Gm[0], chi), m.GU)
        same(HW.split_explicit_forcing(g, m.Gn[1], m.Gm[1], chi), m.GV)
        assert np.abs(m.GU).max() > 0 and np.abs(m.GV).max() > 0
    # the substep iteration
    state = [a.copy() for a in (m.eta[ii, jj], m.U, m.V)]
    dtau, weights = m.frac_dt * 20.0, m.weights
    runs = []
    for iterate, topo in ((HW.iterate_split_explicit, (False, False)), (Hy.iterate_split_explicit, ())):
        s = [a.copy() for a in state] + [np.zeros((g.Nx, g.Ny)) for _ in range(3)]
        iterate(*s, m.GU, m.GV, dtau, weights, G_EARTH, g.Lz, g.dx, g.dy, *topo)
        runs.append(s)
    for a, b in zip(*runs):
        same(a, b)
    assert np.abs(runs[0][3] - state[0]).max() > 0
    # the corrector
    u0, v0 = m.u.copy(), m.v.copy()
    Ub, Vb = HW.barotropic_corrector(g, u0, v0, m.U, m.V)
    m._barotropic_corrector()
    for a, b in ((u0, m.u), (v0, m.v), (Ub, m.Ub), (Vb, m.Vb)):
        same(a, b)


# ---- 4. the product's constructor -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pkg():
    import oceananigans_jl_amd as ocn
    return ocn


class _Stop(Exception):
    pass


def _pgrid(pkg, topo, size=(8, 8, 6), **kw):
    names = tuple({"P": "Periodic", "B": "Bounded", "F": "Flat"}[t] for t in topo)
    return pkg.RectilinearGrid(None, size=size, x=(0, 1), y=(0, 1), z=(-1, 0), topology=names, halo=(3, 3, 3), **kw)


@pytest.fixture
def first_allocation(monkeypatch):
    """the model's first field raises _Stop: a constructor that gets there has accepted its arguments"""
    import oceananigans_jl_amd.fields as fields

    def stop(*a, **k):
        raise _Stop()
    monkeypatch.setattr(fields.Field, "__init__", stop)


@pytest.mark.parametrize("topo", ["PPB", "PBB", "BBB"])
def test_the_default_model_is_accepted_on_the_three_topologies(pkg, first_allocation, topo):
    """HydrostaticFreeSurfaceModel(grid): time_step_hydrostatic_model_works(grid) over topos_3d (test_hydrostatic_free_surface_models.jl:88-90)"""
    with pytest.raises(_Stop):
        pkg.HydrostaticFreeSurfaceModel(_pgrid(pkg, topo))


@pytest.mark.parametrize("topo", ["PBB", "BBB"])
def test_accepted_combinations(pkg, first_allocation, topo):
    g = lambda: _pgrid(pkg, topo)
    HFSM = pkg.HydrostaticFreeSurfaceModel
    surfaces = (lambda: pkg.ImplicitFreeSurface(), lambda: pkg.ExplicitFreeSurface(), lambda: pkg.SplitExplicitFreeSurface(substeps=10),
                lambda: pkg.SplitExplicitFreeSurface(g(), cfl=0.7))
    momenta = (lambda: pkg.VectorInvariant(), lambda: pkg.WENO(), lambda: pkg.UpwindBiased(order=5), lambda: pkg.Centered())
    for fs in surfaces:
        for mom in momenta:
            with pytest.raises(_Stop):
                HFSM(g(), momentum_advection=mom(), free_surface=fs(), tracers=("T", "S"), coriolis=pkg.BetaPlane(f0=1e-4, beta=2e-11),
                     buoyancy=pkg.SeawaterBuoyancy(equation_of_state=pkg.LinearEquationOfState(2e-4, 8e-4)),
                     closure=pkg.ScalarDiffusivity(ν=1e-2, κ=2e-3), fused=False)
    for tracer_scheme in (pkg.WENO(), pkg.UpwindBiased(order=5), pkg.Centered()):
        with pytest.raises(_Stop):
            HFSM(g(), tracer_advection=tracer_scheme, tracers=("b",), buoyancy=pkg.BuoyancyTracer(), coriolis=pkg.FPlane(f=1e-4))
    for mode in (pkg.MATH_STRICT, pkg.MATH_FAST):
        with pytest.raises(_Stop):
            HFSM(g(), math_mode=mode)
    noslip = pkg.FieldBoundaryConditions(south=pkg.ValueBoundaryCondition(0.0), north=pkg.ValueBoundaryCondition(0.0))
    with pytest.raises(_Stop):
        HFSM(g(), boundary_conditions={"u": noslip})


@pytest.mark.parametrize("topo", ["PBB", "BBB"])
def test_refusals_come_before_any_allocation(pkg, monkeypatch, topo):
    import oceananigans_jl_amd.fields as fields

    def no_alloc(*a, **k):
        raise AssertionError("a field was allocated before the refusal")
    monkeypatch.setattr(fields.Field, "__init__", no_alloc)
    g = lambda: _pgrid(pkg, topo)
    HFSM = pkg.HydrostaticFreeSurfaceModel
    split = lambda **kw: pkg.SplitExplicitFreeSurface(substeps=10, **kw)
    vi = pkg.VerticallyImplicitTimeDiscretization()
    refused = [
        (dict(fused=True, free_surface=split()), "fused = True is not implemented"),
        (dict(fused=True, free_surface=pkg.ExplicitFreeSurface()), "fused = True is not implemented"),
        (dict(timestepper="SplitRungeKutta3", free_surface=split()), "SplitRungeKutta3 is not implemented"),
        (dict(free_surface=split(timestepper=pkg.AdamsBashforth3Scheme())), "AdamsBashforth3Scheme substepping is not implemented"),
        (dict(momentum_advection=pkg.WENOVectorInvariant(order=5)), "upwinding VectorInvariant / WENOVectorInvariant is not implemented"),
        (dict(momentum_advection=pkg.VectorInvariant(vorticity_scheme=pkg.WENO())), "upwinding VectorInvariant"),
        (dict(closure=pkg.ScalarDiffusivity(vi, ν=1e-2, κ=1e-3)), "closure must be None or an explicit ScalarDiffusivity"),
        (dict(closure=pkg.ConvectiveAdjustmentVerticalDiffusivity(convective_κz=0.1)), "closure must be None or an explicit ScalarDiffusivity"),
        (dict(closure=pkg.RiBasedVerticalDiffusivity()), "closure must be None or an explicit ScalarDiffusivity"),
        (dict(closure=pkg.HorizontalScalarBiharmonicDiffusivity(ν=1e3)), "closure must be None or an explicit ScalarDiffusivity"),
    ]
    for kw, message in refused:
        with pytest.raises(NotImplementedError, match=message):
            HFSM(g(), **kw)
    slab = g()
    monkeypatch.setattr(slab, "architecture", SimpleNamespace(partition=(2, 1, 1), communicates=False), raising=False)
    with pytest.raises(NotImplementedError, match="slab-partitioned"):
        HFSM(slab)
    with pytest.raises(NotImplementedError, match="Flat directions are not implemented"):
        HFSM(pkg.RectilinearGrid(None, size=(8, 6), x=(0, 1), z=(-1, 0), topology=("Bounded", "Flat", "Bounded"), halo=(3, 3)))
    faces = np.linspace(0, 1, 9) ** 1.3
    with pytest.raises(NotImplementedError, match="stretched in y"):
        HFSM(pkg.RectilinearGrid(None, size=(8, 8, 6), x=(0, 1), y=faces, z=(-1, 0), topology=("Periodic", "Bounded", "Bounded"), halo=(3, 3, 3)))


def test_c_entry_points_name_the_topology_they_need(pkg):
    """the entry points without a Bounded instantiation (blocked, AB3, fused, upwinding) refuse a wall grid by name; the ones with it check
    their pointers next"""
    import ctypes as C
    L = pkg._lib.lib()
    err = lambda: (L.ocn_last_error().decode() if isinstance(L.ocn_last_error(), bytes) else str(L.ocn_last_error()))
    g = _pgrid(pkg, "PBB")
    p, w = C.c_void_p(8), (C.c_double * 2)(0.5, 0.5)   # never dereferenced: every call below is refused
    d = C.c_double
    assert L.ocn_split_explicit_substeps_blocked(g.cref, 2, w, d(1.0), d(9.8), d(1.0), p, p, p, p, p, p, p, p, p, None) != 0
    assert "(Periodic, Periodic, Bounded)" in err()
    assert L.ocn_barotropic_corrector_and_w(g.cref, p, p, p, p, p, p, p, p, p, d(1.0), None) != 0 and "(Periodic, Periodic, Bounded)" in err()
    assert L.ocn_compute_vector_invariant_weno_momentum_tendencies(g.cref, 7, p, p, p, p, p, None, d(9.8), None) != 0
    assert "(Periodic, Periodic, Bounded)" in err()
    assert L.ocn_compute_w_from_continuity(g.cref, None, p, p, None) != 0 and "null field pointer" in err()
    assert L.ocn_split_explicit_substeps(g.cref, 0, w, d(1.0), d(9.8), d(1.0), p, p, p, p, p, p, p, p, None) != 0 and "n >= 1" in err()
    flat = pkg.RectilinearGrid(None, size=(8, 6), x=(0, 1), z=(-1, 0), topology=("Bounded", "Flat", "Bounded"), halo=(3, 3))
    assert L.ocn_compute_w_from_continuity(flat.cref, p, p, p, None) != 0 and "unsupported topology" in err()
