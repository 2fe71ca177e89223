"""ImmersedBoundaryGrid(grid, GridFittedBottom(h)) without a GPU: the materialized bottom height and the masks for both immersed
conditions, the node predicates at all eight locations against the cell-wise definitions, what the grid and the models refuse, the halo
inflation, and the CPU restatement tests/hydrostatic_immersed_numpy.py on its own (flat bottom = oracle/hydrostatic.py bit for bit; no flux
through the bottom)."""
import itertools
import types

import numpy as np
import pytest

import hydrostatic_immersed_numpy as HI

P, B = "Periodic", "Bounded"


@pytest.fixture(scope="module")
def pkg():
    import oceananigans_jl_amd as ocn
    return ocn


def _grid(pkg, size=(6, 5, 4), z=(-4.0, 0.0), halo=(2, 2, 2), topology=(P, P, B)):
    return pkg.RectilinearGrid(None, size=size, x=(0, 6.0), y=(0, 5.0), z=z, topology=topology, halo=halo)


def _bathymetry(Nx, Ny):
    """below the domain everywhere but: exactly at a cell centre, exactly at a face, between the two, above the top (a dry column)"""
    h = np.full((Nx, Ny), -10.0)
    h[1, 1] = -2.5   # the centre of cell 2 (faces -4, -3, -2, -1, 0)
    h[2, 1] = -2.0   # face 3
    h[3, 2] = -2.2   # between the centre of cell 2 and face 3
    h[4, 3] = 1.0    # above the top
    h[0, 0] = -4.0   # exactly the domain's bottom
    h[5, 4] = -0.5   # the centre of the top cell
    return h


# ---- materialization -------------------------------------------------------------------------------------------------------------------
def test_center_condition(pkg):
    g = pkg.ImmersedBoundaryGrid(_grid(pkg), pkg.GridFittedBottom(_bathymetry(6, 5)))
    bh, kb = g.immersed_boundary.bottom_height, g.kbot
    assert isinstance(g.immersed_boundary.immersed_condition, pkg.CenterImmersedCondition)
    # z_centre(k) <= h, with <=: a bottom exactly at the centre of cell 2 immerses cell 2
    assert (kb[1, 1], bh[1, 1]) == (2, -2.0)
    assert (kb[2, 1], bh[2, 1]) == (2, -2.0)
    assert (kb[3, 2], bh[3, 2]) == (2, -2.0)
    assert (kb[4, 3], bh[4, 3]) == (4, 0.0)      # dry
    assert (kb[0, 0], bh[0, 0]) == (0, -4.0)     # at the domain's bottom: nothing is immersed
    assert (kb[5, 4], bh[5, 4]) == (4, 0.0)      # the top cell's centre: dry as well
    assert (kb[0, 1], bh[0, 1]) == (0, -4.0)     # below the domain
    assert kb.dtype == np.int32
    cell = pkg.immersed_cell(g)
    assert cell.shape == (6, 5, 4) and cell.dtype == bool
    zc = g.nodes_1d(2, False)
    np.testing.assert_array_equal(cell, zc[None, None, :] <= bh[:, :, None])
    np.testing.assert_array_equal(cell.sum(axis=2), kb)
    assert g.underlying_grid.Nx == 6 and g.Nx == 6 and g.topology == (P, P, B)   # properties of the underlying grid are the grid's


def test_interface_condition(pkg):
    g = pkg.ImmersedBoundaryGrid(_grid(pkg), pkg.GridFittedBottom(_bathymetry(6, 5), pkg.InterfaceImmersedCondition()))
    bh, kb = g.immersed_boundary.bottom_height, g.kbot
    # z_face(k + 1) <= h
    assert (kb[1, 1], bh[1, 1]) == (1, -3.0)     # h = -2.5: face 2 (-3) is below, face 3 (-2) is not
    assert (kb[2, 1], bh[2, 1]) == (2, -2.0)     # h exactly at face 3: <= holds
    assert (kb[3, 2], bh[3, 2]) == (1, -3.0)
    assert (kb[4, 3], bh[4, 3]) == (4, 0.0)
    assert (kb[0, 0], bh[0, 0]) == (0, -4.0)
    assert (kb[5, 4], bh[5, 4]) == (3, -1.0)


@pytest.mark.parametrize("interface", [False, True])
@pytest.mark.parametrize("stretched", [False, True])
def test_materialization_matches_the_restatement(pkg, oracle, interface, stretched):
    rng = np.random.default_rng(3)
    z = np.array([-4.0, -3.1, -1.9, -0.7, 0.0]) if stretched else (-4.0, 0.0)
    h = rng.uniform(-5.0, 0.5, (6, 5))
    cond = pkg.InterfaceImmersedCondition() if interface else pkg.CenterImmersedCondition()
    g = pkg.ImmersedBoundaryGrid(_grid(pkg, z=z), pkg.GridFittedBottom(h, cond))
    og = oracle.Grid((6, 5, 4), x=(0, 6.0), y=(0, 5.0), z=z, topology="PPB", halo=(2, 2, 2))
    bottom, immersed = HI.materialize(og, h, interface)
    np.testing.assert_array_equal(g.immersed_boundary.bottom_height, bottom)
    np.testing.assert_array_equal(pkg.immersed_cell(g), immersed)
    Bt = HI.Bathymetry(og, h, interface)
    for loc, want in (("cc", Bt.Hcc), ("fc", Bt.Hfc), ("cf", Bt.Hcf)):
        np.testing.assert_array_equal(pkg.static_column_depth(g, loc), want)


def test_bottom_height_forms(pkg):
    u = _grid(pkg)
    a = pkg.ImmersedBoundaryGrid(u, pkg.GridFittedBottom(-2.5))
    assert (a.kbot == 2).all()
    f = pkg.ImmersedBoundaryGrid(u, pkg.GridFittedBottom(lambda x, y: -4.0 + 0.5 * x + 0 * y))
    xc = u.nodes_1d(0, False)
    want = pkg.ImmersedBoundaryGrid(u, pkg.GridFittedBottom(np.repeat((-4.0 + 0.5 * xc)[:, None], 5, axis=1)))
    np.testing.assert_array_equal(f.kbot, want.kbot)
    with pytest.raises(ValueError, match="shape"):
        pkg.ImmersedBoundaryGrid(u, pkg.GridFittedBottom(np.zeros((5, 6))))
    with pytest.raises(TypeError):
        pkg.GridFittedBottom(-1.0, immersed_condition="center")


# ---- predicates ------------------------------------------------------------------------------------------------------------------------
def _cellwise(g, kbot, loc, any_cell, i, j, k):
    """inactive_node / peripheral_node from the cell-wise definitions (Grids/inactive_node.jl:127-155), one node at a time"""
    def cell(a, b, c):
        return c < 1 or c > g.Nz or c <= kbot[(a - 1) % g.Nx, (b - 1) % g.Ny]
    cells = [cell(i - di, j - dj, k - dk) for di in range(1 + (loc & 1)) for dj in range(1 + (loc >> 1 & 1)) for dk in range(1 + (loc >> 2 & 1))]
    return any(cells) if any_cell else all(cells)


@pytest.mark.parametrize("loc", range(8))
def test_predicates_against_the_cellwise_definitions(pkg, loc):
    h = _bathymetry(6, 5)
    h[5, 0] = -1.2   # on the periodic seam in x
    h[2, 4] = -0.9   # ... and in y
    g = pkg.ImmersedBoundaryGrid(_grid(pkg), pkg.GridFittedBottom(h))
    flat = np.zeros_like(g.kbot)
    nk = g.Nz + (1 if loc & 4 else 0)
    got = {"inactive": pkg.inactive_node(g, loc), "peripheral": pkg.peripheral_node(g, loc),
           "immersed_inactive": pkg.immersed_inactive_node(g, loc), "immersed_peripheral": pkg.immersed_peripheral_node(g, loc)}
    for a in got.values():
        assert a.shape == (6, 5, nk) and a.dtype == bool
    for i, j, k in itertools.product(range(1, 7), range(1, 6), range(1, nk + 1)):
        ina, per = _cellwise(g, g.kbot, loc, False, i, j, k), _cellwise(g, g.kbot, loc, True, i, j, k)
        ina0, per0 = _cellwise(g, flat, loc, False, i, j, k), _cellwise(g, flat, loc, True, i, j, k)
        q = (i - 1, j - 1, k - 1)
        assert got["inactive"][q] == ina and got["peripheral"][q] == per, (loc, i, j, k)
        assert got["immersed_inactive"][q] == (ina and not ina0) and got["immersed_peripheral"][q] == (per and not per0), (loc, i, j, k)
    assert got["immersed_peripheral"].any() and not got["immersed_peripheral"].all()


def test_the_restatement_uses_the_same_predicates(pkg, oracle):
    """the brute-force predicates of the CPU restatement (shifted cell arrays) against the product's (comparisons of k with kbot)"""
    h = _bathymetry(6, 5)
    h[5, 0] = -1.2
    g = pkg.ImmersedBoundaryGrid(_grid(pkg), pkg.GridFittedBottom(h))
    og = oracle.Grid((6, 5, 4), x=(0, 6.0), y=(0, 5.0), z=(-4.0, 0.0), topology="PPB", halo=(2, 2, 2))
    Bt = HI.Bathymetry(og, h)
    for loc in range(8):
        nk = 4 + (1 if loc & 4 else 0)
        box = (slice(2, 8), slice(2, 7), slice(2, 2 + nk))
        np.testing.assert_array_equal(Bt.inactive_node(loc)[box], pkg.inactive_node(g, loc))
        np.testing.assert_array_equal(Bt.peripheral_node(loc)[box], pkg.peripheral_node(g, loc))
        np.testing.assert_array_equal(Bt.immersed_inactive_node(loc)[box], pkg.immersed_inactive_node(g, loc))
        np.testing.assert_array_equal(Bt.immersed_peripheral_node(loc)[box], pkg.immersed_peripheral_node(g, loc))


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_the_grid_refuses(pkg):
    u = _grid(pkg)
    with pytest.raises(NotImplementedError, match="PartialCellBottom"):
        pkg.ImmersedBoundaryGrid(u, pkg.PartialCellBottom(-1.0))
    with pytest.raises(NotImplementedError, match="GridFittedBoundary"):
        pkg.ImmersedBoundaryGrid(u, pkg.GridFittedBoundary(np.zeros((6, 5, 4), dtype=bool)))
    with pytest.raises(NotImplementedError, match="active_cells_map"):
        pkg.ImmersedBoundaryGrid(u, pkg.GridFittedBottom(-1.0), active_cells_map=True)
    for topology in ((P, B, B), (B, B, B)):
        with pytest.raises(NotImplementedError, match="walls or a Flat direction"):
            pkg.ImmersedBoundaryGrid(_grid(pkg, topology=topology), pkg.GridFittedBottom(-1.0))
    flat = pkg.RectilinearGrid(None, size=(6, 4), x=(0, 6.0), z=(-4.0, 0.0), topology=(P, "Flat", B), halo=(2, 2))
    with pytest.raises(NotImplementedError, match="walls or a Flat direction"):
        pkg.ImmersedBoundaryGrid(flat, pkg.GridFittedBottom(-1.0))
    dist = _grid(pkg)
    dist.architecture = types.SimpleNamespace(partition=(2, 1, 1))
    with pytest.raises(NotImplementedError, match="Distributed"):
        pkg.ImmersedBoundaryGrid(dist, pkg.GridFittedBottom(-1.0))
    with pytest.raises(NotImplementedError, match="immersed"):
        pkg.FieldBoundaryConditions(immersed=pkg.ValueBoundaryCondition(0.0))


def test_the_models_refuse_before_anything_is_allocated(pkg):
    """(a grid without an architecture holds metadata only: a constructor that got as far as allocating would fail differently)"""
    g = pkg.ImmersedBoundaryGrid(_grid(pkg), pkg.GridFittedBottom(_bathymetry(6, 5)))
    H = lambda **kw: pkg.HydrostaticFreeSurfaceModel(g, **kw)
    with pytest.raises(NotImplementedError, match="HydrostaticFreeSurfaceModel takes"):
        pkg.NonhydrostaticModel(g)
    with pytest.raises(NotImplementedError, match="ImplicitFreeSurface is not implemented"):
        H(free_surface=pkg.ImplicitFreeSurface())
    with pytest.raises(NotImplementedError, match="SplitRungeKutta3 is not implemented"):
        H(free_surface=pkg.SplitExplicitFreeSurface(substeps=6), timestepper="SplitRungeKutta3")
    with pytest.raises(NotImplementedError, match="AdamsBashforth3Scheme"):
        H(free_surface=pkg.SplitExplicitFreeSurface(substeps=6, timestepper=pkg.AdamsBashforth3Scheme()))
    with pytest.raises(NotImplementedError, match="fused = True"):
        H(free_surface=pkg.ExplicitFreeSurface(), fused=True)
    for adv in (pkg.WENO(), pkg.UpwindBiased(order=5), pkg.WENOVectorInvariant(order=5), pkg.Centered()):
        with pytest.raises(NotImplementedError, match="use VectorInvariant"):
            H(free_surface=pkg.ExplicitFreeSurface(), momentum_advection=adv)
    for adv in (pkg.WENO(), pkg.UpwindBiased(order=5)):
        with pytest.raises(NotImplementedError, match="use Centered"):
            H(free_surface=pkg.ExplicitFreeSurface(), tracer_advection=adv, tracers=("c",))
    closures = (pkg.ScalarDiffusivity(pkg.VerticallyImplicitTimeDiscretization(), ν=1e-2, κ=1e-3), pkg.ConvectiveAdjustmentVerticalDiffusivity(),
                pkg.RiBasedVerticalDiffusivity(), pkg.HorizontalScalarBiharmonicDiffusivity(ν=1.0), pkg.CATKEVerticalDiffusivity(),
                pkg.IsopycnalSkewSymmetricDiffusivity(κ_skew=1.0, κ_symmetric=1.0),
                (pkg.ScalarDiffusivity(ν=1e-2), pkg.ScalarDiffusivity(ν=1e-3)))
    for closure in closures:
        with pytest.raises(NotImplementedError, match="closure must be None or an explicit constant ScalarDiffusivity"):
            H(free_surface=pkg.ExplicitFreeSurface(), closure=closure)


def test_reductions_and_operations_refuse(pkg):
    import torch
    g = pkg.ImmersedBoundaryGrid(_grid(pkg), pkg.GridFittedBottom(-2.5))
    c = pkg.Field(0, g, data=torch.zeros(tuple(reversed(g.parent_shape(0))), dtype=torch.float64))
    for operand in (pkg.Average(c, dims=(1, 2)), pkg.Integral(c), c * c):
        with pytest.raises(NotImplementedError, match="ImmersedBoundaryGrid"):
            pkg.ComputedField(operand)


# ---- halo inflation --------------------------------------------------------------------------------------------------------------------
def test_with_halo_carries_the_bathymetry(pkg):
    h = _bathymetry(6, 5)
    for cond in (pkg.CenterImmersedCondition(), pkg.InterfaceImmersedCondition()):
        g = pkg.ImmersedBoundaryGrid(_grid(pkg, halo=(1, 1, 1)), pkg.GridFittedBottom(h, cond))
        w = g.with_halo((3, 2, 2))
        assert isinstance(w, pkg.ImmersedBoundaryGrid) and (w.Hx, w.Hy, w.Hz) == (3, 2, 2) and (g.Hx, g.Hy, g.Hz) == (1, 1, 1)
        np.testing.assert_array_equal(w.kbot, g.kbot)
        np.testing.assert_array_equal(w.immersed_boundary.bottom_height, g.immersed_boundary.bottom_height)
        assert type(w.immersed_boundary.immersed_condition) is type(cond)
        for loc in range(8):
            np.testing.assert_array_equal(pkg.immersed_peripheral_node(w, loc), pkg.immersed_peripheral_node(g, loc))


def test_the_model_inflates_the_halo_by_the_extra_point(pkg, monkeypatch):
    """inflate_halo_size_one_dimension(req_H, old_H, _, ::IBG) = max(req_H + 1, old_H) (immersed_boundary_grid.jl:99-102): VectorInvariant() and
    Centered() need 1, so an immersed grid gets 2 where a plain grid keeps 1; a wider halo is kept"""
    from oceananigans_jl_amd import models
    seen = []

    class Stop(Exception):
        pass

    def clock():
        raise Stop
    monkeypatch.setattr(models, "Clock", clock)   # the first thing the container model builds after it has settled its grid
    real = pkg.ImmersedBoundaryGrid.with_halo
    monkeypatch.setattr(pkg.ImmersedBoundaryGrid, "with_halo", lambda self, halo: seen.append(tuple(halo)) or real(self, halo))
    for halo, want in (((1, 1, 1), [(2, 2, 2)]), ((3, 1, 2), [(3, 2, 2)]), ((2, 2, 2), []), ((4, 5, 3), [])):
        seen.clear()
        g = pkg.ImmersedBoundaryGrid(_grid(pkg, halo=halo), pkg.GridFittedBottom(_bathymetry(6, 5)))
        with pytest.raises(Stop):
            pkg.HydrostaticFreeSurfaceModel(g, free_surface=pkg.ExplicitFreeSurface())
        assert seen == want, (halo, seen)


# ---- the restatement on its own --------------------------------------------------------------------------------------------------------
def _seamount(N, top=-12.0):
    i, j = np.meshgrid(np.arange(N[0]), np.arange(N[1]), indexing="ij")
    return -60.0 + (60.0 + top) * np.exp(-((i - N[0] / 2) ** 2 + (j - N[1] / 2) ** 2) / 6.0)


@pytest.mark.parametrize("substeps", [None, 4])
@pytest.mark.parametrize("closure", [None, (1e-2, 1e-3)])
def test_flat_bottom_restatement_is_the_oracle(oracle, substeps, closure):
    """with h below the domain every predicate is false and the restatement must return the bits of oracle/hydrostatic.py, whose kernels are
    pinned on their own: this ties the NumPy evaluation order of every term to the C oracle's"""
    from oracle import hydrostatic as Hy
    rng = np.random.default_rng(0)
    N = (8, 6, 5)
    og = oracle.Grid(N, x=(0, 80.0), y=(0, 60.0), z=-40.0 + 40.0 * (np.arange(6) / 5) ** 1.5, topology="PPB", halo=(3, 3, 3))
    kw = dict(tracers=("b", "c"), coriolis_f=1e-4, closure=closure, buoyancy="BuoyancyTracer", split_explicit_substeps=substeps)
    a = Hy.HydrostaticFreeSurfaceModel(og, momentum_advection="VectorInvariant", **kw)
    b = HI.HydrostaticFreeSurfaceModel(og, np.full(N[:2], -1e3), **kw)
    init = dict(u=0.1 * rng.uniform(-1, 1, N), v=0.1 * rng.uniform(-1, 1, N), b=1e-3 * rng.uniform(-1, 1, N), c=rng.uniform(0, 1, N),
                eta=0.01 * rng.uniform(-1, 1, N[:2]))
    a.set(**init)
    b.set(**init)
    for _ in range(3):
        a.time_step(0.5)
        b.time_step(0.5)
    for x, y in zip(a.fields, b.fields):
        np.testing.assert_array_equal(og.interior(x), og.interior(y))
    np.testing.assert_array_equal(a.eta, b.eta)
    if substeps:
        np.testing.assert_array_equal(a.U, b.U)
        np.testing.assert_array_equal(a.V, b.V)


def test_the_restatement_keeps_tracer_above_the_bottom(oracle):
    rng = np.random.default_rng(2)
    N = (10, 8, 6)
    og = oracle.Grid(N, x=(0, 100.0), y=(0, 80.0), z=(-60.0, 0.0), topology="PPB", halo=(3, 3, 3))
    h = _seamount(N)
    h[0, :] = 5.0   # a dry row on the seam
    m = HI.HydrostaticFreeSurfaceModel(og, h, tracers=("c",), closure=(0.0, 2.0))
    m.set(c=rng.uniform(0.5, 1.5, N))
    active = ~m.B.immersed
    assert active.any() and (~active).any()
    V = og.dx * og.dy * og.dz
    total = lambda: float((og.interior(m.tracers[0])[active] * V).sum())
    first = total()
    c0 = og.interior(m.tracers[0]).copy()
    for _ in range(20):
        m.time_step(1.0)
    c = og.interior(m.tracers[0])
    assert np.all(c[~active] == 0.0) and np.abs(c - c0)[active].max() > 1e-3
    bound = HI.conservation_bound(20, int(active.sum()), np.abs(c0).max() * V)
    print(f"tracer integral changed by {abs(total() - first):.3e} (bound {bound:.3e})")
    assert abs(total() - first) <= bound
