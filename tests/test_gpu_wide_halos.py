"""The device code at halos wider than 3 and unequal per direction.

Every layer takes Hx, Hy, Hz as run-time numbers, but the rest of the GPU suite runs at (3, 3, 3): a literal 3 where H belongs, or Hx
where Hy or Hz belongs, would pass it.  Here the same comparisons run at

  (4, 4, 4)  the commonest wider choice; an even Hx moves the first interior element of every row to another alignment
  (5, 3, 4)  odd Hx != 3, Hy at the minimum, all three different
  (3, 6, 5)  Hx at the usual value and the others wider: catches Hx used for a y or z offset
  (8, 8, 8)  on 8^3: halo = size, the widest the reference allows (fills and the direct tendency path)

against the CPU oracle on the same-halo grid (tests/test_oracle_wide_halos.py pins the oracle at these halos first).  No tolerance
here is new: a test either states the number of its halo-3 twin or runs the twin's own body.  Where the twin is long (whole models,
drivers, ranks, the newest features) its body is reused as it stands: `at_halo` makes every grid built inside the block -- by
helpers.make_pair, by the twin's own `_grid`, or with a literal halo = (3, 3, 3) -- a halo-H grid, on the oracle's side and the
product's alike, and the twin is then called with one of its own cases."""
import ctypes as C

import numpy as np
import pytest

import operations_cases as OC
import operations_numpy as ON
from helpers import from_dev, make_pair, random_parent, stretched_faces, to_dev

pytestmark = pytest.mark.gpu

LOCS = (1, 2, 4)
SENTINEL = -7.25e300
HALOS = [(4, 4, 4), (5, 3, 4), (3, 6, 5)]
HALOS2 = HALOS[:2]
TWO_PI = 2 * np.pi


def _id(v):
    if isinstance(v, tuple) and all(isinstance(n, (int, np.integer)) for n in v):
        return "x".join(map(str, v))
    return None


# ---------------------------------------------------------------------------------------------------------------------------
# the same test body at another halo
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def at_halo(monkeypatch, oracle, ocn):
    """at_halo(H): from here to the end of the test O.Grid and ocn.RectilinearGrid build halo-H grids whatever halo they are given
    (Flat directions dropped the way each constructor wants them).  Only grids built through these two names are caught.  When the
    test is over, at least one device grid must have been built through ocn.RectilinearGrid -- a twin that got all its grids elsewhere
    would have run at halo 3 and proved nothing -- and every grid seen, the oracle's included, must carry H (0 along Flat)."""
    built, obuilt = [], []

    def install(H):
        real_o, real_p = oracle.Grid, ocn.RectilinearGrid

        def ogrid(size, *a, **kw):
            kw["halo"] = tuple(H)  # three entries: the oracle zeroes the Flat ones itself
            g = real_o(size, *a, **kw)
            obuilt.append(((g.Hx, g.Hy, g.Hz), tuple(0 if t == oracle.FLAT else h for h, t in zip(H, g.topo))))
            return g

        def pgrid(arch, *a, **kw):
            topo = kw.get("topology", ("Periodic", "Periodic", "Bounded"))
            kw["halo"] = tuple(h for h, t in zip(H, topo) if t != "Flat")
            g = real_p(arch, *a, **kw)
            built.append(((g.Hx, g.Hy, g.Hz), tuple(0 if t == "Flat" else h for h, t in zip(H, topo))))
            return g

        monkeypatch.setattr(oracle, "Grid", ogrid)
        monkeypatch.setattr(ocn, "RectilinearGrid", pgrid)

    yield install
    assert built and all(got == want for got, want in built + obuilt), (built, obuilt)


def _pair(O, ocn, size, topo, z, halo, **kw):
    if isinstance(z, str):
        z = stretched_faces(size[2])
    og, pg = make_pair(O, ocn, size, topo, z=z, halo=halo, **kw)
    assert (pg.Hx, pg.Hy, pg.Hz) == (og.Hx, og.Hy, og.Hz) == tuple(0 if t == "F" else h for h, t in zip(halo, topo))
    return og, pg


def _assert_addr32_kernel(ocn, size, halo):
    """the launches with the pressure correction on load of a (Periodic, Periodic, Periodic) model or driver of this size and halo
    go to the 32-bit kernel (momentum_tendencies_pc32): the library says so for the grid (ocn_momentum_tendencies_addr32), and the
    size reaches the tiled launch at all (16 x 8 x 4); a fall-back to the 64-bit or the per-cell kernel would otherwise pass"""
    g = ocn.RectilinearGrid(ocn.GPU(), size=size, x=(0, 1), y=(0, 1), z=(0, 1), topology=("Periodic",) * 3, halo=halo)
    assert (g.Hx, g.Hy, g.Hz) == tuple(halo)
    sel = C.c_int32(-1)
    ocn._lib.call("ocn_momentum_tendencies_addr32", g.cref, C.byref(sel))
    assert sel.value == 1 and size[0] >= 16 and size[1] >= 8 and size[2] >= 4


def _cut(gH, g3, a):
    """the parent of the narrower-halo grid g3 in the middle of a parent of gH"""
    d = (gH.Hx - g3.Hx, gH.Hy - g3.Hy, gH.Hz - g3.Hz)
    return np.asfortranarray(a[d[0]:a.shape[0] - d[0], d[1]:a.shape[1] - d[1], d[2]:a.shape[2] - d[2]])


# ---------------------------------------------------------------------------------------------------------------------------
# a. stencil and stepper kernels, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------
A_GRIDS = [((16, 16, 16), "PPP", (0, TWO_PI)),     # the smallest tiled launch
           ((13, 17, 19), "PPP", (0, 1.0)),        # partial tiles
           ((70, 9, 8), "PPP", (0, 3.0)),          # two x tiles, a 9-row y
           ((16, 12, 10), "PPB", "stretched")]
A_CASES = [g + (h,) for g in A_GRIDS for h in HALOS] + [((24, 16, 1), "PPF", None, h) for h in [(4, 5, 0), (5, 3, 0), (3, 6, 0)]]
TINY = ((8, 8, 8), "PPP", (0, 1.0), (8, 8, 8))


def _device_tendencies(ocn, pg, U, c):
    """Gu, Gv, Gw, Gc as whole parents; every output array starts as SENTINEL"""
    dU = [to_dev(ocn, pg, l, a.copy(order="F")) for l, a in zip(LOCS, U)]  # (copies: the cached inputs are read-only)
    dc = to_dev(ocn, pg, 0, c.copy(order="F"))
    dG = [ocn.Field(l, pg) for l in LOCS + (0,)]
    for f in dG:
        f.data.fill_(SENTINEL)
    ocn._lib.call("ocn_compute_momentum_tendencies", pg.cref, dU[0].ptr, dU[1].ptr, dU[2].ptr, dG[0].ptr, dG[1].ptr, dG[2].ptr, None, 0)
    ocn._lib.call("ocn_compute_tracer_tendency", pg.cref, dU[0].ptr, dU[1].ptr, dU[2].ptr, dc.ptr, dG[3].ptr, None, 0)
    ocn.sync_device()
    return [from_dev(f) for f in dG]


_tendency_inputs = {}


def _tendency_case(O, size, topo, z, halo):
    """random parents (halos included) and the oracle's tendencies over SENTINEL-filled parents: computed once per case, shared by the
    strict and the fast test, read-only"""
    key = (size, topo, str(z), halo)
    if key not in _tendency_inputs:
        rng = np.random.default_rng(1234)
        zz = stretched_faces(size[2]) if isinstance(z, str) else z
        og = O.Grid(size, x=(0, TWO_PI), y=(0, TWO_PI), z=zz, topology=topo, halo=halo)
        U = [random_parent(og, l, rng) for l in LOCS]
        c = random_parent(og, 0, rng, 0.0, 1.0)
        G = [og.zeros(l) for l in LOCS + (0,)]
        for a in G:
            a[...] = SENTINEL
        O.momentum_tendencies(og, *U, *G[:3])
        O.tracer_tendency(og, *U, c, G[3])
        for a in U + [c] + G:
            a.setflags(write=False)
        _tendency_inputs[key] = (U, c, G)
    return _tendency_inputs[key]


@pytest.mark.parametrize("size,topo,z,halo", A_CASES + [TINY], ids=_id)
def test_tendencies_strict_bitwise_and_independent_of_the_halo(oracle, ocn, size, topo, z, halo):
    """ocn_compute_momentum_tendencies and ocn_compute_tracer_tendency of parents that are random everywhere: (1) every parent
    element equals the oracle's on the same-halo grid -- written where the oracle writes, SENTINEL elsewhere; (2) without the
    oracle: the interiors equal the device's own on the halo-3 grid holding the middle of the same parents."""
    O = oracle
    U, c, G = _tendency_case(O, size, topo, z, halo)
    ocn.set_math_mode(ocn.MATH_STRICT)
    ogH, pgH = _pair(O, ocn, size, topo, z, halo)
    got = _device_tendencies(ocn, pgH, U, c)
    for a, b, name in zip(G, got, ("Gu", "Gv", "Gw", "Gc")):
        np.testing.assert_array_equal(b, a, err_msg=f"{name} differs bitwise from the oracle at halo {halo}")
    for a in (G[0], G[1], G[3]):
        assert np.all(ogH.interior_N(a) != SENTINEL) and np.abs(ogH.interior_N(a)).max() > 0
    og3, pg3 = _pair(O, ocn, size, topo, z, tuple(min(3, h) for h in halo))
    got3 = _device_tendencies(ocn, pg3, [_cut(ogH, og3, a) for a in U], _cut(ogH, og3, c))
    for a, b, name in zip(got, got3, ("Gu", "Gv", "Gw", "Gc")):
        np.testing.assert_array_equal(ogH.interior(a), og3.interior(b), err_msg=f"{name}: halo {halo} against halo 3 on the device")


@pytest.mark.parametrize("size,topo,z,halo", A_CASES, ids=_id)
def test_tendencies_fast_tolerance(oracle, ocn, size, topo, z, halo):
    """fast math: within 1e-12 max|G| of the oracle (the bound of test_gpu_kernels.test_momentum_tendencies_fast_tolerance); outside
    the cells the oracle writes nothing is written"""
    O = oracle
    U, c, G = _tendency_case(O, size, topo, z, halo)
    ogH, pgH = _pair(O, ocn, size, topo, z, halo)
    ocn.set_math_mode(ocn.MATH_FAST)
    try:
        got = _device_tendencies(ocn, pgH, U, c)
    finally:
        ocn.set_math_mode(ocn.MATH_STRICT)
    for a, b, name in zip(G, got, ("Gu", "Gv", "Gw", "Gc")):
        written = a != SENTINEL
        np.testing.assert_array_equal(b != SENTINEL, written, err_msg=name)
        scale = max(np.abs(a[written]).max(), 1e-300)
        assert np.abs(b[written] - a[written]).max() <= 1e-12 * scale, name


@pytest.mark.parametrize("size,topo,z,rng_", [g + (None,) for g in A_GRIDS] +
                         [((64, 16, 16), "PPP", (0, 2.0), None), ((63, 8, 5), "PPB", "stretched", None),
                          ((100, 24, 9), "PPB", (-1.0, 0.0), (4, 97, 3, 22, 2, 8))], ids=_id)
@pytest.mark.parametrize("halo", HALOS, ids=_id)
def test_tracer_kernel_ragged_sizes_and_fused_entry(oracle, ocn, at_halo, size, topo, z, rng_, halo):
    """test_gpu_kernels' twin at halo H, on the non-Flat grids of group a and three of the twin's own ragged sizes: the tracer launch
    with and without a range, untouched outside it, and ocn_compute_tracer_tendency_terms_rk3 with diffusion, boundary fluxes and
    the substep folded in (the twin has no Flat case; the plain tracer entry runs on (24, 16, 1) PPF above)"""
    import test_gpu_kernels as TK
    at_halo(halo)
    TK.test_tracer_kernel_ragged_sizes_and_fused_entry(oracle, ocn, size, topo, z, rng_)


@pytest.mark.parametrize("topo,z", [("PPP", (0, 2.0)), ("PPB", "stretched")])
@pytest.mark.parametrize("halo,Ny", [(h, 24) for h in HALOS] + [((3, 6, 5), 70), ((3, 3, 4), 70)], ids=_id)
def test_fused_rk3_entry_and_its_ranges(oracle, ocn, at_halo, topo, z, halo, Ny):
    """ocn_compute_momentum_tendencies_rk3 (tendency + substep in one launch) on (64, Ny, 20): bitwise the oracle's tendency and
    substep, and three ranged launches tile the full one.  The twin's ranges are (4, 61), (1, 3), (62, 64) in x at any halo: from
    Ny = 64 the two 3-wide ones take the 4 x 64 strip kernels of the momentum and the tracer launch (3 columns or fewer, 64 rows or
    more), which carry Hy and Hz offsets -- run here at (3, 6, 5) and (3, 3, 4)"""
    import test_gpu_kernels as TK
    at_halo(halo)
    TK.test_fused_rk3_ranges_tile_the_full_launch(oracle, ocn, topo, z, Ny)


@pytest.mark.parametrize("size,topo,z,halo", A_CASES + [TINY], ids=_id)
def test_halo_fills_bitwise(oracle, ocn, size, topo, z, halo):
    """fill_halo_regions of (u, v, w, c) in one call, both settings of fill_boundary_normal_velocities: every parent element"""
    O = oracle
    rng = np.random.default_rng(7)
    og, pg = _pair(O, ocn, size, topo, z, halo)
    for fbnv in (True, False):
        hosts = [random_parent(og, l, rng) for l in LOCS + (0,)]
        devs = [to_dev(ocn, pg, l, a) for l, a in zip(LOCS + (0,), hosts)]
        for a, l in zip(hosts, LOCS + (0,)):
            O.fill_halo_regions(og, a, l, fill_boundary_normal_velocities=fbnv)
        ocn.fill_halo_regions(devs, fill_boundary_normal_velocities=fbnv)
        ocn.sync_device()
        for a, d, l in zip(hosts, devs, LOCS + (0,)):
            np.testing.assert_array_equal(from_dev(d), a, err_msg=f"loc {l}, halo {halo}")


@pytest.mark.parametrize("size,topo,z,halo", A_CASES + [((10, 9, 8), "PPP", (0, TWO_PI), h) for h in HALOS] + [TINY], ids=_id)
def test_halo_fill_single_direction(oracle, ocn, size, topo, z, halo):
    """ocn_fill_halo_periodic of one Periodic direction touches that direction's halos alone"""
    O = oracle
    rng = np.random.default_rng(8)
    og, pg = _pair(O, ocn, size, topo, z, halo)
    for d in range(3):
        if topo[d] != "P":
            continue
        a = random_parent(og, 0, rng)
        dev = to_dev(ocn, pg, 0, a)
        O.lib().ocn_oracle_fill_periodic(a.ctypes.data_as(O.C.c_void_p), *a.shape, d, size[d], halo[d])
        ocn._lib.call("ocn_fill_halo_periodic", pg.cref, ocn._lib.ptr_array([dev.ptr]), ocn._lib.i32_array([0]), 1, d, 0)
        ocn.sync_device()
        np.testing.assert_array_equal(from_dev(dev), a, err_msg=f"direction {d}")


@pytest.mark.parametrize("size,topo,z,halo", A_CASES, ids=_id)
def test_stepper_kernels_bitwise(oracle, ocn, at_halo, size, topo, z, halo):
    """ocn_rk3_substep (first and later stage), ocn_ab2_step (regular and Euler), ocn_cache_previous_tendencies: whole parents"""
    import test_gpu_kernels as TK
    at_halo(halo)
    TK.test_stepper_kernels_bitwise(oracle, ocn, size, topo, z)


@pytest.mark.parametrize("size,topo,z,halo", A_CASES, ids=_id)
def test_pressure_correct_and_divergence_bitwise(oracle, ocn, at_halo, size, topo, z, halo):
    import test_gpu_kernels as TK
    at_halo(halo)
    TK.test_pressure_correct_and_divergence_bitwise(oracle, ocn, size, topo, z)


# ---------------------------------------------------------------------------------------------------------------------------
# b. grids with walls: the frames of csrc/general.hip around the tiled interior box
# ---------------------------------------------------------------------------------------------------------------------------
B_CASES = [(s, t, h) for s, t in (((41, 29, 9), "BBB"), ((33, 19, 9), "PBP")) for h in HALOS2]


@pytest.mark.parametrize("size,topo,halo", B_CASES, ids=_id)
def test_walls_advective_tendencies_strict_bitwise(oracle, ocn, at_halo, size, topo, halo):
    """momentum and tracer tendencies (the _terms entry points and the plain one) next to x / y walls, whole parents"""
    import test_gpu_general_topologies as TG
    at_halo(halo)
    TG.test_advective_tendencies_strict_bitwise(oracle, ocn, size, topo, "WENO5")


@pytest.mark.parametrize("size,topo,halo", B_CASES, ids=_id)
def test_walls_default_halo_fills(oracle, ocn, at_halo, size, topo, halo):
    import test_gpu_general_topologies as TG
    at_halo(halo)
    TG.test_halo_fills_match_oracle_on_every_parent_cell(oracle, ocn, size, topo)


@pytest.mark.parametrize("size,topo,halo", B_CASES, ids=_id)
def test_walls_value_and_gradient_conditions(oracle, ocn, size, topo, halo):
    """one Value / Gradient condition on every side that has a wall (ocn_fill_halo_regions_bcs): the first halo cell is the
    reference's linear extrapolation, the deeper ones and the Periodic directions follow the oracle, every parent element"""
    O = oracle
    rng = np.random.default_rng(4)
    og, pg = _pair(O, ocn, size, topo, (-0.7, 0.0), halo, x=(0, 1.3), y=(0, 0.9))
    a = random_parent(og, 0, rng)
    d = to_dev(ocn, pg, 0, a)
    sides = {"west": ("gradient", 0.5), "east": ("value", -0.25), "south": ("value", 0.3), "north": ("gradient", -1.7),
             "bottom": ("gradient", 0.125), "top": ("value", 2.0)}
    walls = [s for s, dim in zip(sides, (0, 0, 1, 1, 2, 2)) if topo[dim] == "B"]
    assert len(walls) >= 2
    mk_o = {"value": O.ValueBoundaryCondition, "gradient": O.GradientBoundaryCondition}
    mk_p = {"value": ocn.ValueBoundaryCondition, "gradient": ocn.GradientBoundaryCondition}
    O.fill_halo_regions(og, a, 0, bcs={s: mk_o[sides[s][0]](sides[s][1]) for s in walls})
    d.boundary_conditions = ocn.FieldBoundaryConditions(**{s: mk_p[sides[s][0]](sides[s][1]) for s in walls})
    ocn.fill_halo_regions(d)
    ocn.sync_device()
    np.testing.assert_array_equal(from_dev(d), a)


# ---------------------------------------------------------------------------------------------------------------------------
# c. Poisson solvers
# ---------------------------------------------------------------------------------------------------------------------------
C_GRIDS = [((7, 11, 16), "PPP", (0, 1.0)),          # rocFFT, odd sizes
           ((16, 12, 64), "PPP", (0, 1.0)),         # the fused z column kernel
           ((128, 64, 64), "PPP", (0, 1.0)),        # fully hand-written; rowfft_c2r writes the x halo
           ((128, 64, 12), "PPB", "stretched"),     # row / column kernels plus the Thomas sweep
           ((16, 12, 9), "PPB", "stretched")]


@pytest.mark.parametrize("size,topo,z", C_GRIDS, ids=_id)
@pytest.mark.parametrize("halo", HALOS, ids=_id)
def test_poisson_laplacian_equals_source(oracle, ocn, at_halo, size, topo, z, halo):
    """test_gpu_model's twin with its tolerances and its solver.info()["direct_out"] assertions: ‖∇²ϕ − R‖ ≤ sqrt(eps) ‖R‖, max
    residual 1e-10, ϕ within 1e-10 max(1, max|p|) of the oracle's solve"""
    import test_gpu_model as TM
    at_halo(halo)
    TM.test_poisson_laplacian_equals_source(oracle, ocn, size, topo, z)


@pytest.mark.parametrize("halo", HALOS, ids=_id)
def test_poisson_cosine_transforms(oracle, ocn, at_halo, halo):
    """(Bounded, Bounded, Bounded) 16^3 through FFTBasedPoissonSolver(general=True)"""
    import test_gpu_model as TM
    at_halo(halo)
    TM.test_fft_poisson_all_topologies(oracle, ocn, "BBB", (16, 16, 16))


@pytest.mark.parametrize("halo", HALOS, ids=_id)
def test_custom_pipeline_writes_the_periodic_x_halo_of_the_pressure(oracle, ocn, halo):
    """(128, 64, 64): before any fill_halo_regions(ϕ) the x-halo columns of every interior (j, k) row are that row's periodic images
    bit for bit -- what the drivers' skipped fills rely on -- and no row outside the interior cross-section is written"""
    O = oracle
    size = (128, 64, 64)
    rng = np.random.default_rng(1234)
    og, pg = _pair(O, ocn, size, "PPP", (0, 1.0), halo, x=(0, TWO_PI), y=(0, 3.0))
    hosts = []
    for l in LOCS:
        a = og.zeros(l)
        og.interior(a)[...] = rng.random(og.interior(a).shape)
        O.fill_halo_regions(og, a, l)
        hosts.append(a)
    du, dv, dw = (to_dev(ocn, pg, l, a) for l, a in zip(LOCS, hosts))
    solver = ocn.nonhydrostatic_pressure_solver(pg)
    assert solver.info()["direct_out"] & 2 and solver.info()["direct_out"] & 4
    phi = ocn.CenterField(pg)
    phi.data.fill_(SENTINEL)
    ocn.solve_for_pressure(phi, solver, 1.0, (du, dv, dw))
    ocn.sync_device()
    p = from_dev(phi)
    Hx, Hy, Hz = halo
    rows = p[:, Hy:Hy + size[1], Hz:Hz + size[2]]
    assert np.all(rows != SENTINEL) and np.abs(rows).max() > 0
    np.testing.assert_array_equal(rows[:Hx], rows[size[0]:size[0] + Hx], err_msg="west halo")
    np.testing.assert_array_equal(rows[Hx + size[0]:], rows[Hx:2 * Hx], err_msg="east halo")
    outside = np.ones(p.shape, dtype=bool)
    outside[:, Hy:Hy + size[1], Hz:Hz + size[2]] = False
    assert np.all(p[outside] == SENTINEL)


# ---------------------------------------------------------------------------------------------------------------------------
# d. whole models against the oracle model
# ---------------------------------------------------------------------------------------------------------------------------
D_GRIDS = [((16, 16, 16), "PPP", (0, TWO_PI), "RungeKutta3"),
           ((16, 16, 16), "PPP", (0, TWO_PI), "QuasiAdamsBashforth2"),
           ((128, 64, 64), "PPP", (0, np.pi), "RungeKutta3"),
           ((16, 12, 10), "PPB", "stretched", "RungeKutta3")]


@pytest.mark.parametrize("size,topo,z,ts", D_GRIDS, ids=_id)
@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("halo", HALOS2, ids=_id)
def test_time_steps_match_oracle(oracle, ocn, at_halo, size, topo, z, ts, mode, halo):
    """set! and 3 steps: velocities within 1e-11 (strict) / 1e-10 (fast) of the scale, pressure within 1e-10, max|∇·u| < 5e-8"""
    import test_gpu_model as TM
    at_halo(halo)
    if topo == "PPP":
        _assert_addr32_kernel(ocn, size, halo)
    TM.test_time_steps_match_oracle(oracle, ocn, size, topo, z, ts, mode)


def test_ocean_mixing_model_with_amd_matches_oracle(oracle, ocn, at_halo):
    """config-4 style: AnisotropicMinimumDissipation, T and S, SeawaterBuoyancy, FPlane, wind stress / heat flux / evaporation at the
    top, on (16, 12, 10) stretched, halo (4, 4, 4)"""
    import test_gpu_physics as TP
    at_halo((4, 4, 4))
    TP.test_ocean_wind_mixing_and_convection_matches_oracle(oracle, ocn, "WENO5", "RungeKutta3", "strict")


@pytest.mark.parametrize("fused", [True, False])
def test_hydrostatic_split_explicit_model_matches_oracle(oracle, ocn, at_halo, fused):
    """HydrostaticFreeSurfaceModel, SplitExplicitFreeSurface(substeps = 12), (16, 12, 7) stretched, halo (4, 5, 4): bit for bit"""
    import test_gpu_hydrostatic as TH
    at_halo((4, 5, 4))
    TH.test_split_explicit_free_surface_model_steps_match_oracle(oracle, ocn, fused)


# ---------------------------------------------------------------------------------------------------------------------------
# e. drivers, bit for bit against the Python host
# ---------------------------------------------------------------------------------------------------------------------------
E_CASES = [((32, 16, 12), "PPP", (0, 2.0), False, None),        # default deferral of the third stage's correction
           ((32, 16, 12), "PPP", (0, 2.0), False, False),
           ((128, 64, 64), "PPP", (0, 2.0), True, None),        # own solver handle: the hand-written FFT pipeline
           ((30, 18, 8), "BBB", "stretched", True, None)]       # tiled epilogue on the interior box, finishing kernel on the frames


@pytest.mark.parametrize("size,topo,z,own,defer", E_CASES, ids=_id)
@pytest.mark.parametrize("halo", HALOS2, ids=_id)
def test_rk3_driver_equals_host_orchestration(oracle, ocn, at_halo, size, topo, z, own, defer, halo):
    import test_gpu_model as TM
    at_halo(halo)
    if topo == "PPP":
        _assert_addr32_kernel(ocn, size, halo)
    TM.test_c_driver_equals_host_orchestration(oracle, ocn, size, topo, z, own, defer)


def test_model_rk3_driver_with_amd_equals_python_host(oracle, ocn, at_halo):
    """ModelRK3Driver on (32, 16, 12) PPB stretched with the AMD closure, two tracers, buoyancy, Coriolis and top fluxes, (4, 4, 4)"""
    import test_gpu_physics as TP
    at_halo((4, 4, 4))
    TP._c_model_driver_against_host(ocn, "amd", "PPB")


# ---------------------------------------------------------------------------------------------------------------------------
# f. slab-x ranks (threads of one process over the library's in-process transport) and their pack / unpack kernels
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("halo", HALOS, ids=_id)
def test_two_ranks_match_single_rank(ocn, oracle, at_halo, monkeypatch, halo):
    """R = 2 on (64, 128, 64): local slabs of 32 columns, 32 - 2 Hx >= 1, so the launch splits into interior and Hx-wide buffers; the
    strip epilogue, the Hx + 1 pressure planes and the tupled x pack / unpack all carry Hx.  (3, 6, 5) keeps the buffers 3 wide, the
    width the 4 x 64 strip kernel takes, with Hy and Hz wider.  C driver bitwise the Python host rank by rank, both within
    1e-11 / 1e-10 of the single-rank model"""
    import test_gpu_distributed as TD
    at_halo(halo)
    TD.test_library_transport_ranks_match_single_rank(ocn, 2, (64, 128, 64), "xtri", monkeypatch)


@pytest.mark.parametrize("halo", HALOS, ids=_id)
def test_x_pack_unpack_round_trip(oracle, ocn, halo):
    """ocn_halo_pack_x_fields -> the neighbour's buffers (here: the field's own, x being Periodic) -> ocn_halo_unpack_x_fields equals
    the oracle's periodic fill along x on every parent row of u, v, w, c; one element past each buffer's end is left alone"""
    import torch
    O = oracle
    rng = np.random.default_rng(31)
    og, pg = _pair(O, ocn, (13, 9, 8), "PPP", (0, 1.0), halo)
    locs = LOCS + (0,)
    hosts = [random_parent(og, l, rng) for l in locs]
    devs = [to_dev(ocn, pg, l, a) for l, a in zip(locs, hosts)]
    n = sum(a.shape[1] * a.shape[2] * halo[0] for a in hosts)
    west = torch.full((n + 8,), SENTINEL, dtype=torch.float64, device="cuda")
    east = torch.full((n + 8,), SENTINEL, dtype=torch.float64, device="cuda")
    fp, lp = ocn._lib.ptr_array([f.ptr for f in devs]), ocn._lib.i32_array(list(locs))
    ocn._lib.call("ocn_halo_pack_x_fields", pg.cref, fp, lp, 4, west.data_ptr(), east.data_ptr(), 0)
    ocn._lib.call("ocn_halo_unpack_x_fields", pg.cref, fp, lp, 4, east.data_ptr(), west.data_ptr(), 0)
    ocn.sync_device()
    for buf in (west, east):
        b = buf.cpu().numpy()
        assert np.all(b[n:] == SENTINEL) and np.all(b[:n] != SENTINEL)
    for a, d, l in zip(hosts, devs, locs):
        O.lib().ocn_oracle_fill_periodic(a.ctypes.data_as(O.C.c_void_p), *a.shape, 0, og.Nx, og.Hx)
        np.testing.assert_array_equal(from_dev(d), a, err_msg=f"loc {l}")


@pytest.mark.parametrize("halo", HALOS, ids=_id)
def test_pressure_planes_pack_unpack(oracle, ocn, halo):
    """ocn_halo_pack_pressure / ocn_halo_unpack_pressure against their definition in NumPy: Hx + 1 values per parent row -- Hx pressure
    columns, and to the east the u column nx - Hx + 1 corrected with the pressure of the periodically wrapped interior row"""
    import torch
    O = oracle
    rng = np.random.default_rng(32)
    og, pg = _pair(O, ocn, (13, 9, 8), "PPP", (0, 1.0), halo)
    Hx, Hy, Hz = halo
    nx, W, dt = og.Nx, Hx + 1, 0.37
    p, u = random_parent(og, 0, rng), random_parent(og, 1, rng)
    dp, du = to_dev(ocn, pg, 0, p), to_dev(ocn, pg, 1, u)
    sy, sz = p.shape[1:]
    n = sy * sz * W
    west = torch.full((n + 8,), SENTINEL, dtype=torch.float64, device="cuda")
    east = torch.full((n + 8,), SENTINEL, dtype=torch.float64, device="cuda")
    ocn.set_math_mode(ocn.MATH_STRICT)
    ocn._lib.call("ocn_halo_pack_pressure", pg.cref, dp.ptr, du.ptr, dt, west.data_ptr(), east.data_ptr(), 0)
    ocn.sync_device()
    gw, ge = west.cpu().numpy(), east.cpu().numpy()
    assert np.all(gw[n:] == SENTINEL) and np.all(ge[n:] == SENTINEL)
    J = Hy + (np.arange(sy) - Hy) % og.Ny
    K = Hz + (np.arange(sz) - Hz) % og.Nz
    pw = p[:, J][:, :, K]                                       # p at the wrapped interior row of every parent row
    want_w, want_e = np.zeros((W, sy, sz)), np.zeros((W, sy, sz))
    want_w[:Hx], want_e[:Hx] = p[Hx:2 * Hx], p[nx:nx + Hx]
    want_e[Hx] = u[nx] - ((pw[nx] - pw[nx - 1]) / og.dx) * dt
    np.testing.assert_array_equal(gw[:n].reshape(sz, sy, W).T, want_w)
    np.testing.assert_array_equal(ge[:n].reshape(sz, sy, W).T, want_e)
    # unpack what the neighbours would have sent (x is Periodic: the field's own buffers, crossed over)
    ocn._lib.call("ocn_halo_unpack_pressure", pg.cref, dp.ptr, du.ptr, east.data_ptr(), west.data_ptr(), 0)
    ocn.sync_device()
    p2, u2 = p.copy(order="F"), u.copy(order="F")
    p2[:Hx], p2[nx + Hx:] = want_e[:Hx], want_w[:Hx]
    u2[0] = want_e[Hx]
    np.testing.assert_array_equal(from_dev(dp), p2)
    np.testing.assert_array_equal(from_dev(du), u2)


# ---------------------------------------------------------------------------------------------------------------------------
# g. the newest features
# ---------------------------------------------------------------------------------------------------------------------------
def test_operation_trees_at_a_wide_halo(ocn, at_halo):
    """stretched_70x3x5 of operations_cases rebuilt with halo (4, 3, 5): two pointwise trees bitwise the restatement with nothing
    written outside the interior, and Average(w * u, dims = (1, 2)) within the any-order bound of test_gpu_operations"""
    import test_gpu_operations as TO
    at_halo((4, 3, 5))
    s = TO.Setup(ocn, "stretched_70x3x5")
    assert (s.grid.Hx, s.grid.Hy, s.grid.Hz) == (4, 3, 5)
    cases = OC.pointwise_cases(ocn, s.f)
    for name in ("eta", "zeta"):
        tree, e = cases[name]
        loc, want = ON.pointwise(e, s.leaves, s.g)
        cf = ocn.ComputedField(tree)
        cf.data.fill_(SENTINEL)
        ocn._lib.call("ocn_op_compute", s.grid.cref, C.byref(cf._c), cf.ptr, ocn.architectures.stream_ptr())
        parent = cf.parent()
        sl = TO.interior_slices(cf)
        assert parent[sl].shape == want.shape and np.array_equal(parent[sl], want), name
        outside = np.ones(parent.shape, dtype=bool)
        outside[sl] = False
        assert np.all(parent[outside] == SENTINEL), name
    operand, e = OC.reduction_operands(ocn, s.f)["w*u"]
    cf = ocn.ComputedField(ocn.Average(operand, dims=(1, 2)))
    cf.data.fill_(SENTINEL)
    got = cf.compute().interior()
    _, t, W = ON.reduction_terms("Average", e, (1, 2), s.leaves, s.g)
    exact, n, sabs = ON.reduce_exact(t, (1, 2), W)
    assert got.shape == exact.shape
    assert np.all(np.abs(got - exact) <= ON.reduction_bound(n, sabs, W))


def test_particle_kernel_at_a_wide_halo(ocn, monkeypatch):
    """the particle kernel against particles_numpy on (Periodic, Periodic, Bounded), 7^3 cells (a halo may not exceed the size),
    halo (4, 5, 6)"""
    import test_gpu_particles as TPa

    def grid(ocn_, topo, z="regular", arch="gpu"):
        assert z == "regular" and arch == "gpu"
        return ocn_.RectilinearGrid(ocn_.GPU(), size=(7, 7, 7), x=(-1, 1), y=(-1, 1), z=(-1, 1), topology=topo, halo=(4, 5, 6))

    monkeypatch.setattr(TPa, "small_grid", grid)
    TPa.test_kernel_equals_the_restatement_bit_for_bit(ocn, "PPB", "regular")


def test_stokes_drift_at_a_wide_halo(ocn, oracle, at_halo):
    """(40, 19, 10) PPB stretched, tiled path, Stokes terms after Coriolis + closure + buoyancy, strict: bitwise (G0 + X) + T"""
    import test_gpu_stokes_drift as TS
    at_halo((4, 5, 6))
    TS.test_tendencies_equal_the_unforced_ones_plus_the_stokes_terms(ocn, (40, 19, 10), "PPB", "stretched", True, "strict")


def test_forcing_at_a_wide_halo(ocn, oracle, at_halo):
    """(40, 19, 10) PPB stretched, every kind of forcing term after the other terms, strict: bitwise G0 + F"""
    import test_gpu_forcing as TF
    at_halo((4, 5, 6))
    TF.test_tendencies_equal_the_unforced_ones_plus_F(ocn, (40, 19, 10), "PPB", "stretched", True, "strict")
