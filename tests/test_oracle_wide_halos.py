"""The CPU oracle at halos wider than 3 and unequal per direction, pinned before tests/test_gpu_wide_halos.py leans on it.

Nothing the oracle computes over the interior may depend on how wide the halo is, as long as the halo holds the same numbers: a
halo-H parent that is random everywhere and the halo-3 parent cut out of its middle must give bit-identical interiors for the
tendencies, the divergence, the Laplacian and both Poisson solvers.  The periodic halo fill is checked against plain modular
indexing, up to the widest halo the reference allows (halo = size).

(`ndarray.copy()` of an F-ordered parent returns C order, which the C library would read as garbage: every cut goes through
np.asfortranarray.)"""
import numpy as np
import pytest

from helpers import random_parent, stretched_faces

LOCS = (1, 2, 4)
HALOS = [(4, 4, 4), (5, 3, 4), (3, 6, 5), (4, 5, 6), (6, 3, 4), (5, 7, 3)]
GRIDS = [((13, 17, 19), "PPP", (0, 1.0)),
         ((16, 12, 10), "PPB", "stretched"),
         ((12, 9, 10), "BBB", (-0.7, 0.0)),
         ((24, 16, 1), "PPF", None)]
CASES = [g + (h,) for g in GRIDS for h in HALOS] + [((8, 8, 8), "PPP", (0, 1.0), (8, 8, 8))]


def _grids(O, size, topo, z, halo):
    """the halo-H grid and the halo-min(3, H) grid of the same domain"""
    if isinstance(z, str):
        z = stretched_faces(size[2])
    kw = dict(x=(0, 1.3), y=(0, 0.9), z=z, topology=topo)
    return O.Grid(size, halo=halo, **kw), O.Grid(size, halo=tuple(min(3, h) for h in halo), **kw)


def _cut(gH, g3, a):
    """the halo-3 parent in the middle of a halo-H parent (a Flat direction has no halo on either grid)"""
    d = (gH.Hx - g3.Hx, gH.Hy - g3.Hy, gH.Hz - g3.Hz)
    return np.asfortranarray(a[d[0]:a.shape[0] - d[0], d[1]:a.shape[1] - d[1], d[2]:a.shape[2] - d[2]])


@pytest.mark.parametrize("size,topo,z,halo", CASES)
def test_interiors_do_not_depend_on_the_halo_width(oracle, size, topo, z, halo):
    O = oracle
    rng = np.random.default_rng(2024)
    gH, g3 = _grids(O, size, topo, z, halo)
    u, v, w = (random_parent(gH, l, rng) for l in LOCS)
    c = random_parent(gH, 0, rng, 0.0, 1.0)
    if topo[2] == "F":
        w[...] = 0
    u3, v3, w3, c3 = (_cut(gH, g3, a) for a in (u, v, w, c))
    assert u3.shape == g3.shape(1) and w3.shape == g3.shape(4) and u3.flags.f_contiguous
    G, G3 = [gH.zeros(l) for l in LOCS + (0,)], [g3.zeros(l) for l in LOCS + (0,)]
    O.momentum_tendencies(gH, u, v, w, *G[:3])
    O.momentum_tendencies(g3, u3, v3, w3, *G3[:3])
    O.tracer_tendency(gH, u, v, w, c, G[3])
    O.tracer_tendency(g3, u3, v3, w3, c3, G3[3])
    for a, b, name in zip(G, G3, ("Gu", "Gv", "Gw", "Gc")):
        np.testing.assert_array_equal(gH.interior(a), g3.interior(b), err_msg=name)
        assert not np.any(_cut(gH, g3, a) != b), name  # and nothing is written outside the interior on either grid
    assert all(np.abs(a).max() > 0 for a in (G[0], G[1], G[3]))
    np.testing.assert_array_equal(O.divergence(gH, u, v, w), O.divergence(g3, u3, v3, w3))
    np.testing.assert_array_equal(O.laplacian(gH, c), O.laplacian(g3, c3))


@pytest.mark.parametrize("size,topo,z,halo", CASES)
def test_poisson_solves_do_not_depend_on_the_halo_width(oracle, size, topo, z, halo):
    """velocities with filled halos (what calculate_pressure_correction! hands the solver): the source term, both direct solvers
    and the copy into the haloed pressure give bit-identical interiors"""
    O = oracle
    rng = np.random.default_rng(2025)
    gH, g3 = _grids(O, size, topo, z, halo)
    U = [random_parent(gH, l, rng) for l in LOCS]
    if topo[2] == "F":
        U[2][...] = 0
    for l, a in zip(LOCS, U):
        O.fill_halo_regions(gH, a, l)
    U3 = [_cut(gH, g3, a) for a in U]
    for l, a in zip(LOCS, U3):  # the cut of a filled parent is a filled parent
        b = a.copy(order="F")
        O.fill_halo_regions(g3, b, l)
        np.testing.assert_array_equal(a, b)
    solvers = []
    if gH.dzc is None:
        solvers.append(O.FFTBasedPoissonSolver)
    if topo[2] == "B":
        solvers.append(O.FourierTridiagonalPoissonSolver)
    assert solvers
    for S in solvers:
        pH, p3 = gH.zeros(0), g3.zeros(0)
        for g, V, p in ((gH, U, pH), (g3, U3, p3)):
            s = S(g)
            s.source_term(*V, 1.0)
            s.solve(p)
        assert np.abs(p3).max() > 0
        np.testing.assert_array_equal(gH.interior_N(pH), g3.interior_N(p3), err_msg=S.__name__)


@pytest.mark.parametrize("size,topo,z,halo", CASES)
@pytest.mark.parametrize("loc", [0, 1, 2, 4])
def test_periodic_fill_is_modular_indexing(oracle, size, topo, z, halo, loc):
    """fill_halo_regions! along Periodic directions: parent index p holds interior cell (p - H) mod N, for centre and face
    fields, halo = size included; the interior itself is left alone"""
    O = oracle
    rng = np.random.default_rng(7 + loc)
    gH, _ = _grids(O, size, topo, z, halo)
    a = random_parent(gH, loc, rng)
    before = a.copy(order="F")
    O.fill_halo_regions(gH, a, loc, fill_boundary_normal_velocities=False)
    N, H = (gH.Nx, gH.Ny, gH.Nz), (gH.Hx, gH.Hy, gH.Hz)
    sl = tuple(slice(H[d], H[d] + N[d]) for d in range(3))
    np.testing.assert_array_equal(a[sl], before[sl])
    for d in range(3):
        if topo[d] != "P":
            continue
        src = H[d] + (np.arange(a.shape[d]) - H[d]) % N[d]
        np.testing.assert_array_equal(a, np.take(a, src, axis=d), err_msg=f"direction {d}")
    if topo == "PPP":
        idx = np.ix_(*[H[d] + (np.arange(a.shape[d]) - H[d]) % N[d] for d in range(3)])
        np.testing.assert_array_equal(a, before[idx])
