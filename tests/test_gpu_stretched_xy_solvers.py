"""FourierTridiagonalPoissonSolver and BatchedTridiagonalSolver along a stretched x or y (fourier_tridiagonal_poisson_solver.jl:17-39,
82-177; batched_tridiagonal_solver.jl XDirection / YDirection).  Reference values: numpy restatements of the stretched divergence and
Laplacian (divergence_operators.jl:16-19, laplacian_operators.jl), and the oracle's z-stretched solver / z sweep applied to the
axis-permuted problem."""
import types
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P, B, F = "Periodic", "Bounded", "Flat"
TOPOS = [(P, P, B), (P, B, B), (B, P, B), (B, B, B), (P, B, P), (B, P, P), (B, B, P), (F, B, B), (F, P, B), (B, F, B), (P, F, B)]
FACES_EVEN = [1, 2, 4, 7, 11, 16, 22, 29, 37]
FACES_ODD = [1, 2, 4, 7, 11, 16, 22, 29, 37, 51]
LOCS = (1, 2, 4)


def _size_cases():
    out = [(4, 5, list(range(1, 5))), (8, 8, list(range(1, 9))), (7, 7, list(range(1, 8)))]
    for faces in (FACES_EVEN, FACES_ODD):
        for n1, n2 in ((8, 8), (16, 8), (8, 16), (8, 11), (5, 8), (7, 13)):
            out.append((n1, n2, faces))
    return out


CASES = [(topo, axis, n1, n2, faces) for topo in TOPOS for axis in (0, 1) if topo[axis] == B for (n1, n2, faces) in _size_cases()]
PERM = {0: (1, 2, 0), 1: (0, 2, 1)}  # axes of the permuted problem whose z is the stretched direction


def _grid(ocn, topo, axis, n1, n2, faces, arch=None):
    """stretched_poisson_solver_correct_answer's grid (dependencies_for_poisson_solvers.jl:163-182): sizes circshift([N1, N2, Ns], axis)"""
    ns = len(faces) - 1
    size = {0: (ns, n1, n2), 1: (n2, ns, n1)}[axis]
    ext = [(0, 1), (0, 1), (0, 1)]
    ext[axis] = np.asarray(faces, dtype=np.float64)
    kw = {n: (None if t == F else e) for n, t, e in zip("xyz", topo, ext)}
    return ocn.RectilinearGrid(arch or ocn.GPU(), size=tuple(s for s, t in zip(size, topo) if t != F), topology=topo, **kw)


def _spacings(g):
    """(Δᶜ over the interior cells, Δᶠ over the faces 1 .. N+1) per dimension"""
    out = []
    for d, n in enumerate("xyz"):
        N, H = g.size[d], (g.Hx, g.Hy, g.Hz)[d]
        c = getattr(g, f"_d{n}c_host")
        if c is not None:
            out.append((c[H:H + N], getattr(g, f"_d{n}f_host")[H:H + N + 1]))
        else:
            D = (g.dx, g.dy, g.dz)[d]
            out.append((np.full(N, D), np.full(N + 1, D)))
    return out


def _shape(a, d):
    s = [1, 1, 1]
    s[d] = -1
    return a.reshape(s)


def _velocity_parents(g, rng):
    """random u, v, w parents [i, j, k]: zero on the walls of Bounded directions, periodic images in the halos of Periodic ones"""
    out = []
    for loc in LOCS:
        d = {1: 0, 2: 1, 4: 2}[loc]
        a = rng.uniform(-1, 1, g.parent_shape(loc))
        for e in range(3):
            N, H, t = g.size[e], (g.Hx, g.Hy, g.Hz)[e], g.topology[e]
            if t == P:
                idx = H + (np.arange(a.shape[e]) - H) % N
                a = np.take(a, idx, axis=e)
            elif t == B and e == d:
                sl = [slice(None)] * 3
                for face in (H, H + N):
                    sl[e] = face
                    a[tuple(sl)] = 0.0
        if g.topology[d] == F:
            a[...] = 0.0
        out.append(np.ascontiguousarray(a))
    return out


def _divergence(g, U):
    """divᶜᶜᶜ on the stretched metrics, numpy: 1/V (δx(Ax u) + δy(Ay v) + δz(Az w)), Ax = Δy Δz, Ay = Δx Δz, Az = Δx Δy, V = Δx Δy Δz"""
    (cx, _), (cy, _), (cz, _) = _spacings(g)
    dx, dy, dz = _shape(cx, 0), _shape(cy, 1), _shape(cz, 2)
    H = (g.Hx, g.Hy, g.Hz)
    N = g.size
    terms = []
    for d, a in enumerate(U):
        sl = [slice(H[e], H[e] + N[e]) for e in range(3)]
        if g.topology[d] == F:
            terms.append(0.0)
            continue
        hi = list(sl)
        hi[d] = slice(H[d] + 1, H[d] + N[d] + 1)
        A = (dy * dz, dx * dz, dx * dy)[d]
        terms.append(A * a[tuple(hi)] - A * a[tuple(sl)])
    return (1 / ((dx * dy) * dz)) * ((terms[0] + terms[1]) + terms[2])


def _laplacian(g, phi):
    """∇²ᶜᶜᶜ with the solver's boundary conditions: zero gradient on Bounded walls, periodic images"""
    sp = _spacings(g)
    dx, dy, dz = (_shape(c, d) for d, (c, _) in enumerate(sp))
    out = 0.0
    for d in range(3):
        if g.topology[d] == F:
            continue
        pad = [(0, 0)] * 3
        pad[d] = (1, 1)
        ext = np.pad(phi, pad, mode="wrap" if g.topology[d] == P else "edge")
        grad = np.diff(ext, axis=d) / _shape(sp[d][1], d)
        A = (dy * dz, dx * dz, dx * dy)[d]
        out = out + A * np.diff(grad, axis=d)
    return out / ((dx * dy) * dz)


def _solve_for_pressure(ocn, g, U, dt=0.7):
    fields = []
    for loc, a in zip(LOCS, U):
        f = ocn.Field(loc, g)
        f.data.copy_(ocn.on_architecture(g.architecture, np.ascontiguousarray(a.T)))
        fields.append(f)
    solver = ocn.nonhydrostatic_pressure_solver(g)
    p = ocn.CenterField(g)
    ocn.solve_for_pressure(p, solver, dt, fields)
    ocn.sync_device()
    return solver, p.interior().copy()


def _oracle_phi(O, g, axis, R):
    """the oracle's z-stretched FourierTridiagonalPoissonSolver on the axis-permuted grid and source, permuted back"""
    perm = PERM[axis]
    code = {P: "P", B: "B", F: "F"}
    faces = np.asarray(getattr(g, "xyz"[axis] + "_faces"))[(g.Hx, g.Hy)[axis]:(g.Hx, g.Hy)[axis] + g.size[axis] + 1]
    ext = [None if g.topology[perm[a]] == F else (0, 1) for a in range(2)]
    og = O.Grid(tuple(g.size[perm[a]] for a in range(3)), x=ext[0], y=ext[1], z=faces,
                topology="".join(code[g.topology[perm[a]]] for a in range(3)), halo=tuple((g.Hx, g.Hy, g.Hz)[perm[a]] for a in range(3)))
    S = O.FourierTridiagonalPoissonSolver(og)
    S.set_source_term(np.transpose(R, perm))
    p0 = og.zeros(0)
    S.solve(p0)
    return np.transpose(og.interior(p0), np.argsort(perm))


@pytest.mark.parametrize("topo,axis,n1,n2,faces", CASES,
                         ids=[f"{''.join(t[0] for t in c[0])}-{'xy'[c[1]]}-{c[2]}x{c[3]}-{len(c[4]) - 1}" for c in CASES])
def test_stretched_poisson_solver_correct_answer(oracle, ocn, topo, axis, n1, n2, faces):
    """test_poisson_solvers_stretched_grids.jl:12-50 for stretched_axis 1 and 2: R = div(U) of a random U through solve_for_pressure;
    ∇²ϕ = R to √eps, mean(ϕ) = 0, and ϕ equals the oracle's z-stretched solver on the axis-permuted problem"""
    g = _grid(ocn, topo, axis, n1, n2, faces)
    rng = np.random.default_rng(zlib.crc32(repr((topo, axis, n1, n2, len(faces))).encode()))
    U = _velocity_parents(g, rng)
    dt = 0.7
    solver, phi = _solve_for_pressure(ocn, g, U, dt)
    assert isinstance(solver, ocn.FourierTridiagonalPoissonSolver) and solver.info()["kind"] == 4 + axis
    R = _divergence(g, U) / dt
    assert np.linalg.norm(_laplacian(g, phi) - R) <= np.sqrt(np.finfo(float).eps) * np.linalg.norm(R)
    assert abs(phi.mean()) <= 1e-12 * max(1.0, np.abs(phi).max())
    ref = _oracle_phi(oracle, g, axis, R)
    assert np.abs(phi - ref).max() <= 1e-10 * np.abs(ref).max()
    # set_source_term! (multiplies by Δξᶜ itself) + solve! gives the same solution
    solver.set_source_term(R)
    q = ocn.CenterField(g)
    solver.solve(q)
    ocn.sync_device()
    assert np.abs(q.interior() - phi).max() <= 1e-10 * max(1.0, np.abs(phi).max())


@pytest.mark.parametrize("topo,axis", [((B, P, P), 0), ((B, B, B), 0), ((P, B, B), 1), ((B, B, P), 1), ((F, B, B), 1), ((B, F, B), 0)])
def test_uniform_faces_agree_with_the_regular_fft_solver(ocn, topo, axis):
    """uniform faces given as an array: the Thomas sweep along x / y solves the system the cosine-transform solver solves"""
    size = [12, 10, 9]
    faces = np.linspace(0.0, 1.0, size[axis] + 1)
    ext = [(0, 1), (0, 1), (0, 1)]
    ext[axis] = faces
    kw = {n: (None if t == F else e) for n, t, e in zip("xyz", topo, ext)}
    sz = tuple(s for s, t in zip(size, topo) if t != F)
    gs = ocn.RectilinearGrid(ocn.GPU(), size=sz, topology=topo, **kw)
    gr = ocn.RectilinearGrid(ocn.GPU(), size=sz, topology=topo, **{n: (None if t == F else (0, 1)) for n, t in zip("xyz", topo)})
    U = _velocity_parents(gs, np.random.default_rng(7))
    _, phi_s = _solve_for_pressure(ocn, gs, U)
    fields = []
    for loc, a in zip(LOCS, U):
        f = ocn.Field(loc, gr)
        f.data.copy_(ocn.on_architecture(gr.architecture, np.ascontiguousarray(a.T)))
        fields.append(f)
    p = ocn.CenterField(gr)
    ocn.solve_for_pressure(p, ocn.FFTBasedPoissonSolver(gr), 0.7, fields)
    ocn.sync_device()
    phi_r = p.interior()
    assert np.abs(phi_s - phi_r).max() <= 1e-10 * max(1.0, np.abs(phi_r).max())


@pytest.mark.parametrize("Nx,Ny,Nz", [(2, 5, 3), (3, 7, 11), (63, 5, 3), (64, 4, 4), (65, 9, 7), (257, 3, 5), (512, 6, 11), (64, 64, 2)])
def test_x_sweep_tiling(oracle, ocn, Nx, Ny, Nz):
    """Chunks of the LDS-staged x sweep: ragged last chunks, line counts that are not a multiple of the workgroup's 64"""
    faces = np.cumsum(np.r_[0.0, 1 + 0.5 * np.sin(np.arange(Nx))])
    g = ocn.RectilinearGrid(ocn.GPU(), size=(Nx, Ny, Nz), topology=(B, P, B), x=faces, y=(0, 1), z=(0, 1))
    U = _velocity_parents(g, np.random.default_rng(Nx))
    _, phi = _solve_for_pressure(ocn, g, U)
    R = _divergence(g, U) / 0.7
    assert np.linalg.norm(_laplacian(g, phi) - R) <= np.sqrt(np.finfo(float).eps) * np.linalg.norm(R)
    ref = _oracle_phi(oracle, g, 0, R)
    assert np.abs(phi - ref).max() <= 1e-10 * np.abs(ref).max()


def test_x_sweep_at_256_cubed(ocn):
    """(Bounded, Periodic, Periodic) stretched in x at 256³: the property check on the full size"""
    N = 256
    faces = np.cumsum(np.r_[0.0, 1 + 0.5 * np.cos(np.linspace(0, 3 * np.pi, N))])
    g = ocn.RectilinearGrid(ocn.GPU(), size=(N, N, N), topology=(B, P, P), x=faces, y=(0, 200.0), z=(0, 200.0))
    U = _velocity_parents(g, np.random.default_rng(256))
    solver, phi = _solve_for_pressure(ocn, g, U)
    assert solver.info()["kind"] == 4
    R = _divergence(g, U) / 0.7
    assert np.linalg.norm(_laplacian(g, phi) - R) <= np.sqrt(np.finfo(float).eps) * np.linalg.norm(R)


def _dense_solve(a, b, c, f):
    M = np.diag(b) + np.diag(a, -1) + np.diag(c, 1)
    return np.linalg.solve(M, f)


@pytest.mark.parametrize("direction", ["x", "y"])
@pytest.mark.parametrize("N", [3, 5, 8, 11, 16])
def test_batched_tridiagonal_single_system(ocn, direction, N):
    """can_solve_single_tridiagonal_system (test_batched_tridiagonal_solver.jl:7-42): a 1-D diagonal"""
    rng = np.random.default_rng(N)
    a, c, f = rng.random(N - 1), rng.random(N - 1), rng.random(N)
    b = 3 + rng.random(N)
    d = "xy".index(direction)
    shape = [1, 1, 1]
    shape[d] = N
    solver = ocn.BatchedTridiagonalSolver(ocn.GPU(), a, b, c, tridiagonal_direction=(ocn.XDirection, ocn.YDirection)[d]())
    phi = solver.solve(f.reshape(shape).astype(complex))
    np.testing.assert_allclose(phi.reshape(-1).real, _dense_solve(a, b, c, f), rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("direction", ["x", "y"])
@pytest.mark.parametrize("Nx,Ny,Nz", [(3, 5, 8), (8, 16, 11), (3, 16, 8), (8, 5, 11)])
def test_batched_tridiagonal_3d_rhs(oracle, ocn, direction, Nx, Ny, Nz):
    """can_solve_batched_tridiagonal_system_with_3D_RHS (test_batched_tridiagonal_solver.jl:44-114) along x / y, against numpy; a 3-D
    diagonal bitwise against the oracle's z sweep on the transposed arrays"""
    d = "xy".index(direction)
    Dir = (ocn.XDirection, ocn.YDirection)[d]
    N = (Nx, Ny, Nz)[d]
    rng = np.random.default_rng(N * 100 + Nz)
    a, c = rng.random(N - 1), rng.random(N - 1)
    b1 = 3 + rng.random(N)
    f = rng.standard_normal((Nx, Ny, Nz)) + 1j * rng.standard_normal((Nx, Ny, Nz))
    phi = ocn.BatchedTridiagonalSolver(ocn.GPU(), a, b1, c, tridiagonal_direction=Dir()).solve(f)
    fm = np.moveaxis(f, d, -1)
    want = np.moveaxis(np.apply_along_axis(lambda v: _dense_solve(a, b1, c, v), -1, fm), -1, d)
    np.testing.assert_allclose(phi, want, rtol=1e-12, atol=1e-13)
    # bitwise the z sweep on the transposed problem (both sweeps are built without FMA contraction)
    b = 3 + rng.random((Nx, Ny, Nz))
    perm = PERM[d]
    got = ocn.BatchedTridiagonalSolver(ocn.GPU(), a, b, c, tridiagonal_direction=Dir()).solve(f)
    ref = oracle.batched_tridiagonal_solve_z(a, np.transpose(b, perm), c, np.transpose(f, perm))
    np.testing.assert_array_equal(got, np.transpose(ref, np.argsort(perm)))


@pytest.mark.parametrize("direction", ["x", "y"])
def test_batched_tridiagonal_keeps_storage_at_a_singular_pivot(ocn, direction):
    """test_gpu_model.py's singular-pivot case along x / y: β₂ = 1 - 1 * 1 = 0, so ϕ₂ = ϕ⁰₂ and ϕ₁ = f₁ / b₁ - ϕ⁰₂"""
    d = "xy".index(direction)
    perm = PERM[d]
    inv = np.argsort(perm)
    a, c = np.array([1.0]), np.array([1.0])
    b = np.transpose(np.ones((3, 2, 2)), inv)
    fz = np.arange(12, dtype=np.float64).reshape(3, 2, 2) + 1j * np.arange(12, dtype=np.float64).reshape(3, 2, 2)[::-1]
    f = np.transpose(fz, inv)
    phi0 = np.full(f.shape, 7.0 - 2.0j)
    phi = ocn.BatchedTridiagonalSolver(ocn.GPU(), a, b, c, tridiagonal_direction=(ocn.XDirection, ocn.YDirection)[d]()).solve(f, phi0)
    pz = np.transpose(phi, perm)
    np.testing.assert_array_equal(pz[..., 1], np.full((3, 2), 7.0 - 2.0j))
    np.testing.assert_array_equal(pz[..., 0], fz[..., 0] / 1.0 - 1.0 * (7.0 - 2.0j))


def test_solver_refusals(ocn):
    gp = ocn.RectilinearGrid(ocn.GPU(), size=(8, 8, 4), x=np.linspace(0, 1, 9) ** 2, y=(0, 1), z=(0, 1), topology=(B, P, B))
    solver = ocn.FourierTridiagonalPoissonSolver(gp)
    p = ocn.CenterField(gp)
    solver.set_source_term(np.zeros((8, 8, 4)))
    with pytest.raises(ocn.OcnError, match="FFT-based solvers only"):
        ocn._lib.call("ocn_poisson_solve_shifted", solver._h, p.ptr, 1.0, None)
    with pytest.raises(ValueError):
        ocn.FFTBasedPoissonSolver(gp)
    g2 = ocn.RectilinearGrid(ocn.GPU(), size=(8, 8, 4), x=np.linspace(0, 1, 9) ** 2, y=np.linspace(0, 1, 9) ** 3, z=(0, 1), topology=(B, B, B))
    with pytest.raises(NotImplementedError):
        ocn.FourierTridiagonalPoissonSolver(g2)


def test_models_and_distributed_refuse_stretched_x_or_y(ocn):
    """Time stepping on grids stretched in x / y is out of scope: refused before anything is allocated"""
    for kw in (dict(x=np.linspace(0, 1, 9) ** 2, y=(0, 1)), dict(x=(0, 1), y=np.linspace(0, 1, 9) ** 2)):
        g = ocn.RectilinearGrid(ocn.GPU(), size=(8, 8, 4), z=(0, 1), topology=(B, B, B), **kw)
        with pytest.raises(NotImplementedError):
            ocn.NonhydrostaticModel(g)
        with pytest.raises(NotImplementedError):
            ocn.HydrostaticFreeSurfaceModel(g)
        # the default fills (no flux, impenetrable walls) work; a condition on a stretched wall is refused
        c = ocn.CenterField(g)
        ocn.fill_halo_regions(c)
        side = "west" if "x" in kw and np.ndim(kw["x"]) == 1 and len(kw["x"]) > 2 else "south"
        bc = ocn.FieldBoundaryConditions(**{side: ocn.GradientBoundaryCondition(1.0)})
        with pytest.raises(NotImplementedError):
            ocn.fill_halo_regions(ocn.CenterField(g, boundary_conditions=bc))
    # a model on a regular grid, pointed at a stretched one, is refused by the drivers too
    gr = ocn.RectilinearGrid(ocn.GPU(), size=(8, 8, 8), x=(0, 1), y=(0, 1), z=(0, 1), topology=(P, P, P))
    m = ocn.NonhydrostaticModel(gr, advection=ocn.WENO())
    m.grid = ocn.RectilinearGrid(ocn.GPU(), size=(8, 8, 8), x=np.linspace(0, 1, 9) ** 2, y=(0, 1), z=(0, 1), topology=(B, P, P))
    for drv in (ocn.RK3Driver, ocn.ModelRK3Driver):
        with pytest.raises(NotImplementedError, match="stretched"):
            drv(m)
    arch = ocn.Distributed(ocn.GPU(), fabric=types.SimpleNamespace(rank=0, size=1))
    with pytest.raises(NotImplementedError, match="Distributed"):
        ocn.RectilinearGrid(arch, size=(8, 8, 4), x=np.linspace(0, 1, 9) ** 2, y=(0, 1), z=(0, 1), topology=(B, P, B))
