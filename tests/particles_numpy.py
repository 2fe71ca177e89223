"""The particle kernels of csrc/particles.hip restated with NumPy, vectorised over the particles, in the reference's operand order
(src/Fields/interpolate.jl:15-59, 67-83, 137-188, 298-336; src/Models/LagrangianParticleTracking/lagrangian_particle_advection.jl:10-165).

Every operation is one IEEE double operation in the order the reference writes it, and the kernel is compiled without FMA contraction,
so kernel and restatement agree bit for bit.  Fields are parent arrays indexed [i, j, k] with halos (Field.parent()).

The one thing that is not the reference's: each fractional index is clamped to the open interval whose truncation and right neighbour
lie inside the parent array (the reference would read out of bounds there); tests/test_host_particles.py pins the restatement to what
the reference's own test asserts."""
import numpy as np

PERIODIC, BOUNDED, FLAT = "Periodic", "Bounded", "Flat"


class Geometry:
    """What the kernels know of a grid: sizes, halos, topology, spacings, first nodes, right edges, stretched z nodes."""

    def __init__(self, grid):
        self.N = (grid.Nx, grid.Ny, grid.Nz)
        self.H = (grid.Hx, grid.Hy, grid.Hz)
        self.topo = tuple(grid.topology)
        self.d = (grid.dx, grid.dy, grid.dz)
        self.face0, self.center0, self.right = [0.0] * 3, [0.0] * 3, [0.0] * 3
        for a in range(3):
            if self.topo[a] == FLAT:
                continue
            self.face0[a] = float(grid.nodes_1d(a, True)[0])
            self.center0[a] = float(grid.nodes_1d(a, False)[0])
            self.right[a] = float(grid.domain(a)[1])
        self.znodes = None
        if grid.z_faces is not None:
            self.znodes = (np.asarray(grid.nodes_1d(2, False), dtype=np.float64), np.asarray(grid.nodes_1d(2, True), dtype=np.float64))

    def parent_extent(self, a, face):
        return self.N[a] + 2 * self.H[a] + (1 if (face and self.topo[a] == BOUNDED) else 0)


def index_binary_search(vec, val, N):
    """interpolate.jl:30-46, 1-based results"""
    low, high = 0, N - 1
    while low + 1 < high:
        mid = int((low + high) / 2)
        if vec[mid] == val:
            return mid + 1, mid + 1
        elif vec[mid] < val:
            low = mid
        else:
            high = mid
    return low + 1, high + 1


def fractional_index(val, vec, N):
    """interpolate.jl:48-59"""
    out = np.empty(val.shape, dtype=np.float64)
    with np.errstate(all="ignore"):
        for p, v in enumerate(val):
            i1, i2 = index_binary_search(vec, v, N)
            x1, x2 = vec[i1 - 1], vec[i2 - 1]
            ii = np.float64(i2 - i1) / (x2 - x1) * (v - x1) + np.float64(i1)
            out[p] = np.float64(i1) if i1 == i2 else ii
    return out


def interpolator(geom, a, face, x):
    """(i⁻, i⁺ - i⁻, ξ) along direction a at Face / Center for the coordinates x"""
    n = x.shape[0]
    if geom.topo[a] == FLAT:
        return np.ones(n, dtype=np.int64), 0, np.zeros(n)
    with np.errstate(all="ignore"):
        if a == 2 and geom.znodes is not None:
            vec = geom.znodes[1 if face else 0]
            f = fractional_index(x, vec, len(vec))
        else:
            x0 = geom.face0[a] if face else geom.center0[a]
            f = (x - x0) / geom.d[a] + 1
        L, U = 1 - geom.H[a], geom.N[a] + geom.H[a] + (1 if (face and geom.topo[a] == BOUNDED) else 0)
        flo = np.nextafter(np.float64(L - 1), np.inf) if L <= 0 else np.float64(L)
        fhi = np.nextafter(np.float64(U), -np.inf)
        f = np.fmin(np.fmax(f, flo), fhi)
        return np.trunc(f).astype(np.int64), 1, np.mod(f, 1.0)


def interpolate(geom, data, loc, x, y, z):
    """interpolate((x, y, z), field, location) of a parent array `data` [i, j, k] at bitmask loc (bit 0 / 1 / 2: Face in x / y / z)"""
    assert data.shape == tuple(geom.parent_extent(a, (loc >> a) & 1) for a in range(3)), (data.shape, loc)
    (i, di, xi), (j, dj, eta), (k, dk, zeta) = (interpolator(geom, a, (loc >> a) & 1, c) for a, c in enumerate((x, y, z)))
    i, j, k = i - 1 + geom.H[0], j - 1 + geom.H[1], k - 1 + geom.H[2]
    for lo, step, extent in ((i, di, data.shape[0]), (j, dj, data.shape[1]), (k, dk, data.shape[2])):
        assert lo.size == 0 or (lo.min() >= 0 and lo.max() + step < extent), "an index outside the parent array"
    with np.errstate(all="ignore"):
        s = (1 - xi) * (1 - eta) * (1 - zeta) * data[i, j, k]
        s = s + (1 - xi) * (1 - eta) * zeta * data[i, j, k + dk]
        s = s + (1 - xi) * eta * (1 - zeta) * data[i, j + dj, k]
        s = s + (1 - xi) * eta * zeta * data[i, j + dj, k + dk]
        s = s + xi * (1 - eta) * (1 - zeta) * data[i + di, j, k]
        s = s + xi * (1 - eta) * zeta * data[i + di, j, k + dk]
        s = s + xi * eta * (1 - zeta) * data[i + di, j + dj, k]
        s = s + xi * eta * zeta * data[i + di, j + dj, k + dk]
    return s


def enforce_boundary_conditions(topo, x, xL, xR, Cr):
    with np.errstate(all="ignore"):
        if topo == BOUNDED:
            return np.where(x > xR, xR - Cr * (x - xR), np.where(x < xL, xL + Cr * (xL - x), x))
        if topo == PERIODIC:
            return np.where(x > xR, xL + (x - xR), np.where(x < xL, xR - (xL - x), x))
    return x


def advect(geom, x, y, z, u, v, w, dt, restitution=1.0, unbounded=False):
    """advect_particle for every particle: new (x, y, z); unbounded=True: the positions before enforce_boundary_conditions too"""
    up = interpolate(geom, u, 1, x, y, z)
    vp = interpolate(geom, v, 2, x, y, z)
    wp = interpolate(geom, w, 4, x, y, z)
    with np.errstate(all="ignore"):
        raw = (x + up * dt, y + vp * dt, z + wp * dt)
    new = tuple(enforce_boundary_conditions(geom.topo[a], raw[a], geom.face0[a], geom.right[a], restitution) for a in range(3))
    return (new, raw) if unbounded else new


def crossings(geom, raw):
    """per direction: (any particle left of the domain, any right of it) before the boundary conditions were enforced"""
    return [(bool(np.any(raw[a] < geom.face0[a])), bool(np.any(raw[a] > geom.right[a]))) for a in range(3)]
