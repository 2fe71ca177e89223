"""RectilinearGrid: mirrors src/Grids/rectilinear_grid.jl:248-275 and grid_generation.jl:34-155
for x, y, z each regular or (Bounded) stretched; topologies (Periodic, Periodic, Periodic|Bounded|Flat).
"""
import ctypes as C
import math
import struct
from fractions import Fraction

import numpy as np
import torch

from . import _lib
from .architectures import child_architecture, device

Periodic, Bounded, Flat, FullyConnected = "Periodic", "Bounded", "Flat", "FullyConnected"
# the first / last slab of a grid whose partitioned x is Bounded (Grids.jl:97-108): wall on the west / on the east side only
RightConnected, LeftConnected = "RightConnected", "LeftConnected"
_CODE = {Periodic: _lib.OCN_PERIODIC, Bounded: _lib.OCN_BOUNDED, Flat: _lib.OCN_FLAT, FullyConnected: _lib.OCN_FULLY_CONNECTED,
         RightConnected: _lib.OCN_RIGHT_CONNECTED, LeftConnected: _lib.OCN_LEFT_CONNECTED}
# topologies whose Face fields carry the east boundary face: N + 1 points (BoundedTopology, grid_utils.jl:43)
_EAST_FACE = (Bounded, LeftConnected)


class Center:
    pass


class Face:
    pass


def _exact(x):
    return Fraction(float(x))


class _JuliaRange:
    """range(start, stop, length = n) of Julia's Base for Float64 -- the object the reference stores as a regular coordinate
    (`F = range(FT(F₋), FT(F₊), length = TF)`, src/Grids/grid_generation.jl:117-121): a StepRangeLen whose reference value and step are
    double-double numbers (base/twiceprecision.jl, `_linspace`).  Its elements are what xnodes / ynodes / znodes return, and they
    are NOT c₁ + (i - 1) Δ rounded once: the reference's own doctest prints `x ∈ [3.60072e-17, 6.28319)` for x = (0, 2π)
    (src/Grids/rectilinear_grid.jl:176-182), which this class reproduces (tests/test_reference_fixtures.py)."""

    def __init__(self, start, stop, n):
        self.n = n
        self.rational = None
        if n < 2 or start == stop:
            self.rational = [Fraction(start)] * n
            return
        p, q = self._rat(start), self._rat(stop)
        if p[1] and q[1]:
            den = p[1] * q[1] // math.gcd(p[1], q[1])
            if abs(den * start) <= 2.0 ** 53 and abs(den * stop) <= 2.0 ** 53:
                a, b = round(den * start), round(den * stop)
                if a / den == start and b / den == stop:  # endpoints are exact ratios: interpolate exactly, round once
                    self.rational = [Fraction(a * (n - i) + b * (i - 1), (n - 1) * den) for i in range(1, n + 1)]
                    return
        span = stop - start
        k = round(-(start / span) * (n - 1) + 1)  # index of the element of smallest magnitude
        if 1 < k < n:
            t = (k - 1) / (n - 1)
            ref = (1 - t) * start + t * stop
            step = (ref - start) / (k - 1) if k - 1 < n - k else (stop - ref) / (n - k)
        else:
            k = 1 if k <= 1 else n
            ref, step = (start, span / (n - 1)) if k == 1 else (stop, span / (n - 1))
        bits = min(27, math.ceil(math.log2(max(k - 1, n - k))) + 1)
        hi = struct.unpack("<d", struct.pack("<Q", struct.unpack("<Q", struct.pack("<d", step))[0] >> bits << bits))[0]
        lo_end, hi_end = self._two_sum((1 - k) * hi, ref), self._two_sum((n - k) * hi, ref)
        ea, eb = (start - lo_end[0]) - lo_end[1], (stop - hi_end[0]) - hi_end[1]
        self.k, self.ref, self.step_hi = k, ref, hi
        self.step_lo = (eb - ea) / (n - 1)
        self.ref_lo = ea - (1 - k) * self.step_lo

    @staticmethod
    def _two_sum(x, y):
        if abs(y) > abs(x):
            x, y = y, x
        h = x + y
        return h, (x - h) + y

    @staticmethod
    def _rat(x, limit=1 << 24):
        """Base.rat: the continued-fraction convergent of x with terms up to maxintfloat(Float32)"""
        y, a, b, c, d = x, 1, 0, 0, 1
        while abs(y) <= limit:
            f = math.trunc(y)
            y -= f
            a, c = f * a + c, a
            b, d = f * b + d, b
            if max(abs(a), abs(b)) > limit:
                return c, d
            if y == 0 or a / b == x:
                break
            y = 1.0 / y
        return a, b

    def __getitem__(self, i):
        """element i, 1-based like the reference's indices"""
        if self.rational is not None:
            return float(self.rational[i - 1])
        u = i - self.k
        hi, lo = self._two_sum(self.ref, u * self.step_hi)
        return hi + (lo + (u * self.step_lo + self.ref_lo))


def require_regular_xy(grid, who):
    """What time-steps a grid (tendency kernels, halo fills with boundary fluxes, drivers) reads a regular x and y from ocn_grid:
    refuse a grid stretched in x or y before anything is allocated (only the Poisson solvers run on such grids)."""
    dims = [d for d in getattr(grid, "stretched_dimensions", ()) if d < 2]
    if dims:
        raise NotImplementedError(f"{who} on a grid stretched in {' and '.join('xy'[d] for d in dims)}: time stepping needs a regular x and y "
                                  "(only the Poisson solvers support stretched x / y)")


class RectilinearGrid:
    """RectilinearGrid(arch; size, x, y, z, topology, halo).

    `size`/`halo` omit Flat dimensions like the reference (input_validation.jl:61-95).  `x`, `y`, `z` may each be a
    2-tuple (regular), an array of N+1 increasing face positions or a function of the face index (stretched, needs that
    direction Bounded).  Only the Poisson solvers run on a grid stretched in x or y; the models need a regular x and y."""

    def __init__(self, architecture, size, x=None, y=None, z=None, topology=(Periodic, Periodic, Bounded), halo=None,
                 extent=None, _local=False):
        if extent is not None:
            # validate_rectilinear_domain (input_validation.jl:106-131): an "oceanic" default domain x = (0, Lx), y = (0, Ly), z = (-Lz, 0)
            if x is not None or y is not None or z is not None:
                raise ValueError("Cannot specify both 'extent' and 'x, y, z' keyword arguments.")
            ext_t = tuple(extent) if np.ndim(extent) else (extent,)
            if len(ext_t) != sum(t != Flat for t in topology):
                raise ValueError(f"extent {ext_t} must have one entry per non-Flat dimension of {tuple(topology)}")
            it = iter(ext_t)
            Ls = [None if t == Flat else float(next(it)) for t in topology]
            x = None if Ls[0] is None else (0.0, Ls[0])
            y = None if Ls[1] is None else (0.0, Ls[1])
            z = None if Ls[2] is None else (-Ls[2], 0.0)
        if hasattr(architecture, "partition") and not _local:
            if any(callable(e) or (e is not None and np.ndim(e) == 1 and len(e) != 2) for e in (x, y)):
                raise NotImplementedError("a Distributed grid stretched in x or y: the distributed solvers need a regular x and y")
            # RectilinearGrid(arch::Distributed, ...) returns the rank-local grid (distributed_grids.jl:75-118)
            from .distributed import distributed_rectilinear_grid
            g = distributed_rectilinear_grid(architecture, tuple(size), x=x, y=y, z=z, topology=tuple(topology), halo=halo)
            self.__dict__.update(g.__dict__)
            self._ctor = dict(size=tuple(size), x=x, y=y, z=z, topology=tuple(topology))  # the GLOBAL description (with_halo)
            self._ctor_local = False
            return
        self._ctor = dict(size=tuple(size) if np.ndim(size) else (size,), x=x, y=y, z=z, topology=tuple(topology))
        self._ctor_local = _local
        self.architecture = architecture
        topo = tuple(topology)
        for t in topo:
            if t not in _CODE:
                raise ValueError(f"unknown topology {t!r}")
        nflat = sum(t == Flat for t in topo)
        size = tuple(size) if np.ndim(size) else (size,)
        if len(size) != 3 - nflat:
            raise ValueError(f"size {size} must have {3 - nflat} elements for topology {topo}")  # validate_size
        it = iter(size)
        N = [1 if t == Flat else int(next(it)) for t in topo]
        if halo is None:
            H = [0 if t == Flat else min(3, n) for t, n in zip(topo, N)]  # default halo = 3 capped by N
        else:
            halo = tuple(halo) if np.ndim(halo) else (halo,)
            if len(halo) != 3 - nflat:
                raise ValueError(f"halo {halo} must have {3 - nflat} elements")
            it = iter(halo)
            H = [0 if t == Flat else int(next(it)) for t in topo]
        for d in range(3):
            if topo[d] != Flat and H[d] > N[d]:
                raise ValueError(f"halo {H[d]} must be <= size {N[d]} in dimension {d + 1}")  # validate_halo
        self.topology = topo
        self.Nx, self.Ny, self.Nz = N
        self.Hx, self.Hy, self.Hz = H
        ext = [x, y, z]
        L, D = [1.0] * 3, [1.0] * 3
        self.x_faces = self.y_faces = self.z_faces = None
        self._dxc_host = self._dxf_host = self._dyc_host = self._dyf_host = self._dzc_host = self._dzf_host = None
        self._interval = [(0.0, 1.0)] * 3  # end points of each regular dimension (for node coordinates)
        self._ranges = {}
        for d in range(3):
            if topo[d] == Flat:
                continue
            e = ext[d]
            if e is None:
                raise ValueError(f"coordinate {'xyz'[d]} must be given for a non-Flat dimension")
            if callable(e):  # a function of the face index k = 1 .. N+1 (grid_generation.jl:34-50)
                e = np.array([float(e(k)) for k in range(1, N[d] + 2)])
            if np.ndim(e) == 1 and len(e) == 2:
                c1, c2 = e
                self._interval[d] = (float(c1), float(c2))
                if not c2 > c1:
                    raise ValueError(f"{'xyz'[d]} must be an increasing interval!")
                Lx = _exact(c2) - _exact(c1)
                L[d] = float(Lx)                 # FT(L)
                D[d] = float(Lx / N[d])          # FT(BigFloat(L)/N), grid_generation.jl:105-133
            else:
                L[d] = self._generate_stretched(d, np.asarray(e, dtype=np.float64), N[d], H[d], topo[d])
                D[d] = float("nan")
        self.Lx, self.Ly, self.Lz = L
        self.dx, self.dy, self.dz = D
        self._dxc = self._dxf = self._dyc = self._dyf = self._dzc = self._dzf = None
        dev = None if architecture is None else device(child_architecture(architecture))  # None: metadata only (tests)
        if dev is not None:
            for n in ("x", "y", "z"):
                if getattr(self, f"_d{n}c_host") is not None:
                    setattr(self, f"_d{n}c", torch.from_numpy(getattr(self, f"_d{n}c_host")).to(dev))
                    setattr(self, f"_d{n}f", torch.from_numpy(getattr(self, f"_d{n}f_host")).to(dev))
        # (ocn_grid carries the stretched z only; a stretched x / y is 0.0 there and reaches the solvers through their own entry point)
        self.c = _lib.CGrid(self.Nx, self.Ny, self.Nz, self.Hx, self.Hy, self.Hz,
                            _CODE[topo[0]], _CODE[topo[1]], _CODE[topo[2]], 0,
                            0.0 if self.x_faces is not None else self.dx, 0.0 if self.y_faces is not None else self.dy,
                            0.0 if self._dzc is not None else self.dz, self.Lx, self.Ly, self.Lz,
                            None if self._dzc is None else self._dzc.data_ptr(),
                            None if self._dzf is None else self._dzf.data_ptr())

    @property
    def stretched_dimensions(self):
        """stretched_dimensions(grid): the dimensions (0 x, 1 y, 2 z) given as explicit faces"""
        return tuple(d for d, F in enumerate((self.x_faces, self.y_faces, self.z_faces)) if F is not None)

    def _generate_stretched(self, d, faces, N, H, topo):
        """generate_coordinate for explicit faces (grid_generation.jl:34-95) of dimension d: faces with halos, Δᶜ and Δᶠ with element 0
        <-> index 1 - H (the ocn_grid.dzc / dzf layout)."""
        n = "xyz"[d]
        if topo != Bounded:
            raise NotImplementedError(f"a stretched {n} direction must be Bounded")
        if faces.shape != (N + 1,):
            raise ValueError(f"{n} must hold N{n}+1 = {N + 1} face positions")
        if not np.all(np.diff(faces) > 0):
            raise ValueError(f"The elements of {n} must be increasing!")
        F = faces
        dlo = [F[1] - F[0]] * H
        dhi = [F[-1] - F[-2]] * H
        Fm = [F[0] - sum(dlo[i:]) for i in range(H)]
        Fp = [F[N] + sum(dhi[i:]) for i in range(H)][::-1]
        Fall = np.array(Fm + list(F) + Fp)
        TC = N + 2 * H
        Cc = (Fall[1:TC + 1] + Fall[:TC]) / 2
        d0 = list(Cc[1:] - Cc[:-1])
        dzc = Fall[1:] - Fall[:-1]                   # Δzᵃᵃᶜ[k], k = 1-H .. N+H
        dzf_full = np.array([d0[0], d0[0]] + d0)     # Δzᵃᵃᶠ[k], k = -H .. N+H (shifted copy, :72-75)
        dc = np.ascontiguousarray(dzc[:N + 2 * H])
        df = np.ascontiguousarray(dzf_full[1:])  # element 0 <-> k = 1-H
        assert df.size == N + 2 * H and dc.size == N + 2 * H
        setattr(self, f"{n}_faces", Fall)
        setattr(self, f"_d{n}c_host", dc)
        setattr(self, f"_d{n}f_host", df)
        return float(F[N] - F[0])

    # -- node coordinates: the elements of the reference's coordinate ranges (grid_generation.jl:98-135) --------------------------
    def _coordinate_range(self, d, face):
        """F = range(FT(F₋), FT(F₊), length = TF) or C = range(FT(C₋), FT(C₊), length = TC) of a regular dimension; element
        i + H of the range is the reference's ξ[i] (OffsetArray(F, -H))."""
        key = (d, bool(face))
        r = self._ranges.get(key)
        if r is None:
            N = (self.Nx, self.Ny, self.Nz)[d]
            H = (self.Hx, self.Hy, self.Hz)[d]
            bounded = self.topology[d] in _EAST_FACE
            c1, c2 = (Fraction(v) for v in self._interval[d])
            L = c2 - c1
            D = L / N                                                # BigFloat arithmetic of the reference, here exact
            Fm = c1 - H * D
            if face:
                lo, hi, n = Fm, Fm + (L + 2 * H * D if bounded else L + (2 * H - 1) * D), N + 2 * H + (1 if bounded else 0)
            else:
                lo = Fm + D / 2
                hi, n = lo + L + D * (2 * H - 1), N + 2 * H
            r = self._ranges[key] = _JuliaRange(float(lo), float(hi), n)
        return r

    def nodes_1d(self, d, face, with_halos=False):
        """xnodes / ynodes / znodes(grid, ℓ; with_halos): node coordinates along dimension d (0 x, 1 y, 2 z) at Face or Center
        location; a Face location in a Bounded dimension has N+1 interior nodes."""
        N = (self.Nx, self.Ny, self.Nz)[d]
        H = (self.Hx, self.Hy, self.Hz)[d]
        topo = self.topology[d]
        if topo == Flat:
            return np.zeros(1)
        n = N + 1 if (face and topo in _EAST_FACE) else N
        faces = (self.x_faces, self.y_faces, self.z_faces)[d]
        if faces is not None:
            Fall = np.asarray(faces)
            if with_halos:
                return Fall.copy() if face else 0.5 * (Fall[1:] + Fall[:-1])
            F = Fall[H:H + N + 1]
            return F[:n].copy() if face else 0.5 * (F[1:] + F[:-1])
        r = self._coordinate_range(d, face)
        if with_halos:
            return np.array([r[i] for i in range(1, r.n + 1)])
        return np.array([r[i + H] for i in range(1, n + 1)])

    def domain(self, d):
        """x_domain / y_domain / z_domain: (ξ[1], ξ[N+1]) of the Face coordinate (grid_utils.jl:120), what `show(grid)` prints"""
        N = (self.Nx, self.Ny, self.Nz)[d]
        H = (self.Hx, self.Hy, self.Hz)[d]
        faces = (self.x_faces, self.y_faces, self.z_faces)[d]
        if faces is not None:
            F = np.asarray(faces)
            return float(F[H]), float(F[H + N])
        r = self._coordinate_range(d, True)
        return r[1 + H], r[N + 1 + H]

    def spacing_extrema(self, d, face=False):
        """(min, max) of the interior cell spacings along d: `min(Δz)=…, max(Δz)=…` of the reference's `show` (Center spacings)"""
        n = "xyz"[d]
        if getattr(self, f"_d{n}c_host") is not None:
            H, N = (self.Hx, self.Hy, self.Hz)[d], (self.Nx, self.Ny, self.Nz)[d]
            a = getattr(self, f"_d{n}f_host" if face else f"_d{n}c_host")[H:H + N + (1 if face else 0)]
            return float(a.min()), float(a.max())
        D = (self.dx, self.dy, self.dz)[d]
        return D, D

    def nodes(self, loc):
        """(x, y, z) node coordinate arrays, shaped for broadcasting over [i, j, k], of a field at bitmask `loc`."""
        x = self.nodes_1d(0, loc & 1).reshape(-1, 1, 1)
        y = self.nodes_1d(1, loc & 2).reshape(1, -1, 1)
        z = self.nodes_1d(2, loc & 4).reshape(1, 1, -1)
        return x, y, z

    def with_halo(self, new_halo):
        """with_halo(new_halo, grid) (rectilinear_grid.jl:367-383): the same grid rebuilt with another halo; new_halo has one entry per
        dimension (entries of Flat dimensions are ignored, like the reference's pop_flat_elements)."""
        if self._ctor_local:
            raise NotImplementedError("with_halo of a rank-local grid: rebuild it from the global description")
        halo = tuple(int(h) for h, t in zip(new_halo, self.topology) if t != Flat)
        g = RectilinearGrid(self.architecture, halo=halo, **self._ctor)
        g.c.math = self.c.math
        return g

    # -- sizes ------------------------------------------------------------------------------------
    def parent_shape(self, loc):
        """(sx, sy, sz) of the OffsetArray parent for a field at `loc` (grid_utils.jl:66-72)."""
        N = (self.Nx, self.Ny, self.Nz)
        H = (self.Hx, self.Hy, self.Hz)
        return tuple(N[d] + 2 * H[d] + (1 if ((loc >> d) & 1 and self.topology[d] in _EAST_FACE) else 0) for d in range(3))

    @property
    def size(self):
        return (self.Nx, self.Ny, self.Nz)

    @property
    def cref(self):
        return C.byref(self.c)

    @property
    def math_mode(self):
        """None (the process default, ocn.set_math_mode) or MATH_STRICT / MATH_FAST: the arithmetic variant of every kernel launched
        for this grid (ocn_grid.math)."""
        return {_lib.GRID_MATH_DEFAULT: None, _lib.GRID_MATH_STRICT: _lib.MATH_STRICT, _lib.GRID_MATH_FAST: _lib.MATH_FAST}[self.c.math]

    def with_math_mode(self, mode):
        """The same grid (shared device vectors) whose launches use `mode` whatever the process default is: two models of one process
        may run different arithmetic variants."""
        import copy
        if mode not in (None, _lib.MATH_STRICT, _lib.MATH_FAST):
            raise ValueError(f"math_mode must be None, MATH_STRICT or MATH_FAST, got {mode!r}")
        g = copy.copy(self)
        g.c = _lib.CGrid.from_buffer_copy(self.c)
        g.c.math = {None: _lib.GRID_MATH_DEFAULT, _lib.MATH_STRICT: _lib.GRID_MATH_STRICT, _lib.MATH_FAST: _lib.GRID_MATH_FAST}[mode]
        return g

    def __repr__(self):
        return (f"{self.Nx}x{self.Ny}x{self.Nz} RectilinearGrid on {self.architecture} with "
                f"{self.Hx}x{self.Hy}x{self.Hz} halo, topology {self.topology}")


# ---- ImmersedBoundaryGrid(grid, GridFittedBottom(h)) (src/ImmersedBoundaries) -----------------------------------------------------------
class CenterImmersedCondition:
    """CenterImmersedCondition() (grid_fitted_bottom.jl:12): a cell is immersed when its centre lies at or below the bottom height"""

    def __repr__(self):
        return "CenterImmersedCondition()"


class InterfaceImmersedCondition:
    """InterfaceImmersedCondition() (grid_fitted_bottom.jl:13): a cell is immersed when its upper interface lies at or below the bottom height"""

    def __repr__(self):
        return "InterfaceImmersedCondition()"


class GridFittedBottom:
    """GridFittedBottom(bottom_height, immersed_condition = CenterImmersedCondition()) (grid_fitted_bottom.jl:15-46).  bottom_height: a
    number, an (Nx, Ny) array or a function f(x, y) of the cell-centre coordinates.  On an ImmersedBoundaryGrid, `bottom_height` is the
    materialized (Nx, Ny) array: the z of the upper interface of the highest immersed cell of every column (the domain's bottom where
    there is none)."""

    def __init__(self, bottom_height, immersed_condition=None):
        immersed_condition = CenterImmersedCondition() if immersed_condition is None else immersed_condition
        if isinstance(immersed_condition, type):
            immersed_condition = immersed_condition()
        if not isinstance(immersed_condition, (CenterImmersedCondition, InterfaceImmersedCondition)):
            raise TypeError("immersed_condition must be CenterImmersedCondition() or InterfaceImmersedCondition()")
        self.bottom_height = bottom_height
        self.immersed_condition = immersed_condition

    def __repr__(self):
        return f"GridFittedBottom({self.immersed_condition!r})"


class PartialCellBottom:
    """PartialCellBottom(bottom_height; minimum_fractional_cell_height = 0.2) (partial_cell_bottom.jl): constructible; an
    ImmersedBoundaryGrid with it is not implemented."""

    def __init__(self, bottom_height, minimum_fractional_cell_height=0.2):
        self.bottom_height, self.minimum_fractional_cell_height = bottom_height, float(minimum_fractional_cell_height)


class GridFittedBoundary:
    """GridFittedBoundary(mask) (grid_fitted_boundary.jl): constructible; an ImmersedBoundaryGrid with it is not implemented."""

    def __init__(self, mask):
        self.mask = mask


def materialize_bottom_height(grid, ib):
    """materialize_immersed_boundary (grid_fitted_bottom.jl:99-122) on the host: (the materialized (Nx, Ny) bottom height, kbot).  The
    height starts at face 1 and is raised to face k + 1 for every k whose centre (CenterImmersedCondition) or upper interface
    (InterfaceImmersedCondition) lies at or below h; kbot counts the cells whose centre lies at or below the result (immersed_cell,
    :124-130)."""
    Nx, Ny, Nz = grid.Nx, grid.Ny, grid.Nz
    h = ib.bottom_height
    if callable(h):  # set!(bottom_field, f): f(x, y) at the (Center, Center) nodes
        x, y = grid.nodes_1d(0, False).reshape(-1, 1), grid.nodes_1d(1, False).reshape(1, -1)
        try:
            a = np.asarray(h(x, y), dtype=np.float64)
        except (TypeError, ValueError):
            a = np.vectorize(h, otypes=[np.float64])(x, y)
        h = np.broadcast_to(a, (Nx, Ny))
    elif np.ndim(h) == 0:
        h = np.full((Nx, Ny), float(h))
    else:
        h = np.asarray(h, dtype=np.float64)
        if h.shape != (Nx, Ny):
            raise ValueError(f"bottom_height has shape {h.shape}; the grid needs ({Nx}, {Ny})")
    h = np.array(h, dtype=np.float64)
    zc, zf = grid.nodes_1d(2, False), grid.nodes_1d(2, True)
    interface = isinstance(ib.immersed_condition, InterfaceImmersedCondition)
    bottom = np.full((Nx, Ny), zf[0])
    for k in range(Nz):
        bottom_cell = (zf[k + 1] <= h) if interface else (zc[k] <= h)
        bottom = np.where(bottom_cell, zf[k + 1], bottom)
    kbot = (zc[None, None, :] <= bottom[:, :, None]).sum(axis=2).astype(np.int32)
    return h, bottom, kbot


class ImmersedBoundaryGrid:
    """ImmersedBoundaryGrid(grid, GridFittedBottom(h)) (immersed_boundary_grid.jl:17-67): `grid` with the cells below the bottom height
    taken out of the fluid.  Every property of the underlying grid is a property of this one (Base.getproperty, :80-85).

    Implemented: a (Periodic, Periodic, Bounded) underlying RectilinearGrid on one GPU with GridFittedBottom; HydrostaticFreeSurfaceModel
    steps on it (hydrostatic.py).  The bathymetry is held as `kbot`, the number of immersed cells per column: cell (i, j, k) is immersed
    iff k <= kbot[i, j]."""

    def __init__(self, grid, immersed_boundary, active_cells_map=False, active_z_columns=False):
        who = "ImmersedBoundaryGrid"
        if isinstance(grid, ImmersedBoundaryGrid):
            raise TypeError(f"{who}: the underlying grid is itself an ImmersedBoundaryGrid")
        if isinstance(immersed_boundary, PartialCellBottom):
            raise NotImplementedError(f"{who}: PartialCellBottom is not implemented; use GridFittedBottom(h)")
        if isinstance(immersed_boundary, GridFittedBoundary):
            raise NotImplementedError(f"{who}: GridFittedBoundary is not implemented; use GridFittedBottom(h)")
        if not isinstance(immersed_boundary, GridFittedBottom):
            raise TypeError(f"{who}: immersed_boundary must be GridFittedBottom(h)")
        if active_cells_map or active_z_columns:
            raise NotImplementedError(f"{who}: active_cells_map = true is not implemented; the kernels keep the whole extent in the launch "
                                      "(leave it at false)")
        if hasattr(grid.architecture, "partition"):
            raise NotImplementedError(f"{who}: Distributed grids are not implemented; build the grid on one GPU")
        if tuple(grid.topology) != (Periodic, Periodic, Bounded):
            raise NotImplementedError(f"{who}: the underlying grid must be (Periodic, Periodic, Bounded); walls or a Flat direction in it are "
                                      f"not implemented (got {tuple(grid.topology)})")
        require_regular_xy(grid, who)
        self.underlying_grid = grid
        h, bottom, kbot = materialize_bottom_height(grid, immersed_boundary)
        self.immersed_boundary = GridFittedBottom(bottom, immersed_boundary.immersed_condition)
        self.kbot = kbot
        self._kbot_halo = np.pad(kbot, ((grid.Hx, grid.Hx), (grid.Hy, grid.Hy)), mode="wrap")
        top = grid.nodes_1d(2, True)[grid.Nz]
        Hcc = np.pad(top - bottom, ((1, 0), (1, 0)), mode="wrap")
        self._depth = {"cc": Hcc[1:, 1:], "fc": np.minimum(Hcc[:-1, 1:], Hcc[1:, 1:]), "cf": np.minimum(Hcc[1:, :-1], Hcc[1:, 1:])}
        self._planes = None
        if grid.architecture is not None:
            self._materialize_on_device(h)

    def _materialize_on_device(self, h):
        """the planes the kernels read, by ocn_immersed_compute_bottom: bottom height, kbot (int32), Hᶜᶜ, Hᶠᶜ, Hᶜᶠ, shaped like η with halos"""
        from .architectures import on_architecture, stream_ptr
        g = self.underlying_grid
        dev = device(child_architecture(g.architecture))
        shape = (g.Ny + 2 * g.Hy, g.Nx + 2 * g.Hx)
        hp = torch.zeros(shape, dtype=torch.float64, device=dev)
        hp[g.Hy:g.Hy + g.Ny, g.Hx:g.Hx + g.Nx] = on_architecture(g.architecture, np.ascontiguousarray(h.T))
        zc = on_architecture(g.architecture, np.ascontiguousarray(g.nodes_1d(2, False)))
        zf = on_architecture(g.architecture, np.ascontiguousarray(g.nodes_1d(2, True)))
        P = {n: torch.zeros(shape, dtype=torch.float64, device=dev) for n in ("bottom", "Hcc", "Hfc", "Hcf")}
        P["kbot"] = torch.zeros(shape, dtype=torch.int32, device=dev)
        interface = int(isinstance(self.immersed_boundary.immersed_condition, InterfaceImmersedCondition))
        _lib.call("ocn_immersed_compute_bottom", g.cref, interface, hp.data_ptr(), zc.data_ptr(), zf.data_ptr(), P["bottom"].data_ptr(),
                  P["kbot"].data_ptr(), P["Hcc"].data_ptr(), P["Hfc"].data_ptr(), P["Hcf"].data_ptr(), stream_ptr())
        self._planes = P

    def __getattr__(self, name):
        if name in ("underlying_grid", "__setstate__", "__deepcopy__"):
            raise AttributeError(name)
        return getattr(self.underlying_grid, name)

    def plane_ptr(self, name):
        """device pointer of the plane "kbot", "bottom", "Hcc", "Hfc" or "Hcf" """
        if self._planes is None:
            raise RuntimeError("this ImmersedBoundaryGrid holds metadata only (architecture = None)")
        return self._planes[name].data_ptr()

    def with_halo(self, new_halo):
        """with_halo(halo, ibg) (immersed_boundary_grid.jl:69-76): the underlying grid rebuilt with the new halo, the materialized boundary
        carried along and materialized again on it"""
        return ImmersedBoundaryGrid(self.underlying_grid.with_halo(new_halo), self.immersed_boundary)

    def with_math_mode(self, mode):
        import copy
        g = copy.copy(self)
        g.underlying_grid = self.underlying_grid.with_math_mode(mode)
        return g

    def __repr__(self):
        return (f"{self.Nx}x{self.Ny}x{self.Nz} ImmersedBoundaryGrid on {self.architecture} with {self.Hx}x{self.Hy}x{self.Hz} halo, "
                f"{self.immersed_boundary!r}")


def _require_immersed(grid, who):
    if not isinstance(grid, ImmersedBoundaryGrid):
        raise TypeError(f"{who} needs an ImmersedBoundaryGrid")


def immersed_cell(grid):
    """immersed_cell(i, j, k, ibg) (grid_fitted_bottom.jl:124-130) as a boolean (Nx, Ny, Nz) array"""
    _require_immersed(grid, "immersed_cell")
    return np.arange(1, grid.Nz + 1)[None, None, :] <= grid.kbot[:, :, None]


def static_column_depth(grid, location="cc"):
    """static_column_depthᶜᶜᵃ / ᶠᶜᵃ / ᶜᶠᵃ (grid_fitted_bottom.jl:147-150) as an (Nx, Ny) array: z_top - bottom_height at "cc", the minimum
    over the two columns of the face at "fc" and "cf" """
    _require_immersed(grid, "static_column_depth")
    if location not in ("cc", "fc", "cf"):
        raise ValueError('location must be "cc", "fc" or "cf"')
    return grid._depth[location].copy()


def _node_predicate(grid, loc, kbot_halo, any_cell):
    """inactive_node (any_cell = False: AND over the cells the node touches) or peripheral_node (True: OR) at location `loc` (bit 0 / 1 /
    2: Face in x / y / z) for i = 1..Nx, j = 1..Ny, k = 1..Nz (+ 1 at a z Face), on a grid whose columns hold kbot_halo immersed cells.
    inactive_cell (immersed, or outside 1..Nz) is monotone in kbot, so the AND is the predicate at the minimum of kbot over the columns
    and the OR the one at the maximum (Grids/inactive_node.jl:127-155)."""
    Nx, Ny, Nz, Hx, Hy = grid.Nx, grid.Ny, grid.Nz, grid.Hx, grid.Hy
    pick = np.maximum if any_cell else np.minimum
    m = kbot_halo[Hx:Hx + Nx, Hy:Hy + Ny]
    if loc & 1:
        m = pick(m, kbot_halo[Hx - 1:Hx + Nx - 1, Hy:Hy + Ny])
    if loc & 2:
        m = pick(m, kbot_halo[Hx:Hx + Nx, Hy - 1:Hy + Ny - 1])
        if loc & 1:
            m = pick(m, pick(kbot_halo[Hx - 1:Hx + Nx - 1, Hy - 1:Hy + Ny - 1], kbot_halo[Hx - 1:Hx + Nx - 1, Hy:Hy + Ny]))
    k = np.arange(1, Nz + (2 if loc & 4 else 1))[None, None, :]
    cell = lambda kk: (kk < 1) | (kk > Nz) | (kk <= m[:, :, None])
    if not loc & 4:
        return cell(k)
    return (cell(k - 1) | cell(k)) if any_cell else (cell(k - 1) & cell(k))


def inactive_node(grid, loc):
    """inactive_node(i, j, k, grid, LX, LY, LZ) as a boolean array (see _node_predicate for the index ranges)"""
    _require_immersed(grid, "inactive_node")
    return _node_predicate(grid, loc, grid._kbot_halo, False)


def peripheral_node(grid, loc):
    _require_immersed(grid, "peripheral_node")
    return _node_predicate(grid, loc, grid._kbot_halo, True)


def immersed_inactive_node(grid, loc):
    """inactive_node(ibg) & !inactive_node(underlying grid) (immersed_boundary_interface.jl:53-60)"""
    _require_immersed(grid, "immersed_inactive_node")
    return _node_predicate(grid, loc, grid._kbot_halo, False) & ~_node_predicate(grid, loc, np.zeros_like(grid._kbot_halo), False)


def immersed_peripheral_node(grid, loc):
    _require_immersed(grid, "immersed_peripheral_node")
    return _node_predicate(grid, loc, grid._kbot_halo, True) & ~_node_predicate(grid, loc, np.zeros_like(grid._kbot_halo), True)
