"""Solvers: mirrors src/Solvers/Solvers.jl:3-8 -- FFTBasedPoissonSolver, FourierTridiagonalPoissonSolver,
BatchedTridiagonalSolver, solve! -- on top of libocn_hip's rocFFT-based handle."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .architectures import on_architecture, stream_ptr
from .grids import Bounded, Flat, Periodic


class XDirection:
    """the tridiagonal direction of a BatchedTridiagonalSolver / FourierTridiagonalPoissonSolver (Solvers.jl)"""
    dim = 0


class YDirection:
    dim = 1


class ZDirection:
    dim = 2


def _direction_dim(direction):
    d = getattr(direction, "dim", None)
    if d not in (0, 1, 2):
        raise ValueError(f"tridiagonal_direction must be XDirection(), YDirection() or ZDirection(), got {direction!r}")
    return d


def stretched_direction(grid):
    """stretched_direction (fourier_tridiagonal_poisson_solver.jl:53-55): YZRegularRG -> XDirection, XZRegularRG -> YDirection, otherwise
    ZDirection"""
    dims = grid.stretched_dimensions
    if len(dims) > 1:
        raise NotImplementedError(f"a grid stretched in {' and '.join('xyz'[d] for d in dims)}: the Fourier-tridiagonal solver needs "
                                  "two regular directions")
    return (XDirection, YDirection, ZDirection)[dims[0] if dims else 2]()


class _PoissonHandle:
    def __init__(self, grid, stretched_dim=None):
        self.grid = grid
        self._h = C.c_void_p()
        if stretched_dim is None:
            _lib.call("ocn_poisson_create", C.byref(self._h), grid.cref)
        else:
            n = "xy"[stretched_dim]
            dc, df = getattr(grid, f"_d{n}c"), getattr(grid, f"_d{n}f")
            _lib.call("ocn_poisson_create_stretched", C.byref(self._h), grid.cref, stretched_dim, dc.data_ptr(), df.data_ptr())

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                _lib.lib().ocn_poisson_destroy(h)
            except Exception:
                pass
            self._h = None

    def info(self):
        k, r, d = C.c_int32(), C.c_int32(), C.c_int32()
        _lib.call("ocn_poisson_info", self._h, C.byref(k), C.byref(r), C.byref(d))
        return {"kind": k.value, "r2c": bool(r.value), "direct_out": d.value, "fused_z": bool(d.value & 2), "dct_z": bool(d.value & 8)}

    def passes(self):
        """The handle's three pass lists (ocn_poisson_describe): (source, set_source, solve), each a list of strings
        `PassName(d=…,mode=…,n=a×b×c)` in the order the executor walks them."""
        buf = C.create_string_buffer(4096)
        _lib.call("ocn_poisson_describe", self._h, buf, len(buf))
        lists = {}
        for line in buf.value.decode("utf-8").splitlines():
            name, _, items = line.partition(":")
            lists[name] = items.split()
        return lists["source"], lists["set_source"], lists["solve"]

    def compute_source_term(self, u, v, w, dt):
        """compute_source_term!(pressure, solver, Δt, Ũ) (solve_for_pressure.jl:57-76)"""
        _lib.call("ocn_poisson_compute_source_term", self._h, u.ptr, v.ptr, w.ptr, float(dt), stream_ptr())

    def set_source_term(self, R):
        """R: halo-free array [i, j, k] (numpy) or tensor [k, j, i]."""
        g = self.grid
        if not isinstance(R, torch.Tensor):
            R = on_architecture(g.architecture, np.ascontiguousarray(np.asarray(R, dtype=np.float64).T))
        if tuple(R.shape) != (g.Nz, g.Ny, g.Nx):
            raise ValueError(f"source term shape {tuple(R.shape)} != {(g.Nz, g.Ny, g.Nx)}")
        R = R.contiguous()
        _lib.call("ocn_poisson_set_source_term", self._h, R.data_ptr(), stream_ptr())
        torch.cuda.current_stream().synchronize()  # R may be a temporary

    def solve(self, phi):
        """solve!(ϕ, solver): ϕ is a Center field whose interior receives the solution."""
        _lib.call("ocn_poisson_solve", self._h, phi.ptr, stream_ptr())
        return phi


class FFTBasedPoissonSolver(_PoissonHandle):
    """src/Solvers/fft_based_poisson_solver.jl:52-125.  (Periodic, Periodic, Periodic | Flat): the FFT pipelines of csrc/poisson.hip; any
    topology with a Bounded x or y (regular spacings): the general solver, cosine transforms along the Bounded dimensions
    (plan_transforms.jl:16-34; `general=True` forces it for the other regular topologies, Bounded z included)."""

    def __init__(self, grid, general=False):
        import os
        bounded_xy = Bounded in grid.topology[:2] or Flat in grid.topology[:2]  # (the library routes every non-Periodic x / y to the general solver)
        if grid.stretched_dimensions:
            raise ValueError("FFTBasedPoissonSolver requires a regular grid")
        if grid.topology[2] == Bounded and not (bounded_xy or general):
            raise NotImplementedError("(Periodic, Periodic, Bounded): FourierTridiagonalPoissonSolver in this backend (an exact solver of the "
                                      "same system); FFTBasedPoissonSolver(grid, general=True) selects the cosine-transform solver")
        if general and not bounded_xy:
            old = os.environ.get("OCN_POISSON_GENERAL")
            os.environ["OCN_POISSON_GENERAL"] = "1"
            try:
                super().__init__(grid)
            finally:
                if old is None:
                    os.environ.pop("OCN_POISSON_GENERAL")
                else:
                    os.environ["OCN_POISSON_GENERAL"] = old
        else:
            super().__init__(grid)


class FourierTridiagonalPoissonSolver(_PoissonHandle):
    """src/Solvers/fourier_tridiagonal_poisson_solver.jl:82-147.  The tridiagonal direction is the stretched one (stretched_direction):
    z (Bounded, regular or stretched) with x and y regular (XYRegularRG), or a stretched Bounded x (YZRegularRG) / y (XZRegularRG) with the
    other two regular; the regular directions are transformed with any topology: Periodic -> Fourier, Bounded -> cosine transforms,
    Flat -> none."""

    def __init__(self, grid):
        import os
        t = stretched_direction(grid).dim
        if grid.topology[t] != Bounded:
            raise ValueError("`FourierTridiagonalPoissonSolver` can only be used when the stretched direction's topology is `Bounded`.")
        if t != 2:
            super().__init__(grid, stretched_dim=t)
            return
        if grid.topology[2] != Bounded:
            raise ValueError("`FourierTridiagonalPoissonSolver` can only be used when the stretched direction's topology is `Bounded`.")
        if (Bounded in grid.topology[:2] or Flat in grid.topology[:2]) and grid._dzc is None:
            # a regular z next to walls in x / y: the library would pick the cosine-transform solver; ask for the Thomas sweep
            old = os.environ.get("OCN_POISSON_GENERAL_TRI")
            os.environ["OCN_POISSON_GENERAL_TRI"] = "1"
            try:
                super().__init__(grid)
            finally:
                if old is None:
                    os.environ.pop("OCN_POISSON_GENERAL_TRI")
                else:
                    os.environ["OCN_POISSON_GENERAL_TRI"] = old
        else:
            super().__init__(grid)


def nonhydrostatic_pressure_solver(grid):
    """src/Models/NonhydrostaticModels/NonhydrostaticModels.jl:25-62"""
    hook = getattr(grid.architecture, "pressure_solver", None)
    if hook is not None:
        return hook(grid)
    if any(d < 2 for d in grid.stretched_dimensions):  # YZRegularRG / XZRegularRG: GridWithFourierTridiagonalSolver (Solvers.jl:51-52)
        return FourierTridiagonalPoissonSolver(grid)
    if Bounded in grid.topology[:2] or Flat in grid.topology[:2]:
        if grid._dzc is not None:  # XYRegularRG with a stretched z: GridWithFourierTridiagonalSolver (Solvers.jl:51-52)
            return FourierTridiagonalPoissonSolver(grid)
        return FFTBasedPoissonSolver(grid)  # XYZRegularRG (NonhydrostaticModels.jl:25-62)
    if grid.topology[2] == Bounded:
        return FourierTridiagonalPoissonSolver(grid)
    return FFTBasedPoissonSolver(grid)


class BatchedTridiagonalSolver:
    """BatchedTridiagonalSolver(grid; lower_diagonal, diagonal, upper_diagonal, tridiagonal_direction)
    (src/Solvers/batched_tridiagonal_solver.jl:11-79).  a, c: (N-1,) along the tridiagonal direction (ZDirection by default); b: [i,j,k]
    real, or 1-D (N,) along that direction -- the same diagonal for every line, broadcast on the host over the batch of the first rhs."""

    def __init__(self, arch, lower_diagonal, diagonal, upper_diagonal, tridiagonal_direction=None):
        self.dim = 2 if tridiagonal_direction is None else _direction_dim(tridiagonal_direction)
        self.arch = arch
        self.a = on_architecture(arch, np.ascontiguousarray(lower_diagonal, dtype=np.float64))
        self.c = on_architecture(arch, np.ascontiguousarray(upper_diagonal, dtype=np.float64))
        b = np.asarray(diagonal, dtype=np.float64)
        self._b1 = None
        if b.ndim == 1:
            self._b1 = b
            self.b = self.t = None
        else:
            self._set_diagonal(b)

    def _set_diagonal(self, b):
        self.Nx, self.Ny, self.Nz = b.shape
        n = b.shape[self.dim]
        if self.a.numel() != n - 1 or self.c.numel() != n - 1:
            raise ValueError(f"lower / upper diagonals must have {n - 1} elements along {'xyz'[self.dim]}")
        self.b = on_architecture(self.arch, np.ascontiguousarray(b.T))
        self.t = torch.zeros_like(self.b)

    def solve(self, rhs, phi0=None):
        """solve!(ϕ, solver, rhs): rhs complex [i,j,k]; returns complex [i,j,k] (host)."""
        rhs = np.asarray(rhs, dtype=np.complex128)
        if self.b is None:
            shape = [1, 1, 1]
            shape[self.dim] = self._b1.size
            self._set_diagonal(np.broadcast_to(self._b1.reshape(shape), rhs.shape))
        if rhs.shape != (self.Nx, self.Ny, self.Nz):
            raise ValueError(f"rhs shape {rhs.shape} != {(self.Nx, self.Ny, self.Nz)}")
        f = np.ascontiguousarray(rhs.T)
        fd = on_architecture(self.arch, f.view(np.float64))
        if phi0 is None:
            phi = torch.zeros_like(fd)
        else:
            phi = on_architecture(self.arch, np.ascontiguousarray(np.asarray(phi0, dtype=np.complex128).T).view(np.float64))
        _lib.call("ocn_batched_tridiagonal_solve_" + "xyz"[self.dim], self.Nx, self.Ny, self.Nz, self.a.data_ptr(), self.b.data_ptr(),
                  self.c.data_ptr(), fd.data_ptr(), self.t.data_ptr(), phi.data_ptr(), stream_ptr())
        out = phi.cpu().numpy().view(np.complex128)
        return out.T


def solve(phi, solver, *args):
    """solve!(ϕ, solver, ...)"""
    return solver.solve(phi, *args)
