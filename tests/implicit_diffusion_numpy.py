"""ScalarDiffusivity(VerticallyImplicitTimeDiscretization(), ν, κ) restated in NumPy, operand for operand, on parent arrays indexed
[i, j, k] with halos (Field.parent()):

  explicit part of the closure term     abstract_scalar_diffusivity_closure.jl:214-260 with the flux divergences of
                                        closure_kernel_operators.jl:27-53 (∂ⱼτ₁ⱼ, ∂ⱼτ₂ⱼ, ∂ⱼτ₃ⱼ, ∇_dot_qᶜ)
  ivd_upper / lower_diagonal, ivd_diagonal   vertically_implicit_diffusion_solver.jl:55-110
  solve_batched_tridiagonal_system_z!   Solvers/batched_tridiagonal_solver.jl

Written from those files; tests/test_host_implicit_diffusion.py pins the solve against numpy.linalg.solve of the dense matrix and the
Center rows against conservation.  A difference or flux along a Flat direction is 0."""
from types import SimpleNamespace

import numpy as np

EPS = np.finfo(np.float64).eps


def describe(grid):
    """what the restatement reads of a package grid: sizes, halos, topology, Δx, Δy and Δzᵃᵃᶜ / Δzᵃᵃᶠ with halos (element 0 <-> k = 1 - Hz)"""
    n = grid.Nz + 2 * grid.Hz
    if getattr(grid, "_dzc_host", None) is not None:
        dzc, dzf = np.array(grid._dzc_host, dtype=np.float64), np.array(grid._dzf_host, dtype=np.float64)
    else:
        dzc, dzf = np.full(n, float(grid.dz)), np.full(n, float(grid.dz))
    return SimpleNamespace(Nx=grid.Nx, Ny=grid.Ny, Nz=grid.Nz, Hx=grid.Hx, Hy=grid.Hy, Hz=grid.Hz, topo=tuple(str(t) for t in grid.topology),
                           dx=float(grid.dx), dy=float(grid.dy), dzc=dzc, dzf=dzf)


def column_grid(dzc, dzf, Hz):
    """a description that holds the vertical spacings only (coefficient assembly)"""
    dzc, dzf = np.asarray(dzc, dtype=np.float64), np.asarray(dzf, dtype=np.float64)
    return SimpleNamespace(Nz=dzc.size - 2 * Hz, Hz=Hz, dzc=dzc, dzf=dzf)


# ---------------------------------------------------------------------------------------------------------------------------------
# the explicit part of the closure term
# ---------------------------------------------------------------------------------------------------------------------------------
def _sh(g, a, di, dj, dk):
    """a[i + di, j + dj, k + dk] for (i, j, k) = (1..Nx, 1..Ny, 1..Nz)"""
    return a[g.Hx + di:g.Hx + di + g.Nx, g.Hy + dj:g.Hy + dj + g.Ny, g.Hz + dk:g.Hz + dk + g.Nz]


def _dzC(g, dk):
    return g.dzc[g.Hz + dk:g.Hz + dk + g.Nz].reshape(1, 1, -1)


def _dzF(g, dk):
    return g.dzf[g.Hz + dk:g.Hz + dk + g.Nz].reshape(1, 1, -1)


def _boundary(g, dk):
    """(k == 1) | (k == Nz + 1) at levels k + dk, k = 1..Nz"""
    k = np.arange(1, g.Nz + 1) + dk
    return ((k == 1) | (k == g.Nz + 1)).reshape(1, 1, -1)


def momentum_explicit_part(g, nu, u, v, w, all_explicit=False):
    """(Du, Dv, Dw) over (1..Nx, 1..Ny, 1..Nz): the explicit part of ∂ⱼτᵢⱼ; the tendencies are G - D.
    all_explicit: every flux explicit (the ExplicitTimeDiscretization closure), for the splitting identity"""
    bnd = (lambda c: np.ones((1, 1, g.Nz), dtype=bool)) if all_explicit else (lambda c: _boundary(g, c))
    fx, fy = g.topo[0] == "Flat", g.topo[1] == "Flat"
    dx, dy = g.dx, g.dy
    zero = np.zeros((g.Nx, g.Ny, g.Nz))
    U = lambda a, b, c: _sh(g, u, a, b, c)
    V = lambda a, b, c: _sh(g, v, a, b, c)
    W = lambda a, b, c: _sh(g, w, a, b, c)
    dxu = lambda a, b, c: zero if fx else (U(a + 1, b, c) - U(a, b, c)) / dx
    dyv = lambda a, b, c: zero if fy else (V(a, b + 1, c) - V(a, b, c)) / dy
    dzw = lambda a, b, c: (W(a, b, c + 1) - W(a, b, c)) / _dzC(g, c)
    dyu = lambda a, b, c: zero if fy else (U(a, b, c) - U(a, b - 1, c)) / dy
    dxv = lambda a, b, c: zero if fx else (V(a, b, c) - V(a - 1, b, c)) / dx
    dzu = lambda a, b, c: (U(a, b, c) - U(a, b, c - 1)) / _dzF(g, c)
    dxw = lambda a, b, c: zero if fx else (W(a, b, c) - W(a - 1, b, c)) / dx
    dzv = lambda a, b, c: (V(a, b, c) - V(a, b, c - 1)) / _dzF(g, c)
    dyw = lambda a, b, c: zero if fy else (W(a, b, c) - W(a, b - 1, c)) / dy
    t11 = lambda a, b, c: -2 * (nu * dxu(a, b, c))
    t22 = lambda a, b, c: -2 * (nu * dyv(a, b, c))
    t12 = lambda a, b, c: -2 * (nu * (0.5 * (dyu(a, b, c) + dxv(a, b, c))))
    e13 = lambda a, b, c: -2 * (nu * (0.5 * (dzu(a, b, c) + dxw(a, b, c))))   # the explicit fluxes
    e23 = lambda a, b, c: -2 * (nu * (0.5 * (dzv(a, b, c) + dyw(a, b, c))))
    e33 = lambda a, b, c: -2 * (nu * dzw(a, b, c))
    # viscous_flux_uz / vz / wz(::VerticallyBoundedGrid, ::VITD)
    t13 = lambda a, b, c: np.where(bnd(c), e13(a, b, c), -(nu * dxw(a, b, c)))
    t23 = lambda a, b, c: np.where(bnd(c), e23(a, b, c), -(nu * dyw(a, b, c)))
    t33 = lambda a, b, c: np.where(bnd(c), e33(a, b, c), 0.0)
    Az = dx * dy
    dzc, dzf = _dzC(g, 0), _dzF(g, 0)
    Axc, Ayc = dy * dzc, dx * dzc
    Axf, Ayf = dy * dzf, dx * dzf
    # u
    dxF = 0.0 if fx else Axc * t11(0, 0, 0) - Axc * t11(-1, 0, 0)
    dyF = 0.0 if fy else Ayc * t12(0, 1, 0) - Ayc * t12(0, 0, 0)
    dzF = Az * t13(0, 0, 1) - Az * t13(0, 0, 0)
    Du = 1 / (Az * dzc) * ((dxF + dyF) + dzF)
    # v
    dxF = 0.0 if fx else Axc * t12(1, 0, 0) - Axc * t12(0, 0, 0)
    dyF = 0.0 if fy else Ayc * t22(0, 0, 0) - Ayc * t22(0, -1, 0)
    dzF = Az * t23(0, 0, 1) - Az * t23(0, 0, 0)
    Dv = 1 / (Az * dzc) * ((dxF + dyF) + dzF)
    # w: the x / y fluxes stay the explicit ones
    dxF = 0.0 if fx else Axf * e13(1, 0, 0) - Axf * e13(0, 0, 0)
    dyF = 0.0 if fy else Ayf * e23(0, 1, 0) - Ayf * e23(0, 0, 0)
    dzF = Az * t33(0, 0, 0) - Az * t33(0, 0, -1)
    Dw = 1 / (Az * dzf) * ((dxF + dyF) + dzF)
    return Du, Dv, Dw


def tracer_explicit_part(g, kappa, c, all_explicit=False):
    """D over (1..Nx, 1..Ny, 1..Nz): the explicit part of ∇_dot_qᶜ; Gc - D.  all_explicit: the ExplicitTimeDiscretization closure"""
    fx, fy = g.topo[0] == "Flat", g.topo[1] == "Flat"
    Cc = lambda a, b, d: _sh(g, c, a, b, d)
    qx = lambda a, b, d: -(kappa * ((Cc(a, b, d) - Cc(a - 1, b, d)) / g.dx))
    qy = lambda a, b, d: -(kappa * ((Cc(a, b, d) - Cc(a, b - 1, d)) / g.dy))
    qz_e = lambda a, b, d: -(kappa * ((Cc(a, b, d) - Cc(a, b, d - 1)) / _dzF(g, d)))
    qz = qz_e if all_explicit else (lambda a, b, d: np.where(_boundary(g, d), qz_e(a, b, d), 0.0))
    dzc = _dzC(g, 0)
    Ax, Ay, Az = g.dy * dzc, g.dx * dzc, g.dx * g.dy
    dxF = 0.0 if fx else Ax * qx(1, 0, 0) - Ax * qx(0, 0, 0)
    dyF = 0.0 if fy else Ay * qy(0, 1, 0) - Ay * qy(0, 0, 0)
    dzF = Az * qz(0, 0, 1) - Az * qz(0, 0, 0)
    return 1 / (Az * dzc) * ((dxF + dyF) + dzF)


def written_offsets(g, ranged=False):
    """first index written of Gu (in i), Gv (in j), Gw (in k): the excluded periphery of Face fields along Bounded directions"""
    if ranged:
        return 1, 1, 1
    return (2 if g.topo[0] == "Bounded" and g.Nx > 1 else 1, 2 if g.topo[1] == "Bounded" and g.Ny > 1 else 1, 2 if g.Nz > 1 else 1)


# ---------------------------------------------------------------------------------------------------------------------------------
# the implicit step
# ---------------------------------------------------------------------------------------------------------------------------------
def _dz_at(g, face, k):
    return float((g.dzf if face else g.dzc)[k + g.Hz - 1])


def upper_diagonal(g, zface, dt, kappa, k):
    if zface:  # ivd_upper_diagonal(..., ::Face, ...)
        du = -dt * kappa / (_dz_at(g, False, k) * _dz_at(g, True, k))
        return 0.0 if k < 1 else du
    du = -dt * kappa / (_dz_at(g, False, k) * _dz_at(g, True, k + 1))
    return 0.0 if k > g.Nz - 1 else du


def lower_diagonal(g, zface, dt, kappa, k):
    if k < 1:
        return 0.0
    if zface:  # k′ = k + 2: Δzᶜ(k′) Δzᶠ(k′ - 1)
        return -dt * kappa / (_dz_at(g, False, k + 2) * _dz_at(g, True, k + 1))
    return -dt * kappa / (_dz_at(g, False, k + 1) * _dz_at(g, True, k + 1))  # k = k′ + 1


def diagonals(g, zface, dt, kappa):
    """(a, b, c), element 0 <-> tridiagonal index 1: a[k-1] sits below the diagonal in row k+1, c[k-1] above it in row k (c[Nz-1] is not
    part of the Nz x Nz system: the solver never reads it); a[Nz-1] = 0 (never read either)"""
    Nz = g.Nz
    dt, kappa = float(dt), float(kappa)
    a, b, c = np.zeros(Nz), np.zeros(Nz), np.zeros(Nz)
    for k in range(1, Nz + 1):
        up = upper_diagonal(g, zface, dt, kappa, k)
        a[k - 1] = lower_diagonal(g, zface, dt, kappa, k) if k < Nz else 0.0
        b[k - 1] = (1.0 - up) - lower_diagonal(g, zface, dt, kappa, k - 1)
        c[k - 1] = up
    return a, b, c


def thomas(a, b, c, f):
    """solve_batched_tridiagonal_system_z! with the right-hand side in the solution array; f[..., k - 1], any leading shape"""
    phi = np.array(f, dtype=np.float64)
    Nz = phi.shape[-1]
    t = np.zeros(Nz)
    beta = b[0]
    phi[..., 0] = phi[..., 0] / beta
    for k in range(2, Nz + 1):
        t[k - 1] = c[k - 2] / beta
        beta = b[k - 1] - a[k - 2] * t[k - 1]
        star = (phi[..., k - 1] - a[k - 2] * phi[..., k - 2]) / beta
        if abs(beta) > 10 * EPS:
            phi[..., k - 1] = star
    for k in range(Nz - 1, 0, -1):
        phi[..., k - 1] = phi[..., k - 1] - t[k] * phi[..., k]
    return phi


def dense_matrix(a, b, c):
    Nz = b.size
    A = np.diag(b)
    for k in range(Nz - 1):
        A[k, k + 1] = c[k]
        A[k + 1, k] = a[k]
    return A


def apply_matrix(a, b, c, phi):
    """A φ along the last axis"""
    out = b * phi
    out[..., :-1] = out[..., :-1] + c[:-1] * phi[..., 1:]
    out[..., 1:] = out[..., 1:] + a[:-1] * phi[..., :-1]
    return out


def implicit_step(g, parent, loc, kappa, dt):
    """implicit_step!(field, ...): a copy of the parent array with columns i = 1..Nx, j = 1..Ny, rows k = 1..Nz solved"""
    a, b, c = diagonals(g, bool(loc & 4), dt, kappa)
    out = np.array(parent, dtype=np.float64)
    sl = (slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny), slice(g.Hz, g.Hz + g.Nz))
    out[sl] = thomas(a, b, c, out[sl])
    return out
