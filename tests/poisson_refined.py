"""A solution of the discrete Poisson problem of the pressure solvers that is exact to Float64 working precision: iterative refinement in
`np.longdouble` (64-bit mantissa, eps = 1.08e-19) around an ordinary Float64 direct solve.

    ϕ₀ = 0;   ϕ ← ϕ + S(R − Lϕ)   three times;   the gauge removed in long double after each step.

L is the operator the solvers invert, written with plain shifted slices in long double on the Float64 spacings of the grid: second
differences along every non-Flat direction, Periodic directions wrap, Bounded directions have a zero-gradient edge, a stretched z uses
Δzᶜ / Δzᶠ (∂z(∂zϕ) = [(ϕₖ₊₁ − ϕₖ) / Δzᶠₖ₊₁ − (ϕₖ − ϕₖ₋₁) / Δzᶠₖ] / Δzᶜₖ), and the screened form of `solve!(ϕ, solver, b, m)` is L + m.
The correction solver S is a Float64 solve: scipy.fft `fft` / `dct(type=2)` with the eigenvalues 4 sin²(πk/N)/Δ² (Periodic) and
4 sin²(πk/2N)/Δ² (Bounded) on a regular grid, the oracle's FourierTridiagonalPoissonSolver when z is stretched.  The gauge (m = 0 only) is
the zero mean both of the oracle's solvers produce.  S is accurate to ~1e-14, so the corrections are 1 (the first one is the solution),
≈1e-15 and ≈1e-18 of max|ϕ| and the result is the long-double solution of Lϕ = R to a few long-double eps times the conditioning.

Arrays are halo-free [i, j, k]; a Flat direction has extent 1.  Grids are oracle.Grid objects (they carry the Float64 spacings).

Error measures, both in units of the Float64 eps:
    forward   E = max|ϕ − ϕ*| / max|ϕ*|
    residual  r = max|R − Lϕ| / max|R|     (R and L in long double)
"""
import numpy as np
import scipy.fft as sfft

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
PERIODIC, BOUNDED, FLAT = 0, 1, 2
STEPS = 3

assert np.finfo(LD).eps < 1.1e-19, "np.longdouble has no extended precision on this platform"


class Operator:
    """L (+ m) of an oracle grid"""

    def __init__(self, og, m=0.0):
        self.og = og
        self.N = (og.Nx, og.Ny, og.Nz)
        self.topo = tuple(og.topo)
        self.m = float(m)
        self.d = [LD(og.dx), LD(og.dy), LD(og.dz)]
        self.stretched = og.dzc is not None
        if self.stretched:
            assert og.tz == BOUNDED
            H, Nz = og.Hz, og.Nz
            self.dzc = np.asarray(og.dzc[H:H + Nz], dtype=LD)           # Δzᶜ at centres k = 1 … Nz
            self.dzf = np.asarray(og.dzf[H + 1:H + Nz], dtype=LD)       # Δzᶠ at the interior faces k = 2 … Nz
        self._tri = None

    def _second_difference(self, phi, axis):
        N, t = self.N[axis], self.topo[axis]
        if t == FLAT:
            return None
        def at(a, s):  # a[..., s, ...] along `axis`
            return a[tuple(s if q == axis else slice(None) for q in range(3))]

        stretched = axis == 2 and self.stretched
        d = self.d[axis]
        out = np.zeros(phi.shape, dtype=LD)
        if N == 1:
            return out  # its own neighbour (Periodic) or between two zero-gradient edges (Bounded)
        # differences at the N − 1 interior faces, their differences, and ONE scaling by 1 / Δ² on a regular direction: every rounding
        # of this evaluation is noise in the residual that the refinement cannot get under
        flux = np.diff(phi, axis=axis)
        if stretched:
            flux /= self.dzf
        at(out, slice(1, -1))[...] = at(flux, slice(1, None)) - at(flux, slice(None, -1))
        at(out, 0)[...] = at(flux, 0)
        at(out, -1)[...] = -at(flux, -1)
        if t == PERIODIC:  # the face between cell N and cell 1
            edge = at(phi, 0) - at(phi, -1)
            at(out, 0)[...] -= edge
            at(out, -1)[...] += edge
        if stretched:
            out /= self.dzc
        else:
            out *= 1 / (d * d)
        return out

    def apply(self, phi):
        phi = np.asarray(phi, dtype=LD)
        out = LD(self.m) * phi if self.m != 0 else np.zeros(phi.shape, dtype=LD)
        for axis in range(3):
            t = self._second_difference(phi, axis)
            if t is not None:
                out += t
        return out

    # ---- the Float64 solve S
    def eigenvalues(self, axis):
        N, t = self.N[axis], self.topo[axis]
        k = np.arange(N, dtype=np.float64)
        d = float(self.d[axis])
        if t == PERIODIC:
            return 4 * np.sin(np.pi * k / N) ** 2 / d ** 2
        if t == BOUNDED:
            return 4 * np.sin(np.pi * k / (2 * N)) ** 2 / d ** 2
        return np.zeros(N)

    def solve64(self, R):
        """Float64 in, Float64 out: (L + m) ϕ = R, zero mean when m = 0"""
        R = np.ascontiguousarray(R, dtype=np.float64)
        if self.stretched:
            return self._solve64_tridiagonal(R)
        per = [a for a in range(3) if self.topo[a] == PERIODIC]
        bnd = [a for a in range(3) if self.topo[a] == BOUNDED]
        b = R
        for a in bnd:
            b = sfft.dct(b, type=2, axis=a)
        if per:
            b = sfft.fftn(b, axes=per)
        lam = (self.eigenvalues(0).reshape(-1, 1, 1) + self.eigenvalues(1).reshape(1, -1, 1)) + self.eigenvalues(2).reshape(1, 1, -1)
        with np.errstate(divide="ignore", invalid="ignore"):
            phi = -b / (lam - self.m)
        if self.m == 0:
            phi[0, 0, 0] = 0
        if per:
            phi = sfft.ifftn(phi, axes=per).real
        for a in bnd:
            phi = sfft.dct(phi, type=3, axis=a) * (1 / (2 * self.N[a]))
        return np.ascontiguousarray(phi, dtype=np.float64)

    def _solve64_tridiagonal(self, R):
        """The oracle's FourierTridiagonalPoissonSolver on R minus its horizontal mean, plus the horizontal-mean profile integrated
        directly (two cumulative sums).  That one column is the singular (kx, ky) = (0, 0) system: the Thomas sweep divides its last
        row by a pivot of rounding size, which is harmless for a solver (the constant it adds is the gauge) but adds a constant of
        arbitrary size to the column before the mean is removed, and a correction solver then converges at 1e-2 per step instead of
        1e-15."""
        assert self.m == 0
        from oracle import oracle as O
        if self._tri is None:
            self._tri = O.FourierTridiagonalPoissonSolver(self.og)
        profile = R.mean(axis=(0, 1))
        self._tri.set_source_term(np.asfortranarray(R - profile))
        p = self.og.zeros(0)
        self._tri.solve(p)
        dzc, dzf = self.dzc.astype(np.float64), self.dzf.astype(np.float64)
        flux = np.cumsum(profile * dzc)[:-1]                       # ∂zϕ at the interior faces (zero at the bottom)
        column = np.concatenate([[0.0], np.cumsum(flux * dzf)])
        phi = self.og.interior_N(p) + column
        return np.ascontiguousarray(phi - phi.mean())


def remove_gauge(op, phi):
    return phi - phi.mean(dtype=LD) if op.m == 0 else phi


def refine(op, R, steps=STEPS):
    """(ϕ* in long double, [max|correction| / max|ϕ| per step])"""
    R = np.asarray(R, dtype=LD)
    phi = np.zeros(R.shape, dtype=LD)
    sizes = []
    for _ in range(steps):
        res = R - op.apply(phi) if sizes else R
        delta = op.solve64(res.astype(np.float64))
        phi = remove_gauge(op, phi + delta.astype(LD))
        sizes.append(float(np.abs(delta).max() / np.abs(phi).max()))
    return phi, sizes


def divergence_ld(og, U, dt):
    """divᶜᶜᶜ(U) / Δt of Float64 parent arrays (halos filled) in long double"""
    Nx, Ny, Nz = og.Nx, og.Ny, og.Nz
    Hx, Hy, Hz = og.Hx, og.Hy, og.Hz
    u, v, w = U
    I, J, K = slice(Hx, Hx + Nx), slice(Hy, Hy + Ny), slice(Hz, Hz + Nz)
    out = np.zeros((Nx, Ny, Nz), dtype=LD)
    if og.tx != FLAT:
        out += (u[Hx + 1:Hx + Nx + 1, J, K].astype(LD) - u[I, J, K].astype(LD)) / LD(og.dx)
    if og.ty != FLAT:
        out += (v[I, Hy + 1:Hy + Ny + 1, K].astype(LD) - v[I, J, K].astype(LD)) / LD(og.dy)
    if og.tz != FLAT:
        dz = np.asarray(og.dzc[Hz:Hz + Nz], dtype=LD) if og.dzc is not None else LD(og.dz)
        out += (w[I, J, Hz + 1:Hz + Nz + 1].astype(LD) - w[I, J, K].astype(LD)) / dz
    return out / LD(dt)


def forward_error(phi, phi_star):
    """E in eps"""
    return float(np.abs(np.asarray(phi, dtype=LD) - phi_star).max() / np.abs(phi_star).max()) / EPS


def residual_error(op, R, phi):
    """r in eps"""
    R = np.asarray(R, dtype=LD)
    return float(np.abs(R - op.apply(phi)).max() / np.abs(R).max()) / EPS


# ---------------------------------------------------------------------------------------------------------------------------------
# A dense long-double solve for tiny shapes, independent of the slices above: analytic orthonormal eigenvector matrices of the 1-D
# operators (cosines of a Bounded direction, the real Fourier basis of a Periodic one), Gaussian elimination along a stretched z.
# ---------------------------------------------------------------------------------------------------------------------------------
def _pi():
    return LD(4) * np.arctan(LD(1))


def _eigenbasis(N, t, d):
    """(Q [N, N] orthonormal columns, eigenvalues of the second difference) in long double"""
    j = np.arange(N, dtype=LD).reshape(-1, 1)
    if t == FLAT:
        return np.ones((1, 1), dtype=LD), np.zeros(1, dtype=LD)
    pi = _pi()
    Q = np.zeros((N, N), dtype=LD)
    lam = np.zeros(N, dtype=LD)
    if t == BOUNDED:
        for k in range(N):
            q = np.cos(pi * k * (j[:, 0] + LD(1) / 2) / N)
            Q[:, k] = q / np.sqrt((q * q).sum())
            lam[k] = -4 * np.sin(pi * k / (2 * N)) ** 2 / d ** 2
        return Q, lam
    col = 0
    for k in range(N // 2 + 1):
        for f in (np.cos, np.sin):
            q = f(2 * pi * k * j[:, 0] / N)
            if (q * q).sum() < LD(1e-10):  # sin of k = 0 and of the Nyquist mode
                continue
            Q[:, col] = q / np.sqrt((q * q).sum())
            lam[col] = -4 * np.sin(pi * k / N) ** 2 / d ** 2
            col += 1
    assert col == N
    return Q, lam


def _gauss(A, b):
    """A x = b in long double, partial pivoting (numpy.linalg has no long double)"""
    A = np.array(A, dtype=LD)
    b = np.array(b, dtype=LD)
    n = len(b)
    for c in range(n):
        p = c + int(np.argmax(np.abs(A[c:, c])))
        if p != c:
            A[[c, p]] = A[[p, c]]
            b[[c, p]] = b[[p, c]]
        f = A[c + 1:, c] / A[c, c]
        A[c + 1:] -= f[:, None] * A[c]
        b[c + 1:] -= f * b[c]
    x = np.zeros(n, dtype=LD)
    for c in range(n - 1, -1, -1):
        x[c] = (b[c] - A[c, c + 1:] @ x[c + 1:]) / A[c, c]
    return x


def dense_solution(op, R):
    """(L + m) ϕ = R in long double by explicit eigenvector matrices; zero mean when m = 0"""
    R = np.asarray(R, dtype=LD)
    Nx, Ny, Nz = op.N
    Qx, lx = _eigenbasis(Nx, op.topo[0], op.d[0])
    Qy, ly = _eigenbasis(Ny, op.topo[1], op.d[1])
    m = LD(op.m)
    b = np.einsum("ia,jb,ijk->abk", Qx, Qy, R)
    if not op.stretched:
        Qz, lz = _eigenbasis(Nz, op.topo[2], op.d[2])
        b = np.einsum("kc,abk->abc", Qz, b)
        den = lx.reshape(-1, 1, 1) + ly.reshape(1, -1, 1) + lz.reshape(1, 1, -1) + m
        zero = op.m == 0
        if zero:
            den[0, 0, 0] = 1
        b = b / den
        if zero:
            b[0, 0, 0] = 0
        phi = np.einsum("kc,abc->abk", Qz, b)
    else:
        assert op.m == 0
        T = np.zeros((Nz, Nz), dtype=LD)
        for k in range(Nz):
            if k > 0:
                T[k, k - 1] += 1 / (op.dzf[k - 1] * op.dzc[k])
                T[k, k] -= 1 / (op.dzf[k - 1] * op.dzc[k])
            if k < Nz - 1:
                T[k, k + 1] += 1 / (op.dzf[k] * op.dzc[k])
                T[k, k] -= 1 / (op.dzf[k] * op.dzc[k])
        phi = np.zeros((Nx, Ny, Nz), dtype=LD)
        for a in range(Nx):
            for c in range(Ny):
                s = lx[a] + ly[c]
                if a == 0 and c == 0:  # singular: pin the first cell, the mean goes below
                    phi[a, c, 1:] = _gauss(T[1:, 1:], b[a, c, 1:])
                else:
                    phi[a, c] = _gauss(T + s * np.eye(Nz, dtype=LD), b[a, c])
    phi = np.einsum("ia,jb,abk->ijk", Qx, Qy, phi)
    return remove_gauge(op, phi)
