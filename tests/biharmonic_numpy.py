"""HorizontalScalarBiharmonicDiffusivity (ScalarBiharmonicDiffusivity{HorizontalFormulation}, constant ν and κ) restated in NumPy, operator
for operator and in the reference's order of operations, on parent arrays indexed [i, j, k] with halos (Field.parent()), for a grid that is
Periodic and regular in x and y (the biharmonic masks are identities there):

  ∇²hᶜᶜᶜ, ∇²hᶠᶜᶜ, ∇²hᶜᶠᶜ                    Operators/laplacian_operators.jl:5-18
  δ★ᶜᶜᶜ, ζ★ᶠᶠᶜ, ∂x_∇²h_cᶠᶜᶜ, ∂y_∇²h_cᶜᶠᶜ    abstract_scalar_biharmonic_diffusivity_closure.jl:75-102
  viscous_flux_ux / vx / uy / vy, diffusive_flux_x / y    :46-51, :66-67 (ν_σ, κ_σ: abstract_scalar_diffusivity_closure.jl:158-159, 267-268)
  ∂ⱼ_τ₁ⱼ, ∂ⱼ_τ₂ⱼ, ∇_dot_qᶜ                  closure_kernel_operators.jl:22-34, 43-48 (no z flux: the formulation has none, the generic zero)

Every operator is a function of an index shift (a, b): its value at (i + a, j + b, k) for all interior (i, j, k) at once, so an operator
nested in a difference is written as the reference nests it.  The grid description is tests/implicit_diffusion_numpy.py's `describe`.
The functions return the TERMS (a_u, a_v, [a_c, ...]) over (1..Nx, 1..Ny, 1..Nz): the tendencies are G - a, or G - (a + b) with the
term b of a tuple's other closure.

Rounded operations on the longest path from a loaded value to a term (the same for a_u, a_v, a_c), counted below as (n):
  ∇²h:  δ (1)  / Δ (2)  Ax * (3)  δx (4)  + δy part (5)  1/V * (6);   δ★ or the flux:  Δy * (7)  δ (8)  + (9)  1/Az * (10)  ν * (11);
  divergence:  Ax * (12)  δ (13)  + (14)  + 0 (exact)  1/V * (15)                                                  -> 15 on the data
  metrics entering those products: Ax (1), 1/V (3: Az, Az Δz, the reciprocal) in ∇²h; 1/Az (2); Ax (1), 1/V (3) in the divergence -> 10
so C = 25 rounded operations; OPERATIONS = 32 leaves 7 for the rounding of the inputs and of a closed form they are compared with."""
import numpy as np

import implicit_diffusion_numpy as IDN

_dzC = IDN._dzC
EPS = IDN.EPS
OPERATIONS = 32


def _shift(g, f):
    """f(a, b) = f[i + a, j + b, k] over the interior"""
    return lambda a, b: f[g.Hx + a:g.Hx + a + g.Nx, g.Hy + b:g.Hy + b + g.Ny, g.Hz:g.Hz + g.Nz]


class _Metrics:
    def __init__(self, g):
        if g.topo[0] != "Periodic" or g.topo[1] != "Periodic":
            raise ValueError("the restatement covers grids that are Periodic in x and y")
        self.dx, self.dy = g.dx, g.dy
        dz = _dzC(g, 0)                # Δzᵃᵃᶜ of the cell's own plane
        self.Az = g.dx * g.dy          # Azᶜᶜᶜ = Azᶠᶜᶜ = Azᶜᶠᶜ = Azᶠᶠᶜ on a regular x and y
        self.Ax = g.dy * dz            # Δy Δz
        self.Ay = g.dx * dz            # Δx Δz
        self.V = self.Az * dz


def laplacian_h(g, f):
    """∇²h of a field at (c, c, c), (f, c, c) or (c, f, c): 1 / V * (δx(Ax ∂x f) + δy(Ay ∂y f)).  On a regular Periodic grid the three
    locations index alike: the inner derivative sits half a cell before / behind the outer difference either way."""
    m, F = _Metrics(g), _shift(g, f)
    Ax_dx = lambda a, b: m.Ax * ((F(a + 1, b) - F(a, b)) / m.dx)   # Ax ∂x at the point between a and a + 1
    Ay_dy = lambda a, b: m.Ay * ((F(a, b + 1) - F(a, b)) / m.dy)
    return lambda a, b: 1 / m.V * ((Ax_dx(a, b) - Ax_dx(a - 1, b)) + (Ay_dy(a, b) - Ay_dy(a, b - 1)))


def momentum_terms(g, nu, u, v):
    """(∂ⱼτ₁ⱼ, ∂ⱼτ₂ⱼ) over the interior"""
    m = _Metrics(g)
    Lu, Lv = laplacian_h(g, u), laplacian_h(g, v)
    # δ★ᶜᶜᶜ = 1 / Az * (δxᶜ(Δy ∇²hᶠᶜᶜ u) + δyᶜ(Δx ∇²hᶜᶠᶜ v)): a centre lies between faces a and a + 1
    dstar = lambda a, b: 1 / m.Az * ((m.dy * Lu(a + 1, b) - m.dy * Lu(a, b)) + (m.dx * Lv(a, b + 1) - m.dx * Lv(a, b)))
    # ζ★ᶠᶠᶜ = 1 / Az * (δxᶠ(Δy ∇²hᶜᶠᶜ v) - δyᶠ(Δx ∇²hᶠᶜᶜ u)): a face lies between centres a - 1 and a
    zstar = lambda a, b: 1 / m.Az * ((m.dy * Lv(a, b) - m.dy * Lv(a - 1, b)) - (m.dx * Lu(a, b) - m.dx * Lu(a, b - 1)))
    flux_ux = lambda a, b: nu * dstar(a, b)       # (c, c, c)
    flux_vy = flux_ux
    flux_vx = lambda a, b: nu * zstar(a, b)       # (f, f, c)
    flux_uy = lambda a, b: -(nu * zstar(a, b))
    zero = 0.0  # δz(Az viscous_flux_uz) with the generic zero flux: Az 0 - Az 0
    a_u = 1 / m.V * (((m.Ax * flux_ux(0, 0) - m.Ax * flux_ux(-1, 0)) + (m.Ay * flux_uy(0, 1) - m.Ay * flux_uy(0, 0))) + zero)
    a_v = 1 / m.V * (((m.Ax * flux_vx(1, 0) - m.Ax * flux_vx(0, 0)) + (m.Ay * flux_vy(0, 0) - m.Ay * flux_vy(0, -1))) + zero)
    return a_u, a_v


def tracer_term(g, kappa, c):
    """∇_dot_qᶜ over the interior"""
    m = _Metrics(g)
    Lc = laplacian_h(g, c)
    # ∂x_∇²h_cᶠᶜᶜ = 1 / Az * δxᶠ(Δy ∇²hᶜᶜᶜ c),  ∂y_∇²h_cᶜᶠᶜ = 1 / Az * δyᶠ(Δx ∇²hᶜᶜᶜ c)
    flux_x = lambda a, b: kappa * (1 / m.Az * (m.dy * Lc(a, b) - m.dy * Lc(a - 1, b)))
    flux_y = lambda a, b: kappa * (1 / m.Az * (m.dx * Lc(a, b) - m.dx * Lc(a, b - 1)))
    return 1 / m.V * (((m.Ax * flux_x(1, 0) - m.Ax * flux_x(0, 0)) + (m.Ay * flux_y(0, 1) - m.Ay * flux_y(0, 0))) + 0.0)


def terms(g, nu, u, v, kappas, tracers):
    """(a_u, a_v, [a_c, ...]); u = None: no momentum part"""
    a_u, a_v = momentum_terms(g, nu, u, v) if u is not None else (None, None)
    return a_u, a_v, [tracer_term(g, k, c) for k, c in zip(kappas, tracers)]


def interior(g):
    return (slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny), slice(g.Hz, g.Hz + g.Nz))


def subtract(g, G, a, b=None):
    """a copy of the parent G with G - a, or G - (a + b), over the interior"""
    out = np.array(G, dtype=np.float64)
    sl = interior(g)
    out[sl] = out[sl] - (a if b is None else (a + b))
    return out


def volumes(g):
    return (g.dx * g.dy) * _dzC(g, 0) + np.zeros((g.Nx, g.Ny, g.Nz))


def eigenvalue(g, m, n):
    """λ of -∇²h on the mode cos(2π m x / Lx) cos(2π n y / Ly) of a uniform Periodic grid: the biharmonic term of that mode is ν λ² times it"""
    return 4 / g.dx ** 2 * np.sin(np.pi * m / g.Nx) ** 2 + 4 / g.dy ** 2 * np.sin(np.pi * n / g.Ny) ** 2


def bound(g, coefficient, amplitude):
    """OPERATIONS eps ν (4 / Δx² + 4 / Δy²)² max|u|: every rounded operation errs by at most eps times a value that the remaining (linear)
    operators amplify to at most the operator norm times the largest input"""
    return OPERATIONS * EPS * coefficient * (4 / g.dx ** 2 + 4 / g.dy ** 2) ** 2 * amplitude
