"""The upwinding vector-invariant momentum advection of the reference (VectorInvariant with WENO(order=5) sub-schemes, WENOVectorInvariant)
restated in NumPy, operator for operator and in the reference's order of operations, on parent arrays indexed [i, j, k] with halos
(Field.parent()), for a (Periodic, Periodic, Bounded) grid with regular x and y and a regular or stretched z:

  U_dot_∇u = horizontal_advection_U + vertical_advection_U + bernoulli_head_U        Advection/vector_invariant_advection.jl:269-275
  horizontal_advection_U / V, upwinding vorticity                                    :367-385
  vertical_advection_U / V, upwinding                                                :325-339
  upwinded_divergence_flux_Uᶠᶜᶜ / Vᶜᶠᶜ, bernoulli_head_U / V (OnlySelfUpwinding)    vector_invariant_self_upwinding.jl:5-83
  the conserving forms of each term                                                  vector_invariant_advection.jl:304-319, 360-361
  advective_momentum_flux_Wu / Wv                                                    upwind_biased_advective_fluxes.jl:39-45, 63-69
  WENO(order=5): stencils, smoothness, Z-WENO weights, reconstruction                weno_interpolants.jl:178-183, 341-363, 445-472, 508-554
  order reduction along the Bounded z                                                topologically_conditional_interpolation.jl:49-50, 103-125
  ζ₃ᶠᶠᶜ                                                                              Operators/vorticity_operators.jl:4-11

Every operator is a function of an index shift: its value at (i + a, j + b) of the plane k for all interior (i, j, k) at once, so an
operator nested in a reconstruction is written as the reference nests it.  A biased reconstruction takes the six stencil values and, apart
from them, the values its smoothness is measured on (one set for a FunctionStencil or the DefaultStencil, two for the VelocityStencil).
The coefficients come from oracle/coefficients.py; the grid description is tests/implicit_diffusion_numpy.py's `describe`.

`Scheme` names what the three sub-schemes are; the combinations the package accepts are `SCHEMES`:
  * the divergence scheme is of the kind of the vertical one (the reference dispatches "vertical advection + divergence flux" on both);
  * an upwinding kinetic-energy gradient needs an upwinding divergence scheme: OnlySelfUpwinding's cross scheme is
    extract_centered_scheme(divergence_scheme), and the reference has no symmetric interpolation for EnergyConserving();
  * with the cross scheme of a WENO(order=5) divergence scheme being its advecting_velocity_scheme, Centered(order=4)
    (weno_reconstruction.jl:119).
"""
from collections import namedtuple

import numpy as np

import implicit_diffusion_numpy as IDN
from oracle import coefficients as K

Scheme = namedtuple("Scheme", "vorticity vertical kinetic_energy stencil", defaults=("velocity",))
W, E = "weno", "conserving"
SCHEMES = {"WWW": Scheme(W, W, W), "WWE": Scheme(W, W, E), "WEE": Scheme(W, E, E), "EWW": Scheme(E, W, W), "EWE": Scheme(E, W, E)}

FLAG_VORTICITY, FLAG_VERTICAL, FLAG_KINETIC_ENERGY, FLAG_DEFAULT_STENCIL = 1, 2, 4, 8  # scheme_flags of the C ABI


def flags(s):
    return ((s.vorticity == W) * FLAG_VORTICITY | (s.vertical == W) * FLAG_VERTICAL | (s.kinetic_energy == W) * FLAG_KINETIC_ENERGY
            | (s.stencil == "default") * FLAG_DEFAULT_STENCIL)


F64 = np.float64
C4 = tuple(float(c) for _, c in K.calc_reconstruction_stencil(F64, 2, "symmetric"))        # applied to ψ[n-2 .. n+1]
P5 = tuple(tuple(float(c) for c in K.weno_coeff_p(F64, 3, r)) for r in range(3))           # coeff_p of stencil r
P3 = tuple(tuple(float(c) for c in K.weno_coeff_p(F64, 2, r)) for r in range(2))
UPWIND5 = {side: tuple(float(c) for _, c in K.calc_reconstruction_stencil(F64, 3, side)) for side in ("left", "right")}
EPSILON = float(np.float32(1e-8))                                                          # const ε = 1f-8
OPTIMAL5 = (3 / 10, 3 / 5, 1 / 10)                                                         # C★
OPTIMAL3 = (2 / 3, 1 / 3)
SMOOTHNESS5 = ((10, -31, 11, 25, -19, 4), (4, -13, 5, 13, -13, 4), (4, -19, 11, 25, -31, 10))
SMOOTHNESS3 = ((1, -2, 1), (1, -2, 1))


# ---- WENO -----------------------------------------------------------------------------------------------------------------------
def _pick(left, a, b):
    return np.where(left, a, b)


def _stencils5(S, left):
    """S₀₃, S₁₃, S₂₃ of S = ψ[n-3 .. n+2] (1-based S[1..6] in the reference)"""
    return ((_pick(left, S[2], S[3]), _pick(left, S[3], S[2]), _pick(left, S[4], S[1])),
            (_pick(left, S[1], S[4]), _pick(left, S[2], S[3]), _pick(left, S[3], S[2])),
            (_pick(left, S[0], S[5]), _pick(left, S[1], S[4]), _pick(left, S[2], S[3])))


def _betas5(S, left):
    out = []
    for p, c in zip(_stencils5(S, left), SMOOTHNESS5):
        out.append(p[0] * ((c[0] * p[0] + c[1] * p[1]) + c[2] * p[2]) + p[1] * (c[3] * p[1] + c[4] * p[2]) + (p[2] * p[2]) * c[5])
    return out


def _weights(beta, tau, optimal):
    q = [tau / (b + EPSILON) for b in beta]
    alpha = [c * (1 + x * x) for c, x in zip(optimal, q)]              # (x^2 is x * x in Julia)
    total = alpha[0]
    for a in alpha[1:]:
        total = total + a
    return [a / total for a in alpha]


def weno5(S, left, smoothness=None, optimal_weights=False):
    """inner_biased_interpolate of WENO(order=5) from S = ψ[n-3 .. n+2].  smoothness: None (the values themselves), one list of six
    (FunctionStencil) or two lists (VelocityStencil: β = (βᵤ + βᵥ) / 2).  optimal_weights: ω = C★ (the linear scheme the weights tend to)."""
    if optimal_weights:
        omega = OPTIMAL5
    else:
        sets = [S] if smoothness is None else (list(smoothness) if isinstance(smoothness[0], (list, tuple)) else [smoothness])
        if len(sets) == 1:
            beta = _betas5(sets[0], left)
        else:
            beta = [(b1 + b2) / 2 for b1, b2 in zip(_betas5(sets[0], left), _betas5(sets[1], left))]
        omega = _weights(beta, np.abs(beta[0] - beta[2]), OPTIMAL5)
    p = [(c[0] * s[0] + c[1] * s[1]) + c[2] * s[2] for s, c in zip(_stencils5(S, left), P5)]
    return (omega[0] * p[0] + omega[1] * p[1]) + omega[2] * p[2]


def weno3(S, left):
    """the buffer scheme WENO(order=3) from S = ψ[n-2 .. n+1]"""
    st = ((_pick(left, S[1], S[2]), _pick(left, S[2], S[1])), (_pick(left, S[0], S[3]), _pick(left, S[1], S[2])))
    beta = [p[0] * (c[0] * p[0] + c[1] * p[1]) + (p[1] * p[1]) * c[2] for p, c in zip(st, SMOOTHNESS3)]
    omega = _weights(beta, np.abs(beta[0] - beta[1]), OPTIMAL3)
    p = [c[0] * s[0] + c[1] * s[1] for s, c in zip(st, P3)]
    return omega[0] * p[0] + omega[1] * p[1]


def upwind5(S, left):
    """UpwindBiased(order=5) from S = ψ[n-3 .. n+2]: what weno5 gives with ω = C★, up to rounding"""
    l, r = UPWIND5["left"], UPWIND5["right"]
    a = (((l[0] * S[0] + l[1] * S[1]) + l[2] * S[2]) + l[3] * S[3]) + l[4] * S[4]
    b = (((r[0] * S[1] + r[1] * S[2]) + r[2] * S[3]) + r[3] * S[4]) + r[4] * S[5]
    return _pick(left, a, b)


def centered4(S):
    return ((C4[0] * S[0] + C4[1] * S[1]) + C4[2] * S[2]) + C4[3] * S[3]


# ---- the terms ----------------------------------------------------------------------------------------------------------------------
class _Operators:
    def __init__(self, g, u, v, w):
        if tuple(g.topo) != ("Periodic", "Periodic", "Bounded"):
            raise ValueError("the restatement covers (Periodic, Periodic, Bounded) grids")
        self.g = g
        self.dx, self.dy = g.dx, g.dy
        self.Az = g.dx * g.dy
        self.dz = IDN._dzC(g, 0)                     # Δzᵃᵃᶜ of the cell's own plane
        self.Ax, self.Ay = g.dy * self.dz, g.dx * self.dz
        sh = lambda f: (lambda a=0, b=0, c=0: IDN._sh(g, f, a, b, c))
        self.U, self.V, self.W = sh(u), sh(v), sh(w)

    # values at (i + a, j + b, k)
    def zeta(self, a, b):              # ζ₃ᶠᶠᶜ
        U, V = self.U, self.V
        return ((self.dy * V(a, b) - self.dy * V(a - 1, b)) - (self.dx * U(a, b) - self.dx * U(a, b - 1))) / self.Az

    def u_ff(self, a, b):              # ℑyᵃᶠᵃ u
        return 0.5 * (self.U(a, b - 1) + self.U(a, b))

    def v_ff(self, a, b):              # ℑxᶠᵃᵃ v
        return 0.5 * (self.V(a - 1, b) + self.V(a, b))

    def dx_U(self, a, b):              # δx_U = δxᶜᶜᶜ(Ax_qᶠᶜᶜ, u)
        return self.Ax * self.U(a + 1, b) - self.Ax * self.U(a, b)

    def dy_V(self, a, b):              # δy_V = δyᶜᶜᶜ(Ay_qᶜᶠᶜ, v)
        return self.Ay * self.V(a, b + 1) - self.Ay * self.V(a, b)

    def divergence_smoothness(self, a, b):
        return self.dx_U(a, b) + self.dy_V(a, b)

    def half(self, f, a, b):           # half_ϕ²
        return f(a, b) * f(a, b) / 2


def _vorticity_weights_from(s, o, points):
    """the smoothness argument of the vorticity reconstruction over the (f, f) points given"""
    if s.stencil == "default":
        return None
    return [[o.u_ff(a, b) for a, b in points], [o.v_ff(a, b) for a, b in points]]


def horizontal_advection(s, o, rec):
    U, V, dx, dy = o.U, o.V, o.dx, o.dy
    m = lambda a: 0.5 * (dx * V(a, 0) + dx * V(a, 1))              # ℑyᵃᶜᵃ(Δx_qᶜᶠᶜ, v) at (i + a, j)
    n = lambda b: 0.5 * (dy * U(0, b) + dy * U(1, b))              # ℑxᶜᵃᵃ(Δy_qᶠᶜᶜ, u) at (i, j + b)
    if s.vorticity == E:
        hu = -(0.5 * (o.zeta(0, 0) + o.zeta(0, 1))) * (0.5 * (m(-1) + m(0))) / dx
        hv = (0.5 * (o.zeta(0, 0) + o.zeta(1, 0))) * (0.5 * (n(-1) + n(0))) / dy
        return hu, hv
    v_hat = 0.5 * (m(-1) + m(0)) / dx
    pts = [(0, b) for b in range(-2, 4)]                           # _biased_interpolate_yᵃᶜᵃ(j) = biased_interpolate_yᵃᶠᵃ(j + 1)
    zeta_R = rec([o.zeta(a, b) for a, b in pts], v_hat > 0, _vorticity_weights_from(s, o, pts))
    hu = -v_hat * zeta_R
    u_hat = 0.5 * (n(-1) + n(0)) / dy
    pts = [(a, 0) for a in range(-2, 4)]
    zeta_R = rec([o.zeta(a, b) for a, b in pts], u_hat > 0, _vorticity_weights_from(s, o, pts))
    hv = u_hat * zeta_R
    return hu, hv


def _z_face_value(g, f, kf, left):
    """_biased_interpolate_zᵃᵃᶠ of WENO(order=5) at the face kf (1-based) of a Bounded z: order 5 where outside_biased_haloᶠ holds for
    H = 3, else the buffer scheme's order 3 where it holds for H = 2, else UpwindBiased(order=1).  f: planes [Nx, Ny] by 1-based k."""
    N = g.Nz
    if 4 <= kf <= N + 1 - 3:
        return weno5([f(kf + m) for m in range(-3, 3)], left)
    if 3 <= kf <= N + 1 - 2:
        return weno3([f(kf + m) for m in range(-2, 2)], left)
    return _pick(left, f(kf - 1), f(kf))


def vertical_flux_differences(g, u, v, w):
    """(δzᵃᵃᶜ advective_momentum_flux_Wu, δzᵃᵃᶜ advective_momentum_flux_Wv) over the interior, vertical_scheme = WENO(order=5)"""
    Hx, Hy, Hz, Nx, Ny, Nz = g.Hx, g.Hy, g.Hz, g.Nx, g.Ny, g.Nz
    Az = g.dx * g.dy
    plane = lambda f, a, b: (lambda k: f[Hx + a:Hx + a + Nx, Hy + b:Hy + b + Ny, Hz + k - 1])
    Fu, Fv = [], []
    for kf in range(1, Nz + 2):
        w_u = centered4([Az * plane(w, a, 0)(kf) for a in (-2, -1, 0, 1)])      # _symmetric_interpolate_xᶠᵃᵃ(Az_qᶜᶜᶠ, W)
        Fu.append(w_u * _z_face_value(g, plane(u, 0, 0), kf, w_u > 0))
        w_v = centered4([Az * plane(w, 0, b)(kf) for b in (-2, -1, 0, 1)])      # _symmetric_interpolate_yᵃᶠᵃ(Az_qᶜᶜᶠ, W)
        Fv.append(w_v * _z_face_value(g, plane(v, 0, 0), kf, w_v > 0))
    Fu, Fv = np.stack(Fu, axis=2), np.stack(Fv, axis=2)
    return Fu[:, :, 1:] - Fu[:, :, :-1], Fv[:, :, 1:] - Fv[:, :, :-1]


def vertical_advection(s, o, rec, u, v, w):
    g, U, V, W_ = o.g, o.U, o.V, o.W
    Az = o.Az
    if s.vertical == E:
        dzf = lambda c: IDN._dzF(g, c)
        Zu = lambda c: (0.5 * (Az * W_(-1, 0, c) + Az * W_(0, 0, c))) * ((U(0, 0, c) - U(0, 0, c - 1)) / dzf(c))    # ζ₂wᶠᶜᶠ
        Zv = lambda c: (0.5 * (Az * W_(0, -1, c) + Az * W_(0, 0, c))) * ((V(0, 0, c) - V(0, 0, c - 1)) / dzf(c))    # ζ₁wᶜᶠᶠ
        return (0.5 * (Zu(0) + Zu(1))) / Az, (0.5 * (Zv(0) + Zv(1))) / Az
    Au, Av = vertical_flux_differences(g, u, v, w)
    vol = Az * o.dz                                                                # Vᶠᶜᶜ = Vᶜᶠᶜ = Az Δz
    # upwinded_divergence_flux_Uᶠᶜᶜ: û (δvˢ + δuᴿ)
    u_hat = U(0, 0)
    dv_S = centered4([o.dy_V(a, 0) + 0.0 for a in (-2, -1, 0, 1)])                 # δy_V_plus_∂t_σ, ∂t_σ = 0 on a static grid
    pts = [(a, 0) for a in range(-3, 3)]
    du_R = rec([o.dx_U(a, b) for a, b in pts], u_hat > 0, [o.divergence_smoothness(a, b) for a, b in pts])
    phi_u = u_hat * (dv_S + du_R)
    v_hat = V(0, 0)
    du_S = centered4([o.dx_U(0, b) + 0.0 for b in (-2, -1, 0, 1)])
    pts = [(0, b) for b in range(-3, 3)]
    dv_R = rec([o.dy_V(a, b) for a, b in pts], v_hat > 0, [o.divergence_smoothness(a, b) for a, b in pts])
    phi_v = v_hat * (du_S + dv_R)
    return 1 / vol * (phi_u + Au), 1 / vol * (phi_v + Av)


def bernoulli_head(s, o, rec):
    U, V, dx, dy = o.U, o.V, o.dx, o.dy
    if s.kinetic_energy == E:
        Kh = lambda a, b: (0.5 * (U(a, b) * U(a, b) + U(a + 1, b) * U(a + 1, b)) + 0.5 * (V(a, b) * V(a, b) + V(a, b + 1) * V(a, b + 1))) / 2
        return (Kh(0, 0) - Kh(-1, 0)) / dx, (Kh(0, 0) - Kh(0, -1)) / dy
    hu, hv = (lambda a, b: o.half(U, a, b)), (lambda a, b: o.half(V, a, b))
    # bernoulli_head_U: (δKuᴿ + δKvˢ) / Δx
    dKv_S = centered4([hv(0, b) - hv(-1, b) for b in (-1, 0, 1, 2)])               # _symmetric_interpolate_yᵃᶜᵃ(j) of δx_v² at (f, f)
    pts = [(a, 0) for a in range(-3, 3)]
    dKu_R = rec([hu(a + 1, b) - hu(a, b) for a, b in pts], U(0, 0) > 0, [0.5 * (U(a, b) + U(a + 1, b)) for a, b in pts])
    bu = (dKu_R + dKv_S) / dx
    dKu_S = centered4([hu(a, 0) - hu(a, -1) for a in (-1, 0, 1, 2)])               # _symmetric_interpolate_xᶜᵃᵃ(i) of δy_u² at (f, f)
    pts = [(0, b) for b in range(-3, 3)]
    dKv_R = rec([hv(a, b + 1) - hv(a, b) for a, b in pts], V(0, 0) > 0, [0.5 * (V(a, b) + V(a, b + 1)) for a, b in pts])
    bv = (dKv_R + dKu_S) / dy
    return bu, bv


def terms(g, s, u, v, w, optimal_weights=False):
    """the three terms of (U_dot_∇u, U_dot_∇v) over the interior: ((hadv_u, hadv_v), (vadv_u, vadv_v), (bern_u, bern_v))"""
    o = _Operators(g, u, v, w)
    rec = lambda S, left, smoothness: weno5(S, left, smoothness, optimal_weights)
    return horizontal_advection(s, o, rec), vertical_advection(s, o, rec, u, v, w), bernoulli_head(s, o, rec)


def tendencies(g, s, u, v, w, eta=None, grav=0.0, optimal_weights=False):
    """(Gu, Gv) = (-U_dot_∇u, -U_dot_∇v) over the interior; with eta (a plane [i, j] with halos), - g ∂x η and - g ∂y η are subtracted
    (explicit_barotropic_pressure_x/y_gradient)"""
    (hu, hv), (vu, vv), (bu, bv) = terms(g, s, u, v, w, optimal_weights)
    Gu, Gv = -((hu + vu) + bu), -((hv + vv) + bv)
    if eta is not None:
        e = lambda a, b: eta[g.Hx + a:g.Hx + a + g.Nx, g.Hy + b:g.Hy + b + g.Ny, None]
        Gu = Gu - grav * ((e(0, 0) - e(-1, 0)) / g.dx)
        Gv = Gv - grav * ((e(0, 0) - e(0, -1)) / g.dy)
    return Gu, Gv


def into_parent(g, G, values):
    """a copy of the parent G with `values` over the interior"""
    out = np.array(G, dtype=np.float64)
    out[g.Hx:g.Hx + g.Nx, g.Hy:g.Hy + g.Ny, g.Hz:g.Hz + g.Nz] = values
    return out
