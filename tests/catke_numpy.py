"""CATKEVerticalDiffusivity restated in NumPy, function for function, on parent arrays indexed [i, j, k] with halos (Field.parent()); a (Center,
Center, Face) parent has Nz + 2 Hz + 1 planes, face k at index Hz + k - 1.  Every function of the reference that takes (i, j, k) takes the
1-based k here and returns the (Nx, Ny) array of its values over the interior columns; di / dj shift the column as i + di / j + dj do.

  TKEBasedVerticalDiffusivities.jl:57-156   ϕ², shearᶜᶜᶠ, shearᶜᶜᶜ, Riᶜᶜᶠ, Riᶜᶜᶜ, ℑbzᵃᵃᶜ, buoyancy_fluxᶜᶜᶠ, explicit_buoyancy_flux, shear_production,
                                            turbulent_velocityᶜᶜᶜ, mask_diffusivity, clip
  catke_mixing_length.jl                    the length scales at ccf and ccc, step, scale, the three mixing lengths
  catke_vertical_diffusivity.jl:213-325     compute_diffusivities!, compute_average_surface_buoyancy_flux!, compute_CATKE_diffusivities!, κ★ᶜᶜᶠ
  catke_equation.jl:38-120                  dissipation_length_scaleᶜᶜᶜ, dissipation_rate, top_tke_flux
  tke_top_boundary_condition.jl:64-77       friction_velocity, top_convective_turbulent_velocity_cubed
  time_step_catke_equation.jl:12-173        time_step_catke_equation!, substep_turbulent_kinetic_energy!
  vertically_implicit_diffusion_solver.jl:55-110   the rows of implicit_step!, the linear coefficient in the diagonal
  TurbulenceClosures.jl:136-155             z_top, z_bottom, depth, height_above_bottom;  Grids/inactive_node.jl:145-149  peripheral_node
  Operators/interpolation_operators.jl:21-28   ℑxᶜᵃᵃ, ℑxᶠᵃᵃ, ℑyᵃᶜᵃ, ℑyᵃᶠᵃ, ℑzᵃᵃᶠ = 0.5 (a + b)

Written from those files.  Julia semantics that NumPy does not have are spelled out: max / min propagate a NaN and order the zeros
(`jmax`, `jmin`), x * flag with a Bool flag is x or a zero with x's sign (`bmul`; the zero of a NaN x is +0 here, Julia gives it the NaN's
sign bit, which differs between machines), x^2 and x^3 are x x and x x x, ifelse evaluates both branches and selects.  cbrt is NOT NumPy's:
`cbrt` restates csrc/ocn_catke.h, every operation an IEEE +, -, *, / or an exact scaling.  A face function is only evaluated where ℑbzᵃᵃᶜ uses
its value (the reference evaluates it on peripheral faces too and discards the result), so nothing is read beyond k = Nz + 1.  The
substep reads every e before it writes any (the reference's kernel reads the neighbours' e while other threads write it).
tests/test_host_catke.py pins this file without a GPU."""
import math

import numpy as np

import convective_adjustment_numpy as CAN
import implicit_diffusion_numpy as IDN

ccf_shape, fill_xy_halos = CAN.ccf_shape, CAN.fill_xy_halos

MIXING_LENGTH = dict(C_s=1.131, C_b=0.28, C_sp=0.505, CRi_delta=1.02, CRi_0=0.254, C_hi_u=0.242, C_lo_u=0.361, C_un_u=0.370, C_c_u=3.705,
                     C_e_u=0.0, C_hi_c=0.098, C_lo_c=0.369, C_un_c=0.572, C_c_c=4.793, C_e_c=0.112, C_hi_e=0.548, C_lo_e=7.863, C_un_e=1.447,
                     C_c_e=3.642, C_e_e=0.0)
EQUATION = dict(C_hi_D=0.579, C_lo_D=1.604, C_un_D=0.923, C_c_D=3.254, C_e_D=0.0, C_W_ustar=3.179, C_W_wdelta=0.383, C_W_eps=1.0)
CLOSURE = dict(maximum_tracer_diffusivity=np.inf, maximum_tke_diffusivity=np.inf, maximum_viscosity=np.inf, minimum_tke=1e-9,
               minimum_convective_buoyancy_flux=1e-11, negative_tke_damping_time_scale=60.0)


def closure_dict(**kw):
    """the reference's defaults (catke_mixing_length.jl:15-36, catke_equation.jl:7-16, catke_vertical_diffusivity.jl:96-106), ASCII names"""
    d = {**MIXING_LENGTH, **EQUATION, **CLOSURE}
    for k in kw:
        if k not in d:
            raise TypeError(k)
    d.update(kw)
    return d


# ---------------------------------------------------------------------------------------------------------------------------------
# Julia's scalar semantics
# ---------------------------------------------------------------------------------------------------------------------------------
def _both(a, b):
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    return a, b


def jmax(a, b):
    a, b = _both(a, b)
    with np.errstate(invalid="ignore"):
        tie = np.where(np.signbit(a), b, a)
        return np.where(a != a, a, np.where(b != b, b, np.where(a > b, a, np.where(b > a, b, tie))))


def jmin(a, b):
    a, b = _both(a, b)
    with np.errstate(invalid="ignore"):
        tie = np.where(np.signbit(a), a, b)
        return np.where(a != a, a, np.where(b != b, b, np.where(a < b, a, np.where(b < a, b, tie))))


def clip(x):
    return jmax(0.0, x)


def bmul(x, flag):
    x, flag = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(flag, dtype=bool))
    zero = np.where(x != x, 0.0, np.copysign(0.0, x))
    return np.where(flag, x, zero)


def nan_to_zero(x):
    return np.where(x != x, 0.0, x)


def cbrt(x):
    """csrc/ocn_catke.h cbrt_newton: |x| = m 2^e with 1 <= m < 2, e = 3 q + r, a = m 2^r, y0 = 1 + (a - 1) / 7, six Newton steps
    y <- (2 y + a / (y y)) / 3, ±y 2^q; zeros, infinities and NaN come back as they are"""
    x = np.asarray(x, dtype=np.float64)
    special = (x != x) | (x == 0) | np.isinf(x)
    a = np.where(special, 1.0, np.abs(x))
    f, E = np.frexp(a)  # a = f 2^E, 0.5 <= f < 1 (subnormals included)
    m, e = 2.0 * f, E - 1
    q = np.floor_divide(e, 3)
    r = e - 3 * q
    a = m * np.ldexp(1.0, r)
    y = 1.0 + (a - 1.0) / 7.0
    for _ in range(6):
        y = (2.0 * y + a / (y * y)) / 3.0
    y = np.ldexp(y, q)
    return np.where(special, x, np.where(np.signbit(x), -y, y))


def step(x, c, w):
    with np.errstate(invalid="ignore", divide="ignore"):
        return jmax(0.0, jmin(1.0, (x - c) / w))


def scale(Ri, s_minus, s_zero, s_inf, c, w):
    with np.errstate(invalid="ignore"):
        s_plus = s_zero + (s_inf - s_zero) * step(Ri, c, w)
        return bmul(s_minus, Ri < 0) + bmul(s_plus, Ri >= 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# the state a kernel function reads
# ---------------------------------------------------------------------------------------------------------------------------------
class State:
    """g: IDN.describe(grid); zf, zc: the Nz + 1 interior z faces and the Nz centres; Lz; buoyancy: None, "BuoyancyTracer" (T is b) or
    ("SeawaterBuoyancy", g, α, β); cl: closure_dict(); parents u, v, T, S, e; Jb: (Nx, Ny)"""

    def __init__(self, g, zf, zc, Lz, buoyancy, cl, u, v, T, S, e, Jb):
        self.g, self.zf, self.zc, self.Lz, self.buoyancy, self.cl = g, np.asarray(zf, dtype=np.float64), np.asarray(zc, dtype=np.float64), float(Lz), buoyancy, cl
        self.u, self.v, self.T, self.S, self.e, self.Jb = u, v, T, S, e, Jb

    def col(self, a, k, di=0, dj=0):
        g = self.g
        return a[g.Hx + di:g.Hx + di + g.Nx, g.Hy + dj:g.Hy + dj + g.Ny, g.Hz + k - 1]

    def dzF(self, k):
        return float(self.g.dzf[self.g.Hz + k - 1])

    def dzC(self, k):
        return float(self.g.dzc[self.g.Hz + k - 1])

    def zeros(self):
        return np.zeros((self.g.Nx, self.g.Ny))


def peripheral(s, k):
    """peripheral_node(i, j, k, grid, c, c, f) on a z-Bounded grid: a face with an inactive cell on either side"""
    return k <= 1 or k >= s.g.Nz + 1


def bz(s, f, k):
    """ℑbzᵃᵃᶜ(i, j, k, grid, f, args...) (TKEBasedVerticalDiffusivities.jl:88-102)"""
    p_plus, p_minus = peripheral(s, k + 1), peripheral(s, k)
    f_plus = f(k) if p_plus else f(k + 1)
    f_minus = f_plus if p_minus else f(k)
    with np.errstate(invalid="ignore"):
        return (f_plus + f_minus) / 2


def dz_b(s, k):
    """∂z_b(i, j, k, grid, buoyancy, tracers) (seawater_buoyancy.jl:219-224, buoyancy_tracer.jl:16)"""
    if s.buoyancy is None:
        return s.zeros()
    dT = (s.col(s.T, k) - s.col(s.T, k - 1)) / s.dzF(k) if s.T is not None else 0.0
    if s.buoyancy == "BuoyancyTracer":
        return dT + s.zeros()
    dS = (s.col(s.S, k) - s.col(s.S, k - 1)) / s.dzF(k) if s.S is not None else 0.0
    _, grav, alpha, beta = s.buoyancy[:4]
    return grav * (alpha * dT - beta * dS) + s.zeros()


def dz_u(s, u, k, di=0):
    return (s.col(u, k, di, 0) - s.col(u, k - 1, di, 0)) / s.dzF(k)


def dz_v(s, v, k, dj=0):
    return (s.col(v, k, 0, dj) - s.col(v, k - 1, 0, dj)) / s.dzF(k)


def shear_ccf(s, k):
    """shearᶜᶜᶠ (:59-64)"""
    sq = lambda x: x * x
    dzu2 = 0.5 * (sq(dz_u(s, s.u, k, 0)) + sq(dz_u(s, s.u, k, 1)))
    dzv2 = 0.5 * (sq(dz_v(s, s.v, k, 0)) + sq(dz_v(s, s.v, k, 1)))
    return dzu2 + dzv2


def shear_ccc(s, k):
    """shearᶜᶜᶜ (:66-71): ℑxᶜᵃᵃ(ℑbzᵃᵃᶜ(ϕ²(∂zᶠᶜᶠ u))) + ℑyᵃᶜᵃ(ℑbzᵃᵃᶜ(ϕ²(∂zᶜᶠᶠ v)))"""
    sq = lambda x: x * x
    bu = lambda di: bz(s, lambda kk: sq(dz_u(s, s.u, kk, di)), k)
    bv = lambda dj: bz(s, lambda kk: sq(dz_v(s, s.v, kk, dj)), k)
    return 0.5 * (bu(0) + bu(1)) + 0.5 * (bv(0) + bv(1))


def Ri_ccf(s, k):
    """Riᶜᶜᶠ (:76-83)"""
    S2, N2 = shear_ccf(s, k), dz_b(s, k)
    with np.errstate(invalid="ignore", divide="ignore"):
        Ri = N2 / S2
    return np.where(N2 == 0, 0.0, Ri)


def Ri_ccc(s, k):
    return bz(s, lambda kk: Ri_ccf(s, kk), k)


def turbulent_velocity(s, k):
    """turbulent_velocityᶜᶜᶜ (:145-149)"""
    return np.sqrt(jmax(s.cl["minimum_tke"], s.col(s.e, k)))


def w_ccf(s, k):
    return 0.5 * (turbulent_velocity(s, k - 1) + turbulent_velocity(s, k))


def w3_ccf(s, k):
    cube = lambda x: x * x * x
    return 0.5 * (cube(turbulent_velocity(s, k - 1)) + cube(turbulent_velocity(s, k)))


def depth_ccf(s, k):
    return clip(s.zf[s.g.Nz] - s.zf[k - 1])


def depth_ccc(s, k):
    return clip(s.zf[s.g.Nz] - s.zc[k - 1])


def height_ccf(s, k):
    return jmax(s.dzC(k - 1), s.zf[k - 1] - s.zf[0])


def height_ccc(s, k):
    return jmax(s.dzC(k) / 2, s.zc[k - 1] - s.zf[0])


# ---------------------------------------------------------------------------------------------------------------------------------
# catke_mixing_length.jl
# ---------------------------------------------------------------------------------------------------------------------------------
def _stratification_length(w, N2):
    N2p = clip(N2)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(N2p == 0, np.inf, w / np.sqrt(N2p))


def stable_length_ccf(s, k):
    d = jmin(s.cl["C_s"] * depth_ccf(s, k), s.cl["C_b"] * height_ccf(s, k)) + s.zeros()
    l = jmin(d, _stratification_length(w_ccf(s, k), dz_b(s, k)))
    return np.where(l != l, d, l)


def stable_length_ccc(s, k):
    d = jmin(s.cl["C_s"] * depth_ccc(s, k), s.cl["C_b"] * height_ccc(s, k)) + s.zeros()
    N2 = bz(s, lambda kk: dz_b(s, kk), k)
    l = jmin(d, _stratification_length(turbulent_velocity(s, k), N2))
    return np.where(l != l, d, l)


def convective_length_ccf(s, k, Cc, Ce, with_branches=False):
    Jbe, Jb, Csp = s.cl["minimum_convective_buoyancy_flux"], s.Jb, s.cl["C_sp"]
    w, w3, S2, N2, N2_above = w_ccf(s, k), w3_ccf(s, k), shear_ccf(s, k), dz_b(s, k), dz_b(s, k + 1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        lc = nan_to_zero(Cc * w3 / (Jb + Jbe))
        Rif = depth_ccf(s, k) * w * S2 / (Jb + Jbe)
        lc = clip((1 - Csp * Rif) * lc)
        le = Ce * Jb / (w * N2 + Jbe)
        convecting = (Jb > Jbe) & (N2 < 0)
        entraining = (Jb > Jbe) & (N2 > 0) & (N2_above < 0)
    l = nan_to_zero(np.where(convecting, lc, np.where(entraining, le, 0.0)))
    return (l, convecting, entraining) if with_branches else l


def convective_length_ccc(s, k, Cc, Ce):
    Jbe, Jb, Csp = s.cl["minimum_convective_buoyancy_flux"], s.Jb, s.cl["C_sp"]
    w = turbulent_velocity(s, k)
    w3 = w * w * w
    S2 = shear_ccc(s, k)
    N2 = bz(s, lambda kk: dz_b(s, kk), k)
    N2_above = bz(s, lambda kk: dz_b(s, kk), k + 1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        lc = nan_to_zero(Cc * w3 / (Jb + Jbe))
        convecting = (Jb > Jbe) & (N2 < 0)
        Rif = depth_ccc(s, k) * S2 * w / (Jb + Jbe)
        lc = clip((1 - Csp * Rif) * lc)
        le = Ce * Jb / (w * N2 + Jbe)
        entraining = (Jb > Jbe) & (N2 > 0) & (N2_above < 0)
    return nan_to_zero(np.where(convecting, lc, np.where(entraining, le, 0.0)))


def mixing_length_ccf(s, k, which):
    """momentum_ / tracer_ / TKE_mixing_lengthᶜᶜᶠ (:218-277); which: "u", "c" or "e" """
    cl = s.cl
    lh = convective_length_ccf(s, k, cl[f"C_c_{which}"], cl[f"C_e_{which}"])
    sigma = scale(Ri_ccf(s, k), cl[f"C_un_{which}"], cl[f"C_lo_{which}"], cl[f"C_hi_{which}"], cl["CRi_0"], cl["CRi_delta"])
    with np.errstate(invalid="ignore"):
        ls = sigma * stable_length_ccf(s, k)
    l = jmax(nan_to_zero(ls), nan_to_zero(lh))
    return jmin(s.Lz, l)


KAPPA_MAXIMUM = {"u": "maximum_viscosity", "c": "maximum_tracer_diffusivity", "e": "maximum_tke_diffusivity"}


def kappa_ccf(s, k, which):
    """κuᶜᶜᶠ, κcᶜᶜᶠ, κeᶜᶜᶠ (catke_vertical_diffusivity.jl:297-325) with mask_diffusivity (peripheral faces are exactly 0)"""
    if peripheral(s, k):
        return s.zeros()
    with np.errstate(over="ignore"):
        return jmin(mixing_length_ccf(s, k, which) * w_ccf(s, k), s.cl[KAPPA_MAXIMUM[which]])


def dissipation_length(s, k):
    """dissipation_length_scaleᶜᶜᶜ (catke_equation.jl:38-63)"""
    cl = s.cl
    lh = convective_length_ccc(s, k, cl["C_c_D"], cl["C_e_D"])
    sigma = scale(Ri_ccc(s, k), cl["C_un_D"], cl["C_lo_D"], cl["C_hi_D"], cl["CRi_0"], cl["CRi_delta"])
    with np.errstate(invalid="ignore", divide="ignore"):
        ls = stable_length_ccc(s, k) / sigma
    return jmin(s.Lz, jmax(nan_to_zero(ls), nan_to_zero(lh)))


def dissipation_rate(s, k):
    e = s.col(s.e, k)
    with np.errstate(invalid="ignore", divide="ignore"):
        physical = np.sqrt(np.abs(e)) / dissipation_length(s, k)
    return np.where(e < 0, 1 / s.cl["negative_tke_damping_time_scale"], physical)


# ---------------------------------------------------------------------------------------------------------------------------------
# the boundary conditions and the three kernels
# ---------------------------------------------------------------------------------------------------------------------------------
def bc_value(s, bc, c):
    """getbc of a top condition over the interior columns: None (no flux: 0), a number, an (Nx, Ny) array, or (value, coeff): value + coeff *
    c[i, j, Nz]"""
    if bc is None:
        return s.zeros()
    if isinstance(bc, tuple):
        return bc[0] + bc[1] * s.col(c, s.g.Nz)
    return s.zeros() + np.asarray(bc, dtype=np.float64)


def top_buoyancy_flux(s, top_T, top_S):
    if s.buoyancy is None:
        return s.zeros()
    JT = bc_value(s, top_T, s.T) if s.T is not None else s.zeros()
    if s.buoyancy == "BuoyancyTracer":
        return JT
    JS = bc_value(s, top_S, s.S) if s.S is not None else s.zeros()
    _, grav, alpha, beta = s.buoyancy[:4]
    return grav * (alpha * JT - beta * JS)


def top_tke_flux(s, top_u, top_v, top_T, top_S):
    """_top_tke_flux (catke_equation.jl:109-120): - Cᵂu★ u★³ - CᵂwΔ wΔ³"""
    tau_x, tau_y = bc_value(s, top_u, s.u), bc_value(s, top_v, s.v)
    u_star = np.sqrt(np.sqrt(tau_x * tau_x + tau_y * tau_y))
    w_delta3 = clip(top_buoyancy_flux(s, top_T, top_S)) * s.dzC(s.g.Nz)
    return -s.cl["C_W_ustar"] * (u_star * u_star * u_star) - s.cl["C_W_wdelta"] * w_delta3


def surface_buoyancy_flux(s, top_T, top_S, dt):
    """compute_average_surface_buoyancy_flux! (catke_vertical_diffusivity.jl:253-271): the new Jᵇ, an (Nx, Ny) array"""
    J_star = top_buoyancy_flux(s, top_T, top_S)
    lD = dissipation_length(s, s.g.Nz)
    J_plus = jmax(jmax(s.cl["minimum_convective_buoyancy_flux"], s.Jb), J_star)
    t_star = cbrt(lD * lD / J_plus)
    eps = dt / t_star
    return (s.Jb + eps * J_star) / (1 + eps)


def diffusivities(s, kappa_u, kappa_c, kappa_e):
    """compute_CATKE_diffusivities! over :xyz: copies of the three (Center, Center, Face) parents with faces k = 1..Nz of the interior written"""
    g = s.g
    out = [np.array(a, dtype=np.float64) for a in (kappa_u, kappa_c, kappa_e)]
    for k in range(1, g.Nz + 1):
        for a, which in zip(out, "uce"):
            a[g.Hx:g.Hx + g.Nx, g.Hy:g.Hy + g.Ny, g.Hz + k - 1] = kappa_ccf(s, k, which)
    return out


def shear_production(s, k, kappa_u, u_prev, v_prev):
    """shear_production (TKEBasedVerticalDiffusivities.jl:116-143) with νₑ = κᵘ, uⁿ / vⁿ the previous velocities, u⁺ / v⁺ the current ones"""
    def dz_nu_x(kk, di, a, b):  # Δz_νₑ_az_bzᶠᶜᶠ at i + di
        nu = 0.5 * (s.col(kappa_u, kk, di - 1, 0) + s.col(kappa_u, kk, di, 0))
        return nu * dz_u(s, a, kk, di) * s.dzF(kk) * dz_u(s, b, kk, di)

    def dz_nu_y(kk, dj, a, b):  # Δz_νₑ_az_bzᶜᶠᶠ at j + dj
        nu = 0.5 * (s.col(kappa_u, kk, 0, dj - 1) + s.col(kappa_u, kk, 0, dj))
        return nu * dz_v(s, a, kk, dj) * s.dzF(kk) * dz_v(s, b, kk, dj)

    def Px(di):
        n = bz(s, lambda kk: dz_nu_x(kk, di, u_prev, s.u), k)
        p = bz(s, lambda kk: dz_nu_x(kk, di, s.u, s.u), k)
        return (n + p) / (2 * s.dzC(k))

    def Py(dj):
        n = bz(s, lambda kk: dz_nu_y(kk, dj, v_prev, s.v), k)
        p = bz(s, lambda kk: dz_nu_y(kk, dj, s.v, s.v), k)
        return (n + p) / (2 * s.dzC(k))

    return 0.5 * (Px(0) + Px(1)) + 0.5 * (Py(0) + Py(1))


def substep(s, u_prev, v_prev, kappa_u, kappa_c, kappa_e, Le, Gn_e, Gm_e, dtau, chi, with_terms=False):
    """substep_turbulent_kinetic_energy! (time_step_catke_equation.jl:78-173) over :xyz: (e, κᵉ, Le, G⁻e) as copies of the parents, every
    read of e from the e of before the call.  with_terms: also a dict of (Nx, Ny, Nz) arrays (P, wb, ω, ...: what the tests count)"""
    g, cl = s.g, s.cl
    e_new, ke, L_out, Gm_out = (np.array(a, dtype=np.float64) for a in (s.e, kappa_e, Le, Gm_e))
    alpha, beta = 1.5 + chi, 0.5 + chi
    terms = {name: np.zeros((g.Nx, g.Ny, g.Nz)) for name in ("P", "wb", "omega", "L")}
    for k in range(1, g.Nz + 1):
        I = (slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny), g.Hz + k - 1)
        ke[I] = kappa_ccf(s, k, "e")
        wb = bz(s, lambda kk: -s.col(kappa_c, kk) * dz_b(s, kk), k)  # explicit_buoyancy_flux
        wb_minus, wb_plus = jmin(0.0, wb), jmax(0.0, wb)
        e = s.col(s.e, k)
        with np.errstate(invalid="ignore", divide="ignore"):
            wb_e = bmul(wb_minus / e, e > cl["minimum_tke"])
        on_bottom = k == 1  # !inactive_cell(k) & inactive_cell(k - 1)
        w = np.sqrt(clip(e))
        div_Je = (-1.0 if on_bottom else 0.0) * cl["C_W_eps"] * w / s.dzC(k)
        omega = dissipation_rate(s, k)
        L = wb_e - omega + div_Je
        L_out[I] = L
        P = shear_production(s, k, kappa_u, u_prev, v_prev)
        fast = P + wb_plus - 0.0  # dissipation(::VITD) = 0
        total = s.col(Gn_e, k) + fast
        e_new[I] = e + dtau * (alpha * total - beta * s.col(Gm_e, k))
        Gm_out[I] = total
        for name, a in (("P", P), ("wb", wb), ("omega", omega), ("L", L)):
            terms[name][:, :, k - 1] = a
    return (e_new, ke, L_out, Gm_out, terms) if with_terms else (e_new, ke, L_out, Gm_out)


def implicit_step_e(g, e, kappa_e, Le, dt):
    """implicit_step!(e, ...) with the diagonal of vertically_implicit_diffusion_solver.jl:107-110: 1 - Δt L - upper(k) - lower(k - 1); the
    elimination is IDN.thomas (solve_batched_tridiagonal_system_z!)"""
    Nz, dz = g.Nz, IDN._dz_at
    out = np.array(e, dtype=np.float64)
    for i in range(g.Nx):
        for j in range(g.Ny):
            kz = lambda k: float(kappa_e[g.Hx + i, g.Hy + j, g.Hz + k - 1])
            Lc = lambda k: float(Le[g.Hx + i, g.Hy + j, g.Hz + k - 1])

            def upper(k):
                du = -dt * kz(k + 1) / (dz(g, False, k) * dz(g, True, k + 1))
                return 0.0 if k > Nz - 1 else du

            def lower(kp):
                if kp < 1:
                    return 0.0
                k = kp + 1
                return -dt * kz(k) / (dz(g, False, k) * dz(g, True, k))

            a, b, c = np.zeros(Nz), np.zeros(Nz), np.zeros(Nz)
            for k in range(1, Nz + 1):
                a[k - 1] = lower(k) if k < Nz else 0.0
                b[k - 1] = 1.0 - dt * Lc(k) - upper(k) - lower(k - 1)
                c[k - 1] = upper(k)
            col = (g.Hx + i, g.Hy + j, slice(g.Hz, g.Hz + Nz))
            out[col] = IDN.thomas(a, b, c, out[col])
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the model-level sequence
# ---------------------------------------------------------------------------------------------------------------------------------
def time_step_tke(s, u_prev, v_prev, kappa_u, kappa_c, kappa_e, Le, Gn_e, Gm_e, last_dt, tke_time_step, chi):
    """time_step_catke_equation! (time_step_catke_equation.jl:12-76): (e, κᵉ, Le, G⁻e, [χ of every substep])"""
    if tke_time_step is None:
        M, dtau = 1, last_dt
    else:
        M = math.ceil(last_dt / tke_time_step)
        dtau = last_dt / M
    e, chis = s.e, []
    for m in range(1, M + 1):
        chi_m = -0.5 if (m == 1 and M != 1) else chi
        chis.append(chi_m)
        sm = State(s.g, s.zf, s.zc, s.Lz, s.buoyancy, s.cl, s.u, s.v, s.T, s.S, e, s.Jb)
        e, kappa_e, Le, Gm_e = substep(sm, u_prev, v_prev, kappa_u, kappa_c, kappa_e, Le, Gn_e, Gm_e, dtau, chi_m)
        e = implicit_step_e(s.g, e, kappa_e, Le, dtau)
    return e, kappa_e, Le, Gm_e, chis


def compute_diffusivities(s, d, tops, time, last_dt, tke_time_step, chi, Gn_e, Gm_e):
    """compute_diffusivities! (catke_vertical_diffusivity.jl:219-251) followed by the x / y halo fill of the three κ and the top flux of e.
    d: dict with kappa_u, kappa_c, kappa_e, Le (parents), Jb, u_prev, v_prev, previous_compute_time; tops: dict u, v, T, S of top conditions
    (bc_value).  Returns (the new dict, e, G⁻e, top flux of e)."""
    dt = time - d["previous_compute_time"]
    e, Gm, ke, Le = s.e, Gm_e, d["kappa_e"], d["Le"]
    if math.isfinite(last_dt):
        sj = State(s.g, s.zf, s.zc, s.Lz, s.buoyancy, s.cl, s.u, s.v, s.T, s.S, s.e, d["Jb"])
        e, ke, Le, Gm, _ = time_step_tke(sj, d["u_prev"], d["v_prev"], d["kappa_u"], d["kappa_c"], ke, Le, Gn_e, Gm_e, last_dt, tke_time_step, chi)
    s1 = State(s.g, s.zf, s.zc, s.Lz, s.buoyancy, s.cl, s.u, s.v, s.T, s.S, e, d["Jb"])
    Jb = surface_buoyancy_flux(s1, tops["T"], tops["S"], dt)
    s2 = State(s.g, s.zf, s.zc, s.Lz, s.buoyancy, s.cl, s.u, s.v, s.T, s.S, e, Jb)
    ku, kc, ke = (fill_xy_halos(s.g, a) for a in diffusivities(s2, d["kappa_u"], d["kappa_c"], ke))
    out = dict(kappa_u=ku, kappa_c=kc, kappa_e=ke, Le=Le, Jb=Jb, u_prev=np.array(s.u), v_prev=np.array(s.v), previous_compute_time=time)
    return out, e, Gm, top_tke_flux(s2, tops["u"], tops["v"], tops["T"], tops["S"])
