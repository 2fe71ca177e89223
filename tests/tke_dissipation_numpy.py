"""TKEDissipationVerticalDiffusivity (k-ϵ) restated in NumPy, function for function, on parent arrays indexed [i, j, k] with halos
(Field.parent()), in the conventions of tests/catke_numpy.py, whose shared operators (ℑbzᵃᵃᶜ, ∂z_b, shearᶜᶜᶠ, shear_production, Julia's min / max /
Bool product) it uses: every function of the reference that takes (i, j, k) takes the 1-based k here and returns the (Nx, Ny) array of its
values over the interior columns.

  tke_dissipation_vertical_diffusivity.jl:228-354   compute_diffusivities!, turbulent_kinetic_energyᶜᶜᶜ, minimum_dissipation, dissipationᶜᶜᶜ, κ★ᶜᶜᶠ
  tke_dissipation_stability_functions.jl            square_time_scaleᶜᶜᶜ, the two numbers, their bounds, the stability functions
  tke_dissipation_equations.jl:24-251               time_step_tke_dissipation_equations!, substep_tke_dissipation!, the two top fluxes
  TKEBasedVerticalDiffusivities.jl:57-156           (through catke_numpy) shearᶜᶜᶠ, ℑbzᵃᵃᶜ, explicit_buoyancy_flux, shear_production, mask_diffusivity
  vertically_implicit_diffusion_solver.jl:55-110    the rows of implicit_step!, the linear coefficient in the diagonal; `implicit_matrix` is their
                                                    dense form
  Operators/interpolation_operators.jl:27-28        ℑzᵃᵃᶜ, ℑzᵃᵃᶠ = 0.5 (a + b)

Written from those files, with none of the kernel's economies: a κ★ᶜᶜᶠ is evaluated on face 1 too (from the halo cells below; a halo that is
too thin wraps around, harmlessly) and discarded by mask_diffusivity's ifelse; e², ϵ̄ and the stability function are recomputed for every κ.
Julia semantics spelled out: max / min are jmax / jmin, clamp(x, lo, hi) = ifelse(x > hi, hi, ifelse(x < lo, lo, x)), x * flag is bmul, x^2 and
x^3 are products, 𝕊u₀^4 is (𝕊u₀ 𝕊u₀) (𝕊u₀ 𝕊u₀).  The constants that depend on coefficients alone are computed in Python floats by
`closure_dict`, by the reference's formulas.  The substep reads every e and ϵ before it writes any.  tests/test_host_tke_dissipation.py pins
this file without a GPU."""
import math

import numpy as np

import catke_numpy as CK
import implicit_diffusion_numpy as IDN

jmax, jmin, bmul, fill_xy_halos, ccf_shape = CK.jmax, CK.jmin, CK.bmul, CK.fill_xy_halos, CK.ccf_shape

EQUATIONS = dict(C_eps_eps=1.92, C_P_eps=1.44, C_b_eps_plus=-0.65, C_b_eps_minus=-0.65, C_W_ustar=0.0, C_W_wdelta=0.0, C_W_alpha=0.11,
                 gravitational_acceleration=9.8065, minimum_roughness_length=1e-4)
VARIABLE = dict(C_sigma_e=1.0, C_sigma_eps=1.2, Cu0=0.1067, Cu1=0.0173, Cu2=-0.0001205, Cc0=0.1120, Cc1=0.003766, Cc2=0.0008871, Cd0=1.0, Cd1=0.2398,
                Cd2=0.02872, Cd3=0.005154, Cd4=0.006930, Cd5=-0.0003372, Su0=None)
CONSTANT = dict(C_sigma_e=1.0, C_sigma_eps=1.2, Cu0=0.53, Cc0=0.53, Su0=0.53)
LENGTH_SCALE = dict(C_N=0.75, minimum_buoyancy_frequency=1e-14)
CLOSURE = dict(maximum_tracer_diffusivity=np.inf, maximum_tke_diffusivity=np.inf, maximum_dissipation_diffusivity=np.inf, maximum_viscosity=np.inf,
               minimum_tke=1e-6, minimum_stratification_number_safety_factor=0.73, negative_tke_damping_time_scale=60.0)


def log_layer_Su0(cl):
    """VariableStabilityFunctions(𝕊u₀ = nothing) (tke_dissipation_stability_functions.jl:75-83)"""
    a, b, c = cl["Cd5"] - cl["Cu2"], cl["Cd2"] - cl["Cu0"], cl["Cd0"]
    return (2 * a / (-b - math.sqrt(b * b - 4 * a * c))) ** (1 / 4)


def minimum_stratification_number(cl):
    """minimum_stratification_number(closure) (:150-173)"""
    a, b, c = cl["Cd4"] + cl["Cc1"], cl["Cd1"] + cl["Cc0"], cl["Cd0"]
    return (-b + math.sqrt(b * b - 4 * a * c)) / (2 * a) * cl["minimum_stratification_number_safety_factor"]


def closure_dict(constant=False, **kw):
    """the reference's defaults, ASCII names, plus "constant" (ConstantStabilityFunctions) and the derived constants"""
    d = {**EQUATIONS, **(CONSTANT if constant else VARIABLE), **LENGTH_SCALE, **CLOSURE}
    for k in kw:
        if k not in d:
            raise TypeError(k)
    d.update(kw)
    d["constant"] = bool(constant)
    if d["Su0"] is None:
        d["Su0"] = log_layer_Su0(d)
    S = d["Su0"]
    d["Su0_cubed"] = S * S * S
    d["Su0_fourth_over_sigma_eps"] = (S * S) * (S * S) / d["C_sigma_eps"]
    d["minimum_stratification_number"] = 0.0 if constant else minimum_stratification_number(d)
    return d


def clamp(x, lo, hi):
    with np.errstate(invalid="ignore"):
        return np.where(x > hi, hi, np.where(x < lo, lo, x))


class State(CK.State):
    """catke_numpy.State with the dissipation `eps` in the place of Jᵇ"""

    def __init__(self, g, zf, zc, Lz, buoyancy, cl, u, v, T, S, e, eps):
        super().__init__(g, zf, zc, Lz, buoyancy, cl, u, v, T, S, e, None)
        self.eps = eps

    def with_tracers(self, e, eps):
        return State(self.g, self.zf, self.zc, self.Lz, self.buoyancy, self.cl, self.u, self.v, self.T, self.S, e, eps)


# ---------------------------------------------------------------------------------------------------------------------------------
# tke_dissipation_vertical_diffusivity.jl, tke_dissipation_stability_functions.jl
# ---------------------------------------------------------------------------------------------------------------------------------
def tke(s, k):
    """turbulent_kinetic_energyᶜᶜᶜ"""
    return jmax(s.cl["minimum_tke"], s.col(s.e, k))


def stratification_plus(s, k):
    """ℑbzᵃᵃᶜ(max_a_b, N²min, ∂z_b)"""
    return CK.bz(s, lambda kk: jmax(s.cl["minimum_buoyancy_frequency"], CK.dz_b(s, kk)), k)


def minimum_dissipation(s, k):
    es = tke(s, k)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        l_st = s.cl["C_N"] * np.sqrt(es / stratification_plus(s, k))
        l_min = jmin(s.Lz, l_st)
        w = np.sqrt(es)
        eps_min = s.cl["Su0_cubed"] * (w * w * w) / l_min
    return jmax(1e-12, eps_min)


def dissipation(s, k):
    """dissipationᶜᶜᶜ"""
    return clamp(s.col(s.eps, k), minimum_dissipation(s, k), np.inf)


def square_time_scale(s, k):
    es, ps = tke(s, k), dissipation(s, k)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return (es * es) / (ps * ps)


def to_face(f, s, k):
    """ℑzᵃᵃᶠ"""
    with np.errstate(invalid="ignore", over="ignore"):
        return 0.5 * (f(s, k - 1) + f(s, k))


def maximum_shear_number(cl, aN):
    n0, n1, d0, d1, d2, d3, d4 = (cl[n] for n in ("Cu0", "Cu1", "Cd0", "Cd1", "Cd2", "Cd3", "Cd4"))
    e0, e1, e2, e3, e4, e5, e6 = d0 * n0, d0 * n1 + d1 * n0, d1 * n1 + d4 * n0, d4 * n1, d2 * n0, d2 * n1 + d3 * n0, d3 * n1
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        num = e0 + e1 * aN + e2 * (aN * aN) + e3 * (aN * aN * aN)
        den = e4 + e5 * aN + e6 * (aN * aN)
        return num / den


def clamped_numbers(s, k, with_raw=False):
    """(αᴺ, αᴹ) as the two variable stability functions clamp them"""
    with np.errstate(invalid="ignore", over="ignore"):
        aN_raw = to_face(square_time_scale, s, k) * CK.dz_b(s, k)      # stratification_numberᶜᶜᶠ
        aM_raw = to_face(square_time_scale, s, k) * CK.shear_ccf(s, k)  # shear_numberᶜᶜᶠ
    aN = clamp(aN_raw, s.cl["minimum_stratification_number"], 1e10)
    aM_max = maximum_shear_number(s.cl, aN)
    aM = clamp(aM_raw, 0.0, aM_max)
    return (aN, aM, aN_raw, aM_raw, aM_max) if with_raw else (aN, aM)


def _denominator(cl, aN, aM):
    return cl["Cd0"] + cl["Cd1"] * aN + cl["Cd2"] * aM + cl["Cd3"] * aN * aM + cl["Cd4"] * (aN * aN) + cl["Cd5"] * (aM * aM)


def momentum_stability_function(s, k):
    cl = s.cl
    if cl["constant"]:
        return cl["Cu0"] + s.zeros()
    aN, aM = clamped_numbers(s, k)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return (cl["Cu0"] + cl["Cu1"] * aN + cl["Cu2"] * aM) / _denominator(cl, aN, aM)


def tracer_stability_function(s, k):
    cl = s.cl
    if cl["constant"]:
        return cl["Cc0"] + s.zeros()
    aN, aM = clamped_numbers(s, k)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return (cl["Cc0"] + cl["Cc1"] * aN + cl["Cc2"] * aM) / _denominator(cl, aN, aM)


def tke_stability_function(s, k):
    return momentum_stability_function(s, k) / s.cl["C_sigma_e"]


def dissipation_stability_function(s, k):
    return momentum_stability_function(s, k) / s.cl["C_sigma_eps"]


STABILITY = {"u": (momentum_stability_function, "maximum_viscosity"), "c": (tracer_stability_function, "maximum_tracer_diffusivity"),
             "e": (tke_stability_function, "maximum_tke_diffusivity"), "eps": (dissipation_stability_function, "maximum_dissipation_diffusivity")}


def kappa_unmasked(s, k, which):
    """κuᶜᶜᶠ, κcᶜᶜᶠ, κeᶜᶜᶠ, κϵᶜᶜᶠ"""
    function, maximum = STABILITY[which]
    e2 = to_face(lambda ss, kk: tke(ss, kk) * tke(ss, kk), s, k)
    eps = to_face(dissipation, s, k)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        kappa = function(s, k) * e2 / eps
    return jmin(kappa, s.cl[maximum])


def kappa_ccf(s, k, which):
    """... with mask_diffusivity: ifelse(on_periphery, 0, κ★) (no cell is inactive on these grids)"""
    return np.where(CK.peripheral(s, k), 0.0, kappa_unmasked(s, k, which))


def diffusivities(s, kappa_u, kappa_c, kappa_e, kappa_eps):
    """compute_TKEDissipation_diffusivities! over :xyz: copies of the four (Center, Center, Face) parents, faces k = 1..Nz of the interior written"""
    g = s.g
    out = [np.array(a, dtype=np.float64) for a in (kappa_u, kappa_c, kappa_e, kappa_eps)]
    for k in range(1, g.Nz + 1):
        for a, which in zip(out, ("u", "c", "e", "eps")):
            a[g.Hx:g.Hx + g.Nx, g.Hy:g.Hy + g.Ny, g.Hz + k - 1] = kappa_ccf(s, k, which)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# tke_dissipation_equations.jl
# ---------------------------------------------------------------------------------------------------------------------------------
def substep(s, u_prev, v_prev, kappa_u, kappa_c, kappa_e, kappa_eps, Le, Leps, Gn_e, Gm_e, Gn_eps, Gm_eps, dtau, chi, with_terms=False):
    """substep_tke_dissipation! (:90-185) over :xyz: (e, ϵ, κᵉ, κᵋ, Le, Lϵ, G⁻e, G⁻ϵ) as copies of the parents, every read of e and ϵ from before
    the call.  with_terms: also a dict of (Nx, Ny, Nz) arrays (what the tests count)"""
    g, cl = s.g, s.cl
    e_new, p_new, ke, kp, Le_out, Lp_out, Gme_out, Gmp_out = (np.array(a, dtype=np.float64)
                                                              for a in (s.e, s.eps, kappa_e, kappa_eps, Le, Leps, Gm_e, Gm_eps))
    alpha, beta = 1.5 + chi, 0.5 + chi
    terms = {name: np.zeros((g.Nx, g.Ny, g.Nz)) for name in ("P", "wb", "N2", "omega_e", "omega_eps", "Le", "Leps", "eps_star", "eps_min")}
    for k in range(1, g.Nz + 1):
        I = (slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny), g.Hz + k - 1)
        ke[I] = kappa_ccf(s, k, "e")
        kp[I] = kappa_ccf(s, k, "eps")
        eps_star, e_star = dissipation(s, k), tke(s, k)
        e, eps = s.col(s.e, k), s.col(s.eps, k)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            omega_star = eps_star / e_star
            omega_e = np.where(e < 0, cl["negative_tke_damping_time_scale"], omega_star)  # (the time scale itself, as the reference has it)
            omega_eps = eps / e_star
            wb = CK.bz(s, lambda kk: -s.col(kappa_c, kk) * CK.dz_b(s, kk), k)  # explicit_buoyancy_flux
            wb_minus, wb_plus = jmin(wb, 0.0), jmax(wb, 0.0)
            wb_e = bmul(wb_minus / e, e > cl["minimum_tke"])
            N2 = 0.5 * (CK.dz_b(s, k) + CK.dz_b(s, k + 1))  # the plain ℑzᵃᵃᶜ
            Cb = np.where(N2 >= 0, cl["C_b_eps_plus"], cl["C_b_eps_minus"])
            Cb_wb_minus, Cb_wb_plus = jmin(Cb * wb, 0.0), jmax(Cb * wb, 0.0)
            L_e = wb_e - omega_e
            L_eps = Cb_wb_minus / e_star - cl["C_eps_eps"] * omega_eps
            P = CK.shear_production(s, k, kappa_u, u_prev, v_prev)
            fast_e = P + wb_plus
            fast_eps = omega_eps * (cl["C_P_eps"] * P + Cb_wb_plus)
            total_e = s.col(Gn_e, k) + fast_e
            total_eps = s.col(Gn_eps, k) + fast_eps
            e_new[I] = e + dtau * (alpha * total_e - beta * s.col(Gm_e, k))
            p_new[I] = eps + dtau * (alpha * total_eps - beta * s.col(Gm_eps, k))
        Le_out[I], Lp_out[I], Gme_out[I], Gmp_out[I] = L_e, L_eps, total_e, total_eps
        for name, a in (("P", P), ("wb", wb), ("N2", N2), ("omega_e", omega_e), ("omega_eps", omega_eps), ("Le", L_e), ("Leps", L_eps),
                        ("eps_star", eps_star), ("eps_min", minimum_dissipation(s, k))):
            terms[name][:, :, k - 1] = a
    out = (e_new, p_new, ke, kp, Le_out, Lp_out, Gme_out, Gmp_out)
    return out + (terms,) if with_terms else out


def implicit_rows(g, kappa, L, dt, i, j):
    """(lower, diagonal, upper) of column (i, j) (0-based interior indices): the diagonal is 1 - Δt L - upper(k) - lower(k - 1)
    (vertically_implicit_diffusion_solver.jl:55-110)"""
    Nz, dz = g.Nz, IDN._dz_at
    kz = lambda k: float(kappa[g.Hx + i, g.Hy + j, g.Hz + k - 1])
    Lc = lambda k: float(L[g.Hx + i, g.Hy + j, g.Hz + k - 1])

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
    return a, b, c


def implicit_matrix(g, kappa, L, dt, i, j):
    """the dense Nz x Nz matrix of those rows: a[k] below the diagonal (row k + 1, column k), c[k] above it"""
    a, b, c = implicit_rows(g, kappa, L, dt, i, j)
    return np.diag(b) + np.diag(a[:-1], -1) + np.diag(c[:-1], 1)


def implicit_step(g, field, kappa, L, dt):
    """implicit_step!(field, ...): the elimination is IDN.thomas (solve_batched_tridiagonal_system_z!)"""
    out = np.array(field, dtype=np.float64)
    for i in range(g.Nx):
        for j in range(g.Ny):
            col = (g.Hx + i, g.Hy + j, slice(g.Hz, g.Hz + g.Nz))
            out[col] = IDN.thomas(*implicit_rows(g, kappa, L, dt, i, j), out[col])
    return out


def top_fluxes(s, top_u, top_v):
    """_top_tke_flux and _top_dissipation_flux (:207-251): (Qe, Qϵ); top_u, top_v as catke_numpy.bc_value takes them"""
    cl, Nz = s.cl, s.g.Nz
    tau_x, tau_y = CK.bc_value(s, top_u, s.u), CK.bc_value(s, top_v, s.v)
    u_star = np.sqrt(np.sqrt(tau_x * tau_x + tau_y * tau_y))
    Qe = -cl["C_W_ustar"] * (u_star * u_star * u_star)
    l_charnock = cl["C_W_alpha"] * (u_star * u_star) / cl["gravitational_acceleration"]
    l_r = jmax(cl["minimum_roughness_length"], l_charnock)
    e_star = tke(s, Nz)
    d = -float(s.zc[Nz - 1])
    return Qe, -cl["Su0_fourth_over_sigma_eps"] * (e_star * e_star) / (d + l_r)


# ---------------------------------------------------------------------------------------------------------------------------------
# the model-level sequence
# ---------------------------------------------------------------------------------------------------------------------------------
def time_step(s, d, Gn_e, Gm_e, Gn_eps, Gm_eps, last_dt, time_step_, chi):
    """time_step_tke_dissipation_equations! (:24-88): (e, ϵ, κᵉ, κᵋ, Le, Lϵ, G⁻e, G⁻ϵ, [χ of every substep])"""
    if time_step_ is None:
        M, dtau = 1, last_dt
    else:
        M = math.ceil(last_dt / time_step_)
        dtau = last_dt / M
    e, eps, ke, kp, Le, Lp, chis = s.e, s.eps, d["kappa_e"], d["kappa_eps"], d["Le"], d["Leps"], []
    for m in range(1, M + 1):
        chi_m = -0.5 if (m == 1 and M != 1) else chi
        chis.append(chi_m)
        e, eps, ke, kp, Le, Lp, Gm_e, Gm_eps = substep(s.with_tracers(e, eps), d["u_prev"], d["v_prev"], d["kappa_u"], d["kappa_c"], ke, kp, Le, Lp,
                                                       Gn_e, Gm_e, Gn_eps, Gm_eps, dtau, chi_m)
        e = implicit_step(s.g, e, ke, Le, dtau)
        eps = implicit_step(s.g, eps, kp, Lp, dtau)
    return e, eps, ke, kp, Le, Lp, Gm_e, Gm_eps, chis


def compute_diffusivities(s, d, tops, last_dt, time_step_, chi, Gn_e, Gm_e, Gn_eps, Gm_eps):
    """compute_diffusivities! (tke_dissipation_vertical_diffusivity.jl:228-256), the x / y halo fill of the four κ and the two top fluxes.
    d: dict with kappa_u, kappa_c, kappa_e, kappa_eps, Le, Leps, u_prev, v_prev (parents); tops: dict u, v of top conditions.  Returns (the
    new dict, e, ϵ, G⁻e, G⁻ϵ, Qe, Qϵ)."""
    e, eps, ke, kp, Le, Lp = s.e, s.eps, d["kappa_e"], d["kappa_eps"], d["Le"], d["Leps"]
    if math.isfinite(last_dt):
        e, eps, ke, kp, Le, Lp, Gm_e, Gm_eps, _ = time_step(s, d, Gn_e, Gm_e, Gn_eps, Gm_eps, last_dt, time_step_, chi)
    s1 = s.with_tracers(e, eps)
    ku, kc, ke, kp = (fill_xy_halos(s.g, a) for a in diffusivities(s1, d["kappa_u"], d["kappa_c"], ke, kp))
    out = dict(kappa_u=ku, kappa_c=kc, kappa_e=ke, kappa_eps=kp, Le=Le, Leps=Lp, u_prev=np.array(s.u), v_prev=np.array(s.v))
    Qe, Qeps = top_fluxes(s1, tops["u"], tops["v"])
    return out, e, eps, Gm_e, Gm_eps, Qe, Qeps


# ---------------------------------------------------------------------------------------------------------------------------------
# the seeded inputs of the GPU tests and their branch shares (checked on the CPU by tests/test_host_tke_dissipation.py)
# ---------------------------------------------------------------------------------------------------------------------------------
P_, B_ = "Periodic", "Bounded"
U, V, CC, CCF = 1, 2, 0, 4  # location masks
SEAWATER = ("SeawaterBuoyancy", 9.80665, 1.67e-4, 7.80e-4)
# size, halo, stretched z: the smallest legal Nz, below one workgroup, ragged second blocks in x (64 lanes) and y (4 rows) with stretched z,
# unequal wide halos and a third block in x
CASES = [((3, 3, 2), (1, 1, 1), False), ((5, 6, 4), (3, 3, 3), False), ((67, 13, 9), (4, 4, 3), True), ((130, 9, 7), (5, 6, 4), False)]
IDS = ["3x3x2", "5x6x4", "67x13x9", "130x9x7"]
LZ = 64.0
MAXIMA = dict(maximum_viscosity=2e-3, maximum_tracer_diffusivity=1e-3, maximum_tke_diffusivity=5e-3, maximum_dissipation_diffusivity=4e-3)


def make_grid(ocn, arch, n):
    from helpers import stretched_faces
    size, halo, stretched = CASES[n]
    z = LZ * stretched_faces(size[2]) if stretched else (-LZ, 0.0)
    return ocn.RectilinearGrid(arch, size=size, x=(0, 1000.0), y=(0, 500.0), z=z, topology=(P_, P_, B_), halo=halo)


def make_inputs(pg, n):
    """Seeded parent arrays, NaN beyond the reach of the entry points (include/ocn_hip.h).  T, S random: N² of both signs, of the size 1e-5;
    u, v random; e negative, within [0, minimum_tke] (both ends included) and above; ϵ zero or tiny (clamped up to its floor), and of the size
    of e^(3/2) / ℓ, so that e² / ϵ² N² and e² / ϵ² S² fall on both sides of their bounds"""
    g = IDN.describe(pg)
    rng = np.random.default_rng(4400 + n)
    Nx, Ny, Nz, Hx, Hy, Hz = g.Nx, g.Ny, g.Nz, g.Hx, g.Hy, g.Hz
    sx, sy, sz = slice(Hx, Hx + Nx), slice(Hy, Hy + Ny), slice(Hz, Hz + Nz)

    def masked(full, keep):
        out = np.full(full.shape, np.nan)
        out[keep] = full[keep]
        return out
    u, v = (0.05 * rng.uniform(-1, 1, pg.parent_shape(loc)) for loc in (U, V))
    T = 20 + 0.05 * rng.uniform(-1, 1, pg.parent_shape(CC))
    S = 35 + 0.01 * rng.uniform(-1, 1, pg.parent_shape(CC))
    kind = rng.uniform(0, 1, pg.parent_shape(CC))
    emin = CLOSURE["minimum_tke"]
    e = np.where(kind < 0.2, -1e-5 * rng.uniform(0.1, 1, kind.shape),
                 np.where(kind < 0.4, emin * rng.uniform(0, 1, kind.shape), 10.0 ** rng.uniform(-5.5, -3, kind.shape)))
    e = np.where((kind >= 0.2) & (kind < 0.25), 0.0, np.where((kind >= 0.25) & (kind < 0.28), emin, e))
    pk = rng.uniform(0, 1, pg.parent_shape(CC))
    eps = np.where(pk < 0.15, 0.0, np.where(pk < 0.3, 10.0 ** rng.uniform(-14, -11, pk.shape), 10.0 ** rng.uniform(-9, -6, pk.shape)))
    cells, tops = (sx, sy, sz), (sx, sy, slice(Hz - 1, Hz + Nz + 1))
    return dict(g=g, u=masked(u, (slice(Hx, Hx + Nx + 1), sy, sz)), v=masked(v, (sx, slice(Hy, Hy + Ny + 1), sz)), T=masked(T, tops), S=masked(S, tops),
                e=masked(e, cells), eps=masked(eps, cells),
                u_prev=masked(u + 0.01 * rng.uniform(-1, 1, u.shape), (slice(Hx, Hx + Nx + 1), sy, sz)),
                v_prev=masked(v + 0.01 * rng.uniform(-1, 1, v.shape), (sx, slice(Hy, Hy + Ny + 1), sz)),
                Gn_e=masked(1e-8 * rng.uniform(-1, 1, e.shape), cells), Gm_e=masked(1e-8 * rng.uniform(-1, 1, e.shape), cells),
                Gn_eps=masked(1e-11 * rng.uniform(-1, 1, e.shape), cells), Gm_eps=masked(1e-11 * rng.uniform(-1, 1, e.shape), cells),
                flux_u=1e-4 * rng.uniform(-1, 1, (Nx, Ny)))


def tracers_of(c, buoyancy):
    """(spec of the restatement, T, S): the buoyancy tracer is g (α T - β S) itself"""
    if buoyancy == "SeawaterBuoyancy":
        return SEAWATER, c["T"], c["S"]
    return "BuoyancyTracer", SEAWATER[1] * (SEAWATER[2] * c["T"] - SEAWATER[3] * c["S"]), None


def state_of(pg, c, buoyancy, cl=None, e=None, eps=None):
    spec, T, S = tracers_of(c, buoyancy)
    return State(c["g"], pg.nodes_1d(2, True), pg.nodes_1d(2, False), pg.Lz, spec, cl or closure_dict(), c["u"], c["v"], T, S,
                 c["e"] if e is None else e, c["eps"] if eps is None else eps)


def branch_shares(s, kappas, terms):
    """the share of the interior faces (k = 2..Nz) / cells in every branch; s: a state with the clipping MAXIMA and the variable stability
    functions, kappas: its four diffusivities (parents), terms: the dict of `substep` for the same state"""
    g, cl = s.g, s.cl
    faces = {name: [] for name in ("alpha_N_at_minimum", "alpha_M_at_maximum")}
    for k in range(2, g.Nz + 1):
        aN, aM, aN_raw, aM_raw, aM_max = clamped_numbers(s, k, with_raw=True)
        faces["alpha_N_at_minimum"].append(aN_raw < cl["minimum_stratification_number"])
        faces["alpha_M_at_maximum"].append(aM_raw > aM_max)
    out = {name: float(np.mean(v)) for name, v in faces.items()}
    inner = (slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny))
    e, eps = (a[inner][:, :, g.Hz:g.Hz + g.Nz] for a in (s.e, s.eps))
    out.update(eps_clamped_up=float(np.mean(eps < terms["eps_min"])), e_negative=float(np.mean(e < 0)),
               e_at_most_minimum=float(np.mean(e <= cl["minimum_tke"])), wb_positive=float(np.mean(terms["wb"] > 0)),
               wb_negative=float(np.mean(terms["wb"] < 0)), N2_negative=float(np.mean(terms["N2"] < 0)),
               N2_not_negative=float(np.mean(terms["N2"] >= 0)))
    for which, a in zip(("u", "c", "e", "eps"), kappas):
        interior = a[inner][:, :, g.Hz + 1:g.Hz + g.Nz]
        out[f"kappa_{which}_at_maximum"] = float(np.mean(interior == cl[STABILITY[which][1]]))
    return out


SHARES_CLOSURE = dict(C_W_ustar=2.5, C_b_eps_minus=-0.4, **MAXIMA)  # (variable stability functions, clipping maxima)


def substep_inputs(g, kappas):
    """κᵘ and κᶜ as the substep may read them: κᵘ with its x / y halos filled and NaN beyond one column and outside faces 2..Nz, κᶜ in the column"""
    ku_h = fill_xy_halos(g, kappas[0])
    box, kc = np.full(ku_h.shape, np.nan), np.full(ku_h.shape, np.nan)
    sl1 = (slice(g.Hx - 1, g.Hx + g.Nx + 1), slice(g.Hy - 1, g.Hy + g.Ny + 1), slice(g.Hz + 1, g.Hz + g.Nz))
    sl0 = (slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny), slice(g.Hz + 1, g.Hz + g.Nz))
    box[sl1], kc[sl0] = ku_h[sl1], kappas[1][sl0]
    return box, kc


def shares_of_case(pg, c, buoyancy):
    """the branch shares of a seeded case, from the restatement alone: its diffusivities, then one substep"""
    g = c["g"]
    s = state_of(pg, c, buoyancy, closure_dict(**SHARES_CLOSURE))
    sentinel, cells = np.full(ccf_shape(g), -7.0), np.full(pg.parent_shape(CC), -7.0)
    kappas = diffusivities(s, sentinel, sentinel, sentinel, sentinel)
    box, kc = substep_inputs(g, kappas)
    terms = substep(s, c["u_prev"], c["v_prev"], box, kc, sentinel, sentinel, cells, cells, c["Gn_e"], c["Gm_e"], c["Gn_eps"], c["Gm_eps"], 90.0, 0.1,
                    with_terms=True)[-1]
    return branch_shares(s, kappas, terms)
