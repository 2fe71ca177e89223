"""RiBasedVerticalDiffusivity restated in NumPy, operand for operand, on parent arrays indexed [i, j, k] with halos (Field.parent()); a (Center,
Center, Face) parent has Nz + 2 Hz + 1 planes, face k at index Hz + k - 1:

  taper(::Linear | ::Exp | ::Tanh, x, x₀, δ)      turbulence_closure_implementations/ri_based_vertical_diffusivity.jl:239-241
  shear_squaredᶜᶜᶠ, Riᶜᶜᶠ, compute_ri_number!     :243-267, with ℑxᶜᵃᵃ / ℑyᵃᶜᵃ of Operators/interpolation_operators.jl:21-24
  filter_horizontally(::FivePointHorizontalFilter) :56, ℑxyᶜᶜᵃ / ℑxyᶠᶠᵃ of interpolation_operators.jl:45-47
  _compute_ri_based_diffusivities!                :277-341, launched over :xyz (compute_diffusivities!, :193-229)
  top_buoyancy_flux                               BuoyancyFormulations/seawater_buoyancy.jl:234-246, buoyancy_tracer.jl:18
  ∂z_b                                            tests/convective_adjustment_numpy.py (seawater_buoyancy.jl:219-224, buoyancy_tracer.jl:16)

Written from those files.  exp and tanh are NOT NumPy's: `exp_nonpositive` and `tanh_absolute` restate the hand-written ones of
csrc/ocn_taper.h (no math library on the device either), every operation an IEEE +, -, *, / of Float64 or an exact power of two, in the same
order.  tests/test_host_ri_based.py pins this file without a GPU."""
from types import SimpleNamespace

import numpy as np

import convective_adjustment_numpy as CAN
import implicit_diffusion_numpy as IDN

_sh, _dzF = IDN._sh, IDN._dzF
ccf_shape, fill_xy_halos = CAN.ccf_shape, CAN.fill_xy_halos

LINEAR, EXP, TANH = 0, 1, 2          # OCN_RI_TAPER_*
FILTER_NONE, FILTER_FIVE_POINT = 0, 1  # OCN_RI_FILTER_*

INV_LN2, LN2_HI, LN2_LO = 1.4426950408889634, 6.93147180369123816490e-01, 1.90821492927058770002e-10
MAGIC = 6755399441055744.0  # 1.5 * 2^52
_FACTORIALS = [1.0, 1.0, 2.0, 6.0, 24.0, 120.0, 720.0, 5040.0, 40320.0, 362880.0, 3628800.0, 39916800.0, 479001600.0, 6227020800.0]


# ---------------------------------------------------------------------------------------------------------------------------------
# csrc/ocn_taper.h
# ---------------------------------------------------------------------------------------------------------------------------------
def exp_nonpositive(x):
    """exp(x) for x <= 0: NaN stays, x < -746 gives 0; k = nearest integer to x / ln 2 by the 1.5 * 2^52 trick, r = (x - k LN2_HI) - k LN2_LO,
    Σ r^n / n! (n <= 13) by Horner's rule, scaled by 2^-h then 2^(k + h), h = -k / 2"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        nan, tiny = x != x, x < -746.0
        xs = np.where(nan | tiny, 0.0, x)
        kd = (xs * INV_LN2 + MAGIC) - MAGIC
        r = (xs - kd * LN2_HI) - kd * LN2_LO
        p = np.full(xs.shape, 1.0 / _FACTORIALS[13])
        for n in range(12, 1, -1):
            p = 1.0 / _FACTORIALS[n] + r * p
        p = 1.0 + r * p
        p = 1.0 + r * p
        k = kd.astype(np.int64)
        h = (-k) // 2
        out = (p * np.ldexp(1.0, -h)) * np.ldexp(1.0, k + h)
    return np.where(nan, x, np.where(tiny, 0.0, out))


def tanh_absolute(x):
    """±(1 - e) / (1 + e), e = exp_nonpositive(-2 |x|); ±1 for |x| > 20; NaN stays"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        neg = x < 0
        a = np.where(neg, -x, x)
        big = a > 20.0
        e = exp_nonpositive(-(2.0 * np.where(big, 0.0, a)))
        t = (1.0 - e) / (1.0 + e)
        t = np.where(neg, -t, t)
    return np.where(big, np.where(neg, -1.0, 1.0), t)


def _max_zero(q):
    with np.errstate(invalid="ignore"):
        return np.where(q != q, q, np.where(q > 0.0, q, 0.0))


def _min_one(q):
    with np.errstate(invalid="ignore"):
        return np.where(q != q, q, np.where(q < 1.0, q, 1.0))


def taper(kind, x, x0, delta):
    """taper(tapering, x, x₀, δ) (:239-241) with the hand-written exp / tanh"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = (x - x0) / delta
    if kind == LINEAR:
        return 1.0 - _min_one(_max_zero(q))
    if kind == EXP:
        return exp_nonpositive(-_max_zero(q))
    if kind == TANH:
        return (1.0 - tanh_absolute(q)) / 2.0
    raise ValueError(f"unknown tapering {kind}")


def taper_reference(kind, x, x0, delta, dtype=np.float64):
    """the reference formulas (:239-241) with the dtype's own min, max, exp and tanh: Float64 (τ₆₄) or np.longdouble (the oracle)"""
    x, x0, delta = np.asarray(x, dtype=dtype), dtype(x0), dtype(delta)
    one, zero = dtype(1), dtype(0)
    with np.errstate(invalid="ignore", divide="ignore", under="ignore"):
        q = (x - x0) / delta
        if kind == LINEAR:
            return one - np.minimum(one, np.maximum(zero, q))
        if kind == EXP:
            return np.exp(-np.maximum(zero, q))
        return (one - np.tanh(q)) / dtype(2)


# ---------------------------------------------------------------------------------------------------------------------------------
# compute_ri_number!
# ---------------------------------------------------------------------------------------------------------------------------------
def dz_b(g, buoyancy, T, S, dk=0):
    """∂z_b at faces k + dk, k = 1..Nz (CAN.dz_b is dk = 0)"""
    if buoyancy is None:
        return np.zeros((g.Nx, g.Ny, g.Nz))
    dzf = _dzF(g, dk)
    dT = (_sh(g, T, 0, 0, dk) - _sh(g, T, 0, 0, dk - 1)) / dzf if T is not None else 0.0
    if buoyancy == "BuoyancyTracer":
        return dT + np.zeros((g.Nx, g.Ny, g.Nz))
    dS = (_sh(g, S, 0, 0, dk) - _sh(g, S, 0, 0, dk - 1)) / dzf if S is not None else 0.0
    _, grav, alpha, beta = buoyancy[:4]
    return grav * (alpha * dT - beta * dS) + np.zeros((g.Nx, g.Ny, g.Nz))


def shear_squared(g, u, v):
    """shear_squaredᶜᶜᶠ (:245-249): ℑxᶜᵃᵃ(ϕ², ∂zᶠᶜᶠ, u) + ℑyᵃᶜᵃ(ϕ², ∂zᶜᶠᶠ, v) at faces 1..Nz"""
    dzf = _dzF(g, 0)
    du = lambda di: (_sh(g, u, di, 0, 0) - _sh(g, u, di, 0, -1)) / dzf
    dv = lambda dj: (_sh(g, v, 0, dj, 0) - _sh(g, v, 0, dj, -1)) / dzf
    dzu2 = 0.5 * (du(0) * du(0) + du(1) * du(1))
    dzv2 = 0.5 * (dv(0) * dv(0) + dv(1) * dv(1))
    return dzu2 + dzv2


def ri_number(g, buoyancy, u, v, T, S, Ri):
    """a copy of the (Center, Center, Face) parent Ri with faces k = 1..Nz of the interior written (:251-267): Ri = N² <= 0 ? 0 : N² / S²"""
    N2 = dz_b(g, buoyancy, T, S)
    with np.errstate(divide="ignore", invalid="ignore"):
        ri = np.where(N2 <= 0, 0.0, N2 / shear_squared(g, u, v))
    out = np.array(Ri, dtype=np.float64)
    out[g.Hx:g.Hx + g.Nx, g.Hy:g.Hy + g.Ny, g.Hz:g.Hz + g.Nz] = ri
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# compute_ri_based_diffusivities!
# ---------------------------------------------------------------------------------------------------------------------------------
def five_point_filter(g, Ri):
    """ℑxyᶜᶜᵃ(i, j, k, grid, ℑxyᶠᶠᵃ, Ri) over the interior, faces 1..Nz: ℑxyᶠᶠᵃ = ℑyᵃᶠᵃ(ℑxᶠᵃᵃ ·), ℑxyᶜᶜᵃ = ℑyᵃᶜᵃ(ℑxᶜᵃᵃ ·)"""
    R = lambda di, dj: _sh(g, Ri, di, dj, 0)
    with np.errstate(invalid="ignore"):
        ff = lambda di, dj: 0.5 * (0.5 * (R(di - 1, dj - 1) + R(di, dj - 1)) + 0.5 * (R(di - 1, dj) + R(di, dj)))
        return 0.5 * (0.5 * (ff(0, 0) + ff(1, 0)) + 0.5 * (ff(0, 1) + ff(1, 1)))


def filter_weights():
    """the nine weights of the filter: its response to a unit impulse at each of the 3 x 3 neighbours"""
    g = SimpleNamespace(Nx=1, Ny=1, Nz=1, Hx=1, Hy=1, Hz=0)
    w = np.zeros((3, 3))
    for a in range(3):
        for b in range(3):
            Ri = np.zeros((3, 3, 1))
            Ri[a, b, 0] = 1.0
            w[a, b] = five_point_filter(g, Ri)[0, 0, 0]
    return w


def bc_value(g, bc, c):
    """getbc of a top condition over the interior columns: None (no flux: 0), a number, an (Nx, Ny) array, or (value, coeff): value + coeff *
    c[i, j, Nz]"""
    if bc is None:
        return np.zeros((g.Nx, g.Ny))
    if isinstance(bc, tuple):
        value, coeff = bc
        return value + coeff * c[g.Hx:g.Hx + g.Nx, g.Hy:g.Hy + g.Ny, g.Hz + g.Nz - 1]
    return np.zeros((g.Nx, g.Ny)) + np.asarray(bc, dtype=np.float64)


def top_buoyancy_flux(g, buoyancy, T, S, top_T, top_S):
    if buoyancy is None:
        return np.zeros((g.Nx, g.Ny))
    JT = bc_value(g, top_T, T) if T is not None else np.zeros((g.Nx, g.Ny))
    if buoyancy == "BuoyancyTracer":
        return JT
    JS = bc_value(g, top_S, S) if S is not None else np.zeros((g.Nx, g.Ny))
    _, grav, alpha, beta = buoyancy[:4]
    return grav * (alpha * JT - beta * JS)


def _min_with(a, m):
    with np.errstate(invalid="ignore"):
        return np.where(a != a, a, np.where(a < m, a, m))


def new_diffusivities(g, buoyancy, cl, T, S, top_T, top_S, Ri):
    """(κᶜ⁺, κᵘ⁺, branches) at faces 1..Nz from an Ri parent whose x / y halos are filled: the values before the time average (:293-334).
    cl: a dict with the fields of struct ocn_ri_based.  branches: dict of boolean arrays (what the tests count)"""
    Jb = top_buoyancy_flux(g, buoyancy, T, S, top_T, top_S)[:, :, None]
    N2, N2_above = dz_b(g, buoyancy, T, S), dz_b(g, buoyancy, T, S, 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        convecting = N2 < 0
        entraining = (N2 > cl["minimum_entrainment_buoyancy_gradient"]) & (N2_above < 0) & (Jb > 0)
        k_ca = np.where(convecting, cl["kappa_ca"], 0.0)
        k_en = np.where(entraining, cl["C_en"] * Jb / N2, 0.0)
        ri = five_point_filter(g, Ri) if cl["horizontal_filter"] == FILTER_FIVE_POINT else _sh(g, Ri, 0, 0, 0)
        tau = taper(cl["tapering"], ri, cl["Ri0"], cl["Ri_delta"])
        kc_raw = k_ca + k_en + cl["kappa0"] * tau
        ku_raw = cl["nu0"] * tau
    kc = _min_with(kc_raw, cl["maximum_diffusivity"])
    ku = _min_with(ku_raw, cl["maximum_viscosity"])
    kc[:, :, 0] = 0.0  # peripheral_node(i, j, 1, grid, c, c, f)
    ku[:, :, 0] = 0.0
    branches = dict(convecting=convecting, entraining=entraining, tau=tau, Ri=ri, clipped_c=kc_raw > cl["maximum_diffusivity"],
                    clipped_u=ku_raw > cl["maximum_viscosity"])
    return kc, ku, branches


def diffusivities(g, buoyancy, cl, T, S, top_T, top_S, Ri, kappa_c, kappa_u, with_branches=False):
    """copies of the κᶜ, κᵘ parents with κ <- (Cᵃᵛ κ + κ⁺) / (1 + Cᵃᵛ) at faces 1..Nz of the interior (:337-338); face Nz + 1 and every halo
    keep what they held"""
    kc_new, ku_new, branches = new_diffusivities(g, buoyancy, cl, T, S, top_T, top_S, Ri)
    sl = (slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny), slice(g.Hz, g.Hz + g.Nz))
    kc, ku = np.array(kappa_c, dtype=np.float64), np.array(kappa_u, dtype=np.float64)
    Cav = cl["C_av"]
    with np.errstate(invalid="ignore"):
        kc[sl] = (Cav * kc[sl] + kc_new) / (1 + Cav)
        ku[sl] = (Cav * ku[sl] + ku_new) / (1 + Cav)
    return (kc, ku, branches) if with_branches else (kc, ku)


def closure_dict(**kw):
    """the reference's defaults (:125-139), ASCII names of struct ocn_ri_based"""
    d = dict(nu0=0.7, kappa0=0.5, kappa_ca=1.7, C_en=0.1, C_av=0.6, Ri0=0.1, Ri_delta=0.4, minimum_entrainment_buoyancy_gradient=1e-10,
             maximum_diffusivity=np.inf, maximum_viscosity=np.inf, tapering=TANH, horizontal_filter=FILTER_NONE)
    for k in kw:
        if k not in d:
            raise TypeError(k)
    d.update(kw)
    return d


def fill_xy_halos_topology(g, parent):
    """fill_halo_regions!(Ri) in x and y: Periodic wraps; Bounded with the default (no-flux) condition mirrors the boundary cell into the
    first halo plane (the only one the filter reads) and leaves the others; x first, then y, each over the full extent of the other"""
    a = np.array(parent, dtype=np.float64)
    for axis, (N, H, topo) in enumerate(((g.Nx, g.Hx, g.topo[0]), (g.Ny, g.Hy, g.topo[1]))):
        a = np.moveaxis(a, axis, 0)
        if topo == "Periodic":
            a[:H] = a[N:N + H]
            a[N + H:N + 2 * H] = a[H:2 * H]
        else:
            a[H - 1] = a[H]
            a[N + H] = a[N + H - 1]
        a = np.moveaxis(a, 0, axis)
    return a
