"""ConvectiveAdjustmentVerticalDiffusivity and the field-valued vertically implicit step restated in NumPy, operand for operand, on parent
arrays indexed [i, j, k] with halos (Field.parent()); a (Center, Center, Face) parent has Nz + 2 Hz + 1 planes, face k at index Hz + k - 1:

  compute_convective_adjustment_diffusivities!   turbulence_closure_implementations/convective_adjustment_vertical_diffusivity.jl:91-123,
                                                 launched over :xyz (update_hydrostatic_free_surface_model_state.jl:74-97)
  ∂z_b                                           buoyancy_tracer.jl:16, seawater_buoyancy.jl:219-224
  ivd_upper / lower_diagonal, ivd_diagonal       vertically_implicit_diffusion_solver.jl:55-78, 107-110 (the Center-in-z rows)
  κz at (c, c, c), (f, c, c), (c, f, c)          abstract_scalar_diffusivity_closure.jl:307-315 for a (Center, Center, Face) array
  viscous_flux_uz / vz, diffusive_flux_z         abstract_scalar_diffusivity_closure.jl:198-211 (VerticalFormulation), :221-260 (vertically
                                                 implicit on a vertically bounded grid), divergences closure_kernel_operators.jl:27-53

Written from those files.  The elimination, the dense matrix and the grid description are those of tests/implicit_diffusion_numpy.py;
tests/test_host_convective_adjustment.py pins this file without a GPU."""
import numpy as np

import implicit_diffusion_numpy as IDN

_sh, _dzC, _dzF, _boundary = IDN._sh, IDN._dzC, IDN._dzF, IDN._boundary


def ccf_shape(g):
    return (g.Nx + 2 * g.Hx, g.Ny + 2 * g.Hy, g.Nz + 2 * g.Hz + 1)


# ---------------------------------------------------------------------------------------------------------------------------------
# the diffusivities
# ---------------------------------------------------------------------------------------------------------------------------------
def dz_b(g, buoyancy, T=None, S=None):
    """∂z_b at faces k = 1..Nz over the interior in x and y.  buoyancy: None, "BuoyancyTracer" (T is b) or ("SeawaterBuoyancy", g, α, β);
    a missing (constant) T or S has derivative 0"""
    if buoyancy is None:
        return np.zeros((g.Nx, g.Ny, g.Nz))
    dzf = _dzF(g, 0)
    dT = (_sh(g, T, 0, 0, 0) - _sh(g, T, 0, 0, -1)) / dzf if T is not None else 0.0
    if buoyancy == "BuoyancyTracer":
        return dT + np.zeros((g.Nx, g.Ny, g.Nz))
    dS = (_sh(g, S, 0, 0, 0) - _sh(g, S, 0, 0, -1)) / dzf if S is not None else 0.0
    _, grav, alpha, beta = buoyancy[:4]
    return grav * (alpha * dT - beta * dS) + np.zeros((g.Nx, g.Ny, g.Nz))


def diffusivities(g, buoyancy, T, S, convective_kappa_z, convective_nu_z, background_kappa_z, background_nu_z, kappa_c, kappa_u):
    """copies of the two (Center, Center, Face) parents with faces k = 1..Nz of the interior written: face Nz + 1 and every halo keep what
    they held.  A gradient of exactly 0 is stable."""
    stable = dz_b(g, buoyancy, T, S) >= 0
    kc, ku = np.array(kappa_c, dtype=np.float64), np.array(kappa_u, dtype=np.float64)
    sl = (slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny), slice(g.Hz, g.Hz + g.Nz))
    kc[sl] = np.where(stable, background_kappa_z, convective_kappa_z)
    ku[sl] = np.where(stable, background_nu_z, convective_nu_z)
    return kc, ku


def no_flux_parent(g, interior, random_bottom=None):
    """the parent of a Center field on (Periodic, Periodic, Bounded) with default conditions: periodic x / y halos, the first z halo plane
    mirrors the boundary cell, the others are 0.  random_bottom: a generator -- the bottom halo plane of the columns with an even i holds
    random values instead, as a Value or Gradient condition would leave it (a single layer then has faces of every kind)"""
    a = np.pad(interior, ((g.Hx, g.Hx), (g.Hy, g.Hy), (0, 0)), mode="wrap")
    a = np.pad(a, ((0, 0), (0, 0), (g.Hz, g.Hz)), mode="constant")
    a[:, :, g.Hz - 1] = a[:, :, g.Hz]
    a[:, :, g.Hz + g.Nz] = a[:, :, g.Hz + g.Nz - 1]
    if random_bottom is not None:
        even = (np.arange(a.shape[0]) - g.Hx + 1) % 2 == 0
        a[even, :, g.Hz - 1] = random_bottom.uniform(-1, 1, a[even, :, g.Hz - 1].shape)
    return a


def plateau_inputs(g, seed):
    """Seeded T and S parents that reach every branch of the classification: uniformly random in [-1, 1], a plateau over three levels in
    both where Nz >= 4 (two faces per column with ∂z b == 0 exactly), over a no-flux bottom in the columns with an odd i (face 1:
    ∂z b == 0 exactly) and a random bottom halo in the others"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(2):
        a = rng.uniform(-1, 1, (g.Nx, g.Ny, g.Nz))
        if g.Nz >= 4:
            k0 = g.Nz // 2
            a[:, :, k0:k0 + 3] = a[:, :, k0:k0 + 1]
        out.append(no_flux_parent(g, a, random_bottom=rng))
    return out


def fill_xy_halos(g, parent):
    """the Periodic x and y halos of every plane (fill_halo_regions!(diffusivity_fields; only_local_halos = true) on a (Periodic, Periodic,
    Bounded) grid: a ZFaceField that is no velocity has nothing filled in z)"""
    inner = parent[g.Hx:g.Hx + g.Nx, g.Hy:g.Hy + g.Ny, :]
    return np.pad(inner, ((g.Hx, g.Hx), (g.Hy, g.Hy), (0, 0)), mode="wrap")


# ---------------------------------------------------------------------------------------------------------------------------------
# the implicit step
# ---------------------------------------------------------------------------------------------------------------------------------
def diagonals_fields(g, dt, kappa_column):
    """(a, b, c) as IDN.diagonals returns them, for the Center-in-z rows with κz(k) = kappa_column[k - 1], k = 1..Nz + 1"""
    Nz, dt = g.Nz, float(dt)
    kz = lambda k: float(kappa_column[k - 1])
    dz = IDN._dz_at

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
        up = upper(k)
        a[k - 1] = lower(k) if k < Nz else 0.0
        b[k - 1] = (1.0 - up) - lower(k - 1)
        c[k - 1] = up
    return a, b, c


def kappa_z_column(g, kappa, loc, i, j):
    """κz(i, j, k), k = 1..Nz + 1, for a field at `loc` (bit 0 x-face, bit 1 y-face): κ itself, ℑxᶠᵃᵃ(κ) or ℑyᵃᶠᵃ(κ); i, j 1-based"""
    I, J = g.Hx + i - 1, g.Hy + j - 1
    here = kappa[I, J, g.Hz:g.Hz + g.Nz + 1]
    if loc & 1:
        return 0.5 * (kappa[I - 1, J, g.Hz:g.Hz + g.Nz + 1] + here)
    if loc & 2:
        return 0.5 * (kappa[I, J - 1, g.Hz:g.Hz + g.Nz + 1] + here)
    return here


def implicit_step_fields(g, parent, loc, kappa, dt):
    """implicit_step!(field, ...) with the (Center, Center, Face) parent `kappa`: a copy of the field's parent with columns i = 1..Nx,
    j = 1..Ny, rows k = 1..Nz solved"""
    if loc & 4:
        raise ValueError("Face-in-z fields have no field-valued implicit step")
    out = np.array(parent, dtype=np.float64)
    for i in range(1, g.Nx + 1):
        for j in range(1, g.Ny + 1):
            a, b, c = diagonals_fields(g, dt, kappa_z_column(g, kappa, loc, i, j))
            col = (g.Hx + i - 1, g.Hy + j - 1, slice(g.Hz, g.Hz + g.Nz))
            out[col] = IDN.thomas(a, b, c, out[col])
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the closure term
# ---------------------------------------------------------------------------------------------------------------------------------
def _explicit_faces(g, dk, boundary_only):
    return _boundary(g, dk) if boundary_only else np.ones((1, 1, g.Nz), dtype=bool)


def vertical_fluxes(g, kappa_u, u, v, kappa_c, tracers, boundary_only):
    """(Du, Dv, [Dc, ...]) over (1..Nx, 1..Ny, 1..Nz): ∂ⱼτ₁ⱼ, ∂ⱼτ₂ⱼ and ∇_dot_qᶜ of a VerticalFormulation closure with the (Center, Center,
    Face) parents kappa_u (viscosity) and kappa_c[n]; the tendencies are G - D.  boundary_only: the vertically implicit variant."""
    Az = g.dx * g.dy
    dzc = _dzC(g, 0)
    ex = lambda dk: _explicit_faces(g, dk, boundary_only)
    out = []
    for field, back in ((u, (-1, 0)), (v, (0, -1))):
        if field is None:
            out.append(None)
            continue
        nu = lambda dk: 0.5 * (_sh(g, kappa_u, back[0], back[1], dk) + _sh(g, kappa_u, 0, 0, dk))
        flux = lambda dk: np.where(ex(dk), -(nu(dk) * ((_sh(g, field, 0, 0, dk) - _sh(g, field, 0, 0, dk - 1)) / _dzF(g, dk))), 0.0)
        dzF = Az * flux(1) - Az * flux(0)
        out.append(1 / (Az * dzc) * ((0.0 + 0.0) + dzF))
    Dc = []
    for kappa, c in zip(kappa_c, tracers):
        flux = lambda dk: np.where(ex(dk), -(_sh(g, kappa, 0, 0, dk) * ((_sh(g, c, 0, 0, dk) - _sh(g, c, 0, 0, dk - 1)) / _dzF(g, dk))), 0.0)
        dzF = Az * flux(1) - Az * flux(0)
        Dc.append(1 / (Az * dzc) * ((0.0 + 0.0) + dzF))
    return out[0], out[1], Dc
