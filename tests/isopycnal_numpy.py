"""IsopycnalSkewSymmetricDiffusivity (SmallSlopeIsopycnalTensor, FluxTapering, vertically implicit, number coefficients) restated in NumPy,
operator for operator and in the reference's order of operations, on parent arrays indexed [i, j, k] with halos (Field.parent()), for a
(Periodic, Periodic, Bounded) grid that is regular in x and y:

  ∂x_b, ∂y_b, ∂z_b                                   BuoyancyFormulations/buoyancy_tracer.jl:14-16, seawater_buoyancy.jl:167-224
  ℑxᶠᵃᵃ ... ℑyzᵃᶜᶠ                                    Operators/interpolation_operators.jl:21-28, 45-56
  calc_tapering, tapering_factorᶠᶜᶜ / ᶜᶠᶜ / ᶜᶜᶠ          turbulence_closure_implementations/isopycnal_skew_symmetric_diffusivity.jl:174-212
  isopycnal_rotation_tensor_xz_fcc ... zz_ccf        TurbulenceClosures/isopycnal_rotation_tensor_components.jl:66-127
  compute_tapered_R₃₃!                               isopycnal_skew_symmetric_diffusivity.jl:134-143
  Sxᶠᶜᶠ, Syᶜᶠᶠ, _compute_eddy_velocities!             turbulence_closure_implementations/advective_skew_diffusion.jl:26-76
  diffusive_flux_x / y / z, κzᶜᶜᶠ                      isopycnal_skew_symmetric_diffusivity.jl:229-314, 327-332
  ∇_dot_qᶜ                                           TurbulenceClosures/closure_kernel_operators.jl:43-48
  the halo fill of the diffusivity fields            update_hydrostatic_free_surface_model_state.jl:47 with BoundaryConditions/
                                                     field_boundary_conditions.jl:15-37, fill_halo_regions_open.jl:65-70
  SumOfArrays{2}                                     Utils/sum_of_arrays.jl:23

Every operator is a function of an index shift (a, b, c): its value at (i + a, j + b, k + c) for all interior (i, j, k) at once, so an
operator nested in an interpolation or a difference is written as the reference nests it.  Julia's min, max and ifelse are written with
np.where: both branches are evaluated, the 0 / 0 and x / 0 of the branch not taken are selected away.  The grid description is
tests/implicit_diffusion_numpy.py's `describe`; `buoyancy` is ("BuoyancyTracer",) with T holding b and S = None, or
("SeawaterBuoyancy", g, α, β) with T and S (either may be None: a constant)."""
from types import SimpleNamespace

import numpy as np

import implicit_diffusion_numpy as IDN

_sh, _dzC, _dzF, _boundary = IDN._sh, IDN._dzC, IDN._dzF, IDN._boundary
EPS = IDN.EPS
TRACER = ("BuoyancyTracer",)


def closure(max_slope=1e-2, minimum_bz=0.0):
    return SimpleNamespace(max_slope=float(max_slope), minimum_bz=float(minimum_bz))


# ---- Julia's semantics ------------------------------------------------------------------------------------------------------------------------
def jl_max(a, b):
    """max(a, b): a NaN propagates, max(-0.0, 0.0) is 0.0"""
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    return np.where(np.isnan(a), a, np.where(np.isnan(b), b, np.where(a > b, a, np.where(b > a, b, np.where(np.signbit(a), b, a)))))


def min_one(x):
    """min(one(grid), x)"""
    return np.where(np.isnan(x), x, np.where(x < 1.0, x, 1.0))


# ---- interpolations of a function of a shift --------------------------------------------------------------------------------------------------
ix_f = lambda f: lambda a, b, c: 0.5 * (f(a - 1, b, c) + f(a, b, c))  # ℑxᶠᵃᵃ
ix_c = lambda f: lambda a, b, c: 0.5 * (f(a, b, c) + f(a + 1, b, c))  # ℑxᶜᵃᵃ
iy_f = lambda f: lambda a, b, c: 0.5 * (f(a, b - 1, c) + f(a, b, c))  # ℑyᵃᶠᵃ
iy_c = lambda f: lambda a, b, c: 0.5 * (f(a, b, c) + f(a, b + 1, c))  # ℑyᵃᶜᵃ
iz_f = lambda f: lambda a, b, c: 0.5 * (f(a, b, c - 1) + f(a, b, c))  # ℑzᵃᵃᶠ
iz_c = lambda f: lambda a, b, c: 0.5 * (f(a, b, c) + f(a, b, c + 1))  # ℑzᵃᵃᶜ
ixy_fc = lambda f: iy_c(ix_f(f))  # ℑxyᶠᶜᵃ = ℑyᵃᶜᵃ(ℑxᶠᵃᵃ)
ixy_cf = lambda f: iy_f(ix_c(f))  # ℑxyᶜᶠᵃ = ℑyᵃᶠᵃ(ℑxᶜᵃᵃ)
ixz_fc = lambda f: iz_c(ix_f(f))  # ℑxzᶠᵃᶜ = ℑzᵃᵃᶜ(ℑxᶠᵃᵃ)
ixz_cf = lambda f: iz_f(ix_c(f))  # ℑxzᶜᵃᶠ = ℑzᵃᵃᶠ(ℑxᶜᵃᵃ)
iyz_fc = lambda f: iz_c(iy_f(f))  # ℑyzᵃᶠᶜ = ℑzᵃᵃᶜ(ℑyᵃᶠᵃ)
iyz_cf = lambda f: iz_f(iy_c(f))  # ℑyzᵃᶜᶠ = ℑzᵃᵃᶠ(ℑyᵃᶜᵃ)


def derivatives(g, f):
    """(∂xᶠᶜᶜ, ∂yᶜᶠᶜ, ∂zᶜᶜᶠ) of a centre field; None (a constant): zeros"""
    if f is None:
        zero = lambda a, b, c: np.zeros((g.Nx, g.Ny, g.Nz))
        return zero, zero, zero
    v = lambda a, b, c: _sh(g, f, a, b, c)
    return (lambda a, b, c: (v(a, b, c) - v(a - 1, b, c)) / g.dx, lambda a, b, c: (v(a, b, c) - v(a, b - 1, c)) / g.dy,
            lambda a, b, c: (v(a, b, c) - v(a, b, c - 1)) / _dzF(g, c))


def buoyancy_gradients(g, buoyancy, T, S):
    """(∂x_b, ∂y_b, ∂z_b) at (f, c, c), (c, f, c), (c, c, f)"""
    dT = derivatives(g, T)
    if buoyancy is None:
        return derivatives(g, None)
    if buoyancy[0] == "BuoyancyTracer":
        return dT
    _, grav, alpha, beta = buoyancy
    dS = derivatives(g, S)
    combine = lambda q: lambda a, b, c: grav * (alpha * dT[q](a, b, c) - beta * dS[q](a, b, c))
    return combine(0), combine(1), combine(2)


# ---- slopes -------------------------------------------------------------------------------------------------------------------------------------
def calc_tapering(cl, bx, by, bz):
    with np.errstate(divide="ignore", invalid="ignore"):
        bz = jl_max(bz, cl.minimum_bz)
        slope_x, slope_y = -bx / bz, -by / bz
        slope2 = np.where(bz <= 0, 0.0, slope_x * slope_x + slope_y * slope_y)
        return min_one(cl.max_slope * cl.max_slope / slope2)


def rotation(cl, bh, bz):
    """isopycnal_rotation_tensor_xz / yz: bh is ∂x b or ∂y b at the component's location"""
    with np.errstate(divide="ignore", invalid="ignore"):
        bz = jl_max(bz, cl.minimum_bz)
        slope = -bh / bz
        return np.where(bz == 0, 0.0, slope)


def rotation_zz(cl, bx, by, bz):
    with np.errstate(divide="ignore", invalid="ignore"):
        bz = jl_max(bz, cl.minimum_bz)
        slope_x, slope_y = -bx / bz, -by / bz
        slope2 = slope_x * slope_x + slope_y * slope_y
        return np.where(bz == 0, 0.0, slope2)


def face_gradients(g, buoyancy, T, S):
    """the buoyancy gradient (bx, by, bz) at the three face kinds, each a function of a shift: what every flux, ϵ and R is made of"""
    bx, by, bz = buoyancy_gradients(g, buoyancy, T, S)
    return dict(fcc=(bx, ixy_fc(by), ixz_fc(bz)),    # tapering_factorᶠᶜᶜ (:174-181)
                cfc=(ixy_cf(bx), by, iyz_fc(bz)),    # tapering_factorᶜᶠᶜ (:183-190)
                ccf=(ixz_cf(bx), iyz_cf(by), bz))    # tapering_factorᶜᶜᶠ (:192-199)


def tapered_R33(g, buoyancy, T, S, cl):
    """ϵ_R₃₃ over i = 1..Nx, j = 1..Ny, faces k = 1..Nz"""
    bx, by, bz = (f(0, 0, 0) for f in face_gradients(g, buoyancy, T, S)["ccf"])
    return calc_tapering(cl, bx, by, bz) * rotation_zz(cl, bx, by, bz)


def tapered_slopes(g, buoyancy, T, S, cl):
    """(Sxᶠᶜᶠ, Syᶜᶠᶠ) as functions of a shift"""
    bx, by, bz = buoyancy_gradients(g, buoyancy, T, S)

    def slope(bh, bz_):
        def at(a, b, c):
            with np.errstate(divide="ignore", invalid="ignore"):
                h, z = bh(a, b, c), bz_(a, b, c)
                S_ = np.where(z == 0, 0.0, -h / z)
                eps = min_one(cl.max_slope * cl.max_slope / (S_ * S_))
                S_ = np.where(_boundary(g, c), 0.0, S_)  # peripheral_node: faces 1 and Nz + 1
                return eps * S_
        return at
    return slope(iz_f(bx), ix_f(bz)), slope(iz_f(by), iy_f(bz))


def eddy_velocity_functions(g, buoyancy, T, S, cl, kappa_skew):
    """(uₑ, vₑ, wₑ) of _compute_eddy_velocities! as functions of a shift"""
    Sx, Sy = tapered_slopes(g, buoyancy, T, S, cl)
    kSx = lambda a, b, c: kappa_skew * Sx(a, b, c)
    kSy = lambda a, b, c: kappa_skew * Sy(a, b, c)
    ue = lambda a, b, c: -((kSx(a, b, c + 1) - kSx(a, b, c)) / _dzC(g, c))
    ve = lambda a, b, c: -((kSy(a, b, c + 1) - kSy(a, b, c)) / _dzC(g, c))
    we = lambda a, b, c: (kSx(a + 1, b, c) - kSx(a, b, c)) / g.dx + (kSy(a, b + 1, c) - kSy(a, b, c)) / g.dy
    return ue, ve, we


def eddy_velocities(g, buoyancy, T, S, cl, kappa_skew):
    """(uₑ, vₑ over cells k = 1..Nz, wₑ over faces k = 1..Nz) as _compute_eddy_velocities! computes them (before any fill)"""
    return tuple(f(0, 0, 0) for f in eddy_velocity_functions(g, buoyancy, T, S, cl, kappa_skew))


# ---- fluxes -------------------------------------------------------------------------------------------------------------------------------------
def fluxes(g, buoyancy, T, S, cl, ks, kw, c):
    """(diffusive_flux_x at fcc, _y at cfc, _z at ccf) of tracer c as functions of a shift; ks, kw: κ_symmetric and the κ_skew inside the
    fluxes (0 with the AdvectiveFormulation)"""
    G = face_gradients(g, buoyancy, T, S)
    cx, cy, cz = derivatives(g, c)

    def fx(a, b, k):
        bx, by, bz = (f(a, b, k) for f in G["fcc"])
        eps, R13 = calc_tapering(cl, bx, by, bz), rotation(cl, bx, bz)
        return -eps * (((ks * 1.0) * cx(a, b, k) + (ks * 0.0) * ixy_fc(cy)(a, b, k)) + ((ks - kw) * R13) * ixz_fc(cz)(a, b, k))

    def fy(a, b, k):
        bx, by, bz = (f(a, b, k) for f in G["cfc"])
        eps, R23 = calc_tapering(cl, bx, by, bz), rotation(cl, by, bz)
        return -eps * (((ks * 0.0) * ixy_cf(cx)(a, b, k) + (ks * 1.0) * cy(a, b, k)) + ((ks - kw) * R23) * iyz_fc(cz)(a, b, k))

    def fz(a, b, k):
        bx, by, bz = (f(a, b, k) for f in G["ccf"])
        eps, R31, R32 = calc_tapering(cl, bx, by, bz), rotation(cl, bx, bz), rotation(cl, by, bz)
        # (explicit_κ_∂z_c is zero with the vertically implicit discretization, :325)
        return (-eps) * 0.0 - eps * (((ks + kw) * R31) * ixz_cf(cx)(a, b, k) + ((ks + kw) * R32) * iyz_cf(cy)(a, b, k))
    return fx, fy, fz


def divergence(g, fx, fy, fz):
    """1 / V * (δxᶜ(Ax qx) + δyᶜ(Ay qy) + δzᶜ(Az qz)) over the interior"""
    dz = _dzC(g, 0)
    Az = g.dx * g.dy
    Ax, Ay, V = g.dy * dz, g.dx * dz, Az * dz
    return 1 / V * (((Ax * fx(1, 0, 0) - Ax * fx(0, 0, 0)) + (Ay * fy(0, 1, 0) - Ay * fy(0, 0, 0))) + (Az * fz(0, 0, 1) - Az * fz(0, 0, 0)))


def tracer_term(g, buoyancy, T, S, cl, ks, kw, c):
    """∇_dot_qᶜ over the interior"""
    return divergence(g, *fluxes(g, buoyancy, T, S, cl, ks, kw, c))


# ---- parent arrays ------------------------------------------------------------------------------------------------------------------------------
def interior(g, zface=False):
    """cells (or, zface, faces) k = 1..Nz"""
    return (slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny), slice(g.Hz, g.Hz + g.Nz))


def parent_shape(g, zface=False):
    return (g.Nx + 2 * g.Hx, g.Ny + 2 * g.Hy, g.Nz + 2 * g.Hz + (1 if zface else 0))


def subtract(g, G, a, b=None):
    """a copy of the parent G with G - a, or G - (a + b), over the interior"""
    out = np.array(G, dtype=np.float64)
    sl = interior(g)
    out[sl] = out[sl] - (a if b is None else (a + b))
    return out


def fill_halos(g, parent, zface):
    """the halo fill of a diffusivity field with its default conditions: Periodic copies in x and y over every plane; in z the no-flux mirror
    of the first halo plane for a Center-in-z field (uₑ, vₑ), nothing for a Face-in-z field (ϵ_R₃₃ has no condition there; wₑ's Impenetrable
    condition sets faces 1 and Nz + 1 to 0, which `diffusivity_parents` writes)"""
    p = np.array(parent, dtype=np.float64)
    Hx, Hy, Hz, Nx, Ny, Nz = g.Hx, g.Hy, g.Hz, g.Nx, g.Ny, g.Nz
    if not zface:
        p[Hx:Hx + Nx, Hy:Hy + Ny, Hz - 1] = p[Hx:Hx + Nx, Hy:Hy + Ny, Hz]
        p[Hx:Hx + Nx, Hy:Hy + Ny, Hz + Nz] = p[Hx:Hx + Nx, Hy:Hy + Ny, Hz + Nz - 1]
    for h in range(Hx):
        p[h] = p[Hx + (h - Hx) % Nx]
        p[Hx + Nx + h] = p[Hx + h % Nx]
    for h in range(Hy):
        p[:, h] = p[:, Hy + (h - Hy) % Ny]
        p[:, Hy + Ny + h] = p[:, Hy + h % Ny]
    return p


def diffusivity_parents(g, buoyancy, T, S, cl, kappa_skew, before):
    """what update_state! leaves in the diffusivity fields: `before` = dict(eps_R33=, u=, v=, w=) of parents as they were (u, v, w only with
    eddy velocities: kappa_skew is not None); returns the same dict after compute_diffusivities! and the halo fill"""
    out = {}
    e = np.array(before["eps_R33"], dtype=np.float64)
    e[interior(g)] = tapered_R33(g, buoyancy, T, S, cl)
    out["eps_R33"] = fill_halos(g, e, True)
    if kappa_skew is not None:
        ue, ve, we = eddy_velocities(g, buoyancy, T, S, cl, kappa_skew)
        u, v, w = (np.array(before[n], dtype=np.float64) for n in "uvw")
        u[interior(g)], v[interior(g)], w[interior(g)] = ue, ve, we
        w[g.Hx:g.Hx + g.Nx, g.Hy:g.Hy + g.Ny, g.Hz] = 0.0         # the open fill: Impenetrable bottom and top
        w[g.Hx:g.Hx + g.Nx, g.Hy:g.Hy + g.Ny, g.Hz + g.Nz] = 0.0
        out.update(u=fill_halos(g, u, False), v=fill_halos(g, v, False), w=fill_halos(g, w, True))
    return out


def kz(g, eps_R33_parent, kappa_symmetric, before):
    """κzᶜᶜᶠ = ϵ_R₃₃ κ_symmetric over faces k = 1..Nz of the parent `before`"""
    out = np.array(before, dtype=np.float64)
    out[interior(g)] = eps_R33_parent[interior(g)] * kappa_symmetric
    return out


def implicit_step(g, parent, kz_parent, dt):
    """implicit_step! of a centre field with a κz field at (c, c, f): the rows of vertically_implicit_diffusion_solver.jl:55-78 and the
    elimination of solve_batched_tridiagonal_system_z!, column by column, in the arithmetic of implicit_diffusion_numpy"""
    out = np.array(parent, dtype=np.float64)
    dzc = lambda k: float(g.dzc[k + g.Hz - 1])
    dzf = lambda k: float(g.dzf[k + g.Hz - 1])
    Nz = g.Nz
    for i in range(g.Nx):
        for j in range(g.Ny):
            kap = lambda k: float(kz_parent[g.Hx + i, g.Hy + j, g.Hz + k - 1])
            upper = lambda k: 0.0 if k > Nz - 1 else -dt * kap(k + 1) / (dzc(k) * dzf(k + 1))
            lower = lambda k: 0.0 if k < 1 else -dt * kap(k + 1) / (dzc(k + 1) * dzf(k + 1))
            a, b, c = np.zeros(Nz), np.zeros(Nz), np.zeros(Nz)
            for k in range(1, Nz + 1):
                up = upper(k)
                a[k - 1] = lower(k) if k < Nz else 0.0
                b[k - 1] = (1.0 - up) - lower(k - 1)
                c[k - 1] = up
            col = (g.Hx + i, g.Hy + j, slice(g.Hz, g.Hz + Nz))
            out[col] = IDN.thomas(a, b, c, out[col])
    return out


# ---- the shared test input ----------------------------------------------------------------------------------------------------------------------
def shared_input(g, seed, N2=1.0e-5, slope=0.4e-2, horizontal_noise=3.0, vertical_noise=0.2):
    """b = N² z + M² ramp(x, y) + noise on the whole parent (x and y halos periodic images, z halos the same formula continued), with a block
    of columns of constant b (∂x b = ∂y b = ∂z b = 0 exactly: the 0 / 0 case), a block with inverted stratification (∂z b < 0) and M² / N²
    about max_slope = 1e-2, so that the noise puts about half of the remaining faces on either side of the tapering threshold.
    Returns the parent of b and the parent of a passive tracer."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = parent_shape(g)
    i = (np.arange(nx) - g.Hx) % g.Nx  # the interior column of every parent column: x and y halos are periodic images
    j = (np.arange(ny) - g.Hy) % g.Ny
    zc = np.cumsum(np.asarray(g.dzf[:nz], dtype=np.float64))  # z of the centres, halos included (the origin does not matter)
    M2 = slope * N2
    ramp = np.abs(2.0 * (i + 0.5) / g.Nx - 1.0)[:, None] * g.Nx * g.dx + 0.5 * np.abs(2.0 * (j + 0.5) / g.Ny - 1.0)[None, :] * g.Ny * g.dy
    wiggle = (horizontal_noise * M2 * min(g.dx, g.dy) * rng.uniform(-1, 1, (g.Nx, g.Ny, 1))
              + vertical_noise * N2 * np.min(g.dzf) * rng.uniform(-1, 1, (g.Nx, g.Ny, nz)))[i][:, j]
    b = N2 * zc[None, None, :] + M2 * ramp[:, :, None] + wiggle
    c = rng.uniform(-1, 1, (g.Nx, g.Ny, nz))[i][:, j]
    # the blocks: at least two columns wide where a face must have both of its columns inside
    constant = np.outer(i < max(2, g.Nx // 3), j < max(2, g.Ny // 2))
    zmid = zc[g.Hz + g.Nz // 2]
    b[constant] = N2 * zmid
    inverted = np.outer(i >= g.Nx - max(1, g.Nx // 3), j >= g.Ny - max(1, g.Ny // 2))
    b[inverted] = (N2 * zmid - 3.0 * N2 * (zc - zmid))[None, :] + wiggle[inverted]
    return b, c


def branch_fractions(g, buoyancy, T, S, cl):
    """per face kind, the fraction of the faces that a flux kernel evaluates -- x faces i = 1..Nx + 1, y faces j = 1..Ny + 1, z faces
    k = 1..Nz + 1 -- in each branch: untapered (bz > 0, ϵ == 1), tapered (ϵ < 1), bz < 0, bz == 0"""
    G = face_gradients(g, buoyancy, T, S)
    out = {}
    for kind, shifts in (("fcc", ((0, 0, 0), (1, 0, 0))), ("cfc", ((0, 0, 0), (0, 1, 0))), ("ccf", ((0, 0, 0), (0, 0, 1)))):
        sel = {"fcc": (slice(-1, None), slice(None), slice(None)), "cfc": (slice(None), slice(-1, None), slice(None)),
               "ccf": (slice(None), slice(None), slice(-1, None))}[kind]
        parts = []
        for n, sft in enumerate(shifts):
            bx, by, bz = (f(*sft) for f in G[kind])
            eps = calc_tapering(cl, bx, by, bz)
            q = np.stack([(bz > 0) & (eps == 1), eps < 1, bz < 0, bz == 0])
            parts.append(q if n == 0 else q[(slice(None),) + sel])  # (the shifted evaluation adds the last face only)
        counts = sum(p.reshape(4, -1).sum(axis=1) for p in parts)
        total = sum(p[0].size for p in parts)
        out[kind] = dict(zip(("untapered", "tapered", "bz_negative", "bz_zero"), counts / total))
    return out


# the grids of the GPU tests (tests/test_gpu_isopycnal.py) and the seed of their shared input, chosen on the CPU so that every branch holds
# at least 5 % of the faces of every kind (asserted in tests/test_host_isopycnal.py): size, stretched z, halo
SEAWATER = ("SeawaterBuoyancy", 9.80665, 1.67e-4, 7.80e-4)
SEED = 5
CASES = {"reference_333": ((3, 3, 3), False, (3, 3, 3)),
         "minimal_halo": ((3, 3, 3), False, (1, 1, 1)),
         "one_interior_face": ((5, 4, 2), False, (3, 3, 2)),  # (a halo may not exceed the size: Hz = 2 is the widest that Nz = 2 takes)
         "tile_plus_partial": ((37, 11, 4), True, (3, 3, 3))}


def case_grid_arguments(name):
    """keyword arguments of RectilinearGrid for a case: Δx = Δy = 10 km over Δz of about 10 m, the aspect ratio of a coarse ocean model"""
    size, stretched, halo = CASES[name]
    s = np.linspace(0.0, 1.0, size[2] + 1)
    z = -40.0 * (1 - s) ** 1.6 if stretched else (-10.0 * size[2], 0.0)
    return dict(size=size, x=(0, 1e4 * size[0]), y=(0, 1e4 * size[1]), z=z, topology=("Periodic", "Periodic", "Bounded"), halo=halo)


def case_inputs(g, buoyancy):
    """(T, S, c): the shared input as b itself (S = None), or as a T with g α T = b and an S that is constant where b is"""
    b, c = shared_input(g, SEED)
    if buoyancy[0] == "BuoyancyTracer":
        return b, None, c
    _, grav, alpha, beta = buoyancy
    rng = np.random.default_rng(SEED + 1)
    nx, ny, nz = parent_shape(g)
    i, j = (np.arange(nx) - g.Hx) % g.Nx, (np.arange(ny) - g.Hy) % g.Ny
    S = 35.0 + (1.0e-4 * rng.uniform(-1, 1, (g.Nx, g.Ny, nz)))[i][:, j]
    S[np.outer(i < max(2, g.Nx // 3), j < max(2, g.Ny // 2))] = 35.0
    return b / (grav * alpha), S, c
