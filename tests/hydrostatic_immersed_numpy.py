"""TEST INFRASTRUCTURE (CPU restatement, never imported by the product): the reference's HydrostaticFreeSurfaceModel on
ImmersedBoundaryGrid(grid, GridFittedBottom(h)) over a (Periodic, Periodic, Bounded) grid, on top of oracle/hydrostatic.py (whose periodic model
is subclassed: fields, halo fills, w from continuity, the hydrostatic pressure, the AB2 steps and the order of time_step! are inherited).
Restated here from the rules, in the reference's evaluation order, with every predicate evaluated cell by cell:

  * the materialized bottom height, immersed_cell            ImmersedBoundaries/grid_fitted_bottom.jl:99-130, static_column_depth :147-150
  * inactive_node / peripheral_node and their immersed_ forms Grids/inactive_node.jl:127-155, immersed_boundary_interface.jl:49-60
  * the conditional differences (all 24 follow one rule)      ImmersedBoundaries/conditional_differences.jl:25-92
  * the conditional fluxes                                    Advection/immersed_advective_fluxes.jl:20-59,
                                                              TurbulenceClosures/immersed_diffusive_fluxes.jl:27-44
  * masking                                                   ImmersedBoundaries/mask_immersed_field.jl:53-105,
                                                              update_hydrostatic_free_surface_model_state.jl:32-72
  * the split-explicit surface                                compute_slow_tendencies.jl:17-42, step_split_explicit_free_surface.jl:11-48,
                                                              124-171, barotropic_split_explicit_corrector.jl:13-81

Unlike the product, nothing here is reused on an argument: the Coriolis term, the pressure gradient, the viscous and diffusive terms and the
tracer advection are all written out with the conditional operators, so a reuse in the product that changes a surviving value fails the
comparison.  Scope: VectorInvariant() momentum, Centered(order = 2) tracers, FPlane, closure None or (ν, κ), Explicit / SplitExplicit free
surface.  Every array below is indexed like a centre field's parent: [I, J, K] is the node (I - Hx + 1, J - Hy + 1, K - Hz + 1) of its
location; shifted reads wrap at the array's ends, which only the outermost halo points see (halos are >= 2 wide).
"""
import numpy as np

from oracle import hydrostatic as Hy
from oracle import oracle as O

CCC, FCC, CFC, FFC, CCF, FCF, CFF, FFF = range(8)  # bit 0 / 1 / 2: Face in x / y / z


def materialize(g, h, interface=False):
    """(bottom height, kbot) of an (Nx, Ny) array h: the height starts at face 1 and is raised to face k + 1 whenever z_centre(k) <= h
    (CenterImmersedCondition) or z_face(k + 1) <= h (InterfaceImmersedCondition); a cell is immersed iff z_centre(k) <= bottom height"""
    zf = np.asarray(g.nodes(2, True))[:g.Nz + 1]
    zc = np.asarray(g.nodes(2, False))[:g.Nz]
    bottom = np.full((g.Nx, g.Ny), zf[0])
    for i in range(g.Nx):
        for j in range(g.Ny):
            for k in range(1, g.Nz + 1):
                if (zf[k] <= h[i, j]) if interface else (zc[k - 1] <= h[i, j]):
                    bottom[i, j] = zf[k]
    immersed = zc[None, None, :] <= bottom[:, :, None]
    return bottom, immersed


def sh(a, di=0, dj=0, dk=0):
    """a at (i + di, j + dj, k + dk)"""
    return np.roll(a, (-di, -dj, -dk), axis=(0, 1, 2))


class Bathymetry:
    def __init__(self, g, h, interface=False):
        self.g = g
        self.bottom, self.immersed = materialize(g, np.asarray(h, dtype=np.float64), interface)
        Hx, Hy, Hz, Nz = g.Hx, g.Hy, g.Hz, g.Nz
        k = np.arange(1 - Hz, Nz + Hz + 1)
        outside = (k < 1) | (k > Nz)
        shape = (g.Nx + 2 * Hx, g.Ny + 2 * Hy, Nz + 2 * Hz)
        imm = np.zeros(shape, dtype=bool)
        imm[Hx:Hx + g.Nx, Hy:Hy + g.Ny, Hz:Hz + Nz] = self.immersed
        imm = np.pad(imm[Hx:Hx + g.Nx, Hy:Hy + g.Ny, :], ((Hx, Hx), (Hy, Hy), (0, 0)), mode="wrap")
        self.cell = imm | outside[None, None, :]                      # inactive_cell(i, j, k, ibg)
        self.cell0 = np.broadcast_to(outside[None, None, :], shape)    # inactive_cell(i, j, k, underlying grid)
        zf = np.asarray(g.nodes(2, True))[:Nz + 1]
        Hcc = zf[Nz] - self.bottom
        self.Hcc, self.Hfc, self.Hcf = Hcc, np.minimum(np.roll(Hcc, 1, 0), Hcc), np.minimum(np.roll(Hcc, 1, 1), Hcc)

    @staticmethod
    def _node(cell, loc, op):
        a = cell
        for d in range(3):
            if loc >> d & 1:
                a = op(a, np.roll(a, 1, axis=d))
        return a

    def inactive_node(self, loc):
        return self._node(self.cell, loc, np.logical_and)

    def peripheral_node(self, loc):
        return self._node(self.cell, loc, np.logical_or)

    def immersed_inactive_node(self, loc):
        return self.inactive_node(loc) & ~self._node(self.cell0, loc, np.logical_and)

    def immersed_peripheral_node(self, loc):
        return self.peripheral_node(loc) & ~self._node(self.cell0, loc, np.logical_or)

    # ---- conditional differences: delta(q, d, loc): the difference along d of q that ENDS UP at `loc`; 0 where one of the two differenced
    # nodes (at `loc` with the location along d flipped) is an immersed_inactive_node
    def delta(self, q, d, loc):
        src = loc ^ (1 << d)
        ina = self.immersed_inactive_node(src)
        s = [0, 0, 0]
        if loc >> d & 1:   # Center -> Face: q(i) - q(i - 1)
            s[d] = -1
            return np.where(ina | sh(ina, *s), 0.0, q - sh(q, *s))
        s[d] = 1           # Face -> Center: q(i + 1) - q(i)
        return np.where(ina | sh(ina, *s), 0.0, sh(q, *s) - q)

    def flux(self, q, loc):
        """conditional_flux: 0 on an immersed_peripheral_node of the flux's own location"""
        return np.where(self.immersed_peripheral_node(loc), 0.0, q)

    def interior(self, a):
        g = self.g
        return a[g.Hx:g.Hx + g.Nx, g.Hy:g.Hy + g.Ny, g.Hz:g.Hz + g.Nz]


def _spacings(g):
    """(Δzᶜ, Δzᶠ) as [1, 1, K] arrays over the parent levels"""
    n = g.Nz + 2 * g.Hz
    dzc = np.full(n, g.dz) if g.dzc is None else np.asarray(g.dzc[:n])
    dzf = np.full(n, g.dz) if g.dzf is None else np.asarray(g.dzf[:n])
    return dzc[None, None, :], dzf[None, None, :]


def vector_invariant_tendencies(B, u, v, w, Gu, Gv, eta=None, grav=0.0):
    g = B.g
    dx, dy = g.dx, g.dy
    Az = dx * dy
    _, dzf = _spacings(g)
    w = w[:, :, :u.shape[2]]
    zeta = (B.delta(dy * v, 0, FFC) - B.delta(dx * u, 1, FFC)) / Az
    Kh = (0.5 * (u * u + sh(u, 1) * sh(u, 1)) + 0.5 * (v * v + sh(v, 0, 1) * sh(v, 0, 1))) / 2
    # ---- u
    m = 0.5 * (dx * v + dx * sh(v, 0, 1))
    hadv = -(0.5 * (zeta + sh(zeta, 0, 1))) * (0.5 * (sh(m, -1) + m)) / dx
    Z = (0.5 * (Az * sh(w, -1) + Az * w)) * (B.delta(u, 2, FCF) / dzf)
    vadv = (0.5 * (Z + sh(Z, 0, 0, 1))) / Az
    bern = B.delta(Kh, 0, FCC) / dx
    G = -((hadv + vadv) + bern)
    if eta is not None:
        G = G - (grav * ((eta - np.roll(eta, 1, 0)) / dx))[:, :, None]
    g.interior_N(Gu)[...] = B.interior(G)
    # ---- v
    n = 0.5 * (dy * u + dy * sh(u, 1))
    hadv = (0.5 * (zeta + sh(zeta, 1))) * (0.5 * (sh(n, 0, -1) + n)) / dy
    Z = (0.5 * (Az * sh(w, 0, -1) + Az * w)) * (B.delta(v, 2, CFF) / dzf)
    vadv = (0.5 * (Z + sh(Z, 0, 0, 1))) / Az
    bern = B.delta(Kh, 1, CFC) / dy
    G = -((hadv + vadv) + bern)
    if eta is not None:
        G = G - (grav * ((eta - np.roll(eta, 1, 1)) / dy))[:, :, None]
    g.interior_N(Gv)[...] = B.interior(G)


def coriolis_and_pressure(B, f, u, v, pHY, Gu, Gv):
    """Gu -= x_f_cross_U, Gv -= y_f_cross_U (interpolations: not conditional), then Gu -= ∂xᶠᶜᶜ pHY′, Gv -= ∂yᶜᶠᶜ pHY′ (conditional)"""
    g = B.g
    Gui, Gvi = g.interior_N(Gu), g.interior_N(Gv)
    if f is not None:
        vi = 0.5 * (0.5 * (sh(v, -1) + v) + 0.5 * (sh(v, -1, 1) + sh(v, 0, 1)))
        ui = 0.5 * (0.5 * (sh(u, 0, -1) + sh(u, 1, -1)) + 0.5 * (u + sh(u, 1)))
        Gui[...] = Gui - B.interior(-f * vi)
        Gvi[...] = Gvi - B.interior(f * ui)
    if pHY is not None:
        Gui[...] = Gui - B.interior(B.delta(pHY, 0, FCC) / g.dx)
        Gvi[...] = Gvi - B.interior(B.delta(pHY, 1, CFC) / g.dy)


def viscous_terms(B, nu, u, v, w, Gu, Gv):
    """Gu -= ∂ⱼτ₁ⱼ, Gv -= ∂ⱼτ₂ⱼ with τ = -2 ν Σ, every stress through conditional_flux at its location and every difference conditional"""
    g = B.g
    dx, dy = g.dx, g.dy
    Az = dx * dy
    dzc, dzf = _spacings(g)
    Ax, Ay = dy * dzc, dx * dzc
    w = w[:, :, :u.shape[2]]
    tau = lambda s: -2 * (nu * s)
    t11 = B.flux(tau(B.delta(u, 0, CCC) / dx), CCC)
    t22 = B.flux(tau(B.delta(v, 1, CCC) / dy), CCC)
    t12 = B.flux(tau(0.5 * (B.delta(u, 1, FFC) / dy + B.delta(v, 0, FFC) / dx)), FFC)
    t13 = B.flux(tau(0.5 * (B.delta(u, 2, FCF) / dzf + B.delta(w, 0, FCF) / dx)), FCF)
    t23 = B.flux(tau(0.5 * (B.delta(v, 2, CFF) / dzf + B.delta(w, 1, CFF) / dy)), CFF)
    du = 1 / (Az * dzc) * (((Ax * t11 - Ax * sh(t11, -1)) + (Ay * sh(t12, 0, 1) - Ay * t12)) + (Az * sh(t13, 0, 0, 1) - Az * t13))
    dv = 1 / (Az * dzc) * (((Ax * sh(t12, 1) - Ax * t12) + (Ay * t22 - Ay * sh(t22, 0, -1))) + (Az * sh(t23, 0, 0, 1) - Az * t23))
    Gui, Gvi = g.interior_N(Gu), g.interior_N(Gv)
    Gui[...] = Gui - B.interior(du)
    Gvi[...] = Gvi - B.interior(dv)


def tracer_tendency(B, u, v, w, c, Gc, kappa=None):
    """Gc = - div_Uc (Centered(order = 2): buffer 1, the reconstruction is never replaced) - ∇_dot_qᶜ, every flux conditional"""
    g = B.g
    dx, dy = g.dx, g.dy
    Az = dx * dy
    dzc, dzf = _spacings(g)
    Ax, Ay = dy * dzc, dx * dzc
    w = w[:, :, :c.shape[2]]
    avg = lambda x, y: 0.5 * x + 0.5 * y
    Fx = B.flux((Ax * u) * avg(sh(c, -1), c), FCC)
    Fy = B.flux((Ay * v) * avg(sh(c, 0, -1), c), CFC)
    Fz = B.flux((Az * w) * avg(sh(c, 0, 0, -1), c), CCF)
    rV = 1 / (Az * dzc)
    G = -(rV * (((sh(Fx, 1) - Fx) + (sh(Fy, 0, 1) - Fy)) + (sh(Fz, 0, 0, 1) - Fz)))
    if kappa is not None:
        qx = B.flux(-(kappa * (B.delta(c, 0, FCC) / dx)), FCC)
        qy = B.flux(-(kappa * (B.delta(c, 1, CFC) / dy)), CFC)
        qz = B.flux(-(kappa * (B.delta(c, 2, CCF) / dzf)), CCF)
        G = G - 1 / (Az * dzc) * (((Ax * sh(qx, 1) - Ax * qx) + (Ay * sh(qy, 0, 1) - Ay * qy)) + (Az * sh(qz, 0, 0, 1) - Az * qz))
    g.interior_N(Gc)[...] = B.interior(G)


def mask_field(B, a, loc, value=0.0):
    """mask_immersed_field!: value on the immersed_peripheral_node of the field's location, over 1:Nx, 1:Ny, 1:Nz"""
    g = B.g
    m = B.interior(B.immersed_peripheral_node(loc))
    ai = g.interior_N(a)
    ai[m] = value


def split_explicit_forcing(B, Gn, Gm, chi, loc):
    """Σₖ Δz ifelse(peripheral_node, 0, (3/2 + χ) Gⁿ - (1/2 + χ) G⁻ not_euler) (compute_slow_tendencies.jl:17-42)"""
    g = B.g
    dzc, _ = _spacings(g)
    dz = dzc[0, 0, g.Hz:g.Hz + g.Nz]
    gn, gm, per = g.interior_N(Gn), g.interior_N(Gm), B.interior(B.peripheral_node(loc))
    C1, C2 = 3 * 1.0 / 2 + chi, 1.0 / 2 + chi
    ne = 1.0 if C2 != 0 else 0.0
    term = lambda k: dz[k] * np.where(per[:, :, k], 0.0, C1 * gn[:, :, k] - C2 * gm[:, :, k] * ne)
    acc = term(0)
    for k in range(1, g.Nz):
        acc = acc + term(k)
    return acc


def iterate_split_explicit(B, eta, U, V, etab, Ub, Vb, GU, GV, dtau, weights, grav):
    """iterate_split_explicit! with the ForwardBackwardScheme on interior (Nx, Ny) arrays: transports through conditional_U_fcc / V_cfc (0 on
    a peripheral node at k = Nz), ∂xTᶠᶜᶠ η / ∂yTᶜᶠᶠ η 0 when one of the two (c, c, f) nodes at k = Nz + 1 is inactive, depths Hᶠᶜ / Hᶜᶠ"""
    g = B.g
    dx, dy = g.dx, g.dy
    Az = dx * dy
    ii, jj, kt = slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny), g.Hz + g.Nz - 1
    pu, pv = B.peripheral_node(FCC)[ii, jj, kt], B.peripheral_node(CFC)[ii, jj, kt]
    dry = B.inactive_node(CCF)[ii, jj, kt + 1]
    for wgt in weights:
        Fu, Fv = np.where(pu, 0.0, dy * U), np.where(pv, 0.0, dx * V)
        eta[...] = eta - dtau * ((np.roll(Fu, -1, 0) - Fu) + (np.roll(Fv, -1, 1) - Fv)) / Az
        dex = np.where(dry | np.roll(dry, 1, 0), 0.0, (eta - np.roll(eta, 1, 0)) / dx)
        dey = np.where(dry | np.roll(dry, 1, 1), 0.0, (eta - np.roll(eta, 1, 1)) / dy)
        Un = U + dtau * (-grav * B.Hfc * dex + GU)
        Vn = V + dtau * (-grav * B.Hcf * dey + GV)
        etab += wgt * eta
        Ub += wgt * Un
        Vb += wgt * Vn
        U[...] = Un
        V[...] = Vn


def barotropic_corrector(B, u, v, U, V):
    """barotropic_split_explicit_corrector! (:51-81) on interior planes U, V: U̅ = Σₖ Δz u σ with σ = 1 (a static grid, also where h = 0), then
    u += (U - U̅) / Hᶠᶜ at every level.  A dry face gets 0 / 0, which the next mask removes.  Returns U̅, V̅; u, v corrected in place."""
    g = B.g
    dzc, _ = _spacings(g)
    dz = dzc[0, 0, g.Hz:g.Hz + g.Nz]
    ui, vi = g.interior_N(u), g.interior_N(v)
    Ub, Vb = dz[0] * ui[:, :, 0] * 1.0, dz[0] * vi[:, :, 0] * 1.0
    for k in range(1, g.Nz):
        Ub, Vb = Ub + dz[k] * ui[:, :, k] * 1.0, Vb + dz[k] * vi[:, :, k] * 1.0
    with np.errstate(invalid="ignore", divide="ignore"):
        ui[...] = ui + ((U - Ub) / B.Hfc)[:, :, None]
        vi[...] = vi + ((V - Vb) / B.Hcf)[:, :, None]
    return Ub, Vb


def conservation_bound(steps, cells, scale):
    """The change of Σ c V over the active cells in `steps` steps of pure diffusion with no flux through the bottom.  Every flux leaves one
    active cell and enters another (the conditional fluxes are 0 on every face next to an immersed cell and at the top and bottom), so in
    exact arithmetic the sum telescopes to 0.  In floating point each cell's update c += Δt G rounds a handful of times (six flux
    differences, their sum, the division by the volume, the AB2 combination, the update: fewer than 16 roundings, each at most one ulp of a
    quantity bounded by max |c V|), and the check's own summation adds one rounding per cell: steps x cells x 16 ulps of max |c V|, plus
    cells ulps for each of the two sums."""
    eps = np.finfo(np.float64).eps
    return (steps * cells * 16 + 2 * cells) * eps * scale


class HydrostaticFreeSurfaceModel(Hy.HydrostaticFreeSurfaceModel):
    """oracle/hydrostatic.py's model on ImmersedBoundaryGrid(grid, GridFittedBottom(h[, InterfaceImmersedCondition()]))"""

    def __init__(self, grid, h, interface=False, **kw):
        assert kw.get("momentum_advection", "VectorInvariant") == "VectorInvariant" and kw.get("tracer_advection") in (None, "Centered2")
        assert kw.get("coriolis_beta") is None and not kw.get("implicit_free_surface") and kw.get("timestepper", "QuasiAdamsBashforth2") == "QuasiAdamsBashforth2"
        assert min(grid.Hx, grid.Hy, grid.Hz) >= 2
        kw["momentum_advection"] = "VectorInvariant"
        self.B = Bathymetry(grid, h, interface)
        super().__init__(grid, **kw)

    def mask_immersed_model_fields(self):
        B, g = self.B, self.grid
        for f, l, n in zip(self.fields, self.locs, self.names):
            if n != "w":
                mask_field(B, f, {O.LOC_U: FCC, O.LOC_V: CFC, O.LOC_C: CCC}[l])
        # η in the plane k = Nz + 1: immersed_peripheral_node(c, c, f) there (the plane is on the underlying grid's own periphery)
        ii, jj = slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny)
        self.eta[ii, jj][B.immersed_peripheral_node(CCF)[ii, jj, g.Hz + g.Nz]] = 0.0
        if self.split is not None:  # U (Face, Center, Nothing), V (Center, Face, Nothing): mask_immersed_field_xy! at k = Nz
            kt = g.Hz + g.Nz - 1
            self.U[B.immersed_peripheral_node(FCC)[ii, jj, kt]] = 0.0
            self.V[B.immersed_peripheral_node(CFC)[ii, jj, kt]] = 0.0

    def update_state(self, compute_tendencies=True):
        g = self.grid
        self.mask_immersed_model_fields()
        for f, l, n in zip(self.fields, self.locs, self.names):
            if n != "w":
                O.fill_halo_regions(g, f, l, fill_boundary_normal_velocities=False, bcs=self.bcs.get(n))
        self._fill_eta()
        Hy.compute_w_from_continuity(g, self.u, self.v, self.w)   # (no immersed variant on a static grid with a grid-fitted bottom)
        if self.pHY is not None:
            T, S = self._buoyancy_tracers()
            O.update_hydrostatic_pressure(g, self.physics, T, S, self.pHY)
        if compute_tendencies:
            self.compute_tendencies()

    def compute_tendencies(self):
        g, B, ph = self.grid, self.B, self.physics
        Gu, Gv, Gw = self.Gn[0], self.Gn[1], self.Gn[2]
        explicit = self.split is None
        vector_invariant_tendencies(B, self.u, self.v, self.w, Gu, Gv, self.eta if explicit else None, self.gravity)
        coriolis_and_pressure(B, ph.f, self.u, self.v, self.pHY, Gu, Gv)
        if ph.nu is not None:
            viscous_terms(B, ph.nu, self.u, self.v, self.w, Gu, Gv)
        Gw[...] = 0.0
        for n, c in enumerate(self.tracers):
            tracer_tendency(B, self.u, self.v, self.w, c, self.Gn[3 + n], None if ph.nu is None else self.kappa[self.tracer_names[n]])
        for f, l, n, G in zip(self.fields, self.locs, self.names, self.Gn):
            if n in self.bcs and n != "w":
                O.apply_flux_bcs(g, l, f, G, self.bcs[n])

    def _split_explicit_step(self, dt, chi):
        self.GU[...] = split_explicit_forcing(self.B, self.Gn[0], self.Gm[0], chi, FCC)
        self.GV[...] = split_explicit_forcing(self.B, self.Gn[1], self.Gm[1], chi, CFC)
        self.etab[...] = 0.0
        self.Ub[...] = 0.0
        self.Vb[...] = 0.0

    def _substep(self, dt):
        g = self.grid
        ii, jj = slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny)
        eta = self.eta[ii, jj].copy()
        iterate_split_explicit(self.B, eta, self.U, self.V, self.etab, self.Ub, self.Vb, self.GU, self.GV, self.frac_dt * dt, self.weights,
                               self.gravity)
        self.eta[ii, jj] = self.etab
        self.U[...] = self.Ub
        self.V[...] = self.Vb
        mask_field(self.B, self.u, FCC)   # step_free_surface! ends with mask_immersed_field!(u), (v)
        mask_field(self.B, self.v, CFC)

    def _barotropic_corrector(self):
        self.Ub[...], self.Vb[...] = barotropic_corrector(self.B, self.u, self.v, self.U, self.V)
