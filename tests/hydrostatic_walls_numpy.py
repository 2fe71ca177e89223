"""TEST INFRASTRUCTURE (CPU restatement, never imported by the product): the reference's HydrostaticFreeSurfaceModel on grids with walls,
(Periodic, Bounded, Bounded) channels and (Bounded, Bounded, Bounded) basins, on top of oracle/oracle.py (whose fields, halo fills and
tendency kernels already know Bounded directions) and oracle/hydrostatic.py (whose periodic model is subclassed: everything that indexes
relative to the interior origin is inherited).  Restated here, in the reference's evaluation order:

  * the halo fill of η                      BoundaryConditions/fill_halo_regions.jl:50-68, fill_halo_regions_flux.jl:14-31 (ZFaceField at
                                            k = Nz + 1 with default conditions: no-flux along Bounded x / y, first halo cell only)
  * w from continuity on N + 1-face arrays  compute_w_from_continuity.jl:31-51
  * update_state!                           update_hydrostatic_free_surface_model_state.jl:35-53: tupled_fill_halo_regions! keeps
                                            fill_boundary_normal_velocities = true, so fill_open_boundary_regions! (fill_halo_regions_open.jl:
                                            65-70) resets the wall faces of the wall-normal velocities to 0
  * the split-explicit substeps             step_split_explicit_free_surface.jl:12-46 with δxTᶜᵃᵃ, δyTᵃᶜᵃ, ∂xTᶠᶜᶠ, ∂yTᶜᶠᶠ
                                            (Operators/topology_aware_operators.jl:32-67)
  * the implicit step                       implicit_free_surface.jl:124-145 (the velocities are filled first, :133),
                                            fft_based_implicit_free_surface_solver.jl:76-110 with a cosine transform along Bounded
                                            directions (poisson_eigenvalues.jl:8-31, plan_transforms.jl), barotropic_pressure_correction.jl:21-47

The wall faces.  The reference's tendency, AB2, corrector and pressure-correction kernels all run over 1:N without exclude_periphery
(compute_hydrostatic_free_surface_tendencies.jl:149-157, hydrostatic_free_surface_ab2_step.jl:46-47, barotropic_pressure_correction.jl:22,
barotropic_split_explicit_corrector.jl:43, 64): they write the west / south wall face (index 1) and never the east / north one (N + 1).
Whatever they leave on face 1 is read by nothing outside that face (the topology-aware differences ignore it; the implicit step fills the
velocities before it integrates them) and is reset to 0 by the next update_state!.  The kernels that this restatement and the product
share with NonhydrostaticModel (flux-form advection, Coriolis / pHY′ / diffusion terms, ab2_step) exclude the periphery and leave face 1
alone instead; the kernels of the hydrostatic layer itself run over 1:N.  u, v, w, η and the tracers after every step are the
reference's either way; only the wall-face entries of the barotropic transports U, V (which nothing reads) differ.
"""
import numpy as np

from oracle import hydrostatic as Hy
from oracle import oracle as O

B, P = O.BOUNDED, O.PERIODIC


def fill_eta(g, e):
    """fill_halo_regions!(η): Bounded directions first (no-flux: the first halo cell, over the interior of the other direction), Periodic
    directions last over the whole parent extent"""
    Hx, Hy, Nx, Ny = g.Hx, g.Hy, g.Nx, g.Ny
    if g.tx == B:
        e[Hx - 1, Hy:Hy + Ny] = e[Hx, Hy:Hy + Ny]
        e[Hx + Nx, Hy:Hy + Ny] = e[Hx + Nx - 1, Hy:Hy + Ny]
    if g.ty == B:
        e[Hx:Hx + Nx, Hy - 1] = e[Hx:Hx + Nx, Hy]
        e[Hx:Hx + Nx, Hy + Ny] = e[Hx:Hx + Nx, Hy + Ny - 1]
    if g.tx == P:
        e[:Hx, :] = e[Nx:Nx + Hx, :]
        e[Nx + Hx:, :] = e[Hx:2 * Hx, :]
    if g.ty == P:
        e[:, :Hy] = e[:, Ny:Ny + Hy]
        e[:, Ny + Hy:] = e[:, Hy:2 * Hy]


def compute_w_from_continuity(g, u, v, w):
    """w[i, j, 1] = 0; w[i, j, k] = w[i, j, k-1] - flux_div_xyᶜᶜᶜ(i, j, k-1, u, v) / Azᶜᶜᶜ for i = 1 - Hx .. Nx + Hx - 1, j = 1 - Hy .. Ny + Hy - 1:
    every column of w whose east / north neighbours exist whatever the topology (a superset of w_kernel_parameters, :43-51).  u, v, w
    each in its own parent."""
    Hz, Nz = g.Hz, g.Nz
    dzc = np.full(Nz, g.dz) if g.dzc is None else np.asarray(g.dzc[Hz:Hz + Nz])
    Az = g.dx * g.dy
    nI, nJ = g.Nx + 2 * g.Hx - 1, g.Ny + 2 * g.Hy - 1
    w[:nI, :nJ, Hz] = 0.0
    for k in range(1, Nz + 1):
        kc = Hz + k - 1
        Ax, Ay = g.dy * dzc[k - 1], g.dx * dzc[k - 1]
        dxu = Ax * u[1:nI + 1, :nJ, kc] - Ax * u[:nI, :nJ, kc]
        dyv = Ay * v[:nI, 1:nJ + 1, kc] - Ay * v[:nI, :nJ, kc]
        dh = (dxu + dyv) / Az
        w[:nI, :nJ, Hz + k] = w[:nI, :nJ, Hz + k - 1] - (dh + 0.0)


def delta_T_face_to_centre(F, bounded, axis):
    """δxTᶜᵃᵃ / δyTᵃᶜᵃ of an interior (N) array of transports: f(i+1) - f(i), wrapped (Periodic) or, across a wall, -f(N) at i = N and f(2)
    at i = 1 (topology_aware_operators.jl:35-36, 48-56)"""
    if not bounded:
        return np.roll(F, -1, axis) - F
    F = np.moveaxis(F, axis, 0)
    d = np.empty_like(F)
    d[1:-1] = F[2:] - F[1:-1]
    d[0] = F[1]
    d[-1] = -F[-1]
    return np.moveaxis(d, 0, axis)


def delta_T_centre_to_face(c, bounded, axis):
    """δxTᶠᵃᵃ / δyTᵃᶠᵃ of an interior (N) array at centres: c(i) - c(i-1), wrapped or 0 on the wall face i = 1 (:32-33, 40-41)"""
    if not bounded:
        return c - np.roll(c, 1, axis)
    c = np.moveaxis(c, axis, 0)
    d = np.zeros_like(c)
    d[1:] = c[1:] - c[:-1]
    return np.moveaxis(d, 0, axis)


def iterate_split_explicit(eta, U, V, etab, Ub, Vb, GU, GV, dtau, weights, grav, H, dx, dy, bx, by):
    """iterate_split_explicit! with the ForwardBackwardScheme (step_split_explicit_free_surface.jl:12-46, 62-98), in place on interior
    (Nx, Ny) arrays; bx, by: Bounded x, y"""
    Az = dx * dy
    for wgt in weights:
        eta[...] = eta - dtau * (delta_T_face_to_centre(dy * U, bx, 0) + delta_T_face_to_centre(dx * V, by, 1)) / Az
        Un = U + dtau * (-grav * H * (delta_T_centre_to_face(eta, bx, 0) / dx) + GU)
        Vn = V + dtau * (-grav * H * (delta_T_centre_to_face(eta, by, 1) / dy) + GV)
        etab += wgt * eta
        Ub += wgt * Un
        Vb += wgt * Vn
        U[...] = Un
        V[...] = Vn


def volume_flux(g, u, v):
    """compute_vertically_integrated_volume_flux!: sum!(Ax u), sum!(Ay v) over the interiors of the Face fields, the N + 1 wall face included;
    returns Qu (Nx + bx, Ny), Qv (Nx, Ny + by)"""
    Hx, Hy, Hz = g.Hx, g.Hy, g.Hz
    bx, by = int(g.tx == B), int(g.ty == B)
    dz = np.full(g.Nz, g.dz) if g.dzc is None else np.asarray(g.dzc[Hz:Hz + g.Nz])
    Qu, Qv = np.zeros((g.Nx + bx, g.Ny)), np.zeros((g.Nx, g.Ny + by))
    for k in range(g.Nz):
        Qu = Qu + (g.dy * dz[k]) * u[Hx:Hx + g.Nx + bx, Hy:Hy + g.Ny, Hz + k]
        Qv = Qv + (g.dx * dz[k]) * v[Hx:Hx + g.Nx, Hy:Hy + g.Ny + by, Hz + k]
    return Qu, Qv


def implicit_rhs(g, Qu, Qv, eta_interior, grav, dt):
    """fft_implicit_free_surface_right_hand_side!: (δx Qu + δy Qv - Az η / Δt) / (g Lz Δt Az)"""
    Az = g.dx * g.dy
    dQu = (Qu[1:] - Qu[:-1]) if g.tx == B else (np.roll(Qu, -1, 0) - Qu)
    dQv = (Qv[:, 1:] - Qv[:, :-1]) if g.ty == B else (np.roll(Qv, -1, 1) - Qv)
    return ((dQu + dQv) - Az * eta_interior / dt) / (grav * g.Lz * dt * Az)


def solve_shifted(g, rhs, m):
    """solve!(η, solver, rhs, m) on the horizontal (TX, TY, Flat) grid (fft_based_poisson_solver.jl:95-125): cosine transforms along Bounded
    directions, then Fourier transforms along Periodic ones; η̂ = -rhŝ / (λx + λy + 0 - m)"""
    lx = O.poisson_eigenvalues(g.Nx, g.Lx, g.tx)
    ly = O.poisson_eigenvalues(g.Ny, g.Ly, g.ty)
    hat = O._forward(rhs.astype(np.complex128), g, (0, 1), 1)
    hat = -hat / ((lx[:, None] + ly[None, :]) + 0.0 - m)
    return np.real(O._backward(hat, g, (0, 1), 1))


def barotropic_pressure_correction(g, u, v, e, grav, dt):
    """_barotropic_pressure_correction!: u -= g Δt ∂xᶠᶜᶠ η, v -= g Δt ∂yᶜᶠᶠ η over 1:N at every level (η halos filled)"""
    ii, jj = slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny)
    ui, vi = g.interior_N(u), g.interior_N(v)
    ui[...] = ui - (grav * dt * ((e[ii, jj] - e[g.Hx - 1:g.Hx + g.Nx - 1, jj]) / g.dx))[:, :, None]
    vi[...] = vi - (grav * dt * ((e[ii, jj] - e[ii, g.Hy - 1:g.Hy + g.Ny - 1]) / g.dy))[:, :, None]


def _dz_centres(g):
    return np.full(g.Nz, g.dz) if g.dzc is None else np.asarray(g.dzc[g.Hz:g.Hz + g.Nz])


def barotropic_mode(g, f):
    """integrate_barotropic_mode! (barotropic_split_explicit_corrector.jl:13-32), σ = 1: Σₖ Δz f over 1:Nx, 1:Ny, k upwards"""
    dz, fi = _dz_centres(g), g.interior_N(f)
    out = dz[0] * fi[:, :, 0] * 1.0
    for k in range(1, g.Nz):
        out = out + dz[k] * fi[:, :, k] * 1.0
    return out


def split_explicit_forcing(g, Gn, Gm, chi):
    """compute_split_explicit_forcing! (compute_slow_tendencies.jl:12-32): Σₖ Δz ((3/2 + χ) Gⁿ - (1/2 + χ) G⁻ not_euler)"""
    dz, gn, gm = _dz_centres(g), g.interior_N(Gn), g.interior_N(Gm)
    C1, C2 = 3 * 1.0 / 2 + chi, 1.0 / 2 + chi
    ne = 1.0 if C2 != 0 else 0.0
    acc = dz[0] * (C1 * gn[:, :, 0] - C2 * gm[:, :, 0] * ne)
    for k in range(1, g.Nz):
        acc = acc + dz[k] * (C1 * gn[:, :, k] - C2 * gm[:, :, k] * ne)
    return acc


def barotropic_corrector(g, u, v, U, V):
    """barotropic_split_explicit_corrector! (:44-71) on interior planes U, V: returns the recomputed U̅, V̅; u, v corrected in place"""
    Ub, Vb = barotropic_mode(g, u), barotropic_mode(g, v)
    ui, vi = g.interior_N(u), g.interior_N(v)
    ui[...] = ui + ((U - Ub) / g.Lz)[:, :, None]
    vi[...] = vi + ((V - Vb) / g.Lz)[:, :, None]
    return Ub, Vb


def add_barotropic_pressure_gradient(g, grav, e, Gu, Gv):
    """Gu -= g ∂xᶠᶜᶜ η, Gv -= g ∂yᶜᶠᶜ η over 1:N at every level (explicit_free_surface.jl:36-40)"""
    ii, jj = slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny)
    g.interior_N(Gu)[...] -= (grav * ((e[ii, jj] - e[g.Hx - 1:g.Hx + g.Nx - 1, jj]) / g.dx))[:, :, None]
    g.interior_N(Gv)[...] -= (grav * ((e[ii, jj] - e[ii, g.Hy - 1:g.Hy + g.Ny - 1]) / g.dy))[:, :, None]


def explicit_free_surface_ab2_step(g, w, e, Gn, Gm, dt, chi):
    """Gη = w[i, j, Nz + 1]; η += Δt ((3/2 + χ) Gηⁿ - (1/2 + χ) Gη⁻ not_euler) over the interior (explicit_free_surface.jl:84-140)"""
    ii, jj = slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny)
    Gn[ii, jj] = w[ii, jj, g.Hz + g.Nz]
    ne = 0.0 if chi == -0.5 else 1.0
    e[ii, jj] += dt * ((1.5 + chi) * Gn[ii, jj] - (0.5 + chi) * Gm[ii, jj] * ne)


class HydrostaticFreeSurfaceModel(Hy.HydrostaticFreeSurfaceModel):
    """oracle/hydrostatic.py's model on a (Periodic | Bounded, Bounded, Bounded) grid.  The barotropic planes stay interior (Nx, Ny)
    arrays: U[i, j] sits on face i of cell (i, j), i = 1 .. Nx."""

    def __init__(self, grid, tracers=(), momentum_advection="Centered2", tracer_advection=None, coriolis_f=None, closure=None, coriolis_beta=None,
                 buoyancy=None, boundary_conditions=None, gravitational_acceleration=Hy.g_Earth, split_explicit_substeps=None,
                 implicit_free_surface=False):
        assert grid.topo[2] == B and grid.topo[1] == B and grid.topo[0] in (P, B)
        self.split_rk3 = False
        self.implicit = bool(implicit_free_surface)
        assert not (self.implicit and split_explicit_substeps is not None)
        self.split = split_explicit_substeps
        self.ab3 = None
        if self.split is not None:
            self.frac_dt, self.weights = Hy.weights_from_substeps(int(self.split))
            shp = (grid.Nx, grid.Ny)
            self.U, self.V, self.Ub, self.Vb, self.etab, self.GU, self.GV = (np.zeros(shp) for _ in range(7))
            self.initialized = False
        self.eta = np.zeros((grid.Nx + 2 * grid.Hx, grid.Ny + 2 * grid.Hy), order="F")
        self.g_eta = np.zeros_like(self.eta)
        self.g_eta_m = np.zeros_like(self.eta)
        self.gravity = float(gravitational_acceleration)
        self.tracer_scheme = None
        self.vector_invariant = momentum_advection == "VectorInvariant"
        if self.vector_invariant and tracer_advection is None:
            tracer_advection = "Centered2"
        O.NonhydrostaticModel.__init__(self, grid, tracers=tracers, timestepper="QuasiAdamsBashforth2",
                                       advection=tracer_advection if self.vector_invariant else momentum_advection, coriolis_f=coriolis_f,
                                       coriolis_beta=coriolis_beta, closure=closure, buoyancy=buoyancy, boundary_conditions=boundary_conditions)
        ta = momentum_advection if tracer_advection is None else tracer_advection
        self.tracer_scheme = {"WENO5": O.ADV_WENO5, "Centered2": O.ADV_CENTERED2, "UpwindBiased5": O.ADV_UPWIND5}[ta]
        self.solver = None
        self.update_state(compute_tendencies=False)

    def _fill_eta(self):
        fill_eta(self.grid, self.eta)

    def update_state(self, compute_tendencies=True):
        g = self.grid
        for f, l, n in zip(self.fields, self.locs, self.names):
            if n != "w":  # fill_boundary_normal_velocities = true (the default): the wall faces of u, v are reset
                O.fill_halo_regions(g, f, l, fill_boundary_normal_velocities=True, bcs=self.bcs.get(n))
        self._fill_eta()
        compute_w_from_continuity(g, self.u, self.v, self.w)
        if self.pHY is not None:
            T, S = self._buoyancy_tracers()
            O.update_hydrostatic_pressure(g, self.physics, T, S, self.pHY)
        if compute_tendencies:
            self.compute_tendencies()

    def _substep(self, dt):
        g = self.grid
        Hx, Hy = g.Hx, g.Hy
        eta = self.eta[Hx:Hx + g.Nx, Hy:Hy + g.Ny].copy()
        iterate_split_explicit(eta, self.U, self.V, self.etab, self.Ub, self.Vb, self.GU, self.GV, self.frac_dt * dt, self.weights,
                               self.gravity, g.Lz, g.dx, g.dy, g.tx == B, g.ty == B)
        self.eta[Hx:Hx + g.Nx, Hy:Hy + g.Ny] = self.etab
        self.U[...] = self.Ub
        self.V[...] = self.Vb

    def _implicit_step(self, dt):
        g, grav = self.grid, self.gravity
        for f, l, n in ((self.u, O.LOC_U, "u"), (self.v, O.LOC_V, "v")):  # fill_halo_regions!(model.velocities, ...) (:133)
            O.fill_halo_regions(g, f, l, bcs=self.bcs.get(n))
        Qu, Qv = volume_flux(g, self.u, self.v)
        ii, jj = slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny)
        rhs = implicit_rhs(g, Qu, Qv, self.eta[ii, jj], grav, dt)
        self.eta[ii, jj] = solve_shifted(g, rhs, -1.0 / (grav * g.Lz * dt ** 2))
        self._fill_eta()
        barotropic_pressure_correction(g, self.u, self.v, self.eta, grav, dt)
