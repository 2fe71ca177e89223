// tke_dissipation.hip -- TKEDissipationVerticalDiffusivity, the k-ϵ closure (turbulence_closure_implementations/
// TKEBasedVerticalDiffusivities/): the diffusivities κᵘ, κᶜ, κᵉ, κᵋ at (Center, Center, Face), the top fluxes of e and ϵ and the substep of e
// and ϵ with their two implicit solves, on a (Periodic, Periodic, Bounded) grid.
//
//  tke_dissipation_vertical_diffusivity.jl:228-354   compute_diffusivities!, minimum_dissipation, dissipationᶜᶜᶜ, κuᶜᶜᶠ, κcᶜᶜᶠ, κeᶜᶜᶠ, κϵᶜᶜᶠ
//  tke_dissipation_stability_functions.jl            the constant and the rational stability functions, their two clamps
//  tke_dissipation_equations.jl:90-251               substep_tke_dissipation!, top_tke_flux, top_dissipation_flux
//  TKEBasedVerticalDiffusivities.jl:57-156           shearᶜᶜᶠ, ℑbzᵃᵃᶜ, explicit_buoyancy_flux, shear_production, mask_diffusivity
//  vertically_implicit_diffusion_solver.jl:55-110    the rows of the solves, with the linear coefficient in the diagonal
//
// The geometry of catke.hip: one thread owns one (i, j) column and marches upwards, x fastest across the lanes.  An iteration computes face
// k + 1 from planes k and k + 1 and then finishes cell k.  Carried in registers, so that every input is read once per cell: N² of the faces
// ahead (ϵ★ of cell k + 1 needs N² of faces k + 1 and k + 2, so a face needs three), e★, ϵ★ and e★² / ϵ★² of the lower cell, the velocities
// of the lower plane.  Each quantity is computed once per face or cell (the reference recomputes e², ϵ̄ and the stability function for
// every κ).  κ of face 1 is the 0 of mask_diffusivity, face Nz + 1 is not written.  Every read of e and ϵ is of the values before the call
// (the reference's kernel reads the neighbours while other threads write them).  Rows k of the two solves need κᵉ, κᵋ of faces k, k + 1 and
// Le, Lϵ of cell k, all known when cell k is finished: both forward eliminations run in the same march, the multipliers go to two scratch
// arrays and the two backward sweeps follow in the same thread.
//
// Strict build (no FMA contraction, IEEE division and square root), min / max / Bool products of ocn_catke.h: bit-identical to
// tests/tke_dissipation_numpy.py.  What is shared with the other vertical closures (ocn_buoyancy.h, ocn_tke_columns.h) and what is not:
// DESIGN.md §5.2s.
#include <cmath>
#include <cstddef>

#include "ocn_buoyancy.h"
#include "ocn_catke.h"
#include "ocn_ivd.h"
#include "ocn_tke_columns.h"

namespace ocn {

namespace tked {

using catke::bmul;
using catke::jmax;
using catke::jmin;
using ivd::Spacings;
using tke::bz;

enum Mode { MODE_DIFFUSIVITIES = 0, MODE_SUBSTEP = 1 };

struct Args {
    double Lz;
    const double *u, *v;  // the current (next) velocities
    const double *u_prev, *v_prev;
    const double *e_in, *eps_in;  // MODE_DIFFUSIVITIES
    double *e, *eps;              // MODE_SUBSTEP, in place
    const double *ku_in, *kc_in;  // MODE_SUBSTEP: κᵘ, κᶜ of the last compute_TKEDissipation_diffusivities!
    double *kappa_u, *kappa_c, *kappa_e, *kappa_eps;
    double *Le, *Leps;
    const double *Gn_e, *Gn_eps;
    double *Gm_e, *Gm_eps;
    double *t_e, *t_eps;
    double dtau, chi;
    int solve;
};

// Julia's clamp(x, lo, hi) = ifelse(x > hi, hi, ifelse(x < lo, lo, x)): a NaN x comes back, a NaN bound never binds
__device__ __forceinline__ double jclamp(double x, double lo, double hi) { return x > hi ? hi : (x < lo ? lo : x); }

// what a face needs of one of its two cells
struct Cell {
    double e, eps;  // as stored
    double es;      // e★ = max(minimum_tke, e)
    double epss;    // ϵ★ = clamp(ϵ, ϵmin, inf)
    double es2;     // e★²
    double tau2;    // e★² / ϵ★²
};

// turbulent_kinetic_energyᶜᶜᶜ, minimum_dissipation, dissipationᶜᶜᶜ, square_time_scaleᶜᶜᶜ; n2_lo, n2_hi: ∂z_b of the two faces of the cell,
// p_lo, p_hi: whether they are peripheral (ℑbzᵃᵃᶜ replaces such a face by the other)
__device__ __forceinline__ Cell make_cell(const ocn_tke_dissipation &cl, double Lz, double e, double eps, double n2_lo, double n2_hi, bool p_lo,
                                          bool p_hi)
{
    Cell c;
    c.e = e;
    c.eps = eps;
    c.es = jmax(cl.minimum_tke, e);
    const double a_lo = jmax(cl.minimum_buoyancy_frequency, n2_lo), a_hi = jmax(cl.minimum_buoyancy_frequency, n2_hi);
    const double N2p = bz(a_lo, a_hi, p_lo, p_hi);
    const double lst = cl.C_N * sqrt(c.es / N2p);
    const double lmin = jmin(Lz, lst);
    const double s = sqrt(c.es);
    const double eps_min = jmax(1e-12, cl.Su0_cubed * (s * s * s) / lmin);
    c.epss = jclamp(eps, eps_min, INFINITY);
    c.es2 = c.es * c.es;
    c.tau2 = c.es2 / (c.epss * c.epss);
    return c;
}

// maximum_shear_number (Umlauf & Burchard 2005, eq. 44)
__device__ __forceinline__ double maximum_shear_number(const ocn_tke_dissipation &cl, double aN)
{
    const double n0 = cl.Cu0, n1 = cl.Cu1, d0 = cl.Cd0, d1 = cl.Cd1, d2 = cl.Cd2, d3 = cl.Cd3, d4 = cl.Cd4;
    const double e0 = d0 * n0, e1 = d0 * n1 + d1 * n0, e2 = d1 * n1 + d4 * n0, e3 = d4 * n1, e4 = d2 * n0, e5 = d2 * n1 + d3 * n0, e6 = d3 * n1;
    const double num = e0 + e1 * aN + e2 * (aN * aN) + e3 * (aN * aN * aN);
    const double den = e4 + e5 * aN + e6 * (aN * aN);
    return num / den;
}

struct Kappas {
    double u, c, e, eps;
};

// κuᶜᶜᶠ, κcᶜᶜᶠ, κeᶜᶜᶠ, κϵᶜᶜᶠ of an interior face from its two cells, ∂z_b and shearᶜᶜᶠ; ALL = false: κᵉ and κᵋ only
template <int KIND, bool ALL>
__device__ __forceinline__ Kappas face_kappas(const ocn_tke_dissipation &cl, const Cell &lo, const Cell &hi, double N2, double S2)
{
    const double e2 = 0.5 * (lo.es2 + hi.es2);
    const double eps = 0.5 * (lo.epss + hi.epss);
    double Su, Sc;
    if (KIND == OCN_STABILITY_CONSTANT) {
        Su = cl.Cu0;
        Sc = cl.Cc0;
    } else {
        const double tau2 = 0.5 * (lo.tau2 + hi.tau2);
        double aN = tau2 * N2, aM = tau2 * S2;
        aN = jclamp(aN, cl.minimum_stratification_number, 1e10);
        aM = jclamp(aM, 0.0, maximum_shear_number(cl, aN));
        const double den = cl.Cd0 + cl.Cd1 * aN + cl.Cd2 * aM + cl.Cd3 * aN * aM + cl.Cd4 * (aN * aN) + cl.Cd5 * (aM * aM);
        Su = (cl.Cu0 + cl.Cu1 * aN + cl.Cu2 * aM) / den;
        Sc = (cl.Cc0 + cl.Cc1 * aN + cl.Cc2 * aM) / den;
    }
    Kappas k{};
    if (ALL) {
        k.u = jmin(Su * e2 / eps, cl.maximum_viscosity);
        k.c = jmin(Sc * e2 / eps, cl.maximum_tracer_diffusivity);
    }
    k.e = jmin(Su / cl.C_sigma_e * e2 / eps, cl.maximum_tke_diffusivity);
    k.eps = jmin(Su / cl.C_sigma_eps * e2 / eps, cl.maximum_dissipation_diffusivity);
    return k;
}

// what a cell needs of one of its faces (the substep)
struct Face {
    double wb;                          // buoyancy_fluxᶜᶜᶠ = -κᶜ N²
    double Pn[2], Pp[2], Qn[2], Qp[2];  // Δz_νₑ_az_bzᶠᶜᶠ(uⁿ, u⁺), (u⁺, u⁺) at i, i + 1; ...ᶜᶠᶠ(vⁿ, v⁺), (v⁺, v⁺) at j, j + 1
    double ke, keps;                    // κᵉ, κᵋ (masked)
};

template <int MODE, int KIND>
__global__ __launch_bounds__(256) void tke_dissipation_columns(GridDev g, Buoyancy b, ocn_tke_dissipation cl, Args a)
{
    const int i = 1 + blockIdx.x * 64 + threadIdx.x, j = 1 + blockIdx.y * 4 + threadIdx.y;
    if (i > g.Nx || j > g.Ny) return;
    const int Nz = g.Nz;
    const Spacings M = ivd::spacings_of(g);
    const Lay Lc = make_lay(g, OCN_LOC_CCC), Lu = make_lay(g, OCN_LOC_FCC), Lv = make_lay(g, OCN_LOC_CFC), Lf = make_lay(g, OCN_LOC_CCF);
    const long long c3 = Lc.s3, u3 = Lu.s3, v3 = Lv.s3, f3 = Lf.s3, v2 = Lv.s2, f2 = Lf.s2;
    const long long oc = at(Lc, i, j, 1), of = at(Lf, i, j, 1);  // cell k at oc + (k - 1) c3, face k at of + (k - 1) f3
    const double *__restrict__ Tp = b.T ? b.T + oc : nullptr;
    const double *__restrict__ Sp = b.S ? b.S + oc : nullptr;
    const double *ep = (MODE == MODE_SUBSTEP ? a.e : a.e_in) + oc;
    const double *pp = (MODE == MODE_SUBSTEP ? a.eps : a.eps_in) + oc;
    const double *__restrict__ un = a.u + at(Lu, i, j, 1), *__restrict__ vn = a.v + at(Lv, i, j, 1);
    const double *__restrict__ uo = MODE == MODE_SUBSTEP ? a.u_prev + at(Lu, i, j, 1) : nullptr;
    const double *__restrict__ vo = MODE == MODE_SUBSTEP ? a.v_prev + at(Lv, i, j, 1) : nullptr;
    const double emin = cl.minimum_tke;

    // carried upwards: T, S of the upper plane of the highest face whose N² is known, N² of faces k, k + 1 (and k + 2 inside an iteration),
    // cell k, the velocities of plane k, the face k of the cell
    const double T1 = Tp ? Tp[0] : 0.0, S1 = Sp ? Sp[0] : 0.0;
    double T_up = Tp ? Tp[c3] : 0.0, S_up = Sp ? Sp[c3] : 0.0;
    double n2_lo = 0.0;  // face 1, from the bottom halo plane: only the plain ℑzᵃᵃᶜ of the substep reads it
    if (MODE == MODE_SUBSTEP) n2_lo = dz_b(b, T1, Tp ? Tp[-c3] : 0.0, S1, Sp ? Sp[-c3] : 0.0, M.dzF(1));
    double n2_hi = dz_b(b, T_up, T1, S_up, S1, M.dzF(2));
    Cell c_lo = make_cell(cl, a.Lz, ep[0], pp[0], n2_lo, n2_hi, true, false);
    double un0 = un[0], un1 = un[1], vn0 = vn[0], vn1 = vn[v2];
    double uo0 = 0.0, uo1 = 0.0, vo0 = 0.0, vo1 = 0.0;
    if (MODE == MODE_SUBSTEP) {
        uo0 = uo[0]; uo1 = uo[1]; vo0 = vo[0]; vo1 = vo[v2];
    }
    Face lo{}, hi{};
    if (MODE == MODE_DIFFUSIVITIES) {  // mask_diffusivity: peripheral_node(i, j, 1, grid, c, c, f)
        a.kappa_u[of] = 0.0;
        a.kappa_c[of] = 0.0;
    }
    a.kappa_e[of] = 0.0;
    a.kappa_eps[of] = 0.0;
    tke::Elimination se{}, sp{};
    const double ab_alpha = 1.5 + a.chi, ab_beta = 0.5 + a.chi;
    const long long t2 = (long long)g.Nx * g.Ny, ot = (i - 1) + (long long)g.Nx * (j - 1);

    for (int k = 1; k <= Nz; ++k) {
        // N² of face k + 2; the substep needs that of face Nz + 1 (from the first top halo plane), the diffusivities do not
        double n2_top = n2_hi;
        if (k + 2 <= Nz + (MODE == MODE_SUBSTEP ? 1 : 0)) {
            const double T2 = Tp ? Tp[(k + 1) * c3] : 0.0, S2 = Sp ? Sp[(k + 1) * c3] : 0.0;
            n2_top = dz_b(b, T2, T_up, S2, S_up, M.dzF(k + 2));
            T_up = T2;
            S_up = S2;
        }
        // face k + 1, from planes k and k + 1
        Cell c_hi = c_lo;
        if (k + 1 <= Nz) {
            const int f = k + 1;
            const double dzf = M.dzF(f);
            const double a0 = un[k * u3], a1 = un[k * u3 + 1], b0 = vn[k * v3], b1 = vn[k * v3 + v2];
            const double du0 = (a0 - un0) / dzf, du1 = (a1 - un1) / dzf, dv0 = (b0 - vn0) / dzf, dv1 = (b1 - vn1) / dzf;
            const double S2 = 0.5 * (du0 * du0 + du1 * du1) + 0.5 * (dv0 * dv0 + dv1 * dv1);  // shearᶜᶜᶠ
            const double N2 = n2_hi;
            c_hi = make_cell(cl, a.Lz, ep[k * c3], pp[k * c3], n2_hi, n2_top, false, f == Nz);
            const Kappas kap = face_kappas<KIND, MODE == MODE_DIFFUSIVITIES>(cl, c_lo, c_hi, N2, S2);
            const long long o = of + k * f3;
            if (MODE == MODE_DIFFUSIVITIES) {
                a.kappa_u[o] = kap.u;
                a.kappa_c[o] = kap.c;
            }
            a.kappa_e[o] = kap.e;
            a.kappa_eps[o] = kap.eps;
            if (MODE == MODE_SUBSTEP) {
                hi.ke = kap.e;
                hi.keps = kap.eps;
                hi.wb = -a.kc_in[o] * N2;
                const double *__restrict__ q = a.ku_in + o;
                const double kh = q[0];
                const double nx0 = 0.5 * (q[-1] + kh), nx1 = 0.5 * (kh + q[1]);    // ℑxᶠᵃᵃ(κᵘ) at i, i + 1
                const double ny0 = 0.5 * (q[-f2] + kh), ny1 = 0.5 * (kh + q[f2]);  // ℑyᵃᶠᵃ(κᵘ) at j, j + 1
                const double p0 = uo[k * u3], p1 = uo[k * u3 + 1], r0 = vo[k * v3], r1 = vo[k * v3 + v2];
                const double eu0 = (p0 - uo0) / dzf, eu1 = (p1 - uo1) / dzf, ev0 = (r0 - vo0) / dzf, ev1 = (r1 - vo1) / dzf;
                hi.Pn[0] = nx0 * eu0 * dzf * du0; hi.Pn[1] = nx1 * eu1 * dzf * du1;
                hi.Pp[0] = nx0 * du0 * dzf * du0; hi.Pp[1] = nx1 * du1 * dzf * du1;
                hi.Qn[0] = ny0 * ev0 * dzf * dv0; hi.Qn[1] = ny1 * ev1 * dzf * dv1;
                hi.Qp[0] = ny0 * dv0 * dzf * dv0; hi.Qp[1] = ny1 * dv1 * dzf * dv1;
                uo0 = p0; uo1 = p1; vo0 = r0; vo1 = r1;
            }
            un0 = a0; un1 = a1; vn0 = b0; vn1 = b1;
        }
        if (MODE == MODE_SUBSTEP) {
            // cell k: ℑbzᵃᵃᶜ of its faces k (lo) and k + 1 (hi), a peripheral face replaced by the other
            const bool p_lo = k == 1, p_hi = k == Nz;
            auto bzk = [&](double x_lo, double x_hi) { return bz(x_lo, x_hi, p_lo, p_hi); };
            const double ek = c_lo.e, pk = c_lo.eps, es = c_lo.es, dzc = M.dzC(k);
            const double omega_star = c_lo.epss / es;
            const double omega_e = ek < 0 ? cl.negative_tke_damping_time_scale : omega_star;  // (the time scale itself, as in the reference)
            const double omega_eps = pk / es;
            const double wb = bzk(lo.wb, hi.wb);  // explicit_buoyancy_flux
            const double wb_minus = jmin(wb, 0.0), wb_plus = jmax(wb, 0.0);
            const double wb_e = bmul(wb_minus / ek, ek > emin);
            const double N2 = 0.5 * (n2_lo + n2_hi);  // the plain ℑzᵃᵃᶜ(∂z_b): faces 1 and Nz + 1 from the z halos of the tracers
            const double Cb = N2 >= 0 ? cl.C_b_eps_plus : cl.C_b_eps_minus;
            const double Cb_wb = Cb * wb;
            const double Cb_wb_minus = jmin(Cb_wb, 0.0), Cb_wb_plus = jmax(Cb_wb, 0.0);
            const double L_e = wb_e - omega_e;
            const double L_eps = Cb_wb_minus / es - cl.C_eps_eps * omega_eps;
            const long long og = oc + (k - 1) * c3;
            a.Le[og] = L_e;
            a.Leps[og] = L_eps;
            const double Px0 = (bzk(lo.Pn[0], hi.Pn[0]) + bzk(lo.Pp[0], hi.Pp[0])) / (2 * dzc);
            const double Px1 = (bzk(lo.Pn[1], hi.Pn[1]) + bzk(lo.Pp[1], hi.Pp[1])) / (2 * dzc);
            const double Py0 = (bzk(lo.Qn[0], hi.Qn[0]) + bzk(lo.Qp[0], hi.Qp[0])) / (2 * dzc);
            const double Py1 = (bzk(lo.Qn[1], hi.Qn[1]) + bzk(lo.Qp[1], hi.Qp[1])) / (2 * dzc);
            const double P = 0.5 * (Px0 + Px1) + 0.5 * (Py0 + Py1);  // shear_production
            const double total_e = a.Gn_e[og] + (P + wb_plus);
            const double total_eps = a.Gn_eps[og] + omega_eps * (cl.C_P_eps * P + Cb_wb_plus);
            const double e_new = ek + a.dtau * (ab_alpha * total_e - ab_beta * a.Gm_e[og]);
            const double eps_new = pk + a.dtau * (ab_alpha * total_eps - ab_beta * a.Gm_eps[og]);
            a.Gm_e[og] = total_e;
            a.Gm_eps[og] = total_eps;
            if (!a.solve) {
                a.e[og] = e_new;
                a.eps[og] = eps_new;
            } else {
                const double dzf_lo = M.dzF(k), dzf_hi = M.dzF(k + 1);
                const long long o = ot + t2 * (k - 1);
                a.e[og] = tke::eliminate(se, k, Nz, a.dtau, lo.ke, hi.ke, L_e, e_new, dzc, dzf_lo, dzf_hi, a.t_e + o);
                a.eps[og] = tke::eliminate(sp, k, Nz, a.dtau, lo.keps, hi.keps, L_eps, eps_new, dzc, dzf_lo, dzf_hi, a.t_eps + o);
            }
        }
        lo = hi;
        n2_lo = n2_hi;
        n2_hi = n2_top;
        c_lo = c_hi;
    }
    if (MODE == MODE_SUBSTEP && a.solve) {  // the backward sweeps: c[k] -= t[k + 1] c[k + 1]
        double e_up = se.prev, eps_up = sp.prev;
        for (int k = Nz - 1; k >= 1; --k) {
            const long long og = oc + (k - 1) * c3, o = ot + t2 * k;
            e_up = a.e[og] - a.t_e[o] * e_up;
            eps_up = a.eps[og] - a.t_eps[o] * eps_up;
            a.e[og] = e_up;
            a.eps[og] = eps_up;
        }
    }
}

// the plane kernel: the top fluxes of e (top_tke_flux) and of ϵ (top_dissipation_flux)
struct PlaneArgs {
    const double *zc;
    const double *u, *v, *e;
    ZBc top_u, top_v;
    double *Qe, *Qeps;
};

__global__ __launch_bounds__(256) void top_fluxes(GridDev g, ocn_tke_dissipation cl, PlaneArgs a)
{
    const int i = 1 + blockIdx.x * 64 + threadIdx.x, j = 1 + blockIdx.y * 4 + threadIdx.y;
    if (i > g.Nx || j > g.Ny) return;
    const int Nz = g.Nz;
    const Lay Lc = make_lay(g, OCN_LOC_CCC), Lu = make_lay(g, OCN_LOC_FCC), Lv = make_lay(g, OCN_LOC_CFC);
    const double tau_x = a.top_u.kind == OCN_BC_FLUX ? bc_condition(a.top_u, i, j, g.Nx, a.u[at(Lu, i, j, Nz)]) : 0.0;
    const double tau_y = a.top_v.kind == OCN_BC_FLUX ? bc_condition(a.top_v, i, j, g.Nx, a.v[at(Lv, i, j, Nz)]) : 0.0;
    const double u_star = sqrt(sqrt(tau_x * tau_x + tau_y * tau_y));  // friction_velocity
    const long long op = (i - 1) + (long long)g.Nx * (j - 1);
    a.Qe[op] = -cl.C_W_ustar * (u_star * u_star * u_star);  // (wΔ³ is computed and unused in the reference)
    const double l_charnock = cl.C_W_alpha * (u_star * u_star) / cl.gravitational_acceleration;
    const double l_r = jmax(cl.minimum_roughness_length, l_charnock);
    const double es = jmax(cl.minimum_tke, a.e[at(Lc, i, j, Nz)]);
    const double d = -uniform_load(a.zc, Nz - 1);
    a.Qeps[op] = -cl.Su0_fourth_over_sigma_eps * (es * es) / (d + l_r);
}

// ---- argument checks: nothing here touches a device -----------------------------------------------------------------------------------
static int validate_grid_and_closure(const ocn_grid *grid, const ocn_tke_dissipation *c, const char *who)
{
    OCN_TRY(tke::validate_tke_grid(grid, who));
    OCN_REQUIRE(c, "%s: null closure", who);
    // every member in front of the four maxima is a coefficient or a constant derived from coefficients (doubles only up to there)
    constexpr size_t n_coefficients = offsetof(ocn_tke_dissipation, maximum_tracer_diffusivity) / sizeof(double);
    static_assert(offsetof(ocn_tke_dissipation, C_eps_eps) == 0 && offsetof(ocn_tke_dissipation, maximum_tracer_diffusivity) % sizeof(double) == 0,
                  "ocn_tke_dissipation: coefficients first, doubles");
    OCN_TRY(tke::validate_finite_coefficients(reinterpret_cast<const double *>(c), n_coefficients, who));
    OCN_REQUIRE(!std::isnan(c->maximum_tracer_diffusivity) && !std::isnan(c->maximum_tke_diffusivity) &&
                    !std::isnan(c->maximum_dissipation_diffusivity) && !std::isnan(c->maximum_viscosity),
                "%s: a maximum is a NaN", who);
    OCN_REQUIRE(std::isfinite(c->minimum_tke) && std::isfinite(c->negative_tke_damping_time_scale),
                "%s: minimum_tke and negative_tke_damping_time_scale must be finite", who);
    OCN_REQUIRE(c->stability_functions == OCN_STABILITY_VARIABLE || c->stability_functions == OCN_STABILITY_CONSTANT,
                "%s: unknown stability functions %d", who, c->stability_functions);
    return OCN_SUCCESS;
}

template <int MODE>
static void launch_columns(const ocn_grid *grid, const ocn_model_terms *terms, const ocn_tke_dissipation *closure, const Args &a, void *stream)
{
    if (closure->stability_functions == OCN_STABILITY_CONSTANT)
        hipLaunchKernelGGL((tke_dissipation_columns<MODE, OCN_STABILITY_CONSTANT>), tke::column_blocks(grid), dim3(64, 4, 1), 0,
                           as_stream(stream), to_dev(*grid), make_buoyancy(terms), *closure, a);
    else
        hipLaunchKernelGGL((tke_dissipation_columns<MODE, OCN_STABILITY_VARIABLE>), tke::column_blocks(grid), dim3(64, 4, 1), 0,
                           as_stream(stream), to_dev(*grid), make_buoyancy(terms), *closure, a);
}

}  // namespace tked

}  // namespace ocn

using namespace ocn;

extern "C" {

int ocn_compute_tke_dissipation_top_fluxes(const ocn_grid *grid, const ocn_tke_dissipation *closure, const ocn_bc *top_u, const ocn_bc *top_v,
                                           const double *znodes_c, const double *u, const double *v, const double *e, double *Qe, double *Qeps,
                                           void *stream)
{
    const char *who = "ocn_compute_tke_dissipation_top_fluxes";
    OCN_TRY(tked::validate_grid_and_closure(grid, closure, who));
    const ocn_bc *tops[2] = {top_u, top_v};
    const char *names[2] = {"u", "v"};
    OCN_TRY(tke::validate_top_fluxes(tops, names, 2, who));
    OCN_REQUIRE(znodes_c && u && v && e && Qe && Qeps, "%s: null pointer", who);
    OCN_REQUIRE(Qe != Qeps, "%s: Qe and Qeps must be two different planes", who);
    tked::PlaneArgs a{};
    a.zc = znodes_c; a.u = u; a.v = v; a.e = e; a.Qe = Qe; a.Qeps = Qeps;
    a.top_u = flux_or_default(top_u);
    a.top_v = flux_or_default(top_v);
    hipLaunchKernelGGL(tked::top_fluxes, tke::column_blocks(grid), dim3(64, 4, 1), 0, as_stream(stream), to_dev(*grid), *closure, a);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

int ocn_compute_tke_dissipation_diffusivities(const ocn_grid *grid, const ocn_model_terms *terms, const ocn_tke_dissipation *closure,
                                              const double *u, const double *v, const double *e, const double *eps, double *kappa_u,
                                              double *kappa_c, double *kappa_e, double *kappa_eps, void *stream)
{
    const char *who = "ocn_compute_tke_dissipation_diffusivities";
    OCN_TRY(tked::validate_grid_and_closure(grid, closure, who));
    OCN_TRY(validate_buoyancy_terms(terms, who));
    OCN_REQUIRE(u && v && e && eps && kappa_u && kappa_c && kappa_e && kappa_eps, "%s: null pointer", who);
    OCN_REQUIRE(kappa_u != kappa_c && kappa_u != kappa_e && kappa_u != kappa_eps && kappa_c != kappa_e && kappa_c != kappa_eps &&
                    kappa_e != kappa_eps,
                "%s: kappa_u, kappa_c, kappa_e and kappa_eps must be four different arrays", who);
    OCN_REQUIRE(e != eps, "%s: e and eps must be two different arrays", who);
    tked::Args a{};
    a.Lz = grid->Lz; a.u = u; a.v = v; a.e_in = e; a.eps_in = eps;
    a.kappa_u = kappa_u; a.kappa_c = kappa_c; a.kappa_e = kappa_e; a.kappa_eps = kappa_eps;
    tked::launch_columns<tked::MODE_DIFFUSIVITIES>(grid, terms, closure, a, stream);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

int ocn_tke_dissipation_substep(const ocn_grid *grid, const ocn_model_terms *terms, const ocn_tke_dissipation *closure, const double *u_next,
                                const double *v_next, const double *u_prev, const double *v_prev, double *e, double *eps,
                                const double *kappa_u, const double *kappa_c, double *kappa_e, double *kappa_eps, double *Le, double *Leps,
                                const double *Gn_e, double *Gm_e, const double *Gn_eps, double *Gm_eps, double *scratch, double dtau, double chi,
                                int32_t solve, void *stream)
{
    const char *who = "ocn_tke_dissipation_substep";
    OCN_TRY(tked::validate_grid_and_closure(grid, closure, who));
    OCN_TRY(validate_buoyancy_terms(terms, who));
    OCN_REQUIRE(u_next && v_next && u_prev && v_prev && e && eps && kappa_u && kappa_c && kappa_e && kappa_eps && Le && Leps && Gn_e && Gm_e &&
                    Gn_eps && Gm_eps,
                "%s: null pointer", who);
    OCN_REQUIRE(!solve || scratch, "%s: the solves need a scratch array of 2 Nx Ny Nz doubles", who);
    OCN_REQUIRE(kappa_e != kappa_eps && kappa_e != kappa_u && kappa_e != kappa_c && kappa_eps != kappa_u && kappa_eps != kappa_c,
                "%s: kappa_e and kappa_eps are written: they must differ from each other and from kappa_u and kappa_c", who);
    const double *cells[9] = {e, eps, Le, Leps, Gn_e, Gm_e, Gn_eps, Gm_eps, scratch};
    for (int p = 0; p < 9; ++p)
        for (int q = p + 1; q < 9; ++q)
            OCN_REQUIRE(cells[p] != cells[q], "%s: e, eps, Le, Leps, Gn_e, Gm_e, Gn_eps, Gm_eps and scratch must be different arrays", who);
    OCN_REQUIRE(terms->T != e && terms->S != e && terms->T != eps && terms->S != eps, "%s: e or eps is a buoyancy tracer", who);
    OCN_REQUIRE(std::isfinite(dtau) && dtau >= 0, "%s: dtau = %g must be finite and >= 0", who, dtau);
    OCN_REQUIRE(std::isfinite(chi), "%s: chi = %g must be finite", who, chi);
    tked::Args a{};
    a.Lz = grid->Lz; a.u = u_next; a.v = v_next; a.u_prev = u_prev; a.v_prev = v_prev; a.e = e; a.eps = eps;
    a.ku_in = kappa_u; a.kc_in = kappa_c; a.kappa_e = kappa_e; a.kappa_eps = kappa_eps; a.Le = Le; a.Leps = Leps;
    a.Gn_e = Gn_e; a.Gm_e = Gm_e; a.Gn_eps = Gn_eps; a.Gm_eps = Gm_eps;
    a.t_e = scratch;
    a.t_eps = scratch ? scratch + (size_t)grid->Nx * grid->Ny * grid->Nz : nullptr;
    a.dtau = dtau; a.chi = chi; a.solve = solve != 0;
    tked::launch_columns<tked::MODE_SUBSTEP>(grid, terms, closure, a, stream);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

}  // extern "C"
