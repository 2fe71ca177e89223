// catke.hip -- CATKEVerticalDiffusivity (turbulence_closure_implementations/TKEBasedVerticalDiffusivities/): the diffusivities κᵘ, κᶜ, κᵉ at
// (Center, Center, Face), the time-averaged surface buoyancy flux Jᵇ, the top flux of e and the substep of e with its implicit solve, on a
// (Periodic, Periodic, Bounded) grid.
//
//  catke_vertical_diffusivity.jl:253-325   compute_average_surface_buoyancy_flux!, compute_CATKE_diffusivities!, κuᶜᶜᶠ, κcᶜᶜᶠ, κeᶜᶜᶠ
//  catke_mixing_length.jl                  stable / convective length scales at ccf and ccc, step, scale, the three mixing lengths
//  catke_equation.jl:38-120                dissipation_length_scaleᶜᶜᶜ, dissipation_rate, top_tke_flux
//  TKEBasedVerticalDiffusivities.jl:57-156 shearᶜᶜᶠ, shearᶜᶜᶜ, Riᶜᶜᶠ, Riᶜᶜᶜ, ℑbzᵃᵃᶜ, explicit_buoyancy_flux, shear_production, mask_diffusivity
//  time_step_catke_equation.jl:78-173      substep_turbulent_kinetic_energy!
//  vertically_implicit_diffusion_solver.jl:55-110   the rows of the solve, with the linear coefficient in the diagonal
//
// Everything is column-local but the shear (u at i, i + 1; v at j, j + 1) and the shear production (κᵘ one column away).  One thread owns
// one (i, j) column and marches upwards, x fastest across the lanes (the shape of ri_based_diffusivity.hip).  An iteration computes the
// quantities of face k + 1 from planes k and k + 1 and then finishes cell k, whose two faces it now holds: N², the shear, w★ and e of the
// lower plane are carried in registers, so every input is read once per cell.  ℑbzᵃᵃᶜ (the mean of the two faces of a cell, a peripheral
// face replaced by the other) never uses a value of faces 1 and Nz + 1, so they are not computed; κ of face 1 is the 0 of mask_diffusivity
// and face Nz + 1 is not written (the reference's launch is over k = 1..Nz).  The substep reads e of the cells k - 1, k, k + 1 while it
// writes e of cell k (the reference's kernel does so between threads, a race there): here every read is of the e before the call.  Row
// k of the solve needs κᵉ of faces k, k + 1 and Le of cell k, all known when cell k is finished, so the forward elimination runs in the
// same march, the multipliers go to a scratch array and the backward sweep follows in the same thread: one launch, the bits of two.
//
// Strict build (no FMA contraction, IEEE division and square root), min / max / Bool products / cbrt of ocn_catke.h: bit-identical to
// tests/catke_numpy.py.  What is shared with the other vertical closures (ocn_buoyancy.h, ocn_tke_columns.h) and what is not: DESIGN.md §5.2s.
#include <cmath>
#include <cstddef>

#include "ocn_buoyancy.h"
#include "ocn_catke.h"
#include "ocn_ivd.h"
#include "ocn_tke_columns.h"

namespace ocn {

namespace catke {

using ivd::Spacings;
using tke::bz;

enum Mode { MODE_DIFFUSIVITIES = 0, MODE_SUBSTEP = 1 };

struct Args {
    const double *zf, *zc;
    double Lz;
    const double *u, *v;          // the current (next) velocities
    const double *u_prev, *v_prev;
    const double *e_in;           // MODE_DIFFUSIVITIES
    double *e;                    // MODE_SUBSTEP, in place
    const double *Jb;
    const double *ku_in, *kc_in;  // MODE_SUBSTEP: κᵘ, κᶜ of the last compute_CATKE_diffusivities!
    double *kappa_u, *kappa_c, *kappa_e;
    double *Le;
    const double *Gn;
    double *Gm, *t;
    double dtau, chi;
    int solve;
};

// step and scale (catke_mixing_length.jl:195-202); Ri = ±inf flows through as in Julia
__device__ __forceinline__ double scale(double Ri, double s_un, double s_lo, double s_hi, double c, double w)
{
    const double step = jmax(0.0, jmin(1.0, (Ri - c) / w));
    const double s_plus = s_lo + (s_hi - s_lo) * step;
    return bmul(s_un, Ri < 0) + bmul(s_plus, Ri >= 0);
}

// stable_length_scale (:58-88): depth and height are those of the face or of the centre, N² and w★ likewise
__device__ __forceinline__ double stable_length(const ocn_catke &cl, double depth, double height, double w, double N2)
{
    const double d = jmin(cl.C_s * depth, cl.C_b * height);
    const double N2p = clip(N2);
    const double lN = N2p == 0 ? INFINITY : w / sqrt(N2p);
    const double l = jmin(d, lN);
    return l != l ? d : l;
}

// convective_length_scale (:93-193); center: the operand order of the flux Richardson number at ccc (d S² w★, at ccf d w★ S²)
__device__ __forceinline__ double convective_length(const ocn_catke &cl, double Cc, double Ce, double w, double w3, double S2, double N2,
                                                    double N2_above, double Jb, double depth, bool center)
{
    const double Jbe = cl.minimum_convective_buoyancy_flux;
    double lc = Cc * w3 / (Jb + Jbe);
    lc = lc != lc ? 0.0 : lc;
    const double Rif = (center ? depth * S2 * w : depth * w * S2) / (Jb + Jbe);
    const double eps = 1 - cl.C_sp * Rif;
    lc = clip(eps * lc);
    const double le = Ce * Jb / (w * N2 + Jbe);
    const bool convecting = (Jb > Jbe) & (N2 < 0);
    const bool entraining = (Jb > Jbe) & (N2 > 0) & (N2_above < 0);
    const double l = convecting ? lc : (entraining ? le : 0.0);
    return l != l ? 0.0 : l;
}

// κ = min(ℓ w★, maximum) with ℓ = min(H, max(σ ℓ★, ℓʰ)) (catke_mixing_length.jl:218-277, catke_vertical_diffusivity.jl:297-325)
__device__ __forceinline__ double face_kappa(const ocn_catke &cl, double Cc, double Ce, double C_un, double C_lo, double C_hi, double maximum,
                                             double H, double w, double w3, double S2, double N2, double N2_above, double Ri, double Jb,
                                             double depth, double stable)
{
    double lh = convective_length(cl, Cc, Ce, w, w3, S2, N2, N2_above, Jb, depth, false);
    const double sigma = scale(Ri, C_un, C_lo, C_hi, cl.CRi_0, cl.CRi_delta);
    double ls = sigma * stable;
    lh = lh != lh ? 0.0 : lh;
    ls = ls != ls ? 0.0 : ls;
    const double l = jmin(H, jmax(ls, lh));
    return jmin(l * w, maximum);
}

// dissipation_length_scaleᶜᶜᶜ (catke_equation.jl:38-63) from the centre values
__device__ __forceinline__ double dissipation_length(const ocn_catke &cl, double H, double w, double S2, double N2, double N2_above, double Ri,
                                                     double Jb, double depth, double height)
{
    double lh = convective_length(cl, cl.C_c_D, cl.C_e_D, w, w * w * w, S2, N2, N2_above, Jb, depth, true);
    const double sigma = scale(Ri, cl.C_un_D, cl.C_lo_D, cl.C_hi_D, cl.CRi_0, cl.CRi_delta);
    double ls = stable_length(cl, depth, height, w, N2) / sigma;
    lh = lh != lh ? 0.0 : lh;
    ls = ls != ls ? 0.0 : ls;
    return jmin(H, jmax(ls, lh));
}

// what a cell needs of one of its faces
struct Face {
    double Ri;
    double du2[2], dv2[2];                  // (∂z u)² at i, i + 1 and (∂z v)² at j, j + 1, of the current velocities
    double wb;                              // buoyancy_fluxᶜᶜᶠ = -κᶜ N²
    double Pn[2], Pp[2], Qn[2], Qp[2];      // Δz_νₑ_az_bzᶠᶜᶠ(uⁿ, u⁺), (u⁺, u⁺) at i, i + 1; ...ᶜᶠᶠ(vⁿ, v⁺), (v⁺, v⁺) at j, j + 1
    double ke;                              // κᵉ (masked)
};

template <int MODE>
__global__ __launch_bounds__(256) void catke_columns(GridDev g, SurfaceBuoyancy b, ocn_catke cl, Args a)
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
    const double *__restrict__ un = a.u + at(Lu, i, j, 1), *__restrict__ vn = a.v + at(Lv, i, j, 1);
    const double *__restrict__ uo = MODE == MODE_SUBSTEP ? a.u_prev + at(Lu, i, j, 1) : nullptr;
    const double *__restrict__ vo = MODE == MODE_SUBSTEP ? a.v_prev + at(Lv, i, j, 1) : nullptr;
    const double Jb = a.Jb[(i - 1) + (long long)g.Nx * (j - 1)];
    const double H = a.Lz, ztop = uniform_load(a.zf, Nz), zbot = uniform_load(a.zf, 0);
    const double emin = cl.minimum_tke;
    auto zf = [&](int k) { return uniform_load(a.zf, k - 1); };
    auto zc = [&](int k) { return uniform_load(a.zc, k - 1); };

    // carried upwards: T, S of the upper plane of the highest face whose N² is known, N² of faces k and k + 1, e and w★ of cell k, the
    // velocities of plane k, the face k of the cell
    double T_up = Tp ? Tp[c3] : 0.0, S_up = Sp ? Sp[c3] : 0.0;
    double n2_lo = 0.0, n2_hi = dz_b(b, T_up, Tp ? Tp[0] : 0.0, S_up, Sp ? Sp[0] : 0.0, M.dzF(2));
    double e_lo = ep[0];
    double w_lo = sqrt(jmax(emin, e_lo));
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
    // the elimination: written out, not tke::eliminate of k-ϵ, which costs this kernel 2 %
    double beta = 0.0, up_prev = 0.0, prev = 0.0;
    const double tiny = 10 * 2.220446049250313e-16;  // 10 eps(Float64)
    const double ab_alpha = 1.5 + a.chi, ab_beta = 0.5 + a.chi;

    for (int k = 1; k <= Nz; ++k) {
        // N² of face k + 2 (the first top halo plane at k + 2 == Nz + 1)
        double n2_top = n2_hi;
        if (k + 2 <= Nz + 1) {
            const double T2 = Tp ? Tp[(k + 1) * c3] : 0.0, S2 = Sp ? Sp[(k + 1) * c3] : 0.0;
            n2_top = dz_b(b, T2, T_up, S2, S_up, M.dzF(k + 2));
            T_up = T2;
            S_up = S2;
        }
        // face k + 1, from planes k and k + 1
        double e_hi = e_lo, w_hi = w_lo;
        if (k + 1 <= Nz) {
            const int f = k + 1;
            const double dzf = M.dzF(f);
            const double a0 = un[k * u3], a1 = un[k * u3 + 1], b0 = vn[k * v3], b1 = vn[k * v3 + v2];
            const double du0 = (a0 - un0) / dzf, du1 = (a1 - un1) / dzf, dv0 = (b0 - vn0) / dzf, dv1 = (b1 - vn1) / dzf;
            hi.du2[0] = du0 * du0; hi.du2[1] = du1 * du1; hi.dv2[0] = dv0 * dv0; hi.dv2[1] = dv1 * dv1;
            const double S2 = 0.5 * (hi.du2[0] + hi.du2[1]) + 0.5 * (hi.dv2[0] + hi.dv2[1]);  // shearᶜᶜᶠ
            const double N2 = n2_hi;
            hi.Ri = N2 == 0 ? 0.0 : N2 / S2;  // Riᶜᶜᶠ
            e_hi = ep[k * c3];
            w_hi = sqrt(jmax(emin, e_hi));
            const double w = 0.5 * (w_lo + w_hi);                                      // ℑzᵃᵃᶠ(turbulent_velocityᶜᶜᶜ)
            const double w3 = 0.5 * (w_lo * w_lo * w_lo + w_hi * w_hi * w_hi);        // ℑzᵃᵃᶠ(three_halves_tkeᶜᶜᶜ)
            const double depth = clip(ztop - zf(f)), height = jmax(M.dzC(f - 1), zf(f) - zbot);
            const double stable = stable_length(cl, depth, height, w, N2);
            const long long o = of + k * f3;
            if (MODE == MODE_DIFFUSIVITIES) {
                a.kappa_u[o] = face_kappa(cl, cl.C_c_u, cl.C_e_u, cl.C_un_u, cl.C_lo_u, cl.C_hi_u, cl.maximum_viscosity, H, w, w3, S2, N2, n2_top,
                                          hi.Ri, Jb, depth, stable);
                a.kappa_c[o] = face_kappa(cl, cl.C_c_c, cl.C_e_c, cl.C_un_c, cl.C_lo_c, cl.C_hi_c, cl.maximum_tracer_diffusivity, H, w, w3, S2, N2,
                                          n2_top, hi.Ri, Jb, depth, stable);
            }
            hi.ke = face_kappa(cl, cl.C_c_e, cl.C_e_e, cl.C_un_e, cl.C_lo_e, cl.C_hi_e, cl.maximum_tke_diffusivity, H, w, w3, S2, N2, n2_top, hi.Ri,
                               Jb, depth, stable);
            a.kappa_e[o] = hi.ke;
            if (MODE == MODE_SUBSTEP) {
                hi.wb = -a.kc_in[o] * N2;
                const double *__restrict__ q = a.ku_in + o;
                const double kh = q[0];
                const double nx0 = 0.5 * (q[-1] + kh), nx1 = 0.5 * (kh + q[1]);      // ℑxᶠᵃᵃ(κᵘ) at i, i + 1
                const double ny0 = 0.5 * (q[-f2] + kh), ny1 = 0.5 * (kh + q[f2]);    // ℑyᵃᶠᵃ(κᵘ) at j, j + 1
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
            const double N2 = bzk(n2_lo, n2_hi);
            const double N2_above = bz(n2_hi, n2_top, k + 1 >= Nz + 1, k + 2 >= Nz + 1);  // ℑbzᵃᵃᶜ at k + 1: faces k + 1 and k + 2
            const double Ri = bzk(lo.Ri, hi.Ri);
            const double S2 = 0.5 * (bzk(lo.du2[0], hi.du2[0]) + bzk(lo.du2[1], hi.du2[1])) +
                              0.5 * (bzk(lo.dv2[0], hi.dv2[0]) + bzk(lo.dv2[1], hi.dv2[1]));  // shearᶜᶜᶜ
            const double ek = e_lo, w = w_lo, dzc = M.dzC(k);
            const double depth = clip(ztop - zc(k)), height = jmax(dzc / 2, zc(k) - zbot);
            const double lD = dissipation_length(cl, H, w, S2, N2, N2_above, Ri, Jb, depth, height);
            const double omega = ek < 0 ? 1 / cl.negative_tke_damping_time_scale : sqrt(fabs(ek)) / lD;  // dissipation_rate
            const double wb = bzk(lo.wb, hi.wb);  // explicit_buoyancy_flux
            const double wb_minus = jmin(0.0, wb), wb_plus = jmax(0.0, wb);
            const double wb_e = bmul(wb_minus / ek, ek > emin);
            const double div_Je = (k == 1 ? -1.0 : 0.0) * cl.C_W_eps * sqrt(clip(ek)) / dzc;  // the bottom cell
            const double L = wb_e - omega + div_Je;
            a.Le[oc + (k - 1) * c3] = L;
            const double Px0 = (bzk(lo.Pn[0], hi.Pn[0]) + bzk(lo.Pp[0], hi.Pp[0])) / (2 * dzc);
            const double Px1 = (bzk(lo.Pn[1], hi.Pn[1]) + bzk(lo.Pp[1], hi.Pp[1])) / (2 * dzc);
            const double Py0 = (bzk(lo.Qn[0], hi.Qn[0]) + bzk(lo.Qp[0], hi.Qp[0])) / (2 * dzc);
            const double Py1 = (bzk(lo.Qn[1], hi.Qn[1]) + bzk(lo.Qp[1], hi.Qp[1])) / (2 * dzc);
            const double P = 0.5 * (Px0 + Px1) + 0.5 * (Py0 + Py1);  // shear_production
            const long long og = oc + (k - 1) * c3;
            const double fast = P + wb_plus;                          // (dissipation is implicit: - 0)
            const double total = a.Gn[og] + fast;
            const double e_new = ek + a.dtau * (ab_alpha * total - ab_beta * a.Gm[og]);
            a.Gm[og] = total;
            if (!a.solve) {
                a.e[og] = e_new;
            } else {
                // row k of (1 - Δτ ∂z κᵉ ∂z - Δτ Le) e = e (vertical_diffusivity.hip implicit_step_fields, plus the linear coefficient)
                const double ke_lo = lo.ke, ke_hi = hi.ke;
                const double low = k == 1 ? 0.0 : -a.dtau * ke_lo / (dzc * M.dzF(k));  // ivd_lower_diagonal(k - 1)
                const double du = -a.dtau * ke_hi / (dzc * M.dzF(k + 1));              // ivd_upper_diagonal(k)
                const double upk = k > Nz - 1 ? 0.0 : du;
                const double diag = 1.0 - a.dtau * L - upk - low;
                if (k == 1) {
                    beta = diag;
                    prev = e_new / beta;
                } else {
                    const double t = up_prev / beta;
                    beta = diag - low * t;
                    a.t[(i - 1) + (long long)g.Nx * (j - 1) + (long long)g.Nx * g.Ny * (k - 1)] = t;
                    const double star = (e_new - low * prev) / beta;
                    prev = fabs(beta) > tiny ? star : e_new;
                }
                a.e[og] = prev;
                up_prev = upk;
            }
        }
        lo = hi;
        n2_lo = n2_hi;
        n2_hi = n2_top;
        e_lo = e_hi;
        w_lo = w_hi;
    }
    if (MODE == MODE_SUBSTEP && a.solve) {  // backward sweep: e[k] -= t[k + 1] e[k + 1]
        const long long t3 = (long long)g.Nx * g.Ny;
        const double *tp = a.t + (i - 1) + (long long)g.Nx * (j - 1);
        for (int k = Nz - 1; k >= 1; --k) {
            const long long og = oc + (k - 1) * c3;
            prev = a.e[og] - tp[k * t3] * prev;
            a.e[og] = prev;
        }
    }
}

// the two plane kernels: Jᵇ (compute_average_surface_buoyancy_flux!) and the top flux of e (top_tke_flux)
struct PlaneArgs {
    const double *zf, *zc;
    double Lz;
    const double *u, *v, *e;
    double *Jb;
    double dt;
    ZBc top_u, top_v;
    double *Qe;
};

__global__ __launch_bounds__(256) void surface_buoyancy_flux(GridDev g, SurfaceBuoyancy b, ocn_catke cl, PlaneArgs a)
{
    const int i = 1 + blockIdx.x * 64 + threadIdx.x, j = 1 + blockIdx.y * 4 + threadIdx.y;
    if (i > g.Nx || j > g.Ny) return;
    const int Nz = g.Nz;
    const Spacings M = ivd::spacings_of(g);
    const Lay Lc = make_lay(g, OCN_LOC_CCC), Lu = make_lay(g, OCN_LOC_FCC), Lv = make_lay(g, OCN_LOC_CFC);
    const long long oc = at(Lc, i, j, Nz), ou = at(Lu, i, j, Nz), ov = at(Lv, i, j, Nz);
    auto T = [&](int dk) { return b.T ? b.T[oc + dk * Lc.s3] : 0.0; };
    auto S = [&](int dk) { return b.S ? b.S[oc + dk * Lc.s3] : 0.0; };
    // face Nz and, for N²_above, face Nz + 1; ℑbzᵃᵃᶜ at k = Nz and k = Nz + 1 takes the lower face twice
    const double dzf = M.dzF(Nz);
    const double n2 = dz_b(b, T(0), T(-1), S(0), S(-1), dzf), n2_above = dz_b(b, T(1), T(0), S(1), S(0), M.dzF(Nz + 1));
    const double du0 = (a.u[ou] - a.u[ou - Lu.s3]) / dzf, du1 = (a.u[ou + 1] - a.u[ou + 1 - Lu.s3]) / dzf;
    const double dv0 = (a.v[ov] - a.v[ov - Lv.s3]) / dzf, dv1 = (a.v[ov + Lv.s2] - a.v[ov + Lv.s2 - Lv.s3]) / dzf;
    const double du20 = du0 * du0, du21 = du1 * du1, dv20 = dv0 * dv0, dv21 = dv1 * dv1;
    const double S2f = 0.5 * (du20 + du21) + 0.5 * (dv20 + dv21);
    const double Rif = n2 == 0 ? 0.0 : n2 / S2f;
    auto twice = [](double x) { return (x + x) / 2; };
    const double S2 = 0.5 * (twice(du20) + twice(du21)) + 0.5 * (twice(dv20) + twice(dv21));
    const double w = sqrt(jmax(cl.minimum_tke, a.e[oc]));
    const double ztop = uniform_load(a.zf, Nz), zbot = uniform_load(a.zf, 0), z = uniform_load(a.zc, Nz - 1);
    const double depth = clip(ztop - z), height = jmax(M.dzC(Nz) / 2, z - zbot);
    const long long op = (i - 1) + (long long)g.Nx * (j - 1);
    const double Jb = a.Jb[op];
    const double lD = dissipation_length(cl, a.Lz, w, S2, twice(n2), twice(n2_above), twice(Rif), Jb, depth, height);
    const double J_star = top_buoyancy_flux(b, i, j, g.Nx, T(0), S(0));
    const double J_plus = jmax(jmax(cl.minimum_convective_buoyancy_flux, Jb), J_star);
    const double t_star = cbrt_newton(lD * lD / J_plus);
    const double eps = a.dt / t_star;
    a.Jb[op] = (Jb + eps * J_star) / (1 + eps);
}

__global__ __launch_bounds__(256) void top_tke_flux(GridDev g, SurfaceBuoyancy b, ocn_catke cl, PlaneArgs a)
{
    const int i = 1 + blockIdx.x * 64 + threadIdx.x, j = 1 + blockIdx.y * 4 + threadIdx.y;
    if (i > g.Nx || j > g.Ny) return;
    const int Nz = g.Nz;
    const Spacings M = ivd::spacings_of(g);
    const Lay Lc = make_lay(g, OCN_LOC_CCC), Lu = make_lay(g, OCN_LOC_FCC), Lv = make_lay(g, OCN_LOC_CFC);
    const long long oc = at(Lc, i, j, Nz);
    const double tau_x = a.top_u.kind == OCN_BC_FLUX ? bc_condition(a.top_u, i, j, g.Nx, a.u[at(Lu, i, j, Nz)]) : 0.0;
    const double tau_y = a.top_v.kind == OCN_BC_FLUX ? bc_condition(a.top_v, i, j, g.Nx, a.v[at(Lv, i, j, Nz)]) : 0.0;
    const double u_star = sqrt(sqrt(tau_x * tau_x + tau_y * tau_y));  // friction_velocity
    const double J_star = top_buoyancy_flux(b, i, j, g.Nx, b.T ? b.T[oc] : 0.0, b.S ? b.S[oc] : 0.0);
    const double w_delta3 = clip(J_star) * M.dzC(Nz);                  // top_convective_turbulent_velocity_cubed
    a.Qe[(i - 1) + (long long)g.Nx * (j - 1)] = -cl.C_W_ustar * (u_star * u_star * u_star) - cl.C_W_wdelta * w_delta3;
}

// ---- argument checks: nothing here touches a device -----------------------------------------------------------------------------------
static int validate_grid_and_closure(const ocn_grid *grid, const ocn_model_terms *terms, const ocn_catke *c, const char *who)
{
    OCN_TRY(tke::validate_tke_grid(grid, who));
    OCN_TRY(validate_buoyancy_terms(terms, who));
    OCN_REQUIRE(c, "%s: null closure", who);
    // every member in front of the three maxima is a coefficient (the struct holds doubles only)
    constexpr size_t n_coefficients = offsetof(ocn_catke, maximum_tracer_diffusivity) / sizeof(double);
    static_assert(offsetof(ocn_catke, C_s) == 0 && sizeof(ocn_catke) % sizeof(double) == 0, "ocn_catke: doubles only, coefficients first");
    OCN_TRY(tke::validate_finite_coefficients(reinterpret_cast<const double *>(c), n_coefficients, who));
    OCN_REQUIRE(!std::isnan(c->maximum_tracer_diffusivity) && !std::isnan(c->maximum_tke_diffusivity) && !std::isnan(c->maximum_viscosity),
                "%s: a maximum is a NaN", who);
    OCN_REQUIRE(std::isfinite(c->minimum_tke) && std::isfinite(c->minimum_convective_buoyancy_flux) &&
                    std::isfinite(c->negative_tke_damping_time_scale),
                "%s: minimum_tke, minimum_convective_buoyancy_flux and negative_tke_damping_time_scale must be finite", who);
    return OCN_SUCCESS;
}

}  // namespace catke

}  // namespace ocn

using namespace ocn;

extern "C" {

int ocn_catke_host_cbrt(int64_t n, const double *x, double *out)
{
    OCN_REQUIRE(n >= 0 && (n == 0 || (x && out)), "ocn_catke_host_cbrt: null array or negative length");
    for (int64_t q = 0; q < n; ++q) out[q] = catke::cbrt_newton(x[q]);
    return OCN_SUCCESS;
}

int ocn_compute_catke_surface_buoyancy_flux(const ocn_grid *grid, const ocn_model_terms *terms, const ocn_catke *closure, const ocn_bc *top_T,
                                            const ocn_bc *top_S, const double *znodes_f, const double *znodes_c, const double *u,
                                            const double *v, const double *e, double *Jb, double dt, void *stream)
{
    const char *who = "ocn_compute_catke_surface_buoyancy_flux";
    OCN_TRY(catke::validate_grid_and_closure(grid, terms, closure, who));
    const ocn_bc *tops[2] = {top_T, top_S};
    const char *names[2] = {"the T (or b) tracer", "the S tracer"};
    OCN_TRY(tke::validate_top_fluxes(tops, names, 2, who));
    OCN_REQUIRE(znodes_f && znodes_c && u && v && e && Jb, "%s: null pointer", who);
    OCN_REQUIRE(std::isfinite(dt) && dt >= 0, "%s: dt = %g must be finite and >= 0", who, dt);
    catke::PlaneArgs a{};
    a.zf = znodes_f; a.zc = znodes_c; a.Lz = grid->Lz; a.u = u; a.v = v; a.e = e; a.Jb = Jb; a.dt = dt;
    hipLaunchKernelGGL(catke::surface_buoyancy_flux, tke::column_blocks(grid), dim3(64, 4, 1), 0, as_stream(stream), to_dev(*grid),
                       make_surface_buoyancy(terms, top_T, top_S), *closure, a);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

int ocn_compute_catke_top_tke_flux(const ocn_grid *grid, const ocn_model_terms *terms, const ocn_catke *closure, const ocn_bc *top_u,
                                   const ocn_bc *top_v, const ocn_bc *top_T, const ocn_bc *top_S, const double *u, const double *v, double *Qe,
                                   void *stream)
{
    const char *who = "ocn_compute_catke_top_tke_flux";
    OCN_TRY(catke::validate_grid_and_closure(grid, terms, closure, who));
    const ocn_bc *tops[4] = {top_u, top_v, top_T, top_S};
    const char *names[4] = {"u", "v", "the T (or b) tracer", "the S tracer"};
    OCN_TRY(tke::validate_top_fluxes(tops, names, 4, who));
    OCN_REQUIRE(u && v && Qe, "%s: null pointer", who);
    catke::PlaneArgs a{};
    a.u = u; a.v = v; a.Qe = Qe; a.Lz = grid->Lz;
    a.top_u = flux_or_default(top_u);
    a.top_v = flux_or_default(top_v);
    hipLaunchKernelGGL(catke::top_tke_flux, tke::column_blocks(grid), dim3(64, 4, 1), 0, as_stream(stream), to_dev(*grid),
                       make_surface_buoyancy(terms, top_T, top_S), *closure, a);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

int ocn_compute_catke_diffusivities(const ocn_grid *grid, const ocn_model_terms *terms, const ocn_catke *closure, const double *znodes_f,
                                    const double *znodes_c, const double *u, const double *v, const double *e, const double *Jb,
                                    double *kappa_u, double *kappa_c, double *kappa_e, void *stream)
{
    const char *who = "ocn_compute_catke_diffusivities";
    OCN_TRY(catke::validate_grid_and_closure(grid, terms, closure, who));
    OCN_REQUIRE(znodes_f && znodes_c && u && v && e && Jb && kappa_u && kappa_c && kappa_e, "%s: null pointer", who);
    OCN_REQUIRE(kappa_u != kappa_c && kappa_u != kappa_e && kappa_c != kappa_e, "%s: kappa_u, kappa_c and kappa_e must be three different arrays",
                who);
    catke::Args a{};
    a.zf = znodes_f; a.zc = znodes_c; a.Lz = grid->Lz; a.u = u; a.v = v; a.e_in = e; a.Jb = Jb;
    a.kappa_u = kappa_u; a.kappa_c = kappa_c; a.kappa_e = kappa_e;
    hipLaunchKernelGGL(catke::catke_columns<catke::MODE_DIFFUSIVITIES>, tke::column_blocks(grid), dim3(64, 4, 1), 0, as_stream(stream),
                       to_dev(*grid), make_surface_buoyancy(terms, nullptr, nullptr), *closure, a);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

int ocn_catke_substep_tke(const ocn_grid *grid, const ocn_model_terms *terms, const ocn_catke *closure, const double *znodes_f,
                          const double *znodes_c, const double *u_next, const double *v_next, const double *u_prev, const double *v_prev,
                          double *e, const double *Jb, const double *kappa_u, const double *kappa_c, double *kappa_e, double *Le,
                          const double *Gn_e, double *Gm_e, double *scratch, double dtau, double chi, int32_t solve, void *stream)
{
    const char *who = "ocn_catke_substep_tke";
    OCN_TRY(catke::validate_grid_and_closure(grid, terms, closure, who));
    OCN_REQUIRE(znodes_f && znodes_c && u_next && v_next && u_prev && v_prev && e && Jb && kappa_u && kappa_c && kappa_e && Le && Gn_e && Gm_e,
                "%s: null pointer", who);
    OCN_REQUIRE(!solve || scratch, "%s: the solve needs a scratch array of Nx Ny Nz doubles", who);
    OCN_REQUIRE(kappa_e != kappa_u && kappa_e != kappa_c, "%s: kappa_e is written: it must not be kappa_u or kappa_c", who);
    OCN_REQUIRE(e != Le && e != Gn_e && e != Gm_e && Le != Gn_e && Le != Gm_e && Gn_e != Gm_e && (const double *)scratch != e,
                "%s: e, Le, Gn_e, Gm_e and scratch must be different arrays", who);
    OCN_REQUIRE(terms->T != e && terms->S != e, "%s: e is a buoyancy tracer", who);
    OCN_REQUIRE(std::isfinite(dtau) && dtau >= 0, "%s: dtau = %g must be finite and >= 0", who, dtau);
    OCN_REQUIRE(std::isfinite(chi), "%s: chi = %g must be finite", who, chi);
    catke::Args a{};
    a.zf = znodes_f; a.zc = znodes_c; a.Lz = grid->Lz; a.u = u_next; a.v = v_next; a.u_prev = u_prev; a.v_prev = v_prev; a.e = e; a.Jb = Jb;
    a.ku_in = kappa_u; a.kc_in = kappa_c; a.kappa_e = kappa_e; a.Le = Le; a.Gn = Gn_e; a.Gm = Gm_e; a.t = scratch;
    a.dtau = dtau; a.chi = chi; a.solve = solve != 0;
    hipLaunchKernelGGL(catke::catke_columns<catke::MODE_SUBSTEP>, tke::column_blocks(grid), dim3(64, 4, 1), 0, as_stream(stream),
                       to_dev(*grid), make_surface_buoyancy(terms, nullptr, nullptr), *closure, a);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

}  // extern "C"
