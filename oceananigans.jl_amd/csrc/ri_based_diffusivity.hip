// ri_based_diffusivity.hip -- RiBasedVerticalDiffusivity (turbulence_closure_implementations/ri_based_vertical_diffusivity.jl): the
// Richardson number and the time-averaged κᶜ, κᵘ fields at (Center, Center, Face) on a z-Bounded grid.  Their closure term and their implicit
// step are the field-valued kernels of vertical_diffusivity.hip.
//
//  compute_ri_number! (:245-267) over i = 1..Nx, j = 1..Ny, k = 1..Nz (the :xyz launch: face Nz+1 and the halos are not written)
//       S² = ℑxᶜᵃᵃ((∂zᶠᶜᶠ u)²) + ℑyᵃᶜᵃ((∂zᶜᶠᶠ v)²),   N² = ∂z_b,   Ri = N² <= 0 ? 0 : N² / S²        (+inf where the water is at rest and stable)
//  compute_ri_based_diffusivities! (:277-341) over the same cells, from an Ri whose x / y halos are filled:
//       Jᵇ = top_buoyancy_flux (seawater_buoyancy.jl:234-246, buoyancy_tracer.jl:18),  convecting = N² < 0,
//       entraining = (N² > N²ᵉⁿ) & (N²(k+1) < 0) & (Jᵇ > 0),  κᶜ⁺ = (κᶜᵃ|0 + (Cᵉⁿ Jᵇ / N²)|0) + κ₀ τ(Ri),  κᵘ⁺ = ν₀ τ(Ri),  min with the maxima,
//       0 on the periphery (face 1; no face 1..Nz of a rectilinear grid is inactive),  κ <- (Cᵃᵛ κ + κ⁺) / (1 + Cᵃᵛ) in place;
//       Ri through FivePointHorizontalFilter = ℑxyᶜᶜᵃ(ℑxyᶠᶠᵃ Ri) (:56) when asked.
//
// One thread owns one (i, j) column and marches upwards, x fastest across the lanes (the shape of the implicit step): N²(k+1) of one face is
// N² of the next, and ∂z of u, v, T, S at face k needs plane k - 1, so a thread keeps the lower plane and N² in registers and every plane of
// u, v, T, S is fetched once (the second x / y operand of the shear is the neighbour lane's / row's line: L1 / L2).  Without the filter Ri is
// only needed locally: MODE_FUSED computes it, stores it and goes on to the diffusivities: 72 B per cell (u, v, T, S read, κᶜ, κᵘ read and
// written, Ri written) in one launch.  All three modes are one template and call the same inline functions: the fused launch equals the two
// launches bit for bit.  Strict build (no FMA contraction, IEEE division), no math library (ocn_taper.h): bit-identical to
// tests/ri_based_numpy.py.  The buoyancy is that of ocn_buoyancy.h.
#include "ocn_buoyancy.h"
#include "ocn_ivd.h"
#include "ocn_taper.h"

namespace ocn {

namespace rbd {

using ivd::Spacings;

enum Mode { MODE_RI = 0, MODE_DIFFUSIVITIES = 1, MODE_FUSED = 2 };

struct Args {
    const double *u, *v;  // MODE_RI, MODE_FUSED
    const double *ri_in;  // MODE_DIFFUSIVITIES
    double *ri_out;       // MODE_RI, MODE_FUSED
    double *kappa_c, *kappa_u;
};

// Julia's min(a, m) for a maximum m that is no NaN: a NaN propagates
__device__ __forceinline__ double min_with(double a, double m) { return a != a ? a : (a < m ? a : m); }

template <int MODE>
__global__ __launch_bounds__(256) void ri_based_columns(GridDev g, SurfaceBuoyancy b, ocn_ri_based cl, Args a)
{
    const int i = 1 + blockIdx.x * 64 + threadIdx.x, j = 1 + blockIdx.y * 4 + threadIdx.y;
    if (i > g.Nx || j > g.Ny) return;
    const int Nz = g.Nz;
    const Spacings M = ivd::spacings_of(g);
    const Lay Lc = make_lay(g, OCN_LOC_CCC), Lu = make_lay(g, OCN_LOC_FCC), Lv = make_lay(g, OCN_LOC_CFC), Lf = make_lay(g, OCN_LOC_CCF);
    const double *__restrict__ Tp = b.T ? b.T + at(Lc, i, j, 0) : nullptr;  // plane k at Tp[k s3]
    const double *__restrict__ Sp = b.S ? b.S + at(Lc, i, j, 0) : nullptr;
    const long long c3 = Lc.s3, u3 = Lu.s3, v3 = Lv.s3, f3 = Lf.s3, v2 = Lv.s2, f2 = Lf.s2;
    const long long of = at(Lf, i, j, 1);
    // carried from face to face: T, S of plane k, N² of face k, and the lower plane (k - 1) of u and v
    double T1 = Tp ? Tp[c3] : 0.0, S1 = Sp ? Sp[c3] : 0.0;
    double N2 = dz_b(b, T1, Tp ? Tp[0] : 0.0, S1, Sp ? Sp[0] : 0.0, M.dzF(1));
    const double *up = nullptr, *vp = nullptr;
    double u0 = 0.0, u1 = 0.0, v0 = 0.0, v1 = 0.0;
    if (MODE != MODE_DIFFUSIVITIES) {
        up = a.u + at(Lu, i, j, 0);
        vp = a.v + at(Lv, i, j, 0);
        u0 = up[0]; u1 = up[1]; v0 = vp[0]; v1 = vp[v2];
    }
    double Jb = 0.0;
    if (MODE != MODE_RI && b.kind != OCN_BUOYANCY_NONE) {  // top_buoyancy_flux of ocn_buoyancy.h, the top cell read only under a Flux condition
        const double JT = (Tp && b.top_T.kind == OCN_BC_FLUX) ? bc_condition(b.top_T, i, j, g.Nx, Tp[Nz * c3]) : 0.0;
        if (b.kind == OCN_BUOYANCY_TRACER) {
            Jb = JT;
        } else {
            const double JS = (Sp && b.top_S.kind == OCN_BC_FLUX) ? bc_condition(b.top_S, i, j, g.Nx, Sp[Nz * c3]) : 0.0;
            Jb = b.g * (b.alpha * JT - b.beta * JS);
        }
    }
    for (int k = 1; k <= Nz; ++k) {
        // N² of the face above, from planes k and k + 1 (the top halo at k == Nz)
        const double T2 = Tp ? Tp[(k + 1) * c3] : 0.0, S2 = Sp ? Sp[(k + 1) * c3] : 0.0;
        const double N2_above = dz_b(b, T2, T1, S2, S1, M.dzF(k + 1));
        double Ri;
        if (MODE != MODE_DIFFUSIVITIES) {
            const double dzf = M.dzF(k);
            const double un0 = up[k * u3], un1 = up[k * u3 + 1], vn0 = vp[k * v3], vn1 = vp[k * v3 + v2];
            const double du0 = (un0 - u0) / dzf, du1 = (un1 - u1) / dzf, dv0 = (vn0 - v0) / dzf, dv1 = (vn1 - v1) / dzf;
            const double dzu2 = 0.5 * (du0 * du0 + du1 * du1);  // ℑxᶜᵃᵃ(ϕ², ∂zᶠᶜᶠ, u)
            const double dzv2 = 0.5 * (dv0 * dv0 + dv1 * dv1);  // ℑyᵃᶜᵃ(ϕ², ∂zᶜᶠᶠ, v)
            const double shear2 = dzu2 + dzv2;
            Ri = N2 <= 0 ? 0.0 : N2 / shear2;
            a.ri_out[of + (k - 1) * f3] = Ri;
            u0 = un0; u1 = un1; v0 = vn0; v1 = vn1;
        } else {
            const double *__restrict__ r = a.ri_in + of + (k - 1) * f3;
            if (cl.horizontal_filter == OCN_RI_FILTER_FIVE_POINT) {
                // ℑxyᶠᶠᵃ at the four corners of the cell: ℑyᵃᶠᵃ(ℑxᶠᵃᵃ Ri), then ℑxyᶜᶜᵃ = ℑyᵃᶜᵃ(ℑxᶜᵃᵃ ·)
                auto ff = [&](int di, int dj) {
                    const double *q = r + di + dj * f2;
                    return 0.5 * (0.5 * (q[-1 - f2] + q[-f2]) + 0.5 * (q[-1] + q[0]));
                };
                Ri = 0.5 * (0.5 * (ff(0, 0) + ff(1, 0)) + 0.5 * (ff(0, 1) + ff(1, 1)));
            } else {
                Ri = r[0];
            }
        }
        if (MODE != MODE_RI) {
            const bool convecting = N2 < 0;
            const bool entraining = (N2 > cl.minimum_entrainment_buoyancy_gradient) & (N2_above < 0) & (Jb > 0);
            const double k_ca = convecting ? cl.kappa_ca : 0.0;
            const double k_en = entraining ? cl.C_en * Jb / N2 : 0.0;
            const double tau = taper::apply(cl.tapering, Ri, cl.Ri0, cl.Ri_delta);
            double kc_new = min_with(k_ca + k_en + cl.kappa0 * tau, cl.maximum_diffusivity);
            double ku_new = min_with(cl.nu0 * tau, cl.maximum_viscosity);
            if (k == 1) kc_new = ku_new = 0.0;  // peripheral_node(i, j, k, grid, c, c, f)
            const long long o = of + (k - 1) * f3;
            a.kappa_c[o] = (cl.C_av * a.kappa_c[o] + kc_new) / (1 + cl.C_av);
            a.kappa_u[o] = (cl.C_av * a.kappa_u[o] + ku_new) / (1 + cl.C_av);
        }
        T1 = T2; S1 = S2;
        N2 = N2_above;
    }
}

}  // namespace rbd

// the callers have validated the grid (z Bounded, x and y not Flat, halos >= 1), the closure and the pointers.
// mode: 0 Ri alone, 1 the diffusivities from a stored Ri, 2 both in one launch (no filter)
int launch_ri_based(int mode, const ocn_grid *grid, const ocn_model_terms *terms, const ocn_ri_based *closure, const ocn_bc *top_T,
                    const ocn_bc *top_S, const double *u, const double *v, const double *ri_in, double *ri_out, double *kappa_c,
                    double *kappa_u, hipStream_t stream)
{
    const SurfaceBuoyancy b = make_surface_buoyancy(terms, top_T, top_S);
    const rbd::Args a{u, v, ri_in, ri_out, kappa_c, kappa_u};
    const ocn_ri_based cl = closure ? *closure : ocn_ri_based{};
    const GridDev gd = to_dev(*grid);
    const dim3 block(64, 4, 1), blocks((grid->Nx + 63) / 64, (grid->Ny + 3) / 4, 1);
    switch (mode) {
    case rbd::MODE_RI: hipLaunchKernelGGL(rbd::ri_based_columns<rbd::MODE_RI>, blocks, block, 0, stream, gd, b, cl, a); break;
    case rbd::MODE_DIFFUSIVITIES: hipLaunchKernelGGL(rbd::ri_based_columns<rbd::MODE_DIFFUSIVITIES>, blocks, block, 0, stream, gd, b, cl, a); break;
    default: hipLaunchKernelGGL(rbd::ri_based_columns<rbd::MODE_FUSED>, blocks, block, 0, stream, gd, b, cl, a); break;
    }
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

// the tapering functions on the host: the same inline functions, the same strict build
void ri_taper_host(int kind, long long n, const double *x, double x0, double delta, double *out)
{
    for (long long q = 0; q < n; ++q) out[q] = taper::apply(kind, x[q], x0, delta);
}

}  // namespace ocn
