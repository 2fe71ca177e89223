// vector_invariant_weno.hip -- Gu = -U_dot_∇u, Gv = -U_dot_∇v of the upwinding vector-invariant schemes (VectorInvariant with
// WENO(order=5) sub-schemes, WENOVectorInvariant(order=5)) on a (Periodic, Periodic, Bounded) grid with regular x and y:
//   U_dot_∇u = (horizontal_advection_U + vertical_advection_U) + bernoulli_head_U       (vector_invariant_advection.jl:269-275)
//   hadv_U = -v̂ ζᴿ,  v̂ = ℑxᶠᵃᵃ ℑyᵃᶜᵃ(Δx v) / Δx,  ζᴿ = the biased reconstruction in y of ζ₃ᶠᶠᶜ over faces j-2 .. j+3, bias(v̂);
//            weights from ζ (DefaultStencil) or from ℑyᵃᶠᵃ u and ℑxᶠᵃᵃ v, β = (βᵤ + βᵥ) / 2 (VelocityStencil)   (:367-385, weno_interpolants.jl:350-363)
//   vadv_U = 1 / V (û (δvˢ + δuᴿ) + δz F_Wu),  û = u,  δvˢ = Centered(order=4) in x of δy(Ay v),  δuᴿ = the biased reconstruction in x
//            of δx(Ax u) over centres i-3 .. i+2, weights from δx(Ax u) + δy(Ay v);  F_Wu = advective_momentum_flux_Wu of WENO(order=5)
//            with its order reduction along the Bounded z                     (:325-339, vector_invariant_self_upwinding.jl:5-42)
//   bern_U = (δKuᴿ + δKvˢ) / Δx,  δKuᴿ = the biased reconstruction in x of δx(u² / 2), weights from ℑxᶜᵃᵃ u,  δKvˢ = Centered(order=4) in y
//            of δxᶠᶠᶜ(v² / 2)                                                                                       (:48-83)
// and the mirror image for v.  A sub-scheme left at its conserving default keeps the arithmetic of vector_invariant_kernel (kernels.hip)
// for its term; the three choices and the vorticity stencil are template parameters.  eta != NULL: - g ∇η is subtracted in the same pass.
//
// A workgroup of 256 threads owns a TX x TY = 32 x 8 tile of the xy plane and marches PLANES planes.  Per plane, through LDS (every array
// is the tile with a ring of 3, (TX + 6) x (TY + 6) points, point (a, b) <-> cell (i0 - 3 + a, j0 - 3 + b)):
//   u, v                       from global memory through registers (loaded a plane ahead)
//   ζ, ℑy u, ℑx v              at (f, f)        what the vorticity reconstructions read
//   δx(Ax u), δy(Ay v), sum    at (c, c)        what the divergence reconstructions read
//   δx(u²/2), ℑx u             at (c, c) of x;  δy(v²/2), ℑy v at (c, c) of y;  δxᶠᶠᶜ(v²/2), δyᶠᶠᶜ(u²/2) at (f, f)
// each derived once per tile point (only the arrays the template's scheme reads exist); then every thread reconstructs for its own cell.
// The vertical face fluxes read w (x or y stencil) and u, v (z stencil) from global memory; the flux through the top face of plane k is
// kept in registers as the flux through the bottom face of plane k + 1.
//
// Reach of the reads: 3 cells in x and in y (u, v; 2 for w), for every scheme combination.  Along z one plane below k = 1 and above k = Nz:
// the order reduction of bias_interp<OCN_BOUNDED, false> confines the stencil of face k to planes 1 .. Nz but for the first-order faces
// 1, 2, Nz, Nz + 1, which read planes 0 and Nz + 1 (as the conserving form does); a stencil value is loaded only in the branch that uses it.
//
// One arithmetic variant, the reference's evaluation order (OCN_STRICT = 1, no FMA contraction, IEEE division): bit-identical to
// tests/vector_invariant_weno_numpy.py.  MATH_FAST models call the same kernel.
#define OCN_STRICT 1
#include "ocn_weno.h"

#include "ocn_internal.h"

namespace ocn {

namespace viw {

using namespace ocn_strict;

constexpr int TX = 32, TY = 8, NT = 256, R = 3;
constexpr int EX = TX + 2 * R, EY = TY + 2 * R, NP = EX * EY;
constexpr int PER_THREAD = (NP + NT - 1) / NT;
constexpr int PLANES = 8;  // planes marched by one workgroup

template <bool VORT, bool VERT, bool KE, bool VEL>
struct Arrays {
    static constexpr int U = 0, V = 1, ZETA = 2;
    static constexpr int UFF = 3, VFF = 4;  // VORT && VEL
    static constexpr int N0 = 3 + ((VORT && VEL) ? 2 : 0);
    static constexpr int DXU = N0, DYV = N0 + 1, DIV = N0 + 2;  // VERT
    static constexpr int N1 = N0 + (VERT ? 3 : 0);
    static constexpr int DKU = N1, SU = N1 + 1, DKV = N1 + 2, SV = N1 + 3, CXV = N1 + 4, CYU = N1 + 5;  // KE
    static constexpr int COUNT = N1 + (KE ? 6 : 0);
};

template <bool VORT, bool VERT, bool KE, bool VEL>
__global__ __launch_bounds__(NT) void vector_invariant_weno_kernel(GridDev g, const double *__restrict__ u, const double *__restrict__ v,
                                                                   const double *__restrict__ w, double *__restrict__ Gu,
                                                                   double *__restrict__ Gv, const double *__restrict__ eta, double grav)
{
    using A = Arrays<VORT, VERT, KE, VEL>;
    __shared__ double lds[A::COUNT][NP];

    const int tid = threadIdx.x;
    const int i0 = 1 + blockIdx.x * TX, j0 = 1 + blockIdx.y * TY;  // first interior cell of the tile
    const int k0 = 1 + blockIdx.z * PLANES, k1 = min(k0 + PLANES - 1, g.Nz);
    const Metrics M = make_metrics(g);
    const Lay L = make_lay(g, OCN_LOC_CCC);  // Periodic x and y: u, v and w share strides and offset (w only has one more plane)
    const long long s2 = L.s2, s3 = L.s3;
    const double dx = g.dx, dy = g.dy, Az = dx * dy;
    const int Nz = g.Nz;
    const double *fld[2] = {u, v};

    // this thread's share of the staged tile: offsets within plane 1, -1 where the point lies beyond three cells from the interior
    long long raw_off[PER_THREAD];
#pragma unroll
    for (int q = 0; q < PER_THREAD; ++q) {
        const int p = tid + q * NT, a = p % EX, b = p / EX;
        const int i = i0 - R + a, j = j0 - R + b;
        raw_off[q] = (p < NP && i <= g.Nx + R && j <= g.Ny + R) ? at(L, i, j, 1) : -1;
    }
    double r[2][PER_THREAD];
    auto load_plane = [&](int k) {
        const long long ok = s3 * (k - 1);
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int q = 0; q < PER_THREAD; ++q) r[n][q] = raw_off[q] >= 0 ? fld[n][raw_off[q] + ok] : 0.0;
    };
    load_plane(k0);

    // this thread's cell
    const int ta = tid % TX, tb = tid / TX;
    const int i = i0 + ta, j = j0 + tb;
    const bool active = i <= g.Nx && j <= g.Ny;
    const int c = (tb + R) * EX + (ta + R);
    const long long o1 = at(L, i, j, 1);
#define LD(arr, da, db) lds[arr][c + (db) * EX + (da)]

    // advective_momentum_flux_Wu / Wv (or ζ₂wᶠᶜᶠ / ζ₁wᶜᶠᶠ of the conserving form) at the face kf of this thread's column
    auto face_flux = [&](int kf, double &Fu, double &Fv) {
        const long long of = o1 + s3 * (kf - 1);
        if constexpr (VERT) {
            const double wu = centered4(Az * w[of - 2], Az * w[of - 1], Az * w[of], Az * w[of + 1]);
            const double uR = bias_interp<OCN_BOUNDED, false>([&](int m) { return u[of + m * s3]; }, kf, Nz, wu > 0);
            Fu = wu * uR;
            const double wv = centered4(Az * w[of - 2 * s2], Az * w[of - s2], Az * w[of], Az * w[of + s2]);
            const double vR = bias_interp<OCN_BOUNDED, false>([&](int m) { return v[of + m * s3]; }, kf, Nz, wv > 0);
            Fv = wv * vR;
        } else {
            const double dzf = M.dzF(kf);
            Fu = (0.5 * (Az * w[of - 1] + Az * w[of])) * ((u[of] - u[of - s3]) / dzf);
            Fv = (0.5 * (Az * w[of - s2] + Az * w[of])) * ((v[of] - v[of - s3]) / dzf);
        }
    };
    double Fu_bot = 0.0, Fv_bot = 0.0;
    if (active) face_flux(k0, Fu_bot, Fv_bot);

    for (int k = k0; k <= k1; ++k) {
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int q = 0; q < PER_THREAD; ++q) {
                const int p = tid + q * NT;
                if (p < NP) lds[n][p] = r[n][q];
            }
        __syncthreads();
        if (k < k1) load_plane(k + 1);
        OCN_ISSUE_LOADS_HERE();

        const double dzk = M.dzC(k);
        const double Ax = dy * dzk, Ay = dx * dzk;

        // the intermediates, once per tile point (0 where a neighbour lies outside the staged tile: no cell reads those points)
        for (int p = tid; p < NP; p += NT) {
            const int a = p % EX, b = p / EX;
            const bool w_ = a >= 1, s_ = b >= 1, e_ = a + 1 < EX, n_ = b + 1 < EY;
            const double uc = lds[A::U][p], vc = lds[A::V][p];
            const double vw = w_ ? lds[A::V][p - 1] : 0.0, us = s_ ? lds[A::U][p - EX] : 0.0;
            const double ue = e_ ? lds[A::U][p + 1] : 0.0, vn = n_ ? lds[A::V][p + EX] : 0.0;
            lds[A::ZETA][p] = (w_ && s_) ? ((dy * vc - dy * vw) - (dx * uc - dx * us)) / Az : 0.0;
            if constexpr (VORT && VEL) {
                lds[A::UFF][p] = s_ ? 0.5 * (us + uc) : 0.0;
                lds[A::VFF][p] = w_ ? 0.5 * (vw + vc) : 0.0;
            }
            if constexpr (VERT) {
                const double dxu = e_ ? Ax * ue - Ax * uc : 0.0, dyv = n_ ? Ay * vn - Ay * vc : 0.0;
                lds[A::DXU][p] = dxu;
                lds[A::DYV][p] = dyv;
                lds[A::DIV][p] = dxu + dyv;
            }
            if constexpr (KE) {
                const double hu = (uc * uc) / 2, hv = (vc * vc) / 2;
                lds[A::DKU][p] = e_ ? (ue * ue) / 2 - hu : 0.0;
                lds[A::SU][p] = e_ ? 0.5 * (uc + ue) : 0.0;
                lds[A::DKV][p] = n_ ? (vn * vn) / 2 - hv : 0.0;
                lds[A::SV][p] = n_ ? 0.5 * (vc + vn) : 0.0;
                lds[A::CXV][p] = w_ ? hv - (vw * vw) / 2 : 0.0;
                lds[A::CYU][p] = s_ ? hu - (us * us) / 2 : 0.0;
            }
        }
        __syncthreads();

        if (active) {
            double Fu_top, Fv_top;
            face_flux(k + 1, Fu_top, Fv_top);
            const long long o = o1 + s3 * (k - 1);
            const double u_hat = LD(A::U, 0, 0), v_hat = LD(A::V, 0, 0);
            const double rV = 1 / (Az * dzk);
            auto Kh = [&](int a, int b) {  // Khᶜᶜᶜ at (i + a, j + b)
                return (0.5 * (LD(A::U, a, b) * LD(A::U, a, b) + LD(A::U, a + 1, b) * LD(A::U, a + 1, b)) +
                        0.5 * (LD(A::V, a, b) * LD(A::V, a, b) + LD(A::V, a, b + 1) * LD(A::V, a, b + 1))) / 2;
            };
            {   // ---- u
                auto m = [&](int a) { return 0.5 * (dx * LD(A::V, a, 0) + dx * LD(A::V, a, 1)); };  // ℑyᵃᶜᵃ(Δx_qᶜᶠᶜ v) at (i + a, j)
                double hadv;
                if constexpr (VORT) {
                    const double vh = (0.5 * (m(-1) + m(0))) / dx;
                    const bool left = vh > 0;
                    double S[6], Su[6], Sv[6];
#pragma unroll
                    for (int q = 0; q < 6; ++q) S[q] = LD(A::ZETA, 0, q - 2);
                    double zR;
                    if constexpr (VEL) {
#pragma unroll
                        for (int q = 0; q < 6; ++q) { Su[q] = LD(A::UFF, 0, q - 2); Sv[q] = LD(A::VFF, 0, q - 2); }
                        zR = weno5_smooth2(S, Su, Sv, left);
                    } else {
                        zR = weno5(S[0], S[1], S[2], S[3], S[4], S[5], left);
                    }
                    hadv = -vh * zR;
                } else {
                    hadv = -(0.5 * (LD(A::ZETA, 0, 0) + LD(A::ZETA, 0, 1))) * (0.5 * (m(-1) + m(0))) / dx;
                }
                double vadv;
                if constexpr (VERT) {
                    const double dvS = centered4(LD(A::DYV, -2, 0) + 0.0, LD(A::DYV, -1, 0) + 0.0, LD(A::DYV, 0, 0) + 0.0, LD(A::DYV, 1, 0) + 0.0);
                    double S[6], Sd[6];
#pragma unroll
                    for (int q = 0; q < 6; ++q) { S[q] = LD(A::DXU, q - 3, 0); Sd[q] = LD(A::DIV, q - 3, 0); }
                    const double duR = weno5_smooth(S, Sd, u_hat > 0);
                    vadv = rV * (u_hat * (dvS + duR) + (Fu_top - Fu_bot));
                } else {
                    vadv = (0.5 * (Fu_bot + Fu_top)) / Az;
                }
                double bern;
                if constexpr (KE) {
                    const double dKvS = centered4(LD(A::CXV, 0, -1), LD(A::CXV, 0, 0), LD(A::CXV, 0, 1), LD(A::CXV, 0, 2));
                    double S[6], Ss[6];
#pragma unroll
                    for (int q = 0; q < 6; ++q) { S[q] = LD(A::DKU, q - 3, 0); Ss[q] = LD(A::SU, q - 3, 0); }
                    const double dKuR = weno5_smooth(S, Ss, u_hat > 0);
                    bern = (dKuR + dKvS) / dx;
                } else {
                    bern = (Kh(0, 0) - Kh(-1, 0)) / dx;
                }
                double G = -((hadv + vadv) + bern);
                if (eta) {
                    const long long e = (i - 1 + g.Hx) + (long long)L.sx * (j - 1 + g.Hy);
                    G -= grav * ((eta[e] - eta[e - 1]) / dx);
                }
                Gu[o] = G;
            }
            {   // ---- v
                auto n = [&](int b) { return 0.5 * (dy * LD(A::U, 0, b) + dy * LD(A::U, 1, b)); };  // ℑxᶜᵃᵃ(Δy_qᶠᶜᶜ u) at (i, j + b)
                double hadv;
                if constexpr (VORT) {
                    const double uh = (0.5 * (n(-1) + n(0))) / dy;
                    const bool left = uh > 0;
                    double S[6], Su[6], Sv[6];
#pragma unroll
                    for (int q = 0; q < 6; ++q) S[q] = LD(A::ZETA, q - 2, 0);
                    double zR;
                    if constexpr (VEL) {
#pragma unroll
                        for (int q = 0; q < 6; ++q) { Su[q] = LD(A::UFF, q - 2, 0); Sv[q] = LD(A::VFF, q - 2, 0); }
                        zR = weno5_smooth2(S, Su, Sv, left);
                    } else {
                        zR = weno5(S[0], S[1], S[2], S[3], S[4], S[5], left);
                    }
                    hadv = uh * zR;
                } else {
                    hadv = (0.5 * (LD(A::ZETA, 0, 0) + LD(A::ZETA, 1, 0))) * (0.5 * (n(-1) + n(0))) / dy;
                }
                double vadv;
                if constexpr (VERT) {
                    const double duS = centered4(LD(A::DXU, 0, -2) + 0.0, LD(A::DXU, 0, -1) + 0.0, LD(A::DXU, 0, 0) + 0.0, LD(A::DXU, 0, 1) + 0.0);
                    double S[6], Sd[6];
#pragma unroll
                    for (int q = 0; q < 6; ++q) { S[q] = LD(A::DYV, 0, q - 3); Sd[q] = LD(A::DIV, 0, q - 3); }
                    const double dvR = weno5_smooth(S, Sd, v_hat > 0);
                    vadv = rV * (v_hat * (duS + dvR) + (Fv_top - Fv_bot));
                } else {
                    vadv = (0.5 * (Fv_bot + Fv_top)) / Az;
                }
                double bern;
                if constexpr (KE) {
                    const double dKuS = centered4(LD(A::CYU, -1, 0), LD(A::CYU, 0, 0), LD(A::CYU, 1, 0), LD(A::CYU, 2, 0));
                    double S[6], Ss[6];
#pragma unroll
                    for (int q = 0; q < 6; ++q) { S[q] = LD(A::DKV, 0, q - 3); Ss[q] = LD(A::SV, 0, q - 3); }
                    const double dKvR = weno5_smooth(S, Ss, v_hat > 0);
                    bern = (dKvR + dKuS) / dy;
                } else {
                    bern = (Kh(0, 0) - Kh(0, -1)) / dy;
                }
                double G = -((hadv + vadv) + bern);
                if (eta) {
                    const long long e = (i - 1 + g.Hx) + (long long)L.sx * (j - 1 + g.Hy);
                    G -= grav * ((eta[e] - eta[e - L.sx]) / dy);
                }
                Gv[o] = G;
            }
            Fu_bot = Fu_top;
            Fv_bot = Fv_top;
        }
        __syncthreads();  // every reader of this plane's arrays has passed before the next plane's u and v are written
    }
#undef LD
}

}  // namespace viw

// the caller (ocn_compute_vector_invariant_weno_momentum_tendencies) has validated the grid (Periodic regular x and y, Bounded z, Hx, Hy >= 3,
// Hz >= 1), the flags and the pointers
int launch_vector_invariant_weno(const ocn_grid *grid, int scheme_flags, const double *u, const double *v, const double *w, double *Gu,
                                 double *Gv, const double *eta, double grav, hipStream_t stream)
{
    const GridDev g = to_dev(*grid);
    const dim3 block(viw::NT, 1, 1);
    const dim3 blocks((grid->Nx + viw::TX - 1) / viw::TX, (grid->Ny + viw::TY - 1) / viw::TY, (grid->Nz + viw::PLANES - 1) / viw::PLANES);
    OCN_REQUIRE(blocks.y <= 65535u && blocks.z <= 65535u, "ocn_compute_vector_invariant_weno_momentum_tendencies: grid too large for one launch");
    const bool vort = scheme_flags & OCN_VI_WENO_VORTICITY, vert = scheme_flags & OCN_VI_WENO_VERTICAL, ke = scheme_flags & OCN_VI_WENO_KINETIC_ENERGY;
    const bool vel = !(scheme_flags & OCN_VI_DEFAULT_STENCIL);
#define OCN_VIW_LAUNCH(VORT, VERT, KE, VEL) \
    hipLaunchKernelGGL((viw::vector_invariant_weno_kernel<VORT, VERT, KE, VEL>), blocks, block, 0, stream, g, u, v, w, Gu, Gv, eta, grav)
    if (vort && vert && ke) {
        if (vel) OCN_VIW_LAUNCH(true, true, true, true); else OCN_VIW_LAUNCH(true, true, true, false);
    } else if (vort && vert) {
        if (vel) OCN_VIW_LAUNCH(true, true, false, true); else OCN_VIW_LAUNCH(true, true, false, false);
    } else if (vort) {
        if (vel) OCN_VIW_LAUNCH(true, false, false, true); else OCN_VIW_LAUNCH(true, false, false, false);
    } else if (ke) {
        OCN_VIW_LAUNCH(false, true, true, false);
    } else {
        OCN_VIW_LAUNCH(false, true, false, false);
    }
#undef OCN_VIW_LAUNCH
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

}  // namespace ocn
