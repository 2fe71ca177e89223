// smagorinsky.hip -- Smagorinsky / SmagorinskyLilly eddy viscosity (constant or Lilly coefficient).
//   _compute_smagorinsky_viscosity!   src/TurbulenceClosures/turbulence_closure_implementations/Smagorinskys/smagorinsky.jl:88-102
//   ΣᵢⱼΣᵢⱼᶜᶜᶜ                         .../Smagorinskys/scale_invariant_operators.jl:10-13
//   Σ₁₂, Σ₁₃, Σ₂₃, tr_Σ²              src/TurbulenceClosures/velocity_tracer_gradients.jl:25-46, 78
//   stability, square_smagorinsky_coefficient   .../Smagorinskys/lilly_coefficient.jl:126-139
//   ∂z_b                              src/BuoyancyFormulations/buoyancy_tracer.jl:16, seawater_buoyancy.jl:219-224
//
//   Σ²  = ((tr_Σ² + 2 ℑxyᶜᶜᵃ(Σ₁₂²)) + 2 ℑxzᶜᵃᶜ(Σ₁₃²)) + 2 ℑyzᵃᶜᶜ(Σ₂₃²)
//   Δᶠ  = cbrt(Δxᶜᶜᶜ Δyᶜᶜᶜ Δzᶜᶜᶜ)             (Flat directions: Δ = 1, differences vanish)
//   N²  = ℑzᵃᵃᶜ(∂z_b)                          (no buoyancy: 0)
//   ς   = ifelse(Σ² == 0, 0, sqrt(1 - min(1, Cb max(0, N²) / Σ²)))
//   νₑ  = (ς (C C)) (Δᶠ Δᶠ) sqrt(2 Σ²)         number coefficient: (C C) (Δᶠ Δᶠ) sqrt(2 Σ²), no buoyancy read
//
// One thread per cell, x fastest across the wave; a workgroup marches KZ planes upward and carries in registers what level k+1 of one
// iteration gives level k of the next (the two z-staggered squared strains of the upper row, the own-column velocities, w(k+1), the
// buoyancy tracers and the upper-face ∂z_b), so an iteration loads 19 values.  The stencil reaches ±1 in every direction: halo 1.
// The strict build writes every term as the reference spells it (operand order, nested-halves averages, IEEE division and sqrt); the
// only operation that is not correctly rounded is cbrt (within 1 ulp, and the value is squared).
//
// Tracers: the reference computes κ = ℑ(νₑ) / Pr on every face (smagorinsky.jl:136-138).  Where Pr == 1 the tracer kernels are handed the
// νₑ array itself (bit-identical); where Pr != 1 this kernel also stores κₑ = νₑ / Pr into a Center field of its own, which the tracer
// kernels interpolate: ℑ(νₑ / Pr) instead of ℑ(νₑ) / Pr -- THE ONE DEVIATION, rounding only, none for Pr a power of two.
#include <cstdlib>
#include "ocn_weno.h"

namespace OCN_NS {

using ocn::GridDev;
using ocn::Lay;

// GEN = 0: x, y Periodic -- one parent layout serves u, v, w and the centre fields.  GEN = 1: walls, no Flat direction (per-field
// strides).  GEN = 2: a Flat x / y (zero strides along it: differences vanish, interpolations return the value itself).
template <int GEN>
struct Smag {
    const double *u, *v, *w;  // pointers at the cell (i, j, k)
    long long s2, s3;         // centre fields
    long long u2, u3, v2, v3, w2, w3;
    int sa;
    __device__ __forceinline__ int SA() const { return GEN == 2 ? sa : 1; }
    __device__ __forceinline__ double U(int a, int b, int d) const { return GEN ? u[a * SA() + b * u2 + d * u3] : u[a + b * s2 + d * s3]; }
    __device__ __forceinline__ double V(int a, int b, int d) const { return GEN ? v[a * SA() + b * v2 + d * v3] : v[a + b * s2 + d * s3]; }
    __device__ __forceinline__ double W(int a, int b, int d) const { return GEN ? w[a * SA() + b * w2 + d * w3] : w[a + b * s2 + d * s3]; }
    __device__ __forceinline__ void up()  // one level up
    {
        u += GEN ? u3 : s3; v += GEN ? v3 : s3; w += GEN ? w3 : s3;
    }
};

constexpr int OCN_SMAG_MAX_KAPPA = OCN_MODEL_MAX_TRACERS;
struct SmagArgs {
    double C2, Cb;          // C C, LillyCoefficient.reduction_factor
    int lilly, buoyancy;    // buoyancy: OCN_BUOYANCY_* (NONE when the coefficient is a number)
    double g, alpha, beta;
    const double *T, *S;    // the buoyancy tracers (T: temperature or b), NULL = a constant: its derivative is 0
    int nk;                 // κₑ fields of their own (Pr != 1)
    double *kappa[OCN_SMAG_MAX_KAPPA];
    double Pr[OCN_SMAG_MAX_KAPPA];  // strict: Pr; fast: 1 / Pr
};

// ℑ over a 2x2 set of squares: 0.5 * (0.5*(f00 + f10) + 0.5*(f01 + f11)), first index = the inner interpolation
#if OCN_STRICT
#define SMAG_I4(f00, f10, f01, f11) (0.5 * (0.5 * ((f00) + (f10)) + 0.5 * ((f01) + (f11))))
#define SMAG_D(num, den) ((num) / (den))
#define SMAG_Q(x) (x)
#else  // fast math: one factor 1/4, reciprocal spacings, FMA contraction
#define SMAG_I4(f00, f10, f01, f11) (0.25 * (((f00) + (f10)) + ((f01) + (f11))))
#define SMAG_D(num, den) ((num) * (den))  /* den holds the reciprocal */
#define SMAG_Q(x) fast_rcp(x)
#endif

// ∂z_b on the face between two levels from the tracer differences there (d = δz c / Δzᵃᵃᶠ)
__device__ __forceinline__ double smag_dzb(const SmagArgs &p, double dT, double dS)
{
    if (p.buoyancy == OCN_BUOYANCY_TRACER) return dT;
    return p.g * (p.alpha * dT - p.beta * dS);
}

template <int GEN>
__global__ __launch_bounds__(256, 4) void smagorinsky_kernel(GridDev g, SmagArgs p, const double *__restrict__ u, const double *__restrict__ v,
                                                             const double *__restrict__ w, double *__restrict__ nu_e, int KZ, int xcd)
{
    int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
    if (xcd) {  // each XCD walks a contiguous range of tiles (as amd_fused_kernel)
        const unsigned nx = gridDim.x, ny = gridDim.y, n = nx * ny * gridDim.z;
        const unsigned b = bx + nx * (by + ny * bz);
        const unsigned q = b & 7u, chunk = n >> 3, rem = n & 7u;
        const unsigned logical = q * chunk + (q < rem ? q : rem) + (b >> 3);
        bx = logical % nx;
        by = (logical / nx) % ny;
        bz = logical / (nx * ny);
    }
    const int i = 1 + bx * blockDim.x + threadIdx.x, j = 1 + by * blockDim.y + threadIdx.y;
    if (i > g.Nx || j > g.Ny) return;
    const int kb = 1 + bz * KZ, ke = min(kb + KZ - 1, g.Nz);

    const Lay L = ocn::make_lay(g, OCN_LOC_CCC);
    long long o = ocn::at(L, i, j, kb);
    Smag<GEN> A;
    A.s2 = L.s2; A.s3 = L.s3; A.sa = 1;
    if (GEN) {
        const Lay Lu = ocn::make_lay(g, OCN_LOC_FCC), Lv = ocn::make_lay(g, OCN_LOC_CFC), Lw = ocn::make_lay(g, OCN_LOC_CCF);
        A.u = u + ocn::at(Lu, i, j, kb); A.v = v + ocn::at(Lv, i, j, kb); A.w = w + ocn::at(Lw, i, j, kb);
        A.u2 = Lu.s2; A.u3 = Lu.s3; A.v2 = Lv.s2; A.v3 = Lv.s3; A.w2 = Lw.s2; A.w3 = Lw.s3;
        if (GEN == 2 && g.tx == OCN_FLAT) A.sa = 0;
        if (GEN == 2 && g.ty == OCN_FLAT) A.u2 = A.v2 = A.w2 = A.s2 = 0;
    } else {
        A.u = u + o; A.v = v + o; A.w = w + o;
        A.u2 = A.v2 = A.w2 = L.s2; A.u3 = A.v3 = A.w3 = L.s3;
    }
    const Metrics M = make_metrics(g);
    const double qdx = SMAG_Q(M.dx), qdy = SMAG_Q(M.dy);
    const bool stratified = p.lilly && p.buoyancy != OCN_BUOYANCY_NONE;
    const double *pT = stratified && p.T ? p.T + o : nullptr, *pS = stratified && p.S ? p.S + o : nullptr;

    // level kb: what the iteration below expects from "the level underneath"
    double cU[2], cV[2], cW, q13[2], q23[2], cT = 0.0, cS = 0.0, bz0 = 0.0;
    {
        const double qdzf = SMAG_Q(M.dzF(kb));
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            cU[a] = A.U(a, 0, 0);
            cV[a] = A.V(0, a, 0);
            const double s13 = 0.5 * (SMAG_D(cU[a] - A.U(a, 0, -1), qdzf) + SMAG_D(A.W(a, 0, 0) - A.W(a - 1, 0, 0), qdx));  // Σ₁₃ at (i+a, j, kb)
            const double s23 = 0.5 * (SMAG_D(cV[a] - A.V(0, a, -1), qdzf) + SMAG_D(A.W(0, a, 0) - A.W(0, a - 1, 0), qdy));  // Σ₂₃ at (i, j+a, kb)
            q13[a] = s13 * s13;
            q23[a] = s23 * s23;
        }
        cW = A.W(0, 0, 0);
        if (stratified) {
            double dT = 0.0, dS = 0.0;
            if (pT) { cT = pT[0]; dT = SMAG_D(cT - pT[-L.s3], qdzf); }
            if (pS) { cS = pS[0]; dS = SMAG_D(cS - pS[-L.s3], qdzf); }
            bz0 = smag_dzb(p, dT, dS);
        }
    }
    const double dxdy = M.dx * M.dy;
    double Df2 = 0.0;
    if (!M.dzc) {
        const double Df = cbrt(dxdy * M.dz);
        Df2 = Df * Df;
    }
    for (int k = kb; k <= ke; ++k) {
        if (M.dzc) {  // stretched z: Δᶠ of this level (k is uniform across the workgroup)
            const double Df = cbrt(dxdy * M.dzC(k));
            Df2 = Df * Df;
        }
        const double qdzc = SMAG_Q(M.dzC(k)), qdzf1 = SMAG_Q(M.dzF(k + 1));
        // new values: the in-plane neighbours at level k and everything at level k+1
        const double uT[2] = {A.U(0, 0, 1), A.U(1, 0, 1)}, vT[2] = {A.V(0, 0, 1), A.V(0, 1, 1)};
        const double wT[3] = {A.W(-1, 0, 1), A.W(0, 0, 1), A.W(1, 0, 1)}, wS = A.W(0, -1, 1), wN = A.W(0, 1, 1);
        const double uS[2] = {A.U(0, -1, 0), A.U(1, -1, 0)}, uN[2] = {A.U(0, 1, 0), A.U(1, 1, 0)};
        const double vW[2] = {A.V(-1, 0, 0), A.V(-1, 1, 0)}, vE[2] = {A.V(1, 0, 0), A.V(1, 1, 0)};
        double nT = 0.0, nS = 0.0;
        if (pT) nT = pT[L.s3];
        if (pS) nS = pS[L.s3];

        // Σ₁₂ at (i+a, j+b, k) = 0.5 (∂y_u + ∂x_v)
        double q12[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const double dyu = b ? SMAG_D(uN[a] - cU[a], qdy) : SMAG_D(cU[a] - uS[a], qdy);
                const double dxv = a ? SMAG_D(vE[b] - cV[b], qdx) : SMAG_D(cV[b] - vW[b], qdx);
                const double s = 0.5 * (dyu + dxv);
                q12[a][b] = s * s;
            }
        // Σ₁₃ at (i+a, j, k+1) = 0.5 (∂z_u + ∂x_w),  Σ₂₃ at (i, j+b, k+1) = 0.5 (∂z_v + ∂y_w)
        double t13[2], t23[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const double s13 = 0.5 * (SMAG_D(uT[a] - cU[a], qdzf1) + SMAG_D(wT[a + 1] - wT[a], qdx));
            const double dyw = a ? SMAG_D(wN - wT[1], qdy) : SMAG_D(wT[1] - wS, qdy);
            const double s23 = 0.5 * (SMAG_D(vT[a] - cV[a], qdzf1) + dyw);
            t13[a] = s13 * s13;
            t23[a] = s23 * s23;
        }
        const double dxu = SMAG_D(cU[1] - cU[0], qdx), dyv = SMAG_D(cV[1] - cV[0], qdy), dzw = SMAG_D(wT[1] - cW, qdzc);
        const double tr = (dxu * dxu + dyv * dyv) + dzw * dzw;
        const double S2 = ((tr + 2 * SMAG_I4(q12[0][0], q12[1][0], q12[0][1], q12[1][1])) + 2 * SMAG_I4(q13[0], q13[1], t13[0], t13[1])) +
                          2 * SMAG_I4(q23[0], q23[1], t23[0], t23[1]);
        double cs2 = p.C2;
        if (p.lilly) {
            double bz1 = 0.0;
            if (stratified) bz1 = smag_dzb(p, pT ? SMAG_D(nT - cT, qdzf1) : 0.0, pS ? SMAG_D(nS - cS, qdzf1) : 0.0);
            const double N2 = 0.5 * (bz0 + bz1);
            const double N2p = N2 > 0 ? N2 : 0.0;
            // Σ² == 0: min(1, x / 0) is 1 or NaN in the reference and its ifelse returns 0 either way
#if OCN_STRICT
            const double ratio = p.Cb * N2p / S2;
#else
            // (fast_rcp of a nonzero Σ² below 2^-1024 is NaN -- the ratio then compared as >= 1 and νₑ came out 0: IEEE division there)
            const double ratio = S2 >= 0x1p-1000 ? p.Cb * N2p * fast_rcp(S2) : p.Cb * N2p / S2;
#endif
            const double sig = S2 == 0 ? 0.0 : sqrt(1.0 - (ratio < 1.0 ? ratio : 1.0));
            cs2 = sig * p.C2;
            bz0 = bz1;
        }
        const double nu = cs2 * Df2 * sqrt(2 * S2);
        nu_e[o] = nu;
#pragma unroll
        for (int n = 0; n < OCN_SMAG_MAX_KAPPA; ++n)
            if (n < p.nk) p.kappa[n][o] = SMAG_D(nu, p.Pr[n]);
        // level k+1 becomes level k
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            cU[a] = uT[a]; cV[a] = vT[a];
            q13[a] = t13[a]; q23[a] = t23[a];
        }
        cW = wT[1]; cT = nT; cS = nS;
        A.up();
        o += L.s3;
        if (pT) pT += L.s3;
        if (pS) pS += L.s3;
    }
}
#undef SMAG_I4
#undef SMAG_D
#undef SMAG_Q

int launch_smagorinsky(const ocn_grid *grid, const ocn::TermsDev &t, const ocn_smagorinsky &cl, const double *u, const double *v, const double *w,
                       double *nu_e, double *const *kappa_e, hipStream_t stream)
{
    SmagArgs p{};
    p.C2 = cl.C * cl.C;
    p.Cb = cl.lilly ? cl.Cb : 0.0;
    p.lilly = cl.lilly ? 1 : 0;
    p.buoyancy = cl.lilly ? t.buoyancy : OCN_BUOYANCY_NONE;
    p.g = t.g; p.alpha = t.alpha; p.beta = t.beta;
    if (p.buoyancy == OCN_BUOYANCY_TRACER || p.buoyancy == OCN_BUOYANCY_SEAWATER_TS || p.buoyancy == OCN_BUOYANCY_SEAWATER_T) p.T = t.T;
    if (p.buoyancy == OCN_BUOYANCY_SEAWATER_TS || p.buoyancy == OCN_BUOYANCY_SEAWATER_S) p.S = t.S;
    for (int n = 0; n < cl.n_tracers && n < OCN_MODEL_MAX_TRACERS; ++n) {
        if (cl.Pr[n] == 1.0 || !kappa_e || !kappa_e[n] || kappa_e[n] == nu_e) continue;  // this tracer reads the nu_e array
        bool seen = false;
        for (int q = 0; q < p.nk; ++q) seen = seen || p.kappa[q] == kappa_e[n];
        if (seen) continue;
        p.kappa[p.nk] = kappa_e[n];
#if OCN_STRICT
        p.Pr[p.nk] = cl.Pr[n];
#else
        p.Pr[p.nk] = 1.0 / cl.Pr[n];
#endif
        p.nk += 1;
    }
    GridDev g = ocn::to_dev(*grid);
    static const int kz_env = getenv("OCN_SMAG_KZ") ? atoi(getenv("OCN_SMAG_KZ")) : 16;
    static const int xcd = getenv("OCN_XCD_REMAP") ? atoi(getenv("OCN_XCD_REMAP")) : 1;
    dim3 block = ocn::range_block(g.Nx);
    if (block.x == 64) block = dim3(32, 8, 1);  // squarer tiles: fewer rim rows re-read per plane
    int KZ = kz_env < 1 ? 1 : kz_env;
    const long long tiles = (long long)((g.Nx + block.x - 1) / block.x) * ((g.Ny + block.y - 1) / block.y);
    while (KZ > 1 && tiles * ((g.Nz + KZ - 1) / KZ) < 2048) KZ = (KZ + 1) / 2;  // small grids: keep the chip full
    const dim3 nb = ocn::range_grid(block, g.Nx, g.Ny, (g.Nz + KZ - 1) / KZ);
    if (grid->tx == OCN_FLAT || grid->ty == OCN_FLAT)  // zero strides along a Flat direction
        hipLaunchKernelGGL(smagorinsky_kernel<2>, nb, block, 0, stream, g, p, u, v, w, nu_e, KZ, xcd);
    else if (ocn::x_wall_west(*grid) || ocn::x_wall_east(*grid) || grid->ty == OCN_BOUNDED)  // per-field parent layouts
        hipLaunchKernelGGL(smagorinsky_kernel<1>, nb, block, 0, stream, g, p, u, v, w, nu_e, KZ, xcd);
    else
        hipLaunchKernelGGL(smagorinsky_kernel<0>, nb, block, 0, stream, g, p, u, v, w, nu_e, KZ, xcd);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

}  // namespace OCN_NS
