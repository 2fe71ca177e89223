// biharmonic.hip -- HorizontalScalarBiharmonicDiffusivity (ScalarBiharmonicDiffusivity{HorizontalFormulation}, constant ν and κ) on a
// (Periodic, Periodic, any z) grid with regular x and y: the closure's term subtracted from tendencies that hold every other term,
//   Gu <- Gu - ∂ⱼτ₁ⱼ,  Gv <- Gv - ∂ⱼτ₂ⱼ,  Gc <- Gc - ∇_dot_qᶜ        (closure_kernel_operators.jl:22-34, 43-48)
// with (abstract_scalar_biharmonic_diffusivity_closure.jl:46-51, 66-67, 75-102; the biharmonic masks are identities on Periodic x, y)
//   viscous_flux_ux = viscous_flux_vy = ν δ★ᶜᶜᶜ,   viscous_flux_vx = ν ζ★ᶠᶠᶜ,   viscous_flux_uy = -(ν ζ★ᶠᶠᶜ),   no z flux (the generic zero)
//   δ★ᶜᶜᶜ = 1 / Az * (δxᶜ(Δy ∇²hᶠᶜᶜ u) + δyᶜ(Δx ∇²hᶜᶠᶜ v)),   ζ★ᶠᶠᶜ = 1 / Az * (δxᶠ(Δy ∇²hᶜᶠᶜ v) - δyᶠ(Δx ∇²hᶠᶜᶜ u))
//   diffusive_flux_x = κ (1 / Az * δxᶠ(Δy ∇²hᶜᶜᶜ c)),   diffusive_flux_y = κ (1 / Az * δyᶠ(Δx ∇²hᶜᶜᶜ c))
//   ∇²h φ = 1 / V * (δx(Ax ∂x φ) + δy(Ay ∂y φ))                                       (Operators/laplacian_operators.jl:5-18)
// Ax = Δy Δz, Ay = Δx Δz, V = Az Δz carry Δz of the cell's own plane: on a stretched z it cancels only up to rounding, so it stays.
//
// Three nested difference stages, each a radius-1 stencil of the one before.  A workgroup of 256 threads owns a TX x TY = 64 x 8 tile of
// the xy plane and marches a chunk of k planes (the planes are independent: the march amortises the index arithmetic and lets the loads
// of plane k + 1 leave before the arithmetic of plane k).  Per plane, through LDS:
//   raw   the fields on tile + 2 rings            (TX + 4) x (TY + 4)   from global memory, through registers (loaded a plane ahead)
//   lap   ∇²h on tile + 1 ring                    (TX + 2) x (TY + 2)
//   flux  ν δ★, ν ζ★ (or the tracer's flux pair)   (TX + 1) x (TY + 1)   the one-sided ring each divergence needs
//   the divergence, and G read, updated and written once per cell.
// u and v share a launch (δ★ and ζ★ need both Laplacians); a tracer takes a launch of its own (one field through the same three stages).
// Cells of the rings that lie beyond two cells from the interior are not read (taken as 0; nothing that reaches a written cell uses them).
//
// Bandwidth-bound: one strict build (no FMA contraction, IEEE division), bit-identical to tests/biharmonic_numpy.py.
#include "ocn_ivd.h"

namespace ocn {

namespace bih {

constexpr int TX = 64, TY = 8, NT = 256;
constexpr int RX = TX + 4, RY = TY + 4;  // raw
constexpr int LX = TX + 2, LY = TY + 2;  // Laplacians
constexpr int FX = TX + 1, FY = TY + 1;  // fluxes
constexpr int RAW_PER_THREAD = (RX * RY + NT - 1) / NT;
constexpr int PLANES = 8;  // planes marched by one workgroup

struct PlaneMetrics {
    double dx, dy, Ax, Ay, rV, rAz;
};

// ∇²h at the point whose raw neighbours are W, E (x), S, N (y) and whose own value is C: the same index pattern at ccc, fcc and cfc
__device__ __forceinline__ double laplacian_h(const PlaneMetrics &m, double C, double W, double E, double S, double N)
{
    const double dxF = m.Ax * ((E - C) / m.dx) - m.Ax * ((C - W) / m.dx);
    const double dyF = m.Ay * ((N - C) / m.dy) - m.Ay * ((C - S) / m.dy);
    return m.rV * (dxF + dyF);
}

// G - a, or G - (a + b) where the caller holds -b (the term of the tuple's other closure, formed as 0 - b on a zeroed array)
__device__ __forceinline__ double subtract_term(double G, double a, const double *neg_other, long long o)
{
    return neg_other ? G - (a + (0.0 - neg_other[o])) : G - a;
}

// MOM: f0 = u, f1 = v, G0 = Gu, G1 = Gv, coef = ν.  Else: f0 = c, G0 = Gc, coef = κ (f1, G1, n1 unused).
template <bool MOM>
__global__ __launch_bounds__(NT) void biharmonic_fluxes(GridDev g, double coef, const double *__restrict__ f0, const double *__restrict__ f1,
                                                        double *__restrict__ G0, double *__restrict__ G1, const double *__restrict__ n0,
                                                        const double *__restrict__ n1)
{
    constexpr int NF = MOM ? 2 : 1;
    __shared__ double raw[NF][RY][RX];
    __shared__ double lap[NF][LY][LX];
    __shared__ double flux[2][FY][FX];

    const int tid = threadIdx.x;
    const int i0 = 1 + blockIdx.x * TX, j0 = 1 + blockIdx.y * TY;  // first interior cell of the tile
    const int k0 = 1 + blockIdx.z * PLANES, k1 = min(k0 + PLANES - 1, g.Nz);
    const ivd::Spacings M = ivd::spacings_of(g);
    const Lay L = make_lay(g, OCN_LOC_CCC);  // Periodic x and y: u, v and c share one parent layout
    const double *fld[2] = {f0, f1};

    // this thread's share of the raw tile: offsets within a plane, -1 where the point lies beyond two cells from the interior
    long long raw_off[RAW_PER_THREAD];
#pragma unroll
    for (int q = 0; q < RAW_PER_THREAD; ++q) {
        const int p = tid + q * NT, a = p % RX, b = p / RX;
        const int i = i0 - 2 + a, j = j0 - 2 + b;
        raw_off[q] = (p < RX * RY && i <= g.Nx + 2 && j <= g.Ny + 2) ? at(L, i, j, 1) : -1;
    }
    double r[NF][RAW_PER_THREAD];
    auto load_plane = [&](int k) {
        const long long ok = L.s3 * (k - 1);
#pragma unroll
        for (int n = 0; n < NF; ++n)
#pragma unroll
            for (int q = 0; q < RAW_PER_THREAD; ++q) r[n][q] = raw_off[q] >= 0 ? fld[n][raw_off[q] + ok] : 0.0;
    };
    load_plane(k0);

    const double Az = g.dx * g.dy;
    for (int k = k0; k <= k1; ++k) {
#pragma unroll
        for (int n = 0; n < NF; ++n)
#pragma unroll
            for (int q = 0; q < RAW_PER_THREAD; ++q) {
                const int p = tid + q * NT;
                if (p < RX * RY) raw[n][p / RX][p % RX] = r[n][q];
            }
        __syncthreads();
        if (k < k1) load_plane(k + 1);
        OCN_ISSUE_LOADS_HERE();

        const double dzk = M.dzC(k);
        PlaneMetrics m;
        m.dx = g.dx;
        m.dy = g.dy;
        m.Ax = g.dy * dzk;
        m.Ay = g.dx * dzk;
        m.rV = 1 / (Az * dzk);
        m.rAz = 1 / Az;

        // lap[b][a] <-> (i0 - 1 + a, j0 - 1 + b) <-> raw[b + 1][a + 1]
        for (int p = tid; p < LX * LY; p += NT) {
            const int a = p % LX, b = p / LX;
#pragma unroll
            for (int n = 0; n < NF; ++n)
                lap[n][b][a] = laplacian_h(m, raw[n][b + 1][a + 1], raw[n][b + 1][a], raw[n][b + 1][a + 2], raw[n][b][a + 1], raw[n][b + 2][a + 1]);
        }
        __syncthreads();

        for (int p = tid; p < FX * FY; p += NT) {
            const int a = p % FX, b = p / FX;
            if constexpr (MOM) {
                // flux[0][b][a] = ν δ★ᶜᶜᶜ at (i0 - 1 + a, j0 - 1 + b) <-> lap[b][a];   flux[1][b][a] = ν ζ★ᶠᶠᶜ at (i0 + a, j0 + b) <-> lap[b + 1][a + 1]
                const double dstar =
                    m.rAz * ((m.dy * lap[0][b][a + 1] - m.dy * lap[0][b][a]) + (m.dx * lap[1][b + 1][a] - m.dx * lap[1][b][a]));
                const double zstar = m.rAz * ((m.dy * lap[1][b + 1][a + 1] - m.dy * lap[1][b + 1][a]) -
                                              (m.dx * lap[0][b + 1][a + 1] - m.dx * lap[0][b][a + 1]));
                flux[0][b][a] = coef * dstar;
                flux[1][b][a] = coef * zstar;
            } else {
                // diffusive_flux_x at the x-face, diffusive_flux_y at the y-face of (i0 + a, j0 + b) <-> lap[b + 1][a + 1]
                flux[0][b][a] = coef * (m.rAz * (m.dy * lap[0][b + 1][a + 1] - m.dy * lap[0][b + 1][a]));
                flux[1][b][a] = coef * (m.rAz * (m.dx * lap[0][b + 1][a + 1] - m.dx * lap[0][b][a + 1]));
            }
        }
        __syncthreads();

        const long long ok = L.s3 * (k - 1);
        for (int p = tid; p < TX * TY; p += NT) {
            const int a = p % TX, b = p / TX;
            const int i = i0 + a, j = j0 + b;
            if (i > g.Nx || j > g.Ny) continue;
            const long long o = at(L, i, j, 1) + ok;
            if constexpr (MOM) {
                // δ★ at (i, j) is flux[0][b + 1][a + 1], ζ★ at (i, j) is flux[1][b][a]
                const double uyn = -flux[1][b + 1][a], uys = -flux[1][b][a];
                const double au = m.rV * (((m.Ax * flux[0][b + 1][a + 1] - m.Ax * flux[0][b + 1][a]) + (m.Ay * uyn - m.Ay * uys)) + 0.0);
                const double av = m.rV * (((m.Ax * flux[1][b][a + 1] - m.Ax * flux[1][b][a]) +
                                           (m.Ay * flux[0][b + 1][a + 1] - m.Ay * flux[0][b][a + 1])) + 0.0);
                G0[o] = subtract_term(G0[o], au, n0, o);
                G1[o] = subtract_term(G1[o], av, n1, o);
            } else {
                const double ac = m.rV * (((m.Ax * flux[0][b][a + 1] - m.Ax * flux[0][b][a]) + (m.Ay * flux[1][b + 1][a] - m.Ay * flux[1][b][a])) + 0.0);
                G0[o] = subtract_term(G0[o], ac, n0, o);
            }
        }
        // the next plane's raw, lap and flux are each written behind a barrier that every reader of this plane's has passed
    }
}

}  // namespace bih

// the caller (ocn_add_biharmonic_fluxes) has validated the grid (Periodic regular x and y, Hx, Hy >= 2) and the pointers
int launch_biharmonic_fluxes(const ocn_grid *grid, double nu, const double *u, const double *v, double *Gu, double *Gv, int n_tracers,
                             const double *kappa, const double *const *c, double *const *Gc, const double *neg_other_u,
                             const double *neg_other_v, const double *const *neg_other_c, hipStream_t stream)
{
    const GridDev gd = to_dev(*grid);
    const dim3 block(bih::NT, 1, 1);
    const dim3 blocks((grid->Nx + bih::TX - 1) / bih::TX, (grid->Ny + bih::TY - 1) / bih::TY, (grid->Nz + bih::PLANES - 1) / bih::PLANES);
    OCN_REQUIRE(blocks.y <= 65535u && blocks.z <= 65535u, "ocn_add_biharmonic_fluxes: grid too large for one launch");
    // a zero coefficient gives a term of ±0: its launch is skipped unless the other closure's term has to be subtracted
    if (u && (nu != 0.0 || neg_other_u))
        hipLaunchKernelGGL(bih::biharmonic_fluxes<true>, blocks, block, 0, stream, gd, nu, u, v, Gu, Gv, neg_other_u, neg_other_v);
    for (int n = 0; n < n_tracers; ++n) {
        const double *other = neg_other_c ? neg_other_c[n] : nullptr;
        if (kappa[n] == 0.0 && !other) continue;
        hipLaunchKernelGGL(bih::biharmonic_fluxes<false>, blocks, block, 0, stream, gd, kappa[n], c[n], (const double *)nullptr, Gc[n],
                           (double *)nullptr, other, (const double *)nullptr);
    }
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

}  // namespace ocn
