// implicit_diffusion.hip -- ScalarDiffusivity(VerticallyImplicitTimeDiscretization(), ν, κ) with constant ν, κ on a z-Bounded grid.
//
// Two pieces, neither of which touches an existing kernel (the host computes every other term with the existing entry points and a copy
// of its ocn_model_terms whose closure is 0):
//
//  1. the EXPLICIT part of the closure term (abstract_scalar_diffusivity_closure.jl:214-260), added to a G that holds everything else:
//       horizontal fluxes and the x / y fluxes of w            as for the explicit closure
//       tracer diffusive_flux_z                                the explicit flux at k == 1 | k == Nz+1, zero on interior faces
//       viscous_flux_uz / vz                                   the explicit flux at k == 1 | k == Nz+1, -ν ∂x w / -ν ∂y w elsewhere
//       viscous_flux_wz                                        the explicit flux at k == 1 | k == Nz+1, zero elsewhere
//     One thread per cell, topologies read at run time, the operand order of momentum_extra_general / tracer_diffusion_general
//     (general.hip), which is the reference's (closure_kernel_operators.jl:27-53).
//
//  2. the IMPLICIT step  (1 - Δt ∂z κ ∂z) φⁿ⁺¹ = φ★  in place for n fields in one launch (implicit_step!,
//     vertically_implicit_diffusion_solver.jl:55-110: the Center-in-z rows for u, v and tracers, the Face-in-z rows for w, index shifts
//     and k < 1 guards as written there), eliminated in the order of solve_batched_tridiagonal_system_z!
//     (batched_tridiagonal_solver.jl).  One thread owns one (i, j) column, x fastest across the lanes: every access to a k plane is
//     coalesced, the k loops are sequential.  With constant κ the matrix depends on k only, so the lower diagonal a, the pivots β and the
//     multipliers t are the same for every column: a block computes them ONCE into LDS (the three diagonals in parallel, then one thread
//     runs the Nz-long recurrence), and every lane reads them from there as wave-uniform broadcasts (no bank conflicts, no VGPR arrays).
//     The forward sweep parks its intermediate in the field itself (the reference solves with the field as its own right-hand side), the
//     backward sweep reads it back: 32 B / cell of traffic, no scratch array.  Loads are issued IVD_BATCH planes ahead of the sequential
//     arithmetic so that a column has several independent loads in flight.
//
// Bandwidth-bound: one strict build (no FMA contraction) whatever the math mode, bit-identical to tests/implicit_diffusion_numpy.py.
#include "ocn_ivd.h"

namespace ocn {

namespace ivd {

// G <- G - ∂ⱼτᵢⱼ with the vertically implicit part of τᵢ₃ left out
__global__ __launch_bounds__(256) void momentum_explicit_part(GridDev g, double nu, const double *__restrict__ u, const double *__restrict__ v,
                                                              const double *__restrict__ w, double *__restrict__ Gu, double *__restrict__ Gv,
                                                              double *__restrict__ Gw, Range r)
{
    int i, j, k;
    if (!cell_of(r, i, j, k)) return;
    const Spacings M = spacings_of(g);
    const Lay Lu = make_lay(g, OCN_LOC_FCC), Lv = make_lay(g, OCN_LOC_CFC), Lw = make_lay(g, OCN_LOC_CCF);
    const bool fx = g.tx == OCN_FLAT, fy = g.ty == OCN_FLAT;
    const double dx = g.dx, dy = g.dy;
    const int Nz = g.Nz;
#define U_(a, b, c) u[at(Lu, a, b, c)]
#define V_(a, b, c) v[at(Lv, a, b, c)]
#define W_(a, b, c) w[at(Lw, a, b, c)]
    auto DXU_C = [&](int a, int b, int c) { return fx ? 0.0 : (U_(a + 1, b, c) - U_(a, b, c)) / dx; };
    auto DYV_C = [&](int a, int b, int c) { return fy ? 0.0 : (V_(a, b + 1, c) - V_(a, b, c)) / dy; };
    auto DZW_C = [&](int a, int b, int c) { return (W_(a, b, c + 1) - W_(a, b, c)) / M.dzC(c); };
    auto DYU_FF = [&](int a, int b, int c) { return fy ? 0.0 : (U_(a, b, c) - U_(a, b - 1, c)) / dy; };
    auto DXV_FF = [&](int a, int b, int c) { return fx ? 0.0 : (V_(a, b, c) - V_(a - 1, b, c)) / dx; };
    auto DZU_FF = [&](int a, int b, int c) { return (U_(a, b, c) - U_(a, b, c - 1)) / M.dzF(c); };
    auto DXW_FF = [&](int a, int b, int c) { return fx ? 0.0 : (W_(a, b, c) - W_(a - 1, b, c)) / dx; };
    auto DZV_FF = [&](int a, int b, int c) { return (V_(a, b, c) - V_(a, b, c - 1)) / M.dzF(c); };
    auto DYW_FF = [&](int a, int b, int c) { return fy ? 0.0 : (W_(a, b, c) - W_(a, b - 1, c)) / dy; };
    auto T11 = [&](int a, int b, int c) { return -2 * (nu * DXU_C(a, b, c)); };
    auto T22 = [&](int a, int b, int c) { return -2 * (nu * DYV_C(a, b, c)); };
    auto T12 = [&](int a, int b, int c) { return -2 * (nu * (0.5 * (DYU_FF(a, b, c) + DXV_FF(a, b, c)))); };
    auto boundary = [&](int c) { return (c == 1) | (c == Nz + 1); };
    // viscous_flux_uz / vz / wz(::VerticallyBoundedGrid, ::VITD): explicit on the two boundaries, the ivd flux elsewhere
    auto T13 = [&](int a, int b, int c) {
        return boundary(c) ? -2 * (nu * (0.5 * (DZU_FF(a, b, c) + DXW_FF(a, b, c)))) : -(nu * DXW_FF(a, b, c));
    };
    auto T23 = [&](int a, int b, int c) {
        return boundary(c) ? -2 * (nu * (0.5 * (DZV_FF(a, b, c) + DYW_FF(a, b, c)))) : -(nu * DYW_FF(a, b, c));
    };
    auto T33 = [&](int a, int b, int c) { return boundary(c) ? -2 * (nu * DZW_C(a, b, c)) : 0.0; };
    const double Az = dx * dy;
    const double Axc = dy * M.dzC(k), Ayc = dx * M.dzC(k);
    if (i >= r.ou) {
        const long long o = at(Lu, i, j, k);
        const double dxF = fx ? 0.0 : Axc * T11(i, j, k) - Axc * T11(i - 1, j, k);
        const double dyF = fy ? 0.0 : Ayc * T12(i, j + 1, k) - Ayc * T12(i, j, k);
        const double dzF = Az * T13(i, j, k + 1) - Az * T13(i, j, k);
        Gu[o] = Gu[o] - 1 / (Az * M.dzC(k)) * ((dxF + dyF) + dzF);
    }
    if (j >= r.ov) {
        const long long o = at(Lv, i, j, k);
        const double dxF = fx ? 0.0 : Axc * T12(i + 1, j, k) - Axc * T12(i, j, k);
        const double dyF = fy ? 0.0 : Ayc * T22(i, j, k) - Ayc * T22(i, j - 1, k);
        const double dzF = Az * T23(i, j, k + 1) - Az * T23(i, j, k);
        Gv[o] = Gv[o] - 1 / (Az * M.dzC(k)) * ((dxF + dyF) + dzF);
    }
    if (Gw && k >= r.ow) {
        const long long o = at(Lw, i, j, k);
        const double Axf = dy * M.dzF(k), Ayf = dx * M.dzF(k);
        // (x / y fluxes of w: the explicit ones, ν (∂z u + ∂x w) -- only viscous_flux_uz / vz / wz have vertically implicit methods)
        auto E13 = [&](int a, int b, int c) { return -2 * (nu * (0.5 * (DZU_FF(a, b, c) + DXW_FF(a, b, c)))); };
        auto E23 = [&](int a, int b, int c) { return -2 * (nu * (0.5 * (DZV_FF(a, b, c) + DYW_FF(a, b, c)))); };
        const double dxF = fx ? 0.0 : Axf * E13(i + 1, j, k) - Axf * E13(i, j, k);
        const double dyF = fy ? 0.0 : Ayf * E23(i, j + 1, k) - Ayf * E23(i, j, k);
        const double dzF = Az * T33(i, j, k) - Az * T33(i, j, k - 1);
        Gw[o] = Gw[o] - 1 / (Az * M.dzF(k)) * ((dxF + dyF) + dzF);
    }
#undef U_
#undef V_
#undef W_
}

// Gc <- Gc - ∇_dot_qᶜ with the vertically implicit part of q₃ left out
__global__ __launch_bounds__(256) void tracer_explicit_part(GridDev g, double kappa, const double *__restrict__ c, double *__restrict__ Gc, Range r)
{
    int i, j, k;
    if (!cell_of(r, i, j, k)) return;
    const Spacings M = spacings_of(g);
    const Lay L = make_lay(g, OCN_LOC_CCC);
    const bool fx = g.tx == OCN_FLAT, fy = g.ty == OCN_FLAT;
    const int Nz = g.Nz;
#define C_(a, b, cc) c[at(L, a, b, cc)]
    auto QX = [&](int a, int b, int cc) { return -(kappa * ((C_(a, b, cc) - C_(a - 1, b, cc)) / g.dx)); };
    auto QY = [&](int a, int b, int cc) { return -(kappa * ((C_(a, b, cc) - C_(a, b - 1, cc)) / g.dy)); };
    auto QZ = [&](int a, int b, int cc) {
        return ((cc == 1) | (cc == Nz + 1)) ? -(kappa * ((C_(a, b, cc) - C_(a, b, cc - 1)) / M.dzF(cc))) : 0.0;
    };
    const double Ax = g.dy * M.dzC(k), Ay = g.dx * M.dzC(k), Az = g.dx * g.dy;
    const double dxF = fx ? 0.0 : Ax * QX(i + 1, j, k) - Ax * QX(i, j, k);
    const double dyF = fy ? 0.0 : Ay * QY(i, j + 1, k) - Ay * QY(i, j, k);
    const double dzF = Az * QZ(i, j, k + 1) - Az * QZ(i, j, k);
    const long long o = at(L, i, j, k);
    Gc[o] = Gc[o] - 1 / (Az * M.dzC(k)) * ((dxF + dyF) + dzF);
#undef C_
}

// ---------------------------------------------------------------------------------------------------
// implicit step
// ---------------------------------------------------------------------------------------------------
struct Columns {
    double *f[MAX_TUPLE];
    double kappa[MAX_TUPLE];
    int loc[MAX_TUPLE];
};

// the coefficient functions of vertically_implicit_diffusion_solver.jl:55-110, k the index they are called with
__device__ __forceinline__ double upper_diagonal(const Spacings &M, bool zface, int Nz, double dt, double kappa, int k)
{
    if (zface) {  // ivd_upper_diagonal(..., ::Face, ...)
        const double du = -dt * kappa / (M.dzC(k) * M.dzF(k));
        return k < 1 ? 0.0 : du;
    }
    const double du = -dt * kappa / (M.dzC(k) * M.dzF(k + 1));
    return k > Nz - 1 ? 0.0 : du;
}
__device__ __forceinline__ double lower_diagonal(const Spacings &M, bool zface, double dt, double kappa, int k)
{
    if (zface) {  // k′ = k + 2:  Δzᶜ(k′) Δzᶠ(k′ - 1)
        const double dl = -dt * kappa / (M.dzC(k + 2) * M.dzF(k + 1));
        return k < 1 ? 0.0 : dl;
    }
    const double dl = -dt * kappa / (M.dzC(k + 1) * M.dzF(k + 1));  // k = k′ + 1
    return k < 1 ? 0.0 : dl;
}

constexpr int IVD_BATCH = 8;

__global__ __launch_bounds__(256) void implicit_step(GridDev g, Columns cols, double dt)
{
    extern __shared__ double lds[];  // a[Nz] | β[Nz] | t[Nz], element 0 <-> k = 1
    const int Nz = g.Nz, fld = blockIdx.z;
    double *A = lds, *B = lds + Nz, *T = lds + 2 * Nz;
    const Spacings M = spacings_of(g);
    const int loc = cols.loc[fld];
    const bool zface = (loc & 4) != 0;
    const double kappa = cols.kappa[fld];
    const int tid = threadIdx.y * 64 + threadIdx.x;
    // the three diagonals (every level is independent) ...
    for (int k = 1 + tid; k <= Nz; k += 256) {
        const double up = upper_diagonal(M, zface, Nz, dt, kappa, k);
        A[k - 1] = k < Nz ? lower_diagonal(M, zface, dt, kappa, k) : 0.0;  // (row Nz has no entry below it: never read)
        B[k - 1] = (1.0 - up) - lower_diagonal(M, zface, dt, kappa, k - 1);  // ivd_diagonal (the implicit linear coefficient is zero)
        T[k - 1] = up;
    }
    __syncthreads();
    // ... then the pivots and multipliers of the elimination, once for the block: t[k] = c[k-1] / β, β = b[k] - a[k-1] t[k]
    if (tid == 0) {
        double beta = B[0], cprev = T[0];
        for (int k = 2; k <= Nz; ++k) {
            const double ccur = T[k - 1];
            const double t = cprev / beta;
            beta = B[k - 1] - A[k - 2] * t;
            T[k - 1] = t;
            B[k - 1] = beta;
            cprev = ccur;
        }
    }
    __syncthreads();
    const int i = 1 + blockIdx.x * 64 + threadIdx.x, j = 1 + blockIdx.y * 4 + threadIdx.y;
    if (i > g.Nx || j > g.Ny) return;
    const Lay L = make_lay(g, loc);
    double *__restrict__ p = cols.f[fld] + at(L, i, j, 1);
    const long long s3 = L.s3;
    const double tiny = 10 * 2.220446049250313e-16;  // 10 eps(Float64)
    // forward sweep, the intermediate parked in the field
    double prev = p[0] / B[0];
    p[0] = prev;
    for (int k0 = 2; k0 <= Nz; k0 += IVD_BATCH) {
        double f[IVD_BATCH] = {};
#pragma unroll
        for (int q = 0; q < IVD_BATCH; ++q)
            if (k0 + q <= Nz) f[q] = p[(k0 + q - 1) * s3];
#pragma unroll
        for (int q = 0; q < IVD_BATCH; ++q) {
            const int k = k0 + q;
            if (k <= Nz) {
                const double beta = B[k - 1];
                const double star = (f[q] - A[k - 2] * prev) / beta;
                prev = fabs(beta) > tiny ? star : f[q];
                p[(k - 1) * s3] = prev;
            }
        }
    }
    // backward sweep: φ[k] -= t[k+1] φ[k+1]
    for (int k0 = Nz - 1; k0 >= 1; k0 -= IVD_BATCH) {
        double f[IVD_BATCH] = {};
#pragma unroll
        for (int q = 0; q < IVD_BATCH; ++q)
            if (k0 - q >= 1) f[q] = p[(k0 - q - 1) * s3];
#pragma unroll
        for (int q = 0; q < IVD_BATCH; ++q) {
            const int k = k0 - q;
            if (k >= 1) {
                prev = f[q] - T[k] * prev;
                p[(k - 1) * s3] = prev;
            }
        }
    }
}

}  // namespace ivd

int make_ivd_range(const ocn_grid *grid, const int32_t *range, ivd::Range &r)
{
    if (range) {
        r.i0 = range[0]; r.i1 = range[1]; r.j0 = range[2]; r.j1 = range[3]; r.k0 = range[4]; r.k1 = range[5];
        OCN_REQUIRE(r.i0 >= 1 && r.i1 <= grid->Nx && r.j0 >= 1 && r.j1 <= grid->Ny && r.k0 >= 1 && r.k1 <= grid->Nz,
                    "tendency range {%d:%d,%d:%d,%d:%d} outside the interior %dx%dx%d", r.i0, r.i1, r.j0, r.j1, r.k0, r.k1, grid->Nx, grid->Ny,
                    grid->Nz);
        r.ou = r.ov = r.ow = 1;  // KernelParameters: periphery not excluded
    } else {
        r.i0 = 1; r.i1 = grid->Nx; r.j0 = 1; r.j1 = grid->Ny; r.k0 = 1; r.k1 = grid->Nz;
        r.ou = (x_wall_west(*grid) && grid->Nx > 1) ? 2 : 1;  // periphery_offset(Face, Bounded, N) (kernel_launching.jl:113-114)
        r.ov = (grid->ty == OCN_BOUNDED && grid->Ny > 1) ? 2 : 1;
        r.ow = grid->Nz > 1 ? 2 : 1;
    }
    return OCN_SUCCESS;
}

// both callers have validated the grid (z Bounded, halos >= 1) and the pointers
int launch_ivd_explicit_part(const ocn_grid *grid, double nu, const double *u, const double *v, const double *w, double *Gu, double *Gv,
                             double *Gw, int n_tracers, const double *kappa, const double *const *c, double *const *Gc, const int32_t *range,
                             hipStream_t stream)
{
    ivd::Range r;
    OCN_TRY(make_ivd_range(grid, range, r));
    const int wx = r.i1 - r.i0 + 1, wy = r.j1 - r.j0 + 1, wz = r.k1 - r.k0 + 1;
    if (wx < 1 || wy < 1 || wz < 1) return OCN_SUCCESS;
    const dim3 block(64, 4, 1), blocks((wx + 63) / 64, (wy + 3) / 4, wz);
    const GridDev gd = to_dev(*grid);
    if (u) hipLaunchKernelGGL(ivd::momentum_explicit_part, blocks, block, 0, stream, gd, nu, u, v, w, Gu, Gv, Gw, r);
    for (int n = 0; n < n_tracers; ++n)
        hipLaunchKernelGGL(ivd::tracer_explicit_part, blocks, block, 0, stream, gd, kappa[n], c[n], Gc[n], r);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

int launch_ivd_implicit_step(const ocn_grid *grid, int n, double *const *fields, const int32_t *locs, const double *kappa, double dt,
                             hipStream_t stream)
{
    ivd::Columns cols{};
    for (int f = 0; f < n; ++f) {
        cols.f[f] = fields[f];
        cols.loc[f] = locs[f];
        cols.kappa[f] = kappa[f];
    }
    const dim3 block(64, 4, 1), blocks((grid->Nx + 63) / 64, (grid->Ny + 3) / 4, n);
    const size_t lds = 3 * (size_t)grid->Nz * sizeof(double);
    hipLaunchKernelGGL(ivd::implicit_step, blocks, block, lds, stream, to_dev(*grid), cols, dt);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

}  // namespace ocn
