// immersed.hip -- HydrostaticFreeSurfaceModel on ImmersedBoundaryGrid(grid, GridFittedBottom(h)): (Periodic, Periodic, Bounded) underlying
// grid, regular x and y, one GPU.  Here are the kernels over bathymetry that have no twin in hydrostatic_surface.hip:
// the bottom itself (kbot and the column depths), the masking, and the viscous and tracer kernels, which are the periodic kernels of
// physics.hip with the reference's immersed rules applied, in the same evaluation order, so that over a flat bottom they return the same
// bits.  The vector-invariant, split-explicit and corrector kernels are the grid-fitted instantiations of hydrostatic_surface.hip.
//
//   * conditional differences   ImmersedBoundaries/conditional_differences.jl:25-77: a difference is 0 when one of its two nodes is an
//                               immersed_inactive_node, otherwise the underlying grid's
//   * conditional fluxes        Advection/immersed_advective_fluxes.jl:20-59, TurbulenceClosures/immersed_diffusive_fluxes.jl:27-44: a flux
//                               is 0 on an immersed_peripheral_node of its own location
//   * masking                   ImmersedBoundaries/mask_immersed_field.jl:53-105
//
// The node predicates, and how the bathymetry reaches the kernels (one int32 plane, kbot), are in ocn_immersed.h.
#include "ocn_common.h"
#include "ocn_immersed.h"
#include "ocn_internal.h"

namespace ocn {

namespace {

// ---- materialize_immersed_boundary (grid_fitted_bottom.jl:99-122), immersed_cell (:124-130), static_column_depth (:147-150) -------------
// One thread per point of the parent plane; a halo point computes the column it is the periodic image of (fill_halo_regions! of the
// bottom field).  zc: z of the Nz cell centres, zf: z of the Nz + 1 faces (rnode).
struct Column {
    double bottom;
    int kbot;
};
__device__ __forceinline__ Column materialize_column(double zb, int Nz, int interface_condition, const double *__restrict__ zc,
                                                     const double *__restrict__ zf)
{
    Column c;
    c.bottom = zf[0];
    for (int k = 1; k <= Nz; ++k) {
        const double zp = zf[k], z = zc[k - 1];
        const bool bottom_cell = interface_condition ? zp <= zb : z <= zb;
        c.bottom = bottom_cell ? zp : c.bottom;
    }
    c.kbot = 0;
    for (int k = 1; k <= Nz; ++k) c.kbot += (zc[k - 1] <= c.bottom) ? 1 : 0;
    return c;
}
__global__ void bottom_kernel(int Nx, int Ny, int Nz, int Hx, int Hy, int interface_condition, const double *__restrict__ h,
                              const double *__restrict__ zc, const double *__restrict__ zf, double *__restrict__ bottom,
                              int32_t *__restrict__ kbot, double *__restrict__ Hcc, double *__restrict__ Hfc, double *__restrict__ Hcf)
{
    const int sx = Nx + 2 * Hx, sy = Ny + 2 * Hy;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)sx * sy) return;
    const int I = (int)(t % sx), J = (int)(t / sx);
    auto wrap = [](int q, int N) { return ((q % N) + N) % N; };
    const int si = wrap(I - Hx, Nx), sj = wrap(J - Hy, Ny);  // 0-based interior column
    auto column = [&](int a, int b) { return materialize_column(h[(Hx + wrap(a, Nx)) + (long long)sx * (Hy + wrap(b, Ny))], Nz, interface_condition, zc, zf); };
    const Column c = column(si, sj), w = column(si - 1, sj), s = column(si, sj - 1);
    const double top = zf[Nz];
    const double hc = top - c.bottom, hw = top - w.bottom, hs = top - s.bottom;
    bottom[t] = c.bottom;
    kbot[t] = c.kbot;
    Hcc[t] = hc;
    Hfc[t] = hw < hc ? hw : hc;  // min(static_column_depthᶜᶜᵃ(i - 1, j), static_column_depthᶜᶜᵃ(i, j))
    Hcf[t] = hs < hc ? hs : hc;
}

// ---- mask_immersed_field! of a tuple of fields and the planes η (Center, Center, Face at k = Nz + 1), U (Face, Center, Nothing at k = Nz),
// V (Center, Face, Nothing at k = Nz): field = ifelse(immersed_peripheral_node, value, field); only masked nodes are written --------------
__global__ __launch_bounds__(256) void mask_kernel(GridDev g, const int32_t *__restrict__ kbot, FieldTuple f, double value,
                                                   double *__restrict__ eta, double *__restrict__ U, double *__restrict__ V)
{
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x, j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    if (i > g.Nx || j > g.Ny) return;
    const int Nz = g.Nz, k0 = 1 + blockIdx.z * KZ, k1 = imin(k0 + KZ - 1, Nz);
    const long long e = plane_at(g, i, j), sx = g.Nx + 2 * g.Hx;
    const int kc = kbot[e], kw = kbot[e - 1], ks = kbot[e - sx];
    const int mxu = imax(kw, kc), mxv = imax(ks, kc);
    const Lay L = make_lay(g, OCN_LOC_CCC);  // (Periodic x and y: one parent layout but for the number of planes)
    for (int n = 0; n < f.n; ++n) {
        const int loc = f.loc[n];
        const int mx = (loc & 1) ? mxu : ((loc & 2) ? mxv : kc);
        double *__restrict__ p = f.f[n];
        for (int k = k0; k <= k1; ++k) {
            const bool masked = (loc & 4) ? peripheral_f(mx, k, Nz) : peripheral_c(mx, k, Nz);
            if (masked) p[at(L, i, j, k)] = value;
        }
    }
    if (blockIdx.z == 0) {
        // immersed_peripheral_node(i, j, Nz + 1, c, c, f) for η: the plane lies on the underlying grid's own periphery, so this never holds
        if (eta && peripheral_f(kc, Nz + 1, Nz)) eta[e] = value;
        if (U && peripheral_c(mxu, Nz, Nz)) U[e] = value;
        if (V && peripheral_c(mxv, Nz, Nz)) V[e] = value;
    }
}

// ---- Gu -= ∂ⱼτ₁ⱼ, Gv -= ∂ⱼτ₂ⱼ of an explicit ScalarDiffusivity(ν): the closure term of momentum_extra_cell (physics.hip) with conditional
// fluxes and differences.  τ₁₁, τ₂₂ at (c, c, c) and τ₁₂ at (f, f, c) are 0 on a peripheral node; where they are not, every cell the node
// touches is active, so none of the velocity nodes they difference is inactive (each of those touches one of these cells) and the
// differences are the underlying grid's.  τ₁₃, τ₂₃ at the faces k = 1 and k = Nz + 1 lie on the underlying grid's periphery and are never
// masked: there the differences of u, v and w are conditional.
#define TAU(nuv, s) (-2 * ((nuv) * (s)))
__global__ __launch_bounds__(256) void viscosity_immersed_kernel(GridDev g, const int32_t *__restrict__ kbot, double nu,
                                                                 const double *__restrict__ u, const double *__restrict__ v,
                                                                 const double *__restrict__ w, double *__restrict__ Gu, double *__restrict__ Gv)
{
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x, j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    if (i > g.Nx || j > g.Ny) return;
    const int Nz = g.Nz, k0 = 1 + blockIdx.z * KZ, k1 = imin(k0 + KZ - 1, Nz);
    const Cols c = load_cols(g, kbot, i, j);
    auto mx4 = [&](int a, int b) { return imax(imax(c(a - 1, b - 1), c(a, b - 1)), imax(c(a - 1, b), c(a, b))); };  // (f, f) node at (i + a, j + b)
    const int c00 = c(0, 0), cm0 = c(-1, 0), c0m = c(0, -1);
    const int f00 = mx4(0, 0), f01 = mx4(0, 1), f10 = mx4(1, 0);
    const int mxu = imax(cm0, c00), mnu = imin(cm0, c00), mxv = imax(c0m, c00), mnv = imin(c0m, c00);
    const Lay L = make_lay(g, OCN_LOC_CCC);
    const long long s2 = L.s2, s3 = L.s3;
    const double dx = g.dx, dy = g.dy, Az = dx * dy;
    for (int k = k0; k <= k1; ++k) {
        const long long o = at(L, i, j, k);
        const double dzc = dz_centre(g, k), dzf = dz_face(g, k), dzf1 = dz_face(g, k + 1);
        const double Axc = dy * dzc, Ayc = dx * dzc;
        const double *pu = u + o, *pv = v + o, *pw = w + o;
#define U_(a, b, c) pu[(a) + (b)*s2 + (c)*s3]
#define V_(a, b, c) pv[(a) + (b)*s2 + (c)*s3]
#define W_(a, b, c) pw[(a) + (b)*s2 + (c)*s3]
#define DX(a, b) (((a) - (b)) / dx)
#define DY(a, b) (((a) - (b)) / dy)
        // Σ₁₃ = (∂zᶠᶜᶠ u + ∂xᶠᶜᶠ w) / 2 at face k + q of the u column; Σ₂₃ likewise
        auto t13 = [&](int q, double dzq) {
            if (peripheral_f(mxu, k + q, Nz)) return 0.0;
            const bool zu = inactive_c(mnu, k + q, Nz) || inactive_c(mnu, k + q - 1, Nz);
            const bool zw = inactive_f(c00, k + q, Nz) || inactive_f(cm0, k + q, Nz);
            return TAU(nu, 0.5 * (((zu ? 0.0 : U_(0, 0, q) - U_(0, 0, q - 1)) / dzq) + ((zw ? 0.0 : W_(0, 0, q) - W_(-1, 0, q)) / dx)));
        };
        auto t23 = [&](int q, double dzq) {
            if (peripheral_f(mxv, k + q, Nz)) return 0.0;
            const bool zv = inactive_c(mnv, k + q, Nz) || inactive_c(mnv, k + q - 1, Nz);
            const bool zw = inactive_f(c00, k + q, Nz) || inactive_f(c0m, k + q, Nz);
            return TAU(nu, 0.5 * (((zv ? 0.0 : V_(0, 0, q) - V_(0, 0, q - 1)) / dzq) + ((zw ? 0.0 : W_(0, 0, q) - W_(0, -1, q)) / dy)));
        };
        const double t12c = peripheral_c(f00, k, Nz) ? 0.0 : TAU(nu, 0.5 * (DY(U_(0, 0, 0), U_(0, -1, 0)) + DX(V_(0, 0, 0), V_(-1, 0, 0))));
        {   // ---- u
            const double t11e = peripheral_c(c00, k, Nz) ? 0.0 : TAU(nu, DX(U_(1, 0, 0), U_(0, 0, 0)));
            const double t11w = peripheral_c(cm0, k, Nz) ? 0.0 : TAU(nu, DX(U_(0, 0, 0), U_(-1, 0, 0)));
            const double t12n = peripheral_c(f01, k, Nz) ? 0.0 : TAU(nu, 0.5 * (DY(U_(0, 1, 0), U_(0, 0, 0)) + DX(V_(0, 1, 0), V_(-1, 1, 0))));
            const double dzF = Az * t13(1, dzf1) - Az * t13(0, dzf);
            Gu[o] = Gu[o] - 1 / (Az * dzc) * (((Axc * t11e - Axc * t11w) + (Ayc * t12n - Ayc * t12c)) + dzF);
        }
        {   // ---- v
            const double t12e = peripheral_c(f10, k, Nz) ? 0.0 : TAU(nu, 0.5 * (DY(U_(1, 0, 0), U_(1, -1, 0)) + DX(V_(1, 0, 0), V_(0, 0, 0))));
            const double t22n = peripheral_c(c00, k, Nz) ? 0.0 : TAU(nu, DY(V_(0, 1, 0), V_(0, 0, 0)));
            const double t22s = peripheral_c(c0m, k, Nz) ? 0.0 : TAU(nu, DY(V_(0, 0, 0), V_(0, -1, 0)));
            const double dzF = Az * t23(1, dzf1) - Az * t23(0, dzf);
            Gv[o] = Gv[o] - 1 / (Az * dzc) * (((Axc * t12e - Axc * t12c) + (Ayc * t22n - Ayc * t22s)) + dzF);
        }
    }
}
#undef TAU

// ---- Gc = - div_Uc - ∇_dot_qᶜ: tracer_tendency_centered2 followed by tracer_diffusion_kernel (physics.hip), every flux 0 on a peripheral
// node of its own location.  Where a horizontal flux is not masked both of its cells are active and the difference inside it is the
// underlying grid's; the vertical diffusive fluxes at k = 1 and k = Nz + 1 are never masked and difference conditionally.
#define AVG(x, y) (0.5 * (x) + 0.5 * (y))
__global__ __launch_bounds__(256) void tracer_immersed_kernel(GridDev g, const int32_t *__restrict__ kbot, int diffuse, double kappa,
                                                              const double *__restrict__ u, const double *__restrict__ v,
                                                              const double *__restrict__ w, const double *__restrict__ cc,
                                                              double *__restrict__ Gc)
{
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x, j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    if (i > g.Nx || j > g.Ny) return;
    const int Nz = g.Nz, k0 = 1 + blockIdx.z * KZ, k1 = imin(k0 + KZ - 1, Nz);
    const long long e = plane_at(g, i, j), sx = g.Nx + 2 * g.Hx;
    const int kc = kbot[e];
    const int mxw = imax(kbot[e - 1], kc), mxe = imax(kc, kbot[e + 1]), mxs = imax(kbot[e - sx], kc), mxn = imax(kc, kbot[e + sx]);
    const Lay L = make_lay(g, OCN_LOC_CCC);
    const long long s2 = L.s2, s3 = L.s3;
    const double dx = g.dx, dy = g.dy, Az = dx * dy;
    for (int k = k0; k <= k1; ++k) {
        const long long o = at(L, i, j, k);
        const double dzc = dz_centre(g, k), dzf = dz_face(g, k), dzf1 = dz_face(g, k + 1);
        const double Ax = dy * dzc, Ay = dx * dzc;
        const double *pu = u + o, *pv = v + o, *pw = w + o, *pc = cc + o;
#define C_(a, b, q) pc[(a) + (b)*s2 + (q)*s3]
        const bool pe = peripheral_c(mxe, k, Nz), pwst = peripheral_c(mxw, k, Nz), pn = peripheral_c(mxn, k, Nz), ps = peripheral_c(mxs, k, Nz);
        const bool pt = peripheral_f(kc, k + 1, Nz), pb = peripheral_f(kc, k, Nz);
        const double c0 = C_(0, 0, 0);
        const double fx = (pe ? 0.0 : (Ax * U_(1, 0, 0)) * AVG(c0, C_(1, 0, 0))) - (pwst ? 0.0 : (Ax * U_(0, 0, 0)) * AVG(C_(-1, 0, 0), c0));
        const double fy = (pn ? 0.0 : (Ay * V_(0, 1, 0)) * AVG(c0, C_(0, 1, 0))) - (ps ? 0.0 : (Ay * V_(0, 0, 0)) * AVG(C_(0, -1, 0), c0));
        const double fzz = (pt ? 0.0 : (Az * W_(0, 0, 1)) * AVG(c0, C_(0, 0, 1))) - (pb ? 0.0 : (Az * W_(0, 0, 0)) * AVG(C_(0, 0, -1), c0));
        const double rV = 1 / (Az * dzc);
        double G = -(rV * ((fx + fy) + fzz));
        if (diffuse) {
            const double qxe = pe ? 0.0 : -(kappa * DX(C_(1, 0, 0), c0)), qxw = pwst ? 0.0 : -(kappa * DX(c0, C_(-1, 0, 0)));
            const double qyn = pn ? 0.0 : -(kappa * DY(C_(0, 1, 0), c0)), qys = ps ? 0.0 : -(kappa * DY(c0, C_(0, -1, 0)));
            const bool zt = inactive_c(kc, k + 1, Nz) || inactive_c(kc, k, Nz), zb = inactive_c(kc, k, Nz) || inactive_c(kc, k - 1, Nz);
            const double qzt = pt ? 0.0 : -(kappa * ((zt ? 0.0 : C_(0, 0, 1) - c0) / dzf1));
            const double qzb = pb ? 0.0 : -(kappa * ((zb ? 0.0 : c0 - C_(0, 0, -1)) / dzf));
            const double dzF = Az * qzt - Az * qzb;
            G = G - 1 / (Az * dzc) * (((Ax * qxe - Ax * qxw) + (Ay * qyn - Ay * qys)) + dzF);
        }
        Gc[o] = G;
    }
}
#undef AVG
#undef C_
#undef DX
#undef DY
#undef U_
#undef V_
#undef W_

}  // namespace

int launch_immersed_bottom(const ocn_grid *grid, int interface_condition, const double *h, const double *zc, const double *zf, double *bottom,
                           int32_t *kbot, double *Hcc, double *Hfc, double *Hcf, hipStream_t stream)
{
    const long long n = (long long)(grid->Nx + 2 * grid->Hx) * (grid->Ny + 2 * grid->Hy);
    hipLaunchKernelGGL(bottom_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, grid->Nx, grid->Ny, grid->Nz, grid->Hx, grid->Hy,
                       interface_condition, h, zc, zf, bottom, kbot, Hcc, Hfc, Hcf);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}
int launch_immersed_mask(const ocn_grid *grid, const int32_t *kbot, const FieldTuple &f, double value, double *eta, double *U, double *V,
                         hipStream_t stream)
{
    GridDev g = to_dev(*grid);
    hipLaunchKernelGGL(mask_kernel, xy_blocks(g.Nx, g.Ny, z_chunks(g.Nz)), dim3(64, 4, 1), 0, stream, g, kbot, f, value, eta, U, V);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}
int launch_viscosity_immersed(const ocn_grid *grid, const int32_t *kbot, double nu, const double *u, const double *v, const double *w,
                              double *Gu, double *Gv, hipStream_t stream)
{
    GridDev g = to_dev(*grid);
    hipLaunchKernelGGL(viscosity_immersed_kernel, xy_blocks(g.Nx, g.Ny, z_chunks(g.Nz)), dim3(64, 4, 1), 0, stream, g, kbot, nu, u, v, w, Gu, Gv);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}
int launch_tracer_immersed(const ocn_grid *grid, const int32_t *kbot, int diffuse, double kappa, const double *u, const double *v,
                           const double *w, const double *c, double *Gc, hipStream_t stream)
{
    GridDev g = to_dev(*grid);
    hipLaunchKernelGGL(tracer_immersed_kernel, xy_blocks(g.Nx, g.Ny, z_chunks(g.Nz)), dim3(64, 4, 1), 0, stream, g, kbot, diffuse, kappa, u, v, w, c,
                       Gc);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

}  // namespace ocn
