// immersed.hip -- HydrostaticFreeSurfaceModel on ImmersedBoundaryGrid(grid, GridFittedBottom(h)): (Periodic, Periodic, Bounded) underlying
// grid, regular x and y, one GPU.  The kernels are the periodic hydrostatic kernels of hydrostatic_surface.hip / physics.hip with the
// reference's immersed rules applied, in the same evaluation order, so that over a flat bottom they return the same bits:
//
//   * conditional differences   ImmersedBoundaries/conditional_differences.jl:25-77: a difference is 0 when one of its two nodes is an
//                               immersed_inactive_node, otherwise the underlying grid's
//   * conditional fluxes        Advection/immersed_advective_fluxes.jl:20-59, TurbulenceClosures/immersed_diffusive_fluxes.jl:27-44: a flux
//                               is 0 on an immersed_peripheral_node of its own location
//   * masking                   ImmersedBoundaries/mask_immersed_field.jl:53-105
//   * split-explicit surface    SplitExplicitFreeSurfaces/*.jl with static_column_depth (grid_fitted_bottom.jl:147-150)
//
// The bathymetry reaches the kernels as ONE int32 plane: kbot[i, j], the number of immersed cells of the column (cell k is immersed iff
// k <= kbot), shaped like η with periodically filled halos.  inactive_cell is monotone in kbot, so the AND over the cells a node touches is
// the predicate at the MINIMUM of their kbot and the OR the predicate at the MAXIMUM: every node predicate below is a comparison of k with
// kbot at one, two or four columns (Grids/inactive_node.jl:127-155, immersed_boundary_interface.jl:49-60).  A thread loads the kbot of its
// 3 x 3 columns once and walks KZ levels with them in registers; the z extent stays in the launch.
#include "ocn_common.h"
#include "ocn_internal.h"

namespace ocn {

namespace {

constexpr int KZ = 8;  // levels per thread (1 to 32 measured: DESIGN §5.2q)

// inactive_cell of the immersed grid (immersed, or outside 1..Nz) and of the underlying grid, for a column with kb immersed cells
__device__ __forceinline__ bool ic(int kb, int k, int Nz) { return k < 1 || k > Nz || k <= kb; }
__device__ __forceinline__ bool i0(int k, int Nz) { return k < 1 || k > Nz; }
// immersed_inactive_node / immersed_peripheral_node of a node that is Center in z (mn / mx: min / max of kbot over its columns) ...
__device__ __forceinline__ bool inactive_c(int mn, int k, int Nz) { return ic(mn, k, Nz) && !i0(k, Nz); }
__device__ __forceinline__ bool peripheral_c(int mx, int k, int Nz) { return ic(mx, k, Nz) && !i0(k, Nz); }
// ... and of one that is Face in z (it touches the cells k - 1 and k)
__device__ __forceinline__ bool inactive_f(int mn, int k, int Nz) { return ic(mn, k - 1, Nz) && ic(mn, k, Nz) && !(i0(k - 1, Nz) && i0(k, Nz)); }
__device__ __forceinline__ bool peripheral_f(int mx, int k, int Nz) { return (ic(mx, k - 1, Nz) || ic(mx, k, Nz)) && !(i0(k - 1, Nz) || i0(k, Nz)); }

// inactive_node(i, j, Nz + 1, c, c, f): the column is dry
__device__ __forceinline__ bool inactive_f_top(int kb, int Nz) { return ic(kb, Nz, Nz) && ic(kb, Nz + 1, Nz); }

__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }
inline int z_chunks(int Nz) { return (Nz + KZ - 1) / KZ; }

// kbot of the 3 x 3 columns around (i, j): kb[1 + a][1 + b] is column (i + a, j + b)
struct Cols {
    int kb[3][3];
    __device__ __forceinline__ int operator()(int a, int b) const { return kb[1 + a][1 + b]; }
};
__device__ __forceinline__ Cols load_cols(const GridDev &g, const int32_t *__restrict__ kbot, int i, int j)
{
    Cols c;
    const long long e = plane_at(g, i, j), sx = g.Nx + 2 * g.Hx;
#pragma unroll
    for (int a = -1; a <= 1; ++a)
#pragma unroll
        for (int b = -1; b <= 1; ++b) c.kb[1 + a][1 + b] = kbot[e + a + sx * b];
    return c;
}

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

// ---- vector_invariant_kernel of hydrostatic_surface.hip with the conditional differences: the two differences of ζ₃ᶠᶠᶜ, ∂z u / ∂z v of the vertical
// advection, ∂x / ∂y of Kh.  g ∂x η is taken at k = Nz + 1, where the centre node is inactive on the underlying grid as well: never zeroed.
__global__ __launch_bounds__(256) void vector_invariant_immersed_kernel(GridDev g, const int32_t *__restrict__ kbot, const double *__restrict__ u,
                                                                        const double *__restrict__ v, const double *__restrict__ w,
                                                                        double *__restrict__ Gu, double *__restrict__ Gv,
                                                                        const double *__restrict__ eta, double grav)
{
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x, j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    if (i > g.Nx || j > g.Ny) return;
    const int Nz = g.Nz, k0 = 1 + blockIdx.z * KZ, k1 = imin(k0 + KZ - 1, Nz);
    const Cols c = load_cols(g, kbot, i, j);
    // min of kbot over the two cells of the u node (Face, Center) and of the v node (Center, Face) at (i + a, j + b)
    auto mnu = [&](int a, int b) { return imin(c(a - 1, b), c(a, b)); };
    auto mnv = [&](int a, int b) { return imin(c(a, b - 1), c(a, b)); };
    const int u00 = mnu(0, 0), u0m = mnu(0, -1), u0p = mnu(0, 1), up0 = mnu(1, 0), upm = mnu(1, -1);
    const int v00 = mnv(0, 0), vm0 = mnv(-1, 0), v0p = mnv(0, 1), vmp = mnv(-1, 1), vp0 = mnv(1, 0);
    const int c00 = c(0, 0), cm0 = c(-1, 0), c0m = c(0, -1);
    const Lay L = make_lay(g, OCN_LOC_CCC);
    const long long s2 = L.s2, s3 = L.s3;
    const double dx = g.dx, dy = g.dy, Az = dx * dy;
    const long long e = plane_at(g, i, j), sx = g.Nx + 2 * g.Hx;
    double gex = 0.0, gey = 0.0;
    if (eta) {
        gex = grav * ((eta[e] - eta[e - 1]) / g.dx);
        gey = grav * ((eta[e] - eta[e - sx]) / g.dy);
    }
    for (int k = k0; k <= k1; ++k) {
        const long long o = at(L, i, j, k);
        const double dzf0 = dz_face(g, k), dzf1 = dz_face(g, k + 1);
        const double *pu = u + o, *pv = v + o, *pw = w + o;
#define U_(a, b, c) pu[(a) + (b)*s2 + (c)*s3]
#define V_(a, b, c) pv[(a) + (b)*s2 + (c)*s3]
#define W_(a, b, c) pw[(a) + (b)*s2 + (c)*s3]
        // ζ₃ᶠᶠᶜ at (i + a, j + b): δxᶠᶠᶜ(Δy v) is 0 when one of the v nodes (mv1, mv0) is inactive, δyᶠᶠᶜ(Δx u) when one of the u nodes is
        auto zeta = [&](int a, int b, int mv1, int mv0, int mu1, int mu0) {
            const bool zv = inactive_c(mv1, k, Nz) || inactive_c(mv0, k, Nz), zu = inactive_c(mu1, k, Nz) || inactive_c(mu0, k, Nz);
            const double dv = zv ? 0.0 : dy * V_(a, b, 0) - dy * V_(a - 1, b, 0);
            const double du = zu ? 0.0 : dx * U_(a, b, 0) - dx * U_(a, b - 1, 0);
            return (dv - du) / Az;
        };
        auto Kh = [&](int a, int b) {
            return (0.5 * (U_(a, b, 0) * U_(a, b, 0) + U_(a + 1, b, 0) * U_(a + 1, b, 0)) +
                    0.5 * (V_(a, b, 0) * V_(a, b, 0) + V_(a, b + 1, 0) * V_(a, b + 1, 0))) / 2;
        };
        const double z00 = zeta(0, 0, v00, vm0, u00, u0m);
        {   // ---- u
            auto m = [&](int a) { return 0.5 * (dx * V_(a, 0, 0) + dx * V_(a, 1, 0)); };
            const double z01 = zeta(0, 1, v0p, vmp, u0p, u00);
            const double hadv = -(0.5 * (z00 + z01)) * (0.5 * (m(-1) + m(0))) / dx;
            auto Z = [&](int q, double dzf) {  // ζ₂wᶠᶜᶠ at face k + q: ∂zᶠᶜᶠ u is 0 when u at k + q or at k + q - 1 is inactive
                const bool zz = inactive_c(u00, k + q, Nz) || inactive_c(u00, k + q - 1, Nz);
                return (0.5 * (Az * W_(-1, 0, q) + Az * W_(0, 0, q))) * ((zz ? 0.0 : U_(0, 0, q) - U_(0, 0, q - 1)) / dzf);
            };
            const double vadv = (0.5 * (Z(0, dzf0) + Z(1, dzf1))) / Az;
            const bool zk = inactive_c(c00, k, Nz) || inactive_c(cm0, k, Nz);
            const double bern = (zk ? 0.0 : Kh(0, 0) - Kh(-1, 0)) / dx;
            double G = -((hadv + vadv) + bern);
            if (eta) G -= gex;
            Gu[o] = G;
        }
        {   // ---- v
            auto n = [&](int b) { return 0.5 * (dy * U_(0, b, 0) + dy * U_(1, b, 0)); };
            const double z10 = zeta(1, 0, vp0, v00, up0, upm);
            const double hadv = (0.5 * (z00 + z10)) * (0.5 * (n(-1) + n(0))) / dy;
            auto Z = [&](int q, double dzf) {
                const bool zz = inactive_c(v00, k + q, Nz) || inactive_c(v00, k + q - 1, Nz);
                return (0.5 * (Az * W_(0, -1, q) + Az * W_(0, 0, q))) * ((zz ? 0.0 : V_(0, 0, q) - V_(0, 0, q - 1)) / dzf);
            };
            const double vadv = (0.5 * (Z(0, dzf0) + Z(1, dzf1))) / Az;
            const bool zk = inactive_c(c00, k, Nz) || inactive_c(c0m, k, Nz);
            const double bern = (zk ? 0.0 : Kh(0, 0) - Kh(0, -1)) / dy;
            double G = -((hadv + vadv) + bern);
            if (eta) G -= gey;
            Gv[o] = G;
        }
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

// ---- compute_split_explicit_forcing! (compute_slow_tendencies.jl:17-42): Σₖ Δz ifelse(peripheral_node, 0, ab2 G) -------------------------
__global__ __launch_bounds__(256) void forcing_immersed_kernel(GridDev g, const int32_t *__restrict__ kbot, const double *__restrict__ Gun,
                                                               const double *__restrict__ Gum, const double *__restrict__ Gvn,
                                                               const double *__restrict__ Gvm, double chi, double *__restrict__ GU,
                                                               double *__restrict__ GV)
{
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x, j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    if (i > g.Nx || j > g.Ny) return;
    const Lay L = make_lay(g, OCN_LOC_CCC);
    const long long e = plane_at(g, i, j), sx = g.Nx + 2 * g.Hx;
    const int kc = kbot[e], mxu = imax(kbot[e - 1], kc), mxv = imax(kbot[e - sx], kc), Nz = g.Nz;
    const double C1 = 3 * 1.0 / 2 + chi, C2 = 1.0 / 2 + chi, ne = (C2 != 0) ? 1.0 : 0.0;
    long long o = at(L, i, j, 1);
    double aU = 0.0, aV = 0.0;
    for (int k = 1; k <= Nz; ++k) {
        const double dz = dz_centre(g, k);
        const double tu = dz * (ic(mxu, k, Nz) ? 0.0 : C1 * Gun[o] - C2 * Gum[o] * ne);
        const double tv = dz * (ic(mxv, k, Nz) ? 0.0 : C1 * Gvn[o] - C2 * Gvm[o] * ne);
        aU = k == 1 ? tu : aU + tu;
        aV = k == 1 ? tv : aV + tv;
        o += L.s3;
    }
    GU[e] = aU;
    GV[e] = aV;
}

// ---- _split_explicit_free_surface! (step_split_explicit_free_surface.jl:11-18): the transports through conditional_U_fcc / V_cfc
// (conditional_differences.jl:83-90), 0 on a peripheral node at k = Nz (a dry column on either side) ------------------------------------
__global__ __launch_bounds__(256) void split_explicit_eta_immersed_kernel(GridDev g, const int32_t *__restrict__ kbot, double dtau,
                                                                          double *__restrict__ eta, const double *__restrict__ U,
                                                                          const double *__restrict__ V)
{
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x, j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    if (i > g.Nx || j > g.Ny) return;
    const int ip = i == g.Nx ? 1 : i + 1, jp = j == g.Ny ? 1 : j + 1, Nz = g.Nz;
    const double dx = g.dx, dy = g.dy, Az = dx * dy;
    const long long e = plane_at(g, i, j), sx = g.Nx + 2 * g.Hx;
    const int kc = kbot[e];
    const bool pw = ic(imax(kbot[e - 1], kc), Nz, Nz), pe = ic(imax(kc, kbot[e + 1]), Nz, Nz);
    const bool ps = ic(imax(kbot[e - sx], kc), Nz, Nz), pn = ic(imax(kc, kbot[e + sx]), Nz, Nz);
    const double dU = (pe ? 0.0 : dy * U[plane_at(g, ip, j)]) - (pw ? 0.0 : dy * U[e]);
    const double dV = (pn ? 0.0 : dx * V[plane_at(g, i, jp)]) - (ps ? 0.0 : dx * V[e]);
    eta[e] = eta[e] - dtau * (dU + dV) / Az;
}
// _split_explicit_barotropic_velocity! (:20-48): ∂xTᶠᶜᶠ η, ∂yTᶜᶠᶠ η are 0 when one of the two (c, c, f) nodes at k = Nz + 1 is inactive
// (conditional_differences.jl:86-87); the column depths are the planes Hᶠᶜ, Hᶜᶠ
__global__ __launch_bounds__(256) void split_explicit_velocity_immersed_kernel(GridDev g, const int32_t *__restrict__ kbot,
                                                                               const double *__restrict__ Hfc, const double *__restrict__ Hcf,
                                                                               double w, double dtau, double grav, const double *__restrict__ eta,
                                                                               double *__restrict__ U, double *__restrict__ V,
                                                                               double *__restrict__ etab, double *__restrict__ Ub,
                                                                               double *__restrict__ Vb, const double *__restrict__ GU,
                                                                               const double *__restrict__ GV)
{
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x, j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    if (i > g.Nx || j > g.Ny) return;
    const int im = i == 1 ? g.Nx : i - 1, jm = j == 1 ? g.Ny : j - 1, Nz = g.Nz;
    const long long e = plane_at(g, i, j), sx = g.Nx + 2 * g.Hx;
    const bool dc = inactive_f_top(kbot[e], Nz), dw = inactive_f_top(kbot[e - 1], Nz), ds = inactive_f_top(kbot[e - sx], Nz);
    const double et = eta[e];
    const double dex = (dc || dw) ? 0.0 : (et - eta[plane_at(g, im, j)]) / g.dx;
    const double dey = (dc || ds) ? 0.0 : (et - eta[plane_at(g, i, jm)]) / g.dy;
    const double Un = U[e] + dtau * (-grav * Hfc[e] * dex + GU[e]);
    const double Vn = V[e] + dtau * (-grav * Hcf[e] * dey + GV[e]);
    etab[e] += w * et;
    Ub[e] += w * Un;
    Vb[e] += w * Vn;
    U[e] = Un;
    V[e] = Vn;
}

// ---- _barotropic_split_explicit_corrector! (barotropic_split_explicit_corrector.jl:70-81): u += (U - U̅) / Hᶠᶜ.  On a dry face Hᶠᶜ = 0 and
// U = U̅ = 0: the reference writes 0 / 0 there, and so does this; the face is peripheral, the next mask removes it ------------------------
__global__ __launch_bounds__(256) void corrector_immersed_kernel(GridDev g, const double *__restrict__ Hfc, const double *__restrict__ Hcf,
                                                                 double *__restrict__ u, double *__restrict__ v, const double *__restrict__ U,
                                                                 const double *__restrict__ V, const double *__restrict__ Ub,
                                                                 const double *__restrict__ Vb)
{
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x, j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    if (i > g.Nx || j > g.Ny) return;
    const int k0 = 1 + blockIdx.z * KZ, k1 = imin(k0 + KZ - 1, g.Nz);
    const Lay L = make_lay(g, OCN_LOC_CCC);
    const long long e = plane_at(g, i, j);
    const double du = (U[e] - Ub[e]) / Hfc[e], dv = (V[e] - Vb[e]) / Hcf[e];
    for (int k = k0; k <= k1; ++k) {
        const long long o = at(L, i, j, k);
        u[o] = u[o] + du;
        v[o] = v[o] + dv;
    }
}

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
int launch_vector_invariant_immersed(const ocn_grid *grid, const int32_t *kbot, const double *u, const double *v, const double *w, double *Gu,
                                     double *Gv, const double *eta, double grav, hipStream_t stream)
{
    GridDev g = to_dev(*grid);
    hipLaunchKernelGGL(vector_invariant_immersed_kernel, xy_blocks(g.Nx, g.Ny, z_chunks(g.Nz)), dim3(64, 4, 1), 0, stream, g, kbot, u, v, w, Gu, Gv,
                       eta, grav);
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
int launch_split_explicit_forcing_immersed(const ocn_grid *grid, const int32_t *kbot, const double *Gun, const double *Gum, const double *Gvn,
                                           const double *Gvm, double chi, double *GU, double *GV, hipStream_t stream)
{
    GridDev g = to_dev(*grid);
    hipLaunchKernelGGL(forcing_immersed_kernel, xy_blocks(g.Nx, g.Ny), dim3(64, 4, 1), 0, stream, g, kbot, Gun, Gum, Gvn, Gvm, chi, GU, GV);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}
int launch_split_explicit_substeps_immersed(const ocn_grid *grid, const int32_t *kbot, const double *Hfc, const double *Hcf, int n,
                                            const double *weights, double dtau, double grav, double *eta, double *U, double *V, double *etab,
                                            double *Ub, double *Vb, const double *GU, const double *GV, hipStream_t stream)
{
    GridDev g = to_dev(*grid);
    const size_t bytes = (size_t)(g.Nx + 2 * g.Hx) * (g.Ny + 2 * g.Hy) * sizeof(double);
    for (double *f : {etab, Ub, Vb}) OCN_CHECK_HIP(hipMemsetAsync(f, 0, bytes, stream));  // initialize_free_surface_state!
    const dim3 block(64, 4, 1), nb = xy_blocks(g.Nx, g.Ny);
    for (int m = 0; m < n; ++m) {
        hipLaunchKernelGGL(split_explicit_eta_immersed_kernel, nb, block, 0, stream, g, kbot, dtau, eta, U, V);
        hipLaunchKernelGGL(split_explicit_velocity_immersed_kernel, nb, block, 0, stream, g, kbot, Hfc, Hcf, weights[m], dtau, grav, eta, U, V, etab,
                           Ub, Vb, GU, GV);
    }
    OCN_CHECK_HIP(hipGetLastError());
    // _update_split_explicit_state!: η, U, V <- their averages
    OCN_CHECK_HIP(hipMemcpyAsync(eta, etab, bytes, hipMemcpyDeviceToDevice, stream));
    OCN_CHECK_HIP(hipMemcpyAsync(U, Ub, bytes, hipMemcpyDeviceToDevice, stream));
    OCN_CHECK_HIP(hipMemcpyAsync(V, Vb, bytes, hipMemcpyDeviceToDevice, stream));
    return OCN_SUCCESS;
}
int launch_barotropic_corrector_immersed(const ocn_grid *grid, const double *Hfc, const double *Hcf, double *u, double *v, const double *U,
                                         const double *V, double *Ub, double *Vb, hipStream_t stream)
{
    // integrate_barotropic_mode! (:13-37): on a static grid σ = 1, also where h = 0, and u, v have just been masked: the plain column sums
    OCN_TRY(launch_barotropic_mode(grid, u, v, Ub, Vb, stream));
    GridDev g = to_dev(*grid);
    hipLaunchKernelGGL(corrector_immersed_kernel, xy_blocks(g.Nx, g.Ny, z_chunks(g.Nz)), dim3(64, 4, 1), 0, stream, g, Hfc, Hcf, u, v, U, V, Ub, Vb);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

}  // namespace ocn
