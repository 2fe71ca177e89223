// hydrostatic_surface.hip -- the free-surface and vector-invariant kernels of HydrostaticFreeSurfaceModel on regular x and y, one set for
// every horizontal topology it runs on: (Periodic, Periodic, Bounded), (Periodic, Bounded, Bounded) channels and (Bounded, Bounded, Bounded)
// basins.  The periodic-only variants (AB3 and blocked substepping, slab-x ranks, the fused corrector) are in kernels.hip.
//
// The topology is a template parameter <BX, BY> (Bounded x, Bounded y).  Along a Bounded direction a Face field has one more point, so u has
// a longer row (Bounded x) and v one more row per plane (Bounded y); w and the centre fields share their x / y extents: every location has
// its own parent layout (HLay).  The planes follow: η is (Center, Center), U, U̅, Gᵁ, Qu are shaped like u and V, V̅, Gⱽ, Qv like v.  Without
// a wall, <false, false>, the three layouts are one: Periodic x (or the FullyConnected x of a slab rank, whose interior arithmetic is the
// same) and Periodic y.
//
// Ranges: every kernel runs over the reference's 1:Nx, 1:Ny(, 1:Nz) (launch!(..., :xyz) / :xy without exclude_periphery), which includes
// the WEST / SOUTH wall face (index 1) and not the east / north one (index N + 1).  The wall-normal velocity on both wall faces is reset
// by the halo fill of update_state! (fill_open_boundary_regions!, fill_halo_regions_open.jl:65-70), not here.
// The differences across a wall are the topology-aware operators of Operators/topology_aware_operators.jl:40-56.
//
// The bottom is a second compile-time parameter of the five kernels that meet it, next to <BX, BY>: the pack B is empty over
// a flat bottom -- the kernel then has no argument for it, every predicate is a compile-time false and the column depth is the number H --
// or it is Bottom, the GridFittedBottom of an ImmersedBoundaryGrid, whose kernel takes the kbot and depth planes as one more argument and
// applies the reference's immersed rules in the same evaluation order, so that over a flat bottom both return the same bits:
//   * conditional differences   ImmersedBoundaries/conditional_differences.jl:25-90: a difference is 0 when one of its two nodes is an
//                               immersed_inactive_node, otherwise the underlying grid's
//   * split-explicit surface    SplitExplicitFreeSurfaces/*.jl with static_column_depth (grid_fitted_bottom.jl:147-150)
// Only <false, false, Bottom> is instantiated: bathymetry on a (Periodic, Periodic, Bounded) grid (validate_immersed of capi.hip).
#include <type_traits>

#include "ocn_common.h"
#include "ocn_immersed.h"
#include "ocn_internal.h"

namespace ocn {

namespace {

template <bool BX, bool BY>
struct HLay {
    Lay c, u, v;  // c: centre fields and (x / y extents, plane stride) w
};
template <bool BX, bool BY>
__host__ __device__ inline HLay<BX, BY> hlay(const GridDev &g)
{
    if constexpr (!BX && !BY) {  // one layout: the kernels carry one set of strides
        const Lay c = make_lay(g, OCN_LOC_CCC);
        return {c, c, c};
    } else {
        return {make_lay(g, OCN_LOC_CCC), make_lay(g, OCN_LOC_FCC), make_lay(g, OCN_LOC_CFC)};
    }
}

// topology dispatch of a launch: F is a generic lambda taking std::integral_constant<bool, BX>, <bool, BY> (which convert to their value
// in a constant expression: kernel<bx, by>)
template <class F>
inline void dispatch_walls(const ocn_grid *grid, F f)
{
    // (the C ABI admits these three: validate_hydrostatic; a slab rank's FullyConnected x is not a wall either)
    if (grid->ty != OCN_BOUNDED) f(std::false_type{}, std::false_type{});
    else if (grid->tx == OCN_BOUNDED) f(std::true_type{}, std::true_type{});
    else f(std::false_type{}, std::true_type{});
}
// ... and of the bottom: F also takes the pack of kernel arguments that the bottom adds, none or the Bottom (kernel<bx, by, decltype(b)...>)
template <class F>
inline void dispatch_bottom(const ocn_grid *grid, const Bottom &bottom, F f)
{
    if (bottom.fitted()) f(std::false_type{}, std::false_type{}, bottom);
    else dispatch_walls(grid, f);
}

// What a thread knows of the bottom under the 3 x 3 columns around its own: the node predicates of the immersed rules, at the u node
// (Face, Center), the v node (Center, Face) or the cell of column (i + a, j + b) and level k.  Over a flat bottom nothing, and every
// predicate is a compile-time false: zero_if(false, x) is x.
struct FlatColumns {
    static constexpr bool inactive_u(int, int, int) { return false; }
    static constexpr bool inactive_v(int, int, int) { return false; }
    static constexpr bool inactive_cell(int, int, int) { return false; }
    static constexpr bool peripheral_u(int, int, int) { return false; }
    static constexpr bool peripheral_v(int, int, int) { return false; }
    static constexpr bool dry(int, int) { return false; }
};
// Over a fitted bottom kbot of the nine columns, in registers; this is the only place where the min / max combinations are formed
struct FittedColumns {
    Cols c;
    int Nz;
    __device__ __forceinline__ bool inactive_u(int a, int b, int k) const { return inactive_c(imin(c(a - 1, b), c(a, b)), k, Nz); }
    __device__ __forceinline__ bool inactive_v(int a, int b, int k) const { return inactive_c(imin(c(a, b - 1), c(a, b)), k, Nz); }
    __device__ __forceinline__ bool inactive_cell(int a, int b, int k) const { return inactive_c(c(a, b), k, Nz); }
    // (at 1 <= k <= Nz, where the kernels ask: inactive_cell of the immersed grid alone)
    __device__ __forceinline__ bool peripheral_u(int a, int b, int k) const { return ic(imax(c(a - 1, b), c(a, b)), k, Nz); }
    __device__ __forceinline__ bool peripheral_v(int a, int b, int k) const { return ic(imax(c(a, b - 1), c(a, b)), k, Nz); }
    __device__ __forceinline__ bool dry(int a, int b) const { return inactive_f_top(c(a, b), Nz); }
};
__device__ __forceinline__ FlatColumns columns(const GridDev &, int, int) { return {}; }
__device__ __forceinline__ FittedColumns columns(const GridDev &g, int i, int j, const Bottom &b) { return {load_cols(g, b.kbot, i, j), g.Nz}; }
__device__ __forceinline__ double zero_if(bool p, double x) { return p ? 0.0 : x; }
// static_column_depthᶠᶜᵃ / ᶜᶠᵃ at plane index e: the number H over a flat bottom, the planes Hᶠᶜ, Hᶜᶠ of a fitted one
__device__ __forceinline__ double depth_fc(double H, long long) { return H; }
__device__ __forceinline__ double depth_cf(double H, long long) { return H; }
__device__ __forceinline__ double depth_fc(double, long long e, const Bottom &b) { return b.Hfc[e]; }
__device__ __forceinline__ double depth_cf(double, long long e, const Bottom &b) { return b.Hcf[e]; }
// The levels of a thread: the one of its block over a flat bottom; over a fitted one KZ levels, with the columns' kbot in registers:
//     int k = first_level<B...>();  [before the thread may leave]  ...  do { the cell at level k } while (next_level<B...>(g, k));
// (over a flat bottom the condition is a compile-time false and the body straight-line code, as it always was: around a lambda, an inlined
// function or a for loop of one iteration the compiler orders the flat kernels' code differently)
template <class... B>
constexpr int levels_per_thread = sizeof...(B) ? KZ : 1;
template <class... B>
__device__ __forceinline__ int first_level() { return 1 + blockIdx.z * levels_per_thread<B...>; }
template <class... B>
__device__ __forceinline__ bool next_level(const GridDev &g, int &k)
{
    if constexpr (levels_per_thread<B...> == 1) return false;
    else return k % KZ != 0 && ++k <= g.Nz;
}

// _compute_w_from_continuity! (src/Models/HydrostaticFreeSurfaceModels/compute_w_from_continuity.jl:31-40): w[i,j,1] = 0,
// w[i,j,k] = w[i,j,k-1] - (flux_div_xyᶜᶜᶜ(i,j,k-1,u,v) / Azᶜᶜᶜ + 0) for every column whose east / north neighbours exist in the
// parents (a superset of w_kernel_parameters, :43-51).  One thread per column, i across the lanes.
template <bool BX, bool BY>
__global__ __launch_bounds__(256) void w_from_continuity_kernel(GridDev g, const double *__restrict__ u, const double *__restrict__ v,
                                                                double *__restrict__ w)
{
    const int i = 1 - g.Hx + blockIdx.x * blockDim.x + threadIdx.x, j = 1 - g.Hy + blockIdx.y * blockDim.y + threadIdx.y;
    if (i > g.Nx + g.Hx - 1 || j > g.Ny + g.Hy - 1) return;
    const HLay<BX, BY> L = hlay<BX, BY>(g);
    long long ow = at(L.c, i, j, 1), ou = at(L.u, i, j, 1), ov = at(L.v, i, j, 1);
    const double Az = g.dx * g.dy;
    double wk = 0.0;
    w[ow] = wk;
    for (int k = 1; k <= g.Nz; ++k) {
        const double dzc = dz_centre(g, k);
        const double Ax = g.dy * dzc, Ay = g.dx * dzc;
        const double dxu = Ax * u[ou + 1] - Ax * u[ou];
        const double dyv = Ay * v[ov + L.v.s2] - Ay * v[ov];
        const double dh = (dxu + dyv) / Az;
        wk = wk - (dh + 0.0);
        ow += L.c.s3; ou += L.u.s3; ov += L.v.s3;
        w[ow] = wk;
    }
}

// Gu = -U_dot_∇u, Gv = -U_dot_∇v of the reference's default VectorInvariant() scheme (Advection/vector_invariant_advection.jl:
// 269-275): EnstrophyConserving vorticity flux (:360-361, ζ₃ᶠᶠᶜ of Operators/vorticity_operators.jl:4-11), EnergyConserving
// vertical advection (:315-319) and kinetic-energy gradient (:304-308).  ℑ = 0.5 (a + b), δ = a - b, ∂ = δ / Δ; one thread per cell.
// ζ at the wall corners and the interpolations next to a wall read the filled halos of u and v (no-flux / Value halos of the tangential
// component, zero wall faces of the normal one), as the reference's operators do on a Bounded grid.
// eta != NULL: the barotropic pressure gradient - g ∇η (eta_gradient_kernel below) is subtracted in the same pass.
// Over a fitted bottom the conditional differences: the two differences of ζ₃ᶠᶠᶜ, ∂z u / ∂z v of the vertical advection, ∂x / ∂y of Kh.
// g ∂x η is taken at k = Nz + 1, where the centre node is inactive on the underlying grid as well: never zeroed.
template <bool BX, bool BY, class... B>
__global__ __launch_bounds__(256) void vector_invariant_kernel(GridDev g, B... bottom, const double *__restrict__ u, const double *__restrict__ v,
                                                               const double *__restrict__ w, double *__restrict__ Gu,
                                                               double *__restrict__ Gv, const double *__restrict__ eta, double grav)
{
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x, j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    int k = first_level<B...>();
    if (i > g.Nx || j > g.Ny) return;
    const auto col = columns(g, i, j, bottom...);
    const HLay<BX, BY> L = hlay<BX, BY>(g);
    do {
        const long long ou = at(L.u, i, j, k), ov = at(L.v, i, j, k);
        const double dx = g.dx, dy = g.dy, Az = dx * dy;
        const double dzf0 = dz_face(g, k), dzf1 = dz_face(g, k + 1);  // Δzᶠ at faces k, k+1
        const double *pu = u + ou, *pv = v + ov, *pw = w + at(L.c, i, j, k);
#define U_(a, b, q) pu[(a) + (b)*L.u.s2 + (q)*L.u.s3]
#define V_(a, b, q) pv[(a) + (b)*L.v.s2 + (q)*L.v.s3]
#define W_(a, b, q) pw[(a) + (b)*L.c.s2 + (q)*L.c.s3]
        // ζ₃ᶠᶠᶜ at (i + a, j + b): δxᶠᶠᶜ(Δy v) is 0 when one of its two v nodes is inactive, δyᶠᶠᶜ(Δx u) when one of its two u nodes is
        auto zeta = [&](int a, int b) {
            const double dv = zero_if(col.inactive_v(a, b, k) || col.inactive_v(a - 1, b, k), dy * V_(a, b, 0) - dy * V_(a - 1, b, 0));
            const double du = zero_if(col.inactive_u(a, b, k) || col.inactive_u(a, b - 1, k), dx * U_(a, b, 0) - dx * U_(a, b - 1, 0));
            const double gam = dv - du;
            return gam / Az;
        };
        auto Kh = [&](int a, int b) {    // Khᶜᶜᶜ at (i + a, j + b)
            return (0.5 * (U_(a, b, 0) * U_(a, b, 0) + U_(a + 1, b, 0) * U_(a + 1, b, 0)) +
                    0.5 * (V_(a, b, 0) * V_(a, b, 0) + V_(a, b + 1, 0) * V_(a, b + 1, 0))) / 2;
        };
        {   // ---- u
            auto m = [&](int a) { return 0.5 * (dx * V_(a, 0, 0) + dx * V_(a, 1, 0)); };  // ℑyᵃᶜᵃ(Δx_qᶜᶠᶜ v) at (i + a, j)
            const double hadv = -(0.5 * (zeta(0, 0) + zeta(0, 1))) * (0.5 * (m(-1) + m(0))) / dx;
            auto Z = [&](int q, double dzf) {  // ζ₂wᶠᶜᶠ at face k + q: ∂zᶠᶜᶠ u is 0 when u at k + q or at k + q - 1 is inactive
                const bool zz = col.inactive_u(0, 0, k + q) || col.inactive_u(0, 0, k + q - 1);
                return (0.5 * (Az * W_(-1, 0, q) + Az * W_(0, 0, q))) * (zero_if(zz, U_(0, 0, q) - U_(0, 0, q - 1)) / dzf);
            };
            const double vadv = (0.5 * (Z(0, dzf0) + Z(1, dzf1))) / Az;
            const double bern = zero_if(col.inactive_cell(0, 0, k) || col.inactive_cell(-1, 0, k), Kh(0, 0) - Kh(-1, 0)) / dx;
            double G = -((hadv + vadv) + bern);
            if (eta) {  // (the plane index where it is used, not up front: it would be live, in registers, across both halves)
                const long long e = plane_at(g, L.c, i, j);
                G -= grav * ((eta[e] - eta[e - 1]) / g.dx);
            }
            Gu[ou] = G;
        }
        {   // ---- v
            auto n = [&](int b) { return 0.5 * (dy * U_(0, b, 0) + dy * U_(1, b, 0)); };  // ℑxᶜᵃᵃ(Δy_qᶠᶜᶜ u) at (i, j + b)
            const double hadv = (0.5 * (zeta(0, 0) + zeta(1, 0))) * (0.5 * (n(-1) + n(0))) / dy;
            auto Z = [&](int q, double dzf) {
                const bool zz = col.inactive_v(0, 0, k + q) || col.inactive_v(0, 0, k + q - 1);
                return (0.5 * (Az * W_(0, -1, q) + Az * W_(0, 0, q))) * (zero_if(zz, V_(0, 0, q) - V_(0, 0, q - 1)) / dzf);
            };
            const double vadv = (0.5 * (Z(0, dzf0) + Z(1, dzf1))) / Az;
            const double bern = zero_if(col.inactive_cell(0, 0, k) || col.inactive_cell(0, -1, k), Kh(0, 0) - Kh(0, -1)) / dy;
            double G = -((hadv + vadv) + bern);
            if (eta) {
                const long long e = plane_at(g, L.c, i, j);
                G -= grav * ((eta[e] - eta[e - L.c.sx]) / g.dy);
            }
            Gv[ov] = G;
        }
#undef U_
#undef V_
#undef W_
    } while (next_level<B...>(g, k));
}

// Gu -= g ∂xᶠᶜᶜ η, Gv -= g ∂yᶜᶠᶜ η at every k (explicit_free_surface.jl:36-40); MODE 1: u -= g Δt ∂xᶠᶜᶠ η
// (barotropic_pressure_correction.jl:40-47).  η is the plane k = Nz+1 of the reference's reduced field, halos filled; on a wall face the
// no-flux halo of η makes the difference 0.
template <bool BX, bool BY, int MODE>
__global__ __launch_bounds__(256) void eta_gradient_kernel(GridDev g, double grav, double dt, const double *__restrict__ eta,
                                                           double *__restrict__ a, double *__restrict__ b)
{
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x, j = 1 + blockIdx.y * blockDim.y + threadIdx.y, k = 1 + blockIdx.z;
    if (i > g.Nx || j > g.Ny) return;
    const HLay<BX, BY> L = hlay<BX, BY>(g);
    const long long e = plane_at(g, L.c, i, j), ou = at(L.u, i, j, k), ov = at(L.v, i, j, k);
    if (MODE == 0) {
        a[ou] -= grav * ((eta[e] - eta[e - 1]) / g.dx);
        b[ov] -= grav * ((eta[e] - eta[e - L.c.sx]) / g.dy);
    } else {
        a[ou] -= grav * dt * ((eta[e] - eta[e - 1]) / g.dx);
        b[ov] -= grav * dt * ((eta[e] - eta[e - L.c.sx]) / g.dy);
    }
}

// fill_halo_regions! of η, a (Center, Center) plane with the default conditions (field_boundary_conditions.jl:15-33): a Bounded direction
// is no-flux, which copies the boundary cell into the FIRST halo cell over the interior extent of the other direction
// (fill_halo_regions_flux.jl:14-31); a Periodic direction wraps over the whole parent extent of the other direction and is filled last
// (fill_halo_regions.jl:50-68), so it also copies the halo rows of the Bounded direction, filled or not.  Halo cells beyond the first one
// of a Bounded direction are otherwise not written, nor are the corners of a basin, as in the reference; without a wall every halo cell
// copies from the interior cell it wraps to, corners included.  No cell that is read is written: one launch.
template <bool BX, bool BY>
__global__ void plane_halo_kernel(int Nx, int Ny, int Hx, int Hy, double *__restrict__ e)
{
    const int sx = Nx + 2 * Hx, sy = Ny + 2 * Hy;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)sx * sy) return;
    const int I = (int)(t % sx), J = (int)(t / sx);
    const bool in_x = I >= Hx && I < Hx + Nx, in_y = J >= Hy && J < Hy + Ny;
    if (in_x && in_y) return;
    int si = I, sj = J;
    if (!in_x) {
        if (BX) {
            if (!in_y) return;  // a wall fill covers the interior extent of the other direction
            if (I == Hx - 1) si = Hx;
            else if (I == Hx + Nx) si = Hx + Nx - 1;
            else return;
        } else {
            si = Hx + ((I - Hx) % Nx + Nx) % Nx;
        }
    }
    if (!in_y) {
        if (BY) {
            if (J == Hy - 1 && in_x) sj = Hy;
            else if (J == Hy + Ny && in_x) sj = Hy + Ny - 1;
            else if (in_x || BX) return;  // (a Periodic x copies along this row, whatever it holds: sj = J)
            else if (J == Hy - 1) sj = Hy;          // ... the row the wall fill has filled: the value it was filled from
            else if (J == Hy + Ny) sj = Hy + Ny - 1;
        } else {
            sj = Hy + ((J - Hy) % Ny + Ny) % Ny;
        }
    }
    e[t] = e[si + (long long)sx * sj];
}

// compute_split_explicit_forcing! (compute_slow_tendencies.jl:12-32), FORCING = 1: Gᵁ = Σₖ Δz ((3/2 + χ) Guⁿ - (1/2 + χ) Gu⁻ not_euler);
// integrate_barotropic_mode! on a static grid (σ = 1, barotropic_split_explicit_corrector.jl:13-32), FORCING = 0: Σₖ Δz u σ.
// A u-shaped and a v-shaped field into their planes; the first level starts the sum (no 0 + ...).
// Over a fitted bottom (compute_slow_tendencies.jl:17-42): Σₖ Δz ifelse(peripheral_node, 0, ab2 G).
template <bool BX, bool BY, int FORCING, class... B>
__global__ __launch_bounds__(256) void column_sum_kernel(GridDev g, B... bottom, const double *__restrict__ un, const double *__restrict__ um,
                                                         const double *__restrict__ vn, const double *__restrict__ vm, double chi,
                                                         double *__restrict__ U, double *__restrict__ V)
{
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x, j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    if (i > g.Nx || j > g.Ny) return;
    const auto col = columns(g, i, j, bottom...);
    const HLay<BX, BY> L = hlay<BX, BY>(g);
    const double C1 = 3 * 1.0 / 2 + chi, C2 = 1.0 / 2 + chi, ne = (C2 != 0) ? 1.0 : 0.0;
    long long ou = at(L.u, i, j, 1), ov = at(L.v, i, j, 1);
    double aU = 0.0, aV = 0.0;
    for (int k = 1; k <= g.Nz; ++k) {
        const double dz = dz_centre(g, k);
        // (not zero_if: the conditional operator keeps the two loads of a peripheral node behind a branch, and the column sum over a
        // fitted bottom is 6 % faster with the branch than with loads and a select: DESIGN §5.2v)
        const double tu = FORCING ? dz * (col.peripheral_u(0, 0, k) ? 0.0 : C1 * un[ou] - C2 * um[ou] * ne) : dz * un[ou] * 1.0;
        const double tv = FORCING ? dz * (col.peripheral_v(0, 0, k) ? 0.0 : C1 * vn[ov] - C2 * vm[ov] * ne) : dz * vn[ov] * 1.0;
        aU = k == 1 ? tu : aU + tu;
        aV = k == 1 ? tv : aV + tv;
        ou += L.u.s3; ov += L.v.s3;
    }
    U[plane_at(g, L.u, i, j)] = aU;
    V[plane_at(g, L.v, i, j)] = aV;
}

// ---- SplitExplicitFreeSurface (SplitExplicitFreeSurfaces/*.jl), ForwardBackwardScheme, static grid of column depth H.  Only the interiors
// of the planes are used: indices wrap along a Periodic direction, and across a wall the operators are δxTᶜᵃᵃ / δyTᵃᶜᵃ and ∂xTᶠᶜᶠ / ∂yTᶜᶠᶠ.
// _split_explicit_free_surface! (step_split_explicit_free_surface.jl:12-20): η -= Δτ (δx(Δy U) + δy(Δx V)) / Az.  Across a wall
// (topology_aware_operators.jl:35-56) the transport is zero -- at i = Nx the difference is -f(Nx), at i = 1 it is f(2) -- whatever the
// wall faces of U hold.  Over a fitted bottom the transports go through conditional_U_fcc / V_cfc (conditional_differences.jl:83-90): 0 on
// a peripheral node at k = Nz (a dry column on either side)
template <bool BX, bool BY, class... B>
__global__ __launch_bounds__(256) void split_explicit_eta_kernel(GridDev g, B... bottom, double dtau, double *__restrict__ eta,
                                                                 const double *__restrict__ U, const double *__restrict__ V)
{
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x, j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    if (i > g.Nx || j > g.Ny) return;
    const HLay<BX, BY> L = hlay<BX, BY>(g);
    const double dx = g.dx, dy = g.dy, Az = dx * dy;
    const long long e = plane_at(g, L.c, i, j), eu = plane_at(g, L.u, i, j), ev = plane_at(g, L.v, i, j);
    const auto col = columns(g, i, j, bottom...);
    auto Uw = [&] { return zero_if(col.peripheral_u(0, 0, g.Nz), dy * U[eu]); };  // the transports through the four faces of the column
    auto Ue = [&](long long east) { return zero_if(col.peripheral_u(1, 0, g.Nz), dy * U[east]); };
    auto Vs = [&] { return zero_if(col.peripheral_v(0, 0, g.Nz), dx * V[ev]); };
    auto Vn = [&](long long north) { return zero_if(col.peripheral_v(0, 1, g.Nz), dx * V[north]); };
    double dU, dV;
    if (BX) dU = i == g.Nx ? -Uw() : (i == 1 ? Ue(eu + 1) : Ue(eu + 1) - Uw());
    else dU = Ue(plane_at(g, L.u, i == g.Nx ? 1 : i + 1, j)) - Uw();
    if (BY) dV = j == g.Ny ? -Vs() : (j == 1 ? Vn(ev + L.v.sx) : Vn(ev + L.v.sx) - Vs());
    else dV = Vn(plane_at(g, L.v, i, j == g.Ny ? 1 : j + 1)) - Vs();
    eta[e] = eta[e] - dtau * (dU + dV) / Az;
}
// _split_explicit_barotropic_velocity! (:22-46): U += Δτ (-g H ∂x η + Gᵁ), V likewise; the filtered state accumulates weight x (η, U, V).
// ∂xTᶠᶜᶠ / ∂yTᶜᶠᶠ (topology_aware_operators.jl:32-44, 66-67) are zero on a wall face, and over a fitted bottom when one of the two
// (c, c, f) nodes at k = Nz + 1 is inactive (conditional_differences.jl:86-87): a dry column; the column depths are then the planes Hᶠᶜ, Hᶜᶠ
template <bool BX, bool BY, class... B>
__global__ __launch_bounds__(256) void split_explicit_velocity_kernel(GridDev g, B... bottom, double w, double dtau, double grav, double H,
                                                                      const double *__restrict__ eta, double *__restrict__ U,
                                                                      double *__restrict__ V, double *__restrict__ etab,
                                                                      double *__restrict__ Ub, double *__restrict__ Vb,
                                                                      const double *__restrict__ GU, const double *__restrict__ GV)
{
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x, j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    if (i > g.Nx || j > g.Ny) return;
    const HLay<BX, BY> L = hlay<BX, BY>(g);
    const long long e = plane_at(g, L.c, i, j), eu = plane_at(g, L.u, i, j), ev = plane_at(g, L.v, i, j);
    const double et = eta[e];
    double dex, dey;  // (a Periodic direction wraps the INDEX: a select between two offsets becomes a branch around the load)
    if (BX) dex = i == 1 ? 0.0 : et - eta[e - 1];
    else dex = et - eta[plane_at(g, L.c, i == 1 ? g.Nx : i - 1, j)];
    if (BY) dey = j == 1 ? 0.0 : et - eta[e - L.c.sx];
    else dey = et - eta[plane_at(g, L.c, i, j == 1 ? g.Ny : j - 1)];
    const auto col = columns(g, i, j, bottom...);
    dex = zero_if(col.dry(0, 0) || col.dry(-1, 0), dex);
    dey = zero_if(col.dry(0, 0) || col.dry(0, -1), dey);
    const double Un = U[eu] + dtau * (-grav * depth_fc(H, eu, bottom...) * (dex / g.dx) + GU[eu]);
    const double Vn = V[ev] + dtau * (-grav * depth_cf(H, ev, bottom...) * (dey / g.dy) + GV[ev]);
    etab[e] += w * et;
    Ub[eu] += w * Un;
    Vb[ev] += w * Vn;
    U[eu] = Un;
    V[ev] = Vn;
}

// _barotropic_split_explicit_corrector! (barotropic_split_explicit_corrector.jl:57-81): u += (U - U̅) / Hᶠᶜ at every level.  On a dry face
// of a fitted bottom Hᶠᶜ = 0 and U = U̅ = 0: the reference writes 0 / 0 there, and so does this; the face is peripheral, the next mask removes it
template <bool BX, bool BY, class... B>
__global__ __launch_bounds__(256) void barotropic_corrector_kernel(GridDev g, B... bottom, double *__restrict__ u, double *__restrict__ v,
                                                                   const double *__restrict__ U, const double *__restrict__ V,
                                                                   const double *__restrict__ Ub, const double *__restrict__ Vb, double H)
{
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x, j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    int k = first_level<B...>();
    if (i > g.Nx || j > g.Ny) return;
    const HLay<BX, BY> L = hlay<BX, BY>(g);
    do {  // (the division does not depend on k: over a fitted bottom once per column)
        const long long ou = at(L.u, i, j, k), ov = at(L.v, i, j, k), eu = plane_at(g, L.u, i, j), ev = plane_at(g, L.v, i, j);
        u[ou] = u[ou] + (U[eu] - Ub[eu]) / depth_fc(H, eu, bottom...);
        v[ov] = v[ov] + (V[ev] - Vb[ev]) / depth_cf(H, ev, bottom...);
    } while (next_level<B...>(g, k));
}

// ---- ImplicitFreeSurface with the FFT solver (implicit_free_surface.jl:112-145, fft_based_implicit_free_surface_solver.jl:76-115,
// barotropic_pressure_correction.jl:21-47) on a static grid of constant depth Lz.
// compute_vertically_integrated_volume_flux! (compute_vertically_integrated_variables.jl:34-41): Qu = Σₖ Axᶠᶜᶜ u, Qv = Σₖ Ayᶜᶠᶜ v (sum!
// accumulates k ascending from zero) over the whole interior of a Face field, the east / north wall face included (v there is 0 after the
// fill of step_free_surface!, implicit_free_surface.jl:133)
template <bool BX, bool BY>
__global__ __launch_bounds__(256) void volume_flux_kernel(GridDev g, const double *__restrict__ u, const double *__restrict__ v,
                                                          double *__restrict__ Qu, double *__restrict__ Qv)
{
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x, j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    if (i > g.Nx + (BX ? 1 : 0) || j > g.Ny + (BY ? 1 : 0)) return;
    const HLay<BX, BY> L = hlay<BX, BY>(g);
    const bool do_u = !BY || j <= g.Ny, do_v = !BX || i <= g.Nx;
    long long ou = at(L.u, i, j, 1), ov = at(L.v, i, j, 1);
    double aU = 0.0, aV = 0.0;
#pragma unroll 8
    for (int k = 1; k <= g.Nz; ++k) {
        const double dz = dz_centre(g, k);
        if (do_u) aU = aU + (g.dy * dz) * u[ou];
        if (do_v) aV = aV + (g.dx * dz) * v[ov];
        ou += L.u.s3; ov += L.v.s3;
    }
    if (do_u) Qu[plane_at(g, L.u, i, j)] = aU;
    if (do_v) Qv[plane_at(g, L.v, i, j)] = aV;
}
// fft_implicit_free_surface_right_hand_side! (fft_based_implicit_free_surface_solver.jl:104-110): rhs = (δx Qu + δy Qv - Az η / Δt) /
// (g Lz Δt Az) into a halo-free (Nx, Ny) array; flux_div_xyᶜᶜᶠ reads face N + 1 along a Bounded direction and wraps along a Periodic one
template <bool BX, bool BY>
__global__ __launch_bounds__(256) void implicit_rhs_kernel(GridDev g, double grav, double Lz, double dt, const double *__restrict__ Qu,
                                                           const double *__restrict__ Qv, const double *__restrict__ eta,
                                                           double *__restrict__ rhs)
{
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x, j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    if (i > g.Nx || j > g.Ny) return;
    const HLay<BX, BY> L = hlay<BX, BY>(g);
    const int ip = (!BX && i == g.Nx) ? 1 : i + 1, jp = (!BY && j == g.Ny) ? 1 : j + 1;
    const double Az = g.dx * g.dy;
    const double dQ = (Qu[plane_at(g, L.u, ip, j)] - Qu[plane_at(g, L.u, i, j)]) + (Qv[plane_at(g, L.v, i, jp)] - Qv[plane_at(g, L.v, i, j)]);
    rhs[(i - 1) + (long long)g.Nx * (j - 1)] = (dQ - Az * eta[plane_at(g, L.c, i, j)] / dt) / (grav * Lz * dt * Az);
}

inline size_t plane_bytes(const Lay &L) { return (size_t)L.sx * L.sy * sizeof(double); }
// blocks along z of a launch over every level: one per level, or one per KZ levels over a fitted bottom (first_level)
inline int z_blocks(const GridDev &g, const Bottom &bottom) { return bottom.fitted() ? z_chunks(g.Nz) : g.Nz; }

}  // namespace

int launch_w_from_continuity(const ocn_grid *grid, const double *u, const double *v, double *w, hipStream_t stream)
{
    GridDev g = to_dev(*grid);
    dispatch_walls(grid, [&](auto bx, auto by) {
        hipLaunchKernelGGL((w_from_continuity_kernel<bx, by>), xy_blocks(g.Nx + 2 * g.Hx - 1, g.Ny + 2 * g.Hy - 1), dim3(64, 4, 1), 0, stream, g, u,
                           v, w);
    });
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}
int launch_vector_invariant(const ocn_grid *grid, const Bottom &bottom, const double *u, const double *v, const double *w, double *Gu, double *Gv,
                            const double *eta, double grav, hipStream_t stream)
{
    GridDev g = to_dev(*grid);
    const dim3 nb = xy_blocks(g.Nx, g.Ny, z_blocks(g, bottom));
    dispatch_bottom(grid, bottom, [&](auto bx, auto by, auto... b) {
        hipLaunchKernelGGL((vector_invariant_kernel<bx, by, decltype(b)...>), nb, dim3(64, 4, 1), 0, stream, g, b..., u, v, w, Gu, Gv, eta, grav);
    });
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}
int launch_barotropic_gradient(const ocn_grid *grid, double grav, const double *eta, double *Gu, double *Gv, hipStream_t stream)
{
    GridDev g = to_dev(*grid);
    dispatch_walls(grid, [&](auto bx, auto by) {
        hipLaunchKernelGGL((eta_gradient_kernel<bx, by, 0>), xy_blocks(g.Nx, g.Ny, g.Nz), dim3(64, 4, 1), 0, stream, g, grav, 0.0, eta, Gu, Gv);
    });
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}
int launch_barotropic_pressure_correction(const ocn_grid *grid, double *u, double *v, const double *eta, double grav, double dt,
                                          hipStream_t stream)
{
    GridDev g = to_dev(*grid);
    dispatch_walls(grid, [&](auto bx, auto by) {
        hipLaunchKernelGGL((eta_gradient_kernel<bx, by, 1>), xy_blocks(g.Nx, g.Ny, g.Nz), dim3(64, 4, 1), 0, stream, g, grav, dt, eta, u, v);
    });
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}
int launch_plane_halo(const ocn_grid *grid, double *plane, hipStream_t stream)
{
    const long long n = (long long)(grid->Nx + 2 * grid->Hx) * (grid->Ny + 2 * grid->Hy);
    const dim3 nb((unsigned)((n + 255) / 256));
    dispatch_walls(grid, [&](auto bx, auto by) {
        hipLaunchKernelGGL((plane_halo_kernel<bx, by>), nb, dim3(256), 0, stream, grid->Nx, grid->Ny, grid->Hx, grid->Hy, plane);
    });
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}
int launch_split_explicit_forcing(const ocn_grid *grid, const Bottom &bottom, const double *Gun, const double *Gum, const double *Gvn,
                                  const double *Gvm, double chi, double *GU, double *GV, hipStream_t stream)
{
    GridDev g = to_dev(*grid);
    dispatch_bottom(grid, bottom, [&](auto bx, auto by, auto... b) {
        hipLaunchKernelGGL((column_sum_kernel<bx, by, 1, decltype(b)...>), xy_blocks(g.Nx, g.Ny), dim3(64, 4, 1), 0, stream, g, b..., Gun, Gum, Gvn,
                           Gvm, chi, GU, GV);
    });
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}
int launch_barotropic_mode(const ocn_grid *grid, const double *u, const double *v, double *U, double *V, hipStream_t stream)
{
    GridDev g = to_dev(*grid);
    dispatch_walls(grid, [&](auto bx, auto by) {
        hipLaunchKernelGGL((column_sum_kernel<bx, by, 0>), xy_blocks(g.Nx, g.Ny), dim3(64, 4, 1), 0, stream, g, u, u, v, v, 0.0, U, V);
    });
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}
int launch_barotropic_corrector(const ocn_grid *grid, const Bottom &bottom, double *u, double *v, const double *U, const double *V, double *Ub,
                                double *Vb, double H, hipStream_t stream)
{
    // integrate_barotropic_mode! (:13-37): on a static grid σ = 1, also where h = 0, and over a fitted bottom u, v have just been masked:
    // the plain column sums
    OCN_TRY(launch_barotropic_mode(grid, u, v, Ub, Vb, stream));
    GridDev g = to_dev(*grid);
    const dim3 nb = xy_blocks(g.Nx, g.Ny, z_blocks(g, bottom));
    dispatch_bottom(grid, bottom, [&](auto bx, auto by, auto... b) {
        hipLaunchKernelGGL((barotropic_corrector_kernel<bx, by, decltype(b)...>), nb, dim3(64, 4, 1), 0, stream, g, b..., u, v, U, V, Ub, Vb, H);
    });
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}
int launch_split_explicit_substeps(const ocn_grid *grid, const Bottom &bottom, int n, const double *weights, double dtau, double grav, double H,
                                   double *eta, double *U, double *V, double *etab, double *Ub, double *Vb, const double *GU, const double *GV,
                                   hipStream_t stream)
{
    GridDev g = to_dev(*grid);
    const HLay<true, true> L = hlay<true, true>(g);  // (the extents of any topology: make_lay reads them from g)
    const size_t bc = plane_bytes(L.c), bu = plane_bytes(L.u), bv = plane_bytes(L.v);
    OCN_CHECK_HIP(hipMemsetAsync(etab, 0, bc, stream));  // initialize_free_surface_state!
    OCN_CHECK_HIP(hipMemsetAsync(Ub, 0, bu, stream));
    OCN_CHECK_HIP(hipMemsetAsync(Vb, 0, bv, stream));
    const dim3 block(64, 4, 1), nb = xy_blocks(g.Nx, g.Ny);
    dispatch_bottom(grid, bottom, [&](auto bx, auto by, auto... b) {
        for (int m = 0; m < n; ++m) {
            hipLaunchKernelGGL((split_explicit_eta_kernel<bx, by, decltype(b)...>), nb, block, 0, stream, g, b..., dtau, eta, U, V);
            hipLaunchKernelGGL((split_explicit_velocity_kernel<bx, by, decltype(b)...>), nb, block, 0, stream, g, b..., weights[m], dtau, grav, H, eta,
                               U, V, etab, Ub, Vb, GU, GV);
        }
    });
    OCN_CHECK_HIP(hipGetLastError());
    // _update_split_explicit_state!: η, U, V <- their averages (the halos of these planes are not used by the substepping)
    OCN_CHECK_HIP(hipMemcpyAsync(eta, etab, bc, hipMemcpyDeviceToDevice, stream));
    OCN_CHECK_HIP(hipMemcpyAsync(U, Ub, bu, hipMemcpyDeviceToDevice, stream));
    OCN_CHECK_HIP(hipMemcpyAsync(V, Vb, bv, hipMemcpyDeviceToDevice, stream));
    return OCN_SUCCESS;
}
int launch_implicit_free_surface_rhs(const ocn_grid *grid, const double *u, const double *v, const double *eta, double grav, double dt,
                                     double *Qu, double *Qv, double *rhs, hipStream_t stream)
{
    GridDev g = to_dev(*grid);
    const double Lz = grid->Lz;
    const dim3 block(64, 4, 1);
    dispatch_walls(grid, [&](auto bx, auto by) {
        hipLaunchKernelGGL((volume_flux_kernel<bx, by>), xy_blocks(g.Nx + (bx ? 1 : 0), g.Ny + (by ? 1 : 0)), block, 0, stream, g, u, v, Qu, Qv);
        hipLaunchKernelGGL((implicit_rhs_kernel<bx, by>), xy_blocks(g.Nx, g.Ny), block, 0, stream, g, grav, Lz, dt, Qu, Qv, eta, rhs);
    });
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

}  // namespace ocn
