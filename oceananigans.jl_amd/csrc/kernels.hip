// kernels.hip -- bandwidth-bound kernels of the NonhydrostaticModel step (K5-K9, K12-K19, K22-K23).
// Compiled with -ffp-contract=off: these kernels are HBM-bound, so keeping the reference's
// unfused evaluation order costs nothing and makes them bit-identical to the CPU oracle.
#include <chrono>
#include <thread>

#include "ocn_internal.h"

namespace ocn {

// ---------------------------------------------------------------------------------------------------
// Halo fills (fill_halo_regions.jl:50-196, fill_halo_regions_periodic.jl:40-71,
// fill_halo_regions_flux.jl:14-33, fill_halo_regions_open.jl:65-70)
//
// One launch fills every halo cell of every field of the tuple: each halo cell copies from the cell the
// reference's ordered sequence (non-periodic fills first, then periodic fills over the whole parent
// cross-section) would have propagated into it.  Source cells are never written by the same launch.
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ int wrap1(int i, int N) { return i < 1 ? i + N : (i > N ? i - N : i); }

// ZBcTuple (optional, has_bc): Value / Gradient bottom / top conditions replace the no-flux mirror of the first halo
// plane by a linear extrapolation (fill_halo_regions_value_gradient.jl:5-103):
//   ∇c = gradient, or (c¹ - v)/(Δ/2) [bottom], (v - cᴺ)/(Δ/2) [top];   c[0] = c¹ + ∇c*(-Δ),  c[N+1] = cᴺ + ∇c*Δ,
// Δ = Δzᶜᶜᶠ at the boundary face.  x, y halo columns take the value of their periodic image, as the reference's
// later Periodic fills would copy it.
template <int TZ>
__global__ __launch_bounds__(256) void fill_halos_kernel(GridDev g, FieldTuple a, int wrap_x, int only_dir, ZBcTuple zbc, int has_bc)
{
    const int f = blockIdx.y;
    double *__restrict__ c = a.f[f];
    const int loc = a.loc[f];
    const Lay L = make_lay(g, loc);
    const int zface_b = (TZ == OCN_BOUNDED) && (loc & 4);
    const int nzi = L.sz - 2 * g.Hz;  // planes that are not z-halo planes
    const long long A = (long long)L.sx * L.sy * 2 * g.Hz;
    const long long B = (long long)L.sx * 2 * g.Hy * nzi;
    const long long Cn = wrap_x ? (long long)2 * g.Hx * g.Ny * nzi : 0;
    const long long total = A + B + Cn;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        int I, J, K;  // 0-based parent coordinates
        if (t < A) {
            I = t % L.sx;
            long long q = t / L.sx;
            J = q % L.sy;
            int kk = q / L.sy;  // 0..2Hz-1
            K = kk < g.Hz ? kk : kk - g.Hz + (L.sz - g.Hz);
        } else if (t < A + B) {
            long long s = t - A;
            I = s % L.sx;
            long long q = s / L.sx;
            int jj = q % (2 * g.Hy);
            K = g.Hz + q / (2 * g.Hy);
            J = jj < g.Hy ? jj : jj - g.Hy + (L.sy - g.Hy);
        } else {
            long long s = t - A - B;
            int ii = s % (2 * g.Hx);
            long long q = s / (2 * g.Hx);
            J = g.Hy + q % g.Ny;
            K = g.Hz + q / g.Ny;
            I = ii < g.Hx ? ii : ii - g.Hx + (L.sx - g.Hx);
        }
        const int i = I - g.Hx + 1, j = J - g.Hy + 1, k = K - g.Hz + 1;
        int si = i, sj = j, sk = k;
        if (only_dir < 0 || only_dir == 0) si = wrap_x ? wrap1(i, g.Nx) : i;
        if (only_dir < 0 || only_dir == 1) sj = wrap1(j, g.Ny);
        if (only_dir < 0 || only_dir == 2) {
            if (TZ == OCN_PERIODIC) sk = wrap1(k, g.Nz);
            if (TZ == OCN_BOUNDED && !zface_b && only_dir < 0) sk = (k == 0) ? 1 : (k == g.Nz + 1 ? g.Nz : k);  // no-flux mirror
        }
        if (si == i && sj == j && sk == k) continue;
        double val = c[at(L, si, sj, sk)];
        if (TZ == OCN_BOUNDED && has_bc && sk != k) {  // first z-halo plane of a Center-in-z field
            const ZBc &bc = (k == 0) ? zbc.bottom[f] : zbc.top[f];
            if (bc.kind == OCN_BC_VALUE || bc.kind == OCN_BC_GRADIENT) {
                const int kb = (k == 0) ? 1 : g.Nz + 1;  // boundary face index kᴮ
                const double D = g.dzf ? uniform_load(g.dzf, kb + g.Hz - 1) : g.dz;
                const double bv = bc_condition(bc, si, sj, g.Nx, val);
                double grad;
                if (bc.kind == OCN_BC_GRADIENT) grad = bv;
                else grad = (k == 0) ? (val - bv) / (D / 2) : (bv - val) / (D / 2);
                val = (k == 0) ? val + grad * (-D) : val + grad * D;
            }
        }
        c[at(L, i, j, k)] = val;
    }
}

// Open fill: the wall-normal velocity on both boundary faces <- getbc (fill_halo_regions_open.jl:65-70): 0 for the default Impenetrable
// condition, the number / array of an OpenBoundaryCondition(value) (OCN_BC_OPEN) otherwise
__global__ void open_fill_z_kernel(GridDev g, double *__restrict__ w, ZBc bottom, ZBc top)
{
    const Lay L = make_lay(g, OCN_LOC_CCF);
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x, j = 1 + blockIdx.y;
    if (i > g.Nx) return;
    w[at(L, i, j, 1)] = bottom.kind == OCN_BC_OPEN ? bc_condition(bottom, i, j, g.Nx, 0.0) : 0.0;
    w[at(L, i, j, g.Nz + 1)] = top.kind == OCN_BC_OPEN ? bc_condition(top, i, j, g.Nx, 0.0) : 0.0;
}

int launch_fill_halos(const ocn_grid *grid, const FieldTuple &ft, int open_fill, int only_dir, hipStream_t stream,
                      const ZBcTuple *zbc_in)
{
    ZBcTuple zbc{};
    const int has_bc = zbc_in != nullptr;
    if (zbc_in) zbc = *zbc_in;
    GridDev g = to_dev(*grid);
    if (open_fill && grid->tz == OCN_BOUNDED) {
        for (int f = 0; f < ft.n; ++f)
            if (ft.loc[f] == OCN_LOC_CCF)
                hipLaunchKernelGGL(open_fill_z_kernel, dim3((g.Nx + 63) / 64, g.Ny), dim3(64), 0, stream, g, ft.f[f], zbc.bottom[f], zbc.top[f]);
    }
    const int wrap_x = (grid->tx == OCN_PERIODIC);
    long long maxcells = 0;
    for (int f = 0; f < ft.n; ++f) {
        Lay L = make_lay(g, ft.loc[f]);
        long long nzi = L.sz - 2 * g.Hz;
        long long tot = (long long)L.sx * L.sy * 2 * g.Hz + (long long)L.sx * 2 * g.Hy * nzi + (wrap_x ? (long long)2 * g.Hx * g.Ny * nzi : 0);
        if (tot > maxcells) maxcells = tot;
    }
    if (maxcells == 0) return OCN_SUCCESS;
    long long nb = (maxcells + 255) / 256;
    if (nb > 4096) nb = 4096;
    dim3 gridDim((unsigned)nb, ft.n);
    switch (grid->tz) {
        case OCN_PERIODIC: hipLaunchKernelGGL(fill_halos_kernel<OCN_PERIODIC>, gridDim, dim3(256), 0, stream, g, ft, wrap_x, only_dir, zbc, has_bc); break;
        case OCN_BOUNDED: hipLaunchKernelGGL(fill_halos_kernel<OCN_BOUNDED>, gridDim, dim3(256), 0, stream, g, ft, wrap_x, only_dir, zbc, has_bc); break;
        case OCN_FLAT: hipLaunchKernelGGL(fill_halos_kernel<OCN_FLAT>, gridDim, dim3(256), 0, stream, g, ft, wrap_x, only_dir, zbc, has_bc); break;
        default: set_error("unsupported z topology %d", grid->tz); return OCN_ERR_UNSUPPORTED;
    }
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}


// ---------------------------------------------------------------------------------------------------
// General topologies: any of x, y, z Periodic, Bounded or Flat (fill_halo_regions.jl:50-196).  The reference fills in this order:
// impenetrable walls (wall-normal velocity <- 0 on both boundary faces), then the non-periodic sides -- each over the INTERIOR
// cross-section 1:N of the two other directions (fill_halo_size = :yz / :xz / :xy) and only the FIRST halo cell (no-flux mirror,
// or the Value / Gradient extrapolation) -- then the periodic directions over the whole parent cross-section.  One launch reproduces
// the composition: a halo cell copies from the cell that sequence propagates into it,
//   periodic direction  : wrapped index;
//   Bounded direction   : the mirror cell iff it is the first halo cell of a Center-located field AND every OTHER Bounded direction
//                         sits inside 1:N (so corners of two walls, deeper halo cells and halos behind a Face-located wall keep
//                         their values, exactly as the reference leaves them); otherwise its own index.
// Source cells are never written by the same launch.
// skip_x (bit 0: the west side, bit 1: the east side): that side of x is partitioned (FullyConnected, or the connected side of a
// RightConnected / LeftConnected slab) -- its halos come from the neighbour, this launch leaves them alone (the local y / z fills of those
// halo columns are overwritten by the exchange, which carries the whole cross-section); the other side of a half-Bounded slab is a wall
__global__ __launch_bounds__(256) void fill_halos_general_kernel(GridDev g, FieldTuple a, SideBcTuple bcs, int has_bc, int skip_x)
{
    const int f = blockIdx.y;
    double *__restrict__ c = a.f[f];
    const int loc = a.loc[f];
    const Lay L = make_lay(g, loc);
    const int N[3] = {g.Nx, g.Ny, g.Nz}, H[3] = {g.Hx, g.Hy, g.Hz}, T[3] = {skip_x == 3 ? -1 : g.tx, g.ty, g.tz};
    const int S[3] = {L.sx, L.sy, L.sz};
    const long long nzi = S[2] - 2 * H[2], nyi = S[1] - 2 * H[1];
    const long long A = (long long)S[0] * S[1] * 2 * H[2];
    const long long B = (long long)S[0] * 2 * H[1] * nzi;
    const long long Cn = (long long)2 * H[0] * nyi * nzi;
    const long long total = A + B + Cn;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        int P[3];  // 0-based parent coordinates
        if (t < A) {
            P[0] = t % S[0];
            const long long q = t / S[0];
            P[1] = q % S[1];
            const int kk = q / S[1];
            P[2] = kk < H[2] ? kk : kk - H[2] + (S[2] - H[2]);
        } else if (t < A + B) {
            const long long s = t - A;
            P[0] = s % S[0];
            const long long q = s / S[0];
            const int jj = q % (2 * H[1]);
            P[2] = H[2] + q / (2 * H[1]);
            P[1] = jj < H[1] ? jj : jj - H[1] + (S[1] - H[1]);
        } else {
            const long long s = t - A - B;
            const int ii = s % (2 * H[0]);
            const long long q = s / (2 * H[0]);
            P[1] = H[1] + q % nyi;
            P[2] = H[2] + q / nyi;
            P[0] = ii < H[0] ? ii : ii - H[0] + (S[0] - H[0]);
        }
        int idx[3], src[3];
        int mirror_dir = -1;
        bool mirror_ok = true;
        // a cell beyond the CONNECTED side of a half-Bounded slab belongs to the neighbour: x is then no wall for it
        const int ix = P[0] - H[0] + 1;
        const bool x_connected_here = (skip_x & 1 && ix < 1) || (skip_x & 2 && ix > N[0]);
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            idx[d] = P[d] - H[d] + 1;
            src[d] = idx[d];
            if (d == 0 && x_connected_here) continue;
            if (T[d] == OCN_PERIODIC) {
                src[d] = wrap1(idx[d], N[d]);
            } else if (T[d] == OCN_BOUNDED) {
                const bool face = (loc >> d) & 1;
                if (!face && (idx[d] == 0 || idx[d] == N[d] + 1)) mirror_dir = (mirror_dir < 0) ? d : 3;  // 3: two walls meet
                if (idx[d] < 1 || idx[d] > N[d]) mirror_ok = mirror_ok && (mirror_dir == d);            // another Bounded direction outside 1:N
            }
        }
        // (the test above accepts the mirror direction itself; re-check the OTHER Bounded directions)
        if (mirror_dir >= 0 && mirror_dir < 3) {
#pragma unroll
            for (int d = 0; d < 3; ++d)
                if (d != mirror_dir && T[d] == OCN_BOUNDED && !(d == 0 && x_connected_here) && (idx[d] < 1 || idx[d] > N[d])) mirror_dir = 3;
        }
        const bool mirror = mirror_dir >= 0 && mirror_dir < 3;
        if (mirror) src[mirror_dir] = (idx[mirror_dir] == 0) ? 1 : N[mirror_dir];
        if (src[0] == idx[0] && src[1] == idx[1] && src[2] == idx[2]) continue;
        double val = c[at(L, src[0], src[1], src[2])];
        if (mirror && has_bc) {
            const int d = mirror_dir, lo = idx[d] == 0;
            const ZBc &bc = bcs.side[2 * d + (lo ? 0 : 1)][f];
            if (bc.kind == OCN_BC_VALUE || bc.kind == OCN_BC_GRADIENT) {  // fill_halo_regions_value_gradient.jl:5-103
                const int ib = lo ? 1 : N[d] + 1;  // boundary face index
                const double D = d == 0 ? g.dx : d == 1 ? g.dy : (g.dzf ? uniform_load(g.dzf, ib + g.Hz - 1) : g.dz);
                const int a1 = d == 0 ? src[1] : src[0], a2 = d == 2 ? src[1] : src[2];
                const int n1 = d == 0 ? N[1] : N[0];
                const double bv = bc_condition(bc, a1, a2, n1, val);
                double grad;
                if (bc.kind == OCN_BC_GRADIENT) grad = bv;
                else grad = lo ? (val - bv) / (D / 2) : (bv - val) / (D / 2);
                val = lo ? val + grad * (-D) : val + grad * D;
            }
        }
        c[at(L, idx[0], idx[1], idx[2])] = val;
    }
}

// Impenetrable walls in direction d for the field whose wall-normal direction it is (fill_halo_regions_open.jl:65-70); sides: bit 0 the
// low-index face, bit 1 the high-index one (a half-Bounded slab of a partitioned x has one wall)
__global__ void open_fill_general_kernel(GridDev g, double *__restrict__ c, int loc, int d, ZBc blo, ZBc bhi, int sides)
{
    const Lay L = make_lay(g, loc);
    const int N[3] = {g.Nx, g.Ny, g.Nz};
    const int d1 = d == 0 ? 1 : 0, d2 = d == 2 ? 1 : 2;
    const int a = 1 + blockIdx.x * blockDim.x + threadIdx.x, b = 1 + blockIdx.y;
    if (a > N[d1]) return;
    int lo[3], hi[3];
    lo[d1] = hi[d1] = a;
    lo[d2] = hi[d2] = b;
    lo[d] = 1;
    hi[d] = N[d] + 1;
    // getbc(bc, a, b): 0 for the default Impenetrable condition, the number / array of an OpenBoundaryCondition(value) otherwise
    if (sides & 1) c[at(L, lo[0], lo[1], lo[2])] = blo.kind == OCN_BC_OPEN ? bc_condition(blo, a, b, N[d1], 0.0) : 0.0;
    if (sides & 2) c[at(L, hi[0], hi[1], hi[2])] = bhi.kind == OCN_BC_OPEN ? bc_condition(bhi, a, b, N[d1], 0.0) : 0.0;
}

int launch_fill_halos_general(const ocn_grid *grid, const FieldTuple &ft, int open_fill, hipStream_t stream, const SideBcTuple *bcs_in)
{
    SideBcTuple bcs{};
    const int has_bc = bcs_in != nullptr;
    if (bcs_in) bcs = *bcs_in;
    GridDev g = to_dev(*grid);
    const int T[3] = {g.tx, grid->ty, grid->tz}, N[3] = {g.Nx, g.Ny, g.Nz};  // (g.tx: Bounded also for the half-Bounded slabs)
    if (open_fill) {
        for (int f = 0; f < ft.n; ++f)
            for (int d = 0; d < 3; ++d)
                if (T[d] == OCN_BOUNDED && ft.loc[f] == (1 << d)) {
                    const int d1 = d == 0 ? 1 : 0, d2 = d == 2 ? 1 : 2;
                    const int sides = d == 0 ? (g.xw ? 1 : 0) | (g.xe ? 2 : 0) : 3;
                    hipLaunchKernelGGL(open_fill_general_kernel, dim3((N[d1] + 63) / 64, N[d2]), dim3(64), 0, stream, g, ft.f[f], ft.loc[f], d,
                                       bcs.side[2 * d][f], bcs.side[2 * d + 1][f], sides);
                }
    }
    long long maxcells = 0;
    for (int f = 0; f < ft.n; ++f) {
        Lay L = make_lay(g, ft.loc[f]);
        const long long nzi = L.sz - 2 * g.Hz, nyi = L.sy - 2 * g.Hy;
        const long long tot = (long long)L.sx * L.sy * 2 * g.Hz + (long long)L.sx * 2 * g.Hy * nzi + (long long)2 * g.Hx * nyi * nzi;
        if (tot > maxcells) maxcells = tot;
    }
    if (maxcells == 0) return OCN_SUCCESS;
    long long nb = (maxcells + 255) / 256;
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(fill_halos_general_kernel, dim3((unsigned)nb, ft.n), dim3(256), 0, stream, g, ft, bcs, has_bc,
                       (x_connected_west(*grid) ? 1 : 0) | (x_connected_east(*grid) ? 2 : 0));
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

// ---------------------------------------------------------------------------------------------------
// apply_z_bcs! for a tuple of fields (apply_flux_bcs.jl:107-160):
//   bottom: G[i,j,1]  += flux * Az / V(i,j,1)      top: G[i,j,Nz] -= flux * Az(Nz+1) / V(i,j,Nz)
// Az = Δx*Δy; V at the field's own location (Center in z for u, v, tracers).
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void apply_flux_bcs_kernel(GridDev g, FieldTuple G, FieldTuple c, ZBcTuple zbc)
{
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x, j = 1 + blockIdx.y, f = blockIdx.z;
    if (i > g.Nx) return;
    const Lay L = make_lay(g, G.loc[f]);
    const double Az = g.dx * g.dy;
    const ZBc &bb = zbc.bottom[f], &bt = zbc.top[f];
    if (bb.kind == OCN_BC_FLUX) {
        const long long o = at(L, i, j, 1);
        const double V = Az * (g.dzc ? uniform_load(g.dzc, 1 + g.Hz - 1) : g.dz);
        G.f[f][o] += bc_condition(bb, i, j, g.Nx, c.f[f][o]) * Az / V;
    }
    if (bt.kind == OCN_BC_FLUX) {
        const long long o = at(L, i, j, g.Nz);
        const double V = Az * (g.dzc ? uniform_load(g.dzc, g.Nz + g.Hz - 1) : g.dz);
        G.f[f][o] -= bc_condition(bt, i, j, g.Nx, c.f[f][o]) * Az / V;
    }
}

// apply_x_bcs! / apply_y_bcs! (apply_flux_bcs.jl:38-46, 117-146) of a tuple of fields on a grid with a Bounded x / y: one thread per
// boundary-face cell (a, b) adds the left flux to G[1] and subtracts the right one from G[N], in that order (N = 1: the same cell).
//   area = the cell's face area across `dir` (location flipped along dir), V = the cell volume at the field's location.
__global__ __launch_bounds__(256) void apply_flux_bcs_lateral_kernel(GridDev g, FieldTuple G, FieldTuple c, SideBcTuple bcs, int dir)
{
    const int f = blockIdx.z;
    const int N[3] = {g.Nx, g.Ny, g.Nz};
    const int d1 = dir == 0 ? 1 : 0;
    const int a = 1 + blockIdx.x * blockDim.x + threadIdx.x, k = 1 + blockIdx.y;
    if (a > N[d1]) return;
    const ZBc &lo = bcs.side[2 * dir][f], &hi = bcs.side[2 * dir + 1][f];
    if (lo.kind != OCN_BC_FLUX && hi.kind != OCN_BC_FLUX) return;
    const Lay L = make_lay(g, G.loc[f]);
    const int zf = (G.loc[f] >> 2) & 1;
    const double dz = zf ? (g.dzf ? uniform_load(g.dzf, k + g.Hz - 1) : g.dz) : (g.dzc ? uniform_load(g.dzc, k + g.Hz - 1) : g.dz);
    const double area = (dir == 0 ? g.dy : g.dx) * dz;
    const double V = g.dx * g.dy * dz;
    int q[3];
    q[d1] = a;
    q[2] = k;
    // (x: only the slab that holds the wall applies its flux -- a half-Bounded slab of a partitioned x has one)
    if (lo.kind == OCN_BC_FLUX && (dir != 0 || g.xw)) {
        q[dir] = 1;
        const long long o = at(L, q[0], q[1], q[2]);
        G.f[f][o] += bc_condition(lo, a, k, N[d1], c.f[f][o]) * area / V;
    }
    if (hi.kind == OCN_BC_FLUX && (dir != 0 || g.xe)) {
        q[dir] = N[dir];
        const long long o = at(L, q[0], q[1], q[2]);
        G.f[f][o] -= bc_condition(hi, a, k, N[d1], c.f[f][o]) * area / V;
    }
}

int launch_apply_flux_bcs_lateral(const ocn_grid *grid, const FieldTuple &G, const FieldTuple &fields, const SideBcTuple &bcs, hipStream_t stream)
{
    GridDev g = to_dev(*grid);
    for (int dir = 0; dir < 2; ++dir) {
        bool any = false;
        for (int f = 0; f < G.n; ++f) any = any || bcs.side[2 * dir][f].kind == OCN_BC_FLUX || bcs.side[2 * dir + 1][f].kind == OCN_BC_FLUX;
        if (!any) continue;
        const int n1 = dir == 0 ? g.Ny : g.Nx;
        hipLaunchKernelGGL(apply_flux_bcs_lateral_kernel, dim3((n1 + 63) / 64, g.Nz, G.n), dim3(64), 0, stream, g, G, fields, bcs, dir);
        OCN_CHECK_HIP(hipGetLastError());
    }
    return OCN_SUCCESS;
}

int launch_apply_flux_bcs(const ocn_grid *grid, const FieldTuple &G, const FieldTuple &fields, const ZBcTuple &zbc, hipStream_t stream)
{
    GridDev g = to_dev(*grid);
    hipLaunchKernelGGL(apply_flux_bcs_kernel, dim3((g.Nx + 63) / 64, g.Ny, G.n), dim3(64), 0, stream, g, G, fields, zbc);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

// ---------------------------------------------------------------------------------------------------
// _update_hydrostatic_pressure! (update_hydrostatic_pressure.jl:12-20): one thread per (i, j) column of
// p_kernel_parameters = (0:Nx+1, 0:Ny+1), marching down from k = Nz;  z_dot_g_bᶜᶜᶠ = 1 * ℑzᵃᵃᶠ(b).
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ double buoyancy_perturbation(const TermsDev &t, long long a)
{
    switch (t.buoyancy) {
        case OCN_BUOYANCY_TRACER: return t.T[a];
        case OCN_BUOYANCY_SEAWATER_TS: return t.g * (t.alpha * t.T[a] - t.beta * t.S[a]);
        case OCN_BUOYANCY_SEAWATER_T: return t.g * t.alpha * t.T[a];
        case OCN_BUOYANCY_SEAWATER_S: return -t.g * t.beta * t.S[a];
        default: return 0.0;
    }
}

__global__ __launch_bounds__(256) void hydrostatic_pressure_kernel(GridDev g, TermsDev t, double *__restrict__ pHY, int i0, int i1, int j0, int j1)
{
    // p_kernel_parameters (update_hydrostatic_pressure.jl:48-56): 0 .. N+1 (1 .. N along a Flat direction), or a sub-range in x
    const int i = i0 + blockIdx.x * blockDim.x + threadIdx.x, j = j0 + blockIdx.y * blockDim.y + threadIdx.y;
    if (i > i1 || j > j1) return;
    const Lay L = make_lay(g, OCN_LOC_CCC);
    const int Nz = g.Nz;
    long long o = at(L, i, j, Nz + 1);
    double b_up = buoyancy_perturbation(t, o);  // b[k+1]
    double p = 0.0;
#pragma unroll 8
    for (int k = Nz; k >= 1; --k) {  // (unrolled: the loads of 8 planes are in flight while the recurrence runs)
        o -= L.s3;
        const double b = buoyancy_perturbation(t, o);
        const double zb = 1 * (0.5 * (b + b_up));                       // z_dot_g_bᶜᶜᶠ(k+1)
        const double dz = g.dzf ? uniform_load(g.dzf, k + 1 + g.Hz - 1) : g.dz;       // Δzᶜᶜᶠ(k+1)
        p = (k == Nz) ? -zb * dz : p - zb * dz;
        pHY[o] = p;
        b_up = b;
    }
}

int launch_hydrostatic_pressure(const ocn_grid *grid, const TermsDev &t, double *pHY, hipStream_t stream, const int32_t *irange)
{
    if (grid->tz == OCN_FLAT || t.buoyancy == OCN_BUOYANCY_NONE) return OCN_SUCCESS;
    GridDev g = to_dev(*grid);
    const bool fx = grid->tx == OCN_FLAT, fy = grid->ty == OCN_FLAT;
    const int i0 = irange ? irange[0] : (fx ? 1 : 0), i1 = irange ? irange[1] : (fx ? g.Nx : g.Nx + 1);
    const int j0 = fy ? 1 : 0, j1 = fy ? g.Ny : g.Ny + 1;
    if (i1 < i0) return OCN_SUCCESS;
    const dim3 block = range_block(i1 - i0 + 1), nb = range_grid(block, i1 - i0 + 1, j1 - j0 + 1, 1);
    hipLaunchKernelGGL(hydrostatic_pressure_kernel, nb, block, 0, stream, g, t, pHY, i0, i1, j0, j1);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

// ---------------------------------------------------------------------------------------------------
// HydrostaticFreeSurfaceModel: the variants of the free-surface kernels that exist for a (Periodic, Periodic, Bounded) static grid only
// (SURVEY 8(f) rank 4).  The kernels of every topology are in hydrostatic_surface.hip.  All 2-D quantities are (sx, sy) planes like η.
// ---------------------------------------------------------------------------------------------------
// ---- AdamsBashforth3Scheme of the substepping (split_explicit_timesteppers.jl:19-159): the reference's two kernels per substep with the
// AB3 extrapolations U★ = α Uᵐ + θ Uᵐ⁻¹ + β Uᵐ⁻² and η★ = δ ηᵐ⁺¹ + μ ηᵐ + γ ηᵐ⁻¹ + ϵ ηᵐ⁻² and their history updates
// (cache_previous_free_surface! / cache_previous_velocities!).  A non-default option: kept in the reference's launch shape.
struct AB3Coef {
    double alpha, theta, beta, delta, mu, gamma, epsilon;
};
__global__ void split_explicit_update_state_kernel(GridDev g, double *__restrict__ eta, double *__restrict__ U, double *__restrict__ V,
                                                   const double *__restrict__ etab, const double *__restrict__ Ub, const double *__restrict__ Vb);
__global__ __launch_bounds__(256) void split_explicit_eta_ab3_kernel(GridDev g, double dtau, AB3Coef c, double *__restrict__ eta,
                                                                     double *__restrict__ em, double *__restrict__ em1, double *__restrict__ em2,
                                                                     const double *__restrict__ U, const double *__restrict__ Um1,
                                                                     const double *__restrict__ Um2, const double *__restrict__ V,
                                                                     const double *__restrict__ Vm1, const double *__restrict__ Vm2)
{
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x, j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    if (i > g.Nx || j > g.Ny) return;
    const int ip = i == g.Nx ? 1 : i + 1, jp = j == g.Ny ? 1 : j + 1;
    const double dx = g.dx, dy = g.dy, Az = dx * dy;
    const long long e = plane_at(g, i, j), ee = plane_at(g, ip, j), en = plane_at(g, i, jp);
    em2[e] = em1[e];
    em1[e] = em[e];
    em[e] = eta[e];
    auto Us = [&](long long q) { return c.alpha * U[q] + c.theta * Um1[q] + c.beta * Um2[q]; };
    auto Vs = [&](long long q) { return c.alpha * V[q] + c.theta * Vm1[q] + c.beta * Vm2[q]; };
    eta[e] = eta[e] - dtau * ((dy * Us(ee) - dy * Us(e)) + (dx * Vs(en) - dx * Vs(e))) / Az;
}
__global__ __launch_bounds__(256) void split_explicit_velocity_ab3_kernel(GridDev g, double w, double dtau, double grav, double H, AB3Coef c,
                                                                          const double *__restrict__ eta, const double *__restrict__ em,
                                                                          const double *__restrict__ em1, const double *__restrict__ em2,
                                                                          double *__restrict__ U, double *__restrict__ Um1, double *__restrict__ Um2,
                                                                          double *__restrict__ V, double *__restrict__ Vm1, double *__restrict__ Vm2,
                                                                          double *__restrict__ etab, double *__restrict__ Ub, double *__restrict__ Vb,
                                                                          const double *__restrict__ GU, const double *__restrict__ GV)
{
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x, j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    if (i > g.Nx || j > g.Ny) return;
    const int im = i == 1 ? g.Nx : i - 1, jm = j == 1 ? g.Ny : j - 1;
    const long long e = plane_at(g, i, j), ew = plane_at(g, im, j), es = plane_at(g, i, jm);
    Um2[e] = Um1[e];
    Um1[e] = U[e];
    Vm2[e] = Vm1[e];
    Vm1[e] = V[e];
    auto Es = [&](long long q) { return c.delta * eta[q] + c.mu * em[q] + c.gamma * em1[q] + c.epsilon * em2[q]; };
    const double e0 = Es(e);
    const double Un = U[e] + dtau * (-grav * H * ((e0 - Es(ew)) / g.dx) + GU[e]);
    const double Vn = V[e] + dtau * (-grav * H * ((e0 - Es(es)) / g.dy) + GV[e]);
    etab[e] += w * eta[e];
    Ub[e] += w * Un;
    Vb[e] += w * Vn;
    U[e] = Un;
    V[e] = Vn;
}
// work: 7 planes (ηᵐ, ηᵐ⁻¹, ηᵐ⁻², Uᵐ⁻¹, Uᵐ⁻², Vᵐ⁻¹, Vᵐ⁻²)
int launch_split_explicit_substeps_ab3(const ocn_grid *grid, int n, const double *weights, double dtau, double grav, double H, const double *coef,
                                       double *eta, double *U, double *V, double *etab, double *Ub, double *Vb, const double *GU, const double *GV,
                                       double *work, hipStream_t stream)
{
    GridDev g = to_dev(*grid);
    const long long plane = (long long)(g.Nx + 2 * g.Hx) * (g.Ny + 2 * g.Hy);
    const size_t bytes = (size_t)plane * sizeof(double);
    double *em = work, *em1 = work + plane, *em2 = work + 2 * plane, *Um1 = work + 3 * plane, *Um2 = work + 4 * plane, *Vm1 = work + 5 * plane,
           *Vm2 = work + 6 * plane;
    // initialize_free_surface_state!: history <- current state, filtered state <- 0
    for (double *f : {em, em1, em2}) OCN_CHECK_HIP(hipMemcpyAsync(f, eta, bytes, hipMemcpyDeviceToDevice, stream));
    for (double *f : {Um1, Um2}) OCN_CHECK_HIP(hipMemcpyAsync(f, U, bytes, hipMemcpyDeviceToDevice, stream));
    for (double *f : {Vm1, Vm2}) OCN_CHECK_HIP(hipMemcpyAsync(f, V, bytes, hipMemcpyDeviceToDevice, stream));
    for (double *f : {etab, Ub, Vb}) OCN_CHECK_HIP(hipMemsetAsync(f, 0, bytes, stream));
    const AB3Coef c{coef[0], coef[1], coef[2], coef[3], coef[4], coef[5], coef[6]};
    dim3 block(64, 4, 1), nb((g.Nx + 63) / 64, (g.Ny + 3) / 4, 1);
    for (int m = 0; m < n; ++m) {
        hipLaunchKernelGGL(split_explicit_eta_ab3_kernel, nb, block, 0, stream, g, dtau, c, eta, em, em1, em2, U, Um1, Um2, V, Vm1, Vm2);
        hipLaunchKernelGGL(split_explicit_velocity_ab3_kernel, nb, block, 0, stream, g, weights[m], dtau, grav, H, c, eta, em, em1, em2, U, Um1, Um2,
                           V, Vm1, Vm2, etab, Ub, Vb, GU, GV);
    }
    OCN_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(split_explicit_update_state_kernel, nb, block, 0, stream, g, eta, U, V, etab, Ub, Vb);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

// ---- the substep loop, temporally blocked ------------------------------------------------------------------------------------------
// iterate_split_explicit! launches 2 tiny kernels per substep (the reference notes it is bound by launch latency,
// step_split_explicit_free_surface.jl:84-88; its distributed variant already trades halo width for communication,
// split_explicit_free_surface.jl:283-300).  Here a workgroup loads a (TXO + 2 SH) x (TYO + 2 SH) patch of η, U, V, Gᵁ, Gⱽ into LDS
// (periodic wrap on load; Gᵁ, Gⱽ in registers) and runs up to SH substeps on it: each substep invalidates one more ring of the patch, the TXO x TYO
// centre stays exact.  Every cell is updated with the text of split_explicit_eta_kernel<false, false> / split_explicit_velocity_kernel<false, false> (hydrostatic_surface.hip), so the
// result is bit-identical; the filtered state accumulates in registers for the centre cells in substep order.  Launches
// ping-pong between (η, U, V) and a workspace because neighbouring workgroups read each other's centre cells at load time.
// The (η, U, V, Gᵁ, Gⱽ, filtered state) planes the kernel works on: nx x ny interior cells with x / y halos hx / hy (row stride nx + 2 hx).
// Single rank: the model's own planes (hx = grid.Hx), x wraps periodically.  Slab-x ranks (DistributedSplitExplicitFreeSurface,
// distributed_split_explicit_free_surface.jl: halos extended to the number of substeps, no communication while substepping): wide work
// planes with hx = W >= the number of substeps, x does NOT wrap; launch l owns the cells x0 <= i < x1 that are still exact after its
// substeps (the owned range shrinks by the substeps of each launch and ends at the interior).
struct PlaneLay {
    int nx, ny, hx, hy;
    int x0, x1;   // owned range, 0-based interior index (may extend into the x halo)
    int wrap_x;
};
template <int SH>
struct SubstepArgs {
    int nsub, first, write_state;
    double w[SH];
    double dtau, grav, H;
    const double *eta_in, *U_in, *V_in, *GU, *GV;
    double *eta_out, *U_out, *V_out, *etab, *Ub, *Vb;
};
template <int TXO, int TYO, int SH>
__global__ __launch_bounds__(256) void split_explicit_blocked_kernel(double dx, double dy, PlaneLay P, SubstepArgs<SH> a)
{
    constexpr int W = TXO + 2 * SH, HH = TYO + 2 * SH, NC = W * HH, NQ = (NC + 255) / 256;
    __shared__ double Le[NC], LU[NC], LV[NC];  // Gᵁ, Gⱽ of a cell are only read by the thread that updates it: registers
    const int tid = threadIdx.x;
    const int i0 = P.x0 + blockIdx.x * TXO, j0 = blockIdx.y * TYO;  // 0-based interior origin of the centre
    const int sx = P.nx + 2 * P.hx;
    const double Az = dx * dy;
    long long gp[NQ];   // plane offset of each of this thread's cells
    bool own[NQ];       // centre cell inside the owned range: accumulates the filtered state and is written back
    double ae[NQ], aU[NQ], aV[NQ], gU[NQ], gV[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int c = tid + 256 * q;
        const int lx = c % W, ly = c / W;
        const int ui = i0 + lx - SH, uj = j0 + ly - SH;                       // unwrapped 0-based interior indices
        const int gi = P.wrap_x ? ((ui % P.nx) + P.nx) % P.nx : min(max(ui, -P.hx), P.nx + P.hx - 1);
        const int gj = ((uj % P.ny) + P.ny) % P.ny;
        gp[q] = (gi + P.hx) + (long long)sx * (gj + P.hy);
        own[q] = c < NC && lx >= SH && lx < SH + TXO && ly >= SH && ly < SH + TYO && ui < P.x1 && uj < P.ny;
        if (c < NC) {
            Le[c] = a.eta_in[gp[q]];
            LU[c] = a.U_in[gp[q]];
            LV[c] = a.V_in[gp[q]];
        }
        gU[q] = c < NC ? a.GU[gp[q]] : 0.0;
        gV[q] = c < NC ? a.GV[gp[q]] : 0.0;
        ae[q] = (own[q] && !a.first) ? a.etab[gp[q]] : 0.0;
        aU[q] = (own[q] && !a.first) ? a.Ub[gp[q]] : 0.0;
        aV[q] = (own[q] && !a.first) ? a.Vb[gp[q]] : 0.0;
    }
    __syncthreads();
    for (int m = 0; m < a.nsub; ++m) {
        const double wgt = a.w[m];
#pragma unroll
        for (int q = 0; q < NQ; ++q) {  // _split_explicit_free_surface!
            const int c = tid + 256 * q;
            if (c < NC) {
                const int lx = c % W, ly = c / W;
                const int ce = ly * W + min(lx + 1, W - 1), cn = min(ly + 1, HH - 1) * W + lx;
                Le[c] = Le[c] - a.dtau * ((dy * LU[ce] - dy * LU[c]) + (dx * LV[cn] - dx * LV[c])) / Az;
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < NQ; ++q) {  // _split_explicit_barotropic_velocity!
            const int c = tid + 256 * q;
            if (c < NC) {
                const int lx = c % W, ly = c / W;
                const int cw = ly * W + max(lx - 1, 0), cs = max(ly - 1, 0) * W + lx;
                const double et = Le[c];
                const double Un = LU[c] + a.dtau * (-a.grav * a.H * ((et - Le[cw]) / dx) + gU[q]);
                const double Vn = LV[c] + a.dtau * (-a.grav * a.H * ((et - Le[cs]) / dy) + gV[q]);
                if (own[q]) {
                    ae[q] += wgt * et;
                    aU[q] += wgt * Un;
                    aV[q] += wgt * Vn;
                }
                LU[c] = Un;
                LV[c] = Vn;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        if (!own[q]) continue;
        const int c = tid + 256 * q;
        a.etab[gp[q]] = ae[q];
        a.Ub[gp[q]] = aU[q];
        a.Vb[gp[q]] = aV[q];
        if (a.write_state) {
            a.eta_out[gp[q]] = Le[c];
            a.U_out[gp[q]] = LU[c];
            a.V_out[gp[q]] = LV[c];
        }
    }
}
// _update_split_explicit_state! (step_split_explicit_free_surface.jl:100-108): η, U, V <- their averages, one launch
__global__ __launch_bounds__(256) void split_explicit_update_state_kernel(GridDev g, double *__restrict__ eta, double *__restrict__ U,
                                                                          double *__restrict__ V, const double *__restrict__ etab,
                                                                          const double *__restrict__ Ub, const double *__restrict__ Vb)
{
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x, j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    if (i > g.Nx || j > g.Ny) return;
    const long long e = plane_at(g, i, j);
    eta[e] = etab[e];
    U[e] = Ub[e];
    V[e] = Vb[e];
}
// the launch sequence over planes of layout P0 (x0 / x1 are set per launch): set[0] holds the state on entry, set[1] is scratch
static int run_blocked_substeps(double dx, double dy, PlaneLay P0, int halo_valid, int n, const double *weights, double dtau, double grav, double H,
                                double *const set0[3], double *const set1[3], double *etab, double *Ub, double *Vb, const double *GU,
                                const double *GV, hipStream_t stream)
{
    constexpr int TXO = 64, TYO = 16, SH = 4;
    double *const *set[2] = {set0, set1};
    int cur = 0, done = 0;
    for (int m0 = 0; m0 < n; m0 += SH) {
        SubstepArgs<SH> a{};
        a.nsub = n - m0 < SH ? n - m0 : SH;
        done += a.nsub;
        a.first = m0 == 0;
        a.write_state = m0 + SH < n;  // the last launch only leaves the averages
        for (int q = 0; q < a.nsub; ++q) a.w[q] = weights[m0 + q];
        a.dtau = dtau; a.grav = grav; a.H = H;
        a.eta_in = set[cur][0]; a.U_in = set[cur][1]; a.V_in = set[cur][2];
        a.eta_out = set[1 - cur][0]; a.U_out = set[1 - cur][1]; a.V_out = set[1 - cur][2];
        a.GU = GU; a.GV = GV; a.etab = etab; a.Ub = Ub; a.Vb = Vb;
        PlaneLay P = P0;
        if (!P.wrap_x) {  // the cells still exact after `done` substeps
            P.x0 = -(halo_valid - done);
            P.x1 = P.nx + (halo_valid - done);
        }
        dim3 nb((P.x1 - P.x0 + TXO - 1) / TXO, (P.ny + TYO - 1) / TYO, 1);
        hipLaunchKernelGGL((split_explicit_blocked_kernel<TXO, TYO, SH>), nb, dim3(256), 0, stream, dx, dy, P, a);
        cur = 1 - cur;
    }
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}
int launch_split_explicit_substeps_blocked(const ocn_grid *grid, int n, const double *weights, double dtau, double grav, double H, double *eta,
                                           double *U, double *V, double *etab, double *Ub, double *Vb, const double *GU, const double *GV,
                                           double *work, hipStream_t stream)
{
    GridDev g = to_dev(*grid);
    const long long plane = (long long)(g.Nx + 2 * g.Hx) * (g.Ny + 2 * g.Hy);
    double *const set0[3] = {eta, U, V}, *const set1[3] = {work, work + plane, work + 2 * plane};
    PlaneLay P{g.Nx, g.Ny, g.Hx, g.Hy, 0, g.Nx, 1};
    OCN_TRY(run_blocked_substeps(g.dx, g.dy, P, 0, n, weights, dtau, grav, H, set0, set1, etab, Ub, Vb, GU, GV, stream));
    dim3 block(64, 4, 1), nb2((g.Nx + 63) / 64, (g.Ny + 3) / 4, 1);
    hipLaunchKernelGGL(split_explicit_update_state_kernel, nb2, block, 0, stream, g, eta, U, V, etab, Ub, Vb);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

// ---- slab-x ranks: DistributedSplitExplicitFreeSurface (distributed_split_explicit_free_surface.jl) ----------------------------------
// The reference extends the x halos of η, U, V, Gᵁ, Gⱽ to the number of substeps, fills them ONCE per baroclinic step and substeps
// without communication over kernel ranges that reach into the halos (:29-66 there; split_explicit_free_surface.jl:283-300).  Here
// the wide planes are work buffers of (nx + 2 W) x Ny cells, W = number of substeps (no y halo: y wraps inside the kernel):
//   begin: interiors -> wide planes; the W-wide west / east interior strips of the 5 planes -> send buffers (plane p, row j, column c at
//          c + W (j + Ny p));  [the caller exchanges them with the x neighbours: west strip -> west neighbour's east halo]
//   run:   received strips -> wide halos; the blocked launches over shrinking owned ranges; interior averages -> η, U, V
// work: 11 wide planes (η, U, V twice for the ping-pong, Gᵁ, Gⱽ, filtered η, U, V).
__global__ __launch_bounds__(256) void dist_planes_kernel(int nx, int Ny, int Hx, int Hy, int W, int mode, const double *__restrict__ e,
                                                          const double *__restrict__ U, const double *__restrict__ V,
                                                          const double *__restrict__ GU, const double *__restrict__ GV,
                                                          double *__restrict__ work, double *__restrict__ west, double *__restrict__ east,
                                                          double *__restrict__ eo, double *__restrict__ Uo, double *__restrict__ Vo)
{
    // mode 0: gather (model planes -> wide planes + send strips); 1: scatter received strips into the wide halos;
    // 2: the filtered state of the interior -> η, U, V of the model
    const int c = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y, p = blockIdx.z;
    const int sxw = nx + 2 * W, sxm = nx + 2 * Hx;
    const long long wplane = (long long)sxw * Ny;
    if (mode == 0) {
        if (c >= nx) return;
        const double *src = p == 0 ? e : p == 1 ? U : p == 2 ? V : p == 3 ? GU : GV;
        const double v = src[(c + Hx) + (long long)sxm * (j + Hy)];
        const int slot = p < 3 ? p : p + 3;  // η, U, V -> planes 0..2 (set 0); Gᵁ, Gⱽ -> planes 6, 7
        work[slot * wplane + (c + W) + (long long)sxw * j] = v;
        if (c < W) west[c + (long long)W * (j + (long long)Ny * p)] = v;
        if (c >= nx - W) east[(c - (nx - W)) + (long long)W * (j + (long long)Ny * p)] = v;
    } else if (mode == 1) {
        if (c >= W) return;
        const int slot = p < 3 ? p : p + 3;
        const long long o = c + (long long)W * (j + (long long)Ny * p);
        work[slot * wplane + c + (long long)sxw * j] = west[o];                 // west halo: columns -W .. -1
        work[slot * wplane + (nx + W + c) + (long long)sxw * j] = east[o];      // east halo: columns nx .. nx + W - 1
    } else {
        if (c >= nx || p >= 3) return;
        double *dst = p == 0 ? eo : p == 1 ? Uo : Vo;
        dst[(c + Hx) + (long long)sxm * (j + Hy)] = work[(8 + p) * wplane + (c + W) + (long long)sxw * j];
    }
}
int launch_split_explicit_dist_begin(const ocn_grid *grid, int W, const double *eta, const double *U, const double *V, const double *GU,
                                     const double *GV, double *work, double *send_west, double *send_east, hipStream_t stream)
{
    dim3 nb((grid->Nx + 255) / 256, grid->Ny, 5);
    hipLaunchKernelGGL(dist_planes_kernel, nb, dim3(256), 0, stream, grid->Nx, grid->Ny, grid->Hx, grid->Hy, W, 0, eta, U, V, GU, GV, work,
                       send_west, send_east, nullptr, nullptr, nullptr);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}
int launch_split_explicit_dist_run(const ocn_grid *grid, int W, int n, const double *weights, double dtau, double grav, double H, double *eta,
                                   double *U, double *V, double *work, const double *recv_west, const double *recv_east, hipStream_t stream)
{
    const int nx = grid->Nx, Ny = grid->Ny;
    const long long wplane = (long long)(nx + 2 * W) * Ny;
    hipLaunchKernelGGL(dist_planes_kernel, dim3((W + 255) / 256, Ny, 5), dim3(256), 0, stream, nx, Ny, grid->Hx, grid->Hy, W, 1, nullptr, nullptr,
                       nullptr, nullptr, nullptr, work, const_cast<double *>(recv_west), const_cast<double *>(recv_east), nullptr, nullptr,
                       nullptr);
    OCN_CHECK_HIP(hipGetLastError());
    double *const set0[3] = {work, work + wplane, work + 2 * wplane}, *const set1[3] = {work + 3 * wplane, work + 4 * wplane, work + 5 * wplane};
    PlaneLay P{nx, Ny, W, 0, 0, nx, 0};
    OCN_TRY(run_blocked_substeps(grid->dx, grid->dy, P, W, n, weights, dtau, grav, H, set0, set1, work + 8 * wplane, work + 9 * wplane,
                                 work + 10 * wplane, work + 6 * wplane, work + 7 * wplane, stream));
    hipLaunchKernelGGL(dist_planes_kernel, dim3((nx + 255) / 256, Ny, 3), dim3(256), 0, stream, nx, Ny, grid->Hx, grid->Hy, W, 2, nullptr, nullptr,
                       nullptr, nullptr, nullptr, work, nullptr, nullptr, eta, U, V);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

// barotropic_split_explicit_corrector! (barotropic_split_explicit_corrector.jl:44-71) + compute_w_from_continuity!
// (compute_w_from_continuity.jl:31-40) in one pass over the columns.  us, vs: the AB2-stepped velocities (second storage of
// hydrostatic_momentum_tiled); Us, Vs: their vertical integrals Σ Δz u* (the reference recomputes them into the filtered-state
// arrays here).  u = u* + (U - U̅*) / H is written into the model's arrays, and w integrates the divergence of the CORRECTED
// velocities upwards from w[k = 1] = 0; the east / north neighbours are corrected on the fly with wrapped indices (x, y Periodic),
// so the interior of w equals what w_from_continuity_kernel (hydrostatic_surface.hip) computes after the halo fill, bit for bit.  40 B per cell instead of
// 32 (corrector) + 16 (barotropic mode) + 24 (w).
__global__ __launch_bounds__(256) void barotropic_correct_w_kernel(GridDev g, const double *__restrict__ us, const double *__restrict__ vs,
                                                                   double *__restrict__ u, double *__restrict__ v, double *__restrict__ w,
                                                                   const double *__restrict__ U, const double *__restrict__ V,
                                                                   const double *__restrict__ Us, const double *__restrict__ Vs, double H)
{
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x, j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    if (i > g.Nx || j > g.Ny) return;
    const Lay L = make_lay(g, OCN_LOC_CCC);
    const int ip = i == g.Nx ? 1 : i + 1, jp = j == g.Ny ? 1 : j + 1;
    const long long e = plane_at(g, i, j), ee = plane_at(g, ip, j), en = plane_at(g, i, jp);
    const bool corr = U != nullptr;  // ExplicitFreeSurface: no corrector, u = u*
    const double cu = corr ? (U[e] - Us[e]) / H : 0.0, cue = corr ? (U[ee] - Us[ee]) / H : 0.0;
    const double cv = corr ? (V[e] - Vs[e]) / H : 0.0, cvn = corr ? (V[en] - Vs[en]) / H : 0.0;
    long long o = at(L, i, j, 1), oe = at(L, ip, j, 1), on = at(L, i, jp, 1);
    const double Az = g.dx * g.dy;
    double wk = 0.0;
    w[o] = wk;
#pragma unroll 8
    for (int k = 1; k <= g.Nz; ++k) {
        const double uc = corr ? us[o] + cu : us[o], ue = corr ? us[oe] + cue : us[oe];
        const double vc = corr ? vs[o] + cv : vs[o], vn = corr ? vs[on] + cvn : vs[on];
        u[o] = uc;
        v[o] = vc;
        const double dzc = g.dzc ? uniform_load(g.dzc, k + g.Hz - 1) : g.dz;
        const double Ax = g.dy * dzc, Ay = g.dx * dzc;
        const double dxu = Ax * ue - Ax * uc;
        const double dyv = Ay * vn - Ay * vc;
        const double dh = (dxu + dyv) / Az;
        wk = wk - (dh + 0.0);
        o += L.s3; oe += L.s3; on += L.s3;
        w[o] = wk;
    }
}
int launch_barotropic_correct_w(const ocn_grid *grid, const double *us, const double *vs, double *u, double *v, double *w, const double *U,
                                const double *V, const double *Us, const double *Vs, double H, hipStream_t stream)
{
    GridDev g = to_dev(*grid);
    dim3 block(64, 4, 1), nb((g.Nx + 63) / 64, (g.Ny + 3) / 4, 1);
    hipLaunchKernelGGL(barotropic_correct_w_kernel, nb, block, 0, stream, g, us, vs, u, v, w, U, V, Us, Vs, H);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

// compute_hydrostatic_free_surface_Gη! (Gη = w[i,j,Nz+1], explicit_free_surface.jl:98-140) followed by
// _explicit_ab2_step_free_surface! (:84-96): η += Δt ((1.5 + χ) Gηⁿ - (0.5 + χ) Gη⁻ not_euler); Gηⁿ is left in Gn for the caller to cache
__global__ __launch_bounds__(256) void free_surface_ab2_kernel(GridDev g, const double *__restrict__ w, double *__restrict__ eta,
                                                               double *__restrict__ Gn, const double *__restrict__ Gm, double dt,
                                                               double chi, double not_euler)
{
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x, j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    if (i > g.Nx || j > g.Ny) return;
    const Lay L = make_lay(g, OCN_LOC_CCC);
    const long long e = (i - 1 + g.Hx) + (long long)L.sx * (j - 1 + g.Hy);
    const double gn = w[at(L, i, j, g.Nz + 1)];
    Gn[e] = gn;
    const double G = (1.5 + chi) * gn - (0.5 + chi) * Gm[e] * not_euler;
    eta[e] += dt * G;
}
int launch_free_surface_ab2(const ocn_grid *grid, const double *w, double *eta, double *Gn, const double *Gm, double dt, double chi,
                            hipStream_t stream)
{
    GridDev g = to_dev(*grid);
    dim3 block(64, 4, 1), nb((g.Nx + 63) / 64, (g.Ny + 3) / 4, 1);
    const double not_euler = (chi != -0.5) ? 1.0 : 0.0;
    hipLaunchKernelGGL(free_surface_ab2_kernel, nb, block, 0, stream, g, w, eta, Gn, Gm, dt, chi, not_euler);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

// ---------------------------------------------------------------------------------------------------
// cell_advection_timescale(grid, velocities) (src/Advection/cell_advection_timescale.jl:13-35): the minimum over the interior of
//   1 / (|u|/Δxᶠᶜᶜ + |v|/Δyᶜᶠᶜ + |w|/Δzᶜᶜᶠ)   (terms of Flat dimensions are 0).
// Block reduction, then an atomic min on the bit pattern (non-negative doubles order like their bits; +inf for a fluid at
// rest).  *out must be initialised to +inf by the caller (ocn_cell_advection_timescale does it).
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void advection_timescale_kernel(GridDev g, const double *__restrict__ u, const double *__restrict__ v,
                                                                  const double *__restrict__ w, unsigned long long *__restrict__ out)
{
    // every field through its own parent layout (a Face field has one more point along a Bounded direction); a Flat direction
    // contributes 0 (_inverse_timescale(..., ::Flat) = 0, cell_advection_timescale.jl:21)
    const Lay Lu = make_lay(g, OCN_LOC_FCC), Lv = make_lay(g, OCN_LOC_CFC), Lw = make_lay(g, OCN_LOC_CCF);
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x, j = 1 + blockIdx.y * blockDim.y + threadIdx.y, k = 1 + blockIdx.z;
    double tau = __longlong_as_double(0x7FF0000000000000LL);
    if (i <= g.Nx && j <= g.Ny) {
        const double ix = (g.tx == OCN_FLAT) ? 0.0 : fabs(u[at(Lu, i, j, k)]) / g.dx;
        const double iy = (g.ty == OCN_FLAT) ? 0.0 : fabs(v[at(Lv, i, j, k)]) / g.dy;
        const double iz = (g.tz == OCN_FLAT) ? 0.0 : fabs(w[at(Lw, i, j, k)]) / (g.dzf ? uniform_load(g.dzf, k + g.Hz - 1) : g.dz);
        const double t = 1 / ((ix + iy) + iz);
        if (t == t) tau = t;
    }
    __shared__ double red[256];
    const int tid = threadIdx.y * blockDim.x + threadIdx.x;
    red[tid] = tau;
    __syncthreads();
    for (int s2 = 128; s2 > 0; s2 >>= 1) {
        if (tid < s2) red[tid] = fmin(red[tid], red[tid + s2]);
        __syncthreads();
    }
    if (tid == 0) atomicMin(out, (unsigned long long)__double_as_longlong(red[0]));
}

int launch_advection_timescale(const ocn_grid *grid, const double *u, const double *v, const double *w, double *out, hipStream_t stream)
{
    GridDev g = to_dev(*grid);
    const double inf = __builtin_inf();
    OCN_CHECK_HIP(hipMemcpyAsync(out, &inf, sizeof(double), hipMemcpyHostToDevice, stream));
    dim3 block(64, 4, 1), nb((g.Nx + 63) / 64, (g.Ny + 3) / 4, g.Nz);
    hipLaunchKernelGGL(advection_timescale_kernel, nb, block, 0, stream, g, u, v, w, reinterpret_cast<unsigned long long *>(out));
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

// ---------------------------------------------------------------------------------------------------
// hasnan(field) = any(isnan, parent(field)) (src/Models/nan_checker.jl:33): grid-stride scan, flag <- 1 on the first NaN.
// 16-B loads; the flag lives in device memory so the default NaNChecker callback costs one read pass and no host sync
// until the caller looks at the flag.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hasnan_kernel(const double *__restrict__ a, long long n, int *__restrict__ flag)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    bool bad = false;
    const long long n2 = n / 2;
    const double2 *a2 = reinterpret_cast<const double2 *>(a);
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n2; t += stride) {
        const double2 x = a2[t];
        bad |= (x.x != x.x) | (x.y != x.y);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) bad |= (a[n - 1] != a[n - 1]);
    if (bad) *flag = 1;
}

// rocprofv3's per-dispatch output has no other way to mark a region when counters are collected (see ocn_profile_marker)
__global__ void profile_marker_kernel() {}
int launch_profile_marker(hipStream_t stream)
{
    hipLaunchKernelGGL(profile_marker_kernel, dim3(1), dim3(1), 0, stream);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

// host-side wait with a deadline: polls an event recorded on `stream` (0.2 ms naps) instead of blocking in the runtime
int wait_stream(hipStream_t stream, double seconds, const char *who)
{
    hipEvent_t ev;
    OCN_CHECK_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e = hipEventRecord(ev, stream);
    if (e != hipSuccess) {
        (void)hipEventDestroy(ev);
        set_error("%s: hipEventRecord failed: %s", who, hipGetErrorString(e));
        return OCN_ERR_HIP;
    }
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        e = hipEventQuery(ev);
        if (e == hipSuccess) break;
        if (e != hipErrorNotReady) {
            (void)hipEventDestroy(ev);
            set_error("%s: %s", who, hipGetErrorString(e));
            return OCN_ERR_HIP;
        }
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > seconds) {
            set_error("%s: the device work on this stream did not finish within %.1f s (a collective whose peer never arrived?)", who, seconds);
            return OCN_ERR_TIMEOUT;  // the event is leaked on purpose: destroying an unfinished event may block
        }
        std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
    (void)hipEventDestroy(ev);
    return OCN_SUCCESS;
}

int launch_hasnan(const double *a, long long n, int *flag, hipStream_t stream)
{
    if (n <= 0) return OCN_SUCCESS;
    long long nb = (n / 2 + 255) / 256;
    if (nb > 2048) nb = 2048;
    if (nb < 1) nb = 1;
    hipLaunchKernelGGL(hasnan_kernel, dim3((unsigned)nb), dim3(256), 0, stream, a, n, flag);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

// ---------------------------------------------------------------------------------------------------
// Time-stepper kernels (runge_kutta_3.jl:194-208, quasi_adams_bashforth_2.jl:162-175, store_tendencies.jl:6-9)
// mode 0: rk3 first stage  U += (dt*gamma)*Gn
// mode 1: rk3             U += dt*(gamma*Gn + zeta*Gm)
// mode 2: ab2             U += dt*((1.5+chi)*Gn - (0.5+chi)*Gm*not_euler)   (c2 = not_euler)
// mode 3: cache           Gm <- Gn   (U unused)
// mode 4: split RK3       U = c2 * Psi + c1 * (U + dt * Gn)   (Psi = the field at the start of the step, in the Gm slot)
// ---------------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(256) void stepper_kernel(GridDev g, StepTuple a, double dt, double c1, double c2)
{
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x;
    const int j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    const int k = 1 + blockIdx.z;
    if (i > g.Nx || j > g.Ny) return;
#pragma unroll
    for (int f = 0; f < MAX_TUPLE; ++f) {  // fully unrolled: the loads of all fields are in flight together
        if (f >= a.n) break;
        const int loc = a.loc[f];
        // launch!(..., :xyz; exclude_periphery=true): Face in a Bounded dim starts at 2 (kernel_launching.jl:113-161)
        if (MODE != 3 && (loc & 4) && g.tz == OCN_BOUNDED && g.Nz > 1 && k < 2) continue;
        if (MODE != 3 && (loc & 1) && g.xw && g.Nx > 1 && i < 2) continue;
        if (MODE != 3 && (loc & 2) && g.ty == OCN_BOUNDED && g.Ny > 1 && j < 2) continue;
        const Lay L = make_lay(g, loc);
        const long long o = at(L, i, j, k);
        if (MODE == 0) {
            a.U[f][o] += (dt * c1) * a.Gn[f][o];
        } else if (MODE == 1) {
            a.U[f][o] += dt * (c1 * a.Gn[f][o] + c2 * a.Gm[f][o]);
        } else if (MODE == 2) {
            // `* not_euler` with a Julia Bool is a strong zero: 0.0 even when G⁻ holds NaN (quasi_adams_bashforth_2.jl:169)
            const double G = (1.5 + c1) * a.Gn[f][o] - ((c2 != 0.0) ? (0.5 + c1) * a.Gm[f][o] : 0.0);
            a.U[f][o] += dt * G;
        } else if (MODE == 4) {
            // split_rk3_substep_field! (hydrostatic_free_surface_rk3_step.jl:30-60): Uᵐ⁺¹ = ζ Ψⁿ + γ (Uᵐ + Δt Gᵐ), Ψⁿ in the Gm slot
            a.U[f][o] = c2 * a.Gm[f][o] + c1 * (a.U[f][o] + dt * a.Gn[f][o]);
        } else {
            a.Gm[f][o] = a.Gn[f][o];
        }
    }
}

int launch_stepper(const ocn_grid *grid, const StepTuple &st, int mode, double dt, double c1, double c2, hipStream_t stream)
{
    GridDev g = to_dev(*grid);
    dim3 block(64, 4, 1);
    dim3 nb((g.Nx + 63) / 64, (g.Ny + 3) / 4, g.Nz);
    switch (mode) {
        case 0: hipLaunchKernelGGL(stepper_kernel<0>, nb, block, 0, stream, g, st, dt, c1, c2); break;
        case 1: hipLaunchKernelGGL(stepper_kernel<1>, nb, block, 0, stream, g, st, dt, c1, c2); break;
        case 2: hipLaunchKernelGGL(stepper_kernel<2>, nb, block, 0, stream, g, st, dt, c1, c2); break;
        case 4: hipLaunchKernelGGL(stepper_kernel<4>, nb, block, 0, stream, g, st, dt, c1, c2); break;
        default: hipLaunchKernelGGL(stepper_kernel<3>, nb, block, 0, stream, g, st, dt, c1, c2); break;
    }
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

// ---------------------------------------------------------------------------------------------------
// Pressure kernels
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ double dzC(const GridDev &g, int k) { return g.dzc ? uniform_load(g.dzc, k + g.Hz - 1) : g.dz; }
__device__ __forceinline__ double dzF(const GridDev &g, int k) { return g.dzf ? uniform_load(g.dzf, k + g.Hz - 1) : g.dz; }

// divᶜᶜᶜ (divergence_operators.jl:16-19): 1/V * (δx(Ax u) + δy(Ay v) + δz(Az w)); δ along Flat is 0
__device__ __forceinline__ double div_ccc(const GridDev &g, const double *__restrict__ u, const double *__restrict__ v,
                                          const double *__restrict__ w, const Lay &Lu, const Lay &Lv, const Lay &Lw, int i,
                                          int j, int k, int wrap = 0)
{
    const double dzc = dzC(g, k);
    const double Ax = g.dy * dzc, Ay = g.dx * dzc, Az = g.dx * g.dy;
    // wrap (all-periodic grids): the east / north / top neighbour of the last cell is the first one -- the value its halo image holds
    const int ie = (wrap && i == g.Nx) ? 1 : i + 1, jn = (wrap && j == g.Ny) ? 1 : j + 1, kt = (wrap && k == g.Nz) ? 1 : k + 1;
    const double dxu = (g.tx == OCN_FLAT) ? 0.0 : Ax * u[at(Lu, ie, j, k)] - Ax * u[at(Lu, i, j, k)];
    const double dyv = (g.ty == OCN_FLAT) ? 0.0 : Ay * v[at(Lv, i, jn, k)] - Ay * v[at(Lv, i, j, k)];
    const double dzw = (g.tz == OCN_FLAT) ? 0.0 : Az * w[at(Lw, i, j, kt)] - Az * w[at(Lw, i, j, k)];
    return (1 / (Az * dzc)) * ((dxu + dyv) + dzw);
}

// position q of the permuted sequence v of a cosine transform <-> point s of the natural one: v[q] = x[2q] (q < ceil(N/2)), x[2(N-1-q)+1]
// otherwise; its inverse, used both ways: s -> q when storing, q -> s ... of the INVERSE transform's scatter x[q] = v[dct_perm(q)]
__device__ __forceinline__ int dct_perm(int q, int N) { return (q & 1) ? N - 1 - (q - 1) / 2 : q / 2; }

// out_mode 0: real divergence; 1: complex rhs = div/dt (K8); 2: complex rhs = (dz*div)/dt (K9);
//          3: real rhs = div/dt; 4: real rhs = (dz*div)/dt   (real-to-complex FFT path)
template <int OUT>
__global__ __launch_bounds__(256) void source_term_kernel(GridDev g, const double *__restrict__ u, const double *__restrict__ v,
                                                          const double *__restrict__ w, double dt, double *__restrict__ out,
                                                          long long ld1, long long ld2, int perm_dim, int wrap)
{
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x;
    const int j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    const int k = 1 + blockIdx.z;
    if (i > g.Nx || j > g.Ny) return;
    const Lay Lu = make_lay(g, OCN_LOC_FCC), Lv = make_lay(g, OCN_LOC_CFC), Lw = make_lay(g, OCN_LOC_CCF);
    const double d = div_ccc(g, u, v, w, Lu, Lv, Lw, i, j, k, wrap);
    // perm_dim >= 0: the value of point s along that dimension is stored at the position the even / odd permutation of the FFT-based cosine
    // transform reads it from (index_permutations.jl:38-90: the gather pass of the general solver folded into this store)
    int c[3] = {i - 1, j - 1, k - 1};
    if (perm_dim >= 0) c[perm_dim] = dct_perm(c[perm_dim], perm_dim == 0 ? g.Nx : perm_dim == 1 ? g.Ny : g.Nz);
    const long long o = c[0] + ld1 * c[1] + ld2 * c[2];
    if (OUT == 0) {
        out[o] = d;
    } else if (OUT == 1 || OUT == 2) {
        const double r = (OUT == 2) ? (dzC(g, k) * d) / dt : d / dt;
        reinterpret_cast<double2 *>(out)[o] = make_double2(r, 0.0);
    } else {
        out[o] = (OUT == 4) ? (dzC(g, k) * d) / dt : d / dt;
    }
}

int launch_source_term(const ocn_grid *grid, const double *u, const double *v, const double *w, double dt, SourceOut out_mode,
                       double *out, long long ld1, long long ld2, hipStream_t stream, int perm_dim, int wrap)
{
    GridDev g = to_dev(*grid);
    dim3 block(64, 4, 1);
    dim3 nb((g.Nx + 63) / 64, (g.Ny + 3) / 4, g.Nz);
    switch ((int)out_mode) {
        case 0: hipLaunchKernelGGL(source_term_kernel<0>, nb, block, 0, stream, g, u, v, w, dt, out, ld1, ld2, perm_dim, wrap); break;
        case 1: hipLaunchKernelGGL(source_term_kernel<1>, nb, block, 0, stream, g, u, v, w, dt, out, ld1, ld2, perm_dim, wrap); break;
        case 2: hipLaunchKernelGGL(source_term_kernel<2>, nb, block, 0, stream, g, u, v, w, dt, out, ld1, ld2, perm_dim, wrap); break;
        case 3: hipLaunchKernelGGL(source_term_kernel<3>, nb, block, 0, stream, g, u, v, w, dt, out, ld1, ld2, perm_dim, wrap); break;
        default: hipLaunchKernelGGL(source_term_kernel<4>, nb, block, 0, stream, g, u, v, w, dt, out, ld1, ld2, perm_dim, wrap); break;
    }
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

// set_source_term!: storage <- R (real, halo-free) [* dz] widened to complex (or kept real)
__global__ void set_source_kernel(int Nx, int Ny, int Nz, const double *__restrict__ R, const double *__restrict__ dzc, int Hz,
                                  double *__restrict__ out, int complex_out, long long ld1, long long ld2)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y, k = blockIdx.z;
    if (i >= Nx) return;
    double r = R[i + (long long)Nx * (j + (long long)Ny * k)];
    if (dzc) r = r * dzc[k + Hz];
    const long long o = i + ld1 * j + ld2 * k;
    if (complex_out)
        reinterpret_cast<double2 *>(out)[o] = make_double2(r, 0.0);
    else
        out[o] = r;
}
int launch_set_source(int Nx, int Ny, int Nz, const double *R, const double *dzc, int Hz, double *out, int complex_out,
                      long long ld1, long long ld2, hipStream_t stream)
{
    hipLaunchKernelGGL(set_source_kernel, dim3((Nx + 63) / 64, Ny, Nz), dim3(64), 0, stream, Nx, Ny, Nz, R, dzc, Hz, out, complex_out, ld1, ld2);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

// K12: phi_hat = -b_hat / ((lx + ly) + lz); zero mode <- 0 (fft_based_poisson_solver.jl:110-115).
// nxh = number of stored x modes (Nx for C2C, Nx/2+1 for the Hermitian half spectrum).
__global__ __launch_bounds__(256) void spectral_solve_kernel(int nxh, int Ny, int Nz, const double *__restrict__ lx,
                                                             const double *__restrict__ ly, const double *__restrict__ lz,
                                                             double2 *__restrict__ b, int zero_mode_here, int joff, int koff, double m,
                                                             int shifted)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = blockIdx.y * blockDim.y + threadIdx.y;
    const int k = blockIdx.z;
    if (i >= nxh || j >= Ny) return;
    const long long o = i + (long long)nxh * (j + (long long)Ny * k);
    double lam = (lx[i] + ly[j + joff]) + lz[k + koff];
    if (shifted) lam = lam - m;  // the screened equation (∇² + m) ϕ = b (fft_based_poisson_solver.jl:108-110)
    double2 val = b[o];
    val.x = -val.x / lam;
    val.y = -val.y / lam;
    if (zero_mode_here && i == 0 && j == 0 && k == 0) val = make_double2(0.0, 0.0);
    b[o] = val;
}
int launch_spectral_solve(int nxh, int Ny, int Nz, const double *lx, const double *ly, const double *lz, double *b,
                          int zero_mode_here, int joff, int koff, hipStream_t stream, double m, int shifted)
{
    hipLaunchKernelGGL(spectral_solve_kernel, dim3((nxh + 63) / 64, (Ny + 3) / 4, Nz), dim3(64, 4), 0, stream, nxh, Ny, Nz, lx, ly,
                       lz, reinterpret_cast<double2 *>(b), zero_mode_here && !shifted, joff, koff, m, shifted);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

// K13 copy_real_component! (fft_based_poisson_solver.jl:129-137); STRIDE = 2 reads the real part of a complex array
template <int STRIDE>
__global__ __launch_bounds__(256) void copy_real_kernel(GridDev g, const double *__restrict__ phi, double *__restrict__ p, int perm_dim)
{
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x;
    const int j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    const int k = 1 + blockIdx.z;
    if (i > g.Nx || j > g.Ny) return;
    const Lay L = make_lay(g, OCN_LOC_CCC);
    int c[3] = {i - 1, j - 1, k - 1};  // perm_dim >= 0: the scatter pass of the last inverse cosine transform folded into this read
    if (perm_dim >= 0) c[perm_dim] = dct_perm(c[perm_dim], perm_dim == 0 ? g.Nx : perm_dim == 1 ? g.Ny : g.Nz);
    p[at(L, i, j, k)] = phi[STRIDE * (c[0] + (long long)g.Nx * (c[1] + (long long)g.Ny * c[2]))];
}
int launch_copy_real(const ocn_grid *grid, const double *phi, double *p, hipStream_t stream, CopySource source, int perm_dim)
{
    GridDev g = to_dev(*grid);
    dim3 nb((g.Nx + 63) / 64, (g.Ny + 3) / 4, g.Nz), block(64, 4);
    if (source == CopySource::Real)
        hipLaunchKernelGGL(copy_real_kernel<1>, nb, block, 0, stream, g, phi, p, perm_dim);
    else
        hipLaunchKernelGGL(copy_real_kernel<2>, nb, block, 0, stream, g, phi, p, perm_dim);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

// K17 _pressure_correct_velocities! (pressure_correction.jl:31-37): :xyz over 1:N in every dimension
__global__ __launch_bounds__(256) void pressure_correct_kernel(GridDev g, double *__restrict__ u, double *__restrict__ v,
                                                               double *__restrict__ w, const double *__restrict__ p, double dt)
{
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x;
    const int j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    const int k = 1 + blockIdx.z;
    if (i > g.Nx || j > g.Ny) return;
    const Lay Lu = make_lay(g, OCN_LOC_FCC), Lv = make_lay(g, OCN_LOC_CFC), Lw = make_lay(g, OCN_LOC_CCF),
              Lp = make_lay(g, OCN_LOC_CCC);
    const double pc = p[at(Lp, i, j, k)];
    const double px = (g.tx == OCN_FLAT) ? 0.0 : (pc - p[at(Lp, i - 1, j, k)]) / g.dx;
    const double py = (g.ty == OCN_FLAT) ? 0.0 : (pc - p[at(Lp, i, j - 1, k)]) / g.dy;
    u[at(Lu, i, j, k)] -= px * dt;
    v[at(Lv, i, j, k)] -= py * dt;
    if (g.tz == OCN_FLAT) {
        w[at(Lw, i, j, k)] -= 0.0 * dt;
    } else {
        const double pz = (pc - p[at(Lp, i, j, k - 1)]) / dzF(g, k);
        w[at(Lw, i, j, k)] -= pz * dt;
    }
}
int launch_pressure_correct(const ocn_grid *grid, double *u, double *v, double *w, const double *p, double dt, hipStream_t stream)
{
    GridDev g = to_dev(*grid);
    hipLaunchKernelGGL(pressure_correct_kernel, dim3((g.Nx + 63) / 64, (g.Ny + 3) / 4, g.Nz), dim3(64, 4), 0, stream, g, u, v, w, p, dt);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

// ---------------------------------------------------------------------------------------------------
// Fourier-tridiagonal pieces
// ---------------------------------------------------------------------------------------------------
// K15 compute_main_diagonal! ZDirection (fourier_tridiagonal_poisson_solver.jl:41-51); nxh stored x modes
// D[i + sj j + sk (k-1)], i < ni, j < nj: the single-GPU layout is (sj, sk) = (nxh, nxh Ny); the slab pipeline of the distributed
// solver stores (ky_local, kx, z) with (sj, sk) = (c Nz, c)
__global__ void main_diagonal_kernel(GridDev g, int ni, int nj, long long sj, long long sk, const double *__restrict__ lx,
                                     const double *__restrict__ ly, double *__restrict__ D)
{
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (long long)ni * nj) return;
    const int i = (int)(q % ni), j = (int)(q / ni);
    const double lam = lx[i] + ly[j];
    const int Nz = g.Nz;
    double *d = D + i + sj * j;
    d[0] = -1 / dzF(g, 2) - dzC(g, 1) * lam;
    for (int k = 2; k <= Nz - 1; ++k) d[(k - 1) * sk] = -(1 / dzF(g, k + 1) + 1 / dzF(g, k)) - dzC(g, k) * lam;
    d[(Nz - 1) * sk] = -1 / dzF(g, Nz) - dzC(g, Nz) * lam;
}
int launch_main_diagonal_strided(const ocn_grid *grid, int ni, int nj, long long sj, long long sk, const double *lx, const double *ly,
                                 double *D, hipStream_t stream)
{
    GridDev g = to_dev(*grid);
    const long long n = (long long)ni * nj;
    hipLaunchKernelGGL(main_diagonal_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, g, ni, nj, sj, sk, lx, ly, D);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}
int launch_main_diagonal(const ocn_grid *grid, int nxh, const double *lx, const double *ly, double *D, hipStream_t stream)
{
    return launch_main_diagonal_strided(grid, nxh, grid->Ny, nxh, (long long)nxh * grid->Ny, lx, ly, D, stream);
}

// K14 solve_batched_tridiagonal_system_z! (batched_tridiagonal_solver.jl:209-235).  One thread per (i,j) column,
// i across lanes so every k-plane access is coalesced; serial Thomas sweep in k.
// T: double2 (a complex spectrum: the real and the imaginary part are two independent solves with the same real coefficients) or double (the
// all-real spectrum of a closed box, csrc/poisson.hip).
__device__ __forceinline__ double2 tz_zero(double2) { return make_double2(0.0, 0.0); }
__device__ __forceinline__ double tz_zero(double) { return 0.0; }
__device__ __forceinline__ double2 tz_div(double2 v, double s) { return make_double2(v.x / s, v.y / s); }
__device__ __forceinline__ double tz_div(double v, double s) { return v / s; }
// (v - s * w) / d   and   v - s * w, per component in the reference's order
__device__ __forceinline__ double2 tz_star(double2 v, double s, double2 w, double d) { return make_double2((v.x - s * w.x) / d, (v.y - s * w.y) / d); }
__device__ __forceinline__ double tz_star(double v, double s, double w, double d) { return (v - s * w) / d; }
__device__ __forceinline__ double2 tz_back(double2 v, double s, double2 w) { return make_double2(v.x - s * w.x, v.y - s * w.y); }
__device__ __forceinline__ double tz_back(double v, double s, double w) { return v - s * w; }
template <class T>
__global__ __launch_bounds__(64) void tridiag_z_kernel(int ni, int nj, long long sj, long long s3, int Nz,
                                                       const double *__restrict__ a, const double *__restrict__ b,
                                                       const double *__restrict__ c, const T *__restrict__ f,
                                                       double *__restrict__ t, T *__restrict__ phi, int keep_storage)
{
    // column (i, j) at i + sj j, planes s3 apart (see main_diagonal_kernel for the two layouts in use)
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (long long)ni * nj) return;
    const long long o = (q % ni) + sj * (q / ni);
    const double tiny = 10 * 2.220446049250313e-16;
    // The sweep is a serial recurrence, but its operands (b, f going up; t, phi going down) do not depend on it: they are
    // requested PF planes ahead so that the memory latency is paid once per PF planes instead of once per plane (a slab of a
    // distributed run has too few columns to hide it with occupancy).
    constexpr int PF = 8;
    double beta = b[o];
    T prev = tz_div(f[o], beta);
    phi[o] = prev;
    double bq[PF];
    T fq[PF];
#pragma unroll
    for (int m = 0; m < PF; ++m) {
        const int k = 1 + m;
        bq[m] = (k < Nz) ? b[o + k * s3] : 1.0;
        fq[m] = (k < Nz) ? f[o + k * s3] : tz_zero(T{});
    }
    for (int k0 = 1; k0 < Nz; k0 += PF) {
        double bn[PF];
        T fn[PF];
#pragma unroll
        for (int m = 0; m < PF; ++m) {  // next block's operands
            const int k = k0 + PF + m;
            bn[m] = (k < Nz) ? b[o + k * s3] : 1.0;
            fn[m] = (k < Nz) ? f[o + k * s3] : tz_zero(T{});
        }
#pragma unroll
        for (int m = 0; m < PF; ++m) {
            const int k = k0 + m;
            if (k < Nz) {
                const double ck = c[k - 1], ak = a[k - 1], bk = bq[m];
                const double tk = ck / beta;
                t[o + k * s3] = tk;
                beta = bk - ak * tk;
                const bool dd = fabs(beta) > tiny;
                const T star = tz_star(fq[m], ak, prev, beta);
                if (dd) {
                    phi[o + k * s3] = star;
                    prev = star;
                } else {
                    // batched_tridiagonal_solver.jl:224-228 keeps what the storage held: the singular (kx, ky) = (0, 0) column ends in a pivot
                    // of rounding size, its last unknown is the free constant of the gauge, removed again by the zero-mean step.  "What the
                    // storage held" is whatever an earlier solve -- or, the first time, the allocator -- left there: a constant of 2^99 from
                    // recycled memory cost every digit of that column (seen once in a long test process).  The Poisson solvers take 0 as
                    // the constant; the stand-alone BatchedTridiagonalSolver (keep_storage: the caller's ϕ) keeps the reference's semantics.
                    if (keep_storage) {
                        prev = phi[o + k * s3];
                    } else {
                        prev = tz_zero(T{});
                        phi[o + k * s3] = prev;
                    }
                }
            }
        }
#pragma unroll
        for (int m = 0; m < PF; ++m) {
            bq[m] = bn[m];
            fq[m] = fn[m];
        }
    }
    // back substitution, same prefetch distance (t and phi were written by this thread: visible to it in program order)
    double tq[PF];
    T pq[PF];
#pragma unroll
    for (int m = 0; m < PF; ++m) {
        const int k = Nz - 2 - m;
        tq[m] = (k >= 0) ? t[o + (k + 1) * s3] : 0.0;
        pq[m] = (k >= 0) ? phi[o + k * s3] : tz_zero(T{});
    }
    for (int k0 = Nz - 2; k0 >= 0; k0 -= PF) {
        double tn[PF];
        T pn[PF];
#pragma unroll
        for (int m = 0; m < PF; ++m) {
            const int k = k0 - PF - m;
            tn[m] = (k >= 0) ? t[o + (k + 1) * s3] : 0.0;
            pn[m] = (k >= 0) ? phi[o + k * s3] : tz_zero(T{});
        }
#pragma unroll
        for (int m = 0; m < PF; ++m) {
            const int k = k0 - m;
            if (k >= 0) {
                const T cur = tz_back(pq[m], tq[m], prev);
                phi[o + k * s3] = cur;
                prev = cur;
            }
        }
#pragma unroll
        for (int m = 0; m < PF; ++m) {
            tq[m] = tn[m];
            pq[m] = pn[m];
        }
    }
}
int launch_tridiag_z_strided(int ni, int nj, long long sj, long long sk, int Nz, const double *a, const double *b, const double *c,
                             const double *f, double *t, double *phi, hipStream_t stream, int keep_storage)
{
    const long long n = (long long)ni * nj;
    hipLaunchKernelGGL(tridiag_z_kernel<double2>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, ni, nj, sj, sk, Nz, a, b, c,
                       reinterpret_cast<const double2 *>(f), t, reinterpret_cast<double2 *>(phi), keep_storage);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}
// the same sweep over a REAL right-hand side (Nx, Ny, Nz), and the zero-mean gauge on its (0, 0) column
int launch_tridiag_z_real(int Nx, int Ny, int Nz, const double *a, const double *b, const double *c, const double *f, double *t, double *phi,
                          hipStream_t stream)
{
    const long long n = (long long)Nx * Ny;
    hipLaunchKernelGGL(tridiag_z_kernel<double>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, Nx, Ny, (long long)Nx, (long long)Nx * Ny, Nz, a,
                       b, c, f, t, phi, 0);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}
int launch_tridiag_z(int Nx, int Ny, int Nz, const double *a, const double *b, const double *c, const double *f, double *t,
                     double *phi, hipStream_t stream, int keep_storage)
{
    return launch_tridiag_z_strided(Nx, Ny, Nx, (long long)Nx * Ny, Nz, a, b, c, f, t, phi, stream, keep_storage);
}

// zero-mean gauge (fourier_tridiagonal_poisson_solver.jl:142) applied in spectral space: subtracting the volume
// mean equals subtracting mean_k(phi_hat[0,0,k]) from the (kx,ky) = (0,0) column (the inverse transform carries
// the 1/(Nx Ny) factor).  One block.
__global__ void remove_mean_mode_kernel(long long s3, int Nz, double2 *__restrict__ phi)
{
    __shared__ double sre[256], sim[256];
    double re = 0, im = 0;
    for (int k = threadIdx.x; k < Nz; k += blockDim.x) {
        re += phi[k * s3].x;
        im += phi[k * s3].y;
    }
    sre[threadIdx.x] = re;
    sim[threadIdx.x] = im;
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            sre[threadIdx.x] += sre[threadIdx.x + s];
            sim[threadIdx.x] += sim[threadIdx.x + s];
        }
        __syncthreads();
    }
    const double mre = sre[0] / Nz, mim = sim[0] / Nz;
    for (int k = threadIdx.x; k < Nz; k += blockDim.x) {
        phi[k * s3].x -= mre;
        phi[k * s3].y -= mim;
    }
}
__global__ void remove_mean_mode_real_kernel(long long s3, int Nz, double *__restrict__ phi)
{
    __shared__ double sre[256];
    double re = 0;
    for (int k = threadIdx.x; k < Nz; k += blockDim.x) re += phi[k * s3];
    sre[threadIdx.x] = re;
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) sre[threadIdx.x] += sre[threadIdx.x + s];
        __syncthreads();
    }
    const double mre = sre[0] / Nz;
    for (int k = threadIdx.x; k < Nz; k += blockDim.x) phi[k * s3] -= mre;
}
int launch_remove_mean_mode_real(long long s3, int Nz, double *phi, hipStream_t stream)
{
    hipLaunchKernelGGL(remove_mean_mode_real_kernel, dim3(1), dim3(256), 0, stream, s3, Nz, phi);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}
int launch_remove_mean_mode(long long s3, int Nz, double *phi, hipStream_t stream)
{
    hipLaunchKernelGGL(remove_mean_mode_kernel, dim3(1), dim3(256), 0, stream, s3, Nz, reinterpret_cast<double2 *>(phi));
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

// ---------------------------------------------------------------------------------------------------
// Distributed slab-x staging (field_boundary_buffers.jl:276-308) and transposes (distributed_transpose.jl:25-95)
// ---------------------------------------------------------------------------------------------------
// sides (unpack only): bit 0 the west halo, bit 1 the east halo -- the walled side of a half-Bounded slab keeps its wall fill (what the ring
// delivered there comes from the slab at the other end of the domain and is dropped)
__global__ void halo_pack_x_kernel(int Hx, int nx, int sx, long long rows, const double *__restrict__ c,
                                   double *__restrict__ west, double *__restrict__ east, int unpack, int sides)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= rows * Hx) return;
    const int h = t % Hx;
    const long long row = t / Hx;
    const double *crow = c + row * sx;
    if (!unpack) {
        west[t] = crow[Hx + h];  // parent[1+Hx : 2Hx]
        east[t] = crow[nx + h];  // parent[1+nx : nx+Hx]
    } else {
        double *wrow = const_cast<double *>(crow);
        if (sides & 1) wrow[h] = west[t];            // parent[1 : Hx]
        if (sides & 2) wrow[nx + Hx + h] = east[t];  // parent[1+nx+Hx : nx+2Hx]
    }
}
static int unpack_sides(const ocn_grid *grid) { return (grid->tx != OCN_RIGHT_CONNECTED ? 1 : 0) | (grid->tx != OCN_LEFT_CONNECTED ? 2 : 0); }
int launch_halo_pack_x(const ocn_grid *grid, const double *field, int loc, double *west, double *east, int unpack, hipStream_t stream)
{
    GridDev g = to_dev(*grid);
    Lay L = make_lay(g, loc);
    long long rows = (long long)L.sy * L.sz;
    long long n = rows * g.Hx;
    hipLaunchKernelGGL(halo_pack_x_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, g.Hx, g.Nx, L.sx, rows, field, west, east, unpack,
                       unpack_sides(grid));
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

// One x-plane (full cross-section) of a field: pack the first / last interior plane, unpack into the adjacent halo plane.
// which = 0: west (pack x = 1, unpack x = 0), 1: east (pack x = nx, unpack x = nx + 1).
__global__ void halo_plane_x_kernel(int Hx, int nx, int sx, long long rows, double *__restrict__ c, double *__restrict__ buf, int which,
                                    int unpack)
{
    const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= rows) return;
    double *crow = c + row * sx;
    if (!unpack)
        buf[row] = which ? crow[Hx + nx - 1] : crow[Hx];
    else
        crow[which ? Hx + nx : Hx - 1] = buf[row];
}
int launch_halo_plane_x(const ocn_grid *grid, double *field, int loc, int which, double *buf, int unpack, hipStream_t stream)
{
    GridDev g = to_dev(*grid);
    Lay L = make_lay(g, loc);
    const long long rows = (long long)L.sy * L.sz;
    if (unpack && !(unpack_sides(grid) & (which ? 2 : 1))) return OCN_SUCCESS;  // that side of the slab is a wall: its fill stays
    hipLaunchKernelGGL(halo_plane_x_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, g.Hx, g.Nx, L.sx, rows, field, buf,
                       which, unpack);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

// All fields of a tuple in one launch (blockIdx.y = field); the strips of the fields follow one another in `west` / `east`, so a
// halo exchange is ONE message per neighbour.
struct PackTuple {
    double *f[MAX_TUPLE];
    int sx[MAX_TUPLE];
    long long rows[MAX_TUPLE], off[MAX_TUPLE];
    int sy, Ny, Nz, Hy, Hz;  // unpack == 2: the sender filled interior rows only; a halo row takes its periodic image's
};
__global__ void halo_pack_x_fields_kernel(int Hx, int nx, PackTuple a, double *__restrict__ west, double *__restrict__ east, int unpack, int sides)
{
    const int fi = blockIdx.y;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.rows[fi] * Hx) return;
    const int h = t % Hx;
    const long long row = t / Hx;
    double *crow = a.f[fi] + row * a.sx[fi];
    long long b = a.off[fi] + t;
    if (!unpack) {
        west[b] = crow[Hx + h];
        east[b] = crow[nx + h];
    } else {
        if (unpack == 2) {  // strips written by the tendency launch's epilogue (interior rows): wrap (j, k) periodically
            const int jp = (int)(row % a.sy), kp = (int)(row / a.sy);
            int j = jp - a.Hy + 1, k = kp - a.Hz + 1;
            j = j < 1 ? j + a.Ny : (j > a.Ny ? j - a.Ny : j);
            k = k < 1 ? k + a.Nz : (k > a.Nz ? k - a.Nz : k);
            b = a.off[fi] + h + (long long)Hx * ((j + a.Hy - 1) + (long long)a.sy * (k + a.Hz - 1));
        }
        if (sides & 1) crow[h] = west[b];
        if (sides & 2) crow[nx + Hx + h] = east[b];
    }
}
int launch_halo_pack_x_fields(const ocn_grid *grid, const FieldTuple &ft, double *west, double *east, int unpack, hipStream_t stream)
{
    GridDev g = to_dev(*grid);
    PackTuple a{};
    long long off = 0, most = 0;
    for (int q = 0; q < ft.n; ++q) {
        Lay L = make_lay(g, ft.loc[q]);
        a.f[q] = ft.f[q];
        a.sx[q] = L.sx;
        a.rows[q] = (long long)L.sy * L.sz;
        a.off[q] = off;
        off += a.rows[q] * g.Hx;
        most = a.rows[q] * g.Hx > most ? a.rows[q] * g.Hx : most;
        a.sy = L.sy;  // (unpack == 2 is used on Periodic y, z: every field of the tuple has this cross-section)
    }
    a.Ny = g.Ny; a.Nz = g.Nz; a.Hy = g.Hy; a.Hz = g.Hz;
    hipLaunchKernelGGL(halo_pack_x_fields_kernel, dim3((unsigned)((most + 255) / 256), ft.n), dim3(256), 0, stream, g.Hx, g.Nx, a, west, east, unpack,
                       unpack_sides(grid));
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

// y-local (nx,Ny,Nz) <-> x-local (Nx = R*nx, ny = Ny/R, Nz), complex.
// mode 0 pack y->x : send[i + nx*(k + Nz*j)] = y[i,j,k]                          (:38-42)
// mode 1 unpack x<-y: x[i,j,k] = recv[i' + nx*(k + Nz*j) + m*nx*ny*Nz], i = m*nx+i' (:51-60)
// mode 2 pack x->y : send[j + ny*(k + Nz*i)] = x[i,j,k]                          (:31-35)
// mode 3 unpack y<-x: y[i,j,k] = recv[j' + ny*(k + Nz*i) + m*nx*ny*Nz], j = m*ny+j' (:86-95)
template <int MODE>
__global__ __launch_bounds__(256) void transpose_kernel(int nx, int Ny, int Nz, int R, const double2 *__restrict__ src,
                                                        double2 *__restrict__ dst)
{
    const int ny = Ny / R, Nx = nx * R;
    const long long chunk = (long long)nx * ny * Nz;
    if (MODE == 0 || MODE == 3) {  // thread over y-field (i fastest)
        const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y, k = blockIdx.z;
        if (i >= nx) return;
        const long long yo = i + (long long)nx * (j + (long long)Ny * k);
        if (MODE == 0) {
            dst[i + (long long)nx * (k + (long long)Nz * j)] = src[yo];
        } else {
            const int m = j / ny, jp = j - m * ny;
            dst[yo] = src[jp + (long long)ny * (k + (long long)Nz * i) + m * chunk];
        }
    } else {  // thread over x-field
        const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y, k = blockIdx.z;
        if (i >= Nx) return;
        const long long xo = i + (long long)Nx * (j + (long long)ny * k);
        if (MODE == 1) {
            const int m = i / nx, ip = i - m * nx;
            dst[xo] = src[ip + (long long)nx * (k + (long long)Nz * j) + m * chunk];
        } else {
            dst[j + (long long)ny * (k + (long long)Nz * i)] = src[xo];
        }
    }
}
int launch_transpose(int mode, int nx, int Ny, int Nz, int R, const double *src, double *dst, hipStream_t stream)
{
    const int ny = Ny / R, Nx = nx * R;
    const double2 *s = reinterpret_cast<const double2 *>(src);
    double2 *d = reinterpret_cast<double2 *>(dst);
    switch (mode) {
        case 0: hipLaunchKernelGGL(transpose_kernel<0>, dim3((nx + 63) / 64, Ny, Nz), dim3(64), 0, stream, nx, Ny, Nz, R, s, d); break;
        case 3: hipLaunchKernelGGL(transpose_kernel<3>, dim3((nx + 63) / 64, Ny, Nz), dim3(64), 0, stream, nx, Ny, Nz, R, s, d); break;
        case 1: hipLaunchKernelGGL(transpose_kernel<1>, dim3((Nx + 63) / 64, ny, Nz), dim3(64), 0, stream, nx, Ny, Nz, R, s, d); break;
        default: hipLaunchKernelGGL(transpose_kernel<2>, dim3((Nx + 63) / 64, ny, Nz), dim3(64), 0, stream, nx, Ny, Nz, R, s, d); break;
    }
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

}  // namespace ocn
