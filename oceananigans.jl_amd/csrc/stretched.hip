// stretched.hip -- the pieces of the Fourier-tridiagonal solver along a stretched x (YZRegularRG) or y (XZRegularRG)
// (fourier_tridiagonal_poisson_solver.jl:17-39, 155-177; batched_tridiagonal_solver.jl:209-235 for XDirection).
// Strict IEEE object (-ffp-contract=off): the x sweep is bitwise the z sweep of kernels.hip on transposed data.
#include "ocn_internal.h"

namespace ocn {

// ---------------------------------------------------------------------------------------------------
// Thomas sweep along x.  x is the contiguous dimension: one lane per line with an Nx-element lane stride would touch a
// different cache line per lane and step.  A workgroup of 64 lanes owns 64 consecutive lines instead and walks them in
// chunks of C points: the chunk of all 64 lines is loaded with lanes along x (C consecutive elements per line), each lane
// sweeps its own line through LDS, and the chunk goes back the same way.  β and ϕ[i-1] stay in registers across chunks, so
// a line of any length needs only one chunk of LDS.  Forward elimination runs the chunks upwards, back substitution downwards.
// Arithmetic and order of operations: those of tridiag_z_kernel (kernels.hip), including the 10 eps pivot test and the
// keep_storage semantics.
// LDS rows are padded to C + 1 doubles: with C even, lane l's row starts at bank 2 l (C + 1) mod 64, so the 64-bit reads of
// one 32-lane half hit 32 distinct bank pairs.
// ---------------------------------------------------------------------------------------------------
template <class T> struct XParts;
template <> struct XParts<double> {
    static constexpr int n = 1;
    __device__ static double get(const double *p, long long o, int) { return p[o]; }
    __device__ static void put(double *p, long long o, const double *v) { p[o] = v[0]; }
};
template <> struct XParts<double2> {
    static constexpr int n = 2;
    __device__ static double get(const double2 *p, long long o, int c) { return c ? p[o].y : p[o].x; }
    __device__ static void put(double2 *p, long long o, const double *v) { p[o] = make_double2(v[0], v[1]); }
};

template <class T, int C>
__global__ __launch_bounds__(64) void tridiag_x_kernel(int N, long long nlines, const double *__restrict__ a, const double *__restrict__ b,
                                                       const double *__restrict__ c, const T *__restrict__ f, double *__restrict__ t,
                                                       T *__restrict__ phi, int keep_storage)
{
    constexpr int L = 64, S = C + 1, NP = XParts<T>::n;
    __shared__ double sv[NP][L * S];  // f, then ϕ (real / imaginary part)
    __shared__ double sb[L * S];      // b, then t (forward); t[k + 1] (backward)
    const int lane = threadIdx.x;
    const long long line0 = (long long)blockIdx.x * L;
    const int nl = (int)((nlines - line0) < L ? (nlines - line0) : L);
    const long long base = line0 * N;  // line l of this workgroup starts at base + l N
    const bool mine = lane < nl;
    const double tiny = 10 * 2.220446049250313e-16;
    double beta = 0.0;
    double prev[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) prev[q] = 0.0;

    // ---- forward elimination, chunks upwards
    for (int x0 = 0; x0 < N; x0 += C) {
        const int cw = (N - x0) < C ? (N - x0) : C;
        for (int e = lane; e < L * C; e += L) {
            const int l = e / C, x = e % C;
            if (l < nl && x < cw) {
                const long long o = base + (long long)l * N + x0 + x;
#pragma unroll
                for (int q = 0; q < NP; ++q) sv[q][l * S + x] = XParts<T>::get(f, o, q);
                sb[l * S + x] = b[o];
            }
        }
        __syncthreads();
        if (mine) {
            double *vr[NP];
#pragma unroll
            for (int q = 0; q < NP; ++q) vr[q] = &sv[q][lane * S];
            double *br = &sb[lane * S];
            for (int x = 0; x < cw; ++x) {
                const int k = x0 + x;
                if (k == 0) {
                    beta = br[0];
#pragma unroll
                    for (int q = 0; q < NP; ++q) {
                        prev[q] = vr[q][0] / beta;
                        vr[q][0] = prev[q];
                    }
                    continue;
                }
                const double ck = c[k - 1], ak = a[k - 1], bk = br[x];
                const double tk = ck / beta;
                br[x] = tk;
                beta = bk - ak * tk;
                const bool dd = fabs(beta) > tiny;
                double star[NP];
#pragma unroll
                for (int q = 0; q < NP; ++q) star[q] = (vr[q][x] - ak * prev[q]) / beta;
                if (dd) {
#pragma unroll
                    for (int q = 0; q < NP; ++q) prev[q] = star[q];
                } else if (keep_storage) {  // what the caller's ϕ held (batched_tridiagonal_solver.jl:224-228)
                    const long long o = base + (long long)lane * N + k;
#pragma unroll
                    for (int q = 0; q < NP; ++q) prev[q] = XParts<T>::get(phi, o, q);
                } else {
#pragma unroll
                    for (int q = 0; q < NP; ++q) prev[q] = 0.0;
                }
#pragma unroll
                for (int q = 0; q < NP; ++q) vr[q][x] = prev[q];
            }
        }
        __syncthreads();
        for (int e = lane; e < L * C; e += L) {
            const int l = e / C, x = e % C;
            if (l < nl && x < cw) {
                const long long o = base + (long long)l * N + x0 + x;
                double v[NP];
#pragma unroll
                for (int q = 0; q < NP; ++q) v[q] = sv[q][l * S + x];
                XParts<T>::put(phi, o, v);
                if (x0 + x > 0) t[o] = sb[l * S + x];
            }
        }
        __syncthreads();
    }

    // ---- back substitution, chunks downwards; prev holds ϕ[N-1]
    const int last = ((N - 1) / C) * C;
    for (int x0 = last; x0 >= 0; x0 -= C) {
        const int cw = (N - x0) < C ? (N - x0) : C;
        for (int e = lane; e < L * C; e += L) {
            const int l = e / C, x = e % C;
            if (l < nl && x < cw) {
                const long long o = base + (long long)l * N + x0 + x;
#pragma unroll
                for (int q = 0; q < NP; ++q) sv[q][l * S + x] = XParts<T>::get(phi, o, q);
                if (x0 + x + 1 < N) sb[l * S + x] = t[o + 1];
            }
        }
        __syncthreads();
        if (mine) {
            double *vr[NP];
#pragma unroll
            for (int q = 0; q < NP; ++q) vr[q] = &sv[q][lane * S];
            const double *tr = &sb[lane * S];
            for (int x = cw - 1; x >= 0; --x) {
                if (x0 + x > N - 2) continue;
                const double tk1 = tr[x];
#pragma unroll
                for (int q = 0; q < NP; ++q) {
                    const double cur = vr[q][x] - tk1 * prev[q];
                    vr[q][x] = cur;
                    prev[q] = cur;
                }
            }
        }
        __syncthreads();
        for (int e = lane; e < L * C; e += L) {
            const int l = e / C, x = e % C;
            if (l < nl && x < cw && x0 + x <= N - 2) {
                double v[NP];
#pragma unroll
                for (int q = 0; q < NP; ++q) v[q] = sv[q][l * S + x];
                XParts<T>::put(phi, base + (long long)l * N + x0 + x, v);
            }
        }
        __syncthreads();
    }
}

constexpr int X_CHUNK = 16;

int launch_tridiag_x(int N, long long nlines, const double *a, const double *b, const double *c, const double *f, double *t, double *phi,
                     hipStream_t stream, int keep_storage)
{
    if (nlines <= 0 || N <= 0) return OCN_SUCCESS;
    hipLaunchKernelGGL((tridiag_x_kernel<double2, X_CHUNK>), dim3((unsigned)((nlines + 63) / 64)), dim3(64), 0, stream, N, nlines, a, b, c,
                       reinterpret_cast<const double2 *>(f), t, reinterpret_cast<double2 *>(phi), keep_storage);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

int launch_tridiag_x_real(int N, long long nlines, const double *a, const double *b, const double *c, const double *f, double *t, double *phi,
                          hipStream_t stream, int keep_storage)
{
    if (nlines <= 0 || N <= 0) return OCN_SUCCESS;
    hipLaunchKernelGGL((tridiag_x_kernel<double, X_CHUNK>), dim3((unsigned)((nlines + 63) / 64)), dim3(64), 0, stream, N, nlines, a, b, c, f, t,
                       phi, keep_storage);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

// ---------------------------------------------------------------------------------------------------
// K15 compute_main_diagonal! XDirection / YDirection (fourier_tridiagonal_poisson_solver.jl:17-39) on the (Nx, Ny, Nz) layout of the
// spectrum; l1, l2: the (stored-order) eigenvalues of the two transformed directions in the order (x, y, z) without `dim`.
// dc, df: Δᶜ / Δᶠ of the stretched direction, element 0 <-> index 1 - H.
// ---------------------------------------------------------------------------------------------------
__global__ void main_diagonal_xy_kernel(int dim, int Nx, int Ny, int Nz, int H, const double *__restrict__ dc, const double *__restrict__ df,
                                        const double *__restrict__ l1, const double *__restrict__ l2, double *__restrict__ D)
{
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int n1 = dim == 0 ? Ny : Nx;
    if (q >= (long long)n1 * Nz) return;
    const int p1 = (int)(q % n1), k = (int)(q / n1);
    const double lam = l1[p1] + l2[k];
    const int N = dim == 0 ? Nx : Ny;
    const long long s = dim == 0 ? 1 : Nx;
    double *d = D + (dim == 0 ? (long long)Nx * (p1 + (long long)Ny * k) : p1 + (long long)Nx * Ny * k);
    auto dC = [&](int m) { return dc[m + H - 1]; };
    auto dF = [&](int m) { return df[m + H - 1]; };
    d[0] = -1 / dF(2) - dC(1) * lam;
    for (int m = 2; m <= N - 1; ++m) d[(m - 1) * s] = -(1 / dF(m + 1) + 1 / dF(m)) - dC(m) * lam;
    d[(N - 1) * s] = -1 / dF(N) - dC(N) * lam;
}

int launch_main_diagonal_xy(int dim, int Nx, int Ny, int Nz, int H, const double *dc, const double *df, const double *l1, const double *l2,
                            double *D, hipStream_t stream)
{
    const long long n = (long long)(dim == 0 ? Ny : Nx) * Nz;
    hipLaunchKernelGGL(main_diagonal_xy_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, dim, Nx, Ny, Nz, H, dc, df, l1, l2, D);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

// ---------------------------------------------------------------------------------------------------
// _fourier_tridiagonal_source_term! XDirection / YDirection (solve_for_pressure.jl:12-38): rhs = Δξᶜ divᶜᶜᶜ(U) / Δt, complex, with
// divᶜᶜᶜ (divergence_operators.jl:16-19) on the stretched spacing: Ax = Δy Δz, Ay = Δx Δz, Az = Δx Δy, V = Δx Δy Δz.  z is regular.
// perm_dim >= 0: the gather pass of the first cosine transform folded into the store (as source_term_kernel).
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ int dct_perm_s(int q, int N) { return (q & 1) ? N - 1 - (q - 1) / 2 : q / 2; }

__global__ __launch_bounds__(256) void source_term_stretched_kernel(GridDev g, int dim, const double *__restrict__ dc, const double *__restrict__ u,
                                                                    const double *__restrict__ v, const double *__restrict__ w, double dt,
                                                                    double2 *__restrict__ out, int perm_dim)
{
    const int i = 1 + blockIdx.x * blockDim.x + threadIdx.x;
    const int j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    const int k = 1 + blockIdx.z;
    if (i > g.Nx || j > g.Ny) return;
    const Lay Lu = make_lay(g, OCN_LOC_FCC), Lv = make_lay(g, OCN_LOC_CFC), Lw = make_lay(g, OCN_LOC_CCF);
    const double dx = dim == 0 ? dc[i + g.Hx - 1] : g.dx;
    const double dy = dim == 1 ? dc[j + g.Hy - 1] : g.dy;
    const double dz = g.dz;
    const double Ax = dy * dz, Ay = dx * dz, Az = dx * dy;
    const double dxu = (g.tx == OCN_FLAT) ? 0.0 : Ax * u[at(Lu, i + 1, j, k)] - Ax * u[at(Lu, i, j, k)];
    const double dyv = (g.ty == OCN_FLAT) ? 0.0 : Ay * v[at(Lv, i, j + 1, k)] - Ay * v[at(Lv, i, j, k)];
    const double dzw = (g.tz == OCN_FLAT) ? 0.0 : Az * w[at(Lw, i, j, k + 1)] - Az * w[at(Lw, i, j, k)];
    const double d = (1 / (Az * dz)) * ((dxu + dyv) + dzw);
    const double r = ((dim == 0 ? dx : dy) * d) / dt;
    int cc[3] = {i - 1, j - 1, k - 1};
    if (perm_dim >= 0) cc[perm_dim] = dct_perm_s(cc[perm_dim], perm_dim == 0 ? g.Nx : perm_dim == 1 ? g.Ny : g.Nz);
    out[cc[0] + (long long)g.Nx * (cc[1] + (long long)g.Ny * cc[2])] = make_double2(r, 0.0);
}

int launch_source_term_stretched(const ocn_grid *grid, int dim, const double *dc, const double *u, const double *v, const double *w, double dt,
                                 double *out, int perm_dim, hipStream_t stream)
{
    GridDev g = to_dev(*grid);
    hipLaunchKernelGGL(source_term_stretched_kernel, dim3((g.Nx + 63) / 64, (g.Ny + 3) / 4, g.Nz), dim3(64, 4), 0, stream, g, dim, dc, u, v, w, dt,
                       reinterpret_cast<double2 *>(out), perm_dim);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

// set_source_term! (fourier_tridiagonal_poisson_solver.jl:155-177, multiply_by_stretched_spacing! of YZRegularRG / XZRegularRG):
// storage <- R Δξᶜ, widened to complex
__global__ void set_source_stretched_kernel(int Nx, int Ny, int Nz, const double *__restrict__ R, int dim, const double *__restrict__ dc, int H,
                                            double2 *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y, k = blockIdx.z;
    if (i >= Nx) return;
    const long long o = i + (long long)Nx * (j + (long long)Ny * k);
    const double r = R[o] * dc[(dim == 0 ? i : j) + H];
    out[o] = make_double2(r, 0.0);
}

int launch_set_source_stretched(int Nx, int Ny, int Nz, const double *R, int dim, const double *dc, int H, double *out, hipStream_t stream)
{
    hipLaunchKernelGGL(set_source_stretched_kernel, dim3((Nx + 63) / 64, Ny, Nz), dim3(64), 0, stream, Nx, Ny, Nz, R, dim, dc, H,
                       reinterpret_cast<double2 *>(out));
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

}  // namespace ocn
