// poisson_general.hip -- the kernels of the any-topology FFT-based solver (poisson.hip drives them; poisson_dist.hip borrows the shuffle) and
// their launchers.
#include "poisson_internal.h"

// ---------------------------------------------------------------------------------------------------------------------------------
// kind 2: FFTBasedPoissonSolver on ANY regular topology (fft_based_poisson_solver.jl:5-125 with the transforms of plan_transforms.jl:16-34,
// 129-140: Bounded dimensions first, then Periodic ones; backward in the opposite order).  The reference's GPU path builds the cosine
// transforms from FFTs with index permutations and twiddle factors (K11: index_permutations.jl:38-90, discrete_transforms.jl:141-176);
// here every 1-D transform is the direct sum of its definition over a table of cos / sin values computed on the host in fp64:
//   Periodic forward  X[k] = Σ_n x[n] e^{-2πi k n / N}                      backward x[n] = (1/N) Σ_k X[k] e^{+2πi k n / N}
//   Bounded  forward  X[k] = 2 Σ_n x[n] cos(π (n + 1/2) k / N)  (REDFT10)    backward x[n] = (1/2N) (X[0] + 2 Σ_{k>=1} X[k] cos(π (n + 1/2) k / N))
// O(N) work per output element: this path serves the Bounded-x / Bounded-y topologies of test_poisson_solvers.jl:58-106, which no
// BASELINE configuration uses (their fields are not implemented by the tendency kernels either); it is exact to N eps, not tuned.
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void naive_transform_kernel(int Nx, int Ny, int Nz, int dim, int topo, int inverse, const double2 *__restrict__ in,
                                                              double2 *__restrict__ out, const double *__restrict__ ctab,
                                                              const double *__restrict__ stab)
{
    const long long n = (long long)Nx * Ny * Nz, t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int i = (int)(t % Nx), j = (int)((t / Nx) % Ny), k = (int)(t / ((long long)Nx * Ny));
    const int N = dim == 0 ? Nx : dim == 1 ? Ny : Nz, q = dim == 0 ? i : dim == 1 ? j : k;  // q: output index along the transformed dimension
    const long long stride = dim == 0 ? 1 : dim == 1 ? Nx : (long long)Nx * Ny;
    const double2 *line = in + (t - q * stride);
    double re = 0.0, im = 0.0;
    if (topo == OCN_PERIODIC) {
        for (int m = 0; m < N; ++m) {
            const int idx = (int)(((long long)q * m) % N);
            const double c = ctab[idx], sn = inverse ? stab[idx] : -stab[idx];
            const double2 v = line[m * stride];
            re += v.x * c - v.y * sn;
            im += v.x * sn + v.y * c;
        }
        if (inverse) { re /= N; im /= N; }
    } else {  // Bounded: cosine transforms of the real and imaginary parts; table index (2 n + 1) k mod 4N of cos(π idx / 2N)
        if (!inverse) {
            for (int m = 0; m < N; ++m) {
                const double c = ctab[(int)(((long long)(2 * m + 1) * q) % (4 * N))];
                const double2 v = line[m * stride];
                re += v.x * c;
                im += v.y * c;
            }
            re *= 2; im *= 2;
        } else {
            for (int m = 1; m < N; ++m) {
                const double c = ctab[(int)(((long long)(2 * q + 1) * m) % (4 * N))];
                const double2 v = line[m * stride];
                re += v.x * c;
                im += v.y * c;
            }
            const double2 v0 = line[0];
            re = (v0.x + 2 * re) / (2 * N);
            im = (v0.y + 2 * im) / (2 * N);
        }
    }
    out[t] = make_double2(re, im);
}

// ---- the same transforms from FFTs (Makhoul 1980; the reference's GPU path K11) ------------------------------------------------
// REDFT10 of a line x[0..N):  v[n] = x[2n] (n < ceil(N/2)),  v[N-1-n] = x[2n+1];  V = FFT_N(v);  X[k] = 2 Re(w_k V[k]), w_k = e^{-iπk/2N}.
// The lines here are complex (earlier dimensions are already in spectral space): the real and imaginary parts are two real lines
// transformed by ONE complex FFT and separated through the Hermitian symmetry of their spectra,
//     X[k] = Re(w_k (V[k] + conj V[N-k]))  +  i Im(w_k (V[k] - conj V[N-k])).
// REDFT01 / 2N (the inverse):  V[k] = (1/2) conj(w_k) (X[k] - i X[N-k]),  X[N] := 0;  v = IFFT_N(V) / N;  x[2n] = v[n], x[2n+1] = v[N-1-n].
// mode 0: gather (x -> v), 1: forward post-twiddle (V -> X), 2: inverse pre-twiddle (X -> V), 3: scatter (v -> x); out of place.
// partner != NULL: the spectrum along `dim` is in the column kernels' stage order (position p holds wavenumber k(p)): w[p] = w_k(p),
// partner[p] = position of wavenumber N - k(p) (position 0 is wavenumber 0 in either order).
__global__ __launch_bounds__(256) void dct_shuffle_kernel(int Nx, int Ny, int Nz, int dim, int mode, const double2 *__restrict__ in,
                                                          double2 *__restrict__ out, const double2 *__restrict__ w,
                                                          const int *__restrict__ partner)
{
    const long long n = (long long)Nx * Ny * Nz, t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int i = (int)(t % Nx), j = (int)((t / Nx) % Ny), k = (int)(t / ((long long)Nx * Ny));
    const int N = dim == 0 ? Nx : dim == 1 ? Ny : Nz, q = dim == 0 ? i : dim == 1 ? j : k;
    const long long stride = dim == 0 ? 1 : dim == 1 ? Nx : (long long)Nx * Ny;
    const double2 *line = in + (t - q * stride);
    const int half = (N + 1) / 2;
    if (mode == 0) {         // v[q]
        out[t] = q < half ? line[(long long)(2 * q) * stride] : line[(long long)(2 * (N - 1 - q) + 1) * stride];
    } else if (mode == 3) {  // x[q]
        out[t] = (q & 1) ? line[(long long)(N - 1 - (q - 1) / 2) * stride] : line[(long long)(q / 2) * stride];
    } else if (mode == 1) {
        const int qp = partner ? partner[q] : (N - q) % N;
        const double2 a = line[(long long)q * stride], b = line[(long long)qp * stride], wk = w[q];
        const double sr = a.x + b.x, si = a.y - b.y;  // V[k] + conj V[N-k]
        const double dr = a.x - b.x, di = a.y + b.y;  // V[k] - conj V[N-k]
        out[t] = make_double2(wk.x * sr - wk.y * si, wk.x * di + wk.y * dr);
    } else {
        const double2 a = line[(long long)q * stride];
        const double2 b = q == 0 ? make_double2(0.0, 0.0) : line[(long long)(partner ? partner[q] : N - q) * stride];
        const double2 wk = w[q];
        const double zr = a.x + b.y, zi = a.y - b.x;  // X[k] - i X[N-k]
        out[t] = make_double2(0.5 * (wk.x * zr + wk.y * zi), 0.5 * (wk.x * zi - wk.y * zr));  // (1/2) conj(w_k) z
    }
}

// The same four passes for the lines ALONG x of a REAL array (Nx, Ny, Nz), Ny even: the complex line (i, jp, k), jp < Ny / 2, is the pair of real
// rows j = 2 jp (real part) and 2 jp + 1 (imaginary part) -- a cosine transform maps reals to reals, and the complex transform of a line is the
// transform of its real and of its imaginary part, so two rows ride on one complex FFT.  Modes 0 and 2 read the real array (split: the two
// parts Nx doubles apart) and write an interleaved complex array (Nx, Ny / 2, Nz) for the line FFTs; modes 1 and 3 read that and write the
// real array.  Natural wavenumber order (rocFFT lines).
__global__ __launch_bounds__(256) void dct_rowpair_kernel(int Nx, int Nyp, int Nz, int mode, const double *__restrict__ in, double *__restrict__ out,
                                                          const double2 *__restrict__ w)
{
    const long long n = (long long)Nx * Nyp * Nz, t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int q = (int)(t % Nx), jp = (int)((t / Nx) % Nyp), k = (int)(t / ((long long)Nx * Nyp));
    const int N = Nx, half = (N + 1) / 2;
    const long long row = (long long)Nx * (2 * jp + (long long)2 * Nyp * k);  // the real row j = 2 jp of plane k; the odd row follows at + Nx
    const double2 *cin = reinterpret_cast<const double2 *>(in) + (t - q);      // the interleaved complex line
    double2 *cout = reinterpret_cast<double2 *>(out);
    auto split_in = [&](int m) { return make_double2(in[row + m], in[row + Nx + m]); };
    auto split_out = [&](double2 v) { out[row + q] = v.x; out[row + Nx + q] = v.y; };
    if (mode == 0) {         // v[q], real rows -> complex
        cout[t] = q < half ? split_in(2 * q) : split_in(2 * (N - 1 - q) + 1);
    } else if (mode == 3) {  // x[q], complex -> real rows
        split_out((q & 1) ? cin[N - 1 - (q - 1) / 2] : cin[q / 2]);
    } else if (mode == 1) {  // post-twiddle, complex -> real rows
        const double2 a = cin[q], b = cin[(N - q) % N], wk = w[q];
        const double sr = a.x + b.x, si = a.y - b.y, dr = a.x - b.x, di = a.y + b.y;
        split_out(make_double2(wk.x * sr - wk.y * si, wk.x * di + wk.y * dr));
    } else {                 // pre-twiddle, real rows -> complex
        const double2 a = split_in(q);
        const double2 b = q == 0 ? make_double2(0.0, 0.0) : split_in(N - q);
        const double2 wk = w[q];
        const double zr = a.x + b.y, zi = a.y - b.x;
        cout[t] = make_double2(0.5 * (wk.x * zr + wk.y * zi), 0.5 * (wk.x * zi - wk.y * zr));
    }
}

// -b / (λx + λy + λz [- m]) of a REAL spectrum (every direction a cosine transform), mode (1, 1, 1) := 0 iff m === 0
__global__ __launch_bounds__(256) void spectral_solve_real_kernel(int Nx, int Ny, int Nz, const double *__restrict__ lx, const double *__restrict__ ly,
                                                                  const double *__restrict__ lz, double *__restrict__ b, double m, int shifted)
{
    const long long n = (long long)Nx * Ny * Nz, t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int i = (int)(t % Nx), j = (int)((t / Nx) % Ny), k = (int)(t / ((long long)Nx * Ny));
    double lam = (lx[i] + ly[j]) + lz[k];
    if (shifted) lam = lam - m;
    double val = -b[t] / lam;
    if (!shifted && t == 0) val = 0.0;
    b[t] = val;
}

// A twiddle pass along `dt` (mode mt = 1 forward post-twiddle, 2 inverse pre-twiddle) and a pure permutation along ANOTHER dimension
// `dp` (mode mp = 0 gather, 3 scatter) in ONE pass: the permutation only relabels whole lines of the twiddle direction, so
//   forward:  out = gather_dp(twiddle_dt(in)),   inverse:  out = pretwiddle_dt(scatter_dp(in))
// both read `in` at the permuted position of the output point (and at its N - k partner along dt).
__global__ __launch_bounds__(256) void dct_twiddle_permute_kernel(int Nx, int Ny, int Nz, int dt, int mt, int dp, int mp,
                                                                  const double2 *__restrict__ in, double2 *__restrict__ out,
                                                                  const double2 *__restrict__ w, const int *__restrict__ partner)
{
    const long long n = (long long)Nx * Ny * Nz, t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int idx[3] = {(int)(t % Nx), (int)((t / Nx) % Ny), (int)(t / ((long long)Nx * Ny))};
    const int Ns[3] = {Nx, Ny, Nz};
    const long long strides[3] = {1, Nx, (long long)Nx * Ny};
    // the permuted source position along dp
    const int Np = Ns[dp], qp = idx[dp], half = (Np + 1) / 2;
    const int sp = mp == 0 ? (qp < half ? 2 * qp : 2 * (Np - 1 - qp) + 1) : ((qp & 1) ? Np - 1 - (qp - 1) / 2 : qp / 2);
    const long long src = t + (long long)(sp - qp) * strides[dp];
    const int N = Ns[dt], q = idx[dt];
    const long long st = strides[dt];
    const double2 *line = in + (src - q * st);
    const double2 a = line[(long long)q * st], wk = w[q];
    if (mt == 1) {
        const int qq = partner ? partner[q] : (N - q) % N;
        const double2 b = line[(long long)qq * st];
        const double sr = a.x + b.x, si = a.y - b.y, dr = a.x - b.x, di = a.y + b.y;
        out[t] = make_double2(wk.x * sr - wk.y * si, wk.x * di + wk.y * dr);
    } else {
        const double2 b = q == 0 ? make_double2(0.0, 0.0) : line[(long long)(partner ? partner[q] : N - q) * st];
        const double zr = a.x + b.y, zi = a.y - b.x;
        out[t] = make_double2(0.5 * (wk.x * zr + wk.y * zi), 0.5 * (wk.x * zi - wk.y * zr));
    }
}

namespace ocn {
namespace poisson {

static inline const double2 *c2(const double *p) { return reinterpret_cast<const double2 *>(p); }
static inline double2 *c2(double *p) { return reinterpret_cast<double2 *>(p); }
static inline dim3 blocks(long long n) { return dim3((unsigned)((n + 255) / 256)); }

int launch_naive_transform(const int n[3], int dim, int topo, int inverse, const double *in, double *out, const double *ctab, const double *stab,
                           hipStream_t stream)
{
    hipLaunchKernelGGL(naive_transform_kernel, blocks((long long)n[0] * n[1] * n[2]), dim3(256), 0, stream, n[0], n[1], n[2], dim, topo, inverse,
                       c2(in), c2(out), ctab, stab);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

int launch_dct_shuffle(const int n[3], int dim, DctShuffle mode, const double *in, double *out, const double *w, const int *partner,
                       hipStream_t stream)
{
    hipLaunchKernelGGL(dct_shuffle_kernel, blocks((long long)n[0] * n[1] * n[2]), dim3(256), 0, stream, n[0], n[1], n[2], dim, (int)mode, c2(in),
                       c2(out), c2(w), partner);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

int launch_dct_twiddle_permute(const int n[3], int dt, DctShuffle mt, int dp, DctShuffle mp, const double *in, double *out, const double *w,
                               const int *partner, hipStream_t stream)
{
    hipLaunchKernelGGL(dct_twiddle_permute_kernel, blocks((long long)n[0] * n[1] * n[2]), dim3(256), 0, stream, n[0], n[1], n[2], dt, (int)mt, dp,
                       (int)mp, c2(in), c2(out), c2(w), partner);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

// n: the extents of the complex view (Nx, Ny / 2, Nz)
int launch_dct_rowpair(const int n[3], DctShuffle mode, const double *in, double *out, const double *w, hipStream_t stream)
{
    hipLaunchKernelGGL(dct_rowpair_kernel, blocks((long long)n[0] * n[1] * n[2]), dim3(256), 0, stream, n[0], n[1], n[2], (int)mode, in, out, c2(w));
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

int launch_spectral_solve_real(const int n[3], const double *lx, const double *ly, const double *lz, double *b, double m, int shifted,
                               hipStream_t stream)
{
    hipLaunchKernelGGL(spectral_solve_real_kernel, blocks((long long)n[0] * n[1] * n[2]), dim3(256), 0, stream, n[0], n[1], n[2], lx, ly, lz, b, m,
                       shifted);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

}  // namespace poisson
}  // namespace ocn
