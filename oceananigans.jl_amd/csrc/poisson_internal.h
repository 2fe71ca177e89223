// poisson_internal.h -- shared by the translation units of the pressure solvers (poisson.hip, poisson_general.hip,
// poisson_selftest.hip, poisson_dist.hip): rocFFT plumbing, small upload helpers, the single-device handle.
#pragma once
#include <rocfft/rocfft.h>

#include <cmath>
#include <cstdlib>
#include <memory>
#include <vector>

#include "ocn_internal.h"
#include "poisson_select.h"

#define OCN_CHECK_FFT(expr)                                                                        \
    do {                                                                                           \
        rocfft_status _s = (expr);                                                                 \
        if (_s != rocfft_status_success) {                                                         \
            ocn::set_error("%s failed with rocfft_status %d (%s:%d)", #expr, (int)_s, __FILE__, __LINE__); \
            return OCN_ERR_ROCFFT;                                                                 \
        }                                                                                          \
    } while (0)

// Creation code: return on failure.  The handle under construction is held by a unique_ptr whose deleter frees its device memory
// and plans, so these need no cleanup of their own.
#define TRY(expr)                           \
    do {                                    \
        int _st = (expr);                   \
        if (_st != OCN_SUCCESS) return _st; \
    } while (0)
#define TRY_HIP(expr)                                                      \
    do {                                                                   \
        hipError_t _e = (expr);                                            \
        if (_e != hipSuccess) {                                            \
            ocn::set_error("%s failed: %s", #expr, hipGetErrorString(_e)); \
            return OCN_ERR_ALLOC;                                          \
        }                                                                  \
    } while (0)

namespace ocn {
namespace poisson {

struct FFTSetup {
    FFTSetup() { rocfft_setup(); }
    ~FFTSetup() { rocfft_cleanup(); }
};
inline void ensure_rocfft()
{
    static FFTSetup s;
    (void)s;
}

// poisson_eigenvalues (poisson_eigenvalues.jl:8-31)
inline std::vector<double> eigenvalues(int N, double L, int topo)
{
    std::vector<double> lam(N, 0.0);
    const double pi = 3.141592653589793;
    for (int q = 0; q < N; ++q) {
        if (topo == OCN_PERIODIC || topo == OCN_FULLY_CONNECTED) {
            const double s = 2 * std::sin(q * pi / N) / (L / N);
            lam[q] = s * s;
        } else if (topo == OCN_BOUNDED) {
            const double s = 2 * std::sin(q * pi / (2 * N)) / (L / N);
            lam[q] = s * s;
        }
    }
    return lam;
}

// wavenumber of each stored position: the column kernel's stage order, or the natural one
inline std::vector<int> stored_wavenumbers(int N, bool stage_order)
{
    std::vector<int> k(N);
    for (int p = 0; p < N; ++p) k[p] = stage_order ? colfft_wavenumber(N, p) : p;
    return k;
}
inline std::vector<double> permuted(const std::vector<double> &natural, const std::vector<int> &kofp)
{
    std::vector<double> v(kofp.size());
    for (size_t p = 0; p < kofp.size(); ++p) v[p] = natural[kofp[p]];
    return v;
}
// stored position of wavenumber N - k(p), which the twiddle passes of a cosine transform pair with position p
inline std::vector<int> partner_positions(const std::vector<int> &kofp)
{
    const int N = (int)kofp.size();
    std::vector<int> pofk(N), partner(N);
    for (int p = 0; p < N; ++p) pofk[kofp[p]] = p;
    for (int p = 0; p < N; ++p) partner[p] = pofk[(N - kofp[p]) % N];
    return partner;
}
// w_k = e^{-iπk/2N} of the cosine transforms (Makhoul 1980), by stored position
inline std::vector<double> cosine_twiddles(int N, const std::vector<int> &kofp)
{
    std::vector<double> w(2 * (size_t)N);
    for (int p = 0; p < N; ++p) {
        const long double a = 3.14159265358979323846264338327950288L * kofp[p] / (2.0L * N);
        w[2 * p] = (double)cosl(a);
        w[2 * p + 1] = (double)(-sinl(a));
    }
    return w;
}

template <class T>
int upload(const std::vector<T> &h, T **d)
{
    OCN_CHECK_HIP(hipMalloc(reinterpret_cast<void **>(d), h.size() * sizeof(T)));
    OCN_CHECK_HIP(hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return OCN_SUCCESS;
}

struct Plan {
    rocfft_plan plan = nullptr;
    rocfft_execution_info info = nullptr;
    void *work = nullptr;
    size_t work_bytes = 0;
    int finish()
    {
        OCN_CHECK_FFT(rocfft_plan_get_work_buffer_size(plan, &work_bytes));
        OCN_CHECK_FFT(rocfft_execution_info_create(&info));
        if (work_bytes) {
            OCN_CHECK_HIP(hipMalloc(&work, work_bytes));
            OCN_CHECK_FFT(rocfft_execution_info_set_work_buffer(info, work, work_bytes));
        }
        return OCN_SUCCESS;
    }
    int exec(void *in, void *out, hipStream_t stream)
    {
        OCN_CHECK_FFT(rocfft_execution_info_set_stream(info, stream));
        void *ib[1] = {in};
        void *ob[1] = {out};
        OCN_CHECK_FFT(rocfft_execute(plan, ib, out ? ob : nullptr, info));
        return OCN_SUCCESS;
    }
    void destroy()
    {
        // Plans are destroyed eagerly.  rocFFT (ROCm 7.2) real-transform plans collide with OTHER LIVE real plans: a power-of-two
        // pair whose 2-D (x, y) kernel lengths are the transpose of an existing plan's -- (Nx/2, Ny) = (Ny', Nx'/2), e.g. 16 x 16 x k
        // alive, then 32 x 8 x k, or 64^3 then 128 x 32 -- comes out wrong (forward spectrum, inverse, or both; the earlier plan stays
        // correct), and destroying the first plan BEFORE creating the second cures it (tools/rocfft_repro.hip,
        // profiles/r02_rocfft_repro.md).  Keeping dead plans alive therefore only widens the exposure; every new pair is additionally
        // verified against known answers over its full spectrum at creation (poisson_selftest.hip) and replaced by complex plans
        // if it fails.  OCN_ROCFFT_RETIRE_PLANS=1 restores round 1's behaviour (objects kept until the process ends).
        static const bool retire = env_set("OCN_ROCFFT_RETIRE_PLANS");
        if (!retire) {
            if (plan) rocfft_plan_destroy(plan);
            if (info) rocfft_execution_info_destroy(info);
        }
        if (work) (void)hipFree(work);
        plan = nullptr; info = nullptr; work = nullptr;
    }
};

// Generic plan helper.  dims-long arrays; strides in elements.
inline int make_plan(Plan &P, rocfft_result_placement placement, rocfft_transform_type type, int dims, const size_t *lengths, size_t batch,
                     rocfft_array_type in_type, rocfft_array_type out_type, const size_t *in_strides, size_t in_dist,
                     const size_t *out_strides, size_t out_dist, double scale)
{
    rocfft_plan_description desc = nullptr;
    OCN_CHECK_FFT(rocfft_plan_description_create(&desc));
    OCN_CHECK_FFT(rocfft_plan_description_set_data_layout(desc, in_type, out_type, nullptr, nullptr, dims, in_strides, in_dist,
                                                          dims, out_strides, out_dist));
    if (scale != 1.0) OCN_CHECK_FFT(rocfft_plan_description_set_scale_factor(desc, scale));
    OCN_CHECK_FFT(rocfft_plan_create(&P.plan, placement, type, rocfft_precision_double, dims, lengths, batch, desc));
    OCN_CHECK_FFT(rocfft_plan_description_destroy(desc));
    return P.finish();
}

// poisson_general.hip: launchers of the any-topology kernels (complex arrays as interleaved doubles)
int launch_naive_transform(const int n[3], int dim, int topo, int inverse, const double *in, double *out, const double *ctab, const double *stab,
                           hipStream_t stream);
int launch_dct_shuffle(const int n[3], int dim, DctShuffle mode, const double *in, double *out, const double *w, const int *partner,
                       hipStream_t stream);
int launch_dct_twiddle_permute(const int n[3], int dt, DctShuffle mt, int dp, DctShuffle mp, const double *in, double *out, const double *w,
                               const int *partner, hipStream_t stream);
int launch_dct_rowpair(const int n[3], DctShuffle mode, const double *in, double *out, const double *w, hipStream_t stream);
int launch_spectral_solve_real(const int n[3], const double *lx, const double *ly, const double *lz, double *b, double m, int shifted,
                               hipStream_t stream);

}  // namespace poisson
}  // namespace ocn

// ===================================================================================================
// The single-device solver.  Which pipeline it runs is recorded in the three pass lists (poisson_select.h); the arrays below are
// what the passes read, indexed by direction where a pass carries one.  No member says which pipeline this is.
// ===================================================================================================
struct ocn_poisson {
    ocn_grid grid{};  // dzc / dzf point at the handle's own copies
    ocn::poisson::PassLists passes;
    int info[3] = {0, 0, 0};          // what ocn_poisson_info reports: kind, r2c, the bit-packed direct_out
    bool source_wrap = false;         // read by ocn_poisson_source_wraps: the drivers skip the velocity halo fill in front of the solve
    const char *unshiftable = nullptr;  // read by ocn_poisson_solve_shifted: why the screened equation is not available, or NULL
    // ---- per-call state, read by the executor
    bool source_set = false;       // ocn_poisson_solve: a source term has been given
    bool source_in_rhs = false;    // the source is a real array (set_source_term!) that still awaits its x transform
    bool gathered = false;         // the source pass stored its output already gathered along the first cosine-transform direction
    double shift = 0.0;            // ocn_poisson_solve_shifted: (∇² + m) ϕ = b for this solve
    bool shifted = false;          // ... with m = shift, and no zero-mode gauge (m === 0 is the plain solve)
    // ---- arrays
    double *rhs = nullptr;                 // real Nx Ny Nz: the source of the real rocFFT plans and of the row kernel
    double *spec = nullptr, *spec2 = nullptr;  // the pair the passes alternate between; spec is where the next source goes
    double *lam[3] = {nullptr, nullptr, nullptr};     // eigenvalues, in the order the passes that read them store that direction
    double *coltw[3] = {nullptr, nullptr, nullptr};   // twiddles of the column / row kernel along d
    double *costw[3] = {nullptr, nullptr, nullptr};   // w_k = e^{-iπk/2N} of the cosine transform along d, by stored position
    int *partner[3] = {nullptr, nullptr, nullptr};    // stage order: stored position of wavenumber N - k(p)
    double *tab[3][2] = {{nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}};  // cos / sin tables of the direct sums
    double *twMx = nullptr, *twNx = nullptr;          // twiddles of the row FFT kernel
    double *tdc = nullptr, *tdf = nullptr;            // own copies of the spacings along the sweep direction (ocn_grid.dzc / dzf layout)
    double *lower = nullptr, *diag = nullptr, *tscr = nullptr;  // Thomas sweep: off-diagonal, main diagonal, scratch
    ocn::poisson::Plan fwd, bwd;            // rocFFT (x, y[, z]) plans
    ocn::poisson::Plan xr2c, xc2r;          // real x lines of the packed pipeline
    ocn::poisson::Plan line_fwd[3], line_bwd[3];  // complex lines along d

    ~ocn_poisson();  // frees the arrays and destroys the plans
};

namespace ocn {
namespace poisson {
// poisson_selftest.hip: known-answer checks of rocFFT plans, run at creation right after the plans they check
struct PlanCheck {
    bool c2c, dims3, fused_z, direct_out;
    int nxh;
};
int plans_self_test(ocn_poisson *s, const PlanCheck &c);
int packed_plans_self_test(ocn_poisson *s);
}  // namespace poisson
}  // namespace ocn
