// poisson_selftest.hip -- known-answer checks of rocFFT plans, run at creation right after the plans they check.  rocFFT real-transform
// plans have been observed to return wrong results when certain other real plans already exist in the process (Plan::destroy,
// poisson_internal.h): a failing real pair is replaced by complex plans, a failing complex pair is an error.
#include <algorithm>

#include "poisson_internal.h"

namespace ocn {
namespace poisson {

// Known-answer checks of a forward transform over the FULL spectrum.  The round trip alone does not catch a forward / inverse pair
// that is wrong in a mutually consistent way, and a sample of entries misses permuted spectra.
//  (a) plane waves, any grid size, O(n): the input is a sum of NW real plane waves with distinct amplitudes and phases whose DFT is
//      known in closed form (two conjugate deltas per wave, folded into the half spectrum); every entry of the device spectrum is
//      compared with it.
//  (b) grids of at most 2^16 points: a pseudo-random field against a separable DFT evaluated on the host.
// spec(kx, ky, kz) at kx + nxh (ky + Ny kz); dims3 = the plan transforms z as well (otherwise z is the batch index).
struct Wave {
    int kx, ky, kz;
    double amp, phase;
};
static std::vector<Wave> test_waves(int Nx, int Ny, int Nz, bool dims3)
{
    std::vector<Wave> w;
    unsigned long long x = 0xD1B54A32D192ED03ull;
    auto next = [&]() { x = x * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(x >> 33); };
    for (int q = 0; q < 12; ++q)
        w.push_back(Wave{(int)(next() % (unsigned)Nx), (int)(next() % (unsigned)Ny), dims3 ? (int)(next() % (unsigned)Nz) : 0, 0.5 + 0.125 * q,
                         0.37 * q + 0.11});
    w.push_back(Wave{1 % Nx, 0, 0, 1.7, 0.3});         // the axes, the Nyquist lines and the mean, each with its own amplitude
    w.push_back(Wave{0, 1 % Ny, 0, 2.3, -0.4});
    w.push_back(Wave{Nx / 2, Ny / 2, dims3 ? Nz / 2 : 0, 2.9, 0.0});
    w.push_back(Wave{0, 0, 0, 3.1, 0.0});
    if (dims3) w.push_back(Wave{0, 0, 1 % Nz, 3.7, 0.9});
    return w;
}
// in[i,j,k] = sum_w amp cos(2 pi (kx i / Nx + ky j / Ny + kz k / Nz) + phase)  [2-D plans: every z plane gets (1 + k) x the field]
static void fill_waves(std::vector<double> &in, const std::vector<Wave> &W, int Nx, int Ny, int Nz, bool dims3)
{
    const double two_pi = 6.283185307179586476925286766559;
    std::fill(in.begin(), in.end(), 0.0);
    for (const Wave &w : W) {
        std::vector<double> cx(Nx), sx(Nx), cy(Ny), sy(Ny), cz(Nz), sz(Nz);
        for (int i = 0; i < Nx; ++i) { const double a = two_pi * (double)((long long)w.kx * i % Nx) / Nx; cx[i] = std::cos(a); sx[i] = std::sin(a); }
        for (int j = 0; j < Ny; ++j) { const double a = two_pi * (double)((long long)w.ky * j % Ny) / Ny; cy[j] = std::cos(a); sy[j] = std::sin(a); }
        for (int k = 0; k < Nz; ++k) { const double a = dims3 ? two_pi * (double)((long long)w.kz * k % Nz) / Nz : 0.0; cz[k] = std::cos(a); sz[k] = std::sin(a); }
        const double cp = std::cos(w.phase), sp = std::sin(w.phase);
        for (int k = 0; k < Nz; ++k) {
            const double scale = dims3 ? 1.0 : 1.0 + k;
            for (int j = 0; j < Ny; ++j) {
                // cos(a + b + c + phase) with a = x angle, (b, c, phase) folded into (C, S): cos(a) C - sin(a) S
                const double cyz = cy[j] * cz[k] - sy[j] * sz[k], syz = sy[j] * cz[k] + cy[j] * sz[k];
                const double Cc = cyz * cp - syz * sp, Ss = syz * cp + cyz * sp;
                double *row = &in[(size_t)Nx * (j + (size_t)Ny * k)];
                for (int i = 0; i < Nx; ++i) row[i] += scale * w.amp * (cx[i] * Cc - sx[i] * Ss);
            }
        }
    }
}
// max |device spectrum - closed form| over every stored entry
static double wave_spectrum_error(const std::vector<double> &spec, const std::vector<Wave> &W, int Nx, int Ny, int Nz, int nxh, bool dims3)
{
    std::vector<double> ex(spec.size(), 0.0);
    const double count = (double)Nx * Ny * (dims3 ? Nz : 1);
    for (const Wave &w : W) {
        // amp cos(theta + phase) = amp/2 (e^{i phase} e^{i theta} + c.c.): delta at +k with amp/2 e^{i phase}, at -k with the conjugate
        for (int sgn = 0; sgn < 2; ++sgn) {
            const int kx = sgn ? (Nx - w.kx) % Nx : w.kx, ky = sgn ? (Ny - w.ky) % Ny : w.ky, kz = sgn ? (Nz - w.kz) % Nz : w.kz;
            if (kx >= nxh) continue;  // the other half of the Hermitian spectrum is not stored
            const double re = 0.5 * w.amp * std::cos(w.phase) * count, im = (sgn ? -1.0 : 1.0) * 0.5 * w.amp * std::sin(w.phase) * count;
            for (int k = 0; k < (dims3 ? 1 : Nz); ++k) {
                const size_t o = 2 * ((size_t)kx + (size_t)nxh * (ky + (size_t)Ny * (dims3 ? kz : k)));
                const double scale = dims3 ? 1.0 : 1.0 + k;
                ex[o] += scale * re;
                ex[o + 1] += scale * im;
            }
        }
    }
    double worst = 0.0;
    for (size_t q = 0; q < ex.size(); ++q) worst = std::fmax(worst, std::fabs(ex[q] - spec[q]));
    return worst;
}
// full separable host DFT of a small real field -> max error over every stored entry
static double full_spectrum_error(const std::vector<double> &in, const std::vector<double> &spec, int Nx, int Ny, int Nz, int nxh, bool dims3)
{
    const double two_pi = 6.283185307179586476925286766559;
    const size_t m = (size_t)nxh * Ny * Nz;
    std::vector<double> a(2 * m), b(2 * m);
    for (int k = 0; k < Nz; ++k)
        for (int j = 0; j < Ny; ++j)
            for (int kx = 0; kx < nxh; ++kx) {
                double re = 0, im = 0;
                for (int i = 0; i < Nx; ++i) {
                    const double ph = -two_pi * (double)((long long)kx * i % Nx) / Nx, v = in[i + (size_t)Nx * (j + (size_t)Ny * k)];
                    re += v * std::cos(ph);
                    im += v * std::sin(ph);
                }
                const size_t o = 2 * (kx + (size_t)nxh * (j + (size_t)Ny * k));
                a[o] = re; a[o + 1] = im;
            }
    auto pass = [&](std::vector<double> &src, std::vector<double> &dst, int N, size_t stride, size_t outer_stride, size_t n_outer, size_t n_inner) {
        for (size_t oo = 0; oo < n_outer; ++oo)
            for (size_t ii = 0; ii < n_inner; ++ii)
                for (int kk = 0; kk < N; ++kk) {
                    double re = 0, im = 0;
                    for (int q = 0; q < N; ++q) {
                        const double ph = -two_pi * (double)((long long)kk * q % N) / N, c = std::cos(ph), sn = std::sin(ph);
                        const size_t o = 2 * (ii + stride * q + outer_stride * oo);
                        re += src[o] * c - src[o + 1] * sn;
                        im += src[o] * sn + src[o + 1] * c;
                    }
                    const size_t o = 2 * (ii + stride * kk + outer_stride * oo);
                    dst[o] = re; dst[o + 1] = im;
                }
    };
    pass(a, b, Ny, nxh, (size_t)nxh * Ny, Nz, nxh);              // along y
    if (dims3) { a = b; pass(a, b, Nz, (size_t)nxh * Ny, 0, 1, (size_t)nxh * Ny); }  // along z
    double worst = 0.0;
    for (size_t q = 0; q < 2 * m; ++q) worst = std::fmax(worst, std::fabs(b[q] - spec[q]));
    return worst;
}

// forward then inverse transform of a pseudo-random field must reproduce it (times the plans' net scale), and the forward
// spectrum must be the DFT of the input
int plans_self_test(ocn_poisson *s, const PlanCheck &c)
{
    const ocn_grid *g = &s->grid;
    const int Nx = g->Nx, Ny = g->Ny, Nz = g->Nz;
    const size_t n = (size_t)Nx * Ny * Nz;
    const bool three_d = c.dims3;
    const double count = (double)Nx * Ny * (three_d ? Nz : 1);
    const double net = c.fused_z ? count : 1.0;  // inverse plans carry 1/count unless the column kernel applies it
    std::vector<double> in(n), outv;
    unsigned long long x = 0x9E3779B97F4A7C15ull;
    for (size_t q = 0; q < n; ++q) {  // splitmix-style generator, values in (-1, 1)
        x += 0x9E3779B97F4A7C15ull;
        unsigned long long z = x;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        in[q] = (double)(z >> 11) * (2.0 / 9007199254740992.0) - 1.0;
    }
    double err = 0.0, ferr = 0.0;
    if (c.c2c) {
        std::vector<double> cv(2 * n, 0.0);
        for (size_t q = 0; q < n; ++q) cv[2 * q] = in[q];
        OCN_CHECK_HIP(hipMemcpy(s->spec, cv.data(), 2 * n * sizeof(double), hipMemcpyHostToDevice));
        OCN_TRY(s->fwd.exec(s->spec, nullptr, nullptr));
        OCN_CHECK_HIP(hipDeviceSynchronize());
        OCN_CHECK_HIP(hipMemcpy(cv.data(), s->spec, 2 * n * sizeof(double), hipMemcpyDeviceToHost));
        if (n <= (size_t)1 << 16) ferr = full_spectrum_error(in, cv, Nx, Ny, Nz, Nx, three_d);
        OCN_TRY(s->bwd.exec(s->spec, nullptr, nullptr));
        OCN_CHECK_HIP(hipDeviceSynchronize());
        OCN_CHECK_HIP(hipMemcpy(cv.data(), s->spec, 2 * n * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t q = 0; q < n; ++q) {
            err = std::fmax(err, std::fabs(cv[2 * q] - net * in[q]));
            err = std::fmax(err, std::fabs(cv[2 * q + 1]));
        }
        {   // plane waves: closed-form answer for every entry, any grid size
            const std::vector<Wave> W = test_waves(Nx, Ny, Nz, three_d);
            fill_waves(in, W, Nx, Ny, Nz, three_d);
            std::fill(cv.begin(), cv.end(), 0.0);
            for (size_t q = 0; q < n; ++q) cv[2 * q] = in[q];
            OCN_CHECK_HIP(hipMemcpy(s->spec, cv.data(), 2 * n * sizeof(double), hipMemcpyHostToDevice));
            OCN_TRY(s->fwd.exec(s->spec, nullptr, nullptr));
            OCN_CHECK_HIP(hipDeviceSynchronize());
            OCN_CHECK_HIP(hipMemcpy(cv.data(), s->spec, 2 * n * sizeof(double), hipMemcpyDeviceToHost));
            ferr = std::fmax(ferr, wave_spectrum_error(cv, W, Nx, Ny, Nz, Nx, three_d));
        }
        OCN_CHECK_HIP(hipMemset(s->spec, 0, 2 * n * sizeof(double)));
    } else {
        ocn::GridDev gd = ocn::to_dev(*g);
        ocn::Lay Lp = ocn::make_lay(gd, OCN_LOC_CCC);
        const size_t np = (size_t)Lp.sx * Lp.sy * Lp.sz;
        double *tmp = nullptr;
        OCN_CHECK_HIP(hipMemcpy(s->rhs, in.data(), n * sizeof(double), hipMemcpyHostToDevice));
        OCN_TRY(s->fwd.exec(s->rhs, s->spec, nullptr));
        {
            OCN_CHECK_HIP(hipDeviceSynchronize());
            std::vector<double> sp((size_t)c.nxh * Ny * Nz * 2);
            OCN_CHECK_HIP(hipMemcpy(sp.data(), s->spec, sp.size() * sizeof(double), hipMemcpyDeviceToHost));
            if (n <= (size_t)1 << 16) ferr = full_spectrum_error(in, sp, Nx, Ny, Nz, c.nxh, three_d);
        }
        if (c.direct_out) {
            OCN_CHECK_HIP(hipMalloc((void **)&tmp, np * sizeof(double)));
            OCN_CHECK_HIP(hipMemset(tmp, 0, np * sizeof(double)));
        }
        const int st = c.direct_out ? s->bwd.exec(s->spec, tmp + Lp.o, nullptr) : s->bwd.exec(s->spec, s->rhs, nullptr);
        if (st != OCN_SUCCESS) {
            if (tmp) (void)hipFree(tmp);
            return st;
        }
        OCN_CHECK_HIP(hipDeviceSynchronize());
        if (c.direct_out) {
            outv.resize(np);
            OCN_CHECK_HIP(hipMemcpy(outv.data(), tmp, np * sizeof(double), hipMemcpyDeviceToHost));
            (void)hipFree(tmp);
            for (int k = 0; k < Nz; ++k)
                for (int j = 0; j < Ny; ++j)
                    for (int i = 0; i < Nx; ++i)
                        err = std::fmax(err, std::fabs(outv[Lp.o + i + Lp.s2 * j + Lp.s3 * k] - net * in[i + (size_t)Nx * (j + (size_t)Ny * k)]));
        } else {
            outv.resize(n);
            OCN_CHECK_HIP(hipMemcpy(outv.data(), s->rhs, n * sizeof(double), hipMemcpyDeviceToHost));
            for (size_t q = 0; q < n; ++q) err = std::fmax(err, std::fabs(outv[q] - net * in[q]));
        }
        {   // plane waves: closed-form answer for every entry, any grid size
            const std::vector<Wave> W = test_waves(Nx, Ny, Nz, three_d);
            fill_waves(in, W, Nx, Ny, Nz, three_d);
            OCN_CHECK_HIP(hipMemcpy(s->rhs, in.data(), n * sizeof(double), hipMemcpyHostToDevice));
            OCN_TRY(s->fwd.exec(s->rhs, s->spec, nullptr));
            OCN_CHECK_HIP(hipDeviceSynchronize());
            std::vector<double> sp((size_t)c.nxh * Ny * Nz * 2);
            OCN_CHECK_HIP(hipMemcpy(sp.data(), s->spec, sp.size() * sizeof(double), hipMemcpyDeviceToHost));
            ferr = std::fmax(ferr, wave_spectrum_error(sp, W, Nx, Ny, Nz, c.nxh, three_d));
        }
        OCN_CHECK_HIP(hipMemset(s->rhs, 0, n * sizeof(double)));
        OCN_CHECK_HIP(hipMemset(s->spec, 0, (size_t)c.nxh * Ny * Nz * 2 * sizeof(double)));
    }
    // (amplitudes of the test waves sum to < 40: the same absolute tolerance scale as the unit random field, times the wave amplitudes)
    if (!(err <= 1e-9 * net) || !(ferr <= 4e-8 * count * (three_d ? 1 : Nz))) {
        ocn::set_error("rocFFT %s plan pair for %dx%dx%d failed its self test (round trip: max error %.3e; forward spectrum vs direct DFT: %.3e)",
                       c.c2c ? "complex" : "real", Nx, Ny, Nz, err, ferr);
        return OCN_ERR_ROCFFT;
    }
    return OCN_SUCCESS;
}

// The real x plans of the packed general solver against known answers: the spectrum of one pseudo-random row against the DFT of its
// definition, and the round trip of a block of rows (see Plan::destroy for why rocFFT's real plans are not trusted unverified).
int packed_plans_self_test(ocn_poisson *s)
{
    const ocn_grid *g = &s->grid;
    const int N0 = g->Nx, nxh = N0 / 2 + 1;
    const size_t rows = (size_t)g->Ny * g->Nz, n = (size_t)N0 * rows;
    const size_t m = std::min(n, (size_t)1 << 18) / N0 * N0;  // whole rows
    std::vector<double> in(m), back(m), spec(2 * (size_t)nxh);
    unsigned long long x = 88172645463325252ULL;
    for (size_t q = 0; q < m; ++q) {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        in[q] = (double)(x >> 11) / 9007199254740992.0 - 0.5;
    }
    OCN_CHECK_HIP(hipMemset(s->spec, 0, n * sizeof(double)));
    OCN_CHECK_HIP(hipMemcpy(s->spec, in.data(), m * sizeof(double), hipMemcpyHostToDevice));
    OCN_TRY(s->xr2c.exec(s->spec, s->spec2, nullptr));
    OCN_CHECK_HIP(hipDeviceSynchronize());
    OCN_CHECK_HIP(hipMemcpy(spec.data(), s->spec2, spec.size() * sizeof(double), hipMemcpyDeviceToHost));
    const double two_pi = 6.283185307179586476925286766559;
    double err = 0.0, scale = 0.0;
    for (int k = 0; k < nxh; ++k) {
        double re = 0.0, im = 0.0;
        for (int q = 0; q < N0; ++q) {
            const double ang = two_pi * (double)(((long long)k * q) % N0) / N0;
            re += in[q] * std::cos(ang);
            im -= in[q] * std::sin(ang);
        }
        err = std::max(err, std::max(std::fabs(re - spec[2 * k]), std::fabs(im - spec[2 * k + 1])));
        scale = std::max(scale, std::max(std::fabs(re), std::fabs(im)));
    }
    OCN_TRY(s->xc2r.exec(s->spec2, s->spec, nullptr));
    OCN_CHECK_HIP(hipDeviceSynchronize());
    OCN_CHECK_HIP(hipMemcpy(back.data(), s->spec, m * sizeof(double), hipMemcpyDeviceToHost));
    double rt = 0.0;
    for (size_t q = 0; q < m; ++q) rt = std::max(rt, std::fabs(back[q] - in[q]));
    OCN_CHECK_HIP(hipMemset(s->spec, 0, n * 2 * sizeof(double)));
    if (!(err <= 1e-11 * std::max(scale, 1.0) * N0 && rt <= 1e-12)) {
        ocn::set_error("rocFFT real x plans of the packed general solver failed their self test (spectrum %.3e, round trip %.3e)", err, rt);
        return OCN_ERR_ROCFFT;
    }
    return OCN_SUCCESS;
}

}  // namespace poisson
}  // namespace ocn
