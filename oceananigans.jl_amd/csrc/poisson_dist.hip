// poisson_dist.hip -- DistributedFFTBasedPoissonSolver src/DistributedComputations/distributed_fft_based_poisson_solver.jl:10-188 (slab-x)
// and its Fourier-tridiagonal flavour: the local pieces of the solve (layouts of transposable_field.jl:50-78); the exchanges are comm.hip's.
#include "poisson_internal.h"

using namespace ocn::poisson;

struct ocn_dist_poisson {
    ocn_grid grid{};  // local grid
    int rank = 0, R = 1;
    int nx = 0, Nxg = 0;
    bool r2c = true;   // real-to-complex over (y, z): half the all-to-all volume of the reference's C2C
    int nyt = 0;       // y extent of the transposed (complex) data: Ny (c2c) or Ny/2+1 padded to a multiple of R (r2c)
    int ny = 0;        // nyt / R: y extent of the x-local field
    double *lx = nullptr, *ly = nullptr, *lz = nullptr;
    double *rhs = nullptr;  // real source term (r2c)
    double *yfield = nullptr, *xfield = nullptr, *send = nullptr, *recv = nullptr;
    Plan fyz, byz, fx, bx;
    // z Bounded: DistributedFourierTridiagonalPoissonSolver (distributed_fft_tridiagonal_solver.jl:149-351), ZStretched flavour.
    // FFT in y on the slab, transpose, FFT in x, Thomas sweep in z (z is local in the x-local layout as well, so the
    // reference's extra transpose pair to a z-local pencil is not needed), inverse x, transpose back, inverse y.
    bool tri = false;
    bool ycol = false;             // y transforms by the column-FFT kernel (stage-ordered ky) instead of rocFFT
    bool ybounded = false;         // Bounded y: REDFT10 / REDFT01 from the complex FFT (gather, FFT, twiddle: dct_shuffle_kernel), scratch = send
    double *ytw = nullptr;         // e^{-i pi k / 2 Ny} by stored position
    int *ypartner = nullptr;       // stored position of wavenumber Ny - k (stage order only)
    bool xbounded = false;         // the partitioned x is Bounded: cosine transforms along x of the x-local field (natural order, rocFFT lines)
    double *xtw = nullptr;         // e^{-i pi k / 2 Nxg}
    double *tw_y = nullptr;        // column-FFT twiddles
    double *xsol = nullptr;        // tridiagonal solution (x-local layout)
    double *diag = nullptr, *lower = nullptr, *tscr = nullptr;
    double *dzc = nullptr, *dzf = nullptr;
    // "fast" slab pipeline (colfft.hip; periodic z): real y transform -> z column FFT writing the all-to-all layout -> exchange ->
    // fused FFT_x / divide / IFFT_x column kernel -> exchange -> inverse z -> inverse real y into p.  No rocFFT plans, no pack /
    // unpack passes; yfield aliases recv (the half spectrum A1 lives there between the exchanges' uses of it).
    bool fast = false;
    double *tw_h = nullptr, *tw_z = nullptr, *tw_x = nullptr;  // W_{Ny/2}, W_Nz, W_Nxg  (tw_y = W_Ny)
    // the source term is evaluated inside the real y transform: ocn_dist_poisson_source_term only records its arguments
    const double *src_u = nullptr, *src_v = nullptr, *src_w = nullptr;
    double src_dt = 1.0;
    // transpose-free flavour of the fast pipeline (xtri.hip): y and z transforms in place in `recv`, the x direction as a cyclic
    // tridiagonal solve whose ranks exchange two numbers per mode (one all-gather of gsend into grecv) instead of the spectrum
    bool xtri = false;
    double *gsend = nullptr, *grecv = nullptr;
    size_t gchunk = 0;  // doubles per rank in grecv
};

static void free_all(ocn_dist_poisson *s)
{
    s->fyz.destroy(); s->byz.destroy(); s->fx.destroy(); s->bx.destroy();
    if (s->fast) s->yfield = nullptr;  // alias of recv
    double **ptrs[] = {&s->lx, &s->ly, &s->lz, &s->rhs, &s->yfield, &s->xfield, &s->send, &s->recv,
                       &s->tw_y, &s->xsol, &s->diag, &s->lower, &s->tscr, &s->dzc, &s->dzf, &s->tw_h, &s->tw_z, &s->tw_x, &s->gsend, &s->grecv,
                       &s->ytw, &s->xtw};
    for (auto p : ptrs)
        if (*p) {
            (void)hipFree(*p);
            *p = nullptr;
        }
    if (s->ypartner) {
        (void)hipFree(s->ypartner);
        s->ypartner = nullptr;
    }
}

static int dist_create_impl(ocn_dist_poisson_t *out, const ocn_grid *lg, int32_t rank, int32_t R, double global_Lx, bool force_c2c,
                            int global_tx = OCN_PERIODIC);

extern "C" int ocn_dist_poisson_create(ocn_dist_poisson_t *out, const ocn_grid *lg, int32_t rank, int32_t R, double global_Lx)
{
    return dist_create_impl(out, lg, rank, R, global_Lx, false);
}

// ... of a grid whose partitioned x is Bounded (global_tx = OCN_BOUNDED; the local grids are RightConnected / FullyConnected /
// LeftConnected slabs, so the global topology has to be said): (Bounded, Bounded, Bounded) only (distributed_fft_based_poisson_solver.jl:62-66)
extern "C" int ocn_dist_poisson_create_global(ocn_dist_poisson_t *out, const ocn_grid *lg, int32_t rank, int32_t R, double global_Lx,
                                              int32_t global_tx)
{
    OCN_REQUIRE(global_tx == OCN_PERIODIC || global_tx == OCN_BOUNDED, "ocn_dist_poisson_create_global: global_tx must be Periodic or Bounded");
    return dist_create_impl(out, lg, rank, R, global_Lx, false, global_tx);
}

// real (y, z) plan pair of the slab: forward + inverse must reproduce a pseudo-random field (see poisson_plans_self_test)
static int dist_real_plans_self_test(ocn_dist_poisson *s)
{
    const ocn_grid *g = &s->grid;
    const int nx = g->Nx, Ny = g->Ny, Nz = g->Nz;
    const size_t n = (size_t)nx * Ny * Nz;
    std::vector<double> in(n);
    unsigned long long x = 0x9E3779B97F4A7C15ull;
    for (size_t q = 0; q < n; ++q) {
        x += 0x9E3779B97F4A7C15ull;
        unsigned long long z = x;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        in[q] = (double)(z >> 11) * (2.0 / 9007199254740992.0) - 1.0;
    }
    ocn::GridDev gd = ocn::to_dev(*g);
    ocn::Lay Lp = ocn::make_lay(gd, OCN_LOC_CCC);
    const size_t np = (size_t)Lp.sx * Lp.sy * Lp.sz;
    double *tmp = nullptr;
    OCN_CHECK_HIP(hipMalloc((void **)&tmp, np * sizeof(double)));
    OCN_CHECK_HIP(hipMemset(tmp, 0, np * sizeof(double)));
    OCN_CHECK_HIP(hipMemcpy(s->rhs, in.data(), n * sizeof(double), hipMemcpyHostToDevice));
    int st = s->fyz.exec(s->rhs, s->yfield, nullptr);
    double ferr = 0.0;
    if (st == OCN_SUCCESS) {  // known-answer check of the forward (y, z) transform (samples; the serial handles check every entry): column xl, entry (ky, kz)
        if (hipDeviceSynchronize() != hipSuccess) st = OCN_ERR_ROCFFT;
        std::vector<double> sp((size_t)nx * s->nyt * Nz * 2);
        if (st == OCN_SUCCESS && hipMemcpy(sp.data(), s->yfield, sp.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) st = OCN_ERR_ROCFFT;
        const double two_pi = 6.283185307179586476925286766559;
        const int xs[3] = {0, nx / 2, nx - 1}, kys[3] = {1 % (Ny / 2 + 1), 0, Ny / 2}, kzs[3] = {Nz - 1, 1 % Nz, 0};
        for (int q = 0; q < 3 && st == OCN_SUCCESS; ++q) {
            double re = 0.0, im = 0.0;
            for (int k = 0; k < Nz; ++k)
                for (int j = 0; j < Ny; ++j) {
                    const double ph = -two_pi * ((double)kys[q] * j / Ny + (double)kzs[q] * k / Nz);
                    const double v = in[xs[q] + (size_t)nx * (j + (size_t)Ny * k)];
                    re += v * std::cos(ph);
                    im += v * std::sin(ph);
                }
            const size_t o = 2 * ((size_t)xs[q] + (size_t)nx * (kys[q] + (size_t)s->nyt * kzs[q]));
            ferr = std::fmax(ferr, std::fmax(std::fabs(sp[o] - re), std::fabs(sp[o + 1] - im)));
        }
    }
    if (st == OCN_SUCCESS) st = s->byz.exec(s->yfield, tmp + Lp.o, nullptr);
    if (st != OCN_SUCCESS) {
        (void)hipFree(tmp);
        return st;
    }
    OCN_CHECK_HIP(hipDeviceSynchronize());
    std::vector<double> outv(np);
    OCN_CHECK_HIP(hipMemcpy(outv.data(), tmp, np * sizeof(double), hipMemcpyDeviceToHost));
    (void)hipFree(tmp);
    double err = 0.0;
    for (int k = 0; k < Nz; ++k)
        for (int j = 0; j < Ny; ++j)
            for (int i = 0; i < nx; ++i)
                err = std::fmax(err, std::fabs(outv[Lp.o + i + Lp.s2 * j + Lp.s3 * k] - in[i + (size_t)nx * (j + (size_t)Ny * k)]));
    OCN_CHECK_HIP(hipMemset(s->rhs, 0, n * sizeof(double)));
    OCN_CHECK_HIP(hipMemset(s->yfield, 0, (size_t)nx * s->nyt * Nz * 2 * sizeof(double)));
    if (!(err <= 1e-9) || !(ferr <= 1e-9 * Ny * Nz)) {
        ocn::set_error("rocFFT real (y, z) plan pair for the %dx%dx%d slab failed its self test (round trip: max error %.3e; forward spectrum vs direct DFT: %.3e)",
                       nx, Ny, Nz, err, ferr);
        return OCN_ERR_ROCFFT;
    }
    return OCN_SUCCESS;
}

static int dist_create_impl(ocn_dist_poisson_t *out, const ocn_grid *lg, int32_t rank, int32_t R, double global_Lx, bool force_c2c, int global_tx)
{
    OCN_REQUIRE(out && lg, "ocn_dist_poisson_create: null argument");
    const bool xbounded = global_tx == OCN_BOUNDED;
    {   // the slab's x topology must be the one its rank has in that global grid
        const int want = !xbounded ? (lg->tx == OCN_PERIODIC ? OCN_PERIODIC : OCN_FULLY_CONNECTED)
                                   : (R == 1 ? OCN_BOUNDED : rank == 0 ? OCN_RIGHT_CONNECTED : rank == R - 1 ? OCN_LEFT_CONNECTED : OCN_FULLY_CONNECTED);
        OCN_REQUIRE(lg->tx == want, "ocn_dist_poisson_create: rank %d of %d of a %s x must hold a slab of x topology %d, got %d", rank, R,
                    xbounded ? "Bounded" : "Periodic", want, lg->tx);
        OCN_REQUIRE(!xbounded || (lg->ty == OCN_BOUNDED && lg->tz == OCN_BOUNDED),
                    "ocn_dist_poisson_create: a Bounded x needs Bounded y and z (distributed_fft_based_poisson_solver.jl:62-66)");
    }
    OCN_TRY(ocn::validate_grid_any(lg));
    OCN_REQUIRE(R >= 1 && rank >= 0 && rank < R, "ocn_dist_poisson_create: bad rank %d of %d", rank, R);
    OCN_REQUIRE(global_Lx > 0, "ocn_dist_poisson_create: global_Lx must be positive");
    // (distributed_fft_based_poisson_solver.jl:62-66: a Periodic z needs a Periodic y)
    OCN_REQUIRE((lg->ty == OCN_PERIODIC && ((lg->tz == OCN_PERIODIC && lg->dzc == nullptr) || lg->tz == OCN_BOUNDED)) ||
                    (lg->ty == OCN_BOUNDED && lg->tz == OCN_BOUNDED),
                "ocn_dist_poisson_create: supports (x-partitioned, Periodic, Periodic) regular grids, (x-partitioned, Periodic, Bounded) and "
                "(x-partitioned, Bounded, Bounded)");
    // validate_poisson_solver_distributed_grid (distributed_fft_based_poisson_solver.jl:211-229)
    OCN_REQUIRE(lg->Ny % R == 0, "ocn_dist_poisson_create: Ny = %d must be divisible by the number of ranks %d", lg->Ny, R);
    ensure_rocfft();
    struct Release {
        void operator()(ocn_dist_poisson *h) const { free_all(h); delete h; }
    };
    std::unique_ptr<ocn_dist_poisson, Release> hold(new ocn_dist_poisson());  // (TRY / TRY_HIP return through it)
    ocn_dist_poisson *s = hold.get();
    s->grid = *lg;
    s->rank = rank; s->R = R;
    s->nx = lg->Nx; s->Nxg = lg->Nx * R;
    const int nx = s->nx, Ny = lg->Ny, Nz = lg->Nz, Nxg = s->Nxg;
    s->r2c = !force_c2c && !env_set("OCN_POISSON_C2C");
    const bool efast = env_on("OCN_DIST_POISSON_FAST");
    if (lg->tz == OCN_BOUNDED && lg->ty == OCN_PERIODIC && !xbounded && efast && R >= 1 && Nz > 1 && ocn::realfft_y_supported(Ny) &&
        ocn::colfft_supported(Nxg)) {
        // Slab pipeline, tridiagonal flavour: real y transform (source term x Δzᶜ evaluated on load) writing the all-to-all layout
        // [d][ky_l + c (z + Nz xl)] (ky = d c + ky_l, c = ceil((Ny/2+1) / R), padded entries stay 0) -> exchange -> x is a strided
        // column: FFT_x -> Thomas sweep along z (stride c) with this rank's ky range -> IFFT_x -> exchange -> inverse real y into p.
        s->tri = true;
        s->fast = true;
        s->r2c = true;
        const int NyH = Ny / 2 + 1, c = (NyH + R - 1) / R, Hz = lg->Hz;
        s->ny = c;
        s->nyt = c * R;
        const size_t n = (size_t)s->nyt * Nz * nx;
        if (lg->dzc) {
            const size_t nf = (size_t)Nz + 2 * Hz;
            TRY_HIP(hipMalloc((void **)&s->dzc, nf * sizeof(double)));
            TRY_HIP(hipMalloc((void **)&s->dzf, nf * sizeof(double)));
            TRY_HIP(hipMemcpy(s->dzc, lg->dzc, nf * sizeof(double), hipMemcpyDeviceToDevice));
            TRY_HIP(hipMemcpy(s->dzf, lg->dzf, nf * sizeof(double), hipMemcpyDeviceToDevice));
            s->grid.dzc = s->dzc;
            s->grid.dzf = s->dzf;
        }
        for (double **p : {&s->send, &s->recv}) {
            TRY_HIP(hipMalloc((void **)p, n * 2 * sizeof(double)));
            TRY_HIP(hipMemset(*p, 0, n * 2 * sizeof(double)));
        }
        s->yfield = s->recv;
        TRY_HIP(hipMalloc((void **)&s->diag, n * sizeof(double)));
        TRY_HIP(hipMalloc((void **)&s->tscr, n * sizeof(double)));
        TRY(upload(ocn::colfft_twiddles(Ny / 2), &s->tw_h));
        TRY(upload(ocn::colfft_twiddles(Ny), &s->tw_y));
        TRY(upload(ocn::colfft_twiddles(Nxg), &s->tw_x));
        std::vector<double> lyn = eigenvalues(Ny, lg->Ly, OCN_PERIODIC), lxn = eigenvalues(Nxg, global_Lx, OCN_PERIODIC), lxs(Nxg);
        lyn.resize(NyH);
        lyn.resize(s->nyt, 1.0);  // padded ky: their data is 0, any nonzero eigenvalue keeps the sweep finite
        for (int q = 0; q < Nxg; ++q) lxs[q] = lxn[ocn::colfft_wavenumber(Nxg, q)];
        TRY(upload(lyn, &s->ly));
        TRY(upload(lxs, &s->lx));
        std::vector<double> hf(Nz + 2 * Hz, lg->dz);
        if (lg->dzf) TRY_HIP(hipMemcpy(hf.data(), lg->dzf, hf.size() * sizeof(double), hipMemcpyDeviceToHost));
        std::vector<double> low(Nz - 1, 0.0);
        for (int q = 2; q <= Nz; ++q) low[q - 2] = 1 / hf[q + Hz - 1];
        TRY(upload(low, &s->lower));
        // main diagonal in the exchanged layout: column (ky_l, kx position) at ky_l + c Nz kx, planes c apart
        TRY(ocn::launch_main_diagonal_strided(&s->grid, c, Nxg, (long long)c * Nz, c, s->ly + (size_t)rank * c, s->lx, s->diag, nullptr));
        TRY_HIP(hipDeviceSynchronize());
        *out = hold.release();
        return OCN_SUCCESS;
    }
    if (lg->tz == OCN_BOUNDED) {
        s->tri = true;
        s->r2c = false;
        s->nyt = Ny;
        s->ny = Ny / R;
        const int ny = s->ny, Hz = lg->Hz;
        const size_t n = (size_t)nx * Ny * Nz;
        if (lg->dzc) {  // private copies of the z spacings, like the single-GPU solver
            const size_t nf = (size_t)Nz + 2 * Hz;
            TRY_HIP(hipMalloc((void **)&s->dzc, nf * sizeof(double)));
            TRY_HIP(hipMalloc((void **)&s->dzf, nf * sizeof(double)));
            TRY_HIP(hipMemcpy(s->dzc, lg->dzc, nf * sizeof(double), hipMemcpyDeviceToDevice));
            TRY_HIP(hipMemcpy(s->dzf, lg->dzf, nf * sizeof(double), hipMemcpyDeviceToDevice));
            s->grid.dzc = s->dzc;
            s->grid.dzf = s->dzf;
        }
        for (double **p : {&s->yfield, &s->xfield, &s->send, &s->recv, &s->xsol}) {
            TRY_HIP(hipMalloc((void **)p, n * 2 * sizeof(double)));
            TRY_HIP(hipMemset(*p, 0, n * 2 * sizeof(double)));
        }
        TRY_HIP(hipMalloc((void **)&s->diag, n * sizeof(double)));
        TRY_HIP(hipMalloc((void **)&s->tscr, n * sizeof(double)));
        TRY(upload(eigenvalues(Nxg, global_Lx, xbounded ? OCN_BOUNDED : OCN_PERIODIC), &s->lx));
        s->xbounded = xbounded;
        if (xbounded) {
            TRY(upload(cosine_twiddles(Nxg, stored_wavenumbers(Nxg, false)), &s->xtw));
        }
        // y transforms: the column-FFT kernel leaves ky in stage order, so the eigenvalue of a stored position is permuted
        s->ycol = ocn::colfft_supported(Ny);
        s->ybounded = lg->ty == OCN_BOUNDED;
        std::vector<double> lyn = eigenvalues(Ny, lg->Ly, lg->ty), lys(Ny);
        for (int q = 0; q < Ny; ++q) lys[q] = s->ycol ? lyn[ocn::colfft_wavenumber(Ny, q)] : lyn[q];
        TRY(upload(lys, &s->ly));
        if (s->ybounded) {  // the twiddles of the cosine transforms by stored position, and where wavenumber Ny - k is stored
            const std::vector<int> kofp = stored_wavenumbers(Ny, s->ycol);
            TRY(upload(cosine_twiddles(Ny, kofp), &s->ytw));
            TRY(upload(partner_positions(kofp), &s->ypartner));
        }
        if (s->ycol) {
            TRY(upload(ocn::colfft_twiddles(Ny), &s->tw_y));
        } else {  // rocFFT, one z-plane per execution: (nx columns at distance 1) x (Ny points at stride nx)
            const size_t len[1] = {(size_t)Ny};
            const size_t str[1] = {(size_t)nx};
            TRY(make_plan(s->fyz, rocfft_placement_inplace, rocfft_transform_type_complex_forward, 1, len, nx,
                          rocfft_array_type_complex_interleaved, rocfft_array_type_complex_interleaved, str, 1, str, 1, 1.0));
            TRY(make_plan(s->byz, rocfft_placement_inplace, rocfft_transform_type_complex_inverse, 1, len, nx,
                          rocfft_array_type_complex_interleaved, rocfft_array_type_complex_interleaved, str, 1, str, 1, 1.0));
        }
        {   // x transforms of the x-local field (Nxg, ny, Nz); the inverse reads the tridiagonal solution and carries 1/(Nxg Ny)
            const size_t len[1] = {(size_t)Nxg};
            const size_t str[1] = {1};
            TRY(make_plan(s->fx, rocfft_placement_inplace, rocfft_transform_type_complex_forward, 1, len, (size_t)ny * Nz,
                          rocfft_array_type_complex_interleaved, rocfft_array_type_complex_interleaved, str, Nxg, str, Nxg, 1.0));
            TRY(make_plan(s->bx, rocfft_placement_notinplace, rocfft_transform_type_complex_inverse, 1, len, (size_t)ny * Nz,
                          rocfft_array_type_complex_interleaved, rocfft_array_type_complex_interleaved, str, Nxg, str, Nxg,
                          1.0 / ((double)Nxg * Ny)));
        }
        // lower = upper = 1/Δzᶠ[q], q = 2..Nz; main diagonal with this rank's ky range (fourier_tridiagonal_poisson_solver.jl:41-51, 97-99)
        std::vector<double> hf(Nz + 2 * Hz, lg->dz);
        if (lg->dzf) TRY_HIP(hipMemcpy(hf.data(), lg->dzf, hf.size() * sizeof(double), hipMemcpyDeviceToHost));
        std::vector<double> low(Nz > 1 ? Nz - 1 : 1, 0.0);
        for (int q = 2; q <= Nz; ++q) low[q - 2] = 1 / hf[q + Hz - 1];
        TRY(upload(low, &s->lower));
        ocn_grid xg = s->grid;  // the x-local layout as a "grid": only Ny, Nz and the z spacings are read
        xg.Nx = Nxg;
        xg.Ny = ny;
        TRY(ocn::launch_main_diagonal(&xg, Nxg, s->lx, s->ly + (size_t)rank * ny, s->diag, nullptr));
        TRY_HIP(hipDeviceSynchronize());
        *out = hold.release();
        return OCN_SUCCESS;
    }
    {
        const bool local_ok = !force_c2c && s->r2c && efast && R >= 1 && ocn::realfft_y_supported(Ny) && ocn::colfft_supported(Nz);
        // the transpose-free x solve: default for R > 1 (one rank has nothing to exchange and the fused FFT_x kernel moves fewer
        // bytes); OCN_DIST_POISSON_XTRI=1 forces it, =0 keeps the all-to-all pipeline
        const char *ex = std::getenv("OCN_DIST_POISSON_XTRI");
        const bool want = ex ? ex[0] == '1' : R > 1;
        s->xtri = local_ok && want && ocn::xtri_supported(R, Nxg);
        s->fast = s->xtri || (local_ok && ocn::colfft_supported(Nxg) && Nz % R == 0);
    }
    if (s->fast) {
        const int NyH = Ny / 2 + 1;
        s->nyt = NyH;
        s->ny = 0;  // the transposed layout is partitioned in (stored) kz, not in ky
        const size_t n = (size_t)NyH * nx * Nz;
        TRY_HIP(hipMalloc((void **)&s->rhs, (size_t)nx * Ny * Nz * sizeof(double)));
        TRY_HIP(hipMemset(s->rhs, 0, (size_t)nx * Ny * Nz * sizeof(double)));
        for (double **p : {&s->send, &s->recv}) {
            if (s->xtri && p == &s->send) continue;  // no exchange layout: the spectrum stays in `recv`
            TRY_HIP(hipMalloc((void **)p, n * 2 * sizeof(double)));
            TRY_HIP(hipMemset(*p, 0, n * 2 * sizeof(double)));
        }
        if (s->xtri) {
            s->gchunk = 2 * (2 * (size_t)NyH * Nz + nx);
            TRY_HIP(hipMalloc((void **)&s->gsend, s->gchunk * sizeof(double)));
            TRY_HIP(hipMalloc((void **)&s->grecv, s->gchunk * R * sizeof(double)));
            TRY_HIP(hipMemset(s->gsend, 0, s->gchunk * sizeof(double)));
            TRY_HIP(hipMemset(s->grecv, 0, s->gchunk * R * sizeof(double)));
        }
        s->yfield = s->recv;
        TRY(upload(ocn::colfft_twiddles(Ny / 2), &s->tw_h));
        TRY(upload(ocn::colfft_twiddles(Ny), &s->tw_y));
        TRY(upload(ocn::colfft_twiddles(Nz), &s->tw_z));
        if (!s->xtri) TRY(upload(ocn::colfft_twiddles(Nxg), &s->tw_x));
        // eigenvalues: ky natural (0..Ny/2); kz and kx by STORED position of the column kernels' stage order
        std::vector<double> lyn = eigenvalues(Ny, lg->Ly, OCN_PERIODIC), lzn = eigenvalues(Nz, lg->Lz, OCN_PERIODIC),
                            lxn = eigenvalues(Nxg, global_Lx, OCN_PERIODIC);
        lyn.resize(NyH);
        std::vector<double> lzs(Nz), lxs(Nxg);
        for (int q = 0; q < Nz; ++q) lzs[q] = lzn[ocn::colfft_wavenumber(Nz, q)];
        for (int q = 0; q < Nxg && !s->xtri; ++q) lxs[q] = lxn[ocn::colfft_wavenumber(Nxg, q)];
        TRY(upload(lyn, &s->ly));
        TRY(upload(lzs, &s->lz));
        TRY(upload(lxs, &s->lx));
        TRY_HIP(hipDeviceSynchronize());
        *out = hold.release();
        return OCN_SUCCESS;
    }
    ocn::GridDev gd = ocn::to_dev(*lg);
    ocn::Lay Lp = ocn::make_lay(gd, OCN_LOC_CCC);
    for (int attempt = 0; attempt < 2; ++attempt) {
        const int nyh = Ny / 2 + 1;
        s->nyt = s->r2c ? ((nyh + R - 1) / R) * R : Ny;
        s->ny = s->nyt / R;
        const size_t len[2] = {(size_t)Ny, (size_t)Nz};
        const size_t cstr[2] = {(size_t)nx, (size_t)nx * s->nyt};
        int pst;
        if (s->r2c) {  // real (nx,Ny,Nz) -> Hermitian (nx,nyt,Nz), batched over the nx local columns (distance 1)
            const size_t rstr[2] = {(size_t)nx, (size_t)nx * Ny};
            const size_t pstr[2] = {(size_t)Lp.s2, (size_t)Lp.s3};
            pst = make_plan(s->fyz, rocfft_placement_notinplace, rocfft_transform_type_real_forward, 2, len, nx, rocfft_array_type_real,
                            rocfft_array_type_hermitian_interleaved, rstr, 1, cstr, 1, 1.0);
            if (pst == OCN_SUCCESS)  // inverse writes straight into the local pressure interior
                pst = make_plan(s->byz, rocfft_placement_notinplace, rocfft_transform_type_real_inverse, 2, len, nx,
                                rocfft_array_type_hermitian_interleaved, rocfft_array_type_real, cstr, 1, pstr, 1, 1.0 / ((double)Ny * Nz));
            if (pst != OCN_SUCCESS) {  // rocFFT has no kernel for this strided real layout: complex path
                s->fyz.destroy(); s->byz.destroy();
                s->r2c = false;
                continue;
            }
        } else {  // FFT over (y, z) of the y-local complex field, batched over the nx local columns (no permutedims)
            TRY(make_plan(s->fyz, rocfft_placement_inplace, rocfft_transform_type_complex_forward, 2, len, nx,
                          rocfft_array_type_complex_interleaved, rocfft_array_type_complex_interleaved, cstr, 1, cstr, 1, 1.0));
            TRY(make_plan(s->byz, rocfft_placement_inplace, rocfft_transform_type_complex_inverse, 2, len, nx,
                          rocfft_array_type_complex_interleaved, rocfft_array_type_complex_interleaved, cstr, 1, cstr, 1,
                          1.0 / ((double)Ny * Nz)));
        }
        break;
    }
    const int ny = s->ny;
    const size_t n = (size_t)nx * s->nyt * Nz;  // complex elements of either layout
    // global eigenvalues (distributed_fft_based_poisson_solver.jl:104-106); padded ky (r2c) get 1 (their data is 0)
    TRY(upload(eigenvalues(Nxg, global_Lx, OCN_PERIODIC), &s->lx));
    {
        std::vector<double> ly = eigenvalues(Ny, lg->Ly, OCN_PERIODIC);
        ly.resize(s->nyt > Ny ? s->nyt : Ny, 1.0);
        for (int q = Ny / 2 + 1; s->r2c && q < s->nyt; ++q) ly[q] = 1.0;
        TRY(upload(ly, &s->ly));
    }
    TRY(upload(eigenvalues(Nz, lg->Lz, OCN_PERIODIC), &s->lz));
    for (double **p : {&s->yfield, &s->xfield, &s->send, &s->recv}) {
        TRY_HIP(hipMalloc((void **)p, n * 2 * sizeof(double)));
        TRY_HIP(hipMemset(*p, 0, n * 2 * sizeof(double)));
    }
    if (s->r2c) {
        TRY_HIP(hipMalloc((void **)&s->rhs, (size_t)nx * Ny * Nz * sizeof(double)));
        TRY_HIP(hipMemset(s->rhs, 0, (size_t)nx * Ny * Nz * sizeof(double)));
    }
    {   // FFT over x of the x-local field (Nxg, ny, Nz)
        const size_t len[1] = {(size_t)Nxg};
        const size_t str[1] = {1};
        TRY(make_plan(s->fx, rocfft_placement_inplace, rocfft_transform_type_complex_forward, 1, len, (size_t)ny * Nz,
                      rocfft_array_type_complex_interleaved, rocfft_array_type_complex_interleaved, str, Nxg, str, Nxg, 1.0));
        TRY(make_plan(s->bx, rocfft_placement_inplace, rocfft_transform_type_complex_inverse, 1, len, (size_t)ny * Nz,
                      rocfft_array_type_complex_interleaved, rocfft_array_type_complex_interleaved, str, Nxg, str, Nxg,
                      1.0 / (double)Nxg));
    }
    if (s->r2c && dist_real_plans_self_test(s) != OCN_SUCCESS) {  // see poisson_create_impl: fall back to complex plans
        hold.reset();
        return dist_create_impl(out, lg, rank, R, global_Lx, true, global_tx);
    }
    *out = hold.release();
    return OCN_SUCCESS;
}

extern "C" int ocn_dist_poisson_destroy(ocn_dist_poisson_t s)
{
    if (!s) return OCN_SUCCESS;
    free_all(s);
    delete s;
    return OCN_SUCCESS;
}

extern "C" int ocn_dist_poisson_buffers(ocn_dist_poisson_t s, double **yfield, double **xfield, double **send, double **recv)
{
    OCN_REQUIRE(s, "ocn_dist_poisson_buffers: null solver");
    if (yfield) *yfield = s->yfield;
    if (xfield) *xfield = s->xfield;
    if (send) *send = s->send;
    if (recv) *recv = s->recv;
    return OCN_SUCCESS;
}

extern "C" int ocn_dist_poisson_layout(ocn_dist_poisson_t s, int32_t *ny_transposed, int64_t *complex_elements, int32_t *r2c)
{
    OCN_REQUIRE(s, "ocn_dist_poisson_layout: null solver");
    if (ny_transposed) *ny_transposed = s->nyt;
    if (complex_elements) *complex_elements = (int64_t)s->nx * s->nyt * s->grid.Nz;
    if (r2c) *r2c = s->r2c;
    return OCN_SUCCESS;
}

extern "C" int ocn_dist_poisson_gather_buffers(ocn_dist_poisson_t s, double **send, double **recv, int64_t *doubles_per_rank)
{
    OCN_REQUIRE(s, "ocn_dist_poisson_gather_buffers: null solver");
    if (send) *send = s->gsend;
    if (recv) *recv = s->grecv;
    if (doubles_per_rank) *doubles_per_rank = (int64_t)s->gchunk;
    return OCN_SUCCESS;
}

extern "C" int ocn_dist_poisson_pipeline(ocn_dist_poisson_t s, int32_t *fast)
{
    OCN_REQUIRE(s && fast, "ocn_dist_poisson_pipeline: null argument");
    *fast = s->fast ? (s->tri ? 2 : (s->xtri ? 3 : 1)) : 0;
    return OCN_SUCCESS;
}

extern "C" int ocn_dist_poisson_source_term(ocn_dist_poisson_t s, const double *u, const double *v, const double *w, double dt,
                                            void *stream)
{
    OCN_REQUIRE(s && u && v && w, "ocn_dist_poisson_source_term: null argument");
    const ocn_grid *g = &s->grid;
    if (s->fast) {
        // evaluating the source term inside the real y transform saves a pass (with the XCD-contiguous block order of round 4 also on
        // thin slabs: 4.14 against 4.18 ms per rank-step at nx = 64; OCN_DIST_FUSED_SOURCE=0 keeps the separate pass)
        static const bool separate = !env_on("OCN_DIST_FUSED_SOURCE");
        const bool fused = s->tri || !separate;
        s->src_u = fused ? u : nullptr; s->src_v = v; s->src_w = w; s->src_dt = dt;
        if (fused) return OCN_SUCCESS;  // evaluated by forward_yz from the same (unchanged) velocity arrays
    }
    // _fourier_tridiagonal_source_term! (solve_for_pressure.jl:33-38): rhs = Δzᶜ div(U) / Δt, complex
    if (s->tri) return ocn::launch_source_term(g, u, v, w, dt, ocn::SourceOut::ComplexDz, s->yfield, g->Nx, (long long)g->Nx * g->Ny, ocn::as_stream(stream));
    if (s->r2c) return ocn::launch_source_term(g, u, v, w, dt, ocn::SourceOut::Real, s->rhs, g->Nx, (long long)g->Nx * g->Ny, ocn::as_stream(stream));
    return ocn::launch_source_term(g, u, v, w, dt, ocn::SourceOut::Complex, s->yfield, g->Nx, (long long)g->Nx * g->Ny, ocn::as_stream(stream));
}

// y transform of the slab (nx, Ny, Nz) for the tridiagonal flavour: column-FFT kernel (stage-ordered ky) or rocFFT per plane
static int dist_tri_y_fft(ocn_dist_poisson *s, int inverse, double *a, hipStream_t stream)
{
    const int nx = s->nx, Ny = s->grid.Ny, Nz = s->grid.Nz;
    if (s->ycol)
        return ocn::launch_colfft(Ny, inverse ? ocn::ColFFT::Inverse : ocn::ColFFT::Forward, a, nx, (long long)nx * Ny, nx, Nz, s->tw_y, nullptr, nullptr, nullptr, 1.0, 1, stream);
    Plan &P = inverse ? s->byz : s->fyz;
    for (int k = 0; k < Nz; ++k) {
        OCN_TRY(P.exec(a + 2 * (size_t)nx * Ny * k, nullptr, stream));
    }
    return OCN_SUCCESS;
}
// Bounded y: the cosine transforms of the single-process solver (dct_shuffle_kernel: Makhoul's gather / twiddle around the complex FFT),
// out of place through `send`, which is idle while the spectrum is y-local.  The inverse's 1 / Ny rides on the x inverse like the FFT's.
static int dist_tri_y_transform(ocn_dist_poisson *s, int inverse, hipStream_t stream)
{
    if (!s->ybounded) return dist_tri_y_fft(s, inverse, s->yfield, stream);
    const int nx = s->nx, Ny = s->grid.Ny, Nz = s->grid.Nz;
    const int n[3] = {nx, Ny, Nz};
    using ocn::DctShuffle;
    OCN_TRY(inverse ? launch_dct_shuffle(n, 1, DctShuffle::PreTwiddle, s->yfield, s->send, s->ytw, s->ypartner, stream)
                    : launch_dct_shuffle(n, 1, DctShuffle::Gather, s->yfield, s->send, s->ytw, nullptr, stream));
    OCN_TRY(dist_tri_y_fft(s, inverse, s->send, stream));
    return inverse ? launch_dct_shuffle(n, 1, DctShuffle::Scatter, s->send, s->yfield, s->ytw, nullptr, stream)
                   : launch_dct_shuffle(n, 1, DctShuffle::PostTwiddle, s->send, s->yfield, s->ytw, s->ypartner, stream);
}

extern "C" int ocn_dist_poisson_forward_yz(ocn_dist_poisson_t s, void *stream)
{
    OCN_REQUIRE(s, "ocn_dist_poisson_forward_yz: null solver");
    if (s->tri && s->fast) {  // (Δzᶜ div / Δt)(u, v, w) -> half spectrum in the exchange layout
        const ocn_grid *g = &s->grid;
        OCN_REQUIRE(s->src_u, "ocn_dist_poisson_forward_yz: call ocn_dist_poisson_source_term first");
        return ocn::launch_realfft_y(g->Ny, 0, nullptr, s->send, nullptr, 0, 0, s->nx, g->Nz, s->tw_h, s->tw_y, ocn::as_stream(stream), g,
                                     s->src_u, s->src_v, s->src_w, s->src_dt, s->ny, (long long)s->ny * g->Nz * s->nx, 1, 1.0);
    }
    if (s->tri) return dist_tri_y_transform(s, 0, ocn::as_stream(stream));
    if (s->fast) {  // rhs -> A1 (in recv) -> send, ready for the exchange
        const ocn_grid *g = &s->grid;
        OCN_TRY(s->src_u ? ocn::launch_realfft_y(g->Ny, 0, nullptr, s->recv, nullptr, 0, 0, s->nx, g->Nz, s->tw_h, s->tw_y,
                                                  ocn::as_stream(stream), g, s->src_u, s->src_v, s->src_w, s->src_dt)
                         : ocn::launch_realfft_y(g->Ny, 0, s->rhs, s->recv, nullptr, 0, 0, s->nx, g->Nz, s->tw_h, s->tw_y, ocn::as_stream(stream)));
        if (s->xtri) {  // z in place (stage order), then the local x solves; gsend is ready for the all-gather
            const long long cols = (long long)s->nyt * s->nx;
            OCN_TRY(ocn::launch_colfft(g->Nz, ocn::ColFFT::Forward, s->recv, cols, 0, (int)cols, 1, s->tw_z, nullptr, nullptr, nullptr, 1.0, 1, ocn::as_stream(stream)));
            const double scale = 1.0 / ((double)(g->Ny / 2) * g->Nz);
            return ocn::launch_xtri_sweep(s->recv, s->ly, s->lz, s->nyt, s->nx, g->Nz, g->dx, scale, s->gsend, ocn::as_stream(stream));
        }
        return ocn::launch_colfft_slab_z(g->Nz, 0, s->recv, s->send, s->nx, s->nyt, s->R, s->tw_z, ocn::as_stream(stream));
    }
    if (s->r2c) return s->fyz.exec(s->rhs, s->yfield, ocn::as_stream(stream));
    return s->fyz.exec(s->yfield, nullptr, ocn::as_stream(stream));
}

extern "C" int ocn_dist_poisson_solve_x(ocn_dist_poisson_t s, void *stream_)
{
    OCN_REQUIRE(s, "ocn_dist_poisson_solve_x: null solver");
    hipStream_t stream = ocn::as_stream(stream_);
    if (s->fast && s->tri) {  // recv = [xg S + (ky_l + c z)], S = c Nz
        const int Nz = s->grid.Nz, c = s->ny;
        const long long S = (long long)c * Nz;
        OCN_TRY(ocn::launch_colfft(s->Nxg, ocn::ColFFT::Forward, s->recv, S, 0, (int)S, 1, s->tw_x, nullptr, nullptr, nullptr, 1.0, 1, stream));
        OCN_TRY(ocn::launch_tridiag_z_strided(c, s->Nxg, S, c, Nz, s->lower, s->diag, s->lower, s->recv, s->tscr, s->send, stream));
        if (s->rank == 0) {  // zero-mean gauge on the (kx, ky) = (0, 0) column: stored position 0 of both
            OCN_TRY(ocn::launch_remove_mean_mode(c, Nz, s->send, stream));
        }
        return ocn::launch_colfft(s->Nxg, ocn::ColFFT::Inverse, s->send, S, 0, (int)S, 1, s->tw_x, nullptr, nullptr, nullptr, 1.0, 1, stream);
    }
    if (s->xtri)  // grecv holds every rank's interface values: interface systems, spike correction, the mean mode's line
        return ocn::launch_xtri_finish(s->recv, s->ly, s->lz, s->nyt, s->nx, s->grid.Nz, s->grid.dx, s->grecv, s->rank, s->R, stream);
    if (s->fast) {  // recv = [xg S + (ky + NyH pz_l)]: FFT_x -> -b / ((λy + λz) + λx), rank 0 zeroes the mean mode -> IFFT_x, in place
        const int Nz = s->grid.Nz, cz = Nz / s->R, NyH = s->nyt;
        const long long S = (long long)NyH * cz;
        const double scale = 1.0 / ((double)(s->grid.Ny / 2) * Nz * s->Nxg);
        return ocn::launch_colfft(s->Nxg, ocn::ColFFT::Solve, s->recv, S, 0, (int)S, 1, s->tw_x, s->ly, s->lz + (size_t)s->rank * cz, s->lx, scale, NyH,
                                  stream, s->rank == 0);
    }
    // Bounded x: REDFT10 / REDFT01 along the lines of the x-local field (Nxg, ny, Nz) -- gather / twiddle passes of the single-process
    // solver around the same complex line FFTs, out of place between xfield and xsol; the inverse's 1 / Nxg rides on the plan's scale
    using ocn::DctShuffle;
    auto xshuffle = [&](DctShuffle mode, const double *in, double *outp) {
        const int n[3] = {s->Nxg, s->ny, s->grid.Nz};
        return launch_dct_shuffle(n, 0, mode, in, outp, s->xtw, nullptr, stream);
    };
    if (s->xbounded) {
        OCN_REQUIRE(s->tri, "ocn_dist_poisson_solve_x: a Bounded x runs the tridiagonal flavour");
        OCN_TRY(xshuffle(DctShuffle::Gather, s->xfield, s->xsol));
        OCN_TRY(s->fx.exec(s->xsol, nullptr, stream));
        OCN_TRY(xshuffle(DctShuffle::PostTwiddle, s->xsol, s->xfield));
    } else {
        OCN_TRY(s->fx.exec(s->xfield, nullptr, stream));
    }
    if (s->tri) {
        const int Nz = s->grid.Nz;
        OCN_TRY(ocn::launch_tridiag_z(s->Nxg, s->ny, Nz, s->lower, s->diag, s->lower, s->xfield, s->tscr, s->xsol, stream));
        // zero-mean gauge on the (kx, ky) = (0, 0) column, which lives on rank 0 (stored position 0 is wavenumber 0):
        // the single-process solver's ϕ .- mean(ϕ) (fourier_tridiagonal_poisson_solver.jl:142)
        if (s->rank == 0) {
            OCN_TRY(ocn::launch_remove_mean_mode((long long)s->Nxg * s->ny, Nz, s->xsol, stream));
        }
        if (s->xbounded) {
            OCN_TRY(xshuffle(DctShuffle::PreTwiddle, s->xsol, s->xfield));
            OCN_TRY(s->bx.exec(s->xfield, s->xsol, stream));
            return xshuffle(DctShuffle::Scatter, s->xsol, s->xfield);
        }
        return s->bx.exec(s->xsol, s->xfield, stream);
    }
    // λy partitioned to this rank's j range; rank 0 zeroes mode (1,1,1) (distributed_fft_based_poisson_solver.jl:104-116,162-164)
    OCN_TRY(ocn::launch_spectral_solve(s->Nxg, s->ny, s->grid.Nz, s->lx, s->ly, s->lz, s->xfield, s->rank == 0, s->rank * s->ny, 0, stream));
    return s->bx.exec(s->xfield, nullptr, stream);
}

extern "C" int ocn_dist_poisson_backward_yz(ocn_dist_poisson_t s, double *p, void *stream_)
{
    OCN_REQUIRE(s && p, "ocn_dist_poisson_backward_yz: null argument");
    hipStream_t stream = ocn::as_stream(stream_);
    if (s->tri && s->fast) {  // recv (after the exchange back) -> real rows of p; the packed inverse carries Ny/2, FFT_x Nxg
        const ocn_grid *g = &s->grid;
        ocn::GridDev gd = ocn::to_dev(*g);
        ocn::Lay Lp = ocn::make_lay(gd, OCN_LOC_CCC);
        return ocn::launch_realfft_y(g->Ny, 1, nullptr, s->recv, p + Lp.o, Lp.s2, Lp.s3, s->nx, g->Nz, s->tw_h, s->tw_y, stream, nullptr,
                                     nullptr, nullptr, nullptr, 1.0, s->ny, (long long)s->ny * g->Nz * s->nx, 0,
                                     1.0 / ((double)(g->Ny / 2) * s->Nxg));
    }
    if (s->tri) {
        OCN_TRY(dist_tri_y_transform(s, 1, stream));
        return ocn::launch_copy_real(&s->grid, s->yfield, p, stream, ocn::CopySource::Complex);
    }
    if (s->fast) {  // send (after the exchange back) -> A1 (in recv) -> real rows of the local pressure interior
        const ocn_grid *g = &s->grid;
        ocn::GridDev gd = ocn::to_dev(*g);
        ocn::Lay Lp = ocn::make_lay(gd, OCN_LOC_CCC);
        const long long cols = (long long)s->nyt * s->nx;
        OCN_TRY(s->xtri ? ocn::launch_colfft(g->Nz, ocn::ColFFT::Inverse, s->recv, cols, 0, (int)cols, 1, s->tw_z, nullptr, nullptr, nullptr, 1.0, 1, stream)
                        : ocn::launch_colfft_slab_z(g->Nz, 1, s->send, s->recv, s->nx, s->nyt, s->R, s->tw_z, stream));
        return ocn::launch_realfft_y(g->Ny, 1, nullptr, s->recv, p + Lp.o, Lp.s2, Lp.s3, s->nx, g->Nz, s->tw_h, s->tw_y, stream);
    }
    if (s->r2c) {
        ocn::GridDev gd = ocn::to_dev(s->grid);
        ocn::Lay Lp = ocn::make_lay(gd, OCN_LOC_CCC);
        return s->byz.exec(s->yfield, p + Lp.o, stream);
    }
    OCN_TRY(s->byz.exec(s->yfield, nullptr, stream));
    // copy_real_component! into the local pressure interior; the local grid's parent layout
    return ocn::launch_copy_real(&s->grid, s->yfield, p, stream, ocn::CopySource::Complex);
}
