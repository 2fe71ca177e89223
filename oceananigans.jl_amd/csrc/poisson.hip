// poisson.hip -- direct Poisson solvers on one device: creation, the pass executor and the C entry points.
//   FFTBasedPoissonSolver          src/Solvers/fft_based_poisson_solver.jl:5-125   (z regular; any (Periodic | Bounded | Flat)^3 topology)
//   FourierTridiagonalPoissonSolver src/Solvers/fourier_tridiagonal_poisson_solver.jl:6-147 (a Bounded z, or a stretched x / y)
// Eigenvalues: src/Solvers/poisson_eigenvalues.jl:8-31.  Transforms: plan_transforms.jl:36-146.
// (poisson_dist.hip: the distributed slab solver; poisson_general.hip: the any-topology kernels; poisson_selftest.hip: plan checks.)
//
// MI355X design: the divergence of a real velocity field is real, so the transforms are real-to-complex /
// complex-to-real on the Hermitian half spectrum (Nx/2+1 modes in x): half the HBM traffic of the reference's
// in-place C2C (fft_based_poisson_solver.jl:65) with identical results up to FFT round-off.  The inverse
// transform writes straight into the interior of the haloed pressure field (custom output strides), which
// removes the copy_real_component! pass (K13).  OCN_POISSON_C2C=1 selects the literal complex path instead.
//
// Who decides what: creation calls choose_periodic / choose_general (poisson_select.h) ONCE, allocates what that choice needs,
// and records the ordered passes of the three entry points in the handle.  ocn_poisson_compute_source_term,
// ocn_poisson_set_source_term, ocn_poisson_solve and ocn_poisson_solve_shifted walk those lists (run_passes); none of them looks at
// the topology, the grid size or the environment again.
#include <cstring>
#include <string>
#include <utility>

#include "poisson_internal.h"

using namespace ocn::poisson;
using ocn::ColFFT;
using ocn::CopySource;
using ocn::DctShuffle;

ocn_poisson::~ocn_poisson()
{
    for (Plan *p : {&fwd, &bwd, &xr2c, &xc2r}) p->destroy();
    for (int d = 0; d < 3; ++d) {
        line_fwd[d].destroy();
        line_bwd[d].destroy();
        if (partner[d]) (void)hipFree(partner[d]);
    }
    for (double *p : {rhs, spec, spec2, lam[0], lam[1], lam[2], coltw[0], coltw[1], coltw[2], costw[0], costw[1], costw[2], tab[0][0], tab[0][1],
                      tab[1][0], tab[1][1], tab[2][0], tab[2][1], twMx, twNx, tdc, tdf, lower, diag, tscr})
        if (p) (void)hipFree(p);
}

namespace {

// ---------------------------------------------------------------------------------------------------------------------------------
// Creation helpers, one per decision
// ---------------------------------------------------------------------------------------------------------------------------------

// The arrays of a Thomas sweep along a direction of N cells and halo H: own copies of its spacings Δᶜ / Δᶠ when it is stretched (the
// handle must not depend on caller arrays staying alive), lower = upper = 1 / Δᶠ[q], q = 2..N (fourier_tridiagonal_poisson_solver.jl:
// 97-99), and the main diagonal / scratch arrays of n entries (the diagonal is filled by the caller's launch_main_diagonal*).
int make_sweep_arrays(ocn_poisson *s, int N, int H, double uniform, const double *dc, const double *df, size_t n)
{
    const size_t nf = (size_t)N + 2 * H;
    std::vector<double> hf(nf, uniform);
    if (dc) {
        TRY_HIP(hipMalloc((void **)&s->tdc, nf * sizeof(double)));
        TRY_HIP(hipMalloc((void **)&s->tdf, nf * sizeof(double)));
        TRY_HIP(hipMemcpy(s->tdc, dc, nf * sizeof(double), hipMemcpyDeviceToDevice));
        TRY_HIP(hipMemcpy(s->tdf, df, nf * sizeof(double), hipMemcpyDeviceToDevice));
        TRY_HIP(hipMemcpy(hf.data(), df, nf * sizeof(double), hipMemcpyDeviceToHost));
    }
    TRY_HIP(hipMalloc((void **)&s->diag, n * sizeof(double)));
    TRY_HIP(hipMalloc((void **)&s->tscr, n * sizeof(double)));
    std::vector<double> low(N > 1 ? N - 1 : 1, 0.0);
    for (int q = 2; q <= N; ++q) low[q - 2] = 1 / hf[q + H - 1];
    return upload(low, &s->lower);
}
int make_sweep_arrays_z(ocn_poisson *s, const ocn_grid *grid, size_t n)
{
    TRY(make_sweep_arrays(s, grid->Nz, grid->Hz, grid->dz, grid->dzc, grid->dzf, n));
    if (s->tdc) {
        s->grid.dzc = s->tdc;
        s->grid.dzf = s->tdf;
    }
    return OCN_SUCCESS;
}

// x by the row kernel, y by the column kernel: their twiddles, and the y eigenvalues in the stage order y keeps between its two passes
int make_row_column_tables(ocn_poisson *s, const ocn_grid *grid)
{
    std::vector<double> a, b;
    ocn::rowfft_twiddles(grid->Nx, a, b);
    TRY(upload(a, &s->twMx));
    TRY(upload(b, &s->twNx));
    TRY(upload(ocn::colfft_twiddles(grid->Ny), &s->coltw[1]));
    return upload(permuted(eigenvalues(grid->Ny, grid->Ly, grid->ty), stored_wavenumbers(grid->Ny, true)), &s->lam[1]);
}

// batched complex FFT plans along dimension d of a contiguous n0 x n1 x n2 array (x fastest), in place; d = 1 is planned per z plane
int make_line_plans(ocn_poisson *s, int d, const int N[3])
{
    const size_t len[1] = {(size_t)N[d]};
    size_t stride[1], dist, batch;
    if (d == 0) { stride[0] = 1; dist = (size_t)N[0]; batch = (size_t)N[1] * N[2]; }
    else if (d == 1) { stride[0] = (size_t)N[0]; dist = 1; batch = (size_t)N[0]; }
    else { stride[0] = (size_t)N[0] * N[1]; dist = 1; batch = (size_t)N[0] * N[1]; }
    TRY(make_plan(s->line_fwd[d], rocfft_placement_inplace, rocfft_transform_type_complex_forward, 1, len, batch,
                  rocfft_array_type_complex_interleaved, rocfft_array_type_complex_interleaved, stride, dist, stride, dist, 1.0));
    return make_plan(s->line_bwd[d], rocfft_placement_inplace, rocfft_transform_type_complex_inverse, 1, len, batch,
                     rocfft_array_type_complex_interleaved, rocfft_array_type_complex_interleaved, stride, dist, stride, dist, 1.0 / N[d]);
}

int finish_handle(ocn_poisson_t *out, std::unique_ptr<ocn_poisson> &h, const PoissonChoice &c)
{
    h->passes = build_passes(c);
    h->source_wrap = c.source_wrap;
    h->info[0] = c.info_kind();
    h->info[1] = c.info_r2c();
    h->info[2] = c.info_direct_out();
    if (c.tri) h->unshiftable = "ocn_poisson_solve_shifted: FFT-based solvers only";
    else if (c.custom_xy || c.fused_z)
        h->unshiftable = "ocn_poisson_solve_shifted: not available on the fused transform pipelines (a Flat or small z "
                         "uses the plain path; OCN_POISSON_CUSTOM_XY=0 OCN_POISSON_FUSED_Z=0 select it elsewhere)";
    *out = h.release();
    return OCN_SUCCESS;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Any (Periodic | Bounded | Flat)^3 topology (choose_general): separable transforms -- DFT along Periodic, REDFT10 / REDFT01 along
// Bounded directions (plan_transforms.jl:16-34), built from complex FFTs of the same length with index permutations and twiddle factors
// (the reference's K11: index_permutations.jl:38-90, discrete_transforms.jl:141-176), O(N log N) per line -- or, with a Thomas sweep
// along a stretched direction instead of its transform, FourierTridiagonalPoissonSolver on XYRegularRG / YZRegularRG / XZRegularRG
// grids (fourier_tridiagonal_poisson_solver.jl:82-147).  Lines along y and z of a supported length go through the column kernel (ONE
// launch per pass; rocFFT's strided plan needs one per z plane for y): their spectra are then in STAGE order along that direction, so
// eigenvalues and cosine twiddles are stored permuted and partner[d][p] is the stored position of wavenumber N - k(p); a Bounded
// direction on the column kernel runs its whole cosine transform in one pass with natural order on both sides.
//   packed (x Periodic, even Nx, next to a Bounded y / z): the source is REAL and a cosine transform maps reals to reals, so the
//   transforms along the Bounded directions run on the real array VIEWED as Nx / 2 complex columns of x-adjacent pairs (the complex
//   transform of a line is the transform of its real and of its imaginary part) -- half the bytes per pass -- then x is a
//   real-to-complex transform to the half spectrum, on which the remaining Periodic direction, the solve and the way back run.
//   all-real (x AND y Bounded, z Bounded or Flat, even Nx and Ny): nothing ever becomes complex -- y / z on x-adjacent pairs as above,
//   x on pairs of ROWS, a real division by the eigenvalues or (stretched z) the Thomas sweep on reals.
// retry_unpacked is set when the real x plans of the packed variant failed: the caller creates the complex variant instead.
// ---------------------------------------------------------------------------------------------------------------------------------
int create_general(ocn_poisson_t *out, const ocn_grid *grid, int tdim, const double *tdc, const double *tdf, bool packed_ok, bool *retry_unpacked)
{
    const PoissonChoice c = choose_general(*grid, tdim, packed_ok, ocn::colfft_supported);
    if (c.tri && tdim == 2 && (grid->tz != OCN_BOUNDED || grid->Nz < 2)) {
        ocn::set_error("`FourierTridiagonalPoissonSolver` can only be used when the stretched direction's topology is `Bounded` (and Nz >= 2)");
        return OCN_ERR_UNSUPPORTED;
    }
    for (int t : {grid->tx, grid->ty, grid->tz})
        if (t != OCN_PERIODIC && t != OCN_BOUNDED && t != OCN_FLAT) {
            ocn::set_error("ocn_poisson_create: topology code %d is not supported by the general solver", t);
            return OCN_ERR_UNSUPPORTED;
        }
    std::unique_ptr<ocn_poisson> h(new ocn_poisson());
    ocn_poisson *s = h.get();
    s->grid = *grid;
    const int *N = c.N, *topo = c.topo;
    const double Ls[3] = {grid->Lx, grid->Ly, grid->Lz};
    const size_t n = (size_t)N[0] * N[1] * N[2];
    if (c.fft_dct) ensure_rocfft();
    for (int d = 0; d < 3; ++d) {
        const std::vector<int> kofp = stored_wavenumbers(N[d], c.stage_order(d));
        TRY(upload(permuted(eigenvalues(N[d], Ls[d], topo[d]), kofp), &s->lam[d]));
        if (topo[d] == OCN_FLAT) continue;
        if (!c.fft_dct) {  // the direct sums of the definitions: tables of cos / sin over one period (Periodic) or of cos(π m / 2N) (Bounded)
            const double pi = 3.14159265358979323846;
            const int M = topo[d] == OCN_PERIODIC ? N[d] : 4 * N[d];
            std::vector<double> cs(M), sn(M);
            for (int m = 0; m < M; ++m) {
                const double a = topo[d] == OCN_PERIODIC ? 2 * pi * m / N[d] : pi * m / (2.0 * N[d]);
                cs[m] = std::cos(a);
                sn[m] = std::sin(a);
            }
            TRY(upload(cs, &s->tab[d][0]));
            TRY(upload(sn, &s->tab[d][1]));
            continue;
        }
        if (c.col[d] || (d == 0 && c.rowdct)) TRY(upload(ocn::colfft_twiddles(N[d]), &s->coltw[d]));
        if (c.lines[d]) TRY(make_line_plans(s, d, c.line_n[d]));
        if (topo[d] != OCN_BOUNDED) continue;
        TRY(upload(cosine_twiddles(N[d], kofp), &s->costw[d]));
        if (c.stage_order(d)) TRY(upload(partner_positions(kofp), &s->partner[d]));
    }
    TRY_HIP(hipMalloc((void **)&s->spec, n * 2 * sizeof(double)));
    TRY_HIP(hipMalloc((void **)&s->spec2, n * 2 * sizeof(double)));
    if (c.packed && !c.rowdct) {
        // x: real-to-complex / complex-to-real lines.  rocFFT's real plans are verified at creation like the periodic solver's (see
        // Plan::destroy)
        const size_t len[1] = {(size_t)N[0]}, one[1] = {1};
        const size_t nxh = (size_t)N[0] / 2 + 1, batch = (size_t)N[1] * N[2];
        int st = make_plan(s->xr2c, rocfft_placement_notinplace, rocfft_transform_type_real_forward, 1, len, batch, rocfft_array_type_real,
                           rocfft_array_type_hermitian_interleaved, one, (size_t)N[0], one, nxh, 1.0);
        if (st == OCN_SUCCESS)
            st = make_plan(s->xc2r, rocfft_placement_notinplace, rocfft_transform_type_real_inverse, 1, len, batch,
                           rocfft_array_type_hermitian_interleaved, rocfft_array_type_real, one, nxh, one, (size_t)N[0], 1.0 / N[0]);
        if (st == OCN_SUCCESS) st = packed_plans_self_test(s);
        if (st != OCN_SUCCESS) {
            *retry_unpacked = true;
            return st;
        }
    }
    if (c.tri && tdim != 2) {
        // main diagonal of XDirection / YDirection with the (stored-order) eigenvalues of the two transformed directions
        // (fourier_tridiagonal_poisson_solver.jl:17-39)
        const int Ht = tdim == 0 ? grid->Hx : grid->Hy;
        TRY(make_sweep_arrays(s, N[tdim], Ht, 0.0, tdc, tdf, n));
        TRY(ocn::launch_main_diagonal_xy(tdim, N[0], N[1], N[2], Ht, s->tdc, s->tdf, s->lam[tdim == 0 ? 1 : 0], s->lam[2], s->diag, nullptr));
        OCN_CHECK_HIP(hipDeviceSynchronize());
    } else if (c.tri) {
        // main diagonal with the (stored-order) eigenvalues of x and y (fourier_tridiagonal_poisson_solver.jl:41-51)
        TRY(make_sweep_arrays_z(s, grid, n));
        TRY(ocn::launch_main_diagonal(&s->grid, c.packed ? N[0] / 2 + 1 : N[0], s->lam[0], s->lam[1], s->diag, nullptr));
        OCN_CHECK_HIP(hipDeviceSynchronize());
    }
    TRY_HIP(hipMemset(s->spec, 0, n * 2 * sizeof(double)));
    TRY_HIP(hipMemset(s->spec2, 0, n * 2 * sizeof(double)));
    return finish_handle(out, h, c);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// x and y Periodic (choose_periodic): rocFFT (x, y[, z]) plans around the division by the eigenvalues or the z sweep -- or the row
// kernel along x (fused with the source term and with the write into p) and the column kernel along y and z, where the lengths allow.
// On a REGULAR Bounded z of a supported length the sweep is replaced by its exact spectral twin: cosine transform, division, inverse
// cosine transform in ONE column pass -- what the reference's FFTBasedPoissonSolver does on such a grid (plan_transforms.jl:129-140).
// real_plans = false, or retry_complex set on return: see ocn_poisson_create.
// ---------------------------------------------------------------------------------------------------------------------------------
int create_periodic(ocn_poisson_t *out, const ocn_grid *grid, bool real_plans, bool *retry_complex)
{
    TRY(ocn::validate_grid(grid));
    OCN_REQUIRE(grid->tx == OCN_PERIODIC && grid->ty == OCN_PERIODIC,
                "ocn_poisson_create: x and y must be Periodic or Bounded (distributed grids use ocn_dist_poisson_create)");
    if (grid->tz != OCN_BOUNDED && grid->dzc != nullptr) {
        ocn::set_error("FFTBasedPoissonSolver requires a regular z direction");
        return OCN_ERR_UNSUPPORTED;
    }
    ensure_rocfft();
    PoissonChoice c = choose_periodic(*grid, real_plans, ocn::colfft_supported, ocn::rowfft_supported);
    std::unique_ptr<ocn_poisson> h(new ocn_poisson());
    ocn_poisson *s = h.get();
    s->grid = *grid;
    const int Nx = grid->Nx, Ny = grid->Ny, Nz = grid->Nz;
    const int nxh = c.c2c ? Nx : Nx / 2 + 1;  // stored x modes
    const size_t nspec = (size_t)nxh * Ny * Nz;

    TRY(upload(eigenvalues(Nx, grid->Lx, grid->tx), &s->lam[0]));
    if (c.custom_xy) TRY(make_row_column_tables(s, grid));
    else TRY(upload(eigenvalues(Ny, grid->Ly, grid->ty), &s->lam[1]));
    TRY_HIP(hipMalloc((void **)&s->spec, nspec * 2 * sizeof(double)));
    TRY_HIP(hipMemset(s->spec, 0, nspec * 2 * sizeof(double)));
    if (!c.c2c) {
        TRY_HIP(hipMalloc((void **)&s->rhs, (size_t)Nx * Ny * Nz * sizeof(double)));
        TRY_HIP(hipMemset(s->rhs, 0, (size_t)Nx * Ny * Nz * sizeof(double)));
    }
    if (c.tri) {  // (see DESIGN.md for z regular + Bounded)
        TRY_HIP(hipMalloc((void **)&s->spec2, nspec * 2 * sizeof(double)));
        TRY_HIP(hipMemset(s->spec2, 0, nspec * 2 * sizeof(double)));
        TRY(make_sweep_arrays_z(s, grid, nspec));
        if (c.dct_z) {
            TRY(upload(ocn::colfft_twiddles(Nz), &s->coltw[2]));
            TRY(upload(cosine_twiddles(Nz, stored_wavenumbers(Nz, false)), &s->costw[2]));
            TRY(upload(eigenvalues(Nz, grid->Lz, OCN_BOUNDED), &s->lam[2]));
        }
        TRY(ocn::launch_main_diagonal(&s->grid, nxh, s->lam[0], s->lam[1], s->diag, nullptr));
    } else if (c.fused_z) {  // the eigenvalue of each stored position
        TRY(upload(ocn::colfft_twiddles(Nz), &s->coltw[2]));
        TRY(upload(permuted(eigenvalues(Nz, grid->Lz, grid->tz), stored_wavenumbers(Nz, true)), &s->lam[2]));
    } else {
        TRY(upload(eigenvalues(Nz, grid->Lz, grid->tz), &s->lam[2]));
    }

    if (!c.custom_tri) {
        // (the row / column pipeline of a Periodic z creates these plans as well and never runs them: which plans are alive in the process
        // decides whether a LATER real plan of rocFFT misbehaves, so the set of live plans stays what it has been)
        // Layout of the pressure field interior as an FFT output (real plans): strides (1, sx, sx*sy)
        const ocn::GridDev gd = ocn::to_dev(*grid);
        const ocn::Lay Lp = ocn::make_lay(gd, OCN_LOC_CCC);
        const int fft_dims = c.dims3 ? 3 : 2;
        const size_t batch = (fft_dims == 3) ? 1 : (size_t)Nz;
        const size_t len[3] = {(size_t)Nx, (size_t)Ny, (size_t)Nz};
        // fused z path: the whole 1/(Nx Ny Nz) normalisation is applied in the column kernel
        const double scale = c.fused_z ? 1.0 : (fft_dims == 3) ? 1.0 / ((double)Nx * Ny * Nz) : 1.0 / ((double)Nx * Ny);
        if (c.c2c) {
            const size_t str[3] = {1, (size_t)Nx, (size_t)Nx * Ny};
            const size_t dist = (size_t)Nx * Ny * (fft_dims == 3 ? Nz : 1);
            TRY(make_plan(s->fwd, rocfft_placement_inplace, rocfft_transform_type_complex_forward, fft_dims, len, batch,
                          rocfft_array_type_complex_interleaved, rocfft_array_type_complex_interleaved, str, dist, str, dist, 1.0));
            TRY(make_plan(s->bwd, rocfft_placement_inplace, rocfft_transform_type_complex_inverse, fft_dims, len, batch,
                          rocfft_array_type_complex_interleaved, rocfft_array_type_complex_interleaved, str, dist, str, dist, scale));
        } else {
            const size_t rstr[3] = {1, (size_t)Nx, (size_t)Nx * Ny};
            const size_t cstr[3] = {1, (size_t)nxh, (size_t)nxh * Ny};
            const size_t pstr[3] = {1, (size_t)Lp.s2, (size_t)Lp.s3};
            const size_t rdist = (size_t)Nx * Ny * (fft_dims == 3 ? Nz : 1);
            const size_t cdist = (size_t)nxh * Ny * (fft_dims == 3 ? Nz : 1);
            const size_t pdist = (fft_dims == 3) ? (size_t)Lp.s3 * Lp.sz : (size_t)Lp.s3;
            TRY(make_plan(s->fwd, rocfft_placement_notinplace, rocfft_transform_type_real_forward, fft_dims, len, batch,
                          rocfft_array_type_real, rocfft_array_type_hermitian_interleaved, rstr, rdist, cstr, cdist, 1.0));
            if (c.direct_out && make_plan(s->bwd, rocfft_placement_notinplace, rocfft_transform_type_real_inverse, fft_dims, len, batch,
                                          rocfft_array_type_hermitian_interleaved, rocfft_array_type_real, cstr, cdist, pstr, pdist,
                                          scale) != OCN_SUCCESS) {
                // rocFFT has no kernel for this strided-output shape: transform into the contiguous real buffer and
                // copy into the pressure interior (the reference's copy_real_component! pass).
                s->bwd.destroy();
                c.direct_out = false;
            }
            if (!c.direct_out)
                TRY(make_plan(s->bwd, rocfft_placement_notinplace, rocfft_transform_type_real_inverse, fft_dims, len, batch,
                              rocfft_array_type_hermitian_interleaved, rocfft_array_type_real, cstr, cdist, rstr, rdist, scale));
        }
    }
    // every plan pair that a solve runs is verified by a forward + inverse round trip and against known spectra before the handle is
    // handed out (poisson_selftest.hip); a failing real pair is replaced by complex plans, a failing complex pair is an error
    if (!c.custom_xy) {
        const PlanCheck check{c.c2c, c.dims3, c.fused_z, c.direct_out, nxh};
        const int st = plans_self_test(s, check);
        if (st != OCN_SUCCESS) {
            *retry_complex = !c.c2c;
            return st;
        }
    }
    return finish_handle(out, h, c);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The executor: the only reader of a pass list
// ---------------------------------------------------------------------------------------------------------------------------------
struct PassArgs {
    const double *u = nullptr, *v = nullptr, *w = nullptr;  // source passes
    double dt = 1.0;
    const double *R = nullptr;  // set-source passes
    double *p = nullptr;        // the pressure field
};

int run_passes(ocn_poisson *s, const std::vector<PassRec> &list, const PassArgs &x, hipStream_t stream)
{
    const ocn_grid *g = &s->grid;
    double *a = s->spec, *b = s->spec2;  // cur, alt
    double *const *lam = s->lam;
    int st = OCN_SUCCESS;
    for (const PassRec &r : list) {
        const int *n = r.n, d = r.d;
        const long long plane = (long long)n[0] * n[1];
        const int shifted = s->shifted ? 1 : 0;
        switch (r.pass) {
            case Pass::SourceTerm:
                st = ocn::launch_source_term(g, x.u, x.v, x.w, x.dt, (ocn::SourceOut)r.mode, r.to_rhs ? s->rhs : a, g->Nx, (long long)g->Nx * g->Ny,
                                             stream, r.d2, r.wrap);
                s->gathered = st == OCN_SUCCESS && r.d2 >= 0;
                break;
            case Pass::SourceTermStretched:
                st = ocn::launch_source_term_stretched(g, d, s->tdc, x.u, x.v, x.w, x.dt, a, r.d2, stream);
                s->gathered = st == OCN_SUCCESS && r.d2 >= 0;
                break;
            case Pass::SourceRowFFT:
                st = ocn::launch_rowfft(g, 0, x.u, x.v, x.w, nullptr, x.dt, a, nullptr, s->twMx, s->twNx, 1.0, stream, r.mode, r.wrap);
                break;
            case Pass::SetSource:
                st = ocn::launch_set_source(g->Nx, g->Ny, g->Nz, x.R, r.mode ? g->dzc : nullptr, g->Hz, r.to_rhs ? s->rhs : a, r.mode2, g->Nx,
                                            (long long)g->Nx * g->Ny, stream);
                break;
            case Pass::SetSourceUniformDz: {  // Δz is a scalar: a small temporary array of it
                std::vector<double> hz(g->Nz + 2 * g->Hz, g->dz);
                double *dz = nullptr;
                OCN_CHECK_HIP(hipMalloc((void **)&dz, hz.size() * sizeof(double)));
                OCN_CHECK_HIP(hipMemcpyAsync(dz, hz.data(), hz.size() * sizeof(double), hipMemcpyHostToDevice, stream));
                st = ocn::launch_set_source(g->Nx, g->Ny, g->Nz, x.R, dz, g->Hz, r.to_rhs ? s->rhs : a, r.mode2, g->Nx, (long long)g->Nx * g->Ny,
                                            stream);
                OCN_CHECK_HIP(hipStreamSynchronize(stream));
                OCN_CHECK_HIP(hipFree(dz));
                break;
            }
            case Pass::SetSourceStretched:  // multiply_by_stretched_spacing! of YZRegularRG / XZRegularRG
                st = ocn::launch_set_source_stretched(g->Nx, g->Ny, g->Nz, x.R, d, s->tdc, d == 0 ? g->Hx : g->Hy, a, stream);
                break;
            case Pass::RowFFTOfRealSource:
                if (!s->source_in_rhs) break;
                st = ocn::launch_rowfft(g, 0, nullptr, nullptr, nullptr, s->rhs, 1.0, a, nullptr, s->twMx, s->twNx, 1.0, stream);
                if (st == OCN_SUCCESS) s->source_in_rhs = false;
                break;
            case Pass::FFTForward: st = s->fwd.exec(a, nullptr, stream); break;
            case Pass::FFTRealForward: st = s->fwd.exec(s->rhs, a, stream); break;
            case Pass::FFTInverse: st = s->bwd.exec(a, nullptr, stream); break;
            case Pass::FFTRealInverseToField: {
                const ocn::Lay Lp = ocn::make_lay(ocn::to_dev(*g), OCN_LOC_CCC);
                st = s->bwd.exec(a, x.p + Lp.o, stream);
                break;
            }
            case Pass::FFTRealInverseAndCopy:
                st = s->bwd.exec(a, s->rhs, stream);
                if (st == OCN_SUCCESS) st = ocn::launch_copy_real(g, s->rhs, x.p, stream, CopySource::Real);
                break;
            case Pass::ColumnFFT:
            case Pass::ColumnDCT: {  // along y: columns n[0] apart in every z plane; along z: one batch of n[0] n[1] columns
                const double *wd = r.pass == Pass::ColumnDCT ? s->costw[d] : nullptr;
                st = d == 1 ? ocn::launch_colfft(n[1], (ColFFT)r.mode, a, n[0], plane, n[0], n[2], s->coltw[1], nullptr, nullptr, wd, r.scale, 1, stream)
                            : ocn::launch_colfft(n[2], (ColFFT)r.mode, a, plane, 0, (int)plane, 1, s->coltw[2], nullptr, nullptr, wd, r.scale, 1, stream);
                break;
            }
            case Pass::ColumnFFTSolve:
                st = ocn::launch_colfft(n[2], ColFFT::Solve, a, plane, 0, (int)plane, 1, s->coltw[2], lam[0], lam[1], lam[2], r.scale, n[0], stream);
                break;
            case Pass::ColumnDCTSolve:
                st = ocn::launch_colfft_dct_solve(n[2], a, plane, (int)plane, s->coltw[2], s->costw[2], lam[0], lam[1], lam[2], r.scale, n[0], stream);
                break;
            case Pass::ColumnDCTToField: {
                const ocn::Lay Lp = ocn::make_lay(ocn::to_dev(*g), OCN_LOC_CCC);
                const long long p0 = ocn::at(Lp, 1, 1, 1);
                st = d == 1 ? ocn::launch_colfft_dct_to_field(n[1], a, n[0], plane, n[0], n[2], s->coltw[1], s->costw[1], r.scale, n[0], 1, x.p, p0,
                                                              Lp.s2, Lp.s3, stream)
                            : ocn::launch_colfft_dct_to_field(n[2], a, plane, 0, (int)plane, 1, s->coltw[2], s->costw[2], r.scale, n[0], 2, x.p, p0,
                                                              Lp.s2, Lp.s3, stream);
                break;
            }
            case Pass::LineFFT: {
                Plan &P = r.mode ? s->line_bwd[d] : s->line_fwd[d];
                if (d != 1) { st = P.exec(a, nullptr, stream); break; }
                for (int k = 0; k < n[2] && st == OCN_SUCCESS; ++k) st = P.exec(a + (size_t)2 * n[0] * n[1] * k, nullptr, stream);
                break;
            }
            case Pass::RealToHalf: st = s->xr2c.exec(a, b, stream); std::swap(a, b); break;
            case Pass::HalfToReal: st = s->xc2r.exec(a, b, stream); std::swap(a, b); break;
            case Pass::NaiveTransform:
                st = launch_naive_transform(n, d, r.mode2, r.mode, a, b, s->tab[d][0], s->tab[d][1], stream);
                std::swap(a, b);
                break;
            case Pass::Shuffle: {
                if (r.skip_if_gathered && s->gathered) break;
                const DctShuffle m = (DctShuffle)r.mode;
                st = launch_dct_shuffle(n, d, m, a, b, s->costw[d], (m == DctShuffle::PostTwiddle || m == DctShuffle::PreTwiddle) ? s->partner[d] : nullptr,
                                        stream);
                std::swap(a, b);
                break;
            }
            case Pass::TwiddlePermute:
                st = launch_dct_twiddle_permute(n, d, (DctShuffle)r.mode, r.d2, (DctShuffle)r.mode2, a, b, s->costw[d], s->partner[d], stream);
                std::swap(a, b);
                break;
            case Pass::RowPair:
                st = launch_dct_rowpair(n, (DctShuffle)r.mode, a, b, s->costw[0], stream);
                std::swap(a, b);
                break;
            case Pass::RowDCT:
                st = ocn::launch_rowdct(g->Nx, g->Ny, g->Nz, (ocn::RowDCT)r.mode, a, s->coltw[0], s->costw[0], lam[0], lam[1], lam[2], s->shift, shifted,
                                        stream);
                break;
            case Pass::SpectralSolve:  // mode (1, 1, 1) := 0 iff m === 0
                st = ocn::launch_spectral_solve(n[0], n[1], n[2], lam[0], lam[1], lam[2], a, 1, 0, 0, stream, s->shift, s->shifted);
                break;
            case Pass::SpectralSolveReal: st = launch_spectral_solve_real(n, lam[0], lam[1], lam[2], a, s->shift, shifted, stream); break;
            case Pass::SweepX:  // LDS-staged lines, then the zero-mean gauge on the (ky, kz) = (0, 0) line
                st = ocn::launch_tridiag_x(n[0], (long long)n[1] * n[2], s->lower, s->diag, s->lower, a, s->tscr, b, stream);
                std::swap(a, b);
                if (st == OCN_SUCCESS) st = ocn::launch_remove_mean_mode(1, n[0], a, stream);
                break;
            case Pass::SweepY:  // the z kernel with lanes along x and planes n[0] apart; gauge on the (kx, kz) = (0, 0) line
                st = ocn::launch_tridiag_z_strided(n[0], n[2], plane, n[0], n[1], s->lower, s->diag, s->lower, a, s->tscr, b, stream);
                std::swap(a, b);
                if (st == OCN_SUCCESS) st = ocn::launch_remove_mean_mode(n[0], n[1], a, stream);
                break;
            case Pass::SweepZ:  // gauge on the (kx, ky) = (0, 0) column (stored position 0 in either order)
                st = ocn::launch_tridiag_z(n[0], n[1], n[2], s->lower, s->diag, s->lower, a, s->tscr, b, stream);
                std::swap(a, b);
                if (st == OCN_SUCCESS) st = ocn::launch_remove_mean_mode(plane, n[2], a, stream);
                break;
            case Pass::SweepZReal:
                st = ocn::launch_tridiag_z_real(n[0], n[1], n[2], s->lower, s->diag, s->lower, a, s->tscr, b, stream);
                std::swap(a, b);
                if (st == OCN_SUCCESS) st = ocn::launch_remove_mean_mode_real(plane, n[2], a, stream);
                break;
            case Pass::RowFFTToField:
                st = ocn::launch_rowfft(g, 1, nullptr, nullptr, nullptr, nullptr, 1.0, a, x.p, s->twMx, s->twNx, r.scale, stream);
                break;
            case Pass::CopyReal: st = ocn::launch_copy_real(g, a, x.p, stream, (CopySource)r.mode, r.d2); break;
            case Pass::Count_: break;
        }
        if (st != OCN_SUCCESS) break;
    }
    if (a != s->spec) std::swap(s->spec, s->spec2);  // the result lives in `a`: spec stays the array the next source term goes into
    return st;
}

}  // namespace

// ===================================================================================================
// C entry points
// ===================================================================================================
extern "C" int ocn_poisson_create(ocn_poisson_t *out, const ocn_grid *grid)
{
    OCN_REQUIRE(out && grid, "ocn_poisson_create: null argument");
    const bool bounded_xy = grid->tx == OCN_BOUNDED || grid->ty == OCN_BOUNDED || grid->tx == OCN_FLAT || grid->ty == OCN_FLAT;
    bool retry = false;
    if (bounded_xy || (env_set("OCN_POISSON_GENERAL") && grid->dzc == nullptr)) {
        // (the solver only touches a Center field, whose layout does not depend on the topology: its own light validation)
        OCN_REQUIRE(grid->Nx >= 1 && grid->Ny >= 1 && grid->Nz >= 1 && grid->Hx >= 0 && grid->Hy >= 0 && grid->Hz >= 0, "bad grid size / halo");
        OCN_REQUIRE(grid->dx > 0 && grid->dy > 0 && (grid->dzc || grid->dz > 0) && grid->Lx > 0 && grid->Ly > 0 && grid->Lz > 0, "spacings and extents must be positive");
        OCN_REQUIRE((grid->dzc == nullptr) == (grid->dzf == nullptr), "dzc and dzf must both be set or both be NULL");
        const int st = create_general(out, grid, 2, nullptr, nullptr, /*packed_ok=*/true, &retry);
        return retry ? create_general(out, grid, 2, nullptr, nullptr, /*packed_ok=*/false, &retry) : st;
    }
    const int st = create_periodic(out, grid, /*real_plans=*/true, &retry);
    return retry ? create_periodic(out, grid, /*real_plans=*/false, &retry) : st;
}

extern "C" int ocn_poisson_create_stretched(ocn_poisson_t *out, const ocn_grid *grid, int32_t dim, const double *dc, const double *df)
{
    // every argument is checked before the first HIP call
    OCN_REQUIRE(out && grid, "ocn_poisson_create_stretched: null argument");
    OCN_REQUIRE(dim == 0 || dim == 1, "ocn_poisson_create_stretched: dim must be 0 (x) or 1 (y), got %d", dim);
    OCN_REQUIRE(dc && df, "ocn_poisson_create_stretched: null spacing array");
    OCN_REQUIRE(grid->dzc == nullptr && grid->dzf == nullptr,
                "ocn_poisson_create_stretched: z must be regular (grid->dzc == NULL): one stretched direction per solver");
    OCN_REQUIRE((dim == 0 ? grid->tx : grid->ty) == OCN_BOUNDED,
                "`FourierTridiagonalPoissonSolver` can only be used when the stretched direction's topology is `Bounded`.");
    OCN_REQUIRE((dim == 0 ? grid->Nx : grid->Ny) >= 2, "ocn_poisson_create_stretched: the stretched direction needs N >= 2");
    for (int t : {grid->tx, grid->ty, grid->tz})
        OCN_REQUIRE(t == OCN_PERIODIC || t == OCN_BOUNDED || t == OCN_FLAT, "ocn_poisson_create_stretched: topology code %d is not supported", t);
    OCN_REQUIRE(grid->Nx >= 1 && grid->Ny >= 1 && grid->Nz >= 1 && grid->Hx >= 0 && grid->Hy >= 0 && grid->Hz >= 0, "bad grid size / halo");
    OCN_REQUIRE((dim == 1 || grid->dy > 0) && (dim == 0 || grid->dx > 0) && grid->dz > 0 && grid->Lx > 0 && grid->Ly > 0 && grid->Lz > 0,
                "spacings and extents must be positive");
    bool retry = false;  // (the packed variant assumes a sweep along z and is never chosen here)
    return create_general(out, grid, dim, dc, df, /*packed_ok=*/true, &retry);
}

extern "C" int ocn_poisson_destroy(ocn_poisson_t s)
{
    delete s;
    return OCN_SUCCESS;
}

// kind 0: FFT-based, 1: Fourier-tridiagonal (z), 2: FFT-based on any topology, 3: Fourier-tridiagonal on a grid with a Bounded / Flat x or y,
// 4 / 5: Fourier-tridiagonal along a stretched x / y
extern "C" int ocn_poisson_info(ocn_poisson_t s, int32_t *kind, int32_t *r2c, int32_t *direct_out)
{
    OCN_REQUIRE(s, "ocn_poisson_info: null solver");
    if (kind) *kind = s->info[0];
    if (r2c) *r2c = s->info[1];
    if (direct_out) *direct_out = s->info[2];
    return OCN_SUCCESS;
}

// The three pass lists as text, read-only: one line per list ("source:", "set_source:", "solve:"), one item per pass in the order
// run_passes walks them, `pass_name(d=…,mode=…,n=a×b×c)` separated by single spaces.
extern "C" int ocn_poisson_describe(ocn_poisson_t s, char *buf, size_t len)
{
    OCN_REQUIRE(s && buf, "ocn_poisson_describe: null argument");
    std::string out;
    const std::pair<const char *, const std::vector<PassRec> *> lists[] = {
        {"source:", &s->passes.source}, {"set_source:", &s->passes.set_source}, {"solve:", &s->passes.solve}};
    for (const auto &l : lists) {
        out += l.first;
        for (const PassRec &r : *l.second) {
            char item[160];
            snprintf(item, sizeof(item), " %s(d=%d,mode=%d,n=%d×%d×%d)", pass_name(r.pass), r.d, r.mode, r.n[0], r.n[1], r.n[2]);
            out += item;
        }
        out += "\n";
    }
    OCN_REQUIRE(out.size() + 1 <= len, "ocn_poisson_describe: the description needs %zu bytes, the buffer has %zu", out.size() + 1, len);
    memcpy(buf, out.c_str(), out.size() + 1);
    return OCN_SUCCESS;
}

extern "C" int ocn_poisson_source_wraps(ocn_poisson_t s, int32_t *wraps)
{
    OCN_REQUIRE(s && wraps, "ocn_poisson_source_wraps: null argument");
    *wraps = s->source_wrap ? 1 : 0;
    return OCN_SUCCESS;
}

extern "C" int ocn_poisson_compute_source_term(ocn_poisson_t s, const double *u, const double *v, const double *w, double dt,
                                               void *stream)
{
    OCN_REQUIRE(s && u && v && w, "ocn_poisson_compute_source_term: null argument");
    PassArgs x;
    x.u = u; x.v = v; x.w = w; x.dt = dt;
    s->gathered = false;
    s->source_in_rhs = false;
    const int st = run_passes(s, s->passes.source, x, ocn::as_stream(stream));
    s->source_set = (st == OCN_SUCCESS);
    return st;
}

extern "C" int ocn_poisson_set_source_term(ocn_poisson_t s, const double *R, void *stream)
{
    OCN_REQUIRE(s && R, "ocn_poisson_set_source_term: null argument");
    PassArgs x;
    x.R = R;
    const int st = run_passes(s, s->passes.set_source, x, ocn::as_stream(stream));
    s->source_set = (st == OCN_SUCCESS);
    s->source_in_rhs = true;  // (only the row-kernel pipelines have a pass that asks)
    s->gathered = false;      // natural order
    return st;
}

// solve!(ϕ, solver, b, m) with m != 0 (fft_based_poisson_solver.jl:95-125): the screened equation (∇² + m) ϕ = b, no zero-mode gauge
extern "C" int ocn_poisson_solve_shifted(ocn_poisson_t s, double *p, double m, void *stream_)
{
    OCN_REQUIRE(s && p, "ocn_poisson_solve_shifted: null argument");
    OCN_REQUIRE(!s->unshiftable, "%s", s->unshiftable);
    s->shift = m;
    s->shifted = true;
    const int st = ocn_poisson_solve(s, p, stream_);
    s->shift = 0.0;
    s->shifted = false;
    return st;
}

extern "C" int ocn_poisson_solve(ocn_poisson_t s, double *p, void *stream_)
{
    OCN_REQUIRE(s && p, "ocn_poisson_solve: null argument");
    OCN_REQUIRE(s->source_set, "ocn_poisson_solve: source term not set (call ocn_poisson_compute_source_term first)");
    PassArgs x;
    x.p = p;
    const int st = run_passes(s, s->passes.solve, x, ocn::as_stream(stream_));
    s->gathered = false;
    return st;
}

extern "C" int ocn_solve_for_pressure(ocn_poisson_t s, double *p, const double *u, const double *v, const double *w, double dt,
                                      void *stream)
{
    OCN_TRY(ocn_poisson_compute_source_term(s, u, v, w, dt, stream));
    return ocn_poisson_solve(s, p, stream);
}
