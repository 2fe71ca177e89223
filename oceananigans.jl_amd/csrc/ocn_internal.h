// ocn_internal.h -- C++ launchers shared between the translation units of libocn_hip.
#pragma once
#include <vector>

#include "ocn_common.h"

namespace ocn {

constexpr int MAX_TUPLE = 8;

// The modes of the pressure solver's launchers and kernels.  The values are the integers the kernels are instantiated on or receive as
// arguments: a launcher casts, device code never sees the names.
enum class SourceOut : int {  // launch_source_term: what the divergence is stored as
    Divergence = 0,  // real div(U)
    Complex = 1,     // complex div(U) / Δt (K8)
    ComplexDz = 2,   // complex Δzᶜ div(U) / Δt (K9: the right-hand side of the Fourier-tridiagonal solver)
    Real = 3,        // real div(U) / Δt (the source of a real-to-complex or cosine transform)
    RealDz = 4,      // real Δzᶜ div(U) / Δt
};
enum class CopySource : int { Complex = 0, Real = 1 };  // launch_copy_real: real part of a complex array, or a real array
enum class ColFFT : int {  // launch_colfft (colfft.hip MODE)
    Forward = 0,       // natural -> stage order
    Inverse = 1,       // stage order -> natural
    Solve = 2,         // forward, division by the eigenvalues, inverse
    DctForward = 3,    // REDFT10, natural order on both sides
    DctInverse = 4,    // REDFT01 / 2N (launch_colfft_dct_to_field: stored into the pressure field)
    DctSolve = 5,      // REDFT10, division, REDFT01 / 2N (launch_colfft_dct_solve)
};
enum class RowDCT : int {  // launch_rowdct (colfft.hip rowdct_kernel MODE): the x lines of a real array, two rows per complex line
    Forward = 5,         // REDFT10
    Inverse = 6,         // REDFT01 / 2N
    Solve = 7,           // forward, division by the eigenvalues, inverse
    PeriodicSolve = 8,   // the same around the FFT of a Periodic x
};
enum class DctShuffle : int {  // dct_shuffle_kernel, dct_rowpair_kernel and both halves of dct_twiddle_permute_kernel (poisson_general.hip)
    Gather = 0,       // x -> v: even points, then odd points backwards
    PostTwiddle = 1,  // forward: V -> X
    PreTwiddle = 2,   // inverse: X -> V
    Scatter = 3,      // v -> x
};

struct FieldTuple {
    double *f[MAX_TUPLE];
    int loc[MAX_TUPLE];
    int n;
};
struct StepTuple {
    double *U[MAX_TUPLE];
    const double *Gn[MAX_TUPLE];
    double *Gm[MAX_TUPLE];  // written by the cache mode, read otherwise
    int loc[MAX_TUPLE];
    int n;
};

// bottom / top boundary conditions of the fields of a FieldTuple (kind 0: default fill)
struct ZBcTuple {
    ZBc bottom[MAX_TUPLE], top[MAX_TUPLE];
};
int launch_fill_halos(const ocn_grid *grid, const FieldTuple &ft, int open_fill, int only_dir, hipStream_t stream,
                      const ZBcTuple *zbc = nullptr);
struct SideBcTuple {
    ZBc side[6][MAX_TUPLE];  // west, east, south, north, bottom, top of every field of a tuple
};
int launch_fill_halos_general(const ocn_grid *grid, const FieldTuple &ft, int open_fill, hipStream_t stream, const SideBcTuple *bcs = nullptr);
int launch_apply_flux_bcs(const ocn_grid *grid, const FieldTuple &G, const FieldTuple &fields, const ZBcTuple &zbc, hipStream_t stream);
int launch_apply_flux_bcs_lateral(const ocn_grid *grid, const FieldTuple &G, const FieldTuple &fields, const SideBcTuple &bcs, hipStream_t stream);
int launch_advection_timescale(const ocn_grid *grid, const double *u, const double *v, const double *w, double *out, hipStream_t stream);
int launch_hasnan(const double *a, long long n, int *flag, hipStream_t stream);
// particles.hip: sample the tracked fields and (advect != 0) move the particles, one launch
int launch_particles(const ocn_grid *grid, const ocn_particle_geometry *geom, long long n, double *x, double *y, double *z, int advect,
                     double restitution, const double *u, const double *v, const double *w, double dt, int n_tracked,
                     const double *const *tracked_fields, const int32_t *tracked_locs, double *const *tracked_out, hipStream_t stream);
// diagnostics.hip: an operation tree lowered to a straight-line program, evaluated per cell; both validate the whole program first
int op_compute(const ocn_grid *grid, const ocn_op_program *program, double *out, hipStream_t stream);
int op_accumulate(const ocn_grid *grid, const ocn_op_program *program, double *G, hipStream_t stream);
int op_compute_boundary(const ocn_grid *grid, const ocn_op_program *program, int side, double *values, hipStream_t stream);
int op_reduce_workspace(const ocn_grid *grid, int loc, int dims, long long *n_doubles);
int op_reduce(const ocn_grid *grid, const ocn_op_program *program, int dims, double divisor, double *workspace, long long workspace_doubles,
              double *out, hipStream_t stream);
// implicit_diffusion.hip: the explicit part of a vertically implicit ScalarDiffusivity added to G, and the implicit step of n fields
int launch_ivd_explicit_part(const ocn_grid *grid, double nu, const double *u, const double *v, const double *w, double *Gu, double *Gv,
                             double *Gw, int n_tracers, const double *kappa, const double *const *c, double *const *Gc, const int32_t *range,
                             hipStream_t stream);
int launch_ivd_implicit_step(const ocn_grid *grid, int n, double *const *fields, const int32_t *locs, const double *kappa, double dt,
                             hipStream_t stream);
// vertical_diffusivity.hip: ConvectiveAdjustmentVerticalDiffusivity's κ fields, the term of a closure with (Center, Center, Face) ν / κ fields
// added to G, and the implicit step of n fields with a κ field each
int launch_convective_adjustment_diffusivities(const ocn_grid *grid, const ocn_model_terms *terms, const ocn_convective_adjustment *closure,
                                               double *kappa_c, double *kappa_u, hipStream_t stream);
int launch_vertical_diffusivity_fluxes(const ocn_grid *grid, const double *kappa_u, const double *u, const double *v, double *Gu, double *Gv,
                                       int n_tracers, const double *const *kappa_c, const double *const *c, double *const *Gc,
                                       int boundary_only, const int32_t *range, hipStream_t stream);
int launch_ivd_implicit_step_fields(const ocn_grid *grid, int n, double *const *fields, const int32_t *locs, const double *const *kappa,
                                    double *const *scratch, double dt, hipStream_t stream);
// ri_based_diffusivity.hip: RiBasedVerticalDiffusivity.  mode 0: Ri alone; 1: the diffusivities from a stored Ri; 2: both in one launch
int launch_ri_based(int mode, const ocn_grid *grid, const ocn_model_terms *terms, const ocn_ri_based *closure, const ocn_bc *top_T,
                    const ocn_bc *top_S, const double *u, const double *v, const double *ri_in, double *ri_out, double *kappa_c,
                    double *kappa_u, hipStream_t stream);
void ri_taper_host(int kind, long long n, const double *x, double x0, double delta, double *out);
// biharmonic.hip: the term of HorizontalScalarBiharmonicDiffusivity (constant ν, κ; Periodic regular x and y) subtracted from G; neg_other_*:
// minus the term of a tuple's other closure, or NULL
int launch_biharmonic_fluxes(const ocn_grid *grid, double nu, const double *u, const double *v, double *Gu, double *Gv, int n_tracers,
                             const double *kappa, const double *const *c, double *const *Gc, const double *neg_other_u,
                             const double *neg_other_v, const double *const *neg_other_c, hipStream_t stream);
// isopycnal.hip: IsopycnalSkewSymmetricDiffusivity: ϵ_R₃₃, the κz fields and the eddy velocities; the total velocities; the flux divergence
int launch_isopycnal_diffusivities(const ocn_grid *grid, const ocn_model_terms *terms, const ocn_isopycnal *closure, double kappa_skew,
                                   double *eps_R33, double *ue, double *ve, double *we, int n_kz, const double *kappa_symmetric,
                                   double *const *kz, hipStream_t stream);
int launch_sum_velocities(const ocn_grid *grid, const double *const *a, const double *const *b, double *const *out, hipStream_t stream);
int launch_isopycnal_fluxes(const ocn_grid *grid, const ocn_model_terms *terms, const ocn_isopycnal *closure, int n_tracers,
                            const double *kappa_symmetric, const double *kappa_skew, const double *const *c, double *const *Gc,
                            hipStream_t stream);
int launch_profile_marker(hipStream_t stream);
int wait_stream(hipStream_t stream, double seconds, const char *who);
int launch_hydrostatic_pressure(const ocn_grid *grid, const TermsDev &t, double *pHY, hipStream_t stream, const int32_t *irange = nullptr);
int launch_stepper(const ocn_grid *grid, const StepTuple &st, int mode, double dt, double c1, double c2, hipStream_t stream);
int launch_source_term(const ocn_grid *grid, const double *u, const double *v, const double *w, double dt, SourceOut out_mode,
                       double *out, long long ld1, long long ld2, hipStream_t stream, int perm_dim = -1, int wrap = 0);
int launch_set_source(int Nx, int Ny, int Nz, const double *R, const double *dzc, int Hz, double *out, int complex_out,
                      long long ld1, long long ld2, hipStream_t stream);
int launch_spectral_solve(int nxh, int Ny, int Nz, const double *lx, const double *ly, const double *lz, double *b,
                          int zero_mode_here, int joff, int koff, hipStream_t stream, double m = 0.0, int shifted = 0);
int launch_copy_real(const ocn_grid *grid, const double *phi, double *p, hipStream_t stream, CopySource source, int perm_dim = -1);
int launch_pressure_correct(const ocn_grid *grid, double *u, double *v, double *w, const double *p, double dt, hipStream_t stream);
int launch_main_diagonal(const ocn_grid *grid, int nxh, const double *lx, const double *ly, double *D, hipStream_t stream);
int launch_tridiag_z(int Nx, int Ny, int Nz, const double *a, const double *b, const double *c, const double *f, double *t,
                     double *phi, hipStream_t stream, int keep_storage = 0);
int launch_tridiag_z_real(int Nx, int Ny, int Nz, const double *a, const double *b, const double *c, const double *f, double *t, double *phi,
                          hipStream_t stream);
int launch_remove_mean_mode_real(long long s3, int Nz, double *phi, hipStream_t stream);
int launch_tridiag_z_strided(int ni, int nj, long long sj, long long sk, int Nz, const double *a, const double *b, const double *c,
                             const double *f, double *t, double *phi, hipStream_t stream, int keep_storage = 0);
int launch_main_diagonal_strided(const ocn_grid *grid, int ni, int nj, long long sj, long long sk, const double *lx, const double *ly,
                                 double *D, hipStream_t stream);
int launch_remove_mean_mode(long long s3, int Nz, double *phi, hipStream_t stream);
// stretched.hip: the Fourier-tridiagonal solver along a stretched x (dim 0) or y (dim 1)
int launch_tridiag_x(int N, long long nlines, const double *a, const double *b, const double *c, const double *f, double *t, double *phi,
                     hipStream_t stream, int keep_storage = 0);
int launch_tridiag_x_real(int N, long long nlines, const double *a, const double *b, const double *c, const double *f, double *t, double *phi,
                          hipStream_t stream, int keep_storage = 0);
int launch_main_diagonal_xy(int dim, int Nx, int Ny, int Nz, int H, const double *dc, const double *df, const double *l1, const double *l2,
                            double *D, hipStream_t stream);
int launch_source_term_stretched(const ocn_grid *grid, int dim, const double *dc, const double *u, const double *v, const double *w, double dt,
                                 double *out, int perm_dim, hipStream_t stream);
int launch_set_source_stretched(int Nx, int Ny, int Nz, const double *R, int dim, const double *dc, int H, double *out, hipStream_t stream);
// column FFTs (colfft.hip).  N in {64, 128, 256, 512}.
bool colfft_supported(int N);
int colfft_wavenumber(int N, int p);
std::vector<double> colfft_twiddles(int N);
int launch_colfft(int N, ColFFT mode, double *data, long long col_stride, long long batch_stride, int ncols, int nbatch,
                  const double *tw, const double *lx, const double *ly, const double *lc, double scale, int inner,
                  hipStream_t stream, int zero_mode = 1);
int launch_colfft_dct_solve(int N, double *data, long long col_stride, int ncols, const double *tw, const double *wd, const double *lx,
                            const double *ly, const double *lz, double scale, int inner, hipStream_t stream);
int launch_colfft_dct_to_field(int N, double *data, long long col_stride, long long batch_stride, int ncols, int nbatch, const double *tw,
                               const double *wd, double scale, int inner, int pdim, double *p, long long p0, long long ps2, long long ps3,
                               hipStream_t stream);
// slab pipeline of the distributed solver (colfft.hip): real y transform and z transform into / out of the all-to-all layout
bool realfft_y_supported(int Ny);
int launch_realfft_y(int Ny, int inverse, const double *rhs, double *spec, double *p, long long p_s2, long long p_s3, int nx, int Nz,
                     const double *twH, const double *twN, hipStream_t stream, const ocn_grid *grid = nullptr,
                     const double *u = nullptr, const double *v = nullptr, const double *w = nullptr, double dt = 1.0, int kc = 0,
                     long long chunk = 0, int scale_dz = 0, double scale = 1.0);
// transpose-free x direction of the distributed pressure solve (xtri.hip)
bool xtri_supported(int R, int Nxg);
int launch_xtri_sweep(double *a1, const double *ly, const double *lz, int NyH, int nx, int Nz, double dx, double scale, double *gsend,
                      hipStream_t stream);
int launch_xtri_finish(double *a1, const double *ly, const double *lz, int NyH, int nx, int Nz, double dx, const double *grecv, int rank,
                       int R, hipStream_t stream);
int launch_vector_invariant_weno(const ocn_grid *grid, int scheme_flags, const double *u, const double *v, const double *w, double *Gu,
                                 double *Gv, const double *eta, double grav, hipStream_t stream);  // vector_invariant_weno.hip
int launch_split_explicit_substeps_blocked(const ocn_grid *grid, int n, const double *weights, double dtau, double grav, double H, double *eta,
                                           double *U, double *V, double *etab, double *Ub, double *Vb, const double *GU, const double *GV,
                                           double *work, hipStream_t stream);
int launch_split_explicit_substeps_ab3(const ocn_grid *grid, int n, const double *weights, double dtau, double grav, double H, const double *coef,
                                       double *eta, double *U, double *V, double *etab, double *Ub, double *Vb, const double *GU, const double *GV,
                                       double *work, hipStream_t stream);
int launch_split_explicit_dist_begin(const ocn_grid *grid, int W, const double *eta, const double *U, const double *V, const double *GU,
                                     const double *GV, double *work, double *send_west, double *send_east, hipStream_t stream);
int launch_split_explicit_dist_run(const ocn_grid *grid, int W, int n, const double *weights, double dtau, double grav, double H, double *eta,
                                   double *U, double *V, double *work, const double *recv_west, const double *recv_east, hipStream_t stream);
int launch_barotropic_correct_w(const ocn_grid *grid, const double *us, const double *vs, double *u, double *v, double *w, const double *U,
                                const double *V, const double *Us, const double *Vs, double H, hipStream_t stream);
int launch_free_surface_ab2(const ocn_grid *grid, const double *w, double *eta, double *Gn, const double *Gm, double dt, double chi,
                            hipStream_t stream);
// the hydrostatic kernels of every horizontal topology -- (Periodic, Periodic | Bounded, Bounded), (Bounded, Bounded, Bounded) --
// (hydrostatic_surface.hip): per-location parent layouts and planes.  Bottom: the GridFittedBottom of an ImmersedBoundaryGrid as the
// kernels see it -- kbot, the int32 plane of immersed cells per column, and the column depths at the u and v points; all null: a flat bottom
struct Bottom {
    const int32_t *kbot = nullptr;
    const double *Hfc = nullptr, *Hcf = nullptr;
    bool fitted() const { return kbot || Hfc || Hcf; }
};
int launch_w_from_continuity(const ocn_grid *grid, const double *u, const double *v, double *w, hipStream_t stream);
int launch_vector_invariant(const ocn_grid *grid, const Bottom &bottom, const double *u, const double *v, const double *w, double *Gu, double *Gv,
                            const double *eta, double grav, hipStream_t stream);
int launch_barotropic_gradient(const ocn_grid *grid, double grav, const double *eta, double *Gu, double *Gv, hipStream_t stream);
int launch_implicit_free_surface_rhs(const ocn_grid *grid, const double *u, const double *v, const double *eta, double grav, double dt,
                                     double *Qu, double *Qv, double *rhs, hipStream_t stream);
int launch_barotropic_pressure_correction(const ocn_grid *grid, double *u, double *v, const double *eta, double grav, double dt,
                                          hipStream_t stream);
int launch_plane_halo(const ocn_grid *grid, double *plane, hipStream_t stream);
int launch_split_explicit_forcing(const ocn_grid *grid, const Bottom &bottom, const double *Gun, const double *Gum, const double *Gvn,
                                  const double *Gvm, double chi, double *GU, double *GV, hipStream_t stream);
// (H: the column depth over a flat bottom; a fitted one brings its depths)
int launch_split_explicit_substeps(const ocn_grid *grid, const Bottom &bottom, int n, const double *weights, double dtau, double grav, double H,
                                   double *eta, double *U, double *V, double *etab, double *Ub, double *Vb, const double *GU, const double *GV,
                                   hipStream_t stream);
int launch_barotropic_mode(const ocn_grid *grid, const double *u, const double *v, double *U, double *V, hipStream_t stream);
int launch_barotropic_corrector(const ocn_grid *grid, const Bottom &bottom, double *u, double *v, const double *U, const double *V, double *Ub,
                                double *Vb, double H, hipStream_t stream);
// the kernels over a GridFittedBottom that have no flat twin above (immersed.hip)
int launch_immersed_bottom(const ocn_grid *grid, int interface_condition, const double *h, const double *zc, const double *zf, double *bottom,
                           int32_t *kbot, double *Hcc, double *Hfc, double *Hcf, hipStream_t stream);
int launch_immersed_mask(const ocn_grid *grid, const int32_t *kbot, const FieldTuple &f, double value, double *eta, double *U, double *V,
                         hipStream_t stream);
int launch_viscosity_immersed(const ocn_grid *grid, const int32_t *kbot, double nu, const double *u, const double *v, const double *w,
                              double *Gu, double *Gv, hipStream_t stream);
int launch_tracer_immersed(const ocn_grid *grid, const int32_t *kbot, int diffuse, double kappa, const double *u, const double *v,
                           const double *w, const double *c, double *Gc, hipStream_t stream);
int launch_halo_plane_x(const ocn_grid *grid, double *field, int loc, int which, double *buf, int unpack, hipStream_t stream);
int launch_halo_pack_x_fields(const ocn_grid *grid, const FieldTuple &ft, double *west, double *east, int unpack, hipStream_t stream);
int launch_rowdct(int Nx, int Ny, int Nz, RowDCT mode, double *data, const double *tw, const double *wd, const double *lx, const double *ly,
                  const double *lz, double shift, int shifted, hipStream_t stream);
int launch_colfft_slab_z(int Nz, int inverse, const double *in, double *out, int nx, int NyH, int R, const double *tw, hipStream_t stream);
// row FFTs (rowfft.hip): inverse = 0: [div(u,v,w)/dt | real_in] -> half spectrum;  1: half spectrum -> rows of haloed p
bool rowfft_supported(int Nx);
void rowfft_twiddles(int Nx, std::vector<double> &twM, std::vector<double> &twN);
int launch_rowfft(const ocn_grid *grid, int inverse, const double *u, const double *v, const double *w, const double *real_in,
                  double dt, double *spec, double *p, const double *twM, const double *twN, double scale, hipStream_t stream,
                  int scale_dz = 0, int wrap = 0);
int launch_halo_pack_x(const ocn_grid *grid, const double *field, int loc, double *west, double *east, int unpack, hipStream_t stream);
int launch_transpose(int mode, int nx, int Ny, int Nz, int R, const double *src, double *dst, hipStream_t stream);

}  // namespace ocn

namespace ocn {
// the descriptor of one field's forcing (capi.hip): host memory only, no device pointer is followed
int validate_forcing(const ocn_grid *grid, const ocn_forcing *f, const char *who, const char *field);
}

// The launchers of the kernels that are compiled once per arithmetic variant (and per advection scheme): every signature is written once,
// in the two fragments, and declared from there in each namespace that defines it (ocn_weno.h: OCN_NS).
namespace ocn_strict {
#include "ocn_launchers_scheme.inc"
#include "ocn_launchers_math.inc"
}
namespace ocn_fast {
#include "ocn_launchers_scheme.inc"
#include "ocn_launchers_math.inc"
}
// advection = UpwindBiased(order=5): tendencies.hip and general.hip compiled with OCN_UPWIND=1
namespace ocn_strict_up {
#include "ocn_launchers_scheme.inc"
}
namespace ocn_fast_up {
#include "ocn_launchers_scheme.inc"
}
