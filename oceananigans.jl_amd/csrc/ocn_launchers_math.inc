// ocn_launchers_math.inc -- THE declarations of the launchers that do not depend on the advection scheme (physics.hip, amd.hip,
// smagorinsky.hip, the extra-terms part of general.hip, the pressure planes of tendencies.hip): included inside the two namespaces
// ocn_strict and ocn_fast (ocn_internal.h, general.hip); the UpwindBiased builds do not define them.  Declarations only.
int launch_momentum_centered2(const ocn_grid *grid, const double *u, const double *v, const double *w, double *Gu, double *Gv,
                              double *Gw, const int32_t *range, hipStream_t stream);
int launch_tracer_centered2(const ocn_grid *grid, const double *u, const double *v, const double *w, const double *c,
                            double *Gc, const int32_t *range, hipStream_t stream);
int launch_momentum_extra(const ocn_grid *grid, const ocn::TermsDev &t, const double *u, const double *v, const double *w,
                          double *Gu, double *Gv, double *Gw, const int32_t *range, hipStream_t stream,
                          const ocn::MomentumFinal *fin = nullptr, const ocn::StokesDev *stokes = nullptr,
                          const ocn::MomentumForcingDev *forcing = nullptr);
// the tiled finishing pass over the interior box of a grid with walls in x / y (physics.hip, called by general.hip)
int launch_momentum_extra_box(const ocn_grid *grid, const ocn::TermsDev &t, const double *u, const double *v, const double *w, double *Gu, double *Gv,
                              double *Gw, const int32_t box[4], int *launched, hipStream_t stream, const ocn::MomentumFinal *fin, int ranged = 0,
                              const ocn::StokesDev *stokes = nullptr, const ocn::MomentumForcingDev *forcing = nullptr);
int launch_momentum_extra_general(const ocn_grid *grid, const ocn::TermsDev &t, const double *u, const double *v, const double *w, double *Gu,
                                  double *Gv, double *Gw, const int32_t *range, hipStream_t stream, const ocn::MomentumFinal *fin = nullptr,
                                  const ocn::StokesDev *stokes = nullptr, const ocn::MomentumForcingDev *forcing = nullptr);
int launch_tracer_forcing(const ocn_grid *grid, const ocn::ForcingDev &forcing, const double *c, double *Gc, const int32_t *range,
                          const ocn::TracerFuse *fuse, hipStream_t stream);
int launch_hydrostatic_momentum(const ocn_grid *grid, const ocn::TermsDev &t, const double *u, const double *v, const double *w, double *Gu,
                                double *Gv, const ocn::MomentumFinal &mf, const ocn::HydroFuse &hf, hipStream_t stream);
int launch_tracer_diffusion(const ocn_grid *grid, double kappa, const double *kappa_e, const double *c, double *Gc,
                            const int32_t *range, hipStream_t stream);
int launch_pressure_planes(const ocn_grid *grid, double *p, double *u, double dt, double *west, double *east, int unpack, hipStream_t stream);
int launch_amd_fused(const ocn_grid *grid, double Cnu, const double *u, const double *v, const double *w, double *nu_e, int ntr,
                     const double *Ck, const double *const *c, double *const *kappa_e, hipStream_t stream, const int32_t *irange = nullptr);
int launch_amd_viscosity(const ocn_grid *grid, double Cnu, const double *u, const double *v, const double *w, double *nu_e,
                         hipStream_t stream);
int launch_amd_diffusivity(const ocn_grid *grid, double Ck, const double *u, const double *v, const double *w, const double *c,
                           double *kappa_e, hipStream_t stream);
int launch_smagorinsky(const ocn_grid *grid, const ocn::TermsDev &t, const ocn_smagorinsky &closure, const double *u, const double *v,
                       const double *w, double *nu_e, double *const *kappa_e, hipStream_t stream);
