// ocn_launchers_scheme.inc -- THE declarations of the launchers that depend on the advection scheme (tendencies.hip, general.hip): included
// inside each of the four namespaces ocn_strict, ocn_fast, ocn_strict_up, ocn_fast_up (ocn_internal.h, general.hip).  Declarations only.
int launch_momentum_tendencies(const ocn_grid *grid, const double *u, const double *v, const double *w, double *Gu,
                               double *Gv, double *Gw, const int32_t *range, const ocn::FuseArgs *fuse, hipStream_t stream);
// what launch_momentum_tendencies would launch, and its status, without launching (ocn_momentum_tendencies_plan)
int plan_momentum_tendencies_query(const ocn_grid *grid, const int32_t *range, const ocn::FuseArgs *fuse, int32_t plan[8]);
int launch_tracer_tendency(const ocn_grid *grid, const double *u, const double *v, const double *w, const double *c,
                           double *Gc, const int32_t *range, hipStream_t stream, const ocn::TracerFuse *fuse = nullptr,
                           const ocn::ForcingDev *forcing = nullptr);
int launch_tracer_pair_tendency(const ocn_grid *grid, const double *u, const double *v, const double *w, const double *const c[2],
                                double *const Gc[2], const int32_t *range, hipStream_t stream, const ocn::TracerFuse fuse[2], int *launched);
// the LDS-tiled kernels over the interior box of a grid with walls in x / y (tendencies.hip, called by general.hip)
int launch_momentum_tendencies_box(const ocn_grid *grid, const double *u, const double *v, const double *w, double *Gu, double *Gv, double *Gw,
                                   const int32_t box[4], int *launched, hipStream_t stream, const ocn::FuseArgs *fuse = nullptr, int ranged = 0);
int launch_tracer_tendency_box(const ocn_grid *grid, const double *u, const double *v, const double *w, const double *c, double *Gc,
                               const int32_t box[4], int *launched, hipStream_t stream, const ocn::TracerFuse *fuse = nullptr, int ranged = 0,
                               const ocn::ForcingDev *forcing = nullptr);
// direction-generic kernels for grids with a Bounded or Flat x / y (general.hip)
int launch_momentum_tendencies_general(const ocn_grid *grid, int centered2, const double *u, const double *v, const double *w, double *Gu,
                                       double *Gv, double *Gw, const int32_t *range, hipStream_t stream, const ocn::MomentumFinal *fin = nullptr);
int launch_tracer_tendency_general(const ocn_grid *grid, int centered2, const double *u, const double *v, const double *w, const double *c,
                                   double *Gc, const int32_t *range, hipStream_t stream, const ocn::TracerFuse *fuse = nullptr,
                                   const ocn::ForcingDev *forcing = nullptr);
