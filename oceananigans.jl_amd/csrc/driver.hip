// driver.hip -- time_step!(model::NonhydrostaticModel{<:RungeKutta3TimeStepper}, Δt) as ONE call of the C ABI
// (src/TimeSteppers/runge_kutta_3.jl:77-151), for the model of the north-star benchmark: WENO5 advection, no tracers, no
// extra terms, (Periodic, Periodic, Periodic | Bounded | Flat), one GPU.
//
// Why it exists: the per-kernel entry points are what a Julia backend binds one by one, but the stage-boundary fusion that
// makes the step fast (tendencies + the next substep in one launch writing a SECOND set of velocity
// arrays, G^n / G^- swapped instead of copied, the last tendency launch of a step deferred into the next step, the pressure
// correction folded into the tendency loads on all-periodic grids) needs arrays whose roles alternate -- which a host that
// cannot swap array storage cannot express.  This handle owns the second set and the tendency buffers and does the
// alternation itself; the caller's arrays hold the velocities whenever it asks (ocn_rk3_driver_flush).  Host code only: every
// device operation is one of the public entry points, in the order the Python host (models.py) issues them, so the two are
// bit-identical (tests/test_gpu_model.py::test_c_driver_equals_host_orchestration).
#include <cstring>

#include "ocn_driver_core.h"

// the two sets of u, v, w and their tendencies, and the handles of the projection (a slab-x rank, ocn_rk3_driver_create_distributed:
// RCCL communicator + distributed Poisson handle, both borrowed): ocn_driver_core.h
struct ocn_rk3_driver : ocn::FieldSets<3>, ocn::Projection {
    ocn_grid grid{};
    double *p = nullptr;          // the caller's pressure parent
    bool pending = false;         // the last compute_tendencies! of the previous step is still due
    bool started = false;         // iteration 0 done
    bool correct_on_load = false;
    long long iteration = 0;
    // the third stage's pressure correction is left to the next step's first fused launch (applied on load like stages 1 and 2): the
    // velocities in U are then the UNCORRECTED u*, v*, w* with valid halos, p holds the pressure, ocn_rk3_driver_flush applies it
    bool defer_correction = false;
    bool correction_pending = false;
    double correction_dt = 0.0;
    // the last fused launch also wrote the x strips of its stepped velocities into the communicator's send buffers
    // (ocn_compute_momentum_tendencies_rk3_strips): the next exchange of U is posted without a pack launch
    bool use_strips = false, strips_ready = false;
    // One GPU, all-periodic, correction on load through the 32-bit kernel (ocn_momentum_tendencies_addr32): work of a step whose result
    // nobody reads is left out.  Each has its environment switch (= 0 restores the work), read at creation like OCN_CORRECT_ON_LOAD.
    //   skip_g_store   OCN_DRIVER_SKIP_G_STORE: the third fused launch of a step does not store G^n -- the next step's first launch has no
    //                  G^- term and overwrites the same buffer without a swap in between, and flush recomputes it (pending)
    //   wrapped_loads  OCN_DRIVER_WRAPPED_LOADS: no halo fill of u*, v*, w* in front of the solve -- its two readers, the solver's source
    //                  pass (ocn_poisson_source_wraps) and the next fused launch, wrap their indices instead
    //   fused_flush    OCN_DRIVER_FUSED_FLUSH=1 (off by default: not yet measured against the two passes it replaces): the deferred
    //                  correction and the deferred tendencies of a flush in ONE launch
    bool skip_g_store = false, wrapped_loads = false, fused_flush = false;
};

namespace {
// fill_halo_regions!(velocities): local periodic / wall fills, then -- on a slab -- the x exchange with the neighbours (synchronous)
int fill_velocities(ocn_rk3_driver *d, int fbnv, void *stream)
{
    d->strips_ready = false;  // (this exchange packs into the same send buffers)
    return ocn::fill_and_exchange(&d->grid, d->comm, d->U, d->locs, nullptr, 3, fbnv, stream);
}

int fill_pressure(ocn_rk3_driver *d, void *stream)
{
    const int32_t ploc = OCN_LOC_CCC;
    double *pf[1] = {d->p};
    return ocn::fill_and_exchange(&d->grid, d->comm, pf, &ploc, nullptr, 1, 1, stream);
}

// update_state! + the next rk3_substep! in one launch, then the two velocity sets trade places
int fused_launch(ocn_rk3_driver *d, double dt, double gamma, double zeta, int has_zeta, const double *p_correct, double dt_correct,
                 int32_t flags, void *stream)
{
    int st;
    d->strips_ready = false;
    if (d->use_strips && p_correct) {
        double *sw = nullptr, *se = nullptr;
        int64_t per_field = 0;
        OCN_TRY(ocn_halo_exchange_buffers(d->comm, &d->grid, d->locs, 3, &sw, &se, &per_field));
        st = ocn_compute_momentum_tendencies_rk3_strips(&d->grid, d->U[0], d->U[1], d->U[2], d->Gn[0], d->Gn[1], d->Gn[2], d->Gm[0], d->Gm[1],
                                                        d->Gm[2], d->A[0], d->A[1], d->A[2], dt, gamma, zeta, has_zeta, p_correct, dt_correct,
                                                        sw, se, per_field, stream);
        d->strips_ready = st == OCN_SUCCESS;
    } else if (flags && p_correct) {
        st = ocn_compute_momentum_tendencies_rk3_flags(&d->grid, d->U[0], d->U[1], d->U[2], d->Gn[0], d->Gn[1], d->Gn[2], d->Gm[0], d->Gm[1],
                                                       d->Gm[2], d->A[0], d->A[1], d->A[2], dt, gamma, zeta, has_zeta, p_correct, dt_correct,
                                                       flags, stream);
    } else {
        st = ocn_compute_momentum_tendencies_rk3(&d->grid, d->U[0], d->U[1], d->U[2], d->Gn[0], d->Gn[1], d->Gn[2], d->Gm[0], d->Gm[1],
                                                 d->Gm[2], d->A[0], d->A[1], d->A[2], dt, gamma, zeta, has_zeta, p_correct, dt_correct,
                                                 nullptr, stream);
    }
    if (st != OCN_SUCCESS) return st;
    d->swap_sets();
    d->pending = false;
    return OCN_SUCCESS;
}

// The projection of a stage up to (not including) the correction, for a launch that corrects on load: halos of the uncorrected
// velocities, pressure solve and -- on a slab -- the pressure planes of the neighbours.  On a slab the exchange of u*, v*, w* is posted
// BEFORE the solve (only the plane the divergence reads is waited for) and flies under it on the communication stream.
// wrapped_loads: no fill at all -- the halos of U stay stale until the next fill_velocities (flush), and nothing reads them before.
int project_for_load(ocn_rk3_driver *d, double stage_dt, void *stream)
{
    if (!d->wrapped_loads) OCN_TRY(ocn_fill_halo_regions(&d->grid, d->U, d->locs, 3, 1, stream));
    if (d->comm) {
        OCN_TRY(ocn_halo_exchange_plane(d->comm, &d->grid, d->U[0], OCN_LOC_FCC, 0, stream));  // u[nx+1] <- east neighbour's u[1]
        // the strips of u*, v*, w*: already in the send buffers when the last fused launch wrote them (no pack launch), packed here otherwise
        const int st = d->strips_ready ? ocn_halo_exchange_begin_packed(d->comm, &d->grid, d->U, d->locs, 3, stream)
                                   : ocn_halo_exchange_begin(d->comm, &d->grid, d->U, d->locs, 3, stream);
        d->strips_ready = false;
        if (st != OCN_SUCCESS) return st;
    }
    OCN_TRY(d->solve(d->p, d->U, stage_dt, stream));
    if (d->comm) {
        OCN_TRY(ocn_halo_exchange_end(d->comm, &d->grid, d->U, d->locs, 3, stream));
        OCN_TRY(ocn_halo_exchange_pressure(d->comm, &d->grid, d->p, d->U[0], stage_dt, stream));
    }
    return OCN_SUCCESS;
}

// calculate_pressure_correction! + pressure_correct_velocities! + the halo fill of update_state! (pressure_correction.jl:8-50)
int project_and_correct(ocn_rk3_driver *d, double stage_dt, bool solve_too, void *stream)
{
    if (solve_too) {
        OCN_TRY(fill_velocities(d, 1, stream));
        OCN_TRY(d->solve(d->p, d->U, stage_dt, stream));
    }
    OCN_TRY(fill_pressure(d, stream));
    OCN_TRY(ocn_pressure_correct_velocities(&d->grid, d->U[0], d->U[1], d->U[2], d->p, stage_dt, stream));
    return fill_velocities(d, 0, stream);
}

// everything between two substeps (runge_kutta_3.jl:103-118).  last_of_step: the launch is the last one of a step that ends with the
// tendencies pending, so its G^n is dead (skip_g_store).
int project_and_advance(ocn_rk3_driver *d, double dt, double stage_dt, double gamma_next, double zeta_next, bool last_of_step, void *stream)
{
    if (d->correct_on_load) {
        OCN_TRY(project_for_load(d, stage_dt, stream));
        d->swap_tendencies();
        const int32_t flags = (d->wrapped_loads ? OCN_RK3_WRAPPED_LOADS : 0) | (last_of_step && d->skip_g_store ? OCN_RK3_SKIP_G_STORE : 0);
        return fused_launch(d, dt, gamma_next, zeta_next, 1, d->p, stage_dt, flags, stream);
    }
    OCN_TRY(project_and_correct(d, stage_dt, true, stream));
    d->swap_tendencies();
    return fused_launch(d, dt, gamma_next, zeta_next, 1, nullptr, 0.0, 0, stream);
}
}  // namespace

extern "C" int ocn_rk3_driver_destroy(ocn_rk3_driver_t d)
{
    if (!d) return OCN_SUCCESS;
    d->release_solver();
    d->release();
    delete d;
    return OCN_SUCCESS;
}

static int driver_create(ocn_rk3_driver_t *out, const ocn_grid *grid, double *u, double *v, double *w, double *p, ocn_poisson_t solver,
                         ocn_dist_poisson_t dsolver, ocn_comm_t comm, void *stream)
{
    OCN_REQUIRE(out && grid && u && v && w && p, "ocn_rk3_driver_create: null argument");
    // one GPU: any topology the per-call entry points take -- on grids with walls / Flat directions in x, y the fused launch runs the tiled
    // epilogue on the interior box and the finishing kernel on the wall frames (general.hip), without the correction on load
    OCN_TRY(comm ? ocn::validate_grid(grid) : ocn::validate_grid_any(grid));
    if (comm) {
        OCN_REQUIRE(grid->tx == OCN_FULLY_CONNECTED && grid->ty == OCN_PERIODIC && grid->tz == OCN_PERIODIC && dsolver,
                    "ocn_rk3_driver_create_distributed: a (FullyConnected, Periodic, Periodic) local grid and its distributed Poisson handle");
        int32_t fast = 0;
        OCN_TRY(ocn_dist_poisson_pipeline(dsolver, &fast));
        if (fast != 1 && fast != 3) {
            ocn::set_error("ocn_rk3_driver_create_distributed: the Poisson handle runs the transposing path (sizes outside the slab "
                           "pipelines): drive it through the per-call entry points");
            return OCN_ERR_UNSUPPORTED;
        }
        OCN_REQUIRE(grid->Nx >= 16 && grid->Nx >= grid->Hx + 1 && grid->Ny >= 8 && grid->Nz >= 4,
                    "ocn_rk3_driver_create_distributed: the local slab must be at least 16 x 8 x 4");
    } else {
        OCN_TRY(ocn::require_unpartitioned_x(grid, "ocn_rk3_driver"));
    }
    ocn_rk3_driver *d = new ocn_rk3_driver();
    d->grid = *grid;
    d->user[0] = u; d->user[1] = v; d->user[2] = w;
    d->p = p;
    int st = d->allocate(*grid, "ocn_rk3_driver_create");
    if (st == OCN_SUCCESS) st = d->adopt_solver(grid, solver, dsolver, comm);  // borrowed, the driver's own, or the slab handle
    if (st != OCN_SUCCESS) {
        ocn_rk3_driver_destroy(d);
        return st;
    }
    // fold the pressure correction into the loads of the fused launch: all-periodic grids the tiled kernel covers, one GPU or a slab.
    // OCN_CORRECT_ON_LOAD=0 (on a slab also OCN_DIST_CORRECT_ON_LOAD=0, the Python host's switch) is the conservative path for a first
    // multi-GPU run: every stage = synchronous halo exchange -> solve -> synchronous pressure exchange -> pressure_correct_velocities!
    // -> synchronous exchange -> one plain fused launch; no exchange is in flight while the solver's collective runs.
    const char *e = std::getenv("OCN_CORRECT_ON_LOAD"), *ed = std::getenv("OCN_DIST_CORRECT_ON_LOAD");
    const bool off = (e && e[0] == '0') || (comm && ed && ed[0] == '0');
    const bool all_periodic = grid->tx == OCN_PERIODIC && grid->ty == OCN_PERIODIC && grid->tz == OCN_PERIODIC;
    d->correct_on_load = (comm || (all_periodic && grid->Nx >= 16 && grid->Ny >= 8 && grid->Nz >= 4)) && !off;
    // strips written by the fused launch's epilogue instead of a pack launch: OCN_DIST_EPILOGUE_STRIPS=1.  Off by default -- measured at
    // the local sizes of one rank of 2 / of 8 (512^3, replica transport): 14.79 / 4.09 ms per rank-step with, 14.61 / 4.05 without: the
    // scattered 8-byte stores of the edge tiles and the wrapping unpack cost what the 40-us pack launch saves.
    const char *es = std::getenv("OCN_DIST_EPILOGUE_STRIPS");
    d->use_strips = comm && d->correct_on_load && grid->Nx >= 2 * grid->Hx && es && es[0] == '1';
    const char *dc = std::getenv("OCN_DRIVER_DEFER_CORRECTION");
    d->defer_correction = d->correct_on_load && !(dc && dc[0] == '0');
    // dead work left out (see the struct): the fused launches of a one-GPU box through the 32-bit kernel
    int32_t addr32 = 0, wraps = 0;
    if (!comm && d->correct_on_load) {
        st = ocn_momentum_tendencies_addr32(grid, &addr32);
        if (st == OCN_SUCCESS) st = ocn_poisson_source_wraps(d->solver, &wraps);
        if (st != OCN_SUCCESS) {
            ocn_rk3_driver_destroy(d);
            return st;
        }
    }
    auto enabled = [](const char *name) { const char *v = std::getenv(name); return !(v && v[0] == '0'); };
    d->skip_g_store = addr32 && enabled("OCN_DRIVER_SKIP_G_STORE");
    d->wrapped_loads = addr32 && wraps && enabled("OCN_DRIVER_WRAPPED_LOADS");
    const char *ff = std::getenv("OCN_DRIVER_FUSED_FLUSH");
    d->fused_flush = addr32 && ff && ff[0] == '1';
    st = fill_velocities(d, 0, stream);  // update_state!(model; compute_tendencies = false) of the constructor
    if (st != OCN_SUCCESS) {
        ocn_rk3_driver_destroy(d);
        return st;
    }
    *out = d;
    return OCN_SUCCESS;
}

extern "C" int ocn_rk3_driver_create(ocn_rk3_driver_t *out, const ocn_grid *grid, double *u, double *v, double *w, double *p,
                                     ocn_poisson_t solver, void *stream)
{
    return driver_create(out, grid, u, v, w, p, solver, nullptr, nullptr, stream);
}

extern "C" int ocn_rk3_driver_create_distributed(ocn_rk3_driver_t *out, const ocn_grid *local_grid, double *u, double *v, double *w,
                                                 double *p, ocn_dist_poisson_t solver, ocn_comm_t comm, void *stream)
{
    OCN_REQUIRE(solver && comm, "ocn_rk3_driver_create_distributed: null solver / communicator");
    return driver_create(out, local_grid, u, v, w, p, nullptr, solver, comm, stream);
}

extern "C" int ocn_rk3_driver_configure(ocn_rk3_driver_t d, int32_t defer_correction)
{
    OCN_REQUIRE(d, "ocn_rk3_driver_configure: null driver");
    OCN_REQUIRE(!d->correction_pending, "ocn_rk3_driver_configure: flush first (a deferred pressure correction is pending)");
    OCN_REQUIRE(!defer_correction || d->correct_on_load, "ocn_rk3_driver_configure: deferring the correction needs correction on load (all-periodic grid)");
    d->defer_correction = defer_correction != 0;
    return OCN_SUCCESS;
}

extern "C" int ocn_rk3_driver_time_step(ocn_rk3_driver_t d, double dt, void *stream)
{
    OCN_REQUIRE(d, "ocn_rk3_driver_time_step: null driver");
    using namespace ocn::rk3;
    int st;
    if (!d->started) {  // iteration 0: update_state!(model) with the tendencies
        OCN_TRY(fill_velocities(d, 0, stream));
        OCN_TRY(ocn_compute_momentum_tendencies(&d->grid, d->U[0], d->U[1], d->U[2], d->Gn[0], d->Gn[1], d->Gn[2], nullptr, stream));
        d->started = true;
    }
    const StageDt stage = stage_dt(dt);
    // ---- first stage
    if (d->pending) {
        const bool pc = d->correction_pending;  // the previous step's third-stage correction rides on this launch's loads
        st = fused_launch(d, dt, g1, 0.0, 0, pc ? d->p : nullptr, pc ? d->correction_dt : 0.0,
                          pc && d->wrapped_loads ? OCN_RK3_WRAPPED_LOADS : 0, stream);
        d->correction_pending = false;
    } else {
        st = ocn_rk3_substep(&d->grid, 3, d->U, d->Gn, d->Gm, d->locs, dt, g1, 0.0, 0, stream);
    }
    if (st != OCN_SUCCESS) return st;
    OCN_TRY(project_and_advance(d, dt, stage.first, g2, z2, false, stream));  // ... ends with the second substep
    OCN_TRY(project_and_advance(d, dt, stage.second, g3, z3, true, stream));  // ... ends with the third substep (d->pending = true below)
    // ---- third stage: projection; its compute_tendencies! is fused into the next step's first substep, and so is -- when the
    //      correction is deferred -- pressure_correct_velocities! itself
    if (d->defer_correction) {
        OCN_TRY(project_for_load(d, stage.third, stream));
        d->correction_pending = true;
        d->correction_dt = stage.third;
    } else {
        OCN_TRY(project_and_correct(d, stage.third, true, stream));
    }
    d->pending = true;
    d->iteration += 1;
    return OCN_SUCCESS;
}

extern "C" int ocn_rk3_driver_flush(ocn_rk3_driver_t d, void *stream)
{
    OCN_REQUIRE(d, "ocn_rk3_driver_flush: null driver");
    if (d->correction_pending && d->pending && d->fused_flush) {
        // both in one pass: the launch corrects on load, stores the corrected velocities into the other set and G^n of them; then the p
        // halos a caller sees after the separate passes (fill_pressure) and the velocity halos
        OCN_TRY(ocn_compute_momentum_tendencies_rk3_flags(&d->grid, d->U[0], d->U[1], d->U[2], d->Gn[0], d->Gn[1], d->Gn[2], nullptr, nullptr,
                                                          nullptr, d->A[0], d->A[1], d->A[2], 0.0, 0.0, 0.0, 0, d->p, d->correction_dt,
                                                          OCN_RK3_CORRECT_ONLY | (d->wrapped_loads ? OCN_RK3_WRAPPED_LOADS : 0), stream));
        d->swap_sets();
        d->correction_pending = d->pending = false;
        OCN_TRY(fill_pressure(d, stream));
        OCN_TRY(fill_velocities(d, 0, stream));
    }
    if (d->correction_pending) {  // the deferred third-stage correction: p halos, pressure_correct_velocities!, velocity halos
        OCN_TRY(project_and_correct(d, d->correction_dt, false, stream));
        d->correction_pending = false;
    }
    if (d->pending) {  // complete the deferred compute_tendencies!: G^n of the current state
        OCN_TRY(ocn_compute_momentum_tendencies(&d->grid, d->U[0], d->U[1], d->U[2], d->Gn[0], d->Gn[1], d->Gn[2], nullptr, stream));
        d->pending = false;
    }
    return d->bring_home(stream);  // (an odd number of fused launches since the last flush)
}

extern "C" int ocn_rk3_driver_fields(ocn_rk3_driver_t d, double **u, double **v, double **w, double **Gu, double **Gv, double **Gw)
{
    OCN_REQUIRE(d, "ocn_rk3_driver_fields: null driver");
    if (u) *u = d->U[0];
    if (v) *v = d->U[1];
    if (w) *w = d->U[2];
    if (Gu) *Gu = d->Gn[0];
    if (Gv) *Gv = d->Gn[1];
    if (Gw) *Gw = d->Gn[2];
    return OCN_SUCCESS;
}
