// ocn_driver_core.h -- what the two RK3 drivers (driver.hip: the benchmark's box; model_driver.hip: tracers and the SURVEY §8(f) terms)
// literally share: the two sets of arrays whose roles alternate, the handles of the pressure projection, the halo fill of a tuple and the
// RK3 constants.  Host code only: no kernel, every device operation is a public entry point.  What differs between the drivers -- their
// launch sequences (time_step, the project* families), their distributed-create checks and their texts -- stays in each.
#pragma once
#include <utility>

#include "ocn_internal.h"

namespace ocn {

// γ, ζ each rounded once to Float64 (runge_kutta_3.jl:53-62) and the Δt of the three stages' projections
namespace rk3 {
constexpr double g1 = 8.0 / 15, g2 = 5.0 / 12, g3 = 3.0 / 4, z2 = -17.0 / 60, z3 = -5.0 / 12;
struct StageDt {
    double first, second, third;
};
inline StageDt stage_dt(double dt) { return {g1 * dt, (g2 + z2) * dt, (g3 + z3) * dt}; }
}  // namespace rk3

// The prognostic fields of a driver (u, v, w, then tracers) in two sets: the caller's arrays and a second set the driver owns.  A fused
// launch reads U and writes A, then the two trade places; G^n / G^- swap instead of being copied.
template <int CAP>
struct FieldSets {
    int n = 3;  // fields in use
    int32_t locs[CAP];
    double *user[CAP] = {}, *own[CAP] = {};  // the caller's parents; the second set
    double *U[CAP] = {}, *A[CAP] = {};       // where the fields are now; where the next fused launch writes
    double *Gn[CAP] = {}, *Gm[CAP] = {};
    size_t bytes[CAP] = {};

    FieldSets()
    {
        const int32_t velocity[3] = {OCN_LOC_FCC, OCN_LOC_CFC, OCN_LOC_CCF};
        for (int f = 0; f < CAP; ++f) locs[f] = f < 3 ? velocity[f] : OCN_LOC_CCC;
    }
    // the second set and both tendency sets of the n fields in `user`, zeroed; on failure the caller releases what was allocated
    int allocate(const ocn_grid &grid, const char *who)
    {
        const GridDev g = to_dev(grid);
        for (int f = 0; f < n; ++f) {
            const Lay L = make_lay(g, locs[f]);
            bytes[f] = (size_t)L.sx * L.sy * L.sz * sizeof(double);
            for (double **buf : {&own[f], &Gn[f], &Gm[f]}) {
                if (hipMalloc((void **)buf, bytes[f]) != hipSuccess || hipMemset(*buf, 0, bytes[f]) != hipSuccess) {
                    set_error("%s: device allocation of %zu bytes failed", who, bytes[f]);
                    return OCN_ERR_ALLOC;
                }
            }
            U[f] = user[f];
            A[f] = own[f];
        }
        return OCN_SUCCESS;
    }
    void release()
    {
        for (int f = 0; f < CAP; ++f) {
            for (double **buf : {&own[f], &Gn[f], &Gm[f]}) {
                if (*buf) (void)hipFree(*buf);
                *buf = nullptr;
            }
        }
    }
    void swap_sets()
    {
        for (int f = 0; f < n; ++f) std::swap(U[f], A[f]);
    }
    void swap_tendencies()  // cache_previous_tendencies! (store_tendencies.jl:12-22) as a role swap
    {
        for (int f = 0; f < n; ++f) std::swap(Gn[f], Gm[f]);
    }
    // after an odd number of fused launches the fields are in the second set: copy them into the caller's arrays and swap back
    int bring_home(void *stream)
    {
        if (U[0] == user[0]) return OCN_SUCCESS;
        for (int f = 0; f < n; ++f) {
            OCN_CHECK_HIP(hipMemcpyAsync(user[f], U[f], bytes[f], hipMemcpyDeviceToDevice, as_stream(stream)));
            std::swap(U[f], A[f]);
        }
        return OCN_SUCCESS;
    }
};

// The handles of the pressure projection: one GPU's solver (the caller's or the driver's own), or on a slab-x rank the RCCL communicator and
// the distributed Poisson handle (both borrowed).
struct Projection {
    ocn_poisson_t solver = nullptr;
    bool owns_solver = true;
    ocn_comm_t comm = nullptr;
    ocn_dist_poisson_t dsolver = nullptr;

    int adopt_solver(const ocn_grid *grid, ocn_poisson_t borrowed, ocn_dist_poisson_t dist, ocn_comm_t c)
    {
        comm = c;
        dsolver = dist;
        solver = c ? nullptr : borrowed;
        owns_solver = !c && !borrowed;
        return owns_solver ? ocn_poisson_create(&solver, grid) : OCN_SUCCESS;
    }
    void release_solver()
    {
        if (solver && owns_solver) ocn_poisson_destroy(solver);
        solver = nullptr;
    }
    // solve_for_pressure!(pNHS, solver, Δt, U) (solve_for_pressure.jl:78-82) on one GPU or on a slab (the slab pipelines of the handle:
    // distributed_fft_based_poisson_solver.jl:141-178 without pack / unpack passes)
    int solve(double *p, double *const *U, double stage_dt, void *stream) const
    {
        if (!dsolver) return ocn_solve_for_pressure(solver, p, U[0], U[1], U[2], stage_dt, stream);
        OCN_TRY(ocn_dist_poisson_source_term(dsolver, U[0], U[1], U[2], stage_dt, stream));
        OCN_TRY(ocn_dist_poisson_forward_yz(dsolver, stream));
        OCN_TRY(ocn_dist_poisson_exchange(dsolver, comm, 0, stream));
        OCN_TRY(ocn_dist_poisson_solve_x(dsolver, stream));
        OCN_TRY(ocn_dist_poisson_exchange(dsolver, comm, 1, stream));
        return ocn_dist_poisson_backward_yz(dsolver, p, stream);
    }
};

// fill_halo_regions!(fields) without the neighbours: one launch for the tuple, the fields' own Value / Gradient conditions included (bcs
// NULL, or NULL for every field: the defaults)
inline int fill_local(const ocn_grid *grid, double *const *fields, const int32_t *locs, const ocn_field_bcs *const *bcs, int n, int fbnv,
                      void *stream)
{
    bool any = false;
    for (int f = 0; f < n && bcs; ++f) any = any || bcs[f];
    return any ? ocn_fill_halo_regions_bcs(grid, fields, locs, bcs, n, fbnv, stream) : ocn_fill_halo_regions(grid, fields, locs, n, fbnv, stream);
}
// ... and on a slab (comm != NULL) the x exchange with the neighbours last (fill_halo_regions.jl:148-196); synchronous
inline int fill_and_exchange(const ocn_grid *grid, ocn_comm_t comm, double *const *fields, const int32_t *locs, const ocn_field_bcs *const *bcs,
                             int n, int fbnv, void *stream)
{
    const int st = fill_local(grid, fields, locs, bcs, n, fbnv, stream);
    if (st != OCN_SUCCESS || !comm) return st;
    OCN_TRY(ocn_halo_exchange_begin(comm, grid, fields, locs, n, stream));
    return ocn_halo_exchange_end(comm, grid, fields, locs, n, stream);
}

// the one-GPU constructor of `driver` (its entry-point prefix) takes no slab of a partitioned x
inline int require_unpartitioned_x(const ocn_grid *grid, const char *driver)
{
    OCN_REQUIRE(grid->tx == OCN_PERIODIC || grid->tx == OCN_BOUNDED || grid->tx == OCN_FLAT,
                "%s_create: a partitioned x (topology %d) needs %s_create_distributed", driver, grid->tx, driver);
    return OCN_SUCCESS;
}

}  // namespace ocn
