// driver_core_check.cpp -- the host logic the two RK3 drivers share (csrc/ocn_driver_core.h) exercised on host pointers: no device.
//
// The HIP allocation / copy calls and the solver's create / destroy that the header reaches are defined HERE, over malloc / memcpy / free
// (a link seam: the header has none of its own), so the host sanitizers see every buffer the bookkeeping owns: a swap that loses a buffer
// leaks, a release that frees one twice or frees the caller's array is reported, a copy of the wrong size overruns.  Built with
//
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Ioceananigans.jl_amd/csrc \
//         tools/driver_core_check.cpp -o tools/bin/driver_core_check && tools/bin/driver_core_check
//
// Exit status 0 iff every check holds (and the sanitizers report nothing).
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ocn_driver_core.h"

static int failures = 0, live_solvers = 0, fail_malloc_after = -1;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            failures += 1;                                                 \
        }                                                                  \
    } while (0)

// ---- the seam
extern "C" hipError_t hipMalloc(void **p, size_t n)
{
    if (fail_malloc_after == 0) return hipErrorOutOfMemory;
    if (fail_malloc_after > 0) fail_malloc_after -= 1;
    *p = std::malloc(n);
    std::memset(*p, 0xff, n);  // (allocate must zero it itself)
    return hipSuccess;
}
extern "C" hipError_t hipMemset(void *p, int v, size_t n) { std::memset(p, v, n); return hipSuccess; }
extern "C" hipError_t hipFree(void *p) { std::free(p); return hipSuccess; }
extern "C" hipError_t hipMemcpyAsync(void *dst, const void *src, size_t n, hipMemcpyKind, hipStream_t) { std::memcpy(dst, src, n); return hipSuccess; }
extern "C" const char *hipGetErrorString(hipError_t) { return "stub"; }
extern "C" int ocn_poisson_create(ocn_poisson_t *s, const ocn_grid *)
{
    *s = (ocn_poisson_t)std::malloc(8);
    live_solvers += 1;
    return OCN_SUCCESS;
}
extern "C" int ocn_poisson_destroy(ocn_poisson_t s)
{
    std::free(s);
    live_solvers -= 1;
    return OCN_SUCCESS;
}
static char last_error[256];
void ocn::set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(last_error, sizeof last_error, fmt, ap);
    va_end(ap);
}

static ocn_grid small_grid(int tx)
{
    ocn_grid g{};
    g.Nx = 5; g.Ny = 4; g.Nz = 3;
    g.Hx = 3; g.Hy = 2; g.Hz = 1;
    g.tx = tx; g.ty = OCN_PERIODIC; g.tz = OCN_BOUNDED;
    g.dx = g.dy = g.dz = 1.0;
    return g;
}

template <int CAP>
static void check_sets(int n, int tx)
{
    const ocn_grid grid = small_grid(tx);
    ocn::FieldSets<CAP> s;
    s.n = n;
    CHECK(s.locs[0] == OCN_LOC_FCC && s.locs[1] == OCN_LOC_CFC && s.locs[2] == OCN_LOC_CCF);
    for (int f = 3; f < CAP; ++f) CHECK(s.locs[f] == OCN_LOC_CCC);
    size_t bytes[CAP];
    const ocn::GridDev g = ocn::to_dev(grid);
    for (int f = 0; f < n; ++f) {  // the caller's arrays: exactly the parent extents, so that a copy of another field's size overruns
        const ocn::Lay L = ocn::make_lay(g, s.locs[f]);
        bytes[f] = (size_t)L.sx * L.sy * L.sz * sizeof(double);
        s.user[f] = (double *)std::malloc(bytes[f]);
        for (size_t q = 0; q < bytes[f] / sizeof(double); ++q) s.user[f][q] = 100.0 * f + 1.0;
    }
    CHECK(s.allocate(grid, "check") == OCN_SUCCESS);
    double *own[CAP], *Gn[CAP], *Gm[CAP];
    for (int f = 0; f < n; ++f) {
        own[f] = s.own[f]; Gn[f] = s.Gn[f]; Gm[f] = s.Gm[f];
        CHECK(s.bytes[f] == bytes[f] && s.U[f] == s.user[f] && s.A[f] == s.own[f]);
        CHECK(own[f] && Gn[f] && Gm[f] && own[f][0] == 0.0 && Gn[f][bytes[f] / 8 - 1] == 0.0 && Gm[f][0] == 0.0);
    }
    for (int f = n; f < CAP; ++f) CHECK(!s.own[f] && !s.Gn[f] && !s.Gm[f] && !s.U[f] && !s.A[f]);
    CHECK(s.bring_home(nullptr) == OCN_SUCCESS);  // at home: nothing moves
    for (int f = 0; f < n; ++f) CHECK(s.U[f] == s.user[f] && s.user[f][0] == 100.0 * f + 1.0);
    // an odd number of fused launches: the fields are in the second set
    for (int launch = 0; launch < 3; ++launch) {
        for (int f = 0; f < n; ++f)
            for (size_t q = 0; q < bytes[f] / sizeof(double); ++q) s.A[f][q] = 100.0 * f + 10.0 + launch;
        s.swap_sets();
        s.swap_tendencies();
    }
    for (int f = 0; f < n; ++f) CHECK(s.U[f] == own[f] && s.A[f] == s.user[f] && s.Gn[f] == Gm[f] && s.Gm[f] == Gn[f]);
    CHECK(s.bring_home(nullptr) == OCN_SUCCESS);
    for (int f = 0; f < n; ++f) {
        CHECK(s.U[f] == s.user[f] && s.A[f] == own[f]);
        CHECK(s.user[f][0] == 100.0 * f + 12.0 && s.user[f][bytes[f] / 8 - 1] == 100.0 * f + 12.0);
    }
    CHECK(s.bring_home(nullptr) == OCN_SUCCESS);  // and a second call is a no-op
    for (int f = 0; f < n; ++f) CHECK(s.U[f] == s.user[f]);
    s.swap_sets();  // release with the roles swapped: the caller's arrays are not the driver's to free
    s.release();
    for (int f = 0; f < CAP; ++f) CHECK(!s.own[f] && !s.Gn[f] && !s.Gm[f]);
    s.release();  // (destroy after a failed create releases twice)
    for (int f = 0; f < n; ++f) std::free(s.user[f]);
}

static void check_failed_allocation()
{
    const ocn_grid grid = small_grid(OCN_PERIODIC);
    ocn::FieldSets<3> s;
    double u[1];
    s.user[0] = s.user[1] = s.user[2] = u;  // never touched by allocate / release
    fail_malloc_after = 4;                  // the fifth buffer fails: four are live, all released below
    CHECK(s.allocate(grid, "ocn_x_create") == OCN_ERR_ALLOC);
    CHECK(std::strncmp(last_error, "ocn_x_create: device allocation of ", 35) == 0);
    fail_malloc_after = -1;
    s.release();
}

static void check_projection()
{
    const ocn_grid grid = small_grid(OCN_PERIODIC);
    int some_solver = 0, some_dist = 0, some_comm = 0;
    {  // the driver's own solver
        ocn::Projection p;
        CHECK(p.adopt_solver(&grid, nullptr, nullptr, nullptr) == OCN_SUCCESS);
        CHECK(p.solver && p.owns_solver && !p.comm && !p.dsolver && live_solvers == 1);
        p.release_solver();
        CHECK(!p.solver && live_solvers == 0);
        p.release_solver();
        CHECK(live_solvers == 0);
    }
    {  // the caller's (borrowed)
        ocn::Projection p;
        CHECK(p.adopt_solver(&grid, (ocn_poisson_t)&some_solver, nullptr, nullptr) == OCN_SUCCESS);
        CHECK(p.solver == (ocn_poisson_t)&some_solver && !p.owns_solver && !p.comm && !p.dsolver && live_solvers == 0);
        p.release_solver();
        CHECK(live_solvers == 0);
    }
    {  // a slab-x rank: communicator + distributed handle, both borrowed; no solver of one GPU
        ocn::Projection p;
        CHECK(p.adopt_solver(&grid, nullptr, (ocn_dist_poisson_t)&some_dist, &some_comm) == OCN_SUCCESS);
        CHECK(!p.solver && !p.owns_solver && p.comm == &some_comm && p.dsolver == (ocn_dist_poisson_t)&some_dist && live_solvers == 0);
        p.release_solver();
        CHECK(live_solvers == 0);
    }
    {  // released before anything was adopted (a create that failed early)
        ocn::Projection p;
        p.release_solver();
        CHECK(live_solvers == 0);
    }
}

static void check_constants_and_refusal()
{
    using namespace ocn::rk3;
    const double dt = 0.37;
    const StageDt s = stage_dt(dt);
    CHECK(s.first == (8.0 / 15) * dt && s.second == (5.0 / 12 + -17.0 / 60) * dt && s.third == (3.0 / 4 + -5.0 / 12) * dt);
    ocn_grid g = small_grid(OCN_PERIODIC);
    CHECK(ocn::require_unpartitioned_x(&g, "ocn_x_driver") == OCN_SUCCESS);
    g.tx = OCN_FULLY_CONNECTED;
    CHECK(ocn::require_unpartitioned_x(&g, "ocn_x_driver") == OCN_ERR_INVALID_ARGUMENT);
    char want[256];
    std::snprintf(want, sizeof want, "ocn_x_driver_create: a partitioned x (topology %d) needs ocn_x_driver_create_distributed", OCN_FULLY_CONNECTED);
    CHECK(std::strcmp(last_error, want) == 0);
}

int main()
{
    check_sets<3>(3, OCN_PERIODIC);
    check_sets<3>(3, OCN_BOUNDED);  // (the Face-located u has one more plane: sizes differ between fields)
    check_sets<3 + OCN_MODEL_MAX_TRACERS>(3, OCN_PERIODIC);
    check_sets<3 + OCN_MODEL_MAX_TRACERS>(5, OCN_BOUNDED);
    check_sets<3 + OCN_MODEL_MAX_TRACERS>(3 + OCN_MODEL_MAX_TRACERS, OCN_PERIODIC);
    check_failed_allocation();
    check_projection();
    check_constants_and_refusal();
    std::printf(failures ? "driver_core_check: %d checks FAILED\n" : "driver_core_check: ok\n", failures);
    return failures ? 1 : 0;
}
