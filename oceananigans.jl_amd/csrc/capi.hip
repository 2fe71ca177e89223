// capi.hip -- extern "C" entry points of libocn_hip.so (see include/ocn_hip.h for the contract).
#include <atomic>
#include <cmath>
#include <cstring>
#include <string>

#include "ocn_buoyancy.h"
#include "ocn_internal.h"

namespace ocn {

static thread_local std::string g_last_error;
// process default of the arithmetic variant; a grid that carries its own (ocn_grid.math != OCN_GRID_MATH_DEFAULT) overrides it, so two
// models in one process may differ and a host thread changing the default does not touch another handle's launches
static std::atomic<int> g_math_mode{OCN_MATH_STRICT};
static inline bool strict_math(const ocn_grid *grid)
{
    const int m = grid ? grid->math : OCN_GRID_MATH_DEFAULT;
    if (m == OCN_GRID_MATH_STRICT) return true;
    if (m == OCN_GRID_MATH_FAST) return false;
    return g_math_mode.load(std::memory_order_relaxed) == OCN_MATH_STRICT;
}

// THE place that picks the variant of a launcher.  OCN_LAUNCH(grid, launcher, args...): the arithmetic variant by the grid's math mode
// (the launchers of ocn_launchers_math.inc and, for WENO, of ocn_launchers_scheme.inc).  OCN_LAUNCH_SCHEME(grid, advection, launcher,
// args...): the launchers of ocn_launchers_scheme.inc, whose UpwindBiased(order=5) builds live in the _up namespaces.
#define OCN_LAUNCH(grid, f, ...) (strict_math(grid) ? ocn_strict::f(__VA_ARGS__) : ocn_fast::f(__VA_ARGS__))
#define OCN_LAUNCH_SCHEME(grid, advection, f, ...)                                  \
    ((advection) != OCN_ADVECTION_UPWIND5 ? OCN_LAUNCH(grid, f, __VA_ARGS__)        \
     : strict_math(grid)                 ? ocn_strict_up::f(__VA_ARGS__)            \
                                          : ocn_fast_up::f(__VA_ARGS__))

void set_error(const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
}

// any_xy: the entry point has a direction-generic path (csrc/general.hip, fill_halos_general_kernel, the per-location layouts of the
// steppers and pressure kernels) and accepts Bounded / Flat x and y; the others keep the Periodic (or partitioned) x, Periodic y
// their kernels are written for
static int validate_grid_impl(const ocn_grid *g, bool any_xy)
{
    OCN_REQUIRE(g != nullptr, "grid is NULL");
    OCN_REQUIRE(g->Nx >= 1 && g->Ny >= 1 && g->Nz >= 1, "grid size must be positive, got (%d, %d, %d)", g->Nx, g->Ny, g->Nz);
    OCN_REQUIRE(g->Hx >= 0 && g->Hy >= 0 && g->Hz >= 0, "negative halo");
    const int t[3] = {g->tx, g->ty, g->tz};
    const int N[3] = {g->Nx, g->Ny, g->Nz};
    const int H[3] = {g->Hx, g->Hy, g->Hz};
    for (int d = 0; d < 3; ++d) {
        OCN_REQUIRE(t[d] >= OCN_PERIODIC && t[d] <= (d == 0 ? OCN_LEFT_CONNECTED : OCN_FULLY_CONNECTED), "unknown topology code %d", t[d]);
        if (t[d] == OCN_FLAT) OCN_REQUIRE(N[d] == 1 && H[d] == 0, "Flat dimension %d must have N = 1, H = 0", d);
        // halo must not exceed the interior (Grids/input_validation.jl: halo <= size)
        if (t[d] != OCN_FLAT) OCN_REQUIRE(H[d] <= N[d], "halo %d larger than size %d in dimension %d", H[d], N[d], d);
    }
    if (!any_xy && (!(g->tx == OCN_PERIODIC || g->tx == OCN_FULLY_CONNECTED) || g->ty != OCN_PERIODIC)) {
        set_error("unsupported topology (%d, %d, %d): x must be Periodic (or FullyConnected), y Periodic", g->tx, g->ty, g->tz);
        return OCN_ERR_UNSUPPORTED;
    }
    if (g->ty == OCN_FULLY_CONNECTED) {
        set_error("only x is ever partitioned (slab decomposition)");
        return OCN_ERR_UNSUPPORTED;
    }
    // a slab of a (Periodic, Bounded, *) grid: the direction-generic kernels read the exchanged x halos like periodic images and treat
    // the y walls locally (distributed_grids.jl:75-118)
    const bool part_x = g->tx == OCN_FULLY_CONNECTED || g->tx == OCN_RIGHT_CONNECTED || g->tx == OCN_LEFT_CONNECTED;
    if (any_xy && g->ty == OCN_FLAT && part_x) {
        set_error("a partitioned x needs a Periodic or Bounded y");
        return OCN_ERR_UNSUPPORTED;
    }
    // the first / last slab of a Bounded x (RightConnected / LeftConnected): the interior must reach past the wall stencils
    if (g->tx == OCN_RIGHT_CONNECTED || g->tx == OCN_LEFT_CONNECTED)
        OCN_REQUIRE(g->Nx >= 2, "a half-Bounded slab needs Nx >= 2 (got %d)", g->Nx);
    if (g->tz == OCN_FULLY_CONNECTED) {
        set_error("z is never partitioned (distributed_architectures.jl:223-225)");
        return OCN_ERR_UNSUPPORTED;
    }
    OCN_REQUIRE((g->dzc == nullptr) == (g->dzf == nullptr), "dzc and dzf must both be set or both be NULL");
    OCN_REQUIRE(g->dx > 0 && g->dy > 0 && (g->dzc || g->dz > 0), "spacings must be positive");
    return OCN_SUCCESS;
}
int validate_grid(const ocn_grid *g) { return validate_grid_impl(g, false); }
int validate_grid_any(const ocn_grid *g) { return validate_grid_impl(g, true); }
// x and y Periodic (x possibly partitioned): the tiled / shared-layout kernels apply; otherwise the direction-generic ones
// west / east conditions on a slab of a partitioned x: the slab that holds the wall takes them, the others drop them (the host checks the
// GLOBAL topology: a slab between the walls cannot tell a Bounded from a Periodic x)
static bool partitioned_x(const ocn_grid *g) { return g->tx == OCN_FULLY_CONNECTED || g->tx == OCN_RIGHT_CONNECTED || g->tx == OCN_LEFT_CONNECTED; }
static bool side_has_wall(const ocn_grid *g, int q)
{
    if (q == 0) return x_wall_west(*g);
    if (q == 1) return x_wall_east(*g);
    return (q < 4 ? g->ty : g->tz) == OCN_BOUNDED;
}
static bool xy_periodic(const ocn_grid *g) { return (g->tx == OCN_PERIODIC || g->tx == OCN_FULLY_CONNECTED) && g->ty == OCN_PERIODIC; }

// WENO5 reads 3 halo cells (nonhydrostatic_model.jl:183, 243-257 inflates the halo to >= 3)
static int validate_weno(const ocn_grid *g)
{
    OCN_TRY(validate_grid_any(g));
    OCN_REQUIRE((g->tx == OCN_FLAT || g->Hx >= 3) && (g->ty == OCN_FLAT || g->Hy >= 3) && (g->tz == OCN_FLAT || g->Hz >= 3),
                "WENO(order=5) needs halo >= 3, got (%d, %d, %d)", g->Hx, g->Hy, g->Hz);
    OCN_REQUIRE((g->tx == OCN_FLAT || g->Nx >= 3) && (g->ty == OCN_FLAT || g->Ny >= 3) && (g->tz == OCN_FLAT || g->Nz >= 3),
                "grid too small for WENO(order=5): adapt_advection_order would lower the order (adapt_advection_order.jl:101-108)");
    return OCN_SUCCESS;
}

}  // namespace ocn

using namespace ocn;

extern "C" {

const char *ocn_last_error(void) { return g_last_error.c_str(); }
const char *ocn_version(void) { return "libocn_hip 0.1 (gfx950)"; }

int ocn_device_count(int *count)
{
    OCN_REQUIRE(count, "count is NULL");
    OCN_CHECK_HIP(hipGetDeviceCount(count));
    return OCN_SUCCESS;
}
int ocn_set_device(int device)
{
    OCN_CHECK_HIP(hipSetDevice(device));
    return OCN_SUCCESS;
}
int ocn_malloc(void **ptr, size_t bytes)
{
    OCN_REQUIRE(ptr, "ptr is NULL");
    *ptr = nullptr;
    if (bytes == 0) return OCN_SUCCESS;
    hipError_t e = hipMalloc(ptr, bytes);
    if (e != hipSuccess) {
        set_error("hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
        return OCN_ERR_ALLOC;
    }
    OCN_CHECK_HIP(hipMemset(*ptr, 0, bytes));
    return OCN_SUCCESS;
}
int ocn_free(void *ptr)
{
    if (ptr) OCN_CHECK_HIP(hipFree(ptr));
    return OCN_SUCCESS;
}
int ocn_memcpy_h2d(void *dst, const void *src, size_t bytes, void *stream)
{
    OCN_CHECK_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, as_stream(stream)));
    OCN_CHECK_HIP(hipStreamSynchronize(as_stream(stream)));
    return OCN_SUCCESS;
}
int ocn_memcpy_d2h(void *dst, const void *src, size_t bytes, void *stream)
{
    OCN_CHECK_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, as_stream(stream)));
    OCN_CHECK_HIP(hipStreamSynchronize(as_stream(stream)));
    return OCN_SUCCESS;
}
int ocn_memcpy_d2d(void *dst, const void *src, size_t bytes, void *stream)
{
    OCN_CHECK_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, as_stream(stream)));
    return OCN_SUCCESS;
}
int ocn_memset(void *ptr, int value, size_t bytes, void *stream)
{
    OCN_CHECK_HIP(hipMemsetAsync(ptr, value, bytes, as_stream(stream)));
    return OCN_SUCCESS;
}
int ocn_sync(void *stream)
{
    OCN_CHECK_HIP(hipStreamSynchronize(as_stream(stream)));
    return OCN_SUCCESS;
}

int ocn_sync_timeout(void *stream, double seconds)
{
    return ocn::wait_stream(as_stream(stream), seconds, "ocn_sync_timeout");
}

int ocn_profile_marker(void *stream) { return ocn::launch_profile_marker(as_stream(stream)); }

int ocn_set_math_mode(int mode)
{
    OCN_REQUIRE(mode == OCN_MATH_STRICT || mode == OCN_MATH_FAST, "unknown math mode %d", mode);
    g_math_mode = mode;
    return OCN_SUCCESS;
}
int ocn_get_math_mode(void) { return g_math_mode; }

static int make_field_tuple(const ocn_grid *grid, double *const *fields, const int32_t *locs, int32_t n, FieldTuple &ft)
{
    OCN_REQUIRE(fields && locs, "fields/locs is NULL");
    OCN_REQUIRE(n >= 1 && n <= MAX_TUPLE, "number of fields %d outside 1..%d", n, MAX_TUPLE);
    ft.n = n;
    for (int f = 0; f < n; ++f) {
        OCN_REQUIRE(fields[f] != nullptr, "field %d is NULL", f);
        OCN_REQUIRE(locs[f] == OCN_LOC_CCC || locs[f] == OCN_LOC_FCC || locs[f] == OCN_LOC_CFC || locs[f] == OCN_LOC_CCF,
                    "field %d has unsupported location mask %d", f, locs[f]);
        ft.f[f] = fields[f];
        ft.loc[f] = locs[f];
    }
    (void)grid;
    return OCN_SUCCESS;
}

int ocn_fill_halo_regions(const ocn_grid *grid, double *const *fields, const int32_t *locs, int32_t n,
                          int32_t fill_boundary_normal_velocities, void *stream)
{
    OCN_TRY(validate_grid_any(grid));
    FieldTuple ft;
    OCN_TRY(make_field_tuple(grid, fields, locs, n, ft));
    if (!xy_periodic(grid)) return launch_fill_halos_general(grid, ft, fill_boundary_normal_velocities, as_stream(stream));
    return launch_fill_halos(grid, ft, fill_boundary_normal_velocities, -1, as_stream(stream));
}

int ocn_fill_halo_periodic(const ocn_grid *grid, double *const *fields, const int32_t *locs, int32_t n, int32_t dir, void *stream)
{
    OCN_TRY(validate_grid(grid));
    OCN_REQUIRE(dir >= 0 && dir <= 2, "dir must be 0, 1 or 2");
    const int t = dir == 0 ? grid->tx : dir == 1 ? grid->ty : grid->tz;
    OCN_REQUIRE(t == OCN_PERIODIC, "direction %d is not Periodic", dir);
    FieldTuple ft;
    OCN_TRY(make_field_tuple(grid, fields, locs, n, ft));
    return launch_fill_halos(grid, ft, 0, dir, as_stream(stream));
}

int ocn_compute_momentum_tendencies(const ocn_grid *grid, const double *u, const double *v, const double *w, double *Gu,
                                    double *Gv, double *Gw, const int32_t *range, void *stream)
{
    OCN_TRY(validate_weno(grid));
    OCN_REQUIRE(u && v && w && Gu && Gv && Gw, "ocn_compute_momentum_tendencies: null field pointer");
    if (!xy_periodic(grid)) return OCN_LAUNCH(grid, launch_momentum_tendencies_general, grid, 0, u, v, w, Gu, Gv, Gw, range, as_stream(stream));
    return OCN_LAUNCH(grid, launch_momentum_tendencies, grid, u, v, w, Gu, Gv, Gw, range, nullptr, as_stream(stream));
}

// the next substep as the epilogue of the tiled momentum kernel
static FuseArgs substep_fuse(const double *Gmu, const double *Gmv, const double *Gmw, double *u_out, double *v_out, double *w_out, double dt,
                             double gamma, double zeta, int32_t has_zeta)
{
    FuseArgs fz{};
    fz.Gm[0] = Gmu; fz.Gm[1] = Gmv; fz.Gm[2] = Gmw;
    fz.Uo[0] = u_out; fz.Uo[1] = v_out; fz.Uo[2] = w_out;
    fz.dt = dt; fz.gamma = gamma; fz.zeta = zeta; fz.on = 1; fz.has_zeta = has_zeta ? 1 : 0;
    return fz;
}

static int momentum_tendencies_rk3(const ocn_grid *grid, const double *u, const double *v, const double *w, double *Gu, double *Gv,
                                   double *Gw, const double *Gmu, const double *Gmv, const double *Gmw, double *u_out, double *v_out,
                                   double *w_out, double dt, double gamma, double zeta, int32_t has_zeta, const double *p_correct,
                                   double dt_correct, const int32_t *range, int32_t flags, void *stream)
{
    OCN_TRY(validate_weno(grid));
    OCN_REQUIRE(u && v && w && Gu && Gv && Gw && u_out && v_out && w_out, "ocn_compute_momentum_tendencies_rk3: null field pointer");
    OCN_REQUIRE(!has_zeta || (Gmu && Gmv && Gmw), "ocn_compute_momentum_tendencies_rk3: G⁻ pointers are required when has_zeta != 0");
    OCN_REQUIRE(u_out != u && v_out != v && w_out != w, "ocn_compute_momentum_tendencies_rk3: outputs must not alias the inputs");
    if (!xy_periodic(grid)) {
        // walls in x / y: the substep as the epilogue of the tiled kernel on the interior box, as one more per-cell kernel on the wall frames
        // (wall faces carried over); no correction on load (its wrapped indices are the Periodic grids')
        OCN_REQUIRE(!p_correct, "ocn_compute_momentum_tendencies_rk3: the pressure correction on load needs Periodic x and y");
        OCN_REQUIRE(!range, "ocn_compute_momentum_tendencies_rk3: ranges need Periodic x and y");
        MomentumFinal mf{};
        mf.sub[0] = SubstepDev{Gmu, u_out};
        mf.sub[1] = SubstepDev{Gmv, v_out};
        mf.sub[2] = SubstepDev{Gmw, w_out};
        mf.sc = SubstepCoef{dt, gamma, zeta, 1, has_zeta ? 1 : 0};
        return OCN_LAUNCH(grid, launch_momentum_tendencies_general, grid, 0, u, v, w, Gu, Gv, Gw, nullptr, as_stream(stream), &mf);
    }
    FuseArgs fz = substep_fuse(Gmu, Gmv, Gmw, u_out, v_out, w_out, dt, gamma, zeta, has_zeta);
    fz.pc_p = p_correct; fz.pc_dt = dt_correct; fz.pc_on = p_correct ? 1 : 0;
    fz.skip_g = (flags & OCN_RK3_SKIP_G_STORE) ? 1 : 0;
    fz.wrap_uvw = (flags & OCN_RK3_WRAPPED_LOADS) ? 1 : 0;
    fz.no_step = (flags & OCN_RK3_CORRECT_ONLY) ? 1 : 0;
    return OCN_LAUNCH(grid, launch_momentum_tendencies, grid, u, v, w, Gu, Gv, Gw, range, &fz, as_stream(stream));
}

int ocn_compute_momentum_tendencies_rk3(const ocn_grid *grid, const double *u, const double *v, const double *w, double *Gu,
                                        double *Gv, double *Gw, const double *Gmu, const double *Gmv, const double *Gmw,
                                        double *u_out, double *v_out, double *w_out, double dt, double gamma, double zeta,
                                        int32_t has_zeta, const double *p_correct, double dt_correct, const int32_t *range,
                                        void *stream)
{
    return momentum_tendencies_rk3(grid, u, v, w, Gu, Gv, Gw, Gmu, Gmv, Gmw, u_out, v_out, w_out, dt, gamma, zeta, has_zeta, p_correct,
                                   dt_correct, range, 0, stream);
}

int ocn_compute_momentum_tendencies_rk3_flags(const ocn_grid *grid, const double *u, const double *v, const double *w, double *Gu,
                                              double *Gv, double *Gw, const double *Gmu, const double *Gmv, const double *Gmw,
                                              double *u_out, double *v_out, double *w_out, double dt, double gamma, double zeta,
                                              int32_t has_zeta, const double *p_correct, double dt_correct, int32_t flags, void *stream)
{
    OCN_REQUIRE(!(flags & ~(OCN_RK3_SKIP_G_STORE | OCN_RK3_WRAPPED_LOADS | OCN_RK3_CORRECT_ONLY)),
                "ocn_compute_momentum_tendencies_rk3_flags: unknown flag in %d", flags);
    OCN_REQUIRE(p_correct, "ocn_compute_momentum_tendencies_rk3_flags: the flags belong to the correction-on-load launch (p_correct)");
    return momentum_tendencies_rk3(grid, u, v, w, Gu, Gv, Gw, Gmu, Gmv, Gmw, u_out, v_out, w_out, dt, gamma, zeta, has_zeta, p_correct,
                                   dt_correct, nullptr, flags, stream);
}

int ocn_compute_momentum_tendencies_rk3_strips(const ocn_grid *grid, const double *u, const double *v, const double *w, double *Gu,
                                               double *Gv, double *Gw, const double *Gmu, const double *Gmv, const double *Gmw,
                                               double *u_out, double *v_out, double *w_out, double dt, double gamma, double zeta,
                                               int32_t has_zeta, const double *p_correct, double dt_correct, double *strip_west,
                                               double *strip_east, int64_t field_doubles, void *stream)
{
    OCN_TRY(validate_weno(grid));
    OCN_REQUIRE(u && v && w && Gu && Gv && Gw && u_out && v_out && w_out, "ocn_compute_momentum_tendencies_rk3_strips: null field pointer");
    OCN_REQUIRE(!has_zeta || (Gmu && Gmv && Gmw), "ocn_compute_momentum_tendencies_rk3_strips: G⁻ pointers are required when has_zeta != 0");
    OCN_REQUIRE(u_out != u && v_out != v && w_out != w, "ocn_compute_momentum_tendencies_rk3_strips: outputs must not alias the inputs");
    OCN_REQUIRE(p_correct && strip_west && strip_east && field_doubles > 0,
                "ocn_compute_momentum_tendencies_rk3_strips: the correction-on-load stage of a slab (p_correct) and both strip buffers");
    OCN_REQUIRE(grid->tx == OCN_FULLY_CONNECTED && grid->ty == OCN_PERIODIC && grid->tz == OCN_PERIODIC,
                "ocn_compute_momentum_tendencies_rk3_strips: a (FullyConnected, Periodic, Periodic) local grid");
    FuseArgs fz = substep_fuse(Gmu, Gmv, Gmw, u_out, v_out, w_out, dt, gamma, zeta, has_zeta);
    fz.pc_p = p_correct; fz.pc_dt = dt_correct; fz.pc_on = 1;
    fz.strip_w = strip_west; fz.strip_e = strip_east; fz.strip_field = field_doubles;
    return OCN_LAUNCH(grid, launch_momentum_tendencies, grid, u, v, w, Gu, Gv, Gw, nullptr, &fz, as_stream(stream));
}

int ocn_momentum_tendencies_addr32(const ocn_grid *grid, int32_t *selected)
{
    OCN_REQUIRE(grid && selected, "ocn_momentum_tendencies_addr32: null argument");
    *selected = (tendency_addr32_enabled() && tendency_addr32_fits(*grid)) ? 1 : 0;
    return OCN_SUCCESS;
}

// the FuseArgs that the entry point in question builds, as far as the decision reads them (no pointer is dereferenced), through the
// launcher's own plan function
int ocn_momentum_tendencies_plan(const ocn_grid *grid, const int32_t *range, int32_t correct_on_load, int32_t flags, int32_t strips,
                                 int32_t *plan)
{
    OCN_TRY(validate_weno(grid));
    OCN_REQUIRE(plan, "ocn_momentum_tendencies_plan: plan is NULL");
    OCN_REQUIRE(xy_periodic(grid), "ocn_momentum_tendencies_plan: grids Periodic (or partitioned) in x and Periodic in y");
    OCN_REQUIRE(!(flags & ~(OCN_RK3_SKIP_G_STORE | OCN_RK3_WRAPPED_LOADS | OCN_RK3_CORRECT_ONLY)),
                "ocn_momentum_tendencies_plan: unknown flag in %d", flags);
    OCN_REQUIRE(correct_on_load || (!flags && !strips), "ocn_momentum_tendencies_plan: flags and strips belong to the correction-on-load launch");
    OCN_REQUIRE(!strips || !flags, "ocn_momentum_tendencies_plan: the strip-writing launch takes no flags");
    OCN_REQUIRE(!strips || (grid->tx == OCN_FULLY_CONNECTED && grid->ty == OCN_PERIODIC && grid->tz == OCN_PERIODIC),
                "ocn_momentum_tendencies_plan: strips need a (FullyConnected, Periodic, Periodic) local grid");
    if (!correct_on_load) return ocn_strict::plan_momentum_tendencies_query(grid, range, nullptr, plan);
    static double nowhere;  // (stands for p_correct and the strip buffers: the decision only asks whether they are there)
    FuseArgs fz = substep_fuse(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0.0, 0.0, 0.0, 0);
    fz.pc_p = &nowhere; fz.pc_on = 1;
    fz.skip_g = (flags & OCN_RK3_SKIP_G_STORE) ? 1 : 0;
    fz.wrap_uvw = (flags & OCN_RK3_WRAPPED_LOADS) ? 1 : 0;
    fz.no_step = (flags & OCN_RK3_CORRECT_ONLY) ? 1 : 0;
    if (strips) { fz.strip_w = fz.strip_e = &nowhere; fz.strip_field = 1; }
    return ocn_strict::plan_momentum_tendencies_query(grid, range, &fz, plan);
}

int ocn_cell_advection_timescale(const ocn_grid *grid, const double *u, const double *v, const double *w, double *result_device,
                                 void *stream)
{
    OCN_TRY(validate_grid_any(grid));
    OCN_REQUIRE(u && v && w && result_device, "ocn_cell_advection_timescale: null pointer");
    return launch_advection_timescale(grid, u, v, w, result_device, as_stream(stream));
}

int ocn_hasnan(const double *field, int64_t n_elements, int32_t *flag_device, void *stream)
{
    OCN_REQUIRE(field && flag_device, "ocn_hasnan: null pointer");
    OCN_REQUIRE(n_elements >= 0, "ocn_hasnan: negative element count");
    OCN_REQUIRE((reinterpret_cast<uintptr_t>(field) & 15) == 0, "ocn_hasnan: field must be 16-byte aligned");
    return launch_hasnan(field, n_elements, flag_device, as_stream(stream));
}

// ---- SURVEY §8(f) rank 1 ------------------------------------------------------------------------------
static int validate_terms(const ocn_grid *grid, const ocn_model_terms *t)
{
    OCN_REQUIRE(t != nullptr, "terms is NULL");
    OCN_REQUIRE(t->advection >= OCN_ADVECTION_WENO5 && t->advection <= OCN_ADVECTION_UPWIND5, "unknown advection scheme %d", t->advection);
    OCN_REQUIRE(t->coriolis >= 0 && t->coriolis <= 2, "unknown coriolis code %d", t->coriolis);
    OCN_REQUIRE(t->coriolis != 2 || (t->yc && t->yf && grid->ty != OCN_FLAT), "BetaPlane needs the y node vectors yc, yf (and a non-Flat y)");
    OCN_REQUIRE(t->closure >= 0 && t->closure <= 2, "unknown closure code %d", t->closure);
    OCN_REQUIRE((t->closure == 2) == (t->nu_e != nullptr), "nu_e must be given exactly when closure == 2 (AnisotropicMinimumDissipation)");
    OCN_REQUIRE(t->closure != 2 || grid->tz != OCN_FLAT, "AnisotropicMinimumDissipation needs a non-Flat z");
    OCN_REQUIRE(t->buoyancy >= OCN_BUOYANCY_NONE && t->buoyancy <= OCN_BUOYANCY_SEAWATER_S, "unknown buoyancy code %d", t->buoyancy);
    if (buoyancy_reads_T(t->buoyancy)) OCN_REQUIRE(t->T != nullptr, "buoyancy formulation %d needs the T (or b) tracer", t->buoyancy);
    if (buoyancy_reads_S(t->buoyancy)) OCN_REQUIRE(t->S != nullptr, "buoyancy formulation %d needs the S tracer", t->buoyancy);
    OCN_REQUIRE(!t->pHY || t->buoyancy != OCN_BUOYANCY_NONE, "a hydrostatic pressure anomaly exists only with buoyancy (nonhydrostatic_model.jl:143-158)");
    if (t->advection != OCN_ADVECTION_CENTERED2) return validate_weno(grid);  // UpwindBiased(order=5): same halo / size needs
    OCN_TRY(validate_grid_any(grid));
    OCN_REQUIRE((grid->tx == OCN_FLAT || grid->Hx >= 1) && (grid->ty == OCN_FLAT || grid->Hy >= 1) && (grid->tz == OCN_FLAT || grid->Hz >= 1),
                "Centered(order=2) and the closure stencils need halo >= 1");
    return OCN_SUCCESS;
}

// advective part: the topology picks the launcher (direction-generic / Centered(order=2) / tiled), OCN_LAUNCH* its variant
static int launch_advective_momentum(int advection, const ocn_grid *grid, const double *u, const double *v, const double *w, double *Gu,
                                     double *Gv, double *Gw, const int32_t *range, hipStream_t s)
{
    const int c2 = advection == OCN_ADVECTION_CENTERED2;
    if (!xy_periodic(grid))  // direction-generic kernels (csrc/general.hip)
        return OCN_LAUNCH_SCHEME(grid, advection, launch_momentum_tendencies_general, grid, c2, u, v, w, Gu, Gv, Gw, range, s);
    if (c2) return OCN_LAUNCH(grid, launch_momentum_centered2, grid, u, v, w, Gu, Gv, Gw, range, s);
    return OCN_LAUNCH_SCHEME(grid, advection, launch_momentum_tendencies, grid, u, v, w, Gu, Gv, Gw, range, nullptr, s);
}
static int launch_advective_tracer(int advection, const ocn_grid *grid, const double *u, const double *v, const double *w, const double *c,
                                   double *Gc, const int32_t *range, hipStream_t s, const TracerFuse *tf, const ocn::ForcingDev *frc = nullptr)
{
    const int c2 = advection == OCN_ADVECTION_CENTERED2;
    if (!xy_periodic(grid))  // (tf: diffusion / bottom and top fluxes / the next substep ride along, general.hip)
        return OCN_LAUNCH_SCHEME(grid, advection, launch_tracer_tendency_general, grid, c2, u, v, w, c, Gc, range, s, tf, frc);
    if (c2) return OCN_LAUNCH(grid, launch_tracer_centered2, grid, u, v, w, c, Gc, range, s);
    return OCN_LAUNCH_SCHEME(grid, advection, launch_tracer_tendency, grid, u, v, w, c, Gc, range, s, tf, frc);
}

// stokes_drift = UniformStokesDrift: the device vectors of the profiles (NULL = zero); a vertical shear needs a z direction
static int validate_stokes(const ocn_grid *grid, const ocn_stokes_drift *stokes, const char *who)
{
    OCN_REQUIRE(stokes != nullptr, "%s: stokes is NULL", who);
    OCN_REQUIRE(grid->tz != OCN_FLAT, "%s: UniformStokesDrift needs a non-Flat z", who);
    return OCN_SUCCESS;
}

// forcing of one field: only the descriptor is looked at (host memory), never what its device pointers point to
}  // extern "C"
int ocn::validate_forcing(const ocn_grid *grid, const ocn_forcing *f, const char *who, const char *field)
{
    if (!f) return OCN_SUCCESS;
    OCN_REQUIRE(f->n_terms >= 0 && f->n_terms <= OCN_FORCING_MAX_TERMS, "%s: forcing of %s has n_terms = %d outside 0..%d", who, field, f->n_terms,
                OCN_FORCING_MAX_TERMS);
    const int topo[3] = {grid->tx, grid->ty, grid->tz};
    for (int q = 0; q < f->n_terms; ++q) {
        const ocn_forcing_term &t = f->term[q];
        OCN_REQUIRE(t.kind == OCN_FORCING_ARRAY || t.kind == OCN_FORCING_RELAXATION, "%s: forcing of %s, term %d: unknown kind %d", who, field, q, t.kind);
        if (t.kind == OCN_FORCING_ARRAY) {
            OCN_REQUIRE(t.values != nullptr, "%s: forcing of %s, term %d: values is NULL", who, field, q);
            continue;
        }
        const int dims[2] = {t.mask_dim, t.target_dim};
        const double *ptrs[2] = {t.mask, t.target};
        for (int m = 0; m < 2; ++m) {
            const char *what = m ? "target" : "mask";
            OCN_REQUIRE(dims[m] >= -1 && dims[m] <= 3, "%s: forcing of %s, term %d: %s_dim = %d outside -1..3", who, field, q, what, dims[m]);
            OCN_REQUIRE(dims[m] < 0 || ptrs[m] != nullptr, "%s: forcing of %s, term %d: %s is NULL but %s_dim = %d", who, field, q, what, what, dims[m]);
            OCN_REQUIRE(dims[m] < 0 || dims[m] > 2 || topo[dims[m]] != OCN_FLAT, "%s: forcing of %s, term %d: %s varies along a Flat direction (%d)", who,
                        field, q, what, dims[m]);
        }
    }
    return OCN_SUCCESS;
}
extern "C" {
// The optional parts of the two momentum families, checked and converted.  stokes / forcing stay NULL where the caller gave none (forcing:
// a NULL array, or no term on any of u, v, w): the launchers pick their kernels by these pointers.
struct MomentumOptions {
    ocn::StokesDev sd{};
    ocn::MomentumForcingDev md{};
    const ocn::StokesDev *stokes = nullptr;
    const ocn::MomentumForcingDev *forcing = nullptr;
};
static int momentum_options(const char *who, const ocn_grid *grid, const ocn_stokes_drift *stokes, const ocn_forcing *const *forcing,
                            MomentumOptions &o)
{
    static const char *names[3] = {"u", "v", "w"};
    OCN_REQUIRE(grid != nullptr || (!stokes && !forcing), "grid is NULL");
    for (int f = 0; forcing && f < 3; ++f) {
        OCN_TRY(validate_forcing(grid, forcing[f], who, names[f]));
        o.md.f[f] = ocn::to_dev(forcing[f]);
        if (o.md.f[f].n > 0) o.forcing = &o.md;
    }
    if (!stokes) return OCN_SUCCESS;
    OCN_TRY(validate_stokes(grid, stokes, who));
    o.sd = ocn::to_dev(*stokes);
    o.stokes = &o.sd;
    return OCN_SUCCESS;
}

// THE body of ocn_compute_momentum_tendencies_terms[_stokes | _forced]: stokes and forcing (the array, or every entry of it) may be NULL
static int momentum_tendencies_terms(const char *who, const ocn_grid *grid, const ocn_model_terms *terms, const ocn_stokes_drift *stokes,
                                     const ocn_forcing *const *forcing, const double *u, const double *v, const double *w, double *Gu,
                                     double *Gv, double *Gw, const int32_t *range, void *stream)
{
    MomentumOptions o;
    OCN_TRY(momentum_options(who, grid, stokes, forcing, o));
    OCN_TRY(validate_terms(grid, terms));
    OCN_REQUIRE(u && v && w && Gu && Gv && Gw, "%s: null field pointer", who);
    OCN_REQUIRE((grid->tx == OCN_FLAT || grid->Hx >= 1) && (grid->ty == OCN_FLAT || grid->Hy >= 1) && (grid->tz == OCN_FLAT || grid->Hz >= 1), "halo >= 1 required");
    hipStream_t s = as_stream(stream);
    OCN_TRY(launch_advective_momentum(terms->advection, grid, u, v, w, Gu, Gv, Gw, range, s));
    if (!(terms->coriolis || terms->closure || terms->buoyancy || o.stokes || o.forcing)) return OCN_SUCCESS;
    TermsDev t = to_dev(*terms);
    if (!xy_periodic(grid)) return OCN_LAUNCH(grid, launch_momentum_extra_general, grid, t, u, v, w, Gu, Gv, Gw, range, s, nullptr, o.stokes, o.forcing);
    return OCN_LAUNCH(grid, launch_momentum_extra, grid, t, u, v, w, Gu, Gv, Gw, range, s, nullptr, o.stokes, o.forcing);
}

int ocn_compute_momentum_tendencies_terms(const ocn_grid *grid, const ocn_model_terms *terms, const double *u, const double *v,
                                          const double *w, double *Gu, double *Gv, double *Gw, const int32_t *range,
                                          void *stream)
{
    return momentum_tendencies_terms(__func__, grid, terms, nullptr, nullptr, u, v, w, Gu, Gv, Gw, range, stream);
}

int ocn_compute_momentum_tendencies_terms_stokes(const ocn_grid *grid, const ocn_model_terms *terms, const ocn_stokes_drift *stokes,
                                                 const double *u, const double *v, const double *w, double *Gu, double *Gv, double *Gw,
                                                 const int32_t *range, void *stream)
{
    return momentum_tendencies_terms(__func__, grid, terms, stokes, nullptr, u, v, w, Gu, Gv, Gw, range, stream);
}

int ocn_compute_momentum_tendencies_terms_forced(const ocn_grid *grid, const ocn_model_terms *terms, const ocn_stokes_drift *stokes,
                                                 const ocn_forcing *const *forcing, const double *u, const double *v, const double *w,
                                                 double *Gu, double *Gv, double *Gw, const int32_t *range, void *stream)
{
    return momentum_tendencies_terms(__func__, grid, terms, stokes, forcing, u, v, w, Gu, Gv, Gw, range, stream);
}

// the extra terms alone, added to a G that already holds what precedes them in the reference's sum (used by the hydrostatic
// tendencies, where - g ∂x η comes between the advection and the Coriolis term)
int ocn_add_momentum_terms(const ocn_grid *grid, const ocn_model_terms *terms, const double *u, const double *v, const double *w,
                           double *Gu, double *Gv, double *Gw, const int32_t *range, void *stream)
{
    OCN_TRY(validate_terms(grid, terms));
    OCN_REQUIRE(u && v && w && Gu && Gv && Gw, "ocn_add_momentum_terms: null field pointer");
    OCN_REQUIRE(grid->Hx >= 1 && grid->Hy >= 1 && (grid->tz == OCN_FLAT || grid->Hz >= 1), "halo >= 1 required");
    if (!(terms->coriolis || terms->closure || terms->buoyancy)) return OCN_SUCCESS;
    TermsDev t = to_dev(*terms);
    if (!xy_periodic(grid))  // walls in x / y: per-field parent layouts (general.hip), as ocn_compute_momentum_tendencies_terms dispatches
        return OCN_LAUNCH(grid, launch_momentum_extra_general, grid, t, u, v, w, Gu, Gv, Gw, range, as_stream(stream), nullptr, nullptr, nullptr);
    return OCN_LAUNCH(grid, launch_momentum_extra, grid, t, u, v, w, Gu, Gv, Gw, range, as_stream(stream));
}

// the wall grids of hydrostatic_surface.hip: walls in y (a channel) or in x and y (a closed basin), regular and not partitioned
static bool hydrostatic_walls(const ocn_grid *grid)
{
    return (grid->tx == OCN_PERIODIC || grid->tx == OCN_BOUNDED) && grid->ty == OCN_BOUNDED && grid->tz == OCN_BOUNDED;
}
// walls_ok: the entry point has kernels for (Periodic, Bounded, Bounded) and (Bounded, Bounded, Bounded) grids as well; the others say
// which topology they need
static int validate_hydrostatic(const ocn_grid *grid, const char *who, bool walls_ok = false)
{
    OCN_REQUIRE(grid, "%s: null grid", who);
    if (hydrostatic_walls(grid)) {
        OCN_REQUIRE(walls_ok, "%s: this entry point of the hydrostatic slice needs a (Periodic, Periodic, Bounded) grid", who);
        OCN_TRY(validate_grid_any(grid));
        OCN_REQUIRE(grid->Hx >= 1 && grid->Hy >= 1, "%s: needs x, y halos", who);
        return OCN_SUCCESS;
    }
    OCN_TRY(validate_grid(grid));
    // x may be the partitioned direction of a slab-x rank (FullyConnected: halos come from the neighbours, interior arithmetic as Periodic)
    OCN_REQUIRE((grid->tx == OCN_PERIODIC || grid->tx == OCN_FULLY_CONNECTED) && grid->ty == OCN_PERIODIC && grid->tz == OCN_BOUNDED,
                walls_ok ? "%s: the hydrostatic slice supports (Periodic, Periodic | Bounded, Bounded) and (Bounded, Bounded, Bounded) grids"
                         : "%s: the hydrostatic slice supports (Periodic, Periodic, Bounded) grids", who);
    OCN_REQUIRE(grid->Hx >= 1 && grid->Hy >= 1, "%s: needs x, y halos", who);
    return OCN_SUCCESS;
}
#define OCN_REQUIRE_PERIODIC_X(who) OCN_REQUIRE(grid->tx == OCN_PERIODIC, "%s wraps x periodically: not for a partitioned (FullyConnected) x", who)
int ocn_compute_vector_invariant_momentum_tendencies(const ocn_grid *grid, const double *u, const double *v, const double *w, double *Gu,
                                                     double *Gv, const double *eta, double gravitational_acceleration, void *stream)
{
    OCN_TRY(validate_hydrostatic(grid, "ocn_compute_vector_invariant_momentum_tendencies", true));
    OCN_REQUIRE(u && v && w && Gu && Gv, "ocn_compute_vector_invariant_momentum_tendencies: null field pointer");
    OCN_REQUIRE(grid->Hz >= 1, "ocn_compute_vector_invariant_momentum_tendencies: needs a z halo");
    return launch_vector_invariant(grid, Bottom{}, u, v, w, Gu, Gv, eta, gravitational_acceleration, as_stream(stream));
}
int ocn_compute_vector_invariant_weno_momentum_tendencies(const ocn_grid *grid, int32_t scheme_flags, const double *u, const double *v,
                                                          const double *w, double *Gu, double *Gv, const double *eta,
                                                          double gravitational_acceleration, void *stream)
{
    const char *who = "ocn_compute_vector_invariant_weno_momentum_tendencies";
    OCN_TRY(validate_hydrostatic(grid, who));
    OCN_REQUIRE_PERIODIC_X(who);
    OCN_REQUIRE(u && v && w && Gu && Gv, "%s: null field pointer", who);
    const int32_t weno = OCN_VI_WENO_VORTICITY | OCN_VI_WENO_VERTICAL | OCN_VI_WENO_KINETIC_ENERGY;
    OCN_REQUIRE(!(scheme_flags & ~(weno | OCN_VI_DEFAULT_STENCIL)), "%s: unknown scheme flag bits in %d", who, (int)scheme_flags);
    OCN_REQUIRE(scheme_flags & weno, "%s: no sub-scheme is WENO: that is ocn_compute_vector_invariant_momentum_tendencies", who);
    OCN_REQUIRE(!(scheme_flags & OCN_VI_WENO_KINETIC_ENERGY) || (scheme_flags & OCN_VI_WENO_VERTICAL),
                "%s: an upwinding kinetic-energy gradient needs an upwinding divergence scheme (its Centered(order=4) is the cross scheme)", who);
    OCN_REQUIRE(grid->Hx >= 3 && grid->Hy >= 3 && grid->Hz >= 1, "%s: reads 3 cells beyond the interior in x and y and 1 plane in z; halo is (%d, %d, %d)",
                who, grid->Hx, grid->Hy, grid->Hz);
    return launch_vector_invariant_weno(grid, scheme_flags, u, v, w, Gu, Gv, eta, gravitational_acceleration, as_stream(stream));
}
int ocn_split_explicit_forcing(const ocn_grid *grid, const double *Gu, const double *Gu_previous, const double *Gv, const double *Gv_previous,
                               double chi, double *GU, double *GV, void *stream)
{
    OCN_TRY(validate_hydrostatic(grid, "ocn_split_explicit_forcing", true));
    OCN_REQUIRE(Gu && Gu_previous && Gv && Gv_previous && GU && GV, "ocn_split_explicit_forcing: null pointer");
    return launch_split_explicit_forcing(grid, Bottom{}, Gu, Gu_previous, Gv, Gv_previous, chi, GU, GV, as_stream(stream));
}
int ocn_split_explicit_substeps(const ocn_grid *grid, int32_t n, const double *weights, double dtau, double gravitational_acceleration,
                                double column_depth, double *eta, double *U, double *V, double *eta_filtered, double *U_filtered,
                                double *V_filtered, const double *GU, const double *GV, void *stream)
{
    OCN_TRY(validate_hydrostatic(grid, "ocn_split_explicit_substeps", true));
    OCN_REQUIRE(grid->tx != OCN_FULLY_CONNECTED, "ocn_split_explicit_substeps wraps x periodically: not for a partitioned (FullyConnected) x");
    OCN_REQUIRE(n >= 1 && weights, "ocn_split_explicit_substeps: needs n >= 1 averaging weights (host array)");
    OCN_REQUIRE(eta && U && V && eta_filtered && U_filtered && V_filtered && GU && GV, "ocn_split_explicit_substeps: null pointer");
    return launch_split_explicit_substeps(grid, Bottom{}, n, weights, dtau, gravitational_acceleration, column_depth, eta, U, V, eta_filtered, U_filtered,
                                          V_filtered, GU, GV, as_stream(stream));
}
int ocn_compute_barotropic_mode(const ocn_grid *grid, const double *u, const double *v, double *U, double *V, void *stream)
{
    OCN_TRY(validate_hydrostatic(grid, "ocn_compute_barotropic_mode", true));
    OCN_REQUIRE(u && v && U && V, "ocn_compute_barotropic_mode: null pointer");
    return launch_barotropic_mode(grid, u, v, U, V, as_stream(stream));
}
int ocn_barotropic_split_explicit_corrector(const ocn_grid *grid, double *u, double *v, const double *U, const double *V, double *U_filtered,
                                            double *V_filtered, double column_depth, void *stream)
{
    OCN_TRY(validate_hydrostatic(grid, "ocn_barotropic_split_explicit_corrector", true));
    OCN_REQUIRE(u && v && U && V && U_filtered && V_filtered, "ocn_barotropic_split_explicit_corrector: null pointer");
    return launch_barotropic_corrector(grid, Bottom{}, u, v, U, V, U_filtered, V_filtered, column_depth, as_stream(stream));
}
int ocn_fill_free_surface_halos(const ocn_grid *grid, double *eta, void *stream)
{
    OCN_TRY(validate_hydrostatic(grid, "ocn_fill_free_surface_halos", true));
    OCN_REQUIRE(eta, "ocn_fill_free_surface_halos: null pointer");
    return launch_plane_halo(grid, eta, as_stream(stream));
}
int ocn_compute_w_from_continuity(const ocn_grid *grid, const double *u, const double *v, double *w, void *stream)
{
    OCN_TRY(validate_hydrostatic(grid, "ocn_compute_w_from_continuity", true));
    OCN_REQUIRE(u && v && w, "ocn_compute_w_from_continuity: null field pointer");
    return launch_w_from_continuity(grid, u, v, w, as_stream(stream));
}
int ocn_add_barotropic_pressure_gradient(const ocn_grid *grid, double gravitational_acceleration, const double *eta, double *Gu, double *Gv,
                                         void *stream)
{
    OCN_TRY(validate_hydrostatic(grid, "ocn_add_barotropic_pressure_gradient", true));
    OCN_REQUIRE(eta && Gu && Gv, "ocn_add_barotropic_pressure_gradient: null pointer");
    return launch_barotropic_gradient(grid, gravitational_acceleration, eta, Gu, Gv, as_stream(stream));
}
int ocn_explicit_free_surface_ab2_step(const ocn_grid *grid, const double *w, double *eta, double *G_eta, const double *G_eta_previous,
                                       double dt, double chi, void *stream)
{
    OCN_TRY(validate_hydrostatic(grid, "ocn_explicit_free_surface_ab2_step", true));  // (w and η share x / y extents: one kernel)
    OCN_REQUIRE(w && eta && G_eta && G_eta_previous, "ocn_explicit_free_surface_ab2_step: null pointer");
    return launch_free_surface_ab2(grid, w, eta, G_eta, G_eta_previous, dt, chi, as_stream(stream));
}

// ---- ImmersedBoundaryGrid(grid, GridFittedBottom(h)) on a (Periodic, Periodic, Bounded) grid (immersed.hip)
static int validate_immersed(const ocn_grid *grid, const char *who)
{
    OCN_TRY(validate_hydrostatic(grid, who));
    OCN_REQUIRE(grid->tx == OCN_PERIODIC, "%s: an immersed grid cannot be partitioned (FullyConnected x)", who);
    OCN_REQUIRE(grid->Hz >= 1, "%s: needs a z halo", who);
    return OCN_SUCCESS;
}
int ocn_immersed_compute_bottom(const ocn_grid *grid, int32_t interface_condition, const double *h, const double *z_centers,
                                const double *z_faces, double *bottom_height, int32_t *kbot, double *Hcc, double *Hfc, double *Hcf,
                                void *stream)
{
    OCN_TRY(validate_immersed(grid, "ocn_immersed_compute_bottom"));
    OCN_REQUIRE(interface_condition == 0 || interface_condition == 1, "ocn_immersed_compute_bottom: immersed condition %d is neither 0 (Center) nor 1 (Interface)",
                (int)interface_condition);
    OCN_REQUIRE(h && z_centers && z_faces && bottom_height && kbot && Hcc && Hfc && Hcf, "ocn_immersed_compute_bottom: null pointer");
    return launch_immersed_bottom(grid, interface_condition, h, z_centers, z_faces, bottom_height, kbot, Hcc, Hfc, Hcf, as_stream(stream));
}
int ocn_immersed_mask_fields(const ocn_grid *grid, const int32_t *kbot, int32_t n, double *const *fields, const int32_t *locs, double value,
                             double *eta, double *U, double *V, void *stream)
{
    OCN_TRY(validate_immersed(grid, "ocn_immersed_mask_fields"));
    OCN_REQUIRE(kbot, "ocn_immersed_mask_fields: null kbot");
    FieldTuple ft;
    ft.n = 0;
    if (n != 0) {
        OCN_TRY(make_field_tuple(grid, fields, locs, n, ft));
    }
    OCN_REQUIRE(n != 0 || eta || U || V, "ocn_immersed_mask_fields: nothing to mask");
    return launch_immersed_mask(grid, kbot, ft, value, eta, U, V, as_stream(stream));
}
int ocn_immersed_vector_invariant_momentum_tendencies(const ocn_grid *grid, const int32_t *kbot, const double *u, const double *v,
                                                      const double *w, double *Gu, double *Gv, const double *eta,
                                                      double gravitational_acceleration, void *stream)
{
    OCN_TRY(validate_immersed(grid, "ocn_immersed_vector_invariant_momentum_tendencies"));
    OCN_REQUIRE(kbot && u && v && w && Gu && Gv, "ocn_immersed_vector_invariant_momentum_tendencies: null pointer");
    return launch_vector_invariant(grid, Bottom{kbot}, u, v, w, Gu, Gv, eta, gravitational_acceleration, as_stream(stream));
}
int ocn_immersed_add_viscous_terms(const ocn_grid *grid, const int32_t *kbot, double nu, const double *u, const double *v, const double *w,
                                   double *Gu, double *Gv, void *stream)
{
    OCN_TRY(validate_immersed(grid, "ocn_immersed_add_viscous_terms"));
    OCN_REQUIRE(kbot && u && v && w && Gu && Gv, "ocn_immersed_add_viscous_terms: null pointer");
    OCN_REQUIRE(std::isfinite(nu) && nu >= 0, "ocn_immersed_add_viscous_terms: nu = %g must be finite and >= 0", nu);
    return launch_viscosity_immersed(grid, kbot, nu, u, v, w, Gu, Gv, as_stream(stream));
}
int ocn_immersed_tracer_tendency(const ocn_grid *grid, const int32_t *kbot, int32_t closure, double kappa, const double *u, const double *v,
                                 const double *w, const double *c, double *Gc, void *stream)
{
    OCN_TRY(validate_immersed(grid, "ocn_immersed_tracer_tendency"));
    OCN_REQUIRE(kbot && u && v && w && c && Gc, "ocn_immersed_tracer_tendency: null pointer");
    OCN_REQUIRE(closure == 0 || closure == 1, "ocn_immersed_tracer_tendency: closure must be 0 (none) or 1 (ScalarDiffusivity), got %d", (int)closure);
    OCN_REQUIRE(!closure || (std::isfinite(kappa) && kappa >= 0), "ocn_immersed_tracer_tendency: kappa = %g must be finite and >= 0", kappa);
    return launch_tracer_immersed(grid, kbot, closure, kappa, u, v, w, c, Gc, as_stream(stream));
}
int ocn_immersed_split_explicit_forcing(const ocn_grid *grid, const int32_t *kbot, const double *Gu, const double *Gu_previous,
                                        const double *Gv, const double *Gv_previous, double chi, double *GU, double *GV, void *stream)
{
    OCN_TRY(validate_immersed(grid, "ocn_immersed_split_explicit_forcing"));
    OCN_REQUIRE(kbot && Gu && Gu_previous && Gv && Gv_previous && GU && GV, "ocn_immersed_split_explicit_forcing: null pointer");
    return launch_split_explicit_forcing(grid, Bottom{kbot}, Gu, Gu_previous, Gv, Gv_previous, chi, GU, GV, as_stream(stream));
}
int ocn_immersed_split_explicit_substeps(const ocn_grid *grid, const int32_t *kbot, const double *Hfc, const double *Hcf, int32_t n,
                                         const double *weights, double dtau, double gravitational_acceleration, double *eta, double *U,
                                         double *V, double *eta_filtered, double *U_filtered, double *V_filtered, const double *GU,
                                         const double *GV, void *stream)
{
    OCN_TRY(validate_immersed(grid, "ocn_immersed_split_explicit_substeps"));
    OCN_REQUIRE(n >= 1 && weights, "ocn_immersed_split_explicit_substeps: needs n >= 1 averaging weights (host array)");
    OCN_REQUIRE(kbot && Hfc && Hcf && eta && U && V && eta_filtered && U_filtered && V_filtered && GU && GV,
                "ocn_immersed_split_explicit_substeps: null pointer");
    return launch_split_explicit_substeps(grid, Bottom{kbot, Hfc, Hcf}, n, weights, dtau, gravitational_acceleration, 0.0, eta, U, V, eta_filtered,
                                          U_filtered, V_filtered, GU, GV, as_stream(stream));
}
int ocn_immersed_barotropic_corrector(const ocn_grid *grid, const double *Hfc, const double *Hcf, double *u, double *v, const double *U,
                                      const double *V, double *U_filtered, double *V_filtered, void *stream)
{
    OCN_TRY(validate_immersed(grid, "ocn_immersed_barotropic_corrector"));
    OCN_REQUIRE(Hfc && Hcf && u && v && U && V && U_filtered && V_filtered, "ocn_immersed_barotropic_corrector: null pointer");
    return launch_barotropic_corrector(grid, Bottom{nullptr, Hfc, Hcf}, u, v, U, V, U_filtered, V_filtered, 0.0, as_stream(stream));
}

static int validate_amd(const ocn_grid *grid)
{
    OCN_TRY(validate_grid_any(grid));  // Bounded x / y: the kernel takes per-field parent layouts
    OCN_REQUIRE(grid->tz != OCN_FLAT, "AnisotropicMinimumDissipation needs a non-Flat z");
    OCN_REQUIRE((grid->tx == OCN_FLAT || grid->Hx >= 1) && (grid->ty == OCN_FLAT || grid->Hy >= 1) && grid->Hz >= 1,
                "AnisotropicMinimumDissipation needs halo >= 1");
    return OCN_SUCCESS;
}

int ocn_compute_amd_viscosity(const ocn_grid *grid, double C_nu, const double *u, const double *v, const double *w, double *nu_e,
                              void *stream)
{
    OCN_TRY(validate_amd(grid));
    OCN_REQUIRE(u && v && w && nu_e, "ocn_compute_amd_viscosity: null field pointer");
    return OCN_LAUNCH(grid, launch_amd_viscosity, grid, C_nu, u, v, w, nu_e, as_stream(stream));
}

int ocn_compute_amd_diffusivities(const ocn_grid *grid, double C_nu, const double *u, const double *v, const double *w,
                                  double *nu_e, int32_t n_tracers, const double *C_kappa, const double *const *tracers,
                                  double *const *kappa_e, void *stream)
{
    OCN_TRY(validate_amd(grid));
    OCN_REQUIRE(u && v && w && nu_e, "ocn_compute_amd_diffusivities: null field pointer");
    OCN_REQUIRE(n_tracers >= 0 && n_tracers <= 4, "ocn_compute_amd_diffusivities: n_tracers = %d outside 0..4", n_tracers);
    OCN_REQUIRE(n_tracers == 0 || (C_kappa && tracers && kappa_e), "ocn_compute_amd_diffusivities: null tracer arrays");
    for (int n = 0; n < n_tracers; ++n) OCN_REQUIRE(tracers[n] && kappa_e[n], "ocn_compute_amd_diffusivities: tracer %d is NULL", n);
    return OCN_LAUNCH(grid, launch_amd_fused, grid, C_nu, u, v, w, nu_e, n_tracers, C_kappa, tracers, kappa_e, as_stream(stream));
}

int ocn_compute_amd_diffusivities_range(const ocn_grid *grid, double C_nu, const double *u, const double *v, const double *w,
                                        double *nu_e, int32_t n_tracers, const double *C_kappa, const double *const *tracers,
                                        double *const *kappa_e, int32_t i_first, int32_t i_last, void *stream)
{
    OCN_TRY(validate_amd(grid));
    OCN_REQUIRE(u && v && w && nu_e, "ocn_compute_amd_diffusivities_range: null field pointer");
    OCN_REQUIRE(n_tracers >= 0 && n_tracers <= 4, "ocn_compute_amd_diffusivities_range: n_tracers = %d outside 0..4", n_tracers);
    OCN_REQUIRE(n_tracers == 0 || (C_kappa && tracers && kappa_e), "ocn_compute_amd_diffusivities_range: null tracer arrays");
    for (int n = 0; n < n_tracers; ++n) OCN_REQUIRE(tracers[n] && kappa_e[n], "ocn_compute_amd_diffusivities_range: tracer %d is NULL", n);
    OCN_REQUIRE(i_first >= 0 && i_last <= grid->Nx + 1, "ocn_compute_amd_diffusivities_range: i range %d:%d outside 0:%d", i_first, i_last, grid->Nx + 1);
    OCN_REQUIRE((i_first >= 1 && i_last <= grid->Nx) || grid->Hx >= 2, "the halo columns 0 and Nx+1 need Hx >= 2");
    const int32_t ir[2] = {i_first, i_last};
    return OCN_LAUNCH(grid, launch_amd_fused, grid, C_nu, u, v, w, nu_e, n_tracers, C_kappa, tracers, kappa_e, as_stream(stream), ir);
}

int ocn_compute_amd_diffusivity(const ocn_grid *grid, double C_kappa, const double *u, const double *v, const double *w,
                                const double *c, double *kappa_e, void *stream)
{
    OCN_TRY(validate_amd(grid));
    OCN_REQUIRE(u && v && w && c && kappa_e, "ocn_compute_amd_diffusivity: null field pointer");
    return OCN_LAUNCH(grid, launch_amd_diffusivity, grid, C_kappa, u, v, w, c, kappa_e, as_stream(stream));
}

int ocn_compute_smagorinsky_diffusivities(const ocn_grid *grid, const ocn_model_terms *terms, const ocn_smagorinsky *closure,
                                          const double *u, const double *v, const double *w, double *nu_e, double *const *kappa_e,
                                          void *stream)
{
    OCN_TRY(validate_grid_any(grid));
    OCN_REQUIRE(grid->tz != OCN_FLAT, "Smagorinsky needs a non-Flat z");
    OCN_REQUIRE((grid->tx == OCN_FLAT || grid->Hx >= 1) && (grid->ty == OCN_FLAT || grid->Hy >= 1) && grid->Hz >= 1, "Smagorinsky needs halo >= 1");
    OCN_REQUIRE(terms && closure, "ocn_compute_smagorinsky_diffusivities: null terms / closure");
    OCN_REQUIRE(u && v && w && nu_e, "ocn_compute_smagorinsky_diffusivities: null field pointer");
    OCN_REQUIRE(closure->lilly == 0 || closure->lilly == 1, "ocn_compute_smagorinsky_diffusivities: lilly = %d is neither 0 nor 1", closure->lilly);
    OCN_REQUIRE(closure->n_tracers >= 0 && closure->n_tracers <= OCN_MODEL_MAX_TRACERS, "ocn_compute_smagorinsky_diffusivities: n_tracers = %d outside 0..%d",
                closure->n_tracers, OCN_MODEL_MAX_TRACERS);
    if (closure->lilly) {
        const int b = terms->buoyancy;
        OCN_REQUIRE(b >= OCN_BUOYANCY_NONE && b <= OCN_BUOYANCY_SEAWATER_S, "ocn_compute_smagorinsky_diffusivities: unknown buoyancy %d", b);
        if (buoyancy_reads_T(b))
            OCN_REQUIRE(terms->T != nullptr, "ocn_compute_smagorinsky_diffusivities: LillyCoefficient reads N²: T (or b) tracer is NULL");
        if (buoyancy_reads_S(b))
            OCN_REQUIRE(terms->S != nullptr, "ocn_compute_smagorinsky_diffusivities: LillyCoefficient reads N²: S tracer is NULL");
    }
    for (int n = 0; n < closure->n_tracers; ++n) {
        OCN_REQUIRE(closure->Pr[n] > 0, "ocn_compute_smagorinsky_diffusivities: Pr[%d] = %g must be positive", n, closure->Pr[n]);
        OCN_REQUIRE(closure->Pr[n] == 1.0 || (kappa_e && kappa_e[n]), "ocn_compute_smagorinsky_diffusivities: Pr[%d] != 1 needs a kappa_e field", n);
        OCN_REQUIRE(closure->Pr[n] == 1.0 || kappa_e[n] != nu_e, "ocn_compute_smagorinsky_diffusivities: Pr[%d] != 1 needs a kappa_e field other than nu_e", n);
        OCN_REQUIRE(closure->Pr[n] != 1.0 || !kappa_e || !kappa_e[n] || kappa_e[n] == nu_e,
                    "ocn_compute_smagorinsky_diffusivities: Pr[%d] == 1: kappa_e must be NULL or the nu_e array (the tracer reads nu_e)", n);
    }
    const TermsDev t = to_dev(*terms);
    return OCN_LAUNCH(grid, launch_smagorinsky, grid, t, *closure, u, v, w, nu_e, kappa_e, as_stream(stream));
}

// ---- Lagrangian particles (csrc/particles.hip) --------------------------------------------------------
// everything but the position / velocity pointers; *empty: nothing to launch
static int validate_particles(const char *who, const ocn_grid *grid, const ocn_particle_geometry *geom, int64_t n, int32_t n_tracked,
                              const double *const *tracked_fields, const int32_t *tracked_locs, double *const *tracked_out)
{
    OCN_REQUIRE(n >= 0, "%s: negative particle count %lld", who, (long long)n);
    OCN_TRY(validate_grid_any(grid));
    if (partitioned_x(grid)) {
        set_error("%s: particles on a partitioned x (topology code %d) are not supported", who, grid->tx);
        return OCN_ERR_UNSUPPORTED;
    }
    OCN_REQUIRE(n_tracked >= 0 && n_tracked <= OCN_PARTICLES_MAX_TRACKED, "%s: n_tracked = %d outside 0..%d", who, n_tracked,
                OCN_PARTICLES_MAX_TRACKED);
    if (n == 0) return OCN_SUCCESS;
    OCN_REQUIRE(n <= (int64_t)1 << 39, "%s: more than 2^39 particles", who);
    OCN_REQUIRE(geom != nullptr, "%s: geometry is NULL", who);
    OCN_REQUIRE(!grid->dzc || grid->tz == OCN_FLAT || (geom->zf && geom->zc), "%s: a stretched z needs the node vectors zf, zc", who);
    OCN_REQUIRE(n_tracked == 0 || (tracked_fields && tracked_locs && tracked_out), "%s: null tracked-field arrays", who);
    for (int q = 0; q < n_tracked; ++q) {
        OCN_REQUIRE(tracked_fields[q] && tracked_out[q], "%s: null tracked field / output pointer %d", who, q);
        OCN_REQUIRE(tracked_locs[q] >= 0 && tracked_locs[q] <= 7, "%s: location mask %d of tracked field %d outside 0..7", who, tracked_locs[q], q);
    }
    return OCN_SUCCESS;
}

int ocn_sample_particle_properties(const ocn_grid *grid, const ocn_particle_geometry *geom, int64_t n, const double *x, const double *y,
                                   const double *z, int32_t n_tracked, const double *const *tracked_fields, const int32_t *tracked_locs,
                                   double *const *tracked_out, void *stream)
{
    int st = validate_particles("ocn_sample_particle_properties", grid, geom, n, n_tracked, tracked_fields, tracked_locs, tracked_out);
    if (st != OCN_SUCCESS || n == 0 || n_tracked == 0) return st;
    OCN_REQUIRE(x && y && z, "ocn_sample_particle_properties: null position pointer");
    return launch_particles(grid, geom, n, const_cast<double *>(x), const_cast<double *>(y), const_cast<double *>(z), 0, 0.0, nullptr, nullptr,
                            nullptr, 0.0, n_tracked, tracked_fields, tracked_locs, tracked_out, as_stream(stream));
}

int ocn_advect_particles(const ocn_grid *grid, const ocn_particle_geometry *geom, int64_t n, double *x, double *y, double *z,
                         double restitution, const double *u, const double *v, const double *w, double dt, int32_t n_tracked,
                         const double *const *tracked_fields, const int32_t *tracked_locs, double *const *tracked_out, void *stream)
{
    int st = validate_particles("ocn_advect_particles", grid, geom, n, n_tracked, tracked_fields, tracked_locs, tracked_out);
    if (st != OCN_SUCCESS || n == 0) return st;
    OCN_REQUIRE(x && y && z, "ocn_advect_particles: null position pointer");
    OCN_REQUIRE(u && v && w, "ocn_advect_particles: null velocity pointer");
    return launch_particles(grid, geom, n, x, y, z, 1, restitution, u, v, w, dt, n_tracked, tracked_fields, tracked_locs, tracked_out,
                            as_stream(stream));
}

// ---- on-device diagnostics (diagnostics.hip validates the whole program before it launches anything) ----
int ocn_op_compute(const ocn_grid *grid, const ocn_op_program *program, double *out, void *stream)
{
    return op_compute(grid, program, out, as_stream(stream));
}

int ocn_op_accumulate(const ocn_grid *grid, const ocn_op_program *program, double *G, void *stream)
{
    return op_accumulate(grid, program, G, as_stream(stream));
}

int ocn_op_compute_boundary(const ocn_grid *grid, const ocn_op_program *program, int32_t side, double *values, void *stream)
{
    return op_compute_boundary(grid, program, side, values, as_stream(stream));
}

int ocn_op_reduce_workspace(const ocn_grid *grid, int32_t loc, int32_t dims, int64_t *n_doubles)
{
    long long n = 0;
    int st = op_reduce_workspace(grid, loc, dims, n_doubles ? &n : nullptr);
    if (st == OCN_SUCCESS) *n_doubles = n;
    return st;
}

int ocn_op_reduce(const ocn_grid *grid, const ocn_op_program *program, int32_t dims, double divisor, double *workspace,
                  int64_t workspace_doubles, double *out, void *stream)
{
    return op_reduce(grid, program, dims, divisor, workspace, workspace_doubles, out, as_stream(stream));
}

int ocn_update_hydrostatic_pressure(const ocn_grid *grid, const ocn_model_terms *terms, double *pHY, void *stream)
{
    OCN_TRY(validate_grid_any(grid));
    OCN_REQUIRE(terms != nullptr && pHY != nullptr, "ocn_update_hydrostatic_pressure: null argument");
    OCN_REQUIRE(terms->buoyancy != OCN_BUOYANCY_NONE, "ocn_update_hydrostatic_pressure: buoyancy is nothing");
    if (terms->buoyancy != OCN_BUOYANCY_SEAWATER_S) OCN_REQUIRE(terms->T != nullptr, "T (or b) tracer is NULL");
    if (buoyancy_reads_S(terms->buoyancy)) OCN_REQUIRE(terms->S != nullptr, "S tracer is NULL");
    OCN_REQUIRE((grid->tx == OCN_FLAT || grid->Hx >= 1) && (grid->ty == OCN_FLAT || grid->Hy >= 1) && (grid->tz == OCN_FLAT || grid->Hz >= 1),
                "halo >= 1 required");
    return launch_hydrostatic_pressure(grid, to_dev(*terms), pHY, as_stream(stream));
}

int ocn_update_hydrostatic_pressure_range(const ocn_grid *grid, const ocn_model_terms *terms, double *pHY, int32_t i_first, int32_t i_last,
                                          void *stream)
{
    OCN_TRY(validate_grid_any(grid));
    OCN_REQUIRE(terms != nullptr && pHY != nullptr, "ocn_update_hydrostatic_pressure_range: null argument");
    OCN_REQUIRE(terms->buoyancy != OCN_BUOYANCY_NONE, "ocn_update_hydrostatic_pressure_range: buoyancy is nothing");
    if (terms->buoyancy != OCN_BUOYANCY_SEAWATER_S) OCN_REQUIRE(terms->T != nullptr, "T (or b) tracer is NULL");
    if (buoyancy_reads_S(terms->buoyancy)) OCN_REQUIRE(terms->S != nullptr, "S tracer is NULL");
    OCN_REQUIRE(grid->Hx >= 1 && grid->Hy >= 1 && (grid->tz == OCN_FLAT || grid->Hz >= 1), "halo >= 1 required");
    OCN_REQUIRE(i_first >= 0 && i_last <= grid->Nx + 1, "ocn_update_hydrostatic_pressure_range: i range %d:%d outside 0:%d", i_first, i_last, grid->Nx + 1);
    const int32_t ir[2] = {i_first, i_last};
    return launch_hydrostatic_pressure(grid, to_dev(*terms), pHY, as_stream(stream), ir);
}

static int make_zbc_tuple(const ocn_grid *grid, const int32_t *locs, const ocn_field_bcs *const *bcs, int32_t n, ZBcTuple &z,
                          bool flux_only, bool &any)
{
    any = false;
    for (int f = 0; f < n; ++f) {
        z.bottom[f] = ZBc{OCN_BC_DEFAULT, 0.0, 0.0, nullptr};
        z.top[f] = ZBc{OCN_BC_DEFAULT, 0.0, 0.0, nullptr};
        if (!bcs || !bcs[f]) continue;
        const ocn_field_bcs &b = *bcs[f];
        OCN_REQUIRE(b.west.kind == OCN_BC_DEFAULT && b.east.kind == OCN_BC_DEFAULT && b.south.kind == OCN_BC_DEFAULT &&
                        b.north.kind == OCN_BC_DEFAULT,
                    "field %d: only bottom / top boundary conditions are supported (x, y are Periodic)", f);
        const ocn_bc *side[2] = {&b.bottom, &b.top};
        for (int sd = 0; sd < 2; ++sd) {
            const ocn_bc &c = *side[sd];
            OCN_REQUIRE(c.kind >= OCN_BC_DEFAULT && c.kind <= OCN_BC_OPEN, "field %d: unknown boundary condition kind %d", f, c.kind);
            if (c.kind == OCN_BC_DEFAULT) continue;
            OCN_REQUIRE(grid->tz == OCN_BOUNDED, "bottom / top boundary conditions need a Bounded z (topology %d)", grid->tz);
            OCN_REQUIRE(((locs[f] & 4) != 0) == (c.kind == OCN_BC_OPEN),
                        "field %d: the wall-normal velocity takes an Open condition (its value on the boundary face), the other fields Flux / Value / Gradient", f);
            OCN_REQUIRE(!c.values || grid->tx == OCN_PERIODIC, "array boundary conditions are not supported on a partitioned grid");
            if (flux_only && c.kind != OCN_BC_FLUX) continue;
            ZBc &d = sd ? z.top[f] : z.bottom[f];
            d.kind = c.kind; d.value = c.value; d.coeff = c.coeff; d.values = c.values;
            any = true;
        }
    }
    return OCN_SUCCESS;
}

static int flux_side(const ocn_grid *grid, const ocn_field_bcs *b, const char *name, ZBc &bottom, ZBc &top)
{
    bottom = ZBc{OCN_BC_DEFAULT, 0.0, 0.0, nullptr};
    top = ZBc{OCN_BC_DEFAULT, 0.0, 0.0, nullptr};
    if (!b) return OCN_SUCCESS;
    // (Value / Gradient / Open conditions on x / y walls live in the halo fills; FLUXES through them are added by ocn_apply_flux_bcs on the
    //  unfused path only)
    OCN_REQUIRE(b->west.kind != OCN_BC_FLUX && b->east.kind != OCN_BC_FLUX && b->south.kind != OCN_BC_FLUX && b->north.kind != OCN_BC_FLUX,
                "%s: the fused stage boundaries take flux conditions at the bottom / top only", name);
    const ocn_bc *side[2] = {&b->bottom, &b->top};
    for (int sd = 0; sd < 2; ++sd) {
        const ocn_bc &c = *side[sd];
        OCN_REQUIRE(c.kind >= OCN_BC_DEFAULT && c.kind <= OCN_BC_OPEN, "%s: unknown boundary condition kind %d", name, c.kind);
        if (c.kind != OCN_BC_FLUX) continue;
        OCN_REQUIRE(grid->tz == OCN_BOUNDED, "bottom / top boundary conditions need a Bounded z (topology %d)", grid->tz);
        OCN_REQUIRE(!c.values || grid->tx == OCN_PERIODIC, "array boundary conditions need a Periodic x (not partitioned, no x walls)");
        ZBc &d = sd ? top : bottom;
        d.kind = c.kind; d.value = c.value; d.coeff = c.coeff; d.values = c.values;
    }
    return OCN_SUCCESS;
}

// THE body of ocn_compute_momentum_tendencies_terms_rk3[_stokes | _forced]: stokes, forcing (the array, or every entry of it) and the flux
// conditions may be NULL
static int momentum_tendencies_terms_rk3(const char *who, const ocn_grid *grid, const ocn_model_terms *terms, const ocn_stokes_drift *stokes,
                                         const ocn_forcing *const *forcing, const ocn_field_bcs *bcs_u, const ocn_field_bcs *bcs_v,
                                         const double *u, const double *v, const double *w, double *Gu, double *Gv, double *Gw,
                                         const double *Gmu, const double *Gmv, const double *Gmw, double *u_out, double *v_out, double *w_out,
                                         double dt, double gamma, double zeta, int32_t has_zeta, const int32_t *range, void *stream)
{
    MomentumOptions o;
    OCN_TRY(momentum_options(who, grid, stokes, forcing, o));
    OCN_TRY(validate_terms(grid, terms));
    OCN_REQUIRE(xy_periodic(grid) || !range, "%s: ranges need Periodic x and y", who);
    OCN_REQUIRE(u && v && w && Gu && Gv && Gw && u_out && v_out && w_out, "%s: null field pointer", who);
    OCN_REQUIRE(!has_zeta || (Gmu && Gmv && Gmw), "%s: G⁻ pointers are required when has_zeta != 0", who);
    OCN_REQUIRE(u_out != u && v_out != v && w_out != w, "%s: outputs must not alias the inputs", who);
    MomentumFinal mf{};
    OCN_TRY(flux_side(grid, bcs_u, "u", mf.bottom[0], mf.top[0]));
    OCN_TRY(flux_side(grid, bcs_v, "v", mf.bottom[1], mf.top[1]));
    mf.sub[0] = SubstepDev{Gmu, u_out};
    mf.sub[1] = SubstepDev{Gmv, v_out};
    mf.sub[2] = SubstepDev{Gmw, w_out};
    mf.sc = SubstepCoef{dt, gamma, zeta, 1, has_zeta ? 1 : 0};
    hipStream_t s = as_stream(stream);
    TermsDev t = to_dev(*terms);
    if (!xy_periodic(grid)) {
        // walls in x / y: advection (box + frames), then the finishing pass in the reference's order with the boundary fluxes and the substep --
        // inside the tiled kernel on the interior box, as per-cell kernels on the frames (general.hip)
        OCN_TRY(launch_advective_momentum(terms->advection, grid, u, v, w, Gu, Gv, Gw, nullptr, s));
        return OCN_LAUNCH(grid, launch_momentum_extra_general, grid, t, u, v, w, Gu, Gv, Gw, nullptr, s, &mf, o.stokes, o.forcing);
    }
    static const bool extra_first = !(std::getenv("OCN_EXTRA_FIRST") && std::getenv("OCN_EXTRA_FIRST")[0] == '0');
    if (!strict_math(grid) && extra_first && terms->advection != OCN_ADVECTION_CENTERED2) {
        // Fast math: the finishing pass runs FIRST and leaves the non-advective terms (and the u / v boundary fluxes) in G; the WENO
        // launch -- VALU-bound, with HBM bandwidth to spare -- adds its advective part, stores G and does the substep.  The HBM-bound
        // finishing pass then moves 64 instead of 136 B / cell (no G read-modify-write, no G^-, no second storage); the sum is the
        // reference's with the advective term added last instead of first (a reassociation: ~1 ulp of max|G|; the strict build keeps
        // the reference's order).
        MomentumFinal pre = mf;
        pre.pre = 1;
        pre.sc.on = 0;
        OCN_TRY(OCN_LAUNCH(grid, launch_momentum_extra, grid, t, u, v, w, Gu, Gv, Gw, range, s, &pre, o.stokes, o.forcing));
        FuseArgs fz = substep_fuse(Gmu, Gmv, Gmw, u_out, v_out, w_out, dt, gamma, zeta, has_zeta);
        fz.acc = 1;
        return OCN_LAUNCH_SCHEME(grid, terms->advection, launch_momentum_tendencies, grid, u, v, w, Gu, Gv, Gw, range, &fz, s);
    }
    OCN_TRY(launch_advective_momentum(terms->advection, grid, u, v, w, Gu, Gv, Gw, range, s));
    return OCN_LAUNCH(grid, launch_momentum_extra, grid, t, u, v, w, Gu, Gv, Gw, range, s, &mf, o.stokes, o.forcing);
}

int ocn_compute_momentum_tendencies_terms_rk3(const ocn_grid *grid, const ocn_model_terms *terms, const ocn_field_bcs *bcs_u,
                                              const ocn_field_bcs *bcs_v, const double *u, const double *v, const double *w,
                                              double *Gu, double *Gv, double *Gw, const double *Gmu, const double *Gmv,
                                              const double *Gmw, double *u_out, double *v_out, double *w_out, double dt,
                                              double gamma, double zeta, int32_t has_zeta, const int32_t *range, void *stream)
{
    return momentum_tendencies_terms_rk3(__func__, grid, terms, nullptr, nullptr, bcs_u, bcs_v, u, v, w, Gu, Gv, Gw, Gmu, Gmv, Gmw, u_out, v_out, w_out,
                                         dt, gamma, zeta, has_zeta, range, stream);
}

int ocn_compute_momentum_tendencies_terms_rk3_stokes(const ocn_grid *grid, const ocn_model_terms *terms, const ocn_stokes_drift *stokes,
                                                     const ocn_field_bcs *bcs_u, const ocn_field_bcs *bcs_v, const double *u, const double *v,
                                                     const double *w, double *Gu, double *Gv, double *Gw, const double *Gmu,
                                                     const double *Gmv, const double *Gmw, double *u_out, double *v_out, double *w_out,
                                                     double dt, double gamma, double zeta, int32_t has_zeta, const int32_t *range,
                                                     void *stream)
{
    return momentum_tendencies_terms_rk3(__func__, grid, terms, stokes, nullptr, bcs_u, bcs_v, u, v, w, Gu, Gv, Gw, Gmu, Gmv, Gmw, u_out, v_out, w_out,
                                         dt, gamma, zeta, has_zeta, range, stream);
}

int ocn_compute_momentum_tendencies_terms_rk3_forced(const ocn_grid *grid, const ocn_model_terms *terms, const ocn_stokes_drift *stokes,
                                                     const ocn_forcing *const *forcing, const ocn_field_bcs *bcs_u, const ocn_field_bcs *bcs_v,
                                                     const double *u, const double *v, const double *w, double *Gu, double *Gv, double *Gw,
                                                     const double *Gmu, const double *Gmv, const double *Gmw, double *u_out, double *v_out,
                                                     double *w_out, double dt, double gamma, double zeta, int32_t has_zeta,
                                                     const int32_t *range, void *stream)
{
    return momentum_tendencies_terms_rk3(__func__, grid, terms, stokes, forcing, bcs_u, bcs_v, u, v, w, Gu, Gv, Gw, Gmu, Gmv, Gmw, u_out, v_out, w_out,
                                         dt, gamma, zeta, has_zeta, range, stream);
}

// What rides inside a tracer's advective kernel: the diffusion and -- with a substep (sub != NULL) -- the bottom / top fluxes and the substep
static int make_tracer_fuse(const ocn_grid *grid, const ocn_model_terms *terms, double kappa, const double *kappa_e, const ocn_field_bcs *bcs_c,
                            const SubstepDev *sub, const SubstepCoef &sc, TracerFuse &tf)
{
    tf = TracerFuse{};
    tf.diffusion = terms->closure != 0;
    tf.kappa = kappa;
    tf.kappa_e = kappa_e;
    if (!sub) return OCN_SUCCESS;  // (the tendency alone: ocn_apply_flux_bcs adds the boundary fluxes)
    OCN_TRY(flux_side(grid, bcs_c, "tracer", tf.bottom, tf.top));
    tf.sub = *sub;
    tf.sc = sc;
    return OCN_SUCCESS;
}

// THE body of ocn_compute_tracer_tendency_terms[_forced | _rk3 | _rk3_forced]: forcing (or its terms), the flux conditions and the substep
// (sub, with its coefficients sc) may be absent.
// A forced tracer: F rides inside the tracer kernels (tracer_finish / tracer_finish_general compiled with ocn::TracerFuseForced), between the
// diffusion and the boundary fluxes.  Only Centered(order=2) advection on a (Periodic, Periodic, *) grid, whose kernel has no epilogue, takes
// the small tracer_forcing_kernel after the diffusion kernel.
static int tracer_tendency_terms(const char *who, const ocn_grid *grid, const ocn_model_terms *terms, double kappa, const double *kappa_e,
                                 const ocn_forcing *forcing, const ocn_field_bcs *bcs_c, const double *u, const double *v, const double *w,
                                 const double *c, double *Gc, const SubstepDev *sub, const SubstepCoef &sc, const int32_t *range, void *stream)
{
    if (forcing) {
        OCN_REQUIRE(grid != nullptr, "grid is NULL");
        OCN_TRY(validate_forcing(grid, forcing, who, "the tracer"));
    }
    OCN_TRY(validate_terms(grid, terms));
    if (sub) {
        OCN_REQUIRE(xy_periodic(grid) || !range, "%s: ranges need Periodic x and y", who);
        OCN_REQUIRE(terms->advection != OCN_ADVECTION_CENTERED2, "%s: advection must be WENO5 or UpwindBiased5", who);
    }
    OCN_REQUIRE(u && v && w && c && Gc && (!sub || sub->out), "%s: null field pointer", who);
    if (sub) {
        OCN_REQUIRE(!sc.has_zeta || sub->Gm, "%s: G⁻ is required when has_zeta != 0", who);
        OCN_REQUIRE(sub->out != c, "%s: the output must not alias the input", who);
    }
    OCN_REQUIRE(!kappa_e || terms->closure == 2, "kappa_e is only meaningful with closure == 2");
    TracerFuse tf;
    OCN_TRY(make_tracer_fuse(grid, terms, kappa, kappa_e, bcs_c, sub, sc, tf));
    const ocn::ForcingDev fd = ocn::to_dev(forcing);
    const bool forced = fd.n > 0, periodic = xy_periodic(grid);
    hipStream_t s = as_stream(stream);
    // ONE call: the substep, F (unless the kernel is the Periodic grids' Centered(order=2) one, which has no epilogue) or -- walls in x / y,
    // where the interior box adds advection and diffusion before its store -- the diffusion alone ride along
    if (sub || (forced ? !(periodic && terms->advection == OCN_ADVECTION_CENTERED2) : (!periodic && terms->closure)))
        return launch_advective_tracer(terms->advection, grid, u, v, w, c, Gc, range, s, &tf, forced ? &fd : nullptr);
    int st = launch_advective_tracer(terms->advection, grid, u, v, w, c, Gc, range, s, nullptr);
    if (st == OCN_SUCCESS && terms->closure) st = OCN_LAUNCH(grid, launch_tracer_diffusion, grid, kappa, kappa_e, c, Gc, range, s);
    if (st == OCN_SUCCESS && forced) st = OCN_LAUNCH(grid, launch_tracer_forcing, grid, fd, c, Gc, range, nullptr, s);
    return st;
}

int ocn_compute_tracer_tendency_terms(const ocn_grid *grid, const ocn_model_terms *terms, double kappa, const double *kappa_e,
                                      const double *u, const double *v, const double *w, const double *c, double *Gc,
                                      const int32_t *range, void *stream)
{
    return tracer_tendency_terms(__func__, grid, terms, kappa, kappa_e, nullptr, nullptr, u, v, w, c, Gc, nullptr, SubstepCoef{}, range, stream);
}

int ocn_compute_tracer_tendency_terms_forced(const ocn_grid *grid, const ocn_model_terms *terms, double kappa, const double *kappa_e,
                                             const ocn_forcing *forcing, const double *u, const double *v, const double *w, const double *c,
                                             double *Gc, const int32_t *range, void *stream)
{
    return tracer_tendency_terms(__func__, grid, terms, kappa, kappa_e, forcing, nullptr, u, v, w, c, Gc, nullptr, SubstepCoef{}, range, stream);
}

int ocn_compute_tracer_tendency_terms_rk3(const ocn_grid *grid, const ocn_model_terms *terms, double kappa, const double *kappa_e,
                                          const ocn_field_bcs *bcs_c, const double *u, const double *v, const double *w,
                                          const double *c, double *Gc, const double *Gmc, double *c_out, double dt, double gamma,
                                          double zeta, int32_t has_zeta, const int32_t *range, void *stream)
{
    const SubstepDev sub{Gmc, c_out};
    return tracer_tendency_terms(__func__, grid, terms, kappa, kappa_e, nullptr, bcs_c, u, v, w, c, Gc, &sub,
                                 SubstepCoef{dt, gamma, zeta, 1, has_zeta ? 1 : 0}, range, stream);
}

int ocn_compute_tracer_tendency_terms_rk3_forced(const ocn_grid *grid, const ocn_model_terms *terms, double kappa, const double *kappa_e,
                                                 const ocn_forcing *forcing, const ocn_field_bcs *bcs_c, const double *u, const double *v,
                                                 const double *w, const double *c, double *Gc, const double *Gmc, double *c_out, double dt,
                                                 double gamma, double zeta, int32_t has_zeta, const int32_t *range, void *stream)
{
    const SubstepDev sub{Gmc, c_out};
    return tracer_tendency_terms(__func__, grid, terms, kappa, kappa_e, forcing, bcs_c, u, v, w, c, Gc, &sub,
                                 SubstepCoef{dt, gamma, zeta, 1, has_zeta ? 1 : 0}, range, stream);  // ONE launch, as without forcing
}

int ocn_compute_tracer_pair_tendency_terms_rk3(const ocn_grid *grid, const ocn_model_terms *terms, const double *kappa, const double *const *kappa_e,
                                               const ocn_field_bcs *const *bcs_c, const double *u, const double *v, const double *w,
                                               const double *const *c, double *const *Gc, const double *const *Gc_previous, double *const *c_out,
                                               double dt, double gamma, double zeta, int32_t has_zeta, const int32_t *range,
                                               int32_t *launched, void *stream)
{
    OCN_TRY(validate_terms(grid, terms));
    OCN_REQUIRE(launched, "ocn_compute_tracer_pair_tendency_terms_rk3: launched is NULL");
    *launched = 0;
    if (!xy_periodic(grid)) return OCN_SUCCESS;  // walls in x / y: one tracer per launch (ocn_compute_tracer_tendency_terms_rk3)
    OCN_REQUIRE(terms->advection != OCN_ADVECTION_CENTERED2, "ocn_compute_tracer_pair_tendency_terms_rk3: advection must be WENO5 or UpwindBiased5");
    OCN_REQUIRE(u && v && w && c && Gc && c_out && kappa, "ocn_compute_tracer_pair_tendency_terms_rk3: null pointer");
    TracerFuse tf[2];
    for (int t = 0; t < 2; ++t) {
        OCN_REQUIRE(c[t] && Gc[t] && c_out[t] && c_out[t] != c[t], "ocn_compute_tracer_pair_tendency_terms_rk3: null or aliased field pointer");
        OCN_REQUIRE(!has_zeta || (Gc_previous && Gc_previous[t]), "ocn_compute_tracer_pair_tendency_terms_rk3: G⁻ is required when has_zeta != 0");
        OCN_REQUIRE(!(kappa_e && kappa_e[t]) || terms->closure == 2, "kappa_e is only meaningful with closure == 2");
        const SubstepDev sub{Gc_previous ? Gc_previous[t] : nullptr, c_out[t]};
        OCN_TRY(make_tracer_fuse(grid, terms, kappa[t], kappa_e ? kappa_e[t] : nullptr, bcs_c ? bcs_c[t] : nullptr, &sub,
                                 SubstepCoef{dt, gamma, zeta, 1, has_zeta ? 1 : 0}, tf[t]));
    }
    int did = 0;
    const int st = OCN_LAUNCH_SCHEME(grid, terms->advection, launch_tracer_pair_tendency, grid, u, v, w, c, Gc, range, as_stream(stream), tf, &did);
    *launched = did;
    return st;
}

int ocn_split_explicit_substeps_blocked(const ocn_grid *grid, int32_t n, const double *weights, double dtau, double gravitational_acceleration,
                                        double column_depth, double *eta, double *U, double *V, double *eta_filtered, double *U_filtered,
                                        double *V_filtered, const double *GU, const double *GV, double *work, void *stream)
{
    OCN_TRY(validate_hydrostatic(grid, "ocn_split_explicit_substeps_blocked"));
    OCN_REQUIRE_PERIODIC_X("ocn_split_explicit_substeps_blocked");
    OCN_REQUIRE(n >= 1 && weights, "ocn_split_explicit_substeps_blocked: needs n >= 1 averaging weights (host array)");
    OCN_REQUIRE(eta && U && V && eta_filtered && U_filtered && V_filtered && GU && GV && work, "ocn_split_explicit_substeps_blocked: null pointer");
    return launch_split_explicit_substeps_blocked(grid, n, weights, dtau, gravitational_acceleration, column_depth, eta, U, V, eta_filtered,
                                                  U_filtered, V_filtered, GU, GV, work, as_stream(stream));
}

int ocn_implicit_free_surface_rhs(const ocn_grid *grid, const double *u, const double *v, const double *eta, double gravitational_acceleration,
                                  double dt, double *Qu, double *Qv, double *rhs, void *stream)
{
    OCN_TRY(validate_hydrostatic(grid, "ocn_implicit_free_surface_rhs", true));
    OCN_REQUIRE(grid->tx != OCN_FULLY_CONNECTED, "ocn_implicit_free_surface_rhs wraps x periodically: not for a partitioned (FullyConnected) x");
    OCN_REQUIRE(u && v && eta && Qu && Qv && rhs, "ocn_implicit_free_surface_rhs: null pointer");
    OCN_REQUIRE(dt > 0, "ocn_implicit_free_surface_rhs: dt must be positive");
    return launch_implicit_free_surface_rhs(grid, u, v, eta, gravitational_acceleration, dt, Qu, Qv, rhs, as_stream(stream));
}
int ocn_barotropic_pressure_correction(const ocn_grid *grid, double *u, double *v, const double *eta, double gravitational_acceleration,
                                       double dt, void *stream)
{
    OCN_TRY(validate_hydrostatic(grid, "ocn_barotropic_pressure_correction", true));
    OCN_REQUIRE(u && v && eta, "ocn_barotropic_pressure_correction: null pointer");
    return launch_barotropic_pressure_correction(grid, u, v, eta, gravitational_acceleration, dt, as_stream(stream));
}

int ocn_split_explicit_substeps_ab3(const ocn_grid *grid, int32_t n, const double *weights, double dtau, double gravitational_acceleration,
                                    double column_depth, const double *coefficients, double *eta, double *U, double *V, double *eta_filtered,
                                    double *U_filtered, double *V_filtered, const double *GU, const double *GV, double *work, void *stream)
{
    OCN_TRY(validate_hydrostatic(grid, "ocn_split_explicit_substeps_ab3"));
    OCN_REQUIRE_PERIODIC_X("ocn_split_explicit_substeps_ab3");
    OCN_REQUIRE(n >= 1 && weights && coefficients, "ocn_split_explicit_substeps_ab3: needs n >= 1 weights and the 7 AB3 coefficients (host arrays)");
    OCN_REQUIRE(eta && U && V && eta_filtered && U_filtered && V_filtered && GU && GV && work, "ocn_split_explicit_substeps_ab3: null pointer");
    return launch_split_explicit_substeps_ab3(grid, n, weights, dtau, gravitational_acceleration, column_depth, coefficients, eta, U, V,
                                              eta_filtered, U_filtered, V_filtered, GU, GV, work, as_stream(stream));
}

static int validate_hydrostatic_slab(const ocn_grid *grid, const char *who)
{
    OCN_TRY(validate_grid(grid));
    OCN_REQUIRE((grid->tx == OCN_PERIODIC || grid->tx == OCN_FULLY_CONNECTED) && grid->ty == OCN_PERIODIC && grid->tz == OCN_BOUNDED,
                "%s: (Periodic | FullyConnected, Periodic, Bounded) grids", who);
    return OCN_SUCCESS;
}
int ocn_split_explicit_dist_begin(const ocn_grid *grid, int32_t n, const double *eta, const double *U, const double *V, const double *GU,
                                  const double *GV, double *work, double *send_west, double *send_east, void *stream)
{
    OCN_TRY(validate_hydrostatic_slab(grid, "ocn_split_explicit_dist_begin"));
    OCN_REQUIRE(n >= 1 && n <= grid->Nx, "ocn_split_explicit_dist_begin: the number of substeps (%d) must not exceed the slab's Nx (%d): the extended halo "
                "would reach past the neighbouring rank", n, grid->Nx);
    OCN_REQUIRE(eta && U && V && GU && GV && work && send_west && send_east, "ocn_split_explicit_dist_begin: null pointer");
    return launch_split_explicit_dist_begin(grid, n, eta, U, V, GU, GV, work, send_west, send_east, as_stream(stream));
}
int ocn_split_explicit_dist_run(const ocn_grid *grid, int32_t n, const double *weights, double dtau, double gravitational_acceleration,
                                double column_depth, double *eta, double *U, double *V, double *work, const double *recv_west,
                                const double *recv_east, void *stream)
{
    OCN_TRY(validate_hydrostatic_slab(grid, "ocn_split_explicit_dist_run"));
    OCN_REQUIRE(n >= 1 && n <= grid->Nx && weights, "ocn_split_explicit_dist_run: needs 1 <= n <= Nx averaging weights (host array)");
    OCN_REQUIRE(eta && U && V && work && recv_west && recv_east, "ocn_split_explicit_dist_run: null pointer");
    return launch_split_explicit_dist_run(grid, n, n, weights, dtau, gravitational_acceleration, column_depth, eta, U, V, work, recv_west,
                                          recv_east, as_stream(stream));
}

int ocn_hydrostatic_momentum_ab2_step(const ocn_grid *grid, const ocn_model_terms *terms, const ocn_field_bcs *bcs_u,
                                      const ocn_field_bcs *bcs_v, const double *u, const double *v, const double *w, double *Gu, double *Gv,
                                      const double *Gu_previous, const double *Gv_previous, double *u_out, double *v_out, double dt,
                                      double chi, int32_t euler, const double *eta, double gravitational_acceleration, double *GU,
                                      double *GV, double *U_star, double *V_star, void *stream)
{
    OCN_TRY(validate_hydrostatic_slab(grid, "ocn_hydrostatic_momentum_ab2_step"));
    OCN_TRY(validate_terms(grid, terms));
    OCN_REQUIRE(grid->Hz >= 1, "ocn_hydrostatic_momentum_ab2_step: needs a z halo");
    OCN_REQUIRE(terms->closure != 2, "ocn_hydrostatic_momentum_ab2_step: eddy-viscosity closures are not supported");
    OCN_REQUIRE(u && v && w && Gu && Gv && u_out && v_out, "ocn_hydrostatic_momentum_ab2_step: null field pointer");
    OCN_REQUIRE(euler || (Gu_previous && Gv_previous), "ocn_hydrostatic_momentum_ab2_step: G_previous is required unless euler != 0");
    OCN_REQUIRE(u_out != u && v_out != v, "ocn_hydrostatic_momentum_ab2_step: the outputs must not alias the inputs");
    OCN_REQUIRE((GU && GV && U_star && V_star) || (!GU && !GV && !U_star && !V_star),
                "ocn_hydrostatic_momentum_ab2_step: GU, GV, U_star, V_star go together (all or none)");
    MomentumFinal mf{};
    OCN_TRY(flux_side(grid, bcs_u, "u", mf.bottom[0], mf.top[0]));
    OCN_TRY(flux_side(grid, bcs_v, "v", mf.bottom[1], mf.top[1]));
    mf.sub[0] = SubstepDev{Gu_previous, u_out};
    mf.sub[1] = SubstepDev{Gv_previous, v_out};
    if (euler) chi = -0.5;
    mf.sc = SubstepCoef{dt, 1.5 + chi, -(0.5 + chi), 1, euler ? 0 : 1};
    ocn::HydroFuse hf{eta, gravitational_acceleration, GU, GV, U_star, V_star};
    TermsDev t = to_dev(*terms);
    return OCN_LAUNCH(grid, launch_hydrostatic_momentum, grid, t, u, v, w, Gu, Gv, mf, hf, as_stream(stream));
}

int ocn_barotropic_corrector_and_w(const ocn_grid *grid, const double *u_star, const double *v_star, double *u, double *v, double *w,
                                   const double *U, const double *V, const double *U_star, const double *V_star, double column_depth,
                                   void *stream)
{
    OCN_TRY(validate_hydrostatic(grid, "ocn_barotropic_corrector_and_w"));
    OCN_REQUIRE(u_star && v_star && u && v && w, "ocn_barotropic_corrector_and_w: null field pointer");
    OCN_REQUIRE(u != u_star && v != v_star, "ocn_barotropic_corrector_and_w: the outputs must not alias the inputs");
    OCN_REQUIRE((U && V && U_star && V_star) || (!U && !V), "ocn_barotropic_corrector_and_w: U, V, U_star, V_star go together");
    return launch_barotropic_correct_w(grid, u_star, v_star, u, v, w, U, V, U_star, V_star, column_depth, as_stream(stream));
}

int ocn_fill_halo_regions_bcs(const ocn_grid *grid, double *const *fields, const int32_t *locs,
                              const ocn_field_bcs *const *bcs, int32_t n, int32_t fill_boundary_normal_velocities,
                              void *stream)
{
    OCN_TRY(validate_grid_any(grid));
    FieldTuple ft;
    OCN_TRY(make_field_tuple(grid, fields, locs, n, ft));
    if (!xy_periodic(grid)) {  // every side may carry a condition (fill_halo_regions_value_gradient.jl for west / east / south / north too)
        SideBcTuple sb{};
        bool any = false;
        const int T[3] = {grid->tx, grid->ty, grid->tz};
        for (int f = 0; f < n; ++f) {
            if (!bcs || !bcs[f]) continue;
            const ocn_bc *side[6] = {&bcs[f]->west, &bcs[f]->east, &bcs[f]->south, &bcs[f]->north, &bcs[f]->bottom, &bcs[f]->top};
            for (int q = 0; q < 6; ++q) {
                const ocn_bc &c = *side[q];
                OCN_REQUIRE(c.kind >= OCN_BC_DEFAULT && c.kind <= OCN_BC_OPEN, "field %d: unknown boundary condition kind %d", f, c.kind);
                if (c.kind == OCN_BC_DEFAULT) continue;
                if (q < 2 && partitioned_x(grid) && !(q == 0 ? x_wall_west(*grid) : x_wall_east(*grid))) continue;  // another slab's wall
                OCN_REQUIRE(side_has_wall(grid, q), "field %d: a boundary condition on side %d needs a Bounded direction (topology %d)", f, q, T[q / 2]);
                OCN_REQUIRE((((locs[f] >> (q / 2)) & 1) != 0) == (c.kind == OCN_BC_OPEN),
                            "field %d: the wall-normal velocity takes an Open condition (its value on the boundary face), the other fields Flux / Value / Gradient", f);
                sb.side[q][f] = ZBc{c.kind, c.value, c.coeff, c.values};
                any = true;
            }
        }
        return launch_fill_halos_general(grid, ft, fill_boundary_normal_velocities, as_stream(stream), any ? &sb : nullptr);
    }
    ZBcTuple z;
    bool any;
    OCN_TRY(make_zbc_tuple(grid, locs, bcs, n, z, false, any));
    return launch_fill_halos(grid, ft, fill_boundary_normal_velocities, -1, as_stream(stream), any ? &z : nullptr);
}

int ocn_apply_flux_bcs(const ocn_grid *grid, double *const *G, const double *const *fields, const int32_t *locs,
                       const ocn_field_bcs *const *bcs, int32_t n, void *stream)
{
    OCN_TRY(validate_grid_any(grid));
    FieldTuple gt, ft;
    OCN_TRY(make_field_tuple(grid, G, locs, n, gt));
    OCN_TRY(make_field_tuple(grid, const_cast<double *const *>(fields), locs, n, ft));
    if (!xy_periodic(grid)) {  // apply_x_bcs!, apply_y_bcs!, then apply_z_bcs! (compute_nonhydrostatic_tendencies.jl:204-213)
        SideBcTuple sb{};
        ZBcTuple z{};
        bool any_xy = false, any_z = false;
        const int T[3] = {grid->tx, grid->ty, grid->tz};
        for (int f = 0; f < n; ++f) {
            if (!bcs || !bcs[f]) continue;
            const ocn_bc *side[6] = {&bcs[f]->west, &bcs[f]->east, &bcs[f]->south, &bcs[f]->north, &bcs[f]->bottom, &bcs[f]->top};
            for (int q = 0; q < 6; ++q) {
                const ocn_bc &c = *side[q];
                OCN_REQUIRE(c.kind >= OCN_BC_DEFAULT && c.kind <= OCN_BC_OPEN, "field %d: unknown boundary condition kind %d", f, c.kind);
                if (c.kind != OCN_BC_FLUX) continue;
                if (q < 2 && partitioned_x(grid) && !(q == 0 ? x_wall_west(*grid) : x_wall_east(*grid))) continue;  // another slab's wall
                OCN_REQUIRE(side_has_wall(grid, q), "field %d: a boundary condition on side %d needs a Bounded direction (topology %d)", f, q, T[q / 2]);
                OCN_REQUIRE(!((locs[f] >> (q / 2)) & 1), "field %d: the wall-normal velocity keeps its impenetrable condition", f);
                if (q < 4) {
                    sb.side[q][f] = ZBc{c.kind, c.value, c.coeff, c.values};
                    any_xy = true;
                } else {
                    (q == 4 ? z.bottom[f] : z.top[f]) = ZBc{c.kind, c.value, c.coeff, c.values};
                    any_z = true;
                }
            }
        }
        if (any_xy) {
            OCN_TRY(launch_apply_flux_bcs_lateral(grid, gt, ft, sb, as_stream(stream)));
        }
        return any_z ? launch_apply_flux_bcs(grid, gt, ft, z, as_stream(stream)) : OCN_SUCCESS;
    }
    ZBcTuple z;
    bool any;
    OCN_TRY(make_zbc_tuple(grid, locs, bcs, n, z, true, any));
    if (!any) return OCN_SUCCESS;
    return launch_apply_flux_bcs(grid, gt, ft, z, as_stream(stream));
}

int ocn_compute_tracer_tendency(const ocn_grid *grid, const double *u, const double *v, const double *w, const double *c,
                                double *Gc, const int32_t *range, void *stream)
{
    OCN_TRY(validate_weno(grid));
    OCN_REQUIRE(u && v && w && c && Gc, "ocn_compute_tracer_tendency: null field pointer");
    if (!xy_periodic(grid)) return OCN_LAUNCH(grid, launch_tracer_tendency_general, grid, 0, u, v, w, c, Gc, range, as_stream(stream));
    return OCN_LAUNCH(grid, launch_tracer_tendency, grid, u, v, w, c, Gc, range, as_stream(stream));
}

static int make_step_tuple(int32_t n, double *const *U, const double *const *Gn, double *const *Gm, const int32_t *locs,
                           bool needU, StepTuple &t)
{
    OCN_REQUIRE(n >= 1 && n <= MAX_TUPLE, "number of fields %d outside 1..%d", n, MAX_TUPLE);
    OCN_REQUIRE(Gn && Gm && locs && (U || !needU), "null tuple pointer");
    t.n = n;
    for (int f = 0; f < n; ++f) {
        OCN_REQUIRE(Gn[f] && Gm[f] && (!needU || U[f]), "field %d: null pointer", f);
        t.U[f] = needU ? U[f] : nullptr;
        t.Gn[f] = Gn[f];
        t.Gm[f] = Gm[f];
        t.loc[f] = locs[f];
    }
    return OCN_SUCCESS;
}

int ocn_rk3_substep(const ocn_grid *grid, int32_t n, double *const *U, const double *const *Gn, const double *const *Gm,
                    const int32_t *locs, double dt, double gamma, double zeta, int32_t has_zeta, void *stream)
{
    OCN_TRY(validate_grid_any(grid));
    StepTuple t;
    OCN_TRY(make_step_tuple(n, U, Gn, const_cast<double *const *>(reinterpret_cast<const double *const *>(Gm)), locs, true, t));
    return launch_stepper(grid, t, has_zeta ? 1 : 0, dt, gamma, zeta, as_stream(stream));
}

int ocn_split_rk3_substep(const ocn_grid *grid, int32_t n, double *const *U, const double *const *G, const double *const *Psi,
                          const int32_t *locs, double dt, double gamma, double zeta, void *stream)
{
    OCN_TRY(validate_grid_any(grid));
    StepTuple t;
    OCN_TRY(make_step_tuple(n, U, G, const_cast<double *const *>(reinterpret_cast<const double *const *>(Psi)), locs, true, t));
    for (int f = 0; f < n; ++f) OCN_REQUIRE(Psi[f] != U[f], "ocn_split_rk3_substep: field %d: Psi must not alias U", f);
    return launch_stepper(grid, t, 4, dt, gamma, zeta, as_stream(stream));
}

int ocn_ab2_step(const ocn_grid *grid, int32_t n, double *const *U, const double *const *Gn, const double *const *Gm,
                 const int32_t *locs, double dt, double chi, void *stream)
{
    OCN_TRY(validate_grid_any(grid));
    StepTuple t;
    OCN_TRY(make_step_tuple(n, U, Gn, const_cast<double *const *>(reinterpret_cast<const double *const *>(Gm)), locs, true, t));
    const double not_euler = (chi != -0.5) ? 1.0 : 0.0;
    return launch_stepper(grid, t, 2, dt, chi, not_euler, as_stream(stream));
}

static int validate_vertically_implicit(const ocn_grid *grid, const char *who)
{
    OCN_TRY(validate_grid_any(grid));
    OCN_REQUIRE(grid->tz == OCN_BOUNDED, "%s: VerticallyImplicitTimeDiscretization can only be specified on grids that are Bounded in the z-direction.", who);
    OCN_REQUIRE((grid->tx == OCN_FLAT || grid->Hx >= 1) && (grid->ty == OCN_FLAT || grid->Hy >= 1) && grid->Hz >= 1, "%s: halo >= 1 required", who);
    return OCN_SUCCESS;
}

int ocn_add_vertically_implicit_explicit_fluxes(const ocn_grid *grid, double nu, const double *u, const double *v, const double *w, double *Gu,
                                                double *Gv, double *Gw, int32_t n_tracers, const double *kappa, const double *const *c,
                                                double *const *Gc, const int32_t *range, void *stream)
{
    const char *who = "ocn_add_vertically_implicit_explicit_fluxes";
    OCN_TRY(validate_vertically_implicit(grid, who));
    OCN_REQUIRE(n_tracers >= 0 && n_tracers <= MAX_TUPLE, "%s: number of tracers %d outside 0..%d", who, n_tracers, MAX_TUPLE);
    if (u) {
        OCN_REQUIRE(v && w && Gu && Gv, "%s: null field pointer (u is given: v, w, Gu, Gv are needed; Gw may be NULL)", who);
        OCN_REQUIRE(std::isfinite(nu) && nu >= 0, "%s: nu = %g must be finite and >= 0", who, nu);
    } else {
        OCN_REQUIRE(!v && !w && !Gu && !Gv && !Gw, "%s: u is NULL (no momentum part) but another momentum pointer is not", who);
        OCN_REQUIRE(n_tracers >= 1, "%s: nothing to do (u is NULL and n_tracers is 0)", who);
    }
    if (n_tracers) OCN_REQUIRE(kappa && c && Gc, "%s: null tracer array", who);
    for (int n = 0; n < n_tracers; ++n) {
        OCN_REQUIRE(c[n] && Gc[n], "%s: tracer %d: null pointer", who, n);
        OCN_REQUIRE(std::isfinite(kappa[n]) && kappa[n] >= 0, "%s: tracer %d: kappa = %g must be finite and >= 0", who, n, kappa[n]);
    }
    return launch_ivd_explicit_part(grid, nu, u, v, w, Gu, Gv, Gw, n_tracers, kappa, c, Gc, range, as_stream(stream));
}

int ocn_implicit_vertical_diffusion_step(const ocn_grid *grid, int32_t n, double *const *fields, const int32_t *locs, const double *kappa,
                                         double dt, void *stream)
{
    const char *who = "ocn_implicit_vertical_diffusion_step";
    OCN_TRY(validate_vertically_implicit(grid, who));
    OCN_REQUIRE(n >= 1 && n <= MAX_TUPLE, "%s: number of fields %d outside 1..%d", who, n, MAX_TUPLE);
    OCN_REQUIRE(fields && locs && kappa, "%s: null tuple pointer", who);
    OCN_REQUIRE(grid->Nz <= 2048, "%s: Nz = %d > 2048 (the multipliers of a column are kept in LDS)", who, grid->Nz);
    OCN_REQUIRE(std::isfinite(dt) && dt >= 0, "%s: dt = %g must be finite and >= 0", who, dt);
    for (int f = 0; f < n; ++f) {
        OCN_REQUIRE(fields[f] != nullptr, "%s: field %d: null pointer", who, f);
        OCN_REQUIRE(locs[f] == OCN_LOC_CCC || locs[f] == OCN_LOC_FCC || locs[f] == OCN_LOC_CFC || locs[f] == OCN_LOC_CCF,
                    "%s: field %d: location %d is none of ccc, fcc, cfc, ccf", who, f, locs[f]);
        OCN_REQUIRE(std::isfinite(kappa[f]) && kappa[f] >= 0, "%s: field %d: kappa = %g must be finite and >= 0", who, f, kappa[f]);
        for (int q = 0; q < f; ++q) OCN_REQUIRE(fields[q] != fields[f], "%s: fields %d and %d are the same array", who, q, f);
    }
    return launch_ivd_implicit_step(grid, n, fields, locs, kappa, dt, as_stream(stream));
}

// the three entry points of vertical_diffusivity.hip: a Bounded z, and the x / y neighbours of a κ field are read
static int validate_vertical_diffusivity(const ocn_grid *grid, const char *who)
{
    OCN_TRY(validate_grid_any(grid));
    OCN_REQUIRE(grid->tz == OCN_BOUNDED, "%s: needs a grid that is Bounded in the z-direction", who);
    OCN_REQUIRE(grid->tx != OCN_FLAT && grid->ty != OCN_FLAT, "%s: a Flat x or y is not implemented", who);
    OCN_REQUIRE(grid->Hx >= 1 && grid->Hy >= 1 && grid->Hz >= 1, "%s: halo >= 1 required", who);
    return OCN_SUCCESS;
}

int ocn_compute_convective_adjustment_diffusivities(const ocn_grid *grid, const ocn_model_terms *terms,
                                                    const ocn_convective_adjustment *closure, double *kappa_c, double *kappa_u, void *stream)
{
    const char *who = "ocn_compute_convective_adjustment_diffusivities";
    OCN_TRY(validate_vertical_diffusivity(grid, who));
    OCN_REQUIRE(terms && closure, "%s: null terms / closure", who);
    OCN_REQUIRE(kappa_c && kappa_u, "%s: null field pointer", who);
    OCN_REQUIRE(kappa_c != kappa_u, "%s: kappa_c and kappa_u are the same array", who);
    OCN_TRY(validate_buoyancy_terms(terms, who));
    OCN_REQUIRE(std::isfinite(closure->convective_kappa_z) && std::isfinite(closure->convective_nu_z) &&
                    std::isfinite(closure->background_kappa_z) && std::isfinite(closure->background_nu_z),
                "%s: the four coefficients must be finite", who);
    return launch_convective_adjustment_diffusivities(grid, terms, closure, kappa_c, kappa_u, as_stream(stream));
}

int ocn_add_vertical_diffusivity_fluxes(const ocn_grid *grid, const double *kappa_u, const double *u, const double *v, double *Gu, double *Gv,
                                        int32_t n_tracers, const double *const *kappa_c, const double *const *c, double *const *Gc,
                                        int32_t boundary_only, const int32_t *range, void *stream)
{
    const char *who = "ocn_add_vertical_diffusivity_fluxes";
    OCN_TRY(validate_vertical_diffusivity(grid, who));
    OCN_REQUIRE(n_tracers >= 0 && n_tracers <= MAX_TUPLE, "%s: number of tracers %d outside 0..%d", who, n_tracers, MAX_TUPLE);
    if (u) {
        OCN_REQUIRE(kappa_u && v && Gu && Gv, "%s: null field pointer (u is given: kappa_u, v, Gu, Gv are needed)", who);
    } else {
        OCN_REQUIRE(!kappa_u && !v && !Gu && !Gv, "%s: u is NULL (no momentum part) but another momentum pointer is not", who);
        OCN_REQUIRE(n_tracers >= 1, "%s: nothing to do (u is NULL and n_tracers is 0)", who);
    }
    if (n_tracers) OCN_REQUIRE(kappa_c && c && Gc, "%s: null tracer array", who);
    for (int n = 0; n < n_tracers; ++n) OCN_REQUIRE(kappa_c[n] && c[n] && Gc[n], "%s: tracer %d: null pointer", who, n);
    return launch_vertical_diffusivity_fluxes(grid, kappa_u, u, v, Gu, Gv, n_tracers, kappa_c, c, Gc, boundary_only != 0, range,
                                              as_stream(stream));
}

int ocn_implicit_vertical_diffusion_step_fields(const ocn_grid *grid, int32_t n, double *const *fields, const int32_t *locs,
                                                const double *const *kappa, double *const *scratch, double dt, void *stream)
{
    const char *who = "ocn_implicit_vertical_diffusion_step_fields";
    OCN_TRY(validate_vertical_diffusivity(grid, who));
    OCN_REQUIRE(n >= 1 && n <= MAX_TUPLE, "%s: number of fields %d outside 1..%d", who, n, MAX_TUPLE);
    OCN_REQUIRE(fields && locs && kappa && scratch, "%s: null tuple pointer", who);
    OCN_REQUIRE(std::isfinite(dt) && dt >= 0, "%s: dt = %g must be finite and >= 0", who, dt);
    for (int f = 0; f < n; ++f) {
        OCN_REQUIRE(fields[f] != nullptr && kappa[f] != nullptr, "%s: field %d: null pointer", who, f);
        OCN_REQUIRE(locs[f] == OCN_LOC_CCC || locs[f] == OCN_LOC_FCC || locs[f] == OCN_LOC_CFC,
                    "%s: field %d: location %d is none of ccc, fcc, cfc (Face-in-z fields have no implicit step here)", who, f, locs[f]);
        for (int q = 0; q < f; ++q) OCN_REQUIRE(fields[q] != fields[f], "%s: fields %d and %d are the same array", who, q, f);
    }
    return launch_ivd_implicit_step_fields(grid, n, fields, locs, kappa, scratch, dt, as_stream(stream));
}

// biharmonic.hip: everything is checked on the host before the first HIP call
int ocn_add_biharmonic_fluxes(const ocn_grid *grid, double nu, const double *u, const double *v, double *Gu, double *Gv, int32_t n_tracers,
                              const double *kappa, const double *const *c, double *const *Gc, const double *neg_other_u,
                              const double *neg_other_v, const double *const *neg_other_c, void *stream)
{
    const char *who = "ocn_add_biharmonic_fluxes";
    OCN_TRY(validate_grid_any(grid));
    OCN_REQUIRE(grid->tx == OCN_PERIODIC && grid->ty == OCN_PERIODIC,
                "%s: x and y must be Periodic, got topology (%d, %d, %d) (the biharmonic masks of a wall are not implemented)", who, grid->tx,
                grid->ty, grid->tz);
    OCN_REQUIRE(grid->Hx >= 2 && grid->Hy >= 2, "%s: halo >= 2 required in x and y, got (%d, %d)", who, grid->Hx, grid->Hy);
    OCN_REQUIRE(n_tracers >= 0 && n_tracers <= OCN_MODEL_MAX_TRACERS, "%s: number of tracers %d outside 0..%d", who, n_tracers,
                OCN_MODEL_MAX_TRACERS);
    const void *seen[4 + 3 * OCN_MODEL_MAX_TRACERS];  // every array of the call, to refuse aliases
    int n_seen = 0;
    if (u) {
        OCN_REQUIRE(v && Gu && Gv, "%s: null field pointer (u is given: v, Gu, Gv are needed)", who);
        OCN_REQUIRE(std::isfinite(nu) && nu >= 0, "%s: nu = %g must be finite and >= 0", who, nu);
        OCN_REQUIRE(u != v, "%s: u and v are the same array", who);
        seen[n_seen++] = Gu;
        seen[n_seen++] = Gv;
        if (neg_other_u) seen[n_seen++] = neg_other_u;
        if (neg_other_v) seen[n_seen++] = neg_other_v;
    } else {
        OCN_REQUIRE(!v && !Gu && !Gv && !neg_other_u && !neg_other_v, "%s: u is NULL (no momentum part) but another momentum pointer is not", who);
        OCN_REQUIRE(n_tracers >= 1, "%s: nothing to do (u is NULL and n_tracers is 0)", who);
    }
    if (n_tracers) OCN_REQUIRE(kappa && c && Gc, "%s: null tracer array", who);
    for (int n = 0; n < n_tracers; ++n) {
        OCN_REQUIRE(c[n] && Gc[n], "%s: tracer %d: null pointer", who, n);
        OCN_REQUIRE(std::isfinite(kappa[n]) && kappa[n] >= 0, "%s: tracer %d: kappa = %g must be finite and >= 0", who, n, kappa[n]);
        seen[n_seen++] = Gc[n];
        if (neg_other_c && neg_other_c[n]) seen[n_seen++] = neg_other_c[n];
    }
    for (int q = 0; q < n_seen; ++q) {
        OCN_REQUIRE(!u || (seen[q] != u && seen[q] != v), "%s: a tendency or neg_other array is u or v", who);
        for (int n = 0; n < n_tracers; ++n) OCN_REQUIRE(seen[q] != c[n], "%s: a tendency or neg_other array is tracer %d", who, n);
    }
    for (int q = 0; q < n_seen; ++q)
        for (int p = 0; p < q; ++p) OCN_REQUIRE(seen[p] != seen[q], "%s: two of the tendency / neg_other arrays are the same array", who);
    return launch_biharmonic_fluxes(grid, nu, u, v, Gu, Gv, n_tracers, kappa, c, Gc, neg_other_u, neg_other_v, neg_other_c, as_stream(stream));
}

// the three entry points of ri_based_diffusivity.hip
// isopycnal.hip: everything is checked on the host before the first HIP call
static int validate_isopycnal(const ocn_grid *grid, const ocn_model_terms *terms, const ocn_isopycnal *closure, const char *who)
{
    OCN_TRY(validate_grid_any(grid));
    OCN_REQUIRE(grid->tx == OCN_PERIODIC && grid->ty == OCN_PERIODIC && grid->tz == OCN_BOUNDED,
                "%s: the grid must be (Periodic, Periodic, Bounded), got topology (%d, %d, %d)", who, grid->tx, grid->ty, grid->tz);
    OCN_REQUIRE(grid->Hx >= 1 && grid->Hy >= 1 && grid->Hz >= 1, "%s: halo >= 1 required", who);
    OCN_TRY(validate_buoyancy_terms(terms, who));
    OCN_REQUIRE(closure, "%s: null closure", who);
    OCN_REQUIRE(std::isfinite(closure->max_slope) && closure->max_slope > 0, "%s: max_slope = %g must be finite and > 0", who, closure->max_slope);
    OCN_REQUIRE(!std::isnan(closure->minimum_bz), "%s: minimum_bz is a NaN", who);
    return OCN_SUCCESS;
}

int ocn_compute_isopycnal_diffusivities(const ocn_grid *grid, const ocn_model_terms *terms, const ocn_isopycnal *closure, double kappa_skew,
                                        double *eps_R33, double *ue, double *ve, double *we, int32_t n_kz, const double *kappa_symmetric,
                                        double *const *kz, void *stream)
{
    const char *who = "ocn_compute_isopycnal_diffusivities";
    OCN_TRY(validate_isopycnal(grid, terms, closure, who));
    OCN_REQUIRE(eps_R33, "%s: eps_R33 is NULL", who);
    OCN_REQUIRE(n_kz >= 0 && n_kz <= OCN_MODEL_MAX_TRACERS, "%s: n_kz = %d outside 0..%d", who, n_kz, OCN_MODEL_MAX_TRACERS);
    if (n_kz) OCN_REQUIRE(kappa_symmetric && kz, "%s: null kappa_symmetric / kz array", who);
    const void *out[4 + OCN_MODEL_MAX_TRACERS];
    int n_out = 0;
    out[n_out++] = eps_R33;
    if (ue) {
        OCN_REQUIRE(ve && we, "%s: ue is given: ve and we are needed", who);
        OCN_REQUIRE(std::isfinite(kappa_skew), "%s: kappa_skew = %g must be finite", who, kappa_skew);
        out[n_out++] = ue;
        out[n_out++] = ve;
        out[n_out++] = we;
    } else {
        OCN_REQUIRE(!ve && !we, "%s: ue is NULL (no eddy velocities) but ve or we is not", who);
    }
    for (int q = 0; q < n_kz; ++q) {
        OCN_REQUIRE(kz[q], "%s: kz[%d] is NULL", who, q);
        OCN_REQUIRE(std::isfinite(kappa_symmetric[q]), "%s: kappa_symmetric[%d] = %g must be finite", who, q, kappa_symmetric[q]);
        out[n_out++] = kz[q];
    }
    for (int q = 0; q < n_out; ++q) {
        OCN_REQUIRE(out[q] != terms->T && out[q] != terms->S, "%s: an output array is T or S", who);
        for (int p = 0; p < q; ++p) OCN_REQUIRE(out[p] != out[q], "%s: two of the output arrays are the same array", who);
    }
    return launch_isopycnal_diffusivities(grid, terms, closure, kappa_skew, eps_R33, ue, ve, we, n_kz, kappa_symmetric, kz, as_stream(stream));
}

int ocn_sum_velocities(const ocn_grid *grid, const double *const *a, const double *const *b, double *const *out, void *stream)
{
    const char *who = "ocn_sum_velocities";
    OCN_TRY(validate_grid_any(grid));
    OCN_REQUIRE(a && b && out, "%s: null tuple pointer", who);
    for (int f = 0; f < 3; ++f) OCN_REQUIRE(a[f] && b[f] && out[f], "%s: field %d: null pointer", who, f);
    return launch_sum_velocities(grid, a, b, out, as_stream(stream));
}

int ocn_add_isopycnal_fluxes(const ocn_grid *grid, const ocn_model_terms *terms, const ocn_isopycnal *closure, int32_t n_tracers,
                             const double *kappa_symmetric, const double *kappa_skew, const double *const *c, double *const *Gc, void *stream)
{
    const char *who = "ocn_add_isopycnal_fluxes";
    OCN_TRY(validate_isopycnal(grid, terms, closure, who));
    OCN_REQUIRE(n_tracers >= 1 && n_tracers <= OCN_MODEL_MAX_TRACERS, "%s: number of tracers %d outside 1..%d", who, n_tracers,
                OCN_MODEL_MAX_TRACERS);
    OCN_REQUIRE(kappa_symmetric && kappa_skew && c && Gc, "%s: null tracer array", who);
    for (int n = 0; n < n_tracers; ++n) {
        OCN_REQUIRE(c[n] && Gc[n], "%s: tracer %d: null pointer", who, n);
        OCN_REQUIRE(std::isfinite(kappa_symmetric[n]) && std::isfinite(kappa_skew[n]), "%s: tracer %d: the coefficients must be finite", who, n);
        OCN_REQUIRE(Gc[n] != terms->T && Gc[n] != terms->S, "%s: tendency %d is T or S", who, n);
        for (int m = 0; m < n_tracers; ++m) OCN_REQUIRE(Gc[n] != c[m], "%s: tendency %d is tracer %d", who, n, m);
        for (int m = 0; m < n; ++m) OCN_REQUIRE(Gc[n] != Gc[m], "%s: tendencies %d and %d are the same array", who, m, n);
    }
    return launch_isopycnal_fluxes(grid, terms, closure, n_tracers, kappa_symmetric, kappa_skew, c, Gc, as_stream(stream));
}

static int validate_ri_closure(const ocn_grid *grid, const ocn_ri_based *c, const ocn_bc *top_T, const ocn_bc *top_S, const char *who)
{
    OCN_REQUIRE(c, "%s: null closure", who);
    OCN_REQUIRE(c->tapering >= OCN_RI_TAPER_LINEAR && c->tapering <= OCN_RI_TAPER_TANH, "%s: unknown tapering code %d", who, c->tapering);
    OCN_REQUIRE(c->horizontal_filter == OCN_RI_FILTER_NONE || c->horizontal_filter == OCN_RI_FILTER_FIVE_POINT,
                "%s: unknown horizontal filter code %d", who, c->horizontal_filter);
    OCN_REQUIRE(std::isfinite(c->nu0) && std::isfinite(c->kappa0) && std::isfinite(c->kappa_ca) && std::isfinite(c->C_en) &&
                    std::isfinite(c->C_av) && std::isfinite(c->Ri0) && std::isfinite(c->Ri_delta) &&
                    std::isfinite(c->minimum_entrainment_buoyancy_gradient),
                "%s: the coefficients must be finite (only the two maxima may be +inf)", who);
    OCN_REQUIRE(!std::isnan(c->maximum_diffusivity) && !std::isnan(c->maximum_viscosity), "%s: a maximum is a NaN", who);
    const ocn_bc *tops[2] = {top_T, top_S};
    for (int q = 0; q < 2; ++q) {
        if (!tops[q]) continue;
        OCN_REQUIRE(tops[q]->kind == OCN_BC_DEFAULT || tops[q]->kind == OCN_BC_FLUX,
                    "%s: the top condition of the %s tracer has kind %d: only a Flux (or the default, no flux) is a buoyancy flux", who,
                    q ? "S" : "T (or b)", tops[q]->kind);
        OCN_REQUIRE(!tops[q]->values || grid->tx == OCN_PERIODIC || grid->tx == OCN_BOUNDED,
                    "%s: array boundary conditions are not supported on a partitioned grid", who);
    }
    return OCN_SUCCESS;
}

int ocn_compute_ri_number(const ocn_grid *grid, const ocn_model_terms *terms, const double *u, const double *v, double *Ri, void *stream)
{
    const char *who = "ocn_compute_ri_number";
    OCN_TRY(validate_vertical_diffusivity(grid, who));
    OCN_TRY(validate_buoyancy_terms(terms, who));
    OCN_REQUIRE(u && v && Ri, "%s: null field pointer", who);
    return launch_ri_based(0, grid, terms, nullptr, nullptr, nullptr, u, v, nullptr, Ri, nullptr, nullptr, as_stream(stream));
}

int ocn_compute_ri_based_diffusivities(const ocn_grid *grid, const ocn_model_terms *terms, const ocn_ri_based *closure, const ocn_bc *top_T,
                                       const ocn_bc *top_S, const double *Ri, double *kappa_c, double *kappa_u, void *stream)
{
    const char *who = "ocn_compute_ri_based_diffusivities";
    OCN_TRY(validate_vertical_diffusivity(grid, who));
    OCN_TRY(validate_buoyancy_terms(terms, who));
    OCN_TRY(validate_ri_closure(grid, closure, top_T, top_S, who));
    OCN_REQUIRE(Ri && kappa_c && kappa_u, "%s: null field pointer", who);
    OCN_REQUIRE(kappa_c != kappa_u && Ri != kappa_c && Ri != kappa_u, "%s: Ri, kappa_c and kappa_u must be three different arrays", who);
    return launch_ri_based(1, grid, terms, closure, top_T, top_S, nullptr, nullptr, Ri, nullptr, kappa_c, kappa_u, as_stream(stream));
}

int ocn_compute_ri_based_diffusivities_fused(const ocn_grid *grid, const ocn_model_terms *terms, const ocn_ri_based *closure,
                                             const ocn_bc *top_T, const ocn_bc *top_S, const double *u, const double *v, double *Ri,
                                             double *kappa_c, double *kappa_u, void *stream)
{
    const char *who = "ocn_compute_ri_based_diffusivities_fused";
    OCN_TRY(validate_vertical_diffusivity(grid, who));
    OCN_TRY(validate_buoyancy_terms(terms, who));
    OCN_TRY(validate_ri_closure(grid, closure, top_T, top_S, who));
    OCN_REQUIRE(closure->horizontal_filter == OCN_RI_FILTER_NONE,
                "%s: the horizontal filter reads the neighbours' Ri: ocn_compute_ri_number, a halo fill, ocn_compute_ri_based_diffusivities", who);
    OCN_REQUIRE(u && v && Ri && kappa_c && kappa_u, "%s: null field pointer", who);
    OCN_REQUIRE(kappa_c != kappa_u && Ri != kappa_c && Ri != kappa_u, "%s: Ri, kappa_c and kappa_u must be three different arrays", who);
    return launch_ri_based(2, grid, terms, closure, top_T, top_S, u, v, nullptr, Ri, kappa_c, kappa_u, as_stream(stream));
}

int ocn_ri_taper_host(int32_t kind, int64_t n, const double *x, double x0, double delta, double *out)
{
    OCN_REQUIRE(kind >= OCN_RI_TAPER_LINEAR && kind <= OCN_RI_TAPER_TANH, "ocn_ri_taper_host: unknown tapering code %d", kind);
    OCN_REQUIRE(n >= 0 && (n == 0 || (x && out)), "ocn_ri_taper_host: null array or negative length");
    ri_taper_host(kind, n, x, x0, delta, out);
    return OCN_SUCCESS;
}

int ocn_cache_previous_tendencies(const ocn_grid *grid, int32_t n, double *const *Gm, const double *const *Gn,
                                  const int32_t *locs, void *stream)
{
    OCN_TRY(validate_grid_any(grid));
    StepTuple t;
    OCN_TRY(make_step_tuple(n, nullptr, Gn, Gm, locs, false, t));
    return launch_stepper(grid, t, 3, 0.0, 0.0, 0.0, as_stream(stream));
}

int ocn_pressure_correct_velocities(const ocn_grid *grid, double *u, double *v, double *w, const double *p, double dt, void *stream)
{
    OCN_TRY(validate_grid_any(grid));
    OCN_REQUIRE(u && v && w && p, "ocn_pressure_correct_velocities: null field pointer");
    OCN_REQUIRE((grid->tx == OCN_FLAT || grid->Hx >= 1) && (grid->ty == OCN_FLAT || grid->Hy >= 1) && (grid->tz == OCN_FLAT || grid->Hz >= 1),
                "pressure correction needs halo >= 1");
    return launch_pressure_correct(grid, u, v, w, p, dt, as_stream(stream));
}

int ocn_divergence(const ocn_grid *grid, const double *u, const double *v, const double *w, double *div, void *stream)
{
    OCN_TRY(validate_grid_any(grid));
    OCN_REQUIRE(u && v && w && div, "ocn_divergence: null pointer");
    return launch_source_term(grid, u, v, w, 1.0, SourceOut::Divergence, div, grid->Nx, (long long)grid->Nx * grid->Ny, as_stream(stream));
}

int ocn_batched_tridiagonal_solve_z(int32_t Nx, int32_t Ny, int32_t Nz, const double *a, const double *b, const double *c,
                                    const double *f, double *t, double *phi, void *stream)
{
    OCN_REQUIRE(Nx >= 1 && Ny >= 1 && Nz >= 1, "bad sizes (%d, %d, %d)", Nx, Ny, Nz);
    OCN_REQUIRE(a && b && c && f && t && phi, "ocn_batched_tridiagonal_solve_z: null pointer");
    // (where the pivot is not definitely diagonally dominant the caller's ϕ stays: batched_tridiagonal_solver.jl:224-228)
    return launch_tridiag_z(Nx, Ny, Nz, a, b, c, f, t, phi, as_stream(stream), /*keep_storage=*/1);
}

// XDirection / YDirection of the same solver: a, c of length N - 1 of the tridiagonal direction, the arrays in the same (Nx, Ny, Nz) layout
int ocn_batched_tridiagonal_solve_x(int32_t Nx, int32_t Ny, int32_t Nz, const double *a, const double *b, const double *c,
                                    const double *f, double *t, double *phi, void *stream)
{
    OCN_REQUIRE(Nx >= 1 && Ny >= 1 && Nz >= 1, "bad sizes (%d, %d, %d)", Nx, Ny, Nz);
    OCN_REQUIRE(a && b && c && f && t && phi, "ocn_batched_tridiagonal_solve_x: null pointer");
    return launch_tridiag_x(Nx, (long long)Ny * Nz, a, b, c, f, t, phi, as_stream(stream), /*keep_storage=*/1);
}

int ocn_batched_tridiagonal_solve_y(int32_t Nx, int32_t Ny, int32_t Nz, const double *a, const double *b, const double *c,
                                    const double *f, double *t, double *phi, void *stream)
{
    OCN_REQUIRE(Nx >= 1 && Ny >= 1 && Nz >= 1, "bad sizes (%d, %d, %d)", Nx, Ny, Nz);
    OCN_REQUIRE(a && b && c && f && t && phi, "ocn_batched_tridiagonal_solve_y: null pointer");
    // lanes along x (coalesced), the sweep along y: planes Nx apart, columns (i, k) at i + Nx Ny k
    return launch_tridiag_z_strided(Nx, Nz, (long long)Nx * Ny, Nx, Ny, a, b, c, f, t, phi, as_stream(stream), /*keep_storage=*/1);
}

int ocn_halo_pack_x(const ocn_grid *grid, const double *field, int32_t loc, double *send_west, double *send_east, void *stream)
{
    OCN_TRY(validate_grid_any(grid));
    OCN_REQUIRE(field && send_west && send_east, "ocn_halo_pack_x: null pointer");
    return launch_halo_pack_x(grid, field, loc, send_west, send_east, 0, as_stream(stream));
}
int ocn_halo_unpack_x(const ocn_grid *grid, double *field, int32_t loc, const double *recv_west, const double *recv_east, void *stream)
{
    OCN_TRY(validate_grid_any(grid));
    OCN_REQUIRE(field && recv_west && recv_east, "ocn_halo_unpack_x: null pointer");
    return launch_halo_pack_x(grid, field, loc, const_cast<double *>(recv_west), const_cast<double *>(recv_east), 1, as_stream(stream));
}

int ocn_halo_plane_x(const ocn_grid *grid, double *field, int32_t loc, int32_t which, double *buffer, int32_t unpack, void *stream)
{
    OCN_TRY(validate_grid_any(grid));
    OCN_REQUIRE(field && buffer, "ocn_halo_plane_x: null pointer");
    OCN_REQUIRE(which == 0 || which == 1, "ocn_halo_plane_x: which must be 0 (west) or 1 (east)");
    OCN_REQUIRE(grid->Hx >= 1, "ocn_halo_plane_x: needs an x halo");
    return launch_halo_plane_x(grid, field, loc, which, buffer, unpack ? 1 : 0, as_stream(stream));
}
static int validate_pressure_planes(const ocn_grid *grid, const char *who)
{
    OCN_TRY(validate_grid(grid));
    OCN_REQUIRE(grid->ty == OCN_PERIODIC && grid->tz == OCN_PERIODIC, "%s: y and z must be Periodic", who);
    OCN_REQUIRE(grid->Hx >= 1 && grid->Nx >= grid->Hx + 1, "%s: needs nx >= Hx + 1 (got nx = %d, Hx = %d)", who, grid->Nx, grid->Hx);
    return OCN_SUCCESS;
}
int ocn_halo_pack_pressure(const ocn_grid *grid, const double *p, const double *u, double dt_correct, double *send_west,
                           double *send_east, void *stream)
{
    OCN_TRY(validate_pressure_planes(grid, "ocn_halo_pack_pressure"));
    OCN_REQUIRE(p && u && send_west && send_east, "ocn_halo_pack_pressure: null pointer");
    return OCN_LAUNCH(grid, launch_pressure_planes, grid, const_cast<double *>(p), const_cast<double *>(u), dt_correct, send_west, send_east, 0,
                      as_stream(stream));
}
int ocn_halo_unpack_pressure(const ocn_grid *grid, double *p, double *u, const double *recv_west, const double *recv_east, void *stream)
{
    OCN_TRY(validate_pressure_planes(grid, "ocn_halo_unpack_pressure"));
    OCN_REQUIRE(p && u && recv_west && recv_east, "ocn_halo_unpack_pressure: null pointer");
    return ocn_strict::launch_pressure_planes(grid, p, u, 0.0, const_cast<double *>(recv_west), const_cast<double *>(recv_east), 1, as_stream(stream));
}
int ocn_halo_pack_x_fields(const ocn_grid *grid, double *const *fields, const int32_t *locs, int32_t n, double *send_west,
                           double *send_east, void *stream)
{
    OCN_TRY(validate_grid_any(grid));
    OCN_REQUIRE(send_west && send_east, "ocn_halo_pack_x_fields: null buffer");
    FieldTuple ft;
    OCN_TRY(make_field_tuple(grid, fields, locs, n, ft));
    return launch_halo_pack_x_fields(grid, ft, send_west, send_east, 0, as_stream(stream));
}
int ocn_halo_unpack_x_fields(const ocn_grid *grid, double *const *fields, const int32_t *locs, int32_t n, const double *recv_west,
                             const double *recv_east, void *stream)
{
    OCN_TRY(validate_grid_any(grid));
    OCN_REQUIRE(recv_west && recv_east, "ocn_halo_unpack_x_fields: null buffer");
    FieldTuple ft;
    OCN_TRY(make_field_tuple(grid, fields, locs, n, ft));
    return launch_halo_pack_x_fields(grid, ft, const_cast<double *>(recv_west), const_cast<double *>(recv_east), 1, as_stream(stream));
}

static int check_transpose(int32_t nx, int32_t Ny, int32_t Nz, int32_t R, const void *a, const void *b)
{
    OCN_REQUIRE(nx >= 1 && Ny >= 1 && Nz >= 1 && R >= 1, "bad transpose sizes");
    OCN_REQUIRE(Ny % R == 0, "Ny = %d must be divisible by the number of ranks %d", Ny, R);
    OCN_REQUIRE(a && b, "null transpose buffer");
    return OCN_SUCCESS;
}
int ocn_transpose_pack_y_to_x(int32_t nx, int32_t Ny, int32_t Nz, int32_t R, const double *yfield, double *send, void *stream)
{
    OCN_TRY(check_transpose(nx, Ny, Nz, R, yfield, send));
    return launch_transpose(0, nx, Ny, Nz, R, yfield, send, as_stream(stream));
}
int ocn_transpose_unpack_x_from_y(int32_t nx, int32_t Ny, int32_t Nz, int32_t R, const double *recv, double *xfield, void *stream)
{
    OCN_TRY(check_transpose(nx, Ny, Nz, R, recv, xfield));
    return launch_transpose(1, nx, Ny, Nz, R, recv, xfield, as_stream(stream));
}
int ocn_transpose_pack_x_to_y(int32_t nx, int32_t Ny, int32_t Nz, int32_t R, const double *xfield, double *send, void *stream)
{
    OCN_TRY(check_transpose(nx, Ny, Nz, R, xfield, send));
    return launch_transpose(2, nx, Ny, Nz, R, xfield, send, as_stream(stream));
}
int ocn_transpose_unpack_y_from_x(int32_t nx, int32_t Ny, int32_t Nz, int32_t R, const double *recv, double *yfield, void *stream)
{
    OCN_TRY(check_transpose(nx, Ny, Nz, R, recv, yfield));
    return launch_transpose(3, nx, Ny, Nz, R, recv, yfield, as_stream(stream));
}

}  // extern "C"
