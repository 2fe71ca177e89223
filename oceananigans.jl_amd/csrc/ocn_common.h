// ocn_common.h -- shared host/device helpers for libocn_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <tuple>

#include "../../include/ocn_hip.h"

namespace ocn {

void set_error(const char *fmt, ...);

#define OCN_CHECK_HIP(expr)                                                                       \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess) {                                                                   \
            ocn::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return OCN_ERR_HIP;                                                                   \
        }                                                                                         \
    } while (0)

#define OCN_REQUIRE(cond, ...)                \
    do {                                      \
        if (!(cond)) {                        \
            ocn::set_error(__VA_ARGS__);      \
            return OCN_ERR_INVALID_ARGUMENT;  \
        }                                     \
    } while (0)

// a call that returns a status: the first failure is the enclosing function's result
#define OCN_TRY(expr)                          \
    do {                                       \
        int st_ = (expr);                      \
        if (st_ != OCN_SUCCESS) return st_;    \
    } while (0)

// Device-side copy of the grid, plus derived scalars.  Passed by value to kernels.
struct GridDev {
    int Nx, Ny, Nz, Hx, Hy, Hz, tx, ty, tz;
    double dx, dy, dz;
    const double *dzc, *dzf;
    // walls of the x direction by side: both for Bounded, one for the first (RightConnected: west) and the last (LeftConnected: east)
    // slab of a grid whose partitioned x is Bounded; tx is OCN_BOUNDED for all three (kernels that never meet an x wall ignore these)
    int xw, xe;
};

// The correction-on-load tendency kernel addresses every field with 32-bit byte offsets (momentum_tendencies_pc32): usable when the
// parent array of a (Periodic | FullyConnected, Periodic, Periodic) field -- the one layout of u, v, w, p and G there -- spans fewer than
// 2^31 bytes and the halos hold the full WENO stencil.  OCN_TEND_ADDR32=0 keeps the 64-bit kernel (same-box A/B runs).
inline bool tendency_addr32_fits(const ocn_grid &g)
{
    const long long bytes = 8LL * (g.Nx + 2LL * g.Hx) * (g.Ny + 2LL * g.Hy) * (g.Nz + 2LL * g.Hz);
    return g.Hx >= 3 && g.Hy >= 3 && g.Hz >= 3 && bytes < (1LL << 31);
}
inline bool tendency_addr32_enabled()
{
    static const bool on = !(getenv("OCN_TEND_ADDR32") && atoi(getenv("OCN_TEND_ADDR32")) == 0);
    return on;
}

// x walls of a host-side grid description
inline bool x_wall_west(const ocn_grid &g) { return g.tx == OCN_BOUNDED || g.tx == OCN_RIGHT_CONNECTED; }
inline bool x_wall_east(const ocn_grid &g) { return g.tx == OCN_BOUNDED || g.tx == OCN_LEFT_CONNECTED; }
// x halos that come from a neighbour rank (by side)
inline bool x_connected_west(const ocn_grid &g) { return g.tx == OCN_FULLY_CONNECTED || g.tx == OCN_LEFT_CONNECTED; }
inline bool x_connected_east(const ocn_grid &g) { return g.tx == OCN_FULLY_CONNECTED || g.tx == OCN_RIGHT_CONNECTED; }

inline GridDev to_dev(const ocn_grid &g)
{
    GridDev d;
    d.Nx = g.Nx; d.Ny = g.Ny; d.Nz = g.Nz;
    d.Hx = g.Hx; d.Hy = g.Hy; d.Hz = g.Hz;
    d.xw = x_wall_west(g) ? 1 : 0;
    d.xe = x_wall_east(g) ? 1 : 0;
    // FullyConnected: interior arithmetic identical to Periodic; the half-Bounded slabs: Bounded, qualified by xw / xe
    d.tx = g.tx == OCN_FULLY_CONNECTED ? OCN_PERIODIC : ((d.xw || d.xe) ? OCN_BOUNDED : g.tx);
    d.ty = g.ty; d.tz = g.tz;
    d.dx = g.dx; d.dy = g.dy; d.dz = g.dz;
    d.dzc = g.dzc; d.dzf = g.dzf;
    return d;
}

// Read-only vectors indexed by a wave-uniform index (the stretched-z metrics Δzᵃᵃᶜ[k], Δzᵃᵃᶠ[k]): a pointer that reaches a kernel inside a
// by-value struct is not known to be invariant, so the compiler loads through it with VECTOR memory instructions -- and every
// `s_waitcnt vmcnt(0)` in front of such a value also waits for all the prefetches issued before it, which serialised the software
// pipelines of the Bounded-z kernels (profiles/r03a_config4.md: 45-53 % of the wave cycles parked).  Reading through the CONSTANT address
// space makes them scalar loads (s_load, lgkmcnt): no vector-memory ordering, no VGPRs.  The vectors are never written by a kernel.
typedef const double __attribute__((address_space(4))) *ocn_const_ptr;
__device__ __forceinline__ double uniform_load(const double *p, int idx) { return ((ocn_const_ptr)p)[idx]; }
// A wave-uniform double that the compiler computed with vector instructions (products of kernel arguments, reciprocals) lives in a
// pair of VGPRs; this moves it to scalar registers, which vector instructions read as an operand (one per instruction).  Only for values
// that ARE the same in every lane of the wave.
__device__ __forceinline__ double to_sgpr(double x)
{
    const unsigned long long b = __builtin_bit_cast(unsigned long long, x);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b), hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// Compiler-level fence for software pipelines: memory operations written above it are issued above it (the loads of the NEXT plane must
// leave at the top of an iteration, not where the scheduler finds their first use).  No instruction is emitted.
#define OCN_ISSUE_LOADS_HERE() asm volatile("" ::: "memory")

// Parent-array layout of a field at location `loc` (bit0 x-face, bit1 y-face, bit2 z-face).
struct Lay {
    int sx, sy, sz;       // parent extents
    long long s2, s3;     // strides of j and k
    long long o;          // offset of interior (1,1,1)
};

__host__ __device__ inline int ocn_ext(int N, int H, int topo, int face)
{
    return N + 2 * H + ((face && topo == OCN_BOUNDED) ? 1 : 0);
}

__host__ __device__ inline Lay make_lay(const GridDev &g, int loc)
{
    Lay L;
    // (x: the extra Face point belongs to the side with the EAST wall -- Bounded, or the last slab of a partitioned Bounded x)
    L.sx = g.Nx + 2 * g.Hx + (((loc & 1) && g.xe) ? 1 : 0);
    L.sy = ocn_ext(g.Ny, g.Hy, g.ty, loc & 2);
    L.sz = ocn_ext(g.Nz, g.Hz, g.tz, loc & 4);
    L.s2 = L.sx;
    L.s3 = (long long)L.sx * L.sy;
    L.o = g.Hx + L.s2 * g.Hy + L.s3 * g.Hz;
    return L;
}
// 1-based interior index -> parent offset
__host__ __device__ inline long long at(const Lay &L, int i, int j, int k)
{
    return L.o + (i - 1) + L.s2 * (j - 1) + L.s3 * (k - 1);
}

// x-y planes of the hydrostatic layer (η, U, V, ...: parent x / y extents of their location, no z): the offset of the 1-based interior
// (i, j) of a plane whose rows are as long as layout L's, and of one shaped like η (Center, Center)
__device__ __forceinline__ long long plane_at(const GridDev &g, const Lay &L, int i, int j)
{
    return (i - 1 + g.Hx) + (long long)L.sx * (j - 1 + g.Hy);
}
__device__ __forceinline__ long long plane_at(const GridDev &g, int i, int j)
{
    return (i - 1 + g.Hx) + (long long)(g.Nx + 2 * g.Hx) * (j - 1 + g.Hy);
}
// Δzᵃᵃᶜ / Δzᵃᵃᶠ at level / face k (wave-uniform)
__device__ __forceinline__ double dz_centre(const GridDev &g, int k) { return g.dzc ? uniform_load(g.dzc, k + g.Hz - 1) : g.dz; }
__device__ __forceinline__ double dz_face(const GridDev &g, int k) { return g.dzf ? uniform_load(g.dzf, k + g.Hz - 1) : g.dz; }
// launch grid of 64 x 4 blocks, one thread per column (or per cell: nz planes)
inline dim3 xy_blocks(int nx, int ny, int nz = 1) { return dim3((nx + 63) / 64, (ny + 3) / 4, nz); }

// Optional epilogue of the tendency launch: the NEXT RK3 substep  Uo = U + dt*(gamma*G + zeta*Gm)  (runge_kutta_3.jl:194-200)
struct FuseArgs {
    const double *Gm[3];
    double *Uo[3];
    double dt, gamma, zeta;
    int on;
    int has_zeta;  // 0: first-stage form  Uo = U + (dt*gamma)*G  (runge_kutta_3.jl:202-208)
    // optional prologue: the PREVIOUS stage's pressure correction applied to every velocity value as it is loaded,
    //   u <- u - ((p[i]-p[i-1])/dx)*pc_dt  etc. (pressure_correction.jl:31-37); all-periodic grids only (indices wrap)
    const double *pc_p;
    double pc_dt;
    int pc_on;
    // x-partitioned (FullyConnected) local grid: the x indices of p are NOT wrapped -- the x halos of p hold the neighbours' planes
    // (ocn_halo_exchange_pressure) and the westmost halo column of u, whose correction would need p[-Hx], arrives corrected
    int pc_xhalo;
    // G already holds the terms that do not come from advection (momentum_extra_* in `pre` mode ran first): G <- advection + G before it is
    // stored and used by the substep.  Fast math only: the sum is the reference's with the advective term added last instead of first.
    int acc;
    // slab-x rank, correction-on-load stage: the substep results of the Hx westmost / eastmost columns are ALSO written into the send
    // buffers of the next x-halo exchange (layout of halo_pack_x_fields_kernel: field f at strip_field * f, then h + Hx * parent row), so
    // the exchange needs no pack launch; only interior rows are written -- the receiver wraps (ocn_halo_exchange_begin_packed)
    double *strip_w, *strip_e;
    long long strip_field;
    // The three below are taken by momentum_tendencies_pc32 only (all zero: today's launch).
    // skip_g: G is computed and used by the substep but not stored -- for a caller that knows nobody reads it (the last launch of a step of
    // ocn_rk3_driver_time_step: the next launch has no G⁻ term and overwrites the same buffer).  A permission: other kernels store G.
    int skip_g;
    // wrap_uvw: u, v, w are addressed like p, by periodically wrapped indices: their halos are never read (no halo fill in front of the
    // launch).  Periodic x only; required, not a permission: a launch that cannot honour it is an error.
    int wrap_uvw;
    // no_step: Uo = the corrected velocity itself, no increment (ocn_rk3_driver_flush: pressure_correct_velocities! and compute_tendencies!
    // in one pass).  Not U + 0 * G: that loses the sign of -0.0 and turns a non-finite G into a non-finite velocity.  Required as well.
    int no_step;
};

// device-side copy of ocn_model_terms (physics.hip)
struct TermsDev {
    int coriolis, closure, buoyancy;
    double f, nu, g, alpha, beta;
    const double *T, *S, *pHY;
    const double *nu_e;  // eddy viscosity νₑ (ccc, halos filled) of an LES closure, or NULL: the number `nu`
    double cbeta;        // coriolis == 2 (BetaPlane): f = f + cbeta * y, y = yc[j + Hy - 1] at u points, yf[j + Hy - 1] at v points
    const double *yc, *yf;
};
// the Coriolis parameter at row j of a u point (face = 0) or a v point (face = 1)   (f_plane.jl:44-46, beta_plane.jl:43-57)
__device__ __forceinline__ double coriolis_f_at(const TermsDev &t, int Hy, int j, int face)
{
    if (t.coriolis != 2) return t.f;
    return t.f + t.cbeta * (face ? t.yf : t.yc)[j + Hy - 1];
}
inline TermsDev to_dev(const ocn_model_terms &m)
{
    TermsDev t;
    t.coriolis = m.coriolis; t.closure = m.closure; t.buoyancy = m.buoyancy;
    t.f = m.f; t.nu = m.nu; t.g = m.g; t.alpha = m.alpha; t.beta = m.beta;
    t.T = m.T; t.S = m.S; t.pHY = m.pHY;
    t.nu_e = m.nu_e;
    t.cbeta = m.coriolis_beta; t.yc = m.yc; t.yf = m.yf;
    return t;
}

// device-side copy of ocn_stokes_drift (UniformStokesDrift, StokesDrifts.jl:36-180): the six per-level profiles, element 0 <-> k = 1
// (Nz values at centres, Nz + 1 at faces); NULL: the profile is zero.  Wave-uniform in every kernel that reads them (k is), so they are
// read through the constant address space like dzc / dzf.  Only the kernels compiled with the Stokes terms take this struct as an argument.
struct StokesDev {
    const double *dzu_c, *dzv_c;  // ∂z uˢ, ∂z vˢ at z centres (x / y components of (∇ × uˢ) × u)
    const double *dzu_f, *dzv_f;  // ... at z faces (z component)
    const double *dtu, *dtv;      // ∂t uˢ, ∂t vˢ at z centres
};
__device__ __forceinline__ double stokes_at(const double *p, int k) { return p ? uniform_load(p, k - 1) : 0.0; }
inline StokesDev to_dev(const ocn_stokes_drift &s)
{
    return StokesDev{s.dz_us_center, s.dz_vs_center, s.dz_us_face, s.dz_vs_face, s.dt_us, s.dt_vs};
}

// device-side copy of ocn_forcing (forcing = (u = ..., ...), src/Forcings): up to four sampled terms of ONE field, summed left to right
// (multiple_forcings.jl:34-46).  The struct travels in the kernel arguments, so n, the kinds and the dims are wave-uniform scalars; vectors
// along z are read through the constant address space (k is wave-uniform in every kernel that takes this), vectors along x / y and arrays
// in the parent layout are per-lane loads.  Only the kernels compiled with the forcing terms take this struct as an argument.
struct ForcingTermDev {
    int kind, mask_dim, target_dim;
    double rate, target_value;
    const double *values, *mask, *target;
};
struct ForcingDev {
    int n;
    ForcingTermDev term[OCN_FORCING_MAX_TERMS];
};
inline ForcingDev to_dev(const ocn_forcing *f)
{
    ForcingDev d{};
    if (!f) return d;
    d.n = f->n_terms;
    for (int q = 0; q < f->n_terms && q < OCN_FORCING_MAX_TERMS; ++q) {
        const ocn_forcing_term &s = f->term[q];
        d.term[q] = ForcingTermDev{s.kind, s.mask_dim, s.target_dim, s.rate, s.target_value, s.values, s.mask, s.target};
    }
    return d;
}
// the forcings of u, v, w for the momentum finishing pass compiled with them; `stokes`: the StokesDev argument next to it is in use
struct MomentumForcingDev {
    ForcingDev f[3];
    int stokes;
};
// The momentum finishing-pass kernels (physics.hip, general.hip) are templates on a trailing pack X of descriptor arguments: {} (no extra
// term: the kernels and their arguments as they always were), {StokesDev}, or {StokesDev, MomentumForcingDev} -- ONE variant for forcing
// with and without a Stokes drift (fd.stokes = 0: `sd` is empty and its terms are skipped).
// In a kernel: the I-th descriptor of the pack, or NULL in an instantiation that does not take it.
template <class T, int I, class... X>
__device__ __forceinline__ const T *extra_arg(const X &...x)
{
    if constexpr (I < (int)sizeof...(X))
        return &std::get<I>(std::tie(x...));
    else
        return nullptr;
}
// In a launcher: launch(), launch(sd) or launch(sd, fd), whichever the model asks for.
template <class L>
inline int with_extra_descriptors(const StokesDev *stokes, const MomentumForcingDev *forcing, L launch)
{
    if (forcing) {
        MomentumForcingDev fd = *forcing;
        fd.stokes = stokes != nullptr;
        return launch(stokes ? *stokes : StokesDev{}, fd);
    }
    if (stokes) return launch(*stokes);
    return launch();
}
// mask / target of a Relaxation term at a cell: ix, iy, iz = its indices along the parent array (i - 1 + Hx ...), o its parent offset
__device__ __forceinline__ double forcing_profile(int dim, const double *p, double number, int ix, int iy, int iz, long long o)
{
    if (dim < 0) return number;
    if (dim == 2) return uniform_load(p, iz);
    if (dim == 3) return p[o];
    return p[dim == 0 ? ix : iy];
}
// F of one field at one cell whose value is `c`:  F = t1; F = F + t2; ...   (f.n >= 1)
__device__ __forceinline__ double forcing_at(const ForcingDev &f, int ix, int iy, int iz, long long o, double c)
{
    double F = 0.0;
#pragma unroll
    for (int q = 0; q < OCN_FORCING_MAX_TERMS; ++q) {
        if (q >= f.n) break;
        const ForcingTermDev &t = f.term[q];
        double v;
        if (t.kind == OCN_FORCING_ARRAY) {
            v = t.values[o];
        } else {  // Relaxation: (rate * mask(X)) * (target(X, t) - field[i, j, k])   (relaxation.jl:95-101)
            const double m = forcing_profile(t.mask_dim, t.mask, 1.0, ix, iy, iz, o);
            const double tg = forcing_profile(t.target_dim, t.target, t.target_value, ix, iy, iz, o);
            v = (t.rate * m) * (tg - c);
        }
        F = q == 0 ? v : F + v;
    }
    return F;
}

// bottom / top boundary condition of one field (kind 0: default fill / no flux)
struct ZBc {
    int kind;
    double value, coeff;
    const double *values;
};
// value of a boundary condition at (i, j): array entry, value + coeff * c[boundary cell], or the number
__host__ __device__ inline double bc_condition(const ZBc &bc, int i, int j, int Nx, double c_int)
{
    if (bc.values) return bc.values[(i - 1) + (long long)Nx * (j - 1)];
    if (bc.coeff != 0.0) return bc.value + bc.coeff * c_int;
    return bc.value;
}
// the NEXT stage's rk3 substep of one field, as the epilogue of its tendency kernel:  out = U + dt*(gamma*G + zeta*Gm)
struct SubstepDev {
    const double *Gm;
    double *out;
};
struct SubstepCoef {
    double dt, gamma, zeta;
    int on, has_zeta;
};
// everything the tracer tendency kernel can fold in besides advection (physics.hip / tendencies.hip)
struct TracerFuse {
    static constexpr bool forced = false;
    int diffusion;          // add -∇_dot_qᶜ
    double kappa;
    const double *kappa_e;  // eddy diffusivity field or NULL
    ZBc bottom, top;        // flux boundary conditions (kind OCN_BC_FLUX) folded into Gc
    SubstepDev sub;
    SubstepCoef sc;
};
// ... and the sampled forcing of the tracer (forcing = (T = ...)): the tracer kernels are templates on the descriptor type, so the
// instantiations with TracerFuse keep their arguments and their code, and the ones with TracerFuseForced add F between the diffusion and
// the boundary fluxes (tracer_finish)
struct TracerFuseForced : TracerFuse {
    static constexpr bool forced = true;
    ForcingDev frc;
};
// flux boundary conditions of u, v and the substeps of u, v, w for the momentum "finaliser" (momentum_extra_kernel)
struct MomentumFinal {
    ZBc bottom[2], top[2];
    SubstepDev sub[3];
    SubstepCoef sc;
    int xcd;  // XCD-aware workgroup -> tile mapping (set by the launchers)
    int pre;  // the pass runs BEFORE the advective launch: G does not hold anything yet (taken as 0), no substep (FuseArgs::acc follows)
};

// what hydrostatic_momentum_tiled (physics.hip) folds in besides the tendency and the AB2 step of u, v
struct HydroFuse {
    const double *eta;  // ExplicitFreeSurface: η plane (sx, sy) for - g ∇η, or NULL (SplitExplicitFreeSurface: the gradient is 0)
    double grav;
    double *GU, *GV;    // SplitExplicitFreeSurface: barotropic forcing planes (compute_split_explicit_forcing!), or NULL
    double *Ub, *Vb;    //                           Σ Δz u*, Σ Δz v* of the stepped velocities (for the barotropic corrector)
};

int validate_grid(const ocn_grid *g);      // Periodic (or partitioned) x, Periodic y
int validate_grid_any(const ocn_grid *g);  // any of Periodic / Bounded / Flat in x and y

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

// 256-thread block for a one-thread-per-cell launch over a range wx cells wide: the usual 64 x 4 (one wave = 64 consecutive
// x), but for the thin x-strips of the distributed buffer tendencies (wx = halo width) 64 lanes along x would leave most of
// every wave idle, so the block is folded towards y: (pow2 >= wx) x (256 / that).
inline dim3 range_block(int wx)
{
    int bx = 64;
    while (bx > 4 && bx / 2 >= wx) bx /= 2;
    return dim3(bx, 256 / bx, 1);
}
inline dim3 range_grid(dim3 block, int wx, int wy, int wz)
{
    return dim3((wx + block.x - 1) / block.x, (wy + block.y - 1) / block.y, wz);
}

}  // namespace ocn
