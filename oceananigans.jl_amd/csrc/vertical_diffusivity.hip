// vertical_diffusivity.hip -- closures of the VerticalFormulation whose ν, κ are FIELDS at (Center, Center, Face), on a z-Bounded grid:
// ConvectiveAdjustmentVerticalDiffusivity fills them; the two other pieces take any such fields.
//
//  1. compute_convective_adjustment_diffusivities! (convective_adjustment_vertical_diffusivity.jl:91-123): one thread per cell over
//     i = 1..Nx, j = 1..Ny, k = 1..Nz -- the hydrostatic model launches it over :xyz, so face Nz+1 is never written --,
//       stable = ∂z_b(i, j, k) >= 0      (a gradient of exactly 0 is stable, a NaN is not)
//       κᶜ = stable ? background_κz : convective_κz,   κᵘ = stable ? background_νz : convective_νz
//     with ∂z_b = g (α ∂zᶜᶜᶠ T - β ∂zᶜᶜᶠ S) (seawater_buoyancy.jl:219-224), ∂zᶜᶜᶠ b (buoyancy_tracer.jl:16), or 0 without buoyancy.
//
//  2. the closure's tendency term (abstract_scalar_diffusivity_closure.jl:198-211, 221-260) added to a G that holds every other term:
//       viscous_flux_uz = -ℑxᶠᵃᵃ(κᵘ) ∂zᶠᶜᶠ u,  viscous_flux_vz = -ℑyᵃᶠᵃ(κᵘ) ∂zᶜᶠᶠ v,  diffusive_flux_z = -κᶜ ∂zᶜᶜᶠ c,  no horizontal flux,
//     through the divergences of closure_kernel_operators.jl:27-53 in the operand order of general.hip.  boundary_only: the vertically
//     implicit variant (the flux at k == 1 | k == Nz+1, zero on interior faces).  There the term of a cell with no boundary face is
//     G - 1 / V * ((0 + 0) + (Az 0 - Az 0)) = G - 0, which is G for every G: only the planes k = 1 and k = Nz are launched.
//
//  3. implicit_step! with a κ field per field: (1 - Δt ∂z κ ∂z) φⁿ⁺¹ = φ★ in place, the Center-in-z rows of
//     vertically_implicit_diffusion_solver.jl:55-78 with κz located as abstract_scalar_diffusivity_closure.jl:307-315 locates a
//     (Center, Center, Face) array, eliminated in the order of solve_batched_tridiagonal_system_z!.  One thread owns one (i, j) column,
//     x fastest across the lanes, as in implicit_diffusion.hip -- but the matrix now differs from column to column, so nothing is shared
//     through LDS: a thread assembles the three entries of a row from κ as it goes (two divisions), eliminates (a third), and keeps the
//     multipliers t[k] for the backward sweep in a caller-provided array of Nx Ny Nz doubles (the reference keeps a full t for the same
//     reason; per-thread arrays would spill).  Fields that share a matrix (the same κ array and location: every tracer of
//     ConvectiveAdjustmentVerticalDiffusivity) are swept together by one thread, so κ, t and those three divisions are read / done once
//     per group: 32 n + 24 B per cell for n fields (κ 8, t written 8 and read 8; a field read and written in each sweep).
//     Loads are issued a batch of planes ahead of the sequential arithmetic.
//
// Bandwidth-bound: one strict build (no FMA contraction, IEEE division) whatever the math mode, bit-identical to
// tests/convective_adjustment_numpy.py.  The buoyancy is that of ocn_buoyancy.h.
#include "ocn_buoyancy.h"
#include "ocn_ivd.h"

namespace ocn {

namespace vdf {

using ivd::Range;
using ivd::Spacings;

__global__ __launch_bounds__(256) void convective_adjustment_diffusivities(GridDev g, Buoyancy b, ocn_convective_adjustment cl,
                                                                           double *__restrict__ kappa_c, double *__restrict__ kappa_u)
{
    const int i = 1 + blockIdx.x * 64 + threadIdx.x, j = 1 + blockIdx.y * 4 + threadIdx.y, k = 1 + blockIdx.z;
    if (i > g.Nx || j > g.Ny) return;
    const Spacings M = ivd::spacings_of(g);
    const Lay Lc = make_lay(g, OCN_LOC_CCC), Lf = make_lay(g, OCN_LOC_CCF);
    const long long o = at(Lc, i, j, k);
    double dzb = 0.0;  // dz_b of ocn_buoyancy.h, the tracers read only where the kind needs them
    if (b.kind != OCN_BUOYANCY_NONE) {
        const double dzf = M.dzF(k);
        const double dT = b.T ? (b.T[o] - b.T[o - Lc.s3]) / dzf : 0.0;
        if (b.kind == OCN_BUOYANCY_TRACER) {
            dzb = dT;
        } else {
            const double dS = b.S ? (b.S[o] - b.S[o - Lc.s3]) / dzf : 0.0;
            dzb = b.g * (b.alpha * dT - b.beta * dS);
        }
    }
    const bool stable = dzb >= 0;
    const long long of = at(Lf, i, j, k);
    kappa_c[of] = stable ? cl.background_kappa_z : cl.convective_kappa_z;
    kappa_u[of] = stable ? cl.background_nu_z : cl.convective_nu_z;
}

// ---------------------------------------------------------------------------------------------------
// the closure term
// ---------------------------------------------------------------------------------------------------
// Gu <- Gu - ∂ⱼτ₁ⱼ, Gv <- Gv - ∂ⱼτ₂ⱼ: only τ₁₃, τ₂₃ are not zero
__global__ __launch_bounds__(256) void momentum_fluxes(GridDev g, const double *__restrict__ nu, const double *__restrict__ u,
                                                       const double *__restrict__ v, double *__restrict__ Gu, double *__restrict__ Gv,
                                                       int boundary_only, Range r)
{
    int i, j, k;
    if (!ivd::cell_of(r, i, j, k)) return;
    const Spacings M = ivd::spacings_of(g);
    const Lay Lu = make_lay(g, OCN_LOC_FCC), Lv = make_lay(g, OCN_LOC_CFC), Lf = make_lay(g, OCN_LOC_CCF);
    const int Nz = g.Nz;
    const double Az = g.dx * g.dy;
    const double dzf0 = M.dzF(k), dzf1 = M.dzF(k + 1);
    auto explicit_face = [&](int c) { return !boundary_only || ((c == 1) | (c == Nz + 1)); };
    const long long on = at(Lf, i, j, k);
    const double n00 = nu[on], n01 = nu[on + Lf.s3];
    if (i >= r.ou) {
        const long long o = at(Lu, i, j, k);
        const double nu0 = 0.5 * (nu[on - 1] + n00), nu1 = 0.5 * (nu[on - 1 + Lf.s3] + n01);  // ℑxᶠᵃᵃ at faces k, k + 1
        const double t0 = explicit_face(k) ? -(nu0 * ((u[o] - u[o - Lu.s3]) / dzf0)) : 0.0;
        const double t1 = explicit_face(k + 1) ? -(nu1 * ((u[o + Lu.s3] - u[o]) / dzf1)) : 0.0;
        const double dzF = Az * t1 - Az * t0;
        Gu[o] = Gu[o] - 1 / (Az * M.dzC(k)) * ((0.0 + 0.0) + dzF);
    }
    if (j >= r.ov) {
        const long long o = at(Lv, i, j, k);
        const double nu0 = 0.5 * (nu[on - Lf.s2] + n00), nu1 = 0.5 * (nu[on - Lf.s2 + Lf.s3] + n01);  // ℑyᵃᶠᵃ
        const double t0 = explicit_face(k) ? -(nu0 * ((v[o] - v[o - Lv.s3]) / dzf0)) : 0.0;
        const double t1 = explicit_face(k + 1) ? -(nu1 * ((v[o + Lv.s3] - v[o]) / dzf1)) : 0.0;
        const double dzF = Az * t1 - Az * t0;
        Gv[o] = Gv[o] - 1 / (Az * M.dzC(k)) * ((0.0 + 0.0) + dzF);
    }
}

// Gc <- Gc - ∇_dot_qᶜ: only q₃ is not zero
__global__ __launch_bounds__(256) void tracer_fluxes(GridDev g, const double *__restrict__ kappa, const double *__restrict__ c,
                                                     double *__restrict__ Gc, int boundary_only, Range r)
{
    int i, j, k;
    if (!ivd::cell_of(r, i, j, k)) return;
    const Spacings M = ivd::spacings_of(g);
    const Lay L = make_lay(g, OCN_LOC_CCC), Lf = make_lay(g, OCN_LOC_CCF);
    const int Nz = g.Nz;
    const double Az = g.dx * g.dy;
    auto explicit_face = [&](int cc) { return !boundary_only || ((cc == 1) | (cc == Nz + 1)); };
    const long long o = at(L, i, j, k), on = at(Lf, i, j, k);
    const double q0 = explicit_face(k) ? -(kappa[on] * ((c[o] - c[o - L.s3]) / M.dzF(k))) : 0.0;
    const double q1 = explicit_face(k + 1) ? -(kappa[on + Lf.s3] * ((c[o + L.s3] - c[o]) / M.dzF(k + 1))) : 0.0;
    const double dzF = Az * q1 - Az * q0;
    Gc[o] = Gc[o] - 1 / (Az * M.dzC(k)) * ((0.0 + 0.0) + dzF);
}

// ---------------------------------------------------------------------------------------------------
// implicit step
// ---------------------------------------------------------------------------------------------------
// the fields of one launch that share a matrix
struct Group {
    double *f[MAX_TUPLE];
    const double *kappa;  // (Center, Center, Face) with halos
    double *t;            // Nx Ny Nz multipliers, no halos, x fastest
    int loc;
};
struct Groups {
    Group g[MAX_TUPLE];
};

template <int NF>
struct Batch {  // planes loaded ahead of the arithmetic: (NF fields + κ or t) * planes * 2 VGPRs
    static constexpr int planes = NF <= 2 ? 8 : 4;
};

template <int NF>
__global__ __launch_bounds__(256) void implicit_step_fields(GridDev g, Groups groups, double dt)
{
    constexpr int B = Batch<NF>::planes;
    const int i = 1 + blockIdx.x * 64 + threadIdx.x, j = 1 + blockIdx.y * 4 + threadIdx.y;
    if (i > g.Nx || j > g.Ny) return;
    const Group &G = groups.g[blockIdx.z];
    const int Nz = g.Nz, loc = G.loc;
    const Spacings M = ivd::spacings_of(g);
    const Lay L = make_lay(g, loc), Lf = make_lay(g, OCN_LOC_CCF);
    const long long s3 = L.s3, f3 = Lf.s3, t3 = (long long)g.Nx * g.Ny;
    // κz(i, j, k): κ[i, j, k] for (c, c, c) fields, ℑxᶠᵃᵃ(κ) for (f, c, c), ℑyᵃᶠᵃ(κ) for (c, f, c): `back` reaches the second operand
    const long long back = (loc & 1) ? 1 : ((loc & 2) ? Lf.s2 : 0);
    const double *__restrict__ kp = G.kappa + at(Lf, i, j, 1);
    double *__restrict__ tp = G.t + (i - 1) + (long long)g.Nx * (j - 1);
    double *p[NF];
#pragma unroll
    for (int n = 0; n < NF; ++n) p[n] = G.f[n] + at(L, i, j, 1);
    auto kappa_at = [&](int k) {  // k = 1..Nz+1
        const double here = kp[(k - 1) * f3];
        return back ? 0.5 * (kp[(k - 1) * f3 - back] + here) : here;
    };
    const double tiny = 10 * 2.220446049250313e-16;  // 10 eps(Float64)
    // row 1: ivd_diagonal = (1 - upper(1)) - lower(0), lower(0) = 0
    double prev[NF], beta, up, kap;  // kap: κz at face k of the row about to be eliminated
    {
        const double kn = kappa_at(2);
        const double du = -dt * kn / (M.dzC(1) * M.dzF(2));
        up = 1 > Nz - 1 ? 0.0 : du;
        beta = (1.0 - up) - 0.0;
#pragma unroll
        for (int n = 0; n < NF; ++n) {
            prev[n] = p[n][0] / beta;
            p[n][0] = prev[n];
        }
        kap = kn;
    }
    // forward sweep, the intermediate parked in the fields, t[k] in the scratch array
    for (int k0 = 2; k0 <= Nz; k0 += B) {
        double f[NF][B] = {}, kn[B] = {};
#pragma unroll
        for (int q = 0; q < B; ++q)
            if (k0 + q <= Nz) {
                kn[q] = kappa_at(k0 + q + 1);
#pragma unroll
                for (int n = 0; n < NF; ++n) f[n][q] = p[n][(k0 + q - 1) * s3];
            }
#pragma unroll
        for (int q = 0; q < B; ++q) {
            const int k = k0 + q;
            if (k <= Nz) {
                const double dzc = M.dzC(k);
                const double lo = -dt * kap / (dzc * M.dzF(k));          // ivd_lower_diagonal(k - 1): the entry below the diagonal, row k
                const double du = -dt * kn[q] / (dzc * M.dzF(k + 1));    // ivd_upper_diagonal(k)
                const double upk = k > Nz - 1 ? 0.0 : du;
                const double b = (1.0 - upk) - lo;
                const double t = up / beta;
                beta = b - lo * t;
                tp[(k - 1) * t3] = t;
                const bool regular = fabs(beta) > tiny;
#pragma unroll
                for (int n = 0; n < NF; ++n) {
                    const double star = (f[n][q] - lo * prev[n]) / beta;
                    prev[n] = regular ? star : f[n][q];
                    p[n][(k - 1) * s3] = prev[n];
                }
                up = upk;
                kap = kn[q];
            }
        }
    }
    // backward sweep: φ[k] -= t[k+1] φ[k+1]
    for (int k0 = Nz - 1; k0 >= 1; k0 -= B) {
        double f[NF][B] = {}, t[B] = {};
#pragma unroll
        for (int q = 0; q < B; ++q)
            if (k0 - q >= 1) {
                t[q] = tp[(k0 - q) * t3];
#pragma unroll
                for (int n = 0; n < NF; ++n) f[n][q] = p[n][(k0 - q - 1) * s3];
            }
#pragma unroll
        for (int q = 0; q < B; ++q) {
            const int k = k0 - q;
            if (k >= 1) {
#pragma unroll
                for (int n = 0; n < NF; ++n) {
                    prev[n] = f[n][q] - t[q] * prev[n];
                    p[n][(k - 1) * s3] = prev[n];
                }
            }
        }
    }
}

constexpr int MAX_SHARED = 4;  // fields one thread sweeps together (a larger group is swept in several launches)

template <int NF>
static void launch_groups(const GridDev &gd, const Groups &groups, int n, double dt, hipStream_t stream)
{
    const dim3 block(64, 4, 1), blocks((gd.Nx + 63) / 64, (gd.Ny + 3) / 4, n);
    hipLaunchKernelGGL(implicit_step_fields<NF>, blocks, block, 0, stream, gd, groups, dt);
}

}  // namespace vdf

// the callers have validated the grid (z Bounded, x and y not Flat, halos >= 1) and the pointers
int launch_convective_adjustment_diffusivities(const ocn_grid *grid, const ocn_model_terms *terms, const ocn_convective_adjustment *closure,
                                               double *kappa_c, double *kappa_u, hipStream_t stream)
{
    const dim3 block(64, 4, 1), blocks((grid->Nx + 63) / 64, (grid->Ny + 3) / 4, grid->Nz);
    hipLaunchKernelGGL(vdf::convective_adjustment_diffusivities, blocks, block, 0, stream, to_dev(*grid), make_buoyancy(terms), *closure, kappa_c,
                       kappa_u);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

int launch_vertical_diffusivity_fluxes(const ocn_grid *grid, const double *kappa_u, const double *u, const double *v, double *Gu, double *Gv,
                                       int n_tracers, const double *const *kappa_c, const double *const *c, double *const *Gc,
                                       int boundary_only, const int32_t *range, hipStream_t stream)
{
    ivd::Range whole;
    OCN_TRY(make_ivd_range(grid, range, whole));
    const GridDev gd = to_dev(*grid);
    // boundary_only: the planes k = 1 and k = Nz that lie in the range (one plane when Nz == 1); else one launch over all of it
    const int planes[2] = {1, grid->Nz};
    const int n_launches = boundary_only ? (grid->Nz > 1 ? 2 : 1) : 1;
    for (int q = 0; q < n_launches; ++q) {
        ivd::Range r = whole;
        if (boundary_only) {
            if (planes[q] < whole.k0 || planes[q] > whole.k1) continue;
            r.k0 = r.k1 = planes[q];
        }
        const int wx = r.i1 - r.i0 + 1, wy = r.j1 - r.j0 + 1, wz = r.k1 - r.k0 + 1;
        if (wx < 1 || wy < 1 || wz < 1) continue;
        const dim3 block(64, 4, 1), blocks((wx + 63) / 64, (wy + 3) / 4, wz);
        if (u) hipLaunchKernelGGL(vdf::momentum_fluxes, blocks, block, 0, stream, gd, kappa_u, u, v, Gu, Gv, boundary_only, r);
        for (int n = 0; n < n_tracers; ++n)
            hipLaunchKernelGGL(vdf::tracer_fluxes, blocks, block, 0, stream, gd, kappa_c[n], c[n], Gc[n], boundary_only, r);
    }
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

int launch_ivd_implicit_step_fields(const ocn_grid *grid, int n, double *const *fields, const int32_t *locs, const double *const *kappa,
                                    double *const *scratch, double dt, hipStream_t stream)
{
    // fields share a matrix when they have the same κ array and the same location; the scratch array of a group is its first field's
    int group_of[MAX_TUPLE], first[MAX_TUPLE], size[MAX_TUPLE], n_groups = 0;
    for (int f = 0; f < n; ++f) {
        int gidx = -1;
        for (int q = 0; q < n_groups; ++q)
            if (kappa[first[q]] == kappa[f] && locs[first[q]] == locs[f]) gidx = q;
        if (gidx < 0) {
            gidx = n_groups++;
            first[gidx] = f;
            size[gidx] = 0;
        }
        group_of[f] = gidx;
        ++size[gidx];
    }
    for (int q = 0; q < n_groups; ++q) {
        OCN_REQUIRE(scratch[first[q]] != nullptr, "ocn_implicit_vertical_diffusion_step_fields: field %d opens a group: its scratch array is NULL",
                    first[q]);
        for (int p = 0; p < q; ++p)
            OCN_REQUIRE(scratch[first[p]] != scratch[first[q]],
                        "ocn_implicit_vertical_diffusion_step_fields: fields %d and %d have different matrices but the same scratch array", first[p],
                        first[q]);
    }
    const GridDev gd = to_dev(*grid);
    // one launch per number of fields swept together; a group of more than MAX_SHARED fields takes further rounds (the multipliers are
    // recomputed: same values, and the launches of one stream do not overlap)
    bool more = true;
    for (int round = 0; more; ++round) {
        more = false;
        for (int nf = 1; nf <= vdf::MAX_SHARED; ++nf) {
            vdf::Groups groups{};
            int count = 0;
            for (int q = 0; q < n_groups; ++q) {
                const int left = size[q] - round * vdf::MAX_SHARED;
                if (left > vdf::MAX_SHARED) more = true;
                if ((left > vdf::MAX_SHARED ? vdf::MAX_SHARED : left) != nf) continue;
                vdf::Group &G = groups.g[count++];
                int member = 0, taken = 0;
                for (int f = 0; f < n; ++f) {
                    if (group_of[f] != q) continue;
                    if (member >= round * vdf::MAX_SHARED && taken < nf) G.f[taken++] = fields[f];
                    ++member;
                }
                G.kappa = kappa[first[q]];
                G.t = scratch[first[q]];
                G.loc = locs[first[q]];
            }
            if (!count) continue;
            switch (nf) {
            case 1: vdf::launch_groups<1>(gd, groups, count, dt, stream); break;
            case 2: vdf::launch_groups<2>(gd, groups, count, dt, stream); break;
            case 3: vdf::launch_groups<3>(gd, groups, count, dt, stream); break;
            default: vdf::launch_groups<4>(gd, groups, count, dt, stream); break;
            }
        }
    }
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

}  // namespace ocn
