// isopycnal.hip -- IsopycnalSkewSymmetricDiffusivity (turbulence_closure_implementations/isopycnal_skew_symmetric_diffusivity.jl,
// advective_skew_diffusion.jl, isopycnal_rotation_tensor_components.jl): Gent-McWilliams skew transport and Redi diffusion along isopycnals with
// the SmallSlopeIsopycnalTensor, FluxTapering and the vertically implicit time discretization, on a (Periodic, Periodic, Bounded) grid with
// regular x and y.  Number coefficients.
//
//  diffusivity_columns   compute_tapered_R₃₃! (:134-143) and _compute_eddy_velocities! (advective_skew_diffusion.jl:26-76) over i = 1..Nx,
//                        j = 1..Ny, faces k = 1..Nz, one launch: ϵ_R₃₃ = tapering_factorᶜᶜᶠ · R₃₃, uₑ = -∂z(κ Sxᶠᶜᶠ), vₑ = -∂z(κ Syᶜᶠᶠ),
//                        wₑ = ∂x(κ Sxᶠᶜᶠ) + ∂y(κ Syᶜᶠᶠ), and κz = ϵ_R₃₃ · κ_symmetric for every distinct κ_symmetric (:327-332).  A thread owns a
//                        column and marches upwards (the shape of ri_based_diffusivity.hip): ∂x b, ∂y b of a plane and ∂z b of a face are
//                        formed once and carried from face to face.  wₑ on faces 1 and Nz + 1 is what the halo fill of the reference leaves
//                        there: 0 (the Impenetrable condition of VelocityFields' w, fill_halo_regions_open.jl:65-70).
//  sum_velocities        SumOfArrays{2}(u, uₑ) (Utils/sum_of_arrays.jl:23) materialized over the whole parents, halos included.
//  isopycnal_fluxes      Gc -= 1 / V (δx(Ax qx) + δy(Ay qy) + δz(Az qz)) with diffusive_flux_x / y / z (:229-314) for up to two tracers of a
//                        launch.  A workgroup owns a 32 x 8 tile of the xy plane and marches a chunk of planes.  Per plane, through LDS: the raw
//                        values of the plane on the tile and one ring; from them ∂x, ∂y of the plane and ∂z of the face below it for the
//                        buoyancy (formed from T and S as the reference forms it: g (α ∂T - β ∂S)) and for every tracer, two planes of each
//                        kept; then the fluxes on the 33 x 8 x faces, the 32 x 9 y faces (one thread each: 320 threads) and the z face above
//                        every cell, where ϵ and R₁₃, R₂₃, R₃₁, R₃₂ are computed once per face and used for every tracer; then the divergence.
//                        The z flux below a cell is the one computed above the cell beneath it (a register).  Fluxes through faces 1 and
//                        Nz + 1 come from the formula and the filled halos, as in the reference.
//
// Division-bound rather than bandwidth-bound (a strict IEEE division per derivative): keeping the derivatives in LDS instead of the raw
// planes is what makes every one of them be formed once per point rather than once per face that reads it.
// One strict build (no FMA contraction, IEEE division): bit-identical to tests/isopycnal_numpy.py.  Julia's min, max and ifelse are
// comparisons and selects; the 0 / 0 and x / 0 that the reference selects away are computed and selected away here too.  The buoyancy is
// that of ocn_buoyancy.h.
#include "ocn_buoyancy.h"
#include "ocn_ivd.h"

namespace ocn {

namespace iso {

using ivd::Spacings;

struct Slopes {
    double max_slope2;  // slope_limiter.max_slope^2
    double minimum_bz;  // isopycnal_tensor.minimum_bz
};

// Julia's max(a, b) and min(1, x) for Float64: a NaN propagates, max(-0.0, 0.0) is 0.0
__device__ __forceinline__ double jl_max(double a, double b)
{
    if (a != a) return a;
    if (b != b) return b;
    if (a > b) return a;
    if (b > a) return b;
    return __builtin_signbit(a) ? b : a;
}
__device__ __forceinline__ double min_one(double x) { return x != x ? x : (x < 1.0 ? x : 1.0); }

// calc_tapering (:201-212)
__device__ __forceinline__ double tapering(const Slopes &s, double bx, double by, double bz)
{
    bz = jl_max(bz, s.minimum_bz);
    const double slope_x = -bx / bz, slope_y = -by / bz;
    const double slope2 = bz <= 0 ? 0.0 : slope_x * slope_x + slope_y * slope_y;
    return min_one(s.max_slope2 / slope2);
}
// isopycnal_rotation_tensor_xz / yz (isopycnal_rotation_tensor_components.jl:66-112): bh is ∂x b or ∂y b at the component's location
__device__ __forceinline__ double rotation(const Slopes &s, double bh, double bz)
{
    bz = jl_max(bz, s.minimum_bz);
    const double slope = -bh / bz;
    return bz == 0 ? 0.0 : slope;
}
// isopycnal_rotation_tensor_zz_ccf (:114-127)
__device__ __forceinline__ double rotation_zz(const Slopes &s, double bx, double by, double bz)
{
    bz = jl_max(bz, s.minimum_bz);
    const double slope_x = -bx / bz, slope_y = -by / bz;
    const double slope2 = slope_x * slope_x + slope_y * slope_y;
    return bz == 0 ? 0.0 : slope2;
}
// Sxᶠᶜᶠ, Syᶜᶠᶠ (advective_skew_diffusion.jl:27-56): tapered on its own, no minimum_bz, 0 on the peripheral faces
__device__ __forceinline__ double tapered_slope(const Slopes &s, double bh, double bz, bool inactive)
{
    double S = bz == 0 ? 0.0 : -bh / bz;
    const double eps = min_one(s.max_slope2 / (S * S));
    S = inactive ? 0.0 : S;
    return eps * S;
}

// ---- compute_diffusivities! -----------------------------------------------------------------------------------------------------------------
constexpr int MAX_KZ = OCN_MODEL_MAX_TRACERS;

struct DiffArgs {
    double kappa_skew;
    double *eps, *ue, *ve, *we;
    int n_kz;
    double ks[MAX_KZ];
    double *kz[MAX_KZ];
};

// the values of one plane at the column and its four neighbours
struct Cross {
    double c, w, e, s, n;
};
__device__ __forceinline__ Cross load_cross(const double *p, long long o, long long s2)
{
    if (!p) return Cross{0.0, 0.0, 0.0, 0.0, 0.0};
    return Cross{p[o], p[o - 1], p[o + 1], p[o - s2], p[o + s2]};
}

template <bool EDDY>
__global__ __launch_bounds__(256) void diffusivity_columns(GridDev g, Buoyancy b, Slopes sl, DiffArgs a)
{
    const int i = 1 + blockIdx.x * 64 + threadIdx.x, j = 1 + blockIdx.y * 4 + threadIdx.y;
    if (i > g.Nx || j > g.Ny) return;
    const int Nz = g.Nz;
    const Spacings M = ivd::spacings_of(g);
    const Lay Lc = make_lay(g, OCN_LOC_CCC), Lf = make_lay(g, OCN_LOC_CCF);  // Periodic x and y: u, v and c share one parent layout
    const long long c3 = Lc.s3, c2 = Lc.s2, f3 = Lf.s3;
    const long long oc = at(Lc, i, j, 0), of = at(Lf, i, j, 1);
    const double dx = g.dx, dy = g.dy;
    // plane k - 1 and its horizontal derivatives: ∂x b at faces i, i + 1 and ∂y b at faces j, j + 1
    Cross T0 = load_cross(b.T, oc, c2), S0 = load_cross(b.S, oc, c2);
    auto dxb_w = [&](const Cross &T, const Cross &S) { return b_of(b, (T.c - T.w) / dx, (S.c - S.w) / dx); };
    auto dxb_e = [&](const Cross &T, const Cross &S) { return b_of(b, (T.e - T.c) / dx, (S.e - S.c) / dx); };
    auto dyb_s = [&](const Cross &T, const Cross &S) { return b_of(b, (T.c - T.s) / dy, (S.c - S.s) / dy); };
    auto dyb_n = [&](const Cross &T, const Cross &S) { return b_of(b, (T.n - T.c) / dy, (S.n - S.c) / dy); };
    double bxw0 = dxb_w(T0, S0), bxe0 = dxb_e(T0, S0), bys0 = dyb_s(T0, S0), byn0 = dyb_n(T0, S0);
    double kSx0 = 0.0, kSy0 = 0.0;  // κ Sxᶠᶜᶠ at (i, j), κ Syᶜᶠᶠ at (i, j) of the face below
    for (int k = 1; k <= Nz + 1; ++k) {
        const Cross T1 = load_cross(b.T, oc + k * c3, c2), S1 = load_cross(b.S, oc + k * c3, c2);
        const double dzf = M.dzF(k);
        const double bxw1 = dxb_w(T1, S1), bxe1 = dxb_e(T1, S1), bys1 = dyb_s(T1, S1), byn1 = dyb_n(T1, S1);
        const double bzc = b_of(b, (T1.c - T0.c) / dzf, (S1.c - S0.c) / dzf);
        if (k <= Nz) {
            // ℑxzᶜᵃᶠ(∂x_b) = ℑzᵃᵃᶠ(ℑxᶜᵃᵃ ∂x_b), ℑyzᵃᶜᶠ(∂y_b) = ℑzᵃᵃᶠ(ℑyᵃᶜᵃ ∂y_b)
            const double bx = 0.5 * (0.5 * (bxw0 + bxe0) + 0.5 * (bxw1 + bxe1));
            const double by = 0.5 * (0.5 * (bys0 + byn0) + 0.5 * (bys1 + byn1));
            const double eR33 = tapering(sl, bx, by, bzc) * rotation_zz(sl, bx, by, bzc);
            a.eps[of + (k - 1) * f3] = eR33;
            for (int q = 0; q < a.n_kz; ++q) a.kz[q][of + (k - 1) * f3] = eR33 * a.ks[q];
        }
        if (EDDY) {
            const double bzw = b_of(b, (T1.w - T0.w) / dzf, (S1.w - S0.w) / dzf), bze = b_of(b, (T1.e - T0.e) / dzf, (S1.e - S0.e) / dzf);
            const double bzs = b_of(b, (T1.s - T0.s) / dzf, (S1.s - S0.s) / dzf), bzn = b_of(b, (T1.n - T0.n) / dzf, (S1.n - S0.n) / dzf);
            const bool inactive = k == 1 || k == Nz + 1;  // peripheral_node(i, j, k, grid, f, c, f) and (c, f, f)
            // bx = ℑzᵃᵃᶠ(∂x_b), bz = ℑxᶠᵃᵃ(∂z_b) at (i, j) and at (i + 1, j); the same in y
            const double kSx1 = a.kappa_skew * tapered_slope(sl, 0.5 * (bxw0 + bxw1), 0.5 * (bzw + bzc), inactive);
            const double kSxe = a.kappa_skew * tapered_slope(sl, 0.5 * (bxe0 + bxe1), 0.5 * (bzc + bze), inactive);
            const double kSy1 = a.kappa_skew * tapered_slope(sl, 0.5 * (bys0 + bys1), 0.5 * (bzs + bzc), inactive);
            const double kSyn = a.kappa_skew * tapered_slope(sl, 0.5 * (byn0 + byn1), 0.5 * (bzc + bzn), inactive);
            // the Impenetrable condition of wₑ on the two boundary faces (the open fill of the halo fill that follows)
            a.we[of + (k - 1) * f3] = inactive ? 0.0 : (kSxe - kSx1) / dx + (kSyn - kSy1) / dy;
            if (k >= 2) {
                const double dzc = M.dzC(k - 1);
                a.ue[oc + (k - 1) * c3] = -((kSx1 - kSx0) / dzc);
                a.ve[oc + (k - 1) * c3] = -((kSy1 - kSy0) / dzc);
            }
            kSx0 = kSx1; kSy0 = kSy1;
        }
        T0 = T1; S0 = S1;
        bxw0 = bxw1; bxe0 = bxe1; bys0 = bys1; byn0 = byn1;
    }
}

// ---- the total velocities of the tracer advection ---------------------------------------------------------------------------------------------
struct SumArgs {
    const double *a[3], *b[3];
    double *out[3];
    long long n[3];
};
__global__ __launch_bounds__(256) void sum_velocities(SumArgs s)
{
    const int f = blockIdx.y;
    const double *__restrict__ x = s.a[f], *__restrict__ y = s.b[f];
    double *__restrict__ out = s.out[f];
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < s.n[f]; t += (long long)gridDim.x * blockDim.x) out[t] = x[t] + y[t];
}

// ---- the flux divergence ----------------------------------------------------------------------------------------------------------------------
constexpr int TX = 32, TY = 8, NT = 320;
constexpr int RX = TX + 2, RY = TY + 2, NRING = RX * RY;  // the tile and one ring
constexpr int RPT = (NRING + NT - 1) / NT;                // ring points per thread
constexpr int NXF = (TX + 1) * TY, NYF = TX * (TY + 1);   // x faces, y faces of a tile
constexpr int PLANES = 16;                                // planes marched by one workgroup
constexpr int MAXT = 2;                                   // tracers of one launch
static_assert(NXF <= NT && NYF <= NT && TX * TY <= NT, "one thread per face");

template <int NTR>
struct FluxArgs {
    const double *f[2 + NTR];  // the raw fields: T (or b), S, then the tracers that are neither (NULL: zeros)
    int src[NTR];              // the raw field of tracer n
    double ks[NTR], kw[NTR];   // κ_symmetric, κ_skew (0 with the advective formulation) of tracer n
    double *G[NTR];
    int nt;                    // tracers in use, 1..NTR
};

template <int NTR>
__global__ __launch_bounds__(NT) void isopycnal_fluxes(GridDev g, Buoyancy b, Slopes sl, FluxArgs<NTR> a)
{
    constexpr int NF = 2 + NTR, NSET = 1 + NTR;  // set 0: the buoyancy; set 1 + n: tracer n
    __shared__ double raw[NF][NRING];
    __shared__ double D[NSET][3][2][NRING];      // [set][∂x at fcc, ∂y at cfc, ∂z at ccf][plane or face & 1][ring point]
    __shared__ double fx[NTR][NXF], fy[NTR][NYF];

    const int tid = threadIdx.x;
    const int i0 = 1 + blockIdx.x * TX, j0 = 1 + blockIdx.y * TY;
    const int k0 = 1 + blockIdx.z * PLANES, k1 = min(k0 + PLANES - 1, g.Nz);
    const Spacings M = ivd::spacings_of(g);
    const Lay L = make_lay(g, OCN_LOC_CCC);
    const double dx = g.dx, dy = g.dy;

    // this thread's ring points: (i0 - 1 + ra, j0 - 1 + rb); offsets within plane 1, -1 beyond the first halo cell
    long long ring_off[RPT];
#pragma unroll
    for (int q = 0; q < RPT; ++q) {
        const int p = tid + q * NT, i = i0 - 1 + p % RX, j = j0 - 1 + p / RX;
        ring_off[q] = (p < NRING && i <= g.Nx + 1 && j <= g.Ny + 1) ? at(L, i, j, 1) : -1;
    }
    double rc[NF][RPT], rn[NF][RPT], rp[NF][RPT] = {};  // planes k, k + 1, k + 2
    auto load_plane = [&](double (&r)[NF][RPT], int k) {
        const long long ok = L.s3 * (k - 1);
#pragma unroll
        for (int f = 0; f < NF; ++f)
#pragma unroll
            for (int q = 0; q < RPT; ++q) r[f][q] = (a.f[f] && ring_off[q] >= 0) ? a.f[f][ring_off[q] + ok] : 0.0;
    };
    auto store_raw = [&](const double (&r)[NF][RPT]) {
#pragma unroll
        for (int f = 0; f < NF; ++f)
#pragma unroll
            for (int q = 0; q < RPT; ++q)
                if (tid + q * NT < NRING) raw[f][tid + q * NT] = r[f][q];
    };
    // ∂x, ∂y of plane pl from the raw plane in LDS and (with_dz) ∂z of face pl from the registers of planes pl and pl - 1, into slot pl & 1
    auto derive = [&](int pl, bool with_dz, const double (&hi)[NF][RPT], const double (&lo)[NF][RPT]) {
        const int s = pl & 1;
        const double dzf = with_dz ? M.dzF(pl) : 1.0;
#pragma unroll
        for (int q = 0; q < RPT; ++q) {
            const int p = tid + q * NT;
            if (p >= NRING) continue;
            const int pw = p % RX >= 1 ? p - 1 : p, ps = p / RX >= 1 ? p - RX : p;  // (the first column / row has no face to its west / south)
            double gx[NF], gy[NF], gz[NF];
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                gx[f] = (raw[f][p] - raw[f][pw]) / dx;
                gy[f] = (raw[f][p] - raw[f][ps]) / dy;
                gz[f] = with_dz ? (hi[f][q] - lo[f][q]) / dzf : 0.0;
            }
            D[0][0][s][p] = b_of(b, gx[0], gx[1]);
            D[0][1][s][p] = b_of(b, gy[0], gy[1]);
            D[0][2][s][p] = b_of(b, gz[0], gz[1]);
#pragma unroll
            for (int n = 0; n < NTR; ++n) {
                double tx = gx[2], ty = gy[2], tz = gz[2];
#pragma unroll
                for (int f = 0; f < NF; ++f)
                    if (a.src[n] == f) { tx = gx[f]; ty = gy[f]; tz = gz[f]; }
                D[1 + n][0][s][p] = tx;
                D[1 + n][1][s][p] = ty;
                D[1 + n][2][s][p] = tz;
            }
        }
    };

    const int ca = tid % TX, cb = tid / TX;  // this thread's cell (tid < TX * TY)
    const bool cell = tid < TX * TY && i0 + ca <= g.Nx && j0 + cb <= g.Ny;
    const long long cell_off = cell ? at(L, i0 + ca, j0 + cb, 1) : 0;
    double fz_below[NTR] = {}, fz_above[NTR] = {};

    load_plane(rc, k0 - 1);
    load_plane(rn, k0);
    store_raw(rc);
    __syncthreads();
    derive(k0 - 1, false, rc, rc);
    __syncthreads();
    for (int k = k0 - 1; k <= k1; ++k) {
        store_raw(rn);  // plane k + 1
        __syncthreads();
        if (k + 2 <= k1 + 1) load_plane(rp, k + 2);
        OCN_ISSUE_LOADS_HERE();
        derive(k + 1, true, rn, rc);
        __syncthreads();
        const int s0 = k & 1, s1 = (k + 1) & 1;  // plane k and the face below it; plane k + 1 and the face above plane k

        if (tid < TX * TY) {  // diffusive_flux_z at (c, c, f), face k + 1 (:289-314)
            const int r = (cb + 1) * RX + ca + 1;
            auto at_face = [&](int set, double &hx, double &hy, double &hz) {
                const double(*d)[2][NRING] = D[set];
                hx = 0.5 * (0.5 * (d[0][s0][r] + d[0][s0][r + 1]) + 0.5 * (d[0][s1][r] + d[0][s1][r + 1]));    // ℑxzᶜᵃᶠ
                hy = 0.5 * (0.5 * (d[1][s0][r] + d[1][s0][r + RX]) + 0.5 * (d[1][s1][r] + d[1][s1][r + RX]));  // ℑyzᵃᶜᶠ
                hz = d[2][s1][r];
            };
            double bx, by, bz;
            at_face(0, bx, by, bz);
            const double eps = tapering(sl, bx, by, bz), R31 = rotation(sl, bx, bz), R32 = rotation(sl, by, bz);
#pragma unroll
            for (int n = 0; n < NTR; ++n) {
                double cx, cy, cz;
                at_face(1 + n, cx, cy, cz);
                const double kk = a.ks[n] + a.kw[n];
                fz_above[n] = (-eps) * 0.0 - eps * ((kk * R31) * cx + (kk * R32) * cy);  // (explicit_κ_∂z_c is 0 when vertically implicit)
            }
        }
        if (k >= k0) {
            if (tid < NXF) {  // diffusive_flux_x at (f, c, c) (:229-256)
                const int r = (tid / (TX + 1) + 1) * RX + tid % (TX + 1) + 1;
                auto at_face = [&](int set, double &hx, double &hy, double &hz) {
                    const double(*d)[2][NRING] = D[set];
                    hx = d[0][s0][r];
                    hy = 0.5 * (0.5 * (d[1][s0][r - 1] + d[1][s0][r]) + 0.5 * (d[1][s0][r + RX - 1] + d[1][s0][r + RX]));  // ℑxyᶠᶜᵃ
                    hz = 0.5 * (0.5 * (d[2][s0][r - 1] + d[2][s0][r]) + 0.5 * (d[2][s1][r - 1] + d[2][s1][r]));            // ℑxzᶠᵃᶜ
                };
                double bx, by, bz;
                at_face(0, bx, by, bz);
                const double eps = tapering(sl, bx, by, bz), R13 = rotation(sl, bx, bz);
#pragma unroll
                for (int n = 0; n < NTR; ++n) {
                    double cx, cy, cz;
                    at_face(1 + n, cx, cy, cz);
                    fx[n][tid] = -eps * (((a.ks[n] * 1.0) * cx + (a.ks[n] * 0.0) * cy) + ((a.ks[n] - a.kw[n]) * R13) * cz);
                }
            }
            if (tid < NYF) {  // diffusive_flux_y at (c, f, c) (:259-286)
                const int r = (tid / TX + 1) * RX + tid % TX + 1;
                auto at_face = [&](int set, double &hx, double &hy, double &hz) {
                    const double(*d)[2][NRING] = D[set];
                    hx = 0.5 * (0.5 * (d[0][s0][r - RX] + d[0][s0][r - RX + 1]) + 0.5 * (d[0][s0][r] + d[0][s0][r + 1]));  // ℑxyᶜᶠᵃ
                    hy = d[1][s0][r];
                    hz = 0.5 * (0.5 * (d[2][s0][r - RX] + d[2][s0][r]) + 0.5 * (d[2][s1][r - RX] + d[2][s1][r]));          // ℑyzᵃᶠᶜ
                };
                double bx, by, bz;
                at_face(0, bx, by, bz);
                const double eps = tapering(sl, bx, by, bz), R23 = rotation(sl, by, bz);
#pragma unroll
                for (int n = 0; n < NTR; ++n) {
                    double cx, cy, cz;
                    at_face(1 + n, cx, cy, cz);
                    fy[n][tid] = -eps * (((a.ks[n] * 0.0) * cx + (a.ks[n] * 1.0) * cy) + ((a.ks[n] - a.kw[n]) * R23) * cz);
                }
            }
            __syncthreads();
            if (cell) {  // ∇_dot_qᶜ (closure_kernel_operators.jl:43-48)
                const double dzk = M.dzC(k);
                const double Ax = dy * dzk, Ay = dx * dzk, Az = dx * dy, rV = 1 / (Az * dzk);
                const long long o = cell_off + L.s3 * (k - 1);
#pragma unroll
                for (int n = 0; n < NTR; ++n) {
                    if (n >= a.nt) break;
                    const double *qx = fx[n] + cb * (TX + 1) + ca, *qy = fy[n] + cb * TX + ca;
                    const double div = rV * (((Ax * qx[1] - Ax * qx[0]) + (Ay * qy[TX] - Ay * qy[0])) + (Az * fz_above[n] - Az * fz_below[n]));
                    a.G[n][o] = a.G[n][o] - div;
                }
            }
        }
#pragma unroll
        for (int n = 0; n < NTR; ++n) fz_below[n] = fz_above[n];
#pragma unroll
        for (int f = 0; f < NF; ++f)
#pragma unroll
            for (int q = 0; q < RPT; ++q) {
                rc[f][q] = rn[f][q];
                rn[f][q] = rp[f][q];
            }
        // raw is rewritten behind the barrier after derive; a D slot behind the barrier after store_raw, which every reader of it has
        // passed; fx, fy behind both
    }
}

template <int NTR>
static void launch_fluxes(const GridDev &gd, const Buoyancy &b, const Slopes &sl, int nt, const double *ks, const double *kw,
                          const double *const *c, double *const *G, dim3 blocks, hipStream_t stream)
{
    FluxArgs<NTR> a{};
    a.f[0] = b.T;
    a.f[1] = b.S;
    int nf = 2;
    for (int n = 0; n < NTR; ++n) {
        const int m = n < nt ? n : 0;  // (an unused slot repeats tracer 0: its fluxes are computed and dropped)
        a.ks[n] = ks[m];
        a.kw[n] = kw[m];
        a.G[n] = G[m];
        a.src[n] = -1;
        for (int f = 0; f < nf; ++f)
            if (a.f[f] == c[m]) a.src[n] = f;
        if (a.src[n] < 0) {
            a.f[nf] = c[m];
            a.src[n] = nf++;
        }
    }
    a.nt = nt;
    hipLaunchKernelGGL(isopycnal_fluxes<NTR>, blocks, dim3(NT), 0, stream, gd, b, sl, a);
}

}  // namespace iso

// the callers (capi.hip) have validated the grid ((Periodic, Periodic, Bounded), regular x and y, halos >= 1), the closure and the pointers
int launch_isopycnal_diffusivities(const ocn_grid *grid, const ocn_model_terms *terms, const ocn_isopycnal *closure, double kappa_skew,
                                   double *eps_R33, double *ue, double *ve, double *we, int n_kz, const double *kappa_symmetric,
                                   double *const *kz, hipStream_t stream)
{
    const Buoyancy b = make_buoyancy(terms);
    const iso::Slopes sl{closure->max_slope * closure->max_slope, closure->minimum_bz};
    iso::DiffArgs a{};
    a.kappa_skew = kappa_skew;
    a.eps = eps_R33; a.ue = ue; a.ve = ve; a.we = we;
    a.n_kz = n_kz;
    for (int q = 0; q < n_kz; ++q) {
        a.ks[q] = kappa_symmetric[q];
        a.kz[q] = kz[q];
    }
    const GridDev gd = to_dev(*grid);
    const dim3 block(64, 4, 1), blocks((grid->Nx + 63) / 64, (grid->Ny + 3) / 4, 1);
    if (ue)
        hipLaunchKernelGGL(iso::diffusivity_columns<true>, blocks, block, 0, stream, gd, b, sl, a);
    else
        hipLaunchKernelGGL(iso::diffusivity_columns<false>, blocks, block, 0, stream, gd, b, sl, a);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

int launch_sum_velocities(const ocn_grid *grid, const double *const *a, const double *const *b, double *const *out, hipStream_t stream)
{
    const GridDev gd = to_dev(*grid);
    const int locs[3] = {OCN_LOC_FCC, OCN_LOC_CFC, OCN_LOC_CCF};
    iso::SumArgs s{};
    long long most = 0;
    for (int f = 0; f < 3; ++f) {
        const Lay L = make_lay(gd, locs[f]);
        s.a[f] = a[f]; s.b[f] = b[f]; s.out[f] = out[f];
        s.n[f] = L.s3 * L.sz;
        most = s.n[f] > most ? s.n[f] : most;
    }
    long long nb = (most + 255) / 256;
    if (nb > 2048) nb = 2048;
    hipLaunchKernelGGL(iso::sum_velocities, dim3((unsigned)nb, 3), dim3(256), 0, stream, s);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

int launch_isopycnal_fluxes(const ocn_grid *grid, const ocn_model_terms *terms, const ocn_isopycnal *closure, int n_tracers,
                            const double *kappa_symmetric, const double *kappa_skew, const double *const *c, double *const *Gc,
                            hipStream_t stream)
{
    const Buoyancy b = make_buoyancy(terms);
    const iso::Slopes sl{closure->max_slope * closure->max_slope, closure->minimum_bz};
    const GridDev gd = to_dev(*grid);
    const dim3 blocks((grid->Nx + iso::TX - 1) / iso::TX, (grid->Ny + iso::TY - 1) / iso::TY, (grid->Nz + iso::PLANES - 1) / iso::PLANES);
    OCN_REQUIRE(blocks.y <= 65535u && blocks.z <= 65535u, "ocn_add_isopycnal_fluxes: grid too large for one launch");
    // ϵ and the rotation tensor are computed once per face and launch: two tracers share a launch, an odd one takes the narrower kernel
    for (int n = 0; n < n_tracers; n += iso::MAXT) {
        const int nt = n_tracers - n < iso::MAXT ? n_tracers - n : iso::MAXT;
        if (nt == 2)
            iso::launch_fluxes<2>(gd, b, sl, nt, kappa_symmetric + n, kappa_skew + n, c + n, Gc + n, blocks, stream);
        else
            iso::launch_fluxes<1>(gd, b, sl, nt, kappa_symmetric + n, kappa_skew + n, c + n, Gc + n, blocks, stream);
    }
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

}  // namespace ocn
