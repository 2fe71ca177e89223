// particles.hip -- LagrangianParticles: tracked-field sampling and advection, one thread per particle.
//   _advect_particles!, advect_particle, enforce_boundary_conditions   src/Models/LagrangianParticleTracking/lagrangian_particle_advection.jl:10-194
//   update_property!                                                   .../update_lagrangian_particle_properties.jl:6-15
//   index_binary_search, fractional_index, fractional_x/y/z_index      src/Fields/interpolate.jl:15-59, 67-83, 137-160, 171-188
//   interpolator, ϕ₁ … ϕ₈, _interpolate                                src/Fields/interpolate.jl:298-336
//
// A latency-bound gather: 24 scattered loads per particle (8 per velocity component) against a few dozen flops, so there is one build,
// without FMA contraction, whose results do not depend on the math mode and are bit for bit what the reference's operand order gives.
//
// THE ONE DEVIATION: the reference converts a fractional index to an integer and reads with @inbounds, so a NaN or far-away position
// reads outside the array.  Here every fractional index is first clamped, in floating point, to the open interval whose truncation
// and its right neighbour lie inside the parent array; an index the reference reads in bounds is inside that interval and unchanged.
#include <cmath>

#include "ocn_internal.h"

namespace ocn {

// one direction of the grid as the particle kernel sees it; [0] = Center, [1] = Face
struct ParticleAxis {
    int topo;                // OCN_PERIODIC / OCN_BOUNDED / OCN_FLAT
    int nn[2];               // stretched: number of interior nodes
    const double *nodes[2];  // stretched: the interior nodes; NULL = regular
    double x0[2], d;         // regular: first node and spacing
    double flo[2], fhi[2];   // clamp of the fractional index
    double left, right;      // the domain's edges: Face node 1 and Face node N + 1
};
struct ParticleGeom {
    ParticleAxis ax[3];
};
struct ParticleTracked {
    int n;
    int loc[OCN_PARTICLES_MAX_TRACKED];
    const double *field[OCN_PARTICLES_MAX_TRACKED];
    double *out[OCN_PARTICLES_MAX_TRACKED];
};

// interpolator(fractional_idx) = (i⁻, i⁺, ξ): `up` = i⁺ - i⁻ (0 along a Flat direction, whose interpolator is (1, 1, 0))
struct Interpolator {
    int i, up;
    double xi;
};

// fractional_index(val, vec, N) with index_binary_search inlined; vec is 0-based here, the returned index 1-based like the reference's
__device__ __forceinline__ double fractional_index(double val, const double *vec, int N)
{
    int low = 0, high = N - 1;
    int i1 = -1, i2 = -1;
    while (low + 1 < high) {
        const int mid = (low + high) / 2;  // unsafe_trunc(Int, (l + h) / 2), l + h >= 0
        const double vm = vec[mid];        // vec[mid + 1] of the reference
        if (vm == val) {
            i1 = i2 = mid + 1;
            break;
        } else if (vm < val) {
            low = mid;
        } else {
            high = mid;
        }
    }
    if (i1 < 0) {
        i1 = low + 1;
        i2 = high + 1;
    }
    const double x1 = vec[i1 - 1], x2 = vec[i2 - 1];
    const double ii = (double)(i2 - i1) / (x2 - x1) * (val - x1) + (double)i1;
    return i1 == i2 ? (double)i1 : ii;
}

__device__ __forceinline__ Interpolator particle_interpolator(const ParticleAxis &a, int face, double x)
{
    Interpolator r;
    if (a.topo == OCN_FLAT) {
        r.i = 1; r.up = 0; r.xi = 0.0;
        return r;
    }
    double f;
    if (a.nodes[face])
        f = fractional_index(x, a.nodes[face], a.nn[face]);
    else
        f = (x - a.x0[face]) / a.d + 1;
    f = fmin(fmax(f, a.flo[face]), a.fhi[face]);  // (fmax / fmin return the bound for a NaN)
    r.i = (int)f;  // truncation towards zero
    r.up = 1;
    double m = fmod(f, 1.0);  // mod(f, 1): the sign of the divisor
    if (m == 0.0)
        m = 0.0;
    else if (m < 0.0)
        m = m + 1.0;
    r.xi = m;
    return r;
}

// _interpolate: ϕ₁ … ϕ₈ in the reference's order, each product left-associated, summed left to right
// the Center and the Face interpolator of one direction; at(face): a select per member, so that everything stays in registers
struct InterpolatorPair {
    Interpolator c, f;
    __device__ __forceinline__ Interpolator at(int face) const
    {
        Interpolator r;
        r.i = face ? f.i : c.i;
        r.up = face ? f.up : c.up;
        r.xi = face ? f.xi : c.xi;
        return r;
    }
};
__device__ __forceinline__ double particle_interpolate(const GridDev &g, const double *data, int loc, const InterpolatorPair &X,
                                                       const InterpolatorPair &Y, const InterpolatorPair &Z)
{
    const Lay L = make_lay(g, loc);
    const Interpolator ix = X.at(loc & 1), iy = Y.at(loc & 2), iz = Z.at(loc & 4);
    const long long o = at(L, ix.i, iy.i, iz.i);
    const long long di = ix.up, dj = iy.up * L.s2, dk = iz.up * L.s3;
    const double xi = ix.xi, eta = iy.xi, zeta = iz.xi;
    double s = (1 - xi) * (1 - eta) * (1 - zeta) * data[o];
    s = s + (1 - xi) * (1 - eta) * zeta * data[o + dk];
    s = s + (1 - xi) * eta * (1 - zeta) * data[o + dj];
    s = s + (1 - xi) * eta * zeta * data[o + dj + dk];
    s = s + xi * (1 - eta) * (1 - zeta) * data[o + di];
    s = s + xi * (1 - eta) * zeta * data[o + di + dk];
    s = s + xi * eta * (1 - zeta) * data[o + di + dj];
    s = s + xi * eta * zeta * data[o + di + dj + dk];
    return s;
}

__device__ __forceinline__ double enforce_boundary_conditions(int topo, double x, double xL, double xR, double Cr)
{
    if (topo == OCN_BOUNDED) return x > xR ? xR - Cr * (x - xR) : (x < xL ? xL + Cr * (xL - x) : x);
    if (topo == OCN_PERIODIC) return x > xR ? xL + (x - xR) : (x < xL ? xR - (xL - x) : x);
    return x;
}

template <bool ADVECT>
__global__ __launch_bounds__(256) void particles_kernel(GridDev g, ParticleGeom G, long long n, double *__restrict__ x, double *__restrict__ y,
                                                        double *__restrict__ z, double Cr, const double *__restrict__ u,
                                                        const double *__restrict__ v, const double *__restrict__ w, double dt,
                                                        ParticleTracked T)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const double xp = x[p], yp = y[p], zp = z[p];
    InterpolatorPair X, Y, Z;
    X.c = particle_interpolator(G.ax[0], 0, xp); X.f = particle_interpolator(G.ax[0], 1, xp);
    Y.c = particle_interpolator(G.ax[1], 0, yp); Y.f = particle_interpolator(G.ax[1], 1, yp);
    Z.c = particle_interpolator(G.ax[2], 0, zp); Z.f = particle_interpolator(G.ax[2], 1, zp);
#pragma unroll
    for (int q = 0; q < OCN_PARTICLES_MAX_TRACKED; ++q)
        if (q < T.n) T.out[q][p] = particle_interpolate(g, T.field[q], T.loc[q], X, Y, Z);
    if (!ADVECT) return;
    const double up = particle_interpolate(g, u, OCN_LOC_FCC, X, Y, Z);
    const double vp = particle_interpolate(g, v, OCN_LOC_CFC, X, Y, Z);
    const double wp = particle_interpolate(g, w, OCN_LOC_CCF, X, Y, Z);
    // (x_metric = y_metric = 1 on a RectilinearGrid)
    const double xn = xp + up * dt, yn = yp + vp * dt, zn = zp + wp * dt;
    x[p] = enforce_boundary_conditions(G.ax[0].topo, xn, G.ax[0].left, G.ax[0].right, Cr);
    y[p] = enforce_boundary_conditions(G.ax[1].topo, yn, G.ax[1].left, G.ax[1].right, Cr);
    z[p] = enforce_boundary_conditions(G.ax[2].topo, zn, G.ax[2].left, G.ax[2].right, Cr);
}

int launch_particles(const ocn_grid *grid, const ocn_particle_geometry *geom, long long n, double *x, double *y, double *z, int advect,
                     double restitution, const double *u, const double *v, const double *w, double dt, int n_tracked,
                     const double *const *tracked_fields, const int32_t *tracked_locs, double *const *tracked_out, hipStream_t stream)
{
    const GridDev g = to_dev(*grid);
    const int N[3] = {g.Nx, g.Ny, g.Nz}, H[3] = {g.Hx, g.Hy, g.Hz}, topo[3] = {g.tx, g.ty, g.tz};
    const double D[3] = {g.dx, g.dy, g.dz};
    ParticleGeom G{};
    for (int d = 0; d < 3; ++d) {
        ParticleAxis &a = G.ax[d];
        a.topo = topo[d];
        a.d = D[d];
        a.x0[0] = geom->center0[d];
        a.x0[1] = geom->face0[d];
        a.left = geom->face0[d];
        a.right = geom->right[d];
        for (int face = 0; face < 2; ++face) {
            // parent indices (1-based interior) run from 1 - H to N + H, one more for a Face field along a Bounded direction;
            // trunc(f) >= L and trunc(f) + 1 <= U  <=>  f in (L - 1, U) for L <= 0, [L, U) for L >= 1
            const int L = 1 - H[d], U = N[d] + H[d] + ((face && topo[d] == OCN_BOUNDED) ? 1 : 0);
            a.flo[face] = L <= 0 ? std::nextafter((double)(L - 1), HUGE_VAL) : (double)L;
            a.fhi[face] = std::nextafter((double)U, -HUGE_VAL);
        }
    }
    if (grid->dzc && topo[2] != OCN_FLAT) {
        ParticleAxis &a = G.ax[2];
        a.nodes[0] = geom->zc; a.nn[0] = g.Nz;
        a.nodes[1] = geom->zf; a.nn[1] = topo[2] == OCN_BOUNDED ? g.Nz + 1 : g.Nz;
    }
    ParticleTracked T{};
    T.n = n_tracked;
    for (int q = 0; q < n_tracked; ++q) {
        T.field[q] = tracked_fields[q];
        T.loc[q] = tracked_locs[q];
        T.out[q] = tracked_out[q];
    }
    const dim3 block(256, 1, 1), nb((unsigned)((n + 255) / 256), 1, 1);
    if (advect)
        hipLaunchKernelGGL(particles_kernel<true>, nb, block, 0, stream, g, G, n, x, y, z, restitution, u, v, w, dt, T);
    else
        hipLaunchKernelGGL(particles_kernel<false>, nb, block, 0, stream, g, G, n, x, y, z, restitution, u, v, w, dt, T);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

}  // namespace ocn
