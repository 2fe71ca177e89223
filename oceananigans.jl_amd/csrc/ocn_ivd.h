// ocn_ivd.h -- what the two translation units of the vertically implicit closures share (implicit_diffusion.hip: constant ν, κ;
// vertical_diffusivity.hip: ν, κ fields): the vertical spacings read as wave-uniform scalars, and the range of a tendency launch.
#pragma once
#include "ocn_internal.h"

namespace ocn {

namespace ivd {

struct Spacings {
    double dz;
    const double *dzc, *dzf;
    int Hz;
    __device__ __forceinline__ double dzC(int k) const { return dzc ? uniform_load(dzc, k + Hz - 1) : dz; }
    __device__ __forceinline__ double dzF(int k) const { return dzf ? uniform_load(dzf, k + Hz - 1) : dz; }
};
__device__ __forceinline__ Spacings spacings_of(const GridDev &g) { return Spacings{g.dz, g.dzc, g.dzf, g.Hz}; }

struct Range {
    int i0, i1, j0, j1, k0, k1;
    int ou, ov, ow;  // first index written for Gu (in i), Gv (in j), Gw (in k)
};

__device__ __forceinline__ bool cell_of(const Range &r, int &i, int &j, int &k)
{
    i = r.i0 + blockIdx.x * 64 + threadIdx.x;
    j = r.j0 + blockIdx.y * 4 + threadIdx.y;
    k = r.k0 + blockIdx.z;
    return i <= r.i1 && j <= r.j1;
}

}  // namespace ivd

// range == NULL: the whole interior with the peripheries of Face fields excluded; else the six 1-based bounds, checked against the interior
int make_ivd_range(const ocn_grid *grid, const int32_t *range, ivd::Range &r);

}  // namespace ocn
