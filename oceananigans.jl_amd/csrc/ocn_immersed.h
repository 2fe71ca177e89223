// ocn_immersed.h -- the node predicates of a GridFittedBottom, for every kernel that runs over bathymetry (immersed.hip and the grid-fitted
// instantiations of hydrostatic_surface.hip).
//
// The bathymetry reaches the kernels as ONE int32 plane: kbot[i, j], the number of immersed cells of the column (cell k is immersed iff
// k <= kbot), shaped like η with periodically filled halos.  inactive_cell is monotone in kbot, so the AND over the cells a node touches is
// the predicate at the MINIMUM of their kbot and the OR the predicate at the MAXIMUM: every node predicate below is a comparison of k with
// kbot at one, two or four columns (Grids/inactive_node.jl:127-155, immersed_boundary_interface.jl:49-60).  A thread loads the kbot of its
// 3 x 3 columns once and walks KZ levels with them in registers; the z extent stays in the launch.
#pragma once
#include "ocn_common.h"

namespace ocn {

constexpr int KZ = 8;  // levels per thread (1 to 32 measured: DESIGN §5.2q)

// inactive_cell of the immersed grid (immersed, or outside 1..Nz) and of the underlying grid, for a column with kb immersed cells
__device__ __forceinline__ bool ic(int kb, int k, int Nz) { return k < 1 || k > Nz || k <= kb; }
__device__ __forceinline__ bool i0(int k, int Nz) { return k < 1 || k > Nz; }
// immersed_inactive_node / immersed_peripheral_node of a node that is Center in z (mn / mx: min / max of kbot over its columns) ...
__device__ __forceinline__ bool inactive_c(int mn, int k, int Nz) { return ic(mn, k, Nz) && !i0(k, Nz); }
__device__ __forceinline__ bool peripheral_c(int mx, int k, int Nz) { return ic(mx, k, Nz) && !i0(k, Nz); }
// ... and of one that is Face in z (it touches the cells k - 1 and k)
__device__ __forceinline__ bool inactive_f(int mn, int k, int Nz) { return ic(mn, k - 1, Nz) && ic(mn, k, Nz) && !(i0(k - 1, Nz) && i0(k, Nz)); }
__device__ __forceinline__ bool peripheral_f(int mx, int k, int Nz) { return (ic(mx, k - 1, Nz) || ic(mx, k, Nz)) && !(i0(k - 1, Nz) || i0(k, Nz)); }

// inactive_node(i, j, Nz + 1, c, c, f): the column is dry
__device__ __forceinline__ bool inactive_f_top(int kb, int Nz) { return ic(kb, Nz, Nz) && ic(kb, Nz + 1, Nz); }

__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }
inline int z_chunks(int Nz) { return (Nz + KZ - 1) / KZ; }

// kbot of the 3 x 3 columns around (i, j): kb[1 + a][1 + b] is column (i + a, j + b)
struct Cols {
    int kb[3][3];
    __device__ __forceinline__ int operator()(int a, int b) const { return kb[1 + a][1 + b]; }
};
__device__ __forceinline__ Cols load_cols(const GridDev &g, const int32_t *__restrict__ kbot, int i, int j)
{
    Cols c;
    const long long e = plane_at(g, i, j), sx = g.Nx + 2 * g.Hx;
#pragma unroll
    for (int a = -1; a <= 1; ++a)
#pragma unroll
        for (int b = -1; b <= 1; ++b) c.kb[1 + a][1 + b] = kbot[e + a + sx * b];
    return c;
}

}  // namespace ocn
