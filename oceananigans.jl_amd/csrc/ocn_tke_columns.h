// ocn_tke_columns.h -- what the two TKE-based closures (catke.hip, tke_dissipation.hip) share: ℑbzᵃᵃᶜ of TKEBasedVerticalDiffusivities.jl,
// the row of the implicit solve a substep embeds, the launch shape of their column kernels and the host checks.  What the two files still
// write out each (the shear production, the Adams-Bashforth update, the backward sweep, CATKE's own elimination) and why: DESIGN.md §5.2s.
#pragma once
#include <cmath>

#include "ocn_internal.h"

namespace ocn {

namespace tke {

// ℑbzᵃᵃᶜ of a cell from its faces lo and hi, a peripheral face (p_lo, p_hi) replaced by the other
__device__ __forceinline__ double bz(double x_lo, double x_hi, bool p_lo, bool p_hi)
{
    const double fp = p_hi ? x_lo : x_hi;
    const double fm = p_lo ? fp : x_lo;
    return (fp + fm) / 2;
}

// one unknown of a tridiagonal system: the state of its elimination
struct Elimination {
    double beta, up_prev, prev;
};

// row k of (1 - Δτ ∂z κ ∂z - Δτ L) c = c (the rows of vertical_diffusivity.hip's implicit_step_fields with the linear coefficient in the
// diagonal); returns the value left in cell k, the multiplier of a row k > 1 goes to *t
__device__ __forceinline__ double eliminate(Elimination &s, int k, int Nz, double dtau, double k_lo, double k_hi, double L, double rhs, double dzc,
                                            double dzf_lo, double dzf_hi, double *t)
{
    const double tiny = 10 * 2.220446049250313e-16;                   // 10 eps(Float64)
    const double low = k == 1 ? 0.0 : -dtau * k_lo / (dzc * dzf_lo);  // ivd_lower_diagonal(k - 1)
    const double du = -dtau * k_hi / (dzc * dzf_hi);                  // ivd_upper_diagonal(k)
    const double upk = k > Nz - 1 ? 0.0 : du;
    const double diag = 1.0 - dtau * L - upk - low;
    if (k == 1) {
        s.beta = diag;
        s.prev = rhs / s.beta;
    } else {
        const double m = s.up_prev / s.beta;
        s.beta = diag - low * m;
        *t = m;
        const double star = (rhs - low * s.prev) / s.beta;
        s.prev = fabs(s.beta) > tiny ? star : rhs;
    }
    s.up_prev = upk;
    return s.prev;
}

// ---- host: the launch shape (64 x 4 threads, a thread per column) and the argument checks ------------------------------------------------
inline dim3 column_blocks(const ocn_grid *grid) { return dim3((grid->Nx + 63) / 64, (grid->Ny + 3) / 4, 1); }

inline int validate_tke_grid(const ocn_grid *grid, const char *who)
{
    int st = validate_grid_any(grid);
    if (st != OCN_SUCCESS) return st;
    OCN_REQUIRE(grid->tx == OCN_PERIODIC && grid->ty == OCN_PERIODIC && grid->tz == OCN_BOUNDED,
                "%s: needs a (Periodic, Periodic, Bounded) grid on one GPU, got topology (%d, %d, %d)", who, grid->tx, grid->ty, grid->tz);
    OCN_REQUIRE(grid->Hx >= 1 && grid->Hy >= 1 && grid->Hz >= 1, "%s: halo >= 1 required", who);
    OCN_REQUIRE(grid->Nz >= 2, "%s: Nz = %d: at least two layers are needed", who, grid->Nz);
    OCN_REQUIRE(std::isfinite(grid->Lz) && grid->Lz > 0, "%s: grid.Lz = %g must be finite and > 0", who, grid->Lz);
    return OCN_SUCCESS;
}

inline int validate_top_fluxes(const ocn_bc *const *tops, const char *const *names, int n, const char *who)
{
    for (int q = 0; q < n; ++q) {
        if (!tops[q]) continue;
        OCN_REQUIRE(tops[q]->kind == OCN_BC_DEFAULT || tops[q]->kind == OCN_BC_FLUX,
                    "%s: the top condition of %s has kind %d: only a Flux (or the default, no flux) is a surface flux", who, names[q],
                    tops[q]->kind);
    }
    return OCN_SUCCESS;
}

inline int validate_finite_coefficients(const double *coefficients, size_t n, const char *who)
{
    for (size_t q = 0; q < n; ++q) OCN_REQUIRE(std::isfinite(coefficients[q]), "%s: coefficient %d of the closure is not finite", who, (int)q);
    return OCN_SUCCESS;
}

}  // namespace tke

}  // namespace ocn
