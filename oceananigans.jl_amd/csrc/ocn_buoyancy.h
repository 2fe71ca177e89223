// ocn_buoyancy.h -- the buoyancy of the vertical closures (vertical_diffusivity.hip, ri_based_diffusivity.hip, catke.hip,
// tke_dissipation.hip, isopycnal.hip): which tracers a buoyancy kind reads, its derivatives and its top flux.  DESIGN.md §5.2s.
#pragma once
#include "ocn_internal.h"

namespace ocn {

struct Buoyancy {
    int kind;
    double g, alpha, beta;
    const double *T, *S;  // NULL: a constant, its derivatives and its flux are 0
};
// ... with the top conditions of its tracers.  The base comes first: the kernel arguments are laid out as one flat struct
struct SurfaceBuoyancy : Buoyancy {
    ZBc top_T, top_S;  // kind OCN_BC_FLUX, or OCN_BC_DEFAULT: no flux
};
static_assert(sizeof(SurfaceBuoyancy) == sizeof(Buoyancy) + 2 * sizeof(ZBc), "SurfaceBuoyancy: no padding behind the base");

// a derivative of the buoyancy from the same derivative of T (or b) and S   (buoyancy_tracer.jl:14-16, seawater_buoyancy.jl:167-224)
__device__ __forceinline__ double b_of(const Buoyancy &b, double dT, double dS)
{
    if (b.kind == OCN_BUOYANCY_NONE) return 0.0;
    if (b.kind == OCN_BUOYANCY_TRACER) return dT;
    return b.g * (b.alpha * dT - b.beta * dS);
}

// ∂z_b at a face from the values above and below it (seawater_buoyancy.jl:219-224, buoyancy_tracer.jl:16)
__device__ __forceinline__ double dz_b(const Buoyancy &b, double T1, double T0, double S1, double S0, double dzf)
{
    if (b.kind == OCN_BUOYANCY_NONE) return 0.0;
    const double dT = b.T ? (T1 - T0) / dzf : 0.0;
    if (b.kind == OCN_BUOYANCY_TRACER) return dT;
    const double dS = b.S ? (S1 - S0) / dzf : 0.0;
    return b.g * (b.alpha * dT - b.beta * dS);
}

// top_buoyancy_flux (seawater_buoyancy.jl:234-246, buoyancy_tracer.jl:18): T_top, S_top are the tracers in the top cell
__device__ __forceinline__ double top_buoyancy_flux(const SurfaceBuoyancy &b, int i, int j, int Nx, double T_top, double S_top)
{
    if (b.kind == OCN_BUOYANCY_NONE) return 0.0;
    const double JT = (b.T && b.top_T.kind == OCN_BC_FLUX) ? bc_condition(b.top_T, i, j, Nx, T_top) : 0.0;
    if (b.kind == OCN_BUOYANCY_TRACER) return JT;
    const double JS = (b.S && b.top_S.kind == OCN_BC_FLUX) ? bc_condition(b.top_S, i, j, Nx, S_top) : 0.0;
    return b.g * (b.alpha * JT - b.beta * JS);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
inline bool buoyancy_reads_T(int kind) { return kind == OCN_BUOYANCY_TRACER || kind == OCN_BUOYANCY_SEAWATER_TS || kind == OCN_BUOYANCY_SEAWATER_T; }
inline bool buoyancy_reads_S(int kind) { return kind == OCN_BUOYANCY_SEAWATER_TS || kind == OCN_BUOYANCY_SEAWATER_S; }

inline Buoyancy make_buoyancy(const ocn_model_terms *terms)
{
    return Buoyancy{terms->buoyancy, terms->g, terms->alpha, terms->beta, buoyancy_reads_T(terms->buoyancy) ? terms->T : nullptr,
                    buoyancy_reads_S(terms->buoyancy) ? terms->S : nullptr};
}

// a Flux condition as it is, anything else (a NULL too) as no flux
inline ZBc flux_or_default(const ocn_bc *bc)
{
    if (bc && bc->kind == OCN_BC_FLUX) return ZBc{OCN_BC_FLUX, bc->value, bc->coeff, bc->values};
    return ZBc{OCN_BC_DEFAULT, 0.0, 0.0, nullptr};
}

inline SurfaceBuoyancy make_surface_buoyancy(const ocn_model_terms *terms, const ocn_bc *top_T, const ocn_bc *top_S)
{
    return SurfaceBuoyancy{make_buoyancy(terms), flux_or_default(top_T), flux_or_default(top_S)};
}

inline int validate_buoyancy_terms(const ocn_model_terms *terms, const char *who)
{
    OCN_REQUIRE(terms, "%s: null terms", who);
    const int b = terms->buoyancy;
    OCN_REQUIRE(b >= OCN_BUOYANCY_NONE && b <= OCN_BUOYANCY_SEAWATER_S, "%s: unknown buoyancy %d", who, b);
    if (buoyancy_reads_T(b)) OCN_REQUIRE(terms->T != nullptr, "%s: the T (or b) tracer is NULL", who);
    if (buoyancy_reads_S(b)) OCN_REQUIRE(terms->S != nullptr, "%s: the S tracer is NULL", who);
    return OCN_SUCCESS;
}

}  // namespace ocn
