// poisson_select.h -- what a single-device pressure solver is made of, decided once at creation.
//
// choose_pipeline() turns (grid, environment, supported transform lengths) into a PoissonChoice; build_passes() turns that into the
// three ordered pass lists the handle keeps.  Neither makes a HIP or rocFFT call: everything here is plain host data, so the
// selection can be exercised without a device (tools/poisson_select_check.cpp).  After creation the entry points only walk the lists.
#pragma once
#include <cstdlib>
#include <vector>

#include "ocn_internal.h"

namespace ocn {
namespace poisson {

// every OCN_POISSON_* switch is read through one of these two, at creation
inline bool env_on(const char *name)  // on unless set to 0
{
    const char *e = std::getenv(name);
    return !(e && e[0] == '0');
}
inline bool env_set(const char *name)  // off unless set to 1
{
    const char *e = std::getenv(name);
    return e && e[0] == '1';
}

// One pass over the data: a kernel launch or a rocFFT execution (a sweep comes with its zero-mean gauge).  `cur` is the array the
// previous pass left its result in and `alt` the other one of the handle's pair; "cur -> alt" passes exchange the two afterwards.
// DESIGN.md §5.4 tabulates the kernel or plan and the bytes per element behind each name.
enum class Pass : int {
    // ---- source from velocities (ocn_poisson_compute_source_term)
    SourceTerm,            // div(U) / Δt into cur or rhs: mode = SourceOut, d2 = direction stored gathered (-1: none), wrap
    SourceTermStretched,   // Δξᶜ div(U) / Δt on the stretched x / y spacing (d), d2 as above
    SourceRowFFT,          // div(U) / Δt fused with the forward x transform of the row kernel: mode = scale by Δzᶜ, wrap
    // ---- source given as an array (ocn_poisson_set_source_term)
    SetSource,             // R [Δzᶜ when mode] into cur or rhs, widened to complex when mode2
    SetSourceUniformDz,    // the same with the one Δz of a regular z
    SetSourceStretched,    // R Δξᶜ of the stretched x / y (d)
    // ---- solve (ocn_poisson_solve)
    RowFFTOfRealSource,    // x transform of a source that set_source_term left in rhs; skipped when the source pass already did it
    FFTForward,            // rocFFT complex plan, in place
    FFTRealForward,        // rocFFT real plan, rhs -> cur
    FFTInverse,            // rocFFT complex plan, in place
    FFTRealInverseToField, // rocFFT real plan, cur -> interior of the pressure field
    FFTRealInverseAndCopy, // rocFFT real plan, cur -> rhs, then the copy into the pressure field
    ColumnFFT,             // column kernel along d (1 or 2): mode = ColFFT::Forward / Inverse, scale
    ColumnFFTSolve,        // column kernel along z: forward, division by the eigenvalues, inverse; scale
    ColumnDCT,             // column kernel along d: mode = ColFFT::DctForward / DctInverse, scale
    ColumnDCTSolve,        // column kernel along z: REDFT10, division, REDFT01; scale
    ColumnDCTToField,      // inverse cosine transform along d stored straight into the pressure field; scale
    LineFFT,               // rocFFT lines along d, in place (one execution per z plane for d = 1): mode = inverse
    RealToHalf,            // rocFFT real x lines, cur -> alt (half spectrum)
    HalfToReal,            // rocFFT real x lines back, cur -> alt, scaled 1 / Nx
    NaiveTransform,        // the transform along d as the direct sum of its definition, cur -> alt: mode = inverse, mode2 = topology
    Shuffle,               // dct_shuffle_kernel along d, cur -> alt: mode = DctShuffle
    TwiddlePermute,        // a twiddle along d (mode) and a permutation along d2 (mode2) in one pass, cur -> alt
    RowPair,               // dct_rowpair_kernel along x, cur -> alt: mode = DctShuffle
    RowDCT,                // row kernel along x, in place: mode = RowDCT
    SpectralSolve,         // -b / (λx + λy + λz [- m]) on a complex spectrum
    SpectralSolveReal,     // the same on a real spectrum
    SweepX,                // Thomas sweep along x + zero-mean gauge, cur -> alt
    SweepY,                // ... along y
    SweepZ,                // ... along z
    SweepZReal,            // ... along z of a real array
    RowFFTToField,         // inverse x transform of the row kernel into the rows of the pressure field; scale
    CopyReal,              // copy_real_component!: mode = CopySource, d2 = direction whose last scatter is folded into the read (-1: none)
    Count_
};

inline const char *pass_name(Pass p)
{
    static const char *const names[] = {"SourceTerm", "SourceTermStretched", "SourceRowFFT", "SetSource", "SetSourceUniformDz", "SetSourceStretched",
                                        "RowFFTOfRealSource", "FFTForward", "FFTRealForward", "FFTInverse", "FFTRealInverseToField",
                                        "FFTRealInverseAndCopy", "ColumnFFT", "ColumnFFTSolve", "ColumnDCT", "ColumnDCTSolve", "ColumnDCTToField",
                                        "LineFFT", "RealToHalf", "HalfToReal", "NaiveTransform", "Shuffle", "TwiddlePermute", "RowPair", "RowDCT",
                                        "SpectralSolve", "SpectralSolveReal", "SweepX", "SweepY", "SweepZ", "SweepZReal", "RowFFTToField", "CopyReal"};
    static_assert(sizeof(names) / sizeof(names[0]) == (size_t)Pass::Count_, "one name per pass");
    return names[(int)p];
}

struct PassRec {
    Pass pass;
    int d = 0, mode = 0;       // the direction the pass runs along and its launcher's mode
    int d2 = -1, mode2 = 0;    // a second direction / mode (see Pass)
    int n[3] = {0, 0, 0};      // extents of the array as the pass sees it (complex or real elements, as the pass reads them)
    double scale = 1.0;
    bool to_rhs = false;       // source passes: store into the real buffer rhs instead of cur
    bool wrap = false;         // source passes: read the periodic images of the first cells instead of the velocity halos
    bool skip_if_gathered = false;  // the first gather of a solve: the source pass may have stored its output already gathered
};

// What creation decided.  A local of creation: the handle keeps the pass lists, not this.
struct PoissonChoice {
    int N[3] = {0, 0, 0};
    int topo[3] = {0, 0, 0};  // per direction, with the direction of a tridiagonal sweep marked Flat (no transform along it)
    bool general = false;     // the any-topology solver (a Bounded / Flat x or y, a stretched x or y, or OCN_POISSON_GENERAL=1)
    bool tri = false;         // a Thomas sweep along `tdim` instead of a transform
    int tdim = 2;
    bool stretched_z = false;
    // ---- periodic x and y
    bool c2c = false;         // complex rocFFT plans (OCN_POISSON_C2C=1, or the real plans failed their self test)
    bool fused_z = false;     // Periodic z of a supported length: FFT_z, division and IFFT_z in one column pass  [OCN_POISSON_FUSED_Z]
    bool custom_xy = false;   // x passes by the row kernel (fused with the source term / the write into p), y passes by the column kernel
    bool custom_tri = false;  // ... around the z sweep of a Bounded z: no rocFFT  [OCN_POISSON_CUSTOM_XY]
    bool dct_z = false;       // ... whose regular z of a supported length is a cosine transform in one column pass instead  [OCN_POISSON_DCT_Z]
    bool dims3 = false;       // the rocFFT plans transform z as well
    bool direct_out = false;  // real plans: the inverse writes straight into the haloed pressure field  [OCN_POISSON_DIRECT_OUT; creation clears it
                              // when rocFFT has no kernel for the strided output]
    bool source_wrap = false; // all-periodic: the source pass wraps instead of reading halos  [OCN_POISSON_SOURCE_WRAP]
    // ---- any topology
    bool fft_dct = false;     // cosine transforms from FFTs (off: the direct sums, OCN_POISSON_NAIVE_DCT=1)
    bool packed = false;      // Periodic x next to a Bounded y / z: cosine transforms on x-adjacent pairs of reals, real x transform  [OCN_POISSON_PACKED]
    bool allreal = false;     // x and y Bounded, z Bounded / Flat: nothing becomes complex  [OCN_POISSON_PACKED]
    bool rowdct = false;      // the x lines of those two in the row kernel  [OCN_POISSON_ROW_DCT, OCN_POISSON_GENERAL_COLFFT]
    bool col[3] = {false, false, false};   // lines along d in the column kernel  [OCN_POISSON_GENERAL_COLFFT]
    bool dct[3] = {false, false, false};   // ... as a whole cosine transform in one pass  [OCN_POISSON_FUSED_DCT]
    bool lines[3] = {false, false, false}; // rocFFT line plans along d ...
    int line_n[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};  // ... of an array of these extents
    bool fuse = false;          // twiddle-then-permute in one pass, first gather in the source store, last scatter in the copy  [OCN_POISSON_FUSE_SHUFFLES]
    bool dct_to_field = false;  // a last one-pass inverse cosine transform stores into the pressure field  [OCN_POISSON_DCT_TO_FIELD]
    // ---- what ocn_poisson_info reports
    int info_kind() const { return general ? (tri ? (tdim == 0 ? 4 : tdim == 1 ? 5 : 3) : 2) : (tri ? 1 : 0); }
    int info_r2c() const { return (general || c2c) ? 0 : 1; }
    int info_direct_out() const { return general ? 0 : (!c2c && direct_out) + 2 * (fused_z ? 1 : 0) + 4 * (custom_xy ? 1 : 0) + 8 * (dct_z ? 1 : 0); }
    // stage order of the column kernel along d: eigenvalues, cosine twiddles and partner tables are stored permuted
    bool stage_order(int d) const { return col[d] && !dct[d]; }
};

// x and y Periodic.  real_plans = false: the retry after rocFFT's real plans failed their self test.
inline PoissonChoice choose_periodic(const ocn_grid &g, bool real_plans, bool (*col_ok)(int), bool (*row_ok)(int))
{
    PoissonChoice c;
    c.N[0] = g.Nx; c.N[1] = g.Ny; c.N[2] = g.Nz;
    c.topo[0] = g.tx; c.topo[1] = g.ty; c.topo[2] = g.tz;
    c.stretched_z = g.dzc != nullptr;
    c.tri = g.tz == OCN_BOUNDED;  // nonhydrostatic_pressure_solver dispatch (NonhydrostaticModels.jl:25-62)
    c.source_wrap = g.tx == OCN_PERIODIC && g.ty == OCN_PERIODIC && g.tz == OCN_PERIODIC && env_on("OCN_POISSON_SOURCE_WRAP");
    c.c2c = !real_plans || env_set("OCN_POISSON_C2C");
    const bool xy_ok = row_ok(g.Nx) && col_ok(g.Ny) && env_on("OCN_POISSON_CUSTOM_XY");
    c.custom_tri = c.tri && !c.c2c && xy_ok && g.Nz > 1;
    c.dct_z = c.custom_tri && !c.stretched_z && col_ok(g.Nz) && env_on("OCN_POISSON_DCT_Z");
    c.fused_z = !c.tri && g.tz == OCN_PERIODIC && !c.c2c && col_ok(g.Nz) && env_on("OCN_POISSON_FUSED_Z");
    c.custom_xy = c.custom_tri || (c.fused_z && xy_ok);
    c.dims3 = !c.tri && g.tz == OCN_PERIODIC && !c.fused_z;
    c.direct_out = !c.c2c && env_on("OCN_POISSON_DIRECT_OUT");
    return c;
}

// Any (Periodic | Bounded | Flat)^3 topology; tdim 0 / 1: a stretched x / y.  packed_ok = false: the retry after the real x plans
// of the packed pipeline failed their self test.
inline PoissonChoice choose_general(const ocn_grid &g, int tdim, bool packed_ok, bool (*col_ok)(int))
{
    PoissonChoice c;
    c.general = true;
    c.c2c = true;
    c.N[0] = g.Nx; c.N[1] = g.Ny; c.N[2] = g.Nz;
    c.topo[0] = g.tx; c.topo[1] = g.ty; c.topo[2] = g.tz;
    c.stretched_z = g.dzc != nullptr;
    c.tdim = tdim;
    // a stretched direction (or OCN_POISSON_GENERAL_TRI=1 on a regular Bounded z): transforms along the other two, Thomas sweep along it
    c.tri = tdim != 2 || c.stretched_z || (env_set("OCN_POISSON_GENERAL_TRI") && g.tz == OCN_BOUNDED);
    if (c.tri) c.topo[tdim] = OCN_FLAT;
    const int *N = c.N, *topo = c.topo;
    c.fft_dct = !env_set("OCN_POISSON_NAIVE_DCT");
    c.fuse = env_on("OCN_POISSON_FUSE_SHUFFLES");
    c.dct_to_field = env_on("OCN_POISSON_DCT_TO_FIELD");
    if (!c.fft_dct) return c;
    // the packed and all-real variants assume a sweep along z
    const bool real_ok = tdim == 2 && env_on("OCN_POISSON_PACKED");
    c.packed = real_ok && packed_ok && topo[0] == OCN_PERIODIC && N[0] % 2 == 0 && N[0] >= 4 && (topo[1] == OCN_BOUNDED || topo[2] == OCN_BOUNDED);
    c.allreal = real_ok && topo[0] == OCN_BOUNDED && topo[1] == OCN_BOUNDED && (topo[2] == OCN_BOUNDED || topo[2] == OCN_FLAT) && N[0] % 2 == 0 &&
                N[1] % 2 == 0;
    const bool colfft = env_on("OCN_POISSON_GENERAL_COLFFT");
    // the row kernel: Nx = 64 ... 512 and an even Ny; packed: a regular channel without another Periodic direction
    c.rowdct = topo[0] != OCN_FLAT && colfft && col_ok(N[0]) && env_on("OCN_POISSON_ROW_DCT") &&
               (c.allreal || (c.packed && !c.tri && topo[1] != OCN_PERIODIC && topo[2] != OCN_PERIODIC && N[1] % 2 == 0));
    for (int d = 0; d < 3; ++d) {
        if (topo[d] == OCN_FLAT) continue;
        c.col[d] = d > 0 && colfft && col_ok(N[d]);
        c.dct[d] = c.col[d] && topo[d] == OCN_BOUNDED && env_on("OCN_POISSON_FUSED_DCT");
        // rocFFT lines where no kernel of ours runs them: x of the real variants is the row kernel or the real plans
        c.lines[d] = !c.col[d] && !(d == 0 && (c.rowdct || c.packed));
        int *n = c.line_n[d];
        n[0] = N[0]; n[1] = N[1]; n[2] = N[2];
        if (c.allreal) {  // x lines of row pairs (Nx, Ny / 2, Nz); y / z lines of x-adjacent pairs (Nx / 2, Ny, Nz)
            if (d == 0) n[1] = N[1] / 2; else n[0] = N[0] / 2;
        } else if (c.packed) {  // Nx / 2 complex columns under a cosine transform, the half spectrum under an FFT
            n[0] = topo[d] == OCN_BOUNDED ? N[0] / 2 : N[0] / 2 + 1;
        }
    }
    return c;
}

struct PassLists {
    std::vector<PassRec> source, set_source, solve;
};

namespace detail {

inline PassRec rec(Pass p, int d, int mode, const int n[3], double scale = 1.0)
{
    PassRec r;
    r.pass = p; r.d = d; r.mode = mode; r.scale = scale;
    r.n[0] = n[0]; r.n[1] = n[1]; r.n[2] = n[2];
    return r;
}
inline bool is(const PassRec &r, Pass p, int mode) { return r.pass == p && r.mode == mode; }

// FFT lines along d: one launch of the column kernel (forward: natural -> stage order; inverse back, scaled 1 / N) or rocFFT lines
inline PassRec lines(const PoissonChoice &c, int d, bool inverse, const int n[3])
{
    if (c.col[d]) return rec(Pass::ColumnFFT, d, (int)(inverse ? ColFFT::Inverse : ColFFT::Forward), n, inverse ? 1.0 / c.N[d] : 1.0);
    return rec(Pass::LineFFT, d, inverse, n);
}
// REDFT10 along d (Makhoul 1980): gather, FFT, twiddle -- or the one pass of the column kernel
inline void push_dct(const PoissonChoice &c, std::vector<PassRec> &l, int d, const int n[3])
{
    if (c.dct[d]) { l.push_back(rec(Pass::ColumnDCT, d, (int)ColFFT::DctForward, n)); return; }
    l.push_back(rec(Pass::Shuffle, d, (int)DctShuffle::Gather, n));
    l.push_back(lines(c, d, false, n));
    l.push_back(rec(Pass::Shuffle, d, (int)DctShuffle::PostTwiddle, n));
}
// REDFT01 / 2N along d: twiddle, inverse FFT (scaled 1 / N), scatter -- or the one pass
inline void push_idct(const PoissonChoice &c, std::vector<PassRec> &l, int d, const int n[3])
{
    if (c.dct[d]) { l.push_back(rec(Pass::ColumnDCT, d, (int)ColFFT::DctInverse, n, 1.0 / c.N[d])); return; }
    l.push_back(rec(Pass::Shuffle, d, (int)DctShuffle::PreTwiddle, n));
    l.push_back(lines(c, d, true, n));
    l.push_back(rec(Pass::Shuffle, d, (int)DctShuffle::Scatter, n));
}
// A twiddle followed by a pure permutation along ANOTHER direction (forward: post-twiddle then gather; inverse: scatter then pre-twiddle)
// runs as one pass: the permutation only relabels whole lines of the twiddle direction.
inline void append_fused(const PoissonChoice &c, std::vector<PassRec> &out, const std::vector<PassRec> &l)
{
    for (size_t q = 0; q < l.size(); ++q) {
        const PassRec &o = l[q];
        if (c.fuse && q + 1 < l.size() && o.pass == Pass::Shuffle && l[q + 1].pass == Pass::Shuffle && o.d != l[q + 1].d) {
            const PassRec &o2 = l[q + 1];
            const bool fwd = o.mode == (int)DctShuffle::PostTwiddle && o2.mode == (int)DctShuffle::Gather;
            const bool bwd = o.mode == (int)DctShuffle::Scatter && o2.mode == (int)DctShuffle::PreTwiddle;
            if (fwd || bwd) {
                const PassRec &tw = fwd ? o : o2, &pm = fwd ? o2 : o;
                PassRec r = rec(Pass::TwiddlePermute, tw.d, tw.mode, o.n);
                r.d2 = pm.d; r.mode2 = pm.mode;
                out.push_back(r);
                ++q;
                continue;
            }
        }
        out.push_back(o);
    }
}
// The forward cosine transforms open a solve: their first gather is skipped when the source pass stored its output gathered.
inline void append_forward(const PoissonChoice &c, std::vector<PassRec> &out, std::vector<PassRec> l, int gathered_dim)
{
    if (!l.empty() && is(l[0], Pass::Shuffle, (int)DctShuffle::Gather) && l[0].d == gathered_dim) l[0].skip_if_gathered = true;
    append_fused(c, out, l);
}
// The way back into the pressure field.  real: the inverse cosine transforms ran on x-adjacent pairs of reals -- when the last of them
// is a one-pass column transform it stores straight into p (no copy_real_component! pass).  Otherwise the last scatter is folded
// into the read of the copy.
inline void append_backward(const PoissonChoice &c, std::vector<PassRec> &out, std::vector<PassRec> l, bool real)
{
    if (real && c.dct_to_field && !l.empty() && is(l.back(), Pass::ColumnDCT, (int)ColFFT::DctInverse)) {
        l.back().pass = Pass::ColumnDCTToField;
        append_fused(c, out, l);
        return;
    }
    int last_scatter = -1;
    if (c.fuse && !l.empty() && is(l.back(), Pass::Shuffle, (int)DctShuffle::Scatter)) {
        last_scatter = l.back().d;
        l.pop_back();
    }
    append_fused(c, out, l);
    PassRec r = rec(Pass::CopyReal, 0, (int)(real ? CopySource::Real : CopySource::Complex), c.N);
    r.d2 = last_scatter;
    out.push_back(r);
}

inline void build_periodic(const PoissonChoice &c, PassLists &L)
{
    const int kind1 = c.tri;
    const int H[3] = {c.c2c ? c.N[0] : c.N[0] / 2 + 1, c.N[1], c.N[2]};  // the stored spectrum: all of x, or the Hermitian half
    const double count = (double)c.N[0] * c.N[1] * c.N[2];
    // ---- source: K8 / K9, straight into the half spectrum where the row kernel runs x (Δzᶜ rides on the tridiagonal system only)
    PassRec src = c.custom_xy ? rec(Pass::SourceRowFFT, 0, c.custom_tri && !c.dct_z, c.N)
                              : rec(Pass::SourceTerm, 0, (int)(c.c2c ? (kind1 ? SourceOut::ComplexDz : SourceOut::Complex) : (kind1 ? SourceOut::RealDz : SourceOut::Real)), c.N);
    src.to_rhs = !c.custom_xy && !c.c2c;
    src.wrap = c.source_wrap;
    L.source.push_back(src);
    // ---- solve
    std::vector<PassRec> &S = L.solve;
    const PassRec sweep = rec(Pass::SweepZ, 2, 0, H);  // (diagonal built with the eigenvalues in the order y is stored in)
    if (c.custom_xy) {
        // FFT_y (stage order out) -> the z part -> IFFT_y -> inverse x transform into the rows of p.  The packed real inverse of the row
        // kernel returns (Nx / 2) x, y contributes Ny; the fused z pass carries the whole 1 / (Nx Ny Nz) (assuming Nx x: hence the 2)
        S.push_back(rec(Pass::RowFFTOfRealSource, 0, 0, H));
        S.push_back(rec(Pass::ColumnFFT, 1, (int)ColFFT::Forward, H));
        if (c.dct_z) S.push_back(rec(Pass::ColumnDCTSolve, 2, 0, H, 1.0 / c.N[2]));
        else if (c.custom_tri) S.push_back(sweep);
        else S.push_back(rec(Pass::ColumnFFTSolve, 2, 0, H, 1.0 / count));
        S.push_back(rec(Pass::ColumnFFT, 1, (int)ColFFT::Inverse, H));
        S.push_back(rec(Pass::RowFFTToField, 0, 0, H, c.custom_tri ? 2.0 / ((double)c.N[0] * c.N[1]) : 2.0));
    } else {
        // forward transforms (solve! :104-107), the z part, backward transforms (:118-121) and the real part into the pressure interior (:123)
        S.push_back(rec(c.c2c ? Pass::FFTForward : Pass::FFTRealForward, 0, 0, H));
        if (c.fused_z) S.push_back(rec(Pass::ColumnFFTSolve, 2, 0, H, 1.0 / count));
        else if (kind1) S.push_back(sweep);
        else S.push_back(rec(Pass::SpectralSolve, 0, 0, H));
        if (c.c2c) {
            S.push_back(rec(Pass::FFTInverse, 0, 0, H));
            S.push_back(rec(Pass::CopyReal, 0, (int)CopySource::Complex, c.N));
        } else {
            S.push_back(rec(c.direct_out ? Pass::FFTRealInverseToField : Pass::FFTRealInverseAndCopy, 0, 0, H));
        }
    }
}

inline void build_general(const PoissonChoice &c, PassLists &L)
{
    const int *N = c.N, *topo = c.topo;
    const int Pair[3] = {N[0] / 2, N[1], N[2]}, Half[3] = {N[0] / 2 + 1, N[1], N[2]}, Row[3] = {N[0], N[1] / 2, N[2]};
    const bool real = c.packed || c.allreal;
    // forward transforms Bounded first, then Periodic (plan_transforms.jl:53-57, 129-140); backward in the opposite order
    int order[3], no = 0;
    for (int d = 0; d < 3; ++d) if (topo[d] == OCN_BOUNDED) order[no++] = d;
    for (int d = 0; d < 3; ++d) if (topo[d] == OCN_PERIODIC) order[no++] = d;
    // ---- source (divᶜᶜᶜ reads u, v, w through their own layouts and treats Flat directions: any topology).  The gather of the first
    // cosine transform is folded into its store (all-real boxes transform y first: their x lines pair rows; the one-pass column
    // transform gathers on its own load).  The tridiagonal flavour's right-hand side carries Δᶜ of the sweep direction; the real
    // variants keep a REAL array whose x-adjacent pairs the cosine transforms read as complex numbers.
    int first = -1;
    if (c.fft_dct && c.fuse)
        for (int d = 2; d >= (c.allreal ? 1 : 0); --d)
            if (topo[d] == OCN_BOUNDED) first = d;
    if (first >= 0 && c.dct[first]) first = -1;
    PassRec src = c.tri && c.tdim != 2 ? rec(Pass::SourceTermStretched, c.tdim, 0, N)
                                       : rec(Pass::SourceTerm, 0, (int)(real ? (c.tri ? SourceOut::RealDz : SourceOut::Real) : (c.tri ? SourceOut::ComplexDz : SourceOut::Complex)), N);
    src.d2 = first;
    L.source.push_back(src);
    // ---- solve
    std::vector<PassRec> &S = L.solve;
    std::vector<PassRec> F, B;
    // the division by the eigenvalues, or the Thomas sweep, on a complex spectrum of extents n
    auto solve = [&](const int n[3]) { return rec(!c.tri ? Pass::SpectralSolve : c.tdim == 0 ? Pass::SweepX : c.tdim == 1 ? Pass::SweepY : Pass::SweepZ, c.tdim, 0, n); };
    if (c.allreal) {
        // y, z on the pair view; x on pairs of rows (one pass of the row kernel, two around the sweep of a stretched z, or gather,
        // rocFFT lines and twiddle back to the real array each way); a real division or sweep; and back
        for (int d = 1; d < 3; ++d) if (topo[d] == OCN_BOUNDED) push_dct(c, F, d, Pair);
        for (int d = 2; d >= 1; --d) if (topo[d] == OCN_BOUNDED) push_idct(c, B, d, Pair);
        append_forward(c, S, F, first);
        if (c.rowdct && !c.tri) {
            S.push_back(rec(Pass::RowDCT, 0, (int)RowDCT::Solve, N));
        } else {
            if (c.rowdct) {
                S.push_back(rec(Pass::RowDCT, 0, (int)RowDCT::Forward, N));
            } else {
                S.push_back(rec(Pass::RowPair, 0, (int)DctShuffle::Gather, Row));
                S.push_back(rec(Pass::LineFFT, 0, 0, Row));
                S.push_back(rec(Pass::RowPair, 0, (int)DctShuffle::PostTwiddle, Row));
            }
            S.push_back(rec(c.tri ? Pass::SweepZReal : Pass::SpectralSolveReal, 2, 0, N));
            if (c.rowdct) {
                S.push_back(rec(Pass::RowDCT, 0, (int)RowDCT::Inverse, N));
            } else {
                S.push_back(rec(Pass::RowPair, 0, (int)DctShuffle::PreTwiddle, Row));
                S.push_back(rec(Pass::LineFFT, 0, 1, Row));
                S.push_back(rec(Pass::RowPair, 0, (int)DctShuffle::Scatter, Row));
            }
        }
        append_backward(c, S, B, true);
    } else if (c.packed) {
        // cosine transforms along the Bounded y / z on the real array viewed as Nx / 2 complex columns; x in the row kernel (transform,
        // division and inverse of row pairs in place), or real rows -> half spectrum, the other Periodic direction and the solve on
        // the half spectrum, and back
        for (int q = 0; q < no; ++q) if (topo[order[q]] == OCN_BOUNDED) push_dct(c, F, order[q], Pair);
        for (int q = no - 1; q >= 0; --q) if (topo[order[q]] == OCN_BOUNDED) push_idct(c, B, order[q], Pair);
        append_forward(c, S, F, first);
        if (c.rowdct) {
            S.push_back(rec(Pass::RowDCT, 0, (int)RowDCT::PeriodicSolve, N));
        } else {
            S.push_back(rec(Pass::RealToHalf, 0, 0, N));
            for (int d = 1; d < 3; ++d) if (topo[d] == OCN_PERIODIC) S.push_back(lines(c, d, false, Half));
            S.push_back(solve(Half));
            for (int d = 2; d >= 1; --d) if (topo[d] == OCN_PERIODIC) S.push_back(lines(c, d, true, Half));
            S.push_back(rec(Pass::HalfToReal, 0, 0, N));
        }
        append_backward(c, S, B, true);
    } else {
        for (int q = 0; q < no; ++q) {
            const int d = order[q];
            if (!c.fft_dct) { F.push_back(rec(Pass::NaiveTransform, d, 0, N)); F.back().mode2 = topo[d]; }
            else if (topo[d] == OCN_PERIODIC) F.push_back(lines(c, d, false, N));
            else push_dct(c, F, d, N);
        }
        for (int q = no - 1; q >= 0; --q) {
            const int d = order[q];
            if (!c.fft_dct) { B.push_back(rec(Pass::NaiveTransform, d, 1, N)); B.back().mode2 = topo[d]; }
            else if (topo[d] == OCN_PERIODIC) B.push_back(lines(c, d, true, N));
            else push_idct(c, B, d, N);
        }
        append_forward(c, S, F, first);
        S.push_back(solve(N));
        append_backward(c, S, B, false);
    }
}

}  // namespace detail

inline PassLists build_passes(const PoissonChoice &c)
{
    PassLists L;
    if (c.general) detail::build_general(c, L);
    else detail::build_periodic(c, L);
    // ---- set_source_term!: multiplies by Δᶜ of the sweep direction for the Fourier-tridiagonal solvers
    // (fourier_tridiagonal_poisson_solver.jl:155-177); a regular z has one Δz
    const bool scaled = c.general ? c.tri : (c.tri && !c.dct_z);
    PassRec r = c.general && c.tri && c.tdim != 2 ? detail::rec(Pass::SetSourceStretched, c.tdim, 0, c.N)
                                                  : detail::rec(scaled && !c.stretched_z ? Pass::SetSourceUniformDz : Pass::SetSource, 2, scaled, c.N);
    r.to_rhs = !c.c2c;
    r.mode2 = c.c2c && !c.packed && !c.allreal;  // widened to complex
    L.set_source.push_back(r);
    return L;
}

}  // namespace poisson
}  // namespace ocn
