// diagnostics.hip -- on-device diagnostics: compute!(Field(operation)) and the Average / Integral reductions of an AbstractOperation tree.
//   BinaryOperation, UnaryOperation, Derivative        src/AbstractOperations/binary_operations.jl, unary_operations.jl, derivatives.jl
//   ℑx, ℑy, ℑz and their compositions                  src/Operators/interpolation_operators.jl:8-71
//   ∂x, ∂y, ∂z = δ / Δ                                 src/Operators/derivative_operators.jl
//   Average, Integral, reduction_grid_metric           src/AbstractOperations/metric_field_reductions.jl:11-113
//
// The reference compiles one fused kernel per tree.  Here the host lowers the tree to a straight-line program (include/ocn_hip.h:
// ocn_op_program) and the kernels below interpret it, two cells per lane at a time.  The program travels by value in the kernel arguments: it is the
// same for every lane, so fetching and decoding an instruction is scalar work, and every lane of a block executes the same instruction on
// its own cells.  The values of a cell live in LDS, laid out [register][cell][lane]: a lane only ever touches its own column, so there are no bank
// conflicts (consecutive lanes, consecutive doubles) and no barriers, and nothing is indexed at run time in private memory (which would
// be scratch).  A lane evaluates two cells per decoded instruction, and the LDS of a launch is sized by the registers its program uses:
// n_registers x 2 cells x 256 lanes x 8 bytes = 4 KiB per register, 64 KiB at the limit of 16 (two blocks in the 160 KiB of a CU).
//
// One build, without FMA contraction: diagnostics are bandwidth-bound, and one arithmetic variant keeps them bit-identical to the
// restatement (tests/operations_numpy.py) whatever math mode the grid carries.
//
// Reductions: a wave owns a task = (output element or 64 of them, a contiguous chunk of the reduced rows); a lane adds its cells in index
// order; where x is reduced the 64 lane sums are folded by shuffles.  The partial sums go to a workspace and a second small launch adds
// them in a fixed order (across waves through LDS where an element has many partials) and divides: no atomics anywhere.
//
// Boundary functions (ContinuousBoundaryFunction with field_dependencies, src/BoundaryConditions/continuous_boundary_function.jl:124-157):
// the same interpreter on one boundary plane of the grid, the boundary-normal index fixed at domain_boundary_indices' I; the result goes
// to the array a flux condition's ocn_bc.values points to, which the apply_flux_bcs* kernels read as they read any array-valued condition.
//
// Forcing functions of the model's fields (ContinuousForcing with field_dependencies, src/Forcings/continuous_forcing.jl:109-142): the same
// interpreter over the cells a tendency is computed at (the interior without the faces on a wall), its value ADDED to the tendency array,
// which is read once and written once per cell.  MIN / MAX carry Julia's NaN and signed-zero rules; the instruction set stays IEEE-only
// (what is transcendental is folded by the host into constants and vectors: forcing_programs.py).
#include <algorithm>
#include <cmath>

#include "ocn_internal.h"

namespace ocn {

constexpr int OP_BLOCK = 256;           // 64 lanes along x times 4 waves
constexpr int OP_CELLS = 2;             // cells a lane evaluates per decoded instruction
constexpr long long OP_TARGET_WAVES = 8192;  // wave-tasks a reduction is cut into (256 CUs x 4 SIMDs x 8)

struct OpInsDev {
    unsigned char op, dst, a, b;  // a, b: REGISTERS of the operands (LOAD: a = field, SPACING: a = kind)
    int imm;                      // LOAD: element offset of (di, dj, dk) in the field's parent; SPACING of Δz: Hz + dk
    double value;
};
struct OpFieldDev {
    const double *p;
    long long o;           // offset of the first interior element
    long long s1, s2, s3;  // strides of i, j, k; 0 along a direction the field was reduced in
};
struct OpProgramDev {
    int n;
    OpFieldDev f[OCN_OP_MAX_FIELDS];
    OpInsDev ins[OCN_OP_MAX_INSTRUCTIONS];
};
// parent layout of a result: offset of the first interior element, strides (0 along reduced directions are never used: extent 1)
struct OpOut {
    long long o, s1, s2, s3;
    int n1, n2;  // kept extents along x and y of a reduced result (1 where reduced): element e = i + n1 * (j + n2 * k)
};
struct OpReduceGeom {
    int nx;
    int njk, nkk;      // kept extents along y, z (1 where reduced)
    int njr;           // reduced extent along y (1 where kept)
    long long rows;    // reduced rows: (y extent if reduced) * (z extent if reduced)
    long long rb;      // rows per task
    long long ntasks;  // P * Ek
    long long Ek;      // njk * nkk
    long long E;       // output elements: Ek, times nx where x is kept
};

// Julia's min / max (Base.min, Base.max of two Float64), as comparisons and selects: a NaN in either operand propagates (NaN compares
// false, so the first select yields b, and a NaN in a is put back by the last one) and of the two zeros, which compare equal, max takes
// +0.0 and min -0.0 in either operand order.  Not fmin / fmax: they drop a NaN.
__device__ __forceinline__ double julia_max(double a, double b)
{
    double r = a > b ? a : b;
    r = a == b ? (__builtin_signbit(a) ? b : a) : r;
    return a != a ? a : r;
}
__device__ __forceinline__ double julia_min(double a, double b)
{
    double r = a < b ? a : b;
    r = a == b ? (__builtin_signbit(a) ? a : b) : r;
    return a != a ? a : r;
}

// The program at OP_CELLS 0-based interior cells (i[c], j[c], k[c]) of the tree's location at once: one fetch and decode per instruction
// serves both cells, and their two dependency chains (load or LDS read -> operation -> LDS write) overlap.  R = this lane's column of the
// register file, laid out [register][cell][lane].  The next instruction is fetched while the current one executes.
__device__ __forceinline__ void op_eval(const OpProgramDev &P, const GridDev &g, double *R, const int (&i)[OP_CELLS], const int (&j)[OP_CELLS],
                                        const int (&k)[OP_CELLS], double (&v)[OP_CELLS])
{
    OpInsDev next = P.ins[0];
    for (int pc = 0; pc < P.n; ++pc) {
        const OpInsDev I = next;
        if (pc + 1 < P.n) next = P.ins[pc + 1];
        const double *A = R + I.a * (OP_CELLS * OP_BLOCK), *B = R + I.b * (OP_CELLS * OP_BLOCK);
        switch (I.op) {
        case OCN_OP_LOAD: {
            const OpFieldDev &F = P.f[I.a];
            const double *base = F.p + (F.o + I.imm);
#pragma unroll
            for (int c = 0; c < OP_CELLS; ++c) v[c] = base[F.s1 * i[c] + F.s2 * j[c] + F.s3 * k[c]];
            break;
        }
        case OCN_OP_CONST:
#pragma unroll
            for (int c = 0; c < OP_CELLS; ++c) v[c] = I.value;
            break;
        case OCN_OP_SPACING:
#pragma unroll
            for (int c = 0; c < OP_CELLS; ++c) {
                if (I.a == 0) v[c] = g.dx;
                else if (I.a == 1) v[c] = g.dy;
                else if (!g.dzc) v[c] = g.dz;
                else v[c] = uniform_load(I.a == 2 ? g.dzc : g.dzf, k[c] + I.imm);
            }
            break;
        case OCN_OP_NEG:
#pragma unroll
            for (int c = 0; c < OP_CELLS; ++c) v[c] = -A[c * OP_BLOCK];
            break;
        case OCN_OP_ABS:
#pragma unroll
            for (int c = 0; c < OP_CELLS; ++c) v[c] = fabs(A[c * OP_BLOCK]);
            break;
        case OCN_OP_SQRT:
#pragma unroll
            for (int c = 0; c < OP_CELLS; ++c) v[c] = sqrt(A[c * OP_BLOCK]);
            break;
        case OCN_OP_ADD:
#pragma unroll
            for (int c = 0; c < OP_CELLS; ++c) v[c] = A[c * OP_BLOCK] + B[c * OP_BLOCK];
            break;
        case OCN_OP_SUB:
#pragma unroll
            for (int c = 0; c < OP_CELLS; ++c) v[c] = A[c * OP_BLOCK] - B[c * OP_BLOCK];
            break;
        case OCN_OP_MUL:
#pragma unroll
            for (int c = 0; c < OP_CELLS; ++c) v[c] = A[c * OP_BLOCK] * B[c * OP_BLOCK];
            break;
        case OCN_OP_DIV:
#pragma unroll
            for (int c = 0; c < OP_CELLS; ++c) v[c] = A[c * OP_BLOCK] / B[c * OP_BLOCK];
            break;
        case OCN_OP_MIN:
#pragma unroll
            for (int c = 0; c < OP_CELLS; ++c) v[c] = julia_min(A[c * OP_BLOCK], B[c * OP_BLOCK]);
            break;
        case OCN_OP_MAX:
#pragma unroll
            for (int c = 0; c < OP_CELLS; ++c) v[c] = julia_max(A[c * OP_BLOCK], B[c * OP_BLOCK]);
            break;
        default:  // (the host admits no other opcode)
            break;
        }
        double *D = R + I.dst * (OP_CELLS * OP_BLOCK);
#pragma unroll
        for (int c = 0; c < OP_CELLS; ++c) D[c * OP_BLOCK] = v[c];
    }
}

// a block covers 64 x 8 cells of one plane: a lane takes rows j and j + 4
__global__ __launch_bounds__(OP_BLOCK) void op_compute_kernel(GridDev g, OpProgramDev P, int nx, int ny, double *__restrict__ out, OpOut O)
{
    extern __shared__ double regs[];  // n_registers x OP_CELLS x OP_BLOCK
    const int i = blockIdx.x * 64 + threadIdx.x, j0 = blockIdx.y * 8 + threadIdx.y, k = blockIdx.z;
    if (i >= nx || j0 >= ny) return;
    const bool two = j0 + 4 < ny;  // (a missing second cell repeats the first: always in bounds, never stored)
    const int ii[OP_CELLS] = {i, i}, jj[OP_CELLS] = {j0, two ? j0 + 4 : j0}, kk[OP_CELLS] = {k, k};
    double v[OP_CELLS];
    op_eval(P, g, regs + threadIdx.y * 64 + threadIdx.x, ii, jj, kk, v);
    out[O.o + i + O.s2 * jj[0] + O.s3 * k] = v[0];
    if (two) out[O.o + i + O.s2 * jj[1] + O.s3 * k] = v[1];
}

// G += the program, over the cells a tendency is computed at: the box of 0-based indices (i0.., j0.., k0..) of extents nx, ny and the
// launch's z blocks.  The same tile as op_compute_kernel; a cell's G is read once, before the evaluation (the load is in flight under it),
// and written once.  G is none of the program's fields (the host checks), so no cell reads what another one writes.
__global__ __launch_bounds__(OP_BLOCK) void op_accumulate_kernel(GridDev g, OpProgramDev P, int i0, int j0, int k0, int nx, int ny,
                                                                 double *__restrict__ G, OpOut O)
{
    extern __shared__ double regs[];  // n_registers x OP_CELLS x OP_BLOCK
    const int a = blockIdx.x * 64 + threadIdx.x, b = blockIdx.y * 8 + threadIdx.y, k = k0 + blockIdx.z;
    if (a >= nx || b >= ny) return;
    const bool two = b + 4 < ny;  // (a missing second cell repeats the first: always in bounds, never stored)
    const int i = i0 + a;
    const int ii[OP_CELLS] = {i, i}, jj[OP_CELLS] = {j0 + b, two ? j0 + b + 4 : j0 + b}, kk[OP_CELLS] = {k, k};
    const long long o0 = O.o + i + O.s2 * jj[0] + O.s3 * k, o1 = O.o + i + O.s2 * jj[1] + O.s3 * k;
    const double G0 = G[o0], G1 = G[o1];
    double v[OP_CELLS];
    op_eval(P, g, regs + threadIdx.y * 64 + threadIdx.x, ii, jj, kk, v);
    G[o0] = G0 + v[0];
    if (two) G[o1] = G1 + v[1];
}

// One boundary plane: the point (a1, a2) of the two tangential directions (first one fastest, as ocn_bc.values is indexed), the normal index
// fixed at I0.  A block covers 64 x 8 points; a lane takes the points a2 and a2 + 4, as op_compute_kernel does with its rows.
// axis 2 (bottom / top) and axis 1 (south / north) have x as a1, so consecutive lanes load consecutive doubles; on axis 0 (west / east)
// a1 is y and the loads are a row apart.  Those planes are Ny x Nz points of a run whose cost is Nx x Ny x Nz per launch: not tuned.
struct OpPlane {
    int axis, I0, n1, n2;
};
__global__ __launch_bounds__(OP_BLOCK) void op_boundary_kernel(GridDev g, OpProgramDev P, OpPlane B, double *__restrict__ values)
{
    extern __shared__ double regs[];  // n_registers x OP_CELLS x OP_BLOCK
    const int a1 = blockIdx.x * 64 + threadIdx.x, b0 = blockIdx.y * 8 + threadIdx.y;
    if (a1 >= B.n1 || b0 >= B.n2) return;
    const bool two = b0 + 4 < B.n2;  // (a missing second point repeats the first: always in bounds, never stored)
    const int b1 = two ? b0 + 4 : b0;
    // (i, j, k) = (I0, a1, a2) on west / east, (a1, I0, a2) on south / north, (a1, a2, I0) on bottom / top
    const int ii[OP_CELLS] = {B.axis == 0 ? B.I0 : a1, B.axis == 0 ? B.I0 : a1};
    const int jj[OP_CELLS] = {B.axis == 0 ? a1 : (B.axis == 1 ? B.I0 : b0), B.axis == 0 ? a1 : (B.axis == 1 ? B.I0 : b1)};
    const int kk[OP_CELLS] = {B.axis == 2 ? B.I0 : b0, B.axis == 2 ? B.I0 : b1};
    double v[OP_CELLS];
    op_eval(P, g, regs + threadIdx.y * 64 + threadIdx.x, ii, jj, kk, v);
    values[a1 + (long long)B.n1 * b0] = v[0];
    if (two) values[a1 + (long long)B.n1 * b1] = v[1];
}

template <bool XRED>
__global__ __launch_bounds__(OP_BLOCK) void op_reduce_kernel(GridDev g, OpProgramDev P, OpReduceGeom G, double *__restrict__ ws)
{
    extern __shared__ double regs[];
    double *R = regs + threadIdx.y * 64 + threadIdx.x;
    const long long task = (long long)blockIdx.x * 4 + threadIdx.y;  // one wave, one task
    if (task >= G.ntasks) return;
    const long long p = task / G.Ek;
    const int e = (int)(task % G.Ek);
    const int jk = e % G.njk, kk = e / G.njk;
    const long long q0 = p * G.rb, q1 = q0 + G.rb < G.rows ? q0 + G.rb : G.rows;
    const int i0 = XRED ? (int)threadIdx.x : (int)(blockIdx.y * 64 + threadIdx.x);
    double acc = 0.0, v[OP_CELLS];
    if (XRED) {  // cells i and i + 64 of a row at once; a lane adds its cells in index order
        for (long long q = q0; q < q1; ++q) {
            const int j = jk + (int)(q % G.njr), k = kk + (int)(q / G.njr);  // (one of each pair is 0)
            for (int i = i0; i < G.nx; i += 2 * 64) {
                const bool two = i + 64 < G.nx;
                const int ii[OP_CELLS] = {i, two ? i + 64 : i}, jj[OP_CELLS] = {j, j}, kc[OP_CELLS] = {k, k};
                op_eval(P, g, R, ii, jj, kc, v);
                acc = acc + v[0];
                if (two) acc = acc + v[1];
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) acc = acc + __shfl_down(acc, off, 64);
        if (threadIdx.x == 0) ws[p * G.E + e] = acc;
    } else if (i0 < G.nx) {  // rows q and q + 1 at once
        for (long long q = q0; q < q1; q += 2) {
            const bool two = q + 1 < q1;
            const long long qb = two ? q + 1 : q;
            const int ii[OP_CELLS] = {i0, i0}, jj[OP_CELLS] = {jk + (int)(q % G.njr), jk + (int)(qb % G.njr)},
                      kc[OP_CELLS] = {kk + (int)(q / G.njr), kk + (int)(qb / G.njr)};
            op_eval(P, g, R, ii, jj, kc, v);
            acc = acc + v[0];
            if (two) acc = acc + v[1];
        }
        ws[p * G.E + (long long)e * G.nx + i0] = acc;
    }
}

__device__ __forceinline__ long long op_out_offset(const OpOut &O, long long e)
{
    const long long i = e % O.n1, r = e / O.n1;
    return O.o + O.s1 * i + O.s2 * (r % O.n2) + O.s3 * (r / O.n2);
}
// BLOCK: one block per output element (few elements, many partials); otherwise one thread per element
template <bool BLOCK>
__global__ __launch_bounds__(OP_BLOCK) void op_finish_kernel(const double *__restrict__ ws, long long P, long long E, double divisor,
                                                             double *__restrict__ out, OpOut O)
{
    if (BLOCK) {
        __shared__ double part[OP_BLOCK / 64];
        const long long e = blockIdx.x;
        double s = 0.0;
        for (long long p = threadIdx.x; p < P; p += OP_BLOCK) s = s + ws[p * E + e];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s = s + __shfl_down(s, off, 64);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
        __syncthreads();
        if (threadIdx.x == 0) out[op_out_offset(O, e)] = (((part[0] + part[1]) + part[2]) + part[3]) / divisor;
    } else {
        const long long e = (long long)blockIdx.x * OP_BLOCK + threadIdx.x;
        if (e >= E) return;
        double s = 0.0;
        for (long long p = 0; p < P; ++p) s = s + ws[p * E + e];
        out[op_out_offset(O, e)] = s / divisor;
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
struct OpSpace {
    int N[3], H[3], topo[3], n[3];  // n: interior extents of the tree's location
    int lo[3], hi[3];               // the 0-based indices the program runs over: 0 .. n - 1, or one index along the normal of a boundary plane
};
static int op_space(const ocn_grid *grid, int loc, const char *who, OpSpace &S)
{
    OCN_TRY(validate_grid_any(grid));
    OCN_REQUIRE(grid->tx <= OCN_FLAT, "%s: a slab of a partitioned grid (diagnostics on a Distributed architecture are not implemented)", who);
    OCN_REQUIRE(loc >= 0 && loc <= 7, "%s: location mask %d outside 0..7", who, loc);
    const int N[3] = {grid->Nx, grid->Ny, grid->Nz}, H[3] = {grid->Hx, grid->Hy, grid->Hz}, T[3] = {grid->tx, grid->ty, grid->tz};
    for (int d = 0; d < 3; ++d) {
        S.N[d] = N[d]; S.H[d] = H[d]; S.topo[d] = T[d];
        S.n[d] = T[d] == OCN_FLAT ? 1 : N[d] + ((((loc >> d) & 1) && T[d] == OCN_BOUNDED) ? 1 : 0);
        S.lo[d] = 0; S.hi[d] = S.n[d] - 1;
    }
    return OCN_SUCCESS;
}
// The index space of a boundary plane (side 0..5 = west, east, south, north, bottom, top): N points along the two tangential directions
// -- the extents of ocn_bc.values, whatever the location -- and the one index I - 1 of domain_boundary_indices along the normal
static int op_plane(OpSpace &S, int side, const char *who)
{
    OCN_REQUIRE(side >= 0 && side <= 5, "%s: side %d outside 0..5 (west, east, south, north, bottom, top)", who, side);
    const int dn = side >> 1;
    OCN_REQUIRE(S.topo[dn] == OCN_BOUNDED, "%s: side %d lies on direction %d, which is not Bounded", who, side, dn);
    for (int d = 0; d < 3; ++d) {
        S.n[d] = d == dn ? 1 : S.N[d];
        S.lo[d] = 0; S.hi[d] = S.n[d] - 1;
    }
    S.lo[dn] = S.hi[dn] = (side & 1) ? S.N[dn] - 1 : 0;
    return OCN_SUCCESS;
}
// The index space of a tendency: the interior without the faces on a wall -- along a Face & Bounded direction the faces 2 .. N of the
// N + 1 (periphery_offset, kernel_launching.jl:113-114; the one face of N = 1 stays), as the tendency entry points run (r.ou, r.ov, r.ow)
static void op_tendency_cells(OpSpace &S, int loc)
{
    for (int d = 0; d < 3; ++d) {
        if (!(((loc >> d) & 1) && S.topo[d] == OCN_BOUNDED)) continue;
        S.lo[d] = S.N[d] > 1 ? 1 : 0;
        S.hi[d] = S.N[d] - 1;
        S.n[d] = S.hi[d] - S.lo[d] + 1;
    }
}
// parent layout of a field at `loc` reduced along the directions of `reduced`
static void op_layout(const OpSpace &S, int loc, int reduced, long long ext[3], long long stride[3], long long &o)
{
    for (int d = 0; d < 3; ++d) ext[d] = ((reduced >> d) & 1) ? 1 : ocn_ext(S.N[d], S.H[d], S.topo[d], (loc >> d) & 1);
    stride[0] = 1; stride[1] = ext[0]; stride[2] = ext[0] * ext[1];
    o = 0;
    for (int d = 0; d < 3; ++d) o += ((reduced >> d) & 1) ? 0 : S.H[d] * stride[d];
}

// side == nullptr: the program runs over the interior of its location (tendency_cells: without the faces on a wall); otherwise over the
// boundary plane *side
static int op_validate(const ocn_grid *grid, const ocn_op_program *p, const char *who, OpSpace &S, OpProgramDev &D, const int *side = nullptr,
                       bool tendency_cells = false)
{
    OCN_REQUIRE(grid && p, "%s: null grid or program", who);
    OCN_TRY(op_space(grid, p->loc, who, S));
    if (side) {
        OCN_TRY(op_plane(S, *side, who));
    }
    if (tendency_cells) op_tendency_cells(S, p->loc);
    OCN_REQUIRE(p->n_instructions >= 1 && p->n_instructions <= OCN_OP_MAX_INSTRUCTIONS, "%s: %d instructions outside 1..%d", who,
                p->n_instructions, OCN_OP_MAX_INSTRUCTIONS);
    OCN_REQUIRE(p->n_registers >= 1 && p->n_registers <= OCN_OP_MAX_REGISTERS, "%s: %d registers outside 1..%d", who, p->n_registers,
                OCN_OP_MAX_REGISTERS);
    OCN_REQUIRE(p->n_fields >= 0 && p->n_fields <= OCN_OP_MAX_FIELDS, "%s: %d fields outside 0..%d", who, p->n_fields, OCN_OP_MAX_FIELDS);
    D = OpProgramDev{};
    D.n = p->n_instructions;
    long long ext[OCN_OP_MAX_FIELDS][3], stride[OCN_OP_MAX_FIELDS][3];
    for (int f = 0; f < p->n_fields; ++f) {
        OCN_REQUIRE(p->fields[f], "%s: field %d is a null pointer", who, f);
        OCN_REQUIRE(p->field_loc[f] >= 0 && p->field_loc[f] <= 7 && p->field_reduced[f] >= 0 && p->field_reduced[f] <= 7,
                    "%s: field %d: location mask %d / reduced mask %d outside 0..7", who, f, p->field_loc[f], p->field_reduced[f]);
        long long o;
        op_layout(S, p->field_loc[f], p->field_reduced[f], ext[f], stride[f], o);
        OpFieldDev &F = D.f[f];
        F.p = p->fields[f];
        F.o = o;
        F.s1 = (p->field_reduced[f] & 1) ? 0 : stride[f][0];
        F.s2 = (p->field_reduced[f] & 2) ? 0 : stride[f][1];
        F.s3 = (p->field_reduced[f] & 4) ? 0 : stride[f][2];
    }
    int holder[OCN_OP_MAX_REGISTERS];
    for (int r = 0; r < OCN_OP_MAX_REGISTERS; ++r) holder[r] = -1;
    for (int q = 0; q < p->n_instructions; ++q) {
        const ocn_op_instruction &I = p->ins[q];
        OpInsDev &J = D.ins[q];
        OCN_REQUIRE(I.opcode >= OCN_OP_LOAD && I.opcode <= OCN_OP_MAX, "%s: instruction %d: unknown opcode %d", who, q, I.opcode);
        OCN_REQUIRE(I.reg >= 0 && I.reg < p->n_registers, "%s: instruction %d: register %d outside 0..%d", who, q, I.reg, p->n_registers - 1);
        J.op = (unsigned char)I.opcode;
        J.dst = (unsigned char)I.reg;
        if (I.opcode == OCN_OP_LOAD) {
            OCN_REQUIRE(I.field >= 0 && I.field < p->n_fields, "%s: instruction %d: field %d outside 0..%d", who, q, I.field, p->n_fields - 1);
            const int f = I.field, off[3] = {I.di, I.dj, I.dk};
            long long imm = 0;
            for (int d = 0; d < 3; ++d) {
                if ((p->field_reduced[f] >> d) & 1) {
                    OCN_REQUIRE(off[d] == 0, "%s: instruction %d: offset %d along direction %d, in which field %d is reduced", who, q, off[d], d, f);
                    continue;
                }
                // the cells lo .. hi of the index space, shifted, must lie in the field's parent array along d
                const long long lo = (long long)S.H[d] + S.lo[d] + off[d], hi = (long long)S.H[d] + S.hi[d] + off[d];
                OCN_REQUIRE(lo >= 0 && hi <= ext[f][d] - 1, "%s: instruction %d: offset %d along direction %d reaches beyond the halo (%d) of field %d",
                            who, q, off[d], d, S.H[d], f);
                imm += off[d] * stride[f][d];
            }
            OCN_REQUIRE(imm > -(1LL << 31) && imm < (1LL << 31), "%s: instruction %d: offset does not fit 32 bits", who, q);
            J.a = (unsigned char)f;
            J.imm = (int)imm;
        } else if (I.opcode == OCN_OP_CONST) {
            J.value = I.value;
        } else if (I.opcode == OCN_OP_SPACING) {
            OCN_REQUIRE(I.field >= 0 && I.field <= 3, "%s: instruction %d: spacing kind %d outside 0..3", who, q, I.field);
            J.a = (unsigned char)I.field;
            if (I.field >= 2 && grid->dzc) {
                OCN_REQUIRE(grid->dzf, "%s: dzc without dzf", who);
                const long long lo = (long long)S.H[2] + S.lo[2] + I.dk, hi = (long long)S.H[2] + S.hi[2] + I.dk;
                OCN_REQUIRE(lo >= 0 && hi <= S.N[2] + 2LL * S.H[2] - 1, "%s: instruction %d: z spacing offset %d reaches beyond the halo (%d)", who, q,
                            I.dk, S.H[2]);
                J.imm = S.H[2] + I.dk;
            }
        } else {
            const int nop = I.opcode >= OCN_OP_ADD ? 2 : 1;
            const int ops[2] = {I.a, I.b};
            for (int t = 0; t < nop; ++t) {
                OCN_REQUIRE(ops[t] >= 0 && ops[t] < q, "%s: instruction %d: operand %d is not an earlier instruction", who, q, ops[t]);
                const int r = p->ins[ops[t]].reg;
                OCN_REQUIRE(holder[r] == ops[t], "%s: instruction %d: register %d of operand %d was overwritten by instruction %d", who, q, r, ops[t],
                            holder[r]);
                (t == 0 ? J.a : J.b) = (unsigned char)r;
            }
        }
        holder[I.reg] = q;
    }
    return OCN_SUCCESS;
}

// the register file of a block: [register][cell][lane]
static size_t op_lds_bytes(const ocn_op_program *p) { return (size_t)p->n_registers * OP_CELLS * OP_BLOCK * sizeof(double); }

static OpOut op_out(const OpSpace &S, int loc, int dims)
{
    long long ext[3], stride[3], o;
    op_layout(S, loc, dims, ext, stride, o);
    OpOut O;
    O.o = o; O.s1 = stride[0]; O.s2 = stride[1]; O.s3 = stride[2];
    O.n1 = (dims & 1) ? 1 : S.n[0];
    O.n2 = (dims & 2) ? 1 : S.n[1];
    return O;
}

static OpReduceGeom op_reduce_geometry(const OpSpace &S, int dims, long long &P)
{
    OpReduceGeom G;
    G.nx = S.n[0];
    G.njk = (dims & 2) ? 1 : S.n[1];
    G.nkk = (dims & 4) ? 1 : S.n[2];
    G.njr = (dims & 2) ? S.n[1] : 1;
    G.rows = (long long)G.njr * ((dims & 4) ? S.n[2] : 1);
    G.Ek = (long long)G.njk * G.nkk;
    const long long waves_per_task = (dims & 1) ? 1 : (S.n[0] + 63) / 64;
    const long long want = (OP_TARGET_WAVES + G.Ek * waves_per_task - 1) / (G.Ek * waves_per_task);
    P = std::max(1LL, std::min(G.rows, want));
    G.rb = (G.rows + P - 1) / P;
    P = (G.rows + G.rb - 1) / G.rb;
    G.ntasks = P * G.Ek;
    G.E = G.Ek * ((dims & 1) ? 1 : S.n[0]);
    return G;
}

int op_compute(const ocn_grid *grid, const ocn_op_program *p, double *out, hipStream_t stream)
{
    OpSpace S;
    OpProgramDev D;
    OCN_TRY(op_validate(grid, p, "ocn_op_compute", S, D));
    OCN_REQUIRE(out, "ocn_op_compute: null output pointer");
    const OpOut O = op_out(S, p->loc, 0);
    const dim3 block(64, 4, 1), nb((S.n[0] + 63) / 64, (S.n[1] + 7) / 8, S.n[2]);
    OCN_REQUIRE(nb.y <= 65535u && nb.z <= 65535u, "ocn_op_compute: grid too large for one launch");
    hipLaunchKernelGGL(op_compute_kernel, nb, block, op_lds_bytes(p), stream, to_dev(*grid), D, S.n[0], S.n[1], out, O);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

int op_accumulate(const ocn_grid *grid, const ocn_op_program *p, double *G, hipStream_t stream)
{
    OpSpace S;
    OpProgramDev D;
    OCN_TRY(op_validate(grid, p, "ocn_op_accumulate", S, D, nullptr, true));
    OCN_REQUIRE(G, "ocn_op_accumulate: null tendency pointer");
    for (int f = 0; f < p->n_fields; ++f)
        OCN_REQUIRE(G != p->fields[f], "ocn_op_accumulate: the tendency array is field %d of the program (cells would read what others write)", f);
    const OpOut O = op_out(S, p->loc, 0);
    const dim3 block(64, 4, 1), nb((S.n[0] + 63) / 64, (S.n[1] + 7) / 8, S.n[2]);
    OCN_REQUIRE(nb.y <= 65535u && nb.z <= 65535u, "ocn_op_accumulate: grid too large for one launch");
    hipLaunchKernelGGL(op_accumulate_kernel, nb, block, op_lds_bytes(p), stream, to_dev(*grid), D, S.lo[0], S.lo[1], S.lo[2], S.n[0], S.n[1], G, O);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

int op_compute_boundary(const ocn_grid *grid, const ocn_op_program *p, int side, double *values, hipStream_t stream)
{
    OpSpace S;
    OpProgramDev D;
    OCN_TRY(op_validate(grid, p, "ocn_op_compute_boundary", S, D, &side));
    OCN_REQUIRE(values, "ocn_op_compute_boundary: null values pointer");
    OpPlane B;
    B.axis = side >> 1;
    B.I0 = S.lo[B.axis];
    B.n1 = S.n[B.axis == 0 ? 1 : 0];
    B.n2 = S.n[B.axis == 2 ? 1 : 2];
    const dim3 block(64, 4, 1), nb((B.n1 + 63) / 64, (B.n2 + 7) / 8, 1);
    OCN_REQUIRE(nb.y <= 65535u, "ocn_op_compute_boundary: plane too large for one launch");
    hipLaunchKernelGGL(op_boundary_kernel, nb, block, op_lds_bytes(p), stream, to_dev(*grid), D, B, values);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

int op_reduce_workspace(const ocn_grid *grid, int loc, int dims, long long *n_doubles)
{
    OCN_REQUIRE(grid && n_doubles, "ocn_op_reduce_workspace: null pointer");
    OCN_REQUIRE(dims >= 1 && dims <= 7, "ocn_op_reduce_workspace: dims mask %d outside 1..7", dims);
    OpSpace S;
    OCN_TRY(op_space(grid, loc, "ocn_op_reduce_workspace", S));
    long long P;
    const OpReduceGeom G = op_reduce_geometry(S, dims, P);
    *n_doubles = P * G.E;
    return OCN_SUCCESS;
}

int op_reduce(const ocn_grid *grid, const ocn_op_program *p, int dims, double divisor, double *workspace, long long workspace_doubles,
              double *out, hipStream_t stream)
{
    OpSpace S;
    OpProgramDev D;
    OCN_TRY(op_validate(grid, p, "ocn_op_reduce", S, D));
    OCN_REQUIRE(dims >= 1 && dims <= 7, "ocn_op_reduce: dims mask %d outside 1..7", dims);
    OCN_REQUIRE(workspace && out, "ocn_op_reduce: null workspace or output pointer");
    OCN_REQUIRE(divisor == divisor && divisor != 0.0, "ocn_op_reduce: divisor %g", divisor);
    long long P;
    const OpReduceGeom G = op_reduce_geometry(S, dims, P);
    OCN_REQUIRE(workspace_doubles >= P * G.E, "ocn_op_reduce: workspace of %lld doubles, %lld needed (ocn_op_reduce_workspace)",
                (long long)workspace_doubles, P * G.E);
    const OpOut O = op_out(S, p->loc, dims);
    const long long nblocks = (G.ntasks + 3) / 4;
    OCN_REQUIRE(nblocks < (1LL << 31), "ocn_op_reduce: grid too large for one launch");
    const dim3 block(64, 4, 1);
    const GridDev g = to_dev(*grid);
    if (dims & 1)
        hipLaunchKernelGGL(op_reduce_kernel<true>, dim3((unsigned)nblocks, 1, 1), block, op_lds_bytes(p), stream, g, D, G, workspace);
    else
        hipLaunchKernelGGL(op_reduce_kernel<false>, dim3((unsigned)nblocks, (S.n[0] + 63) / 64, 1), block, op_lds_bytes(p), stream, g, D, G,
                           workspace);
    OCN_CHECK_HIP(hipGetLastError());
    if (G.E < 64)
        hipLaunchKernelGGL(op_finish_kernel<true>, dim3((unsigned)G.E, 1, 1), dim3(OP_BLOCK, 1, 1), 0, stream, workspace, P, G.E, divisor, out, O);
    else
        hipLaunchKernelGGL(op_finish_kernel<false>, dim3((unsigned)((G.E + OP_BLOCK - 1) / OP_BLOCK), 1, 1), dim3(OP_BLOCK, 1, 1), 0, stream,
                           workspace, P, G.E, divisor, out, O);
    OCN_CHECK_HIP(hipGetLastError());
    return OCN_SUCCESS;
}

}  // namespace ocn
