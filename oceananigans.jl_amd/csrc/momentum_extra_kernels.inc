// momentum_extra_kernels.inc -- the momentum finishing pass of physics.hip (direct and LDS-tiled kernels), included THREE times: as
// momentum_extra_kernel / momentum_extra_tiled (no Stokes drift: the kernels and their arguments as they always were), as
// momentum_extra_kernel_stokes / momentum_extra_tiled_stokes, which take one more argument (ocn::StokesDev) and compile the Stokes-drift
// terms of momentum_extra_cell in, and as momentum_extra_kernel_forced / momentum_extra_tiled_forced, which take ocn::StokesDev and
// ocn::MomentumForcingDev and compile both in (either may be empty at run time).  The includer defines
//   OCN_EXTRA_KERNEL, OCN_EXTRA_TILED   the kernel names
//   OCN_EXTRA_STK, OCN_EXTRA_FRC        true / false: momentum_extra_cell's STK and FRC
//   OCN_EXTRA_SD_PARAM                  empty, `, ocn::StokesDev sd` or `, ocn::StokesDev sd, ocn::MomentumForcingDev fd` (additional parameters)
//   OCN_EXTRA_SD, OCN_EXTRA_FD          nullptr, or &sd / &fd
// One text for all keeps the families identical except for the terms themselves.

// `mf`: the flux boundary contributions of u, v (apply_flux_bcs.jl:107-160) and the NEXT stage's rk3 substep of u, v, w into a
// second storage, folded into this last pass over G (same operations as apply_flux_bcs_kernel / stepper_kernel).
template <int TZ>
__global__ __launch_bounds__(256) void OCN_EXTRA_KERNEL(GridDev g, TermsDev t, const double *__restrict__ u,
                                                             const double *__restrict__ v, const double *__restrict__ w,
                                                             double *__restrict__ Gu, double *__restrict__ Gv,
                                                             double *__restrict__ Gw, PRange r, ocn::MomentumFinal mf OCN_EXTRA_SD_PARAM)
{
    const int i = r.i0 + blockIdx.x * blockDim.x + threadIdx.x;
    const int j = r.j0 + blockIdx.y * blockDim.y + threadIdx.y;
    const int k = r.k0 + blockIdx.z;
    if (i > r.i1 || j > r.j1) return;
    constexpr bool ZF = (TZ == OCN_FLAT);
    const Metrics M = make_metrics(g);
    const Lay L = ocn::make_lay(g, OCN_LOC_CCC);
    const long long s2 = L.s2, s3 = ZF ? 0 : L.s3, o = ocn::at(L, i, j, k);
    const double *pu = u + o, *pv = v + o, *pw = w + o, *pn = t.nu_e ? t.nu_e + o : nullptr;
    const ExtraLoads ld = momentum_extra_loads<TZ>(t, mf, r, k, o, s2, s3, Gu, Gv, Gw);
    momentum_extra_cell<TZ, false, OCN_EXTRA_STK, OCN_EXTRA_FRC>(
        g, t, M, i, j, k, o, s2, s3, pn != nullptr, [&](int a, int b, int c) { return pu[a + b * s2 + c * s3]; },
        [&](int a, int b, int c) { return pv[a + b * s2 + c * s3]; }, [&](int a, int b, int c) { return pw[a + b * s2 + c * s3]; },
        [&](int a, int b, int c) { return pn[a + b * s2 + c * s3]; }, Gu, Gv, Gw, r, mf, ld, 0.0, 0.0, nullptr, nullptr, nullptr, OCN_EXTRA_SD, OCN_EXTRA_FD);
}

// Tiled variant of the finishing pass: a workgroup owns a 32 x 8 patch of columns and marches KZ planes upward; planes
// k-1, k, k+1 of u, v, w (and νₑ) live in a 3-slot LDS ring with a one-cell rim, so every value enters the workgroup once per
// plane (1.33x with the rim) instead of once per stencil tap (~60 taps per cell hit L2 in the direct kernel: the 3 planes x
// 4 fields of a workgroup do not fit the 32 KB L1).  pHY′, G, G⁻ are touched once per cell and stay in global memory.
// GL ("general layouts"): the interior box of a grid with a Bounded x / y (general.hip) -- u, v, w (and their G, G⁻, stepped copies) have
// their own parent layouts; every cell of the box is a full stencil away from the walls, where the expressions are the Periodic ones.
// With the Stokes-drift terms of momentum_extra_cell: w at k, k + 1 and u, v at k - 1, k are in the LDS ring already.
template <int TZ, bool SH, bool GL = false>
__global__ __launch_bounds__(256, SH ? 3 : 4) void OCN_EXTRA_TILED(GridDev g, TermsDev t, const double *__restrict__ u,
                                                            const double *__restrict__ v, const double *__restrict__ w,
                                                            double *__restrict__ Gu, double *__restrict__ Gv,
                                                            double *__restrict__ Gw, PRange r, ocn::MomentumFinal mf, int KZ OCN_EXTRA_SD_PARAM)
{
    constexpr int TX = 32, TY = 8, SX = TX + 2, SY = TY + 2, PL = SX * SY;
    __shared__ double Lu[3][PL], Lv[3][PL], Lw[3][PL], Ln[3][PL];
    // Stresses shared between the cells that read them (closure != 0): every cell evaluates the six stresses it OWNS -- T11, T22, T33 at
    // its centre, T12 at its south-west edge, T13, T23 at its lower west / south edges -- once per plane instead of the 18 values its three
    // components read (each stress is read by 2 to 4 cells); T33 stays in registers (same column), T13 / T23 of plane k + 1 become plane k
    // of the next iteration.  Same expressions, same operands: bit-identical to the unshared evaluation.
    constexpr int SPL = SH ? PL : 1;
    __shared__ double S11[SPL], S22[SPL], S12[SPL], S13[2][SPL], S23[2][SPL];
    const int tid = threadIdx.x, tx = tid % TX, ty = tid / TX;
    int bx, by, bz;
    xcd_block_coords(mf.xcd, bx, by, bz);
    const int i0 = r.i0 + bx * TX, j0 = r.j0 + by * TY;
    const int kb = r.k0 + bz * KZ, ke = min(kb + KZ - 1, r.k1);
    const int i = i0 + tx, j = j0 + ty;
    const bool active = (i <= r.i1) && (j <= r.j1);
    const Metrics M = make_metrics(g);
    const Lay L = ocn::make_lay(g, OCN_LOC_CCC);
    const long long s2 = L.s2, s3 = L.s3;
    const Lay LFu = GL ? ocn::make_lay(g, OCN_LOC_FCC) : L, LFv = GL ? ocn::make_lay(g, OCN_LOC_CFC) : L, LFw = GL ? ocn::make_lay(g, OCN_LOC_CCF) : L;
    const bool has_nu = t.nu_e != nullptr;
    // Staging of plane kk (tile + rim, indices clamped to the first halo cell) into ring slot kk % 3 is split in two so that the
    // global loads of plane k+2 are in flight while plane k is being computed: fetch() -> registers, commit() -> LDS.
    constexpr int NS = (PL + TX * TY - 1) / (TX * TY);  // cells staged per thread (2)
    long long soff[NS], soffu[GL ? NS : 1], soffv[GL ? NS : 1], soffw[GL ? NS : 1];
    bool son[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) {
        const int idx = tid + q * TX * TY;
        son[q] = idx < PL;
        const int li = son[q] ? idx % SX : 0, lj = son[q] ? idx / SX : 0;
        const int si = min(i0 - 1 + li, g.Nx + 1), sj = min(j0 - 1 + lj, g.Ny + 1);
        soff[q] = ocn::at(L, si, sj, 0);  // plane 0: add kk * s3
        if (GL) {
            soffu[q] = ocn::at(LFu, si, sj, 0);
            soffv[q] = ocn::at(LFv, si, sj, 0);
            soffw[q] = ocn::at(LFw, si, sj, 0);
        }
    }
    double fu[NS], fv[NS], fw[NS], fn[NS];
    auto fetch = [&](int kk) {
#pragma unroll
        for (int q = 0; q < NS; ++q) {
            const long long oo = soff[q] + (long long)kk * s3;
            fu[q] = son[q] ? u[GL ? soffu[q] + (long long)kk * LFu.s3 : oo] : 0.0;
            fv[q] = son[q] ? v[GL ? soffv[q] + (long long)kk * LFv.s3 : oo] : 0.0;
            fw[q] = son[q] ? w[GL ? soffw[q] + (long long)kk * LFw.s3 : oo] : 0.0;
            fn[q] = (son[q] && has_nu) ? t.nu_e[oo] : 0.0;
        }
    };
    auto commit = [&](int kk) {
        const int slot = kk % 3;
#pragma unroll
        for (int q = 0; q < NS; ++q) {
            if (!son[q]) continue;
            const int idx = tid + q * TX * TY;
            Lu[slot][idx] = fu[q];
            Lv[slot][idx] = fv[q];
            Lw[slot][idx] = fw[q];
            if (has_nu) Ln[slot][idx] = fn[q];
        }
    };
    fetch(kb - 1);
    commit(kb - 1);
    fetch(kb);
    commit(kb);
    fetch(kb + 1);
    const int c0 = (ty + 1) * SX + (tx + 1);
    // rim positions whose stresses the tile's cells read: one per lane of the first 32 / 32 / 8 / 8 lanes of waves 0 .. 3
    //   wave 0: south row (T22 of row j0 - 1), wave 1: north row (T12, T23 of row j0 + TY), wave 2: west column (T11 of column i0 - 1),
    //   wave 3: east column (T12, T13 of column i0 + TX)
    const int wv = tid >> 6, ln = tid & 63;
    const int rim = (wv == 0 && ln < TX) ? 1 : (wv == 1 && ln < TX) ? 2 : (wv == 2 && ln < TY) ? 3 : (wv == 3 && ln < TY) ? 4 : 0;
    const int cr = rim == 1 ? (ln + 1) : rim == 2 ? (TY + 1) * SX + (ln + 1) : rim == 3 ? (ln + 1) * SX : rim == 4 ? (ln + 1) * SX + (TX + 1) : c0;
    constexpr bool shared = SH;
    const double dx = M.dx, dy = M.dy, nu = t.nu;
#if !OCN_STRICT
    const double rdx = fast_rcp(dx), rdy = fast_rcp(dy);
#endif
    double t33_prev = 0.0;
    for (int k = kb; k <= ke; ++k) {
        commit(k + 1);
        __syncthreads();
        const int ia = active ? i : r.i1, ja = active ? j : r.j1;
        const long long o = ocn::at(L, ia, ja, k);
        const FieldOffs fov{GL ? ocn::at(LFu, ia, ja, k) : o, GL ? ocn::at(LFv, ia, ja, k) : o, GL ? ocn::at(LFw, ia, ja, k) : o, GL ? LFw.s3 : s3};
        const FieldOffs *fo = GL ? &fov : nullptr;
        ExtraLoads ld{};
        if (active) ld = momentum_extra_loads<TZ>(t, mf, r, k, o, s2, s3, Gu, Gv, Gw, fo);  // this plane's own values first ...
        OCN_ISSUE_LOADS_HERE();
        if (k < ke) fetch(k + 2);  // ... then the staging values of plane k + 2, consumed by the next iteration's commit
        OCN_ISSUE_LOADS_HERE();
        const int base = k + 3;  // (k + c) % 3 for c in {-1, 0, 1} without negative operands
        Stresses sh{};
        if (shared) {
            const double dzc = M.dzC(k), dzf = M.dzF(k), dzf1 = M.dzF(k + 1), dzcm = M.dzC(k - 1);
#if !OCN_STRICT
            const double rdzc = fast_rcp(dzc), rdzf = fast_rcp(dzf), rdzf1 = fast_rcp(dzf1), rdzcm = fast_rcp(dzcm);
#endif
            auto sU = [&](int c, int a, int b, int d) { return Lu[(base + d) % 3][c + a + b * SX]; };
            auto sV = [&](int c, int a, int b, int d) { return Lv[(base + d) % 3][c + a + b * SX]; };
            auto sW = [&](int c, int a, int b, int d) { return Lw[(base + d) % 3][c + a + b * SX]; };
            auto sN = [&](int c, int a, int b, int d) { return Ln[(base + d) % 3][c + a + b * SX]; };
            auto nuC = [&](int c, int d) { return has_nu ? sN(c, 0, 0, d) : nu; };
            auto nuFFC = [&](int c) {
                return has_nu ? 0.5 * (0.5 * (sN(c, -1, -1, 0) + sN(c, 0, -1, 0)) + 0.5 * (sN(c, -1, 0, 0) + sN(c, 0, 0, 0))) : nu;
            };
            auto nuFCF = [&](int c, int d) {
                return has_nu ? 0.5 * (0.5 * (sN(c, -1, 0, d - 1) + sN(c, 0, 0, d - 1)) + 0.5 * (sN(c, -1, 0, d) + sN(c, 0, 0, d))) : nu;
            };
            auto nuCFF = [&](int c, int d) {
                return has_nu ? 0.5 * (0.5 * (sN(c, 0, -1, d - 1) + sN(c, 0, 0, d - 1)) + 0.5 * (sN(c, 0, -1, d) + sN(c, 0, 0, d))) : nu;
            };
            // the expressions of momentum_extra_cell, with the centre of evaluation as an argument (d: z-face k + d)
            auto T11 = [&](int c) { return TAU(nuC(c, 0), DX(sU(c, 1, 0, 0), sU(c, 0, 0, 0))); };
            auto T22 = [&](int c) { return TAU(nuC(c, 0), DY(sV(c, 0, 1, 0), sV(c, 0, 0, 0))); };
            auto T12 = [&](int c) { return TAU(nuFFC(c), 0.5 * (DY(sU(c, 0, 0, 0), sU(c, 0, -1, 0)) + DX(sV(c, 0, 0, 0), sV(c, -1, 0, 0)))); };
            auto T13 = [&](int c, int d) {
                const double dzu = d ? OCN_DIV(sU(c, 0, 0, 1) - sU(c, 0, 0, 0), dzf1, rdzf1) : OCN_DIV(sU(c, 0, 0, 0) - sU(c, 0, 0, -1), dzf, rdzf);
                return TAU(nuFCF(c, d), 0.5 * (dzu + DX(sW(c, 0, 0, d), sW(c, -1, 0, d))));
            };
            auto T23 = [&](int c, int d) {
                const double dzv = d ? OCN_DIV(sV(c, 0, 0, 1) - sV(c, 0, 0, 0), dzf1, rdzf1) : OCN_DIV(sV(c, 0, 0, 0) - sV(c, 0, 0, -1), dzf, rdzf);
                return TAU(nuCFF(c, d), 0.5 * (dzv + DY(sW(c, 0, 0, d), sW(c, 0, -1, d))));
            };
            const int cur = k & 1, nxt = cur ^ 1;
            const bool first = (k == kb);
            // own position (every thread, active or not: the neighbours of the last active column / row read these)
            const double o11 = T11(c0), o22 = T22(c0), o12 = T12(c0), o13n = T13(c0, 1), o23n = T23(c0, 1);
            double o13c, o23c;
            if (first) {
                o13c = T13(c0, 0);
                o23c = T23(c0, 0);
                S13[cur][c0] = o13c;
                S23[cur][c0] = o23c;
                t33_prev = TAU(nuC(c0, -1), OCN_DIV(sW(c0, 0, 0, 0) - sW(c0, 0, 0, -1), dzcm, rdzcm));
            } else {
                o13c = S13[cur][c0];  // (written by this thread in the previous iteration)
                o23c = S23[cur][c0];
            }
            S11[c0] = o11; S22[c0] = o22; S12[c0] = o12; S13[nxt][c0] = o13n; S23[nxt][c0] = o23n;
            const double o33 = TAU(nuC(c0, 0), OCN_DIV(sW(c0, 0, 0, 1) - sW(c0, 0, 0, 0), dzc, rdzc));
            // rim positions
            if (rim == 1) {
                S22[cr] = T22(cr);
            } else if (rim == 2) {
                S12[cr] = T12(cr);
                S23[nxt][cr] = T23(cr, 1);
                if (first) S23[cur][cr] = T23(cr, 0);
            } else if (rim == 3) {
                S11[cr] = T11(cr);
            } else if (rim == 4) {
                S12[cr] = T12(cr);
                S13[nxt][cr] = T13(cr, 1);
                if (first) S13[cur][cr] = T13(cr, 0);
            }
            __syncthreads();
            sh.t11e = o11; sh.t11w = S11[c0 - 1];
            sh.t12c = o12; sh.t12n = S12[c0 + SX]; sh.t12e = S12[c0 + 1];
            sh.t13t = o13n; sh.t13c = o13c; sh.t13e = S13[cur][c0 + 1];
            sh.t22n = o22; sh.t22s = S22[c0 - SX];
            sh.t23t = o23n; sh.t23c = o23c; sh.t23n = S23[cur][c0 + SX];
            sh.t33t = o33; sh.t33b = t33_prev;
            t33_prev = o33;
        }
        if (active) {
            momentum_extra_cell<TZ, false, OCN_EXTRA_STK, OCN_EXTRA_FRC>(
                g, t, M, i, j, k, o, s2, s3, has_nu, [&](int a, int b, int c) { return Lu[(base + c) % 3][c0 + a + b * SX]; },
                [&](int a, int b, int c) { return Lv[(base + c) % 3][c0 + a + b * SX]; },
                [&](int a, int b, int c) { return Lw[(base + c) % 3][c0 + a + b * SX]; },
                [&](int a, int b, int c) { return Ln[(base + c) % 3][c0 + a + b * SX]; }, Gu, Gv, Gw, r, mf, ld, 0.0, 0.0, nullptr,
                SH ? &sh : nullptr, fo, OCN_EXTRA_SD, OCN_EXTRA_FD);
        }
        // Unshared: everyone must be done with slot (k - 1) % 3 before the next iteration's commit overwrites it.  Shared: nothing reads plane
        // k - 1 after the first iteration's stress phase (T13, T23 of plane k and T33 of k - 1 are carried), which the barrier above already
        // closed; the plane-k stress arrays are next written after the NEXT iteration's first barrier, which every wave reaches only after its
        // cell phase -- so two barriers per plane suffice.
        // With the Stokes-drift terms the cell phase reads u, v of plane k - 1 again (Gw), so the shared variant keeps this barrier too.
        if (!SH || OCN_EXTRA_STK) __syncthreads();
    }
}
