// momentum_extra_general.inc -- the per-cell kernel of the non-advective momentum terms (general.hip), included TWICE: as
// momentum_extra_general (the kernel and its arguments as they always were) and as momentum_extra_general_stokes, which takes one more
// argument (ocn::StokesDev sd) and adds (∇ × uˢ) × u + ∂t uˢ last (StokesDrifts.jl:165-180), with the plain nested two-point averages of
// interpolation_operators.jl:50-56 (the value itself along a Flat x / y).  The includer defines OCN_EXTRA_GENERAL (the kernel's name),
// OCN_EXTRA_STK (1 / 0) and OCN_EXTRA_SD_PARAM (empty, or `ocn::StokesDev sd,`).  A THIRD inclusion, momentum_extra_general_forced
// (OCN_EXTRA_FRC = 1, `ocn::StokesDev sd, ocn::MomentumForcingDev fd,`), adds the sampled forcing of each component after the Stokes terms
// (which then run only when fd.stokes says the drift is in use).
__global__ __launch_bounds__(256) void OCN_EXTRA_GENERAL(gen::Fields F, ocn::TermsDev t, double *__restrict__ Gu, double *__restrict__ Gv,
                                                              double *__restrict__ Gw, OCN_EXTRA_SD_PARAM gen::GFrames fr)
{
    using namespace gen;
    gen::GRange r;
    int i, j, k;
    if (!gen::frame_cell(fr, r, i, j, k)) return;
    const GridDev &g = F.g;
    const Metrics M = make_metrics(g);
    const Lay &Lu = F.Lu, &Lv = F.Lv, &Lw = F.Lw, &Lc = F.Lc;
    const double *u = F.u, *v = F.v, *w = F.w, *nu_e = t.nu_e;
    const bool fx = g.tx == OCN_FLAT, fy = g.ty == OCN_FLAT, fz = g.tz == OCN_FLAT;
    const double dx = M.dx, dy = M.dy, nu = t.nu;
#define U_(a, b, c) u[ocn::at(Lu, a, b, c)]
#define V_(a, b, c) v[ocn::at(Lv, a, b, c)]
#define W_(a, b, c) w[ocn::at(Lw, a, b, c)]
#define NE(a, b, c) nu_e[ocn::at(Lc, a, b, c)]
    // derivative operators (derivative_operators.jl:20-30); a difference along a Flat direction is 0
    auto DXU_C = [&](int a, int b, int c) { return fx ? 0.0 : (U_(a + 1, b, c) - U_(a, b, c)) / dx; };
    auto DYV_C = [&](int a, int b, int c) { return fy ? 0.0 : (V_(a, b + 1, c) - V_(a, b, c)) / dy; };
    auto DZW_C = [&](int a, int b, int c) { return fz ? 0.0 : (W_(a, b, c + 1) - W_(a, b, c)) / M.dzC(c); };
    auto DYU_FF = [&](int a, int b, int c) { return fy ? 0.0 : (U_(a, b, c) - U_(a, b - 1, c)) / dy; };
    auto DXV_FF = [&](int a, int b, int c) { return fx ? 0.0 : (V_(a, b, c) - V_(a - 1, b, c)) / dx; };
    auto DZU_FF = [&](int a, int b, int c) { return fz ? 0.0 : (U_(a, b, c) - U_(a, b, c - 1)) / M.dzF(c); };
    auto DXW_FF = [&](int a, int b, int c) { return fx ? 0.0 : (W_(a, b, c) - W_(a - 1, b, c)) / dx; };
    auto DZV_FF = [&](int a, int b, int c) { return fz ? 0.0 : (V_(a, b, c) - V_(a, b, c - 1)) / M.dzF(c); };
    auto DYW_FF = [&](int a, int b, int c) { return fy ? 0.0 : (W_(a, b, c) - W_(a, b - 1, c)) / dy; };
    // viscosity at the stress locations (abstract_scalar_diffusivity_closure.jl:291-296)
    auto NU_C = [&](int a, int b, int c) { return nu_e ? NE(a, b, c) : nu; };
    auto NU_FFC = [&](int a, int b, int c) { return nu_e ? 0.5 * (0.5 * (NE(a - 1, b - 1, c) + NE(a, b - 1, c)) + 0.5 * (NE(a - 1, b, c) + NE(a, b, c))) : nu; };
    auto NU_FCF = [&](int a, int b, int c) { return nu_e ? 0.5 * (0.5 * (NE(a - 1, b, c - 1) + NE(a, b, c - 1)) + 0.5 * (NE(a - 1, b, c) + NE(a, b, c))) : nu; };
    auto NU_CFF = [&](int a, int b, int c) { return nu_e ? 0.5 * (0.5 * (NE(a, b - 1, c - 1) + NE(a, b, c - 1)) + 0.5 * (NE(a, b - 1, c) + NE(a, b, c))) : nu; };
    auto T11 = [&](int a, int b, int c) { return -2 * (NU_C(a, b, c) * DXU_C(a, b, c)); };
    auto T22 = [&](int a, int b, int c) { return -2 * (NU_C(a, b, c) * DYV_C(a, b, c)); };
    auto T33 = [&](int a, int b, int c) { return -2 * (NU_C(a, b, c) * DZW_C(a, b, c)); };
    auto T12 = [&](int a, int b, int c) { return -2 * (NU_FFC(a, b, c) * (0.5 * (DYU_FF(a, b, c) + DXV_FF(a, b, c)))); };
    auto T13 = [&](int a, int b, int c) { return -2 * (NU_FCF(a, b, c) * (0.5 * (DZU_FF(a, b, c) + DXW_FF(a, b, c)))); };
    auto T23 = [&](int a, int b, int c) { return -2 * (NU_CFF(a, b, c) * (0.5 * (DZV_FF(a, b, c) + DYW_FF(a, b, c)))); };
    // inactive_cell (Grids/inactive_node.jl:35-95) and the peripheral-node tests of the Coriolis average
    auto inactive = [&](int a, int b, int c) {
        bool q = false;
        if (g.tx == OCN_BOUNDED) q |= (g.xw && a < 1) | (g.xe && a > g.Nx);  // (inactive_node.jl:5-25: by side on the half-Bounded slabs)
        if (g.ty == OCN_BOUNDED) q |= (b < 1) | (b > g.Ny);
        if (g.tz == OCN_BOUNDED) q |= (c < 1) | (c > g.Nz);
        return q;
    };
    auto act_cfc = [&](int a, int b, int c) { return (inactive(a, b, c) || inactive(a, b - 1, c)) ? 0.0 : 1.0; };
    auto act_fcc = [&](int a, int b, int c) { return (inactive(a, b, c) || inactive(a - 1, b, c)) ? 0.0 : 1.0; };
    const double Axc = M.Ax(k), Ayc = M.Ay(k), Az = M.Az;
    if (i >= r.ou) {
        const long long o = ocn::at(Lu, i, j, k);
        double G = Gu[o];
        if (t.buoyancy) G = G + 0.0;
        if (t.coriolis) {  // x_f_cross_U = -f * active_weighted_ℑxyᶠᶜᶜ(v)
            auto IXF = [&](int jj) { return fx ? V_(i, jj, k) : 0.5 * (V_(i - 1, jj, k) + V_(i, jj, k)); };
            auto IXFa = [&](int jj) { return fx ? act_cfc(i, jj, k) : 0.5 * (act_cfc(i - 1, jj, k) + act_cfc(i, jj, k)); };
            const double an = fy ? IXFa(j) : 0.5 * (IXFa(j) + IXFa(j + 1));
            const double vi = (an == 0) ? 0.0 : (fy ? IXF(j) : 0.5 * (IXF(j) + IXF(j + 1))) / an;
            G = G - (-ocn::coriolis_f_at(t, g.Hy, j, 0) * vi);
        }
        if (t.pHY) G = G - (fx ? 0.0 : (t.pHY[ocn::at(Lc, i, j, k)] - t.pHY[ocn::at(Lc, i - 1, j, k)]) / dx);
        if (t.closure) {
            const double dxF = fx ? 0.0 : Axc * T11(i, j, k) - Axc * T11(i - 1, j, k);
            const double dyF = fy ? 0.0 : Ayc * T12(i, j + 1, k) - Ayc * T12(i, j, k);
            const double dzF = fz ? 0.0 : Az * T13(i, j, k + 1) - Az * T13(i, j, k);
            G = G - 1 / (Az * M.dzC(k)) * ((dxF + dyF) + dzF);
        }
#if OCN_EXTRA_STK
#if OCN_EXTRA_FRC
        if (fd.stokes)
#endif
        {  // ℑxzᶠᵃᶜ(w) ∂z_uˢ(z centre k) + ∂t_uˢ
            auto IX = [&](int c) { return fx ? W_(i, j, c) : 0.5 * (W_(i - 1, j, c) + W_(i, j, c)); };
            G = G + (0.5 * (IX(k) + IX(k + 1))) * ocn::stokes_at(sd.dzu_c, k);
            G = G + ocn::stokes_at(sd.dtu, k);
        }
#endif
#if OCN_EXTRA_FRC
        if (fd.f[0].n) G = G + ocn::forcing_at(fd.f[0], i - 1 + g.Hx, j - 1 + g.Hy, k - 1 + g.Hz, o, u[o]);
#endif
        Gu[o] = G;
    }
    if (j >= r.ov) {
        const long long o = ocn::at(Lv, i, j, k);
        double G = Gv[o];
        if (t.buoyancy) G = G + 0.0;
        if (t.coriolis) {  // y_f_cross_U = f * active_weighted_ℑxyᶜᶠᶜ(u)
            auto IXC = [&](int jj) { return fx ? U_(i, jj, k) : 0.5 * (U_(i, jj, k) + U_(i + 1, jj, k)); };
            auto IXCa = [&](int jj) { return fx ? act_fcc(i, jj, k) : 0.5 * (act_fcc(i, jj, k) + act_fcc(i + 1, jj, k)); };
            const double an = fy ? IXCa(j) : 0.5 * (IXCa(j - 1) + IXCa(j));
            const double ui = (an == 0) ? 0.0 : (fy ? IXC(j) : 0.5 * (IXC(j - 1) + IXC(j))) / an;
            G = G - ocn::coriolis_f_at(t, g.Hy, j, 1) * ui;
        }
        if (t.pHY) G = G - (fy ? 0.0 : (t.pHY[ocn::at(Lc, i, j, k)] - t.pHY[ocn::at(Lc, i, j - 1, k)]) / dy);
        if (t.closure) {
            const double dxF = fx ? 0.0 : Axc * T12(i + 1, j, k) - Axc * T12(i, j, k);
            const double dyF = fy ? 0.0 : Ayc * T22(i, j, k) - Ayc * T22(i, j - 1, k);
            const double dzF = fz ? 0.0 : Az * T23(i, j, k + 1) - Az * T23(i, j, k);
            G = G - 1 / (Az * M.dzC(k)) * ((dxF + dyF) + dzF);
        }
#if OCN_EXTRA_STK
#if OCN_EXTRA_FRC
        if (fd.stokes)
#endif
        {  // ℑyzᵃᶠᶜ(w) ∂z_vˢ(z centre k) + ∂t_vˢ
            auto IY = [&](int c) { return fy ? W_(i, j, c) : 0.5 * (W_(i, j - 1, c) + W_(i, j, c)); };
            G = G + (0.5 * (IY(k) + IY(k + 1))) * ocn::stokes_at(sd.dzv_c, k);
            G = G + ocn::stokes_at(sd.dtv, k);
        }
#endif
#if OCN_EXTRA_FRC
        if (fd.f[1].n) G = G + ocn::forcing_at(fd.f[1], i - 1 + g.Hx, j - 1 + g.Hy, k - 1 + g.Hz, o, v[o]);
#endif
        Gv[o] = G;
    }
    if (k >= r.ow) {
        const long long o = ocn::at(Lw, i, j, k);
        double G = Gw[o];
        if (t.buoyancy) {
            double zb = 0.0;
            if (!t.pHY) zb = fz ? gen_buoyancy(t, ocn::at(Lc, i, j, k))
                                : 1 * (0.5 * (gen_buoyancy(t, ocn::at(Lc, i, j, k - 1)) + gen_buoyancy(t, ocn::at(Lc, i, j, k))));
            G = G + zb;
        }
        if (t.coriolis) G = G - 0.0;
        if (t.closure) {
            const double Axf = dy * M.dzF(k), Ayf = dx * M.dzF(k);
            const double dxF = fx ? 0.0 : Axf * T13(i + 1, j, k) - Axf * T13(i, j, k);
            const double dyF = fy ? 0.0 : Ayf * T23(i, j + 1, k) - Ayf * T23(i, j, k);
            const double dzF = fz ? 0.0 : Az * T33(i, j, k) - Az * T33(i, j, k - 1);
            G = G - 1 / (Az * M.dzF(k)) * ((dxF + dyF) + dzF);
        }
#if OCN_EXTRA_STK
#if OCN_EXTRA_FRC
        if (fd.stokes)
#endif
        {  // -ℑxzᶜᵃᶠ(u) ∂z_uˢ(z face k) - ℑyzᵃᶜᶠ(v) ∂z_vˢ(z face k), ∂t_wˢ = 0
            auto IX = [&](int c) { return fx ? U_(i, j, c) : 0.5 * (U_(i, j, c) + U_(i + 1, j, c)); };
            auto IY = [&](int c) { return fy ? V_(i, j, c) : 0.5 * (V_(i, j, c) + V_(i, j + 1, c)); };
            const double ui = 0.5 * (IX(k - 1) + IX(k)), vi = 0.5 * (IY(k - 1) + IY(k));
            G = G + (-(ui * ocn::stokes_at(sd.dzu_f, k)) - vi * ocn::stokes_at(sd.dzv_f, k));
            G = G + 0.0;
        }
#endif
#if OCN_EXTRA_FRC
        if (fd.f[2].n) G = G + ocn::forcing_at(fd.f[2], i - 1 + g.Hx, j - 1 + g.Hy, k - 1 + g.Hz, o, w[o]);
#endif
        Gw[o] = G;
    }
#undef U_
#undef V_
#undef W_
#undef NE
}
