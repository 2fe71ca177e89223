"""TKEDissipationVerticalDiffusivity (k-ϵ) on the GPU (csrc/tke_dissipation.hip): the entry points against the NumPy restatement of the reference
(tests/tke_dissipation_numpy.py, pinned without a GPU in tests/test_host_tke_dissipation.py) bit for bit on whole parent arrays; the hydrostatic
model's closure state after every step against the restatement's sequence applied to the model's own fields; the top fluxes in the tendencies,
reproducibility, the pair with the biharmonic in either order, a bit-identical checkpoint restart and a forced column that mixes.

Shapes (tke_dissipation_numpy.CASES) are the smallest at which the column kernels can still go wrong: 3 x 3 x 2 has one interior face per
column and both cells next to a boundary; 5 x 6 x 4 is below one workgroup; 67 x 13 x 9 (stretched z) has ragged second blocks in x (64 lanes)
and y (4 rows); 130 x 9 x 7 has unequal wide halos and a third block in x."""
import ctypes as C

import numpy as np
import pytest

import implicit_diffusion_numpy as IDN
import tke_dissipation_numpy as TD
from helpers import from_dev, to_dev

pytestmark = pytest.mark.gpu

P, B = "Periodic", "Bounded"
U, V, CC, CCF = TD.U, TD.V, TD.CC, TD.CCF
SEAWATER = TD.SEAWATER
SENTINEL = -7.0

_cases = {}


def _case(ocn, n):
    if n not in _cases:
        pg = TD.make_grid(ocn, ocn.GPU(), n)
        _cases[n] = (pg, TD.make_inputs(pg, n))
    return _cases[n]


def _terms(ocn, buoyancy, T, S):
    L = ocn._lib
    terms = L.CModelTerms()
    if buoyancy == "SeawaterBuoyancy":
        terms.buoyancy, terms.g, terms.alpha, terms.beta, terms.T, terms.S = L.BUOYANCY_SEAWATER_TS, *SEAWATER[1:], T.ptr, S.ptr
    else:
        terms.buoyancy, terms.T = L.BUOYANCY_TRACER, T.ptr
    return terms


def _plane(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a.T)).to("cuda")


def _from_plane(t):
    return t.cpu().numpy().T


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


def _c_struct(ocn, cl):
    L = ocn._lib
    return L.CTKEDissipation(*[cl[name] for name in L.TKE_DISSIPATION_FIELDS], L.STABILITY_CONSTANT if cl["constant"] else L.STABILITY_VARIABLE, 0)


def _closure_dict(constant, **kw):
    cl = TD.closure_dict(constant=constant, **kw)
    for name in ("Cu1", "Cu2", "Cc1", "Cc2", "Cd0", "Cd1", "Cd2", "Cd3", "Cd4", "Cd5"):  # (what ConstantStabilityFunctions does not have)
        cl.setdefault(name, 0.0)
    return cl


# ---- 1. the entry points bit for bit -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("buoyancy", ["SeawaterBuoyancy", "BuoyancyTracer"])
@pytest.mark.parametrize("n", range(len(TD.CASES)), ids=TD.IDS)
def test_entry_points_equal_the_restatement_bit_for_bit(ocn, n, buoyancy):
    """The two top fluxes, the four diffusivities, then the substep alone (solve = 0) and the fused substep + two solves with M = 1 (χ = 0.1)
    and M = 3 (χ = -1/2, 0.1, 0.1): with VariableStabilityFunctions and ConstantStabilityFunctions, with clipping maxima and with the
    reference's +inf.  Whole parent arrays, prefilled with a sentinel where they are only written, so halos and face Nz + 1 are shown untouched;
    the inputs are NaN beyond the documented reach.  The branch shares of the inputs are asserted first, on the restatement's output."""
    pg, c = _case(ocn, n)
    g, L = c["g"], ocn._lib
    spec, Th, Sh = TD.tracers_of(c, buoyancy)
    T, S = to_dev(ocn, pg, CC, Th), to_dev(ocn, pg, CC, Sh if Sh is not None else c["S"])
    u, v = to_dev(ocn, pg, U, c["u"]), to_dev(ocn, pg, V, c["v"])
    up, vp = to_dev(ocn, pg, U, c["u_prev"]), to_dev(ocn, pg, V, c["v_prev"])
    e0, p0 = to_dev(ocn, pg, CC, c["e"]), to_dev(ocn, pg, CC, c["eps"])
    terms = _terms(ocn, buoyancy, T, S)
    zc = _plane(np.asarray(pg.nodes_1d(2, False), dtype=np.float64))
    dev = _plane(c["flux_u"])
    top_u = L.CBc(L.BC_FLUX, 0, 0.0, 0.0, dev.data_ptr())
    top_v = L.CBc(L.BC_FLUX, 0, -3e-5, 0.0, None)
    import torch
    sentinel, zero_c = np.full(TD.ccf_shape(g), SENTINEL), np.full(pg.parent_shape(CC), SENTINEL)
    inner = (slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny), slice(g.Hz, g.Hz + g.Nz))
    sh = TD.shares_of_case(pg, c, buoyancy)
    print(f"case {TD.IDS[n]} {buoyancy}: " + ", ".join(f"{k} {100 * v:.0f} %" for k, v in sh.items()))
    assert all(0 < v < 1 for v in sh.values()), sh
    for constant in (False, True):
        for maxima in (TD.MAXIMA, dict()):
            cl = _closure_dict(constant, C_W_ustar=2.5, C_b_eps_minus=-0.4, **maxima)
            cs = _c_struct(ocn, cl)
            s = TD.state_of(pg, c, buoyancy, cl)
            tag0 = f"constant = {constant} maxima = {bool(maxima)}"
            # the top fluxes
            Qe, Qp = (_plane(np.full((g.Nx, g.Ny), SENTINEL)) for _ in range(2))
            L.call("ocn_compute_tke_dissipation_top_fluxes", pg.cref, C.byref(cs), C.pointer(top_u), C.pointer(top_v), zc.data_ptr(), u.ptr, v.ptr,
                   e0.ptr, Qe.data_ptr(), Qp.data_ptr(), 0)
            want_Qe, want_Qp = TD.top_fluxes(s, c["flux_u"], -3e-5)
            assert np.all(want_Qe < 0) and np.all(want_Qp < 0) and _same(_from_plane(Qe), want_Qe) and _same(_from_plane(Qp), want_Qp), tag0
            # κᵘ, κᶜ, κᵉ, κᵋ
            kd = [to_dev(ocn, pg, CCF, sentinel) for _ in range(4)]
            L.call("ocn_compute_tke_dissipation_diffusivities", pg.cref, C.byref(terms), C.byref(cs), u.ptr, v.ptr, e0.ptr, p0.ptr,
                   *[k.ptr for k in kd], 0)
            ocn.sync_device()
            want = TD.diffusivities(s, sentinel, sentinel, sentinel, sentinel)
            for name, got, w in zip(("u", "c", "e", "eps"), kd, want):
                assert np.isfinite(w).all() and _same(from_dev(got), w), f"κ{name} {tag0}: {np.abs(from_dev(got) - w).max():.3e}"
                col = w[g.Hx:g.Hx + g.Nx, g.Hy:g.Hy + g.Ny]
                assert np.all(col[:, :, g.Hz] == 0) and np.all(col[:, :, g.Hz + g.Nz:] == SENTINEL) and np.all(col[:, :, :g.Hz] == SENTINEL)
                if maxima:
                    m = cl[TD.STABILITY[name][1]]
                    assert (w[w != SENTINEL] == m).any() and (w[w != SENTINEL] <= m).all()
            box, kc_h = TD.substep_inputs(g, want)  # κᵘ with its x / y halos filled and NaN beyond one column, κᶜ in the column only
            ku_d, kc_d = to_dev(ocn, pg, CCF, box), to_dev(ocn, pg, CCF, kc_h)
            scratch = torch.zeros((2, g.Nz, g.Ny, g.Nx), dtype=torch.float64, device="cuda")
            for chis, dtau in (((0.1,), 90.0), ((-0.5, 0.1, 0.1), 30.0)):
                for solve in (0, 1):
                    names = ("e", "ϵ", "κe", "κϵ", "Le", "Lϵ", "G⁻e", "G⁻ϵ")
                    w = [c["e"], c["eps"], sentinel, sentinel, zero_c, zero_c, c["Gm_e"], c["Gm_eps"]]
                    d = [to_dev(ocn, pg, CCF if q in (2, 3) else CC, a) for q, a in enumerate(w)]
                    Gn_e, Gn_p = to_dev(ocn, pg, CC, c["Gn_e"]), to_dev(ocn, pg, CC, c["Gn_eps"])
                    for chi in chis:
                        L.call("ocn_tke_dissipation_substep", pg.cref, C.byref(terms), C.byref(cs), u.ptr, v.ptr, up.ptr, vp.ptr, d[0].ptr, d[1].ptr,
                               ku_d.ptr, kc_d.ptr, d[2].ptr, d[3].ptr, d[4].ptr, d[5].ptr, Gn_e.ptr, d[6].ptr, Gn_p.ptr, d[7].ptr,
                               scratch.data_ptr(), dtau, chi, solve, 0)
                        sm = TD.state_of(pg, c, buoyancy, cl, e=w[0], eps=w[1])
                        w = list(TD.substep(sm, c["u_prev"], c["v_prev"], box, kc_h, w[2], w[3], w[4], w[5], c["Gn_e"], w[6], c["Gn_eps"], w[7], dtau, chi))
                        if solve:
                            w[0] = TD.implicit_step(g, w[0], w[2], w[4], dtau)
                            w[1] = TD.implicit_step(g, w[1], w[3], w[5], dtau)
                    ocn.sync_device()
                    tag = f"M = {len(chis)} solve = {solve} {tag0}"
                    assert all(np.isfinite(a[inner]).all() for q, a in enumerate(w) if q not in (2, 3)), tag
                    for name, got, a in zip(names, d, w):
                        assert _same(from_dev(got), a), f"{name} {tag}: {np.nanmax(np.abs(from_dev(got) - a)):.3e}"
                    assert _same(from_dev(Gn_e), c["Gn_e"]) and _same(from_dev(Gn_p), c["Gn_eps"])
                    assert not np.array_equal(w[0][inner], c["e"][inner]) and not np.array_equal(w[1][inner], c["eps"][inner])


# ---- 2. the model ------------------------------------------------------------------------------------------------------------------------------
T_FLUX, U_FLUX = 2e-5, -1e-4  # cooling (an upward heat flux), wind stress


def _model_grid(ocn, size=(16, 12, 8)):
    return ocn.RectilinearGrid(ocn.GPU(), size=size, x=(0, 1.6e6), y=(0, 1.2e6), z=(-64.0, 0.0), topology=(P, P, B), halo=(3, 3, 3))


def _free_surface(ocn, kind):
    return {"split": lambda: ocn.SplitExplicitFreeSurface(substeps=10), "implicit": lambda: ocn.ImplicitFreeSurface()}[kind]()


def _bcs(ocn, eps):
    return {"T": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(T_FLUX)),
            "u": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(U_FLUX)),
            "e": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(1.0)),  # (both replaced by the closure's own, as in the reference)
            eps: ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(1.0))}


def _initial(pg, eps, noise=1.0):
    rng = np.random.default_rng(12)
    Nx, Ny, Nz = pg.Nx, pg.Ny, pg.Nz
    zc = np.asarray(pg.nodes_1d(2, False))
    T = 20 + np.where(zc < -24, 0.01 * (zc + 24), 0.0)  # a mixed layer over a stratified interior
    init = {name: np.broadcast_to(0.05 * (zc / 64 + 1.0) ** 2, (Nx, Ny, Nz)) + noise * 1e-3 * rng.uniform(-1, 1, (Nx, Ny, Nz)) for name in "uv"}
    init["T"] = np.broadcast_to(T, (Nx, Ny, Nz)) + noise * 1e-3 * rng.uniform(-1, 1, (Nx, Ny, Nz))
    init["S"] = 35 + noise * 1e-3 * rng.uniform(-1, 1, (Nx, Ny, Nz))
    init["e"] = 2e-6 + noise * 1e-6 * rng.uniform(-1, 1, (Nx, Ny, Nz))
    init[eps] = 1e-8 + noise * 5e-9 * rng.uniform(-1, 1, (Nx, Ny, Nz))  # (above its floor everywhere: at most 𝕊u₀³ e^(3/2) / ℓ ≈ 4e-9 here)
    return init


def _model(ocn, kind, closure=None, pg=None, eps="epsilon", **kw):
    base = dict(tracers=("T", "S", "e", eps), buoyancy=ocn.SeawaterBuoyancy(), coriolis=ocn.FPlane(f=1e-4), math_mode=ocn.MATH_STRICT)
    base.update(kw)
    closure = ocn.TKEDissipationVerticalDiffusivity() if closure is None else closure
    return ocn.HydrostaticFreeSurfaceModel(pg or _model_grid(ocn), closure=closure, boundary_conditions=_bcs(ocn, eps),
                                           free_surface=_free_surface(ocn, kind), **base)


KAPPAS = ("kappa_u", "kappa_c", "kappa_e", "kappa_eps")


def _digests(m, eps="epsilon"):
    import hashlib
    out = {name: hashlib.sha256(np.ascontiguousarray(m.field(name).parent()).tobytes()).hexdigest() for name in ("u", "v", "w", "T", "S", "e", eps)}
    out["eta"] = hashlib.sha256(np.ascontiguousarray(m.eta.cpu().numpy()).tobytes()).hexdigest()
    for name in KAPPAS + ("Le", "Leps"):
        out[name] = hashlib.sha256(np.ascontiguousarray(m.diffusivity_fields[name].parent()).tobytes()).hexdigest()
    return out


class _Shadow:
    """wraps the closure object's compute_diffusivities: the state it is about to read is copied to the host, the restatement's sequence is
    applied to it, and the two results are compared after the launches.  chi: the χ the reference's time stepper holds during the
    update_state! in progress (quasi_adams_bashforth_2.jl:91-112), which the TEST sets before every step from its own list of steps: -1/2
    on the first step, on a step whose Δt differs from the one before and with euler = true, 0.1 otherwise -- never read from the model"""

    def __init__(self, ocn, m, time_step, eps, cl):
        self.ocn, self.m, self.tau, self.eps, self.cl, self.calls, self.chi = ocn, m, time_step, eps, cl, 0, None
        self.inner = m._closure.other if hasattr(m._closure, "other") else m._closure
        self.original = self.inner.compute_diffusivities
        m._closure.compute_diffusivities = self
        self.g = IDN.describe(m.grid)

    def __call__(self, nh):
        m, inner, g, eps = self.m, self.inner, self.g, self.eps
        self.ocn.sync_device()
        b = nh.buoyancy
        spec = ("SeawaterBuoyancy", b.gravitational_acceleration, b.equation_of_state.thermal_expansion, b.equation_of_state.haline_contraction)
        (Gn_e, Gm_e), (Gn_p, Gm_p) = inner._tendencies(nh, "e"), inner._tendencies(nh, eps)
        d = {name: inner.fields[name].parent() for name in KAPPAS + ("Le", "Leps")}
        d.update(u_prev=inner.u_prev.parent(), v_prev=inner.v_prev.parent())
        s = TD.State(g, m.grid.nodes_1d(2, True), m.grid.nodes_1d(2, False), m.grid.Lz, spec, self.cl, nh.u.parent(), nh.v.parent(),
                     nh.field("T").parent(), nh.field("S").parent(), nh.field("e").parent(), nh.field(eps).parent())
        want, e, p, Gm_e_w, Gm_p_w, Qe, Qp = TD.compute_diffusivities(s, d, dict(u=U_FLUX, v=None), nh.clock.last_dt, self.tau, self.chi,
                                                                      Gn_e.parent(), Gm_e.parent(), Gn_p.parent(), Gm_p.parent())
        self.original(nh)
        self.ocn.sync_device()
        tag = f"call {self.calls} iteration {nh.clock.iteration}"
        for name in KAPPAS + ("Le", "Leps"):
            assert _same(inner.fields[name].parent(), want[name]), f"{name} {tag}"
        assert _same(nh.field("e").parent(), e), f"e {tag}: {np.abs(nh.field('e').parent() - e).max():.3e}"
        assert _same(nh.field(eps).parent(), p), f"ϵ {tag}: {np.abs(nh.field(eps).parent() - p).max():.3e}"
        assert _same(inner._tendencies(nh, "e")[1].parent(), Gm_e_w), f"G⁻e {tag}"
        assert _same(inner._tendencies(nh, eps)[1].parent(), Gm_p_w), f"G⁻ϵ {tag}"
        assert _same(inner.tops["e"]._device_values.cpu().numpy().T, Qe), f"top flux of e {tag}"
        assert _same(inner.tops[eps]._device_values.cpu().numpy().T, Qp), f"top flux of ϵ {tag}"
        assert _same(inner.u_prev.parent(), nh.u.parent()) and _same(inner.v_prev.parent(), nh.v.parent())
        self.calls += 1


# (Δt, euler, the χ of the reference's time stepper during the step): the first step and every step with a changed Δt or euler = true are
# Euler steps (quasi_adams_bashforth_2.jl:88-96); written down here, not read from the model
STEPS = [(300.0, False, -0.5), (300.0, False, 0.1), (300.0, False, 0.1), (150.0, False, -0.5), (150.0, False, 0.1), (150.0, True, -0.5)]


@pytest.mark.parametrize("kind,time_step,eps,constant", [("split", None, "epsilon", False), ("implicit", 100.0, "ϵ", False),
                                                          ("split", 100.0, "ε", True)])
def test_model_closure_state_equals_the_restatement_s_sequence(ocn, kind, time_step, eps, constant):
    """16 x 12 x 8, wind stress and cooling, three steps of 300 s, then two of 150 s and one more with euler = true: at every
    compute_diffusivities! (set's, every update_state!'s) the four κ, Le, Lϵ, e, ϵ, G⁻e, G⁻ϵ and the two top fluxes equal the restatement's
    sequence applied to the model's own fields, with the χ of STEPS.  With tke_dissipation_time_step = 100 s three substeps per 300 s step and
    two per 150 s step, the first of them with χ = -1/2.  The dissipation tracer under each of its three names."""
    pg = _model_grid(ocn)
    sf = ocn.ConstantStabilityFunctions() if constant else ocn.VariableStabilityFunctions()
    eq = ocn.TKEDissipationEquations(C_W_ustar=1.5)
    m = _model(ocn, kind, ocn.TKEDissipationVerticalDiffusivity(tke_dissipation_time_step=time_step, stability_functions=sf,
                                                                tke_dissipation_equations=eq), pg, eps=eps)
    assert m.fused is False and sorted(m.diffusivity_fields) == sorted(KAPPAS + ("Le", "Leps"))
    assert all(m.diffusivity_fields[name].loc == CCF for name in KAPPAS) and all(m.diffusivity_fields[name].loc == CC for name in ("Le", "Leps"))
    shadow = _Shadow(ocn, m, time_step, eps, _closure_dict(constant, C_W_ustar=1.5))
    m.set(**_initial(pg, eps))
    e_before, p_before = m.field("e").parent(), m.field(eps).parent()
    for dt, euler, chi in STEPS:
        shadow.chi = chi
        m.time_step(dt, euler=euler)
        assert m._nh.timestepper.chi == 0.1  # restored after the step
    assert shadow.calls == 1 + 1 + len(STEPS)  # set, the update_state! that opens the first step, one per step
    g = shadow.g
    ke = m.diffusivity_fields["kappa_eps"].parent()[g.Hx:g.Hx + g.Nx, g.Hy:g.Hy + g.Ny]
    assert np.all(ke[:, :, g.Hz] == 0) and np.all(ke[:, :, g.Hz + g.Nz] == 0) and ke.max() > 1e-5
    for name, before in (("e", e_before), (eps, p_before)):
        assert np.isfinite(m.field(name).parent()).all() and not np.array_equal(m.field(name).parent(), before)


def test_top_fluxes_reach_the_tendencies(ocn):
    """The closure's own top conditions of e and ϵ are applied, and the user's (fluxes of 1.0 in _bcs) are not: after compute_tendencies! Gⁿe
    and Gⁿϵ of the top cells differ from those of a twin with Cᵂu★ = 0 and 𝕊u₀ = 0 (whose top fluxes are 0; ϵ is above its floor in both, so
    nothing else depends on 𝕊u₀) by -Q / Δz, Qe = -Cᵂu★ u★³, Qϵ = -𝕊u₀⁴ / Cσϵ e★² / (d + ℓᵣ); nowhere else.  Allowance: the kernel forms
    Q Az / (Az Δz) in three roundings and rounds the sum, the test rounds Q / Δz: five roundings of at most ε / 2 of the larger addend, 3 ε."""
    pg = _model_grid(ocn)
    init = _initial(pg, "epsilon")
    forced = ocn.TKEDissipationVerticalDiffusivity(tke_dissipation_equations=ocn.TKEDissipationEquations(C_W_ustar=1.5))
    calm = ocn.TKEDissipationVerticalDiffusivity(stability_functions=ocn.VariableStabilityFunctions(Su0=0.0))
    G = {}
    for name, closure in (("forced", forced), ("calm", calm)):
        m = _model(ocn, "split", closure, pg)
        m.set(**init)
        m.update_state(compute_tendencies=True)
        ocn.sync_device()
        G[name] = {t: m._closure._tendencies(m._nh, t)[0].interior()[:, :, :8] for t in ("e", "epsilon")}
        for t in ("e", "epsilon"):
            assert np.array_equal(m._closure.tops[t]._device_values.cpu().numpy() == 0, np.full((12, 16), name == "calm"))
    dz, d = 64.0 / 8, 64.0 / 16
    u_star = np.sqrt(np.sqrt(U_FLUX * U_FLUX + 0.0))
    Su0 = TD.closure_dict()["Su0"]
    l_r = max(1e-4, 0.11 * (u_star * u_star) / 9.8065)
    e_star = np.maximum(1e-6, init["e"][:, :, 7])
    Q = {"e": -1.5 * (u_star * u_star * u_star) + 0 * e_star, "epsilon": -((Su0 * Su0) * (Su0 * Su0) / 1.2) * (e_star * e_star) / (d + l_r)}
    for t in ("e", "epsilon"):
        assert np.all(Q[t] < 0) and np.array_equal(G["forced"][t][:, :, :7], G["calm"][t][:, :, :7])
        difference = G["forced"][t][:, :, 7] - G["calm"][t][:, :, 7]
        allowance = 3 * np.finfo(np.float64).eps * np.maximum(np.abs(G["calm"][t][:, :, 7]), -Q[t] / dz)
        print(f"{t}: -Q / Δz = {(-Q[t] / dz).min():.6e} .. {(-Q[t] / dz).max():.6e}, Gⁿ(top) differs by {difference.min():.6e} .. "
              f"{difference.max():.6e}, |Gⁿ(top)| of the calm twin up to {np.abs(G['calm'][t][:, :, 7]).max():.3e}")
        assert np.all(np.abs(difference - (-Q[t] / dz)) <= allowance)
        assert np.abs(G["calm"][t][:, :, 7]).max() < 1e-3 * (1.0 / dz)  # the user's top flux of 1.0 was replaced


def test_identical_runs_tuple_orders_and_checkpoint_restart(ocn, tmp_path):
    """two identical runs give identical digests; the pair with the biharmonic gives the same digests in either order; a checkpoint written
    after step 2 and restored into a fresh model continues to step 4 with the digests of the uninterrupted run"""
    pg = _model_grid(ocn)
    init = _initial(pg, "epsilon")
    new = lambda: ocn.TKEDissipationVerticalDiffusivity(tke_dissipation_time_step=200.0)

    def run(closure, steps=4, checkpoint=None):
        m = _model(ocn, "split", closure, pg)
        m.set(**init)
        for step in range(steps):
            m.time_step(300.0)
            if checkpoint and step == 1:
                ocn.write_checkpoint(m, checkpoint)
        ocn.sync_device()
        return m
    a, b = run(new()), run(new())
    assert _digests(a) == _digests(b)
    bih = lambda: ocn.HorizontalScalarBiharmonicDiffusivity(ν=1e15, κ=5e14)
    path = str(tmp_path / "tke_dissipation")
    p = run((new(), bih()), checkpoint=path)
    q = run((bih(), new()))
    assert _digests(p) == _digests(q) and _digests(p) != _digests(a)
    r = _model(ocn, "split", (bih(), new()), pg)
    ocn.set_from_checkpoint(r, path)
    assert r.clock.iteration == 2
    for _ in range(2):
        r.time_step(300.0)
    ocn.sync_device()
    assert r.clock.iteration == 4 and _digests(r) == _digests(p)
    plain = _model(ocn, "split", ocn.RiBasedVerticalDiffusivity(warning=False), pg)
    other = ocn.write_checkpoint(plain, str(tmp_path / "plain"))
    with pytest.raises(KeyError, match="TKEDissipationVerticalDiffusivity"):
        ocn.set_from_checkpoint(_model(ocn, "split", new(), pg), other)


def test_cooled_and_wind_forced_column_mixes(ocn):
    """4 x 4 x 32, uniform in x and y, 100 m deep, stratified with N² = 1e-5, cooled (Jᵇ = 1e-7) and wind-forced for 200 steps of 120 s: every
    field stays finite, and the column mixes more than a twin whose four maxima are 0 (which diffuses nothing): the spread of b over the upper
    quarter of the cells, max - min, is smaller"""
    grid = ocn.RectilinearGrid(ocn.GPU(), size=(4, 4, 32), x=(0, 4e5), y=(0, 4e5), z=(-100.0, 0.0), topology=(P, P, B), halo=(3, 3, 3))
    bcs = {"b": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(1e-7)),
           "u": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(-1e-4))}
    still = dict(maximum_tracer_diffusivity=0.0, maximum_tke_diffusivity=0.0, maximum_dissipation_diffusivity=0.0, maximum_viscosity=0.0)
    spread = {}
    for name, closure in (("k_epsilon", ocn.TKEDissipationVerticalDiffusivity()), ("still", ocn.TKEDissipationVerticalDiffusivity(**still))):
        model = ocn.HydrostaticFreeSurfaceModel(grid, tracers=("b", "e", "epsilon"), buoyancy=ocn.BuoyancyTracer(), closure=closure,
                                                boundary_conditions=bcs, free_surface=ocn.SplitExplicitFreeSurface(substeps=10),
                                                coriolis=ocn.FPlane(f=1e-4))
        model.set(b=lambda x, y, z: 1e-5 * z + 0 * x + 0 * y, e=1e-6, epsilon=1e-9)
        for step in range(200):
            model.time_step(120.0)
        ocn.sync_device()
        for f in model._nh.prognostic_fields():
            assert np.isfinite(f.interior()).all(), name
        for k in KAPPAS:
            assert np.isfinite(model.diffusivity_fields[k].parent()).all(), name
        b = model.field("b").interior()[0, 0, 24:32]
        spread[name] = float(b.max() - b.min())
        print(f"{name}: spread of b over the upper 8 cells {spread[name]:.3e}, max κc {model.diffusivity_fields['kappa_c'].interior().max():.3e}, "
              f"max e {model.field('e').interior().max():.3e}, max ϵ {model.field('epsilon').interior().max():.3e}")
        if name == "still":
            assert model.diffusivity_fields["kappa_c"].interior().max() <= 0.0
    assert spread["k_epsilon"] < spread["still"]
