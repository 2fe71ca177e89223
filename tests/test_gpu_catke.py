"""CATKEVerticalDiffusivity on the GPU (csrc/catke.hip): the entry points against the NumPy restatement of the reference (tests/catke_numpy.py,
pinned without a GPU in tests/test_host_catke.py) bit for bit on whole parent arrays; the hydrostatic model's closure state after every step
against the restatement's sequence applied to the model's own fields; reproducibility, the pair with the biharmonic in either order, a
bit-identical checkpoint restart, the reference's own time-stepping tests and a deepening mixed layer.

Shapes are the smallest at which the column kernels can still go wrong: 3 x 3 x 2 has one interior face per column, whose N²_above comes from
the top halo; 5 x 6 x 4 is below one workgroup; 67 x 13 x 9 (stretched z) has ragged second blocks in x (64 lanes) and y (4 rows); 130 x 9 x 7
has unequal wide halos and a third block in x."""
import ctypes as C

import numpy as np
import pytest

import catke_numpy as CK
import implicit_diffusion_numpy as IDN
from helpers import from_dev, stretched_faces, to_dev

pytestmark = pytest.mark.gpu

P, B = "Periodic", "Bounded"
U, V, CC, CCF = 1, 2, 0, 4  # location masks
SEAWATER = ("SeawaterBuoyancy", 9.80665, 1.67e-4, 7.80e-4)
SENTINEL = -7.0
# size, halo, stretched z, seed (chosen on the CPU so that the branch shares asserted in _shares hold)
CASES = [((3, 3, 2), (1, 1, 1), False, 0), ((5, 6, 4), (3, 3, 3), False, 0), ((67, 13, 9), (4, 4, 3), True, 0), ((130, 9, 7), (5, 6, 4), False, 0)]
IDS = ["3x3x2", "5x6x4", "67x13x9", "130x9x7"]
LZ = 64.0
JBE, EMIN = 1e-11, 1e-9


def make_grid(ocn, arch, n):
    size, halo, stretched, _ = CASES[n]
    z = LZ * stretched_faces(size[2]) if stretched else (-LZ, 0.0)
    return ocn.RectilinearGrid(arch, size=size, x=(0, 1000.0), y=(0, 500.0), z=z, topology=(P, P, B), halo=halo)


def make_inputs(pg, seed):
    """Seeded parent arrays, NaN beyond the reach of the entry points (include/ocn_hip.h).  T, S random (N² of both signs, of the size
    1e-5) but vertically constant in a share of the columns (N² == 0 exactly); u, v random (Ri of order one) but vertically constant on a
    block of columns (S² == 0 exactly there); e negative, within [0, minimum_tke] (the two end points included) and above; Jᵇ above the
    minimum in most columns, equal to it, zero and negative in the others"""
    g = IDN.describe(pg)
    rng = np.random.default_rng(8800 + seed)
    Nx, Ny, Nz, Hx, Hy, Hz = g.Nx, g.Ny, g.Nz, g.Hx, g.Hy, g.Hz
    sx, sy, sz = slice(Hx, Hx + Nx), slice(Hy, Hy + Ny), slice(Hz, Hz + Nz)

    def masked(full, keep):
        out = np.full(full.shape, np.nan)
        out[keep] = full[keep]
        return out
    u, v = (0.05 * rng.uniform(-1, 1, pg.parent_shape(loc)) for loc in (U, V))
    bx, by = max(1, (Nx + 1) // 3), max(1, (2 * Ny) // 3)  # the block at rest relative to itself: columns 1..bx, 1..by
    u[Hx:Hx + bx + 1, Hy:Hy + by, :] = u[Hx:Hx + bx + 1, Hy:Hy + by, Hz:Hz + 1]
    v[Hx:Hx + bx, Hy:Hy + by + 1, :] = v[Hx:Hx + bx, Hy:Hy + by + 1, Hz:Hz + 1]
    T = 20 + 0.05 * rng.uniform(-1, 1, pg.parent_shape(CC))
    S = 35 + 0.01 * rng.uniform(-1, 1, pg.parent_shape(CC))
    flat = rng.uniform(0, 1, (Nx, Ny)) < 0.15
    flat.flat[rng.integers(0, flat.size)] = True
    for a in (T, S):
        a[sx, sy, :] = np.where(flat[:, :, None], a[sx, sy, Hz:Hz + 1], a[sx, sy, :])
    kind = rng.uniform(0, 1, pg.parent_shape(CC))
    e = np.where(kind < 0.25, -1e-5 * rng.uniform(0.1, 1, kind.shape),
                 np.where(kind < 0.5, EMIN * rng.uniform(0, 1, kind.shape), 10.0 ** rng.uniform(-6, -3, kind.shape)))
    e = np.where((kind >= 0.25) & (kind < 0.30), 0.0, np.where((kind >= 0.30) & (kind < 0.33), EMIN, e))
    jk = rng.uniform(0, 1, (Nx, Ny))
    Jb = np.where(jk < 0.07, 0.0, np.where(jk < 0.14, JBE, np.where(jk < 0.22, -1e-8, 10.0 ** rng.uniform(-9, -7, (Nx, Ny)))))
    c = dict(g=g, flat=flat, Jb=Jb,
             u=masked(u, (slice(Hx, Hx + Nx + 1), sy, sz)), v=masked(v, (sx, slice(Hy, Hy + Ny + 1), sz)),
             T=masked(T, (sx, sy, slice(Hz, Hz + Nz + 1))), S=masked(S, (sx, sy, slice(Hz, Hz + Nz + 1))), e=masked(e, (sx, sy, sz)),
             u_prev=masked(u + 0.01 * rng.uniform(-1, 1, u.shape), (slice(Hx, Hx + Nx + 1), sy, sz)),
             v_prev=masked(v + 0.01 * rng.uniform(-1, 1, v.shape), (sx, slice(Hy, Hy + Ny + 1), sz)),
             Gn=masked(1e-8 * rng.uniform(-1, 1, e.shape), (sx, sy, sz)), Gm=masked(1e-8 * rng.uniform(-1, 1, e.shape), (sx, sy, sz)),
             flux_T=1e-5 * rng.uniform(-1, 1, (Nx, Ny)), flux_u=1e-4 * rng.uniform(-1, 1, (Nx, Ny)))
    return c


def tracers_of(c, buoyancy):
    """(spec of the restatement, T, S): the buoyancy tracer is g (α T - β S) itself"""
    if buoyancy == "SeawaterBuoyancy":
        return SEAWATER, c["T"], c["S"]
    return "BuoyancyTracer", SEAWATER[1] * (SEAWATER[2] * c["T"] - SEAWATER[3] * c["S"]), None


def state_of(pg, c, buoyancy, cl=None, e=None, Jb=None):
    spec, T, S = tracers_of(c, buoyancy)
    return CK.State(c["g"], pg.nodes_1d(2, True), pg.nodes_1d(2, False), pg.Lz, spec, cl or CK.closure_dict(), c["u"], c["v"], T, S,
                    c["e"] if e is None else e, c["Jb"] if Jb is None else Jb)


def shares(s):
    """the share of the interior faces (k = 2..Nz) / cells / columns in every branch, counted in the restatement"""
    g = s.g
    faces = {name: [] for name in ("convecting", "entraining", "neither", "N2_zero", "S2_zero")}
    for k in range(2, g.Nz + 1):
        _, conv, entr = CK.convective_length_ccf(s, k, 4.793, 0.112, with_branches=True)
        faces["convecting"].append(conv)
        faces["entraining"].append(entr)
        faces["neither"].append(~conv & ~entr)
        faces["N2_zero"].append(CK.dz_b(s, k) == 0)
        faces["S2_zero"].append(CK.shear_ccf(s, k) == 0)
    out = {name: float(np.mean(v)) for name, v in faces.items()}
    e = s.e[g.Hx:g.Hx + g.Nx, g.Hy:g.Hy + g.Ny, g.Hz:g.Hz + g.Nz]
    out.update(e_negative=float(np.mean(e < 0)), e_small=float(np.mean((e >= 0) & (e <= s.cl["minimum_tke"]))),
               Jb_below=float(np.mean(s.Jb <= s.cl["minimum_convective_buoyancy_flux"])))
    return out


_cases = {}


def _case(ocn, n):
    if n not in _cases:
        pg = make_grid(ocn, ocn.GPU(), n)
        _cases[n] = (pg, make_inputs(pg, CASES[n][3]))
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


def _flux(ocn, a):
    """a top flux condition with an array (kept alive with the struct)"""
    L = ocn._lib
    dev = _plane(a)
    return L.CBc(L.BC_FLUX, 0, 0.0, 0.0, dev.data_ptr()), dev


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


# ---- 1. the entry points bit for bit -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("buoyancy", ["SeawaterBuoyancy", "BuoyancyTracer"])
@pytest.mark.parametrize("n", range(len(CASES)), ids=IDS)
def test_entry_points_equal_the_restatement_bit_for_bit(ocn, n, buoyancy):
    """Jᵇ, the top flux of e, the three diffusivities, then the substep alone and the fused substep + solve with M = 1 (χ = 0.1) and M = 3
    (χ = -1/2, 0.1, 0.1), with clipping maxima and with the reference's +inf: whole parent arrays, prefilled with a sentinel where they are
    only written, so halos and face Nz + 1 are shown untouched.  The branch shares of the inputs are asserted first."""
    pg, c = _case(ocn, n)
    g, L = c["g"], ocn._lib
    spec, Th, Sh = tracers_of(c, buoyancy)
    sh = shares(state_of(pg, c, buoyancy))
    print(f"case {IDS[n]} {buoyancy}: " + ", ".join(f"{k} {100 * v:.0f} %" for k, v in sh.items()))
    assert all(0.05 <= v <= 0.60 for v in sh.values()), sh
    T, S = to_dev(ocn, pg, CC, Th), to_dev(ocn, pg, CC, Sh if Sh is not None else c["S"])
    u, v, e0 = to_dev(ocn, pg, U, c["u"]), to_dev(ocn, pg, V, c["v"]), to_dev(ocn, pg, CC, c["e"])
    up, vp = to_dev(ocn, pg, U, c["u_prev"]), to_dev(ocn, pg, V, c["v_prev"])
    terms = _terms(ocn, buoyancy, T, S)
    zf, zc = (_plane(np.asarray(pg.nodes_1d(2, face), dtype=np.float64)) for face in (True, False))
    top_T, keep_T = _flux(ocn, c["flux_T"])
    top_u, keep_u = _flux(ocn, c["flux_u"])
    top_v = L.CBc(L.BC_FLUX, 0, -3e-5, 0.0, None)
    none = C.POINTER(L.CBc)()
    import torch
    for maxima in (dict(), dict(maximum_viscosity=2e-3, maximum_tracer_diffusivity=1e-3, maximum_tke_diffusivity=5e-3)):
        cl = CK.closure_dict(**maxima)
        cs = L.CCatke(*[cl[name] for name in L.CATKE_FIELDS])
        s = state_of(pg, c, buoyancy, cl)
        # Jᵇ
        Jb = _plane(c["Jb"])
        L.call("ocn_compute_catke_surface_buoyancy_flux", pg.cref, C.byref(terms), C.byref(cs), C.pointer(top_T), none, zf.data_ptr(), zc.data_ptr(),
               u.ptr, v.ptr, e0.ptr, Jb.data_ptr(), 37.5, 0)
        want_Jb = CK.surface_buoyancy_flux(s, c["flux_T"], None, 37.5)
        assert np.isfinite(want_Jb).all() and not np.array_equal(want_Jb, c["Jb"])
        assert _same(_from_plane(Jb), want_Jb)
        # the top flux of e
        Qe = _plane(np.full((g.Nx, g.Ny), SENTINEL))
        L.call("ocn_compute_catke_top_tke_flux", pg.cref, C.byref(terms), C.byref(cs), C.pointer(top_u), C.pointer(top_v), C.pointer(top_T), none,
               u.ptr, v.ptr, Qe.data_ptr(), 0)
        want_Q = CK.top_tke_flux(s, c["flux_u"], -3e-5, c["flux_T"], None)
        assert np.all(want_Q < 0) and _same(_from_plane(Qe), want_Q)
        # κᵘ, κᶜ, κᵉ with the Jᵇ of the inputs
        sentinel = np.full(CK.ccf_shape(g), SENTINEL)
        Jb0 = _plane(c["Jb"])
        ku, kc, ke = (to_dev(ocn, pg, CCF, sentinel) for _ in range(3))
        L.call("ocn_compute_catke_diffusivities", pg.cref, C.byref(terms), C.byref(cs), zf.data_ptr(), zc.data_ptr(), u.ptr, v.ptr, e0.ptr,
               Jb0.data_ptr(), ku.ptr, kc.ptr, ke.ptr, 0)
        ocn.sync_device()
        want = CK.diffusivities(s, sentinel, sentinel, sentinel)
        for name, got, w in zip("uce", (ku, kc, ke), want):
            assert np.isfinite(w).all() and _same(from_dev(got), w), f"κ{name}: {np.abs(from_dev(got) - w).max():.3e}"
            inner = w[g.Hx:g.Hx + g.Nx, g.Hy:g.Hy + g.Ny]
            assert np.all(inner[:, :, g.Hz] == 0) and np.all(inner[:, :, g.Hz + g.Nz:] == SENTINEL) and np.all(inner[:, :, g.Hz + 1:g.Hz + g.Nz] >= 0)
        if maxima:
            assert all((w[w != SENTINEL] == m).any() and (w[w != SENTINEL] <= m).all() for w, m in zip(want, (2e-3, 1e-3, 5e-3)))
        # the substep: κᵘ with its x / y halos filled and NaN beyond one column, κᶜ in the column only
        ku_h = CK.fill_xy_halos(g, want[0])
        box = np.full(ku_h.shape, np.nan)
        sl1 = (slice(g.Hx - 1, g.Hx + g.Nx + 1), slice(g.Hy - 1, g.Hy + g.Ny + 1), slice(g.Hz + 1, g.Hz + g.Nz))
        box[sl1] = ku_h[sl1]
        kc_h = np.full(ku_h.shape, np.nan)
        sl0 = (slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny), slice(g.Hz + 1, g.Hz + g.Nz))
        kc_h[sl0] = want[1][sl0]
        ku_d, kc_d = to_dev(ocn, pg, CCF, box), to_dev(ocn, pg, CCF, kc_h)
        zero_c = np.full(pg.parent_shape(CC), SENTINEL)
        scratch = torch.zeros((g.Nz, g.Ny, g.Nx), dtype=torch.float64, device="cuda")
        for chis, dtau in (((0.1,), 90.0), ((-0.5, 0.1, 0.1), 30.0)):
            for solve in (0, 1):
                e, Gm = to_dev(ocn, pg, CC, c["e"]), to_dev(ocn, pg, CC, c["Gm"])
                Gn, Le, ke2 = to_dev(ocn, pg, CC, c["Gn"]), to_dev(ocn, pg, CC, zero_c), to_dev(ocn, pg, CCF, sentinel)
                w_e, w_ke, w_Le, w_Gm = c["e"], sentinel, zero_c, c["Gm"]
                for chi in chis:
                    L.call("ocn_catke_substep_tke", pg.cref, C.byref(terms), C.byref(cs), zf.data_ptr(), zc.data_ptr(), u.ptr, v.ptr, up.ptr, vp.ptr,
                           e.ptr, Jb0.data_ptr(), ku_d.ptr, kc_d.ptr, ke2.ptr, Le.ptr, Gn.ptr, Gm.ptr, scratch.data_ptr(), dtau, chi, solve, 0)
                    sm = state_of(pg, c, buoyancy, cl, e=w_e)
                    w_e, w_ke, w_Le, w_Gm = CK.substep(sm, c["u_prev"], c["v_prev"], box, kc_h, w_ke, w_Le, c["Gn"], w_Gm, dtau, chi)
                    if solve:
                        w_e = CK.implicit_step_e(g, w_e, w_ke, w_Le, dtau)
                ocn.sync_device()
                tag = f"M = {len(chis)} solve = {solve} maxima = {bool(maxima)}"
                inner = (slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny), slice(g.Hz, g.Hz + g.Nz))
                assert np.isfinite(w_e[inner]).all() and np.isfinite(w_Le[inner]).all() and np.isfinite(w_Gm[inner]).all(), tag
                for name, got, w in (("e", e, w_e), ("κe", ke2, w_ke), ("Le", Le, w_Le), ("G⁻e", Gm, w_Gm)):
                    assert _same(from_dev(got), w), f"{name} {tag}: {np.nanmax(np.abs(from_dev(got) - w)):.3e}"
                assert _same(from_dev(Gn), c["Gn"])
                assert not np.array_equal(w_e[inner], c["e"][inner])


# ---- 2. the model ------------------------------------------------------------------------------------------------------------------------------
T_FLUX, U_FLUX = 2e-5, -1e-4  # cooling (an upward heat flux), wind stress


def _model_grid(ocn, size=(16, 12, 8)):
    return ocn.RectilinearGrid(ocn.GPU(), size=size, x=(0, 1.6e6), y=(0, 1.2e6), z=(-64.0, 0.0), topology=(P, P, B), halo=(3, 3, 3))


def _free_surface(ocn, kind):
    return {"split": lambda: ocn.SplitExplicitFreeSurface(substeps=10), "implicit": lambda: ocn.ImplicitFreeSurface()}[kind]()


def _bcs(ocn):
    return {"T": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(T_FLUX)),
            "u": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(U_FLUX)),
            "e": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(1.0))}  # (replaced by the closure's own, as in the reference)


def _initial(pg, noise=1.0):
    rng = np.random.default_rng(12)
    Nx, Ny, Nz = pg.Nx, pg.Ny, pg.Nz
    zc = np.asarray(pg.nodes_1d(2, False))
    T = 20 + np.where(zc < -24, 0.01 * (zc + 24), 0.0)  # a mixed layer over a stratified interior
    init = {name: np.broadcast_to(0.05 * (zc / 64 + 1.0) ** 2, (Nx, Ny, Nz)) + noise * 1e-3 * rng.uniform(-1, 1, (Nx, Ny, Nz)) for name in "uv"}
    init["T"] = np.broadcast_to(T, (Nx, Ny, Nz)) + noise * 1e-3 * rng.uniform(-1, 1, (Nx, Ny, Nz))
    init["S"] = 35 + noise * 1e-3 * rng.uniform(-1, 1, (Nx, Ny, Nz))
    init["e"] = 1e-6 + noise * 1e-6 * rng.uniform(-1, 1, (Nx, Ny, Nz))
    return init


def _model(ocn, kind, closure=None, pg=None, **kw):
    base = dict(tracers=("T", "S", "e"), buoyancy=ocn.SeawaterBuoyancy(), coriolis=ocn.FPlane(f=1e-4), math_mode=ocn.MATH_STRICT)
    base.update(kw)
    closure = ocn.CATKEVerticalDiffusivity() if closure is None else closure
    return ocn.HydrostaticFreeSurfaceModel(pg or _model_grid(ocn), closure=closure, boundary_conditions=_bcs(ocn),
                                           free_surface=_free_surface(ocn, kind), **base)


def _digests(m):
    import hashlib
    out = {name: hashlib.sha256(np.ascontiguousarray(m.field(name).parent()).tobytes()).hexdigest() for name in ("u", "v", "w", "T", "S", "e")}
    out["eta"] = hashlib.sha256(np.ascontiguousarray(m.eta.cpu().numpy()).tobytes()).hexdigest()
    for name in ("kappa_u", "kappa_c", "kappa_e", "Le"):
        out[name] = hashlib.sha256(np.ascontiguousarray(m.diffusivity_fields[name].parent()).tobytes()).hexdigest()
    out["Jb"] = hashlib.sha256(np.ascontiguousarray(m.diffusivity_fields["Jb"].cpu().numpy()).tobytes()).hexdigest()
    return out


class _Shadow:
    """wraps the closure object's compute_diffusivities: the state it is about to read is copied to the host, the restatement's sequence is
    applied to it, and the two results are compared after the launches.  chi: the χ the reference's time stepper holds during the
    update_state! in progress (quasi_adams_bashforth_2.jl:91-112), which the TEST sets before every step from its own list of steps: -1/2
    on the first step, on a step whose Δt differs from the one before and with euler = true, 0.1 otherwise -- never read from the model"""

    def __init__(self, ocn, m, tke_time_step):
        self.ocn, self.m, self.tau, self.calls, self.chi = ocn, m, tke_time_step, 0, None
        self.inner = m._closure.other if hasattr(m._closure, "other") else m._closure
        self.original = self.inner.compute_diffusivities
        m._closure.compute_diffusivities = self
        self.g = IDN.describe(m.grid)

    def __call__(self, nh):
        m, inner, g = self.m, self.inner, self.g
        self.ocn.sync_device()
        b = nh.buoyancy
        spec = ("SeawaterBuoyancy", b.gravitational_acceleration, b.equation_of_state.thermal_expansion, b.equation_of_state.haline_contraction)
        Gn, Gm = inner._e_tendencies(nh)
        d = {name: inner.fields[name].parent() for name in ("kappa_u", "kappa_c", "kappa_e", "Le")}
        d.update(Jb=inner.fields["Jb"].cpu().numpy().T, u_prev=inner.u_prev.parent(), v_prev=inner.v_prev.parent(),
                 previous_compute_time=inner.previous_compute_time)
        cs = inner.struct
        cl = CK.closure_dict(**{name: getattr(cs, name) for name in CK.closure_dict()})
        s = CK.State(g, m.grid.nodes_1d(2, True), m.grid.nodes_1d(2, False), m.grid.Lz, spec, cl, nh.u.parent(), nh.v.parent(),
                     nh.field("T").parent(), nh.field("S").parent(), nh.field("e").parent(), d["Jb"])
        tops = dict(u=U_FLUX, v=None, T=T_FLUX, S=None)
        want, e, Gm_w, Qe = CK.compute_diffusivities(s, d, tops, nh.clock.time, nh.clock.last_dt, self.tau, self.chi, Gn.parent(), Gm.parent())
        self.original(nh)
        self.ocn.sync_device()
        tag = f"call {self.calls} iteration {nh.clock.iteration}"
        for name in ("kappa_u", "kappa_c", "kappa_e", "Le"):
            assert _same(inner.fields[name].parent(), want[name]), f"{name} {tag}"
        assert _same(inner.fields["Jb"].cpu().numpy().T, want["Jb"]), f"Jb {tag}"
        assert _same(nh.field("e").parent(), e), f"e {tag}: {np.abs(nh.field('e').parent() - e).max():.3e}"
        assert _same(inner._e_tendencies(nh)[1].parent(), Gm_w), f"G⁻e {tag}"
        assert _same(inner.top_e._device_values.cpu().numpy().T, Qe), f"top flux of e {tag}"
        assert _same(inner.u_prev.parent(), nh.u.parent()) and inner.previous_compute_time == nh.clock.time
        self.calls += 1


# (Δt, euler, the χ of the reference's time stepper during the step): the first step and every step with a changed Δt or euler = true are
# Euler steps (quasi_adams_bashforth_2.jl:88-96); written down here, not read from the model
STEPS = [(300.0, False, -0.5), (300.0, False, 0.1), (300.0, False, 0.1), (150.0, False, -0.5), (150.0, False, 0.1), (150.0, True, -0.5)]


@pytest.mark.parametrize("kind,tke_time_step", [("split", None), ("implicit", 100.0)])
def test_model_closure_state_equals_the_restatement_s_sequence(ocn, kind, tke_time_step):
    """16 x 12 x 8, wind stress and cooling, three steps of 300 s, then two of 150 s and one more with euler = true: at every
    compute_diffusivities! (set's, every update_state!'s) κᵘ, κᶜ, κᵉ, Le, Jᵇ, e, G⁻e and the top flux of e equal the restatement's sequence
    applied to the model's own fields, with the χ of STEPS: e takes an Euler substep on the first step, after a change of Δt and with
    euler = true.  With tke_time_step = 100 s three substeps per 300 s step and two per 150 s step."""
    pg = _model_grid(ocn)
    m = _model(ocn, kind, ocn.CATKEVerticalDiffusivity(tke_time_step=tke_time_step), pg)
    assert m.fused is False and sorted(m.diffusivity_fields) == ["Jb", "Le", "kappa_c", "kappa_e", "kappa_u"]
    assert tuple(m.diffusivity_fields["Jb"].shape) == (12, 16) and m.diffusivity_fields["Le"].loc == CC
    assert all(m.diffusivity_fields[name].loc == CCF for name in ("kappa_u", "kappa_c", "kappa_e"))
    shadow = _Shadow(ocn, m, tke_time_step)
    m.set(**_initial(pg))
    e_before = m.field("e").parent()
    for dt, euler, chi in STEPS:
        shadow.chi = chi
        m.time_step(dt, euler=euler)
        assert m._nh.timestepper.chi == 0.1  # restored after the step
    assert shadow.calls == 1 + 1 + len(STEPS)  # set, the update_state! that opens the first step, one per step
    g = shadow.g
    ke = m.diffusivity_fields["kappa_e"].parent()[g.Hx:g.Hx + g.Nx, g.Hy:g.Hy + g.Ny]
    assert np.all(ke[:, :, g.Hz] == 0) and np.all(ke[:, :, g.Hz + g.Nz] == 0) and ke.max() > 1e-4
    assert np.isfinite(m.field("e").parent()).all() and not np.array_equal(m.field("e").parent(), e_before)
    assert m.diffusivity_fields["Jb"].min().item() > 0  # the cooling has been averaged in


def test_top_flux_of_e_reaches_its_tendency(ocn):
    """The closure's own top condition of e is applied, and the user's (a flux of 1.0 in _bcs) is not: after compute_tendencies! Gⁿe of the top
    cells differs from that of a twin with Cᵂu★ = CᵂwΔ = 0 (whose top flux is 0) by -Qe / Δz, Qe = -Cᵂu★ u★³ - CᵂwΔ wΔ³ of the restatement; nowhere
    else.  Allowance: the kernel forms Qe Az / (Az Δz) in three roundings and rounds the sum, the test rounds Qe / Δz: five roundings of at most
    ε / 2 of the larger addend, 3 ε."""
    pg = _model_grid(ocn)
    init = _initial(pg)
    calm = ocn.CATKEEquation(C_W_ustar=0.0, C_W_wdelta=0.0)
    G = {}
    for name, closure in (("forced", ocn.CATKEVerticalDiffusivity()), ("calm", ocn.CATKEVerticalDiffusivity(turbulent_kinetic_energy_equation=calm))):
        m = _model(ocn, "split", closure, pg)
        m.set(**init)
        m.update_state(compute_tendencies=True)
        ocn.sync_device()
        G[name] = m._closure._e_tendencies(m._nh)[0].interior()[:, :, :8]
        assert np.array_equal(m._closure.top_e._device_values.cpu().numpy() == 0, np.full((12, 16), name == "calm"))
    dz = 64.0 / 8
    u_star = np.sqrt(np.sqrt(U_FLUX * U_FLUX + 0.0))
    Jb = SEAWATER[1] * (ocn.SeawaterBuoyancy().equation_of_state.thermal_expansion * T_FLUX - 0.0)
    Qe = -3.179 * (u_star * u_star * u_star) - 0.383 * (max(0.0, Jb) * dz)
    assert Qe < 0 and np.array_equal(G["forced"][:, :, :7], G["calm"][:, :, :7])
    difference = G["forced"][:, :, 7] - G["calm"][:, :, 7]
    allowance = 3 * np.finfo(np.float64).eps * max(np.abs(G["calm"][:, :, 7]).max(), -Qe / dz)
    print(f"-Qe / Δz = {-Qe / dz:.6e}, Gⁿe(top) differs by {difference.min():.6e} .. {difference.max():.6e}, allowance {allowance:.1e}, "
          f"|Gⁿe(top)| of the calm twin up to {np.abs(G['calm'][:, :, 7]).max():.3e}")
    assert np.all(np.abs(difference - (-Qe / dz)) <= allowance)
    assert np.abs(G["calm"][:, :, 7]).max() < 1e-3 * (1.0 / dz)  # the user's top flux of 1.0 on e was replaced


def test_identical_runs_tuple_orders_and_checkpoint_restart(ocn, tmp_path):
    """two identical runs give identical digests; the pair with the biharmonic gives the same digests in either order; a checkpoint written
    after step 2 and restored into a fresh model continues to step 4 with the digests of the uninterrupted run"""
    pg = _model_grid(ocn)
    init = _initial(pg)

    def run(closure, steps=4, checkpoint=None):
        m = _model(ocn, "split", closure, pg)
        m.set(**init)
        for step in range(steps):
            m.time_step(300.0)
            if checkpoint and step == 1:
                ocn.write_checkpoint(m, checkpoint)
        ocn.sync_device()
        return m
    a, b = run(ocn.CATKEVerticalDiffusivity()), run(ocn.CATKEVerticalDiffusivity())
    assert _digests(a) == _digests(b)
    bih = lambda: ocn.HorizontalScalarBiharmonicDiffusivity(ν=1e15, κ=5e14)
    path = str(tmp_path / "catke")
    p = run((ocn.CATKEVerticalDiffusivity(), bih()), checkpoint=path)
    q = run((bih(), ocn.CATKEVerticalDiffusivity()))
    assert _digests(p) == _digests(q) and _digests(p) != _digests(a)
    r = _model(ocn, "split", (bih(), ocn.CATKEVerticalDiffusivity()), pg)
    ocn.set_from_checkpoint(r, path)
    assert r.clock.iteration == 2
    for _ in range(2):
        r.time_step(300.0)
    ocn.sync_device()
    assert r.clock.iteration == 4 and _digests(r) == _digests(p)
    plain = _model(ocn, "split", ocn.RiBasedVerticalDiffusivity(warning=False), pg)
    other = ocn.write_checkpoint(plain, str(tmp_path / "plain"))
    with pytest.raises(KeyError, match="CATKEVerticalDiffusivity"):
        ocn.set_from_checkpoint(_model(ocn, "split", None, pg), other)


@pytest.mark.parametrize("scheme", ["default", "weno"])
def test_reference_time_stepping_tests(ocn, scheme):
    """time_step_hydrostatic_model_works (test_hydrostatic_free_surface_models.jl:11-30) with CATKEVerticalDiffusivity(): tracers b and e,
    one step of Δt = 1, with the default schemes and with WENOVectorInvariant(order=5) / WENO(); every field finite"""
    grid = ocn.RectilinearGrid(ocn.GPU(), size=(8, 8, 8), x=(0, 2 * np.pi), y=(0, 2 * np.pi), z=(-2 * np.pi, 0), topology=(P, P, B), halo=(3, 3, 3))
    kw = dict(momentum_advection=ocn.WENOVectorInvariant(order=5), tracer_advection=ocn.WENO()) if scheme == "weno" else {}
    model = ocn.HydrostaticFreeSurfaceModel(grid, tracers=("b", "e"), buoyancy=ocn.BuoyancyTracer(), closure=ocn.CATKEVerticalDiffusivity(), **kw)
    model.time_step(1.0)
    ocn.sync_device()
    assert model.clock.iteration == 1
    for f in model._nh.prognostic_fields():
        assert np.isfinite(f.interior()).all()
    for name in ("kappa_u", "kappa_c", "kappa_e", "Le"):
        assert np.isfinite(model.diffusivity_fields[name].parent()).all()


def test_cooled_and_wind_forced_column_deepens(ocn):
    """4 x 4 x 32, uniform in x and y, 100 m deep, stratified with N² = 1e-5, cooled (Jᵇ = 1e-7) and wind-forced for 200 steps of 120 s: the
    mixed layer (the depth of the deepest cell whose b is within 2e-5 of the top cell's) deepens monotonically, e stays >= 0 to
    rounding, every field is finite"""
    grid = ocn.RectilinearGrid(ocn.GPU(), size=(4, 4, 32), x=(0, 4e5), y=(0, 4e5), z=(-100.0, 0.0), topology=(P, P, B), halo=(3, 3, 3))
    bcs = {"b": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(1e-7)),
           "u": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(-1e-4))}
    model = ocn.HydrostaticFreeSurfaceModel(grid, tracers=("b", "e"), buoyancy=ocn.BuoyancyTracer(), closure=ocn.CATKEVerticalDiffusivity(),
                                            boundary_conditions=bcs, free_surface=ocn.SplitExplicitFreeSurface(substeps=10),
                                            coriolis=ocn.FPlane(f=1e-4))
    zc = np.asarray(grid.nodes_1d(2, False))
    model.set(b=lambda x, y, z: 1e-5 * z + 0 * x + 0 * y, e=1e-6)

    def mixed_layer_depth():
        b = model.field("b").interior()[0, 0, :32]
        below = np.nonzero(b < b[-1] - 2e-5)[0]  # the cells denser than the surface cell by more than Δb = 2e-5
        return -zc[below[-1]] if below.size else 100.0
    depths, e_min = [mixed_layer_depth()], 0.0
    for step in range(200):
        model.time_step(120.0)
        if step % 20 == 19:
            ocn.sync_device()
            depths.append(mixed_layer_depth())
            e_min = min(e_min, float(model.field("e").interior().min()))
    print(f"mixed-layer depth every 20 steps: {depths}; min e {e_min:.3e}; max e {model.field('e').interior().max():.3e}")
    assert all(b >= a for a, b in zip(depths, depths[1:])) and depths[-1] > depths[0] + 5.0
    assert e_min >= -1e-12
    for f in model._nh.prognostic_fields():
        assert np.isfinite(f.interior()).all()
    assert model.field("e").interior().max() > 1e-5  # turbulent
