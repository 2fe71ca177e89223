"""IsopycnalSkewSymmetricDiffusivity on the GPU (csrc/isopycnal.hip): every entry point against the NumPy restatement of the reference
(tests/isopycnal_numpy.py, pinned without a GPU in tests/test_host_isopycnal.py) bit for bit on whole parent arrays, and steps of the
hydrostatic model against a twin whose closure is composed by hand from those entry points.

The grids (ISN.CASES): 3 x 3 x 3, the reference's own test grid, with halos (3, 3, 3) and (1, 1, 1); 5 x 4 x 2 with one interior z face
(halo (3, 3, 2): a halo may not exceed the size); and 37 x 11 x 4 with a stretched z: the flux kernel works on 32 x 8 tiles of the xy plane
(iso::TX, iso::TY), the diffusivity kernel on 64 x 4 blocks of columns, so 37 x 11 is one full tile plus a partial one in x and in y for the
first and a partial block in x and three blocks in y for the second.  Every grid marches fewer planes than a chunk of 16 holds; the chunk
boundary is met by the 20-plane grid of the last entry-point test.  The shared input (ISN.case_inputs) puts at least 5 % of the faces of every
kind into each branch: untapered, tapered, ∂z b < 0, ∂z b == 0 with 0 / 0 slopes."""
import ctypes as C

import numpy as np
import pytest

import implicit_diffusion_numpy as IDN
import isopycnal_numpy as ISN
from helpers import from_dev, to_dev

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
U, V, CC, CCF = 1, 2, 0, 4  # location masks
BUOYANCIES = {"b": ISN.TRACER, "TS": ISN.SEAWATER}
KS, KW = (900.0, 250.0, 40.0), (400.0, 0.0, 100.0)
# (κ_symmetric, κ_skew inside the fluxes) of up to three tracers: the AdvectiveFormulation (or κ_skew = nothing) has κ_skew = 0 there
VARIANTS = {"advective": ((900.0,) * 3, (0.0,) * 3), "diffusive": ((900.0,) * 3, (400.0,) * 3),
            "symmetric_nothing": ((0.0,) * 3, (400.0,) * 3), "per_tracer": (KS, KW)}


def _terms(ocn, buoyancy, T, S):
    t = ocn._lib.CModelTerms()
    if buoyancy[0] == "BuoyancyTracer":
        t.buoyancy, t.T = ocn._lib.BUOYANCY_TRACER, T.ptr
    else:
        t.buoyancy, t.g, t.alpha, t.beta, t.T, t.S = ocn._lib.BUOYANCY_SEAWATER_TS, buoyancy[1], buoyancy[2], buoyancy[3], T.ptr, S.ptr
    return t


def _poisoned(g, a):
    """a copy whose cells beyond the first halo cell hold NaN: the kernels may not read them"""
    p = np.full(a.shape, np.nan)
    keep = (slice(g.Hx - 1, g.Hx + g.Nx + 1), slice(g.Hy - 1, g.Hy + g.Ny + 1), slice(g.Hz - 1, g.Hz + g.Nz + 1))
    p[keep] = a[keep]
    return p


_cases = {}


def _case(ocn, name, key):
    """the grid, the inputs on the host and (poisoned) on the device, the closure struct: built once per case and buoyancy"""
    if (name, key) not in _cases:
        pg = ocn.RectilinearGrid(ocn.GPU(), **ISN.case_grid_arguments(name))
        g, buoyancy = IDN.describe(pg), BUOYANCIES[key]
        T, S, c = ISN.case_inputs(g, buoyancy)
        dT = to_dev(ocn, pg, CC, _poisoned(g, T))
        dS = to_dev(ocn, pg, CC, _poisoned(g, S)) if S is not None else None
        dc = to_dev(ocn, pg, CC, _poisoned(g, c))
        cl = ISN.closure()
        _cases[(name, key)] = dict(pg=pg, g=g, buoyancy=buoyancy, T=T, S=S, c=c, dT=dT, dS=dS, dc=dc, cl=cl,
                                   struct=ocn._lib.CIsopycnal(cl.max_slope, cl.minimum_bz), terms=_terms(ocn, buoyancy, dT, dS))
    return _cases[(name, key)]


def _random_parents(g, seed):
    rng = np.random.default_rng(seed)
    return {n: rng.uniform(-1, 1, ISN.parent_shape(g, n in ("eps_R33", "w", "kz0", "kz1"))) for n in ("eps_R33", "u", "v", "w", "kz0", "kz1")}


def _compute_diffusivities(ocn, k, before, kappa_skew, ks):
    """the launch and the halo fill of update_state!; returns the device fields"""
    L, pg = ocn._lib, k["pg"]
    d = {n: to_dev(ocn, pg, {"u": U, "v": V}.get(n, CCF), before[n]) for n in before}
    eddy = [d[n].ptr for n in "uvw"] if kappa_skew is not None else [None] * 3
    L.call("ocn_compute_isopycnal_diffusivities", pg.cref, C.byref(k["terms"]), C.byref(k["struct"]), kappa_skew or 0.0, d["eps_R33"].ptr, *eddy,
           len(ks), (C.c_double * len(ks))(*ks) if ks else None, L.ptr_array([d[f"kz{q}"].ptr for q in range(len(ks))]) if ks else None, 0)
    filled = ("eps_R33", "u", "v", "w") if kappa_skew is not None else ("eps_R33",)
    ocn.fill_halo_regions(tuple(d[n] for n in filled), fill_boundary_normal_velocities=False)
    ocn.sync_device()
    return d


# ---- 1. compute_diffusivities! ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(BUOYANCIES))
@pytest.mark.parametrize("name", list(ISN.CASES))
def test_diffusivity_fields_and_total_velocities_equal_the_restatement_bit_for_bit(ocn, name, key):
    """ϵ_R₃₃, uₑ, vₑ, wₑ after the halo fill and two κz arrays on whole parents that held random numbers before (face Nz + 1 of ϵ_R₃₃ and of
    the κz arrays, the z halos of ϵ_R₃₃ and wₑ and the deeper z halos of uₑ, vₑ keep them), then u + uₑ, v + vₑ, w + wₑ over the whole
    parents.  The device reads T, S (or b) whose cells beyond the first halo cell are NaN."""
    k = _case(ocn, name, key)
    g, pg, L = k["g"], k["pg"], ocn._lib
    before = _random_parents(g, 17)
    d = _compute_diffusivities(ocn, k, before, 1000.0, KS[:2])
    want = ISN.diffusivity_parents(g, k["buoyancy"], k["T"], k["S"], k["cl"], 1000.0, before)
    for n in ("eps_R33", "u", "v", "w"):
        got = from_dev(d[n])
        assert np.isfinite(got).all(), n
        assert np.array_equal(got, want[n]), f"{n}: max difference {np.abs(got - want[n]).max():.3e}"
        assert np.abs(want[n][ISN.interior(g)]).max() > 0
    for q in range(2):  # κz over faces 1..Nz; everything else untouched
        assert np.array_equal(from_dev(d[f"kz{q}"]), ISN.kz(g, want["eps_R33"], KS[q], before[f"kz{q}"]))
    assert np.all(want["w"][g.Hx:g.Hx + g.Nx, g.Hy:g.Hy + g.Ny, [g.Hz, g.Hz + g.Nz]] == 0)
    # the total velocities
    rng = np.random.default_rng(23)
    vel = {n: rng.uniform(-1, 1, want[n].shape) for n in "uvw"}
    dv = {n: to_dev(ocn, pg, loc, vel[n]) for n, loc in zip("uvw", (U, V, CCF))}
    total = {n: to_dev(ocn, pg, loc, np.full(vel[n].shape, np.nan)) for n, loc in zip("uvw", (U, V, CCF))}
    pa = L.ptr_array
    L.call("ocn_sum_velocities", pg.cref, pa([dv[n].ptr for n in "uvw"]), pa([d[n].ptr for n in "uvw"]), pa([total[n].ptr for n in "uvw"]), 0)
    ocn.sync_device()
    for n in "uvw":
        assert np.array_equal(from_dev(total[n]), vel[n] + want[n]), n
    # without eddy velocities (κ_skew = nothing) and without κz arrays (κ_symmetric = nothing): ϵ_R₃₃ alone, the same bits
    alone = _compute_diffusivities(ocn, k, before, None, ())
    assert np.array_equal(from_dev(alone["eps_R33"]), want["eps_R33"])
    for n in ("u", "v", "w", "kz0", "kz1"):
        assert np.array_equal(from_dev(alone[n]), before[n]), n
    for n, f in (("T", k["dT"]), ("c", k["dc"])):  # the inputs are read only
        assert np.array_equal(from_dev(f), _poisoned(g, k[n]), equal_nan=True)


# ---- 2. the flux divergence ---------------------------------------------------------------------------------------------------------------------
def _add_fluxes(ocn, k, tracers, Gs, ks, kw):
    L, n = ocn._lib, len(tracers)
    L.call("ocn_add_isopycnal_fluxes", k["pg"].cref, C.byref(k["terms"]), C.byref(k["struct"]), n, (C.c_double * n)(*ks[:n]), (C.c_double * n)(*kw[:n]),
           L.ptr_array([c.ptr for c in tracers]), L.ptr_array([G.ptr for G in Gs]), 0)
    ocn.sync_device()


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("key", list(BUOYANCIES))
@pytest.mark.parametrize("name", list(ISN.CASES))
def test_tendencies_after_the_flux_divergence_equal_the_restatement_bit_for_bit(ocn, name, key, variant):
    """G - ∇·q of every tracer -- T, S and a passive c (three tracers: a launch of two and a launch of one), or b and c -- from random G, whole
    parents compared: nothing outside the interior is written.  Variants: the skew coefficient 0 inside the fluxes (AdvectiveFormulation,
    or κ_skew = nothing), the DiffusiveFormulation, κ_symmetric = nothing with it, and coefficients per tracer."""
    k = _case(ocn, name, key)
    g, pg = k["g"], k["pg"]
    ks, kw = VARIANTS[variant]
    host = [k["T"], k["S"], k["c"]] if k["S"] is not None else [k["T"], k["c"]]
    dev = [k["dT"], k["dS"], k["dc"]] if k["S"] is not None else [k["dT"], k["dc"]]
    rng = np.random.default_rng(31)
    scale = max(np.abs(ISN.tracer_term(g, k["buoyancy"], k["T"], k["S"], k["cl"], ks[n], kw[n], c)).max() for n, c in enumerate(host))
    G = [scale * rng.uniform(-1, 1, c.shape) for c in host]  # (of the size of the term: the subtraction rounds)
    dG = [to_dev(ocn, pg, CC, a) for a in G]
    _add_fluxes(ocn, k, dev, dG, ks, kw)
    for n, c in enumerate(host):
        term = ISN.tracer_term(g, k["buoyancy"], k["T"], k["S"], k["cl"], ks[n], kw[n], c)
        got, want = from_dev(dG[n]), ISN.subtract(g, G[n], term)
        assert np.isfinite(got).all() and np.abs(term).max() > 0
        assert np.array_equal(got, want), f"tracer {n}: max difference {np.abs(got - want).max():.3e} of {np.abs(term).max():.3e}"
        assert not np.array_equal(want, G[n])
    # into zeroed arrays the call leaves 0 - ∇·q: what the pair with the biharmonic closure hands on
    zero = [ocn.Field(CC, pg) for _ in host]
    _add_fluxes(ocn, k, dev, zero, ks, kw)
    for n, c in enumerate(host):
        term = ISN.tracer_term(g, k["buoyancy"], k["T"], k["S"], k["cl"], ks[n], kw[n], c)
        assert np.array_equal(from_dev(zero[n]), ISN.subtract(g, np.zeros_like(c), term))


def test_the_march_crosses_chunks_of_planes(ocn):
    """Nz = 20: a chunk of 16 planes and one of 4; the z flux between planes 16 and 17 is computed by both workgroups"""
    pg = ocn.RectilinearGrid(ocn.GPU(), size=(5, 4, 20), x=(0, 5e4), y=(0, 4e4), z=(-200, 0), topology=("Periodic", "Periodic", "Bounded"), halo=(2, 2, 2))
    g, cl = IDN.describe(pg), ISN.closure()
    b, c = ISN.shared_input(g, ISN.SEED)
    db, dc = to_dev(ocn, pg, CC, b), to_dev(ocn, pg, CC, c)
    k = dict(pg=pg, terms=_terms(ocn, ISN.TRACER, db, None), struct=ocn._lib.CIsopycnal(cl.max_slope, cl.minimum_bz))
    rng = np.random.default_rng(5)
    terms = [ISN.tracer_term(g, ISN.TRACER, b, None, cl, 900.0, 400.0, f) for f in (b, c)]
    G = [np.abs(t).max() * rng.uniform(-1, 1, b.shape) for t in terms]
    dG = [to_dev(ocn, pg, CC, a) for a in G]
    _add_fluxes(ocn, k, [db, dc], dG, (900.0,) * 2, (400.0,) * 2)
    for n in range(2):
        assert np.array_equal(from_dev(dG[n]), ISN.subtract(g, G[n], terms[n])), n


# ---- 3. the implicit step -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["reference_333", "one_interior_face", "tile_plus_partial"])
def test_implicit_step_with_kz_equals_the_thomas_solve(ocn, name):
    """implicit_step! of two tracers with their own κz = ϵ_R₃₃ κ_symmetric arrays (computed on the device) against the NumPy elimination in the
    arithmetic of tests/implicit_diffusion_numpy.py.  Δt κz / Δz² reaches 0.4."""
    k = _case(ocn, name, "b")
    g, pg, L = k["g"], k["pg"], ocn._lib
    d = _compute_diffusivities(ocn, k, {n: np.zeros_like(a) for n, a in _random_parents(g, 1).items()}, None, KS[:2])
    kz = [from_dev(d["kz0"]), from_dev(d["kz1"])]
    dt = 0.4 * float(np.min(g.dzc)) ** 2 / max(kz[0].max(), 1e-300)
    fields = [to_dev(ocn, pg, CC, k["T"]), to_dev(ocn, pg, CC, k["c"])]
    import torch
    scratch = torch.zeros((2, g.Nz, g.Ny, g.Nx), dtype=torch.float64, device=fields[0].data.device)
    L.call("ocn_implicit_vertical_diffusion_step_fields", pg.cref, 2, L.ptr_array([f.ptr for f in fields]), L.i32_array([CC, CC]),
           L.ptr_array([d["kz0"].ptr, d["kz1"].ptr]), L.ptr_array([scratch[0].data_ptr(), scratch[1].data_ptr()]), float(dt), 0)
    ocn.sync_device()
    for f, a, kap in zip(fields, (k["T"], k["c"]), kz):
        want = ISN.implicit_step(g, a, kap, dt)
        assert kap.max() > 0 and not np.array_equal(want, a)
        assert np.array_equal(from_dev(f), want), f"max difference {np.abs(from_dev(f) - want).max():.3e}"


# ---- 4. the model -----------------------------------------------------------------------------------------------------------------------------
DT = 60.0  # sqrt(g Lz) Δt / Δx = 20 x 60 / 1e4 = 0.12; κ Δt / Δx² = 5e-4; the vertical part is implicit


class ByHand:
    """the closure object of a twin model, composed from the entry points tested above and from nothing of hydrostatic_closures.py's
    IsopycnalFields: ϵ_R₃₃, κz and the eddy velocities in update_state!, their halo fill, the total velocities, the flux divergence after
    the tracer tendencies -- into a zeroed array first when a biharmonic closure takes the sum --, the implicit step of the tracers"""
    container_closure, unfused, state_fields, self_stepped = None, True, (), ()

    def __init__(self, ocn, model, kappa_skew, kappa_symmetric, bih=None):
        g = model.grid
        self.ocn, self.bih, self.kappa_skew, self.ks = ocn, bih, kappa_skew, [kappa_symmetric[n] for n in model.tracer_names]
        self.struct = ocn._lib.CIsopycnal(1e-2, 0.0)
        self.eps, self.eddy, self.total = ocn.Field(CCF, g), [ocn.Field(loc, g) for loc in (U, V, CCF)], [ocn.Field(loc, g) for loc in (U, V, CCF)]
        self.kz = [ocn.Field(CCF, g) for _ in self.ks]
        import torch
        self.scratch = torch.zeros((len(self.ks) + 1,) + tuple(model.u.data.shape), dtype=torch.float64, device=model.u.data.device)

    def boundary_conditions(self, user_bcs, grid):
        return user_bcs

    def checkpoint_state(self, nh):
        return {}

    def tracer_kappa(self, name):
        return 0.0

    def compute_diffusivities(self, nh):
        L, pa, g = self.ocn._lib, self.ocn._lib.ptr_array, nh.grid
        nh._refresh_term_pointers()
        n = len(self.ks)
        L.call("ocn_compute_isopycnal_diffusivities", g.cref, C.byref(nh._terms), C.byref(self.struct), self.kappa_skew, self.eps.ptr,
               *[f.ptr for f in self.eddy], n, (C.c_double * n)(*self.ks), pa([f.ptr for f in self.kz]), 0)
        self.ocn.fill_halo_regions((self.eps,) + tuple(self.eddy), fill_boundary_normal_velocities=False)
        L.call("ocn_sum_velocities", g.cref, pa([nh.u.ptr, nh.v.ptr, nh.w.ptr]), pa([f.ptr for f in self.eddy]), pa([f.ptr for f in self.total]), 0)

    def advecting_velocities(self, nh):
        return tuple(f.ptr for f in self.total)

    def add_fluxes(self, nh, Gn, s):
        L, pa, g, n = self.ocn._lib, self.ocn._lib.ptr_array, nh.grid, len(self.ks)
        cs, Gs = [c.ptr for c in nh.tracers], [G.ptr for G in Gn[3:]]
        args = (C.byref(nh._terms), C.byref(self.struct), n, (C.c_double * n)(*self.ks), (C.c_double * n)(*[0.0] * n), pa(cs))
        if self.bih is None:
            return L.call("ocn_add_isopycnal_fluxes", g.cref, *args, pa(Gs), s)
        S = self.scratch[:n]
        S.zero_()
        Ss = [S[q].data_ptr() for q in range(n)]
        L.call("ocn_add_isopycnal_fluxes", g.cref, *args, pa(Ss), s)
        L.call("ocn_add_biharmonic_fluxes", g.cref, self.bih.nu, nh.u.ptr, nh.v.ptr, Gn[0].ptr, Gn[1].ptr, n,
               (C.c_double * n)(*[self.bih.kappa_of(t) for t in nh.tracer_names]), pa(cs), pa(Gs), None, None, pa(Ss), s)

    def implicit_step(self, nh, fields, dt, s):
        L, pa, tracers, g = self.ocn._lib, self.ocn._lib.ptr_array, fields[2:], nh.grid
        w = self.scratch.view(-1)  # (the multipliers: Nx Ny Nz doubles per tracer)
        size = g.Nx * g.Ny * g.Nz
        L.call("ocn_implicit_vertical_diffusion_step_fields", g.cref, len(tracers), pa([f.ptr for f in tracers]), L.i32_array([CC] * len(tracers)),
               pa([f.ptr for f in self.kz]), pa([w[q * size:].data_ptr() for q in range(len(tracers))]), float(dt), s)


def _model(ocn, name, closure, free_surface, tracer_advection, halo=None):
    args = ISN.case_grid_arguments(name)
    if halo is not None:
        args["halo"] = halo
    fs = {"explicit": lambda: ocn.ExplicitFreeSurface(), "split": lambda: ocn.SplitExplicitFreeSurface(substeps=10)}[free_surface]()
    return ocn.HydrostaticFreeSurfaceModel(ocn.RectilinearGrid(ocn.GPU(), **args), closure=closure, tracers=("b", "c"), buoyancy=ocn.BuoyancyTracer(),
                                           coriolis=ocn.FPlane(f=1e-4), free_surface=fs, math_mode=ocn.MATH_STRICT, fused=False if closure is None else None,
                                           tracer_advection=ocn.WENO() if tracer_advection == "WENO" else None)


def _initial(m):
    g = IDN.describe(m.grid)
    b, c = ISN.shared_input(g, ISN.SEED)
    sl = ISN.interior(g)
    rng = np.random.default_rng(2)
    return dict(b=b[sl], c=c[sl], u=0.01 * rng.uniform(-1, 1, b[sl].shape), v=0.01 * rng.uniform(-1, 1, b[sl].shape))


KAPPA_SKEW, KAPPA_SYMMETRIC = 500.0, {"b": 900.0, "c": 250.0}


def _pair(ocn, name, free_surface, tracer_advection, order=None):
    """the model with the closure (alone, or in a pair with the biharmonic closure in the given order) and its twin by hand, both set"""
    issd = ocn.IsopycnalSkewSymmetricDiffusivity(κ_skew=KAPPA_SKEW, κ_symmetric=KAPPA_SYMMETRIC)
    bih = ocn.HorizontalScalarBiharmonicDiffusivity(ν=1e9, κ={"b": 2e9, "c": 5e8}) if order is not None else None
    closure = issd if bih is None else ((bih, issd), (issd, bih))[order]
    m = _model(ocn, name, closure, free_surface, tracer_advection)
    assert m.fused is False and m._nh._terms.closure == 0
    assert set(m.diffusivity_fields) == {"eps_R33", "u", "v", "w"}
    r = _model(ocn, name, bih, free_surface, tracer_advection, halo=(m.grid.Hx, m.grid.Hy, m.grid.Hz))
    r._closure = ByHand(ocn, r, KAPPA_SKEW, KAPPA_SYMMETRIC, bih)
    init = _initial(m)
    m.set(**init)
    r.set(**init)
    return m, r


def _assert_same_state(ocn, m, r):
    ocn.sync_device()
    for n in ("u", "v", "w", "b", "c"):
        a, b = m.field(n).parent(), r.field(n).parent()
        assert np.isfinite(a).all(), n
        assert np.array_equal(a, b), f"{n}: max difference {np.abs(a - b).max():.3e}"
    assert np.array_equal(m.eta.cpu().numpy(), r.eta.cpu().numpy())
    for Gm_, Gr_ in zip(m._nh.timestepper._Gn, r._nh.timestepper._Gn):
        assert np.array_equal(Gm_.parent(), Gr_.parent())
    h = r._closure
    for n, f in zip(("eps_R33", "u", "v", "w"), [h.eps] + h.eddy):
        assert np.array_equal(m.diffusivity_fields[n].parent(), f.parent()), n
        assert np.abs(f.parent()).max() > 0, n


@pytest.mark.parametrize("free_surface", ["explicit", "split"])
def test_model_steps_equal_the_sequence_composed_by_hand(ocn, free_surface):
    """two QAB2 steps (an Euler step and an Adams-Bashforth one) on 37 x 11 x 4 with a stretched z, WENO() tracers, b and a passive c with
    their own κ_symmetric: u, v, w, η, the tracers, the tendencies and the diffusivity fields bit for bit"""
    m, r = _pair(ocn, "tile_plus_partial", free_surface, "WENO")
    for _ in range(2):
        m.time_step(DT)
        r.time_step(DT)
    _assert_same_state(ocn, m, r)
    assert not np.array_equal(m.field("c").interior(), _initial(m)["c"])


def test_model_with_the_minimal_halo_and_centered_tracers(ocn):
    """3 x 3 x 3 with halo (1, 1, 1): VectorInvariant() momentum and Centered() tracers need no more, nor does the closure"""
    m, r = _pair(ocn, "minimal_halo", "explicit", None)
    assert (m.grid.Hx, m.grid.Hy, m.grid.Hz) == (1, 1, 1)
    for _ in range(2):
        m.time_step(DT)
        r.time_step(DT)
    _assert_same_state(ocn, m, r)


@pytest.mark.parametrize("order", [0, 1], ids=["biharmonic_first", "biharmonic_last"])
def test_pair_with_the_biharmonic_closure_equals_the_sequence_composed_by_hand(ocn, order):
    """(HorizontalScalarBiharmonicDiffusivity, IsopycnalSkewSymmetricDiffusivity) in either order: the sum of the two terms is formed before
    it is subtracted (0 - ∇·q in a zeroed array, then G - (a + (0 - S))); momentum gets the biharmonic term alone"""
    m, r = _pair(ocn, "tile_plus_partial", "split", "WENO", order)
    assert m._closure.halo == 2 and m._closure.implicit
    for _ in range(2):
        m.time_step(DT)
        r.time_step(DT)
    _assert_same_state(ocn, m, r)


def test_tracer_tendency_is_the_restatement_and_momentum_tendencies_are_those_without_the_closure(ocn):
    """after set!: Gu, Gv are the bits of the same model with closure = nothing (the closure has no viscosity and the eddy velocities do not
    advect momentum); Gc is the tracer entry point run with u + uₑ, v + vₑ, w + wₑ of the restatement minus the restatement's ∇·q"""
    m = _model(ocn, "tile_plus_partial", ocn.IsopycnalSkewSymmetricDiffusivity(κ_skew=KAPPA_SKEW, κ_symmetric=KAPPA_SYMMETRIC), "explicit", "WENO")
    r = _model(ocn, "tile_plus_partial", None, "explicit", "WENO")
    init = _initial(m)
    for model in (m, r):
        model.set(**init)
        model.compute_tendencies()
    ocn.sync_device()
    Gm_, Gr_ = m._nh.timestepper._Gn, r._nh.timestepper._Gn
    for q in (0, 1):
        assert np.array_equal(Gm_[q].parent(), Gr_[q].parent()) and np.abs(Gm_[q].parent()).max() > 0
    g, cl, L = IDN.describe(m.grid), ISN.closure(), ocn._lib
    b, c = m.field("b").parent(), m.field("c").parent()
    zeros = {n: np.zeros(ISN.parent_shape(g, n in ("eps_R33", "w"))) for n in ("eps_R33", "u", "v", "w")}
    d = ISN.diffusivity_parents(g, ISN.TRACER, b, None, cl, KAPPA_SKEW, zeros)
    total = [to_dev(ocn, m.grid, loc, f.parent() + d[n]) for n, loc, f in zip("uvw", (U, V, CCF), (m.u, m.v, m.w))]
    for q, (name, f) in enumerate((("b", b), ("c", c))):
        G = ocn.Field(CC, m.grid)
        L.call("ocn_compute_tracer_tendency_terms", m.grid.cref, C.byref(m._nh._terms), 0.0, None, total[0].ptr, total[1].ptr, total[2].ptr,
               m.field(name).ptr, G.ptr, None, 0)
        ocn.sync_device()
        want = ISN.subtract(g, G.parent(), ISN.tracer_term(g, ISN.TRACER, b, None, cl, KAPPA_SYMMETRIC[name], 0.0, f))
        assert np.array_equal(Gm_[3 + q].parent(), want), name
        assert not np.array_equal(Gm_[3 + q].parent(), Gr_[3 + q].parent())


def test_a_passive_tracer_is_conserved(ocn):
    """default (no-flux) conditions: Σ c V over ten steps drifts by no more than N_cells eps max|c V| per step (every cell's update rounds
    once at the size of its content; the fluxes through the bottom and the top vanish because ∂z b of the filled halos does, and wₑ is 0
    there).  The model's linear free surface lets w c through the top face, which is not the closure's business: the fluid starts at rest
    and b is the shared input times 2^-40, which leaves every slope, ϵ, R and eddy velocity as it is (they are ratios of gradients of b; the
    factor is exact) and the resolved flow and its surface flux forty binary orders below the tolerance."""
    m = _model(ocn, "tile_plus_partial", ocn.IsopycnalSkewSymmetricDiffusivity(κ_skew=KAPPA_SKEW, κ_symmetric=KAPPA_SYMMETRIC), "split", "WENO")
    init = _initial(m)
    m.set(b=init["b"] * 2.0 ** -40, c=init["c"])
    assert np.abs(m.diffusivity_fields["u"].interior()).max() > 1e-4 and m.diffusivity_fields["eps_R33"].interior().max() > 1e-6
    g = IDN.describe(m.grid)
    V_ = (g.dx * g.dy) * IDN._dzC(g, 0) + np.zeros((g.Nx, g.Ny, g.Nz))
    content = lambda: float(np.sum(m.field("c").interior() * V_))
    start, steps = content(), 10
    tolerance = g.Nx * g.Ny * g.Nz * EPS * np.abs(m.field("c").interior() * V_).max()
    previous = start
    for step in range(steps):
        m.time_step(DT)
        now = content()
        print(f"step {step + 1}: drift {now - previous:.3e}, tolerance {tolerance:.3e}")
        assert abs(now - previous) <= tolerance
        previous = now
    assert np.isfinite(m.field("c").interior()).all() and not np.array_equal(m.field("c").interior(), _initial(m)["c"])
