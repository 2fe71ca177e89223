"""HydrostaticFreeSurfaceModel on channels (Periodic, Bounded, Bounded) and closed basins (Bounded, Bounded, Bounded) on the GPU
(csrc/hydrostatic_surface.hip) against the CPU restatement tests/hydrostatic_walls_numpy.py.  Strict math unless said otherwise: the
explicit and split-explicit models and every entry point bit for bit, the implicit model to the project's bounds for "the same arithmetic
with a different transform".  The entry points run on (Periodic, Periodic, Bounded) as well: the same kernels without a wall, where the
restatement is the oracle's own arithmetic (test_host_hydrostatic_walls.py)."""
import ctypes as C

import numpy as np
import pytest

import hydrostatic_walls_numpy as HW
from helpers import from_dev, make_pair, stretched_faces, to_dev

pytestmark = pytest.mark.gpu

TOPOS = ["PBB", "BBB"]
ENTRY_TOPOS = ["PPB"] + TOPOS   # the entry-point tests (the `case` fixture); the periodic models are in test_gpu_hydrostatic.py
# (16, 12, 7): the shape of the periodic tests; (67, 6, 3) with halo (4, 5, 3): across the 64-lane block edge in x, a partial block in y,
# unequal halos
SHAPES = [((16, 12, 7), (3, 3, 3)), ((67, 6, 3), (4, 5, 3))]
GRAV = 9.80665
UNWRITTEN = 777.0   # what outputs hold before a launch: a cell the kernel should not write still holds it afterwards


def _pair(O, ocn, topo, size, halo, stretched):
    z = stretched_faces(size[2], 40.0) if stretched else (-40.0, 0.0)
    return make_pair(O, ocn, size, topo, x=(0, 2.0e3), y=(0, 1.5e3), z=z, halo=halo)


class Case:
    """one grid on both sides, with the arrays of an entry-point test: NaN everywhere but a box (the kernel's documented reach)"""

    def __init__(self, O, ocn, topo, size, halo, stretched, seed=5):
        self.O, self.ocn = O, ocn
        self.og, self.pg = _pair(O, ocn, topo, size, halo, stretched)
        self.rng = np.random.default_rng(seed)
        g = self.og
        self.H, self.N = (g.Hx, g.Hy, g.Hz), (g.Nx, g.Ny, g.Nz)
        self.bx, self.by = int(g.tx == 1), int(g.ty == 1)

    def box(self, loc, lo=(0, 0, 0), hi=(0, 0, 0), faces=False, fill=np.nan, scale=1.0):
        """parent array of a field at `loc`: random over interior indices 1 - lo .. N + hi (+ the N + 1 wall faces if `faces`), `fill` elsewhere"""
        a = np.full(self.og.shape(loc), fill, order="F")
        ext = [(1 if faces and ((loc >> d) & 1) and self.og.topo[d] == 1 else 0) for d in range(3)]
        if loc == 4:
            ext[2] = 1  # w: faces 1 .. Nz + 1
        sl = tuple(slice(self.H[d] - lo[d], self.H[d] + self.N[d] + hi[d] + ext[d]) for d in range(3))
        a[sl] = scale * self.rng.uniform(-1, 1, a[sl].shape)
        return a

    def plane(self, loc=0, lo=(0, 0), hi=(0, 0), faces=False, fill=np.nan):
        """a 2-D plane [i, j] with the x / y extents of a field at `loc`"""
        shp = self.og.shape(loc)[:2]
        a = np.full(shp, fill, order="F")
        ext = [(1 if faces and ((loc >> d) & 1) and self.og.topo[d] == 1 else 0) for d in range(2)]
        sl = tuple(slice(self.H[d] - lo[d], self.H[d] + self.N[d] + hi[d] + ext[d]) for d in range(2))
        a[sl] = self.rng.uniform(-1, 1, a[sl].shape)
        return a

    def dev(self, loc, a):
        return to_dev(self.ocn, self.pg, loc, a)

    def dplane(self, a):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a.T)).to("cuda")

    def call(self, name, *args):
        self.ocn._lib.call(name, self.pg.cref, *args)
        self.ocn.sync_device()

    @property
    def interior2(self):
        return slice(self.H[0], self.H[0] + self.N[0]), slice(self.H[1], self.H[1] + self.N[1])


def _host(t):
    return t.cpu().numpy().T


CASES = [(t, s, h, st) for t in ENTRY_TOPOS for (s, h) in SHAPES for st in (False, True)]
IDS = [f"{t}-{'x'.join(map(str, s))}-{'stretched' if st else 'uniform'}" for t, s, h, st in CASES]


@pytest.fixture(params=CASES, ids=IDS)
def case(request, oracle, ocn):
    ocn.set_math_mode(ocn.MATH_STRICT)
    return Case(oracle, ocn, *request.param)


# ---- 5. the entry points on whole parents ---------------------------------------------------------------------------------------------
def test_w_from_continuity(case):
    """reach: u, v of the columns i = 1 - Hx .. Nx + Hx (j likewise) at the levels 1 .. Nz; the extra face column / row of a wall direction
    beyond Nx + Hx and the z halos hold NaN"""
    c = case
    u = c.box(1, lo=(c.H[0], c.H[1], 0), hi=(c.H[0], c.H[1], 0))
    v = c.box(2, lo=(c.H[0], c.H[1], 0), hi=(c.H[0], c.H[1], 0))
    w = np.full(c.og.shape(4), UNWRITTEN, order="F")
    du, dv, dw = c.dev(1, u), c.dev(2, v), c.dev(4, w)
    HW.compute_w_from_continuity(c.og, u, v, w)
    c.call("ocn_compute_w_from_continuity", du.ptr, dv.ptr, dw.ptr, 0)
    np.testing.assert_array_equal(from_dev(dw), w)
    assert np.isfinite(c.og.interior(w)).all() and (w == UNWRITTEN).any()


def test_free_surface_halo_fill(case):
    c = case
    e = c.plane()
    de = c.dplane(e)
    HW.fill_eta(c.og, e)
    c.call("ocn_fill_free_surface_halos", de.data_ptr(), 0)
    np.testing.assert_array_equal(_host(de), e)
    ii, jj = c.interior2
    assert np.isfinite(e[ii, c.H[1] - 1]).all() and np.isfinite(e[ii, c.H[1] + c.N[1]]).all()
    if not c.by:
        assert np.isfinite(e).all()   # the periodic fill writes every halo cell, corners included
    else:
        assert np.isnan(e[ii, c.H[1] - 2]).all()   # no-flux fills the first halo cell only
    if c.bx:
        assert np.isnan(e[c.H[0] - 1, c.H[1] - 1])   # corner of a basin: not written


def test_barotropic_pressure_gradient_and_correction(case):
    """reach of η: the interior and the first halo cell to the west / south"""
    c = case
    e = c.plane(lo=(1, 1))
    for entry, dt in (("ocn_add_barotropic_pressure_gradient", None), ("ocn_barotropic_pressure_correction", 30.0)):
        a, b = c.box(1, faces=True, fill=UNWRITTEN), c.box(2, faces=True, fill=UNWRITTEN)
        da, db, de = c.dev(1, a), c.dev(2, b), c.dplane(e)
        if dt is None:
            HW.add_barotropic_pressure_gradient(c.og, GRAV, e, a, b)
            c.call(entry, GRAV, de.data_ptr(), da.ptr, db.ptr, 0)
        else:
            HW.barotropic_pressure_correction(c.og, a, b, e, GRAV, dt)
            c.call(entry, da.ptr, db.ptr, de.data_ptr(), GRAV, dt, 0)
        np.testing.assert_array_equal(from_dev(da), a, err_msg=entry)
        np.testing.assert_array_equal(from_dev(db), b, err_msg=entry)
        assert np.isfinite(a).all()


@pytest.mark.parametrize("with_eta", [False, True])
def test_vector_invariant_tendencies(case, with_eta):
    """reach: one cell around the interior in every direction (the wall faces N + 1 included), w at the faces 1 .. Nz + 1"""
    from oracle import hydrostatic as Hy
    c = case
    one = (1, 1, 1)
    u, v = c.box(1, lo=one, hi=one, faces=True), c.box(2, lo=one, hi=one, faces=True)
    w = c.box(4, lo=(1, 1, 0), hi=(0, 0, 0))
    e = c.plane(lo=(1, 1))
    Gu, Gv = np.full(c.og.shape(1), UNWRITTEN, order="F"), np.full(c.og.shape(2), UNWRITTEN, order="F")
    du, dv, dw, dGu, dGv, de = c.dev(1, u), c.dev(2, v), c.dev(4, w), c.dev(1, Gu), c.dev(2, Gv), c.dplane(e)
    Hy.vector_invariant_momentum_tendencies(c.og, u, v, w, Gu, Gv)
    if with_eta:
        HW.add_barotropic_pressure_gradient(c.og, GRAV, e, Gu, Gv)
    c.call("ocn_compute_vector_invariant_momentum_tendencies", du.ptr, dv.ptr, dw.ptr, dGu.ptr, dGv.ptr, de.data_ptr() if with_eta else None,
           GRAV, 0)
    np.testing.assert_array_equal(from_dev(dGu), Gu)
    np.testing.assert_array_equal(from_dev(dGv), Gv)
    assert np.isfinite(c.og.interior_N(Gu)).all() and np.isfinite(c.og.interior_N(Gv)).all()


def _embed(c, loc, interior, fill):
    a = np.full(c.og.shape(loc)[:2], fill, order="F")
    a[c.interior2] = interior
    return a


@pytest.mark.parametrize("chi", [0.1, -0.5])
def test_barotropic_mode_and_forcing(case, chi):
    c = case
    u, v = c.box(1), c.box(2)
    U, V = (np.full(c.og.shape(l)[:2], UNWRITTEN, order="F") for l in (1, 2))
    du, dv, dU, dV = c.dev(1, u), c.dev(2, v), c.dplane(U), c.dplane(V)
    c.call("ocn_compute_barotropic_mode", du.ptr, dv.ptr, dU.data_ptr(), dV.data_ptr(), 0)
    np.testing.assert_array_equal(_host(dU), _embed(c, 1, HW.barotropic_mode(c.og, u), UNWRITTEN))
    np.testing.assert_array_equal(_host(dV), _embed(c, 2, HW.barotropic_mode(c.og, v), UNWRITTEN))
    um, vm = c.box(1), c.box(2)
    dum, dvm, dU, dV = c.dev(1, um), c.dev(2, vm), c.dplane(U), c.dplane(V)
    c.call("ocn_split_explicit_forcing", du.ptr, dum.ptr, dv.ptr, dvm.ptr, chi, dU.data_ptr(), dV.data_ptr(), 0)
    np.testing.assert_array_equal(_host(dU), _embed(c, 1, HW.split_explicit_forcing(c.og, u, um, chi), UNWRITTEN))
    np.testing.assert_array_equal(_host(dV), _embed(c, 2, HW.split_explicit_forcing(c.og, v, vm, chi), UNWRITTEN))


@pytest.mark.parametrize("n", [1, 5])
def test_split_explicit_substeps(case, n):
    """reach: the interiors 1:Nx, 1:Ny of every plane -- the halos, the N + 1 wall faces and the corners hold NaN.  The filtered planes are
    zeroed whole and the state is copied from them whole, as in the periodic launch."""
    c = case
    g = c.og
    e, U, V, GU, GV = c.plane(), c.plane(1), c.plane(2), c.plane(1), c.plane(2)
    dtau = 0.5 * min(g.dx, g.dy) / np.sqrt(GRAV * g.Lz)
    weights = c.rng.uniform(0.1, 1.0, n)
    weights /= weights.sum()
    dev = [c.dplane(a) for a in (e, U, V)] + [c.dplane(np.full(a.shape, UNWRITTEN, order="F")) for a in (e, U, V)] + [c.dplane(GU), c.dplane(GV)]
    ii, jj = c.interior2
    ei, Ui, Vi = e[ii, jj].copy(), U[ii, jj].copy(), V[ii, jj].copy()
    eb, Ub, Vb = (np.zeros((g.Nx, g.Ny)) for _ in range(3))
    HW.iterate_split_explicit(ei, Ui, Vi, eb, Ub, Vb, GU[ii, jj], GV[ii, jj], dtau, weights, GRAV, g.Lz, g.dx, g.dy, bool(c.bx), bool(c.by))
    c.call("ocn_split_explicit_substeps", n, (C.c_double * n)(*weights), float(dtau), GRAV, float(g.Lz), *[t.data_ptr() for t in dev], 0)
    for loc, state, filtered, want in ((0, dev[0], dev[3], eb), (1, dev[1], dev[4], Ub), (2, dev[2], dev[5], Vb)):
        np.testing.assert_array_equal(_host(filtered), _embed(c, loc, want, 0.0))
        np.testing.assert_array_equal(_host(state), _embed(c, loc, want, 0.0))
    assert np.isfinite(eb).all() and np.abs(Ub).max() > 0


def test_barotropic_corrector(case):
    c = case
    u, v, U, V = c.box(1), c.box(2), c.plane(1), c.plane(2)
    du, dv, dU, dV = c.dev(1, u), c.dev(2, v), c.dplane(U), c.dplane(V)
    dUb, dVb = (c.dplane(np.full(a.shape, UNWRITTEN, order="F")) for a in (U, V))
    ii, jj = c.interior2
    Ub, Vb = HW.barotropic_corrector(c.og, u, v, U[ii, jj], V[ii, jj])
    c.call("ocn_barotropic_split_explicit_corrector", du.ptr, dv.ptr, dU.data_ptr(), dV.data_ptr(), dUb.data_ptr(), dVb.data_ptr(), float(c.og.Lz), 0)
    np.testing.assert_array_equal(from_dev(du), u)
    np.testing.assert_array_equal(from_dev(dv), v)
    np.testing.assert_array_equal(_host(dUb), _embed(c, 1, Ub, UNWRITTEN))
    np.testing.assert_array_equal(_host(dVb), _embed(c, 2, Vb, UNWRITTEN))


@pytest.mark.parametrize("chi", [0.1, -0.5])
def test_explicit_free_surface_ab2_step(case, chi):
    c = case
    w = np.full(c.og.shape(4), np.nan, order="F")
    ii, jj = c.interior2
    w[ii, jj, c.H[2] + c.N[2]] = c.rng.uniform(-1, 1, c.N[:2])
    e, Gn, Gm = c.plane(), np.full(c.og.shape(0)[:2], UNWRITTEN, order="F"), c.plane()
    dw, de, dGn, dGm = c.dev(4, w), c.dplane(e), c.dplane(Gn), c.dplane(Gm)
    HW.explicit_free_surface_ab2_step(c.og, w, e, Gn, Gm, 3.0, chi)
    c.call("ocn_explicit_free_surface_ab2_step", dw.ptr, de.data_ptr(), dGn.data_ptr(), dGm.data_ptr(), 3.0, chi, 0)
    np.testing.assert_array_equal(_host(de), e)
    np.testing.assert_array_equal(_host(dGn), Gn)


def test_implicit_free_surface_rhs(case):
    """reach: the interiors of u and v with their N + 1 wall faces, the interior of η"""
    import torch
    c = case
    g = c.og
    u, v, e = c.box(1, faces=True), c.box(2, faces=True), c.plane()
    du, dv, de = c.dev(1, u), c.dev(2, v), c.dplane(e)
    dQu, dQv = (c.dplane(np.full(g.shape(l)[:2], UNWRITTEN, order="F")) for l in (1, 2))
    drhs = torch.full((g.Ny, g.Nx), UNWRITTEN, dtype=torch.float64, device="cuda")
    Qu, Qv = HW.volume_flux(g, u, v)
    ii, jj = c.interior2
    rhs = HW.implicit_rhs(g, Qu, Qv, e[ii, jj], GRAV, 25.0)
    c.call("ocn_implicit_free_surface_rhs", du.ptr, dv.ptr, de.data_ptr(), GRAV, 25.0, dQu.data_ptr(), dQv.data_ptr(), drhs.data_ptr(), 0)
    np.testing.assert_array_equal(_host(drhs), rhs)
    wantQu, wantQv = np.full(g.shape(1)[:2], UNWRITTEN, order="F"), np.full(g.shape(2)[:2], UNWRITTEN, order="F")
    wantQu[c.H[0]:c.H[0] + g.Nx + c.bx, jj] = Qu
    wantQv[ii, c.H[1]:c.H[1] + g.Ny + c.by] = Qv
    np.testing.assert_array_equal(_host(dQu), wantQu)
    np.testing.assert_array_equal(_host(dQv), wantQv)
    assert np.isfinite(rhs).all()


# ---- 6. models --------------------------------------------------------------------------------------------------------------------------
SURFACES = {"explicit": ({}, 2.0), "split": (dict(split_explicit_substeps=12), 20.0), "implicit": (dict(implicit_free_surface=True), None)}


def _models(O, ocn, topo, momentum, surface, size=(16, 12, 7), beta=None, noslip=False, seed=12):
    og, pg = _pair(O, ocn, topo, size, (3, 3, 3), stretched=True)
    bx = int(topo[0] == "B")
    rng = np.random.default_rng(seed)
    N = size
    init = dict(u=1e-2 * rng.uniform(-1, 1, (N[0] + bx, N[1], N[2])), v=1e-2 * rng.uniform(-1, 1, (N[0], N[1] + 1, N[2])),
                eta=1e-2 * rng.uniform(-1, 1, N[:2]), T=20 + 1e-2 * rng.uniform(-1, 1, N), S=35 + 1e-2 * rng.uniform(-1, 1, N))
    obc = {"u": {"top": O.FluxBoundaryCondition(-1e-4)}, "T": {"top": O.FluxBoundaryCondition(5e-5)}}
    pu = dict(top=ocn.FluxBoundaryCondition(-1e-4))
    if noslip:
        obc["u"].update(south=O.ValueBoundaryCondition(0.0), north=O.ValueBoundaryCondition(0.0))
        pu.update(south=ocn.ValueBoundaryCondition(0.0), north=ocn.ValueBoundaryCondition(0.0))
    okw, dt = SURFACES[surface]
    om = HW.HydrostaticFreeSurfaceModel(og, tracers=("T", "S"), momentum_advection=momentum, coriolis_f=1e-4, coriolis_beta=beta,
                                        closure=(1e-2, 2e-3), buoyancy=("SeawaterBuoyancy", GRAV, 2e-4, 8e-4), boundary_conditions=obc, **okw)
    om.set(**init)
    scheme = {"VectorInvariant": ocn.VectorInvariant, "WENO5": ocn.WENO, "Centered2": ocn.Centered}[momentum]()
    fs = {"explicit": ocn.ExplicitFreeSurface, "split": lambda: ocn.SplitExplicitFreeSurface(substeps=12), "implicit": ocn.ImplicitFreeSurface}[surface]()
    pm = ocn.HydrostaticFreeSurfaceModel(pg, momentum_advection=scheme, tracers=("T", "S"), free_surface=fs,
                                         coriolis=ocn.FPlane(f=1e-4) if beta is None else ocn.BetaPlane(f0=1e-4, beta=beta),
                                         closure=ocn.ScalarDiffusivity(ν=1e-2, κ=2e-3),
                                         buoyancy=ocn.SeawaterBuoyancy(equation_of_state=ocn.LinearEquationOfState(2e-4, 8e-4)),
                                         boundary_conditions={"u": ocn.FieldBoundaryConditions(**pu),
                                                              "T": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(5e-5))})
    assert not pm.fused
    pm.set(**init)
    if dt is None:
        dt = 5 * og.dx / np.sqrt(GRAV * 40.0)
    return og, om, pm, dt


def _compare(og, om, pm, tol):
    """tol = None: bit for bit; else (η, velocities, tracers) relative to each field's maximum"""
    def cmp(name, got, want, t):
        if tol is None:
            np.testing.assert_array_equal(got, want, err_msg=name)
        else:
            err = np.abs(got - want).max() / np.abs(want).max()
            print(f"{name}: {err:.3e} (bound {t:.0e})")
            assert err <= t, (name, err)
    te, tv, tc = tol or (None,) * 3
    ii, jj = slice(og.Hx, og.Hx + og.Nx), slice(og.Hy, og.Hy + og.Ny)
    cmp("eta", pm.eta_interior().cpu().numpy().T, om.eta[ii, jj], te)
    for name, a, d in zip(("u", "v", "w"), (om.u, om.v, om.w), pm.velocities):
        cmp(name, og.interior(from_dev(d)), og.interior(a), tv)
    for name, a, d in zip(om.tracer_names, om.tracers, pm.tracers):
        cmp(name, og.interior(from_dev(d)), og.interior(a), tc)


def _wall_faces_are_zero(og, pm):
    v = from_dev(pm.v)
    assert np.all(v[:, og.Hy, :] == 0.0) and np.all(v[:, og.Hy + og.Ny, :] == 0.0)
    if og.tx == 1:
        u = from_dev(pm.u)
        assert np.all(u[og.Hx, :, :] == 0.0) and np.all(u[og.Hx + og.Nx, :, :] == 0.0)


IMPLICIT_BOUNDS = (1e-12, 1e-11, 1e-13)   # test_implicit_free_surface_model_matches_oracle: η, velocities, tracers


@pytest.mark.parametrize("surface", list(SURFACES))
@pytest.mark.parametrize("momentum", ["VectorInvariant", "WENO5", "Centered2"])
@pytest.mark.parametrize("topo", TOPOS)
def test_model_steps_match_the_restatement(oracle, ocn, topo, momentum, surface):
    """three QAB2 steps (the first one Euler) with T, S, FPlane, SeawaterBuoyancy, ScalarDiffusivity and a top flux condition"""
    ocn.set_math_mode(ocn.MATH_STRICT)
    og, om, pm, dt = _models(oracle, ocn, topo, momentum, surface)
    for _ in range(3):
        om.time_step(dt)
        pm.time_step(dt)
        ocn.sync_device()
        _wall_faces_are_zero(og, pm)
    _compare(og, om, pm, IMPLICIT_BOUNDS if surface == "implicit" else None)
    assert np.abs(og.interior(om.w)).max() > 0


@pytest.mark.parametrize("topo", TOPOS)
def test_model_on_a_beta_plane(oracle, ocn, topo):
    ocn.set_math_mode(ocn.MATH_STRICT)
    og, om, pm, dt = _models(oracle, ocn, topo, "VectorInvariant", "split", beta=2e-8)
    for _ in range(3):
        om.time_step(dt)
        pm.time_step(dt)
    ocn.sync_device()
    _compare(og, om, pm, None)


@pytest.mark.parametrize("topo", TOPOS)
def test_model_with_no_slip_walls(oracle, ocn, topo):
    """u = 0 on the south and north walls (ValueBoundaryCondition(0)): the Value halo of u enters ζ and the viscous flux at the walls"""
    ocn.set_math_mode(ocn.MATH_STRICT)
    og, om, pm, dt = _models(oracle, ocn, topo, "VectorInvariant", "explicit", noslip=True)
    og2, om2, _, _ = _models(oracle, ocn, topo, "VectorInvariant", "explicit")
    for _ in range(3):
        om.time_step(dt)
        om2.time_step(dt)
        pm.time_step(dt)
    ocn.sync_device()
    _compare(og, om, pm, None)
    assert np.abs(og.interior(om.u) - og2.interior(om2.u)).max() > 0   # the condition matters


@pytest.mark.parametrize("topo", TOPOS)
def test_model_in_fast_math(oracle, ocn, topo):
    """MATH_FAST: contracted arithmetic in the tendency kernels shared with NonhydrostaticModel; the bound of the periodic fast-math
    hydrostatic tests (test_config5_combination_matches_oracle): 1e-10 of each field's maximum"""
    ocn.set_math_mode(ocn.MATH_FAST)
    try:
        og, om, pm, dt = _models(oracle, ocn, topo, "WENO5", "split")
        for _ in range(3):
            om.time_step(dt)
            pm.time_step(dt)
        ocn.sync_device()
        _compare(og, om, pm, (1e-10, 1e-10, 1e-10))
    finally:
        ocn.set_math_mode(ocn.MATH_STRICT)


# ---- 7. the reference's smoke tests -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topo", ["PPB", "PBB", "BBB"])
def test_time_step_hydrostatic_model_works(ocn, topo):
    """time_step_hydrostatic_model_works(grid) over topos_3d (test_hydrostatic_free_surface_models.jl:88-90, 198-205): defaults, one step"""
    names = tuple({"P": "Periodic", "B": "Bounded"}[t] for t in topo)
    grid = ocn.RectilinearGrid(ocn.GPU(), size=(8, 6, 4), x=(0, 1), y=(0, 1), z=(-1, 0), topology=names)
    model = ocn.HydrostaticFreeSurfaceModel(grid)
    assert isinstance(model.free_surface, ocn.ImplicitFreeSurface) and isinstance(model.momentum_advection, ocn.VectorInvariant)
    model.time_step(1.0)
    ocn.sync_device()
    assert model.clock.iteration == 1 and model.clock.time == 1.0
    assert not ocn.hasnan(model.u) and not ocn.hasnan(model.v)


@pytest.mark.parametrize("topo", TOPOS)
def test_shapes_of_the_planes(ocn, topo):
    names = tuple({"P": "Periodic", "B": "Bounded"}[t] for t in topo)
    g = ocn.RectilinearGrid(ocn.GPU(), size=(8, 6, 4), x=(0, 1), y=(0, 1), z=(-1, 0), topology=names, halo=(3, 2, 1))
    m = ocn.HydrostaticFreeSurfaceModel(g, free_surface=ocn.SplitExplicitFreeSurface(substeps=6))
    bx = int(topo[0] == "B")
    assert tuple(m.eta.shape) == (6 + 4, 8 + 6) and tuple(m.eta_interior().shape) == (6, 8)
    assert tuple(m.U.shape) == (6 + 4, 8 + 6 + bx) and tuple(m.V.shape) == (6 + 4 + 1, 8 + 6)
    assert tuple(m.U.shape) == tuple(m.u.data.shape[1:]) and tuple(m.V.shape) == tuple(m.v.data.shape[1:])
    m.set(eta=np.ones((8, 6)))
    assert float(m.eta_interior().sum()) == 48.0


def test_baroclinic_adjustment_setup_runs(ocn):
    """twenty steps of examples/baroclinic_adjustment.py at 16 x 16 x 4 (the reference's example: a (Periodic, Bounded, Bounded) channel,
    flux-form WENO, BetaPlane, BuoyancyTracer, the default ImplicitFreeSurface): finite fields, exact zeros on the wall faces"""
    ocn.set_math_mode(ocn.MATH_STRICT)
    Lx, Ly, Lz = 1.0e6, 1.0e6, 1.0e3
    grid = ocn.RectilinearGrid(ocn.GPU(), size=(16, 16, 4), x=(0, Lx), y=(-Ly / 2, Ly / 2), z=(-Lz, 0),
                               topology=("Periodic", "Bounded", "Bounded"))
    model = ocn.HydrostaticFreeSurfaceModel(grid, coriolis=ocn.BetaPlane(latitude=-45), buoyancy=ocn.BuoyancyTracer(), tracers=("b",),
                                            momentum_advection=ocn.WENO(), tracer_advection=ocn.WENO())
    rng = np.random.default_rng(1)
    N2, M2, dy_front, db = 1e-5, 1e-7, Ly / 10, Ly / 10 * 1e-7

    def ramp(y):
        return np.minimum(np.maximum(0.0, y / dy_front + 0.5), 1.0)
    model.set(b=lambda x, y, z: N2 * z + db * ramp(y) + 1e-2 * db * rng.standard_normal(np.broadcast(x, y, z).shape))
    for _ in range(20):
        model.time_step(1200.0)
    ocn.sync_device()
    for f in (model.u, model.v, model.w, model.tracers[0]):
        assert np.isfinite(from_dev(f)).all()
    assert np.isfinite(model.eta.cpu().numpy()).all()
    v = from_dev(model.v)
    assert np.all(v[:, grid.Hy, :] == 0.0) and np.all(v[:, grid.Hy + grid.Ny, :] == 0.0)
    assert np.abs(from_dev(model.u)).max() > 0
