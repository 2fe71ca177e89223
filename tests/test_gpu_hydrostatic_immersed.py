"""HydrostaticFreeSurfaceModel on ImmersedBoundaryGrid(grid, GridFittedBottom(h)) on the GPU (csrc/immersed.hip) against the CPU restatement
tests/hydrostatic_immersed_numpy.py, in strict math: every entry point and three steps of the model bit for bit, the flat-bottom model
against the plain-grid model, a lake at rest, no flux through the bottom, exact zeros inside the bottom, a bit-identical restart."""
import numpy as np
import pytest

import hydrostatic_immersed_numpy as HI
from helpers import from_dev, stretched_faces, to_dev

pytestmark = pytest.mark.gpu

# (16, 12, 7) with halo 3; (67, 6, 5) with halo (4, 5, 3): across the 64-lane block edge in x, a partial block in y, unequal halos;
# (16, 12, 10) with halo 3: more levels than the 8 a thread of the z-walking kernels takes, so a second, partial chunk in z
SHAPES = [((16, 12, 7), (3, 3, 3)), ((67, 6, 5), (4, 5, 3)), ((16, 12, 10), (3, 3, 3))]
LX, LY, LZ = 2.0e3, 1.5e3, 40.0
GRAV = 9.80665
UNWRITTEN = 777.0   # what outputs hold before a launch: a cell the kernel should not write still holds it afterwards
U, V, W, Cc = 1, 2, 4, 0


def z_of(size, stretched):
    return stretched_faces(size[2], LZ) if stretched else (-LZ, 0.0)


def bathymetry(og):
    """h for GridFittedBottom: below the domain (no immersed cell) but for
      * a plateau two cells high next to untouched columns (a step of more than one level), across the 64-lane edge when Nx > 64;
      * a 3 x 3 block of dry columns around one wet column;
      * two ridges three cells high with a one-cell-wide trench between them, running through the periodic seam in y;
      * a dry column and a raised one on the periodic seam in x;
      * when Nz > 8, next to an untouched column: a column with 8 immersed cells, whose bottom lies on the edge between the two z chunks
        of a thread, and beside it one with 9.
    Heights are cell-centre values, so each is also the case `h exactly at a centre`."""
    Nx, Ny, Nz = og.Nx, og.Ny, og.Nz
    zc = np.asarray(og.nodes(2, False))[:Nz]
    level = lambda n: -1e3 if n == 0 else (1.0 if n >= Nz else zc[n - 1])   # h that immerses n cells (CenterImmersedCondition)
    h = np.full((Nx, Ny), level(0))
    h[2:5, 1:4] = level(2)
    if Nx > 64:
        h[62:66, 2:5] = level(2)
    h[7:10, 1:4] = level(Nz)
    h[8, 2] = level(0)
    h[12, :] = level(3)
    h[14, :] = level(3)
    h[0, Ny - 1] = level(Nz)
    h[Nx - 1, 0] = level(1)
    if Nz > 8:
        h[5, 7] = level(8)
        h[6, 7] = level(9)
    return h


def make_grids(O, ocn, size, halo, stretched, h=None, interface=False):
    z = z_of(size, stretched)
    og = O.Grid(size, x=(0, LX), y=(0, LY), z=z, topology="PPB", halo=halo)
    under = ocn.RectilinearGrid(ocn.GPU(), size=size, x=(0, LX), y=(0, LY), z=z, topology=("Periodic", "Periodic", "Bounded"), halo=halo)
    h = bathymetry(og) if h is None else h
    cond = ocn.InterfaceImmersedCondition() if interface else ocn.CenterImmersedCondition()
    return og, ocn.ImmersedBoundaryGrid(under, ocn.GridFittedBottom(h, cond)), HI.Bathymetry(og, h, interface), h


class Case:
    def __init__(self, O, ocn, size, halo, stretched, seed=11):
        self.O, self.ocn = O, ocn
        self.og, self.pg, self.B, self.h = make_grids(O, ocn, size, halo, stretched)
        self.rng = np.random.default_rng(seed)
        self.H, self.N, self.stretched = halo, size, stretched

    def box(self, loc, lo=(0, 0, 0), hi=(0, 0, 0), fill=np.nan, scale=1.0):
        """parent array of a field at `loc`: random over the indices 1 - lo .. N + hi (w: up to Nz + 1 + hi), `fill` elsewhere"""
        a = np.full(self.og.shape(loc), fill, order="F")
        ext = (0, 0, 1 if loc == W else 0)
        sl = tuple(slice(self.H[d] - lo[d], self.H[d] + self.N[d] + hi[d] + ext[d]) for d in range(3))
        a[sl] = scale * self.rng.uniform(-1, 1, a[sl].shape)
        return a

    def plane(self, lo=(0, 0), hi=(0, 0), fill=np.nan):
        a = np.full(self.og.shape(0)[:2], fill, order="F")
        sl = tuple(slice(self.H[d] - lo[d], self.H[d] + self.N[d] + hi[d]) for d in range(2))
        a[sl] = self.rng.uniform(-1, 1, a[sl].shape)
        return a

    def dev(self, loc, a):
        return to_dev(self.ocn, self.pg, loc, a)

    def dplane(self, a, dtype=None):
        import torch
        t = torch.from_numpy(np.ascontiguousarray(a.T)).to("cuda")
        return t if dtype is None else t.to(dtype)

    def call(self, name, *args):
        self.ocn._lib.call(name, self.pg.cref, *args)
        self.ocn.sync_device()

    @property
    def kbot(self):
        return self.pg.plane_ptr("kbot")

    @property
    def ii(self):
        return slice(self.H[0], self.H[0] + self.N[0])

    @property
    def jj(self):
        return slice(self.H[1], self.H[1] + self.N[1])


def _host(t):
    return t.cpu().numpy().T


CASES = [(s, h, st) for (s, h) in SHAPES for st in (False, True)]
IDS = [f"{'x'.join(map(str, s))}-{'stretched' if st else 'uniform'}" for s, h, st in CASES]


@pytest.fixture(params=CASES, ids=IDS)
def case(request, oracle, ocn):
    ocn.set_math_mode(ocn.MATH_STRICT)
    return Case(oracle, ocn, *request.param)


def test_the_bathymetry_holds_every_feature(case):
    B, Nz = case.B, case.N[2]
    kb = B.immersed.sum(axis=2)
    dry = kb == Nz
    assert (kb == 0).any() and dry.any()
    assert dry[7:10, 1:4].sum() == 8 and kb[8, 2] == 0                                    # one wet column enclosed by dry ones
    assert (kb[12] == 3).all() and (kb[14] == 3).all() and (kb[13] == 0).all()            # a one-cell-wide trench, through the seam in y
    assert kb[2, 1] - kb[1, 1] == 2                                                       # a step of more than one level
    assert dry[0, -1] and kb[-1, 0] == 1                                                  # on the seam in x
    if Nz > 8:
        assert kb[4, 7] == 0 and kb[5, 7] == 8 and kb[6, 7] == 9                          # a bottom on the z-chunk edge, one past it


# ---- the entry points -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interface", [False, True])
def test_bottom_height_kbot_and_column_depths(case, interface):
    """reach: the whole parent plane (halos are the periodic images); the product's host-side arrays are the same"""
    import torch
    c = case
    rng = np.random.default_rng(4)
    zf = np.asarray(c.og.nodes(2, True))[:c.N[2] + 1]
    h = rng.uniform(-1.2 * LZ, 0.1 * LZ, c.N[:2])
    h[3, 2], h[4, 2], h[5, 2] = zf[2], 0.5 * (zf[1] + zf[2]), zf[0]   # exactly at a face, exactly at a centre, at the domain's bottom
    og, pg, B, _ = make_grids(c.O, c.ocn, c.N, c.H, c.stretched, h, interface)
    Hx, Hy = c.H[:2]
    pad = lambda a: np.pad(a, ((Hx, Hx), (Hy, Hy)), mode="wrap")
    hp = np.full(og.shape(0)[:2], np.nan)
    hp[c.ii, c.jj] = h
    out = {n: torch.full((c.N[1] + 2 * Hy, c.N[0] + 2 * Hx), UNWRITTEN, dtype=torch.float64, device="cuda") for n in ("bottom", "Hcc", "Hfc", "Hcf")}
    kb = torch.full((c.N[1] + 2 * Hy, c.N[0] + 2 * Hx), -7, dtype=torch.int32, device="cuda")
    zc = torch.from_numpy(np.ascontiguousarray(np.asarray(og.nodes(2, False))[:c.N[2]])).to("cuda")
    zfd = torch.from_numpy(np.ascontiguousarray(zf)).to("cuda")
    dh = c.dplane(hp)
    c.ocn._lib.call("ocn_immersed_compute_bottom", pg.cref, int(interface), dh.data_ptr(), zc.data_ptr(), zfd.data_ptr(),
                    out["bottom"].data_ptr(), kb.data_ptr(), out["Hcc"].data_ptr(), out["Hfc"].data_ptr(), out["Hcf"].data_ptr(), 0)
    c.ocn.sync_device()
    np.testing.assert_array_equal(_host(out["bottom"]), pad(B.bottom))
    np.testing.assert_array_equal(_host(kb), pad(B.immersed.sum(axis=2)))
    for n, want in (("Hcc", B.Hcc), ("Hfc", B.Hfc), ("Hcf", B.Hcf)):
        np.testing.assert_array_equal(_host(out[n]), pad(want))
    # the grid object: its planes are this launch's, its host arrays the same numbers
    for n in out:
        np.testing.assert_array_equal(_host(pg._planes[n]), _host(out[n]))
    np.testing.assert_array_equal(_host(pg._planes["kbot"]), _host(kb))
    np.testing.assert_array_equal(pg.immersed_boundary.bottom_height, B.bottom)
    np.testing.assert_array_equal(c.ocn.immersed_cell(pg), B.immersed)
    np.testing.assert_array_equal(c.ocn.static_column_depth(pg, "fc"), B.Hfc)


def test_mask_fields(case):
    """reach: the immersed_peripheral_node of each field over 1:N, the planes U, V at k = Nz; η is never masked (its plane lies on the
    underlying grid's periphery); NaN on a masked node is replaced"""
    c = case
    full = tuple(c.H)
    fields = [(loc, c.box(loc, lo=full, hi=full)) for loc in (U, V, Cc, Cc)]
    for loc, a in fields:
        a[c.H[0] + 7:c.H[0] + 10, c.H[1] + 1:c.H[1] + 4, :] = np.nan   # the dry block: masked but for the wet column's own nodes
        a[c.H[0] + 8, c.H[1] + 2, :] = 0.25
    eta, Up, Vp = c.plane(lo=full[:2], hi=full[:2]), c.plane(lo=full[:2], hi=full[:2]), c.plane(lo=full[:2], hi=full[:2])
    devs = [c.dev(loc, a) for loc, a in fields]
    de, dU, dV = c.dplane(eta), c.dplane(Up), c.dplane(Vp)
    pa, ia = c.ocn._lib.ptr_array, c.ocn._lib.i32_array
    c.call("ocn_immersed_mask_fields", c.kbot, len(devs), pa([d.ptr for d in devs]), ia([loc for loc, _ in fields]), 0.0, de.data_ptr(),
           dU.data_ptr(), dV.data_ptr(), 0)
    kt = c.H[2] + c.N[2] - 1
    for (loc, a), d in zip(fields, devs):
        before = a.copy()
        HI.mask_field(c.B, a, {U: HI.FCC, V: HI.CFC, Cc: HI.CCC}[loc])
        np.testing.assert_array_equal(from_dev(d), a)
        assert (a != before).sum() > 0
    Up[c.ii, c.jj][c.B.immersed_peripheral_node(HI.FCC)[c.ii, c.jj, kt]] = 0.0
    Vp[c.ii, c.jj][c.B.immersed_peripheral_node(HI.CFC)[c.ii, c.jj, kt]] = 0.0
    np.testing.assert_array_equal(_host(de), eta)
    np.testing.assert_array_equal(_host(dU), Up)
    np.testing.assert_array_equal(_host(dV), Vp)
    assert (Up[c.ii, c.jj] == 0.0).sum() > 0
    # the tracer in the wet column enclosed by dry ones survives; u on its faces does not
    assert np.all(fields[2][1][c.H[0] + 8, c.H[1] + 2, c.H[2]:c.H[2] + c.N[2]] == 0.25)
    assert np.all(fields[0][1][c.H[0] + 8, c.H[1] + 2, c.H[2]:c.H[2] + c.N[2]] == 0.0)
    # the public function, with another value
    a = c.box(Cc, lo=full, hi=full)
    d = c.dev(Cc, a)
    c.ocn.mask_immersed_field(d, -3.0)
    c.ocn.sync_device()
    HI.mask_field(c.B, a, HI.CCC, -3.0)
    np.testing.assert_array_equal(from_dev(d), a)


def _velocities(c):
    one = (1, 1, 1)
    return c.box(U, lo=one, hi=one), c.box(V, lo=one, hi=one), c.box(W, lo=(1, 1, 0), hi=(0, 0, 0))


@pytest.mark.parametrize("with_eta", [False, True])
def test_vector_invariant_tendencies(case, with_eta):
    """reach: u, v one cell around the interior in every direction, w at the faces 1 .. Nz + 1 and one column to the west / south, η one
    cell to the west / south; written: Gu, Gv over 1:N"""
    c = case
    u, v, w = _velocities(c)
    eta = c.plane(lo=(1, 1))
    Gu, Gv = np.full(c.og.shape(U), UNWRITTEN, order="F"), np.full(c.og.shape(V), UNWRITTEN, order="F")
    du, dv, dw, dGu, dGv, de = c.dev(U, u), c.dev(V, v), c.dev(W, w), c.dev(U, Gu), c.dev(V, Gv), c.dplane(eta)
    with np.errstate(invalid="ignore"):
        HI.vector_invariant_tendencies(c.B, u, v, w, Gu, Gv, eta if with_eta else None, GRAV)
    c.call("ocn_immersed_vector_invariant_momentum_tendencies", c.kbot, du.ptr, dv.ptr, dw.ptr, dGu.ptr, dGv.ptr,
           de.data_ptr() if with_eta else None, GRAV, 0)
    np.testing.assert_array_equal(from_dev(dGu), Gu)
    np.testing.assert_array_equal(from_dev(dGv), Gv)
    assert np.isfinite(Gu).all() and (Gu == UNWRITTEN).any() and np.isfinite(Gv).all()


def test_the_conditional_differences_matter(case):
    """the same launch with a flat kbot gives other numbers next to the bottom and the same ones away from it"""
    import torch
    c = case
    u, v, w = _velocities(c)
    du, dv, dw = c.dev(U, u), c.dev(V, v), c.dev(W, w)
    out = []
    for kb in (c.pg._planes["kbot"], torch.zeros_like(c.pg._planes["kbot"])):
        dGu, dGv = c.dev(U, np.full(c.og.shape(U), UNWRITTEN, order="F")), c.dev(V, np.full(c.og.shape(V), UNWRITTEN, order="F"))
        c.call("ocn_immersed_vector_invariant_momentum_tendencies", kb.data_ptr(), du.ptr, dv.ptr, dw.ptr, dGu.ptr, dGv.ptr, None, GRAV, 0)
        out.append(c.og.interior(from_dev(dGu)))
    differs = out[0] != out[1]
    assert differs.any() and not differs[4:6, 5:, -1].any()
    # and the flat one is the plain kernel
    dGu, dGv = c.dev(U, np.full(c.og.shape(U), UNWRITTEN, order="F")), c.dev(V, np.full(c.og.shape(V), UNWRITTEN, order="F"))
    c.call("ocn_compute_vector_invariant_momentum_tendencies", du.ptr, dv.ptr, dw.ptr, dGu.ptr, dGv.ptr, None, GRAV, 0)
    np.testing.assert_array_equal(c.og.interior(from_dev(dGu)), out[1])


def test_viscous_terms(case):
    """reach: as the vector-invariant launch; Gu, Gv are updated over 1:N"""
    c = case
    u, v, w = _velocities(c)
    Gu, Gv = c.box(U, fill=UNWRITTEN), c.box(V, fill=UNWRITTEN)
    du, dv, dw, dGu, dGv = c.dev(U, u), c.dev(V, v), c.dev(W, w), c.dev(U, Gu), c.dev(V, Gv)
    with np.errstate(invalid="ignore"):
        HI.viscous_terms(c.B, 1e-2, u, v, w, Gu, Gv)
    c.call("ocn_immersed_add_viscous_terms", c.kbot, 1e-2, du.ptr, dv.ptr, dw.ptr, dGu.ptr, dGv.ptr, 0)
    np.testing.assert_array_equal(from_dev(dGu), Gu)
    np.testing.assert_array_equal(from_dev(dGv), Gv)
    assert np.isfinite(Gu).all() and (Gu == UNWRITTEN).any()


@pytest.mark.parametrize("closure", [0, 1])
def test_tracer_tendency(case, closure):
    """reach: c one cell around the interior in every direction, u / v one face to the east / north, w at the faces k and k + 1"""
    c = case
    one = (1, 1, 1)
    u, v, w, t = c.box(U, hi=(1, 0, 0)), c.box(V, hi=(0, 1, 0)), c.box(W), c.box(Cc, lo=one, hi=one)
    G = np.full(c.og.shape(Cc), UNWRITTEN, order="F")
    du, dv, dw, dt_, dG = c.dev(U, u), c.dev(V, v), c.dev(W, w), c.dev(Cc, t), c.dev(Cc, G)
    with np.errstate(invalid="ignore"):
        HI.tracer_tendency(c.B, u, v, w, t, G, 1e-3 if closure else None)
    c.call("ocn_immersed_tracer_tendency", c.kbot, closure, 1e-3, du.ptr, dv.ptr, dw.ptr, dt_.ptr, dG.ptr, 0)
    np.testing.assert_array_equal(from_dev(dG), G)
    assert np.isfinite(G).all() and (G == UNWRITTEN).any()
    if not closure:
        assert np.all(c.og.interior(G)[c.B.immersed & ((np.arange(1, c.N[2] + 1) > 1) & (np.arange(1, c.N[2] + 1) < c.N[2]))[None, None, :]] == 0.0)


@pytest.mark.parametrize("chi", [-0.5, 0.1])
def test_split_explicit_forcing(case, chi):
    c = case
    Gs = [c.box(loc) for loc in (U, U, V, V)]
    if chi == -0.5:   # an Euler step multiplies G⁻ by false: whatever it holds, NaN in the halos included, stays out
        Gs[1][...] = np.where(np.isnan(Gs[1]), np.nan, 1e300)
    GU, GV = np.full(c.og.shape(0)[:2], UNWRITTEN, order="F"), np.full(c.og.shape(0)[:2], UNWRITTEN, order="F")
    dG = [c.dev(loc, a) for loc, a in zip((U, U, V, V), Gs)]
    dGU, dGV = c.dplane(GU), c.dplane(GV)
    GU[c.ii, c.jj] = HI.split_explicit_forcing(c.B, Gs[0], Gs[1], chi, HI.FCC)
    GV[c.ii, c.jj] = HI.split_explicit_forcing(c.B, Gs[2], Gs[3], chi, HI.CFC)
    c.call("ocn_immersed_split_explicit_forcing", c.kbot, *[d.ptr for d in dG], chi, dGU.data_ptr(), dGV.data_ptr(), 0)
    np.testing.assert_array_equal(_host(dGU), GU)
    np.testing.assert_array_equal(_host(dGV), GV)
    assert np.isfinite(GU).all() and (GU[c.ii, c.jj] == 0.0).any()


@pytest.mark.parametrize("n", [1, 4])
def test_split_explicit_substeps(case, n):
    """reach: the interiors of the planes (the kernels wrap their neighbour indices)"""
    c = case
    planes = {k: c.plane() for k in ("eta", "U", "V", "GU", "GV")}
    for k in ("etab", "Ub", "Vb"):
        planes[k] = np.full(c.og.shape(0)[:2], np.nan, order="F")
    d = {k: c.dplane(a) for k, a in planes.items()}
    weights = np.array([0.4, 0.3, 0.2, 0.1])[:n] / np.array([0.4, 0.3, 0.2, 0.1])[:n].sum()
    host = {k: planes[k][c.ii, c.jj].copy() for k in planes}
    for k in ("etab", "Ub", "Vb"):
        host[k][...] = 0.0
    HI.iterate_split_explicit(c.B, host["eta"], host["U"], host["V"], host["etab"], host["Ub"], host["Vb"], host["GU"], host["GV"], 0.7, weights,
                              GRAV)
    import ctypes as C
    c.call("ocn_immersed_split_explicit_substeps", c.kbot, c.pg.plane_ptr("Hfc"), c.pg.plane_ptr("Hcf"), n, (C.c_double * n)(*weights), 0.7, GRAV,
           *[d[k].data_ptr() for k in ("eta", "U", "V", "etab", "Ub", "Vb", "GU", "GV")], 0)
    for k in ("eta", "U", "V"):   # _update_split_explicit_state!: the averages
        np.testing.assert_array_equal(_host(d[k])[c.ii, c.jj], host[k + "b"], err_msg=k)
        np.testing.assert_array_equal(_host(d[k + "b"])[c.ii, c.jj], host[k + "b"], err_msg=k)
    assert np.isfinite(host["etab"]).all()
    if n == 1:   # no transport reaches a dry column: its η stays
        dry = c.B.immersed.all(axis=2)
        np.testing.assert_array_equal(host["etab"][dry], planes["eta"][c.ii, c.jj][dry])


def test_barotropic_corrector(case):
    """u += (U - U̅) / Hᶠᶜ with U̅ = Σ Δz u; a dry face gets 0 / 0 in the reference, in the restatement and here"""
    c = case
    u, v = c.box(U, fill=UNWRITTEN), c.box(V, fill=UNWRITTEN)
    HI.mask_field(c.B, u, HI.FCC)
    HI.mask_field(c.B, v, HI.CFC)
    Up, Vp = c.plane(fill=UNWRITTEN), c.plane(fill=UNWRITTEN)
    kt = c.H[2] + c.N[2] - 1
    Up[c.ii, c.jj][c.B.peripheral_node(HI.FCC)[c.ii, c.jj, kt]] = 0.0
    Vp[c.ii, c.jj][c.B.peripheral_node(HI.CFC)[c.ii, c.jj, kt]] = 0.0
    du, dv, dU, dV = c.dev(U, u), c.dev(V, v), c.dplane(Up), c.dplane(Vp)
    dUb, dVb = c.dplane(np.full_like(Up, UNWRITTEN)), c.dplane(np.full_like(Up, UNWRITTEN))
    Ub, Vb = HI.barotropic_corrector(c.B, u, v, Up[c.ii, c.jj], Vp[c.ii, c.jj])
    c.call("ocn_immersed_barotropic_corrector", c.pg.plane_ptr("Hfc"), c.pg.plane_ptr("Hcf"), du.ptr, dv.ptr, dU.data_ptr(), dV.data_ptr(),
           dUb.data_ptr(), dVb.data_ptr(), 0)
    np.testing.assert_array_equal(from_dev(du), u)
    np.testing.assert_array_equal(from_dev(dv), v)
    np.testing.assert_array_equal(_host(dUb)[c.ii, c.jj], Ub)
    np.testing.assert_array_equal(_host(dVb)[c.ii, c.jj], Vb)
    assert np.isnan(c.og.interior(u)).any() and (u == UNWRITTEN).any()
    assert not np.isnan(c.og.interior(u)[~c.B.interior(c.B.peripheral_node(HI.FCC))]).any()


# ---- the model --------------------------------------------------------------------------------------------------------------------------
SURFACES = {"explicit": None, "split": 4}
MODEL_CASES = [(SHAPES[0], False), (SHAPES[1], True)]
MODEL_IDS = ["16x12x7-uniform", "67x6x5-stretched"]


def _models(O, ocn, shape, stretched, surface, closure, h=None, plain=False, seed=3, tracers=("b", "c"), buoyancy=True, coriolis=True, rest=False):
    size, halo = shape
    og, pg, B, h = make_grids(O, ocn, size, halo, stretched, h)
    sub = SURFACES[surface]
    fs = ocn.ExplicitFreeSurface() if sub is None else ocn.SplitExplicitFreeSurface(substeps=sub)
    kw = dict(tracers=tracers, buoyancy=ocn.BuoyancyTracer() if buoyancy else None, coriolis=ocn.FPlane(f=1e-4) if coriolis else None,
              free_surface=fs, closure=ocn.ScalarDiffusivity(ν=closure[0], κ=closure[1]) if closure else None)
    pm = ocn.HydrostaticFreeSurfaceModel(pg.underlying_grid if plain else pg, fused=False if plain else None, **kw)
    om = HI.HydrostaticFreeSurfaceModel(og, h, tracers=tracers, coriolis_f=1e-4 if coriolis else None, closure=closure,
                                        buoyancy="BuoyancyTracer" if buoyancy else None, split_explicit_substeps=sub)
    rng = np.random.default_rng(seed)
    init = {}
    if not rest:
        init = dict(u=0.1 * rng.uniform(-1, 1, size), v=0.1 * rng.uniform(-1, 1, size), eta=0.01 * rng.uniform(-1, 1, size[:2]))
    for name in tracers:
        init[name] = 1e-3 * rng.uniform(-1, 1, size) if name == "b" else rng.uniform(0.5, 1.5, size)
    return og, B, om, pm, init


def _invariants(og, B, pm, split):
    """after any step: u, v exactly 0 on every peripheral face, tracers exactly 0 in immersed cells, no NaN anywhere in the interior"""
    u, v = og.interior_N(from_dev(pm.u)), og.interior_N(from_dev(pm.v))
    assert np.all(u[B.interior(B.immersed_peripheral_node(HI.FCC))] == 0.0) and np.all(v[B.interior(B.immersed_peripheral_node(HI.CFC))] == 0.0)
    for t in pm.tracers:
        assert np.all(og.interior_N(from_dev(t))[B.immersed] == 0.0)
    for f in (pm.u, pm.v, pm.w) + tuple(pm.tracers):
        assert np.isfinite(og.interior(from_dev(f))).all()
    assert np.isfinite(pm.eta_interior().cpu().numpy()).all()
    if split:
        assert np.isfinite(pm.U.cpu().numpy()).all() and np.isfinite(pm.V.cpu().numpy()).all()


def _compare(og, om, pm, split):
    ii, jj = slice(og.Hx, og.Hx + og.Nx), slice(og.Hy, og.Hy + og.Ny)
    np.testing.assert_array_equal(pm.eta_interior().cpu().numpy().T, om.eta[ii, jj], err_msg="eta")
    for name, a, d in zip(("u", "v", "w"), (om.u, om.v, om.w), pm.velocities):
        np.testing.assert_array_equal(og.interior(from_dev(d)), og.interior(a), err_msg=name)
    for name, a, d in zip(om.tracer_names, om.tracers, pm.tracers):
        np.testing.assert_array_equal(og.interior(from_dev(d)), og.interior(a), err_msg=name)
    if split:
        np.testing.assert_array_equal(pm.U.cpu().numpy().T[ii, jj], om.U, err_msg="U")
        np.testing.assert_array_equal(pm.V.cpu().numpy().T[ii, jj], om.V, err_msg="V")


@pytest.mark.parametrize("closure", [None, (1e-2, 1e-3)], ids=["no-closure", "ScalarDiffusivity"])
@pytest.mark.parametrize("surface", list(SURFACES))
@pytest.mark.parametrize("shape,stretched", MODEL_CASES, ids=MODEL_IDS)
def test_model_steps_match_the_restatement(oracle, ocn, shape, stretched, surface, closure):
    """three QAB2 steps, the first an Euler step: u, v, w, η, the tracers, U, V bit for bit"""
    ocn.set_math_mode(ocn.MATH_STRICT)
    og, B, om, pm, init = _models(oracle, ocn, shape, stretched, surface, closure)
    assert pm.fused is False
    om.set(**init)
    pm.set(**init)
    ocn.sync_device()
    _invariants(og, B, pm, surface == "split")
    for _ in range(3):
        om.time_step(2.0)
        pm.time_step(2.0)
        ocn.sync_device()
        _invariants(og, B, pm, surface == "split")
    _compare(og, om, pm, surface == "split")
    assert np.abs(og.interior(om.w)).max() > 0 and np.abs(og.interior(om.u)).max() > 0


@pytest.mark.parametrize("surface", list(SURFACES))
@pytest.mark.parametrize("shape,stretched", MODEL_CASES, ids=MODEL_IDS)
def test_flat_bottom_is_the_plain_grid_model(oracle, ocn, shape, stretched, surface):
    """with h at the domain's bottom nothing is immersed: the model equals the plain-grid model with fused = False, whose kernels are
    tested against the oracle, bit for bit after three steps"""
    ocn.set_math_mode(ocn.MATH_STRICT)
    size = shape[0]
    h = np.full(size[:2], -LZ)
    h[::2, :] = -2 * LZ
    _, _, _, pa, init = _models(oracle, ocn, shape, stretched, surface, (1e-2, 1e-3), h=h)
    og, _, _, pb, _ = _models(oracle, ocn, shape, stretched, surface, (1e-2, 1e-3), h=h, plain=True)
    assert int(pa.grid._planes["kbot"].abs().sum()) == 0 and pb.fused is False
    pa.set(**init)
    pb.set(**init)
    for _ in range(3):
        pa.time_step(2.0)
        pb.time_step(2.0)
    ocn.sync_device()
    for name, a, b in zip(("u", "v", "w", "b", "c"), pa.velocities + tuple(pa.tracers), pb.velocities + tuple(pb.tracers)):
        np.testing.assert_array_equal(og.interior(from_dev(a)), og.interior(from_dev(b)), err_msg=name)
    np.testing.assert_array_equal(pa.eta_interior().cpu().numpy(), pb.eta_interior().cpu().numpy())
    if surface == "split":
        np.testing.assert_array_equal(pa.U.cpu().numpy(), pb.U.cpu().numpy())
    assert np.abs(og.interior(from_dev(pa.w))).max() > 0


def _seamount(og, height=0.6):
    x = np.asarray(og.nodes(0, False))[:, None]
    y = np.asarray(og.nodes(1, False))[None, :]
    return -LZ + height * LZ * np.exp(-((x - LX / 2) ** 2 / (LX / 6) ** 2 + (y - LY / 2) ** 2 / (LY / 6) ** 2))


@pytest.mark.parametrize("surface", list(SURFACES))
def test_lake_at_rest_over_a_seamount(oracle, ocn, surface):
    """u = v = 0, η = 0, b = N² z, closure = None: ten steps leave u, v, w exactly 0 and b unchanged bit for bit"""
    ocn.set_math_mode(ocn.MATH_STRICT)
    shape = SHAPES[0]
    og = oracle.Grid(shape[0], x=(0, LX), y=(0, LY), z=(-LZ, 0.0), topology="PPB", halo=shape[1])
    og, B, _, pm, _ = _models(oracle, ocn, shape, False, surface, None, h=_seamount(og), tracers=("b",), rest=True)
    assert B.immersed.any() and not B.immersed.all(axis=2).any()
    pm.set(b=lambda x, y, z: 1e-5 * z + 0 * x + 0 * y)
    ocn.sync_device()
    b0 = og.interior(from_dev(pm.tracers[0])).copy()
    assert np.all(b0[B.immersed] == 0.0) and np.all(b0[~B.immersed] != 0.0)
    for _ in range(10):
        pm.time_step(5.0)
    ocn.sync_device()
    for f in pm.velocities:
        assert np.all(og.interior(from_dev(f)) == 0.0)
    np.testing.assert_array_equal(og.interior(from_dev(pm.tracers[0])), b0)
    assert np.all(pm.eta_interior().cpu().numpy() == 0.0)


def test_no_flux_through_the_bottom(oracle, ocn):
    """no buoyancy, zero velocities, a random passive tracer, ScalarDiffusivity(κ), twenty steps: the integral of the tracer over the active
    cells changes by rounding only (the bound: hydrostatic_immersed_numpy.conservation_bound) and every immersed cell holds exactly 0.
    A kernel that differences against the masked zeros loses tracer at first order in κ Δt / Δz²: many orders above the bound."""
    ocn.set_math_mode(ocn.MATH_STRICT)
    shape = SHAPES[0]
    og, B, om, pm, init = _models(oracle, ocn, shape, False, "explicit", (0.0, 2.0), tracers=("c",), buoyancy=False, coriolis=False, rest=True)
    pm.set(**init)
    ocn.sync_device()
    active = ~B.immersed
    V = og.dx * og.dy * og.dz
    c0 = og.interior(from_dev(pm.tracers[0])).copy()
    for _ in range(20):
        pm.time_step(1.0)
    ocn.sync_device()
    c = og.interior(from_dev(pm.tracers[0]))
    assert np.all(c[~active] == 0.0) and np.abs(c - c0)[active].max() > 1e-3
    change = abs(float((c[active] * V).sum()) - float((c0[active] * V).sum()))
    bound = HI.conservation_bound(20, int(active.sum()), np.abs(c0).max() * V)
    print(f"tracer integral changed by {change:.3e} (bound {bound:.3e}); first-order loss would be ~{2.0 * 20 / og.dz ** 2 * np.abs(c0).max() * V:.3e}")
    assert change <= bound
    for f in pm.velocities:
        assert np.all(og.interior(from_dev(f)) == 0.0)


@pytest.mark.parametrize("surface", list(SURFACES))
def test_restart_from_a_checkpoint_is_bit_identical(oracle, ocn, surface, tmp_path):
    ocn.set_math_mode(ocn.MATH_STRICT)
    shape = SHAPES[0]
    og, B, _, pa, init = _models(oracle, ocn, shape, True, surface, (1e-2, 1e-3))
    _, _, _, pb, _ = _models(oracle, ocn, shape, True, surface, (1e-2, 1e-3))
    pa.set(**init)
    for _ in range(2):
        pa.time_step(2.0)
    path = ocn.write_checkpoint(pa, str(tmp_path / "immersed"))
    ocn.set_from_checkpoint(pb, path)
    for _ in range(2):
        pa.time_step(2.0)
        pb.time_step(2.0)
    ocn.sync_device()
    assert pb.clock.iteration == 4
    for name, a, b in zip(("u", "v", "w", "b", "c"), pa.velocities + tuple(pa.tracers), pb.velocities + tuple(pb.tracers)):
        np.testing.assert_array_equal(from_dev(a), from_dev(b), err_msg=name)
    np.testing.assert_array_equal(pa.eta.cpu().numpy(), pb.eta.cpu().numpy())
    if surface == "split":
        np.testing.assert_array_equal(pa.U.cpu().numpy(), pb.U.cpu().numpy())


def test_defaults_on_an_immersed_grid(oracle, ocn):
    """free_surface = None on an immersed grid is SplitExplicitFreeSurface(grid, cfl = 0.7) (default_free_surface(grid),
    hydrostatic_free_surface_model.jl:54-55), not the implicit one; the halo gets the reference's extra point; the dry-column case steps"""
    ocn.set_math_mode(ocn.MATH_STRICT)
    og, pg, B, h = make_grids(oracle, ocn, (16, 12, 7), (1, 1, 1), False)
    model = ocn.HydrostaticFreeSurfaceModel(pg, tracers=("b",), buoyancy=ocn.BuoyancyTracer(), math_mode=ocn.MATH_STRICT)
    assert isinstance(model.free_surface, ocn.SplitExplicitFreeSurface) and model.free_surface.Δt_barotropic is not None
    assert model.grid.math_mode == ocn.MATH_STRICT and pg.math_mode is None   # (a model's own math mode: the bathymetry is carried along)
    assert isinstance(model.grid, ocn.ImmersedBoundaryGrid) and (model.grid.Hx, model.grid.Hy, model.grid.Hz) == (2, 2, 2)
    np.testing.assert_array_equal(model.grid.kbot, pg.kbot)
    assert model.fused is False and isinstance(model.momentum_advection, ocn.VectorInvariant)
    rng = np.random.default_rng(8)
    model.set(u=0.05 * rng.uniform(-1, 1, (16, 12, 7)), b=1e-3 * rng.uniform(-1, 1, (16, 12, 7)))
    for _ in range(2):
        model.time_step(2.0)
    ocn.sync_device()
    assert model.clock.iteration == 2
    for f in (model.u, model.v, model.w, model.tracers[0]):
        a = from_dev(f)
        assert np.isfinite(a[2:18, 2:14, 2:9]).all()
    assert np.abs(from_dev(model.u)).max() > 0
