"""Operation trees, ComputedField, Average and Integral on the device against the NumPy restatement (tests/operations_numpy.py).

Pointwise results are compared bit for bit: + - * / sqrt are correctly rounded on both sides and the library's diagnostics are built
without FMA contraction.  A reduction is compared with the exact sum of the restatement's per-cell terms (math.fsum) within
(n + 8) ε Σ|tᵢ| / W, ε = 2⁻⁵³: the first-order bound (n - 1) ε Σ|tᵢ| of a sum of n terms added in any order, plus one rounding each for the
division, the divisor W and the two roundings of the exact value itself; it holds for every summation order and needs no measured number.
Fields are seeded random over their WHOLE parent arrays and no halo fill is called, so a wrong offset shows."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import operations_cases as OC
import operations_numpy as ON

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = -7.25e300


class Setup:
    def __init__(self, ocn, gname):
        self.grid = ocn.RectilinearGrid(ocn.GPU(), **OC.GRIDS[gname])
        self.parents = OC.random_parents(self.grid, 1 + list(OC.GRIDS).index(gname))
        self.f = {}
        for n, a in self.parents.items():
            self.f[n] = ocn.Field(OC.mask_of(OC.LOCS[n]), self.grid)
            self.f[n].data.copy_(torch.from_numpy(np.ascontiguousarray(a.T)))
        self.leaves, self.g = OC.leaves(self.parents), ON.Grid(self.grid)


_setups = {}


@pytest.fixture(scope="module")
def setup(ocn):
    def get(gname):
        if gname not in _setups:
            _setups[gname] = Setup(ocn, gname)
        return _setups[gname]
    yield get
    _setups.clear()


def interior_slices(cf):
    g = cf.grid
    H = [0 if (cf.reduced >> d) & 1 else h for d, h in enumerate((g.Hx, g.Hy, g.Hz))]
    shape = cf.parent_shape()
    return tuple(slice(H[d], shape[d] - H[d]) for d in range(3))


@pytest.mark.parametrize("gname", list(OC.GRIDS))
def test_pointwise_is_bitwise_the_restatement(ocn, setup, gname):
    s = setup(gname)
    for name, (tree, e) in OC.pointwise_cases(ocn, s.f).items():
        loc, want = ON.pointwise(e, s.leaves, s.g)
        cf = ocn.ComputedField(tree)
        assert OC.location_names(ocn, cf.location) == loc and cf.halos_filled == (cf.loc in (0, 1, 2, 4)), (gname, name)
        # the kernel alone: every interior element is written, nothing outside the interior is
        cf.data.fill_(SENTINEL)
        ocn._lib.call("ocn_op_compute", s.grid.cref, C.byref(cf._c), cf.ptr, ocn.architectures.stream_ptr())
        parent = cf.parent()
        sl = interior_slices(cf)
        assert parent[sl].shape == want.shape, (gname, name)
        assert np.array_equal(parent[sl], want), (gname, name, float(np.max(np.abs(parent[sl] - want))))
        outside = np.ones(parent.shape, dtype=bool)
        outside[sl] = False
        assert np.all(parent[outside] == SENTINEL), (gname, name)
        # compute!: the same interior (and the default halo fill where the library has one)
        assert cf.compute() is cf
        assert np.array_equal(cf.interior(), want), (gname, name)


def reduction_cases(ocn, s):
    ops = dict(OC.reduction_operands(ocn, s.f))
    U = ocn.compute(ocn.Average(s.f["u"], dims=(1, 2)))
    assert U.location == (None, None, ocn.Center) and U.data.shape == (s.grid.parent_shape(1)[2], 1, 1)
    leaves = dict(s.leaves)
    leaves["U"] = ON.Leaf(U.parent(), (None, None, "C"))   # (U itself is checked as Average of u over (1, 2))
    ops["u'"] = (s.f["u"] - U, ("-", ("f", "u"), ("f", "U")))
    return ops, leaves


@pytest.mark.parametrize("gname", list(OC.GRIDS))
def test_reductions_within_the_any_order_bound(ocn, setup, gname):
    s = setup(gname)
    ops, leaves = reduction_cases(ocn, s)
    worst = 0.0
    for oname, (operand, e) in ops.items():
        for dims in OC.DIMS:
            for kind in ("Average", "Integral"):
                cf = ocn.ComputedField(getattr(ocn, kind)(operand, dims=dims))
                cf.data.fill_(SENTINEL)
                got = cf.compute().interior()
                loc, t, W = ON.reduction_terms(kind, e, dims, leaves, s.g)
                exact, n, sabs = ON.reduce_exact(t, dims, W)
                assert got.shape == exact.shape, (gname, oname, dims, kind)
                bound = ON.reduction_bound(n, sabs, W)
                err = np.abs(got - exact)
                worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
                assert np.all(err <= bound), (gname, oname, dims, kind, float(np.max(err)), float(np.max(bound)))
                assert tuple(None if (d + 1) in dims else loc[d] for d in range(3)) == OC.location_names(ocn, cf.location)
                # bit-identical from call to call
                again = cf.compute().interior()
                assert np.array_equal(got, again), (gname, oname, dims, kind)
    print(f"{gname}: largest error / bound = {worst:.3f}")


def test_reference_values_of_the_2x2x2_test(ocn):
    golden = json.load(open(os.path.join(HERE, "golden", "field_scans_2x2x2.json")))
    for stretched in (False, True):
        grid = OC.scans_grid(ocn, ocn.GPU(), stretched)
        f = {}
        for n, a in OC.trilinear_parents(grid).items():
            f[n] = ocn.Field(OC.mask_of(OC.LOCS[n]), grid)
            f[n].data.copy_(torch.from_numpy(np.ascontiguousarray(a.T)))
        OC.check_scans(golden, lambda kind, name, dims: ocn.compute(getattr(ocn, kind)(f[name], dims=dims)).interior())


def test_malformed_programs_launch_nothing(ocn, setup):
    s = setup("stretched_70x3x5")
    L = ocn._lib
    out = ocn.Field(0, s.grid)
    ws = torch.full((1 << 16,), SENTINEL, dtype=torch.float64, device=out.data.device)
    good = ocn.ComputedField(ocn.ddx(s.f["u"]) + s.f["c"])._c
    for what, (change, message) in OC.MALFORMED.items():
        p = L.COpProgram.from_buffer_copy(good)
        if what == "forward operand":
            p.ins[p.n_instructions - 1].b = p.n_instructions - 1
        elif what == "register out of range":
            p.ins[0].reg = p.n_registers
        elif what == "field out of range":
            p.ins[0].field = p.n_fields
        else:
            p.ins[0].di = s.grid.Hx + 1
        out.data.fill_(SENTINEL)
        for call in (lambda: L.lib().ocn_op_compute(s.grid.cref, C.byref(p), out.ptr, None),
                     lambda: L.lib().ocn_op_reduce(s.grid.cref, C.byref(p), 3, 1.0, ws.data_ptr(), ws.numel(), out.ptr, None)):
            assert call() == -1, what
        torch.cuda.synchronize()
        assert bool((out.data == SENTINEL).all()) and bool((ws == SENTINEL).all()), what


def test_model_state_after_time_step_has_the_halos_the_operations_read(ocn):
    P, B = OC.P, OC.B
    grid = ocn.RectilinearGrid(ocn.GPU(), size=(16, 16, 16), x=(0, 1), y=(0, 1), z=(-1, 0), topology=(P, P, B))
    model = ocn.NonhydrostaticModel(grid, advection=ocn.WENO(), tracers=("b",))
    rng = np.random.default_rng(3)
    ocn.set(model, u=rng.uniform(-1, 1, (16, 16, 16)), v=rng.uniform(-1, 1, (16, 16, 16)), w=rng.uniform(-1, 1, (16, 16, 17)),
            b=rng.uniform(-1, 1, (16, 16, 16)))
    u, v, w, b = model.u, model.v, model.w, model.field("b")
    wb = ocn.ComputedField(ocn.Average(w * b, dims=(1, 2)))
    ke = ocn.ComputedField(ocn.Integral(0.5 * (u ** 2 + v ** 2 + w ** 2)))
    for _ in range(3):
        ocn.time_step(model, 1e-3)
    got = {"wb": wb.compute().interior(), "ke": ke.compute().interior()}
    leaves = {n: ON.Leaf(f.parent(), OC.LOCS[n]) for n, f in (("u", u), ("v", v), ("w", w), ("c", b))}
    assert all(np.isfinite(l.parent).all() for l in leaves.values())
    U, V, W, Bt = (("f", n) for n in ("u", "v", "w", "c"))
    cases = {"wb": ("Average", ("*", W, Bt), (1, 2)),
             "ke": ("Integral", ("*", 0.5, ("+", ("+", ("sq", U), ("sq", V)), ("sq", W))), (1, 2, 3))}
    g = ON.Grid(grid)
    for name, (kind, e, dims) in cases.items():
        loc, t, Wd = ON.reduction_terms(kind, e, dims, leaves, g)
        exact, n, sabs = ON.reduce_exact(t, dims, Wd)
        assert got[name].shape == exact.shape
        assert np.all(np.abs(got[name] - exact) <= ON.reduction_bound(n, sabs, Wd)), name
    assert float(np.abs(got["ke"]).max()) > 0
