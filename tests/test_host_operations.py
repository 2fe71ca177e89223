"""Operation trees, their lowering and the reductions without a GPU: locations, refusals, the lowered program (interpreted in NumPy)
against the restatement (tests/operations_numpy.py), the restatement against the values the reference's own test expects
(test/test_field_scans.jl:19-70, 154-174; tests/golden/field_scans_2x2x2.json), and the argument checks of the C entry points (host code:
nothing is launched)."""
import ctypes as C
import json
import os
import types

import numpy as np
import pytest
import torch

import operations_cases as OC
import operations_numpy as ON

P, B, F = OC.P, OC.B, OC.F
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def pkg():
    import oceananigans_jl_amd as ocn
    return ocn


def host_fields(pkg, grid, parents):
    """fields of the package over host memory (the lowering never touches the data)"""
    return {n: pkg.Field(OC.mask_of(OC.LOCS[n]), grid, data=torch.from_numpy(np.ascontiguousarray(a.T))) for n, a in parents.items()}


@pytest.fixture(scope="module")
def small(pkg):
    grid = pkg.RectilinearGrid(None, size=(6, 5, 4), x=(0, 3), y=(0, 1), z=[-1.0, -0.6, -0.3, -0.1, 0.0], topology=(P, P, B))
    parents = OC.random_parents(grid, 11)
    return grid, parents, host_fields(pkg, grid, parents)


def test_locations_of_results(pkg, small):
    grid, parents, f = small
    u, v, w, c = f["u"], f["v"], f["w"], f["c"]
    Ce, Fa = pkg.Center, pkg.Face
    assert (w * u).location == (Ce, Ce, Fa)           # the first field-like operand decides
    assert (u * w).location == (Fa, Ce, Ce)
    assert (2 * u).location == (Fa, Ce, Ce) and (np.float64(2) * u).location == (Fa, Ce, Ce) and (u / 2).location == (Fa, Ce, Ce)
    assert (pkg.ddx(v) - pkg.ddy(u)).location == (Fa, Fa, Ce)
    assert pkg.ddz(c).location == (Ce, Ce, Fa) and pkg.ddz(w).location == (Ce, Ce, Ce)
    assert pkg.at((Ce,) * 3, u * u + w * w).location == (Ce, Ce, Ce)
    assert (u * u + w * w).location == (Fa, Ce, Ce) and (-u).location == (Fa, Ce, Ce)
    leaves = OC.leaves(parents)
    for name, (tree, e) in OC.pointwise_cases(pkg, f).items():
        assert OC.location_names(pkg, tree.location) == ON.location(e, leaves), name


def test_refusals(pkg, small):
    grid, parents, f = small
    u, w, c = f["u"], f["w"], f["c"]
    for bad in (0.5, 4, -1):
        with pytest.raises(NotImplementedError, match="sqrt"):
            u ** bad
    for fn in (pkg.exp, pkg.log, pkg.tanh):
        with pytest.raises(NotImplementedError):
            fn(c)
    with pytest.raises(NotImplementedError):
        pkg.Average(c, dims=1, condition=lambda *a: True)
    with pytest.raises(NotImplementedError):
        pkg.Integral(c, mask=0.0)
    with pytest.raises(NotImplementedError):
        pkg.CumulativeIntegral(c, dims=3)
    with pytest.raises(NotImplementedError):
        pkg.KernelFunctionOperation(lambda i, j, k, grid: 0.0, grid)
    with pytest.raises(ValueError, match="dims"):
        pkg.Average(c, dims=(1, 4))
    # operands on different grids
    other = pkg.RectilinearGrid(None, size=(6, 5, 4), x=(0, 3), y=(0, 1), z=(-1, 0), topology=(P, P, B))
    c2 = pkg.Field(0, other, data=torch.zeros(tuple(reversed(other.parent_shape(0))), dtype=torch.float64))
    with pytest.raises(ValueError, match="different grids"):
        c + c2
    # a Distributed architecture, a grid stretched in x: refused by the constructor, before anything is allocated
    dist = pkg.RectilinearGrid(None, size=(6, 5, 4), x=(0, 3), y=(0, 1), z=(-1, 0), topology=(P, P, B))
    dist.architecture = types.SimpleNamespace(partition=object())
    cd = pkg.Field(0, dist, data=torch.zeros(tuple(reversed(dist.parent_shape(0))), dtype=torch.float64))
    for operand in (cd * cd, pkg.Average(cd, dims=(1, 2))):
        with pytest.raises(NotImplementedError, match="Distributed"):
            pkg.ComputedField(operand)
    sx = pkg.RectilinearGrid(None, size=(4, 5, 4), x=[0, 0.1, 0.3, 0.6, 1.0], y=(0, 1), z=(-1, 0), topology=(B, P, B))
    cs = pkg.Field(0, sx, data=torch.zeros(tuple(reversed(sx.parent_shape(0))), dtype=torch.float64))
    for operand in (cs * cs, pkg.Integral(cs)):
        with pytest.raises(NotImplementedError, match="stretched in x"):
            pkg.ComputedField(operand)


def test_lowering_of_w_times_u(pkg, small):
    grid, parents, f = small
    p = pkg.lower(f["w"] * f["u"])
    assert len(p.fields) == 2 and len(p.loads) == 5      # w once, u at the four points of ℑxz
    assert sorted(i["off"] for i in p.loads if p.fields[i["field"]] is f["u"]) == [(0, 0, -1), (0, 0, 0), (1, 0, -1), (1, 0, 0)]
    assert p.loc == 4 and p.n_registers <= 6
    regs_ok = all(0 <= i["reg"] < p.n_registers for i in p.instructions)
    assert regs_ok


def test_reach_and_the_halo_check(pkg, small):
    """Nested derivatives alternate between Face and Center, so n of them reach ceil(n / 2) cells on one side and floor(n / 2) on the other
    (from a Center field: i - 1 .. i, i - 1 .. i + 1, i - 2 .. i + 1, i - 2 .. i + 2, ...).  A four-fold nested ddx therefore reaches two
    cells: a halo of 3 holds it, a halo of 1 refuses it; on the halo-3 grid the seventh derivative is the first to leave the halo."""
    grid, parents, f = small
    p = pkg.lower(pkg.ddz(f["u"]) - pkg.ddx(f["w"]))
    assert p.reach == ((1, 0), (0, 0), (1, 0)) and max(max(r) for r in p.reach) == 1

    def nested(field, n):
        for _ in range(n):
            field = pkg.ddx(field)
        return field
    c = f["c"]
    assert pkg.lower(nested(c, 4)).reach[0] == (2, 2)
    assert pkg.lower(nested(c, 6)).reach[0] == (3, 3)
    with pytest.raises(ValueError, match="halo"):
        pkg.lower(nested(c, 7))
    one = pkg.RectilinearGrid(None, size=(6, 5, 4), x=(0, 3), y=(0, 1), z=(-1, 0), topology=(P, P, B), halo=(1, 1, 1))
    c1 = pkg.Field(0, one, data=torch.zeros(tuple(reversed(one.parent_shape(0))), dtype=torch.float64))
    assert pkg.lower(nested(c1, 2)).reach[0] == (1, 1)
    with pytest.raises(ValueError, match="halo"):
        pkg.lower(nested(c1, 4))
    # the products' interpolations add to the reach: w * u reads u at i + 1, so its sixth x-derivative is the first to leave a halo of 3
    assert pkg.lower(nested(f["w"] * f["u"], 4)).reach[0] == (2, 3)
    with pytest.raises(ValueError, match="halo"):
        pkg.lower(nested(f["w"] * f["u"], 6))


def test_common_subexpressions_are_merged(pkg, small):
    grid, parents, f = small
    a = f["c"]
    p = pkg.lower(a * a + a * a)
    assert len(p.loads) == 1 and len(p.instructions) == 3   # LOAD, MUL, ADD
    w, u = f["w"], f["u"]
    q = pkg.lower(w * u + w * u)
    assert len(q.loads) == 5                                 # once per (field, offset)


def test_limits_name_the_limit(pkg, small):
    grid, parents, f = small
    u, v, w, c = f["u"], f["v"], f["w"], f["c"]
    big = w * u
    for _ in range(3):
        big = big * v + pkg.ddx(big) * pkg.ddz(big)
    with pytest.raises(ValueError, match="OCN_OP_MAX_INSTRUCTIONS = 128"):
        pkg.lower(big)
    # a right-leaning quotient of twenty distinct products keeps twenty values alive
    terms = [(c * float(n + 2)) for n in range(20)]
    tree = terms[-1]
    for t in reversed(terms[:-1]):
        tree = t / tree
    with pytest.raises(ValueError, match="OCN_OP_MAX_REGISTERS = 16"):
        pkg.lower(tree)
    many = [pkg.Field(0, grid, data=f["c"].data) for _ in range(9)]
    tree = many[0]
    for m in many[1:]:
        tree = tree + m
    with pytest.raises(ValueError, match="OCN_OP_MAX_FIELDS = 8"):
        pkg.lower(tree)
    for name, (tree, e) in OC.pointwise_cases(pkg, f).items():
        p = pkg.lower(tree)
        assert p.n_registers <= 12 and len(p.instructions) <= 64, (name, p.n_registers, len(p.instructions))


def test_unfilled_and_reduced_leaves(pkg, small):
    grid, parents, f = small
    # stand-ins for computed fields (no device): a field at FFC whose halos are not filled, and a horizontal mean
    ffc = pkg.Field.__new__(pkg.ComputedField)
    ffc.grid, ffc.loc, ffc.reduced, ffc.halos_filled, ffc.data = grid, 3, 0, False, None
    pkg.lower(ffc * ffc)                       # no neighbour is read
    with pytest.raises(ValueError, match="halos are not filled"):
        pkg.lower(pkg.ddx(ffc))
    U = pkg.Field.__new__(pkg.ComputedField)
    U.grid, U.loc, U.reduced, U.halos_filled, U.data = grid, 1, 3, False, None
    assert U.location == (None, None, pkg.Center)
    assert (f["u"] - U).location == (pkg.Face, pkg.Center, pkg.Center)
    p = pkg.lower((f["u"] - U) * (f["u"] - U))
    assert len(p.loads) == 2
    pkg.lower(pkg.ddx(f["u"] - U))             # broadcast along x: no neighbour of U is read
    with pytest.raises(NotImplementedError, match="reduced"):
        pkg.lower(f["w"] - U)                  # interpolated along z, a direction it keeps
    with pytest.raises(NotImplementedError, match="reduced"):
        pkg.lower(pkg.ddz(U))
    with pytest.raises(ValueError, match="reduced along x"):
        pkg.ddx(U)


GRIDS_HOST = {
    "stretched": dict(size=(6, 5, 4), x=(0, 3), y=(0, 1), z=[-1.0, -0.6, -0.3, -0.1, 0.0], topology=(P, P, B)),
    "walls": dict(size=(4, 5, 3), x=(0, 1), y=(0, 2), z=(0, 1), topology=(B, B, B)),
    "flat": dict(size=(7, 5), x=(0, 1), z=(-1, 0), topology=(P, F, B)),
}


@pytest.mark.parametrize("gname", list(GRIDS_HOST))
def test_interpreted_program_is_bitwise_the_restatement(pkg, gname):
    grid = pkg.RectilinearGrid(None, **GRIDS_HOST[gname])
    parents = OC.random_parents(grid, 5)
    f, leaves, g = host_fields(pkg, grid, parents), OC.leaves(parents), ON.Grid(grid)
    for name, (tree, e) in OC.pointwise_cases(pkg, f).items():
        p = pkg.lower(tree)
        got = ON.interpret_program(p, [parents[[n for n in f if f[n] is q][0]] for q in p.fields], grid)
        loc, want = ON.pointwise(e, leaves, g)
        assert got.shape == want.shape and OC.mask_of(loc) == p.loc, (gname, name)
        assert np.array_equal(got, want, equal_nan=True), (gname, name)
    # the summands of the reductions, metric included
    for oname, (operand, e) in OC.reduction_operands(pkg, f).items():
        for dims in OC.DIMS:
            for kind in ("Average", "Integral"):
                p = pkg.lower(getattr(pkg, kind)(operand, dims=dims))
                got = ON.interpret_program(p, [parents[[n for n in f if f[n] is q][0]] for q in p.fields], grid)
                loc, t, W = ON.reduction_terms(kind, e, dims, leaves, g)
                assert np.array_equal(got, t), (gname, oname, dims, kind)
                d = pkg.operations._divisor(getattr(pkg, kind)(operand, dims=dims), p)
                assert abs(d - W) <= 2 * ON.EPS * W, (gname, oname, dims, kind, d, W)


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(HERE, "golden", "field_scans_2x2x2.json")))


@pytest.mark.parametrize("stretched", [False, True])
def test_restatement_reproduces_the_reference_test(pkg, golden, stretched):
    grid = OC.scans_grid(pkg, None, stretched)
    leaves, g = OC.leaves(OC.trilinear_parents(grid)), ON.Grid(grid)

    def value(kind, name, dims):
        loc, t, W = ON.reduction_terms(kind, ("f", name), dims, leaves, g)
        return ON.reduce_exact(t, dims, W)[0]
    OC.check_scans(golden, value)


def _program(pkg, **kw):
    """c[i + 1] + c[i]: LOAD, LOAD, ADD"""
    L = pkg._lib
    p = L.COpProgram()
    p.n_instructions, p.n_registers, p.n_fields, p.loc = 3, 2, 1, 0
    p.fields[0], p.field_loc[0], p.field_reduced[0] = 0x10000, 0, 0
    for q, (op, a, b, reg, di) in enumerate(((L.OP_LOAD, 0, 0, 0, 1), (L.OP_LOAD, 0, 0, 1, 0), (L.OP_ADD, 0, 1, 0, 0))):
        i = p.ins[q]
        i.opcode, i.a, i.b, i.reg, i.field, i.di = op, a, b, reg, 0, di
    for k, v in kw.items():
        q, name = k.split("_", 1)
        setattr(p.ins[int(q[1:])], name, v)
    return p


@pytest.mark.parametrize("what", list(OC.MALFORMED))
def test_malformed_programs_are_error_codes(pkg, what):
    """host checks of ocn_op_compute / ocn_op_reduce: they return before anything touches a device, so fake pointers do"""
    L = pkg._lib
    grid = L.CGrid(Nx=8, Ny=8, Nz=8, Hx=3, Hy=3, Hz=3, tx=0, ty=0, tz=1, math=0, dx=1.0, dy=1.0, dz=1.0, Lx=8.0, Ly=8.0, Lz=8.0)
    change, message = OC.MALFORMED[what]
    p = _program(pkg, **change)
    assert L.lib().ocn_op_compute(C.byref(grid), C.byref(p), 0x20000, None) == -1
    assert message in L.lib().ocn_last_error().decode()
    assert L.lib().ocn_op_reduce(C.byref(grid), C.byref(p), 3, 1.0, 0x30000, 1 << 20, 0x20000, None) == -1
    assert message in L.lib().ocn_last_error().decode()


def test_other_argument_checks(pkg):
    L = pkg._lib
    grid = L.CGrid(Nx=8, Ny=8, Nz=8, Hx=3, Hy=3, Hz=3, tx=0, ty=0, tz=1, math=0, dx=1.0, dy=1.0, dz=1.0, Lx=8.0, Ly=8.0, Lz=8.0)
    good = _program(pkg)
    n = C.c_int64()
    L.call("ocn_op_reduce_workspace", C.byref(grid), 0, 7, C.byref(n))
    assert n.value >= 1
    with pytest.raises(pkg.OcnError, match="null output"):
        L.call("ocn_op_compute", C.byref(grid), C.byref(good), None, None)
    with pytest.raises(pkg.OcnError, match="workspace of 1 doubles"):
        L.call("ocn_op_reduce", C.byref(grid), C.byref(good), 7, 1.0, 0x30000, 1, 0x20000, None)
    with pytest.raises(pkg.OcnError, match="dims mask"):
        L.call("ocn_op_reduce", C.byref(grid), C.byref(good), 8, 1.0, 0x30000, 1 << 20, 0x20000, None)
    with pytest.raises(pkg.OcnError, match="overwritten"):      # the register of an operand reused while it is live
        L.call("ocn_op_compute", C.byref(grid), C.byref(_program(pkg, i1_reg=0)), 0x20000, None)
    with pytest.raises(pkg.OcnError, match="instructions outside"):
        bad = _program(pkg)
        bad.n_instructions = 129
        L.call("ocn_op_compute", C.byref(grid), C.byref(bad), 0x20000, None)
    slab = L.CGrid.from_buffer_copy(grid)
    slab.tx = L.OCN_FULLY_CONNECTED
    with pytest.raises(pkg.OcnError, match="partitioned"):
        L.call("ocn_op_compute", C.byref(slab), C.byref(good), 0x20000, None)
