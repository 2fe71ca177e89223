"""Flux boundary conditions with field_dependencies without a GPU: the constructors and their refusals, the traced program (which fields
it loads, where, and the one patched CONST of the time), the refusals of the models, the argument checks of ocn_op_compute_boundary (host
code: nothing is launched) and the NumPy restatement of the tangential interpolation (tests/boundary_functions_numpy.py), pinned on
hand-computed values before anything else uses it and then compared bit for bit with the interpreted program."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import boundary_functions_numpy as BN

P, B, F = BN.P, BN.B, BN.F
INVALID = -1


@pytest.fixture(scope="module")
def pkg():
    import oceananigans_jl_amd as ocn
    return ocn


def _grid(pkg, gname="ppb", **kw):
    return pkg.RectilinearGrid(None, **dict(BN.GRIDS[gname], **kw))


def host_fields(pkg, grid, parents):
    """fields of the package over host memory (tracing never touches the data)"""
    return {n: pkg.Field(BN.loc_of(n), grid, data=torch.from_numpy(np.ascontiguousarray(a.T))) for n, a in parents.items()}


def drag_u(x, y, t, u, v, p):
    import oceananigans_jl_amd as ocn
    return -p["cd"] * ocn.sqrt(u ** 2 + v ** 2) * u


# ---- the restatement, pinned independently of its author ------------------------------------------------------------------------------
def test_restatement_of_the_interpolation_is_pinned(pkg):
    """v[i, j] = i + 10 j (the reference's 1-based indices, halos included).  By hand:
      v at u points, ℑxyᶠᶜᵃ = ¼ (v[i-1, j] + v[i, j] + v[i-1, j+1] + v[i, j+1]) = (i - ½) + 10 (j + ½) = i + 10 j + 4.5
      u at v points, ℑxyᶜᶠᵃ = (i + ½) + 10 (j - ½)                                                       = i + 10 j - 4.5
      a tracer at u points, ℑxᶠᵃᵃ = ½ (c[i-1, j] + c[i, j])                                              = i + 10 j - 0.5
      w at a tracer point on bottom / top: the identity at k = 1 / k = Nz (NOT Nz + 1), whatever w's location along z
    all exactly representable, so the comparison is exact.  The nesting of a double interpolation is pinned separately."""
    grid = _grid(pkg)
    Hx, Hy, Hz = grid.Hx, grid.Hy, grid.Hz
    i1 = np.arange(1, grid.Nx + 1).reshape(-1, 1)
    j1 = np.arange(1, grid.Ny + 1).reshape(1, -1)

    def linear(loc):
        sx, sy, sz = grid.parent_shape(loc)
        i = (np.arange(sx) - Hx + 1).reshape(-1, 1, 1)
        j = (np.arange(sy) - Hy + 1).reshape(1, -1, 1)
        k = (np.arange(sz) - Hz + 1).reshape(1, 1, -1)
        return i + 10.0 * j + 1000.0 * k
    for side, k in (("bottom", 1), ("top", grid.Nz)):
        assert np.array_equal(BN.interpolated(linear(2), 2, 1, grid, side), i1 + 10.0 * j1 + 4.5 + 1000.0 * k)
        assert np.array_equal(BN.interpolated(linear(1), 1, 2, grid, side), i1 + 10.0 * j1 - 4.5 + 1000.0 * k)
        assert np.array_equal(BN.interpolated(linear(0), 0, 1, grid, side), i1 + 10.0 * j1 - 0.5 + 1000.0 * k)
        assert np.array_equal(BN.interpolated(linear(4), 4, 0, grid, side), i1 + 10.0 * j1 + 1000.0 * k)
        assert np.array_equal(BN.interpolated(linear(1), 1, 1, grid, side), i1 + 10.0 * j1 + 1000.0 * k)
    # lateral sides of a box with walls: u at a tracer point on the south side is ℑxᶜᵃᵃ = ½ (u[i, 1, k] + u[i+1, 1, k]); on north j = Ny
    box = _grid(pkg, "bbb")
    ib, kb = np.arange(1, box.Nx + 1).reshape(-1, 1), np.arange(1, box.Nz + 1).reshape(1, -1)

    def linear_box(loc):
        sx, sy, sz = box.parent_shape(loc)
        i = (np.arange(sx) - box.Hx + 1).reshape(-1, 1, 1)
        j = (np.arange(sy) - box.Hy + 1).reshape(1, -1, 1)
        k = (np.arange(sz) - box.Hz + 1).reshape(1, 1, -1)
        return i + 10.0 * j + 1000.0 * k
    assert np.array_equal(BN.interpolated(linear_box(1), 1, 0, box, "south"), ib + 0.5 + 10.0 + 1000.0 * kb)
    assert np.array_equal(BN.interpolated(linear_box(1), 1, 0, box, "north"), ib + 0.5 + 10.0 * box.Ny + 1000.0 * kb)
    # w at a v point on the west side: ℑyzᵃᶠᶜ = ℑz(ℑy): (j - ½) and (k + ½), at i = 1; on east at i = Nx
    jb = np.arange(1, box.Ny + 1).reshape(-1, 1)
    assert np.array_equal(BN.interpolated(linear_box(4), 4, 2, box, "west"), 1 + 10.0 * (jb - 0.5) + 1000.0 * (kb + 0.5))
    assert np.array_equal(BN.interpolated(linear_box(4), 4, 2, box, "east"), box.Nx + 10.0 * (jb - 0.5) + 1000.0 * (kb + 0.5))


def test_restatement_nests_x_inside_y(pkg):
    """ℑxyᶠᶜᵃ = ℑyᵃᶜᵃ(ℑxᶠᵃᵃ) (interpolation_operators.jl:46): with v[i-1, j] = 1, v[i, j] = 2⁻⁵³, v[i-1, j+1] = -1, v[i, j+1] = 2⁻⁵³
      x inside:  ½ (½ (1 + 2⁻⁵³) + ½ (-1 + 2⁻⁵³)) = ½ (½ + (-½ + 2⁻⁵⁴)) = 2⁻⁵⁵      (1 + 2⁻⁵³ rounds to 1)
      y inside:  ½ (½ (1 - 1) + ½ (2⁻⁵³ + 2⁻⁵³))  = 2⁻⁵⁴"""
    grid = _grid(pkg)
    v = np.zeros(grid.parent_shape(2))
    i, j, k = grid.Hx + 2, grid.Hy + 1, grid.Hz  # 0-based parent indices of the u point (i = 3, j = 2, k = 1)
    v[i - 1, j, k], v[i, j, k], v[i - 1, j + 1, k], v[i, j + 1, k] = 1.0, 2.0 ** -53, -1.0, 2.0 ** -53
    got = BN.interpolated(v, 2, 1, grid, "bottom")
    assert got[2, 1] == 2.0 ** -55


# ---- constructors ----------------------------------------------------------------------------------------------------------------------
def test_constructor_and_its_refusals(pkg):
    bc = pkg.FluxBoundaryCondition(drag_u, field_dependencies=("u", "v"), parameters=dict(cd=1e-3))
    assert bc.field_dependencies == ("u", "v") and bc.func is drag_u and bc.kind == pkg._lib.BC_FLUX
    assert pkg.FluxBoundaryCondition(lambda x, y, t, u: -u, field_dependencies="u").field_dependencies == ("u",)
    # an empty field_dependencies keeps the host-sampled path
    plain = pkg.FluxBoundaryCondition(lambda x, y, t: x + y)
    assert plain.field_dependencies == () and plain.func is not None
    assert pkg.FluxBoundaryCondition(1.5, coeff=-2.0).field_dependencies == ()
    with pytest.raises(ValueError, match="coeff"):
        pkg.FluxBoundaryCondition(lambda x, y, t, u: -u, coeff=-1.0, field_dependencies="u")
    with pytest.raises(TypeError, match="function"):
        pkg.FluxBoundaryCondition(1.0, field_dependencies="u")
    with pytest.raises(NotImplementedError, match=r"discrete_form.*DESIGN\.md"):
        pkg.FluxBoundaryCondition(lambda i, j, grid, clock, fields: 0.0, discrete_form=True)
    for ctor in (pkg.ValueBoundaryCondition, pkg.GradientBoundaryCondition, pkg.OpenBoundaryCondition):
        with pytest.raises(NotImplementedError, match=r"field_dependencies.*halo fills.*DESIGN\.md"):
            ctor(lambda x, y, t, u: u, field_dependencies="u")
        with pytest.raises(NotImplementedError, match="discrete_form"):
            ctor(lambda i, j, grid, clock, fields: 0.0, discrete_form=True)
        assert ctor(2.0).field_dependencies == ()


def test_sqrt_and_abs_take_numpy_arrays(pkg):
    a = np.array([4.0, 9.0, -1.0])
    with np.errstate(invalid="ignore"):
        assert np.array_equal(pkg.sqrt(a), np.sqrt(a), equal_nan=True)
    assert np.array_equal(pkg.abs(a), np.abs(a))
    assert pkg.sqrt(4.0) == 2.0 and isinstance(pkg.sqrt(4.0), float) and pkg.abs(-3) == 3.0


# ---- tracing ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(pkg):
    grid = _grid(pkg)
    parents = BN.random_parents(grid, 3)
    return grid, parents, host_fields(pkg, grid, parents)


def test_traced_drag_loads_u_once_and_v_at_four_points(pkg, small):
    grid, parents, f = small
    L = pkg._lib
    bc = pkg.FluxBoundaryCondition(drag_u, field_dependencies=("u", "v"), parameters=dict(cd=2.5e-3))
    for side, I in (("bottom", 1), ("top", grid.Nz)):
        p = pkg.boundary_functions.trace(bc, grid, 1, side, f)
        assert isinstance(p, pkg.BoundaryProgram) and p.loc == 1 and p.side == side
        assert [i["off"] for i in p.loads if p.fields[i["field"]] is f["u"]] == [(0, 0, 0)]
        assert sorted(i["off"] for i in p.loads if p.fields[i["field"]] is f["v"]) == [(-1, 0, 0), (-1, 1, 0), (0, 0, 0), (0, 1, 0)]  # ℑxyᶠᶜᵃ
        assert len(p.fields) == 2 and p.time_index is None            # x, y and t are not used: no leaf for them
        assert p.index_range() == ((0, grid.Nx - 1), (0, grid.Ny - 1), (I - 1, I - 1))
        assert p.interior_size() == (grid.Nx, grid.Ny, 1)
        assert all(0 <= i["reg"] < p.n_registers for i in p.instructions) and p.n_registers <= 8
        c = p.c_struct()
        assert c.n_fields == 2 and c.loc == 1 and c.n_instructions == len(p.instructions)
        assert sorted((c.ins[q].di, c.ins[q].dj, c.ins[q].dk) for q in range(c.n_instructions) if c.ins[q].opcode == L.OP_LOAD) == \
            sorted(i["off"] for i in p.loads)


def test_time_is_one_patched_const(pkg, small):
    grid, parents, f = small
    L = pkg._lib
    bc = pkg.FluxBoundaryCondition(lambda x, y, t, u: -(1 + t) * u + 0.0 * t, field_dependencies="u")
    p1 = pkg.boundary_functions.trace(bc, grid, 1, "bottom", f, time=0.25)
    p2 = pkg.boundary_functions.trace(bc, grid, 1, "bottom", f, time=7.0)
    q = p1.time_index
    assert q is not None and q == p2.time_index
    assert p1.instructions[q]["op"] == L.OP_CONST and p1.instructions[q]["value"] == 0.25 and p2.instructions[q]["value"] == 7.0
    assert sum(1 for i in p1.instructions if i.get("time")) == 1     # used twice, lowered once
    strip = lambda p: [dict(i, value=None) if n == q else i for n, i in enumerate(p.instructions)]
    assert strip(p1) == strip(p2)                                    # the two programs differ in that one value only
    # a constant equal to the time is NOT merged with it: patching the time must not change the constant
    bc1 = pkg.FluxBoundaryCondition(lambda x, y, t, u: (u * 1.0) * t, field_dependencies="u")
    p = pkg.boundary_functions.trace(bc1, grid, 1, "bottom", f, time=1.0)
    consts = [n for n, i in enumerate(p.instructions) if i["op"] == L.OP_CONST]
    assert len(consts) == 2 and p.time_index in consts
    # a plain number is a constant program; a function that ignores t has no time instruction
    p0 = pkg.boundary_functions.trace(pkg.FluxBoundaryCondition(lambda x, y, t, u: 1.5, field_dependencies="u"), grid, 1, "bottom", f)
    assert len(p0.instructions) == 1 and p0.instructions[0]["op"] == L.OP_CONST and p0.instructions[0]["value"] == 1.5 and p0.time_index is None


def test_signature_coordinates_and_parameters(pkg, small):
    grid, parents, f = small
    seen = {}

    def func(*args):
        seen["args"] = args
        return args[0] * args[2] + args[1] - args[3]
    marker = object()
    BF = pkg.boundary_functions
    BF.trace(pkg.FluxBoundaryCondition(func, field_dependencies=("w",), parameters=marker), grid, 0, "top", f)
    x, y, t, w, p = seen["args"]
    assert p is marker                                               # passed through untouched
    assert isinstance(x, BF.Coordinate) and (x.d, x.face) == (0, False) and isinstance(y, BF.Coordinate) and (y.d, y.face) == (1, False)
    assert isinstance(t, BF.Time) and isinstance(w, BF.Dependency) and w.location == (pkg.Center, pkg.Center, None)
    assert np.array_equal(x.nodes()[grid.Hx:grid.Hx + grid.Nx], grid.nodes_1d(0, False)) and x.nodes().size == grid.parent_shape(0)[0]
    # the coordinates are taken at the field's own location: x at Faces for u
    BF.trace(pkg.FluxBoundaryCondition(func, field_dependencies=("w",)), grid, 1, "bottom", f)
    assert len(seen["args"]) == 4 and seen["args"][0].face and not seen["args"][1].face
    # west / east: (y, z); south / north: (x, z)
    box = _grid(pkg, "bbb")
    fb = host_fields(pkg, box, BN.random_parents(box, 1))
    BF.trace(pkg.FluxBoundaryCondition(func, field_dependencies=("w",)), box, 0, "west", fb)
    assert [(a.d, a.face) for a in seen["args"][:2]] == [(1, False), (2, False)]
    BF.trace(pkg.FluxBoundaryCondition(func, field_dependencies=("w",)), box, 4, "north", fb)
    assert [(a.d, a.face) for a in seen["args"][:2]] == [(0, False), (2, True)]
    # a Flat direction's coordinate is left out: the tilted-boundary-layer example's drag_u(x, t, u, v, p) as written
    flat = _grid(pkg, "pfb")
    ff = host_fields(pkg, flat, BN.random_parents(flat, 1))

    def drag(x, t, u, v, p):
        return -p["cd"] * pkg.sqrt(u ** 2 + (v + p["V"]) ** 2) * u
    pr = BF.trace(pkg.FluxBoundaryCondition(drag, field_dependencies=("u", "v"), parameters=dict(cd=1e-3, V=0.1)), flat, 1, "bottom", ff)
    assert sorted(i["off"] for i in pr.loads if pr.fields[i["field"]] is ff["v"]) == [(-1, 0, 0), (0, 0, 0)]   # ℑxᶠᵃᵃ only: y is Flat


def test_tracing_refusals(pkg, small):
    grid, parents, f = small
    trace = pkg.boundary_functions.trace
    mk = lambda func, deps="u": pkg.FluxBoundaryCondition(func, field_dependencies=deps)
    with pytest.raises(TypeError, match="field_dependencies"):
        trace(mk(lambda x, y, t, u: u if u > 0 else 0.0), grid, 1, "bottom", f)
    with pytest.raises(TypeError, match="field_dependencies"):
        trace(mk(lambda x, y, t, u: u if u * u else 0.0), grid, 1, "bottom", f)
    with pytest.raises(NotImplementedError, match="only sqrt and abs"):
        trace(mk(lambda x, y, t, u: pkg.exp(u)), grid, 1, "bottom", f)
    with pytest.raises(NotImplementedError, match="use sqrt"):
        trace(mk(lambda x, y, t, u: u ** 0.5), grid, 1, "bottom", f)
    with pytest.raises(ValueError, match=r"\('u', 'q'\) are required to be model fields but only \('u', 'v', 'w', 'T'\) are present"):
        trace(mk(lambda x, y, t, u, q: u, ("u", "q")), grid, 1, "bottom", f)
    with pytest.raises(TypeError, match="must return"):
        trace(mk(lambda x, y, t, u: "u"), grid, 1, "bottom", f)
    # over the limits: raised when the function is traced, that is at model construction

    def long(x, y, t, u, v):
        e = u * v
        for n in range(70):
            e = e * float(n + 2) + v
        return e
    with pytest.raises(ValueError, match="OCN_OP_MAX_INSTRUCTIONS = 128"):
        trace(mk(long, ("u", "v")), grid, 1, "bottom", f)

    def wide(x, y, t, u):
        terms = [u * float(n + 2) for n in range(20)]
        e = terms[-1]
        for s in reversed(terms[:-1]):
            e = s / e
        return e
    with pytest.raises(ValueError, match="OCN_OP_MAX_REGISTERS = 16"):
        trace(mk(wide), grid, 1, "bottom", f)
    many = dict(f, **{f"c{n}": pkg.Field(0, grid, data=f["T"].data) for n in range(8)})
    names = tuple(f"c{n}" for n in range(8)) + ("T",)
    with pytest.raises(ValueError, match="OCN_OP_MAX_FIELDS = 8"):
        trace(mk(lambda x, y, t, *c: sum(c[1:], c[0]), names), grid, 0, "bottom", many)
    # a tangential derivative reaches one cell further; beyond the halo it is refused here, as the library would
    thin = _grid(pkg, halo=(1, 1, 1))
    ft = host_fields(pkg, thin, BN.random_parents(thin, 1))
    trace(mk(lambda x, y, t, u: pkg.ddx(u)), thin, 1, "bottom", ft)
    with pytest.raises(ValueError, match="halo"):
        trace(mk(lambda x, y, t, u: pkg.ddx(pkg.ddx(pkg.ddx(u)))), thin, 1, "bottom", ft)


@pytest.mark.parametrize("gname", list(BN.GRIDS))
def test_interpreted_program_is_bitwise_the_restatement(pkg, gname):
    """the lowering against the restatement without a device: the kernel test on the GPU then only has the interpreter left to check"""
    grid = _grid(pkg, gname)
    parents = BN.random_parents(grid, 7)
    f = host_fields(pkg, grid, parents)
    BF = pkg.boundary_functions

    def parents_of(leaf):
        if isinstance(leaf, BF.Coordinate):
            return leaf.nodes().reshape(tuple(-1 if d == leaf.d else 1 for d in range(3)))
        return parents[[n for n in f if f[n] is leaf][0]]
    for side in BN.GRID_SIDES[gname]:
        for fname, (name, func, deps, params) in BN.functions_on(pkg, grid, side).items():
            bc = pkg.FluxBoundaryCondition(func, field_dependencies=deps, parameters=params)
            p = BF.trace(bc, grid, BN.loc_of(name), side, f, time=0.375)
            got = BN.interpret(p, parents_of, grid)
            want = BN.expected(func, grid, name, side, parents, deps, params, 0.375)
            assert got.shape == want.shape and np.array_equal(got, want, equal_nan=True), (gname, side, fname)


# ---- models ----------------------------------------------------------------------------------------------------------------------------
def test_model_refusals_before_anything_is_allocated(pkg):
    """grids without an architecture: whatever these constructors raised after allocating a field would be another error"""
    grid = _grid(pkg)
    dep = pkg.FluxBoundaryCondition(lambda x, y, t, u: -u, field_dependencies="u")
    bcs = {"u": pkg.FieldBoundaryConditions(bottom=dep)}
    with pytest.raises(NotImplementedError, match="field_dependencies"):
        pkg.HydrostaticFreeSurfaceModel(grid, boundary_conditions=bcs)
    dist = _grid(pkg)
    dist.architecture = types.SimpleNamespace(partition=object())
    with pytest.raises(NotImplementedError, match="Distributed"):
        pkg.NonhydrostaticModel(dist, advection=pkg.WENO(), boundary_conditions=bcs)
    with pytest.raises(ValueError, match=r"\('u', 'S'\) are required to be model fields but only \('u', 'v', 'w', 'T'\) are present"):
        pkg.NonhydrostaticModel(grid, advection=pkg.WENO(), tracers=("T",), boundary_conditions={
            "T": pkg.FieldBoundaryConditions(top=pkg.FluxBoundaryCondition(lambda x, y, t, u, S: u * S, field_dependencies=("u", "S")))})
    for key, value in (("νₑ", pkg.FieldBoundaryConditions(bottom=dep)), ("κₑ", {"T": pkg.FieldBoundaryConditions(bottom=dep)})):
        with pytest.raises(NotImplementedError, match=r"field_dependencies.*DESIGN\.md"):
            pkg.NonhydrostaticModel(grid, advection=pkg.WENO(), tracers=("T",), closure=pkg.AnisotropicMinimumDissipation(),
                                    boundary_conditions={key: value})
    # a condition on a Periodic side keeps the reference's wording
    with pytest.raises(ValueError, match="Cannot set west boundary condition"):
        pkg.NonhydrostaticModel(grid, advection=pkg.WENO(), boundary_conditions={"v": pkg.FieldBoundaryConditions(west=dep)})


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def _program(pkg, **kw):
    """c[i + 1, j, k] + c[i, j - 1, k + 1]: LOAD, LOAD, ADD"""
    L = pkg._lib
    p = L.COpProgram()
    p.n_instructions, p.n_registers, p.n_fields, p.loc = 3, 2, 1, 0
    p.fields[0], p.field_loc[0], p.field_reduced[0] = 0x10000, 0, 0
    for q, (op, a, b, reg, off) in enumerate(((L.OP_LOAD, 0, 0, 0, (1, 0, 0)), (L.OP_LOAD, 0, 0, 1, (0, -1, 1)), (L.OP_ADD, 0, 1, 0, (0, 0, 0)))):
        i = p.ins[q]
        i.opcode, i.a, i.b, i.reg, i.field, (i.di, i.dj, i.dk) = op, a, b, reg, 0, off
    for k, v in kw.items():
        q, name = k.split("_", 1)
        setattr(p.ins[int(q[1:])], name, v)
    return p


def test_c_abi_argument_checks_touch_no_device(pkg):
    """OCN_ERR_INVALID_ARGUMENT before any HIP call: runs on a machine without a GPU; the pointers are never dereferenced"""
    L = pkg._lib
    lib = L.lib()
    f = lib.ocn_op_compute_boundary
    grid = L.CGrid(Nx=8, Ny=6, Nz=4, Hx=3, Hy=3, Hz=3, tx=0, ty=0, tz=1, math=0, dx=1.0, dy=1.0, dz=1.0, Lx=8.0, Ly=6.0, Lz=4.0)
    good, values = _program(pkg), C.c_void_p(0x20000)
    err = lambda: lib.ocn_last_error().decode()
    for side in (-1, 6, 100):
        assert f(C.byref(grid), C.byref(good), side, values, None) == INVALID and "outside 0..5" in err()
    for side in (0, 1, 2, 3):  # west .. north of a grid that is Periodic in x and y
        assert f(C.byref(grid), C.byref(good), side, values, None) == INVALID and "not Bounded" in err()
    flat = L.CGrid(Nx=8, Ny=1, Nz=4, Hx=3, Hy=0, Hz=3, tx=0, ty=2, tz=1, math=0, dx=1.0, dy=1.0, dz=1.0, Lx=8.0, Ly=1.0, Lz=4.0)
    assert f(C.byref(flat), C.byref(_program(pkg, i1_dj=0)), 2, values, None) == INVALID and "not Bounded" in err()
    assert f(None, C.byref(good), 4, values, None) == INVALID and "null grid or program" in err()
    assert f(C.byref(grid), None, 4, values, None) == INVALID and "null grid or program" in err()
    assert f(C.byref(grid), C.byref(good), 4, None, None) == INVALID and "null values" in err()
    nofield = _program(pkg)
    nofield.fields[0] = None
    assert f(C.byref(grid), C.byref(nofield), 4, values, None) == INVALID and "null pointer" in err()
    # offsets are checked against the PLANE, at its normal index: k + 4 leaves the parent from k = Nz (top), k - 4 from k = 1 (bottom)
    # (the accepting half -- k + 4 from the bottom plane, which no program over the volume may read -- needs a device: the GPU tests)
    reach = _program(pkg, i1_dk=4)
    assert f(C.byref(grid), C.byref(reach), 5, values, None) == INVALID and "beyond the halo" in err()
    down = _program(pkg, i1_dk=-4)
    assert f(C.byref(grid), C.byref(down), 4, values, None) == INVALID and "beyond the halo" in err()
    # ... and along the tangential directions against all N points
    for change in (dict(i0_di=4), dict(i1_dj=-4), dict(i0_di=-4)):
        assert f(C.byref(grid), C.byref(_program(pkg, **change)), 4, values, None) == INVALID and "beyond the halo" in err()
    # the checks of every ocn_op_* entry hold here too
    assert f(C.byref(grid), C.byref(_program(pkg, i1_reg=0)), 4, values, None) == INVALID and "overwritten" in err()
    assert f(C.byref(grid), C.byref(_program(pkg, i2_opcode=17)), 4, values, None) == INVALID and "unknown opcode" in err()
    slab = L.CGrid.from_buffer_copy(grid)
    slab.tx = L.OCN_FULLY_CONNECTED
    assert f(C.byref(slab), C.byref(good), 4, values, None) == INVALID and "partitioned" in err()
    assert "ocn_op_compute_boundary" in L.EXPORTED_SYMBOLS
