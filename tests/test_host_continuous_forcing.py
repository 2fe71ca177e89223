"""ContinuousForcing without a GPU: the constructor, the argument lists, every refusal (before anything is allocated), what the host folds,
what a new time changes in the lowered program, the lowered program interpreted on the CPU against the hand-written restatement
(tests/continuous_forcing_numpy.py), bit for bit, and the argument checks of ocn_op_accumulate (host code: nothing is launched)."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import continuous_forcing_numpy as CN

P, B, F = CN.P, CN.B, CN.F
INVALID = -1  # OCN_ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def pkg():
    import oceananigans_jl_amd as ocn
    return ocn


def _grid(pkg, gname="ppb", host_memory=False, **kw):
    g = pkg.RectilinearGrid(None, **dict(CN.GRIDS[gname], **kw))
    if host_memory:  # what the package asks of an architecture when it allocates: a torch device
        g.architecture = types.SimpleNamespace(device=torch.device("cpu"))
    return g


def host_fields(pkg, grid, parents):
    """fields of the package over host memory (tracing never touches the data)"""
    return {n: pkg.Field(CN.loc_of(n), grid, data=torch.from_numpy(np.ascontiguousarray(a.T))) for n, a in parents.items()}


def lower(pkg, value, grid, name, fields, time=0.0):
    from oceananigans_jl_amd.forcings import validate_forcing
    terms = validate_forcing({name: value}, grid, tuple(fields))[name]
    return pkg.forcing_programs.lower_forcing(terms, grid, name, fields, time)


# ---- the restatement's own min / max, pinned -------------------------------------------------------------------------------------------
def test_restatement_min_max_are_julias(pkg):
    nan, inf = np.nan, np.inf
    bits = lambda a: np.asarray(a, dtype=np.float64).view(np.int64)
    a = np.array([-0.0, 0.0, -0.0, 0.0, nan, 1.0, nan, -inf, inf, 2.0, -3.0])
    b = np.array([0.0, -0.0, -0.0, 0.0, 1.0, nan, nan, inf, -inf, 2.0, 5.0])
    assert np.array_equal(bits(CN.julia_max(a, b)), bits([0.0, 0.0, -0.0, 0.0, nan, nan, nan, inf, inf, 2.0, 5.0]))
    assert np.array_equal(bits(CN.julia_min(a, b)), bits([-0.0, -0.0, -0.0, 0.0, nan, nan, nan, -inf, -inf, 2.0, -3.0]))
    # ... and the package's host versions (used where the host folds a sub-tree) agree, bit pattern by bit pattern
    assert np.array_equal(bits(pkg.maximum(a, b)), bits(CN.julia_max(a, b)))
    assert np.array_equal(bits(pkg.minimum(a, b)), bits(CN.julia_min(a, b)))
    assert bits(pkg.maximum(-0.0, 0.0)) == bits(0.0) and bits(pkg.minimum(0.0, -0.0)) == bits(-0.0) and np.isnan(pkg.maximum(1.0, nan))


# ---- constructor and argument lists ----------------------------------------------------------------------------------------------------
def test_constructor(pkg):
    f = lambda x, y, z, t, u: -u
    assert pkg.ContinuousForcing(f, field_dependencies="u").field_dependencies == ("u",)
    assert pkg.ContinuousForcing(f, field_dependencies=("u", "T")).field_dependencies == ("u", "T")
    assert pkg.ContinuousForcing(f).field_dependencies == () and pkg.ContinuousForcing(f).parameters is None
    with pytest.raises(TypeError, match="callable"):
        pkg.ContinuousForcing(np.zeros(3))
    with pytest.raises(NotImplementedError, match=r"forcing.*discrete_form"):
        pkg.ContinuousForcing(lambda i, j, k, grid, clock, fields: 0.0, discrete_form=True)
    # the sampled Forcing still refuses dependencies, with its exception type and the word `forcing`, and now says where to go
    with pytest.raises(NotImplementedError, match=r"forcing.*ContinuousForcing"):
        pkg.Forcing(f, field_dependencies=("u",))


@pytest.mark.parametrize("spec,expect", [
    (dict(size=(6, 5, 4), x=(0, 1), y=(0, 1), z=(-1, 0), topology=(P, P, B), halo=(3, 3, 3)), [0, 1, 2]),
    (dict(size=(6, 4), x=(0, 1), z=(-1, 0), topology=(P, F, B), halo=(3, 3)), [0, 2]),
    (dict(size=(4,), z=(-1, 0), topology=(F, F, B), halo=(3,)), [2]),
])
def test_argument_lists(pkg, spec, expect):
    """func(X..., t, deps..., parameters): Flat directions omitted, the dependencies in the order given, the parameters last"""
    FP, BF = pkg.forcing_programs, pkg.boundary_functions
    grid = pkg.RectilinearGrid(None, **spec)
    f = host_fields(pkg, grid, CN.random_parents(grid, 3))
    seen = {}
    params = dict(a=1.0)

    def func(*args):
        seen["args"] = args
        return args[-2] * args[-1]["a"]
    for name in ("u", "w", "T"):
        p, _ = lower(pkg, pkg.ContinuousForcing(func, field_dependencies=("v", "T"), parameters=params), grid, name, f)
        args, loc = seen["args"], CN.loc_of(name)
        assert len(args) == len(expect) + 4 and args[-1] is params
        assert [(a.d, a.face) for a in args[:len(expect)]] == [(d, bool((loc >> d) & 1)) for d in expect]   # the field's OWN location
        assert isinstance(args[len(expect)], BF.Time)
        assert [a.field for a in args[len(expect) + 1:-1]] == [f["v"], f["T"]]
        assert p.fields == [f["T"]] and p.loc == loc
    # without parameters the list ends with the dependencies; without dependencies with the time
    lower(pkg, pkg.ContinuousForcing(lambda *a: seen.update(args=a) or 0.0, field_dependencies="u"), grid, "T", f)
    assert isinstance(seen["args"][-1], BF.Dependency) and len(seen["args"]) == len(expect) + 2
    lower(pkg, pkg.ContinuousForcing(lambda *a: seen.update(args=a) or 0.0), grid, "T", f)
    assert isinstance(seen["args"][-1], BF.Time) and len(seen["args"]) == len(expect) + 1


def test_dependencies_are_interpolated_to_the_forced_location(pkg):
    grid = _grid(pkg, "bbb")
    f = host_fields(pkg, grid, CN.random_parents(grid, 3))
    offsets = lambda p, leaf: sorted(i["off"] for i in p.loads if p.fields[i["field"]] is leaf)
    p, _ = lower(pkg, pkg.ContinuousForcing(lambda x, y, z, t, u: u, field_dependencies="u"), grid, "v", f)
    assert offsets(p, f["u"]) == [(0, -1, 0), (0, 0, 0), (1, -1, 0), (1, 0, 0)]                    # ℑxyᶜᶠᵃ
    p, _ = lower(pkg, pkg.ContinuousForcing(lambda x, y, z, t, T: T, field_dependencies="T"), grid, "w", f)
    assert offsets(p, f["T"]) == [(0, 0, -1), (0, 0, 0)]                                            # ℑzᵃᵃᶠ
    p, _ = lower(pkg, pkg.ContinuousForcing(lambda x, y, z, t, u: -0.5 * u, field_dependencies="u"), grid, "u", f)
    assert offsets(p, f["u"]) == [(0, 0, 0)] and [i["op"] for i in p.instructions] == [1, 0, 8]    # CONST, LOAD, MUL
    # the index space: the faces on the walls are no tendency cells
    assert p.index_range() == ((1, 11), (0, 9), (0, 7)) and p.interior_size() == (11, 10, 8)
    assert pkg.forcing_programs.tendency_index_range(grid, 4) == ((0, 11), (0, 9), (1, 7))
    assert pkg.forcing_programs.tendency_index_range(_grid(pkg, "ppb"), 1) == ((0, 69), (0, 12), (0, 4))


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_allocation(pkg, monkeypatch):
    import oceananigans_jl_amd.fields as fields

    def no_alloc(*a, **k):
        raise AssertionError("a field was allocated before the refusal")
    monkeypatch.setattr(fields.Field, "__init__", no_alloc)
    g = _grid(pkg, "short")
    dep = pkg.ContinuousForcing(lambda x, y, z, t, u: -u, field_dependencies="u")
    model = lambda forcing, grid=g, **kw: pkg.NonhydrostaticModel(grid, advection=pkg.WENO(), forcing=forcing, **kw)
    gd = _grid(pkg, "short")
    gd.architecture = types.SimpleNamespace(partition=object())
    with pytest.raises(NotImplementedError, match="forcing.*Distributed"):
        model({"u": dep}, grid=gd)
    with pytest.raises(NotImplementedError, match="forcing.*discrete_form"):
        model({"u": pkg.ContinuousForcing(lambda i, j, k, grid, clock, fields: 0.0, discrete_form=True)})
    for aux in ("νₑ", "κₑ", "pNHS"):
        with pytest.raises(NotImplementedError, match="forcing.*auxiliary"):
            model({"u": pkg.ContinuousForcing(lambda x, y, z, t, a: -a, field_dependencies=aux)})
    with pytest.raises(ValueError, match=r"\('u', 'S'\) are required to be model fields but only \('u', 'v', 'w', 'T'\) are present"):
        model({"T": pkg.ContinuousForcing(lambda x, y, z, t, u, S: u * S, field_dependencies=("u", "S"))}, tracers=("T",))
    with pytest.raises(NotImplementedError, match="forcing"):
        pkg.HydrostaticFreeSurfaceModel(g, forcing={"u": dep})
    with pytest.raises(NotImplementedError, match="forcing"):                          # MAX_TERMS = 4 stays
        model({"u": (dep,) * 5})
    # the drivers ask the model, not a device
    fake = types.SimpleNamespace(grid=g, _forcing_programs=[object()])
    for driver in (pkg.RK3Driver, pkg.ModelRK3Driver):
        with pytest.raises(NotImplementedError, match="ContinuousForcing.*Python host"):
            driver(fake)


def test_tracing_refusals(pkg):
    grid = _grid(pkg, "short")
    f = host_fields(pkg, grid, CN.random_parents(grid, 3))
    cf = lambda func, deps=("u",): pkg.ContinuousForcing(func, field_dependencies=deps)
    with pytest.raises(TypeError, match=r"ocn\.minimum / ocn\.maximum"):
        lower(pkg, cf(lambda x, y, z, t, u: u if z < -0.5 else 0.0), grid, "u", f)
    with pytest.raises(TypeError, match=r"ocn\.minimum / ocn\.maximum"):
        lower(pkg, cf(lambda x, y, z, t, u: u if u else 0.0), grid, "u", f)
    for name, fn in (("exp", pkg.exp), ("tanh", pkg.tanh), ("log", pkg.log), ("sin", np.sin), ("cos", pkg.cos)):
        with pytest.raises(NotImplementedError, match=name + r".*varies cell by cell"):           # of a field
            lower(pkg, cf(lambda x, y, z, t, u: fn(u * u)), grid, "u", f)
        with pytest.raises(NotImplementedError, match=name + r".*varies cell by cell.*two coordinate directions"):
            lower(pkg, cf(lambda x, y, z, t, u: fn(x + z) * u), grid, "u", f)
    with pytest.raises(TypeError, match="must return"):
        lower(pkg, cf(lambda x, y, z, t, u: "u"), grid, "u", f)
    with pytest.raises(NotImplementedError, match="device"):
        pkg.operations.log10(f["u"])
    # outside a forcing the host folds nothing: a diagnostics tree says so
    with pytest.raises(NotImplementedError, match="ContinuousForcing"):
        pkg.lower(pkg.exp(pkg.boundary_functions.Coordinate(grid, 2, False)) * f["T"])


# ---- folding ---------------------------------------------------------------------------------------------------------------------------
def test_folding_decisions(pkg):
    FP = pkg.forcing_programs
    grid = _grid(pkg, "ppb")
    f = host_fields(pkg, grid, CN.random_parents(grid, 3))
    ops = lambda p: [i["op"] for i in p.instructions]
    L = pkg._lib
    # sin(ω t) * u: ONE patched constant, no vector, no time instruction of its own
    p, _ = lower(pkg, pkg.ContinuousForcing(lambda x, y, z, t, u: pkg.sin(2.0 * t) * u, field_dependencies="u"), grid, "u", f, time=0.25)
    assert ops(p) == [L.OP_CONST, L.OP_LOAD, L.OP_MUL] and p.time_index is None and p.folded_vectors == [] and len(p.folded_constants) == 1
    assert p.instructions[0]["value"] == float(np.sin(np.float64(2.0) * np.float64(0.25)))
    # (μ₀ exp(z / λ) - m) * P: the LARGEST sub-tree without a field is one steady vector on the z nodes with halos
    p, _ = lower(pkg, CN.cases(pkg)["plankton"].terms(grid), grid, "b", f)
    assert ops(p) == [L.OP_LOAD, L.OP_LOAD, L.OP_MUL] and p.folded_constants == [] and p.time_index is None
    (v,) = p.folded_vectors
    z = np.ascontiguousarray(grid.nodes_1d(2, False, with_halos=True))
    assert (v.d, v.face, v.time_dependent, v.reduced) == (2, False, False, 3)
    assert np.array_equal(v.values, CN.PLANKTON["mu0"] * np.exp(z / CN.PLANKTON["lam"]) - CN.PLANKTON["m"])
    # sin(k x - ω t): a vector that reads the time
    p, _ = lower(pkg, pkg.ContinuousForcing(lambda x, y, z, t: pkg.sin(2.5 * x - 1.5 * t) * z + t), grid, "u", f, time=0.5)
    (v,) = p.folded_vectors
    assert (v.d, v.face, v.time_dependent) == (0, True, True) and p.time_index is not None and p.folded_constants == []
    assert np.array_equal(v.values, np.sin(2.5 * np.ascontiguousarray(grid.nodes_1d(0, True, with_halos=True)) - 1.5 * np.float64(0.5)))
    # no transcendental: nothing is folded, the device evaluates the coordinates and the time itself
    p, _ = lower(pkg, CN.cases(pkg)["coordinates"].terms(grid), grid, "T", f)
    assert p.folded_vectors == [] and p.folded_constants == [] and p.time_index is not None
    assert all(isinstance(x, pkg.boundary_functions.Coordinate) for x in p.fields)
    # a number alone is folded by Python while the function runs
    p, _ = lower(pkg, pkg.ContinuousForcing(lambda x, y, z, t: pkg.exp(0.0) * 3.0), grid, "T", f)
    assert ops(p) == [L.OP_CONST] and p.instructions[0]["value"] == 3.0


def test_a_new_time_changes_the_constants_and_the_vectors_only(pkg):
    grid = _grid(pkg, "ppb")
    f = host_fields(pkg, grid, CN.random_parents(grid, 3))

    def func(x, y, z, t, u):
        return np.sin(2.5 * x - 1.5 * t) * u + (np.cos(3.0 * t) * u) * np.exp(z) + t
    p, _ = lower(pkg, pkg.ContinuousForcing(func, field_dependencies="u"), grid, "u", f, time=0.0)
    steady = [v for v in p.folded_vectors if not v.time_dependent]
    moving = [v for v in p.folded_vectors if v.time_dependent]
    assert len(steady) == 1 and len(moving) == 1 and len(p.folded_constants) == 1 and p.time_index is not None
    before = [dict(i) for i in p.instructions]
    fields, n_registers = list(p.fields), p.n_registers
    kept, moved = steady[0].values.copy(), moving[0].values.copy()
    p.set_time(0.75)
    changed = [q for q, (a, b) in enumerate(zip(before, p.instructions)) if a != b]
    assert sorted(changed) == sorted(p.patched_instructions()) and len(changed) == 2
    assert len(p.instructions) == len(before) and p.fields == fields and p.n_registers == n_registers
    for q in changed:
        assert {k for k in before[q] if before[q][k] != p.instructions[q][k]} == {"value"}
    assert p.instructions[p.time_index]["value"] == 0.75
    assert p.instructions[p.folded_constants[0][0]]["value"] == float(np.cos(np.float64(3.0) * np.float64(0.75)))
    assert np.array_equal(steady[0].values, kept) and not np.array_equal(moving[0].values, moved)
    x = np.ascontiguousarray(grid.nodes_1d(0, True, with_halos=True))
    assert np.array_equal(moving[0].values, np.sin(2.5 * x - 1.5 * np.float64(0.75)))


# ---- the lowering against the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gname", list(CN.GRIDS))
def test_interpreted_program_is_bitwise_the_restatement(pkg, gname):
    """the lowering against the restatement without a device: the kernel test on the GPU then only has the interpreter left to check"""
    FP, BF = pkg.forcing_programs, pkg.boundary_functions
    grid = _grid(pkg, gname, host_memory=True)
    parents = CN.random_parents(grid, 7)
    parents["T"][grid.Hx + 1, grid.Hy, grid.Hz + 1] = -0.0
    f = host_fields(pkg, grid, parents)
    shape = lambda leaf: tuple(-1 if d == leaf.d else 1 for d in range(3))
    for cname, case in CN.cases(pkg).items():
        p, leaves = lower(pkg, case.terms(grid), grid, case.forced, f, time=-1.0)   # (traced at another time: the patch must take)
        p.set_time(0.375)

        def parents_of(leaf):
            if isinstance(leaf, BF.Coordinate):
                return leaf.nodes().reshape(shape(leaf))
            if isinstance(leaf, FP.Vector):
                return leaf.values.reshape(shape(leaf))
            for n in f:
                if f[n] is leaf:
                    return parents[n]
            return leaf.parent()
        got = CN.interpret(p, parents_of, grid)
        want = case.expected(grid, parents, 0.375)
        assert got.shape == want.shape and np.array_equal(got.view(np.int64), want.view(np.int64)), (gname, cname)


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
    f = lib.ocn_op_accumulate
    grid = L.CGrid(Nx=8, Ny=6, Nz=4, Hx=3, Hy=3, Hz=3, tx=0, ty=0, tz=1, math=0, dx=1.0, dy=1.0, dz=1.0, Lx=8.0, Ly=6.0, Lz=4.0)
    good, G = _program(pkg), C.c_void_p(0x20000)
    err = lambda: lib.ocn_last_error().decode()
    assert f(C.byref(grid), C.byref(good), None, None) == INVALID and "null tendency" in err()
    assert f(C.byref(grid), C.byref(good), C.c_void_p(0x10000), None) == INVALID and "is field 0 of the program" in err()
    assert f(None, C.byref(good), G, None) == INVALID and "null grid or program" in err()
    assert f(C.byref(grid), None, G, None) == INVALID and "null grid or program" in err()
    for opcode in (12, 17, -1):
        assert f(C.byref(grid), C.byref(_program(pkg, i2_opcode=opcode)), G, None) == INVALID and "unknown opcode" in err()
    assert f(C.byref(grid), C.byref(_program(pkg, i1_reg=0)), G, None) == INVALID and "overwritten" in err()
    assert f(C.byref(grid), C.byref(_program(pkg, i0_di=4)), G, None) == INVALID and "beyond the halo" in err()
    # offsets are checked against the TENDENCY cells: from the faces 2 .. N of w, k - 4 stays inside the parent array; from all N + 1
    # faces, which ocn_op_compute runs over, it leaves it
    reach = _program(pkg, i1_dk=-4)
    reach.loc = reach.field_loc[0] = 4
    assert lib.ocn_op_compute(C.byref(grid), C.byref(reach), G, None) == INVALID and "beyond the halo" in err()
    for change in (dict(i1_dk=-5), dict(i1_dk=5)):
        deeper = _program(pkg, **change)
        deeper.loc = deeper.field_loc[0] = 4
        assert f(C.byref(grid), C.byref(deeper), G, None) == INVALID and "beyond the halo" in err()
    slab = L.CGrid.from_buffer_copy(grid)
    slab.tx = L.OCN_FULLY_CONNECTED
    assert f(C.byref(slab), C.byref(good), G, None) == INVALID and "partitioned" in err()
    # the two new opcodes are binary: their operands are checked as those of ADD are
    assert f(C.byref(grid), C.byref(_program(pkg, i2_opcode=L.OP_MAX, i2_b=2)), G, None) == INVALID and "not an earlier instruction" in err()
    assert (L.OP_MIN, L.OP_MAX) == (10, 11) and "ocn_op_accumulate" in L.EXPORTED_SYMBOLS
