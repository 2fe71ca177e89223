"""Flux boundary conditions with field_dependencies on the device.

1. The evaluation kernel against the NumPy restatement (tests/boundary_functions_numpy.py, pinned by the host tests), bit for bit: + - * /
   sqrt are correctly rounded on both sides and the kernel is built without FMA contraction.  Fields are seeded random over their WHOLE
   parent arrays and no halo fill is called, so a wrong offset or a wrong boundary-normal index shows.
2. Nothing but values[0 .. n1 n2 - 1] is written, and two calls give the same bits.
3.-5. Models: a linear drag written as a function of u against the same drag written as `coeff`; a model with drag laws against a twin
   with array-valued conditions that this test drives through the exported unfused functions, evaluating the functions itself after
   every halo fill; the same with a function of the time, whose three RK3 stage times differ.  All bit for bit.
6. A known answer after one Euler step.  7. What refuses."""
import ctypes as C

import numpy as np
import pytest
import torch

import boundary_functions_numpy as BN

pytestmark = pytest.mark.gpu
SENTINEL = -7.25e300
EPS = 2.0 ** -52


def device_fields(ocn, grid, parents):
    f = {}
    for n, a in parents.items():
        f[n] = ocn.Field(BN.loc_of(n), grid)
        f[n].data.copy_(torch.from_numpy(np.ascontiguousarray(a.T)))
    return f


def evaluate_into(ocn, bf, time, pointer):
    """ocn_op_compute_boundary of a traced condition into the device array at `pointer`"""
    c, p = bf._c, bf.program
    for q, f in enumerate(p.fields):
        c.fields[q] = f.ptr
    if p.time_index is not None:
        c.ins[p.time_index].value = float(time)
    ocn._lib.call("ocn_op_compute_boundary", bf.grid.cref, C.byref(c), BN.SIDES.index(bf.side), pointer, ocn.architectures.stream_ptr())


_setups = {}


@pytest.fixture(scope="module")
def setup(ocn):
    def get(gname):
        if gname not in _setups:
            grid = ocn.RectilinearGrid(ocn.GPU(), **BN.GRIDS[gname])
            parents = BN.random_parents(grid, 11 + list(BN.GRIDS).index(gname))
            _setups[gname] = (grid, parents, device_fields(ocn, grid, parents))
        return _setups[gname]
    yield get
    _setups.clear()


# ---- 1. kernel parity --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gname,side", [(g, s) for g in BN.GRIDS for s in BN.GRID_SIDES[g]])
def test_kernel_is_bitwise_the_restatement(ocn, setup, gname, side):
    grid, parents, f = setup(gname)
    time = 0.375
    for fname, (name, func, deps, params) in BN.functions_on(ocn, grid, side).items():
        bc = ocn.FluxBoundaryCondition(func, field_dependencies=deps, parameters=params)
        bf = ocn.BoundaryFunction(bc, grid, BN.loc_of(name), side, f, time=-1.0)  # (traced with another time: the patch must take)
        bf.compute(time)
        got = bc._device_values.cpu().numpy().T
        want = BN.expected(func, grid, name, side, parents, deps, params, time)
        assert got.shape == want.shape, (gname, side, fname)
        assert np.array_equal(got, want, equal_nan=True), (gname, side, fname, float(np.nanmax(np.abs(got - want))))
        if fname == "coords":  # the time is current at every call, with nothing traced again
            program = bf.program
            bf.compute(2.0)
            assert bf.program is program
            assert np.array_equal(bc._device_values.cpu().numpy().T, BN.expected(func, grid, name, side, parents, deps, params, 2.0))


# ---- 2. nothing else is written ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gname,side", [("ppb", "top"), ("bbb", "west"), ("bbb", "north")])
def test_nothing_else_is_written(ocn, setup, gname, side):
    grid, parents, f = setup(gname)
    name, func, deps, params = BN.functions_on(ocn, grid, side)["bulk"]
    bf = ocn.BoundaryFunction(ocn.FluxBoundaryCondition(func, field_dependencies=deps, parameters=params), grid, BN.loc_of(name), side, f)
    d1, d2 = BN.tangential(side)
    n = grid.size[d1] * grid.size[d2]
    out = [torch.full((n + 64,), SENTINEL, dtype=torch.float64, device="cuda") for _ in range(2)]
    for o in out:
        evaluate_into(ocn, bf, 0.5, o.data_ptr())
    a, b = (o.cpu().numpy() for o in out)
    want = BN.expected(func, grid, name, side, parents, deps, params, 0.5)
    assert np.array_equal(a[:n].reshape(grid.size[d2], grid.size[d1]).T, want)
    assert np.all(a[n:] == SENTINEL)
    assert np.array_equal(a, b)                                       # two calls, identical bits
    for fname, field in f.items():
        assert np.array_equal(field.parent(), parents[fname]), fname  # every field parent is unchanged


def test_offsets_are_validated_against_the_plane(ocn, setup):
    """c[i, j, k + 4]: from the bottom plane (k = 1) of a grid with Nz = 4, Hz = 3 that is inside the parent array, so the boundary entry
    takes it and reads the right element; over the volume it would leave the array at k = Nz, and ocn_op_compute refuses it"""
    grid, parents, f = setup("ppb")
    L = ocn._lib
    p = L.COpProgram()
    p.n_instructions, p.n_registers, p.n_fields, p.loc = 1, 1, 1, 0
    p.fields[0], p.field_loc[0] = f["T"].ptr, 0
    p.ins[0].opcode, p.ins[0].dk = L.OP_LOAD, 4
    out = torch.full((grid.Nx * grid.Ny,), SENTINEL, dtype=torch.float64, device="cuda")
    with pytest.raises(ocn.OcnError, match="beyond the halo"):
        L.call("ocn_op_compute", grid.cref, C.byref(p), out.data_ptr(), None)
    with pytest.raises(ocn.OcnError, match="beyond the halo"):
        L.call("ocn_op_compute_boundary", grid.cref, C.byref(p), 5, out.data_ptr(), ocn.architectures.stream_ptr())
    L.call("ocn_op_compute_boundary", grid.cref, C.byref(p), 4, out.data_ptr(), ocn.architectures.stream_ptr())
    want = parents["T"][grid.Hx:grid.Hx + grid.Nx, grid.Hy:grid.Hy + grid.Ny, grid.Hz + 4]
    assert np.array_equal(out.cpu().numpy().reshape(grid.Ny, grid.Nx).T, want)


# ---- models ------------------------------------------------------------------------------------------------------------------------------
MODEL_GRID = dict(size=(8, 6, 4), x=(0, 3), y=(0, 1), z=BN.STRETCHED_Z, topology=(BN.P, BN.P, BN.B), halo=(3, 3, 3))
DT = 2.0e-3


def initial_state(grid, seed=5):
    rng = np.random.default_rng(seed)
    return dict(u=rng.uniform(-1, 1, (grid.Nx, grid.Ny, grid.Nz)), v=rng.uniform(-1, 1, (grid.Nx, grid.Ny, grid.Nz)),
                w=rng.uniform(-1, 1, (grid.Nx, grid.Ny, grid.Nz + 1)), T=rng.uniform(0, 1, (grid.Nx, grid.Ny, grid.Nz)))


def build(ocn, boundary_conditions, timestepper="RungeKutta3", monkeypatch=None):
    if monkeypatch is not None:  # the switch that gives a model of the general fused path the reference's launch sequence
        monkeypatch.setenv("OCN_FUSE_GENERAL", "0")
    grid = ocn.RectilinearGrid(ocn.GPU(), **MODEL_GRID)
    model = ocn.NonhydrostaticModel(grid, advection=ocn.WENO(), tracers=("T",), closure=ocn.ScalarDiffusivity(nu=1e-2, kappa=2e-2),
                                    timestepper=timestepper, boundary_conditions=boundary_conditions, math_mode=ocn.MATH_STRICT)
    if monkeypatch is not None:
        monkeypatch.delenv("OCN_FUSE_GENERAL")
    ocn.set(model, **initial_state(model.grid))
    return model


def assert_same_state(ocn, a, b, what):
    ocn.flush_tendencies(a)
    ocn.flush_tendencies(b)
    ocn.sync_device()
    for name, fa, fb in zip(("u", "v", "w") + a.tracer_names, a.prognostic_fields(), b.prognostic_fields()):
        pa, pb = fa.parent(), fb.parent()
        assert np.all(np.isfinite(pa)), (what, name)
        assert np.array_equal(pa, pb), (what, name, float(np.max(np.abs(pa - pb))))


# ---- 3. linear drag twin -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("timestepper", ["RungeKutta3", "QuasiAdamsBashforth2"])
def test_linear_drag_is_bitwise_the_coeff_form(ocn, monkeypatch, timestepper):
    """-p * u is (-p) * u in Python: one multiplication, as condition + coeff * c with condition = 0 (adding 0.0 changes no bit that a
    comparison sees).  The coeff model is built with OCN_FUSE_GENERAL=0, so both run the reference's launch sequence."""
    r = 0.37
    dep = ocn.FluxBoundaryCondition(lambda x, y, t, u, p: -p * u, field_dependencies="u", parameters=r)
    a = build(ocn, {"u": ocn.FieldBoundaryConditions(bottom=dep)}, timestepper)
    b = build(ocn, {"u": ocn.FieldBoundaryConditions(bottom=ocn.FluxBoundaryCondition(0.0, coeff=-r))}, timestepper, monkeypatch)
    assert not a.fuse_stage_boundaries and not b.fuse_stage_boundaries and len(a._boundary_functions) == 1
    for _ in range(3):
        ocn.time_step(a, DT)
        ocn.time_step(b, DT)
    assert_same_state(ocn, a, b, timestepper)
    # ... and the drag did something: the same model without it differs
    c = build(ocn, None, timestepper)
    for _ in range(3):
        ocn.time_step(c, DT)
    ocn.flush_tendencies(c)
    assert not np.array_equal(a.u.parent(), c.u.parent())


# ---- 4., 5. composed sequence ------------------------------------------------------------------------------------------------------------
def manual_rk3_step(ocn, m, dt, evaluate):
    """time_step!(model::RungeKutta3, Δt) through the exported unfused functions, with `evaluate(time)` after every halo fill of
    update_state! and before its compute_tendencies!"""
    ts, clock = m.timestepper, m.clock

    def update_state():
        ocn.fill_halo_regions(m.prognostic_fields(), fill_boundary_normal_velocities=False)
        evaluate(clock.time)
        ocn.compute_auxiliaries(m)
        ocn.compute_tendencies(m)

    def project(stage_dt):
        ocn.calculate_pressure_correction(m, stage_dt)
        ocn.pressure_correct_velocities(m, stage_dt)
    if clock.iteration == 0:
        update_state()
    t_next = clock.time + dt
    first, second, third = ts.g1 * dt, (ts.g2 + ts.z2) * dt, (ts.g3 + ts.z3) * dt
    ocn.rk3_substep(m, dt, ts.g1, None)
    clock.time += first
    project(first)
    ocn.cache_previous_tendencies(m)
    update_state()
    ocn.rk3_substep(m, dt, ts.g2, ts.z2)
    clock.time += second
    project(second)
    ocn.cache_previous_tendencies(m)
    update_state()
    ocn.rk3_substep(m, dt, ts.g3, ts.z3)
    clock.time = t_next
    clock.iteration += 1
    project(third)
    update_state()


def composed_check(ocn, conditions, what):
    """conditions: {field name: (function, field_dependencies, parameters)} on the bottom"""
    mk = lambda spec: ocn.FluxBoundaryCondition(spec[0], field_dependencies=spec[1], parameters=spec[2])
    a = build(ocn, {n: ocn.FieldBoundaryConditions(bottom=mk(spec)) for n, spec in conditions.items()})
    assert len(a._boundary_functions) == len(conditions) and not a.fuse_stage_boundaries
    g = a.grid
    arrays = {n: ocn.FluxBoundaryCondition(np.zeros((g.Nx, g.Ny))) for n in conditions}
    b = build(ocn, {n: ocn.FieldBoundaryConditions(bottom=bc) for n, bc in arrays.items()})
    assert not b._boundary_functions
    fields = dict(zip(("u", "v", "w") + b.tracer_names, b.prognostic_fields()))
    traced = {n: ocn.BoundaryFunction(mk(spec), b.grid, fields[n].loc, "bottom", fields) for n, spec in conditions.items()}
    for n in conditions:
        fields[n].boundary_conditions.c_struct(b.grid)  # (allocates the device array of an array-valued condition)
    times = []

    def evaluate(time):
        times.append(time)
        for n, bf in traced.items():
            evaluate_into(ocn, bf, time, arrays[n]._device_values.data_ptr())
    for _ in range(3):
        ocn.time_step(a, DT)
        manual_rk3_step(ocn, b, DT, evaluate)
    assert len(set(times[:4])) == 4                                   # t = 0 and three distinct stage times
    assert a.clock.time == b.clock.time
    assert_same_state(ocn, a, b, what)
    # the values the model holds are those of its final state and clock
    parents = {n: f.parent() for n, f in zip(("u", "v", "w") + a.tracer_names, a.prognostic_fields())}
    for bf in a._boundary_functions:
        name = [n for n, f in zip(("u", "v", "w") + a.tracer_names, a.prognostic_fields()) if f.loc == bf.program.loc][0]
        func, deps, params = conditions[name]
        want = BN.expected(func, a.grid, name, "bottom", parents, deps, params, a.clock.time)
        assert np.array_equal(bf.bc._device_values.cpu().numpy().T, want), (what, name)
    return a


def test_drag_laws_are_bitwise_the_composed_sequence(ocn):
    fn = BN.functions(ocn)
    a = composed_check(ocn, {n: fn["drag_" + n][1:] for n in ("u", "v")}, "drag")
    assert np.max(np.abs(a._boundary_functions[0].bc._device_values.cpu().numpy())) > 0


def test_time_is_current_at_every_stage(ocn):
    """-(1 + t) u: a time that is stale by one stage changes the flux by Δt-sized factors, far above a bit"""
    composed_check(ocn, {"u": (lambda x, y, t, u: -(1 + t) * u, ("u",), None)}, "time")


# ---- 6. known answer ---------------------------------------------------------------------------------------------------------------------
def test_known_answer_after_one_euler_step(ocn):
    """A horizontally uniform (u0, v0), w = 0, no closure: every tendency but the drag is exactly 0 (all fluxes are equal from face to
    face), the flow stays divergence-free and the pressure is 0.  apply_z_bcs! adds +flux / Δz to the tendency of the bottom cell
    (flux_bcs: Gc[i, j, 1] += getbc(bottom) * Az / V), so after the first QAB2 step, an Euler step,
        u[i, j, 1] = u0 + Δt flux_u / Δzᵃᵃᶜ[1],   flux_u = -cd sqrt(u0² + (v0 + V)²) u0
    within 16 ulp of |u0| (a handful of roundings of half an ulp each, of numbers no larger than |u0|); every cell above is unchanged."""
    u0, v0, dt = 0.7, -0.4, 0.05
    name_u, drag_u, deps, params = BN.functions(ocn)["drag_u"]
    name_v, drag_v, _, _ = BN.functions(ocn)["drag_v"]
    grid = ocn.RectilinearGrid(ocn.GPU(), **MODEL_GRID)
    mk = lambda f: ocn.FieldBoundaryConditions(bottom=ocn.FluxBoundaryCondition(f, field_dependencies=deps, parameters=params))
    model = ocn.NonhydrostaticModel(grid, advection=ocn.WENO(), timestepper="QuasiAdamsBashforth2", math_mode=ocn.MATH_STRICT,
                                    boundary_conditions={"u": mk(drag_u), "v": mk(drag_v)})
    g = model.grid
    ocn.set(model, u=np.full((g.Nx, g.Ny, g.Nz), u0), v=np.full((g.Nx, g.Ny, g.Nz), v0))
    ocn.time_step(model, dt)
    ocn.flush_tendencies(model)
    u, v, w = (f.interior() for f in model.velocities)
    dz1 = BN.STRETCHED_Z[1] - BN.STRETCHED_Z[0]
    speed = np.sqrt(u0 ** 2 + (v0 + params["V"]) ** 2)
    for got, start, flux, ref in ((u, u0, -params["cd"] * speed * u0, abs(u0)), (v, v0, -params["cd"] * speed * (v0 + params["V"]), abs(v0))):
        want = start + dt * (flux / dz1)
        err = float(np.max(np.abs(got[:, :, 0] - want)))
        print(f"bottom cell: |got - want| = {err:.3e} = {err / (EPS * ref):.2f} ulp of |start|; change {want - start:.3e}")
        assert abs(want - start) > 1e4 * EPS * ref                    # the drag is far above the tolerance
        assert err <= 16 * EPS * ref
        assert np.array_equal(got[:, :, 1:], np.full_like(got[:, :, 1:], start))
    assert np.array_equal(w, np.zeros_like(w))


# ---- 7. refusals and what stays as it was ------------------------------------------------------------------------------------------------
def test_drivers_refuse_and_other_conditions_keep_their_path(ocn):
    dep = ocn.FluxBoundaryCondition(lambda x, y, t, u: -0.1 * u, field_dependencies="u")
    model = build(ocn, {"u": ocn.FieldBoundaryConditions(bottom=dep)})
    for driver in (ocn.RK3Driver, ocn.ModelRK3Driver):
        with pytest.raises(NotImplementedError, match="Python host"):
            driver(model)
    # number, coeff, array and host-sampled function conditions: no boundary function, fused stage boundaries as before
    g = model.grid
    for bc in (ocn.FluxBoundaryCondition(0.3), ocn.FluxBoundaryCondition(0.0, coeff=-0.2), ocn.FluxBoundaryCondition(np.ones((g.Nx, g.Ny))),
               ocn.FluxBoundaryCondition(lambda x, y, t: x + t)):
        other = build(ocn, {"u": ocn.FieldBoundaryConditions(bottom=bc)})
        assert other._boundary_functions == [] and other.fuse_stage_boundaries


def test_tilted_boundary_layer_drag_as_written(ocn):
    """examples/tilted_bottom_boundary_layer.jl:122-126 on a (Periodic, Flat, Bounded) grid: drag_u(x, t, u, v, p), √ spelled ocn.sqrt"""
    V, cd = 0.1, (0.4 / np.log(0.2 / 0.1)) ** 2

    def drag_u(x, t, u, v, p):
        return -p["cᴰ"] * ocn.sqrt(u ** 2 + (v + p["V∞"]) ** 2) * u

    def drag_v(x, t, u, v, p):
        return -p["cᴰ"] * ocn.sqrt(u ** 2 + (v + p["V∞"]) ** 2) * (v + p["V∞"])
    p = {"cᴰ": cd, "V∞": V}
    grid = ocn.RectilinearGrid(ocn.GPU(), size=(8, 4), x=(0, 3), z=BN.STRETCHED_Z, topology=(BN.P, BN.F, BN.B), halo=(3, 3))
    bcs = {"u": ocn.FieldBoundaryConditions(bottom=ocn.FluxBoundaryCondition(drag_u, field_dependencies=("u", "v"), parameters=p)),
           "v": ocn.FieldBoundaryConditions(bottom=ocn.FluxBoundaryCondition(drag_v, field_dependencies=("u", "v"), parameters=p))}
    model = ocn.NonhydrostaticModel(grid, advection=ocn.WENO(), closure=ocn.ScalarDiffusivity(nu=1e-2), boundary_conditions=bcs,
                                    math_mode=ocn.MATH_STRICT)
    g = model.grid
    rng = np.random.default_rng(2)
    ocn.set(model, u=rng.uniform(-1, 1, (g.Nx, 1, g.Nz)), v=rng.uniform(-1, 1, (g.Nx, 1, g.Nz)))
    ocn.time_step(model, DT)
    ocn.flush_tendencies(model)
    parents = {n: f.parent() for n, f in zip("uvw", model.velocities)}
    assert all(np.all(np.isfinite(a)) for a in parents.values())
    for bf, (name, func) in zip(model._boundary_functions, (("u", drag_u), ("v", drag_v))):
        want = BN.expected(func, g, name, "bottom", parents, ("u", "v"), p, model.clock.time)
        assert np.any(want != 0) and np.array_equal(bf.bc._device_values.cpu().numpy().T, want), name
