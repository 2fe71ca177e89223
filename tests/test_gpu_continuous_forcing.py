"""ContinuousForcing on the device.

1. ocn_op_accumulate against the hand-written restatement (tests/continuous_forcing_numpy.py, pinned by the host tests), bit for bit: + - * /
   are correctly rounded on both sides, the kernel is built without FMA contraction and what the host folds is the same NumPy call on the
   same vector.  Fields and G are seeded random over their WHOLE parent arrays and no halo fill is called, so a wrong offset shows.
2. Nothing but the tendency cells of G is written (NaN sentinel in its halos), two calls give the same bits.
3. MIN / MAX: NaN, the two zeros in both operand orders, infinities, bit pattern by bit pattern, through a diagnostics tree.
4. compute_tendencies with Forcing(func, steady=True) and with ContinuousForcing(func) gives the same Gⁿ; a Relaxation with and without a
   zero ContinuousForcing next to it too.
5. The time is current at every RK3 stage.  6. A known answer after one Euler step.  7. One RK3 step against the composed sequence.
8. The example runs."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import continuous_forcing_numpy as CN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIME = 0.375


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def device_fields(ocn, grid, parents):
    f = {}
    for n, a in parents.items():
        f[n] = ocn.Field(CN.loc_of(n), grid)
        f[n].data.copy_(torch.from_numpy(np.ascontiguousarray(a.T)))
    return f


def program_forcing(ocn, value, grid, name, fields, time=0.0):
    from oceananigans_jl_amd.forcings import validate_forcing
    return ocn.ProgramForcing(validate_forcing({name: value}, grid, tuple(fields))[name], grid, name, fields, time)


_setups = {}


@pytest.fixture(scope="module")
def setup(ocn):
    def get(gname):
        if gname not in _setups:
            grid = ocn.RectilinearGrid(ocn.GPU(), **CN.GRIDS[gname])
            parents = CN.random_parents(grid, 11 + list(CN.GRIDS).index(gname))
            parents["T"][grid.Hx + 1, grid.Hy, grid.Hz + 1] = -0.0
            _setups[gname] = (grid, parents, device_fields(ocn, grid, parents))
        return _setups[gname]
    yield get
    _setups.clear()


# ---- 1. kernel parity --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gname", list(CN.GRIDS))
def test_kernel_is_bitwise_the_restatement(ocn, setup, gname):
    grid, parents, f = setup(gname)
    rng = np.random.default_rng(5)
    for cname, case in CN.cases(ocn).items():
        loc = CN.loc_of(case.forced)
        pf = program_forcing(ocn, case.terms(grid), grid, case.forced, f, time=-1.0)   # (traced at another time: the patch must take)
        G0 = rng.uniform(-1, 1, grid.parent_shape(loc))
        G = ocn.Field(loc, grid)
        G.data.copy_(torch.from_numpy(np.ascontiguousarray(G0.T)))
        pf.accumulate(G, TIME)
        got = G.parent()
        want = G0.copy()
        sl = CN.cell_slices(grid, loc)
        want[sl] = G0[sl] + case.expected(grid, parents, TIME)
        assert np.array_equal(bits(got[sl]), bits(want[sl])), (gname, cname, float(np.nanmax(np.abs(got[sl] - want[sl]))))
        assert np.array_equal(bits(got), bits(want)), (gname, cname, "outside the tendency cells")
        assert not np.array_equal(got[sl], G0[sl]), (gname, cname)
    for n, field in f.items():
        assert np.array_equal(bits(field.parent()), bits(parents[n])), (gname, n)


# ---- 2. nothing else is written ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gname,cname", [("ppb", "on_w"), ("bbb", "two_directions"), ("bbb", "on_w"), ("wide", "mixed")])
def test_nothing_else_is_written(ocn, setup, gname, cname):
    grid, parents, f = setup(gname)
    case = CN.cases(ocn)[cname]
    loc = CN.loc_of(case.forced)
    pf = program_forcing(ocn, case.terms(grid), grid, case.forced, f)
    sl = CN.cell_slices(grid, loc)
    G0 = np.full(grid.parent_shape(loc), np.nan)   # halos AND the faces on a wall
    G0[sl] = 0.5
    out = []
    for _ in range(2):
        G = ocn.Field(loc, grid)
        G.data.copy_(torch.from_numpy(np.ascontiguousarray(G0.T)))
        pf.accumulate(G, TIME)
        out.append(G.parent())
    want = G0.copy()
    want[sl] = 0.5 + case.expected(grid, parents, TIME)
    assert np.array_equal(bits(out[0]), bits(want))
    assert np.array_equal(bits(out[0]), bits(out[1]))                       # two calls, identical bits
    for n, field in f.items():
        assert np.array_equal(bits(field.parent()), bits(parents[n])), n   # every dependency, halos included, is unchanged
    # the library refuses a tendency array that the program reads
    with pytest.raises(ocn.OcnError, match="of the program"):
        pf.accumulate(f[{"on_w": "b", "two_directions": "u", "mixed": "T"}[cname]], TIME)


# ---- 3. MIN / MAX --------------------------------------------------------------------------------------------------------------------------
def test_min_max_have_julias_semantics(ocn, setup):
    grid, _, _ = setup("short")
    nan, inf = np.nan, np.inf
    a = np.array([-0.0, 0.0, -0.0, 0.0, nan, 1.0, nan, -inf, inf, 2.0, -3.0, inf])
    b = np.array([0.0, -0.0, -0.0, 0.0, 1.0, nan, nan, inf, -inf, 2.0, 5.0, nan])
    n = (grid.Nx, grid.Ny, grid.Nz)
    A, Bf = ocn.CenterField(grid), ocn.CenterField(grid)
    A.set(np.resize(a, n))
    Bf.set(np.resize(b, n))
    for tree, want in ((ocn.maximum(A, Bf), CN.julia_max(np.resize(a, n), np.resize(b, n))),
                       (ocn.minimum(A, Bf), CN.julia_min(np.resize(a, n), np.resize(b, n))),
                       (np.maximum(A * 1.0, 0), CN.julia_max(np.resize(a, n), 0.0)),
                       (ocn.maximum(0, A), CN.julia_max(0.0, np.resize(a, n))),
                       (ocn.minimum(A, -0.0), CN.julia_min(np.resize(a, n), -0.0)),
                       (ocn.minimum(0.0, A), CN.julia_min(0.0, np.resize(a, n)))):
        got = ocn.ComputedField(tree).compute().interior()
        assert np.array_equal(bits(got), bits(want))
    # by hand, the cases that np.maximum / fmax get wrong
    got = ocn.ComputedField(ocn.maximum(A, Bf)).compute().interior().ravel()[:12]
    assert np.array_equal(bits(got), bits([0.0, 0.0, -0.0, 0.0, nan, nan, nan, inf, inf, 2.0, 5.0, nan]))
    got = ocn.ComputedField(ocn.minimum(A, Bf)).compute().interior().ravel()[:12]
    assert np.array_equal(bits(got), bits([-0.0, -0.0, -0.0, 0.0, nan, nan, nan, -inf, -inf, 2.0, -3.0, nan]))


# ---- models ------------------------------------------------------------------------------------------------------------------------------
DT = 2.0e-3


def initial_state(grid, names, seed=5):
    rng = np.random.default_rng(seed)
    from oceananigans_jl_amd.forcings import interior_shape
    return {n: rng.uniform(-1, 1, interior_shape(grid, CN.loc_of(n))) for n in names}


def build(ocn, gname, forcing, tracers=("T",), timestepper="RungeKutta3", closure=None, unfused=None):
    if unfused is not None:  # the switch that gives a model of the general fused path the reference's launch sequence
        unfused.setenv("OCN_FUSE_GENERAL", "0")
    grid = ocn.RectilinearGrid(ocn.GPU(), **CN.GRIDS[gname])
    model = ocn.NonhydrostaticModel(grid, advection=ocn.WENO(), tracers=tracers, timestepper=timestepper, closure=closure, forcing=forcing,
                                    math_mode=ocn.MATH_STRICT)
    if unfused is not None:
        unfused.delenv("OCN_FUSE_GENERAL")
    ocn.set(model, **initial_state(model.grid, ("u", "v", "w") + tuple(tracers)))
    return model


def tendencies(ocn, model):
    ocn.update_state(model, compute_tendencies=True)
    ocn.sync_device()
    return [G.parent() for G in model.timestepper.Gn]


# ---- 4. equivalence with the sampled path --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gname", ["ppb", "bbb", "pfb"])
def test_traced_and_sampled_functions_give_the_same_tendencies(ocn, gname):
    def sampled(*a):   # (x, [y,] z, t)
        return 0.3 * a[0] - a[-2] * a[-2]
    names = ("u", "v", "w", "T")
    a = build(ocn, gname, {n: ocn.Forcing(sampled, steady=True) for n in names})
    b = build(ocn, gname, {n: ocn.ContinuousForcing(sampled) for n in names})
    c = build(ocn, gname, None)
    assert all(p is not None for p in b._forcing_programs) and all(f is None for f in b._forcing) and not b.fuse_stage_boundaries
    assert all(p is None for p in a._forcing_programs)
    Ga, Gb, Gc = tendencies(ocn, a), tendencies(ocn, b), tendencies(ocn, c)
    for n, x, y, z in zip(names, Ga, Gb, Gc):
        np.testing.assert_array_equal(x, y, err_msg=f"{gname} {n}")
        assert np.all(np.isfinite(x)) and not np.array_equal(x, z), (gname, n)   # ... and the forcing did something


def test_a_zero_program_next_to_a_relaxation_changes_nothing(ocn):
    sponge = lambda: ocn.Relaxation(0.25, mask=ocn.GaussianMask("z", center=-0.4, width=0.3), target=ocn.LinearTarget("z", intercept=0.5, gradient=-0.2))
    a = build(ocn, "bbb", {"T": sponge(), "w": ocn.Relaxation(0.5)})
    b = build(ocn, "bbb", {"T": (sponge(), ocn.ContinuousForcing(lambda x, y, z, t: 0.0)),
                           "w": (ocn.Relaxation(0.5), ocn.ContinuousForcing(lambda x, y, z, t: 0.0))})
    assert b._forcing_programs[2] is not None and b._forcing_programs[3] is not None and b._forcing[3] is None
    for n, x, y in zip("uvwT", tendencies(ocn, a), tendencies(ocn, b)):
        np.testing.assert_array_equal(x, y, err_msg=n)


# ---- 5. the time at every stage ------------------------------------------------------------------------------------------------------------
def test_time_is_current_at_every_stage(ocn, monkeypatch):
    model = build(ocn, "short", {"T": ocn.ContinuousForcing(lambda x, y, z, t: t * 0.5)})
    pf = model._forcing_programs[3]
    seen = []
    call = ocn._lib.call

    def recording(name, *args):
        if name == "ocn_op_accumulate":
            seen.append(args[1]._obj.ins[pf.program.time_index].value)
        return call(name, *args)
    monkeypatch.setattr(ocn._lib, "call", recording)
    ts, dt = model.timestepper, DT
    ocn.time_step(model, dt)
    ocn.flush_tendencies(model)
    t1 = 0.0 + ts.g1 * dt
    t2 = t1 + (ts.g2 + ts.z2) * dt
    assert seen == [0.0, t1, t2, 0.0 + dt] and len(set(seen)) == 4
    ocn.time_step(model, dt)
    ocn.flush_tendencies(model)
    assert seen[4:] == [dt + ts.g1 * dt, (dt + ts.g1 * dt) + (ts.g2 + ts.z2) * dt, dt + dt]


# ---- 6. known answer -----------------------------------------------------------------------------------------------------------------------
def test_known_answer_after_one_euler_step(ocn):
    """A uniform u = u0, v = w = 0: every flux is the same from face to face, so the advective tendency is exactly 0, the flow stays
    divergence-free and the pressure is 0.  The first QAB2 step is an Euler step: u = u0 + Δt (0.0 + (-μ u0)), bit for bit."""
    u0, mu, dt = 0.7, 0.375, 0.05
    grid = ocn.RectilinearGrid(ocn.GPU(), **CN.GRIDS["short"])
    model = ocn.NonhydrostaticModel(grid, advection=ocn.WENO(), timestepper="QuasiAdamsBashforth2", math_mode=ocn.MATH_STRICT,
                                    forcing={"u": ocn.ContinuousForcing(lambda x, y, z, t, u, p: -p * u, field_dependencies="u", parameters=mu)})
    g = model.grid
    ocn.set(model, u=np.full((g.Nx, g.Ny, g.Nz), u0))
    ocn.time_step(model, dt)
    ocn.flush_tendencies(model)
    u, v, w = (f.interior() for f in model.velocities)
    want = np.float64(u0) + np.float64(dt) * (np.float64(0.0) + (-np.float64(mu) * np.float64(u0)))
    assert want != u0
    assert np.array_equal(bits(u), bits(np.full_like(u, want)))
    assert np.array_equal(v, np.zeros_like(v)) and np.array_equal(w, np.zeros_like(w))


# ---- 7. composed sequence ------------------------------------------------------------------------------------------------------------------
def manual_rk3_step(ocn, m, dt, add_forcing):
    """time_step!(model::RungeKutta3, Δt) through the exported unfused functions, with `add_forcing(time)` between the interior and the
    boundary contributions of every compute_tendencies!"""
    ts, clock = m.timestepper, m.clock

    def update_state():
        ocn.fill_halo_regions(m.prognostic_fields(), fill_boundary_normal_velocities=False)
        ocn.compute_auxiliaries(m)
        ocn.compute_tendencies(m, boundary_contributions=False)
        add_forcing(clock.time)
        ocn.compute_boundary_tendency_contributions(m)

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


@pytest.mark.parametrize("gname", ["ppb", "pfb"])
def test_one_rk3_step_is_bitwise_the_composed_sequence(ocn, monkeypatch, gname):
    case = CN.cases(ocn)["plankton"]
    closure = lambda: ocn.ScalarDiffusivity(nu=1e-2, kappa=2e-2)
    flux = lambda: {"b": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(0.125))}
    grid = ocn.RectilinearGrid(ocn.GPU(), **CN.GRIDS[gname])

    def model(forcing, unfused=None):
        if unfused is not None:
            unfused.setenv("OCN_FUSE_GENERAL", "0")
        m = ocn.NonhydrostaticModel(ocn.RectilinearGrid(ocn.GPU(), **CN.GRIDS[gname]), advection=ocn.WENO(), tracers=("b",), closure=closure(),
                                    forcing=forcing, boundary_conditions=flux(), math_mode=ocn.MATH_STRICT)
        if unfused is not None:
            unfused.delenv("OCN_FUSE_GENERAL")
        ocn.set(m, **initial_state(m.grid, ("u", "v", "w", "b")))
        return m
    a = model({"b": case.terms(grid)})
    b = model(None, monkeypatch)
    assert a._forcing_programs[3] is not None and not a.fuse_stage_boundaries and not b.fuse_stage_boundaries
    times = []

    def add_forcing(time):
        times.append(time)
        ocn.sync_device()
        parents = {"b": b.tracers[0].parent()}
        F = case.expected(b.grid, parents, time)
        b.timestepper._Gn[3].interior_view().add_(torch.from_numpy(np.ascontiguousarray(F.T)).cuda())
    ocn.time_step(a, DT)
    manual_rk3_step(ocn, b, DT, add_forcing)
    ocn.flush_tendencies(a)
    ocn.sync_device()
    assert len(set(times)) == 4 and a.clock.time == b.clock.time
    for n, fa, fb in zip(("u", "v", "w", "b"), a.prognostic_fields(), b.prognostic_fields()):
        pa, pb = fa.parent(), fb.parent()
        assert np.all(np.isfinite(pa)), (gname, n)
        assert np.array_equal(bits(pa), bits(pb)), (gname, n, float(np.max(np.abs(pa - pb))))
    for Ga, Gb in zip(a.timestepper.Gn, b.timestepper._Gn):
        assert np.array_equal(bits(Ga.parent()), bits(Gb.parent())), gname


# ---- 8. refusals and the example -----------------------------------------------------------------------------------------------------------
def test_drivers_refuse_and_other_forcings_keep_their_path(ocn):
    model = build(ocn, "short", {"T": ocn.ContinuousForcing(lambda x, y, z, t, T: -0.1 * T, field_dependencies="T")})
    for driver in (ocn.RK3Driver, ocn.ModelRK3Driver):
        with pytest.raises(NotImplementedError, match="Python host"):
            driver(model)
    other = build(ocn, "short", {"T": ocn.Relaxation(0.1), "u": ocn.Forcing(lambda x, y, z, t: x, steady=True)})
    assert all(p is None for p in other._forcing_programs) and other._forcing[0] is not None and other._forcing[3] is not None
    assert other.fuse_stage_boundaries


def test_convecting_plankton_example_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "convecting_plankton.py"), "--size", "16", "8", "--steps", "3"],
                         capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "finite fields: True" in out.stdout and "P changed: True" in out.stdout, out.stdout[-2000:]
