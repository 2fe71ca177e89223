"""Smagorinsky / SmagorinskyLilly on the GPU: the eddy-viscosity kernel (csrc/smagorinsky.hip) through the C ABI against the NumPy
restatement of the reference (tests/smagorinsky_numpy.py) on seeded inputs that reach every branch (asserted without a GPU in
tests/test_host_smagorinsky.py), the κₑ = νₑ / Pr fields, the model wiring against the oracle's tendencies, the C model driver against
the Python host, and the reference's time-stepping smoke entries (test/test_time_stepping.jl:254-255)."""
import ctypes as C

import numpy as np
import pytest

import smagorinsky_numpy as SN
from helpers import from_dev, make_pair, to_dev

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
LOCS = (1, 2, 4)
INVALID = -1  # OCN_ERR_INVALID_ARGUMENT
ALL_SETTINGS = [(c, s) for c in SN.CASES for s in SN.SETTINGS] + [(SN.CASES[2], SN.HALF_CB)]
IDS = [f"{c[0]}-{c[1]}-{s[0]}" for c, s in ALL_SETTINGS]

_reference = {}


def _case(O, ocn, case, setting):
    """grids, inputs and the restated νₑ of one (case, setting); computed once and shared (never modified)"""
    key = (case[0], case[1], setting[0])
    if key not in _reference:
        size, topo, z, halo = case
        _, lilly, Cs, Cb, buoyancy = setting
        og, pg = make_pair(O, ocn, size, topo, z=SN.case_z(size, z), halo=halo)
        f = SN.random_inputs(og, buoyancy)
        nu = SN.smagorinsky_viscosity(og, f["u"], f["v"], f["w"], Cs, lilly=lilly, Cb=Cb, buoyancy=buoyancy, T=f["T"], S=f["S"])
        _reference[key] = (og, pg, f, np.array(nu))
    return _reference[key]


def _closure(ocn, setting, Pr=()):
    _, lilly, Cs, Cb, _ = setting
    s = ocn._lib.CSmagorinsky()
    s.C, s.Cb, s.lilly, s.n_tracers = Cs, Cb if lilly else 0.0, int(lilly), len(Pr)
    for n, p in enumerate(Pr):
        s.Pr[n] = p
    return s


def _terms(ocn, buoyancy, T, S):
    L = ocn._lib
    t = L.CModelTerms()
    if buoyancy == "BuoyancyTracer":
        t.buoyancy, t.T = L.BUOYANCY_TRACER, T.ptr
    elif buoyancy is not None:
        t.buoyancy, t.g, t.alpha, t.beta = L.BUOYANCY_SEAWATER_TS, buoyancy[1], buoyancy[2], buoyancy[3]
        t.T, t.S = T.ptr, S.ptr
    return t


def _device_nu(ocn, pg, f, setting, mode):
    ocn.set_math_mode(mode)
    try:
        du, dv, dw = (to_dev(ocn, pg, l, f[n]) for l, n in zip(LOCS, "uvw"))
        dT = None if f["T"] is None else to_dev(ocn, pg, 0, f["T"])
        dS = None if f["S"] is None else to_dev(ocn, pg, 0, f["S"])
        dnu = ocn.Field(0, pg)
        dnu.data.fill_(-7.0)  # every interior cell must be written
        t, cs = _terms(ocn, setting[4], dT, dS), _closure(ocn, setting)
        ocn._lib.call("ocn_compute_smagorinsky_diffusivities", pg.cref, C.byref(t), C.byref(cs), du.ptr, dv.ptr, dw.ptr, dnu.ptr, None, 0)
        ocn.sync_device()
    finally:
        ocn.set_math_mode(ocn.MATH_STRICT)
    return from_dev(dnu)


@pytest.mark.parametrize("case,setting", ALL_SETTINGS, ids=IDS)
def test_viscosity_strict_against_the_restatement(oracle, ocn, case, setting):
    """Every operation is IEEE and in the reference's order except cbrt (libm's and the device library's are each within 1 ulp and the
    value is squared): per-cell relative difference <= 8 ε, exact zeros where the restatement gives 0; halos are not written."""
    og, pg, f, nu = _case(oracle, ocn, case, setting)
    parent = _device_nu(ocn, pg, f, setting, ocn.MATH_STRICT)
    got = og.interior_N(parent)
    rel = np.abs(got - nu) / np.where(nu == 0, 1.0, nu)
    print(f"max relative difference {rel.max() / EPS:.2f} eps, zeros {np.count_nonzero(nu == 0)}, max nu_e {nu.max():.3e}")
    assert np.all(got[nu == 0] == 0.0)
    assert rel.max() <= 8 * EPS
    assert nu.max() > 0 and np.count_nonzero(nu == 0) >= 1
    halo = np.ones(parent.shape, dtype=bool)
    halo[og.Hx:og.Hx + og.Nx, og.Hy:og.Hy + og.Ny, og.Hz:og.Hz + og.Nz] = False
    assert np.all(parent[halo] == -7.0)


@pytest.mark.parametrize("case,setting", ALL_SETTINGS, ids=IDS)
def test_viscosity_fast_within_the_fast_build_bound(oracle, ocn, case, setting):
    """the fast variant (single-factor averages, reciprocal spacings, FMA): 1e-12 max|νₑ| per launch, the project's fast-build bound"""
    og, pg, f, nu = _case(oracle, ocn, case, setting)
    got = og.interior_N(_device_nu(ocn, pg, f, setting, ocn.MATH_FAST))
    err = np.abs(got - nu).max()
    print(f"max difference {err / nu.max():.3e} of max nu_e")
    assert err <= 1e-12 * nu.max()
    assert np.all(got[nu == 0] == 0.0)


def _stratified_model(ocn, pg, closure, tracers=("T", "S"), **kw):
    return ocn.NonhydrostaticModel(pg, advection=ocn.WENO(), tracers=tracers, coriolis=ocn.FPlane(f=1e-4), closure=closure,
                                   buoyancy=ocn.SeawaterBuoyancy(equation_of_state=ocn.LinearEquationOfState(2e-4, 8e-4)), **kw)


def _set_random(ocn, og, model, f, extra=()):
    init = {n: np.array(og.interior(f[n])) for n in ("u", "v", "w", "T", "S")}
    rng = np.random.default_rng(SN.SEED + 1)
    for n in extra:
        init[n] = rng.uniform(-1, 1, (og.Nx, og.Ny, og.Nz))
    ocn.set(model, **init)


def test_prandtl_numbers_share_or_scale_the_viscosity(oracle, ocn):
    """Pr = {T: 1, S: 0.5, c: 3}: κₑ of T IS the νₑ array, the others hold νₑ / Pr bit for bit (IEEE division in the same pass), and
    update_state leaves the halos of every distinct field filled with the default conditions."""
    O = oracle
    case, setting = SN.CASES[1], SN.SETTINGS[2]
    og, pg, f, _ = _case(O, ocn, case, setting)
    ocn.set_math_mode(ocn.MATH_STRICT)
    Pr = {"T": 1, "S": 0.5, "c": 3}
    m = _stratified_model(ocn, pg, ocn.SmagorinskyLilly(C=0.23, Cb=1, Pr=Pr), tracers=("T", "S", "c"))
    _set_random(ocn, og, m, f, extra=("c",))
    ocn.update_state(m, compute_tendencies=False)
    ocn.sync_device()
    d = m.diffusivity_fields
    assert d["kappa_e"][0] is d["nu_e"] and d["kappa_e"][0].data.data_ptr() == d["nu_e"].data.data_ptr()
    assert len({k.data.data_ptr() for k in d["kappa_e"]} | {d["nu_e"].data.data_ptr()}) == 3
    assert len(ocn.models.distinct_diffusivity_fields(m)) == 3
    nu = np.asfortranarray(from_dev(d["nu_e"]))
    assert og.interior_N(nu).max() > 0
    for k, name in zip(d["kappa_e"][1:], ("S", "c")):
        kap = np.asfortranarray(from_dev(k))
        np.testing.assert_array_equal(og.interior_N(kap), og.interior_N(nu) / Pr[name], err_msg=f"kappa_e of {name}")
    for a in [nu] + [np.asfortranarray(from_dev(k)) for k in d["kappa_e"][1:]]:
        filled = a.copy(order="F")
        filled[...] = np.nan
        og.interior_N(filled)[...] = og.interior_N(a)
        O.fill_halo_regions(og, filled, 0)
        known = np.isfinite(filled)  # (corners a single pass of the oracle's fill does not reach stay out of the comparison)
        assert known.sum() > og.Nx * og.Ny * og.Nz
        np.testing.assert_array_equal(a[known], filled[known])


@pytest.mark.parametrize("case", [SN.CASES[2], SN.CASES[3]], ids=["PPB-stretched", "BBB"])
def test_model_hands_the_right_fields_to_the_tendency_kernels(oracle, ocn, case):
    """After set! and update_state! every Gⁿ equals, bit for bit, the oracle's tendencies evaluated with the device's own νₑ / κₑ parents:
    the momentum stress reads νₑ, tracer n reads kappa_e[n] (νₑ itself for Pr == 1, νₑ / Pr otherwise)."""
    O = oracle
    og, pg, f, _ = _case(O, ocn, case, SN.SETTINGS[2])
    ocn.set_math_mode(ocn.MATH_STRICT)
    m = _stratified_model(ocn, pg, ocn.SmagorinskyLilly(C=0.23, Cb=1, Pr={"T": 1, "S": 0.5}))
    _set_random(ocn, og, m, f)
    ocn.update_state(m, compute_tendencies=True)
    Gdev = [np.asfortranarray(from_dev(G)) for G in m.timestepper.Gn]
    ocn.sync_device()
    host = lambda fld: np.asfortranarray(from_dev(fld))
    u, v, w, T, S = (host(x) for x in m.prognostic_fields())
    d = m.diffusivity_fields
    nu, kap, pHY = host(d["nu_e"]), [host(k) for k in d["kappa_e"]], host(m.pHY)
    assert og.interior_N(nu).max() > 0 and not np.array_equal(kap[1], nu)
    ph = O.Physics(f=1e-4, nu=0.0, buoyancy=SN.SEAWATER)
    G = [og.zeros(l) for l in LOCS + (0, 0)]
    O.momentum_tendencies(og, u, v, w, *G[:3])
    O.momentum_extra_tendencies(og, ph, u, v, w, T, S, pHY, *G[:3], nu_e=nu)
    for n, c in enumerate((T, S)):
        O.tracer_tendency(og, u, v, w, c, G[3 + n])
        O.tracer_diffusion(og, 0.0, c, G[3 + n], kappa_e=kap[n])
    for a, b, name in zip(G, Gdev, "uvwTS"):
        assert np.abs(og.interior(a)).max() > 0
        np.testing.assert_array_equal(og.interior(b), og.interior(a), err_msg=f"G{name} differs bitwise from the oracle")


@pytest.mark.parametrize("mode", ["strict", "fast"])
def test_c_model_driver_equals_python_host(ocn, mode):
    """three RK3 steps by ModelRK3Driver + flush() against three time_step(model, dt) on the Python host: bit-identical fields; the setter
    is refused while a step's tendencies are deferred"""
    rng = np.random.default_rng(SN.SEED + 2)
    N = (70, 9, 8)
    init = {"u": 1e-2 * rng.uniform(-1, 1, N), "v": 1e-2 * rng.uniform(-1, 1, N), "T": 20 + 1e-2 * rng.uniform(-1, 1, N),
            "S": 35 + 1e-2 * rng.uniform(-1, 1, N)}

    def build():
        g = ocn.RectilinearGrid(ocn.GPU(), size=N, x=(0, 64), y=(0, 64), z=(-32, 0), topology=("Periodic", "Periodic", "Bounded"))
        return _stratified_model(ocn, g, ocn.SmagorinskyLilly(C=0.23, Cb=1, Pr={"T": 1, "S": 0.5}))

    ocn.set_math_mode(ocn.MATH_STRICT if mode == "strict" else ocn.MATH_FAST)
    try:
        ref = build()
        ocn.set(ref, **init)
        for _ in range(3):
            ocn.time_step(ref, 1.5)
        ocn.flush_tendencies(ref)
        m = build()
        ocn.set(m, **init)
        drv = ocn.ModelRK3Driver(m)
        drv.time_step(1.5)
        cs = m.closure.c_struct(m.tracer_names)
        assert ocn._lib.lib().ocn_model_driver_set_smagorinsky(drv._h, C.byref(cs)) == INVALID
        assert b"ocn_model_driver_flush" in ocn._lib.lib().ocn_last_error()
        drv.time_step(1.5)
        drv.time_step(1.5)
        drv.flush()
        ocn.sync_device()
    finally:
        ocn.set_math_mode(ocn.MATH_STRICT)
    assert m.clock.iteration == 3 and m.clock.time == ref.clock.time
    dr, dm = ref.diffusivity_fields, m.diffusivity_fields
    pairs = list(zip(ref.prognostic_fields() + (ref.pNHS, ref.pHY, dr["nu_e"], dr["kappa_e"][1]),
                     m.prognostic_fields() + (m.pNHS, m.pHY, dm["nu_e"], dm["kappa_e"][1])))
    pairs += list(zip(ref.timestepper.Gn, m.timestepper.Gn))
    for q, (a, b) in enumerate(pairs):
        assert np.isfinite(a.parent()).all()
        np.testing.assert_array_equal(a.parent(), b.parent(), err_msg=f"array {q}")
    assert float(dm["nu_e"].data.max()) > 0
    del drv


@pytest.mark.parametrize("ts", ["RungeKutta3", "QuasiAdamsBashforth2"])
@pytest.mark.parametrize("closure", ["Smagorinsky", "SmagorinskyLilly"])
def test_time_stepping_smoke(ocn, ts, closure):
    """test_time_stepping.jl:254-255: one step with each closure and time stepper leaves every field finite, reaches νₑ > 0 and keeps
    max|∇·u| under the bound of the model tests (5e-8)"""
    import torch
    rng = np.random.default_rng(SN.SEED + 3)
    N = (16, 16, 16)
    g = ocn.RectilinearGrid(ocn.GPU(), size=N, x=(0, 1), y=(0, 1), z=(0, 1), topology=("Periodic", "Periodic", "Bounded"))
    ocn.set_math_mode(ocn.MATH_STRICT)
    m = ocn.NonhydrostaticModel(g, advection=ocn.WENO(), tracers=("b",), timestepper=ts, buoyancy=ocn.BuoyancyTracer(),
                                closure=getattr(ocn, closure)())
    g = m.grid
    ocn.set(m, u=rng.uniform(-1, 1, N), v=rng.uniform(-1, 1, N), w=rng.uniform(-1, 1, (N[0], N[1], N[2] + 1)), b=rng.uniform(-1, 1, N))
    umax = max(float(f.data.abs().max()) for f in m.velocities)
    ocn.time_step(m, 0.1 * (1 / 16) / umax)
    ocn.flush_tendencies(m)
    ocn.sync_device()
    for f in m.prognostic_fields() + (m.pNHS, m.diffusivity_fields["nu_e"]):
        assert bool(torch.isfinite(f.data).all())
    assert float(m.diffusivity_fields["nu_e"].data.max()) > 0
    assert m.diffusivity_fields["kappa_e"][0] is m.diffusivity_fields["nu_e"]
    ddiv = torch.zeros((N[2], N[1], N[0]), dtype=torch.float64, device=m.u.data.device)
    ocn._lib.call("ocn_divergence", g.cref, m.u.ptr, m.v.ptr, m.w.ptr, ddiv.data_ptr(), 0)
    assert float(ddiv.abs().max()) < 5e-8
    assert m.clock.iteration == 1


def test_argument_errors_through_the_c_abi(oracle, ocn):
    og, pg, f, _ = _case(oracle, ocn, SN.CASES[1], SN.SETTINGS[2])
    lib, L = ocn._lib.lib(), ocn._lib
    du, dv, dw = (to_dev(ocn, pg, l, f[n]) for l, n in zip(LOCS, "uvw"))
    dT, dS, dnu, dk = to_dev(ocn, pg, 0, f["T"]), to_dev(ocn, pg, 0, f["S"]), ocn.Field(0, pg), ocn.Field(0, pg)
    dnu.data.fill_(-7.0)
    fn = lib.ocn_compute_smagorinsky_diffusivities

    def call(terms, cs, kappa=None):
        return fn(pg.cref, C.byref(terms), C.byref(cs), du.ptr, dv.ptr, dw.ptr, dnu.ptr, kappa, None)
    good = _terms(ocn, SN.SEAWATER, dT, dS)
    noS = _terms(ocn, SN.SEAWATER, dT, dS)
    noS.S = None
    assert call(noS, _closure(ocn, SN.SETTINGS[2])) == INVALID and b"S tracer is NULL" in lib.ocn_last_error()
    assert call(noS, _closure(ocn, SN.SETTINGS[0])) == 0  # a number coefficient reads no buoyancy
    noT = _terms(ocn, "BuoyancyTracer", dT, None)
    noT.T = None
    assert call(noT, _closure(ocn, SN.SETTINGS[1])) == INVALID and b"tracer is NULL" in lib.ocn_last_error()
    assert call(good, _closure(ocn, SN.SETTINGS[2], Pr=(1.0, 0.0)), L.ptr_array([None, dk.ptr])) == INVALID
    assert b"must be positive" in lib.ocn_last_error()
    assert call(good, _closure(ocn, SN.SETTINGS[2], Pr=(1.0, 0.5)), L.ptr_array([None, None])) == INVALID
    assert b"needs a kappa_e field" in lib.ocn_last_error()
    assert call(good, _closure(ocn, SN.SETTINGS[2], Pr=(1.0, 0.5)), L.ptr_array([dnu.ptr, dk.ptr])) == 0  # kappa_e == nu_e where Pr == 1
    ocn.sync_device()
    np.testing.assert_array_equal(og.interior_N(from_dev(dk)), og.interior_N(from_dev(dnu)) / 0.5)
    gf = ocn.RectilinearGrid(ocn.GPU(), size=(16, 16), x=(0, 1), y=(0, 1), topology=("Periodic", "Periodic", "Flat"), halo=(3, 3))
    assert fn(gf.cref, C.byref(good), C.byref(_closure(ocn, SN.SETTINGS[0])), du.ptr, dv.ptr, dw.ptr, dnu.ptr, None, None) == INVALID
    assert b"non-Flat z" in lib.ocn_last_error()
    # the driver's setter: a driver created for another closure kind, a wrong tracer count
    g = ocn.RectilinearGrid(ocn.GPU(), size=(16, 16, 8), x=(0, 1), y=(0, 1), z=(-1, 0), topology=("Periodic", "Periodic", "Bounded"))
    m = ocn.NonhydrostaticModel(g, advection=ocn.WENO(), tracers=("c",), closure=ocn.ScalarDiffusivity(ν=1e-3, κ=1e-3))
    drv = ocn.ModelRK3Driver(m)
    cs = ocn.Smagorinsky().c_struct(("c",))
    assert lib.ocn_model_driver_set_smagorinsky(drv._h, C.byref(cs)) == INVALID and b"closure 1" in lib.ocn_last_error()
    assert lib.ocn_model_driver_set_smagorinsky(drv._h, None) == 0
    del drv
