"""ConvectiveAdjustmentVerticalDiffusivity on the GPU (csrc/vertical_diffusivity.hip): the three kernels against the NumPy restatement of the
reference (tests/convective_adjustment_numpy.py, pinned without a GPU in tests/test_host_convective_adjustment.py) bit for bit, the existing
constant-κ kernels as yardsticks, the maximum principle and conservation of the device result, and five steps of the hydrostatic model
against the same sequence composed from the public stage functions plus the restatement.

Grids are at most 13 x 6 x 12, for the reasons at the top of tests/test_gpu_implicit_diffusion.py: Nx = 13 leaves most of the one wave of a
block row idle (and is no multiple of the wave width), Ny = 6 needs two blocks of four rows, Nz = 12 takes one full and one partial batch
of the column sweeps' eight-plane load batches (three batches of the four-plane ones of three or four fields swept together)."""
import ctypes as C

import numpy as np
import pytest

import convective_adjustment_numpy as CAN
import implicit_diffusion_numpy as IDN
from helpers import from_dev, stretched_faces, to_dev

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
P, B = "Periodic", "Bounded"
U, V, CC, CCF = 1, 2, 0, 4  # location masks
SEAWATER = ("SeawaterBuoyancy", 9.80665, 1.67e-4, 7.80e-4)
SENTINEL = -7.0
# size, z ("stretched" or an interval), halo (a halo is at most the size: Nz = 1, 2 take Hz = Nz)
CASES = [((13, 6, 12), "stretched", (3, 3, 3)),
         ((13, 6, 12), (-1.0, 0.0), (3, 3, 3)),
         ((13, 6, 1), (-1.0, 0.0), (3, 3, 1)),
         ((13, 6, 2), "stretched", (3, 3, 2)),
         ((13, 6, 12), "stretched", (4, 3, 5))]
IDS = ["stretched", "uniform", "Nz1", "Nz2", "halo435"]
NUMBERS = [0.1, 100.0]  # diffusion numbers Δt κ_max / min Δz²


def _grid(ocn, size, z, halo):
    zz = stretched_faces(size[2]) if isinstance(z, str) else z
    return ocn.RectilinearGrid(ocn.GPU(), size=size, x=(0, 1), y=(0, 0.5), z=zz, topology=(P, P, B), halo=halo)


_inputs = {}


def _case(ocn, n):
    """grid, its description, random parent arrays (halos included) of u, v, two tracers and their tendencies, the T and S of
    CAN.plateau_inputs, the κ field ConvectiveAdjustmentVerticalDiffusivity (background 0, convective 1) makes of them with x / y halos
    filled, and three random positive κ fields; shared, never modified"""
    if n not in _inputs:
        pg = _grid(ocn, *CASES[n])
        g = IDN.describe(pg)
        rng = np.random.default_rng(4242 + n)
        locs = {"u": U, "v": V, "c": CC, "c2": CC}
        f = {name: rng.uniform(-1, 1, pg.parent_shape(loc)) for name, loc in locs.items()}
        G = {name: rng.uniform(-1, 1, pg.parent_shape(loc)) for name, loc in locs.items()}
        T, S = CAN.plateau_inputs(g, 77 + n)
        zeros = np.zeros(CAN.ccf_shape(g))
        kc, _ = CAN.diffusivities(g, SEAWATER, T, S, 1.0, 1.0, 0.0, 0.0, zeros, zeros)
        rand = [rng.uniform(0.05, 1.0, CAN.ccf_shape(g)) for _ in range(3)]
        _inputs[n] = dict(pg=pg, g=g, f=f, G=G, T=T, S=S, cavd=CAN.fill_xy_halos(g, kc), rand=rand, locs=locs)
    return _inputs[n]


def _dzmin(g):
    return float(np.min(g.dzc[g.Hz:g.Hz + g.Nz]))


def _interior(g):
    return (slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny), slice(g.Hz, g.Hz + g.Nz))


def _assert_every_kind_of_face(N2):
    assert (N2 < 0).sum() >= 1 and (N2 > 0).sum() >= 1 and (N2 == 0).sum() >= 1


# ---- 1. the diffusivities, bit for bit --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("buoyancy", ["SeawaterBuoyancy", "BuoyancyTracer", None])
@pytest.mark.parametrize("n", range(len(CASES)), ids=IDS)
def test_diffusivities_equal_the_restatement_bit_for_bit(ocn, n, buoyancy):
    """κᶜ and κᵘ into arrays prefilled with a sentinel, whole parent arrays compared: only faces k = 1..Nz of the interior are written, face
    Nz + 1 and every halo keep the sentinel.  The inputs hold unstable, strictly stable and exactly neutral faces (asserted on the
    restatement's ∂z b); the neutral ones come out stable."""
    c = _case(ocn, n)
    pg, g, L = c["pg"], c["g"], ocn._lib
    spec = SEAWATER if buoyancy == "SeawaterBuoyancy" else buoyancy
    T, S = to_dev(ocn, pg, CC, c["T"]), to_dev(ocn, pg, CC, c["S"])
    terms = L.CModelTerms()
    if buoyancy == "SeawaterBuoyancy":
        terms.buoyancy, terms.g, terms.alpha, terms.beta, terms.T, terms.S = L.BUOYANCY_SEAWATER_TS, *SEAWATER[1:], T.ptr, S.ptr
    elif buoyancy == "BuoyancyTracer":
        terms.buoyancy, terms.T = L.BUOYANCY_TRACER, T.ptr
    coeffs = (1.0, 0.5, 1e-3, 1e-2)  # convective κ, ν, background κ, ν
    sentinel = np.full(CAN.ccf_shape(g), SENTINEL)
    kc, ku = to_dev(ocn, pg, CCF, sentinel), to_dev(ocn, pg, CCF, sentinel)
    L.call("ocn_compute_convective_adjustment_diffusivities", pg.cref, C.byref(terms), C.byref(L.CConvectiveAdjustment(*coeffs)), kc.ptr, ku.ptr, 0)
    ocn.sync_device()
    want_c, want_u = CAN.diffusivities(g, spec, c["T"], c["S"] if buoyancy == "SeawaterBuoyancy" else None, *coeffs, sentinel, sentinel)
    N2 = CAN.dz_b(g, spec, c["T"], c["S"])
    if buoyancy is None:
        assert np.all(want_c[_interior(g)] == 1e-3)
    else:
        _assert_every_kind_of_face(N2)
        assert np.all(want_c[_interior(g)][N2 == 0] == 1e-3) and np.all(want_u[_interior(g)][N2 < 0] == 0.5)
    got_c, got_u = from_dev(kc), from_dev(ku)
    assert np.array_equal(got_c, want_c) and np.array_equal(got_u, want_u)
    assert np.all(got_c[:, :, g.Hz + g.Nz:] == SENTINEL) and np.all(got_c[:g.Hx] == SENTINEL) and np.all(got_u[:, :g.Hy] == SENTINEL)


# ---- 2. the implicit step, bit for bit -------------------------------------------------------------------------------------------------------
def _device_step(ocn, c, names, kappas, dt):
    """one call over the fields `names` with the κ parents `kappas` (the same array object: the same device field); the scratch arrays carry
    a sentinel so that a write outside Nx Ny Nz doubles would show"""
    import torch
    pg, g, L = c["pg"], c["g"], ocn._lib
    dev = [to_dev(ocn, pg, c["locs"][name], c["f"][name]) for name in names]
    kdev, kptr = {}, []
    for k in kappas:
        if id(k) not in kdev:
            kdev[id(k)] = to_dev(ocn, pg, CCF, k)
        kptr.append(kdev[id(k)].ptr)
    n = g.Nx * g.Ny * g.Nz
    scratch = torch.full((len(names), n + 8), SENTINEL, dtype=torch.float64, device=dev[0].data.device)
    L.call("ocn_implicit_vertical_diffusion_step_fields", pg.cref, len(names), L.ptr_array([d.ptr for d in dev]),
           L.i32_array([c["locs"][name] for name in names]), L.ptr_array(kptr), L.ptr_array([scratch[q].data_ptr() for q in range(len(names))]),
           float(dt), 0)
    ocn.sync_device()
    assert torch.all(scratch[:, n:] == SENTINEL)
    return [from_dev(d) for d in dev]


_stepped = {}


def _cavd_step(ocn, n, number):
    """u, v and two tracers in ONE call with the κ field of the restatement's ConvectiveAdjustmentVerticalDiffusivity: the two tracers share
    one κ array (and with it one matrix: swept together), u and v average it in x and y"""
    if (n, number) not in _stepped:
        c = _case(ocn, n)
        dt = number * _dzmin(c["g"]) ** 2 / 1.0
        names = ("u", "v", "c", "c2")
        _stepped[(n, number)] = (dt, dict(zip(names, _device_step(ocn, c, names, [c["cavd"]] * 4, dt))))
    return _stepped[(n, number)]


@pytest.mark.parametrize("number", NUMBERS)
@pytest.mark.parametrize("n", range(len(CASES)), ids=IDS)
def test_implicit_step_with_the_convective_diffusivities_equals_the_restatement(ocn, n, number):
    """whole parent arrays compared (halos stay untouched).  The library's build of this file has no FMA contraction and IEEE division: no
    tolerance."""
    c = _case(ocn, n)
    g = c["g"]
    dt, got = _cavd_step(ocn, n, number)
    assert set(np.unique(c["cavd"][_interior(g)])) <= {0.0, 1.0} and (g.Nz == 1 or len(np.unique(c["cavd"][_interior(g)])) == 2)
    for name, a in got.items():
        want = CAN.implicit_step_fields(g, c["f"][name], c["locs"][name], c["cavd"], dt)
        assert np.isfinite(a).all()
        assert np.array_equal(a, want), f"{name}: max difference {np.abs(a - want).max():.3e}"
        if g.Nz > 1:  # (the Center rows of a single layer are the identity: nothing to diffuse against)
            assert not np.array_equal(a, c["f"][name])


@pytest.mark.parametrize("number", NUMBERS)
@pytest.mark.parametrize("n", range(len(CASES)), ids=IDS)
def test_implicit_step_with_random_diffusivities_equals_the_restatement(ocn, n, number):
    """the solver independently of the closure: uniformly random positive κ fields (halos included), a different one for each of the two
    tracers (two groups of one field) and a third for u and v"""
    c = _case(ocn, n)
    g = c["g"]
    dt = number * _dzmin(g) ** 2 / 1.0
    names = ("u", "v", "c", "c2")
    kappas = [c["rand"][0], c["rand"][0], c["rand"][1], c["rand"][2]]
    got = _device_step(ocn, c, names, kappas, dt)
    for name, kappa, a in zip(names, kappas, got):
        want = CAN.implicit_step_fields(g, c["f"][name], c["locs"][name], kappa, dt)
        assert np.isfinite(a).all()
        assert np.array_equal(a, want), f"{name}: max difference {np.abs(a - want).max():.3e}"
        if g.Nz > 1:
            assert not np.array_equal(a, c["f"][name])


def test_implicit_step_sweeps_groups_of_every_size(ocn):
    """one to six tracers that share a κ array: one thread sweeps up to four fields, a larger group takes a second launch"""
    c = _case(ocn, 0)
    pg, g = c["pg"], c["g"]
    rng = np.random.default_rng(8)
    dt = 100.0 * _dzmin(g) ** 2
    for count in (3, 4, 6):
        cc = dict(c, f={f"t{q}": rng.uniform(-1, 1, pg.parent_shape(CC)) for q in range(count)}, locs={f"t{q}": CC for q in range(count)})
        got = _device_step(ocn, cc, tuple(cc["f"]), [c["rand"][1]] * count, dt)
        for name, a in zip(cc["f"], got):
            assert np.array_equal(a, CAN.implicit_step_fields(g, cc["f"][name], CC, c["rand"][1], dt)), f"{count} fields: {name}"


# ---- 3. the constant-κ kernel as yardstick ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", range(len(CASES)), ids=IDS)
def test_constant_field_gives_the_constant_kappa_step_bit_for_bit(ocn, n):
    c = _case(ocn, n)
    pg, g, L = c["pg"], c["g"], ocn._lib
    kappa = 0.7
    dt = 100.0 * _dzmin(g) ** 2 / kappa
    names = ("u", "v", "c")
    got = _device_step(ocn, c, names, [np.full(CAN.ccf_shape(g), kappa)] * 3, dt)
    dev = [to_dev(ocn, pg, c["locs"][name], c["f"][name]) for name in names]
    L.call("ocn_implicit_vertical_diffusion_step", pg.cref, 3, L.ptr_array([d.ptr for d in dev]), L.i32_array([c["locs"][name] for name in names]),
           (C.c_double * 3)(kappa, kappa, kappa), dt, 0)
    ocn.sync_device()
    for name, a, d in zip(names, got, dev):
        assert np.array_equal(a, from_dev(d)), name


# ---- 4. the closure term, bit for bit ------------------------------------------------------------------------------------------------------------
def _fluxes_device(ocn, c, kappa_u, kappa_c, boundary_only, ranged=None, G=None, f=None):
    pg, L = c["pg"], ocn._lib
    f, G = f or c["f"], G or c["G"]
    names = ("u", "v", "c", "c2")
    df = {name: to_dev(ocn, pg, c["locs"][name], f[name]) for name in names}
    dG = {name: to_dev(ocn, pg, c["locs"][name], G[name]) for name in names}
    ku = to_dev(ocn, pg, CCF, kappa_u)
    kc = [to_dev(ocn, pg, CCF, k) for k in kappa_c]
    L.call("ocn_add_vertical_diffusivity_fluxes", pg.cref, ku.ptr, df["u"].ptr, df["v"].ptr, dG["u"].ptr, dG["v"].ptr, 2,
           L.ptr_array([k.ptr for k in kc]), L.ptr_array([df["c"].ptr, df["c2"].ptr]), L.ptr_array([dG["c"].ptr, dG["c2"].ptr]),
           int(boundary_only), None if ranged is None else L.i32_array(list(ranged)), 0)
    ocn.sync_device()
    return {name: from_dev(dG[name]) for name in names}


def _fluxes_expected(c, kappa_u, kappa_c, boundary_only, ranged=None, G=None, f=None):
    g = c["g"]
    f, G = f or c["f"], G or c["G"]
    Du, Dv, Dc = CAN.vertical_fluxes(g, kappa_u, f["u"], f["v"], kappa_c, [f["c"], f["c2"]], boundary_only)
    i0, i1, j0, j1, k0, k1 = ranged if ranged is not None else (1, g.Nx, 1, g.Ny, 1, g.Nz)  # (Periodic x, y: no periphery is excluded)
    out = {}
    for name, D in (("u", Du), ("v", Dv), ("c", Dc[0]), ("c2", Dc[1])):
        a = np.array(G[name])
        sl = (slice(i0 - 1, i1), slice(j0 - 1, j1), slice(k0 - 1, k1))
        psl = tuple(slice(H + s.start, H + s.stop) for H, s in zip((g.Hx, g.Hy, g.Hz), sl))
        a[psl] = a[psl] - D[sl]
        out[name] = a
    return out


@pytest.mark.parametrize("boundary_only", [0, 1], ids=["explicit", "boundary_only"])
@pytest.mark.parametrize("n", range(len(CASES)), ids=IDS)
def test_fluxes_equal_the_restatement_bit_for_bit(ocn, n, boundary_only):
    """G - (closure term) for u, v and two tracers with random positive ν and κ fields (a field of its own for each tracer), whole parent
    arrays compared: the halos and everything outside a range keep their values.  No tolerance (strict build)."""
    c = _case(ocn, n)
    g = c["g"]
    ku, kc = c["rand"][0], [c["rand"][1], c["rand"][2]]
    for ranged in (None, (2, g.Nx - 1, 1, max(1, g.Ny - 1), 1, g.Nz), (1, g.Nx, 2, g.Ny, min(2, g.Nz), g.Nz)):
        want = _fluxes_expected(c, ku, kc, boundary_only, ranged)
        got = _fluxes_device(ocn, c, ku, kc, boundary_only, ranged)
        for name in want:
            assert np.isfinite(got[name]).all()
            assert np.array_equal(got[name], want[name]), f"range {ranged} {name}: max difference {np.abs(got[name] - want[name]).max():.3e}"
            assert not np.array_equal(got[name], c["G"][name])


# ---- 5. the explicit isotropic closure as yardstick ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("z", ["stretched", (-1.0, 0.0)], ids=["stretched", "uniform"])
def test_explicit_term_equals_the_isotropic_closure_on_horizontally_uniform_fields(ocn, z):
    """Fields that depend on k only (random in k, w = 0) and ν, κ fields filled with one constant: every horizontal flux of the EXISTING
    isotropic closure (closure = 1: ocn_add_momentum_terms on G = 0, and ocn_compute_tracer_tendency_terms with a fluid at rest, whose
    advective part is exactly zero) vanishes and its vertical fluxes are -2 (ν (0.5 (∂z u + 0))) = -(ν ∂z u): the boundary_only = 0 term must
    equal it.  Bound: the same identity evaluated with the two restatements alone on the CPU (IDN all-explicit against CAN), times 10 --
    operand by operand both come out bit-identical, so the bound is 0."""
    pg = _grid(ocn, (13, 6, 12), z, (3, 3, 3)).with_math_mode(ocn.MATH_STRICT)
    g = IDN.describe(pg)
    L = ocn._lib
    rng = np.random.default_rng(12)
    nu, kappa = 0.6, 0.8
    prof = {name: rng.uniform(-1, 1, g.Nz + 2 * g.Hz) for name in ("u", "v", "c")}
    f = {name: np.broadcast_to(prof[name], pg.parent_shape(loc)).copy() for name, loc in (("u", U), ("v", V), ("c", CC))}
    f["w"] = np.zeros(pg.parent_shape(CCF))
    sl = _interior(g)
    du, dv, dw, dc = (to_dev(ocn, pg, loc, f[name]) for name, loc in (("u", U), ("v", V), ("w", CCF), ("c", CC)))
    Gu, Gv, Gw, Gc = (ocn.Field(loc, pg) for loc in (U, V, CCF, CC))
    terms = L.CModelTerms()
    terms.closure, terms.nu = 1, nu
    L.call("ocn_add_momentum_terms", pg.cref, C.byref(terms), du.ptr, dv.ptr, dw.ptr, Gu.ptr, Gv.ptr, Gw.ptr, None, 0)
    rest = [ocn.Field(loc, pg) for loc in (U, V, CCF)]
    L.call("ocn_compute_tracer_tendency_terms", pg.cref, C.byref(terms), kappa, None, rest[0].ptr, rest[1].ptr, rest[2].ptr, dc.ptr, Gc.ptr, None, 0)
    ocn.sync_device()
    existing = {"u": from_dev(Gu)[sl], "v": from_dev(Gv)[sl], "c": from_dev(Gc)[sl]}
    case = dict(pg=pg, g=g, locs={"u": U, "v": V, "c": CC, "c2": CC})
    ff = dict(f, c2=f["c"])
    zeros = {name: np.zeros(pg.parent_shape(loc)) for name, loc in case["locs"].items()}
    knu, kka = np.full(CAN.ccf_shape(g), nu), np.full(CAN.ccf_shape(g), kappa)
    new = _fluxes_device(ocn, case, knu, [kka, kka], 0, G=zeros, f=ff)
    Fu, Fv, _ = IDN.momentum_explicit_part(g, nu, f["u"], f["v"], f["w"], all_explicit=True)
    Fc = IDN.tracer_explicit_part(g, kappa, f["c"], all_explicit=True)
    Du, Dv, Dc = CAN.vertical_fluxes(g, knu, f["u"], f["v"], [kka], [f["c"]], False)
    for name, old, mine in (("u", Fu, Du), ("v", Fv, Dv), ("c", Fc, Dc[0])):
        cpu = np.abs(-old - (-mine)).max()
        gpu = np.abs(existing[name] - new[name][sl]).max()
        print(f"{name}: restatements alone {cpu:.3e}, GPU {gpu:.3e}, max |term| {np.abs(existing[name]).max():.3e}")
        assert np.abs(existing[name]).max() > 1.0
        assert gpu <= 10 * cpu


@pytest.mark.parametrize("z", ["stretched", (-1.0, 0.0)], ids=["stretched", "uniform"])
def test_explicit_term_is_boundary_term_plus_implicit_operator(ocn, z):
    """For general fields and the κ field of the restatement's closure (background 0.05, convective 1): the boundary_only = 0 term equals the
    boundary_only = 1 term plus (φ - A φ) / Δt, A assembled column by column by the restatement -- what the tendencies lose, the implicit
    step gives back.  Bound: 10 times what the same identity is off by with the restatement alone on the CPU (about 1e-15 of the largest
    term: the cancellation in φ - A φ at Δt = 0.1 min Δz² / κ, divided by Δt)."""
    n = 0 if z == "stretched" else 1
    c = _case(ocn, n)
    g = c["g"]
    kappa = np.where(c["cavd"] == 1.0, 1.0, 0.05)
    dt = 0.1 * _dzmin(g) ** 2
    zeros = {name: np.zeros_like(a) for name, a in c["G"].items()}
    full = _fluxes_device(ocn, c, kappa, [kappa, kappa], 0, G=zeros)
    edge = _fluxes_device(ocn, c, kappa, [kappa, kappa], 1, G=zeros)
    Du, Dv, Dc = CAN.vertical_fluxes(g, kappa, c["f"]["u"], c["f"]["v"], [kappa], [c["f"]["c"]], False)
    Eu, Ev, Ec = CAN.vertical_fluxes(g, kappa, c["f"]["u"], c["f"]["v"], [kappa], [c["f"]["c"]], True)
    sl = _interior(g)
    for name, Df, De in (("u", Du, Eu), ("v", Dv, Ev), ("c", Dc[0], Ec[0])):
        implicit = np.zeros_like(Df)
        for i in range(1, g.Nx + 1):
            for j in range(1, g.Ny + 1):
                a, b, cc = CAN.diagonals_fields(g, dt, CAN.kappa_z_column(g, kappa, c["locs"][name], i, j))
                phi = c["f"][name][sl][i - 1, j - 1]
                implicit[i - 1, j - 1] = (phi - IDN.apply_matrix(a, b, cc, phi)) / dt
        cpu = np.abs(-Df - (-De + implicit)).max()
        gpu = np.abs(full[name][sl] - (edge[name][sl] + implicit)).max()
        scale = np.abs(full[name][sl]).max()
        print(f"{name}: restatement alone {cpu:.3e}, GPU {gpu:.3e}, max |term| {scale:.3e}")
        assert cpu <= 1e-12 * scale, "the restatement itself does not split the term"
        assert gpu <= 10 * cpu
        assert np.abs(implicit).max() > 0.1 * scale  # (the implicit operator carries most of the term: the identity is not vacuous)


# ---- 6. model steps against the composed sequence ---------------------------------------------------------------------------------------------
COEFFS = dict(convective_κz=1.0, background_κz=1e-3, convective_νz=0.5, background_νz=1e-2)
T_FLUX = 1e-3  # upward heat flux through the top: cooling


def _model_grid(ocn):
    """z refined towards the bottom (Δz from 0.019 to 0.13), Δx = Δy = 1 (tests/test_gpu_implicit_diffusion.py)"""
    faces = -1.0 + np.linspace(0.0, 1.0, 13) ** 1.6
    return ocn.RectilinearGrid(ocn.GPU(), size=(13, 6, 12), x=(0, 13), y=(0, 6), z=faces, topology=(P, P, B), halo=(3, 3, 3))


def _free_surface(ocn, kind):
    return {"explicit": lambda: ocn.ExplicitFreeSurface(), "split": lambda: ocn.SplitExplicitFreeSurface(substeps=10),
            "implicit": lambda: ocn.ImplicitFreeSurface()}[kind]()


def _initial(pg):
    """a stable lower half under an unstable upper half (T falls towards the surface there), noise on everything"""
    rng = np.random.default_rng(9)
    zc = np.asarray(pg.nodes_1d(2, False))[:12]
    T = 20 + np.where(zc < -0.5, 2.0 * (zc + 0.5), -1.5 * (zc + 0.5))
    init = {n: 1e-3 * rng.uniform(-1, 1, (13, 6, 12)) for n in "uv"}
    init["T"] = np.broadcast_to(T, (13, 6, 12)) + 0.05 * rng.uniform(-1, 1, (13, 6, 12))
    init["S"] = 35 + 0.01 * rng.uniform(-1, 1, (13, 6, 12))
    return init


def _upload(field, a):
    import torch
    field.data.copy_(torch.from_numpy(np.ascontiguousarray(a.T)))


class _Twin:
    """a HydrostaticFreeSurfaceModel WITHOUT closure stepped through its public stage functions and the library's entry points in the order
    of hydrostatic.py time_step (fused = False), with the three new pieces done by the restatement on the host"""

    def __init__(self, ocn, r, implicit):
        self.ocn, self.r, self.implicit = ocn, r, implicit
        self.g = IDN.describe(r.grid)
        self.kappa_c = self.kappa_u = None

    def update_state(self):
        from oceananigans_jl_amd import models
        r, g = self.r, self.g
        r.update_state(compute_tendencies=False)
        T, S = r.field("T").parent(), r.field("S").parent()
        zeros = np.zeros(CAN.ccf_shape(g))
        spec = ("SeawaterBuoyancy", r._nh.buoyancy.gravitational_acceleration, r._nh.buoyancy.equation_of_state.thermal_expansion,
                r._nh.buoyancy.equation_of_state.haline_contraction)
        kc, ku = CAN.diffusivities(g, spec, T, S, COEFFS["convective_κz"], COEFFS["convective_νz"], COEFFS["background_κz"],
                                   COEFFS["background_νz"], zeros if self.kappa_c is None else self.kappa_c,
                                   zeros if self.kappa_u is None else self.kappa_u)
        self.kappa_c, self.kappa_u = CAN.fill_xy_halos(g, kc), CAN.fill_xy_halos(g, ku)
        r.compute_tendencies(boundary_contributions=False)
        Gn = r._nh.timestepper._Gn
        tracers = [c.parent() for c in r.tracers]
        Du, Dv, Dc = CAN.vertical_fluxes(g, self.kappa_u, r.u.parent(), r.v.parent(), [self.kappa_c] * len(tracers), tracers, self.implicit)
        sl = _interior(g)
        for q, D in zip([0, 1] + [3 + n for n in range(len(tracers))], [Du, Dv] + Dc):
            a = Gn[q].parent()
            a[sl] = a[sl] - D
            _upload(Gn[q], a)
        models.compute_boundary_tendency_contributions(r._nh)

    def time_step(self, dt):
        ocn, r, g = self.ocn, self.r, self.g
        L, nh, clock, s, pg = ocn._lib, r._nh, r.clock, 0, r.grid
        if clock.iteration == 0:
            if r.split and not r._initialized:
                L.call("ocn_compute_barotropic_mode", pg.cref, r.u.ptr, r.v.ptr, r.U.data_ptr(), r.V.data_ptr(), s)
                r._initialized = True
            self.update_state()
        chi = -0.5 if dt != clock.last_dt else nh.timestepper.chi
        Gn, Gm = nh.timestepper._Gn, nh.timestepper._Gm
        idx = [0, 1] + [3 + n for n in range(len(r.tracers))]
        fields = [r.u, r.v] + list(r.tracers)
        L.call("ocn_ab2_step", pg.cref, len(idx), L.ptr_array([f.ptr for f in fields]), L.ptr_array([Gn[q].ptr for q in idx]),
               L.ptr_array([Gm[q].ptr for q in idx]), L.i32_array([f.loc for f in fields]), float(dt), float(chi), s)
        if self.implicit:  # with the diffusivities of the last update_state
            for f in fields:
                _upload(f, CAN.implicit_step_fields(g, f.parent(), f.loc, self.kappa_u if f.loc in (U, V) else self.kappa_c, dt))
        fs = r.free_surface
        if r.split:
            L.call("ocn_split_explicit_forcing", pg.cref, Gn[0].ptr, Gm[0].ptr, Gn[1].ptr, Gm[1].ptr, float(chi), r._GU.data_ptr(), r._GV.data_ptr(), s)
            r._substep_free_surface(dt, s)
            L.call("ocn_barotropic_split_explicit_corrector", pg.cref, r.u.ptr, r.v.ptr, r.U.data_ptr(), r.V.data_ptr(), r._Ub.data_ptr(),
                   r._Vb.data_ptr(), float(pg.Lz), s)
        elif r.implicit:
            L.call("ocn_implicit_free_surface_rhs", pg.cref, r.u.ptr, r.v.ptr, r.eta.data_ptr(), fs.gravitational_acceleration, float(dt),
                   r._Qu.data_ptr(), r._Qv.data_ptr(), r._fs_rhs.data_ptr(), s)
            h = r._fs_solver._h
            L.call("ocn_poisson_set_source_term", h, r._fs_rhs.data_ptr(), s)
            L.call("ocn_poisson_solve_shifted", h, r.eta.data_ptr(), -1.0 / (fs.gravitational_acceleration * float(pg.Lz) * float(dt) ** 2), s)
            r._fill_eta_halos()
            L.call("ocn_barotropic_pressure_correction", pg.cref, r.u.ptr, r.v.ptr, r.eta.data_ptr(), fs.gravitational_acceleration, float(dt), s)
        else:
            L.call("ocn_explicit_free_surface_ab2_step", pg.cref, r.w.ptr, r.eta.data_ptr(), r._Geta.data_ptr(), r._Geta_m.data_ptr(), float(dt),
                   float(chi), s)
        clock.time += dt
        clock.iteration += 1
        clock.last_dt = dt
        clock.last_stage_dt = dt
        nh.timestepper._Gn, nh.timestepper._Gm = Gm, Gn
        r._Geta, r._Geta_m = r._Geta_m, r._Geta
        self.update_state()


def _run_model_against_twin(ocn, kind, td, dt_number):
    pg = _model_grid(ocn)
    closure = ocn.ConvectiveAdjustmentVerticalDiffusivity(td, **COEFFS)
    bcs = lambda: {"T": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(T_FLUX))}
    kw = dict(tracers=("T", "S"), buoyancy=ocn.SeawaterBuoyancy(), coriolis=ocn.FPlane(f=1e-4), math_mode=ocn.MATH_STRICT)
    m = ocn.HydrostaticFreeSurfaceModel(pg, closure=closure, boundary_conditions=bcs(), free_surface=_free_surface(ocn, kind), **kw)
    r = ocn.HydrostaticFreeSurfaceModel(pg, closure=None, boundary_conditions=bcs(), free_surface=_free_surface(ocn, kind), fused=False, **kw)
    assert m.fused is False and sorted(m.diffusivity_fields) == ["kappa_c", "kappa_u"]
    g = IDN.describe(m.grid)
    for f in m.diffusivity_fields.values():  # ZFaceFields, zero at creation apart from what the first update_state wrote
        assert f.loc == CCF and f.parent().shape == CAN.ccf_shape(g) and np.all(f.parent()[:, :, g.Hz + g.Nz:] == 0)
    init = _initial(pg)
    m.set(**init)
    r.set(**init)
    twin = _Twin(ocn, r, isinstance(closure.time_discretization, ocn.VerticallyImplicitTimeDiscretization))
    dt = dt_number * _dzmin(g) ** 2 / COEFFS["convective_κz"]
    for step in range(5):
        m.time_step(dt)
        twin.time_step(dt)
        kc, ku = m.diffusivity_fields["kappa_c"], m.diffusivity_fields["kappa_u"]
        assert np.array_equal(kc.parent(), twin.kappa_c) and np.array_equal(ku.parent(), twin.kappa_u), f"step {step}"
        assert set(np.unique(kc.interior()[:, :, :12])) == {1e-3, 1.0} and set(np.unique(ku.interior()[:, :, :12])) == {1e-2, 0.5}
    ocn.sync_device()
    for name in ("u", "v", "w", "T", "S"):
        a, b = m.field(name).parent(), r.field(name).parent()
        print(f"{kind} {td} {name}: max |value| after five steps {np.abs(a).max():.3e}")
        assert np.isfinite(a).all(), name
        assert np.array_equal(a, b), f"{name}: max difference {np.abs(a - b).max():.3e}"
    assert np.array_equal(m.eta.cpu().numpy(), r.eta.cpu().numpy())
    for Gm_, Gr_ in zip(m._nh.timestepper._Gn, r._nh.timestepper._Gn):
        assert np.array_equal(Gm_.parent(), Gr_.parent())
    assert np.abs(m.u.interior()).max() > 0 and np.abs(m.eta.cpu().numpy()).max() > 0
    return m, init


@pytest.mark.parametrize("kind", ["explicit", "split", "implicit"])
def test_hydrostatic_model_steps_equal_the_composed_sequence(ocn, kind):
    """Five QAB2 steps at diffusion number Δt convective_κz / min Δz² = 20 on a stretched z with SeawaterBuoyancy, T and S, an FPlane and a
    cooling flux through the top, from a state whose upper half is unstable, with each of the three free surfaces: u, v, w, η, the
    tracers and the tendencies bit for bit (strict math), κᶜ and κᵘ (whole parent arrays, both coefficient values present) after every step."""
    m, init = _run_model_against_twin(ocn, kind, "VerticallyImplicit", 20.0)
    # the unstable half is being mixed: the spread of T over it has shrunk
    assert m.field("T").interior()[:, :, 8:].std() < init["T"][:, :, 8:].std()


def test_hydrostatic_model_with_the_explicit_discretization_equals_the_composed_sequence(ocn):
    """the same with ExplicitTimeDiscretization at a stable step (diffusion number 0.2): no implicit step, every vertical flux in the tendencies"""
    _run_model_against_twin(ocn, "split", "Explicit", 0.2)


# ---- 7. maximum principle and conservation of the device result ---------------------------------------------------------------------------
@pytest.mark.parametrize("number", NUMBERS)
@pytest.mark.parametrize("n", range(len(CASES)), ids=IDS)
def test_tracer_columns_stay_within_their_bounds_and_keep_their_integral(ocn, n, number):
    """On the device result of the convective case: backward Euler with an M-matrix (positive diagonal, non-positive off-diagonals, rows
    of A summing to 1) keeps every column within [min, max] of its input, and the Center rows keep Σ Δz φ.  Both to 10 cond(A) ε, cond from
    the restatement's matrix of that column, relative to max |φ| of the column / to Σ Δz |φ|."""
    c = _case(ocn, n)
    g = c["g"]
    dt, got = _cavd_step(ocn, n, number)
    dz = g.dzc[g.Hz:g.Hz + g.Nz]
    sl = _interior(g)
    worst = 0.0
    for name in ("c", "c2"):
        before, after = c["f"][name][sl], got[name][sl]
        for i in range(1, g.Nx + 1):
            for j in range(1, g.Ny + 1):
                a, b, cc = CAN.diagonals_fields(g, dt, CAN.kappa_z_column(g, c["cavd"], CC, i, j))
                tol = 10 * np.linalg.cond(IDN.dense_matrix(a, b, cc)) * EPS
                x0, x1 = before[i - 1, j - 1], after[i - 1, j - 1]
                slack = tol * np.abs(x0).max()
                assert x1.min() >= x0.min() - slack and x1.max() <= x0.max() + slack
                err = abs((dz * x1).sum() - (dz * x0).sum()) / (dz * np.abs(x0)).sum()
                worst = max(worst, err / tol)
                assert err <= tol
    print(f"case {IDS[n]} number {number}: worst conservation error {worst:.3g} of the tolerance")


# ---- 8. the README snippet -----------------------------------------------------------------------------------------------------------------
def test_readme_snippet_constructs_and_steps(ocn):
    grid = _model_grid(ocn)
    closure = ocn.ConvectiveAdjustmentVerticalDiffusivity(convective_κz=1.0, background_κz=1e-5, convective_νz=0.1, background_νz=1e-4)
    model = ocn.HydrostaticFreeSurfaceModel(grid, tracers=("T", "S"), buoyancy=ocn.SeawaterBuoyancy(), closure=closure)
    model.set(T=lambda x, y, z: 20 - 2 * np.abs(z + 0.5) + 0 * x + 0 * y, S=35.0)
    model.time_step(1e-2)
    ocn.sync_device()
    kappa = model.diffusivity_fields["kappa_c"].interior()
    assert set(np.unique(kappa[:, :, :12])) == {1e-5, 1.0}
    for f in model._nh.prognostic_fields():
        assert np.isfinite(f.interior()).all()
    # the other buoyancy formulations construct and step too: b itself, and none (every face stable)
    for kw in (dict(tracers=("b",), buoyancy=ocn.BuoyancyTracer()), dict(tracers=("c",), buoyancy=None)):
        h = ocn.HydrostaticFreeSurfaceModel(grid, closure=closure, **kw)
        h.set(**{kw["tracers"][0]: lambda x, y, z: -np.abs(z + 0.5) + 0 * x + 0 * y})
        h.time_step(1e-2)
        ocn.sync_device()
        k = h.diffusivity_fields["kappa_c"].interior()[:, :, :12]
        assert set(np.unique(k)) == ({1e-5, 1.0} if kw["buoyancy"] is not None else {1e-5})
