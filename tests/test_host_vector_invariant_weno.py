"""The upwinding vector-invariant momentum advection without a GPU: the constructor rules of VectorInvariant / WENOVectorInvariant and
their refusals (before any allocation), the halo a model ends up with, the argument checks of
ocn_compute_vector_invariant_weno_momentum_tendencies (no device is touched), and the NumPy restatement
(tests/vector_invariant_weno_numpy.py) pinned to what is certain independently of its author: a uniform flow, the linear scheme behind the
weights, the symmetry of the equations under a swap of x and y, the CPU oracle's flux-form WENO for the vertical fluxes, and the order
of accuracy on a Taylor-Green flow."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import vector_invariant_weno_numpy as VIN
from helpers import stretched_faces

P, B = "Periodic", "Bounded"
INVALID, UNSUPPORTED = -1, -2  # OCN_ERR_INVALID_ARGUMENT, OCN_ERR_UNSUPPORTED (include/ocn_hip.h)
EPS = np.finfo(np.float64).eps
# every accepted combination of sub-schemes, and both vorticity stencils where the vorticity scheme is WENO
VARIANTS = [(name, stencil) for name, s in VIN.SCHEMES.items() for stencil in (("velocity", "default") if s.vorticity == VIN.W else ("velocity",))]
VARIANT_IDS = [f"{n}-{st}" for n, st in VARIANTS]


def _scheme(name, stencil):
    return VIN.SCHEMES[name]._replace(stencil=stencil)


def _describe(size, halo, dx, dy, faces=None, dz=None):
    """the grid description the restatement reads (tests/implicit_diffusion_numpy.py `describe`), built without the package"""
    Nz, Hz = size[2], halo[2]
    if faces is None:
        dzc = dzf = np.full(Nz + 2 * Hz, float(dz))
    else:
        from oracle import oracle as O
        og = O.Grid(size, x=(0, dx * size[0]), y=(0, dy * size[1]), z=faces, topology="PPB", halo=halo)
        dzc, dzf = np.array(og.dzc[:Nz + 2 * Hz]), np.array(og.dzf[:Nz + 2 * Hz])
    return SimpleNamespace(Nx=size[0], Ny=size[1], Nz=Nz, Hx=halo[0], Hy=halo[1], Hz=Hz, topo=(P, P, B), dx=float(dx), dy=float(dy), dzc=dzc, dzf=dzf)


def _shape(g):
    return (g.Nx + 2 * g.Hx, g.Ny + 2 * g.Hy, g.Nz + 2 * g.Hz)


def _w_shape(g):
    return (g.Nx + 2 * g.Hx, g.Ny + 2 * g.Hy, g.Nz + 2 * g.Hz + 1)


@pytest.fixture(scope="module")
def pkg():
    import oceananigans_jl_amd as ocn
    return ocn


# ---- 1. the restatement -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,stencil", VARIANTS, ids=VARIANT_IDS)
def test_a_uniform_flow_has_no_tendency(name, stencil):
    """u = 0.3, v = -0.2, w = 0 everywhere: every difference is exactly 0, every reconstruction of zeros is 0 whatever its weights, and
    so Gu = Gv = 0 exactly (and finite: the weights of a constant stencil are not 0 / 0)"""
    g = _describe((7, 6, 5), (3, 3, 3), 0.5, 0.25, faces=stretched_faces(5))
    u, v, w = np.full(_shape(g), 0.3), np.full(_shape(g), -0.2), np.zeros(_w_shape(g))
    Gu, Gv = VIN.tendencies(g, _scheme(name, stencil), u, v, w)
    assert Gu.shape == (7, 6, 5) and np.all(Gu == 0) and np.all(Gv == 0)


def test_weno5_of_the_restatement_is_the_oracles():
    """the reconstruction with its own smoothness equals ocn_oracle_weno5 bit for bit on random stencils of both biases (zeros included)"""
    from oracle import oracle as O
    L = O.lib()
    rng = np.random.default_rng(11)
    for trial in range(200):
        S = rng.uniform(-1, 1, 6)
        if trial % 7 == 0:
            S[rng.integers(0, 6, 2)] = 0.0
        for left in (0, 1):
            want = L.ocn_oracle_weno5(S.ctypes.data_as(C.c_void_p), left)
            got = float(VIN.weno5([np.float64(x) for x in S], bool(left)))
            assert got == want
            S4 = np.ascontiguousarray(S[:4])
            assert float(VIN.weno3([np.float64(x) for x in S4], bool(left))) == L.ocn_oracle_weno3(S4.ctypes.data_as(C.c_void_p), left)
    S4 = rng.uniform(-1, 1, 4)
    assert float(VIN.centered4(list(S4))) == L.ocn_oracle_centered4(S4.ctypes.data_as(C.c_void_p))


def test_optimal_weights_give_the_fifth_order_upwind_stencil():
    """ω = C★ turns every WENO reconstruction (whatever its smoothness stencil) into UpwindBiased(order=5): equal to the oracle's
    upwind5 -- the stencil of csrc/ocn_weno.h -- to 1e-15 of the largest stencil value, on a seeded sample.  (Both sides sum five products
    of magnitude <= 0.79 max|S|, the WENO side through three partial sums: a few units of eps / 2 each.)"""
    from oracle import oracle as O
    L = O.lib()
    rng = np.random.default_rng(12)
    worst = 0.0
    for _ in range(500):
        S = rng.uniform(-1, 1, 6)
        other = [np.float64(x) for x in rng.uniform(-1, 1, 6)]
        for left in (0, 1):
            want = L.ocn_oracle_upwind5(S.ctypes.data_as(C.c_void_p), left)
            assert float(VIN.upwind5([np.float64(x) for x in S], bool(left))) == want
            for smoothness in (None, other, [other, other[::-1]]):
                got = float(VIN.weno5([np.float64(x) for x in S], bool(left), smoothness, optimal_weights=True))
                worst = max(worst, abs(got - want) / np.abs(S).max())
    print(f"largest relative difference {worst:.3e}")
    assert worst <= 1e-15


def _random_inputs(g, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, _shape(g)), rng.uniform(-1, 1, _shape(g)), rng.uniform(-1, 1, _w_shape(g))


@pytest.mark.parametrize("name,stencil", VARIANTS, ids=VARIANT_IDS)
def test_swapping_x_and_y_swaps_the_tendencies_bit_for_bit(name, stencil):
    """On the grid with Δx and Δy (and the sizes and halos) swapped, u' = vᵀ, v' = uᵀ, w' = wᵀ give Gu' = Gvᵀ and Gv' = Guᵀ exactly: ζ
    changes sign exactly, a reconstruction is odd in its values and even in its smoothness, and the sums the swap reorders have two terms."""
    g = _describe((9, 7, 6), (3, 4, 3), 0.5, 0.3, faces=stretched_faces(6))
    gt = _describe((7, 9, 6), (4, 3, 3), 0.3, 0.5, faces=stretched_faces(6))
    u, v, w = _random_inputs(g, 21)
    eta = np.random.default_rng(22).uniform(-1, 1, _shape(g)[:2])
    s = _scheme(name, stencil)
    T = lambda a: np.ascontiguousarray(np.swapaxes(a, 0, 1))
    Gu, Gv = VIN.tendencies(g, s, u, v, w, eta, 9.8)
    Gut, Gvt = VIN.tendencies(gt, s, T(v), T(u), T(w), T(eta), 9.8)
    assert np.isfinite(Gu).all() and np.abs(Gu).max() > 0.1
    assert np.array_equal(Gut, T(Gv)) and np.array_equal(Gvt, T(Gu))


@pytest.mark.parametrize("stretched", [False, True], ids=["regular", "stretched"])
def test_vertical_flux_difference_is_the_flux_form_oracles(stretched):
    """The CPU oracle does not expose the z part of its flux-form WENO momentum advection on its own, but inputs isolate it: with
    u = u(y, z) and v = 0 the x fluxes of u cancel exactly and the y fluxes vanish, so the oracle's Gu is -(1 / V) δz F_Wu bit for bit
    (and with v = v(x, z), u = 0 its Gv is -(1 / V) δz F_Wv).  w is random, of both signs, on every face.  Nz = 9: faces 4 .. 7 are of
    full order, 3 and 8 of order 3, the others of order 1."""
    from oracle import oracle as O
    size, halo = (6, 5, 9), (3, 3, 3)
    faces = stretched_faces(9) if stretched else (-1.0, 0.0)
    og = O.Grid(size, x=(0, 3.0), y=(0, 2.0), z=faces, topology="PPB", halo=halo)
    g = _describe(size, halo, og.dx, og.dy, faces=faces if stretched else None, dz=None if stretched else og.dz)
    rng = np.random.default_rng(31)
    w = np.asfortranarray(rng.uniform(-1, 1, og.shape(O.LOC_W)))
    assert w.shape == _w_shape(g)
    vol = (g.dx * g.dy) * g.dzc[g.Hz:g.Hz + g.Nz].reshape(1, 1, -1)
    for which in (0, 1):
        profile = rng.uniform(-1, 1, _shape(g))
        f = np.asfortranarray(np.broadcast_to(profile[:1, :, :] if which == 0 else profile[:, :1, :], _shape(g)))
        zero = og.zeros(O.LOC_C)
        u, v = (f, zero) if which == 0 else (zero, f)
        G = [og.zeros(O.LOC_U), og.zeros(O.LOC_V), og.zeros(O.LOC_W)]
        O.momentum_tendencies(og, u, v, w, *G)
        A = VIN.vertical_flux_differences(g, u, v, w)[which]
        assert np.abs(A).max() > 1e-2
        assert np.array_equal(og.interior_N(G[which]), -(1 / vol * A))


@pytest.mark.parametrize("name,stencil", VARIANTS, ids=VARIANT_IDS)
def test_taylor_green_error_falls_at_second_order(name, stencil):
    """the flow and the threshold of test_vector_invariant_advection_is_second_order (tests/test_oracle_hydrostatic.py): the error of
    U·∇u against (k / 2) sin(2 k x) falls by more than 3.5 from N = 16 to N = 32"""
    errs = []
    L = 2.0e3
    k = 2 * np.pi / L
    for N in (16, 32):
        g = _describe((N, N, 4), (3, 3, 3), L / N, L / N, dz=10.0)
        xc, xf = (np.arange(N) + 0.5) * g.dx, np.arange(N) * g.dx
        u0 = np.sin(k * xf)[:, None, None] * np.cos(k * xc)[None, :, None] * np.ones((1, 1, 4))
        v0 = -np.cos(k * xc)[:, None, None] * np.sin(k * xf)[None, :, None] * np.ones((1, 1, 4))
        wrap = lambda a: np.pad(a, ((3, 3), (3, 3), (3, 3)), mode="wrap")  # (periodic images; z: the flow is uniform in z and w = 0)
        Gu, _ = VIN.tendencies(g, _scheme(name, stencil), wrap(u0), wrap(v0), np.zeros(_w_shape(g)))
        exact = 0.5 * k * np.sin(2 * k * xf)[:, None, None] * np.ones((1, N, 4))
        errs.append(np.abs(-Gu - exact).max())
    print(f"errors {errs[0]:.3e} {errs[1]:.3e} ratio {errs[0] / errs[1]:.2f}")
    assert errs[0] / errs[1] > 3.5


# ---- 2. constructors ----------------------------------------------------------------------------------------------------------------
def test_accepted_spellings(pkg):
    VI, WVI, WENO = pkg.VectorInvariant, pkg.WENOVectorInvariant, pkg.WENO
    EC, ENS = pkg.EnergyConserving, pkg.EnstrophyConserving
    F = VIN
    table = [
        (VI(), 0, (1, 1, 1)),
        (WVI(order=5), F.FLAG_VORTICITY | F.FLAG_VERTICAL | F.FLAG_KINETIC_ENERGY, (4, 4, 3)),
        (WVI(vorticity_order=5), 7, (4, 4, 3)),
        (WVI(order=5, vorticity_stencil=pkg.DefaultStencil()), 15, (4, 4, 3)),
        (WVI(order=5, upwinding=pkg.OnlySelfUpwinding(cross_scheme=WENO())), 7, (4, 4, 3)),
        (VI(vorticity_scheme=WENO(), vertical_scheme=WENO()), 7, (4, 4, 3)),                       # the reference's docstring example at order 5
        (VI(vorticity_scheme=WENO()), 1, (4, 4, 1)),                                               # WENO vorticity, conserving vertical terms
        (VI(vorticity_scheme=WENO(), vorticity_stencil=pkg.DefaultStencil()), 9, (4, 4, 1)),
        (VI(vorticity_scheme=WENO(), vertical_scheme=WENO(), kinetic_energy_gradient_scheme=EC()), 3, (4, 4, 3)),
        (VI(vertical_scheme=WENO()), 6, (4, 4, 3)),
        (VI(vertical_scheme=WENO(), kinetic_energy_gradient_scheme=EC()), 2, (4, 4, 3)),
        (VI(vorticity_scheme=ENS(), vertical_scheme=EC(), divergence_scheme=EC(), kinetic_energy_gradient_scheme=EC()), 0, (1, 1, 1)),
    ]
    for scheme, flags_, halo in table:
        assert scheme.scheme_flags == flags_, scheme
        assert scheme.required_halo == halo, scheme
        assert scheme.upwinds == bool(flags_ & 7)
    for name, s in VIN.SCHEMES.items():  # the restatement's table and the package's agree on what exists
        kw = dict(vorticity_scheme=WENO() if s.vorticity == VIN.W else None, vertical_scheme=WENO() if s.vertical == VIN.W else None,
                  kinetic_energy_gradient_scheme=WENO() if s.kinetic_energy == VIN.W else EC())
        assert VI(**kw).scheme_flags == VIN.flags(s), name
    # the defaulting chain (vector_invariant_advection.jl:104-110)
    a = VI(vertical_scheme=WENO())
    assert a.divergence_scheme is a.vertical_scheme and a.kinetic_energy_gradient_scheme is a.divergence_scheme
    assert isinstance(a.upwinding, pkg.OnlySelfUpwinding) and a.upwinding.cross_scheme == "Centered(order=4)"
    assert isinstance(a.vorticity_scheme, ENS) and isinstance(a.vorticity_stencil, pkg.VelocityStencil)
    assert repr(VI()) == "VectorInvariant()" and isinstance(VI().vertical_scheme, EC)


def test_what_is_not_implemented_says_so(pkg):
    VI, WVI, WENO, UB = pkg.VectorInvariant, pkg.WENOVectorInvariant, pkg.WENO, pkg.UpwindBiased
    EC = pkg.EnergyConserving
    refused = [
        (lambda: WVI(), "pass `order=5` or `vorticity_order=5`"),
        (lambda: WVI(order=9), "order=5"),
        (lambda: WVI(order=5, vertical_order=3), "vertical_order = 3"),
        (lambda: WVI(vorticity_order=5, kinetic_energy_gradient_order=7), "kinetic_energy_gradient_order = 7"),
        (lambda: VI(vorticity_scheme=WENO(order=7)), "WENO\\(order=5\\)"),
        (lambda: VI(vorticity_scheme=UB()), "use WENO\\(order=5\\) or EnstrophyConserving\\(\\)"),
        (lambda: VI(vertical_scheme=UB()), "use WENO\\(order=5\\) or EnergyConserving\\(\\)"),
        (lambda: VI(vorticity_scheme=WENO(), kinetic_energy_gradient_scheme=UB()), "use WENO\\(order=5\\) or EnergyConserving\\(\\)"),
        (lambda: VI(vorticity_scheme=EC()), "use EnstrophyConserving\\(\\) or WENO\\(order=5\\)"),
        (lambda: VI(vertical_scheme=WENO(), divergence_scheme=EC()), "divergence_scheme must be of the kind of vertical_scheme"),
        (lambda: VI(kinetic_energy_gradient_scheme=WENO()), "needs vertical_scheme = WENO\\(\\)"),
        (lambda: WVI(order=5, upwinding=pkg.CrossAndSelfUpwinding(cross_scheme=WENO())), "use the default OnlySelfUpwinding"),
        (lambda: WVI(order=5, upwinding=pkg.OnlySelfUpwinding(cross_scheme=WENO(), δU_stencil=pkg.FunctionStencil(abs))), "custom FunctionStencil"),
        (lambda: WVI(order=5, upwinding=pkg.OnlySelfUpwinding(cross_scheme=WENO(), δu2_stencil=pkg.DefaultStencil())), "custom FunctionStencil"),
        (lambda: WVI(order=5, upwinding=pkg.OnlySelfUpwinding()), "cross_scheme other than the default"),
        (lambda: WVI(order=5, multi_dimensional_stencil=True), "dimension-by-dimension"),
        (lambda: VI(vorticity_scheme=WENO(), vorticity_stencil=pkg.FunctionStencil(abs)), "VelocityStencil\\(\\) or DefaultStencil\\(\\)"),
    ]
    for make, message in refused:
        with pytest.raises(NotImplementedError, match=message):
            make()


class _Stop(Exception):
    pass


def _grid(pkg, halo=(3, 3, 3), size=(8, 8, 6), topo=(P, P, B), arch=None):
    return pkg.RectilinearGrid(arch, size=size, x=(0, 1), y=(0, 1), z=(-1, 0), topology=topo, halo=halo)


def test_model_refusals_come_before_any_allocation(pkg, monkeypatch):
    import oceananigans_jl_amd.fields as fields

    def no_alloc(*a, **k):
        raise AssertionError("a field was allocated before the refusal")
    monkeypatch.setattr(fields.Field, "__init__", no_alloc)
    HFSM, WVI = pkg.HydrostaticFreeSurfaceModel, pkg.WENOVectorInvariant
    with pytest.raises(NotImplementedError, match="fused = True with an upwinding"):
        HFSM(_grid(pkg), momentum_advection=WVI(order=5), free_surface=pkg.ExplicitFreeSurface(), fused=True)
    with pytest.raises(NotImplementedError, match="fused = True with an upwinding"):
        HFSM(_grid(pkg), momentum_advection=pkg.VectorInvariant(vorticity_scheme=pkg.WENO()), free_surface=pkg.SplitExplicitFreeSurface(substeps=10), fused=True)
    arch = SimpleNamespace(partition=(1, 1, 1), communicates=False)  # what the model asks of a Distributed architecture
    g = _grid(pkg)
    monkeypatch.setattr(g, "architecture", arch, raising=False)
    with pytest.raises(NotImplementedError, match="on a Distributed grid"):
        HFSM(g, momentum_advection=WVI(order=5), free_surface=pkg.SplitExplicitFreeSurface(substeps=10))


@pytest.mark.parametrize("given,advection,want", [
    ((3, 3, 3), "weno", (4, 4, 3)), ((1, 1, 1), "weno", (4, 4, 3)), ((5, 6, 4), "weno", (5, 6, 4)), ((3, 5, 2), "weno", (4, 5, 3)),
    ((3, 3, 3), "vorticity", (4, 4, 3)), ((1, 1, 1), "vorticity", (4, 4, 1)), ((3, 3, 3), "default", (3, 3, 3)), ((1, 1, 1), "default", (1, 1, 1))])
def test_the_halo_a_model_ends_up_with(pkg, monkeypatch, given, advection, want):
    """required_halo_size_x/y = 3 + 1, required_halo_size_z = the vertical scheme's (vector_invariant_advection.jl:241-251), per direction,
    never less than given; VectorInvariant() keeps what it got.  The first field a model allocates is built on the inflated grid."""
    import oceananigans_jl_amd.fields as fields
    seen = []

    def first_field(self, loc, grid, *a, **k):
        seen.append((grid.Hx, grid.Hy, grid.Hz))
        raise _Stop()
    monkeypatch.setattr(fields.Field, "__init__", first_field)
    scheme = {"weno": lambda: pkg.WENOVectorInvariant(order=5), "vorticity": lambda: pkg.VectorInvariant(vorticity_scheme=pkg.WENO()),
              "default": lambda: pkg.VectorInvariant()}[advection]()
    with pytest.raises(_Stop):
        pkg.HydrostaticFreeSurfaceModel(_grid(pkg, halo=given), momentum_advection=scheme, free_surface=pkg.ExplicitFreeSurface())
    assert seen == [want]


# ---- 3. the entry point's argument checks -------------------------------------------------------------------------------------------
def test_entry_point_refuses_without_touching_a_device(pkg):
    L = pkg._lib
    fn = L.lib().ocn_compute_vector_invariant_weno_momentum_tendencies
    last = lambda: L.lib().ocn_last_error().decode() if isinstance(L.lib().ocn_last_error(), bytes) else str(L.lib().ocn_last_error())
    ok = _grid(pkg)
    p = C.c_void_p(8)  # never dereferenced: every call below is refused
    call = lambda grid, flags_, u=p, Gv=p: fn(grid.cref, flags_, u, p, p, p, Gv, None, 9.8, None)
    assert call(_grid(pkg, halo=(2, 3, 3)), 7) == INVALID and "halo is (2, 3, 3)" in last()
    assert call(_grid(pkg, halo=(3, 2, 3)), 7) == INVALID
    assert call(_grid(pkg, topo=(P, B, B)), 7) in (INVALID, UNSUPPORTED) and last()   # a Bounded y
    assert call(_grid(pkg, topo=(P, P, P)), 7) == INVALID and "(Periodic, Periodic, Bounded)" in last()
    assert call(ok, 0) == INVALID and "ocn_compute_vector_invariant_momentum_tendencies" in last()
    assert call(ok, 8) == INVALID                       # the stencil bit alone: still no WENO sub-scheme
    assert call(ok, 16) == INVALID and "unknown scheme flag bits" in last()
    assert call(ok, 4) == INVALID and "cross scheme" in last()   # kinetic-energy gradient without the divergence scheme
    assert call(ok, 5) == INVALID
    assert call(ok, 7, u=None) == INVALID and "null field pointer" in last()
    assert call(ok, 7, Gv=None) == INVALID
