"""forcing = {...} without a GPU: sampling on the nodes of the forced field's own location, the `steady` rule, `show`, refusals before anything
is allocated, and the argument checks of the C entry points that take struct ocn_forcing."""
import ctypes as C

import numpy as np
import pytest

P, B, F = "Periodic", "Bounded", "Flat"
INVALID = -1  # OCN_ERR_INVALID_ARGUMENT (include/ocn_hip.h)

# the two docstring outputs of relaxation.jl:44-47 and :66-69
SHOW_DAMPING = ("Relaxation{Float64, typeof(Oceananigans.Forcings.onefunction), typeof(Oceananigans.Forcings.zerofunction)}\n"
                "├── rate: 0.0002777777777777778\n"
                "├── mask: 1\n"
                "└── target: 0")
SHOW_SPONGE = ("Relaxation{Float64, GaussianMask{:z, Float64}, LinearTarget{:z, Float64}}\n"
               "├── rate: 0.016666666666666666\n"
               "├── mask: exp(-(z + 100.0)^2 / (2 * 25.0^2))\n"
               "└── target: 20.0 + 0.001 * z")


@pytest.fixture(scope="module")
def pkg():
    import oceananigans_jl_amd as ocn
    return ocn


def _stretched(N, L):
    k = np.arange(N + 1)
    return -L * (1 - k / N) ** 1.5


def _grid(pkg, topo=(P, P, B), z=(-8, 0), size=(4, 5, 6)):
    return pkg.RectilinearGrid(None, size=size, x=(0, 1), y=(0, 2), z=z, topology=topo, halo=(3, 3, 3))


def test_show_matches_the_reference_doctests(pkg):
    assert repr(pkg.Relaxation(rate=1 / 3600)) == SHOW_DAMPING
    sponge = pkg.Relaxation(rate=1 / 60, target=pkg.LinearTarget("z", intercept=20, gradient=0.001), mask=pkg.GaussianMask("z", center=-100, width=100 / 4))
    assert repr(sponge) == SHOW_SPONGE
    assert sponge.summary() == "Relaxation(rate=0.016666666666666666, mask=exp(-(z + 100.0)^2 / (2 * 25.0^2)), target=20.0 + 0.001 * z)"
    assert pkg.GaussianMask("x", center=0, width=1).summary() == "exp(-x^2 / (2 * 1.0^2))"
    assert pkg.GaussianMask("y", center=2, width=1).summary() == "exp(-(y - 2.0)^2 / (2 * 1.0^2))"


@pytest.mark.parametrize("name,loc", [("u", 1), ("v", 2), ("w", 4), ("T", 0)])
def test_masks_and_targets_are_sampled_on_the_fields_own_nodes(pkg, name, loc):
    """GaussianMask / LinearTarget on a stretched-z (Periodic, Periodic, Bounded) grid equal their closed forms on the nodes of the forced
    field's location -- x faces for u, z faces for w -- halos included"""
    from oceananigans_jl_amd.forcings import field_location, sample_term
    g = _grid(pkg, z=_stretched(6, 8.0))
    assert field_location(name) == loc
    for d, D in enumerate("xyz"):
        X = np.asarray(g.nodes_1d(d, bool(loc & (1 << d)), with_halos=True))[:g.parent_shape(loc)[d]]
        assert X.size == g.parent_shape(loc)[d]
        h = sample_term(pkg.Relaxation(0.5, mask=pkg.GaussianMask(D, center=-2.0, width=3.0), target=pkg.LinearTarget(D, intercept=1.5, gradient=-0.25)),
                        g, loc)
        assert (h["kind"], h["rate"], h["mask_dim"], h["target_dim"]) == (2, 0.5, d, d)
        assert np.array_equal(h["mask"], np.exp(-(X + 2.0) ** 2 / (2 * 3.0 ** 2)))
        assert np.array_equal(h["target"], 1.5 + -0.25 * X)
    # faces differ from centres where the location says so
    zf, zc = np.asarray(g.nodes_1d(2, True, with_halos=True)), np.asarray(g.nodes_1d(2, False, with_halos=True))
    assert zf.size == zc.size + 1 and not np.array_equal(zf[:-1], zc)


def test_forcing_function_is_evaluated_at_the_fields_own_location(pkg):
    from oceananigans_jl_amd.forcings import interior_shape, sample_term
    g = _grid(pkg, z=_stretched(6, 8.0))
    f = pkg.Forcing(lambda x, y, z, t, p: p["a"] * x + 10 * y + 100 * z + 1000 * t, parameters={"a": 2.0})
    for loc in (1, 2, 4, 0):
        x, y, z = g.nodes(loc)
        h = sample_term(f, g, loc, t=0.5)
        assert h["kind"] == 1 and h["values"].shape == interior_shape(g, loc)
        assert np.array_equal(h["values"], np.broadcast_to(2.0 * x + 10 * y + 100 * z + 500.0, h["values"].shape))
    assert interior_shape(g, 4) == (4, 5, 7) and interior_shape(g, 1) == (4, 5, 6)
    # a function that cannot take arrays is called node by node
    import math
    h = sample_term(pkg.Forcing(lambda x, y, z, t: math.exp(z) + t), g, 0, t=1.0)
    assert np.allclose(h["values"], np.broadcast_to(np.exp(g.nodes(0)[2]) + 1.0, h["values"].shape), rtol=0, atol=0)


def test_flat_directions_are_dropped_from_the_argument_list(pkg):
    from oceananigans_jl_amd.forcings import sample_term
    g = pkg.RectilinearGrid(None, size=(4, 6), x=(0, 1), z=(-8, 0), topology=(P, F, B), halo=(3, 3))
    seen = []

    def func(*args):
        seen.append(len(args))
        x, z, t = args
        return x + z + t
    h = sample_term(pkg.Forcing(func), g, 0, t=2.0)
    assert seen[0] == 3
    x, _, z = g.nodes(0)
    assert np.array_equal(h["values"], np.broadcast_to(x + z + 2.0, h["values"].shape))
    h = sample_term(pkg.Relaxation(1.0, mask=lambda x, z: x * z, target=lambda x, z, t: x - z + t), g, 0, t=3.0)
    assert np.array_equal(h["mask"], np.broadcast_to(x * z, h["mask"].shape)) and np.array_equal(h["target"], np.broadcast_to(x - z + 3.0, h["target"].shape))
    with pytest.raises(ValueError, match="Flat"):
        from oceananigans_jl_amd.forcings import validate_forcing
        validate_forcing({"u": pkg.Relaxation(1.0, mask=pkg.GaussianMask("y", center=0, width=1))}, g, ("u", "v", "w"))


def test_steady_rule(pkg):
    func = lambda x, y, z, t: t
    assert pkg.Relaxation(1.0).steady is True
    assert pkg.Relaxation(1.0, mask=pkg.GaussianMask("z", center=0, width=1), target=pkg.LinearTarget("z", intercept=0, gradient=1)).steady is True
    assert pkg.Relaxation(1.0, mask=lambda x, y, z: z).steady is True            # masks never receive t
    assert pkg.Relaxation(1.0, target=np.zeros((4, 5, 6))).steady is True
    assert pkg.Relaxation(1.0, target=func).steady is False                        # a function that receives t ...
    assert pkg.Relaxation(1.0, target=func, steady=True).steady is True            # ... unless declared steady
    assert pkg.Forcing(func).steady is False
    assert pkg.Forcing(func, steady=True).steady is True
    with pytest.raises(ValueError):
        pkg.Relaxation(1.0, steady=False)


def test_refusals_come_before_any_allocation(pkg, monkeypatch):
    import oceananigans_jl_amd.fields as fields

    def no_alloc(*a, **k):
        raise AssertionError("a field was allocated before the refusal")
    monkeypatch.setattr(fields.Field, "__init__", no_alloc)
    g = _grid(pkg)
    model = lambda forcing, grid=g, **kw: pkg.NonhydrostaticModel(grid, advection=pkg.WENO(), forcing=forcing, **kw)
    with pytest.raises(NotImplementedError, match=r"forcing.*ocn\.Forcing\(func\)"):   # a bare callable: told to wrap it
        model({"u": lambda x, y, z, t: 0.0})
    with pytest.raises(NotImplementedError, match="forcing"):                          # five terms
        model({"u": tuple(pkg.Relaxation(1.0) for _ in range(5))})
    with pytest.raises(ValueError, match="unknown field"):
        model({"T": pkg.Relaxation(1.0)})
    with pytest.raises(ValueError, match="shape"):                                     # w has Nz + 1 faces on a Bounded z
        model({"w": np.zeros((4, 5, 6))})
    with pytest.raises(ValueError, match="shape"):
        model({"T": pkg.Relaxation(1.0, mask=np.zeros((4, 5, 7)))}, tracers=("T",))
    with pytest.raises(NotImplementedError, match="forcing"):
        pkg.Forcing(lambda x, y, z, t, u: -u, field_dependencies=("u",))
    with pytest.raises(NotImplementedError, match="forcing"):
        pkg.Forcing(lambda i, j, k, grid, clock, fields: 0.0, discrete_form=True)
    with pytest.raises(NotImplementedError, match="forcing"):
        pkg.AdvectiveForcing(w=1.0)
    with pytest.raises(NotImplementedError, match="forcing"):
        model({"u": object()})
    with pytest.raises(NotImplementedError, match="forcing"):
        pkg.HydrostaticFreeSurfaceModel(g, forcing={"u": pkg.Relaxation(1.0)})

    class FakeDistributed:  # what models.py asks of a Distributed architecture: a `partition`
        partition = object()
    gd = _grid(pkg)
    gd.architecture = FakeDistributed()
    with pytest.raises(NotImplementedError, match="forcing.*Distributed"):
        model({"u": pkg.Relaxation(1.0)}, grid=gd)


def test_c_abi_argument_checks_touch_no_device(pkg):
    """OCN_ERR_INVALID_ARGUMENT before any HIP call: runs on a machine without a GPU"""
    lib, L = pkg._lib.lib(), pkg._lib
    g = _grid(pkg, size=(16, 16, 8))
    terms = L.CModelTerms()
    one = C.c_void_p(8)  # never dereferenced

    def forcing(**kw):
        f = L.CForcing()
        f.n_terms = kw.pop("n_terms", 1)
        f.term[0].kind, f.term[0].mask_dim, f.term[0].target_dim = 2, -1, -1
        for k, v in kw.items():
            setattr(f.term[0], k, v)
        return f

    def momentum(f, grid=g):
        return lib.ocn_compute_momentum_tendencies_terms_forced(grid.cref, C.byref(terms), None, L.forcing_array([C.pointer(f), None, None]),
                                                                one, one, one, one, one, one, None, None)

    def tracer(f, grid=g):
        return lib.ocn_compute_tracer_tendency_terms_forced(grid.cref, C.byref(terms), 0.0, None, C.byref(f), one, one, one, one, one, None, None)
    for call in (momentum, tracer):
        assert call(forcing(n_terms=5)) == INVALID and b"n_terms" in lib.ocn_last_error()
        assert call(forcing(n_terms=-1)) == INVALID
        assert call(forcing(kind=7)) == INVALID and b"unknown kind" in lib.ocn_last_error()
        assert call(forcing(kind=1)) == INVALID and b"values is NULL" in lib.ocn_last_error()
        assert call(forcing(mask_dim=2)) == INVALID and b"mask is NULL" in lib.ocn_last_error()
        assert call(forcing(target_dim=3)) == INVALID and b"target is NULL" in lib.ocn_last_error()
        assert call(forcing(target_dim=4, target=8)) == INVALID and b"outside -1..3" in lib.ocn_last_error()
        gf = pkg.RectilinearGrid(None, size=(16, 8), x=(0, 1), z=(-1, 0), topology=(P, F, B), halo=(3, 3))
        assert call(forcing(mask_dim=1, mask=8), gf) == INVALID and b"Flat" in lib.ocn_last_error()
    # a valid descriptor reaches the checks of the entry point without the suffix
    ok = forcing(mask_dim=2, mask=8)
    assert lib.ocn_compute_momentum_tendencies_terms_forced(g.cref, C.byref(terms), None, L.forcing_array([C.pointer(ok), None, None]), None, one, one,
                                                            one, one, one, None, None) == INVALID
    assert b"null field pointer" in lib.ocn_last_error()
    args = [one] * 12
    assert lib.ocn_compute_momentum_tendencies_terms_rk3_forced(g.cref, C.byref(terms), None, L.forcing_array([C.pointer(ok), None, None]), None, None,
                                                                *args, 1.0, 0.5, 0.0, 0, None, None) == INVALID
    assert b"alias" in lib.ocn_last_error()
    assert lib.ocn_compute_tracer_tendency_terms_rk3_forced(g.cref, C.byref(terms), 0.0, None, C.byref(ok), None, one, one, one, one, one, None, one,
                                                            1.0, 0.5, 0.0, 0, None, None) == INVALID
    assert b"alias" in lib.ocn_last_error()
    assert lib.ocn_compute_tracer_tendency_terms_rk3_forced(g.cref, C.byref(terms), 0.0, None, C.byref(forcing(kind=9)), None, *([one] * 7),
                                                            1.0, 0.5, 0.0, 0, None, None) == INVALID
    # the driver's setter
    assert lib.ocn_model_driver_set_forcing(None, None, 0) == INVALID
    assert b"null driver" in lib.ocn_last_error()
