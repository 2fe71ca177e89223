"""UniformStokesDrift without a GPU: construction, `show`, sampling on the grid's z nodes, refusals before anything is allocated, and the
argument checks of the C entry points that take struct ocn_stokes_drift."""
import ctypes as C
import json
import os
from collections import namedtuple

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHOW = json.load(open(os.path.join(ROOT, "tests", "golden", "stokes_drift_show.json"), encoding="utf-8"))
P, B, F = "Periodic", "Bounded", "Flat"
INVALID = -1  # OCN_ERR_INVALID_ARGUMENT (include/ocn_hip.h)


@pytest.fixture(scope="module")
def pkg():
    import oceananigans_jl_amd as ocn
    return ocn


def uniform_stokes_shear(z, t):
    return 0.005 * np.exp(z / 20)


def _grid(pkg, topo=(P, P, B), z=(-8, 0), size=(4, 5, 6), arch=None):
    return pkg.RectilinearGrid(arch, size=size, x=(0, 1), y=(0, 1), z=z, topology=topo, halo=(3, 3, 3))


def test_three_forms_of_construction(pkg):
    a = pkg.UniformStokesDrift(dz_us=uniform_stokes_shear)
    assert a.dz_us is uniform_stokes_shear and a.dz_vs is None and a.dt_us is None and a.dt_vs is None and a.parameters is None
    b = pkg.UniformStokesDrift(dz_us=lambda z, t, p: p["U"] * np.exp(z / p["h"]), dt_vs=lambda z, t, p: p["U"] * t, parameters={"U": 0.005, "h": 20})
    assert b.parameters == {"U": 0.005, "h": 20} and callable(b.dt_vs)
    g = _grid(pkg)
    c = pkg.UniformStokesDrift(g, dz_us=np.arange(7.0), dt_us=np.ones(6))
    assert c.grid is g and c.dz_us.shape == (7,) and c.dt_us.shape == (6,)
    with pytest.raises(ValueError):
        pkg.UniformStokesDrift(g, dz_us=np.arange(6.0))  # faces of a Bounded z: Nz + 1 values
    with pytest.raises(TypeError):
        pkg.UniformStokesDrift(dz_us=np.arange(7.0))     # arrays need the grid form
    with pytest.raises(TypeError):
        pkg.UniformStokesDrift(g, dz_us=uniform_stokes_shear)


def test_show_matches_the_reference_doctests(pkg):
    assert repr(pkg.UniformStokesDrift(dz_us=uniform_stokes_shear)) == SHOW["uniform_stokes_shear_no_parameters"]

    def shear(z, t, p):
        return p.uˢ * np.exp(z / p.h)
    shear.__name__ = "uniform_stokes_shear"
    params = namedtuple("P", ("uˢ", "h"))(0.005, 20)
    assert repr(pkg.UniformStokesDrift(dz_us=shear, parameters=params)) == SHOW["uniform_stokes_shear_with_parameters"]
    assert repr(pkg.UniformStokesDrift(dz_us=shear, parameters={"uˢ": 0.005, "h": 20})) == SHOW["uniform_stokes_shear_with_parameters"]


@pytest.mark.parametrize("topo,z", [((P, P, B), (-8, 0)), ((P, P, P), (-8, 0)), ((P, P, B), "stretched")])
def test_functions_are_sampled_on_centres_and_faces_bitwise(pkg, topo, z):
    Nz, h = 6, 20.0
    if z == "stretched":
        z = -8.0 * (1 - np.linspace(0, 1, Nz + 1)) ** 1.6
    g = _grid(pkg, topo, z)
    from oceananigans_jl_amd.stokes import z_nodes
    zc, zf = z_nodes(g)
    assert zc.shape == (Nz,) and zf.shape == (Nz + 1,)
    assert np.array_equal(zc, g.nodes_1d(2, False)) and np.array_equal(zf[:Nz], g.nodes_1d(2, True)[:Nz])
    s = pkg.UniformStokesDrift(dz_us=lambda z, t: np.exp(z / h), dt_vs=lambda z, t, : np.exp(z / h) * (1 + t)).sample(g, 2.0)
    assert s["dz_us_center"].tobytes() == np.exp(zc / h).tobytes()
    assert s["dz_us_face"].tobytes() == np.exp(zf / h).tobytes()
    assert s["dt_vs"].tobytes() == (np.exp(zc / h) * 3.0).tobytes()
    assert s["dz_vs_center"] is None and s["dz_vs_face"] is None and s["dt_us"] is None
    # with parameters; a function that cannot take a vector is called node by node
    import math
    q = pkg.UniformStokesDrift(dz_vs=lambda z, t, p: p["a"] * math.exp(z / p["h"]), parameters={"a": 0.5, "h": h}).sample(g, 0.0)
    assert q["dz_vs_face"].tobytes() == np.array([0.5 * math.exp(x / h) for x in zf]).tobytes()


def test_array_form_interpolates_to_centres(pkg):
    g = _grid(pkg)
    face = np.array([0.0, 1.0, 4.0, 9.0, 16.0, 25.0, 36.0])
    s = pkg.UniformStokesDrift(g, dz_us=face, dt_us=np.arange(6.0)).sample(g)
    assert np.array_equal(s["dz_us_face"], face)
    assert s["dz_us_center"].tobytes() == (0.5 * (face[:-1] + face[1:])).tobytes()   # ℑzᵃᵃᶜ
    assert np.array_equal(s["dt_us"], np.arange(6.0))
    gp = _grid(pkg, (P, P, P))
    sp = pkg.UniformStokesDrift(gp, dz_vs=face[:6]).sample(gp)  # Periodic z: face Nz + 1 is face 1
    assert sp["dz_vs_face"][-1] == face[0] and sp["dz_vs_center"][-1] == 0.5 * (face[5] + face[0])


def test_steady_rule(pkg):
    g = _grid(pkg)
    assert pkg.UniformStokesDrift(g, dz_us=np.zeros(7)).steady is True          # arrays: nothing to re-evaluate
    assert pkg.UniformStokesDrift(dz_us=1e-3).steady is True                     # numbers
    assert pkg.UniformStokesDrift(dz_us=uniform_stokes_shear).steady is False    # functions: resampled at every tendency evaluation ...
    assert pkg.UniformStokesDrift(dz_us=uniform_stokes_shear, steady=True).steady is True  # ... unless declared steady
    with pytest.raises(ValueError):
        pkg.UniformStokesDrift(g, dz_us=np.zeros(7), steady=False)


def test_refusals_come_before_any_allocation(pkg, monkeypatch):
    import oceananigans_jl_amd.fields as fields

    def no_alloc(*a, **k):
        raise AssertionError("a field was allocated before the refusal")
    monkeypatch.setattr(fields.Field, "__init__", no_alloc)
    with pytest.raises(NotImplementedError):
        pkg.StokesDrift(dz_us=uniform_stokes_shear)
    g = _grid(pkg)
    sd = pkg.UniformStokesDrift(dz_us=uniform_stokes_shear)
    with pytest.raises(NotImplementedError, match="stokes_drift"):
        pkg.NonhydrostaticModel(g, advection=pkg.WENO(), stokes_drift=object())
    with pytest.raises(NotImplementedError, match="stokes_drift"):
        pkg.HydrostaticFreeSurfaceModel(g, stokes_drift=sd)
    with pytest.raises(NotImplementedError, match="forcing"):
        pkg.NonhydrostaticModel(g, advection=pkg.WENO(), forcing={"u": lambda *a: 0.0})
    with pytest.raises(NotImplementedError, match="Flat"):
        pkg.NonhydrostaticModel(pkg.RectilinearGrid(None, size=(8, 8), x=(0, 1), y=(0, 1), topology=(P, P, F), halo=(3, 3)),
                                advection=pkg.WENO(), stokes_drift=sd)

    class FakeDistributed:  # what models.py asks of a Distributed architecture: a `partition`
        partition = object()
    gd = _grid(pkg)
    gd.architecture = FakeDistributed()
    with pytest.raises(NotImplementedError, match="Distributed"):
        pkg.NonhydrostaticModel(gd, advection=pkg.WENO(), stokes_drift=sd)


def test_c_abi_argument_checks_touch_no_device(pkg):
    """OCN_ERR_INVALID_ARGUMENT before any HIP call: runs on a machine without a GPU"""
    lib, L = pkg._lib.lib(), pkg._lib
    g = _grid(pkg, size=(16, 16, 8))
    terms, sd = L.CModelTerms(), L.CStokesDrift()
    one = C.c_void_p(8)  # never dereferenced
    # null field pointers
    assert lib.ocn_compute_momentum_tendencies_terms_stokes(g.cref, C.byref(terms), C.byref(sd), None, one, one, one, one, one, None, None) == INVALID
    assert b"null field pointer" in lib.ocn_last_error()
    # unknown advection scheme in terms
    bad = L.CModelTerms()
    bad.advection = 7
    assert lib.ocn_compute_momentum_tendencies_terms_stokes(g.cref, C.byref(bad), C.byref(sd), one, one, one, one, one, one, None, None) == INVALID
    # terms NULL
    assert lib.ocn_compute_momentum_tendencies_terms_stokes(g.cref, None, C.byref(sd), one, one, one, one, one, one, None, None) == INVALID
    # a Flat z has no vertical shear
    gf = pkg.RectilinearGrid(None, size=(16, 16), x=(0, 1), y=(0, 1), topology=(P, P, F), halo=(3, 3))
    assert lib.ocn_compute_momentum_tendencies_terms_stokes(gf.cref, C.byref(terms), C.byref(sd), one, one, one, one, one, one, None, None) == INVALID
    assert b"non-Flat z" in lib.ocn_last_error()
    # the fused form: outputs must not alias, G^- needed with zeta, range outside the interior
    args = [one] * 12
    f = lib.ocn_compute_momentum_tendencies_terms_rk3_stokes
    assert f(g.cref, C.byref(terms), C.byref(sd), None, None, *([one] * 9), None, one, one, 1.0, 0.5, 0.0, 0, None, None) == INVALID
    assert b"null field pointer" in lib.ocn_last_error()
    assert f(g.cref, C.byref(terms), C.byref(sd), None, None, *args, 1.0, 0.5, 0.0, 0, None, None) == INVALID
    assert b"alias" in lib.ocn_last_error()
    assert f(gf.cref, C.byref(terms), C.byref(sd), None, None, *args, 1.0, 0.5, 0.0, 0, None, None) == INVALID
    # the driver's setter
    assert lib.ocn_model_driver_set_stokes_drift(None, C.byref(sd), 0) == INVALID
    assert b"null driver" in lib.ocn_last_error()
