"""Grids stretched in x or y (generate_coordinate's explicit-face branch, grid_generation.jl:34-95, for every Bounded direction) and the
argument checks of the Fourier-tridiagonal entry points along x / y, without a GPU."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_fixtures.json")))
P, B, F = "Periodic", "Bounded", "Flat"


@pytest.fixture(scope="module")
def pkg():
    import oceananigans_jl_amd as ocn
    return ocn


def _faces(case):
    N, L = case["N"], case["L"]
    if case["formula"] == "hyperbolic":
        s = case["sigma"]
        return [-L * (1 - math.tanh(s * (k - 1) / N) / math.tanh(s)) for k in range(1, N + 2)]
    if case["formula"] == "chebychev_centered":
        return [-L / 2 * math.cos(math.pi * (j - 1) / N) for j in range(1, N + 2)]
    if case["formula"] == "chebychev_y":
        return [L * (1 - math.cos(math.pi * (j - 1) / N)) / 2 for j in range(1, N + 2)]
    if case["formula"] == "chebychev_z":
        return [-L * (1 + math.cos(math.pi * (k - 1) / N)) / 2 for k in range(1, N + 2)]
    raise KeyError(case["formula"])


def _sig6(x):
    return float(f"{x:.6g}")


@pytest.mark.parametrize("case", FX["stretched_faces"], ids=[c["source"] for c in FX["stretched_faces"]])
def test_x_and_y_faces_give_the_metric_vectors_of_z(oracle, pkg, case):
    """The same faces along x, along y and along z: bitwise the same Δᶜ / Δᶠ vectors, faces and extrema, and those of the oracle's z"""
    faces = np.array(_faces(case))
    N = case["N"]
    gz = pkg.RectilinearGrid(None, size=(4, 5, N), x=(0, 1), y=(0, 1), z=faces, topology=(P, P, B))
    gx = pkg.RectilinearGrid(None, size=(N, 5, 4), x=faces, y=(0, 1), z=(0, 1), topology=(B, P, P))
    gy = pkg.RectilinearGrid(None, size=(4, N, 5), x=(0, 1), y=faces, z=(0, 1), topology=(P, B, P))
    og = oracle.Grid((4, 5, N), x=(0, 1), y=(0, 1), z=faces, topology="PPB")
    for c, f in ((gx._dxc_host, gx._dxf_host), (gy._dyc_host, gy._dyf_host)):
        assert c.tobytes() == gz._dzc_host.tobytes() == og.dzc.tobytes()
        assert f.tobytes() == gz._dzf_host.tobytes() == og.dzf.tobytes()
    assert np.array_equal(gx.x_faces, gz.z_faces) and np.array_equal(gy.y_faces, gz.z_faces)
    assert gx.Lx == gy.Ly == gz.Lz == og.Lz
    assert math.isnan(gx.dx) and math.isnan(gy.dy) and gx.c.dx == 0.0 and gy.c.dy == 0.0
    assert gx.stretched_dimensions == (0,) and gy.stretched_dimensions == (1,) and gz.stretched_dimensions == (2,)
    for g, d in ((gx, 0), (gy, 1)):
        assert g.spacing_extrema(d) == gz.spacing_extrema(2)
        assert g.spacing_extrema(d, face=True) == gz.spacing_extrema(2, face=True)
        assert g.domain(d) == gz.domain(2)
        for face in (False, True):
            for wh in (False, True):
                assert np.array_equal(g.nodes_1d(d, face, with_halos=wh), gz.nodes_1d(2, face, with_halos=wh))
    lo, hi = gx.spacing_extrema(0)
    assert _sig6(lo) == float(case["min"]) and _sig6(hi) == float(case["max"])
    # a function of the face index gives the same grid
    gf = pkg.RectilinearGrid(None, size=(N, 5, 4), x=lambda i: _faces(case)[i - 1], y=(0, 1), z=(0, 1), topology=(B, P, P))
    assert gf._dxc_host.tobytes() == gx._dxc_host.tobytes() and gf._dxf_host.tobytes() == gx._dxf_host.tobytes()


def test_grids_md_example_with_stretched_y_and_z(pkg):
    """docs/src/grids.md:343-367: (Periodic, Bounded, Bounded), Chebychev-spaced y AND z, given as functions"""
    Nx = Ny = 64
    Nz = 32
    Lx = Ly = 1e4
    Lz = 1e3
    grid = pkg.RectilinearGrid(None, size=(Nx, Ny, Nz), topology=(P, B, B), x=(0, Lx),
                               y=lambda j: Ly * (1 - math.cos(math.pi * (j - 1) / Ny)) / 2,
                               z=lambda k: -Lz * (1 + math.cos(math.pi * (k - 1) / Nz)) / 2)
    want = {c["formula"]: c for c in FX["stretched_faces"]}
    assert grid.stretched_dimensions == (1, 2)
    assert grid.dx == 156.25 and grid.domain(0) == (0.0, 10000.0)
    for d, name in ((1, "chebychev_y"), (2, "chebychev_z")):
        lo, hi = grid.spacing_extrema(d)
        assert (_sig6(lo), _sig6(hi)) == (float(want[name]["min"]), float(want[name]["max"]))
        assert tuple(_sig6(v) for v in grid.domain(d)) == tuple(float(v) for v in want[name]["domain"])
    assert str(grid.domain(1)) == "(0.0, 10000.0)"
    assert grid._dyc_host.size == Ny + 2 * grid.Hy and grid._dzc_host.size == Nz + 2 * grid.Hz


def test_stretched_periodic_x_or_y_still_refused(pkg):
    faces = [0, 1, 2, 3, 4, 5, 6, 7, 9]
    with pytest.raises(NotImplementedError):
        pkg.RectilinearGrid(None, size=(8, 8, 2), x=faces, y=(0, 1), z=(0, 1), topology=(P, P, P))
    with pytest.raises(NotImplementedError):
        pkg.RectilinearGrid(None, size=(8, 8, 2), x=(0, 1), y=faces, z=(0, 1), topology=(P, P, B))
    with pytest.raises(ValueError, match="increasing"):
        pkg.RectilinearGrid(None, size=(2, 8, 2), x=[0, 2, 1], y=(0, 1), z=(0, 1), topology=(B, P, B))
    with pytest.raises(ValueError, match="face positions"):
        pkg.RectilinearGrid(None, size=(3, 8, 2), x=[0, 1, 2], y=(0, 1), z=(0, 1), topology=(B, P, B))


def test_solver_choice_and_model_refusals_need_no_gpu(pkg):
    """Two stretched directions: no Fourier-tridiagonal method (NotImplementedError); the time steppers refuse x / y stretching"""
    g2 = pkg.RectilinearGrid(None, size=(8, 8, 4), x=(0, 1), y=np.linspace(0, 1, 9) ** 2, z=np.linspace(-1, 0, 5) ** 3, topology=(P, B, B))
    with pytest.raises(NotImplementedError):
        pkg.stretched_direction(g2)
    gx = pkg.RectilinearGrid(None, size=(8, 8, 4), x=np.linspace(0, 1, 9) ** 2, y=(0, 1), z=(0, 1), topology=(B, P, B))
    assert isinstance(pkg.stretched_direction(gx), pkg.XDirection)
    for ctor in (pkg.NonhydrostaticModel, pkg.HydrostaticFreeSurfaceModel):
        with pytest.raises(NotImplementedError, match="stretched in x"):
            ctor(gx)


def _grid(pkg, **kw):
    d = dict(Nx=8, Ny=8, Nz=8, Hx=1, Hy=1, Hz=1, tx=1, ty=0, tz=1, math=0, dx=0.0, dy=0.125, dz=0.125, Lx=1.0, Ly=1.0, Lz=1.0,
             dzc=None, dzf=None)
    d.update(kw)
    return pkg._lib.CGrid(*d.values())


def test_stretched_entry_points_validate_before_any_hip_call(pkg):
    lib = pkg._lib.lib()
    fake = np.zeros(64)
    p = fake.ctypes.data
    h = C.c_void_p()

    def err(name, *args):
        st = getattr(lib, name)(*args)
        assert st != 0
        return lib.ocn_last_error().decode()

    assert "dim" in err("ocn_poisson_create_stretched", C.byref(h), C.byref(_grid(pkg)), 2, p, p)
    assert "dim" in err("ocn_poisson_create_stretched", C.byref(h), C.byref(_grid(pkg)), -1, p, p)
    assert "Bounded" in err("ocn_poisson_create_stretched", C.byref(h), C.byref(_grid(pkg, tx=0)), 0, p, p)
    assert "Bounded" in err("ocn_poisson_create_stretched", C.byref(h), C.byref(_grid(pkg)), 1, p, p)  # y Periodic
    assert "N >= 2" in err("ocn_poisson_create_stretched", C.byref(h), C.byref(_grid(pkg, Nx=1, Hx=1)), 0, p, p)
    assert "null" in err("ocn_poisson_create_stretched", C.byref(h), C.byref(_grid(pkg)), 0, None, p)
    assert "null" in err("ocn_poisson_create_stretched", C.byref(h), C.byref(_grid(pkg)), 0, p, None)
    assert "null" in err("ocn_poisson_create_stretched", None, C.byref(_grid(pkg)), 0, p, p)
    assert "null" in err("ocn_poisson_create_stretched", C.byref(h), None, 0, p, p)
    assert "regular" in err("ocn_poisson_create_stretched", C.byref(h), C.byref(_grid(pkg, dzc=p, dzf=p)), 0, p, p)
    assert h.value is None
    for n in "xy":
        name = f"ocn_batched_tridiagonal_solve_{n}"
        assert "bad sizes" in err(name, 0, 4, 4, p, p, p, p, p, p, None)
        assert "null" in err(name, 4, 4, 4, p, None, p, p, p, p, None)
        assert "null" in err(name, 4, 4, 4, p, p, p, p, p, None, None)


def test_header_documents_the_new_kinds():
    h = open(os.path.join(ROOT, "include", "ocn_hip.h")).read()
    assert "ocn_poisson_create_stretched" in h and "4 / 5 = Fourier-tridiagonal along a stretched x / y" in h
