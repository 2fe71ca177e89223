"""LagrangianParticles without a GPU: the constructor and its refusals, the NumPy restatement (tests/particles_numpy.py) pinned to what the
reference's own test asserts (test/test_lagrangian_particle_tracking.jl:79-98, 178-185), and the argument checks of the C entry points
(no device is touched)."""
import ctypes as C

import numpy as np
import pytest

import particles_numpy as PN

P, B, F = "Periodic", "Bounded", "Flat"
STRETCHED = [-1, -0.5, 0.0, 0.4, 0.7, 1]
RTOL = np.sqrt(np.finfo(np.float64).eps)  # the reference's `≈`


@pytest.fixture(scope="module")
def pkg():
    import oceananigans_jl_amd as ocn
    return ocn


def _grid(pkg, z=(-1, 1), topo=(P, P, B)):
    kw = dict(x=(-1, 1), y=(-1, 1), z=z)
    size = tuple(5 for t in topo if t != F)
    for n, t in zip("xyz", topo):
        if t == F:
            kw[n] = None
    return pkg.RectilinearGrid(None, size=size, topology=topo, **kw)


def test_constructor_mirrors_the_reference(pkg):
    p = pkg.LagrangianParticles(x=np.zeros(10), y=np.zeros(10), z=0.5 * np.ones(10))
    assert len(p) == 10 and p.size == (10,) and list(p.properties) == ["x", "y", "z"]
    assert p.restitution == 1.0 and p.dynamics is None and p.parameters is None and p.tracked_fields == {}
    assert repr(p) == ("10 LagrangianParticles with eltype Particle:\n"
                       "├── 3 properties: (:x, :y, :z)\n"
                       "├── particle-wall restitution coefficient: 1.0\n"
                       "├── 0 tracked fields: ()\n"
                       "└── dynamics: no_dynamics")
    assert p.summary() == "10 LagrangianParticles with eltype Particle and properties (:x, :y, :z)"
    q = pkg.LagrangianParticles(x=np.zeros(3), y=np.zeros(3), z=np.zeros(3), restitution=0.5, tracked_fields={"u": "u", "s": "T"},
                                properties={"u": np.zeros(3), "s": np.zeros(3)}, parameters={"a": 1})
    assert list(q.properties) == ["x", "y", "z", "u", "s"] and q.restitution == 0.5 and q.parameters == {"a": 1}
    assert "├── 2 tracked fields: (:u, :s)" in repr(q) and "├── 5 properties: (:x, :y, :z, :u, :s)" in repr(q)
    assert np.array_equal(q.u.numpy(), np.zeros(3))
    empty = pkg.LagrangianParticles(x=np.zeros(0), y=np.zeros(0), z=np.zeros(0))
    assert len(empty) == 0


def test_constructor_errors(pkg):
    with pytest.raises(ValueError, match="x, y, z must all have the same size!"):
        pkg.LagrangianParticles(x=np.zeros(3), y=np.zeros(4), z=np.zeros(3))
    with pytest.raises(ValueError, match=r"x, y, z must have dimension 1 but ndims=\(2, 2, 2\)"):
        pkg.LagrangianParticles(x=np.zeros((2, 2)), y=np.zeros((2, 2)), z=np.zeros((2, 2)))
    with pytest.raises(ValueError, match="s is a tracked field but Particle has no s field"):
        pkg.LagrangianParticles(x=np.zeros(3), y=np.zeros(3), z=np.zeros(3), tracked_fields={"s": "u"})
    with pytest.raises(ValueError, match="property T must be a 1-D array of length 3"):
        pkg.LagrangianParticles(x=np.zeros(3), y=np.zeros(3), z=np.zeros(3), properties={"T": np.zeros(4)})
    with pytest.raises(TypeError, match="tracked field T"):
        pkg.LagrangianParticles(x=np.zeros(3), y=np.zeros(3), z=np.zeros(3), tracked_fields={"T": 3.0}, properties={"T": np.zeros(3)})


def test_model_refusals_come_before_any_allocation(pkg, monkeypatch):
    import oceananigans_jl_amd.fields as fields

    def no_alloc(*a, **k):
        raise AssertionError("a field was allocated before the refusal")
    monkeypatch.setattr(fields.Field, "__init__", no_alloc)
    g = _grid(pkg)
    with pytest.raises(TypeError, match="particles must be LagrangianParticles"):
        pkg.NonhydrostaticModel(g, advection=pkg.WENO(), particles={"x": np.zeros(3)})

    class FakeDistributed:  # what models.py asks of a Distributed architecture: a `partition`
        partition = object()
    gd = _grid(pkg)
    gd.architecture = FakeDistributed()
    p = pkg.LagrangianParticles(x=np.zeros(3), y=np.zeros(3), z=np.zeros(3))
    with pytest.raises(NotImplementedError, match="particles on a Distributed architecture"):
        pkg.NonhydrostaticModel(gd, advection=pkg.WENO(), particles=p)


def _zeros(geom, loc):
    return np.zeros(tuple(geom.parent_extent(a, (loc >> a) & 1) for a in range(3)))


@pytest.mark.parametrize("z", [(-1, 1), STRETCHED], ids=["regular", "stretched"])
def test_restatement_reproduces_the_reference_restitution_case(pkg, z):
    """test_lagrangian_particle_tracking.jl:79-98: from the centre of cell Nz - 1 a particle overshoots the top by 0.15 and bounces back"""
    g = _grid(pkg, z)
    geom = PN.Geometry(g)
    Nz, Hz = g.Nz, g.Hz
    z0 = float(g.nodes_1d(2, False)[Nz - 2])
    top = float(g.nodes_1d(2, True)[Nz])
    assert top == 1.0
    dt = 0.01
    u, v, w = _zeros(geom, 1), _zeros(geom, 2), _zeros(geom, 4)
    w[:, :, Nz - 1 + Hz] = (0.1 + top - z0) / dt
    w[:, :, Nz - 2 + Hz] = (0.2 + top - z0) / dt
    x, y, zp = PN.advect(geom, np.array([0.0]), np.array([0.0]), np.array([z0]), u, v, w, dt)
    np.testing.assert_allclose(zp, top - 0.15, rtol=RTOL, atol=0)
    assert x[0] == 0.0 and y[0] == 0.0


@pytest.mark.parametrize("topo", [(P, P, B), (P, F, B)], ids=["PPB", "PFB"])
@pytest.mark.parametrize("z", [(-1, 1), STRETCHED], ids=["regular", "stretched"])
def test_restatement_reproduces_the_reference_uniform_flow(pkg, topo, z):
    """:178-185: u = v = 1 carries (0, 0, 0.5) to (0.01, 0.01, 0.5) in a step of 0.01; the tracked velocities read 1, 1, 0"""
    g = _grid(pkg, z, topo)
    geom = PN.Geometry(g)
    u, v, w = _zeros(geom, 1) + 1.0, _zeros(geom, 2) + 1.0, _zeros(geom, 4)
    pos = (np.zeros(10), np.zeros(10), 0.5 * np.ones(10))
    x, y, zp = PN.advect(geom, *pos, u, v, w, 0.01)
    np.testing.assert_allclose(x, 0.01, rtol=RTOL, atol=0)
    np.testing.assert_allclose(y, 0.01, rtol=RTOL, atol=0)
    np.testing.assert_allclose(zp, 0.5, rtol=RTOL, atol=0)
    np.testing.assert_allclose(PN.interpolate(geom, u, 1, *pos), 1.0, rtol=RTOL, atol=0)
    np.testing.assert_allclose(PN.interpolate(geom, v, 2, *pos), 1.0, rtol=RTOL, atol=0)
    assert np.all(PN.interpolate(geom, w, 4, *pos) == 0.0)


def test_restatement_fractional_index_follows_the_reference(pkg):
    """fractional_index on the stretched faces: exact nodes, the interior and the reference's linear extrapolation past both ends"""
    vec = np.array(STRETCHED, dtype=np.float64)
    val = np.array([-1.0, 0.0, 1.0, -0.75, 0.55, -1.25, 1.15])
    f = PN.fractional_index(val, vec, len(vec))
    np.testing.assert_allclose(f, [1.0, 3.0, 6.0, 1.5, 4.5, 0.5, 6.5], rtol=4e-16, atol=0)


def test_restatement_clamps_what_the_reference_would_read_out_of_bounds(pkg):
    g = _grid(pkg)
    geom = PN.Geometry(g)
    rng = np.random.default_rng(0)
    u = rng.uniform(-1, 1, _zeros(geom, 1).shape)
    bad = np.array([np.nan, 1e300, -1e300, np.inf, -np.inf, 0.3])
    ok = np.zeros_like(bad)
    for pos in ((bad, ok, ok), (ok, bad, ok), (ok, ok, bad)):
        s = PN.interpolate(geom, u, 1, *pos)  # (an index outside the parent array would raise IndexError)
        assert s.shape == bad.shape
    # ... and a position whose indices the reference reads in bounds is untouched: the whole parent range but its last cell
    i, up, xi = PN.interpolator(geom, 0, False, np.array([geom.center0[0] + geom.d[0] * (-2.5 - 1), geom.center0[0] + geom.d[0] * (6.75 - 1)]))
    assert list(i) == [-2, 6] and up == 1
    np.testing.assert_allclose(xi, [0.5, 0.75], rtol=1e-12)


def _cgrid(pkg, **kw):
    base = dict(Nx=8, Ny=8, Nz=8, Hx=3, Hy=3, Hz=3, tx=0, ty=0, tz=1, math=0, dx=1.0, dy=1.0, dz=1.0, Lx=8.0, Ly=8.0, Lz=8.0)
    base.update(kw)
    return pkg._lib.CGrid(**base)


def test_argument_validation_needs_no_gpu(pkg):
    call, pa, ia = pkg._lib.call, pkg._lib.ptr_array, pkg._lib.i32_array
    lib = pkg._lib.lib()
    geom = pkg._lib.CParticleGeometry()
    g = C.byref(_cgrid(pkg))
    gm = C.byref(geom)
    fake = 0x1000
    # n == 0: success without a launch, whatever the pointers
    assert lib.ocn_advect_particles(g, gm, 0, None, None, None, 1.0, None, None, None, 0.1, 0, None, None, None, None) == 0
    assert lib.ocn_sample_particle_properties(g, gm, 0, None, None, None, 0, None, None, None, None) == 0
    with pytest.raises(pkg.OcnError, match="negative particle count"):
        call("ocn_advect_particles", g, gm, -1, fake, fake, fake, 1.0, fake, fake, fake, 0.1, 0, None, None, None, None)
    with pytest.raises(pkg.OcnError, match="null position pointer"):
        call("ocn_advect_particles", g, gm, 4, fake, None, fake, 1.0, fake, fake, fake, 0.1, 0, None, None, None, None)
    with pytest.raises(pkg.OcnError, match="null velocity pointer"):
        call("ocn_advect_particles", g, gm, 4, fake, fake, fake, 1.0, fake, fake, None, 0.1, 0, None, None, None, None)
    with pytest.raises(pkg.OcnError, match="n_tracked = 9 outside 0..8"):
        call("ocn_advect_particles", g, gm, 4, fake, fake, fake, 1.0, fake, fake, fake, 0.1, 9, None, None, None, None)
    with pytest.raises(pkg.OcnError, match="n_tracked = -1 outside"):
        call("ocn_sample_particle_properties", g, gm, 4, fake, fake, fake, -1, None, None, None, None)
    with pytest.raises(pkg.OcnError, match="null tracked-field arrays"):
        call("ocn_advect_particles", g, gm, 4, fake, fake, fake, 1.0, fake, fake, fake, 0.1, 1, None, None, None, None)
    with pytest.raises(pkg.OcnError, match="null tracked field / output pointer 1"):
        call("ocn_sample_particle_properties", g, gm, 4, fake, fake, fake, 2, pa([fake, fake]), ia([0, 1]), pa([fake, None]), None)
    with pytest.raises(pkg.OcnError, match="location mask 8"):
        call("ocn_sample_particle_properties", g, gm, 4, fake, fake, fake, 1, pa([fake]), ia([8]), pa([fake]), None)
    with pytest.raises(pkg.OcnError, match="null position pointer"):
        call("ocn_sample_particle_properties", g, gm, 4, None, fake, fake, 1, pa([fake]), ia([0]), pa([fake]), None)
    with pytest.raises(pkg.OcnError, match="geometry is NULL"):
        call("ocn_advect_particles", g, None, 4, fake, fake, fake, 1.0, fake, fake, fake, 0.1, 0, None, None, None, None)
    with pytest.raises(pkg.OcnError, match="stretched z needs the node vectors"):
        call("ocn_advect_particles", C.byref(_cgrid(pkg, dzc=fake, dzf=fake)), gm, 4, fake, fake, fake, 1.0, fake, fake, fake, 0.1, 0, None,
             None, None, None)
    # a partitioned x: unsupported (-2), for every partitioned topology code
    for tx in (3, 4, 5):
        assert lib.ocn_advect_particles(C.byref(_cgrid(pkg, tx=tx, ty=1)), gm, 4, fake, fake, fake, 1.0, fake, fake, fake, 0.1, 0, None, None,
                                        None, None) == -2
        assert b"partitioned x" in lib.ocn_last_error()
        assert lib.ocn_sample_particle_properties(C.byref(_cgrid(pkg, tx=tx, ty=1)), gm, 4, fake, fake, fake, 1, pa([fake]), ia([0]),
                                                  pa([fake]), None) == -2
    assert lib.ocn_advect_particles(g, gm, -1, fake, fake, fake, 1.0, fake, fake, fake, 0.1, 0, None, None, None, None) == -1
    assert C.sizeof(pkg._lib.CParticleGeometry) == 9 * 8 + 2 * 8
