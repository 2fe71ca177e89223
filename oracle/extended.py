"""oracle/extended.py -- TEST INFRASTRUCTURE ONLY.  NOT PART OF THE PRODUCT.

Loader of oracle/libocn_oracle_ld.so: oracle/ocn_oracle.c compiled with -DOCN_REAL='long double'.  It evaluates the same real
function of the same Float64 inputs, metrics and constants as libocn_oracle.so, with 64-bit-mantissa intermediates and outputs
(x87 extended precision, eps = 2^-63), so that

    |G_64 - G_ext|    is the rounding error of the Float64 restatement itself, and
    |G_fast - G_ext|  the rounding error of a fast-math kernel,

cell by cell, to within 2^-11 of a Float64 ulp.  Every wrapper takes an oracle.Grid (and oracle.Physics), widens Float64 parent
arrays to np.longdouble on the way in (exact) and returns new np.longdouble parent arrays; no input is modified.
"""
import ctypes as C
import os

import numpy as np

from . import oracle as O

LD = np.longdouble
# an 80-bit (or wider) long double is what makes this build a reference; a platform whose long double is a double must fail loudly
assert np.finfo(LD).nmant >= 63, "np.longdouble has no more mantissa bits than Float64 on this platform"
assert C.sizeof(C.c_longdouble) == LD().itemsize

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class _CGrid(C.Structure):
    _fields_ = [("Nx", C.c_int32), ("Ny", C.c_int32), ("Nz", C.c_int32),
                ("Hx", C.c_int32), ("Hy", C.c_int32), ("Hz", C.c_int32),
                ("tx", C.c_int32), ("ty", C.c_int32), ("tz", C.c_int32),
                ("dx", C.c_longdouble), ("dy", C.c_longdouble), ("dz", C.c_longdouble),
                ("dzc", C.c_void_p), ("dzf", C.c_void_p)]


class _CPhysics(C.Structure):
    _fields_ = [("coriolis", C.c_int32), ("closure", C.c_int32), ("buoyancy", C.c_int32), ("_pad", C.c_int32),
                ("f", C.c_longdouble), ("nu", C.c_longdouble), ("g", C.c_longdouble), ("alpha", C.c_longdouble),
                ("beta", C.c_longdouble), ("coriolis_beta", C.c_longdouble), ("yc", C.c_void_p), ("yf", C.c_void_p)]


def lib():
    global _LIB
    if _LIB is None:
        path = os.path.join(_HERE, "libocn_oracle_ld.so")
        if not os.path.exists(path):
            O.build()
        _LIB = C.CDLL(path)  # (only entry points that return through arrays are used: ctypes narrows a long double return value)
    return _LIB


def widen(a):
    """Float64 (or already extended) array -> a new column-major np.longdouble array; None stays None.  Exact."""
    return None if a is None else np.array(a, dtype=LD, order="F")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class _Grid:
    """the long double ocn_grid of an oracle.Grid (keeps the widened metric arrays alive)"""

    def __init__(self, g):
        self.dzc = None if g.dzc is None else np.ascontiguousarray(g.dzc, dtype=LD)
        self.dzf = None if g.dzf is None else np.ascontiguousarray(g.dzf, dtype=LD)
        self.c = _CGrid(g.Nx, g.Ny, g.Nz, g.Hx, g.Hy, g.Hz, g.tx, g.ty, g.tz, g.dx, g.dy, g.dz,
                        None if self.dzc is None else self.dzc.ctypes.data, None if self.dzf is None else self.dzf.ctypes.data)

    @property
    def ref(self):
        return C.byref(self.c)


class _Physics:
    def __init__(self, ph):
        c = ph.c
        self.yc = None if not c.yc else np.ascontiguousarray(ph._yc, dtype=LD)
        self.yf = None if not c.yf else np.ascontiguousarray(ph._yf, dtype=LD)
        self.c = _CPhysics(c.coriolis, c.closure, c.buoyancy, 0, c.f, c.nu, c.g, c.alpha, c.beta, c.coriolis_beta,
                           None if self.yc is None else self.yc.ctypes.data, None if self.yf is None else self.yf.ctypes.data)

    @property
    def ref(self):
        return C.byref(self.c)


def zeros(g, loc):
    return np.zeros(g.shape(loc), dtype=LD, order="F")


def fill_halo_regions(g, a, loc, fill_boundary_normal_velocities=True):
    """oracle.fill_halo_regions with the default boundary conditions, in place on an np.longdouble parent array"""
    assert a.dtype == LD and a.flags.f_contiguous
    L, G = lib(), _Grid(g)
    N, H = (g.Nx, g.Ny, g.Nz), (g.Hx, g.Hy, g.Hz)
    if fill_boundary_normal_velocities:
        for d in range(3):
            if g.topo[d] == O.BOUNDED and (loc >> d) & 1 and loc in (1, 2, 4):
                L.ocn_oracle_fill_open_bcs(G.ref, loc, _p(a), d, None, None)
    for d in range(3):
        if g.topo[d] == O.BOUNDED and not ((loc >> d) & 1):
            L.ocn_oracle_fill_flux(G.ref, loc, _p(a), d)
    sx, sy, sz = a.shape
    for d in range(3):
        if g.topo[d] == O.PERIODIC:
            L.ocn_oracle_fill_periodic(_p(a), sx, sy, sz, d, N[d], H[d])


def momentum_tendencies(g, u, v, w, scheme=O.ADV_WENO5):
    G = _Grid(g)
    u, v, w = widen(u), widen(v), widen(w)
    out = [zeros(g, l) for l in (O.LOC_U, O.LOC_V, O.LOC_W)]
    lib().ocn_oracle_momentum_tendencies_scheme(G.ref, scheme, _p(u), _p(v), _p(w), *(_p(a) for a in out))
    return out


def tracer_tendency(g, u, v, w, c, scheme=O.ADV_WENO5):
    G = _Grid(g)
    u, v, w, c = widen(u), widen(v), widen(w), widen(c)
    Gc = zeros(g, O.LOC_C)
    lib().ocn_oracle_tracer_tendency_scheme(G.ref, scheme, _p(u), _p(v), _p(w), _p(c), _p(Gc))
    return Gc


def momentum_extra_tendencies(g, ph, u, v, w, T, S, pHY, Gu, Gv, Gw, nu_e=None):
    """returns (Gu, Gv, Gw) + the non-advective terms; the given tendencies (Float64 or extended) are not modified"""
    G, P = _Grid(g), _Physics(ph)
    u, v, w, T, S, pHY, nu_e = (widen(a) for a in (u, v, w, T, S, pHY, nu_e))
    out = [widen(a) for a in (Gu, Gv, Gw)]
    lib().ocn_oracle_momentum_extra_tendencies_nu(G.ref, P.ref, _p(u), _p(v), _p(w), _p(T), _p(S), _p(pHY), _p(nu_e),
                                                  *(_p(a) for a in out))
    return out


def tracer_diffusion(g, kappa, c, Gc, kappa_e=None):
    """returns Gc - ∇·q; Gc itself is not modified"""
    G = _Grid(g)
    c, kappa_e, out = widen(c), widen(kappa_e), widen(Gc)
    lib().ocn_oracle_tracer_diffusion_kappa(G.ref, C.c_longdouble(kappa), _p(kappa_e), _p(c), _p(out))
    return out


def amd_viscosity(g, Cnu, u, v, w):
    G = _Grid(g)
    u, v, w = widen(u), widen(v), widen(w)
    nu_e = zeros(g, O.LOC_C)
    lib().ocn_oracle_amd_viscosity(G.ref, C.c_longdouble(Cnu), _p(u), _p(v), _p(w), _p(nu_e))
    return nu_e


def amd_diffusivity(g, Ck, u, v, w, c):
    G = _Grid(g)
    u, v, w, c = widen(u), widen(v), widen(w), widen(c)
    kappa_e = zeros(g, O.LOC_C)
    lib().ocn_oracle_amd_diffusivity(G.ref, C.c_longdouble(Ck), _p(u), _p(v), _p(w), _p(c), _p(kappa_e))
    return kappa_e


def divergence(g, u, v, w):
    G = _Grid(g)
    u, v, w = widen(u), widen(v), widen(w)
    out = np.zeros((g.Nx, g.Ny, g.Nz), dtype=LD, order="F")
    lib().ocn_oracle_divergence(G.ref, _p(u), _p(v), _p(w), _p(out))
    return out

