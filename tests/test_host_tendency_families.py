"""The `_terms` entry-point families of the C ABI without a GPU: every sibling of a family -- with its optional parts (stokes drift, forcing)
absent and present -- refuses the same bad argument with the same status and the same message text.  The checks run before any HIP call,
so fake device pointers are never followed.  A message may begin with the name of the entry point that raised it; that prefix is
not part of the compared text."""
import ctypes as C
import re

import pytest

P, B = "Periodic", "Bounded"
INVALID = -1  # OCN_ERR_INVALID_ARGUMENT (include/ocn_hip.h)
CENTERED2 = 1


@pytest.fixture(scope="module")
def pkg():
    import oceananigans_jl_amd as ocn
    return ocn


def _grid(pkg, topo=(P, P, B)):
    return pkg.RectilinearGrid(None, size=(16, 16, 8), x=(0, 1), y=(0, 1), z=(-1, 0), topology=topo, halo=(3, 3, 3))


def _ptr(k):
    return C.c_void_p(8 * k)  # distinct, never dereferenced


class Args:
    """one valid argument set; a test case changes exactly one thing"""

    def __init__(self, pkg):
        L = pkg._lib
        self.grid, self.terms = _grid(pkg), L.CModelTerms()
        self.u, self.v, self.w, self.Gu, self.Gv, self.Gw = (_ptr(k) for k in range(1, 7))
        self.Gmu, self.Gmv, self.Gmw, self.uo, self.vo, self.wo = (_ptr(k) for k in range(7, 13))
        self.c, self.Gc, self.Gmc, self.co = (_ptr(k) for k in range(13, 17))
        self.c2, self.Gc2, self.Gmc2, self.co2 = (_ptr(k) for k in range(17, 21))
        self.kappa_e, self.has_zeta, self.range = None, 0, None

    def set(self, **kw):
        for k, v in kw.items():
            assert hasattr(self, k)
            setattr(self, k, v)
        return self


def _stokes(L):
    return L.CStokesDrift()


def _forcing(L):
    f = L.CForcing()
    f.n_terms = 1
    f.term[0].kind, f.term[0].mask_dim, f.term[0].target_dim = 2, -1, -1  # a Relaxation with a number for mask and target
    return f


def _families(pkg):
    """family -> [(label, call(a))]: every sibling, with each optional part absent (NULL, and an array of three NULLs) and present"""
    lib, L = pkg._lib.lib(), pkg._lib
    sd, fr = _stokes(L), _forcing(L)
    keep = [sd, fr]  # referenced by the closures below
    stokes = [("no stokes", None), ("stokes", C.byref(sd))]
    mforcing = [("no forcing", None), ("three NULLs", L.forcing_array([None, None, None])), ("forcing", L.forcing_array([C.pointer(fr), None, None]))]
    tforcing = [("no forcing", None), ("forcing", C.byref(fr))]

    def mom(a):
        return (a.u, a.v, a.w, a.Gu, a.Gv, a.Gw)

    def mom_rk3(a):
        return mom(a) + (a.Gmu, a.Gmv, a.Gmw, a.uo, a.vo, a.wo, 1.0, 0.5, 0.25, a.has_zeta, a.range, None)

    def tr(a):
        return (a.u, a.v, a.w, a.c, a.Gc)

    def tr_rk3(a):
        return tr(a) + (a.Gmc, a.co, 1.0, 0.5, 0.25, a.has_zeta, a.range, None)

    fam = {"momentum": [], "momentum_rk3": [], "tracer": [], "tracer_rk3": [], "tracer_pair": []}
    fam["momentum"].append(("terms", lambda a: lib.ocn_compute_momentum_tendencies_terms(a.grid.cref, C.byref(a.terms), *mom(a), a.range, None)))
    fam["momentum_rk3"].append(("terms_rk3", lambda a: lib.ocn_compute_momentum_tendencies_terms_rk3(a.grid.cref, C.byref(a.terms), None, None, *mom_rk3(a))))
    for sl, s in stokes:
        fam["momentum"].append((f"terms_stokes, {sl}", lambda a, s=s: lib.ocn_compute_momentum_tendencies_terms_stokes(
            a.grid.cref, C.byref(a.terms), s, *mom(a), a.range, None)))
        fam["momentum_rk3"].append((f"terms_rk3_stokes, {sl}", lambda a, s=s: lib.ocn_compute_momentum_tendencies_terms_rk3_stokes(
            a.grid.cref, C.byref(a.terms), s, None, None, *mom_rk3(a))))
        for fl, f in mforcing:
            fam["momentum"].append((f"terms_forced, {sl}, {fl}", lambda a, s=s, f=f: lib.ocn_compute_momentum_tendencies_terms_forced(
                a.grid.cref, C.byref(a.terms), s, f, *mom(a), a.range, None)))
            fam["momentum_rk3"].append((f"terms_rk3_forced, {sl}, {fl}", lambda a, s=s, f=f: lib.ocn_compute_momentum_tendencies_terms_rk3_forced(
                a.grid.cref, C.byref(a.terms), s, f, None, None, *mom_rk3(a))))
    fam["tracer"].append(("terms", lambda a: lib.ocn_compute_tracer_tendency_terms(a.grid.cref, C.byref(a.terms), 0.0, a.kappa_e, *tr(a), a.range, None)))
    fam["tracer_rk3"].append(("terms_rk3", lambda a: lib.ocn_compute_tracer_tendency_terms_rk3(a.grid.cref, C.byref(a.terms), 0.0, a.kappa_e, None, *tr_rk3(a))))
    for fl, f in tforcing:
        fam["tracer"].append((f"terms_forced, {fl}", lambda a, f=f: lib.ocn_compute_tracer_tendency_terms_forced(
            a.grid.cref, C.byref(a.terms), 0.0, a.kappa_e, f, *tr(a), a.range, None)))
        fam["tracer_rk3"].append((f"terms_rk3_forced, {fl}", lambda a, f=f: lib.ocn_compute_tracer_tendency_terms_rk3_forced(
            a.grid.cref, C.byref(a.terms), 0.0, a.kappa_e, f, None, *tr_rk3(a))))

    def pair(a):
        did = C.c_int32(-1)
        return lib.ocn_compute_tracer_pair_tendency_terms_rk3(
            a.grid.cref, C.byref(a.terms), (C.c_double * 2)(0.0, 0.0), L.ptr_array([a.kappa_e, None]), None, a.u, a.v, a.w,
            L.ptr_array([a.c, a.c2]), L.ptr_array([a.Gc, a.Gc2]), L.ptr_array([a.Gmc, a.Gmc2]), L.ptr_array([a.co, a.co2]), 1.0, 0.5, 0.25,
            a.has_zeta, a.range, C.byref(did), None)
    fam["tracer_pair"].append(("pair", pair))
    return fam, keep


def _refusal(pkg, family, a, expect):
    """every sibling refuses `a` with OCN_ERR_INVALID_ARGUMENT and one message text (the leading entry-point name aside) containing `expect`"""
    lib = pkg._lib.lib()
    fam, keep = _families(pkg)
    texts = {}
    for label, call in fam[family]:
        assert call(a) == INVALID, (family, label)
        msg = lib.ocn_last_error().decode()
        texts[label] = re.sub(r"^ocn_compute_\w+: ", "", msg)
        assert expect in texts[label], (family, label, msg)
    assert len(set(texts.values())) == 1, texts


WALLED = (B, B, B)


@pytest.mark.parametrize("family,field", [("momentum", "u"), ("momentum", "Gw"), ("momentum_rk3", "v"), ("momentum_rk3", "wo"), ("tracer", "c"),
                                          ("tracer", "Gc"), ("tracer_rk3", "w"), ("tracer_rk3", "co")])
def test_null_field_pointer(pkg, family, field):
    _refusal(pkg, family, Args(pkg).set(**{field: None}), "null field pointer")


def test_null_field_pointer_pair(pkg):
    _refusal(pkg, "tracer_pair", Args(pkg).set(u=None), "null pointer")
    _refusal(pkg, "tracer_pair", Args(pkg).set(Gc2=None), "null or aliased field pointer")


def test_output_aliasing_its_input(pkg):
    a = Args(pkg)
    _refusal(pkg, "momentum_rk3", Args(pkg).set(vo=a.v), "outputs must not alias the inputs")
    _refusal(pkg, "tracer_rk3", Args(pkg).set(co=a.c), "the output must not alias the input")
    _refusal(pkg, "tracer_pair", Args(pkg).set(co2=a.c2), "null or aliased field pointer")


def test_has_zeta_needs_previous_tendencies(pkg):
    _refusal(pkg, "momentum_rk3", Args(pkg).set(has_zeta=1, Gmv=None), "G⁻ pointers are required when has_zeta != 0")
    _refusal(pkg, "tracer_rk3", Args(pkg).set(has_zeta=1, Gmc=None), "G⁻ is required when has_zeta != 0")
    _refusal(pkg, "tracer_pair", Args(pkg).set(has_zeta=1, Gmc=None), "G⁻ is required when has_zeta != 0")


@pytest.mark.parametrize("family", ["tracer", "tracer_rk3", "tracer_pair"])
def test_kappa_e_needs_closure_2(pkg, family):
    _refusal(pkg, family, Args(pkg).set(kappa_e=_ptr(30)), "kappa_e is only meaningful with closure == 2")


@pytest.mark.parametrize("family", ["momentum_rk3", "tracer_rk3"])
def test_range_on_a_walled_grid(pkg, family):
    rng = (C.c_int32 * 6)(1, 16, 1, 16, 1, 8)
    _refusal(pkg, family, Args(pkg).set(grid=_grid(pkg, WALLED), range=rng), "ranges need Periodic x and y")


@pytest.mark.parametrize("family", ["tracer_rk3", "tracer_pair"])
def test_centered2_with_a_substep(pkg, family):
    a = Args(pkg)
    a.terms.advection = CENTERED2
    _refusal(pkg, family, a, "advection must be WENO5 or UpwindBiased5")
