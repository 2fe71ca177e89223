"""What the Python host relies on when it always calls the widest entry point of a `_terms` family: called with a NULL stokes drift and a
NULL forcing (both a NULL array and an array of three NULLs), the widest entry point returns what every narrower sibling returns, bit for
bit -- G for the tendency calls, G and the substep outputs for the `_rk3` calls -- and two tracers sent down the pair route
(fused_tracer_launches: ocn_compute_tracer_pair_tendency_terms_rk3, which declines unless it is switched on, then the single launches)
return what two ocn_compute_tracer_tendency_terms_rk3 calls return.

Terms that make every pass run: FPlane, a constant-ν closure, BuoyancyTracer, one bottom flux on u and on the tracer."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

P, B = "Periodic", "Bounded"
SHAPES = [((16, 8, 8), (P, P, B)),    # the tiled kernels (their threshold is 16 x 8 x 4)
          ((8, 8, 4), (P, P, B)),     # the per-cell kernels
          ((24, 16, 8), (B, B, B))]   # interior box (18 x 10 after three cells per wall) + wall frames
LOCS = {"u": 1, "v": 2, "w": 4, "c": 0}
DT, GAMMA, ZETA, KAPPA = 0.01, 5 / 12, -17 / 60, 2e-2


class _Case:
    def __init__(self, ocn, size, topo, advection, mode):
        import torch
        self.ocn, self.L, self.torch = ocn, ocn._lib, torch
        L = self.L
        pg = ocn.RectilinearGrid(ocn.GPU(), size=size, x=(0, 2.0), y=(0, 3.0), z=(-1.0, 0.0), topology=topo, halo=(3, 3, 3))
        self.pg = pg.with_math_mode(ocn.MATH_STRICT if mode == "strict" else ocn.MATH_FAST)  # (the process default stays as it is)
        gen = torch.Generator().manual_seed(20261019)

        def rand(loc, bcs=None):
            f = ocn.Field(loc, self.pg, boundary_conditions=bcs)
            f.data.copy_(torch.rand(tuple(f.data.shape), generator=gen, dtype=torch.float64) * 2 - 1)
            return f
        bottom = lambda q: ocn.FieldBoundaryConditions(bottom=ocn.FluxBoundaryCondition(q))
        self.f = {"u": rand(1, bottom(-3.7e-2)), "v": rand(2), "w": rand(4), "c": rand(0, bottom(2.3e-2)), "c2": rand(0)}
        self.Gm = {n: rand(LOCS[n[0]]) for n in self.f}
        t = self.terms = L.CModelTerms()
        t.advection = advection
        t.coriolis, t.f = 1, 0.7
        t.closure, t.nu = 1, 3e-2
        t.buoyancy, t.T = L.BUOYANCY_TRACER, self.f["c"].ptr
        self.bcs = {n: self.f[n].boundary_conditions.c_struct(self.pg) for n in ("u", "c")}

    def zeros(self, names):
        return [self.ocn.Field(LOCS[n[0]], self.pg) for n in names]

    def same(self, results, what):
        """every result (a list of fields) equals the first one, bit for bit, and is not trivially zero"""
        self.ocn.sync_device()
        first = results[0][1]
        assert all(float(x.data.abs().max()) > 0 for x in first), what
        for label, fields in results[1:]:
            for q, (a, b) in enumerate(zip(first, fields)):
                assert self.torch.equal(a.data, b.data), f"{what}: {label} differs from {results[0][0]} in output {q}"

    def momentum(self):
        L, f, t, g = self.L, self.f, C.byref(self.terms), self.pg.cref
        uvw = (f["u"].ptr, f["v"].ptr, f["w"].ptr)
        res = []
        for label, name, extra in (("terms", "ocn_compute_momentum_tendencies_terms", ()),
                                   ("terms_stokes(NULL)", "ocn_compute_momentum_tendencies_terms_stokes", (None,)),
                                   ("terms_forced(NULL, NULL)", "ocn_compute_momentum_tendencies_terms_forced", (None, None)),
                                   ("terms_forced(NULL, three NULLs)", "ocn_compute_momentum_tendencies_terms_forced",
                                    (None, L.forcing_array([None, None, None])))):
            G = self.zeros("uvw")
            L.call(name, g, t, *extra, *uvw, *[x.ptr for x in G], None, 0)
            res.append((label, G))
        self.same(res, "momentum tendencies")

    def tracer(self):
        L, f, t, g = self.L, self.f, C.byref(self.terms), self.pg.cref
        args = (f["u"].ptr, f["v"].ptr, f["w"].ptr, f["c"].ptr)
        res = []
        for label, name, extra in (("terms", "ocn_compute_tracer_tendency_terms", ()), ("terms_forced(NULL)", "ocn_compute_tracer_tendency_terms_forced", (None,))):
            G = self.zeros("c")
            L.call(name, g, t, KAPPA, None, *extra, *args, G[0].ptr, None, 0)
            res.append((label, G))
        self.same(res, "tracer tendency")

    def momentum_rk3(self):
        L, f, t, g = self.L, self.f, C.byref(self.terms), self.pg.cref
        uvw = (f["u"].ptr, f["v"].ptr, f["w"].ptr)
        bcs = (C.byref(self.bcs["u"]), None)
        Gm = [self.Gm[n].ptr for n in "uvw"]
        res = []
        for label, name, extra in (("terms_rk3", "ocn_compute_momentum_tendencies_terms_rk3", ()),
                                   ("terms_rk3_stokes(NULL)", "ocn_compute_momentum_tendencies_terms_rk3_stokes", (None,)),
                                   ("terms_rk3_forced(NULL, NULL)", "ocn_compute_momentum_tendencies_terms_rk3_forced", (None, None)),
                                   ("terms_rk3_forced(NULL, three NULLs)", "ocn_compute_momentum_tendencies_terms_rk3_forced",
                                    (None, L.forcing_array([None, None, None])))):
            out = self.zeros("uvwuvw")
            L.call(name, g, t, *extra, *bcs, *uvw, *[x.ptr for x in out[:3]], *Gm, *[x.ptr for x in out[3:]], DT, GAMMA, ZETA, 1, None, 0)
            res.append((label, out))
        self.same(res, "momentum tendencies + substep")

    def tracer_rk3(self):
        L, f, t, g = self.L, self.f, C.byref(self.terms), self.pg.cref
        res = []
        for label, name, extra in (("terms_rk3", "ocn_compute_tracer_tendency_terms_rk3", ()),
                                   ("terms_rk3_forced(NULL)", "ocn_compute_tracer_tendency_terms_rk3_forced", (None,))):
            out = self.zeros("cc")
            L.call(name, g, t, KAPPA, None, *extra, C.byref(self.bcs["c"]), f["u"].ptr, f["v"].ptr, f["w"].ptr, f["c"].ptr, out[0].ptr,
                   self.Gm["c"].ptr, out[1].ptr, DT, GAMMA, ZETA, 1, None, 0)
            res.append((label, out))
        self.same(res, "tracer tendency + substep")

    def tracer_pair(self):
        from oceananigans_jl_amd.models import fused_tracer_launches
        L, f, t, g = self.L, self.f, C.byref(self.terms), self.pg.cref
        names, kappas = ("c", "c2"), (KAPPA, 0.5 * KAPPA)
        single = self.zeros("cccc")
        for q, n in enumerate(names):
            b = C.byref(self.bcs[n]) if n in self.bcs else None
            L.call("ocn_compute_tracer_tendency_terms_rk3", g, t, kappas[q], None, b, f["u"].ptr, f["v"].ptr, f["w"].ptr, f[n].ptr, single[q].ptr,
                   self.Gm[n].ptr, single[2 + q].ptr, DT, GAMMA, ZETA, 1, None, 0)
        pair = self.zeros("cccc")
        fused_tracer_launches(self.pg, t, f["u"], f["v"], f["w"], [f[n] for n in names], list(kappas), [None, None], pair[:2],
                              [self.Gm[n] for n in names], [x.data for x in pair[2:]], DT, GAMMA, ZETA, 1, None, 0)
        self.same([("two terms_rk3 calls", single), ("the pair route", pair)], "two tracers + substep")


ADVECTION = {"WENO5": 0, "Centered2": 1, "UpwindBiased5": 2}


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("advection", list(ADVECTION))
@pytest.mark.parametrize("size,topo", SHAPES, ids=["x".join(map(str, s)) + "_" + "".join(n[0] for n in t) for s, t in SHAPES])
def test_widest_entry_point_with_nothing_optional_equals_every_narrower_sibling(ocn, size, topo, advection, mode):
    case = _Case(ocn, size, topo, ADVECTION[advection], mode)
    case.momentum()
    case.tracer()
    if advection != "Centered2":  # (the tracer kernels of Centered(order=2) have no substep)
        case.momentum_rk3()
        case.tracer_rk3()
        case.tracer_pair()
