"""RiBasedVerticalDiffusivity on the GPU (csrc/ri_based_diffusivity.hip): Ri, κᶜ and κᵘ against the NumPy restatement of the reference
(tests/ri_based_numpy.py, pinned without a GPU in tests/test_host_ri_based.py) bit for bit, the one-launch entry against the two launches,
five steps of the hydrostatic model against a twin without closure driven through the public stage functions and the library's entry
points in the reference's order, conservation of the column integrals, a bit-identical checkpoint restart and the README snippet.

Shapes are the smallest at which the column kernels can still go wrong: (70, 5, 6) has a partial second block in x (64 lanes wide) and in y
(4 rows), (8, 8, 1) writes only the peripheral face, (8, 8, 2) has a single interior face whose N²(k + 1) comes from the top halo, (9, 7, 11)
has unequal halos wider than the stencils, (12, 10, 5) has walls in x and y next to the filter."""
import ctypes as C

import numpy as np
import pytest

import convective_adjustment_numpy as CAN
import implicit_diffusion_numpy as IDN
import ri_based_numpy as RBN
from helpers import from_dev, stretched_faces, to_dev

pytestmark = pytest.mark.gpu

P, B = "Periodic", "Bounded"
U, V, CC, CCF = 1, 2, 0, 4  # location masks
SEAWATER = ("SeawaterBuoyancy", 9.80665, 1.67e-4, 7.80e-4)
SENTINEL = -7.0
# size, z ("stretched" or an interval), halo, topology
CASES = [((70, 5, 6), "stretched", (3, 3, 3), (P, P, B)),
         ((8, 8, 1), (-1.0, 0.0), (3, 3, 1), (P, P, B)),
         ((8, 8, 2), "stretched", (3, 3, 2), (P, P, B)),
         ((9, 7, 11), (-1.0, 0.0), (4, 3, 5), (P, P, B)),
         ((12, 10, 5), "stretched", (3, 3, 3), (B, B, B))]
IDS = ["70x5x6", "Nz1", "Nz2", "halo435", "walls"]
TAPERS = [RBN.LINEAR, RBN.EXP, RBN.TANH]
# a finite maximum_diffusivity / maximum_viscosity that clip (κᶜᵃ = 1.7, ν₀ = 0.7), and the reference's +inf
MAXIMA = [(1.0, 0.5), (np.inf, np.inf)]


def _grid(ocn, size, z, halo, topo):
    zz = stretched_faces(size[2]) if isinstance(z, str) else z
    return ocn.RectilinearGrid(ocn.GPU(), size=size, x=(0, 1), y=(0, 0.5), z=zz, topology=topo, halo=halo)


_inputs = {}


def _case(ocn, n):
    """grid, its description and seeded parent arrays (halos included): uniformly random T, S in [-1, 1] (N² of both signs on every kind of
    face), u and v uniformly random of amplitude 0.02 (Ri of order one) but exactly 0 in the columns i <= Nx / 3 + 1 (at rest: S² = 0, so
    Ri = +inf where stable and 0 where not), random positive κ fields to average from, and a top flux array of both signs; shared, never
    modified"""
    if n not in _inputs:
        pg = _grid(ocn, *CASES[n])
        g = IDN.describe(pg)
        rng = np.random.default_rng(9100 + n)
        u, v = (0.02 * rng.uniform(-1, 1, pg.parent_shape(loc)) for loc in (U, V))
        rest = g.Hx + g.Nx // 3 + 1
        u[:rest + 1] = 0.0
        v[:rest] = 0.0
        T, S = (rng.uniform(-1, 1, pg.parent_shape(CC)) for _ in range(2))
        k0 = [rng.uniform(0.05, 1.0, CAN.ccf_shape(g)) for _ in range(2)]
        flux = rng.uniform(-1e-3, 1e-3, (g.Nx, g.Ny))
        _inputs[n] = dict(pg=pg, g=g, u=u, v=v, T=T, S=S, k0=k0, flux=flux)
    return _inputs[n]


def _interior(g):
    return (slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny), slice(g.Hz, g.Hz + g.Nz))


def _terms(ocn, buoyancy, T, S):
    L = ocn._lib
    terms = L.CModelTerms()
    if buoyancy == "SeawaterBuoyancy":
        terms.buoyancy, terms.g, terms.alpha, terms.beta, terms.T, terms.S = L.BUOYANCY_SEAWATER_TS, *SEAWATER[1:], T.ptr, S.ptr
    elif buoyancy == "BuoyancyTracer":
        terms.buoyancy, terms.T = L.BUOYANCY_TRACER, T.ptr
    return terms


def _tracers(c, buoyancy):
    """(spec of the restatement, T, S): the buoyancy tracer is 2e-3 T so that its Ri is of order one too"""
    if buoyancy == "SeawaterBuoyancy":
        return SEAWATER, c["T"], c["S"]
    if buoyancy == "BuoyancyTracer":
        return "BuoyancyTracer", 2e-3 * c["T"], None
    return None, None, None


class _Top:
    """a top flux condition for the device (struct ocn_bc, kept alive with its array) and for the restatement"""

    def __init__(self, ocn, spec):
        import torch
        L = ocn._lib
        self.host, self.dev = spec, None
        if spec is None:
            self.bc = L.CBc(L.BC_DEFAULT, 0, 0.0, 0.0, None)
        elif isinstance(spec, tuple):
            self.bc = L.CBc(L.BC_FLUX, 0, spec[0], spec[1], None)
        elif np.ndim(spec) == 0:
            self.bc = L.CBc(L.BC_FLUX, 0, float(spec), 0.0, None)
        else:
            self.dev = torch.from_numpy(np.ascontiguousarray(spec.T)).to("cuda")
            self.bc = L.CBc(L.BC_FLUX, 0, 0.0, 0.0, self.dev.data_ptr())

    @property
    def ref(self):
        return C.pointer(self.bc)


def _fluxes(ocn, c):
    """(name, top condition of T or b, of S): a positive, a negative and a zero flux as numbers, an array of both signs, none at all, and
    value + coeff c[i, j, Nz]"""
    return [("positive", _Top(ocn, 1e-3), _Top(ocn, -2e-4)), ("negative", _Top(ocn, -1e-3), _Top(ocn, None)),
            ("zero", _Top(ocn, 0.0), _Top(ocn, 0.0)), ("array", _Top(ocn, c["flux"]), _Top(ocn, None)),
            ("none", _Top(ocn, None), _Top(ocn, None)), ("coeff", _Top(ocn, (2e-4, 1e-3)), _Top(ocn, c["flux"][::-1].copy()))]


def _fill_ri_halos(ocn, c, ri_field, want_filled):
    """the halo fill between the two launches: the package's own on (Periodic, Periodic, Bounded) -- compared, whole parent, with the
    restatement's --, the restatement's uploaded next to walls (first halo plane mirrored: all the filter reads)"""
    if c["g"].topo[0] == P:
        ocn.fill_halo_regions((ri_field,), fill_boundary_normal_velocities=False)
        ocn.sync_device()
        assert np.array_equal(from_dev(ri_field), want_filled)
        return ri_field
    return to_dev(ocn, c["pg"], CCF, want_filled)


# ---- 1. Ri, κᶜ, κᵘ bit for bit; the one-launch entry ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("buoyancy", ["SeawaterBuoyancy", "BuoyancyTracer", None])
@pytest.mark.parametrize("n", range(len(CASES)), ids=IDS)
def test_kernels_equal_the_restatement_bit_for_bit(ocn, n, buoyancy):
    """For every tapering, with and without the filter, clipping and not, and six top conditions: Ri into an array prefilled with a
    sentinel, then two successive diffusivity calls on κ arrays prefilled with random values (the second averages from the first's
    result); whole parent arrays compared, so face Nz + 1 and every halo are shown untouched; NaN positions equal (there are none).
    Without the filter the one-launch entry must give the same three arrays as the two launches.  The branch counts of the
    restatement (convecting, entraining, neither; taper = 1 and = 0 for Linear; clipped and not; Ri = +inf, 0 and in between) are asserted
    first: they are a condition on the inputs."""
    c = _case(ocn, n)
    pg, g, L = c["pg"], c["g"], ocn._lib
    spec, Th, Sh = _tracers(c, buoyancy)
    T = to_dev(ocn, pg, CC, Th if Th is not None else c["T"])
    S = to_dev(ocn, pg, CC, c["S"])
    u, v = to_dev(ocn, pg, U, c["u"]), to_dev(ocn, pg, V, c["v"])
    terms = _terms(ocn, buoyancy, T, S)
    sentinel = np.full(CAN.ccf_shape(g), SENTINEL)
    sl = _interior(g)

    # the restatement first, with its branch counts: a condition on the inputs, checked before any comparison
    want_ri = RBN.ri_number(g, spec, c["u"], c["v"], Th, Sh, sentinel)
    assert not np.isnan(want_ri).any()
    want_filled = RBN.fill_xy_halos(g, want_ri) if g.topo[0] == P else RBN.fill_xy_halos_topology(g, want_ri)
    seen = dict(convecting=0, entraining=0, neither=0, tau_one=0, tau_zero=0, clipped=0, unclipped=0, clipped_u=0, unclipped_u=0,
                Ri_inf=int(np.isinf(want_ri[sl]).sum()), Ri_zero=int((want_ri[sl] == 0).sum()),
                Ri_finite=int(((want_ri[sl] > 0) & np.isfinite(want_ri[sl])).sum()))
    plan = []
    for name, top_T, top_S in _fluxes(ocn, c):
        for taper in TAPERS:
            for filt in (RBN.FILTER_NONE, RBN.FILTER_FIVE_POINT):
                for max_c, max_u in MAXIMA:
                    cl = RBN.closure_dict(tapering=taper, horizontal_filter=filt, maximum_diffusivity=max_c, maximum_viscosity=max_u)
                    cs = L.CRiBased(cl["nu0"], cl["kappa0"], cl["kappa_ca"], cl["C_en"], cl["C_av"], cl["Ri0"], cl["Ri_delta"],
                                    cl["minimum_entrainment_buoyancy_gradient"], max_c, max_u, taper, filt)
                    w_c, w_u = c["k0"]
                    stages = []
                    for call in range(2):
                        w_c, w_u, br = RBN.diffusivities(g, spec, cl, Th, Sh, top_T.host, top_S.host if buoyancy == "SeawaterBuoyancy" else None,
                                                         want_filled, w_c, w_u, with_branches=True)
                        assert not np.isnan(w_c).any() and not np.isnan(w_u).any()
                        stages.append((w_c, w_u))
                    seen["convecting"] += int(br["convecting"].sum())
                    seen["entraining"] += int(br["entraining"].sum())
                    seen["neither"] += int((~br["convecting"] & ~br["entraining"]).sum())
                    if taper == RBN.LINEAR:
                        seen["tau_one"] += int((br["tau"] == 1.0).sum())
                        seen["tau_zero"] += int((br["tau"] == 0.0).sum())
                    if np.isfinite(max_c):
                        seen["clipped"] += int(br["clipped_c"].sum())
                        seen["unclipped"] += int((~br["clipped_c"]).sum())
                        seen["clipped_u"] += int(br["clipped_u"].sum())
                        seen["unclipped_u"] += int((~br["clipped_u"]).sum())
                    plan.append((f"{name} taper {taper} filter {filt} max {max_c}", top_T, top_S, cs, filt, stages))
    print(f"case {IDS[n]} {buoyancy}: {seen}")
    if buoyancy is not None:
        assert all(count >= 1 for count in seen.values()), seen
    else:  # no buoyancy: N² = 0, Ri = 0, neither branch
        assert seen["convecting"] == 0 and seen["entraining"] == 0 and seen["neither"] > 0 and np.all(want_ri[sl] == 0)

    # the device
    ri = to_dev(ocn, pg, CCF, sentinel)
    L.call("ocn_compute_ri_number", pg.cref, C.byref(terms), u.ptr, v.ptr, ri.ptr, 0)
    ocn.sync_device()
    got_ri = from_dev(ri)
    assert np.array_equal(got_ri, want_ri)
    assert np.all(got_ri[:, :, g.Hz + g.Nz:] == SENTINEL) and np.all(got_ri[:g.Hx] == SENTINEL) and np.all(got_ri[:, :g.Hy] == SENTINEL)
    ri_filled = _fill_ri_halos(ocn, c, ri, want_filled)
    for tag, top_T, top_S, cs, filt, stages in plan:
        kc, ku = to_dev(ocn, pg, CCF, c["k0"][0]), to_dev(ocn, pg, CCF, c["k0"][1])
        for call in range(2):
            L.call("ocn_compute_ri_based_diffusivities", pg.cref, C.byref(terms), C.byref(cs), top_T.ref, top_S.ref, ri_filled.ptr, kc.ptr, ku.ptr, 0)
            ocn.sync_device()
            got_c, got_u = from_dev(kc), from_dev(ku)
            assert np.array_equal(got_c, stages[call][0]), f"κc {tag} call {call}: {np.abs(got_c - stages[call][0]).max():.3e}"
            assert np.array_equal(got_u, stages[call][1]), f"κu {tag} call {call}: {np.abs(got_u - stages[call][1]).max():.3e}"
        assert np.array_equal(got_c[:, :, g.Hz + g.Nz:], c["k0"][0][:, :, g.Hz + g.Nz:])  # face Nz + 1 and the top halo
        assert np.all(got_c[sl][:, :, 0] < stages[0][0][sl][:, :, 0])                    # face 1: κ⁺ = 0, the average decays
        if filt == RBN.FILTER_NONE:  # the one-launch entry: twice, from fresh arrays
            ri2 = to_dev(ocn, pg, CCF, sentinel)
            kc2, ku2 = to_dev(ocn, pg, CCF, c["k0"][0]), to_dev(ocn, pg, CCF, c["k0"][1])
            for call in range(2):
                L.call("ocn_compute_ri_based_diffusivities_fused", pg.cref, C.byref(terms), C.byref(cs), top_T.ref, top_S.ref, u.ptr, v.ptr,
                       ri2.ptr, kc2.ptr, ku2.ptr, 0)
            ocn.sync_device()
            assert np.array_equal(from_dev(ri2), got_ri) and np.array_equal(from_dev(kc2), got_c) and np.array_equal(from_dev(ku2), got_u), tag


def test_constant_salinity_and_constant_temperature_kinds(ocn):
    """SeawaterBuoyancy(constant_salinity) / (constant_temperature): the missing tracer is a NULL pointer, its derivative and flux are 0"""
    c = _case(ocn, 0)
    pg, g, L = c["pg"], c["g"], ocn._lib
    u, v = to_dev(ocn, pg, U, c["u"]), to_dev(ocn, pg, V, c["v"])
    cl = RBN.closure_dict()
    cs = L.CRiBased(*[cl[k] for k in ("nu0", "kappa0", "kappa_ca", "C_en", "C_av", "Ri0", "Ri_delta", "minimum_entrainment_buoyancy_gradient",
                                       "maximum_diffusivity", "maximum_viscosity", "tapering", "horizontal_filter")])
    top = _Top(ocn, 1e-3)
    zeros = np.zeros(CAN.ccf_shape(g))
    for kind, Th, Sh, tops, hostT, hostS in ((L.BUOYANCY_SEAWATER_T, c["T"], None, (top.ref, C.POINTER(L.CBc)()), 1e-3, None),
                                             (L.BUOYANCY_SEAWATER_S, None, c["S"], (C.POINTER(L.CBc)(), top.ref), None, 1e-3)):
        terms = L.CModelTerms()
        terms.buoyancy, terms.g, terms.alpha, terms.beta = kind, *SEAWATER[1:]
        held = to_dev(ocn, pg, CC, Th if Th is not None else Sh)
        if Th is not None:
            terms.T = held.ptr
        else:
            terms.S = held.ptr
        ri, kc, ku = (to_dev(ocn, pg, CCF, zeros) for _ in range(3))
        L.call("ocn_compute_ri_based_diffusivities_fused", pg.cref, C.byref(terms), C.byref(cs), *tops, u.ptr, v.ptr, ri.ptr, kc.ptr, ku.ptr, 0)
        ocn.sync_device()
        want_ri = RBN.ri_number(g, SEAWATER, c["u"], c["v"], Th, Sh, zeros)
        want_c, want_u, br = RBN.diffusivities(g, SEAWATER, cl, Th, Sh, hostT, hostS, want_ri, zeros, zeros, with_branches=True)
        assert br["convecting"].any() and (~br["convecting"]).any()
        assert br["entraining"].any() == (Th is not None)  # Jᵇ = g α J_T > 0 with T alone, -g β J_S < 0 with S alone
        assert np.array_equal(from_dev(ri), want_ri) and np.array_equal(from_dev(kc), want_c) and np.array_equal(from_dev(ku), want_u)


# ---- 2. model steps against a twin without closure ---------------------------------------------------------------------------------------------
T_FLUX = 1e-3    # upward heat flux through the top: cooling, Jᵇ = g α J_T > 0
U_FLUX = -1e-4   # wind stress
PARAMETERS = dict(maximum_diffusivity=5.0)  # otherwise the defaults of the reference


def _model_grid(ocn):
    """z refined towards the bottom (Δz from 0.019 to 0.13), Δx = Δy = 1 (tests/test_gpu_convective_adjustment.py)"""
    faces = -1.0 + np.linspace(0.0, 1.0, 13) ** 1.6
    return ocn.RectilinearGrid(ocn.GPU(), size=(13, 6, 12), x=(0, 13), y=(0, 6), z=faces, topology=(P, P, B), halo=(3, 3, 3))


def _free_surface(ocn, kind):
    return {"explicit": lambda: ocn.ExplicitFreeSurface(), "split": lambda: ocn.SplitExplicitFreeSurface(substeps=10),
            "implicit": lambda: ocn.ImplicitFreeSurface()}[kind]()


def _initial(pg, noise=1.0):
    """a stable lower half under an unstable upper half (T falls towards the surface there), a sheared current, noise on everything"""
    rng = np.random.default_rng(9)
    zc = np.asarray(pg.nodes_1d(2, False))[:12]
    T = 20 + np.where(zc < -0.5, 2.0 * (zc + 0.5), -1.5 * (zc + 0.5))
    init = {name: np.broadcast_to(0.05 * (zc + 1.0) ** 2, (13, 6, 12)) + noise * 1e-3 * rng.uniform(-1, 1, (13, 6, 12)) for name in "uv"}
    init["T"] = np.broadcast_to(T, (13, 6, 12)) + noise * 0.05 * rng.uniform(-1, 1, (13, 6, 12))
    init["S"] = 35 + noise * 0.01 * rng.uniform(-1, 1, (13, 6, 12))
    return init


def _bcs(ocn):
    return {"T": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(T_FLUX)),
            "u": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(U_FLUX))}


def _dzmin(g):
    return float(np.min(g.dzc[g.Hz:g.Hz + g.Nz]))


class _Twin:
    """a HydrostaticFreeSurfaceModel WITHOUT closure stepped through its public stage functions and the library's entry points in the
    order of the reference (hydrostatic.py time_step, fused = False): the diffusivities by the new entries on fields of its own -- advanced
    at construction, in set and once per update_state!, as the reference's call sequence does --, their term and implicit step by the
    existing field-valued entries.  A NumPy copy of κᶜ, κᵘ is advanced by the restatement alongside."""

    def __init__(self, ocn, r, closure):
        import torch
        self.ocn, self.r, self.closure = ocn, r, closure
        self.implicit = isinstance(closure.time_discretization, ocn.VerticallyImplicitTimeDiscretization)
        self.filtered = closure.horizontal_Ri_filter is not None
        self.g = IDN.describe(r.grid)
        self.d = {name: ocn.ZFaceField(r.grid) for name in ("kappa_c", "kappa_u", "Ri")}
        self.cs = closure.c_struct()
        self.cl = RBN.closure_dict(**{k: getattr(self.cs, k) for k in RBN.closure_dict()})
        self.top_T = _Top(ocn, T_FLUX)
        self.scratch = torch.zeros((3, r.grid.Nz, r.grid.Ny, r.grid.Nx), dtype=torch.float64, device=r.u.data.device)
        self.host_c = self.host_u = np.zeros(CAN.ccf_shape(self.g))
        self.advance()  # the update_state! of the model's constructor

    def advance(self):
        """compute_diffusivities! + the halo fills, after r.update_state"""
        ocn, r, g, d = self.ocn, self.r, self.g, self.d
        L, nh, pg = ocn._lib, r._nh, r.grid
        nh._refresh_term_pointers()
        none = C.POINTER(L.CBc)()
        L.call("ocn_compute_ri_number", pg.cref, C.byref(nh._terms), r.u.ptr, r.v.ptr, d["Ri"].ptr, 0)
        ocn.fill_halo_regions((d["Ri"],), fill_boundary_normal_velocities=False)
        L.call("ocn_compute_ri_based_diffusivities", pg.cref, C.byref(nh._terms), C.byref(self.cs), self.top_T.ref, none, d["Ri"].ptr,
               d["kappa_c"].ptr, d["kappa_u"].ptr, 0)
        ocn.fill_halo_regions((d["kappa_c"], d["kappa_u"]), fill_boundary_normal_velocities=False)
        spec = ("SeawaterBuoyancy", nh.buoyancy.gravitational_acceleration, nh.buoyancy.equation_of_state.thermal_expansion,
                nh.buoyancy.equation_of_state.haline_contraction)
        T, S = r.field("T").parent(), r.field("S").parent()
        ri = RBN.fill_xy_halos(g, RBN.ri_number(g, spec, r.u.parent(), r.v.parent(), T, S, np.zeros(CAN.ccf_shape(g))))
        kc, ku = RBN.diffusivities(g, spec, self.cl, T, S, T_FLUX, None, ri, self.host_c, self.host_u)
        self.host_c, self.host_u = RBN.fill_xy_halos(g, kc), RBN.fill_xy_halos(g, ku)

    def set(self, **init):
        self.r.set(**init)
        self.advance()  # the update_state! of set!

    def update_state(self):
        from oceananigans_jl_amd import models
        ocn, r, d = self.ocn, self.r, self.d
        L, pg = ocn._lib, r.grid
        r.update_state(compute_tendencies=False)
        self.advance()
        r.compute_tendencies(boundary_contributions=False)
        Gn, nt = r._nh.timestepper._Gn, len(r.tracers)
        L.call("ocn_add_vertical_diffusivity_fluxes", pg.cref, d["kappa_u"].ptr, r.u.ptr, r.v.ptr, Gn[0].ptr, Gn[1].ptr, nt,
               L.ptr_array([d["kappa_c"].ptr] * nt), L.ptr_array([c.ptr for c in r.tracers]), L.ptr_array([G.ptr for G in Gn[3:]]),
               int(self.implicit), None, 0)
        models.compute_boundary_tendency_contributions(r._nh)

    def time_step(self, dt):
        ocn, r, d = self.ocn, self.r, self.d
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
            w = self.scratch
            kappas = [d["kappa_u"].ptr] * 2 + [d["kappa_c"].ptr] * len(r.tracers)
            scratch = [w[0].data_ptr(), w[1].data_ptr()] + [w[2].data_ptr()] * len(r.tracers)
            L.call("ocn_implicit_vertical_diffusion_step_fields", pg.cref, len(fields), L.ptr_array([f.ptr for f in fields]),
                   L.i32_array([f.loc for f in fields]), L.ptr_array(kappas), L.ptr_array(scratch), float(dt), s)
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


def _model(ocn, kind, closure, pg=None, **kw):
    base = dict(tracers=("T", "S"), buoyancy=ocn.SeawaterBuoyancy(), coriolis=ocn.FPlane(f=1e-4), math_mode=ocn.MATH_STRICT)
    base.update(kw)
    return ocn.HydrostaticFreeSurfaceModel(pg or _model_grid(ocn), closure=closure, boundary_conditions=_bcs(ocn),
                                           free_surface=_free_surface(ocn, kind), **base)


def _run_model_against_twin(ocn, kind, td, dt_number, **closure_kw):
    pg = _model_grid(ocn)
    closure = ocn.RiBasedVerticalDiffusivity(td, warning=False, **PARAMETERS, **closure_kw)
    m = _model(ocn, kind, closure, pg)
    r = _model(ocn, kind, None, pg, fused=False)
    assert m.fused is False and sorted(m.diffusivity_fields) == ["Ri", "kappa_c", "kappa_u"]
    g = IDN.describe(m.grid)
    for f in m.diffusivity_fields.values():
        assert f.loc == CCF and f.parent().shape == CAN.ccf_shape(g) and np.all(f.parent()[:, :, g.Hz + g.Nz:] == 0)
    twin = _Twin(ocn, r, closure)
    init = _initial(pg)
    m.set(**init)
    twin.set(**init)
    dt = dt_number * _dzmin(g) ** 2 / closure.kappa_ca
    for step in range(5):
        m.time_step(dt)
        twin.time_step(dt)
        for name in ("kappa_c", "kappa_u", "Ri"):
            assert np.array_equal(m.diffusivity_fields[name].parent(), twin.d[name].parent()), f"step {step} {name}"
        assert np.array_equal(twin.d["kappa_c"].parent(), twin.host_c) and np.array_equal(twin.d["kappa_u"].parent(), twin.host_u), f"step {step}"
    ocn.sync_device()
    for name in ("u", "v", "w", "T", "S"):
        a, b = m.field(name).parent(), r.field(name).parent()
        print(f"{kind} {td} {name}: max |value| after five steps {np.abs(a).max():.3e}")
        assert np.isfinite(a).all(), name
        assert np.array_equal(a, b), f"{name}: max difference {np.abs(a - b).max():.3e}"
    assert np.array_equal(m.eta.cpu().numpy(), r.eta.cpu().numpy())
    for Gm_, Gr_ in zip(m._nh.timestepper._Gn, r._nh.timestepper._Gn):
        assert np.array_equal(Gm_.parent(), Gr_.parent())
    kc = m.diffusivity_fields["kappa_c"].interior()[:, :, :12]
    assert np.abs(m.u.interior()).max() > 0 and np.abs(m.eta.cpu().numpy()).max() > 0
    assert np.all(kc >= 0) and kc.max() > 1.0 and np.all(kc[:, :, 0] < 1e-2)  # convecting faces; the peripheral face decays towards 0
    return m, init, dt


@pytest.mark.parametrize("kind", ["explicit", "split", "implicit"])
def test_hydrostatic_model_steps_equal_the_composed_sequence(ocn, kind):
    """Five QAB2 steps, vertically implicit at diffusion number Δt κᶜᵃ / min Δz² = 20, on a stretched z with SeawaterBuoyancy, T and S, an
    FPlane, a wind stress and a cooling flux at the top, from a state whose upper half is unstable, with each of the three free surfaces
    (the split-explicit one with the filter): u, v, w, η, the tracers and the tendencies bit for bit (strict math); κᶜ, κᵘ and Ri (whole
    parent arrays) after every step, and κᶜ, κᵘ against the restatement's own running average."""
    kw = dict(horizontal_Ri_filter=ocn.FivePointHorizontalFilter()) if kind == "split" else {}
    m, init, _ = _run_model_against_twin(ocn, kind, "VerticallyImplicit", 20.0, **kw)
    assert m.field("T").interior()[:, :, 8:].std() < init["T"][:, :, 8:].std()  # the unstable half is being mixed


def test_hydrostatic_model_with_the_explicit_discretization_equals_the_composed_sequence(ocn):
    """the same with ExplicitTimeDiscretization at a stable step (diffusion number 0.2 of the clipped maximum): no implicit step, every
    vertical flux in the tendencies; the exponential taper"""
    _run_model_against_twin(ocn, "split", "Explicit", 0.2 * 1.7 / 5.0, Ri_dependent_tapering=ocn.ExponentialRiDependentTapering())


# ---- 3. conservation ----------------------------------------------------------------------------------------------------------------------------
def test_column_integrals_change_only_by_the_surface_flux(ocn):
    """A horizontally uniform state (no noise, so no horizontal flux and w = 0) under the cooling flux J_T and no salt flux: after five
    vertically implicit steps Σ Δz T of every column has changed by -J_T t and Σ Δz S not at all.  Allowance: per step 8 x the larger of
    (a) what ONE implicit step of the restatement (CAN.implicit_step_fields with the model's final κᶜ and Δt) is off by on the model's
    final T / S column, and (b) ε Σ Δz |c| (the AB2 update and the sum itself).  Measured on one MI355X: T changed by -2.070957e-05 as the flux
    says, error 1.8e-15 against the restatement's one-step defect 3.6e-15 and an allowance of 1.7e-13; S: error 0, allowance 3.1e-13."""
    pg = _model_grid(ocn)
    closure = ocn.RiBasedVerticalDiffusivity(warning=False, **PARAMETERS)
    m = _model(ocn, "implicit", closure, pg)
    g = IDN.describe(m.grid)
    init = _initial(pg, noise=0.0)
    m.set(**init)
    dt = 20.0 * _dzmin(g) ** 2 / closure.kappa_ca
    dz = g.dzc[g.Hz:g.Hz + g.Nz]
    before = {name: (dz * m.field(name).interior()[:, :, :12]).sum(axis=-1) for name in ("T", "S")}
    steps = 5
    for _ in range(steps):
        m.time_step(dt)
    ocn.sync_device()
    kappa = m.diffusivity_fields["kappa_c"].parent()
    assert np.abs(m.w.interior()).max() == 0.0
    for name, flux in (("T", T_FLUX), ("S", 0.0)):
        parent = m.field(name).parent()
        after = (dz * m.field(name).interior()[:, :, :12]).sum(axis=-1)
        stepped = CAN.implicit_step_fields(g, parent, CC, kappa, dt)
        sl = _interior(g)
        defect = np.abs((dz * stepped[sl]).sum(axis=-1) - (dz * parent[sl]).sum(axis=-1)).max()
        scale = (dz * np.abs(parent[sl])).sum(axis=-1).max()
        allowance = steps * 8 * max(defect, np.finfo(np.float64).eps * scale)
        error = np.abs((after - before[name]) - (-flux * steps * dt)).max()
        print(f"{name}: Σ Δz c changed by {(after - before[name]).mean():.6e}, flux {-flux * steps * dt:.6e}, error {error:.3e}, "
              f"restatement's one-step defect {defect:.3e}, allowance {allowance:.3e}")
        assert error <= allowance
    assert np.abs((dz * m.field("T").interior()[:, :, :12]).sum(axis=-1) - before["T"]).min() > 100 * allowance  # the flux is resolved


# ---- 4. checkpoint restart ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("td", ["VerticallyImplicit", "Explicit"])
def test_checkpoint_restart_is_bit_identical(ocn, tmp_path, td):
    """2 N steps equal N steps + write + restore into a fresh model + N steps, the time-averaged κᶜ and κᵘ included (N = 2)"""
    pg = _model_grid(ocn)
    make = lambda: _model(ocn, "split", ocn.RiBasedVerticalDiffusivity(td, warning=False, **PARAMETERS), pg)
    g = IDN.describe(pg)
    dt = (20.0 if td == "VerticallyImplicit" else 0.2 * 1.7 / 5.0) * _dzmin(g) ** 2 / 1.7
    a = make()
    a.set(**_initial(pg))
    for _ in range(2):
        a.time_step(dt)
    path = ocn.write_checkpoint(a, str(tmp_path / "ri_based"))
    with np.load(path if str(path).endswith(".npz") else str(path) + ".npz") as z:
        assert sum("diffusivity_fields" in k for k in z.files) == 2
    held = {name: a.diffusivity_fields[name].parent() for name in ("kappa_c", "kappa_u")}
    for _ in range(2):
        a.time_step(dt)
    b = make()
    ocn.set_from_checkpoint(b, path)
    for name in held:  # (not what update_state! makes of a fresh model's zeros)
        assert np.array_equal(b.diffusivity_fields[name].parent(), held[name]), name
    for _ in range(2):
        b.time_step(dt)
    ocn.sync_device()
    assert a.clock.iteration == b.clock.iteration == 4
    for name in ("u", "v", "w", "T", "S"):
        assert np.array_equal(a.field(name).parent(), b.field(name).parent()), name
    assert np.array_equal(a.eta.cpu().numpy(), b.eta.cpu().numpy())
    for name in ("kappa_c", "kappa_u", "Ri"):
        assert np.array_equal(a.diffusivity_fields[name].parent(), b.diffusivity_fields[name].parent()), name
    assert a.diffusivity_fields["kappa_c"].interior().max() > 1.0
    # a checkpoint without the κ fields cannot restart this closure
    plain = _model(ocn, "split", None, pg, fused=False)
    other = ocn.write_checkpoint(plain, str(tmp_path / "plain"))
    with np.load(other if str(other).endswith(".npz") else str(other) + ".npz") as z:
        assert not any("diffusivity_fields" in k for k in z.files)
    with pytest.raises(KeyError, match="kappa_c"):
        ocn.set_from_checkpoint(make(), other)


# ---- 5. the README snippet -----------------------------------------------------------------------------------------------------------------------
def test_readme_snippet_constructs_and_steps(ocn):
    grid = _model_grid(ocn)
    with pytest.warns(UserWarning, match="experimental"):
        closure = ocn.RiBasedVerticalDiffusivity(κᶜᵃ=1.7, Cᵉⁿ=0.1, horizontal_Ri_filter=ocn.FivePointHorizontalFilter())
    cooling = ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(1e-3))
    model = ocn.HydrostaticFreeSurfaceModel(grid, tracers=("T", "S"), buoyancy=ocn.SeawaterBuoyancy(), closure=closure,
                                            boundary_conditions={"T": cooling})
    model.set(T=lambda x, y, z: 20 - 2 * np.abs(z + 0.5) + 0 * x + 0 * y, S=35.0)
    model.time_step(1e-2)
    ocn.sync_device()
    kappa, Ri = model.diffusivity_fields["kappa_c"].interior()[:, :, :12], model.diffusivity_fields["Ri"].interior()[:, :, :12]
    assert kappa.max() > 1.0 and np.all(kappa[:, :, 0] == 0) and np.isinf(Ri).any() and (Ri == 0).any()
    for f in model._nh.prognostic_fields():
        assert np.isfinite(f.interior()).all()
    # the other buoyancy formulations construct and step too: b itself, and none
    for kw in (dict(tracers=("b",), buoyancy=ocn.BuoyancyTracer()), dict(tracers=("c",), buoyancy=None)):
        h = ocn.HydrostaticFreeSurfaceModel(grid, closure=ocn.RiBasedVerticalDiffusivity(warning=False), **kw)
        h.set(**{kw["tracers"][0]: lambda x, y, z: -np.abs(z + 0.5) + 0 * x + 0 * y})
        h.time_step(1e-2)
        ocn.sync_device()
        k = h.diffusivity_fields["kappa_c"].interior()[:, :, :12]
        assert np.isfinite(k).all() and (k.max() > 1.0) == (kw["buoyancy"] is not None)
