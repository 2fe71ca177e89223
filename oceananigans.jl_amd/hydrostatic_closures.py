"""Everything HydrostaticFreeSurfaceModel knows about its closure (src/TurbulenceClosures/closure_tuples.jl: a closure answers
compute_diffusivities!, the flux divergences, implicit_step! and required_halo_size, and a tuple is the sum of its members).

`resolve_closure` turns the user's closure into ONE object, or refuses; it allocates nothing and touches no device.  The model asks that
object: at construction `container_closure` (what ocn_model_terms carries: an explicit ScalarDiffusivity or None), `halo`, `unfused` and
`allocate(nh)` (the diffusivity_fields dict, or None) and `boundary_conditions(user_bcs, grid)` (the conditions the fields are built with); in
update_state `compute_diffusivities(nh)`; in compute_tendencies `tracer_kappa(name)` and `advecting_velocities(nh)` (u, v, w, plus the eddy
velocities of IsopycnalSkewSymmetricDiffusivity) for the built-in tracer entry point and `add_fluxes(nh, Gn, s)` after those entry points; in time_step `self_stepped` (the tracers that ab2_step, implicit_step and
cache_previous_tendencies leave to the closure) and `implicit_step(nh, fields, dt, s)` after ocn_ab2_step; checkpoints read `state_fields`,
`checkpoint_state(nh)` and call `restore_state(nh, get)`.  Every kind but InModelTerms keeps the closure out of ocn_model_terms and runs the
reference's launch sequence (fused = False) with QAB2 on one GPU."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .architectures import stream_ptr
from .fields import CenterField, XFaceField, YFaceField, ZFaceField, fill_halo_regions
from .models import implicit_diffusion_step
from .physics import (BuoyancyTracer, CATKEVerticalDiffusivity, FieldBoundaryConditions, FluxBoundaryCondition, IsopycnalSkewSymmetricDiffusivity,
                      RiBasedVerticalDiffusivity, ScalarBiharmonicDiffusivity, SeawaterBuoyancy, TKEDissipationVerticalDiffusivity,
                      has_diffusivity_fields, is_vertically_implicit, owns_eddy_fields)


def _refuse(what, fused, split_rk3, slabs):
    if fused:
        raise NotImplementedError(f"{what} runs the reference's launch sequence (fused = False)")
    if split_rk3:
        raise NotImplementedError(f"{what} with SplitRungeKutta3 is not implemented")
    if slabs:
        raise NotImplementedError(f"{what} on a slab-partitioned (Distributed) grid is not implemented")


def resolve_closure(closure, fused, split_rk3, partitioned, distributed, buoyancy, boundary_conditions, tracers=()):
    """closure: a closure, a two-element tuple or list, or None; partitioned: the architecture has a `partition`; distributed: it also
    communicates (a slab-x rank)."""
    biharmonic = None
    if isinstance(closure, np.ndarray):
        raise NotImplementedError("arrays of closures (ensembles) are not implemented: give one closure")
    if isinstance(closure, (tuple, list)):  # (closure_tuples.jl) the biharmonic with a closure that has κ fields, in either order
        biharmonic = [c for c in closure if isinstance(c, ScalarBiharmonicDiffusivity)]
        vertical = [c for c in closure if has_diffusivity_fields(c) or isinstance(c, IsopycnalSkewSymmetricDiffusivity)]
        if len(closure) != 2 or len(biharmonic) != 1 or len(vertical) != 1:
            raise NotImplementedError("closure tuples are not implemented, except (HorizontalScalarBiharmonicDiffusivity, "
                                      "ConvectiveAdjustmentVerticalDiffusivity, RiBasedVerticalDiffusivity or CATKEVerticalDiffusivity) in either order, "
                                      "and the same pair with TKEDissipationVerticalDiffusivity: give one closure")
        biharmonic, closure = biharmonic[0], vertical[0]
    elif isinstance(closure, ScalarBiharmonicDiffusivity):
        biharmonic, closure = closure, None
    if biharmonic is not None:  # (SplitRungeKutta3 is fine: the term has no state)
        _refuse("ScalarBiharmonicDiffusivity", fused, False, partitioned)
        fused = False
    if owns_eddy_fields(closure):
        raise NotImplementedError("eddy-viscosity closures are not part of this slice")
    other = None
    if isinstance(closure, IsopycnalSkewSymmetricDiffusivity):
        _refuse("IsopycnalSkewSymmetricDiffusivity", fused, split_rk3, partitioned)
        for kappa in (closure.kappa_symmetric, closure.kappa_skew):  # tracer_diffusivities (with_tracers, :76-86)
            for name in tuple(tracers) if isinstance(kappa, dict) else ():
                if name not in kappa:
                    raise ValueError(f"no diffusivity κ given for tracer {name}")
        other = IsopycnalFields(closure)
    elif has_diffusivity_fields(closure):
        _refuse(type(closure).__name__, fused, split_rk3, partitioned)
        carriers = None
        if isinstance(closure, CATKEVerticalDiffusivity):
            if "e" not in tuple(tracers):  # with_tracers (catke_vertical_diffusivity.jl:122-128)
                raise ValueError(closure.MISSING_TRACER)
        if isinstance(closure, TKEDissipationVerticalDiffusivity):  # with_tracers (tke_dissipation_vertical_diffusivity.jl:131-137)
            if "e" not in tuple(tracers) or closure.dissipation_name(tracers) is None:
                raise ValueError(closure.MISSING_TRACER)
        stress_driven = isinstance(closure, (CATKEVerticalDiffusivity, TKEDissipationVerticalDiffusivity))
        if isinstance(closure, (RiBasedVerticalDiffusivity, CATKEVerticalDiffusivity, TKEDissipationVerticalDiffusivity)):
            # top_buoyancy_flux reads the top condition of the buoyancy tracers as a flux; the reference would read the number of a Value or
            # Gradient condition as one too, which is not reproduced
            carriers = ("b", None) if isinstance(buoyancy, BuoyancyTracer) else (("T", "S") if isinstance(buoyancy, SeawaterBuoyancy) else (None, None))
            name = type(closure).__name__
            for tracer in filter(None, carriers):
                top = getattr((boundary_conditions or {}).get(tracer), "sides", {}).get("top")
                if top is not None and top.kind != _lib.BC_FLUX:
                    raise NotImplementedError(f"{name}: the top boundary condition of {tracer} must be a "
                                              "FluxBoundaryCondition (or the default): it is the surface buoyancy flux of the entrainment term")
            for velocity in ("u", "v") if stress_driven else ():
                top = getattr((boundary_conditions or {}).get(velocity), "sides", {}).get("top")
                if top is not None and top.kind != _lib.BC_FLUX:
                    raise NotImplementedError(f"{name}: the top boundary condition of {velocity} must be a "
                                              "FluxBoundaryCondition (or the default): it is the wind stress of the friction velocity")
        if isinstance(closure, TKEDissipationVerticalDiffusivity):
            other = TKEDissipationFields(closure, carriers, closure.dissipation_name(tracers))
        else:
            other = CATKEFields(closure, carriers) if isinstance(closure, CATKEVerticalDiffusivity) else KappaFields(closure, carriers)
    elif is_vertically_implicit(closure):
        _refuse("a VerticallyImplicitTimeDiscretization closure", fused, split_rk3, distributed)
        if partitioned:
            raise NotImplementedError("a VerticallyImplicitTimeDiscretization closure on a Distributed architecture is not implemented (see DESIGN.md)")
        return ImplicitScalar(closure)
    if biharmonic is not None:
        return Biharmonic(biharmonic, other)
    return other or InModelTerms(closure)


class InModelTerms:
    """no closure, or an explicit ScalarDiffusivity: its term lives in ocn_model_terms, everything else is a no-op"""
    halo, unfused, implicit, state_fields, self_stepped = 0, False, False, (), ()

    def __init__(self, closure):
        self.container_closure = closure

    def boundary_conditions(self, user_bcs, grid):
        """add_closure_specific_boundary_conditions: what the fields are built with"""
        return user_bcs

    def allocate(self, nh):
        return None

    def checkpoint_state(self, nh):
        """what a restart needs beyond the prognostic fields, the tendencies and `state_fields`: {name: host array}"""
        return {}

    def restore_state(self, nh, get):
        """after the update_state! of set!(model, filepath); get(name): the array of checkpoint_state, or None"""

    def compute_diffusivities(self, nh):
        pass

    def tracer_kappa(self, name):
        return 0.0 if self.container_closure is None else self.container_closure.kappa_of(name)

    def add_fluxes(self, nh, Gn, s):
        pass

    def implicit_step(self, nh, fields, dt, s):
        pass

    def advecting_velocities(self, nh):
        """pointers to the velocities that advect the tracers (div_Uc): u, v, w, plus the eddy velocities of a closure that has some"""
        return nh.u.ptr, nh.v.ptr, nh.w.ptr


class ImplicitScalar(InModelTerms):
    """hydrostatic_free_surface_ab2_step.jl:39-108: implicit_step! of u, v and every tracer after its ab2 step; w is diagnostic"""
    container_closure, unfused, implicit = None, True, True

    def __init__(self, closure):
        self.closure = closure

    def add_fluxes(self, nh, Gn, s):
        """the explicit part of the closure term (Gu, Gv and the tracers)"""
        nt, cl = len(nh.tracers), self.closure
        _lib.call("ocn_add_vertically_implicit_explicit_fluxes", nh.grid.cref, cl.nu, nh.u.ptr, nh.v.ptr, nh.w.ptr, Gn[0].ptr, Gn[1].ptr, None,
                  nt, (C.c_double * max(nt, 1))(*[cl.kappa_of(n) for n in nh.tracer_names]),
                  _lib.ptr_array([c.ptr for c in nh.tracers] or [None]), _lib.ptr_array([G.ptr for G in Gn[3:]] or [None]), None, s)

    def implicit_step(self, nh, fields, dt, s):
        """u, v (ν) and every tracer (its own κ) with the full Δt"""
        implicit_diffusion_step(nh.grid, fields, [self.closure.nu] * 2 + [self.closure.kappa_of(n) for n in nh.tracer_names], dt, s)


def top_condition(nh, field):
    """a reference to the struct ocn_bc of the top condition of a field, NULL where there is none (no field, default conditions: no flux)"""
    b = getattr(field, "boundary_conditions", None)
    return C.pointer(b.c_struct(nh.grid).top) if b is not None and b.sides["top"] is not None else C.POINTER(_lib.CBc)()


class KappaFields(InModelTerms):
    """ConvectiveAdjustmentVerticalDiffusivity or RiBasedVerticalDiffusivity, in both discretizations: κᶜ, κᵘ fields computed in update_state!
    (csrc/vertical_diffusivity.hip, csrc/ri_based_diffusivity.hip).  carriers: None, or for the Ri-based one -- which differs in how the
    fields are computed and in their being state -- the tracers whose top conditions make up the surface buoyancy flux: (T or b, S)"""
    container_closure, unfused = None, True

    def __init__(self, closure, carriers):
        self.closure, self.carriers, self.implicit = closure, carriers, is_vertically_implicit(closure)
        self.state_fields = () if carriers is None else ("kappa_c", "kappa_u")  # time averages (the reference does not checkpoint them)

    def allocate(self, nh):
        """build_diffusivity_fields (convective_adjustment_vertical_diffusivity.jl:85, ri_based_vertical_diffusivity.jl:186-191): κᶜ and κᵘ
        (and Ri), ZFaceFields with default conditions, and the multipliers of the three distinct matrices of the implicit step (u, v,
        every tracer)"""
        g = nh.grid
        self.fields = {"kappa_c": ZFaceField(g), "kappa_u": ZFaceField(g)}
        if self.carriers is not None:
            self.fields["Ri"] = ZFaceField(g)
        self.struct = self.closure.c_struct()
        if self.implicit:
            self.ivd_scratch = torch.zeros((3, g.Nz, g.Ny, g.Nx), dtype=torch.float64, device=nh.u.data.device)
        return self.fields

    def top_conditions(self, nh):
        """top_condition of the carriers (NULL for a carrier that is no tracer of the model)"""
        return tuple(top_condition(nh, nh.field(name) if name in nh.tracer_names else None) for name in self.carriers or ())

    def compute_diffusivities(self, nh):
        """compute_diffusivities!, then fill_halo_regions!(diffusivity_fields; only_local_halos = true).  RiBasedVerticalDiffusivity
        (ri_based_vertical_diffusivity.jl:193-229), after update_boundary_conditions, so the `values` arrays of function-valued flux
        conditions are current: compute_ri_number!, the halo fill of Ri, compute_ri_based_diffusivities! -- or, without a horizontal
        filter, where Ri is only read at its own cell, all of it in one launch (bit-identical).  Every call advances the time average."""
        g, d, s = nh.grid, self.fields, stream_ptr()
        nh._refresh_term_pointers()
        terms, cl = C.byref(nh._terms), C.byref(self.struct)
        tops = self.top_conditions(nh)
        if self.carriers is None:
            _lib.call("ocn_compute_convective_adjustment_diffusivities", g.cref, terms, cl, d["kappa_c"].ptr, d["kappa_u"].ptr, s)
        elif self.closure.horizontal_Ri_filter is None:
            _lib.call("ocn_compute_ri_based_diffusivities_fused", g.cref, terms, cl, *tops, nh.u.ptr, nh.v.ptr, d["Ri"].ptr,
                      d["kappa_c"].ptr, d["kappa_u"].ptr, s)
        else:
            _lib.call("ocn_compute_ri_number", g.cref, terms, nh.u.ptr, nh.v.ptr, d["Ri"].ptr, s)
            fill_halo_regions((d["Ri"],), fill_boundary_normal_velocities=False)
            _lib.call("ocn_compute_ri_based_diffusivities", g.cref, terms, cl, *tops, d["Ri"].ptr, d["kappa_c"].ptr, d["kappa_u"].ptr, s)
        fill_halo_regions(tuple(d.values()), fill_boundary_normal_velocities=False)  # (ZFaceFields that are no velocities)

    def kappa_of_tracer(self, name):
        """diffusivity(closure, diffusivity_fields, Val(id)): the κ array of a tracer"""
        return self.fields["kappa_c"].ptr

    def add_to(self, g, u, v, Gu, Gv, nt, c, G, s, kappas=None):
        """G -= ∂ⱼτ: every vertical flux (explicit), or the fluxes through the two boundaries (vertically implicit).  Pointers; u = None:
        no momentum; c, G: lists, or None for a launch without tracer arrays; kappas: the κ arrays of the tracers (default: κᶜ for all)"""
        d, pa = self.fields, _lib.ptr_array
        _lib.call("ocn_add_vertical_diffusivity_fluxes", g.cref, u and d["kappa_u"].ptr, u, v, Gu, Gv, nt,
                  c and pa(kappas or [d["kappa_c"].ptr] * len(c)), c and pa(c), G and pa(G), int(self.implicit), None, s)

    def add_fluxes(self, nh, Gn, s):
        self.add_to(nh.grid, nh.u.ptr, nh.v.ptr, Gn[0].ptr, Gn[1].ptr, len(nh.tracers), [c.ptr for c in nh.tracers] or [None],
                    [G.ptr for G in Gn[3:]] or [None], s, kappas=[self.kappa_of_tracer(n) for n in nh.tracer_names] or None)

    def implicit_step(self, nh, fields, dt, s):
        """implicit_step! with the κ fields of the last update_state! (the reference does not recompute them)"""
        if not self.implicit:
            return
        d, w, nt = self.fields, self.ivd_scratch, len(fields) - 2
        kappas = [d["kappa_u"].ptr] * 2 + [d["kappa_c"].ptr] * nt
        scratch = [w[0].data_ptr(), w[1].data_ptr()] + [w[2].data_ptr()] * nt
        _lib.call("ocn_implicit_vertical_diffusion_step_fields", nh.grid.cref, len(fields), _lib.ptr_array([f.ptr for f in fields]),
                  _lib.i32_array([f.loc for f in fields]), _lib.ptr_array(kappas), _lib.ptr_array(scratch), float(dt), s)


class TKEBasedFields(KappaFields):
    """What CATKEVerticalDiffusivity and TKEDissipationVerticalDiffusivity share (TKEBasedVerticalDiffusivities.jl): the closure steps the
    tracers `self_stepped` itself, inside compute_diffusivities!, in substeps of one launch each; their tendencies are the ordinary tracer
    tendencies; ab2_step, the implicit step of the other fields (KappaFields.implicit_step: both closures are always vertically implicit)
    and cache_previous_tendencies leave them alone.  Their top conditions are the closure's own
    (add_closure_specific_boundary_conditions): array-valued fluxes, `tops`, that the closure's kernel writes.  A subclass gives `name`,
    `self_stepped` (and `state_keys`, what its tracers are called in a checkpoint) and `diffusivity_fields`."""
    name, state_keys = None, {"e": "e"}

    def __init__(self, closure, carriers):
        super().__init__(closure, carriers)
        self.state_fields = ()  # (everything goes through checkpoint_state / restore_state)

    def boundary_conditions(self, user_bcs, grid):
        """the top conditions of the self-stepped tracers are replaced, as in the reference; the user's other sides are kept (the
        reference's branch for user conditions on ϵ copies the sides of e's, a slip: here ϵ keeps its own)"""
        bcs = dict(user_bcs or {})
        self.tops = {}
        for name in self.self_stepped:
            sides = dict(bcs[name].sides) if bcs.get(name) is not None else {}
            self.tops[name] = sides["top"] = FluxBoundaryCondition(np.zeros((grid.Nx, grid.Ny)))
            bcs[name] = FieldBoundaryConditions(**{k: v for k, v in sides.items() if v is not None})
        return bcs

    def allocate(self, nh):
        g, dev = nh.grid, nh.u.data.device
        self.fields = self.diffusivity_fields(g, dev)
        self.u_prev, self.v_prev = XFaceField(g), YFaceField(g)
        self.struct = self.closure.c_struct()
        # the multipliers of u, v, the other tracers, and of every self-stepped tracer (those last, contiguous)
        self.ivd_scratch = torch.zeros((3 + len(self.self_stepped), g.Nz, g.Ny, g.Nx), dtype=torch.float64, device=dev)
        for top in self.tops.values():
            top.c_struct(g, "top")  # (allocates the device array of the condition)
        return self.fields

    def refresh_previous_velocities(self, nh):
        self.u_prev.data.copy_(nh.u.data)
        self.v_prev.data.copy_(nh.v.data)

    def _tendencies(self, nh, name):
        q = 3 + nh.tracer_names.index(name)
        return nh.timestepper._Gn[q], nh.timestepper._Gm[q]

    @staticmethod
    def substeps(nh, tau):
        """(Δτ, χ) of every substep of a model step (time_step_catke_equation.jl:12-76, tke_dissipation_equations.jl:24-88): an Euler step
        opens several substeps; otherwise the time stepper's χ, which is -1/2 during an Euler step of the model"""
        Dt = nh.clock.last_dt
        M = 1 if tau is None else math.ceil(Dt / tau)
        dtau = Dt if tau is None else Dt / M
        return [(dtau, -0.5 if (m == 1 and M != 1) else nh.timestepper.chi) for m in range(1, M + 1)]

    def _state(self, nh):
        """{name in a checkpoint: the device tensor}: everything a bit-identical restart needs"""
        out = {name: getattr(f, "data", f) for name, f in self.fields.items()}
        out.update(u_prev=self.u_prev.data, v_prev=self.v_prev.data)
        for name, key in self.state_keys.items():
            out["top_" + key], out[key] = self.tops[name]._device_values, nh.field(name).data
            out["Gm_" + key] = self._tendencies(nh, name)[1].data
        return out

    def checkpoint_state(self, nh):
        return {name: np.ascontiguousarray(t.cpu().numpy().T) for name, t in self._state(nh).items()}

    def restore_state(self, nh, get):
        """the update_state! of set!(model, filepath) has stepped the closure's tracers once more: put back what the checkpointed
        tendencies were computed with, so that the restart continues bit for bit"""
        for name, t in self._state(nh).items():
            a = get(name)
            if a is None:
                raise KeyError(f"Field {name} of {self.name} does not exist in checkpoint and could not be restored.")
            t.copy_(torch.from_numpy(np.ascontiguousarray(np.asarray(a).T)))


class CATKEFields(TKEBasedFields):
    """CATKEVerticalDiffusivity (csrc/catke.hip): κᵘ, κᶜ, κᵉ, the linear coefficient Le, the averaged surface buoyancy flux Jᵇ and the previous
    velocities (build_diffusivity_fields, catke_vertical_diffusivity.jl:180-208).  The closure steps e in M substeps of
    substep_turbulent_kinetic_energy! + implicit_step! (:219-251, hydrostatic_free_surface_ab2_step.jl:72-108,
    cache_hydrostatic_free_surface_tendencies.jl:30-57); ocn_compute_catke_top_tke_flux writes e's top flux (catke_equation.jl:126-155)."""
    name, self_stepped = "CATKEVerticalDiffusivity", ("e",)
    top_e = property(lambda self: self.tops["e"])

    @staticmethod
    def diffusivity_fields(g, dev):
        return {"kappa_u": ZFaceField(g), "kappa_c": ZFaceField(g), "kappa_e": ZFaceField(g), "Le": CenterField(g),
                "Jb": torch.zeros((g.Ny, g.Nx), dtype=torch.float64, device=dev)}

    def allocate(self, nh):
        g = nh.grid
        self.previous_compute_time = nh.clock.time
        self.znodes = [torch.from_numpy(np.ascontiguousarray(g.nodes_1d(2, face), dtype=np.float64)).to(nh.u.data.device) for face in (True, False)]
        return super().allocate(nh)

    def kappa_of_tracer(self, name):
        return self.fields["kappa_e" if name == "e" else "kappa_c"].ptr

    def _e_tendencies(self, nh):
        return self._tendencies(nh, "e")

    def time_step_tke(self, nh, s):
        """time_step_catke_equation! (time_step_catke_equation.jl:12-76)"""
        g, d, zf, zc = nh.grid, self.fields, *self.znodes
        Gn, Gm = self._e_tendencies(nh)
        for dtau, chi in self.substeps(nh, self.closure.tke_time_step):
            _lib.call("ocn_catke_substep_tke", g.cref, C.byref(nh._terms), C.byref(self.struct), zf.data_ptr(), zc.data_ptr(), nh.u.ptr, nh.v.ptr,
                      self.u_prev.ptr, self.v_prev.ptr, nh.field("e").ptr, d["Jb"].data_ptr(), d["kappa_u"].ptr, d["kappa_c"].ptr,
                      d["kappa_e"].ptr, d["Le"].ptr, Gn.ptr, Gm.ptr, self.ivd_scratch[3].data_ptr(), float(dtau), float(chi), 1, s)

    def compute_diffusivities(self, nh):
        g, d, s, zf, zc = nh.grid, self.fields, stream_ptr(), *self.znodes
        nh._refresh_term_pointers()
        terms, cl = C.byref(nh._terms), C.byref(self.struct)
        dt = nh.clock.time - self.previous_compute_time  # update_previous_compute_time!
        self.previous_compute_time = nh.clock.time
        if math.isfinite(nh.clock.last_dt):  # the model has taken a step
            self.time_step_tke(nh, s)
        self.refresh_previous_velocities(nh)
        tops, e = self.top_conditions(nh), nh.field("e")
        _lib.call("ocn_compute_catke_surface_buoyancy_flux", g.cref, terms, cl, *tops, zf.data_ptr(), zc.data_ptr(), nh.u.ptr, nh.v.ptr, e.ptr,
                  d["Jb"].data_ptr(), float(dt), s)
        _lib.call("ocn_compute_catke_diffusivities", g.cref, terms, cl, zf.data_ptr(), zc.data_ptr(), nh.u.ptr, nh.v.ptr, e.ptr,
                  d["Jb"].data_ptr(), d["kappa_u"].ptr, d["kappa_c"].ptr, d["kappa_e"].ptr, s)
        fill_halo_regions((d["kappa_u"], d["kappa_c"], d["kappa_e"]), fill_boundary_normal_velocities=False)
        # the top flux of e, for the compute_boundary_tendency_contributions! of this state
        _lib.call("ocn_compute_catke_top_tke_flux", g.cref, terms, cl, top_condition(nh, nh.u), top_condition(nh, nh.v), *tops, nh.u.ptr,
                  nh.v.ptr, self.top_e._device_values.data_ptr(), s)

    def checkpoint_state(self, nh):
        return dict(super().checkpoint_state(nh), previous_compute_time=np.float64(self.previous_compute_time))

    def restore_state(self, nh, get):
        """... and Jᵇ has been averaged once more"""
        super().restore_state(nh, get)
        self.previous_compute_time = float(get("previous_compute_time"))


class TKEDissipationFields(TKEBasedFields):
    """TKEDissipationVerticalDiffusivity (csrc/tke_dissipation.hip): κᵘ, κᶜ, κᵉ, κᵋ, the linear coefficients Le, Lϵ and the previous velocities
    (build_diffusivity_fields, tke_dissipation_vertical_diffusivity.jl:184-223).  The closure steps e and ϵ in M substeps of
    substep_tke_dissipation! + the implicit_step! of e + that of ϵ (:228-256); their slow tendencies carry κᵉ / κᵋ;
    ocn_compute_tke_dissipation_top_fluxes writes their top fluxes (tke_dissipation_equations.jl:258-303).  `eps`: the name the user gave
    the dissipation tracer."""
    name = "TKEDissipationVerticalDiffusivity"

    def __init__(self, closure, carriers, eps):
        super().__init__(closure, carriers)
        self.eps, self.self_stepped, self.state_keys = eps, ("e", eps), {"e": "e", eps: "eps"}

    @staticmethod
    def diffusivity_fields(g, dev):
        return {"kappa_u": ZFaceField(g), "kappa_c": ZFaceField(g), "kappa_e": ZFaceField(g), "kappa_eps": ZFaceField(g),
                "Le": CenterField(g), "Leps": CenterField(g)}

    def allocate(self, nh):
        self.zc = torch.from_numpy(np.ascontiguousarray(nh.grid.nodes_1d(2, False), dtype=np.float64)).to(nh.u.data.device)
        return super().allocate(nh)

    def kappa_of_tracer(self, name):
        return self.fields["kappa_e" if name == "e" else ("kappa_eps" if name == self.eps else "kappa_c")].ptr

    def time_step_tke_dissipation(self, nh, s):
        """time_step_tke_dissipation_equations! (tke_dissipation_equations.jl:24-88)"""
        g, d = nh.grid, self.fields
        (Gn_e, Gm_e), (Gn_eps, Gm_eps) = self._tendencies(nh, "e"), self._tendencies(nh, self.eps)
        for dtau, chi in self.substeps(nh, self.closure.tke_dissipation_time_step):
            _lib.call("ocn_tke_dissipation_substep", g.cref, C.byref(nh._terms), C.byref(self.struct), nh.u.ptr, nh.v.ptr, self.u_prev.ptr,
                      self.v_prev.ptr, nh.field("e").ptr, nh.field(self.eps).ptr, d["kappa_u"].ptr, d["kappa_c"].ptr, d["kappa_e"].ptr,
                      d["kappa_eps"].ptr, d["Le"].ptr, d["Leps"].ptr, Gn_e.ptr, Gm_e.ptr, Gn_eps.ptr, Gm_eps.ptr, self.ivd_scratch[3].data_ptr(),
                      float(dtau), float(chi), 1, s)

    def compute_diffusivities(self, nh):
        g, d, s = nh.grid, self.fields, stream_ptr()
        nh._refresh_term_pointers()
        terms, cl = C.byref(nh._terms), C.byref(self.struct)
        if math.isfinite(nh.clock.last_dt):  # the model has taken a step
            self.time_step_tke_dissipation(nh, s)
        self.refresh_previous_velocities(nh)
        e, eps = nh.field("e"), nh.field(self.eps)
        kappas = [d[name] for name in ("kappa_u", "kappa_c", "kappa_e", "kappa_eps")]
        _lib.call("ocn_compute_tke_dissipation_diffusivities", g.cref, terms, cl, nh.u.ptr, nh.v.ptr, e.ptr, eps.ptr, *[k.ptr for k in kappas], s)
        # (the reference's fill_halo_regions!(::TKEDissipationDiffusivityFields) names an undefined variable: what it evidently means)
        fill_halo_regions(tuple(kappas), fill_boundary_normal_velocities=False)
        # the top fluxes of e and ϵ, for the compute_boundary_tendency_contributions! of this state
        _lib.call("ocn_compute_tke_dissipation_top_fluxes", g.cref, cl, top_condition(nh, nh.u), top_condition(nh, nh.v), self.zc.data_ptr(),
                  nh.u.ptr, nh.v.ptr, e.ptr, self.tops["e"]._device_values.data_ptr(), self.tops[self.eps]._device_values.data_ptr(), s)


class IsopycnalFields(InModelTerms):
    """IsopycnalSkewSymmetricDiffusivity (csrc/isopycnal.hip): the tapered ϵ_R₃₃ at (Center, Center, Face) and, with skew advection, the eddy
    velocities u, v, w (build_diffusivity_fields, isopycnal_skew_symmetric_diffusivity.jl:102-116), computed in update_state! in one launch with
    the κz = ϵ_R₃₃ κ_symmetric arrays of the implicit step, one per distinct κ_symmetric.  The tracers are advected by u + uₑ, v + vₑ, w + wₑ
    (SumOfArrays, hydrostatic_free_surface_tendency_kernel_functions.jl), materialized after the halo fill; momentum keeps u, v, w and has no
    term (the closure has no viscosity).  Nothing is state: every field is recomputed from the tracers."""
    container_closure, unfused = None, True

    def __init__(self, closure):
        self.closure, self.halo = closure, closure.required_halo_size
        self.eddy = closure.advective and closure.kappa_skew is not None          # (:110-113)
        self.no_diffusion = closure.advective and closure.kappa_symmetric is None  # NoDiffusionISSD: the three fluxes are zero (:215-217)
        self.implicit = closure.kappa_symmetric is not None

    def allocate(self, nh):
        g, cl = nh.grid, self.closure
        self.fields = {"eps_R33": ZFaceField(g)}
        if self.eddy:
            self.fields.update(u=XFaceField(g), v=YFaceField(g), w=ZFaceField(g))
            self.total = (XFaceField(g), YFaceField(g), ZFaceField(g))
        self.struct, self._terms = cl.c_struct(), nh._terms
        # κz of the implicit step: one array and one set of multipliers per distinct κ_symmetric
        self.kz = {}
        for name in nh.tracer_names if self.implicit else ():
            self.kz.setdefault(cl.kappa_symmetric_of(name), ZFaceField(g))
        if len(self.kz) > _lib.MODEL_MAX_TRACERS:
            raise NotImplementedError(f"IsopycnalSkewSymmetricDiffusivity: more than {_lib.MODEL_MAX_TRACERS} distinct κ_symmetric")
        if self.kz:
            self.ivd_scratch = torch.zeros((len(self.kz), g.Nz, g.Ny, g.Nx), dtype=torch.float64, device=nh.u.data.device)
        return self.fields

    def compute_diffusivities(self, nh):
        """compute_diffusivities! (:118-132), then fill_halo_regions!(diffusivity_fields; only_local_halos = true): ϵ_R₃₃ has no condition
        in z; uₑ, vₑ take the no-flux mirror; wₑ's Impenetrable condition (0 on faces 1 and Nz + 1) is written by the kernel"""
        g, d, s, pa = nh.grid, self.fields, stream_ptr(), _lib.ptr_array
        nh._refresh_term_pointers()
        eddy = [d[n].ptr for n in "uvw"] if self.eddy else [None] * 3
        ks = list(self.kz)
        _lib.call("ocn_compute_isopycnal_diffusivities", g.cref, C.byref(nh._terms), C.byref(self.struct),
                  self.closure.kappa_skew if self.eddy else 0.0, d["eps_R33"].ptr, *eddy, len(ks), (C.c_double * len(ks))(*ks) if ks else None,
                  pa([self.kz[k].ptr for k in ks]) if ks else None, s)
        fill_halo_regions(tuple(d.values()), fill_boundary_normal_velocities=False)
        if self.eddy:
            _lib.call("ocn_sum_velocities", g.cref, pa([nh.u.ptr, nh.v.ptr, nh.w.ptr]), pa(eddy), pa([f.ptr for f in self.total]), s)

    def advecting_velocities(self, nh):
        return tuple(f.ptr for f in self.total) if self.eddy else (nh.u.ptr, nh.v.ptr, nh.w.ptr)

    def kappa_of_tracer(self, name):
        """(κ_symmetric, κ_skew) of a tracer as the diffusive fluxes take them"""
        return self.closure.kappa_symmetric_of(name), self.closure.kappa_skew_of(name)

    def add_to(self, g, u, v, Gu, Gv, nt, c, G, s, kappas=None):
        """G -= ∇·q of the tracers (pointers; c, G: lists; kappas: kappa_of_tracer of each); no momentum term.  The arguments of
        KappaFields.add_to, so that the pair with the biharmonic closure calls both alike"""
        if not nt or self.no_diffusion:
            return
        M = _lib.MODEL_MAX_TRACERS
        for q in range(0, nt, M):
            n = min(M, nt - q)
            ks, kw = zip(*kappas[q:q + n])
            _lib.call("ocn_add_isopycnal_fluxes", g.cref, C.byref(self._terms), C.byref(self.struct), n, (C.c_double * n)(*ks), (C.c_double * n)(*kw),
                      _lib.ptr_array(c[q:q + n]), _lib.ptr_array(G[q:q + n]), s)

    def add_fluxes(self, nh, Gn, s):
        self.add_to(nh.grid, None, None, None, None, len(nh.tracers), [c.ptr for c in nh.tracers], [G.ptr for G in Gn[3:]], s,
                    kappas=[self.kappa_of_tracer(n) for n in nh.tracer_names])

    def implicit_step(self, nh, fields, dt, s):
        """implicit_step! of the tracers with κz = ϵ_R₃₃ κ_symmetric (:327-332) of the last update_state!; u and v are not stepped"""
        tracers = fields[2:]
        if not self.implicit or not tracers:
            return
        ks = list(self.kz)
        index = [ks.index(self.closure.kappa_symmetric_of(n)) for n in nh.tracer_names]
        _lib.call("ocn_implicit_vertical_diffusion_step_fields", nh.grid.cref, len(tracers), _lib.ptr_array([f.ptr for f in tracers]),
                  _lib.i32_array([f.loc for f in tracers]), _lib.ptr_array([self.kz[ks[q]].ptr for q in index]),
                  _lib.ptr_array([self.ivd_scratch[q].data_ptr() for q in index]), float(dt), s)


class Biharmonic(InModelTerms):
    """G -= ∂ⱼτ of HorizontalScalarBiharmonicDiffusivity -- or, in a pair with a closure V that has κ fields, G -= (∂ⱼτ + ∂ⱼτ(V)), the sum
    formed before it is subtracted (closure_tuples.jl:41-43): V's kernel leaves 0 - ∂ⱼτ(V) in a zeroed array, which the biharmonic kernel
    adds to its own term.  Two such arrays: u and v first, then tracer by tracer.  Everything else of a pair is V's."""
    container_closure, unfused = None, True

    def __init__(self, closure, other):
        self.closure, self.other, self.halo = closure, other, max(closure.required_halo_size, getattr(other, "halo", 0))
        if other is not None:
            self.implicit, self.state_fields, self.self_stepped = other.implicit, other.state_fields, other.self_stepped
            self.compute_diffusivities, self.implicit_step = other.compute_diffusivities, other.implicit_step
            self.boundary_conditions, self.checkpoint_state, self.restore_state = other.boundary_conditions, other.checkpoint_state, other.restore_state
            self.advecting_velocities = other.advecting_velocities

    def allocate(self, nh):
        if self.other is None:
            return None
        fields = self.other.allocate(nh)
        self.scratch = torch.zeros((2,) + tuple(nh.u.data.shape), dtype=torch.float64, device=nh.u.data.device)
        return fields

    @staticmethod
    def add_to(g, nu, u, v, Gu, Gv, nt, kappa, c, G, neg_u, neg_v, neg_c, s):
        """pointers; u = None: no momentum; kappa, c, G: lists, or None for a launch without tracer arrays; neg_*: minus the other closure's
        term, or None"""
        pa = _lib.ptr_array
        _lib.call("ocn_add_biharmonic_fluxes", g.cref, nu, u, v, Gu, Gv, nt, kappa and (C.c_double * len(kappa))(*kappa), c and pa(c), G and pa(G),
                  neg_u, neg_v, neg_c and pa(neg_c), s)

    def add_fluxes(self, nh, Gn, s):
        g, bih, V = nh.grid, self.closure, self.other
        u, v, Gu, Gv = nh.u.ptr, nh.v.ptr, Gn[0].ptr, Gn[1].ptr
        kappa, cs, Gs = [bih.kappa_of(n) for n in nh.tracer_names], [c.ptr for c in nh.tracers], [G.ptr for G in Gn[3:]]
        if V is None:
            return self.add_to(g, bih.nu, u, v, Gu, Gv, len(cs), kappa or [0.0], cs or [None], Gs or [None], None, None, None, s)
        S = self.scratch
        Su, Sv = S[0].data_ptr(), S[1].data_ptr()
        S.zero_()
        V.add_to(g, u, v, Su, Sv, 0, None, None, s)
        self.add_to(g, bih.nu, u, v, Gu, Gv, 0, None, None, None, Su, Sv, None, s)
        for name, k, c, G in zip(nh.tracer_names, kappa, cs, Gs):
            S[0].zero_()
            V.add_to(g, None, None, None, None, 1, [c], [Su], s, kappas=[V.kappa_of_tracer(name)])
            self.add_to(g, 0.0, None, None, None, None, 1, [k], [c], [G], None, None, [Su], s)
