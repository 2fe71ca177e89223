"""LagrangianParticles: mirrors src/Models/LagrangianParticleTracking.

  LagrangianParticles(; x, y, z, restitution, dynamics, parameters)        LagrangianParticleTracking.jl:40-97
  update_lagrangian_particle_properties!(particles, model, Δt)             update_lagrangian_particle_properties.jl:17-36
  advect_lagrangian_particles!(particles, model, Δt)                       lagrangian_particle_advection.jl:196-206
  step_lagrangian_particles!(particles, model, Δt)                         LagrangianParticleTracking.jl:134-143

The reference keeps the particles in a StructArray (one vector per property); here `properties` is a dict of 1-D float64 device
vectors in the same order: x, y, z, then the custom properties.  Both kernels are csrc/particles.hip, one thread per particle; sampling
the tracked fields and moving the particles are ONE launch unless a `dynamics` callback has to run in between.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .architectures import child_architecture, device, on_architecture, stream_ptr
from .fields import Field
from .grids import Flat, require_regular_xy


def _ndim(a):
    return a.dim() if isinstance(a, torch.Tensor) else np.ndim(a)


def _shape(a):
    return tuple(a.shape) if isinstance(a, torch.Tensor) else np.shape(a)


def _julia_names(names):
    names = tuple(names)
    if len(names) == 1:
        return f"(:{names[0]},)"
    return "(" + ", ".join(f":{n}" for n in names) + ")"


class LagrangianParticles:
    """LagrangianParticles(x=, y=, z=, restitution=1.0, dynamics=None, parameters=None, tracked_fields=None, properties=None).

    x, y, z: 1-D arrays (numpy or tensors) of equal length, moved to the model's architecture when the model is built.
    tracked_fields: {property_name: field}; a field is the name of a model field ("u", "v", "w", a tracer) or an ocn.Field on the model's
    grid.  Every tracked name needs a vector in `properties` (the reference's custom particle type), a dict of extra 1-D arrays.
    dynamics(particles, model, Δt) is called between sampling the tracked fields and advecting; `parameters` is kept for it."""

    def __init__(self, x=None, y=None, z=None, restitution=1.0, dynamics=None, parameters=None, tracked_fields=None, properties=None):
        if x is None or y is None or z is None:
            raise TypeError("LagrangianParticles needs x, y and z")
        if not (_shape(x) == _shape(y) == _shape(z)):
            raise ValueError("x, y, z must all have the same size!")
        if not (_ndim(x) == 1 and _ndim(y) == 1 and _ndim(z) == 1):
            raise ValueError(f"x, y, z must have dimension 1 but ndims=({_ndim(x)}, {_ndim(y)}, {_ndim(z)})")
        props = {"x": x, "y": y, "z": z}
        for name, a in dict(properties or {}).items():
            if name in props:
                raise ValueError(f"property {name} is given twice")
            if _ndim(a) != 1 or _shape(a) != _shape(x):
                raise ValueError(f"particle property {name} must be a 1-D array of length {_shape(x)[0]}")
            props[name] = a
        tracked_fields = dict(tracked_fields or {})
        for name in tracked_fields:
            if name not in props:
                raise ValueError(f"{name} is a tracked field but Particle has no {name} field! "
                                 "You might have to define your own particle type.")
        if len(tracked_fields) > _lib.PARTICLES_MAX_TRACKED:
            raise NotImplementedError(f"at most {_lib.PARTICLES_MAX_TRACKED} tracked fields")
        for name, f in tracked_fields.items():
            if not isinstance(f, (str, Field)):
                raise TypeError(f"tracked field {name} must be the name of a model field or an ocn.Field")
        self.properties = {n: self._as_vector(a) for n, a in props.items()}
        self.restitution = float(restitution)
        self.tracked_fields = tracked_fields
        self.dynamics = dynamics
        self.parameters = parameters
        self._resolved = None  # {property name: Field} once a model has adopted the particles

    @staticmethod
    def _as_vector(a):
        if isinstance(a, torch.Tensor):
            return a.to(torch.float64).contiguous()
        return torch.from_numpy(np.array(a, dtype=np.float64, order="C"))

    def to_architecture(self, arch):
        """on_architecture(arch, particles): every property vector on the device"""
        dev = device(child_architecture(arch))
        for n, a in self.properties.items():
            if a.device != dev:
                self.properties[n] = on_architecture(arch, a)
        return self

    def __getattr__(self, name):  # particles.x, particles.u: the property vectors
        props = self.__dict__.get("properties")
        if props is not None and name in props:
            return props[name]
        raise AttributeError(name)

    def __len__(self):
        return int(self.properties["x"].shape[0])

    @property
    def size(self):
        return (len(self),)

    def summary(self):
        return f"{len(self)} LagrangianParticles with eltype Particle and properties {_julia_names(self.properties)}"

    def __repr__(self):
        dyn = "no_dynamics" if self.dynamics is None else getattr(self.dynamics, "__name__", repr(self.dynamics))
        return (f"{len(self)} LagrangianParticles with eltype Particle:\n"
                f"├── {len(self.properties)} properties: {_julia_names(self.properties)}\n"
                f"├── particle-wall restitution coefficient: {self.restitution}\n"
                f"├── {len(self.tracked_fields)} tracked fields: {_julia_names(self.tracked_fields) if self.tracked_fields else '()'}\n"
                f"└── dynamics: {dyn}")

    def resolve_tracked_fields(self, grid, model=None):
        """{property: Field}: names are looked up in the model; Fields must live on `grid` (same parent arrays as the model's own)"""
        out = {}
        for name, f in self.tracked_fields.items():
            if isinstance(f, str):
                if model is None:
                    raise ValueError(f"tracked field {name} = {f!r} names a model field: it needs a model")
                f = model.field(f)
            g = f.grid
            if (g.size, (g.Hx, g.Hy, g.Hz), tuple(g.topology)) != (grid.size, (grid.Hx, grid.Hy, grid.Hz), tuple(grid.topology)):
                raise ValueError(f"tracked field {name} lives on another grid than the particles are advected on "
                                 "(build it on model.grid: the model may have inflated the halo)")
            out[name] = f
        return out


def particle_geometry(grid):
    """struct ocn_particle_geometry of a grid (cached on it): the first Face and Center node and the right edge of every direction, and
    the interior z nodes of a stretched z as device vectors."""
    cached = grid.__dict__.get("_particle_geometry")
    if cached is not None:
        return cached[0]
    require_regular_xy(grid, "LagrangianParticles")
    c = _lib.CParticleGeometry()
    for d in range(3):
        if grid.topology[d] == Flat:
            continue
        c.face0[d] = float(grid.nodes_1d(d, True)[0])
        c.center0[d] = float(grid.nodes_1d(d, False)[0])
        c.right[d] = float(grid.domain(d)[1])
    keep = ()
    if grid.z_faces is not None and grid.architecture is not None:
        keep = tuple(on_architecture(grid.architecture, np.ascontiguousarray(grid.nodes_1d(2, face))) for face in (True, False))
        c.zf, c.zc = keep[0].data_ptr(), keep[1].data_ptr()
    grid.__dict__["_particle_geometry"] = (c, keep)
    return c


def _tracked_arrays(particles, grid, model):
    fields = particles._resolved if (model is not None and particles._resolved is not None) else particles.resolve_tracked_fields(grid, model)
    if not fields:
        return 0, None, None, None
    names = list(fields)
    return (len(names), _lib.ptr_array([fields[n].ptr for n in names]), _lib.i32_array([fields[n].loc for n in names]),
            _lib.ptr_array([particles.properties[n].data_ptr() for n in names]))


def _on_device(particles, grid):
    if grid.architecture is not None:
        particles.to_architecture(grid.architecture)
    return particles.properties["x"], particles.properties["y"], particles.properties["z"]


def update_lagrangian_particle_properties(particles, grid, model=None):
    """update_lagrangian_particle_properties!: every tracked field interpolated to the particle positions, into the property of its name"""
    x, y, z = _on_device(particles, grid)
    n, fields, locs, outs = _tracked_arrays(particles, grid, model)
    if n == 0 or len(particles) == 0:
        return
    _lib.call("ocn_sample_particle_properties", grid.cref, C.byref(particle_geometry(grid)), len(particles), x.data_ptr(), y.data_ptr(),
              z.data_ptr(), n, fields, locs, outs, stream_ptr())


def advect_lagrangian_particles(particles, grid, velocities, dt, model=None, update_properties=False):
    """advect_lagrangian_particles!(particles, model, Δt) with the velocities spelled out: (u, v, w) Fields on `grid` with filled halos.
    update_properties: the tracked fields are sampled at the positions before the move in the same launch."""
    x, y, z = _on_device(particles, grid)
    if len(particles) == 0:
        return
    u, v, w = velocities
    n, fields, locs, outs = _tracked_arrays(particles, grid, model) if update_properties else (0, None, None, None)
    _lib.call("ocn_advect_particles", grid.cref, C.byref(particle_geometry(grid)), len(particles), x.data_ptr(), y.data_ptr(), z.data_ptr(),
              float(particles.restitution), u.ptr, v.ptr, w.ptr, float(dt), n, fields, locs, outs, stream_ptr())


def step_lagrangian_particles(model, dt):
    """step_lagrangian_particles!(model, Δt): sample the tracked fields, dynamics(particles, model, Δt), advect with the model's velocities
    (total_velocities: a Stokes drift does not advect particles).  Without dynamics the three are one launch."""
    particles = model.particles
    if particles is None:
        return
    if particles.dynamics is None:
        advect_lagrangian_particles(particles, model.grid, model.velocities, dt, model=model, update_properties=True)
        return
    update_lagrangian_particle_properties(particles, model.grid, model)
    particles.dynamics(particles, model, dt)
    advect_lagrangian_particles(particles, model.grid, model.velocities, dt, model=model)
