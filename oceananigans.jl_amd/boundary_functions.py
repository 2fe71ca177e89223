"""Flux boundary conditions that are functions of the model's fields: FluxBoundaryCondition(func, field_dependencies=..., parameters=...).

Mirrors the reference's ContinuousBoundaryFunction with field dependencies:
  regularize_boundary_condition, getbc, domain_boundary_indices   src/BoundaryConditions/continuous_boundary_function.jl:60-157
  user_function_arguments                                          src/Utils/user_function_arguments.jl
  interpolation_operator, assumed_field_location                   src/Operators/interpolation_utils.jl:55-112

The reference compiles `func` into the kernel that applies the condition.  The library is compiled ahead of time, so `func` is called
HERE, once, at model construction, with symbolic operands -- the tangential coordinates, the time and every dependency interpolated to the
boundary location -- and the tree it returns is lowered by operations.Program to the straight-line program of include/ocn_hip.h
(ocn_op_program).  ocn_op_compute_boundary evaluates that program on the boundary plane into the device array the flux kernels read for an
array-valued condition; the host samples nothing and no field is copied.  The time is one OCN_OP_CONST instruction whose value is patched
in the host struct before every evaluation: nothing is traced or lowered again.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .architectures import child_architecture, device, on_architecture, stream_ptr
from .grids import Center, Face, Flat
from .operations import AbstractOperation, Program, _is_fieldlike, _is_number

SIDES = ("west", "east", "south", "north", "bottom", "top")
# the two directions tangential to a side, in the order ocn_bc.values is indexed (physics.BoundaryCondition._TANGENTIAL)
TANGENTIAL = {"west": (1, 2), "east": (1, 2), "south": (0, 2), "north": (0, 2), "bottom": (0, 1), "top": (0, 1)}


def normal_direction(side):
    return SIDES.index(side) >> 1


def boundary_normal_index(grid, side):
    """I of domain_boundary_indices (continuous_boundary_function.jl:94-95), 1-based: 1 on west / south / bottom, N on east / north / top"""
    return grid.size[normal_direction(side)] if SIDES.index(side) & 1 else 1


def boundary_location(loc, side):
    """(LX, LY, LZ) of the conditioned field with the boundary-normal location set to None (the reference's Nothing)"""
    dn = normal_direction(side)
    return tuple(None if d == dn else (Face if (loc >> d) & 1 else Center) for d in range(3))


class Coordinate(AbstractOperation):
    """ξnode / ηnode / rnode along direction d at Face or Center: a leaf that reads a 1-D vector of nodes, halos included -- to the
    program a field reduced along the two other directions (ocn_op_program.field_reduced), so one LOAD broadcasts it over the plane."""

    def __init__(self, grid, d, face):
        self.grid, self.d, self.face = grid, d, bool(face)
        self.reduced = 7 & ~(1 << d)
        self.location = tuple((Face if self.face else Center) if e == d else None for e in range(3))  # (.loc: the mask of it)
        self._data = None

    def reads(self):
        return False, frozenset((self.d,)), False

    def nodes(self):
        return np.ascontiguousarray(self.grid.nodes_1d(self.d, self.face, with_halos=True), dtype=np.float64)

    @property
    def ptr(self):
        if self._data is None:
            self._data = on_architecture(self.grid.architecture, self.nodes())
        return self._data.data_ptr()


class Time(AbstractOperation):
    """clock.time: lowered to ONE OCN_OP_CONST that is never merged with another constant, so its value can be patched"""
    location = (None, None, None)

    def __init__(self, grid):
        self.grid = grid

    def reads(self):
        return False, frozenset(), True


class Dependency(AbstractOperation):
    """ℑ(i, j, I, grid, field): a model field interpolated to the boundary location -- along the tangential directions only, the normal
    location being None there -- by the operator interpolation_operator(assumed_field_location(name), (LX, LY, LZ)) selects (the
    velocities and tracers of a model ARE at their assumed locations)"""

    def __init__(self, field, location):
        self.field, self.grid, self.location = field, field.grid, tuple(location)


class BoundaryProgram(Program):
    """The program of a boundary function: its index space is the boundary plane -- N points along each tangential direction (the extents
    of ocn_bc.values) and the one index I along the normal.  `time_index`: the instruction that holds the time, or None.
    (forcing_programs.ForcingProgram is this class over another index_range: the cells of a tendency.)"""

    def __init__(self, grid, loc, side, time=0.0):
        super().__init__(grid, loc)
        self.side, self.time = side, float(time)
        self._time = None
        self.time_index = None

    def _lower(self, node, off):
        if isinstance(node, Coordinate):
            return self.load(node, (0, 0, 0))
        if isinstance(node, Time):
            if self._time is None:  # (not through _emit: equal constants are merged there)
                self._time = len(self.instructions)
                self.instructions.append(dict(op=_lib.OP_CONST, a=-1, b=-1, field=-1, off=(0, 0, 0), value=self.time, reg=-1, time=True))
            return self._time
        if isinstance(node, Dependency):
            return self.interpolated(node.field, node.field.location, node.location, off)
        return super()._lower(node, off)

    def finish(self, result):
        super().finish(result)
        marked = [q for q, i in enumerate(self.instructions) if i.get("time")]
        self.time_index = marked[0] if marked else None
        return self

    def index_range(self):
        """(first, last) 0-based index the program runs over, per direction"""
        g, dn = self.grid, normal_direction(self.side)
        I = boundary_normal_index(g, self.side) - 1
        return tuple((I, I) if d == dn else (0, g.size[d] - 1) for d in range(3))

    def interior_size(self, loc=None):
        return tuple(hi - lo + 1 for lo, hi in self.index_range())

    def _check_halos(self):
        """every point of the index range (the PLANE), shifted, lies in the parent array of the field it reads (the check the library repeats)"""
        g = self.grid
        H, rng = (g.Hx, g.Hy, g.Hz), self.index_range()
        for i in self.loads:
            f = self.fields[i["field"]]
            reduced = getattr(f, "reduced", 0)
            ext = g.parent_shape(f.loc)
            for d in range(3):
                if (reduced >> d) & 1:
                    continue
                if H[d] + rng[d][0] + i["off"][d] < 0 or H[d] + rng[d][1] + i["off"][d] > ext[d] - 1:
                    raise ValueError(f"the traced function reads {i['off'][d]:+d} cells along {'xyz'[d]}: further than the grid's halo ({H[d]}) holds")
        for i in self.instructions:
            if i["op"] == _lib.OP_SPACING and i["field"] >= _lib.SPACING_DZC and g._dzc_host is not None:
                dk = i["off"][2]
                if H[2] + rng[2][0] + dk < 0 or H[2] + rng[2][1] + dk > g.Nz + 2 * H[2] - 1:
                    raise ValueError(f"the traced function reads the z spacing {dk:+d} cells away: further than the grid's halo ({H[2]})")


def validate_dependencies(field_dependencies, model_field_names):
    """index_and_interp_dependencies (interpolation_utils.jl:99-109), with its wording"""
    if any(n not in model_field_names for n in field_dependencies):
        raise ValueError(f"{tuple(field_dependencies)} are required to be model fields but only {tuple(model_field_names)} are present")


def trace(bc, grid, loc, side, model_fields, time=0.0):
    """The BoundaryProgram of `bc` (a flux condition with field_dependencies) on `side` of a field at `loc`: bc.func is called once as
    func(ξ, η, t, *dependencies[, parameters]) -- ξ, η the coordinates tangential to the side at the field's own location (x, y on
    bottom / top; y, z on west / east; x, z on south / north; those of Flat directions left out), as getbc calls it.
    model_fields: {name: Field} of the velocities and tracers.  Pure Python: no device is touched."""
    validate_dependencies(bc.field_dependencies, tuple(model_fields))
    location = boundary_location(loc, side)
    coordinates = [Coordinate(grid, d, (loc >> d) & 1) for d in TANGENTIAL[side] if grid.topology[d] != Flat]
    dependencies = [Dependency(model_fields[n], location) for n in bc.field_dependencies]
    args = coordinates + [Time(grid)] + dependencies + ([] if bc.parameters is None else [bc.parameters])
    result = bc.func(*args)
    p = BoundaryProgram(grid, loc, side, time)
    if _is_number(result):
        return p.finish(p.const(result))
    if not _is_fieldlike(result):
        raise TypeError(f"a boundary function with field_dependencies must return a number or an expression of its arguments (+, -, *, /, "
                        f"** 2, ** 3, ocn.sqrt, ocn.abs), not {type(result).__name__}")
    return p.finish(p.value(result, (0, 0, 0)))


class BoundaryFunction:
    """A traced condition bound to its model: the program, its host struct and the device array of the values (bc._device_values, which
    struct ocn_bc.values points to).  compute(time) enqueues ONE kernel on the current stream."""

    def __init__(self, bc, grid, loc, side, model_fields, time=0.0):
        self.bc, self.grid, self.side = bc, grid, side
        self.program = trace(bc, grid, loc, side, model_fields, time)  # (refuses before anything is allocated)
        n1, n2 = bc._extents(grid, side)
        bc._device_values = torch.zeros((n2, n1), dtype=torch.float64, device=device(child_architecture(grid.architecture)))
        self._c = self.program.c_struct()

    def compute(self, time):
        c, p = self._c, self.program
        for q, f in enumerate(p.fields):  # (a model may exchange the buffers of its fields between steps)
            c.fields[q] = f.ptr
        if p.time_index is not None:
            c.ins[p.time_index].value = float(time)
        _lib.call("ocn_op_compute_boundary", self.grid.cref, C.byref(c), SIDES.index(self.side), self.bc._device_values.data_ptr(), stream_ptr())
