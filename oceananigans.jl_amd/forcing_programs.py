"""Forcing functions of the model's fields, on the device: ContinuousForcing(func, parameters=, field_dependencies=).

Mirrors the reference's ContinuousForcing and MultipleForcings:
  ContinuousForcing, regularize_forcing, the call F.func(X..., t, deps..., [parameters])   src/Forcings/continuous_forcing.jl:109-142
  user_function_arguments                                                                   src/Utils/user_function_arguments.jl
  index_and_interp_dependencies, assumed_field_location                                     src/Operators/interpolation_utils.jl:55-112
  MultipleForcings: ((F1 + F2) + F3) + F4                                                   src/Forcings/multiple_forcings.jl:34-46

The reference compiles `func` into the tendency kernel.  The library is compiled ahead of time, so `func` is called HERE, once, at model
construction, with symbolic operands -- the node coordinates of the forced field's own location (boundary_functions.Coordinate), the time
(Time) and every dependency interpolated from its assumed location to that location (Dependency) -- and the tree it returns is lowered by
operations.Program to the straight-line program of include/ocn_hip.h (ocn_op_program).  ocn_op_accumulate adds the value of that program to
the tendency, as its last interior addend.  Nothing is traced or lowered again: the time is one OCN_OP_CONST that is patched before every
evaluation.

The device has no transcendental functions.  ocn.exp / log / tanh / sin / cos are accepted where the device never has to evaluate them: a
sub-tree that contains one, reads no field and at most ONE coordinate direction is evaluated by the host with NumPy -- into one patched
constant where it reads no coordinate (sin(ω t)), into a vector on that direction's nodes, halos included, which the program loads as it
loads a Coordinate (exp(z / λ), sin(k x - ω t)).  The LARGEST such sub-tree is folded.  A vector that reads the time is evaluated and
uploaded again when the time has changed since its last evaluation (N doubles); the others once.

If a field has a ContinuousForcing among the terms of its forcing, ALL its terms are lowered into the one program -- arrays and sampled
Forcing(func) as leaves in the field's parent layout, a Relaxation with the arithmetic of the sampled path, (rate * mask) * (target -
field) -- and that field's struct ocn_forcing is NULL.
"""
import ctypes as C

import numpy as np

from . import _lib
from .architectures import on_architecture, stream_ptr
from .boundary_functions import BoundaryProgram, Coordinate, Dependency, Time, validate_dependencies
from .fields import Field
from .forcings import (_DIRS, ContinuousForcing, GaussianMask, LinearTarget, Relaxation, _evaluate, _node_args, _vector, field_location,
                       interior_shape, is_steady)
from .grids import Bounded, Center, Face, Flat
from .operations import (HOST_FOLDED_UNARY, AbstractOperation, BinaryOperation, UnaryOperation, _is_fieldlike, _is_number, binary_operation,
                         julia_max, julia_min, reads)


def tendency_index_range(grid, loc):
    """(first, last) 0-based index of the cells a tendency is computed at, per direction: the interior without the faces on a wall --
    faces 2 .. N of the N + 1 along a Face & Bounded direction (periphery_offset, kernel_launching.jl:113-114), as ocn_op_accumulate runs"""
    out = []
    for d in range(3):
        N, topo = grid.size[d], grid.topology[d]
        if topo == Flat:
            out.append((0, 0))
        elif (loc >> d) & 1 and topo == Bounded:
            out.append((1 if N > 1 else 0, N - 1))
        else:
            out.append((0, N - 1))
    return tuple(out)


class Vector(AbstractOperation):
    """A leaf that reads a 1-D vector on the nodes of direction d at Face or Center, halos included -- to the program a field reduced along
    the two other directions, as a Coordinate is.  `tree`: the folded sub-tree it holds (None: fixed `values`, a mask or a target)."""

    def __init__(self, grid, d, face, values=None, tree=None, time_dependent=False, time=0.0):
        self.grid, self.d, self.face = grid, d, bool(face)
        self.reduced = 7 & ~(1 << d)
        self.location = tuple((Face if self.face else Center) if e == d else None for e in range(3))
        self.tree, self.time_dependent, self.time = tree, bool(time_dependent), float(time)
        self.values = np.ascontiguousarray(values, dtype=np.float64) if tree is None else self.evaluate(time)
        self._data = None

    def reads(self):
        return False, frozenset((self.d,)), self.time_dependent

    def evaluate(self, time):
        n = Coordinate(self.grid, self.d, self.face).nodes().size
        return np.array(np.broadcast_to(host_value(self.tree, time), (n,)), dtype=np.float64)

    def set_time(self, time):
        """the values at `time`; uploaded if the device copy exists and they were evaluated at another time"""
        if self.tree is None or not self.time_dependent or time == self.time:
            return
        self.values, self.time = self.evaluate(time), float(time)
        if self._data is not None:
            self._data.copy_(on_architecture(self.grid.architecture, self.values))

    @property
    def ptr(self):
        if self._data is None:
            self._data = on_architecture(self.grid.architecture, self.values)
        return self._data.data_ptr()


def host_value(node, time):
    """A sub-tree without fields and with at most one coordinate direction, evaluated with NumPy on that direction's nodes with halos"""
    with np.errstate(all="ignore"):
        return _host_value(node, time)


def _host_value(node, time):
    if _is_number(node):
        return np.float64(node)
    if isinstance(node, Coordinate):
        return node.nodes()
    if isinstance(node, Vector):
        return node.values
    if isinstance(node, Time):
        return np.float64(time)
    if isinstance(node, BinaryOperation):
        a, b = _host_value(node.a, time), _host_value(node.b, time)
        op = node.op
        return (a + b if op == "+" else a - b if op == "-" else a * b if op == "*" else a / b if op == "/" else julia_min(a, b) if op == "min"
                else julia_max(a, b))
    if isinstance(node, UnaryOperation):
        x, op = _host_value(node.arg, time), node.op
        if op in HOST_FOLDED_UNARY:
            return HOST_FOLDED_UNARY[op](x)
        return -x if op == "neg" else np.abs(x) if op == "abs" else np.sqrt(x) if op == "sqrt" else x * x if op == "sq" else (x * x) * x
    raise TypeError(f"cannot evaluate {type(node).__name__} on the host")


def _has_folded_function(node, seen):
    if not isinstance(node, (BinaryOperation, UnaryOperation)):
        return False
    q = seen.get(id(node))
    if q is None:
        if isinstance(node, UnaryOperation):
            q = node.op in HOST_FOLDED_UNARY or _has_folded_function(node.arg, seen)
        else:
            q = _has_folded_function(node.a, seen) or _has_folded_function(node.b, seen)
        seen[id(node)] = q
    return q


def _coordinate_leaf(node):
    """the Coordinate (or Vector) a foldable sub-tree reads: all of them are along one direction, at the forced field's own location"""
    if isinstance(node, (Coordinate, Vector)):
        return node
    if isinstance(node, BinaryOperation):
        a = _coordinate_leaf(node.a)  # (an operation has no truth value: no `or`)
        return a if a is not None else _coordinate_leaf(node.b)
    if isinstance(node, UnaryOperation):
        return _coordinate_leaf(node.arg)
    return None


class ForcingProgram(BoundaryProgram):
    """The program of one field's forcing: a BoundaryProgram (Coordinate, Time, Dependency leaves; the halo check over an index range)
    whose index space is that of a tendency (tendency_index_range), not a plane.  `time_index`: the instruction that holds the time, or
    None; `folded_constants`: [(instruction, sub-tree)] of the constants the host folds at every time; `folded_vectors`: the Vector leaves
    the host folded, steady and time-dependent."""

    def __init__(self, grid, loc, time=0.0):
        super().__init__(grid, loc, None, time)
        self.folded_constants, self.folded_vectors = [], []
        self._folded, self._has = {}, {}

    # -- lowering --
    def value(self, node, off):
        if isinstance(node, (BinaryOperation, UnaryOperation)) and _has_folded_function(node, self._has):
            field, dirs, _ = reads(node)
            if not field and len(dirs) <= 1:
                return self._fold(node, dirs, off)
        return super().value(node, off)

    def _unmerged_constant(self, value, **mark):
        """a CONST that is patched later (not through _emit: equal constants are merged there)"""
        self.instructions.append(dict(op=_lib.OP_CONST, a=-1, b=-1, field=-1, off=(0, 0, 0), value=float(value), reg=-1, **mark))
        return len(self.instructions) - 1

    def _fold(self, node, dirs, off):
        leaf = self._folded.get(id(node))
        if leaf is None:
            if not dirs:  # reads the time only (numbers alone are folded by Python as the function runs)
                leaf = self._folded[id(node)] = self._unmerged_constant(host_value(node, self.time), fold=node)
            else:
                c = _coordinate_leaf(node)
                leaf = self._folded[id(node)] = Vector(self.grid, c.d, c.face, tree=node, time_dependent=reads(node)[2], time=self.time)
        return leaf if isinstance(leaf, int) else self.load(leaf, off)

    def _lower(self, node, off):
        if isinstance(node, (Coordinate, Vector)):  # (with the offset: a vector read at a neighbour is refused, not read in place)
            return self.load(node, off)
        return super()._lower(node, off)

    def finish(self, result):
        super().finish(result)
        self.folded_constants = [(q, i["fold"]) for q, i in enumerate(self.instructions) if i.get("fold") is not None]
        self.folded_vectors = [f for f in self.fields if isinstance(f, Vector) and f.tree is not None]
        return self

    # -- the index space --
    def index_range(self):
        return tendency_index_range(self.grid, self.loc)

    # -- the time --
    def set_time(self, time):
        """the program at `time`: the time constant, the folded constants and the time-dependent folded vectors -- nothing else changes"""
        self.time = float(time)
        if self.time_index is not None:
            self.instructions[self.time_index]["value"] = self.time
        for q, tree in self.folded_constants:
            self.instructions[q]["value"] = float(host_value(tree, self.time))
        for v in self.folded_vectors:
            v.set_time(self.time)

    def patched_instructions(self):
        return ([] if self.time_index is None else [self.time_index]) + [q for q, _ in self.folded_constants]


def user_function_arguments(grid, loc, dependencies, parameters, model_fields):
    """X..., t, deps..., [parameters]: the node coordinates of the location (those of Flat directions left out), the time, the
    dependencies interpolated to the location, in the order given"""
    location = tuple(Face if (loc >> d) & 1 else Center for d in range(3))
    coordinates = [Coordinate(grid, d, (loc >> d) & 1) for d in range(3) if grid.topology[d] != Flat]
    deps = [Dependency(model_fields[n], location) for n in dependencies]
    return coordinates + [Time(grid)] + deps + ([] if parameters is None else [parameters])


def _traced(term, grid, loc, model_fields):
    validate_dependencies(term.field_dependencies, tuple(model_fields))
    result = term.func(*user_function_arguments(grid, loc, term.field_dependencies, term.parameters, model_fields))
    if _is_number(result):
        return float(result)
    if not _is_fieldlike(result):
        raise TypeError("a ContinuousForcing function must return a number or an expression of its arguments (+, -, *, /, ** 2, ** 3, ocn.sqrt, "
                        f"ocn.abs, ocn.minimum, ocn.maximum, and ocn.exp / log / tanh / sin / cos of the time or one coordinate), not "
                        f"{type(result).__name__}")
    return result


class SampledLeaf:
    """An array, a Forcing(func) or a function-valued mask / target of a Relaxation among the terms of a program: a field in the forced
    field's parent layout (zero halos) that the host samples -- again at every new time unless it is steady"""

    def __init__(self, grid, loc, sample, steady):
        self.grid, self.loc, self.sample, self.steady, self.time = grid, loc, sample, steady, 0.0
        self.field = Field(loc, grid).set(sample(0.0))

    def set_time(self, time):
        if not self.steady and time != self.time:
            self.field.set(self.sample(time))
            self.time = time


def _relaxation_tree(term, grid, loc, field, leaves):
    """(rate * mask) * (target - field) (relaxation.jl:95-101) with the operands of the sampled path: rate * 1.0 is rate, bit for bit"""
    shape = interior_shape(grid, loc)

    def operand(what, x, with_time):
        if isinstance(x, (GaussianMask, LinearTarget)):
            d = _DIRS[x.direction]
            return Vector(grid, d, (loc >> d) & 1, values=_vector(grid, loc, d, x))
        if isinstance(x, np.ndarray):
            sample, steady = (lambda t: x), True
        else:
            args = _node_args(grid, loc)
            sample, steady = (lambda t: _evaluate(x, args + ([t] if with_time else []), shape)), (term.steady or not with_time)
        leaves.append(SampledLeaf(grid, loc, sample, steady))
        return leaves[-1].field
    m, g = term.mask, term.target
    factor = term.rate if m is None else binary_operation("*", term.rate, operand("mask", m, False))
    target = 0.0 if g is None else g if isinstance(g, float) else operand("target", g, True)
    return binary_operation("*", factor, binary_operation("-", target, field))


def lower_forcing(terms, grid, name, model_fields, time=0.0):
    """(ForcingProgram, [SampledLeaf]) of ALL the terms of one field's forcing, summed left to right"""
    loc = field_location(name)
    shape, leaves, total = interior_shape(grid, loc), [], None
    for term in terms:
        if isinstance(term, ContinuousForcing):
            v = _traced(term, grid, loc, model_fields)
        elif isinstance(term, Relaxation):
            v = _relaxation_tree(term, grid, loc, model_fields[name], leaves)
        else:
            if isinstance(term, np.ndarray):
                sample, steady = (lambda t, a=term: a), True
            else:  # Forcing(func): sampled by the host, as on the path without programs
                args, tail = _node_args(grid, loc), ([] if term.parameters is None else [term.parameters])
                sample, steady = (lambda t, f=term.func, a=args, p=tail: _evaluate(f, a + [t] + p, shape)), is_steady(term)
            leaves.append(SampledLeaf(grid, loc, sample, steady))
            v = leaves[-1].field
        if total is None:
            total = v
        elif _is_number(total) and _is_number(v):
            total = total + v
        else:
            total = binary_operation("+", total, v)
    p = ForcingProgram(grid, loc, time)
    return p.finish(p.const(total) if _is_number(total) else p.value(total, (0, 0, 0))), leaves


class ProgramForcing:
    """The forcing program of one field bound to its model: the program, its host struct and the leaves the host samples.
    accumulate(G, time) enqueues ONE kernel on the current stream (plus the uploads of what depends on the time and is not traced)."""

    def __init__(self, terms, grid, name, model_fields, time=0.0):
        self.grid, self.name = grid, name
        self.program, self.leaves = lower_forcing(terms, grid, name, model_fields, time)
        self._c = self.program.c_struct()

    def accumulate(self, G, time):
        c, p = self._c, self.program
        p.set_time(time)
        for leaf in self.leaves:
            leaf.set_time(time)
        for q, f in enumerate(p.fields):  # (a model may exchange the buffers of its fields between steps)
            c.fields[q] = f.ptr
        for q in p.patched_instructions():
            c.ins[q].value = p.instructions[q]["value"]
        _lib.call("ocn_op_accumulate", self.grid.cref, C.byref(c), G.ptr, stream_ptr())
