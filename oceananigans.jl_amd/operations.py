"""On-device diagnostics: AbstractOperations, ComputedField, Average and Integral.

Mirrors src/AbstractOperations of the reference: arithmetic on fields builds a tree (binary_operations.jl, unary_operations.jl,
derivatives.jl, at.jl), `ComputedField(tree).compute()` is `compute!(Field(tree))` (computed_field.jl:65-75) and `Average` / `Integral`
are the metric reductions of metric_field_reductions.jl:11-113.  ASCII names stand for the reference's `∂x`, `∂y`, `∂z` and `@at`.

The reference compiles one fused kernel per tree.  The library is compiled ahead of time, so the tree is lowered HERE, in pure Python, to
a straight-line program in static single assignment form (include/ocn_hip.h: ocn_op_program) which one kernel of csrc/diagnostics.hip
evaluates per cell, with the reduction fused in.  A derivative or an interpolation of a sub-tree evaluates that sub-tree at two shifted
index offsets, so the lowering pushes offsets down to the leaves; equal instructions are merged and a linear scan assigns registers.
"""
import ctypes as C
import numbers
import struct
from fractions import Fraction

import numpy as np

from . import _lib
from .architectures import stream_ptr, zeros
from .fields import Field, fill_halo_regions
from .grids import Bounded, Center, Face, Flat, require_regular_xy

_MODEL_LOCATIONS = (_lib.LOC_CCC, _lib.LOC_FCC, _lib.LOC_CFC, _lib.LOC_CCF)
_OPCODE = {"+": _lib.OP_ADD, "-": _lib.OP_SUB, "*": _lib.OP_MUL, "/": _lib.OP_DIV, "neg": _lib.OP_NEG, "abs": _lib.OP_ABS, "sqrt": _lib.OP_SQRT,
           "min": _lib.OP_MIN, "max": _lib.OP_MAX}
_REFUSED_UNARY = ("log10", "tan", "sinh", "cosh", "asin", "acos", "atan")
# transcendentals the device never evaluates: accepted where the host can fold them (forcing_programs.py), each with its NumPy function
HOST_FOLDED_UNARY = {"exp": np.exp, "log": np.log, "tanh": np.tanh, "sin": np.sin, "cos": np.cos}


def location_of(mask, reduced=0):
    """(LX, LY, LZ) of a location bitmask; None (the reference's Nothing) along reduced directions"""
    return tuple(None if (reduced >> d) & 1 else (Face if (mask >> d) & 1 else Center) for d in range(3))


def location_mask(location):
    return sum(1 << d for d in range(3) if location[d] is Face)


def _is_number(x):
    return isinstance(x, (numbers.Real, np.number)) and not isinstance(x, bool)


def _is_fieldlike(x):
    return isinstance(x, (Field, AbstractOperation))


def _location(x):
    return x.location if _is_fieldlike(x) else (None, None, None)


class AbstractOperation:
    """A node of an operation tree: `grid`, `location`, and arithmetic that builds larger trees."""

    def __array_ufunc__(self, ufunc, method, *inputs, **kwargs):
        """np.exp(z), np.maximum(P, 0), np.float64(2) * operation: the NumPy ufuncs that have a node build that node, so a function body
        written with `np.` traces unchanged; anything else is refused by NumPy (TypeError)"""
        build = _UFUNC_NODES.get(ufunc.__name__)
        if method != "__call__" or kwargs or build is None or not all(_is_fieldlike(x) or _is_number(x) for x in inputs):
            return NotImplemented
        return build(*inputs)

    def reads(self):
        """(reads a field, the coordinate directions read, reads the time): what decides whether the host can fold a sub-tree.  A node
        that does not say is taken to read a field."""
        return True, frozenset(), False

    @property
    def loc(self):
        return location_mask(self.location)

    def __add__(self, o): return binary_operation("+", self, o)
    def __radd__(self, o): return binary_operation("+", o, self)
    def __sub__(self, o): return binary_operation("-", self, o)
    def __rsub__(self, o): return binary_operation("-", o, self)
    def __mul__(self, o): return binary_operation("*", self, o)
    def __rmul__(self, o): return binary_operation("*", o, self)
    def __truediv__(self, o): return binary_operation("/", self, o)
    def __rtruediv__(self, o): return binary_operation("/", o, self)
    def __neg__(self): return unary_operation("neg", self)
    def __pow__(self, n): return power(self, n)

    def _no_branch(self, *other):
        raise TypeError("an operation has no truth value and no order: it is a tree that is evaluated on the device, cell by cell.  A function "
                        "that is traced with symbolic operands (a boundary function with field_dependencies, a ContinuousForcing) cannot "
                        "branch on them: write the branch with ocn.minimum / ocn.maximum")

    __bool__ = __lt__ = __le__ = __gt__ = __ge__ = _no_branch


def _validate_grid(*operands):
    """validate_grid (grid_validation.jl): the one grid of all field-like operands"""
    grids = [x.grid for x in operands if _is_fieldlike(x)]
    if not grids:
        raise TypeError("an operation needs at least one field or operation among its operands")
    for g in grids[1:]:
        if g is not grids[0]:
            raise ValueError("the operands of an operation live on different grids")
    return grids[0]


def _choose_location(la, lb, lc):
    """choose_location (binary_operations.jl:47-52) along one direction"""
    if la is not None and la is lb:
        return la
    if la is not None and lb is None:
        return la
    if la is None and lb is not None:
        return lb
    return lc


class BinaryOperation(AbstractOperation):
    """op(▶a(a), ▶b(b)) at `location`: both operands are interpolated there, numbers never are"""

    def __init__(self, op, a, b, location, grid):
        self.op, self.a, self.b, self.location, self.grid = op, a, b, tuple(location), grid

    def reads(self):
        (fa, da, ta), (fb, db, tb) = reads(self.a), reads(self.b)
        return fa or fb, da | db, ta or tb


class UnaryOperation(AbstractOperation):
    """▶(op(arg)): op at the argument's location, interpolated to `location`; `sq` and `cube` are x*x and (x*x)*x"""

    def __init__(self, op, arg, location, grid):
        self.op, self.arg, self.location, self.grid = op, arg, tuple(location), grid

    def reads(self):
        return reads(self.arg)


class Derivative(AbstractOperation):
    """▶(∂(arg)): the difference quotient at the argument's location flipped along `dim`, interpolated to `location`"""

    def __init__(self, dim, arg, location, grid):
        la = list(arg.location)
        if la[dim] is None:
            raise ValueError(f"a derivative along {'xyz'[dim]} of an operand that was reduced along {'xyz'[dim]}")
        la[dim] = Center if la[dim] is Face else Face
        self.derivative_location = tuple(la)
        self.dim, self.arg, self.grid = dim, arg, grid
        self.location = self.derivative_location if location is None else tuple(location)


def binary_operation(op, a, b, location=None):
    """`op(Lc, a, b)` of binary_operations.jl:104-130; Lc defaults to the location of the first field-like operand"""
    if op not in ("+", "-", "*", "/", "min", "max"):
        raise NotImplementedError(f"binary operator {op!r}")
    for x in (a, b):
        if not (_is_fieldlike(x) or _is_number(x)):
            if callable(x):
                raise NotImplementedError("functions of (x, y, z) as operands (FunctionField / KernelFunctionOperation) are not implemented")
            raise TypeError(f"cannot combine a field with {type(x).__name__}")
    grid = _validate_grid(a, b)
    la, lb = _location(a), _location(b)
    lc = location if location is not None else (la if _is_fieldlike(a) else lb)
    return BinaryOperation(op, a, b, tuple(_choose_location(la[d], lb[d], lc[d]) for d in range(3)), grid)


def unary_operation(op, a, location=None):
    if not _is_fieldlike(a):
        raise TypeError(f"{op} of {type(a).__name__}: not a field or an operation")
    return UnaryOperation(op, a, a.location if location is None else location, a.grid)


def power(a, n):
    if _is_number(n) and n == 2:
        return unary_operation("sq", a)
    if _is_number(n) and n == 3:
        return unary_operation("cube", a)
    raise NotImplementedError(f"exponent {n!r}: only ** 2 and ** 3 (evaluated as x*x and x*x*x) are implemented; use sqrt for ** 0.5")


def sqrt(a):
    """sqrt of a number, of a field / an operation (a tree node) or of a NumPy array (np.sqrt: one function body then serves the device
    and a NumPy check of it)"""
    if isinstance(a, np.ndarray):
        return np.sqrt(a)
    return float(np.sqrt(a)) if _is_number(a) else unary_operation("sqrt", a)


def abs(a):  # noqa: A001 (mirrors the reference's Base.abs on fields)
    if isinstance(a, np.ndarray):
        return np.abs(a)
    return float(np.abs(a)) if _is_number(a) else unary_operation("abs", a)


def reads(x):
    """(reads a field, the coordinate directions read, reads the time) of a number, a field or an operation"""
    if _is_number(x):
        return False, frozenset(), False
    return x.reads() if isinstance(x, AbstractOperation) else (True, frozenset(), False)


def _refused_unary(name):
    def f(a):
        raise NotImplementedError(f"{name} of a field: only sqrt and abs (and unary minus, ** 2, ** 3, minimum, maximum) are implemented "
                                  "on the device")
    f.__name__ = name
    return f


log10, tan, sinh, cosh, asin, acos, atan = (_refused_unary(n) for n in _REFUSED_UNARY)


def _host_folded_unary(name):
    fn = HOST_FOLDED_UNARY[name]

    def f(a):
        if isinstance(a, np.ndarray):
            return fn(a)
        if _is_number(a):
            return float(fn(a))
        if not _is_fieldlike(a):
            raise TypeError(f"{name} of {type(a).__name__}: not a number, an array, a field or an operation")
        field, dirs, _ = reads(a)
        if field or len(dirs) > 1:
            raise NotImplementedError(f"{name} of an operand that varies cell by cell (it reads {'a field' if field else 'two coordinate directions'}"
                                      "): only sqrt and abs (and unary minus, ** 2, ** 3, minimum, maximum) are implemented on the device.  "
                                      f"{name} is accepted where the host can evaluate it once per time: of the time, of numbers and of ONE "
                                      "coordinate direction, in a ContinuousForcing")
        return unary_operation(name, a)
    f.__name__ = name
    f.__doc__ = f"{name} of a number or a NumPy array (np.{name}), or of a sub-tree the host folds (no field, at most one coordinate direction)"
    return f


exp, log, tanh, sin, cos = (_host_folded_unary(n) for n in HOST_FOLDED_UNARY)


def julia_max(a, b):
    """Julia's max on NumPy operands, with the selects of the device (csrc/diagnostics.hip): a NaN in either operand propagates and
    max(-0.0, +0.0) = +0.0 in either operand order (np.maximum gives the first of two equal operands)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    r = np.where(a > b, a, b)
    r = np.where(a == b, np.where(np.signbit(a), b, a), r)
    return np.where(a != a, a, r)


def julia_min(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    r = np.where(a < b, a, b)
    r = np.where(a == b, np.where(np.signbit(a), a, b), r)
    return np.where(a != a, a, r)


def _min_max(op, fn, a, b):
    if _is_fieldlike(a) or _is_fieldlike(b):
        return binary_operation(op, a, b)
    with np.errstate(invalid="ignore"):
        r = fn(a, b)
    return float(r) if r.ndim == 0 else r


def minimum(a, b):
    """min(a, b) with Julia's semantics (OCN_OP_MIN) of fields / operations, numbers or NumPy arrays"""
    return _min_max("min", julia_min, a, b)


def maximum(a, b):
    """max(a, b) with Julia's semantics (OCN_OP_MAX) of fields / operations, numbers or NumPy arrays"""
    return _min_max("max", julia_max, a, b)


_UFUNC_NODES = {"add": lambda a, b: binary_operation("+", a, b), "subtract": lambda a, b: binary_operation("-", a, b),
                "multiply": lambda a, b: binary_operation("*", a, b), "divide": lambda a, b: binary_operation("/", a, b),
                "negative": lambda a: unary_operation("neg", a), "square": lambda a: power(a, 2), "power": lambda a, n: power(a, n),
                "exp": exp, "log": log, "tanh": tanh, "sin": sin, "cos": cos, "sqrt": sqrt, "absolute": abs, "minimum": minimum,
                "maximum": maximum}


def _derivative(dim, a, location=None):
    if not _is_fieldlike(a):
        raise TypeError(f"dd{'xyz'[dim]} of {type(a).__name__}: not a field or an operation")
    return Derivative(dim, a, location, a.grid)


def ddx(a):
    """∂x(a) (derivatives.jl:47-107): lives at the location of `a` flipped along x"""
    return _derivative(0, a)


def ddy(a):
    return _derivative(1, a)


def ddz(a):
    return _derivative(2, a)


def at(location, op):
    """@at location op (at.jl; binary_operations.jl:32, unary_operations.jl:37, derivatives.jl:39): rebuild the tree at `location`"""
    location = tuple(location)
    if len(location) != 3 or any(l not in (Center, Face, None) for l in location):
        raise ValueError("a location is a 3-tuple of Center / Face")
    if isinstance(op, BinaryOperation):
        return binary_operation(op.op, at(location, op.a), at(location, op.b), location)
    if isinstance(op, UnaryOperation):
        return unary_operation(op.op, at(location, op.arg), location)
    if isinstance(op, Derivative):
        return _derivative(op.dim, op.arg, location)
    return op  # fields and numbers stay where they are


def KernelFunctionOperation(*args, **kwargs):
    raise NotImplementedError("KernelFunctionOperation: the library is compiled ahead of time and takes no kernel functions")


def CumulativeIntegral(*args, **kwargs):
    raise NotImplementedError("CumulativeIntegral is not implemented")


# ---- reductions ---------------------------------------------------------------------------------------------------------------------
def _tupleit_dims(dims):
    if dims is None:
        return (1, 2, 3)
    dims = (dims,) if _is_number(dims) else tuple(dims)
    if not dims or any(d not in (1, 2, 3) for d in dims) or len(set(dims)) != len(dims):
        raise ValueError(f"dims = {dims}: an int or a tuple out of (1, 2, 3)")
    return tuple(sorted(int(d) for d in dims))


class Reduction:
    """Average / Integral of `operand` over `dims` (Scan of metric_field_reductions.jl); computed by ComputedField"""

    def __init__(self, kind, operand, dims, condition, mask):
        if condition is not None or mask is not None:
            raise NotImplementedError(f"{kind}(...; condition, mask): conditional reductions are not implemented")
        if isinstance(operand, Reduction):
            operand = ComputedField(operand)
        if not _is_fieldlike(operand):
            raise TypeError(f"{kind} of {type(operand).__name__}: not a field or an operation")
        self.kind, self.operand, self.dims, self.grid = kind, operand, _tupleit_dims(dims), operand.grid
        for d in self.dims:
            if operand.location[d - 1] is None:
                raise ValueError(f"{kind} over dims = {self.dims}: the operand was already reduced along dimension {d}")

    @property
    def dims_mask(self):
        return sum(1 << (d - 1) for d in self.dims)

    @property
    def location(self):
        return tuple(None if (d + 1) in self.dims else self.operand.location[d] for d in range(3))


def Average(operand, dims=None, condition=None, mask=None):
    """Average(field; dims): the plain mean over the operand's interior over regular dims; Σ a·m / Σ m with the metric m of
    reduction_grid_metric at the operand's location if a stretched z is among them"""
    return Reduction("Average", operand, dims, condition, mask)


def Integral(operand, dims=None, condition=None, mask=None):
    """Integral(field; dims): Σ a·m"""
    return Reduction("Integral", operand, dims, condition, mask)


# ---- lowering -----------------------------------------------------------------------------------------------------------------------
# interpolation directions from the OUTERMOST average inwards (interpolation_operators.jl:45-71): xy has y outside, xz and yz have z
# outside, xyz has x outside and z inside
_INTERPOLATION_ORDER = {(): (), (0,): (0,), (1,): (1,), (2,): (2,), (0, 1): (1, 0), (0, 2): (2, 0), (1, 2): (2, 1), (0, 1, 2): (0, 1, 2)}


def _shift(off, d, s):
    o = list(off)
    o[d] += s
    return tuple(o)


class Program:
    """A lowered tree: `instructions` (dicts with op, a, b, field, off, value, reg), the distinct leaf `fields`, the tree's location mask
    `loc`, the registers used and `reach[d] = (furthest offset read below, above)` per direction."""

    def __init__(self, grid, loc):
        self.grid, self.loc = grid, loc
        self.instructions, self.fields = [], []
        self._by_key, self._by_node = {}, {}
        self.n_registers = 0

    # -- emission with merging of equal instructions --
    def _emit(self, op, a=-1, b=-1, field=-1, off=(0, 0, 0), value=0.0):
        key = (op, a, b, field, off, struct.pack("<d", value))
        q = self._by_key.get(key)
        if q is None:
            q = self._by_key[key] = len(self.instructions)
            self.instructions.append(dict(op=op, a=a, b=b, field=field, off=off, value=float(value), reg=-1))
        return q

    def const(self, value):
        return self._emit(_lib.OP_CONST, value=float(value))

    def spacing(self, d, face, dk):
        """Δ along d at a Face / Center location (Flat: ocn_grid's 1.0)"""
        if d < 2:
            return self._emit(_lib.OP_SPACING, field=(_lib.SPACING_DX, _lib.SPACING_DY)[d])
        stretched = self.grid._dzc_host is not None
        return self._emit(_lib.OP_SPACING, field=_lib.SPACING_DZF if face else _lib.SPACING_DZC, off=(0, 0, dk if stretched else 0))

    def _field_index(self, f):
        for q, g in enumerate(self.fields):
            if g is f:
                return q
        self.fields.append(f)
        return len(self.fields) - 1

    def load(self, f, off):
        reduced = getattr(f, "reduced", 0)
        # a reduced field is broadcast along its reduced directions; along a Flat direction there is one cell
        eff = tuple(0 if (reduced >> d) & 1 or self.grid.topology[d] == Flat else off[d] for d in range(3))
        if any(eff) and reduced:
            raise NotImplementedError("a reduced field interpolated or differentiated along a direction it keeps is not implemented")
        if any(eff) and not getattr(f, "halos_filled", True):
            raise ValueError("the tree reads a neighbour of a computed field whose halos are not filled (a reduced field, or a field at one of "
                             "the locations FFC, FCF, CFF, FFF)")
        return self._emit(_lib.OP_LOAD, field=self._field_index(f), off=eff)

    # -- the tree --
    def value(self, node, off):
        """SSA value of `node` at index offset `off` on the grid of its own location"""
        if _is_number(node):
            return self.const(node)
        key = (id(node), off)
        q = self._by_node.get(key)
        if q is None:
            q = self._by_node[key] = self._lower(node, off)
        return q

    def _lower(self, node, off):
        if isinstance(node, Field):
            return self.load(node, off)
        if isinstance(node, BinaryOperation):
            a = self.interpolated(node.a, _location(node.a), node.location, off)
            b = self.interpolated(node.b, _location(node.b), node.location, off)
            return self._emit(_OPCODE[node.op], a, b)
        if isinstance(node, UnaryOperation):
            return self.interpolated(("unary", node), node.arg.location, node.location, off)
        if isinstance(node, Derivative):
            return self.interpolated(("derivative", node), node.derivative_location, node.location, off)
        raise TypeError(f"cannot lower {type(node).__name__}")

    def _inner(self, what, off):
        """what the interpolation of a unary operation / a derivative averages: the operation at its own location"""
        if not isinstance(what, tuple):
            return self.value(what, off)
        kind, node = what
        key = (kind, id(node), off)
        q = self._by_node.get(key)
        if q is not None:
            return q
        if kind == "unary":
            if node.op in HOST_FOLDED_UNARY:
                raise NotImplementedError(f"{node.op} of the time or of a coordinate is folded by the host in a ContinuousForcing only: the "
                                          "device has no transcendental functions")
            x = self.value(node.arg, off)
            if node.op == "sq":
                q = self._emit(_lib.OP_MUL, x, x)
            elif node.op == "cube":
                q = self._emit(_lib.OP_MUL, self._emit(_lib.OP_MUL, x, x), x)
            else:
                q = self._emit(_OPCODE[node.op], x)
        else:
            d, arg = node.dim, node.arg
            if self.grid.topology[d] == Flat:
                q = self.const(0.0)  # ∂ along a Flat direction
            else:
                face = node.derivative_location[d] is Face
                # δᶠ(c) = c[i] - c[i-1] over Δᶠ[i];  δᶜ(u) = u[i+1] - u[i] over Δᶜ[i]   (derivative_operators.jl)
                hi, lo = (self.value(arg, off), self.value(arg, _shift(off, d, -1))) if face else (self.value(arg, _shift(off, d, 1)), self.value(arg, off))
                q = self._emit(_lib.OP_DIV, self._emit(_lib.OP_SUB, hi, lo), self.spacing(d, face, off[2]))
        self._by_node[key] = q
        return q

    def interpolated(self, what, l_from, l_to, off):
        """▶(what) from l_from to l_to at `off` (interpolation_operator): two-point averages along the directions in which both locations are
        concrete and differ; identity for numbers, along None and along Flat"""
        if _is_number(what):
            return self.const(what)
        dirs = tuple(d for d in range(3) if l_from[d] is not None and l_to[d] is not None and l_from[d] is not l_to[d]
                     and self.grid.topology[d] != Flat)
        return self._average(what, _INTERPOLATION_ORDER[dirs], l_to, off)

    def _average(self, what, dirs, l_to, off):
        if not dirs:
            return self._inner(what, off)
        d = dirs[0]
        # ℑᶜ(u) = 0.5 (u[i] + u[i+1]);  ℑᶠ(c) = 0.5 (c[i-1] + c[i])   (interpolation_operators.jl:8-15)
        o1, o2 = (-1, 0) if l_to[d] is Face else (0, 1)
        a = self._average(what, dirs[1:], l_to, _shift(off, d, o1))
        b = self._average(what, dirs[1:], l_to, _shift(off, d, o2))
        return self._emit(_lib.OP_MUL, self.const(0.5), self._emit(_lib.OP_ADD, a, b))

    # -- finishing --
    def finish(self, result):
        """Drop what the result does not need, order, assign registers (linear scan) and check the limits and the halos."""
        ins = self.instructions
        needed, stack = set(), [result]
        while stack:
            q = stack.pop()
            if q in needed:
                continue
            needed.add(q)
            stack.extend(x for x in (ins[q]["a"], ins[q]["b"]) if x >= 0)
        order = sorted(needed)  # (operands are always emitted before their users)
        assert order[-1] == result  # the value of the tree is the last instruction
        renumber = {q: n for n, q in enumerate(order)}
        self.instructions = [dict(ins[q], a=renumber.get(ins[q]["a"], -1), b=renumber.get(ins[q]["b"], -1)) for q in order]
        used_fields = sorted({i["field"] for i in self.instructions if i["op"] == _lib.OP_LOAD})
        fmap = {f: n for n, f in enumerate(used_fields)}
        self.fields = [self.fields[f] for f in used_fields]
        for i in self.instructions:
            if i["op"] == _lib.OP_LOAD:
                i["field"] = fmap[i["field"]]
        ins = self.instructions
        if len(ins) > _lib.OP_MAX_INSTRUCTIONS:
            raise ValueError(f"the tree lowers to {len(ins)} instructions, more than OCN_OP_MAX_INSTRUCTIONS = {_lib.OP_MAX_INSTRUCTIONS}: "
                             "compute a sub-tree into a ComputedField first")
        if len(self.fields) > _lib.OP_MAX_FIELDS:
            raise ValueError(f"the tree reads {len(self.fields)} fields, more than OCN_OP_MAX_FIELDS = {_lib.OP_MAX_FIELDS}")
        last_use = list(range(len(ins)))
        for q, i in enumerate(ins):
            for x in (i["a"], i["b"]):
                if x >= 0:
                    last_use[x] = q
        free, top = [], 0
        for q, i in enumerate(ins):
            for x in {i["a"], i["b"]}:
                if x >= 0 and last_use[x] == q:
                    free.append(ins[x]["reg"])  # (operands are read before the result is written)
            if free:
                free.sort()
                i["reg"] = free.pop(0)
            else:
                i["reg"], top = top, top + 1
        self.n_registers = top
        if top > _lib.OP_MAX_REGISTERS:
            raise ValueError(f"the tree needs {top} live values, more than OCN_OP_MAX_REGISTERS = {_lib.OP_MAX_REGISTERS}: "
                             "compute a sub-tree into a ComputedField first")
        self._check_halos()
        return self

    @property
    def loads(self):
        return [i for i in self.instructions if i["op"] == _lib.OP_LOAD]

    @property
    def reach(self):
        r = [[0, 0], [0, 0], [0, 0]]
        for i in self.instructions:
            if i["op"] in (_lib.OP_LOAD, _lib.OP_SPACING):
                for d in range(3):
                    r[d][0] = max(r[d][0], -i["off"][d])
                    r[d][1] = max(r[d][1], i["off"][d])
        return tuple(tuple(x) for x in r)

    def interior_size(self, loc=None):
        loc = self.loc if loc is None else loc
        g = self.grid
        return tuple(1 if g.topology[d] == Flat else g.size[d] + (1 if (loc >> d) & 1 and g.topology[d] == Bounded else 0) for d in range(3))

    def _check_halos(self):
        """every cell of the tree's interior, shifted, lies in the parent array of the field it reads (the check the library repeats)"""
        g = self.grid
        n, H = self.interior_size(), (g.Hx, g.Hy, g.Hz)
        for i in self.loads:
            f = self.fields[i["field"]]
            reduced = getattr(f, "reduced", 0)
            ext = g.parent_shape(f.loc)
            for d in range(3):
                if (reduced >> d) & 1:
                    continue
                if H[d] + i["off"][d] < 0 or H[d] + n[d] - 1 + i["off"][d] > ext[d] - 1:
                    raise ValueError(f"the tree reads {i['off'][d]:+d} cells along {'xyz'[d]}: further than the grid's halo ({H[d]}) holds for a "
                                     f"field at {_location_name(f)}")
        for i in self.instructions:
            if i["op"] == _lib.OP_SPACING and i["field"] >= _lib.SPACING_DZC and g._dzc_host is not None:
                dk = i["off"][2]
                if H[2] + dk < 0 or H[2] + n[2] - 1 + dk > g.Nz + 2 * H[2] - 1:
                    raise ValueError(f"the tree reads the z spacing {dk:+d} cells away: further than the grid's halo ({H[2]})")

    def c_struct(self):
        p = _lib.COpProgram()
        p.n_instructions, p.n_registers, p.n_fields, p.loc = len(self.instructions), self.n_registers, len(self.fields), self.loc
        for q, f in enumerate(self.fields):
            p.fields[q], p.field_loc[q], p.field_reduced[q] = f.ptr, f.loc, getattr(f, "reduced", 0)
        for q, i in enumerate(self.instructions):
            c = p.ins[q]
            c.opcode, c.a, c.b, c.reg, c.field, c.value = i["op"], max(i["a"], 0), max(i["b"], 0), i["reg"], max(i["field"], 0), i["value"]
            c.di, c.dj, c.dk = i["off"]
        return p


def _location_name(f):
    return "(" + ", ".join("Nothing" if l is None else l.__name__ for l in f.location) + ")"


def _metric(program, dims, location):
    """reduction_grid_metric(dims) at `location` (metric_field_reductions.jl:11-20; spacings_and_areas_and_volumes.jl:278-343):
    Δx, Δy, Δz, Az = Δx Δy, Ay = Δx Δz, Ax = Δy Δz, V = Az Δz"""
    m = None
    for d in dims:
        s = program.spacing(d - 1, location[d - 1] is Face, 0)
        m = s if m is None else program._emit(_lib.OP_MUL, m, s)
    return m


def _refuse(grid, who):
    if hasattr(grid, "immersed_boundary"):
        # (the reference's reductions there are conditional on the active cells, and its operations mask their result)
        raise NotImplementedError(f"{who} of a field on an ImmersedBoundaryGrid is not implemented: conditional reductions and masked "
                                  "operations do not exist here; compute on the host with ocn.immersed_cell(grid)")
    if hasattr(grid.architecture, "partition"):
        raise NotImplementedError(f"{who} on a Distributed architecture is not implemented")
    require_regular_xy(grid, who)


def lower(operand):
    """The Program of an operation (or a field), or of the summand of an Average / Integral: pure Python, no device is touched."""
    if isinstance(operand, Reduction):
        tree, grid = operand.operand, operand.grid
        _refuse(grid, operand.kind)
        p = Program(grid, location_mask(tree.location))
        v = p.value(tree, (0, 0, 0))
        p.weighted = operand.kind == "Integral" or (3 in operand.dims and grid._dzc_host is not None)
        if p.weighted:
            v = p._emit(_lib.OP_MUL, v, _metric(p, operand.dims, tree.location))
        return p.finish(v)
    if not _is_fieldlike(operand):
        raise TypeError(f"cannot compute {type(operand).__name__}: not an operation, a field or a reduction")
    _refuse(operand.grid, "an operation")
    p = Program(operand.grid, location_mask(operand.location))
    return p.finish(p.value(operand, (0, 0, 0)))


def _divisor(reduction, program):
    """what the sum is divided by: 1 for an Integral, the number of points for a plain mean, Σ m (rounded once) otherwise"""
    if reduction.kind == "Integral":
        return 1.0
    g, n = reduction.grid, program.interior_size()
    if not program.weighted:
        return float(np.prod([n[d - 1] for d in reduction.dims]))
    loc = reduction.operand.location
    dz = (g._dzf_host if loc[2] is Face else g._dzc_host)[g.Hz:g.Hz + n[2]]
    total = Fraction(0)
    for k in range(n[2]):
        m = None
        for d in reduction.dims:  # the products of the device, in its order
            s = float(dz[k]) if d == 3 else (g.dx, g.dy)[d - 1]
            m = s if m is None else m * s
        total += Fraction(m)
    return float(total * int(np.prod([n[d - 1] for d in reduction.dims if d != 3])))


def _dependencies(program):
    return [f for f in program.fields if isinstance(f, ComputedField)]


class ComputedField(Field):
    """Field(operation) / Field(Average(...)) of the reference: lowering, validation and allocation happen here, once; `compute()` only
    enqueues kernels on the current stream.  Reduced directions have extent 1 and location None.  `halos_filled`: after compute() the
    halos hold the default fill (fields at the four model locations) or nothing (reduced fields and the locations FFC, FCF, CFF, FFF)."""

    def __init__(self, operand):
        if isinstance(operand, ComputedField):
            operand = operand.operand
        self.operand = operand
        self.program = lower(operand)  # (refuses before anything is allocated)
        grid = self.grid = self.program.grid
        self.boundary_conditions = None
        self.loc = self.program.loc
        self.reduced = operand.dims_mask if isinstance(operand, Reduction) else 0
        self.halos_filled = self.reduced == 0 and self.loc in _MODEL_LOCATIONS
        self.dependencies = _dependencies(self.program)
        self.data = zeros(grid.architecture, self.parent_shape())
        self._c = self.program.c_struct()
        self._workspace = None
        if self.reduced:
            self._divisor = _divisor(operand, self.program)
            n = C.c_int64()
            _lib.call("ocn_op_reduce_workspace", grid.cref, self.loc, self.reduced, C.byref(n))
            self._workspace = zeros(grid.architecture, (n.value, 1, 1))

    @property
    def location(self):
        return location_of(self.loc, self.reduced)

    def parent_shape(self):
        full = self.grid.parent_shape(self.loc)
        return tuple(1 if (self.reduced >> d) & 1 else full[d] for d in range(3))

    def interior_view(self):
        g = self.grid
        H = [0 if (self.reduced >> d) & 1 else h for d, h in enumerate((g.Hx, g.Hy, g.Hz))]
        sz, sy, sx = self.data.shape
        return self.data[H[2]:sz - H[2], H[1]:sy - H[1], H[0]:sx - H[0]]

    def compute(self):
        """compute!(field): the computed fields among the leaves first (compute_at!), then this one; returns self"""
        for f in self.dependencies:
            f.compute()
        grid = self.grid
        for q, f in enumerate(self.program.fields):  # (a model may exchange the buffers of its fields between steps)
            self._c.fields[q] = f.ptr
        if self.reduced:
            _lib.call("ocn_op_reduce", grid.cref, C.byref(self._c), self.reduced, self._divisor, self._workspace.data_ptr(),
                      self._workspace.numel(), self.ptr, stream_ptr())
        else:
            _lib.call("ocn_op_compute", grid.cref, C.byref(self._c), self.ptr, stream_ptr())
            if self.halos_filled:
                # (the interior, boundary faces included, stays what the tree gives: no wall-normal zeroing)
                fill_halo_regions(self, fill_boundary_normal_velocities=False)
        return self


def compute(x):
    """compute!(Field(x)) for an operation or a reduction; compute!(x) for a ComputedField"""
    return (x if isinstance(x, ComputedField) else ComputedField(x)).compute()
