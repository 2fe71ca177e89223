"""User forcing of NonhydrostaticModel (src/Forcings): forcing = {"u": ..., "T": ...}.

    Relaxation(; rate, mask, target), GaussianMask{:z}(; center, width), LinearTarget{:z}(; intercept, gradient)     relaxation.jl:17-197
        -> Relaxation(rate, mask=None, target=None), GaussianMask("z", center=, width=), LinearTarget("z", intercept=, gradient=)
    Forcing(func; parameters)                                                                                    forcing.jl, continuous_forcing.jl
        -> Forcing(func, parameters=None, steady=None)
    ContinuousForcing(func; parameters, field_dependencies)                                                      continuous_forcing.jl:109-142
        -> ContinuousForcing(func, parameters=None, field_dependencies=()): traced once, evaluated on the device (forcing_programs.py)
    an array on the field's grid (regularize_forcing(array::AbstractArray, ...)), a tuple / list of up to four of these (MultipleForcings)

Python has no type parameters, so the direction of a mask / target is its first argument.  A bare Python function is NOT a forcing value
here: wrap it, forcing={"u": Forcing(func)} (a spelling the reference has too).

The forcing of a field is the LAST addend of its tendency (nonhydrostatic_tendency_kernel_functions.jl:77, 137, 199, 258): after the
Stokes-drift terms of u, v, w, after the diffusion of a tracer, before the boundary fluxes.  The device never calls a user function: the
host samples every term on the nodes of the forced field's OWN location (continuous_forcing.jl:135-142) into struct ocn_forcing --
arrays in the field's parent layout, Nx / Ny / Nz-long vectors (halos included) for masks and targets that vary along one direction.
Flat directions are omitted from the argument list of a function, as for the boundary functions.

When are the functions sampled?  ONE rule, the one stokes.py documents: `steady`.  A steady term is sampled once, when the model is built
(t = 0); any other term is resampled at clock.time before every tendency evaluation, every RK3 stage included.  `steady` defaults to True
when nothing that receives `t` is callable (arrays, numbers, GaussianMask, LinearTarget -- which ignores t -- and masks, which never
receive t) and to False as soon as a Forcing(func) or a function-valued Relaxation target is there; steady=True declares that the function
ignores t.  A forcing that is not steady runs through the Python host only (ModelRK3Driver refuses it).
"""
import numpy as np

from . import _lib

MAX_TERMS = 4  # OCN_FORCING_MAX_TERMS
FORCING_ARRAY, FORCING_RELAXATION = 1, 2
_DIRS = {"x": 0, "y": 1, "z": 2}
_NUMBER = (int, float, np.floating, np.integer)


def _jl(x):
    """a Float64 as Julia prints it"""
    return repr(float(x))


def _direction(d, who):
    d = str(d).lstrip(":")
    if d not in _DIRS:
        raise ValueError(f'{who}: the direction must be "x", "y" or "z", got {d!r}')
    return d


class GaussianMask:
    """GaussianMask{D}(; center, width): exp(-(D - center)^2 / (2 * width^2))   (relaxation.jl:113-155)"""

    def __init__(self, direction, center, width):
        self.direction = _direction(direction, "GaussianMask")
        self.center, self.width = float(center), float(width)

    def along(self, X):
        return np.exp(-(X - self.center) ** 2 / (2 * self.width ** 2))

    def __call__(self, x, y, z):
        return self.along((x, y, z)[_DIRS[self.direction]])

    def summary(self):
        D, c = self.direction, self.center
        arg = f"{D}^2" if c == 0 else (f"({D} - {_jl(c)})^2" if c > 0 else f"({D} + {_jl(-c)})^2")
        return f"exp(-{arg} / (2 * {_jl(self.width)}^2))"

    def type_name(self):
        return f"GaussianMask{{:{self.direction}, Float64}}"

    __repr__ = summary


class LinearTarget:
    """LinearTarget{D}(; intercept, gradient): intercept + gradient * D   (relaxation.jl:157-197)"""

    def __init__(self, direction, intercept, gradient):
        self.direction = _direction(direction, "LinearTarget")
        self.intercept, self.gradient = float(intercept), float(gradient)

    def along(self, X):
        return self.intercept + self.gradient * X

    def __call__(self, x, y, z, t):
        return self.along((x, y, z)[_DIRS[self.direction]])

    def summary(self):
        return f"{_jl(self.intercept)} + {_jl(self.gradient)} * {self.direction}"

    def type_name(self):
        return f"LinearTarget{{:{self.direction}, Float64}}"

    __repr__ = summary


def _summary(x, default):
    if x is None:
        return default
    if hasattr(x, "summary"):
        return x.summary()
    if isinstance(x, np.ndarray):
        return "×".join(map(str, x.shape)) + " Array{Float64, %d}" % x.ndim
    if callable(x):
        return getattr(x, "__name__", type(x).__name__)
    return _jl(x)


def _type_name(x, default):
    if x is None:
        return f"typeof(Oceananigans.Forcings.{default})"
    if hasattr(x, "type_name"):
        return x.type_name()
    if isinstance(x, np.ndarray):
        return "Array{Float64, %d}" % x.ndim
    if callable(x):
        return f"typeof({getattr(x, '__name__', type(x).__name__)})"
    return "Float64"


class Relaxation:
    """Relaxation(rate, mask=None, target=None, steady=None):  F = (rate * mask(X)) * (target(X, t) - field[i, j, k])   (relaxation.jl:17-101)

    mask: None (1), GaussianMask(direction, ...), a function mask(x, y, z) or an array on the field's grid.
    target: None (0), a number, LinearTarget(direction, ...), a function target(x, y, z, t) or an array on the field's grid.
    Masks never receive t: they are sampled once.  See the module docstring for `steady`."""

    def __init__(self, rate, mask=None, target=None, steady=None):
        self.rate = float(rate)
        if mask is not None and not callable(mask):
            mask = np.asarray(mask, dtype=np.float64)
            if mask.ndim == 0:
                raise TypeError("Relaxation: mask must be None, GaussianMask(...), a function of (x, y, z) or an array")
        if target is not None and not callable(target):
            target = float(target) if isinstance(target, _NUMBER) else np.asarray(target, dtype=np.float64)
        self.mask, self.target = mask, target
        receives_t = callable(target) and not isinstance(target, LinearTarget)
        self.steady = (not receives_t) if steady is None else bool(steady)
        if not self.steady and not receives_t:
            raise ValueError("Relaxation: steady=False needs a function-valued target")

    def summary(self):
        return f"Relaxation(rate={_jl(self.rate)}, mask={_summary(self.mask, '1')}, target={_summary(self.target, '0')})"

    def __repr__(self):
        """Base.show(io, ::Relaxation) (relaxation.jl:104-108)"""
        return (f"Relaxation{{Float64, {_type_name(self.mask, 'onefunction')}, {_type_name(self.target, 'zerofunction')}}}\n"
                f"├── rate: {_jl(self.rate)}\n"
                f"├── mask: {_summary(self.mask, '1')}\n"
                f"└── target: {_summary(self.target, '0')}")


class Forcing:
    """Forcing(func, parameters=None, steady=None): func(x, y, z, t) or func(x, y, z, t, parameters), evaluated by the host on the nodes of
    the forced field's own location (Flat directions omitted from the arguments).  See the module docstring for `steady`."""

    def __init__(self, func, parameters=None, steady=None, field_dependencies=(), discrete_form=False):
        if field_dependencies not in ((), None, []):
            raise NotImplementedError("forcing: Forcing(func, field_dependencies=...) is not implemented: the host samples the function, "
                                      "it cannot read the fields cell by cell; ContinuousForcing(func, field_dependencies=...) traces the "
                                      "function and evaluates it on the device (see DESIGN.md §5.2d')")
        if discrete_form:
            raise NotImplementedError("forcing: Forcing(func, discrete_form=True) is not implemented (see DESIGN.md §10)")
        if not callable(func):
            raise TypeError("Forcing(func, ...): func must be callable; an array is a forcing value by itself")
        self.func, self.parameters = func, parameters
        self.steady = False if steady is None else bool(steady)

    def summary(self):
        return f"ContinuousForcing{{{'Nothing' if self.parameters is None else type(self.parameters).__name__}}}"

    def __repr__(self):
        return f"{self.summary()}\n├── func: {getattr(self.func, '__name__', type(self.func).__name__)}\n└── parameters: {self.parameters!r}"


class ContinuousForcing:
    """ContinuousForcing(func, parameters=None, field_dependencies=()): func(X..., t, deps..., [parameters]) -- the coordinates of the forced
    field's own location (Flat directions omitted), the time, the dependencies in the order given, interpolated to that location -- is
    called ONCE, when the model is built, with symbolic operands; the tree it returns is evaluated on the device (forcing_programs.py).
    field_dependencies: a name or a tuple of names of velocities and tracers; () gives the traced, device-evaluated form of Forcing(func)."""

    def __init__(self, func, parameters=None, field_dependencies=(), discrete_form=False):
        if discrete_form:
            raise NotImplementedError("forcing: ContinuousForcing(func, discrete_form=True) is not implemented: a function of (i, j, k, grid, "
                                      "clock, fields) cannot be traced (see DESIGN.md §10)")
        if not callable(func):
            raise TypeError("ContinuousForcing(func, ...): func must be callable; an array is a forcing value by itself")
        if field_dependencies is None:
            field_dependencies = ()
        if isinstance(field_dependencies, str):
            field_dependencies = (field_dependencies,)
        field_dependencies = tuple(field_dependencies)
        if not all(isinstance(n, str) for n in field_dependencies):
            raise TypeError("ContinuousForcing: field_dependencies is a field name or a tuple of field names")
        self.func, self.parameters, self.field_dependencies = func, parameters, field_dependencies

    def summary(self):
        return f"ContinuousForcing{{{'Nothing' if self.parameters is None else type(self.parameters).__name__}}}"

    def __repr__(self):
        return (f"{self.summary()}\n├── func: {getattr(self.func, '__name__', type(self.func).__name__)}\n├── parameters: {self.parameters!r}\n"
                f"└── field dependencies: {self.field_dependencies!r}")


# names a forcing function may not depend on: the model computes them, they are no prognostic fields
_AUXILIARY_FIELDS = ("νₑ", "nu_e", "κₑ", "kappa_e", "pNHS", "pHY′", "pHY")


class AdvectiveForcing:
    def __init__(self, *args, **kwargs):
        raise NotImplementedError("forcing: AdvectiveForcing is not implemented (see DESIGN.md §10)")


# ---------------------------------------------------------------------------------------------------------------------------------------
# validation (before anything is allocated) and sampling
# ---------------------------------------------------------------------------------------------------------------------------------------
def field_location(name):
    return {"u": _lib.LOC_FCC, "v": _lib.LOC_CFC, "w": _lib.LOC_CCF}.get(name, _lib.LOC_CCC)


def interior_shape(grid, loc):
    """shape [i, j, k] of what ocn.set accepts for a field at `loc`"""
    sx, sy, sz = grid.parent_shape(loc)
    return (sx - 2 * grid.Hx, sy - 2 * grid.Hy, sz - 2 * grid.Hz)


def _terms_of(value):
    return list(value) if isinstance(value, (tuple, list)) else [value]


def validate_forcing(forcing, grid, field_names):
    """forcing = {name: value} -> {name: [terms]}; raises before any allocation.  NotImplementedError messages name `forcing`."""
    if not isinstance(forcing, dict):
        raise TypeError("forcing must be a dict {field name: forcing}")
    if hasattr(grid.architecture, "partition"):
        raise NotImplementedError("forcing on a Distributed architecture is not implemented (see DESIGN.md §10)")
    out = {}
    for name, value in forcing.items():
        if name not in field_names:
            raise ValueError(f"forcing given for unknown field {name!r}; the model has {tuple(field_names)}")
        terms = _terms_of(value)
        if len(terms) > MAX_TERMS:
            raise NotImplementedError(f"forcing of {name}: {len(terms)} terms; at most {MAX_TERMS} are implemented (see DESIGN.md §10)")
        shape = interior_shape(grid, field_location(name))
        checked = []
        for term in terms:
            if isinstance(term, ContinuousForcing):
                for dep in term.field_dependencies:
                    if dep in _AUXILIARY_FIELDS and dep not in field_names:
                        raise NotImplementedError(f"forcing of {name}: a dependency on the diffusivity / auxiliary field {dep!r} is not "
                                                  "implemented: the dependencies are velocities and tracers (see DESIGN.md §10)")
                from .boundary_functions import validate_dependencies
                validate_dependencies(term.field_dependencies, tuple(field_names))
                checked.append(term)
            elif isinstance(term, (Relaxation, Forcing)):
                if isinstance(term, Relaxation):
                    for what, a in (("mask", term.mask), ("target", term.target)):
                        if isinstance(a, np.ndarray) and a.shape != shape:
                            raise ValueError(f"forcing of {name}: Relaxation {what} has shape {a.shape}, expected the interior shape {shape}")
                        if isinstance(a, (GaussianMask, LinearTarget)) and grid.topology[_DIRS[a.direction]] == "Flat":
                            raise ValueError(f"forcing of {name}: {a.type_name()} varies along a Flat direction")
                checked.append(term)
            elif callable(term):
                raise NotImplementedError(f"forcing of {name}: a bare function is not a forcing value here; wrap it: "
                                          f'forcing={{"{name}": ocn.Forcing(func)}} with func(x, y, z, t[, parameters])')
            elif type(term).__name__ in ("FieldTimeSeries", "AdvectiveForcing"):
                raise NotImplementedError(f"forcing of {name}: {type(term).__name__} is not implemented (see DESIGN.md §10)")
            else:
                try:
                    a = np.asarray(term, dtype=np.float64)
                except (TypeError, ValueError):
                    raise NotImplementedError(f"forcing of {name}: unsupported forcing {type(term).__name__}; use an array, Relaxation(...), "
                                              "Forcing(func), ContinuousForcing(func, ...) or a tuple of them") from None
                if a.shape != shape:
                    raise ValueError(f"forcing of {name}: array shape {a.shape} != interior shape {shape}")
                checked.append(a)
        if checked:
            out[name] = checked
    return out


def _node_args(grid, loc):
    """broadcastable node coordinates of a field at `loc`, Flat directions omitted"""
    return [c for c, t in zip(grid.nodes(loc), grid.topology) if t != "Flat"]


def _evaluate(f, args, shape):
    try:
        a = np.asarray(f(*args), dtype=np.float64)
        return np.array(np.broadcast_to(a, shape), dtype=np.float64)
    except (TypeError, ValueError) as first:  # a function that cannot take arrays (math.exp ...): node by node
        try:
            a = np.vectorize(lambda *q: float(f(*q)), otypes=[np.float64])(*args)
        except Exception as second:
            raise second from first  # both tracebacks: the array call is usually the one that tells what is wrong
    return np.array(np.broadcast_to(a, shape), dtype=np.float64)


def _vector(grid, loc, d, profile):
    """a mask / target that varies along direction d, on the nodes of the field's location with halos: element 0 <-> index 1 - H"""
    n = grid.parent_shape(loc)[d]
    X = np.asarray(grid.nodes_1d(d, bool(loc & (1 << d)), with_halos=True), dtype=np.float64)[:n]
    if X.size != n:
        raise NotImplementedError(f"forcing: the grid gives {X.size} nodes with halos along {'xyz'[d]}, the parent array has {n}")
    return np.ascontiguousarray(profile.along(X))


def sample_term(term, grid, loc, t=0.0):
    """One term on the host: {"kind", "rate", "values", "mask_dim", "mask", "target_dim", "target", "target_value"} with interior-shaped
    [i, j, k] arrays for dim 3 / values and vectors with halos for dims 0, 1, 2."""
    shape = interior_shape(grid, loc)
    out = dict(kind=FORCING_ARRAY, rate=0.0, values=None, mask_dim=-1, mask=None, target_dim=-1, target=None, target_value=0.0)
    if isinstance(term, np.ndarray):
        out["values"] = term
        return out
    if isinstance(term, Forcing):
        args = _node_args(grid, loc) + [t] + ([] if term.parameters is None else [term.parameters])
        out["values"] = _evaluate(term.func, args, shape)
        return out
    out["kind"], out["rate"] = FORCING_RELAXATION, term.rate
    m, g = term.mask, term.target
    if isinstance(m, GaussianMask):
        out["mask_dim"] = _DIRS[m.direction]
        out["mask"] = _vector(grid, loc, out["mask_dim"], m)
    elif isinstance(m, np.ndarray):
        out["mask_dim"], out["mask"] = 3, m
    elif m is not None:
        out["mask_dim"], out["mask"] = 3, _evaluate(m, _node_args(grid, loc), shape)
    if isinstance(g, LinearTarget):
        out["target_dim"] = _DIRS[g.direction]
        out["target"] = _vector(grid, loc, out["target_dim"], g)
    elif isinstance(g, np.ndarray):
        out["target_dim"], out["target"] = 3, g
    elif isinstance(g, float):
        out["target_value"] = g
    elif g is not None:
        out["target_dim"], out["target"] = 3, _evaluate(g, _node_args(grid, loc) + [t], shape)
    return out


def has_program(terms):
    """a ContinuousForcing among the terms: all of them are then lowered into one program (forcing_programs.py)"""
    return any(isinstance(t, ContinuousForcing) for t in terms)


def is_steady(term):
    return isinstance(term, np.ndarray) or term.steady


class DeviceForcing:
    """The device side of ONE field's forcing: struct ocn_forcing and the vectors / arrays it points to (allocated once, so the struct never
    changes), refreshed at clock.time for terms that are not steady."""

    def __init__(self, terms, grid, loc):
        from .architectures import on_architecture
        self.terms, self.grid, self.loc = terms, grid, loc
        self.steady = all(is_steady(t) for t in terms)
        self.c = _lib.CForcing()
        self.c.n_terms = len(terms)
        self.buffers = []
        for q, term in enumerate(terms):
            host = sample_term(term, grid, loc, 0.0)
            ct = self.c.term[q]
            ct.kind, ct.rate, ct.target_value = host["kind"], host["rate"], host["target_value"]
            ct.mask_dim, ct.target_dim = host["mask_dim"], host["target_dim"]
            dev = {}
            for key, dim in (("values", 3 if host["values"] is not None else -1), ("mask", host["mask_dim"]), ("target", host["target_dim"])):
                if dim < 0:
                    continue
                dev[key] = self._parent(host[key]) if dim == 3 else on_architecture(grid.architecture, host[key])
                setattr(ct, key, dev[key].data_ptr())
            self.buffers.append(dev)
        self.time = 0.0

    def _parent(self, interior):
        """an interior-shaped [i, j, k] host array -> a zero-haloed device array in the field's parent layout"""
        from .fields import Field
        return Field(self.loc, self.grid).set(interior).data

    def refresh(self, t):
        if self.steady or t == self.time:
            return
        from .architectures import on_architecture
        g = self.grid
        for term, dev in zip(self.terms, self.buffers):
            if is_steady(term):
                continue
            host = sample_term(term, g, self.loc, t)
            key = "values" if isinstance(term, Forcing) else "target"
            sz, sy, sx = dev[key].shape
            dev[key][g.Hz:sz - g.Hz, g.Hy:sy - g.Hy, g.Hx:sx - g.Hx].copy_(on_architecture(g.architecture, np.ascontiguousarray(host[key].T)))
        self.time = t

    @property
    def ref(self):
        import ctypes as C
        return C.pointer(self.c)
