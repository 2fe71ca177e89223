"""Hand-written case pairs for ContinuousForcing (oceananigans.jl_amd/forcing_programs.py): the user function, and a NumPy restatement of
the forcing over the cells at which a tendency is computed, written from the reference and independent of the package's lowering:

  the call func(X..., t, deps..., [parameters])              src/Forcings/continuous_forcing.jl:135-142, src/Utils/user_function_arguments.jl
  dependencies interpolated to the forced field's location   src/Operators/interpolation_utils.jl:99-109, interpolation_operators.jl:8-71
  ((F1 + F2) + F3) + F4                                      src/Forcings/multiple_forcings.jl:34-46
  (rate * mask) * (target - field)                           src/Forcings/relaxation.jl:95-101
  min, max                                                   Julia's Base.min / Base.max of two Float64

Arrays are parents indexed [i, j, k] with halos.  The cells: the interior of the forced field's location without the faces on a wall
(faces 2 .. N of the N + 1 along a Face & Bounded direction: periphery_offset, kernel_launching.jl:113-114), where the tendency kernels add a
forcing.  The restatement interpolates with its own 0.5 * (a + b) slices, applies min / max through its own function (np.maximum gives -0.0
for (-0.0, +0.0)) and evaluates a foldable transcendental with the same NumPy call on the same halo-included 1-D node vector, then slices.

The velocities and tracers of a model live at (F,C,C), (C,F,C), (C,C,F) and (C,C,C): two of those locations differ along two directions
at the most, so an interpolation along three directions cannot occur in a forcing; one and two are covered.
Not a test module."""
import numpy as np

P, B, F = "Periodic", "Bounded", "Flat"
LOCS = {"u": 1, "v": 2, "w": 4}
NAMES = ("u", "v", "w", "T", "b")

STRETCHED_Z = [-1.0, -0.7, -0.45, -0.25, -0.1, 0.0]
GRIDS = {
    # x crosses a 64-wide block; in the last block of 8 rows some lanes have a second row (j + 4 < 13) and some do not
    "ppb": dict(size=(70, 13, 5), x=(0, 3), y=(0, 1), z=STRETCHED_Z, topology=(P, P, B), halo=(3, 3, 3)),
    # no lane has a second row
    "short": dict(size=(12, 3, 6), x=(0, 3), y=(0, 1), z=(-1, 0), topology=(P, P, B), halo=(3, 3, 3)),
    # faces on walls in every direction; the interpolations read wall halos
    "bbb": dict(size=(12, 10, 8), x=(0, 3), y=(0, 1), z=(-1, 0), topology=(B, B, B), halo=(3, 3, 3)),
    "pfb": dict(size=(16, 8), x=(0, 3), z=(-1, 0), topology=(P, F, B), halo=(3, 3)),
    "wide": dict(size=(9, 5, 5), x=(0, 3), y=(0, 1), z=STRETCHED_Z, topology=(P, P, B), halo=(4, 3, 5)),
}


def loc_of(name):
    return LOCS.get(name, 0)


def random_parents(grid, seed, names=NAMES):
    """name -> parent array [i, j, k], seeded random everywhere, halos included"""
    rng = np.random.default_rng(seed)
    return {n: rng.uniform(-1.0, 1.0, grid.parent_shape(loc_of(n))) for n in names}


def cells(grid, loc):
    """(first, last) 0-based interior index of the cells a tendency is computed at, per direction"""
    out = []
    for d in range(3):
        N, t = grid.size[d], grid.topology[d]
        if t == F:
            out.append((0, 0))
        elif (loc >> d) & 1 and t == B and N > 1:
            out.append((1, N - 1))
        else:
            out.append((0, N - 1))
    return tuple(out)


def cell_slices(grid, loc, off=(0, 0, 0)):
    H = (grid.Hx, grid.Hy, grid.Hz)
    return tuple(slice(0, 1) if grid.topology[d] == F else slice(H[d] + lo + off[d], H[d] + hi + 1 + off[d])
                 for d, (lo, hi) in enumerate(cells(grid, loc)))


def julia_max(a, b):
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    out = np.where(a >= b, a, b)
    zeros = (a == 0) & (b == 0)
    out = np.where(zeros, np.where(np.signbit(a) & np.signbit(b), -0.0, 0.0), out)
    return np.where(np.isnan(a), a, np.where(np.isnan(b), b, out))


def julia_min(a, b):
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    out = np.where(a <= b, a, b)
    zeros = (a == 0) & (b == 0)
    out = np.where(zeros, np.where(np.signbit(a) | np.signbit(b), -0.0, 0.0), out)
    return np.where(np.isnan(a), a, np.where(np.isnan(b), b, out))


class Restatement:
    """What a restatement reads: parents over the cells of the forced location `loc`, shifted; node vectors with halos, cut to the cells"""

    def __init__(self, grid, parents, loc):
        self.grid, self.parents, self.loc = grid, parents, loc
        self.shape = tuple(hi - lo + 1 for lo, hi in cells(grid, loc))

    def at(self, name):
        return lambda off=(0, 0, 0): self.parents[name][cell_slices(self.grid, self.loc, off)]

    def _two_point(self, fn, d):
        """ℑ along d TO the forced location: ℑᶠ(c) = 0.5 (c[i-1] + c[i]), ℑᶜ(u) = 0.5 (u[i] + u[i+1]); the identity along Flat"""
        if self.grid.topology[d] == F:
            return fn
        o1, o2 = (-1, 0) if (self.loc >> d) & 1 else (0, 1)

        def shifted(off, s):
            o = list(off)
            o[d] += s
            return tuple(o)
        return lambda off=(0, 0, 0): 0.5 * (fn(shifted(off, o1)) + fn(shifted(off, o2)))

    def ix(self, fn):
        return self._two_point(fn, 0)

    def iy(self, fn):
        return self._two_point(fn, 1)

    def iz(self, fn):
        return self._two_point(fn, 2)

    def nodes_with_halos(self, d):
        return np.ascontiguousarray(self.grid.nodes_1d(d, (self.loc >> d) & 1, with_halos=True), dtype=np.float64)

    def cut(self, vector, d):
        """a vector on the nodes of direction d with halos -> its cells, shaped for broadcasting over [i, j, k]"""
        H = (self.grid.Hx, self.grid.Hy, self.grid.Hz)[d]
        lo, hi = cells(self.grid, self.loc)[d]
        return vector[H + lo:H + hi + 1].reshape(tuple(-1 if e == d else 1 for e in range(3)))

    def node(self, d):
        return self.cut(self.nodes_with_halos(d), d)

    def full(self, a):
        return np.array(np.broadcast_to(a, self.shape), dtype=np.float64)


def split(grid, args, ndeps, has_parameters):
    """the arguments a forcing function is given -> ({"x": ., "y": ., "z": .} without the Flat directions, t, [deps], parameters)"""
    names = [n for n, t in zip("xyz", grid.topology) if t != F]
    X = dict(zip(names, args[:len(names)]))
    t = args[len(names)]
    deps = list(args[len(names) + 1:len(names) + 1 + ndeps])
    return X, t, deps, (args[-1] if has_parameters else None)


class Case:
    """forced: the forced field; terms(ocn, grid): the forcing value (a term or a tuple); restate(R, t): the forcing over the cells"""

    def __init__(self, forced, terms, restate):
        self.forced, self.terms, self.restate = forced, terms, restate

    def expected(self, grid, parents, t):
        R = Restatement(grid, parents, loc_of(self.forced))
        with np.errstate(all="ignore"):
            return R.full(self.restate(R, np.float64(t)))


PLANKTON = dict(mu0=1 / 86400, lam=5.0, m=0.1 / 86400)
MIXED = dict(rate=0.25, center=-0.4, width=0.3, intercept=0.5, gradient=-0.2, mu=0.125)


def mixed_array(grid):
    n = tuple(s - 2 * h for s, h in zip(grid.parent_shape(0), (grid.Hx, grid.Hy, grid.Hz)))
    return np.random.default_rng(99).uniform(-1, 1, n)


def cases(ocn):
    def drag_u(grid):
        return ocn.ContinuousForcing(lambda *a: -a[-1]["mu"] * a[-2], field_dependencies="u", parameters=dict(mu=0.375))

    def plankton(grid):
        def growing_and_grazing(*a):
            X, t, (Pl,), p = split(grid, a, 1, True)
            return (p["mu0"] * ocn.exp(X["z"] / p["lam"]) - p["m"]) * Pl
        return ocn.ContinuousForcing(growing_and_grazing, field_dependencies="b", parameters=PLANKTON)

    def restate_plankton(R, t):
        p = PLANKTON
        growth = p["mu0"] * np.exp(R.nodes_with_halos(2) / p["lam"]) - p["m"]
        return R.cut(growth, 2) * R.at("b")()

    def one_direction(grid):
        def f(*a):
            X, t, (u, T), p = split(grid, a, 2, False)
            return u * T
        return ocn.ContinuousForcing(f, field_dependencies=("u", "T"))

    def two_directions(grid):  # with a sub-tree of the time alone: one folded constant
        def f(*a):
            X, t, (u,), p = split(grid, a, 1, True)
            return -(p["f0"] * ocn.cos(p["om"] * t)) * u
        return ocn.ContinuousForcing(f, field_dependencies="u", parameters=dict(f0=0.7, om=3.0))

    def on_w(grid):  # a sub-tree of one coordinate and the time: a vector that is folded again at every time; np. spelling
        def f(*a):
            X, t, (u, b), p = split(grid, a, 2, False)
            return np.sin(2.5 * X["x"] - 1.5 * t) * b + u * 0.25
        return ocn.ContinuousForcing(f, field_dependencies=("u", "b"))

    def restate_on_w(R, t):
        wave = np.sin(2.5 * R.nodes_with_halos(0) - 1.5 * t)
        return R.cut(wave, 0) * R.iz(R.at("b"))() + R.iz(R.ix(R.at("u")))() * 0.25   # ℑxzᶜᵃᶠ = ℑz(ℑx)

    def min_max(grid):
        def f(*a):
            X, t, (T, w), p = split(grid, a, 2, False)
            return ocn.maximum(T, 0.0) - np.minimum(w, 0.25 * T)
        return ocn.ContinuousForcing(f, field_dependencies=("T", "w"))

    def restate_min_max(R, t):
        T = R.at("T")()
        return julia_max(T, 0.0) - julia_min(R.iz(R.at("w"))(), 0.25 * T)

    def coordinates(grid):
        def f(*a):
            X, t, _, p = split(grid, a, 0, False)
            return 0.3 * X["x"] - X["z"] * X["z"] + t * 0.5
        return ocn.ContinuousForcing(f)

    def mixed(grid):
        m = MIXED

        def sampled(*a):
            X, t, _, p = split(grid, a, 0, False)
            return 0.3 * X["x"] - X["z"] * X["z"]
        return (mixed_array(grid),
                ocn.Relaxation(m["rate"], mask=ocn.GaussianMask("z", center=m["center"], width=m["width"]),
                               target=ocn.LinearTarget("z", intercept=m["intercept"], gradient=m["gradient"])),
                ocn.Forcing(sampled, steady=True),
                ocn.ContinuousForcing(lambda *a: -a[-1] * a[-2], field_dependencies="T", parameters=m["mu"]))

    def restate_mixed(R, t):
        m, g = MIXED, R.grid
        z = R.nodes_with_halos(2)[:g.parent_shape(0)[2]]
        mask = np.exp(-(z - m["center"]) ** 2 / (2 * m["width"] ** 2))
        target = m["intercept"] + m["gradient"] * z
        T = R.at("T")()
        array = np.zeros(g.parent_shape(0))
        array[g.Hx:g.Hx + g.Nx, g.Hy:g.Hy + g.Ny, g.Hz:g.Hz + g.Nz] = mixed_array(g)
        relaxation = (m["rate"] * R.cut(mask, 2)) * (R.cut(target, 2) - T)
        sampled = 0.3 * R.node(0) - R.node(2) * R.node(2)
        return ((array[cell_slices(g, 0)] + relaxation) + sampled) + (-m["mu"]) * T

    return {
        "drag_u": Case("u", drag_u, lambda R, t: (-0.375) * R.at("u")()),
        "plankton": Case("b", plankton, restate_plankton),
        "one_direction": Case("T", one_direction, lambda R, t: R.ix(R.at("u"))() * R.at("T")()),                           # ℑxᶜᵃᵃ
        "two_directions": Case("v", two_directions, lambda R, t: (-(0.7 * np.cos(3.0 * t))) * R.iy(R.ix(R.at("u")))()),    # ℑxyᶜᶠᵃ = ℑy(ℑx)
        "on_w": Case("w", on_w, restate_on_w),
        "min_max": Case("T", min_max, restate_min_max),
        "coordinates": Case("T", coordinates, lambda R, t: 0.3 * R.node(0) - R.node(2) * R.node(2) + t * 0.5),
        "mixed": Case("T", mixed, restate_mixed),
    }


def interpret(program, parents_of, grid):
    """A pure-Python interpreter of a ForcingProgram over its cells (what the device kernel does per cell, here per array).
    parents_of(leaf) -> the [i, j, k] array a LOAD of that leaf reads (1-D vectors reshaped along their direction)."""
    rng = program.index_range()
    H = (grid.Hx, grid.Hy, grid.Hz)
    vals = []
    with np.errstate(all="ignore"):
        for ins in program.instructions:
            op, off = ins["op"], ins["off"]
            if op == 0:
                f = program.fields[ins["field"]]
                red = getattr(f, "reduced", 0)
                sl = tuple(slice(0, 1) if (red >> d) & 1 else slice(H[d] + rng[d][0] + off[d], H[d] + rng[d][1] + off[d] + 1) for d in range(3))
                v = parents_of(f)[sl]
            elif op == 1:
                v = np.float64(ins["value"])
            elif op == 2:
                raise NotImplementedError("SPACING in a forcing program")
            else:
                a = vals[ins["a"]]
                b = vals[ins["b"]] if op >= 6 else None
                v = (-a if op == 3 else np.abs(a) if op == 4 else np.sqrt(a) if op == 5 else a + b if op == 6 else a - b if op == 7
                     else a * b if op == 8 else a / b if op == 9 else julia_min(a, b) if op == 10 else julia_max(a, b))
            vals.append(v)
    n = tuple(hi - lo + 1 for lo, hi in rng)
    return np.array(np.broadcast_to(vals[-1], n))
