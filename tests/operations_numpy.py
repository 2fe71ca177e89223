"""NumPy restatement of the operation trees, ComputedField, Average and Integral (oceananigans.jl_amd/operations.py), written from the
reference and independent of the package's lowering:

  location of a binary operation         src/AbstractOperations/binary_operations.jl:47-52, 104-130
  at                                     at.jl; binary_operations.jl:32, unary_operations.jl:37, derivatives.jl:39
  derivatives                            src/AbstractOperations/derivatives.jl:47-107, src/Operators/derivative_operators.jl (δ / Δ)
  interpolation                          src/Operators/interpolation_operators.jl:8-15, composed in the order of :45-71
  Average, Integral and their metric     src/AbstractOperations/metric_field_reductions.jl:11-20, 41-61, 108-113

Expressions are nested tuples: ("f", name), a number, ("+", a, b), ("-", a, b), ("*", a, b), ("/", a, b), ("neg", a), ("abs", a),
("sqrt", a), ("sq", a), ("cube", a), ("ddx", a), ("ddy", a), ("ddz", a), ("at", location, a).  Locations are 3-tuples out of "C", "F", None.
Fields are parent arrays indexed [i, j, k], halos included (extent 1 and no halo along a reduced direction, whose location is None), so a
halo read here is the same read as on the device.  Every step is its own IEEE operation, in the reference's order.
"""
import math

import numpy as np

EPS = 2.0 ** -53  # unit roundoff of Float64


class Grid:
    """What the restatement reads of a grid: sizes, halos, topology, spacings (dzc / dzf: element 0 <-> k = 1 - Hz, or None)"""

    def __init__(self, g):
        self.N, self.H, self.topo = (g.Nx, g.Ny, g.Nz), (g.Hx, g.Hy, g.Hz), tuple(g.topology)
        self.d = (g.dx, g.dy, g.dz)
        self.dzc, self.dzf = g._dzc_host, g._dzf_host

    def interior(self, loc):
        return tuple(1 if self.topo[d] == "Flat" else self.N[d] + (1 if loc[d] == "F" and self.topo[d] == "Bounded" else 0) for d in range(3))


class Leaf:
    def __init__(self, parent, loc):
        self.parent, self.loc = parent, tuple(loc)


class Node:
    def __init__(self, kind, loc, args, dim=None, lder=None):
        self.kind, self.loc, self.args, self.dim, self.lder = kind, tuple(loc), args, dim, lder


def _loc(x):
    return x.loc if isinstance(x, Node) else (None, None, None)


def _choose(la, lb, lc):
    if la is not None and la == lb:
        return la
    if la is not None and lb is None:
        return la
    if la is None and lb is not None:
        return lb
    return lc


def place(e, fields, at=None):
    """the tree with its locations; `at`: the location an enclosing ("at", ...) asks for"""
    if not isinstance(e, tuple):
        return float(e)
    k = e[0]
    if k == "f":
        return Node("f", fields[e[1]].loc, (e[1],))
    if k == "at":
        return place(e[2], fields, tuple(e[1]))
    if k in ("+", "-", "*", "/"):
        a, b = place(e[1], fields, at), place(e[2], fields, at)
        la, lb = _loc(a), _loc(b)
        lc = at if at is not None else (la if isinstance(a, Node) else lb)
        return Node(k, tuple(_choose(la[d], lb[d], lc[d]) for d in range(3)), (a, b))
    if k in ("neg", "abs", "sqrt", "sq", "cube"):
        a = place(e[1], fields, at)
        return Node(k, at if at is not None else a.loc, (a,))
    if k in ("ddx", "ddy", "ddz"):
        dim = "xyz".index(k[2])
        a = place(e[1], fields, None)  # at(loc, derivative) keeps the argument where it is
        l = list(a.loc)
        l[dim] = "C" if l[dim] == "F" else "F"
        return Node("dd", at if at is not None else tuple(l), (a,), dim=dim, lder=tuple(l))
    raise ValueError(k)


def location(e, fields):
    return _loc(place(e, fields))


def _sh(off, d, s):
    o = list(off)
    o[d] += s
    return tuple(o)


class Evaluator:
    """values over the interior of the tree's location: arrays of shape `n`, element [i, j, k] <-> 0-based interior index"""

    def __init__(self, grid, fields, n):
        self.g, self.fields, self.n = grid, fields, n

    def leaf(self, name, off):
        f, g = self.fields[name], self.g
        sl = []
        for d in range(3):
            if f.loc[d] is None or g.topo[d] == "Flat":
                sl.append(slice(0, 1))  # the one element: broadcast
            else:
                lo = g.H[d] + off[d]
                assert lo >= 0 and lo + self.n[d] <= f.parent.shape[d], "the tree reads beyond the halo"
                sl.append(slice(lo, lo + self.n[d]))
        return f.parent[tuple(sl)]

    def spacing(self, d, face, off):
        g = self.g
        if d < 2 or g.dzc is None:
            return g.d[d]
        v = (g.dzf if face else g.dzc)
        lo = g.H[2] + off[2]
        return v[lo:lo + self.n[2]].reshape(1, 1, -1)

    def interp(self, fn, lf, lt, off):
        need = tuple(d for d in range(3) if lf[d] is not None and lt[d] is not None and lf[d] != lt[d] and self.g.topo[d] != "Flat")

        def two_point(g, d):
            o1, o2 = (-1, 0) if lt[d] == "F" else (0, 1)
            return lambda o: 0.5 * (g(_sh(o, d, o1)) + g(_sh(o, d, o2)))
        x, y, z = (lambda g: two_point(g, 0)), (lambda g: two_point(g, 1)), (lambda g: two_point(g, 2))
        if need == ():
            h = fn
        elif need == (0,):
            h = x(fn)
        elif need == (1,):
            h = y(fn)
        elif need == (2,):
            h = z(fn)
        elif need == (0, 1):
            h = y(x(fn))        # ℑxy = ℑy(ℑx f)
        elif need == (0, 2):
            h = z(x(fn))        # ℑxz = ℑz(ℑx f)
        elif need == (1, 2):
            h = z(y(fn))        # ℑyz = ℑz(ℑy f)
        else:
            h = x(y(z(fn)))     # ℑxyz = ℑx(ℑy(ℑz f))
        return h(off)

    def ev(self, n, off):
        if not isinstance(n, Node):
            return np.float64(n)
        k = n.kind
        if k == "f":
            return self.leaf(n.args[0], off)
        if k in ("+", "-", "*", "/"):
            a, b = n.args
            va = self.interp(lambda o: self.ev(a, o), _loc(a), n.loc, off) if isinstance(a, Node) else np.float64(a)
            vb = self.interp(lambda o: self.ev(b, o), _loc(b), n.loc, off) if isinstance(b, Node) else np.float64(b)
            return va + vb if k == "+" else va - vb if k == "-" else va * vb if k == "*" else va / vb
        if k == "dd":
            return self.interp(lambda o: self.derivative(n, o), n.lder, n.loc, off)
        a = n.args[0]
        return self.interp(lambda o: self.unary(k, self.ev(a, o)), a.loc, n.loc, off)

    @staticmethod
    def unary(k, x):
        if k == "neg":
            return -x
        if k == "abs":
            return np.abs(x)
        if k == "sqrt":
            return np.sqrt(x)
        if k == "sq":
            return x * x
        return (x * x) * x

    def derivative(self, n, off):
        d, a = n.dim, n.args[0]
        if self.g.topo[d] == "Flat":
            return np.float64(0.0)
        if n.lder[d] == "F":   # δᶠ c = c[i] - c[i-1], over Δᶠ[i]
            return (self.ev(a, off) - self.ev(a, _sh(off, d, -1))) / self.spacing(d, True, off)
        return (self.ev(a, _sh(off, d, 1)) - self.ev(a, off)) / self.spacing(d, False, off)


def pointwise(e, fields, grid):
    """(location, values over the interior of that location)"""
    tree = place(e, fields)
    n = grid.interior(tree.loc)
    with np.errstate(all="ignore"):
        v = Evaluator(grid, fields, n).ev(tree, (0, 0, 0))
    return tree.loc, np.array(np.broadcast_to(v, n))


def reduction_terms(kind, e, dims, fields, grid):
    """(location of the operand, per-cell terms tᵢ with the metric where it applies, divisor W)"""
    loc, a = pointwise(e, fields, grid)
    n = a.shape
    stretched = grid.dzc is not None
    weighted = kind == "Integral" or (3 in dims and stretched)
    if not weighted:
        return loc, a, float(np.prod([n[d - 1] for d in dims]))
    m = None
    for d in sorted(dims):  # Δx; Δy; Δz; Az = Δx Δy; Ay = Δx Δz; Ax = Δy Δz; V = Az Δz
        if d == 3 and stretched:
            s = (grid.dzf if loc[2] == "F" else grid.dzc)[grid.H[2]:grid.H[2] + n[2]].reshape(1, 1, -1)
        else:
            s = np.float64(grid.d[d - 1])
        m = s if m is None else m * s
    t = a * m
    if kind == "Integral":
        return loc, t, 1.0
    mm = np.broadcast_to(m, n)
    one = tuple(slice(None) if (d + 1) in dims else slice(0, 1) for d in range(3))
    return loc, t, math.fsum(mm[one].ravel().tolist())


def reduce_exact(t, dims, W):
    """per output element: (fsum of the terms / W, number of terms, Σ|tᵢ|); reduced directions keep extent 1"""
    kept = [d for d in range(3) if (d + 1) not in dims]
    red = [d for d in range(3) if (d + 1) in dims]
    shape = tuple(1 if (d + 1) in dims else t.shape[d] for d in range(3))
    rows = np.transpose(t, kept + red).reshape(int(np.prod([t.shape[d] for d in kept], dtype=np.int64)), -1)
    exact = np.array([math.fsum(r) for r in rows.tolist()]) / W
    sabs = np.array([math.fsum(r) for r in np.abs(rows).tolist()])
    back = [t.shape[d] for d in kept]
    exact = exact.reshape(back) if back else exact.reshape(())
    sabs = sabs.reshape(back) if back else sabs.reshape(())
    # kept axes are in increasing order already: put the unit axes back
    return exact.reshape(shape), rows.shape[1], sabs.reshape(shape)


def reduction_bound(n_terms, sabs, W):
    """|computed - exact| <= (n + 8) ε Σ|tᵢ| / W: the first-order bound (n - 1) ε Σ|tᵢ| of a sum of n terms added in ANY order, plus a few
    roundings for the division, the divisor and the rounding of the exact value itself"""
    return (n_terms + 8) * EPS * sabs / W


def interpret_program(program, parents, grid):
    """A pure-Python interpreter of a lowered program (oceananigans.jl_amd.operations.Program) over the interior of its location: what the
    device kernel does per cell, here per array.  `parents[q]`: parent array [i, j, k] of program.fields[q]."""
    n = program.interior_size()
    g = Grid(grid)
    vals = []
    with np.errstate(all="ignore"):
        for ins in program.instructions:
            op, off = ins["op"], ins["off"]
            if op == 0:
                f = program.fields[ins["field"]]
                red = getattr(f, "reduced", 0)
                sl = tuple(slice(0, 1) if (red >> d) & 1 else slice(g.H[d] + off[d], g.H[d] + off[d] + n[d]) for d in range(3))
                v = parents[ins["field"]][sl]
            elif op == 1:
                v = np.float64(ins["value"])
            elif op == 2:
                kind = ins["field"]
                if kind < 2 or g.dzc is None:
                    v = np.float64(g.d[min(kind, 2)])
                else:
                    lo = g.H[2] + off[2]
                    v = (g.dzc if kind == 2 else g.dzf)[lo:lo + n[2]].reshape(1, 1, -1)
            else:
                a = vals[ins["a"]]
                b = vals[ins["b"]] if op >= 6 else None
                v = (-a if op == 3 else np.abs(a) if op == 4 else np.sqrt(a) if op == 5 else a + b if op == 6 else a - b if op == 7
                     else a * b if op == 8 else a / b)
            vals.append(v)
    return np.array(np.broadcast_to(vals[-1], n))
