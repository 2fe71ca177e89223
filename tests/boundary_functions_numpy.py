"""NumPy restatement of what a boundary function with field_dependencies is given (continuous_boundary_function.jl:124-157,
interpolation_utils.jl:55-112, interpolation_operators.jl:8-71), written from the reference and independent of the package's lowering:
the tangential node coordinates, and every dependency interpolated -- along the tangential directions only -- to the location of the
conditioned field, indexed at the boundary-normal index I of domain_boundary_indices.  Shared by the host and the GPU tests.

Arrays are parents indexed [i, j, k] with halos; a plane is indexed [a1, a2] over the two tangential directions in the order x, y, z, N
points along each: the layout of ocn_bc.values (values[(a1 - 1) + n1 (a2 - 1)])."""
import numpy as np

P, B, F = "Periodic", "Bounded", "Flat"
SIDES = ("west", "east", "south", "north", "bottom", "top")
LOCS = {"u": 1, "v": 2, "w": 4}  # assumed_field_location: everything else is (Center, Center, Center)

# the grids of the GPU parity test (and of its host twin): the smallest with distinct extents and tangential halos in use.
# The halo (4, 3, 5) needs Nz >= 5 (validate_halo: a halo is at most the size), so that case has five cells along z, not four.
STRETCHED_Z = [-1.0, -0.6, -0.3, -0.1, 0.0]
GRIDS = {
    "ppb": dict(size=(8, 6, 4), x=(0, 3), y=(0, 1), z=STRETCHED_Z, topology=(P, P, B), halo=(3, 3, 3)),
    "ppb_wide": dict(size=(8, 6, 5), x=(0, 3), y=(0, 1), z=[-1.5] + STRETCHED_Z, topology=(P, P, B), halo=(4, 3, 5)),
    "bbb": dict(size=(6, 5, 4), x=(0, 3), y=(0, 1), z=STRETCHED_Z, topology=(B, B, B), halo=(3, 3, 3)),
    "pfb": dict(size=(8, 4), x=(0, 3), z=STRETCHED_Z, topology=(P, F, B), halo=(3, 3)),
}
GRID_SIDES = {"ppb": ("bottom", "top"), "ppb_wide": ("bottom", "top"), "bbb": ("west", "east", "south", "north"), "pfb": ("bottom",)}


def loc_of(name):
    return LOCS.get(name, 0)


def normal(side):
    return SIDES.index(side) >> 1


def tangential(side):
    return tuple(d for d in range(3) if d != normal(side))


def normal_index(grid, side):
    """I - 1 (0-based) of domain_boundary_indices: 1 on the left sides, N on the right ones, whatever the field's location"""
    return grid.size[normal(side)] - 1 if SIDES.index(side) & 1 else 0


def plane(parent, grid, side, off=(0, 0, 0)):
    """parent[i + off, j + off, k + off] over the plane of `side`: N points along each tangential direction, the normal index at I"""
    H, dn = (grid.Hx, grid.Hy, grid.Hz), normal(side)
    sl = [slice(H[d] + off[d], H[d] + off[d] + grid.size[d]) for d in range(3)]
    sl[dn] = H[dn] + normal_index(grid, side)
    return parent[tuple(sl)]


def interpolated(parent, loc_from, loc_to, grid, side):
    """ℑ(i, j, I, grid, field) with ℑ = interpolation_operator(from, to), `to` having Nothing along the normal: the identity there and
    along Flat directions; ℑxᶠ = 0.5 (c[i-1] + c[i]), ℑxᶜ = 0.5 (u[i] + u[i+1]); a double interpolation applies the HIGHER direction
    outside (ℑxy = ℑy ℑx, ℑxz = ℑz ℑx, ℑyz = ℑz ℑy: interpolation_operators.jl:45-58)."""
    dirs = [d for d in tangential(side) if ((loc_from >> d) & 1) != ((loc_to >> d) & 1) and grid.topology[d] != F]

    def shifts(d):
        return (-1, 0) if (loc_to >> d) & 1 else (0, 1)

    def unit(d, s):
        return tuple(s if e == d else 0 for e in range(3))

    def add(a, b):
        return tuple(x + y for x, y in zip(a, b))

    def at(off):
        return plane(parent, grid, side, off)
    if not dirs:
        return at((0, 0, 0)).copy()
    if len(dirs) == 1:
        d = dirs[0]
        return 0.5 * (at(unit(d, shifts(d)[0])) + at(unit(d, shifts(d)[1])))
    inner, outer = dirs  # (ascending: the higher direction is the outer average)

    def inner_average(o):
        return 0.5 * (at(add(o, unit(inner, shifts(inner)[0]))) + at(add(o, unit(inner, shifts(inner)[1]))))
    return 0.5 * (inner_average(unit(outer, shifts(outer)[0])) + inner_average(unit(outer, shifts(outer)[1])))


def coordinates(grid, loc, side):
    """the tangential node coordinates at the field's own location, shaped for broadcasting over [a1, a2]; Flat ones left out"""
    d1, d2 = tangential(side)
    out = []
    for d, shape in ((d1, (-1, 1)), (d2, (1, -1))):
        if grid.topology[d] != F:
            out.append(np.asarray(grid.nodes_1d(d, (loc >> d) & 1))[:grid.size[d]].reshape(shape))
    return out


def expected(func, grid, name, side, parents, dependencies, parameters, time):
    """func(ξ, η, t, *dependencies[, parameters]) on NumPy arrays over the plane [a1, a2]"""
    loc = loc_of(name)
    deps = [interpolated(parents[n], loc_of(n), loc, grid, side) for n in dependencies]
    args = coordinates(grid, loc, side) + [np.float64(time)] + deps + ([] if parameters is None else [parameters])
    d1, d2 = tangential(side)
    with np.errstate(all="ignore"):
        return np.array(np.broadcast_to(func(*args), (grid.size[d1], grid.size[d2])), dtype=np.float64)


def interpret(program, parents_of, grid):
    """A pure-Python interpreter of a BoundaryProgram over its plane (what the device kernel does per point, here per array).
    parents_of(field) -> the [i, j, k] array a LOAD of that field reads (1-D node vectors reshaped along their direction)."""
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
                raise NotImplementedError("SPACING in a boundary program")
            else:
                a = vals[ins["a"]]
                b = vals[ins["b"]] if op >= 6 else None
                v = (-a if op == 3 else np.abs(a) if op == 4 else np.sqrt(a) if op == 5 else a + b if op == 6 else a - b if op == 7
                     else a * b if op == 8 else a / b)
            vals.append(v)
    n = tuple(hi - lo + 1 for lo, hi in rng)
    full = np.array(np.broadcast_to(vals[-1], n))
    return np.squeeze(full, axis=normal(program.side))


# ---- the functions of the parity tests: one body serves the device (symbolic operands) and NumPy (arrays) ------------------------------
def functions(ocn):
    def drag_u(x, y, t, u, v, p):
        return -p["cd"] * ocn.sqrt(u ** 2 + (v + p["V"]) ** 2) * u

    def drag_v(x, y, t, u, v, p):
        return -p["cd"] * ocn.sqrt(u ** 2 + (v + p["V"]) ** 2) * (v + p["V"])

    def bulk(x, y, t, u, v, T, p):
        return -p["c"] * ocn.sqrt(u ** 2 + v ** 2) * (T - p["T0"])

    def coords(x, y, t, w):
        return x * t + y - w
    drag = dict(cd=2.5e-3, V=0.1)
    # name -> (conditioned field, function, field_dependencies, parameters)
    return {"drag_u": ("u", drag_u, ("u", "v"), drag), "drag_v": ("v", drag_v, ("u", "v"), drag),
            "bulk": ("T", bulk, ("u", "v", "T"), dict(c=1.2e-3, T0=0.3)), "coords": ("T", coords, ("w",), None)}


def functions_flat_y(ocn):
    """the same on a (Periodic, Flat, Bounded) grid: the coordinate of the Flat direction is not an argument -- f(x, t, u, v, p)"""
    def drag_u(x, t, u, v, p):
        return -p["cd"] * ocn.sqrt(u ** 2 + (v + p["V"]) ** 2) * u

    def drag_v(x, t, u, v, p):
        return -p["cd"] * ocn.sqrt(u ** 2 + (v + p["V"]) ** 2) * (v + p["V"])

    def bulk(x, t, u, v, T, p):
        return -p["c"] * ocn.sqrt(u ** 2 + v ** 2) * (T - p["T0"])

    def coords(x, t, w):
        return x * t - w
    drag = dict(cd=2.5e-3, V=0.1)
    return {"drag_u": ("u", drag_u, ("u", "v"), drag), "drag_v": ("v", drag_v, ("u", "v"), drag),
            "bulk": ("T", bulk, ("u", "v", "T"), dict(c=1.2e-3, T0=0.3)), "coords": ("T", coords, ("w",), None)}


def functions_on(ocn, grid, side):
    """the four functions with the coordinate arguments of `side` (two, or one where a tangential direction is Flat)"""
    return functions_flat_y(ocn) if grid.topology[1] == F and side in ("bottom", "top") else functions(ocn)


def random_parents(grid, seed, names=("u", "v", "w", "T")):
    """name -> parent array [i, j, k], seeded random everywhere, halos included"""
    rng = np.random.default_rng(seed)
    return {n: rng.uniform(-1.0, 1.0, grid.parent_shape(loc_of(n))) for n in names}
