"""Shared by tests/test_host_operations.py and tests/test_gpu_operations.py: every expression is written twice, once with the package's
public interface and once in the tuple language of the restatement (tests/operations_numpy.py)."""
import numpy as np

import operations_numpy as ON

P, B, F = "Periodic", "Bounded", "Flat"
CCC = ("C", "C", "C")
LOCS = {"u": ("F", "C", "C"), "v": ("C", "F", "C"), "w": ("C", "C", "F"), "c": CCC}
_f = {n: ("f", n) for n in LOCS}


def pointwise_cases(ocn, f):
    """name -> (tree of the package, tree of the restatement); f: dict of the package's fields u, v, w, c"""
    u, v, w, c = f["u"], f["v"], f["w"], f["c"]
    U, V, W, Cc = _f["u"], _f["v"], _f["w"], _f["c"]
    C3 = (ocn.Center,) * 3
    return {
        "w*u": (w * u, ("*", W, U)),
        "u*w": (u * w, ("*", U, W)),
        "ke": (0.5 * (u ** 2 + v ** 2 + w ** 2), ("*", 0.5, ("+", ("+", ("sq", U), ("sq", V)), ("sq", W)))),
        "zeta": (ocn.ddx(v) - ocn.ddy(u), ("-", ("ddx", V), ("ddy", U))),
        "eta": (ocn.ddz(u) - ocn.ddx(w), ("-", ("ddz", U), ("ddx", W))),
        "sqrtabs": (ocn.sqrt(ocn.abs(c)) / (1 + c * c), ("/", ("sqrt", ("abs", Cc)), ("+", 1.0, ("*", Cc, Cc)))),
        "at_ccc": (ocn.at(C3, u * u + w * w), ("at", CCC, ("+", ("*", U, U), ("*", W, W)))),
        "ddzddz": (ocn.ddz(ocn.ddz(c)), ("ddz", ("ddz", Cc))),
    }


def reduction_operands(ocn, f):
    """name -> (operand of the package, of the restatement); "u'" is added by the caller (it needs a computed mean)"""
    u, w, c = f["u"], f["w"], f["c"]
    return {"c": (c, _f["c"]), "u": (u, _f["u"]), "w": (w, _f["w"]), "w*u": (w * u, ("*", _f["w"], _f["u"]))}


DIMS = [(1,), (2,), (3,), (1, 2), (1, 3), (2, 3), (1, 2, 3)]

GRIDS = {
    "stretched_70x3x5": dict(size=(70, 3, 5), x=(0, 7), y=(0, 1.5), z=[-1.0, -0.7, -0.45, -0.25, -0.1, 0.0], topology=(P, P, B)),
    "walls_5x67x4": dict(size=(5, 67, 4), x=(0, 1), y=(-2, 2), z=(0, 0.5), topology=(B, B, B)),
    "flat_130x9": dict(size=(130, 9), x=(0, 13), z=(-1, 0), topology=(P, F, B)),
    "blocks_96x80x40": dict(size=(96, 80, 40), x=(0, 1), y=(0, 2), z=(-1, 0), topology=(P, P, B)),
}


def mask_of(loc):
    return sum(1 << d for d in range(3) if loc[d] == "F")


def random_parents(grid, seed):
    """name -> parent array [i, j, k] of u, v, w, c, seeded random, halos included"""
    rng = np.random.default_rng(seed)
    return {n: rng.uniform(-1.0, 1.0, grid.parent_shape(mask_of(l))) for n, l in LOCS.items()}


def leaves(parents):
    return {n: ON.Leaf(a, LOCS[n]) for n, a in parents.items()}


def location_names(ocn, location):
    return tuple(None if l is None else ("F" if l is ocn.Face else "C") for l in location)


# the reference's own test of the reductions (test/test_field_scans.jl:19-70, 154-174; tests/golden/field_scans_2x2x2.json)
def scans_grid(pkg, arch, stretched):
    return pkg.RectilinearGrid(arch, size=(2, 2, 2), x=(0, 2), y=(0, 2), z=[0, 1, 2] if stretched else (0, 2), topology=(P, P, B),
                               halo=(1, 1, 1))


def trilinear_parents(grid):
    out = {}
    for n in ("c", "w"):
        loc = mask_of(LOCS[n])
        x, y, z = (grid.nodes_1d(d, (loc >> d) & 1, with_halos=True) for d in range(3))
        a = x.reshape(-1, 1, 1) + y.reshape(1, -1, 1) + z.reshape(1, 1, -1)
        assert a.shape == grid.parent_shape(loc)
        out[n] = a
    return out


def check_scans(golden, value):
    """value(kind, name, dims) -> array with unit extents along the reduced directions"""
    for name, key in (("c", "T"), ("w", "w")):
        A = golden["Average"][key]
        a123, a12, a1 = value("Average", name, (1, 2, 3)), value("Average", name, (1, 2)), value("Average", name, (1,))
        assert np.allclose(a123.ravel(), [A["dims_123"]], rtol=1e-14, atol=0)
        assert np.allclose(a12[0, 0, :], A["dims_12"], rtol=1e-14, atol=0)
        assert np.allclose(a1[0, :, :], A["dims_1"], rtol=1e-14, atol=0)
        R = golden["Integral_over_Average"][key]
        assert np.allclose(value("Integral", name, (1,)), R["dims_1"] * a1, rtol=1e-14, atol=0)
        assert np.allclose(value("Integral", name, (1, 2)), R["dims_12"] * a12, rtol=1e-14, atol=0)
        assert np.allclose(value("Integral", name, (1, 2, 3)), R["dims_123"] * a123, rtol=1e-14, atol=0)


# four malformed programs: a change to the three-instruction program of test_host_operations._program, and the message it earns
MALFORMED = {
    "forward operand": (dict(i2_b=2), "not an earlier instruction"),
    "register out of range": (dict(i1_reg=2), "register 2 outside"),
    "field out of range": (dict(i1_field=1), "field 1 outside"),
    "offset beyond the halo": (dict(i0_di=4), "beyond the halo"),
}
