"""Every pipeline the single-device pressure solver can select, at the smallest shape that reaches it: the solver reports the expected
`info()` and solves the discrete Poisson equation.

The column kernel runs lengths 64 / 128 / 256 / 512 and the row kernel 128 / 256 / 512 / 1024 (64 ... 512 for the cosine rows), so the
shapes below are the thresholds between the rocFFT pipelines and the kernels of csrc/colfft.hip / rowfft.hip, per topology.  Operator
and tolerance are those of test_gpu_model.py::test_fft_poisson_all_topologies / test_poisson_laplacian_equals_source (the oracle's
divergence and Laplacian, ‖∇²ϕ − R‖ ≤ √eps ‖R‖); the rows with a stretched x or y, which the oracle does not have, use the numpy
operators of test_gpu_stretched_xy_solvers.py with the same tolerance.

EXPECTED_INFO was produced by `info_table` below running on the commit BEFORE the solver recorded its passes at creation (the values are
that commit's, not the ones of the code under test).

The rows run in ONE fresh child process, one after the other, which is what the selection is a function of besides the grid: rocFFT's real
plans can fail their self test at creation when certain OTHER real plans are alive in the process (csrc/poisson_internal.h, Plan::destroy),
and the handle then falls back to complex plans by design -- `info()` reports r2c = 0 and solves just as well.  Inside the suite's
process which handles of earlier tests are still alive depends on when Python collects them, so the expected table would describe that
history and not the solver."""
import gc
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import from_dev, make_pair, stretched_faces, to_dev

pytestmark = pytest.mark.gpu
LOCS = (1, 2, 4)

# (id, topology, size, z: "regular" | "stretched" | None (Flat), how the solver is made: "model" | "general" | stretched dimension 0 / 1)
ROWS = [
    # ---- periodic x and y
    ("PPP-16", "PPP", (16, 16, 16), "regular", "model"),               # rocFFT 3-D real plans
    ("PPP-16x16x64", "PPP", (16, 16, 64), "regular", "model"),         # fused z column pass
    ("PPP-128x64x64", "PPP", (128, 64, 64), "regular", "model"),       # row / column pipeline; the source wraps
    ("PPF-16x16", "PPF", (16, 16, 1), None, "model"),
    ("PPB-16", "PPB", (16, 16, 16), "regular", "model"),               # rocFFT + Thomas
    ("PPB-16-stretched", "PPB", (16, 16, 16), "stretched", "model"),
    ("PPB-128x64x64", "PPB", (128, 64, 64), "regular", "model"),       # cosine z pass
    ("PPB-128x64x16", "PPB", (128, 64, 16), "regular", "model"),       # custom x / y + Thomas
    ("PPB-128x64x64-stretched", "PPB", (128, 64, 64), "stretched", "model"),
    # ---- any topology
    ("BBB-7", "BBB", (7, 7, 7), "regular", "model"),                   # complex lines
    ("BBB-16", "BBB", (16, 16, 16), "regular", "model"),               # all-real, rocFFT lines, row pairs
    ("BBB-64", "BBB", (64, 64, 64), "regular", "model"),               # all-real, one-pass column and row transforms
    ("BBB-64x64x16-stretched", "BBB", (64, 64, 16), "stretched", "model"),  # row modes forward / inverse around the real Thomas sweep
    ("BBF-64x64", "BBF", (64, 64, 1), None, "model"),
    ("PBB-16", "PBB", (16, 16, 16), "regular", "model"),               # packed, real x plans
    ("PBB-64", "PBB", (64, 64, 64), "regular", "model"),               # packed, row kernel
    ("PBB-16-stretched", "PBB", (16, 16, 16), "stretched", "model"),
    ("PBP-16x64x16", "PBP", (16, 64, 16), "regular", "model"),
    ("BPB-16x64x64", "BPB", (16, 64, 64), "regular", "model"),         # complex, column lines
    ("BPP-16", "BPP", (16, 16, 16), "regular", "model"),
    ("PBF-128x6", "PBF", (128, 6, 1), None, "model"),
    ("PPP-16-general", "PPP", (16, 16, 16), "regular", "general"),
    # ---- stretched x or y
    ("BPP-16-xstretched", "BPP", (16, 16, 16), "regular", 0),
    ("PBP-16-ystretched", "PBP", (16, 16, 16), "regular", 1),
    ("BBB-64-xstretched", "BBB", (64, 64, 64), "regular", 0),
]

# id -> (kind, r2c, direct_out) of ocn_poisson_info
EXPECTED_INFO = {
    "PPP-16": (0, 1, 1),
    "PPP-16x16x64": (0, 1, 2),
    "PPP-128x64x64": (0, 1, 7),
    "PPF-16x16": (0, 1, 0),
    "PPB-16": (1, 1, 0),
    "PPB-16-stretched": (1, 1, 0),
    "PPB-128x64x64": (1, 1, 13),
    "PPB-128x64x16": (1, 1, 5),
    "PPB-128x64x64-stretched": (1, 1, 5),
    "BBB-7": (2, 0, 0),
    "BBB-16": (2, 0, 0),
    "BBB-64": (2, 0, 0),
    "BBB-64x64x16-stretched": (3, 0, 0),
    "BBF-64x64": (2, 0, 0),
    "PBB-16": (2, 0, 0),
    "PBB-64": (2, 0, 0),
    "PBB-16-stretched": (3, 0, 0),
    "PBP-16x64x16": (2, 0, 0),
    "BPB-16x64x64": (2, 0, 0),
    "BPP-16": (2, 0, 0),
    "PBF-128x6": (2, 0, 0),
    "PPP-16-general": (2, 0, 0),
    "BPP-16-xstretched": (4, 0, 0),
    "PBP-16-ystretched": (5, 0, 0),
    "BBB-64-xstretched": (4, 0, 0),
}


def _product_grid(ocn, topo, size, z, how):
    """the grid of a row with a stretched x / y (the others come from helpers.make_pair)"""
    import test_gpu_stretched_xy_solvers as TS
    names = {"P": TS.P, "B": TS.B, "F": TS.F}
    faces = -stretched_faces(size[how], 1.0)[::-1]  # increasing, refined towards the upper end
    ext = [(0, 1), (0, 2.5), (0, 4)]
    ext[how] = np.asarray(faces, dtype=np.float64)
    kw = {n: e for n, e in zip("xyz", ext)}
    return ocn.RectilinearGrid(ocn.GPU(), size=size, topology=tuple(names[t] for t in topo), **kw)


def make_solver(ocn, pg, how):
    if how == "general":
        return ocn.FFTBasedPoissonSolver(pg, general=True)
    return ocn.nonhydrostatic_pressure_solver(pg)  # (a stretched x / y: the Fourier-tridiagonal solver along it)


def solve_row(O, ocn, row):
    """(info, ∇²ϕ, R) of one row: R = div(U) of a random velocity, ϕ from compute_source_term + solve"""
    _, topo, size, z, how = row
    rng = np.random.default_rng(1234)
    if isinstance(how, int):
        import test_gpu_stretched_xy_solvers as TS
        pg = _product_grid(ocn, topo, size, z, how)
        U = TS._velocity_parents(pg, rng)
        solver, phi = TS._solve_for_pressure(ocn, pg, U, 1.0)
        return solver.info(), TS._laplacian(pg, phi), TS._divergence(pg, U)
    zext = None if z is None else stretched_faces(size[2], 2.0) if z == "stretched" else (0, 4)
    og, pg = make_pair(O, ocn, size, topo, x=(0, 1), y=(0, 2.5), z=zext)
    U = []
    for loc in LOCS:
        a = og.zeros(loc)
        og.interior(a)[...] = rng.uniform(-1, 1, og.interior(a).shape)
        if topo[{1: 0, 2: 1, 4: 2}[loc]] == "F":
            a[...] = 0
        O.fill_halo_regions(og, a, loc)
        U.append(a)
    R = O.divergence(og, *U)
    solver = make_solver(ocn, pg, how)
    phi = ocn.CenterField(pg)
    ocn.solve_for_pressure(phi, solver, 1.0, [to_dev(ocn, pg, l, a) for l, a in zip(LOCS, U)])
    ocn.sync_device()
    p = np.asfortranarray(from_dev(phi))
    O.fill_halo_regions(og, p, 0)
    return solver.info(), O.laplacian(og, p), R


def all_rows(O, ocn):
    """id -> {info: [kind, r2c, direct_out], residual: ‖∇²ϕ − R‖, norm: ‖R‖}, the rows in order (each solver is gone before the next is made)"""
    out = {}
    for row in ROWS:
        i, lap, R = solve_row(O, ocn, row)
        out[row[0]] = {"info": [i["kind"], int(i["r2c"]), i["direct_out"]], "residual": float(np.linalg.norm(lap - R)), "norm": float(np.linalg.norm(R))}
        gc.collect()
    return out


def info_table(O, ocn):
    """EXPECTED_INFO as this library reports it"""
    return {k: tuple(v["info"]) for k, v in all_rows(O, ocn).items()}


@pytest.fixture(scope="module")
def results(ocn, tmp_path_factory):
    """all_rows() of a fresh process (this file run as a script)"""
    out = tmp_path_factory.mktemp("poisson_pipelines") / "rows.json"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, f"child exited {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    with open(out) as f:
        return json.load(f)


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_pipeline_reports_its_selection_and_solves(results, row):
    got = results[row[0]]
    bound = np.sqrt(np.finfo(float).eps) * got["norm"]
    print(f"{row[0]}: info {tuple(got['info'])}  residual {got['residual']:.3e}  bound {bound:.3e}")
    assert tuple(got["info"]) == EXPECTED_INFO[row[0]]
    assert got["norm"] > 0 and got["residual"] <= bound


if __name__ == "__main__":
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, ROOT)
    os.environ.setdefault("OMP_NUM_THREADS", "8")  # (under pytest both are inherited from conftest.py)
    os.environ.setdefault("OMP_WAIT_POLICY", "passive")
    import oceananigans_jl_amd
    from oracle import oracle
    oracle.lib()
    with open(sys.argv[1], "w") as f:
        json.dump(all_rows(oracle, oceananigans_jl_amd), f)
