"""Case tables and helpers of the kernel-level tests of the split-explicit substep loop (csrc/kernels.hip: the plain pair of kernels, the
temporally blocked LDS kernel, the AB3 variant and the slab-x variant of the blocked kernel).  No GPU is needed to import this:
tests/test_host_split_explicit_cases.py checks the tables and their oracle results, tests/test_gpu_split_explicit_substeps.py runs the
kernels on them.

The expected result of every case is oracle/hydrostatic.py: iterate_split_explicit (or _ab3) on the GLOBAL periodic arrays; everything in
kernels.hip is compiled without contraction, so every comparison is bit for bit.

What the shapes are for (the blocked kernel: 64 x 16 centre, SH = 4 substeps per launch, a 72 x 24 patch that wraps on load):
  * n = 1 .. 9 covers every residue of n mod 4, n < 4 (one launch that is both the first and the last), n = 4 (exactly one full launch),
    n = 8 (two full launches) and the short tail launches;
  * (1, 1) and (3, 2): Nx, Ny below SH, the patch wraps the domain several times;
  * 63 / 64 / 65 and 15 / 16 / 17: one cell either side of the tile edges; (129, 33): three workgroups each way;
  * (16, 12) at n = 21: six launches, the ping-pong between the state and the workspace three times over."""
import functools

import numpy as np

GRAV = 9.80665
DX, DY = 125.0, 80.0      # unequal: a swapped metric shows
DEPTH = 40.0              # H = Lz
DTAU = 0.5 * min(DX, DY) / np.sqrt(GRAV * DEPTH)   # gravity-wave CFL 0.32 in x, 0.5 in y: (0.32² + 0.5²) < 1, the forward-backward scheme is stable

# ---- single rank: (Nx, Ny, n, halo of the planes) -----------------------------------------------------------------------------------
# halos 1 and 3 alternate where the size allows 3 (a halo may not exceed the size)
SWEEP_SIZE = (65, 17)
SWEEP = [SWEEP_SIZE + (n, 3 if n % 2 else 1) for n in range(1, 10)]
EDGE_SIZES = [((1, 1), 1), ((3, 2), 1), ((63, 15), 3), ((64, 16), 1), ((65, 17), 1), ((129, 33), 3)]
EDGES = [size + (n, halo) for size, halo in EDGE_SIZES for n in (3, 7)]
LONG = [(16, 12, 21, 3)]
SINGLE_RANK_CASES = SWEEP + EDGES + LONG
AB3_CASES = SWEEP + [(3, 2, n, 1) for n in range(1, 10)]

# ---- slab-x ranks: (nx per rank, Ny, n, ranks R, halo of the model's planes) -----------------------------------------------------
SLAB_CASES = [
    (5, 3, 5, 2, 3),       # n == nx, the cap of the C ABI: the strips are the whole interior
    (3, 1, 3, 1, 1),       # a rank that is its own neighbour, Ny = 1
    (130, 33, 3, 2, 3),    # n < 4: the clamped loads of the first launch; 3 workgroups in x, 3 in y
    (60, 17, 9, 2, 1),     # owned widths 70 -> 62 -> 60: two workgroups in x, then one
    (70, 5, 30, 3, 3),     # owned widths 122 -> ... -> 70 over eight launches
    (16, 12, 8, 4, 3),     # the shape of the distributed model test
]


def case_id(case):
    return "-".join(str(c) for c in case)


def owned_widths(nx, n, SH=4):
    """the owned x range nx + 2 (n - done) of each launch of the slab path (run_blocked_substeps in kernels.hip)"""
    done, out = 0, []
    for m0 in range(0, n, SH):
        done += min(SH, n - m0)
        out.append(nx + 2 * (n - done))
    return out


def _readonly(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def fields(Nx, Ny):
    """interior arrays [i, j] of a case, all different: η, U, V of O(1e-2); Gᵁ, Gⱽ of O(1e-5).  Read-only: shared between tests."""
    rng = np.random.default_rng([Nx, Ny, 7])
    eta, U, V = (1e-2 * rng.uniform(-1, 1, (Nx, Ny)) for _ in range(3))
    GU, GV = (1e-5 * rng.uniform(-1, 1, (Nx, Ny)) for _ in range(2))
    return _readonly(eta, U, V, GU, GV)


@functools.lru_cache(maxsize=None)
def weights(n):
    """n distinct random positives normalised to 1: a shifted index w[m0 + q] shows"""
    w = np.random.default_rng([n, 11]).uniform(0.1, 1.0, n)
    assert len(set(w)) == n
    return _readonly(w / w.sum())[0]


@functools.lru_cache(maxsize=None)
def reference(Nx, Ny, n, ab3=False):
    """(η̄, Ū, V̄) of the oracle on the global periodic (Nx, Ny) arrays; the state after the loop is these averages.  Read-only."""
    from oracle import hydrostatic as Hy
    eta, U, V, GU, GV = fields(Nx, Ny)
    eta, U, V = eta.copy(), U.copy(), V.copy()
    etab, Ub, Vb = (np.zeros((Nx, Ny)) for _ in range(3))
    args = (eta, U, V, etab, Ub, Vb, GU, GV, DTAU, weights(n), GRAV, DEPTH, DX, DY)
    if ab3:
        Hy.iterate_split_explicit_ab3(*args, Hy.ab3_coefficients())
    else:
        Hy.iterate_split_explicit(*args)
    return _readonly(etab, Ub, Vb)


def place(interior, hx, hy, fill=np.nan):
    """the interior array [i, j] in a C-ordered [y, x] plane with halos (hx, hy); `fill` (NaN) everywhere else"""
    Nx, Ny = interior.shape
    plane = np.full((Ny + 2 * hy, Nx + 2 * hx), fill)
    plane[hy:hy + Ny, hx:hx + Nx] = interior.T
    return plane


def interior_of(plane, Nx, Ny, hx, hy):
    """the inverse of place: the interior [i, j] of a [y, x] plane"""
    return plane[hy:hy + Ny, hx:hx + Nx].T


def grid_arguments(Nx, Ny, halo):
    """keywords of the (Nx, Ny, 1) RectilinearGrid of a case: spacings DX, DY, depth DEPTH, Hz = 1"""
    return dict(size=(Nx, Ny, 1), x=(0.0, DX * Nx), y=(0.0, DY * Ny), z=(-DEPTH, 0.0), topology=("Periodic", "Periodic", "Bounded"),
                halo=(halo, halo, 1))
