"""Pins the reference of test_gpu_poisson_accuracy.py itself (tests/poisson_refined.py), on the CPU.

1. Tiny shapes: the refined long-double solution equals a dense long-double solve built from explicit eigenvector matrices (Gaussian
   elimination along a stretched z), to 1e-17 relative, on every topology of {P, B}³ plus PPF, BBF, PBF, one stretched z and one
   screened equation.
2. Every case of the accuracy table: the refinement converges (third correction ≤ 1e-3 of the second) and the oracle's Float64 solve of
   the same inputs is finite and within E_64 ≤ 1e-13 of the refined solution.  This is a condition on the INPUTS: the reference alone is
   inside every bound the GPU test uses.  Measured: third / second correction ≤ 7.7e-4 (the ratio of the two precisions, 2⁻¹¹ = 4.9e-4,
   times the ratio of the two evaluations' constants), E_64 ≤ 371 eps = 8.2e-14 (BBB 512 × 6 × 5 stretched, route (a))."""
import itertools

import numpy as np
import pytest

import poisson_accuracy_cases as PC
import poisson_refined as PR
from helpers import stretched_faces

TINY = [("".join(t), (8, 6, 5), "regular", 0.0) for t in itertools.product("PB", repeat=3)]
TINY += [("PPF", (8, 6, 1), None, 0.0), ("BBF", (8, 6, 1), None, 0.0), ("PBF", (8, 6, 1), None, 0.0)]
TINY += [("PPB", (8, 6, 5), "stretched", 0.0), ("BPB", (8, 6, 5), "stretched", 0.0), ("BBB", (8, 6, 5), "regular", -2.5), ("PPF", (8, 6, 1), None, -2.5)]


@pytest.mark.parametrize("topo,size,z,m", TINY, ids=[f"{t}-{z}-m{m:g}" for t, _, z, m in TINY])
def test_refined_solution_equals_a_dense_long_double_solve(oracle, topo, size, z, m):
    og = oracle.Grid(size, x=PC.EXTENT[0], y=PC.EXTENT[1], z=PC.z_extent(z, size[2]), topology=topo)
    op = PR.Operator(og, m)
    rng = np.random.default_rng(7)
    R = rng.standard_normal(size).astype(PR.LD)
    if m == 0:  # a consistent right-hand side: zero volume-weighted mean
        dz = np.asarray(og.dzc[og.Hz:og.Hz + og.Nz], dtype=PR.LD) if og.dzc is not None else np.ones(og.Nz, dtype=PR.LD)
        R = R - (R * dz).sum() / (dz.sum() * og.Nx * og.Ny)
    phi, sizes = PR.refine(op, R)
    dense = PR.dense_solution(op, R)
    # the dense solution solves the sliced operator (the two are written independently) ...
    res = float(np.abs(R - op.apply(dense)).max() / np.abs(R).max())
    err = float(np.abs(phi - dense).max() / np.abs(dense).max())
    print(f"{topo} {size} {z} m={m}: corrections {sizes}  dense residual {res:.2e}  |refined - dense| {err:.2e}")
    assert res <= 1e-17
    # ... and the refinement reaches it
    assert err <= 1e-17
    if m == 0:
        assert abs(float(phi.mean())) <= 1e-18 * float(np.abs(phi).max())


def test_divergence_ld_is_the_oracles_divergence(oracle):
    """divergence_ld against the oracle's Float64 divᶜᶜᶜ on a stretched (Periodic, Bounded, Bounded) grid"""
    og = oracle.Grid((8, 6, 5), x=(0, 1), y=(0, 2.5), z=stretched_faces(5, 2.0), topology="PBB", halo=(4, 3, 5))
    rng = np.random.default_rng(3)
    U = []
    for loc in PC.LOCS:
        a = og.zeros(loc)
        og.interior(a)[...] = rng.uniform(-1, 1, og.interior(a).shape)
        oracle.fill_halo_regions(og, a, loc)
        U.append(a)
    d = PR.divergence_ld(og, U, 1.0)
    d64 = oracle.divergence(og, *U)
    assert float(np.abs(d - d64).max()) <= 8 * PR.EPS * float(np.abs(d64).max())
    assert abs(float((d * np.asarray(og.dzc[5:10], dtype=PR.LD)).sum())) <= 1e-17 * d.size  # walls and periodicity: the volume integral telescopes


@pytest.mark.parametrize("case", PC.CASES, ids=[c.id for c in PC.CASES])
def test_reference_converges_and_the_float64_solve_is_close(oracle, case):
    ref = PC.reference(oracle, case)
    for route in "ab":
        r = ref[route]
        s = r["sizes"]
        print(f"{case.id} ({route}): corrections {s[0]:.1e} {s[1]:.1e} {s[2]:.1e}  E_64 {r['E64']:.2f} eps  r_64 {r['r64']:.2f} eps")
        assert np.isfinite(r["phi"]).all() and r["finite64"]
        assert s[2] <= 1e-3 * s[1]
        assert r["E64"] * PR.EPS <= 1e-13
