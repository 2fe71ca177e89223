"""The inputs of tests/test_gpu_split_explicit_substeps.py, checked before anyone needs a GPU: the oracle alone on every case of
tests/split_explicit_cases.py, what the tables are meant to contain, and the refusals of the C entry points of the substep loop (their
pointers are never dereferenced)."""
import ctypes as C

import numpy as np
import pytest

import split_explicit_cases as SC

SINGLE = [(c[:3], False) for c in SC.SINGLE_RANK_CASES] + [(c[:3], True) for c in SC.AB3_CASES]
SLABS = [((nx * R, Ny, n), False) for nx, Ny, n, R, _ in SC.SLAB_CASES]


@pytest.mark.parametrize("size_n,ab3", sorted(set(SINGLE + SLABS)), ids=lambda v: SC.case_id(v) if isinstance(v, tuple) else ("ab3" if v else "fb"))
def test_the_oracle_result_of_every_case_is_a_sane_input(size_n, ab3):
    """finite, a stable run (max|η̄| < 1 from η of O(1e-2)) and not trivially zero"""
    Nx, Ny, n = size_n
    etab, Ub, Vb = SC.reference(Nx, Ny, n, ab3)
    for a in (etab, Ub, Vb):
        assert a.shape == (Nx, Ny) and np.isfinite(a).all()
    assert np.abs(etab).max() < 1 and np.abs(Ub).max() > 0 and np.abs(Vb).max() > 0


def test_fields_and_weights_are_what_the_cases_need():
    eta, U, V, GU, GV = SC.fields(65, 17)
    planes = (eta, U, V, GU, GV)
    for a in range(5):
        for b in range(a + 1, 5):
            assert not np.array_equal(planes[a], planes[b])
    assert all(1e-3 < np.abs(a).max() <= 1e-2 for a in (eta, U, V)) and all(1e-6 < np.abs(a).max() <= 1e-5 for a in (GU, GV))
    assert SC.DX != SC.DY and SC.DTAU == 0.5 * 80.0 / np.sqrt(SC.GRAV * 40.0)
    for n in range(1, 31):
        w = SC.weights(n)
        assert len(w) == n and len(set(w)) == n and (w > 0).all() and abs(w.sum() - 1) < 1e-14
    with pytest.raises(ValueError):
        eta[0, 0] = 1.0   # shared between tests: read-only


def test_the_sweep_covers_every_launch_shape():
    ns = [n for _, _, n, _ in SC.SWEEP]
    assert ns == list(range(1, 10)) and all(c[:2] == (65, 17) for c in SC.SWEEP)
    assert {n % 4 for n in ns} == {0, 1, 2, 3} and any(n < 4 for n in ns) and 4 in ns
    sizes = {c[:2] for c in SC.EDGES}
    assert sizes == {(1, 1), (3, 2), (63, 15), (64, 16), (65, 17), (129, 33)}
    assert all({n for Nx, Ny, n, _ in SC.EDGES if (Nx, Ny) == s} == {3, 7} for s in sizes)
    assert (16, 12, 21) in {c[:3] for c in SC.SINGLE_RANK_CASES}
    halos = {h for *_, h in SC.SINGLE_RANK_CASES}
    assert halos == {1, 3} and all(h <= min(Nx, Ny) for Nx, Ny, _, h in SC.SINGLE_RANK_CASES + SC.AB3_CASES)
    assert {c[:3] for c in SC.AB3_CASES} == {(65, 17, n) for n in range(1, 10)} | {(3, 2, n) for n in range(1, 10)}


def test_the_slab_cases_are_what_their_comments_say():
    assert {c[:4] for c in SC.SLAB_CASES} == {(5, 3, 5, 2), (3, 1, 3, 1), (130, 33, 3, 2), (60, 17, 9, 2), (70, 5, 30, 3), (16, 12, 8, 4)}
    for nx, Ny, n, R, halo in SC.SLAB_CASES:
        assert 1 <= n <= nx and R >= 1 and halo <= min(nx, Ny)
    assert any(n == nx for nx, _, n, _, _ in SC.SLAB_CASES) and any(n < 4 for _, _, n, _, _ in SC.SLAB_CASES)
    assert any(R == 1 for *_, R, _ in SC.SLAB_CASES)
    assert SC.owned_widths(60, 9) == [70, 62, 60]          # 64-wide workgroups: two, then one
    assert SC.owned_widths(130, 3) == [130]                # the first launch is the last: its patch reaches 4 cells past a halo of 3
    w = SC.owned_widths(70, 30)
    assert w[0] == 122 and w[-1] == 70 and len(w) == 8 and all(a > b for a, b in zip(w, w[1:]))


def test_place_and_interior_of():
    a = np.arange(6.0).reshape(3, 2)
    p = SC.place(a, 3, 1)
    assert p.shape == (2 + 2, 3 + 6) and p.flags.c_contiguous and np.isnan(p).sum() == p.size - 6
    assert p[1, 3] == a[0, 0] and p[2, 3] == a[0, 1] and p[1, 5] == a[2, 0]     # [y, x]
    np.testing.assert_array_equal(SC.interior_of(p, 3, 2, 3, 1), a)


# ---- the C entry points refuse what the launchers cannot run --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pkg():
    import oceananigans_jl_amd as ocn
    return ocn


def test_c_entry_points_refuse_substep_counts_they_cannot_run(pkg):
    """the slab path needs n <= Nx (the extended halo must not reach past the neighbouring rank); every variant needs n >= 1"""
    L = pkg._lib.lib()
    err = lambda: L.ocn_last_error().decode()
    Nx = 8
    g = pkg.RectilinearGrid(None, **SC.grid_arguments(Nx, 6, 1))
    p, w = C.c_void_p(8), (C.c_double * (Nx + 1))(*([1.0 / (Nx + 1)] * (Nx + 1)))   # never dereferenced: every call below is refused
    d = C.c_double
    run_tail = (w, d(1.0), d(9.8), d(1.0), p, p, p, p, p, p, None)
    assert L.ocn_split_explicit_dist_begin(g.cref, Nx, p, p, p, p, p, None, p, p, None) != 0 and "null pointer" in err()   # n == Nx is accepted
    assert L.ocn_split_explicit_dist_begin(g.cref, Nx + 1, p, p, p, p, p, p, p, p, None) != 0
    assert f"number of substeps ({Nx + 1})" in err() and f"Nx ({Nx})" in err()
    assert L.ocn_split_explicit_dist_run(g.cref, Nx + 1, *run_tail) != 0 and "n <= Nx" in err()
    assert L.ocn_split_explicit_dist_begin(g.cref, 0, p, p, p, p, p, p, p, p, None) != 0 and "number of substeps (0)" in err()
    assert L.ocn_split_explicit_dist_run(g.cref, 0, *run_tail) != 0 and "1 <= n" in err()
    assert L.ocn_split_explicit_substeps_blocked(g.cref, 0, w, d(1.0), d(9.8), d(1.0), p, p, p, p, p, p, p, p, p, None) != 0
    assert "ocn_split_explicit_substeps_blocked" in err() and "n >= 1" in err()
    assert L.ocn_split_explicit_substeps_ab3(g.cref, 0, w, d(1.0), d(9.8), d(1.0), (d * 7)(), p, p, p, p, p, p, p, p, p, None) != 0
    assert "ocn_split_explicit_substeps_ab3" in err() and "n >= 1" in err()
