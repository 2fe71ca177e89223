"""The four implementations of the barotropic substep loop in csrc/kernels.hip, through the C ABI, against oracle/hydrostatic.py on the
cases of tests/split_explicit_cases.py -- bit for bit (kernels.hip is compiled without contraction in both math modes):

  * ocn_split_explicit_substeps          the reference-shaped pair of kernels
  * ocn_split_explicit_substeps_blocked  the temporally blocked LDS kernel of the fused step
  * ocn_split_explicit_substeps_ab3      the AdamsBashforth3Scheme variant
  * ocn_split_explicit_dist_begin/_run   the blocked kernel on the wide planes of slab-x ranks

NaN poisoning.  Before every call the halos of every input plane, the whole filtered planes and the whole work buffer hold NaN, and no NaN
may reach an interior.  That pins three properties read from the code: the kernels wrap on load and never read a halo; the first launch
never reads the filtered state; a launch reads from the ping-pong set only cells that the previous launch wrote (the ownership argument
above PlaneLay in kernels.hip).  Halo contents afterwards are not asserted: the plain launcher zeroes and copies whole planes, the others
write interiors only, and the model refills η's halos either way."""
import ctypes as C

import numpy as np
import pytest

import split_explicit_cases as SC

pytestmark = pytest.mark.gpu

STATE = ("eta", "U", "V")


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _nan(*shape):
    import torch
    return torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")


def _grid(ocn, Nx, Ny, halo):
    g = ocn.RectilinearGrid(ocn.GPU(), **SC.grid_arguments(Nx, Ny, halo))
    assert (g.dx, g.dy, g.Lz) == (SC.DX, SC.DY, SC.DEPTH)
    return g


def _weights(n):
    return (C.c_double * n)(*SC.weights(n))


def _check(planes, want, Nx, Ny, halo, what):
    """the interiors of the [y, x] device planes equal the oracle's (η̄, Ū, V̄) bit for bit, and are finite"""
    for name, plane, w in zip(STATE, planes, want):
        got = SC.interior_of(plane.cpu().numpy(), Nx, Ny, halo, halo)
        assert np.isfinite(got).all(), f"{what} {name}: a NaN reached the interior"
        np.testing.assert_array_equal(got, w, err_msg=f"{what} {name}")


def _run_single_rank(ocn, kernel, case):
    Nx, Ny, n, halo = case
    ocn.set_math_mode(ocn.MATH_STRICT)
    g = _grid(ocn, Nx, Ny, halo)
    eta, U, V, GU, GV = (_dev(SC.place(a, halo, halo)) for a in SC.fields(Nx, Ny))
    shape = tuple(eta.shape)
    filtered = [_nan(*shape) for _ in range(3)]
    head = (g.cref, n, _weights(n), float(SC.DTAU), SC.GRAV, SC.DEPTH)
    planes = [t.data_ptr() for t in (eta, U, V, *filtered, GU, GV)]
    if kernel == "plain":
        ocn._lib.call("ocn_split_explicit_substeps", *head, *planes, 0)
    elif kernel == "blocked":
        work = _nan(3, *shape)
        ocn._lib.call("ocn_split_explicit_substeps_blocked", *head, *planes, work.data_ptr(), 0)
    else:
        work = _nan(7, *shape)
        ocn._lib.call("ocn_split_explicit_substeps_ab3", *head, ocn.AdamsBashforth3Scheme().c_array(), *planes, work.data_ptr(), 0)
    ocn.sync_device()
    want = SC.reference(Nx, Ny, n, ab3=kernel == "ab3")
    _check(filtered, want, Nx, Ny, halo, f"{kernel} filtered")
    _check((eta, U, V), want, Nx, Ny, halo, f"{kernel} state")     # _update_split_explicit_state!: η, U, V <- their averages


@pytest.mark.parametrize("case", SC.SINGLE_RANK_CASES, ids=SC.case_id)
@pytest.mark.parametrize("kernel", ["plain", "blocked"])
def test_forward_backward_substeps_match_oracle(ocn, kernel, case):
    """the plain pair of kernels and the blocked kernel on the same inputs: every n of 1 .. 9 at (65, 17) (n < 4: one launch, both first and
    last; n = 4: exactly one full launch; the tails n mod 4 = 1, 2, 3), sizes below SH and either side of the 64 x 16 tile edges at n = 3
    and n = 7, six launches at (16, 12)"""
    _run_single_rank(ocn, kernel, case)


@pytest.mark.parametrize("case", SC.AB3_CASES, ids=SC.case_id)
def test_ab3_substeps_match_oracle(ocn, case):
    """AdamsBashforth3Scheme() with its default coefficients, as the model passes them; n = 1, 2: the three history planes are still copies
    of each other.  The launcher copies the history from whole planes (NaN halos included); the kernels read interiors only."""
    from oracle import hydrostatic as Hy
    c = Hy.ab3_coefficients()
    assert list(ocn.AdamsBashforth3Scheme().c_array()) == [c[k] for k in ("alpha", "theta", "beta", "delta", "mu", "gamma", "epsilon")]
    _run_single_rank(ocn, "ab3", case)


@pytest.mark.parametrize("case", SC.SLAB_CASES, ids=SC.case_id)
def test_slab_substeps_match_the_global_oracle(ocn, case):
    """R slabs of a global periodic domain on one GPU in one process: _begin on every slab, the strips handed over by tensor copy (rank r's
    west strip is the east halo of rank r - 1), _run on every slab.  Every slab's η, U, V equal the matching columns of the global oracle
    result bit for bit.  The 11-plane work buffer and the send buffers start as NaN: no launch reads a cell outside what the previous
    launch owned, and the clamped loads of a first launch with n < 4 stay out of the owned range."""
    nx, Ny, n, R, halo = case
    ocn.set_math_mode(ocn.MATH_STRICT)
    glob = SC.fields(nx * R, Ny)
    grids = [_grid(ocn, nx, Ny, halo) for _ in range(R)]
    ranks = []
    for r, g in enumerate(grids):
        planes = [_dev(SC.place(a[r * nx:(r + 1) * nx], halo, halo)) for a in glob]
        work = _nan(11 * (nx + 2 * n) * Ny)
        send_west, send_east = _nan(5 * n * Ny), _nan(5 * n * Ny)
        ocn._lib.call("ocn_split_explicit_dist_begin", g.cref, n, *[t.data_ptr() for t in planes], work.data_ptr(), send_west.data_ptr(),
                      send_east.data_ptr(), 0)
        ranks.append((planes, work, send_west, send_east))
    ocn.sync_device()
    for r, (g, (planes, work, _, _)) in enumerate(zip(grids, ranks)):
        recv_west = ranks[(r - 1) % R][3].clone()     # the west neighbour's east strip
        recv_east = ranks[(r + 1) % R][2].clone()     # the east neighbour's west strip
        assert bool(recv_west.isfinite().all()) and bool(recv_east.isfinite().all())
        ocn._lib.call("ocn_split_explicit_dist_run", g.cref, n, _weights(n), float(SC.DTAU), SC.GRAV, SC.DEPTH,
                      *[t.data_ptr() for t in planes[:3]], work.data_ptr(), recv_west.data_ptr(), recv_east.data_ptr(), 0)
    ocn.sync_device()
    want = SC.reference(nx * R, Ny, n)
    for r, (planes, *_) in enumerate(ranks):
        _check(planes[:3], [w[r * nx:(r + 1) * nx] for w in want], nx, Ny, halo, f"rank {r} of {R}")
