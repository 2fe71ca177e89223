"""The correction-on-load momentum tendency kernels of csrc/tendencies.hip against the oracle, one hop, on the tables of
tests/tendency_variant_cases.py:

  * momentum_tendencies_pc32 (17 x 15 patches, 32-bit addressing: the kernel of the benchmarked RK3 box step) in its eight instantiations,
    through ocn_compute_momentum_tendencies_rk3 with p_correct and ocn_compute_momentum_tendencies_rk3_flags;
  * its 64-bit sibling momentum_tendencies_tiled<P, 17, 15, 3, true> (OCN_TEND_ADDR32=0), with the two refusals that setting implies;
  * the strip-writing kernels of a slab rank (ocn_compute_momentum_tendencies_rk3_strips), 32 x 8 and 17 x 15 patches, R slabs of a global
    periodic box in one process;
  * z chunks longer than 16 planes (OCN_TEND_MIN_BLOCKS=1: the 512^3 box marches 64) of these and of the plain momentum and tracer kernels;
  * the 4 x 64 patches of a halo-wide x-strip (plain ranged launches).

Strict math: G and U_out equal oracle.pressure_correct -> fill_halo_regions -> momentum_tendencies -> rk3_substep bit for bit on the interior,
and every output keeps its sentinel outside it.  The device's p has NaN halos (the header: p needs no halos), with OCN_RK3_WRAPPED_LOADS
u, v, w have NaN halos too, and with has_zeta = 0 the G⁻ pointers are NULL: nothing may read them.  After OCN_RK3_SKIP_G_STORE the contents
of G are not asserted (a permission, not a promise).  Every case first asserts that ocn_momentum_tendencies_plan reports the kernel, patch
and z chunk the table expects, so a changed dispatch fails here instead of silently testing another kernel.

The switches (OCN_TEND_ADDR32, OCN_TEND_MIN_BLOCKS, OCN_NARROW_TILE) are function-local statics read once per process: one child process
per setting runs all the cases of that setting, compares them itself and prints one JSON line per case.

Fast math (the default of the benchmark): E_fast <= FACTOR max(E_64, 1) with FACTOR = 4, ε = 2^-52 and per-cell local magnitudes, the bound
of tests/test_gpu_fast_math_accuracy.py, for all eight variants on (33, 29, 9) and (19, 9, 36) with the inputs noise, smooth and mean_T of
tests/fast_math_cases.py and p = 1e-2 x smooth: the correction dt_correct Δp / Δ is at most 2.7e-3 (against |u| of 1, 1 and 10), G⁻ uniform
with the amplitude max|u|² / Δy of the advective tendency.  Local magnitudes: for G the advective s of the corrected fields; for U_out
(largest |u| in the neighbourhood) + dt_correct (largest |difference of neighbouring p| in 5³) / (smallest spacing) + dt (|γ| s_G + |ζ| |G⁻|).
tests/test_host_tendency_variant_cases.py checks on the CPU that E_64 is finite and s > 0 wherever the reference is nonzero."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fast_math_cases as FC
import tendency_variant_cases as TC
from helpers import from_dev
from helpers import to_dev as _helpers_to_dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTOR = 4.0  # tests/test_gpu_fast_math_accuracy.py


def to_dev(ocn, pg, loc, a):
    """helpers.to_dev of a writable copy (the shared inputs are read-only; torch wants writable memory)"""
    return _helpers_to_dev(ocn, pg, loc, np.array(a, order="F"))


def _sentinels(ocn, pg, locs=TC.LOCS):
    out = [ocn.Field(l, pg) for l in locs]
    for f in out:
        f.data.fill_(TC.SENTINEL)
    return out


def _assert_plan(ocn, c, pg, kind=None):
    """the launch of this case takes the kernel, patch and z chunk its table entry names (kind: the 64-bit kernel of OCN_TEND_ADDR32=0)"""
    st, plan = TC.plan_of(ocn, c, g=pg)
    want = (kind or c["kind"], *c["patch"], c["KZ"])
    got = (plan["kind"], plan["TX"], plan["TY"], plan["KZ"])
    assert st == 0 and got == want, f"{TC.case_id(c)}: plan {got} (status {st}), the table expects {want}"
    assert plan["strips"] == bool(c.get("strips"))
    return plan


def _ptrs(fields):
    return [None if f is None else f.ptr for f in fields]


def _rk3_args(pg, dev, G, Uo, has_zeta, dp):
    Gm = dev["Gm"] if has_zeta else [None] * 3   # has_zeta = 0: G⁻ is unused, so it is not there
    return (pg.cref, *_ptrs(dev["U"]), *_ptrs(G), *_ptrs(Gm), *_ptrs(Uo), TC.DT, TC.GAMMA, TC.ZETA, int(has_zeta), dp.ptr, TC.DT_CORRECT)


def _upload(ocn, og, pg, f, wrapped):
    """u, v, w (NaN halos when nothing may read them), G⁻ and p with NaN halos"""
    U = [TC.poison_halos(og, f[n]) if wrapped else f[n] for n in "uvw"]
    return dict(U=[to_dev(ocn, pg, l, a) for l, a in zip(TC.LOCS, U)], Gm=[to_dev(ocn, pg, l, a) for l, a in zip(TC.LOCS, f["Gm"])],
                p=to_dev(ocn, pg, 0, TC.poison_halos(og, f["p"])))


def run_pc_case(ocn, O, c, has_zeta, flags=0, entry="rk3", kind=None):
    """one correction-on-load launch in strict math against the composed reference: None, or the failure message"""
    ocn.set_math_mode(ocn.MATH_STRICT)
    og, f, _ = TC.setup(O, c)
    pg = TC.product_grid(ocn, c, ocn.GPU())
    plan = _assert_plan(ocn, dict(c, flags=flags), pg, kind)
    correct_only = bool(flags & TC.CORRECT_ONLY)
    Gref, Uref, _ = TC.reference(O, c, has_zeta, correct_only)
    dev = _upload(ocn, og, pg, f, flags & TC.WRAPPED_LOADS)
    G, Uo = _sentinels(ocn, pg), _sentinels(ocn, pg)
    args = _rk3_args(pg, dev, G, Uo, has_zeta, dev["p"])
    if entry == "rk3":
        ocn._lib.call("ocn_compute_momentum_tendencies_rk3", *args, None, 0)
    else:
        ocn._lib.call("ocn_compute_momentum_tendencies_rk3_flags", *args, int(flags), 0)
    ocn.sync_device()
    msgs = []
    for q, n in enumerate("uvw"):
        if not (flags & TC.SKIP_G_STORE):
            msgs.append(TC.compare(og, c, plan, "G" + n, from_dev(G[q]), Gref[q]))
        msgs.append(TC.compare(og, c, plan, n + "_out", from_dev(Uo[q]), Uref[q]))
    return "; ".join(m for m in msgs if m) or None


# ---------------------------------------------------------------------------------------------------------------------------------------
# in process: default switches, strict math
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("has_zeta", [0, 1])
@pytest.mark.parametrize("c", TC.PC_EDGES, ids=TC.case_id)
def test_pc32_edges_match_the_oracle(oracle, ocn, c, has_zeta):
    msg = run_pc_case(ocn, oracle, c, has_zeta)
    assert msg is None, f"{TC.case_id(c)} has_zeta={has_zeta}: {msg}"


@pytest.mark.gpu
@pytest.mark.parametrize("c", TC.PC_FLAGS, ids=TC.case_id)
def test_pc32_flag_variants_match_the_oracle(oracle, ocn, c):
    msg = run_pc_case(ocn, oracle, c, c["has_zeta"], c["flags"], entry="flags")
    assert msg is None, f"{TC.case_id(c)}: {msg}"


def run_plain_case(ocn, O, c, tracer=False):
    """ocn_compute_momentum_tendencies / ocn_compute_tracer_tendency (full or ranged) against the oracle, as tests/test_gpu_kernels.py does:
    Gw at a wall face k = 1 is written by a ranged launch and excluded by :xyz, so it is compared in neither"""
    ocn.set_math_mode(ocn.MATH_STRICT)
    og, f, _ = TC.setup(O, c)
    pg = TC.product_grid(ocn, c, ocn.GPU())
    plan = _assert_plan(ocn, c, pg)
    rng_ = c.get("range")
    r = None if rng_ is None else ocn._lib.i32_array(list(rng_))
    dU = [to_dev(ocn, pg, l, f[n]) for l, n in zip(TC.LOCS, "uvw")]
    if tracer:
        want = og.zeros(0)
        O.tracer_tendency(og, f["u"], f["v"], f["w"], f["c"], want)
        dc, (Gc,) = to_dev(ocn, pg, 0, f["c"]), _sentinels(ocn, pg, (0,))
        ocn._lib.call("ocn_compute_tracer_tendency", pg.cref, *_ptrs(dU), dc.ptr, Gc.ptr, r, 0)
        ocn.sync_device()
        return TC.compare(og, c, plan, "Gc", from_dev(Gc), want, rng_)
    want = [og.zeros(l) for l in TC.LOCS]
    O.momentum_tendencies(og, f["u"], f["v"], f["w"], *want)
    G = _sentinels(ocn, pg)
    ocn._lib.call("ocn_compute_momentum_tendencies", pg.cref, *_ptrs(dU), *_ptrs(G), r, 0)
    ocn.sync_device()
    msgs = []
    for q, n in enumerate("uvw"):
        wall = n == "w" and c["topo"] == "PPB"
        got = from_dev(G[q])
        if wall and rng_ is None:   # :xyz leaves the wall face alone: it belongs to the outside
            full = (1, og.Nx, 1, og.Ny, 2, og.Nz)
            msgs.append(TC.compare(og, c, plan, "G" + n, got[:, :, :want[q].shape[2]], want[q], full))
        else:
            msgs.append(TC.compare(og, c, plan, "G" + n, got, want[q], rng_, skip_k1=wall))
    return "; ".join(m for m in msgs if m) or None


@pytest.mark.gpu
@pytest.mark.parametrize("c", TC.STRIP_PATCHES, ids=TC.case_id)
def test_strip_patches_match_the_oracle(oracle, ocn, c):
    msg = run_plain_case(ocn, oracle, c)
    assert msg is None, f"{TC.case_id(c)}: {msg}"


def run_slab_case(ocn, O, c):
    """ocn_compute_momentum_tendencies_rk3_strips on every slab of the global box: G, U_out against the matching columns of the global
    reference, the strip buffers against the stepped border columns with NaN kept everywhere else"""
    import torch
    ocn.set_math_mode(ocn.MATH_STRICT)
    (nx, Ny, Nz), R = c["size"], c["R"]
    og, ranks = TC.slab_inputs(O, c)
    Gref, Uref, _ = TC.reference(O, c, 1, Nx=nx * R)
    msgs = []
    for r, d in enumerate(ranks):
        pg = TC.product_grid(ocn, c, ocn.GPU(), "FullyConnected", x=(TC.DX * nx * r, TC.DX * nx * (r + 1)))
        lg = O.Grid(c["size"], topology="PPP", halo=c["halo"], **TC.extents(c))   # (the local shape: masks and indices of compare)
        assert (pg.dx, pg.dy, pg.dz) == (og.dx, og.dy, og.dz)
        plan = _assert_plan(ocn, c, pg)
        dev = dict(U=[to_dev(ocn, pg, l, d[n]) for l, n in zip(TC.LOCS, "uvw")], Gm=[to_dev(ocn, pg, l, a) for l, a in zip(TC.LOCS, d["Gm"])])
        dp = to_dev(ocn, pg, 0, d["p"])
        G, Uo = _sentinels(ocn, pg), _sentinels(ocn, pg)
        field_doubles = og.Hx * (Ny + 2 * og.Hy) * (Nz + 2 * og.Hz)
        west, east = (torch.full((3 * field_doubles,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(2))
        ocn._lib.call("ocn_compute_momentum_tendencies_rk3_strips", *_rk3_args(pg, dev, G, Uo, 1, dp), west.data_ptr(), east.data_ptr(),
                      field_doubles, 0)
        ocn.sync_device()
        cols = slice(r * nx, r * nx + nx + 2 * og.Hx)
        for q, n in enumerate("uvw"):
            msgs.append(TC.compare(lg, c, plan, f"rank {r} G{n}", from_dev(G[q]), Gref[q][cols]))
            msgs.append(TC.compare(lg, c, plan, f"rank {r} {n}_out", from_dev(Uo[q]), Uref[q][cols]))
        for name, buf, want in zip(("west", "east"), (west, east), TC.expected_strips(og, c, Uref, r)):
            got = buf.cpu().numpy().reshape(want.shape, order="F")
            same = (got == want) | (np.isnan(got) & np.isnan(want))
            if not same.all():
                at = tuple(int(x) for x in np.argwhere(~same)[0])
                msgs.append(f"rank {r} {name} strip: {np.count_nonzero(~same)} elements differ, first at (h, parent j, parent k, field) = {at}: "
                            f"got {got[at]!r}, want {want[at]!r}")
    return "; ".join(m for m in msgs if m) or None


@pytest.mark.gpu
@pytest.mark.parametrize("c", [c for c in TC.SLABS if c["narrow"] is None], ids=TC.case_id)
def test_slab_strips_match_the_global_oracle(oracle, ocn, c):
    msg = run_slab_case(ocn, oracle, c)
    assert msg is None, f"{TC.case_id(c)}: {msg}"


def _refused(ocn, O, c, entry, flags=0):
    """status of a launch that must be refused, and whether every output kept its sentinel (nothing was launched)"""
    import torch
    og = TC.oracle_grid(O, c)
    x_topology = "FullyConnected" if entry == "strips" else None
    pg = TC.product_grid(ocn, c, ocn.GPU(), x_topology, x=(0.0, TC.DX * c["size"][0]))
    f = TC.make_inputs(O, og, c["size"])
    dev = _upload(ocn, og, pg, f, False)
    G, Uo = _sentinels(ocn, pg), _sentinels(ocn, pg)
    args = _rk3_args(pg, dev, G, Uo, 0, dev["p"])
    if entry == "strips":
        n = og.Hx * (og.Ny + 2 * og.Hy) * (og.Nz + 2 * og.Hz)
        bufs = [torch.full((3 * n,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(2)]
        st = ocn._lib.lib().ocn_compute_momentum_tendencies_rk3_strips(*args, bufs[0].data_ptr(), bufs[1].data_ptr(), n, 0)
    else:
        st = ocn._lib.lib().ocn_compute_momentum_tendencies_rk3_flags(*args, int(flags), 0)
    ocn.sync_device()
    return st, all(bool((a.data == TC.SENTINEL).all()) for a in G + Uo)


@pytest.mark.gpu
def test_slab_below_the_tile_is_refused_not_launched(oracle, ocn):
    """(6, 8, 4): wide enough for two strips (wx >= 2 Hx) but below the 16 columns of the tiled kernel: OCN_ERR_UNSUPPORTED, nothing written"""
    c = TC.SLAB_REFUSED
    st, _ = TC.plan_of(ocn, c, x_topology="FullyConnected")
    assert st == TC.UNSUPPORTED
    st, untouched = _refused(ocn, oracle, c, "strips")
    assert st == TC.UNSUPPORTED and untouched


# ---------------------------------------------------------------------------------------------------------------------------------------
# one child process per switch setting
# ---------------------------------------------------------------------------------------------------------------------------------------
def run_setting(setting):
    """the body of a child: every case of the setting, one JSON line each"""
    import torch
    import oceananigans_jl_amd as ocn
    from oracle import oracle as O
    torch.cuda.set_device(0)
    O.lib()

    def report(c, what, fn):
        try:
            msg = fn()
        except Exception as e:  # (a refused launch or a wrong plan: reported like a mismatch)
            msg = f"{type(e).__name__}: {e}"
        print(json.dumps({"case": f"{what} {TC.case_id(c)}", "ok": msg is None, "msg": msg}), flush=True)

    if setting == "addr32_off":   # PC_EDGES on the 64-bit kernel, and the two refusals
        for c in TC.PC_EDGES:
            for hz in (0, 1):
                report(c, f"pc64 has_zeta={hz}", lambda: run_pc_case(ocn, O, c, hz, kind="tiled"))
        c = TC.PC_EDGES[4]
        for flags in (TC.WRAPPED_LOADS, TC.CORRECT_ONLY):
            def refusal():
                st, _ = TC.plan_of(ocn, dict(c, flags=flags))
                got, untouched = _refused(ocn, O, c, "flags", flags)
                ok = st == TC.UNSUPPORTED and got == TC.UNSUPPORTED and untouched
                return None if ok else f"flags {flags}: plan status {st}, launch status {got}, outputs untouched: {untouched}"
            report(c, f"refusal flags={flags}", refusal)
    elif setting == "min_blocks_1":
        for c in TC.LONG_PC:
            for hz in (0, 1):
                report(c, f"pc32 has_zeta={hz}", lambda: run_pc_case(ocn, O, c, hz))
        for c in TC.LONG_PLAIN:
            report(c, "plain", lambda: run_plain_case(ocn, O, c))
        for c in TC.LONG_TRACER:
            report(c, "tracer", lambda: run_plain_case(ocn, O, c, tracer=True))
    else:
        narrow = {"narrow_0": 0, "narrow_1": 1}[setting]
        for c in TC.SLABS:
            if c["narrow"] == narrow:
                report(c, "slab", lambda: run_slab_case(ocn, O, c))


EXPECTED_LINES = {"addr32_off": 2 * len(TC.PC_EDGES) + 2, "min_blocks_1": 2 * len(TC.LONG_PC) + len(TC.LONG_PLAIN) + len(TC.LONG_TRACER),
                  "narrow_0": 2, "narrow_1": 2}

CHILD = r'''
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import test_gpu_tendency_variants as T
T.run_setting(sys.argv[2])
'''


@pytest.mark.gpu
@pytest.mark.parametrize("setting", list(TC.SETTINGS))
def test_switch_settings_in_child_processes(tmp_path, ocn, setting):
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    env = dict(os.environ, **TC.SETTINGS[setting])
    r = subprocess.run([sys.executable, str(script), ROOT, setting], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"child ({setting}) exited {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == EXPECTED_LINES[setting], f"{setting}: {len(lines)} cases reported, {EXPECTED_LINES[setting]} expected"
    failed = [f"{l['case']}: {l['msg']}" for l in lines if not l["ok"]]
    assert not failed, f"{setting}: " + "\n".join(failed)


# ---------------------------------------------------------------------------------------------------------------------------------------
# fast math
# ---------------------------------------------------------------------------------------------------------------------------------------
def fast_errors(og, plan, label, names, got, r64, ext, scales):
    """prints E_fast and E_64 per field; returns the failures of: finite, exact where s == 0, E_fast <= FACTOR max(E_64, 1)"""
    failures = []
    for n, a, b, x, s in zip(names, got, r64, ext, scales):
        a, b, x = (og.interior_N(q) for q in (a, b, x))
        if not np.isfinite(a).all():
            failures.append(f"{n}: {np.count_nonzero(~np.isfinite(a))} non-finite values")
            continue
        Ef, at, exact_f = FC.error_in_eps(a, x, s)
        E64, _, _ = FC.error_in_eps(b, x, s)
        print(f"{label:44s} {n:6s} E_fast {Ef:8.3f}  E_64 {E64:8.3f}")
        if not exact_f:
            failures.append(f"{n}: differs from the extended reference where the local magnitude is 0")
        if Ef > FACTOR * max(E64, 1.0):
            i, j, k = at
            failures.append(f"{n}: E_fast = {Ef:.2f} > {FACTOR:g} max(E_64 = {E64:.2f}, 1) at (i, j, k) = {at}; mod the 16 x 14 owned columns "
                            f"({(i - 1) % 16}, {(j - 1) % 14}), chunk {(k - 1) // plan['KZ']} plane {(k - 1) % plan['KZ']} of KZ = {plan['KZ']}")
    return failures


@pytest.mark.gpu
@pytest.mark.parametrize("c", TC.FAST_CASES, ids=lambda c: TC.case_id(c) + "-" + c["inp"])
def test_pc32_fast_error_per_cell(oracle, ocn, c):
    has_zeta, flags = c["has_zeta"], c["flags"]
    og, f, G64, Uo64, Gext, Uoext, sG, sU = TC.fast_reference(c["size"], c["inp"], bool(has_zeta), bool(flags & TC.CORRECT_ONLY))
    pg = TC.product_grid(ocn, c, ocn.GPU())
    plan = _assert_plan(ocn, c, pg)
    ocn.set_math_mode(ocn.MATH_FAST)
    try:
        dev = _upload(ocn, og, pg, f, flags & TC.WRAPPED_LOADS)
        G, Uo = _sentinels(ocn, pg), _sentinels(ocn, pg)
        ocn._lib.call("ocn_compute_momentum_tendencies_rk3_flags", *_rk3_args(pg, dev, G, Uo, has_zeta, dev["p"]), int(flags), 0)
        ocn.sync_device()
    finally:
        ocn.set_math_mode(ocn.MATH_STRICT)
    label = f"pc32 {c['size']} {c['inp']} has_zeta={has_zeta} flags={flags}"
    failures = fast_errors(og, plan, label, ("u_out", "v_out", "w_out"), [from_dev(a) for a in Uo], Uo64, Uoext, sU)
    if not (flags & TC.SKIP_G_STORE):
        failures += fast_errors(og, plan, label, ("Gu", "Gv", "Gw"), [from_dev(a) for a in G], G64, Gext, sG)
    for a in G + Uo:   # nothing outside the interior is written in either math mode
        arr = from_dev(a)
        assert (arr[~TC.interior_mask(og, arr.shape)] == TC.SENTINEL).all(), f"{label}: an output lost its sentinel outside the interior"
    assert not failures, f"{label}: " + "; ".join(failures)
