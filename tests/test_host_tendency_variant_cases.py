"""Host-side checks of tests/tendency_variant_cases.py (no GPU): the tables reach the geometries they are written for, judged by the
launcher's own decision code through ocn_momentum_tendencies_plan (host only); the plan query on the benchmark's sizes and under every
switch; the reference composition against the oracle's own pieces; and the preconditions of the fast-math bound.

The switches are function-local statics read once per process, so every plan is taken in a child process with exactly the switches of its
setting in the environment: five children in all (default and the four of TC.SETTINGS), each answering every query of its setting."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fast_math_cases as FC
import tendency_variant_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("OCN_TEND_ADDR32", "OCN_TEND_MIN_BLOCKS", "OCN_NARROW_TILE", "OCN_STRIP_MIN_KZ", "OCN_TENDENCY_KERNEL", "OCN_XCD_REMAP")

# the benchmark's own sizes: the 512^3 box of the RK3 step (correction on load) and config 4 (plain, Bounded z)
BENCH_BOX = TC.case((512, 512, 512), KZ=64, **TC.PC)
BENCH_CONFIG4 = TC.case((512, 512, 256), kind="tiled", patch=(32, 8), KZ=32, topo="PPB")
TABLES = dict(PC_EDGES=TC.PC_EDGES, PC_FLAGS=TC.PC_FLAGS, LONG_CHUNKS=TC.LONG_CHUNKS, STRIP_PATCHES=TC.STRIP_PATCHES, SLABS=TC.SLABS,
              SLAB_REFUSED=[TC.SLAB_REFUSED], BENCH=[BENCH_BOX, BENCH_CONFIG4],
              REFUSALS=[dict(TC.PC_EDGES[4], flags=fl) for fl in (TC.SKIP_G_STORE, TC.WRAPPED_LOADS, TC.CORRECT_ONLY)])

CHILD = r'''
import json, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import oceananigans_jl_amd as ocn
import tendency_variant_cases as TC
import test_host_tendency_variant_cases as H
out = {}
for name, table in H.TABLES.items():
    out[name] = [TC.plan_of(ocn, c, x_topology="FullyConnected" if c.get("strips") else None) for c in table]
print(json.dumps(out))
'''

_plans = {}


def plans(setting):
    """{table name: [(status, plan) per case]} under the switches of TC.SETTINGS[setting] (None: none set), from one child process"""
    if setting not in _plans:
        env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        env.update(TC.SETTINGS[setting] if setting else {})
        r = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        _plans[setting] = json.loads(r.stdout.splitlines()[-1])
    return _plans[setting]


def _named(c, status, plan, kind=None):
    return status == 0 and (plan["kind"], plan["TX"], plan["TY"], plan["KZ"]) == (kind or c["kind"], *c["patch"], c["KZ"])


def _blocks(plan):
    return int(np.prod(plan["blocks"]))


def test_every_case_takes_the_kernel_patch_and_chunk_it_names():
    default = plans(None)
    for name in ("PC_EDGES", "PC_FLAGS", "STRIP_PATCHES"):
        for c, (st, plan) in zip(TABLES[name], default[name]):
            assert _named(c, st, plan), f"{name} {TC.case_id(c)}: {st} {plan}"
            if name != "STRIP_PATCHES":
                assert plan["correct_on_load"] and not plan["strips"]
            ox, oy = TC.OWNED[c["patch"]]
            wx, wy = (c["range"][1] - c["range"][0] + 1, c["range"][3] - c["range"][2] + 1) if c.get("range") else c["size"][:2]
            assert tuple(plan["blocks"][:2]) == (-(-wx // ox), -(-wy // oy))
    long_ = plans("min_blocks_1")["LONG_CHUNKS"]
    for c, (st, plan) in zip(TC.LONG_CHUNKS, long_):
        # (the tracer cases: the tracer launcher calls the same patch_grid with 32 x 8 patches; their Ny = 9 gives the momentum launch of the
        # same range 32 x 8 patches too, so its plan is theirs)
        assert _named(c, st, plan), f"LONG_CHUNKS {TC.case_id(c)}: {st} {plan}"
        assert plan["KZ"] == c["size"][2] and plan["blocks"][2] == 1
    for c, (st, plan) in zip(TC.LONG_CHUNKS, default["LONG_CHUNKS"]):
        assert st == 0 and plan["KZ"] <= 16, "without the switch no case of LONG_CHUNKS marches more than 16 planes"
    for setting, narrow in ((None, None), ("narrow_0", 0), ("narrow_1", 1)):
        for c, (st, plan) in zip(TC.SLABS, plans(setting)["SLABS"]):
            if c["narrow"] == narrow:
                assert _named(c, st, plan) and plan["strips"] and plan["correct_on_load"], f"SLABS {TC.case_id(c)} under {setting}: {st} {plan}"
    assert {c["patch"] for c in TC.SLABS} == {(32, 8), (17, 15)}
    st, plan = default["SLAB_REFUSED"][0]
    assert st == TC.UNSUPPORTED and plan["kind"] == "none"


def test_chunk_starts_lengths_workgroup_counts_and_patch_edges():
    default = plans(None)
    cases = TC.PC_EDGES + TC.PC_FLAGS
    got = default["PC_EDGES"] + default["PC_FLAGS"]
    starts = {s % 6 for c, (_, plan) in zip(cases, got) for s in TC.chunk_starts(c, plan)}
    assert starts == set(range(6)), f"chunk starts cover only the residues {sorted(starts)} modulo 6"
    lengths = [TC.chunk_lengths(c, plan) for c, (_, plan) in zip(cases, got)]
    flat = {n for ls in lengths for n in ls}
    assert {4, 16} <= flat
    assert any(len(ls) > 1 and ls[-1] < ls[0] for ls in lengths), "no case has a last chunk shorter than the others"
    long_pc = [TC.chunk_lengths(c, plan) for c, (_, plan) in zip(TC.LONG_CHUNKS, plans("min_blocks_1")["LONG_CHUNKS"]) if c["kind"] == "pc32"]
    assert {17, 36, 64} <= {ls[0] for ls in long_pc} and all(len(ls) == 1 for ls in long_pc)
    counts = {_blocks(plan) for _, plan in got}
    assert {n % 8 for n in counts} == set(range(8)), f"workgroup counts {sorted(counts)} miss a residue modulo 8"
    assert min(counts) < 8 < max(counts)
    ox, oy = TC.OWNED[(17, 15)]
    Nx, Ny = {c["size"][0] for c in cases}, {c["size"][1] for c in cases}
    for N, o, name in ((Nx, ox, "Nx"), (Ny, oy, "Ny")):
        assert {0, 1, o - 1} <= {n % o for n in N}, f"{name} = {sorted(N)}: an exact multiple of {o}, one more and one less are needed"
    # the strips: a second and a third patch that own one row, two exact patches, a range narrower than the patch, chunked and not
    strips = list(zip(TC.STRIP_PATCHES, default["STRIP_PATCHES"]))
    assert {(c["size"][1], plan["blocks"][1]) for c, (_, plan) in strips} == {(64, 2), (126, 2), (127, 3)}
    assert {c["range"][1] - c["range"][0] + 1 for c, _ in strips} == {2, 3}
    assert {plan["blocks"][2] for _, (_, plan) in strips} == {1, 2, 4}
    assert {c["topo"] for c, _ in strips} == {"PPP", "PPB"}


def test_plan_on_the_benchmark_sizes_and_under_every_switch():
    default, off = plans(None), plans("addr32_off")
    (st, box), (st4, config4) = default["BENCH"]
    assert st == 0 and (box["kind"], box["TX"], box["TY"], box["KZ"]) == ("pc32", 17, 15, 64)
    assert tuple(box["blocks"]) == (32, 37, 8) and _blocks(box) == 9472
    assert st4 == 0 and (config4["kind"], config4["KZ"]) == ("tiled", 32) and not config4["correct_on_load"]
    # OCN_TEND_ADDR32=0: the same patches, chunks and launch grids on the 64-bit kernel; wrapped loads and correct-only are refused
    for name in ("PC_EDGES", "BENCH"):
        for c, (st, plan), (_, was) in zip(TABLES[name], off[name], default[name]):
            if c["kind"] == "pc32":
                assert _named(c, st, plan, kind="tiled") and plan["correct_on_load"], f"{TC.case_id(c)}: {st} {plan}"
                assert plan["blocks"] == was["blocks"]
    assert [st for st, _ in default["REFUSALS"]] == [0, 0, 0]
    assert [st for st, _ in off["REFUSALS"]] == [0, TC.UNSUPPORTED, TC.UNSUPPORTED]
    assert off["REFUSALS"][0][1]["kind"] == "tiled"   # (SKIP_G_STORE is a permission: the 64-bit kernel stores G)
    # OCN_TEND_MIN_BLOCKS=1: one chunk whatever the depth; OCN_NARROW_TILE forces the patch of the strip-writing and the plain kernels only
    one = plans("min_blocks_1")
    assert all(plan["blocks"][2] == 1 and plan["KZ"] == c["size"][2] for c, (_, plan) in zip(TABLES["BENCH"], one["BENCH"]))
    for setting, patch in (("narrow_0", (32, 8)), ("narrow_1", (17, 15))):
        p = plans(setting)
        assert all((plan["TX"], plan["TY"]) == patch for _, plan in p["SLABS"])
        assert all((plan["TX"], plan["TY"]) == (17, 15) and plan["kind"] == "pc32" for _, plan in p["PC_EDGES"])
        plain = [plan for c, (_, plan) in zip(TC.LONG_CHUNKS, p["LONG_CHUNKS"]) if c["kind"] == "tiled" and c["size"][:2] == (16, 14)]
        assert plain and all((plan["TX"], plan["TY"]) == patch for plan in plain)


def test_plan_query_refuses_what_the_entry_points_refuse():
    import oceananigans_jl_amd as ocn
    g = TC.product_grid(ocn, TC.PC_EDGES[4], None)
    plan = ocn._lib.momentum_tendencies_plan
    assert plan(g.c, flags=TC.WRAPPED_LOADS)[0] == TC.INVALID_ARGUMENT                                # flags without the correction
    assert plan(g.c, correct_on_load=True, flags=8)[0] == TC.INVALID_ARGUMENT                         # unknown flag
    assert plan(g.c, correct_on_load=True, strips=True)[0] == TC.INVALID_ARGUMENT                     # strips on a Periodic x
    assert plan(g.c, range=(1, 33, 1, 29, 1, 9), correct_on_load=True)[0] == TC.UNSUPPORTED           # correction on load with a range
    assert plan(g.c, range=(0, 33, 1, 29, 1, 9))[0] == TC.INVALID_ARGUMENT                            # range outside the interior
    st, p = plan(g.c, range=(5, 4, 1, 29, 1, 9))
    assert st == 0 and p["kind"] == "none"                                                            # empty range: nothing to launch
    st, p = plan(TC.product_grid(ocn, TC.case((13, 17, 19), None, None, None), None).c)
    assert st == 0 and (p["kind"], p["KZ"], p["blocks"][2]) == ("direct", 1, 19)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the reference composition
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_composition_with_zero_pressure_is_tendencies_then_substep(oracle):
    O = oracle
    c = TC.PC_EDGES[2]
    og, f, _ = TC.setup(O, c)
    for has_zeta in (0, 1):
        G, Uo, U = TC.compose_reference(O, og, f, has_zeta, p=og.zeros(0))
        Gw = [og.zeros(l) for l in TC.LOCS]
        O.momentum_tendencies(og, f["u"], f["v"], f["w"], *Gw)
        for q, n in enumerate("uvw"):
            np.testing.assert_array_equal(U[q], f[n])
            np.testing.assert_array_equal(G[q], Gw[q])
            a = f[n].copy(order="F")
            O.rk3_substep(og, TC.LOCS[q], a, Gw[q], f["Gm"][q], TC.DT, TC.GAMMA, TC.ZETA if has_zeta else None)
            np.testing.assert_array_equal(Uo[q], a)
    G, Uo, U = TC.compose_reference(O, og, f, 0, correct_only=True)
    for q in range(3):
        np.testing.assert_array_equal(Uo[q], U[q])
        assert np.abs(og.interior_N(U[q]) - og.interior_N(f["uvw"[q]])).max() > 0.5    # the correction is O(1) against |u| <= 1


def test_composition_does_not_depend_on_the_halo_width(oracle):
    O = oracle
    narrow, wide = TC.PC_EDGES[2], TC.PC_EDGES[10]
    assert narrow["size"] == wide["size"] and narrow["halo"] != wide["halo"]
    og, f, _ = TC.setup(O, narrow)
    ow = TC.oracle_grid(O, wide)
    fw = {}
    for n, l in zip(("u", "v", "w", "p"), TC.LOCS + (0,)):
        fw[n] = ow.zeros(l)
        ow.interior_N(fw[n])[...] = og.interior_N(f[n])
        O.fill_halo_regions(ow, fw[n], l)
    fw["Gm"] = []
    for a, l in zip(f["Gm"], TC.LOCS):
        b = ow.zeros(l)
        ow.interior_N(b)[...] = og.interior_N(a)
        fw["Gm"].append(b)
    for has_zeta in (0, 1):
        for A, B in zip(TC.compose_reference(O, og, f, has_zeta), TC.compose_reference(O, ow, fw, has_zeta)):
            for a, b in zip(A, B):
                np.testing.assert_array_equal(og.interior_N(a), ow.interior_N(b))


def test_reference_is_computed_once_and_read_only(oracle):
    c = TC.PC_FLAGS[0]
    a, b = TC.reference(oracle, c, 1), TC.reference(oracle, c, 1)
    assert a is b
    with pytest.raises(ValueError):
        a[0][0][0, 0, 0] = 1.0


def test_slab_inputs_follow_the_header(oracle):
    """the x halos of p hold the neighbours' planes, its y / z halos NaN; column u[1 - Hx] corrected, the other halo columns not"""
    O = oracle
    c = TC.SLABS[0]
    og, ranks = TC.slab_inputs(O, c)
    nx, H = c["size"][0], og.Hx
    _, f, _ = TC.setup(O, c, nx * c["R"])
    _, _, U = TC.reference(O, c, 1, Nx=nx * c["R"])
    inner = (slice(None), slice(og.Hy, -og.Hy), slice(og.Hz, -og.Hz))
    for r, d in enumerate(ranks):
        assert np.isfinite(d["p"][inner]).all() and np.isnan(d["p"][:, :og.Hy]).all() and np.isnan(d["p"][:, :, -og.Hz:]).all()
        west_columns = [(r * nx - H + h) % (nx * c["R"]) for h in range(H)]
        np.testing.assert_array_equal(d["p"][inner][:H], og.interior_N(f["p"])[west_columns])
        np.testing.assert_array_equal(d["u"][0], U[0][r * nx])
        np.testing.assert_array_equal(d["u"][1:], f["u"][r * nx + 1:r * nx + nx + 2 * H])
        assert np.abs(d["u"][0] - f["u"][r * nx]).max() > 0
    west, east = TC.expected_strips(og, c, U, 1)
    assert np.isnan(west[:, :og.Hy]).all() and np.isfinite(west[:, og.Hy:-og.Hy, og.Hz:-og.Hz]).all()
    np.testing.assert_array_equal(east[:, og.Hy:-og.Hy, og.Hz:-og.Hz, 0], og.interior_N(U[0])[2 * nx - H:2 * nx])


# ---------------------------------------------------------------------------------------------------------------------------------------
# the preconditions of the fast-math bound, on the CPU
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inp", TC.FAST_INPUTS)
@pytest.mark.parametrize("size", [s for s, _ in TC.FAST_SIZES], ids=lambda s: "x".join(map(str, s)))
def test_fast_math_reference_error_is_finite_and_scales_are_positive(size, inp):
    """E_64 (the Float64 composition against the extended one, in units of ε s) is finite and s > 0 wherever the reference is nonzero, for
    G and U_out of every variant's reference"""
    for has_zeta, correct_only in ((0, 0), (1, 0), (0, 1)):
        og, f, G64, Uo64, Gext, Uoext, sG, sU = TC.fast_reference(size, inp, bool(has_zeta), bool(correct_only))
        for name, r64, ext, scales in (("G", G64, Gext, sG), ("U_out", Uo64, Uoext, sU)):
            for q, (a, x, s) in enumerate(zip(r64, ext, scales)):
                a, x = og.interior_N(a), og.interior_N(x)
                assert x.dtype == np.longdouble and np.isfinite(np.asarray(x, dtype=np.float64)).all()
                assert (s[x != 0] > 0).all(), f"{name}[{q}]: a nonzero reference value with local magnitude 0"
                E64, at, exact = FC.error_in_eps(a, x, s)
                print(f"{size} {inp} has_zeta={has_zeta} correct_only={correct_only} {name}[{q}]: E_64 = {E64:.3f} at {at}")
                assert np.isfinite(E64) and exact, f"{name}[{q}]: E_64 = {E64}"
        corr = max(float(np.abs(og.interior_N(b) - og.interior_N(f[n])).max()) for b, n in zip(TC.compose_reference(oracle_module(), og, f, 0, True)[2], "uvw"))
        print(f"{size} {inp}: largest correction {corr:.3e}")
        assert corr > 0


def oracle_module():
    from oracle import oracle as O
    O.lib()
    return O
