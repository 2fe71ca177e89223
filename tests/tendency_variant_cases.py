"""Case tables, seeded inputs and the reference composition of the kernel-level tests of the correction-on-load momentum tendency kernels
(csrc/tendencies.hip: momentum_tendencies_pc32 in its eight instantiations, its 64-bit sibling momentum_tendencies_tiled<P, 17, 15, 3,
true>, the strip-writing kernels of a slab rank) and of the launch geometries next to them that no other test reaches (z chunks longer
than 16 planes, the 4 x 64 patches of a halo-wide x-strip).  No GPU is needed to import this: tests/test_host_tendency_variant_cases.py
checks the tables against ocn_momentum_tendencies_plan (host only) and the reference composition against the oracle's own pieces,
tests/test_gpu_tendency_variants.py runs the kernels on them.

The expected result of every case is oracle/oracle.py, one hop: pressure_correct on copies of u, v, w; fill_halo_regions;
momentum_tendencies; rk3_substep (zeta=None for has_zeta = 0).  With OCN_RK3_CORRECT_ONLY, U_out is the corrected velocity itself.  In
strict math every comparison is bit for bit.

What the shapes are for.  Patches of 17 x 15 own 16 x 14 columns, 32 x 8 own 31 x 7, 4 x 64 own 3 x 63; a launch marches chunks of KZ
planes, KZ halved from the depth while it is longer than 16 and the launch has fewer than OCN_TEND_MIN_BLOCKS = 8192 workgroups; the LDS
slots of the correction-on-load kernels rotate with the absolute k (k & 1 and k % 3), so the chunk start 1 + n KZ modulo 6 is geometry;
block_coords remaps workgroups over the 8 XCDs, so the workgroup count modulo 8 is geometry.  Every case names the kernel, patch and KZ it
expects under the default switches; the plan query confirms them, so a change of the dispatch cannot empty a table silently."""
import functools

import numpy as np

from helpers import stretched_faces

GAMMA, ZETA = 5 / 12, -17 / 60
DT, DT_CORRECT = 0.05, 0.037          # dt_correct != dt: a swapped time step shows
DX, DY, DZ = 0.125, 0.09375, 0.15625  # unequal: a swapped metric shows; dyadic: a slab's Δx is bit for bit the global one
P_AMPLITUDE = DY / DT_CORRECT         # dt_correct Δp / Δy = O(1) against |u| <= 1 (0.75 and 0.6 of that along x and z)
SENTINEL = -7.0
SKIP_G_STORE, WRAPPED_LOADS, CORRECT_ONLY = 1, 2, 4   # OCN_RK3_* (include/ocn_hip.h)
UNSUPPORTED = -2                                      # OCN_ERR_UNSUPPORTED
INVALID_ARGUMENT = -1
LOCS = (1, 2, 4)                                      # u, v, w
H3 = (3, 3, 3)
OWNED = {(17, 15): (16, 14), (32, 8): (31, 7), (4, 64): (3, 63)}


def case(size, kind, patch, KZ, halo=H3, topo="PPP", z=None, **more):
    return dict(size=tuple(size), halo=tuple(halo), topo=topo, z=z, kind=kind, patch=patch, KZ=KZ, **more)


def case_id(c):
    s = "x".join(map(str, c["size"]))
    if c["halo"] != H3:
        s += "-h" + "".join(map(str, c["halo"]))
    if c["topo"] != "PPP":
        s += "-" + c["topo"]
    for key in ("flags", "has_zeta", "range", "R", "narrow"):
        if c.get(key) is not None:
            s += f"-{key}{'_'.join(map(str, c[key])) if isinstance(c[key], tuple) else c[key]}"
    return s


# ---- PC_EDGES: (Periodic, Periodic, Periodic), correction on load, flags = 0; pc32 with 17 x 15 patches ---------------------------------
PC = dict(kind="pc32", patch=(17, 15))
PC_EDGES = [
    case((16, 8, 4), KZ=4, **PC),                       # the smallest accepted; 1 workgroup
    case((16, 14, 4), KZ=4, **PC),                      # exactly one patch
    case((17, 15, 5), KZ=5, **PC),                      # a second patch that owns one column and one row; 4 workgroups
    case((32, 28, 16), KZ=16, **PC),                    # 2 x 2 exactly, one chunk of 16
    case((33, 29, 9), KZ=9, **PC),                      # 3 x 3 with clipped last patches; 9 workgroups
    case((31, 27, 17), KZ=9, **PC),                     # chunks 9 + 8: the last one shorter
    case((19, 9, 36), KZ=9, **PC),                      # chunk starts 1, 10, 19, 28
    case((16, 8, 40), KZ=10, **PC),                     # 1, 11, 21, 31
    case((18, 10, 44), KZ=11, **PC),                    # 1, 12, 23, 34
    case((20, 8, 52), KZ=13, **PC),                     # 1, 14, 27, 40
    case((17, 15, 5), KZ=5, halo=(4, 5, 3), **PC),      # unequal halos
    case((33, 29, 9), KZ=9, halo=(3, 6, 5), **PC),      # unequal strides
    # workgroup counts 2, 3, 5, 6, 7 (the others give 1, 4, 8 and 9): every residue modulo 8 of the XCD remap
    case((17, 8, 4), KZ=4, **PC),                       # 2 x 1
    case((33, 9, 4), KZ=4, **PC),                       # 3 x 1
    case((65, 8, 4), KZ=4, **PC),                       # 5 x 1
    case((33, 15, 4), KZ=4, **PC),                      # 3 x 2
    case((97, 8, 4), KZ=4, **PC),                       # 7 x 1
]

# ---- PC_FLAGS: the eight instantiations of momentum_tendencies_pc32 -------------------------------------------------------------------
# (has_zeta, flags): no G⁻; G⁻ with G stored; G⁻ with SKIP_G_STORE; CORRECT_ONLY -- each with own and with wrapped loads
VARIANTS = [(hz, fl | wr) for wr in (0, WRAPPED_LOADS) for hz, fl in ((0, 0), (1, 0), (1, SKIP_G_STORE), (0, CORRECT_ONLY))]
PC_FLAG_SIZES = [((33, 29, 9), 9), ((19, 9, 36), 9)]
PC_FLAGS = [case(size, KZ=KZ, has_zeta=hz, flags=fl, **PC) for size, KZ in PC_FLAG_SIZES for hz, fl in VARIANTS]

# ---- LONG_CHUNKS: OCN_TEND_MIN_BLOCKS=1, the chunk is the whole depth -----------------------------------------------------------------
LONG_PC = [case((16, 8, 17), KZ=17, **PC), case((17, 15, 36), KZ=36, **PC), case((16, 14, 64), KZ=64, **PC)]
LONG_PLAIN = [
    case((16, 14, 64), kind="tiled", patch=(17, 15), KZ=64),
    case((17, 15, 32), kind="tiled", patch=(32, 8), KZ=32, topo="PPB", z="stretched"),
    case((70, 9, 32), kind="tiled", patch=(32, 8), KZ=32, topo="PPB", z="stretched"),
]
LONG_TRACER = [case((33, 9, 64), kind="tiled", patch=(32, 8), KZ=64), case((33, 9, 32), kind="tiled", patch=(32, 8), KZ=32, topo="PPB", z="stretched")]
LONG_CHUNKS = LONG_PC + LONG_PLAIN + LONG_TRACER

# ---- STRIP_PATCHES: plain ranged launches of width 3 (one of width 2) on Nx = 16: the 4 x 64 patches (wy >= 64) --------------------------
# chunks of a strip: halved while longer than OCN_STRIP_MIN_KZ = 8 and fewer than 2048 workgroups: Nz = 20 -> 5, Nz = 9 -> 5 + 4, Nz = 8 -> 8
def _strip(Ny, Nz, rng_, topo):
    return case((16, Ny, Nz), kind="strip-patch", patch=(4, 64), KZ=8 if Nz == 8 else 5, topo=topo, z="stretched" if topo == "PPB" else None, range=rng_)


STRIP_PATCHES = []
for _topo in ("PPP", "PPB"):
    for _Ny, _Nz in ((64, 20), (126, 9), (127, 20)):    # two patches, the second owns one row; two exact; a third that owns one row
        STRIP_PATCHES += [_strip(_Ny, _Nz, (1, 3, 1, _Ny, 1, _Nz), _topo), _strip(_Ny, _Nz, (14, 16, 1, _Ny, 1, _Nz), _topo)]
    STRIP_PATCHES.append(_strip(64, 8, (15, 16, 1, 64, 1, 8), _topo))   # a range narrower than the patch, unchunked

# ---- SLABS: (nx per rank, Ny, Nz, R ranks): ocn_compute_momentum_tendencies_rk3_strips on the slabs of a global periodic box -----------
# narrow: the OCN_NARROW_TILE setting the case runs under (None: default switches); patch = what narrow_tile() then gives
ST = dict(kind="tiled", strips=True)
SLABS = [
    case((16, 14, 4), KZ=4, R=2, narrow=0, patch=(32, 8), **ST),
    case((16, 14, 4), KZ=4, R=2, narrow=1, patch=(17, 15), **ST),
    case((33, 15, 9), KZ=9, R=2, narrow=0, patch=(32, 8), **ST),
    case((33, 15, 9), KZ=9, R=2, narrow=1, patch=(17, 15), **ST),
    case((64, 29, 20), KZ=10, R=2, narrow=None, patch=(17, 15), **ST),   # the slab of one rank of eight: 64 = 4 x 16
]
SLAB_REFUSED = case((6, 8, 4), kind=None, patch=None, KZ=None, R=1, narrow=None, strips=True)   # wx >= 2 Hx but below 16: not a launch

# ---- the child processes of the GPU test: one per switch setting ----------------------------------------------------------------------
SETTINGS = {
    "addr32_off": {"OCN_TEND_ADDR32": "0"},        # PC_EDGES on the 64-bit kernel; flags 2 and 4 refused
    "min_blocks_1": {"OCN_TEND_MIN_BLOCKS": "1"},  # LONG_CHUNKS
    "narrow_0": {"OCN_NARROW_TILE": "0"},          # SLABS with narrow = 0
    "narrow_1": {"OCN_NARROW_TILE": "1"},          # SLABS with narrow = 1
}


# ---------------------------------------------------------------------------------------------------------------------------------------
# grids
# ---------------------------------------------------------------------------------------------------------------------------------------
def extents(c, Nx=None):
    """x, y, z of the case's grid: spacings DX, DY, DZ (Bounded z: helpers.stretched_faces)"""
    Nx0, Ny, Nz = c["size"]
    Nx = Nx0 if Nx is None else Nx
    z = stretched_faces(Nz) if c["z"] == "stretched" else (0.0, DZ * Nz)
    return dict(x=(0.0, DX * Nx), y=(0.0, DY * Ny), z=z)


def oracle_grid(O, c, Nx=None):
    size = c["size"] if Nx is None else (Nx,) + c["size"][1:]
    return O.Grid(size, topology=c["topo"], halo=c["halo"], **extents(c, Nx))


def product_grid(ocn, c, architecture, x_topology=None, x=None):
    """the product's RectilinearGrid of a case (architecture None: metadata only, no device); x_topology "FullyConnected" with the slab's
    own x interval: the local grid of one slab rank"""
    names = {"P": "Periodic", "B": "Bounded"}
    topo = tuple(names[t] for t in c["topo"])
    e = extents(c)
    if x_topology is not None:
        topo = (x_topology,) + topo[1:]
        e["x"] = x
    return ocn.RectilinearGrid(architecture, size=c["size"], topology=topo, halo=c["halo"], **e)


def plan_of(ocn, c, g=None, x_topology=None):
    """(status, plan) of ocn_momentum_tendencies_plan for the launch the case makes"""
    if g is None:   # metadata only, no device: a regular z stands for a stretched one (the decision does not read the spacings)
        g = product_grid(ocn, dict(c, z=None), None, x_topology, x=(0.0, DX * c["size"][0]))
    pc = c["kind"] == "pc32" or c.get("strips") or c.get("pc", False)
    return ocn._lib.momentum_tendencies_plan(g.c, range=c.get("range"), correct_on_load=pc, flags=c.get("flags") or 0, strips=bool(c.get("strips")))


def chunk_starts(c, plan):
    k0, k1 = (c["range"][4], c["range"][5]) if c.get("range") else (1, c["size"][2])
    return list(range(k0, k1 + 1, plan["KZ"]))


def chunk_lengths(c, plan):
    k1 = c["range"][5] if c.get("range") else c["size"][2]
    return [min(plan["KZ"], k1 - s + 1) for s in chunk_starts(c, plan)]


# ---------------------------------------------------------------------------------------------------------------------------------------
# inputs and the reference composition
# ---------------------------------------------------------------------------------------------------------------------------------------
def _readonly(a):
    a.setflags(write=False)
    return a


def _uniform(og, loc, rng, amplitude=1.0):
    a = og.zeros(loc)
    a[...] = amplitude * rng.uniform(-1, 1, a.shape)
    return a


def poison_halos(og, a, dims=(0, 1, 2)):
    """a copy of the parent array a with NaN in the halos of the given dimensions"""
    b = a.copy(order="F")
    H = (og.Hx, og.Hy, og.Hz)
    for d in dims:
        if H[d] == 0:
            continue
        sl = [slice(None)] * 3
        sl[d] = slice(0, H[d])
        b[tuple(sl)] = np.nan
        sl[d] = slice(b.shape[d] - H[d], None)
        b[tuple(sl)] = np.nan
    return b


def make_inputs(O, og, seed):
    """u, v, w (uncorrected) and G⁻: uniform [-1, 1] on whole parents, the halos of u, v, w then filled by the oracle; p of amplitude
    P_AMPLITUDE with periodic halos (the oracle's pressure_correct reads p[0]; the device gets them as NaN, poison_halos); c for the tracer
    cases.  Read-only."""
    rng = np.random.default_rng([*seed, 31])
    f = {n: _uniform(og, l, rng) for n, l in zip("uvw", LOCS)}
    for n, l in zip("uvw", LOCS):
        O.fill_halo_regions(og, f[n], l)
    f["Gm"] = [_uniform(og, l, rng) for l in LOCS]
    f["p"] = _uniform(og, 0, rng, P_AMPLITUDE)
    O.fill_halo_regions(og, f["p"], 0)
    f["c"] = _uniform(og, 0, rng)
    O.fill_halo_regions(og, f["c"], 0)
    for a in (f["u"], f["v"], f["w"], f["p"], f["c"], *f["Gm"]):
        _readonly(a)
    return f


def compose_reference(O, og, f, has_zeta, correct_only=False, p=None, dt=DT, dt_correct=DT_CORRECT):
    """(G, U_out, corrected U) as parent arrays, from the oracle's own pieces: pressure_correct on copies, fill_halo_regions,
    momentum_tendencies, rk3_substep.  p=None: the case's own p."""
    U = [f[n].copy(order="F") for n in "uvw"]
    O.pressure_correct(og, *U, f["p"] if p is None else p, dt_correct)
    for a, l in zip(U, LOCS):
        O.fill_halo_regions(og, a, l)
    G = [og.zeros(l) for l in LOCS]
    O.momentum_tendencies(og, *U, *G)
    if correct_only:
        return G, [a.copy(order="F") for a in U], U
    Uo = [a.copy(order="F") for a in U]
    for l, a, g, gm in zip(LOCS, Uo, G, f["Gm"]):
        O.rk3_substep(og, l, a, g, gm, dt, GAMMA, ZETA if has_zeta else None)
    return G, Uo, U


_store = {}


def setup(O, c, Nx=None):
    """(oracle grid, inputs) of a case, built once per (size, halo, topology) and shared; Nx: the global width of a slab case"""
    key = (c["size"] if Nx is None else (Nx,) + c["size"][1:], c["halo"], c["topo"], c["z"])
    if key not in _store:
        og = oracle_grid(O, c, Nx)
        _store[key] = (og, make_inputs(O, og, key[0] + key[1]), {})
    return _store[key]


def reference(O, c, has_zeta, correct_only=False, Nx=None):
    """compose_reference of a case, computed once and shared; read-only"""
    og, f, refs = setup(O, c, Nx)
    key = (bool(has_zeta), bool(correct_only))
    if key not in refs:
        refs[key] = tuple([_readonly(a) for a in part] for part in compose_reference(O, og, f, has_zeta, correct_only))
    return refs[key]


def interior_mask(og, shape, rng_=None):
    i0, i1, j0, j1, k0, k1 = rng_ if rng_ is not None else (1, og.Nx, 1, og.Ny, 1, og.Nz)
    m = np.zeros(shape, dtype=bool)
    m[og.Hx + i0 - 1:og.Hx + i1, og.Hy + j0 - 1:og.Hy + j1, og.Hz + k0 - 1:og.Hz + k1] = True
    return m


def compare(og, c, plan, name, got, want, rng_=None, skip_k1=False):
    """None when `got` equals `want` bit for bit on the interior (the range) and keeps SENTINEL outside; otherwise a message that names the
    worst cell with its indices modulo the columns a patch owns and its z chunk.  skip_k1: leave out the plane k = 1 (Gw at a wall face:
    written by a ranged launch, excluded by the oracle's :xyz)"""
    m = interior_mask(og, got.shape, rng_)
    if skip_k1:
        m[:, :, og.Hz] = False
    outside = ~interior_mask(og, got.shape, rng_)
    bad = m & ~((got == want) & (np.signbit(got) == np.signbit(want)))
    msgs = []
    if bad.any():
        err = np.where(bad, np.abs(got - want), -1.0)
        err[bad & ~np.isfinite(err)] = np.inf
        ip, jp, kp = (int(q) for q in np.unravel_index(int(np.argmax(err)), err.shape))
        i, j, k = ip - og.Hx + 1, jp - og.Hy + 1, kp - og.Hz + 1
        i0, j0, k0 = (rng_[0], rng_[2], rng_[4]) if rng_ is not None else (1, 1, 1)
        ox, oy = OWNED.get((plan["TX"], plan["TY"]), (plan["TX"], plan["TY"]))
        msgs.append(f"{name}: {np.count_nonzero(bad)} cells differ from the oracle, worst {err[ip, jp, kp]:.3e} at (i, j, k) = ({i}, {j}, {k}): "
                    f"got {got[ip, jp, kp]!r}, want {want[ip, jp, kp]!r}; mod the {ox} x {oy} owned columns ({(i - i0) % ox}, {(j - j0) % oy}), "
                    f"chunk {(k - k0) // plan['KZ']} plane {(k - k0) % plan['KZ']} of KZ = {plan['KZ']}")
    touched = outside & (got != SENTINEL)
    if touched.any():
        at = tuple(int(q) for q in np.argwhere(touched)[0])
        msgs.append(f"{name}: {np.count_nonzero(touched)} elements outside the written range lost the sentinel, first at parent index {at}")
    return "; ".join(msgs) or None


# ---------------------------------------------------------------------------------------------------------------------------------------
# slabs
# ---------------------------------------------------------------------------------------------------------------------------------------
def slab_inputs(O, c):
    """per rank r: the parent arrays of the local (FullyConnected, Periodic, Periodic) grid, copied from the filled global ones as the
    header prescribes: u, v, w uncorrected with periodic y / z halos and the neighbours' columns in x, column u[1 - Hx] already corrected;
    p with the neighbours' planes in its x halos and NaN in its y / z halos; G⁻.  Returns (global oracle grid, [dict per rank])."""
    nx, R = c["size"][0], c["R"]
    og, f, _ = setup(O, c, nx * R)
    _, _, U = reference(O, c, 1, Nx=nx * R)
    Hx = og.Hx
    ranks = []
    for r in range(R):
        cols = slice(r * nx, r * nx + nx + 2 * Hx)            # parent columns of the global arrays: local i = 1 - Hx .. nx + Hx
        d = {n: f[n][cols].copy(order="F") for n in "uvw"}
        d["u"][0] = U[0][cols][0]
        d["p"] = poison_halos(og, f["p"], dims=(1, 2))[cols].copy(order="F")
        d["Gm"] = [a[cols].copy(order="F") for a in f["Gm"]]
        ranks.append(d)
    return og, ranks


def expected_strips(og, c, Uo, r):
    """the two strip buffers of rank r as [h, parent row j, parent row k, field] arrays: the stepped u, v, w of the Hx westmost and eastmost
    columns on interior rows, NaN everywhere else"""
    nx, Hx = c["size"][0], og.Hx
    west, east = (np.full((Hx, og.Ny + 2 * og.Hy, og.Nz + 2 * og.Hz, 3), np.nan, order="F") for _ in range(2))
    rows = (slice(og.Hy, og.Hy + og.Ny), slice(og.Hz, og.Hz + og.Nz))
    for q in range(3):
        west[(slice(None), *rows, q)] = Uo[q][(slice(Hx + r * nx, 2 * Hx + r * nx), *rows)]
        east[(slice(None), *rows, q)] = Uo[q][(slice((r + 1) * nx, Hx + (r + 1) * nx), *rows)]
    return west, east


# ---------------------------------------------------------------------------------------------------------------------------------------
# fast math: the composition in np.longdouble and the local magnitudes
# ---------------------------------------------------------------------------------------------------------------------------------------
FAST_SIZES = [((33, 29, 9), 9), ((19, 9, 36), 9)]
FAST_INPUTS = ("noise", "smooth", "mean_T")
FAST_CASES = [case(size, KZ=KZ, has_zeta=hz, flags=fl, inp=inp, **PC) for size, KZ in FAST_SIZES for inp in FAST_INPUTS for hz, fl in VARIANTS]


@functools.lru_cache(maxsize=None)
def _fast_setup(size, inp):
    import fast_math_cases as FC
    from oracle import oracle as O
    c = case(size, KZ=None, **PC)
    og = oracle_grid(O, c)
    f = dict(FC.make(og, inp))
    sm = FC.make(og, "smooth")
    f["p"] = np.asfortranarray(1e-2 * sm["c"])                    # p = 1e-2 x smooth (halos filled)
    rng = np.random.default_rng([*size, 37])
    amp = max(float(np.abs(f[n]).max()) for n in "uvw")
    f["Gm"] = [_uniform(og, l, rng, amp * amp / DY) for l in LOCS]  # G⁻ of the size of the advective tendency of these fields
    for a in f.values():
        for b in (a if isinstance(a, list) else [a]):
            _readonly(b)
    return og, f


@functools.lru_cache(maxsize=None)
def fast_reference(size, inp, has_zeta, correct_only):
    """(og, f, G64, Uo64, Gext, Uoext, sG, sU): the Float64 composition, the same composition in np.longdouble (the fill and the tendencies
    from oracle/extended.py; the correction and the substep are the arithmetic below) and the local magnitudes, interior (1..N) arrays"""
    import fast_math_cases as FC
    from oracle import extended as X
    from oracle import oracle as O
    LD = np.longdouble
    og, f = _fast_setup(size, inp)
    G64, Uo64, _ = compose_reference(O, og, f, has_zeta, correct_only)
    p = X.widen(f["p"])
    U = [X.widen(f[n]) for n in "uvw"]
    h = (LD(og.dx), LD(og.dy), LD(og.dz))
    for d, (a, l) in enumerate(zip(U, LOCS)):
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[d], hi[d] = slice(0, -1), slice(1, None)
        a[tuple(hi)] = a[tuple(hi)] - ((p[tuple(hi)] - p[tuple(lo)]) / h[d]) * LD(DT_CORRECT)   # u - ((p[i] - p[i-1]) / Δx) dt_correct
        X.fill_halo_regions(og, a, l)
    Gext = X.momentum_tendencies(og, *U)
    if correct_only:
        Uoext = [a.copy(order="F") for a in U]
    elif has_zeta:
        Uoext = [a + LD(DT) * (LD(GAMMA) * g + LD(ZETA) * X.widen(gm)) for a, g, gm in zip(U, Gext, f["Gm"])]
    else:
        Uoext = [a + (LD(DT) * LD(GAMMA)) * g for a, g in zip(U, Gext)]
    sG = [FC.advective_scale(og, *U, a) for a in U]
    hmin = FC.smallest_spacing(og)
    dp = LD(DT_CORRECT) * FC.local_max_difference(og, p, 2) / hmin
    r = FC.halo_radius(og)
    sU = []
    for q, a in enumerate(U):
        s = FC.local_max(og, f["uvw"[q]], r) + dp
        if not correct_only:
            s = s + LD(DT) * (abs(LD(GAMMA)) * sG[q] + (abs(LD(ZETA)) * np.abs(X.widen(og.interior_N(f["Gm"][q]))) if has_zeta else 0))
        sU.append(s)
    return og, f, G64, Uo64, Gext, Uoext, sG, sU
