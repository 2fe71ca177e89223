"""Structured inputs for the accuracy tests of the fast-math kernels (tests/test_oracle_extended.py on the host,
tests/test_gpu_fast_math_accuracy.py on the GPU), and the per-cell local magnitudes their errors are measured against.

Every case is a dict of Float64 parent arrays u, v, w, c ([i, j, k], Fortran order) on an oracle.Grid, seeded, with the halos filled by
the oracle under the default boundary conditions (wall-normal velocities vanish on the walls):

  noise          uniform [-1, 1]: the input of the older fast-math tests, kept as the baseline
  smooth         products of sines in index space, at least 8 cells per wavelength, amplitude 1 (see _smooth)
  mean_T, mean_S velocities 10 + 1e-3 smooth; tracer 20 + 1e-3 smooth (temperature-like), 35 + 1e-6 smooth (salinity-like)
  front_x, front_z  a tanh step one cell wide across the middle of x (z): 0.75 + 0.25 smooth on one side, 1e-8 noise on the other
  aspect         u, v ~ 1, w ~ 1e-6 (ocean aspect ratio), tracer ~ 1
  rest, rest_one exact zeros; zeros with one nonzero cell per field
  patchy         smooth times a mask that is exactly 0 in one octant (faces included), so that the q == 0 / σ == 0 / Σ² == 0 /
                 zero-advecting-velocity branches and the general path meet inside one launch
  scale_<f>      smooth times f, f in SCALES
  patchy_1e-160  patchy times 1e-160: denominators that are exactly 0 next to subnormal ones
"""
import numpy as np

from oracle import oracle as O

LD = np.longdouble
EPS = 2.0 ** -52
LOCS = {"u": O.LOC_U, "v": O.LOC_V, "w": O.LOC_W, "c": O.LOC_C}
SCALES = (1e-160, 1e-100, 1e-30, 1e-12, 1e20)
NAMES = ("noise", "smooth", "mean_T", "mean_S", "front_x", "front_z", "aspect", "rest", "rest_one", "patchy") + tuple(
    f"scale_{f:g}" for f in SCALES) + ("patchy_1e-160",)
SEED = 20260


def _xi(og, d, face, n):
    """index-space coordinate of the n points of a parent axis: (cell index - 1 [+ 1/2 at centres]) / N, halos included"""
    N, H = (og.Nx, og.Ny, og.Nz)[d], (og.Hx, og.Hy, og.Hz)[d]
    return (np.arange(n) - H + (0.0 if face else 0.5)) / N


def _smooth(og, loc, rng):
    """sin(2π m ξ + φ) along every direction with at least 8 cells (m = 1 below 32 cells, 2 from there: at least 8 cells per wavelength),
    1 along the others; random phases; filled everywhere, then the halos are overwritten by the fill"""
    a = og.zeros(loc)
    shape = a.shape
    f = np.ones(shape)
    for d in range(3):
        N = (og.Nx, og.Ny, og.Nz)[d]
        if og.topo[d] == O.FLAT or N < 8:
            continue
        m = 2 if N >= 32 else 1
        s = np.sin(2 * np.pi * m * _xi(og, d, (loc >> d) & 1, shape[d]) + rng.uniform(0, 2 * np.pi))
        f = f * s.reshape([-1 if e == d else 1 for e in range(3)])
    a[...] = f
    return a


def _noise(og, loc, rng):
    a = og.zeros(loc)
    a[...] = rng.uniform(-1, 1, a.shape)
    return a


def _step(og, loc, d):
    """0.5 (1 + tanh(cells from the middle of direction d)): a step one cell wide"""
    n = og.shape(loc)[d]
    N = (og.Nx, og.Ny, og.Nz)[d]
    t = 0.5 * (1 + np.tanh((_xi(og, d, (loc >> d) & 1, n) - 0.5) * N))
    return t.reshape([-1 if e == d else 1 for e in range(3)])


def _octant_mask(og, loc):
    """1 everywhere except the octant i <= Nx/2, j <= Ny/2, k <= Nz/2 (faces on its far side included), where it is exactly 0"""
    m = np.ones(og.shape(loc))
    H, N = (og.Hx, og.Hy, og.Hz), (og.Nx, og.Ny, og.Nz)
    sl = []
    for d in range(3):
        if og.topo[d] == O.FLAT:
            sl.append(slice(None))
        else:
            sl.append(slice(0, H[d] + N[d] // 2 + ((loc >> d) & 1)))
    m[tuple(sl)] = 0.0
    return m


def make(og, name, seed=SEED):
    """the fields of case `name` on the oracle grid og"""
    rng = np.random.default_rng(seed)
    sm = {n: _smooth(og, l, rng) for n, l in LOCS.items()}
    no = {n: _noise(og, l, rng) for n, l in LOCS.items()}
    if name == "noise":
        f = no
    elif name == "smooth":
        f = sm
    elif name in ("mean_T", "mean_S"):
        f = {n: 10 + 1e-3 * sm[n] for n in "uvw"}
        f["c"] = 20 + 1e-3 * sm["c"] if name == "mean_T" else 35 + 1e-6 * sm["c"]
    elif name in ("front_x", "front_z"):
        d = 0 if name == "front_x" else 2
        f = {}
        for n, l in LOCS.items():
            t, lo = _step(og, l, d), 1e-8 * no[n]
            f[n] = lo + t * ((0.75 + 0.25 * sm[n]) - lo)
    elif name == "aspect":
        f = dict(sm)
        f["w"] = 1e-6 * sm["w"]
    elif name in ("rest", "rest_one"):
        f = {n: og.zeros(l) for n, l in LOCS.items()}
        if name == "rest_one":
            for q, (n, l) in enumerate(LOCS.items()):  # a different cell for every field, away from the walls
                og.interior_N(f[n])[og.Nx // 2 + (q & 1), og.Ny // 2, og.Nz // 2 - (q >> 1 if og.Nz > 2 else 0)] = 1.0 + 0.25 * q
    elif name in ("patchy", "patchy_1e-160"):
        a = 1.0 if name == "patchy" else 1e-160
        f = {n: a * sm[n] * _octant_mask(og, l) for n, l in LOCS.items()}
    elif name.startswith("scale_"):
        s = float(name[6:])
        f = {n: s * sm[n] for n in LOCS}
    else:
        raise KeyError(name)
    out = {}
    for n, l in LOCS.items():
        a = np.asfortranarray(f[n], dtype=np.float64)
        O.fill_halo_regions(og, a, l)
        out[n] = a
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# local magnitudes (np.longdouble: a product of two values of 1e-160 must not underflow), over the cells (1..Nx, 1..Ny, 1..Nz)
# ---------------------------------------------------------------------------------------------------------------------------------
def _window_max(a, r):
    """max of a over the (2r+1)³ neighbourhood of every element (clipped at the array's edges)"""
    for d in range(3):
        n = a.shape[d]
        if n == 1:
            continue
        out = a.copy()
        for s in range(1, min(r, n - 1) + 1):
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[d], hi[d] = slice(0, n - s), slice(s, n)
            lo, hi = tuple(lo), tuple(hi)
            out[lo] = np.maximum(out[lo], a[hi])
            out[hi] = np.maximum(out[hi], a[lo])
        a = out
    return a


def local_max(og, a, r):
    """largest |a| in the (2r+1)³ neighbourhood, at the cells (1..Nx, 1..Ny, 1..Nz)"""
    return np.array(og.interior_N(_window_max(np.abs(np.asarray(a, dtype=LD)), r)))


def local_max_difference(og, a, r):
    """largest |difference of two neighbouring values of a| in the (2r+1)³ neighbourhood"""
    a = np.asarray(a, dtype=LD)
    D = np.zeros(a.shape, dtype=LD)
    for d in range(3):
        if a.shape[d] == 1:
            continue
        df = np.abs(np.diff(a, axis=d))
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[d], hi[d] = slice(0, -1), slice(1, None)
        D[tuple(lo)] = np.maximum(D[tuple(lo)], df)
        D[tuple(hi)] = np.maximum(D[tuple(hi)], df)
    return np.array(og.interior_N(_window_max(D, r)))


def smallest_spacing(og):
    """min over the non-Flat directions of Δx, Δy, Δzᶜ(k), Δzᶠ(k), Δzᶠ(k+1), shape (1, 1, Nz)"""
    d = [LD(s) for s, t in zip((og.dx, og.dy), og.topo) if t != O.FLAT]
    h = np.full(og.Nz, min(d) if d else LD(np.inf), dtype=LD)
    if og.tz != O.FLAT:
        if og.dzc is None:
            h = np.minimum(h, LD(og.dz))
        else:
            H = og.Hz
            for a in (og.dzc[H:H + og.Nz], og.dzf[H:H + og.Nz], og.dzf[H + 1:H + 1 + og.Nz]):
                h = np.minimum(h, a.astype(LD))
    return h.reshape(1, 1, -1)


def halo_radius(og):
    return max(og.Hx, og.Hy, og.Hz)


def advective_scale(og, u, v, w, q):
    """(largest |u|, |v|, |w| in the (2H+1)³ neighbourhood) x (largest |q| there) / (smallest spacing of the cell)"""
    r = halo_radius(og)
    U = np.maximum(np.maximum(local_max(og, u, r), local_max(og, v, r)), local_max(og, w, r))
    return U * local_max(og, q, r) / smallest_spacing(og)


def diffusive_scale(og, kmax, q):
    """(largest diffusivity) x (largest |difference of neighbouring q| in the 5³ neighbourhood) / (smallest spacing)²; kmax a number or
    a field"""
    h = smallest_spacing(og)
    k = LD(kmax) if np.isscalar(kmax) else local_max(og, kmax, 2)
    return k * local_max_difference(og, q, 2) / (h * h)


def eddy_scale(og, C_delta2, u, v, w):
    """C Δ² x (largest |velocity difference| in the 5³ neighbourhood) / (smallest spacing); C_delta2: a number or (1, 1, Nz)"""
    D = np.maximum(np.maximum(local_max_difference(og, u, 2), local_max_difference(og, v, 2)), local_max_difference(og, w, 2))
    return np.asarray(C_delta2, dtype=LD) * D / smallest_spacing(og)


def error_in_eps(got, ext, s):
    """max over the cells with s > 0 of |got - ext| / (ε s), its location, and whether got == ext wherever s == 0"""
    got, ext = np.asarray(got, dtype=LD), np.asarray(ext, dtype=LD)
    pos = s > 0
    exact0 = bool(np.all(got[~pos] == ext[~pos]))
    if not pos.any():
        return 0.0, (0, 0, 0), exact0
    e = np.zeros(s.shape, dtype=LD)
    e[pos] = np.abs(got - ext)[pos] / (LD(EPS) * s[pos])
    at = np.unravel_index(int(np.argmax(e)), e.shape)
    return float(e[at]), tuple(int(q) + 1 for q in at), exact0
