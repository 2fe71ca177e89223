"""The Smagorinsky / SmagorinskyLilly eddy viscosity restated in NumPy, operand for operand, on the oracle's parent arrays
([i, j, k], Fortran order, halos filled by oracle.fill_halo_regions):

  _compute_smagorinsky_viscosity!   Smagorinskys/smagorinsky.jl:88-102
  ΣᵢⱼΣᵢⱼᶜᶜᶜ                         Smagorinskys/scale_invariant_operators.jl:10-13
  Σ₁₂, Σ₁₃, Σ₂₃, tr_Σ²              velocity_tracer_gradients.jl:25-46, 78
  stability, square_smagorinsky_coefficient   Smagorinskys/lilly_coefficient.jl:126-139
  ∂z_b                              buoyancy_tracer.jl:16, seawater_buoyancy.jl:219-224

Nested-halves 2x2 averages (ℑy(ℑx), ℑz(ℑx), ℑz(ℑy)), left-associated sums, x^2 as x * x.  Along a Flat direction the reference's
differences are 0 and its interpolations return the value itself; here the shifted view along such a direction is the unshifted one, which
gives the same bits ((x - x) / Δ = 0, 0.5 (x + x) = x).  Also the seeded random inputs shared by the host and the GPU tests.

The arithmetic type is that of the velocity arrays: with np.longdouble parents (oracle/extended.py: widen) the metrics are widened too and
every operation, cbrt and sqrt included, is carried out in extended precision -- the same real function of the same Float64 inputs."""
import numpy as np

from oracle import oracle as O

# the cases of tests/test_gpu_smagorinsky.py: size, topology, z, halo
CASES = [((13, 17, 19), "PPP", (0, 1.0), (1, 2, 3)),        # GEN 0, partial tiles, minimum halo
         ((70, 9, 8), "PPB", (-1.0, 0.0), (3, 3, 3)),       # more than one tile in x, one z march
         ((16, 12, 10), "PPB", "stretched", (3, 3, 3)),     # per-k Δᶠ
         ((9, 10, 8), "BBB", "stretched", (3, 3, 3)),       # per-field strides
         ((12, 1, 8), "PFB", (-1.0, 0.0), (3, 3, 3))]       # Flat y
SEAWATER = ("SeawaterBuoyancy", 9.80665, 2e-4, 8e-4)
# coefficient settings: name, lilly, C, Cb, buoyancy
SETTINGS = [("number", False, 0.16, 0.0, None),
            ("lilly_b", True, 0.16, 1.0, "BuoyancyTracer"),
            ("lilly_TS", True, 0.23, 1.0, SEAWATER)]  # C = 0.23, Cb = 1: the reference's LES regression setup
HALF_CB = ("lilly_TS_Cb0.5", True, 0.23, 0.5, SEAWATER)
SEED = 4711


def stretched_faces(Nz, Lz=1.0, power=1.6):
    s = np.linspace(0.0, 1.0, Nz + 1)
    return -Lz * (1 - s) ** power


def case_z(size, z):
    return stretched_faces(size[2]) if isinstance(z, str) else z


def _sh(og, a, di, dj, dk):
    """a[i + di, j + dj, k + dk] for every interior cell (i, j, k) = (1..Nx, 1..Ny, 1..Nz)"""
    H, N = (og.Hx, og.Hy, og.Hz), (og.Nx, og.Ny, og.Nz)
    sl = []
    for d, s in enumerate((di, dj, dk)):
        if og.topo[d] == O.FLAT:
            s = 0
        sl.append(slice(H[d] + s, H[d] + s + N[d]))
    return a[tuple(sl)]


def _dz(og, face, dk, dtype=np.float64):
    """Δzᵃᵃᶜ (face = False) or Δzᵃᵃᶠ (True) at levels k + dk, k = 1..Nz, broadcastable over the interior"""
    if og.dzc is None:
        return dtype(og.dz)
    a = og.dzf if face else og.dzc  # element 0 <-> k = 1 - Hz
    return a[og.Hz + dk:og.Hz + dk + og.Nz].reshape(1, 1, -1).astype(dtype)


def strain_dot(og, u, v, w):
    """ΣᵢⱼΣᵢⱼᶜᶜᶜ over the interior"""
    ft = u.dtype.type
    dx, dy = ft(og.dx), ft(og.dy)
    dzc, dzf = _dz(og, False, 0, ft), (_dz(og, True, 0, ft), _dz(og, True, 1, ft))
    U = lambda a, b, d: _sh(og, u, a, b, d)
    V = lambda a, b, d: _sh(og, v, a, b, d)
    W = lambda a, b, d: _sh(og, w, a, b, d)
    dxu = (U(1, 0, 0) - U(0, 0, 0)) / dx
    dyv = (V(0, 1, 0) - V(0, 0, 0)) / dy
    dzw = (W(0, 0, 1) - W(0, 0, 0)) / dzc
    tr = (dxu * dxu + dyv * dyv) + dzw * dzw

    def s12(a, b):  # Σ₁₂ at (i + a, j + b, k), ffc
        return 0.5 * ((U(a, b, 0) - U(a, b - 1, 0)) / dy + (V(a, b, 0) - V(a - 1, b, 0)) / dx)

    def s13(a, d):  # Σ₁₃ at (i + a, j, k + d), fcf
        return 0.5 * ((U(a, 0, d) - U(a, 0, d - 1)) / dzf[d] + (W(a, 0, d) - W(a - 1, 0, d)) / dx)

    def s23(b, d):  # Σ₂₃ at (i, j + b, k + d), cff
        return 0.5 * ((V(0, b, d) - V(0, b, d - 1)) / dzf[d] + (W(0, b, d) - W(0, b - 1, d)) / dy)

    def i4sq(f):  # outer(inner(f²)): 0.5 (0.5 (f00² + f10²) + 0.5 (f01² + f11²)), first index inner
        q = lambda a, b: f(a, b) * f(a, b)
        return 0.5 * (0.5 * (q(0, 0) + q(1, 0)) + 0.5 * (q(0, 1) + q(1, 1)))

    return ((tr + 2 * i4sq(s12)) + 2 * i4sq(s13)) + 2 * i4sq(s23)


def buoyancy_frequency(og, buoyancy, T, S):
    """ℑzᵃᵃᶜ(∂z_b) over the interior; buoyancy as oracle.Physics takes it; a missing (constant) T or S has derivative 0"""
    if buoyancy is None:
        return np.zeros((og.Nx, og.Ny, og.Nz))

    ft = (T if T is not None else S).dtype.type

    def dzb(d):
        dzf = _dz(og, True, d, ft)
        dT = 0.0 if T is None else (_sh(og, T, 0, 0, d) - _sh(og, T, 0, 0, d - 1)) / dzf
        dS = 0.0 if S is None else (_sh(og, S, 0, 0, d) - _sh(og, S, 0, 0, d - 1)) / dzf
        if buoyancy == "BuoyancyTracer":
            return dT
        _, g, alpha, beta = buoyancy[:4]
        return g * (alpha * dT - beta * dS)

    return 0.5 * (dzb(0) + dzb(1))


def smagorinsky_viscosity(og, u, v, w, C, lilly=False, Cb=0.0, buoyancy=None, T=None, S=None, parts=False):
    """νₑ over the interior (Nx, Ny, Nz); parts: also Σ², N², ς"""
    S2 = strain_dot(og, u, v, w)
    ft = u.dtype.type
    Df = np.cbrt((ft(og.dx) * ft(og.dy)) * _dz(og, False, 0, ft))
    N2 = sig = None
    if lilly:
        N2 = buoyancy_frequency(og, buoyancy, T, S)
        N2p = np.where(N2 > 0, N2, 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            sig = np.where(S2 == 0, 0.0, np.sqrt(1.0 - np.minimum(1.0, Cb * N2p / S2)))
        cs2 = sig * (C * C)
    else:
        cs2 = C * C
    nu = cs2 * (Df * Df) * np.sqrt(2 * S2)
    nu = np.broadcast_to(nu, (og.Nx, og.Ny, og.Nz))
    return (nu, S2, N2, sig) if parts else nu


def random_inputs(og, buoyancy):
    """Seeded velocities and buoyancy tracers (parent arrays, halos filled with the default conditions) that reach every branch of the
    closure: u, v, w vanish in a 4 x 4 x 4 block of cells including its faces (Σ² == 0 in the block's core), and the tracer amplitude puts
    Cb N² on both sides of Σ² (N² ~ amplitude / Δz against Σ² ~ (1 / Δ)² for velocities of order one)."""
    rng = np.random.default_rng(SEED)
    N = (og.Nx, og.Ny, og.Nz)
    fields = {}
    for name, loc in (("u", 1), ("v", 2), ("w", 4)):
        a = og.zeros(loc)
        og.interior(a)[...] = rng.uniform(-1, 1, og.interior(a).shape)
        lo = [1 if n >= 6 else 0 for n in N]            # block of cells lo .. lo + 3 (0-based interior index), clipped to the grid
        hi = [min(l + 4, n) for l, n in zip(lo, N)]
        ext = [1 if (loc >> d) & 1 else 0 for d in range(3)]  # ... including the faces on its far side
        og.interior(a)[lo[0]:hi[0] + ext[0], lo[1]:hi[1] + ext[1], lo[2]:hi[2] + ext[2]] = 0.0
        O.fill_halo_regions(og, a, loc)
        fields[name] = a
    dzmin = og.dz if og.dzc is None else float(np.min(og.dzc[og.Hz:og.Hz + og.Nz]))
    spacings = [s for s, t in zip((og.dx, og.dy, dzmin), og.topo) if t != O.FLAT]
    amp = 1.0 / min(spacings)  # δb ~ amp  =>  N² ~ amp / Δz ~ Σ²
    T = S = None
    if buoyancy == "BuoyancyTracer":
        T = og.zeros(0)
        og.interior(T)[...] = amp * rng.uniform(-1, 1, N)
    elif buoyancy is not None:
        _, g, alpha, beta = buoyancy[:4]
        T, S = og.zeros(0), og.zeros(0)
        og.interior(T)[...] = 20 + amp / (g * alpha) * rng.uniform(-1, 1, N)
        og.interior(S)[...] = 35 + 0.5 * amp / (g * beta) * rng.uniform(-1, 1, N)
    for a in (T, S):
        if a is not None:
            O.fill_halo_regions(og, a, 0)
    fields["T"], fields["S"] = T, S
    return fields
