"""Stokes drift of a horizontally uniform surface-wave field (src/StokesDrifts.jl:36-180).

    UniformStokesDrift(; ∂z_uˢ, ∂z_vˢ, ∂t_uˢ, ∂t_vˢ, parameters)      -> UniformStokesDrift(dz_us=, dz_vs=, dt_us=, dt_vs=, parameters=)
    UniformStokesDrift(grid; ∂z_uˢ = Field{Nothing, Nothing, Face}...) -> UniformStokesDrift(grid, dz_us=array, ...)

`∂` is not a legal character of a Python identifier, hence the ASCII keywords: dz_us = ∂z_uˢ, dz_vs = ∂z_vˢ, dt_us = ∂t_uˢ, dt_vs = ∂t_vˢ.

The momentum tendencies gain, after the closure term (nonhydrostatic_tendency_kernel_functions.jl:73-74, 135-136, 197-198),
    Gu += ℑxzᶠᵃᶜ(w) ∂z_uˢ(z centre, t) + ∂t_uˢ(z centre, t),   Gv += ℑyzᵃᶠᶜ(w) ∂z_vˢ(z centre, t) + ∂t_vˢ(z centre, t),
    Gw += -ℑxzᶜᵃᶠ(u) ∂z_uˢ(z face, t) - ℑyzᵃᶜᶠ(v) ∂z_vˢ(z face, t)
inside the finishing pass of the momentum tendencies (csrc/physics.hip, csrc/general.hip).  The device only ever sees six small vectors
(struct ocn_stokes_drift): the host samples every profile on the grid's z centres and z faces.

When are the profiles sampled?  ONE rule: `steady`.  A steady drift is sampled once, when the model is built (at t = 0); any other
drift is resampled at clock.time before every tendency evaluation -- every RK3 stage included, exactly as the function-valued boundary
conditions are.  `steady` defaults to True when every profile is an array, a number or None (nothing to re-evaluate) and to False as soon as
one of them is a function; pass steady=True for functions that ignore `t` (the Langmuir example does), which is also what
ModelRK3Driver requires.
"""
import numpy as np

_NAMES = ("dz_us", "dz_vs", "dt_us", "dt_vs")


def _prettysummary(x):
    """prettysummary(x, false) of src/Utils/prettysummary.jl for what a profile can be here"""
    if x is None:
        return "zerofunction"  # the reference's default profile
    if callable(x):
        return getattr(x, "__name__", type(x).__name__)
    if isinstance(x, np.ndarray):
        return f"{x.size}-element Vector{{Float64}}"
    return repr(x)


def _parameters_summary(p):
    """prettysummary of a NamedTuple: (a=1, b=2)"""
    if hasattr(p, "_asdict"):
        p = p._asdict()
    elif not isinstance(p, dict) and hasattr(p, "__dict__"):
        p = vars(p)
    if isinstance(p, dict):
        return "(" + ", ".join(f"{k}={v!r}" for k, v in p.items()) + ")"
    return repr(p)


class StokesDrift:
    """StokesDrift(; ∂x_vˢ, ∂x_wˢ, ∂y_uˢ, ∂y_wˢ, ∂z_uˢ, ∂z_vˢ, ∂t_uˢ, ∂t_vˢ, ∂t_wˢ) (StokesDrifts.jl:182-290): profiles that depend on
    x, y are not implemented -- the kernels read per-level numbers."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError("StokesDrift with x- / y-dependent profiles is not implemented; UniformStokesDrift is (see DESIGN.md §10)")


class UniformStokesDrift:
    """UniformStokesDrift(dz_us=None, dz_vs=None, dt_us=None, dt_vs=None, parameters=None, steady=None)   [∂z_uˢ, ∂z_vˢ, ∂t_uˢ, ∂t_vˢ]
    UniformStokesDrift(grid, dz_us=..., ...)

    Without a grid the profiles are functions `(z, t)`, or `(z, t, parameters)` when `parameters` is not None (numbers are taken as
    constants).  Each is called ONCE per sampling with the NumPy vector of the z nodes; a function that cannot take a vector (math.exp ...)
    is then called node by node with np.float64 arguments.
    With a grid they are arrays, as the reference's reduced Fields: dz_us / dz_vs on the z faces (Nz + 1 values; Nz on a Periodic z, where
    face Nz + 1 is face 1), dt_us / dt_vs on the z centres (Nz values).  At the centres ∂z_uˢ is then ℑzᵃᵃᶜ of the face array
    (StokesDrifts.jl:150-151).
    None is the reference's `zerofunction` / `nothing`: the term is zero.  See the module docstring for `steady`."""

    def __init__(self, grid=None, dz_us=None, dz_vs=None, dt_us=None, dt_vs=None, parameters=None, steady=None):
        self.grid = grid
        self.parameters = parameters
        given = {"dz_us": dz_us, "dz_vs": dz_vs, "dt_us": dt_us, "dt_vs": dt_vs}
        for name, p in given.items():
            if p is None:
                continue
            if callable(p):
                if grid is not None:
                    raise TypeError(f"UniformStokesDrift(grid, ...): {name} must be an array on the grid's z nodes (functions go without a grid)")
                continue
            if grid is None:
                if not isinstance(p, (int, float, np.floating, np.integer)):
                    raise TypeError(f"UniformStokesDrift: {name} must be a function of (z, t[, parameters]), a number or None; "
                                    "arrays need the grid form UniformStokesDrift(grid, ...)")
                given[name] = float(p)
                continue
            a = np.ascontiguousarray(np.asarray(p, dtype=np.float64).reshape(-1))
            Nz, periodic, face = grid.Nz, grid.topology[2] == "Periodic", name.startswith("dz")
            want = ((Nz + 1, Nz) if periodic else (Nz + 1,)) if face else (Nz,)
            if a.size not in want:
                raise ValueError(f"UniformStokesDrift(grid, ...): {name} has {a.size} values, expected {' or '.join(map(str, want))} "
                                 f"({'z faces' if face else 'z centres'})")
            given[name] = a
        self.dz_us, self.dz_vs, self.dt_us, self.dt_vs = (given[n] for n in _NAMES)
        has_function = any(callable(given[n]) for n in _NAMES)
        self.steady = (not has_function) if steady is None else bool(steady)
        if not self.steady and not has_function:
            raise ValueError("UniformStokesDrift: steady=False needs at least one function profile")

    # ---- show
    def summary(self):
        if self.parameters is None:
            return "UniformStokesDrift{Nothing}"
        return f"UniformStokesDrift with parameters {_parameters_summary(self.parameters)}"

    def __repr__(self):
        """Base.show(io, ::UniformStokesDrift) (StokesDrifts.jl:63-69)"""
        return (f"{self.summary()}:\n"
                f"├── ∂z_uˢ: {_prettysummary(self.dz_us)}\n"
                f"├── ∂z_vˢ: {_prettysummary(self.dz_vs)}\n"
                f"├── ∂t_uˢ: {_prettysummary(self.dt_us)}\n"
                f"└── ∂t_vˢ: {_prettysummary(self.dt_vs)}")

    # ---- sampling
    def _evaluate(self, f, z, t):
        args = (t,) if self.parameters is None else (t, self.parameters)
        try:
            v = np.asarray(f(z, *args), dtype=np.float64)
            if v.shape == z.shape:
                return np.ascontiguousarray(v)
            if v.shape == ():
                return np.full(z.shape, float(v))
        except (TypeError, ValueError):
            pass
        return np.array([float(f(np.float64(zk), *args)) for zk in z], dtype=np.float64)

    def sample(self, grid, t=0.0):
        """The six host vectors of struct ocn_stokes_drift at time t: {dz_us_center, dz_vs_center, dz_us_face, dz_vs_face, dt_us, dt_vs}
        (None where the profile is None).  Centres: Nz values; faces: Nz + 1 (znode(k, grid, Face), k = 1 .. Nz + 1)."""
        if grid.topology[2] == "Flat":
            raise NotImplementedError("UniformStokesDrift needs a non-Flat z")
        zc, zf = z_nodes(grid)
        out = {}
        for comp in ("us", "vs"):
            dz, dt = getattr(self, "dz_" + comp), getattr(self, "dt_" + comp)
            if dz is None:
                out[f"dz_{comp}_center"] = out[f"dz_{comp}_face"] = None
            elif callable(dz):
                out[f"dz_{comp}_center"], out[f"dz_{comp}_face"] = self._evaluate(dz, zc, t), self._evaluate(dz, zf, t)
            elif isinstance(dz, float):
                out[f"dz_{comp}_center"], out[f"dz_{comp}_face"] = np.full(zc.shape, dz), np.full(zf.shape, dz)
            else:
                face = dz if dz.size == grid.Nz + 1 else np.concatenate([dz, dz[:1]])  # Periodic z: face Nz + 1 is face 1
                out[f"dz_{comp}_face"] = np.ascontiguousarray(face)
                out[f"dz_{comp}_center"] = 0.5 * (face[:-1] + face[1:])  # ℑzᵃᵃᶜ
            if dt is None:
                out[f"dt_{comp}"] = None
            elif callable(dt):
                out[f"dt_{comp}"] = self._evaluate(dt, zc, t)
            elif isinstance(dt, float):
                out[f"dt_{comp}"] = np.full(zc.shape, dt)
            else:
                out[f"dt_{comp}"] = dt
        return out


FIELDS = ("dz_us_center", "dz_vs_center", "dz_us_face", "dz_vs_face", "dt_us", "dt_vs")  # order of struct ocn_stokes_drift


def z_nodes(grid):
    """(z centres k = 1 .. Nz, z faces k = 1 .. Nz + 1) of the grid: znode(k, grid, Center()), znode(k, grid, Face())"""
    H, N = grid.Hz, grid.Nz
    zf = np.ascontiguousarray(np.asarray(grid.nodes_1d(2, True, with_halos=True))[H:H + N + 1])
    zc = np.ascontiguousarray(grid.nodes_1d(2, False))
    if zf.size != N + 1:
        raise NotImplementedError("UniformStokesDrift needs a z halo of at least 1")
    return zc, zf


class DeviceStokesDrift:
    """The device side of a model's UniformStokesDrift: the six vectors (allocated once, so struct ocn_stokes_drift never changes) and
    their refresh at clock.time for profiles that depend on time."""

    def __init__(self, drift, grid):
        from . import _lib
        from .architectures import on_architecture
        self.drift, self.grid = drift, grid
        host = drift.sample(grid, 0.0)
        self.vectors = {n: (None if host[n] is None else on_architecture(grid.architecture, host[n])) for n in FIELDS}
        self.c = _lib.CStokesDrift(*[(None if self.vectors[n] is None else self.vectors[n].data_ptr()) for n in FIELDS])
        self.time = 0.0

    def refresh(self, t):
        """time-dependent profiles: resample at t into the same device vectors (stream-ordered copies)"""
        if self.drift.steady or t == self.time:
            return
        import torch
        host = self.drift.sample(self.grid, t)
        for n in FIELDS:
            if self.vectors[n] is not None:
                self.vectors[n].copy_(torch.from_numpy(host[n]))
        self.time = t
