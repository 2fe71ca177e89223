#!/usr/bin/env python3
"""Flux boundary conditions with field_dependencies (quadratic bottom drag) at config 4's grid (512 x 512 x 256, stretched z):

  tools/bench_boundary_functions.py [Nx] [Nz] [steps] [rounds]

1. the evaluation kernel alone (device events around repeated launches): drag_u on the Nx x Nx bottom plane, with its achieved bytes/s
   against its minimum traffic of 48 B per point (u once, v at four points of which three are shared with the neighbours: 8 + 8 read,
   8 written, counted generously as 8 x (1 + 4 + 1));
2. one RK3 step of the config-4-like model (tools/bench_config4.py physics = 1: SeawaterBuoyancy, T and S, FPlane, wind stress, heat
   flux, ScalarDiffusivity), three ways in this one process on this one device:
     a. without bottom conditions on u and v              (fused stage boundaries)
     b. with array-valued bottom conditions on u and v    (fused)
     c. the same with OCN_FUSE_GENERAL=0                  (the reference's launch sequence: what a model with drag laws runs)
     d. with drag_u / drag_v                              (the reference's launch sequence + two evaluation launches per update_state!)
     e. as d with the evaluation launches skipped          (the values stay frozen: d - e is the evaluation alone)
   c - b is what the unfused sequence costs, d - c what the evaluation adds on top of it.  All five models are built first (about 12 GB
   each at the default size) and then take turns, one timing window of `steps` steps at a time, `rounds` times: the median window is the
   figure, min .. max its spread.
Prints one line per figure."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import oceananigans_jl_amd as ocn

Nx = int(sys.argv[1]) if len(sys.argv) > 1 else 512
Nz = int(sys.argv[2]) if len(sys.argv) > 2 else 256
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 5
Lz, refinement, stretching = 32.0, 1.2, 12.0
h = lambda k: (k - 1) / Nz
zeta0 = lambda k: 1 + (h(k) - 1) / refinement
Sigma = lambda k: (1 - np.exp(-stretching * h(k))) / (1 - np.exp(-stretching))
z_faces = np.array([Lz * (zeta0(k) * Sigma(k) - 1) for k in range(1, Nz + 2)])
ocn.set_math_mode(ocn.MATH_FAST)
g = ocn.RectilinearGrid(ocn.GPU(), size=(Nx, Nx, Nz), x=(0, 64), y=(0, 64), z=z_faces, topology=("Periodic", "Periodic", "Bounded"), halo=(3, 3, 3))

# the tilted-bottom-boundary-layer example's drag law (examples/tilted_bottom_boundary_layer.jl:110-126)
z1 = 0.5 * (z_faces[0] + z_faces[1]) - z_faces[0]
parameters = dict(cd=(0.4 / np.log(z1 / 1e-4)) ** 2, V=0.1)


def drag_u(x, y, t, u, v, p):
    return -p["cd"] * ocn.sqrt(u ** 2 + (v + p["V"]) ** 2) * u


def drag_v(x, y, t, u, v, p):
    return -p["cd"] * ocn.sqrt(u ** 2 + (v + p["V"]) ** 2) * (v + p["V"])


def device_ms(call, repeats=50):
    call(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(repeats):
        call()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / repeats


def model(bottom):
    """bottom: None, "array" or "function" """
    Q, rho, cp, dTdz = 200.0, 1026.0, 3991.0, 0.01
    taux = -1.225 / rho * 2.5e-3 * 10 * 10
    flux = lambda f: ocn.FluxBoundaryCondition(f, field_dependencies=("u", "v"), parameters=parameters)
    bottom_u = {None: {}, "array": dict(bottom=ocn.FluxBoundaryCondition(np.full((Nx, Nx), -1e-6))), "function": dict(bottom=flux(drag_u))}[bottom]
    bottom_v = {None: {}, "array": dict(bottom=ocn.FluxBoundaryCondition(np.full((Nx, Nx), -1e-6))), "function": dict(bottom=flux(drag_v))}[bottom]
    bcs = {"u": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(taux), **bottom_u),
           "T": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(Q / (rho * cp)), bottom=ocn.GradientBoundaryCondition(dTdz)),
           "S": ocn.FieldBoundaryConditions(top=ocn.FluxBoundaryCondition(0.0, coeff=-1e-3 / 3600))}
    if bottom_v:
        bcs["v"] = ocn.FieldBoundaryConditions(**bottom_v)
    m = ocn.NonhydrostaticModel(g, advection=ocn.WENO(), tracers=("T", "S"), coriolis=ocn.FPlane(f=1e-4), closure=ocn.ScalarDiffusivity(ν=1e-4, κ=1e-4),
                                buoyancy=ocn.SeawaterBuoyancy(equation_of_state=ocn.LinearEquationOfState(2e-4, 8e-4)), boundary_conditions=bcs)
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    zc = 0.5 * (z_faces[1:] + z_faces[:-1])
    T = m.field("T").interior_view()
    T.copy_(torch.from_numpy(20 + dTdz * zc)[:, None, None].to("cuda") + 1e-6 * torch.rand(T.shape, generator=gen, device="cuda", dtype=torch.float64))
    m.field("S").interior_view().fill_(35.0)
    for f in m.velocities:
        iv = f.interior_view(); iv.copy_(1e-2 * (torch.rand(iv.shape, generator=gen, device="cuda", dtype=torch.float64) * 2 - 1))
    ocn.set(m)
    return m


def step_ms(m, dt):
    """one timing window: `steps` steps between two device events (the window ends in a synchronise)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        ocn.time_step(m, dt)
    ocn.flush_tendencies(m)
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


# ---- 1. the kernel
m = model("function")
umax = float(torch.stack([f.interior_view().abs().max() for f in m.velocities]).max())
dt = 0.1 * min(g.dx, float(np.diff(z_faces).min())) / umax
bf = m._boundary_functions[0]
ms = device_ms(lambda: bf.compute(0.0))
print(f"evaluation kernel, drag_u on the {Nx}x{Nx} bottom plane ({len(bf.program.instructions)} instructions, {bf.program.n_registers} registers): "
      f"{ms * 1e3:.1f} us per launch by device events, {48 * Nx * Nx / ms / 1e6:.1f} GB/s of its 48 B/point", flush=True)
del m, bf
torch.cuda.empty_cache()


# ---- 2. steps: every model is built first, then the models take turns, window by window, so that whatever else the device and the host
# are doing is spread over all of them; the median of the windows is the figure, min .. max the spread
def build(bottom, fuse="1", evaluate=True):
    os.environ["OCN_FUSE_GENERAL"] = fuse  # (read when a model is built)
    mm = model(bottom)
    if not evaluate:  # the launch sequence of (d) without its evaluation launches: the values stay what the construction left
        mm._boundary_functions = mm._boundary_functions[:0]
    return mm


cases = [("a. no bottom conditions on u, v", build(None)),
         ("b. array-valued bottom conditions on u, v", build("array")),
         ("c. array-valued bottom conditions on u, v, OCN_FUSE_GENERAL=0", build("array", fuse="0")),
         ("d. drag_u / drag_v", build("function")),
         ("e. drag_u / drag_v, evaluation launches skipped (values frozen)", build("function", evaluate=False))]
for _, mm in cases:  # warm-up: every kernel of every model, the first deferred launch included
    for _ in range(3):
        ocn.time_step(mm, dt)
    ocn.flush_tendencies(mm)
torch.cuda.synchronize()
windows = {label: [] for label, _ in cases}
for _ in range(rounds):
    for label, mm in cases:
        windows[label].append(step_ms(mm, dt))
for label, mm in cases:
    w = sorted(windows[label])
    ok = bool(all(torch.isfinite(f.data).all() for f in mm.prognostic_fields()))
    print(f"config-4-like RK3 step, {label}: median {w[len(w) // 2]:.2f} ms/step by device events over {rounds} windows of {steps} steps "
          f"(min {w[0]:.2f}, max {w[-1]:.2f}; finite={ok}, fused stage boundaries={mm.fuse_stage_boundaries}, "
          f"boundary functions={len(mm._boundary_functions)})", flush=True)
