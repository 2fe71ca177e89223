#!/usr/bin/env python3
"""Time of the on-device diagnostics (oceananigans.jl_amd/operations.py) on an N x N x Nz (Periodic, Periodic, Bounded) grid:
compute() of  Average(u, (1,2)),  Average(w*u, (1,2)),  Integral(0.5*(u**2+v**2+w**2)),  Average(b, 1)  and  ddx(v) - ddy(u),
each next to two yardsticks taken in the same run, neither of which is the code under test:
  (a) the way to the same quantity without the feature: Field.interior() of every operand (a device-to-host copy of the whole parent
      array) and the arithmetic in NumPy, as examples/two_dimensional_turbulence.py and examples/horizontal_convection.py do it;
  (b) ocn_hasnan over the same distinct operand fields: the library's plain streaming read of those bytes.

  tools/bench_diagnostics.py [N] [Nz] [reps]
Per case: median of `reps` timings after a warm-up (device work: host clock around a window that ends in a synchronise), the effective
bandwidth = bytes of the distinct operand parents / time, and the ratios (a) / device and device / (b)."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import oceananigans_jl_amd as ocn

N = int(sys.argv[1]) if len(sys.argv) > 1 else 256
Nz = int(sys.argv[2]) if len(sys.argv) > 2 else 128
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20

grid = ocn.RectilinearGrid(ocn.GPU(), size=(N, N, Nz), x=(0, 1), y=(0, 1), z=(-0.5, 0), topology=("Periodic", "Periodic", "Bounded"))
gen = torch.Generator(device="cuda")
gen.manual_seed(1)
u, v, w, b = ocn.XFaceField(grid), ocn.YFaceField(grid), ocn.ZFaceField(grid), ocn.CenterField(grid)
for f in (u, v, w, b):
    f.data.copy_(torch.rand(f.data.shape, generator=gen, device="cuda", dtype=torch.float64) * 2 - 1)
ocn.fill_halo_regions((u, v, w, b), fill_boundary_normal_velocities=False)


def ix(a):  # ℑx to faces / centres of a periodic direction, on interiors [i, j, k]
    return 0.5 * (np.roll(a, 1, axis=0) + a)


def host_wu():
    ui, wi = u.interior(), w.interior()                  # w: Nz + 1 faces
    uk = np.concatenate([ui[:, :, :1], ui, ui[:, :, -1:]], axis=2)  # no-flux halos in z
    uf = 0.5 * (uk[:, :, :-1] + uk[:, :, 1:])
    return (wi * 0.5 * (uf + np.roll(uf, -1, axis=0))).mean(axis=(0, 1))


def host_ke():
    ui, vi, wi = u.interior(), v.interior(), w.interior()
    v2 = vi * vi
    v2 = ix(0.5 * (v2 + np.roll(v2, -1, axis=1)))
    w2 = wi * wi
    w2 = ix(0.5 * (w2[:, :, :-1] + w2[:, :, 1:]))
    return float((0.5 * (ui * ui + v2 + w2)).sum() * (grid.dx * grid.dy * grid.dz))


def host_zeta():
    ui, vi = u.interior(), v.interior()
    return (vi - np.roll(vi, 1, axis=0)) / grid.dx - (ui - np.roll(ui, 1, axis=1)) / grid.dy


cases = [
    ("Average(u, (1,2))", ocn.Average(u, dims=(1, 2)), (u,), lambda: u.interior().mean(axis=(0, 1))),
    ("Average(w*u, (1,2))", ocn.Average(w * u, dims=(1, 2)), (w, u), host_wu),
    ("Integral(0.5*(u**2+v**2+w**2))", ocn.Integral(0.5 * (u ** 2 + v ** 2 + w ** 2)), (u, v, w), host_ke),
    ("Average(b, 1)", ocn.Average(b, dims=1), (b,), lambda: b.interior().mean(axis=0)),
    ("ddx(v) - ddy(u)", ocn.ddx(v) - ocn.ddy(u), (v, u), host_zeta),
]


def timed(fn, n):
    out = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return statistics.median(out), min(out), max(out)


flag = torch.zeros(1, dtype=torch.int32, device="cuda")
print(f"grid {N} x {N} x {Nz}, halo 3, {reps} repetitions (median [min, max])")
for name, operand, fields, host in cases:
    cf = ocn.ComputedField(operand)
    nbytes = sum(f.data.numel() * 8 for f in fields)

    def scan():
        for f in fields:
            ocn._lib.call("ocn_hasnan", f.ptr, f.data.numel(), flag.data_ptr(), ocn.architectures.stream_ptr())

    def device():
        inner = 10  # (one call is tens of microseconds at the small size: time ten, report one)
        for _ in range(inner):
            cf.compute()
    for _ in range(3):
        device()
        scan()
    td = tuple(x / 10 for x in timed(device, reps))
    ts = timed(scan, reps)
    host()
    th = timed(host, max(3, reps // 5))
    got, want = cf.interior(), np.asarray(host())
    err = float(np.max(np.abs(got.reshape(want.shape) - want)) / max(1e-300, float(np.max(np.abs(want)))))
    print(f"{name:32s} device {td[0] * 1e3:8.3f} ms [{td[1] * 1e3:.3f}, {td[2] * 1e3:.3f}]  {nbytes / td[0] / 1e9:7.1f} GB/s | "
          f"(a) interior()+NumPy {th[0] * 1e3:9.1f} ms = {th[0] / td[0]:8.1f} x device | "
          f"(b) hasnan {ts[0] * 1e3:7.3f} ms, device = {td[0] / ts[0]:5.2f} x hasnan | host vs device rel. diff {err:.1e}", flush=True)
