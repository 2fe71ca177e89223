"""The correction-on-load tendency kernel with 32-bit buffer offsets (csrc/tendencies.hip, momentum_tendencies_pc32) against the 64-bit
kernel it replaces (OCN_TEND_ADDR32=0): the same seeded model, several RK3 steps, each run in a fresh child process (the switch is read
once per process).  Strict math must agree bit for bit, fast math bit for bit or within 1e-12 relative.  The host-side selection falls
back to the 64-bit kernel for fields of 2^31 bytes or more; that predicate is exercised without allocating such a field."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import torch
import oceananigans_jl_amd as ocn
case, math, out = sys.argv[2], sys.argv[3], sys.argv[4]
N = {"box64": (64, 64, 64), "box128": (128, 96, 64), "slab": (64, 64, 32)}[case]
ocn.set_math_mode(ocn.MATH_STRICT if math == "strict" else ocn.MATH_FAST)
P = "Periodic"
ext = dict(x=(0, 2 * np.pi), y=(0, 2 * np.pi), z=(0, 2 * np.pi), topology=(P, P, P), halo=(3, 3, 3))
rng = np.random.default_rng(2718)
init = {n: rng.uniform(-1, 1, N) for n in "uvw"}
dt, steps = 0.01, 3

def run(arch, sl):
    g = ocn.RectilinearGrid(arch, size=N, **ext)
    m = ocn.NonhydrostaticModel(g, advection=ocn.WENO())
    assert m.correct_on_load or m.dist_correct_on_load
    ocn.set(m, **{k: v[sl] for k, v in init.items()})
    for _ in range(steps):
        ocn.time_step(m, dt)
    ocn.sync_device()
    return [f.interior() for f in m.velocities] + [m.pNHS.interior()]

torch.cuda.set_device(0)
if case != "slab":
    fields = run(ocn.GPU(), slice(None))
else:
    import threading
    from test_gpu_distributed import ThreadWorld, ThreadFabric
    R = 2
    world, outs, errs = ThreadWorld(R), [None] * R, []
    def target(r):
        try:
            torch.cuda.set_device(0)
            arch = ocn.Distributed(ocn.GPU(), partition=ocn.Partition(R), fabric=ThreadFabric(world, r))
            outs[r] = run(arch, slice(r * N[0] // R, (r + 1) * N[0] // R))
        except Exception:
            import traceback
            errs.append(traceback.format_exc())
            world.barrier.abort()
    ts = [threading.Thread(target=target, args=(r,)) for r in range(R)]
    for t in ts: t.start()
    for t in ts: t.join(300)
    assert not errs, "\n".join(errs)
    fields = [np.concatenate([o[q] for o in outs], axis=0) for q in range(4)]
np.savez(out, *fields)
'''


def _run(tmp_path, case, math, addr32):
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    out = tmp_path / f"{case}_{math}_{addr32}.npz"
    env = dict(os.environ, OCN_TEND_ADDR32=str(addr32))
    r = subprocess.run([sys.executable, str(script), ROOT, case, math, str(out)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"child ({case}, {math}, OCN_TEND_ADDR32={addr32}) exited {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    d = np.load(out)
    return [d[f"arr_{q}"] for q in range(4)]


@pytest.mark.gpu
@pytest.mark.parametrize("math", ["strict", "fast"])
@pytest.mark.parametrize("case", ["box64", "box128", "slab"])
def test_addr32_kernel_matches_64bit_kernel(tmp_path, case, math):
    new = _run(tmp_path, case, math, 1)
    old = _run(tmp_path, case, math, 0)
    for a, b, name in zip(new, old, ("u", "v", "w", "p")):
        assert np.isfinite(a).all(), f"{name}: non-finite values"
        if math == "strict":
            assert np.array_equal(a, b), f"{case} {name}: not bitwise equal in strict math (max diff {np.abs(a - b).max()})"
        else:
            err = np.abs(a - b).max()
            assert err <= 1e-12 * max(1.0, np.abs(b).max()), f"{case} {name}: {err}"


def _selected(ocn, Nx, Ny, Nz, H=3):
    g = ocn._lib.CGrid(Nx, Ny, Nz, H, H, H, 0, 0, 0, 0, 1.0, 1.0, 1.0, float(Nx), float(Ny), float(Nz), None, None)
    sel = C.c_int32(-1)
    ocn._lib.call("ocn_momentum_tendencies_addr32", C.byref(g), C.byref(sel))
    return sel.value


def test_addr32_selection_falls_back_for_large_fields():
    """Runs in a child process so that the per-process switch is read fresh; the predicate is host code (no GPU needed)."""
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); import oceananigans_jl_amd as ocn; "
            f"from tests.test_gpu_tendency_addr32 import _selected; "
            f"print(_selected(ocn, 512, 512, 512), _selected(ocn, 1018, 1018, 249), _selected(ocn, 1018, 1018, 250), "
            f"_selected(ocn, 2048, 1024, 512), _selected(ocn, 64, 64, 64, H=2))")
    for addr32, want in (("1", "1 1 0 0 0"), ("0", "0 0 0 0 0")):
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, OCN_TEND_ADDR32=addr32), capture_output=True, text=True,
                           timeout=120, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        assert r.stdout.split() == want.split(), (addr32, r.stdout)
