"""Dead work left out of the RK3 box step (csrc/driver.hip, momentum_tendencies_pc32, the source passes of the pressure solver): the third
launch of a step does not store its G^n, no halo fill runs in front of the solve (wrapped loads instead), and a flush with a deferred
correction is one launch (OCN_DRIVER_FUSED_FLUSH=1; the first two are on by default).  Each part has an environment switch read when the
driver / the solver handle is created; with every switch at 0 the driver runs the sequence it ran before.  The new paths -- the default
configuration and the one with the one-launch flush as well -- must reproduce that sequence BIT FOR BIT -- u, v, w, p and G^n with their halos,
strict and fast math -- and, in strict math, the Python host's ocn.time_step (what test_c_driver_equals_host_orchestration asserts).

Sequence: 4 steps, flush, 3 steps, flush; the state is compared after each flush.  The odd count exercises the copy home, consecutive steps
without a flush the G^n that was never written.

Grids (Periodic, Periodic, Periodic):
  16 x 14 x 4    one tile; the z window wraps through the whole depth
  33 x 29 x 9    3 x 3 tiles with clipped last tiles; ring columns that wrap in x and y
  37 x 21 x 11   the shape of the Stokes-drift tests
  128 x 64 x 64  the solver's row-FFT source pass (Nx >= 128), the one the 512^3 box takes
  40 x 22 x 6 and 40 x 22 x 36 with OCN_TEND_MIN_BLOCKS=64, in a child process (the switch is read once per process).  The z chunk is only
                 halved while it is longer than 16 planes, so at Nz = 6 it stays the whole depth whatever the value; 40 x 22 x 36 is the
                 smallest such grid whose chunks (9 planes) start and end inside the depth, so that chunk windows wrap in z."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OLD = {"OCN_DRIVER_SKIP_G_STORE": "0", "OCN_DRIVER_WRAPPED_LOADS": "0", "OCN_DRIVER_FUSED_FLUSH": "0", "OCN_POISSON_SOURCE_WRAP": "0"}
GRIDS = [(16, 14, 4), (33, 29, 9), (37, 21, 11), (128, 64, 64)]
CHUNKED = [(40, 22, 6), (40, 22, 36)]
NEW = {"OCN_DRIVER_FUSED_FLUSH": "1"}
DT = 0.01


class _Env:
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _model(ocn, size, math, env, arch=None):
    P = "Periodic"
    with _Env(env):  # (the solver handle reads its switch here)
        g = ocn.RectilinearGrid(arch or ocn.GPU(), size=size, x=(0, 2 * np.pi), y=(0, 3.0), z=(0, 2.0), topology=(P, P, P), halo=(3, 3, 3))
        m = ocn.NonhydrostaticModel(g, advection=ocn.WENO(), math_mode=ocn.MATH_STRICT if math == "strict" else ocn.MATH_FAST)
    rng = np.random.default_rng(5)
    ocn.set(m, **{n: rng.uniform(-1, 1, size) for n in "uvw"})
    return m


def _state(ocn, m):
    ocn.sync_device()
    return [f.data.clone() for f in m.velocities + (m.pNHS,)] + [G.data.clone() for G in m.timestepper._Gn]


def _driver_states(ocn, size, math, env):
    m = _model(ocn, size, math, env)
    with _Env(env):  # (... and the driver its three)
        drv = ocn.RK3Driver(m)
    out = []
    for steps in (4, 3):
        for _ in range(steps):
            drv.time_step(DT)
        drv.flush()
        out.append(_state(ocn, m))
    del drv
    return out


def _host_states(ocn, size, math):
    m = _model(ocn, size, math, {})
    out = []
    for steps in (4, 3):
        for _ in range(steps):
            ocn.time_step(m, DT)
        ocn.flush_tendencies(m)
        out.append(_state(ocn, m))
    return out


NAMES = ("u", "v", "w", "p", "Gu", "Gv", "Gw")


def _compare(ocn, size, math):
    import torch
    new, old = _driver_states(ocn, size, math, NEW), _driver_states(ocn, size, math, OLD)
    for tag, states in (("all three parts", new), ("default", _driver_states(ocn, size, math, {}))):
        for q, (a, b) in enumerate(zip(states, old)):
            for x, y, name in zip(a, b, NAMES):
                assert torch.isfinite(x).all(), f"{size} {math} {tag} flush {q}: {name} not finite"
                diff = (x - y).abs().max().item()
                print(f"{size} {math} {tag} flush {q} {name}: max |new - old| over the parent array = {diff:.3e}")
                assert torch.equal(x, y), f"{size} {math} {tag} flush {q}: {name} (with halos) differs from the switched-off driver by {diff:.3e}"
    if math == "strict":  # the Python host: bit for bit, G^n over the interior (its halos are the host's own)
        H = 3
        for q, (a, b) in enumerate(zip(new, _host_states(ocn, size, math))):
            for x, y, name in zip(a[:4], b[:4], NAMES):
                assert torch.equal(x, y), f"{size} flush {q}: {name} differs from the Python host"
            for x, y, name in zip(a[4:], b[4:], NAMES[4:]):
                assert torch.equal(x[H:-H, H:-H, H:-H], y[H:-H, H:-H, H:-H]), f"{size} flush {q}: {name} differs from the Python host"


def _selected(ocn, m):
    sel = C.c_int32(-1)
    ocn._lib.call("ocn_momentum_tendencies_addr32", m.grid.cref, C.byref(sel))
    return sel.value


@pytest.mark.gpu
@pytest.mark.parametrize("math", ["strict", "fast"])
@pytest.mark.parametrize("size", GRIDS)
def test_driver_without_dead_work_equals_driver_with_it(ocn, size, math):
    assert _selected(ocn, _model(ocn, size, math, {})) == 1  # (the paths under test are the 32-bit kernel's)
    _compare(ocn, size, math)


@pytest.mark.gpu
@pytest.mark.parametrize("math", ["strict", "fast"])
def test_chunked_z_windows_wrap(ocn, math):
    """OCN_TEND_MIN_BLOCKS=64: see the module docstring."""
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); import oceananigans_jl_amd as ocn\n"
            f"from tests.test_gpu_rk3_driver_dead_work import _compare, CHUNKED\n"
            f"for size in CHUNKED: _compare(ocn, size, {math!r})\n")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, OCN_TEND_MIN_BLOCKS="64"), capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    print(r.stdout[-4000:])
    assert r.returncode == 0, f"{r.stdout[-3000:]}\n{r.stderr[-4000:]}"


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(16, 8, 4), (33, 29, 9), (128, 64, 64)])
def test_source_pass_wraps_instead_of_reading_halos(ocn, size):
    """ocn_solve_for_pressure with the velocity halos full of finite garbage (wrapped source pass) against the same call with filled halos
    and OCN_POISSON_SOURCE_WRAP=0: bitwise equal pressure.  (128, 64, 64) takes the row-FFT source pass, the others the plain one."""
    import torch
    from oceananigans_jl_amd.architectures import stream_ptr
    out = []
    for env, want in ((OLD, 0), ({}, 1)):
        m = _model(ocn, size, "strict", env)
        wraps = C.c_int32(-1)
        ocn._lib.call("ocn_poisson_source_wraps", m.pressure_solver._h, C.byref(wraps))
        assert wraps.value == want
        if want:
            gen = torch.Generator(device="cpu").manual_seed(7)
            for f in m.velocities:
                keep = f.interior_view().clone()
                f.data.copy_(torch.empty(f.data.shape, dtype=torch.float64).uniform_(-1e3, 1e3, generator=gen))
                f.interior_view().copy_(keep)
        else:
            ocn.fill_halo_regions(m.velocities)
        ocn._lib.call("ocn_solve_for_pressure", m.pressure_solver._h, m.pNHS.ptr, m.u.ptr, m.v.ptr, m.w.ptr, 0.37, stream_ptr())
        ocn.sync_device()
        out.append(m.pNHS.interior_view().clone())
    assert torch.isfinite(out[0]).all() and out[0].abs().max() > 0
    assert torch.equal(out[0], out[1]), f"{size}: max diff {(out[0] - out[1]).abs().max().item():.3e}"


@pytest.mark.gpu
def test_slab_driver_keeps_its_fills(ocn):
    """A slab-x rank (a world of one over the RCCL transport) keeps its halo fills, its G^n stores and the separate passes of its flush: the
    switches change nothing there.  Same sequence, every switch at its default against every switch at 0, in child processes."""
    import torch
    code = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import torch
import oceananigans_jl_amd as ocn
from tests.test_gpu_rk3_driver_dead_work import _model, _state, DT
import os, socket
import torch.distributed as dist
torch.cuda.set_device(0)
with socket.socket() as s:
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
dist.init_process_group("gloo", rank=0, world_size=1)
arch = ocn.distributed.make_distributed(0, 1, 0, force_communication=True)
m = _model(ocn, (16, 128, 64), "fast", {}, arch=arch)  # (the smallest slab its distributed solver runs without transposes)
drv = ocn.RK3Driver(m)
for _ in range(3):
    drv.time_step(DT)
drv.flush()
torch.save([t.cpu() for t in _state(ocn, m)], sys.argv[2])
del drv
arch.fabric.close()
'''
    import tempfile
    got = []
    with tempfile.TemporaryDirectory() as tmp:
        for tag, env in (("new", NEW), ("old", OLD)):
            out = os.path.join(tmp, tag + ".pt")
            r = subprocess.run([sys.executable, "-c", code, ROOT, out], env=dict(os.environ, OCN_DIST_POISSON_XTRI="1", **env), capture_output=True, text=True, timeout=300,
                               cwd=ROOT)
            assert r.returncode == 0, f"{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
            got.append(torch.load(out))
    for a, b, name in zip(got[0], got[1], NAMES):
        assert torch.isfinite(a).all() and torch.equal(a, b), name
