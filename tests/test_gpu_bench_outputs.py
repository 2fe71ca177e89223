"""bench.py on one GPU: a plain run times exactly --steps steps and carries no extra figures, --dump-outputs writes the same arrays for the
same arguments, --full adds the checks and figures the plain run leaves out."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args, timeout=400):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "OCN_FORCE_DISTRIBUTED"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--size", "128", *args], env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, (p.stdout[-2000:], p.stderr[-4000:])
    return json.loads(lines[0])


def test_plain_run_times_its_steps_and_dumps_the_same_outputs_every_time(tmp_path):
    runs = []
    for name in ("a", "b"):
        d = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / name))
        assert d["steps"] == 3 and d["warmup"] == 1 and d["full"] is False and d["dumped_outputs"] == str(tmp_path / name)
        assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(128 ** 3 * 1e3 / d["ms_per_step"], rel=1e-9)
        assert d["unit"] == "cell-updates/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
        assert d["strict_ms_per_step"] is None and d["roofline"] is None and d["cpu_baseline"] is None
        runs.append({n: np.load(tmp_path / name / f"{n}.npy") for n in "uvw"})
    total = sum(a.nbytes for a in runs[0].values())
    assert total <= 64e6
    for n in "uvw":
        a, b = runs[0][n], runs[1][n]
        assert a.dtype == np.float64 and a.shape == (1 << 20,) and np.isfinite(a).all() and np.abs(a).max() > 0
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-12)


def test_full_run_adds_the_checks_and_figures():
    d = _bench("--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline")
    assert d["full"] is True and d["steps"] == 2 and d["ms_per_step"] > 0
    assert d["config"]["finite"] is True and len(d["config"]["state_checksum"]["sum_of_squares"]) == 3
    assert d["strict_ms_per_step"] > 0 and d["roofline"]["kernel_ms"] > 0 and d["step_roofline"] is not None
