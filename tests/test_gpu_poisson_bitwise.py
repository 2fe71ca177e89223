"""solve_for_pressure! reproduces, bit for bit, the pressure of the commit named in tests/golden/poisson_digests.json.

The transform kernels of csrc/colfft.hip and rowfft.hip request their tables and their data in an order chosen for memory latency
(OCN_FFT_EARLY_LOADS); reordering requests cannot change a rounding, so the comparison is exact: the SHA-256 of the interior pressure
bytes and a few sampled values, per shape, against the record tools/record_poisson_digests.py wrote with a library built from that
commit.  A mismatch is an indexing bug.  Shapes, all (Periodic, Periodic, Periodic) unless noted:

  128 x 64 x 64, 128 x 64 x 512     the row / column pipeline (rowfft_source_r2c, colfft MODE 0 / 2 / 1, rowfft_c2r); the y pass has 65
                                    columns per batch, so the inactive lanes of the last block run
  16 x 12 x 64 / 128 / 256 / 512    rocFFT x / y around the fused z pass at every column length, including the 16-column workgroups of
                                    length 256; 108 columns leave the last block partly inactive, and column 0 carries the zero mode
  128 x 64 x 64 (P, P, Bounded)     the cosine twin of the fused z pass (MODE 5)
  64^3 (Bounded, Bounded, Bounded)  the one-pass cosine columns (MODE 3 / 4) around the cosine rows

The cases run in ONE fresh child process, in the recorder's order (rocFFT's choice of real plans can depend on the plans alive in the
process: test_gpu_poisson_pipelines.py)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_poisson_digests as R  # noqa: E402

with open(os.path.join(ROOT, "tests", "golden", "poisson_digests.json")) as f:
    GOLDEN = json.load(f)


@pytest.fixture(scope="module")
def computed(ocn, tmp_path_factory):
    out = tmp_path_factory.mktemp("poisson_bitwise") / "digests.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "record_poisson_digests.py"), str(out)], capture_output=True, text=True,
                       timeout=280)
    assert r.returncode == 0, f"child exited {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    with open(out) as f:
        return json.load(f)["cases"]


def test_record_covers_the_cases():
    assert [c[0] for c in R.CASES] == list(GOLDEN["cases"]) and GOLDEN["commit"] and GOLDEN["dt"] == R.DT


@pytest.mark.parametrize("case", R.CASES, ids=[c[0] for c in R.CASES])
def test_pressure_bits_are_those_of_the_recorded_commit(computed, case):
    got, want = computed[case[0]], GOLDEN["cases"][case[0]]
    print(f"{case[0]}: info {got['info']} (recorded {want['info']})  sha256 {got['sha256'][:16]} (recorded {want['sha256'][:16]})")
    assert got["info"] == want["info"]  # the same pipeline, or the digests compare different solvers
    assert got["samples"] == want["samples"]
    assert got["sha256"] == want["sha256"]
