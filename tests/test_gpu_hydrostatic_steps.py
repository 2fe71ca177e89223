"""HydrostaticFreeSurfaceModel launches what the commit named in tests/golden/hydrostatic_steps.json launched, and computes its bits.

The Python host that sequences the closure's launches (hydrostatic.py, hydrostatic_closures.py, models.py) decides nothing that the device
could round differently, so the comparison is exact: per case the ordered names of the library calls of the construction plus `set`, of
each of three time steps and of `flush_tendencies`, and the SHA-256 of the parent bytes of u, v, w, T, S, η, every Gⁿ and every diffusivity
field after the third step, against the record tools/record_hydrostatic_steps.py wrote from a checkout of that commit.  A mismatch is a
launch that moved, went missing or received another argument.  All cases: 13 x 6 x 4, stretched z, SeawaterBuoyancy, an FPlane, a top flux
on T, strict math, an initial state whose upper half is unstable (both values of κᶜ, κᵘ occur); WENO() tracers unless noted.

  none-defaults                      closure = None, Centered() tracers: the fused step, its unfused tracer branch
  scalar-fused                       explicit ScalarDiffusivity in ocn_model_terms: the κ numbers of the fused tracer launches
  scalar-unfused-explicit_fs         the same with the reference's launch sequence: the κ number of the built-in tracer entry point
  implicit_scalar, -flux_form        vertically implicit ScalarDiffusivity: κ = 0 to the built-in entry points, the explicit part of the
                                     term, the implicit step; with VectorInvariant() and with flux-form WENO() momentum
  cavd-implicit_fs, cavd_explicit    ConvectiveAdjustmentVerticalDiffusivity in both discretizations (the field-valued implicit step or none)
  ri_based, ri_based-filter-...      RiBasedVerticalDiffusivity: one launch, or with a FivePointHorizontalFilter three and the Ri halo fill
  biharmonic, biharmonic-split_rk3   HorizontalScalarBiharmonicDiffusivity alone, QAB2 and SplitRungeKutta3 (the halo of 2 is the container's)
  biharmonic+cavd, +cavd_explicit,   the pairs: the other closure's term into zeroed scratch, the biharmonic launch subtracts the sum; u
  ri_based+biharmonic                and v first, then tracer by tracer

The cases run in ONE fresh child process, in the recorder's order."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_hydrostatic_steps as R  # noqa: E402

with open(os.path.join(ROOT, "tests", "golden", "hydrostatic_steps.json")) as f:
    GOLDEN = json.load(f)


@pytest.fixture(scope="module")
def computed(ocn, tmp_path_factory):
    out = tmp_path_factory.mktemp("hydrostatic_steps") / "steps.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "record_hydrostatic_steps.py"), str(out)], capture_output=True, text=True,
                       timeout=280)
    assert r.returncode == 0, f"child exited {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    with open(out) as f:
        return json.load(f)["cases"]


def test_record_covers_the_cases():
    assert list(R.CASES) == list(GOLDEN["cases"]) and GOLDEN["commit"]


@pytest.mark.parametrize("case", list(R.CASES))
def test_launches_and_bits_are_those_of_the_recorded_commit(computed, case):
    got, want = computed[case], GOLDEN["cases"][case]
    assert got["fused"] == want["fused"]
    assert got["construction"].split() == want["construction"].split()
    for step, (a, b) in enumerate(zip(got["steps"], want["steps"])):
        assert a.split() == b.split(), f"time step {step + 1}"
    assert len(got["steps"]) == len(want["steps"]) == R.STEPS and got["flush"].split() == want["flush"].split()
    assert list(got["sha256"]) == list(want["sha256"])
    different = [name for name in want["sha256"] if got["sha256"][name] != want["sha256"][name]]
    assert not different, f"other bits than the recorded commit's in {different}"
