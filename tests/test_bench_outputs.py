"""bench.dump_outputs on host tensors: small interiors are written whole, larger ones as a fixed seeded sample that does not depend on
the run or on how the x direction is split over ranks."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


class _Capture:
    """a one-rank stand-in for the transport: records what each rank contributes to the sum"""

    def __init__(self):
        self.parts = []

    def allreduce_sum(self, t):
        self.parts.append(t.clone())
        return t


def _import_bench():
    """bench.py sets an IPC switch of the HIP runtime on import; a host-only test leaves the environment of later GPU tests as it was"""
    had = "HSA_ENABLE_IPC_MODE_LEGACY" in os.environ
    import bench
    if not had:
        os.environ.pop("HSA_ENABLE_IPC_MODE_LEGACY", None)
    return bench


def _interior(full, halo=3):
    import torch
    parent = torch.zeros(tuple(s + 2 * halo for s in full.shape), dtype=full.dtype)
    view = parent[tuple(slice(halo, halo + s) for s in full.shape)]
    view.copy_(full)
    return view


def test_small_interiors_are_written_whole(tmp_path):
    import torch
    bench = _import_bench()
    full = torch.rand((6, 5, 40), dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    view = _interior(full)
    bench.dump_outputs(str(tmp_path), [("u", view), ("eta", view[0])], 0, 1, None)
    np.testing.assert_array_equal(np.load(tmp_path / "u.npy"), full.numpy())
    np.testing.assert_array_equal(np.load(tmp_path / "eta.npy"), full[0].numpy())


def test_large_interiors_are_sampled_at_the_same_points_for_any_split(tmp_path, monkeypatch):
    import torch
    bench = _import_bench()
    monkeypatch.setattr(bench, "DUMP_MAX_POINTS", 100)
    full = torch.rand((6, 5, 40), dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    bench.dump_outputs(str(tmp_path / "one"), [("T", _interior(full))], 0, 1, None)
    one = np.load(tmp_path / "one" / "T.npy")
    assert one.shape == (100,) and one.dtype == np.float64
    assert np.isin(one, full.numpy().ravel()).all()
    bench.dump_outputs(str(tmp_path / "again"), [("T", _interior(full))], 0, 1, None)
    np.testing.assert_array_equal(np.load(tmp_path / "again" / "T.npy"), one)
    cap = _Capture()
    for r in range(2):  # two x-slabs of 20 points: each rank fills the sampled points of its slab, zeros elsewhere
        bench.dump_outputs(str(tmp_path / f"r{r}"), [("T", _interior(full[:, :, 20 * r:20 * (r + 1)].contiguous()))], r, 2, cap)
    np.testing.assert_array_equal((cap.parts[0] + cap.parts[1]).numpy(), one)
