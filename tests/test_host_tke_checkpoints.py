"""The checkpoints of the two TKE-based closures keep their format.  tests/golden/tke_checkpoint_{catke,tke_dissipation}.npz hold the
closure_state of an 8 x 6 x 5 model after two steps as the commit before TKEBasedFields wrote it (recorded once on the GPU: CATKEFields
through its two hand-kept dictionaries, TKEDissipationFields through _state).  Today's closure objects restore those arrays bit for bit, and
what they then write is the fixture again: key names, shapes, dtypes and values.  No GPU: the objects are given host tensors of the
fixture's shapes in place of the fields a model would allocate."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = {"catke": {"kappa_u", "kappa_c", "kappa_e", "Le", "Jb", "u_prev", "v_prev", "top_e", "previous_compute_time", "e", "Gm_e"},
        "tke_dissipation": {"kappa_u", "kappa_c", "kappa_e", "kappa_eps", "Le", "Leps", "u_prev", "v_prev", "top_e", "top_eps", "e", "eps",
                            "Gm_e", "Gm_eps"}}


def _closure_on_host(kind, z):
    """the closure object of `kind` and a stand-in for the model, every array zero, shaped as the device keeps it: the transposed fixture"""
    import torch
    import oceananigans_jl_amd as ocn
    from oceananigans_jl_amd.hydrostatic_closures import CATKEFields, TKEDissipationFields
    zeros = lambda name: torch.zeros(z[name].T.shape, dtype=torch.float64)
    field = lambda name: SimpleNamespace(data=zeros(name))
    if kind == "catke":
        c, tracers, keys = CATKEFields(ocn.CATKEVerticalDiffusivity(), ("T", "S")), ("T", "S", "e"), {"e": "e"}
        c.fields = {name: field(name) for name in ("kappa_u", "kappa_c", "kappa_e", "Le")}
        c.fields["Jb"] = zeros("Jb")  # (a plane: a tensor, not a field)
        c.previous_compute_time = -1.0
    else:
        c = TKEDissipationFields(ocn.TKEDissipationVerticalDiffusivity(), ("T", "S"), "dissipation")  # (the user's name for ϵ is no key)
        tracers, keys = ("T", "S", "e", "dissipation"), {"e": "e", "dissipation": "eps"}
        c.fields = {name: field(name) for name in ("kappa_u", "kappa_c", "kappa_e", "kappa_eps", "Le", "Leps")}
    c.u_prev, c.v_prev = field("u_prev"), field("v_prev")
    c.tops = {name: SimpleNamespace(_device_values=zeros("top_" + key)) for name, key in keys.items()}
    prognostic = {name: field(key) for name, key in keys.items()}
    G = lambda prefix: [None] * 3 + [field(prefix + keys[name]) if name in keys else None for name in tracers]
    nh = SimpleNamespace(tracer_names=tracers, field=lambda name: prognostic[name], timestepper=SimpleNamespace(_Gn=G("Gm_"), _Gm=G("Gm_")))
    return c, nh


@pytest.mark.parametrize("kind", ["catke", "tke_dissipation"])
def test_checkpoint_of_the_parent_commit_restores_bit_for_bit_and_is_written_again(kind):
    z = np.load(os.path.join(GOLDEN, f"tke_checkpoint_{kind}.npz"))
    assert set(z.files) == KEYS[kind]
    assert any(np.any(z[name] != 0) for name in z.files if name.startswith("kappa")) and np.any(z["Gm_e"] != 0)  # (no fixture of zeros)
    c, nh = _closure_on_host(kind, z)
    c.restore_state(nh, lambda name: z[name] if name in z.files else None)
    state = c._state(nh)
    assert set(state) | ({"previous_compute_time"} if kind == "catke" else set()) == KEYS[kind]
    for name, t in state.items():  # the restored state is the fixture, exactly
        assert np.array_equal(t.numpy().T.view(np.uint64), z[name].view(np.uint64)), name
    if kind == "catke":
        assert c.previous_compute_time == float(z["previous_compute_time"]) == 600.0
    written = c.checkpoint_state(nh)
    assert set(written) == KEYS[kind]
    for name in z.files:  # ... and is written as the parent commit wrote it
        a = np.asarray(written[name])
        assert a.shape == z[name].shape and a.dtype == z[name].dtype == np.float64, name
        assert np.array_equal(a.reshape(-1).view(np.uint64), z[name].reshape(-1).view(np.uint64)), name


@pytest.mark.parametrize("kind,closure_name", [("catke", "CATKEVerticalDiffusivity"), ("tke_dissipation", "TKEDissipationVerticalDiffusivity")])
def test_a_checkpoint_without_the_closure_state_names_the_closure(kind, closure_name):
    z = np.load(os.path.join(GOLDEN, f"tke_checkpoint_{kind}.npz"))
    c, nh = _closure_on_host(kind, z)
    with pytest.raises(KeyError, match=f"Field kappa_u of {closure_name} does not exist in checkpoint"):
        c.restore_state(nh, lambda name: None)
