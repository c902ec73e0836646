"""HARL_MIXED_256 on the host side (harl_amd/configs.py, csrc/rect.hip's argument checks): without the switch a trunk that mixes
256-wide layers with narrower ones is refused with the text it always had; with it the four shapes tests/test_gpu_mixed_256.py
runs are accepted and what stays refused answers with its own text."""
import pytest

from harl_amd.configs import CAT_WIDE_REFUSALS, MIXED_256_REFUSALS, unsupported_reason

# (hidden_sizes, action space, act_dim, obs_dim): the whole-path specs of tests/test_gpu_mixed_256.py
ACCEPTED = [([256, 128], "Box", 5, 18), ([128, 256], "Discrete", 14, 40), ([64, 256, 64], "Box", 20, 77),
            ([256, 64, 128], "Discrete", 33, 31)]


def _args(hs, **model):
    return dict(model=dict(dict(hidden_sizes=hs, activation_func="relu"), **model), algo={})


def test_refused_as_before_without_the_switch(monkeypatch):
    monkeypatch.delenv("HARL_MIXED_256", raising=False)
    assert unsupported_reason("happo", _args([256, 128])) == "hidden widths [256, 128]: 256-wide layers cannot be mixed with narrower ones"


@pytest.mark.parametrize("hs,space,act_dim,obs_dim", ACCEPTED, ids=[str(a[0]) for a in ACCEPTED])
def test_accepted_with_the_switch(monkeypatch, hs, space, act_dim, obs_dim):
    monkeypatch.setenv("HARL_MIXED_256", "1")
    for algo in ("happo", "haa2c", "mappo"):
        assert unsupported_reason(algo, _args(hs), obs_dim=obs_dim, act_space_name=space, act_dim=act_dim) is None


@pytest.mark.parametrize("algo,model,space,act_dim,want", [
    ("hatrpo", {}, "Box", 5, MIXED_256_REFUSALS["hatrpo"]),
    ("happo", dict(use_recurrent_policy=True), "Box", 5, MIXED_256_REFUSALS["recurrent"]),
    ("happo", dict(activation_func="tanh"), "Box", 5, MIXED_256_REFUSALS["act"]),
    ("happo", {}, "Discrete", 100, CAT_WIDE_REFUSALS["panel"]),
], ids=["hatrpo", "gru", "tanh", "discrete100"])
def test_refusals_with_the_switch(monkeypatch, algo, model, space, act_dim, want):
    monkeypatch.setenv("HARL_MIXED_256", "1")
    assert unsupported_reason(algo, _args([256, 128], **model), obs_dim=18, act_space_name=space, act_dim=act_dim) == want


def test_entry_points_refuse_other_shapes():
    from harl_amd import _lib
    lib = _lib.load()
    assert lib.harl_mlp_rect_fwd(None, 33, 256, None, 256, None, 96, None, None, None, None) == -2
    assert b"harl_mlp_rect_fwd" in lib.harl_last_error()
    assert lib.harl_mlp_rect_fwd(None, 33, 80, None, 77, None, 64, None, None, None, None) == -2
    assert lib.harl_mlp_rect_bwd(None, None, None, None, 33, 256, 32, None, None, None) == -2
    assert b"harl_mlp_rect_bwd" in lib.harl_last_error()
