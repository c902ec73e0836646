"""HARL_TRPO_MIXED_256 on the host side (harl_amd/configs.py, harl_mlp_rect_tangent's argument checks): next to HARL_MIXED_256=1
HATRPO takes the four shapes tests/test_gpu_trpo_mixed_256.py runs, what stays refused keeps its text; alone it changes nothing."""
import pytest

from harl_amd.configs import CAT_WIDE_REFUSALS, MIXED_256_REFUSALS, unsupported_reason
from tests.test_mixed_256_cpu import ACCEPTED, _args

BOTH = ("HARL_MIXED_256", "HARL_TRPO_MIXED_256")
CASES = [(BOTH, hs, {}, space, act_dim, obs_dim, None) for hs, space, act_dim, obs_dim in ACCEPTED] + [
    (BOTH, [256, 128], dict(use_recurrent_policy=True), "Box", 5, 18, MIXED_256_REFUSALS["recurrent"]),
    (BOTH, [256, 128], dict(activation_func="tanh"), "Box", 5, 18, MIXED_256_REFUSALS["act"]),
    (BOTH, [256, 128], {}, "Discrete", 100, 18, CAT_WIDE_REFUSALS["hatrpo"]),
    (BOTH[1:], [256, 128], {}, "Box", 5, 18, "hidden widths [256, 128]: 256-wide layers cannot be mixed with narrower ones")]


@pytest.mark.parametrize("switches,hs,model,space,act_dim,obs_dim,want", CASES, ids=[f"{len(c[0])}-{c[1]}-{c[2]}-{c[4]}" for c in CASES])
def test_unsupported_reason_for_hatrpo(monkeypatch, switches, hs, model, space, act_dim, obs_dim, want):
    for v in BOTH:
        monkeypatch.setenv(v, "1" if v in switches else "0")
    assert unsupported_reason("hatrpo", _args(hs, **model), obs_dim=obs_dim, act_space_name=space, act_dim=act_dim) == want


def test_entry_point_refuses_other_shapes():
    from harl_amd import _lib
    lib = _lib.load()
    for xin_dot, KP, HO, Wp, D in [(64, 256, 96, 64, 256), (64, 256, 128, None, 256), (None, 80, 64, None, 77)]:  # (64: a non-NULL pointer)
        assert lib.harl_mlp_rect_tangent(xin_dot, None, 33, KP, HO, Wp, None, D, None, None, None, None, None, None) == -2
        assert b"harl_mlp_rect_tangent" in lib.harl_last_error()
