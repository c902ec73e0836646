"""HARL_TRPO_ACT_256 on the host side: it lifts HATRPO's refusal only next to HARL_ACT_256=1 (mixed trunks: and both mixed switches),
every other refusal keeps its text, and a Fisher-vector product on such a network is one harl_mlp_rect_act_tangent per layer."""
import pytest
import torch

from harl_amd.configs import ACT_256_REFUSALS as R, CAT_WIDE_REFUSALS, MIXED_256_REFUSALS, unsupported_reason
from tests.gpu_checks import Box, Discrete, MultiDiscrete, default_args
from tests.test_hatrpo_cpu import TRPO, _fvp_calls
from tests.test_multidiscrete_cpu import stub_kernels  # noqa: F401  (fixture)

A, T, MIX, TMIX = ALL = ("HARL_ACT_256", "HARL_TRPO_ACT_256", "HARL_MIXED_256", "HARL_TRPO_MIXED_256")
GRU = dict(use_recurrent_policy=True)
CASES = [  # (switches that are on, hidden sizes, model, action space, its name and width, obs_dim, unsupported_reason, the constructor's text)
    ((A,), [256, 256], {}, Box((5,)), "Box", 5, 18, R["hatrpo"], R["hatrpo"]),
    ((T,), [256, 256], {}, Box((5,)), "Box", 5, 18, "activation 'tanh': feed-forward policies of width 64 / 128 only", "activation functions other than relu"),
    ((A, T), [256, 256], {}, Box((5,)), "Box", 5, 18, None, None),
    ((A, T, MIX), [256, 128], {}, Discrete(14), "Discrete", 14, 40, MIXED_256_REFUSALS["hatrpo"], MIXED_256_REFUSALS["hatrpo"]),
    (ALL, [256, 128], {}, Discrete(14), "Discrete", 14, 40, None, None),
    ((A, T), [256, 256], GRU, Box((5,)), "Box", 5, 18, R["recurrent"], R["recurrent"]),
    ((A, T), [256, 256], {}, MultiDiscrete([3, 4]), "MultiDiscrete", 4, 18, R["md"], "only continuous and discrete action space"),  # (the reference's assertion)
    ((A, T), [256, 256], {}, Box((5,)), "Box", 5, 600, R["obs"], R["obs"]),
    ((A, T), [256, 256], {}, Discrete(100), "Discrete", 100, 18, CAT_WIDE_REFUSALS["hatrpo"], CAT_WIDE_REFUSALS["hatrpo"]),
]


@pytest.mark.parametrize("on,hs,model,space,name,act_dim,obs_dim,want,raised", CASES, ids=[f"{'+'.join(v[5:] for v in c[0])}-{c[1]}-{c[4]}{c[5]}-{c[6]}{'-gru' * bool(c[2])}" for c in CASES])
def test_refusal_follows_the_switches(monkeypatch, stub_kernels, on, hs, model, space, name, act_dim, obs_dim, want, raised):  # noqa: F811
    from harl_amd.hatrpo import HATRPO
    for v in ALL:
        monkeypatch.setenv(v, "1" if v in on else "0")
    assert unsupported_reason("hatrpo", dict(model=dict(hidden_sizes=hs, activation_func="tanh", **model), algo={}), obs_dim, name, act_dim) == want
    build = lambda: HATRPO(default_args(hs, activation_func="tanh", **TRPO, **model), Box((obs_dim,)), space, torch.device("cpu"))  # noqa: E731
    if want is None:
        assert build().actor.act_256
    else:
        assert str(pytest.raises((NotImplementedError, AssertionError), build).value).startswith(raised)


def test_fvp_is_one_launch_per_layer(monkeypatch, stub_kernels):  # noqa: F811
    for v in ALL:
        monkeypatch.setenv(v, "1")
    t, n = _fvp_calls(stub_kernels, [256, 128], 40, Box((5,)), activation_func="tanh")
    # (xin_dot is NULL, KP, HO, D, act) of each launch: the first layer from the x0n image, then 256 -> 128
    assert [(a[0] is None, a[3], a[4], a[7], a[9]) for a in stub_kernels["harl_mlp_rect_act_tangent"]] == [(True, 64, 256, 40, 2), (False, 256, 128, 256, 2)]
    assert not {"harl_mlp_linear", "harl_mlp_linear_wide", "harl_act_ln_tangent", "harl_mlp_rect_tangent", "harl_mlp_panel_tangent"} & set(n)
    assert "zd" not in t._tangent_ws and n["harl_actor_head_fvp"] == 1 and n["harl_mlp_rect_act_bwd"] == 1
