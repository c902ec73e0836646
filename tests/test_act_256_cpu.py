"""HARL_ACT_256 on the host side: without the switch the refusals keep their texts; with it the shapes of tests/test_gpu_act_256.py
are accepted, what stays refused answers with its own text, and such a network launches csrc/rect.hip's ``_act_`` entry points."""
import pytest
import torch

from harl_amd.configs import ACT_256_REFUSALS as R, CAT_WIDE_REFUSALS, MIXED_256_REFUSALS, unsupported_reason
from tests.gpu_checks import Box, MultiDiscrete, default_args
from tests.test_multidiscrete_cpu import stub_kernels  # noqa: F401  (fixture)

CPU, GRU = torch.device("cpu"), dict(use_recurrent_policy=True)


@pytest.fixture(autouse=True)
def switches(monkeypatch):
    monkeypatch.setenv("HARL_MIXED_256", "1")
    monkeypatch.setenv("HARL_ACT_256", "1")


@pytest.mark.parametrize("on,algo,hs,model,space,act_dim,obs_dim,want", [
    (False, "happo", [256, 256], {}, "Box", 5, 18, "activation 'tanh': feed-forward policies of width 64 / 128 only"),
    (False, "happo", [256, 128], {}, "Box", 5, 18, MIXED_256_REFUSALS["act"]),
    (True, "happo", [256, 256], {}, "Box", 5, 18, None),
    (True, "haa2c", [256, 128], {}, "Discrete", 14, 40, None),
    (True, "mappo", [128, 256], {}, "Box", 5, 512, None),
    (True, "hatrpo", [256, 256], GRU, "Box", 5, 18, R["hatrpo"]),  # (the order of precedence: HATRPO, GRU, MultiDiscrete, inputs)
    (True, "happo", [256, 256], GRU, "MultiDiscrete", 5, 18, R["recurrent"]),
    (True, "happo", [256, 256], {}, "MultiDiscrete", 5, 600, R["md"]),
    (True, "happo", [256, 256], {}, "Box", 5, 600, R["obs"]),
    (True, "happo", [256, 256], {}, "Discrete", 100, 18, CAT_WIDE_REFUSALS["panel"]),
    (True, "hatrpo", [256, 128], {}, "Box", 5, 18, MIXED_256_REFUSALS["hatrpo"]),  # (a mixed trunk's own refusals first)
])
def test_unsupported_reason(monkeypatch, on, algo, hs, model, space, act_dim, obs_dim, want):
    if not on:
        monkeypatch.delenv("HARL_ACT_256")
    for act in ("leaky_relu", "tanh", "sigmoid", "selu") if want is None else ("tanh",):
        args = dict(model=dict(hidden_sizes=hs, activation_func=act, **model), algo=dict(share_param=True))
        assert unsupported_reason(algo, args, obs_dim, space, act_dim) == want


def test_constructors_and_launches(stub_kernels, monkeypatch):  # noqa: F811
    from harl_amd.hatrpo import HATRPO
    from harl_amd.nets import StochasticPolicy, VNet
    M, tanh = 70, default_args([256, 256], activation_func="tanh")
    for key, make in (("hatrpo", lambda: HATRPO(tanh, Box((18,)), Box((5,)), CPU)), ("recurrent", lambda: VNet(dict(tanh, **GRU), Box((18,)), CPU)),
                      ("md", lambda: StochasticPolicy(tanh, Box((18,)), MultiDiscrete([3, 4]), CPU)), ("obs", lambda: VNet(tanh, Box((600,)), CPU))):
        pytest.raises(NotImplementedError, make).match(R[key].split(" (")[0])
    net = VNet(default_args([256, 128], activation_func="tanh"), Box((40,)), CPU)
    stub_kernels.clear()
    net.forward_trunk(torch.zeros(M, 40), None, M)
    assert [(a[2], a[4], a[6], a[7]) for a in stub_kernels["harl_mlp_rect_act_fwd"]] == [(64, 40, 256, 2), (256, 256, 128, 2)]  # KP, D, HO, act
    assert not {"harl_act_ln_fwd", "harl_mlp_linear", "harl_mlp_linear_wide", "harl_mlp_rect_fwd", "harl_mlp_panel_fwd"} & set(stub_kernels)
    assert net._first_launch(True, False).kind == "panel" and net._backward_route(M).family == "panel"
    assert not hasattr(net, "zraw") and len(net.amean) == 2 and net.ones_mask.numel() == 3 * 64 * 2 and net.feat()[1] is net.ones_mask
    stub_kernels.clear()
    net.backward_trunk(torch.zeros(M, 40), None, M, head_dw_done=True)
    assert [(a[4], a[5], a[6]) for a in stub_kernels["harl_act_bwd"]] == [(M, 128, 2)]  # the top layer only
    assert [(a[5], a[6], a[7]) for a in stub_kernels["harl_mlp_rect_act_bwd"]] == [(128, 256, 2)]
    assert len(stub_kernels["harl_mlp_dw_partials"]) == 2 and not {"harl_mlp_bwd_dx", "harl_mlp_rect_bwd"} & set(stub_kernels)
    wide = VNet(tanh, Box((18,)), CPU)  # a 256-wide last layer: four mask words per lane under the head kernels
    wide.forward_trunk(torch.zeros(M, 18), None, M)
    assert wide.ones_mask.numel() == 3 * 64 * 4
    monkeypatch.delenv("HARL_ACT_256")
    with pytest.raises(NotImplementedError, match="activation functions other than relu: feed-forward MLPs of width 64 / 128"):
        VNet(tanh, Box((18,)), CPU)
