"""HARL_CAT_WIDE_256 on the host side (harl_amd/configs.py, the constructors): without the switch a Categorical head of more than
64 actions on a trunk that holds a 256-wide layer is refused with the text it always had; with it the specs that
tests/test_gpu_cat_wide_256.py runs are accepted and what stays refused answers with its existing text."""
import pytest
import torch

from harl_amd.configs import CAT_WIDE_REFUSALS, unsupported_reason
from tests.gpu_checks import Box, Discrete, default_args
from tests.test_multidiscrete_cpu import stub_kernels  # noqa: F401  (fixture: the C-ABI dispatcher replaced by a recorder)

ACCEPTED = [([256, 256], 65), ([128, 256], 192), ([256, 128], 300), ([256, 256, 256], 512)]  # (hidden_sizes, n)


def _reason(algo, n, hs=(256, 256), **model):
    args = dict(model=dict(dict(hidden_sizes=list(hs), activation_func="relu"), **model), algo={})
    return unsupported_reason(algo, args, obs_dim=19, act_space_name="Discrete", act_dim=n)


def _build(n, hs=(256, 256), cls=None, **over):
    from harl_amd.nets import StochasticPolicy
    return (cls or StochasticPolicy)(default_args(hs, **over), Box((19,)), Discrete(n), torch.device("cpu"))


def test_refused_as_before_without_the_switch(monkeypatch, stub_kernels):  # noqa: F811
    monkeypatch.delenv("HARL_CAT_WIDE_256", raising=False)
    assert _reason("happo", 100) == CAT_WIDE_REFUSALS["panel"]
    with pytest.raises(NotImplementedError) as e:
        _build(100)
    assert str(e.value) == CAT_WIDE_REFUSALS["panel"]


@pytest.mark.parametrize("hs,n", ACCEPTED, ids=[f"{a[0]}_{a[1]}" for a in ACCEPTED])
def test_accepted_with_the_switch(monkeypatch, stub_kernels, hs, n):  # noqa: F811
    monkeypatch.setenv("HARL_CAT_WIDE_256", "1")
    monkeypatch.setenv("HARL_MIXED_256", "1")
    assert [_reason(algo, n, hs) for algo in ("happo", "haa2c", "mappo")] == [None] * 3
    net = _build(n, hs)
    assert net.cat_wide and net.panel and sum(r[4] for r in net._table_rows[-len(net._md_sp):]) == n


def test_refusals_with_the_switch(monkeypatch, stub_kernels):  # noqa: F811
    from harl_amd.hatrpo import HATRPO
    monkeypatch.setenv("HARL_CAT_WIDE_256", "1")
    monkeypatch.setenv("HARL_TRPO_CAT_WIDE", "1")
    assert _reason("hatrpo", 100) == CAT_WIDE_REFUSALS["panel"] and _reason("happo", 513) == CAT_WIDE_REFUSALS["n"]
    assert _reason("happo", 100, activation_func="tanh") == "activation 'tanh': feed-forward policies of width 64 / 128 only"
    assert _reason("happo", 100, use_recurrent_policy=True) == "hidden width 256 is feed-forward only"
    trpo = dict(cls=HATRPO, kl_threshold=0.01, ls_step=10, accept_ratio=0.5, backtrack_coeff=0.8)
    for kw, want in ((trpo, CAT_WIDE_REFUSALS["panel"]), (dict(n=513), CAT_WIDE_REFUSALS["n"]), (dict(activation_func="tanh"), None),
                     (dict(use_recurrent_policy=True), None)):  # (None: a text of the trunk's own, as on every 256-wide trunk)
        with pytest.raises(NotImplementedError) as e:
            _build(**dict(dict(n=100), **kw))
        assert want is None or str(e.value) == want
