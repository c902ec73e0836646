"""Where an optimiser step of an actor waits for its sequential-update factor (HAPPO._await_factor), host side without a GPU.
The wait is a stream wait and no C-ABI call, so the recorded launch traces (tests/test_launch_trace_cpu.py) cannot see it: here
it leaves a marker in the order of the recorded calls.  The loss launch is the factor's only consumer and the runner produces
the factor next to this agent's first forward, so on every kind of step -- the one-launch step, the last hidden layer inside the
loss launch, the layer kernels -- the wait sits behind every forward and image launch and directly in front of the loss launch."""
import numpy as np
import pytest
import torch

from tests.gpu_checks import Box, default_args
from tests.test_multidiscrete_cpu import stub_kernels  # noqa: F401  (fixture)

MODS = ("nets", "buffers", "happo", "hatrpo", "mappo", "v_critic", "valuenorm", "runner")
MARK = "await_factor"
# kind of step -> (hidden sizes of a 19-input Box(3) actor that takes it, entry point of its loss launch)
STEPS = {"fused": ([128, 128], "harl_update_fwd_actor"), "last": ([128, 128, 128], "harl_update_last_actor"),
         "layers": ([128, 64], "harl_actor_head_loss")}


@pytest.mark.parametrize("kind", sorted(STEPS))
def test_the_factor_is_awaited_directly_in_front_of_the_loss_launch(stub_kernels, monkeypatch, kind):  # noqa: F811
    from harl_amd import _lib
    from harl_amd.happo import HAPPO
    monkeypatch.delenv("HARL_FUSED_UPDATE", raising=False)
    order, inner, wait = [], _lib.call, HAPPO._await_factor

    def ordered(name, *args, tag=None):
        order.append(name)
        return inner(name, *args, tag=tag)

    def marked(self):
        order.append(MARK)
        return wait(self)
    monkeypatch.setattr(_lib, "call", ordered)
    for mod in MODS:
        m = __import__(f"harl_amd.{mod}", fromlist=["x"])
        if hasattr(m, "call"):
            monkeypatch.setattr(m, "call", ordered)
    monkeypatch.setattr(HAPPO, "_await_factor", marked)
    hidden, loss = STEPS[kind]
    torch.manual_seed(11)
    actor = HAPPO(default_args(hidden), Box((19,)), Box((3,)), device=torch.device("cpu"))
    M, rng = 24, np.random.default_rng(0)
    ones = lambda *shape: np.ones(shape, np.float32)  # noqa: E731
    obs = rng.standard_normal((M, 19)).astype(np.float32)
    del order[:]
    # (obs, rnn_states, actions, masks, active_masks, old_logp, advantages, available_actions, factor)
    actor.update((obs, None, ones(M, 3), ones(M, 1), ones(M, 1), np.full((M, 3), -2.0, np.float32), ones(M, 1), None, ones(M, 1)))
    assert order.count(MARK) == 1 and order.count(loss) == 1, order
    at = order.index(MARK)
    assert order[at + 1] == loss, order
    forwards = [i for i, n in enumerate(order) if n.startswith("harl_mlp_fwd_") or n == "harl_mlp_x0n_wide"]
    assert forwards and max(forwards) < at, order  # every forward / image launch of the step: in front of the wait
    assert not any(n.startswith("harl_update_") or n.endswith("_head_loss") for n in order[:at]), order
