"""Gaussian heads of 33..64 dimensions (HARL_GAUSS_WIDE=1), host side (no GPU): the switch, the refusals and their texts, and
the launch sequence of update() / get_actions() with the C-ABI calls recorded instead of executed (the arithmetic is covered by
the `-m gpu` tests of tests/test_gpu_gauss_wide.py)."""
import numpy as np
import pytest
import torch

from harl_amd.configs import GAUSS_WIDE_REFUSALS, unsupported_reason
from tests.gpu_checks import Box, default_args
from tests.test_cat_wide_cpu import _names, ordered_calls  # noqa: F401  (fixture: the recorder as ONE list in launch order)
from tests.test_multidiscrete_cpu import stub_kernels  # noqa: F401  (fixture: the C-ABI dispatcher replaced by a recorder)

CPU = torch.device("cpu")


@pytest.fixture
def wide(monkeypatch):
    monkeypatch.setenv("HARL_GAUSS_WIDE", "1")


def _policy(n, hidden, obs_dim=19, **over):
    from harl_amd.nets import StochasticPolicy
    return StochasticPolicy(default_args(hidden, **over), Box((obs_dim,)), Box((n,)), CPU)


def _cfg(hidden=(128, 128), algo=None, **model):
    return dict(model=dict(dict(hidden_sizes=list(hidden), activation_func="relu"), **model), algo=dict(algo or {}))


@pytest.mark.parametrize("value", [None, "0"])
def test_switch_off_refuses_as_before(stub_kernels, monkeypatch, value):  # noqa: F811
    if value is None:
        monkeypatch.delenv("HARL_GAUSS_WIDE", raising=False)
    else:
        monkeypatch.setenv("HARL_GAUSS_WIDE", value)
    for algo in ("happo", "haa2c", "mappo", "hatrpo"):
        assert unsupported_reason(algo, _cfg(), act_space_name="Box", act_dim=40) == (
            "action heads wider than 32 (Categorical: 64) are not implemented (act_dim = 40)")
    assert unsupported_reason("happo", _cfg(), act_space_name="Box", act_dim=100) is not None
    assert unsupported_reason("happo", _cfg(), act_space_name="Box", act_dim=32) is None
    with pytest.raises(NotImplementedError) as e:
        _policy(40, [128, 128])
    assert str(e.value) == "action heads wider than 32 (Categorical: 64) are not instantiated"
    assert not _policy(32, [128, 128]).gauss_wide


def test_unsupported_reason_with_the_switch_on(wide):
    for algo in ("happo", "haa2c", "mappo"):
        for n in (33, 40, 64):
            assert unsupported_reason(algo, _cfg([64, 64]), act_space_name="Box", act_dim=n) is None
            assert unsupported_reason(algo, _cfg([128, 128]), act_space_name="Box", act_dim=n) is None
            assert unsupported_reason(algo, _cfg([64], use_recurrent_policy=True), act_space_name="Box", act_dim=n) is None
    assert unsupported_reason("mappo", _cfg(algo=dict(share_param=True)), act_space_name="Box", act_dim=36) is None
    R = GAUSS_WIDE_REFUSALS
    assert unsupported_reason("happo", _cfg(), act_space_name="Box", act_dim=65) == R["n"]
    assert unsupported_reason("happo", _cfg([256, 256]), act_space_name="Box", act_dim=40) == R["panel"]
    assert unsupported_reason("happo", _cfg(activation_func="tanh"), act_space_name="Box", act_dim=40) == R["act"]
    assert unsupported_reason("hatrpo", _cfg(), act_space_name="Box", act_dim=40) == R["hatrpo"]
    assert unsupported_reason("happo", _cfg(), act_space_name="Box", act_dim=40, world_size=2) == R["dp"]
    assert unsupported_reason("happo", _cfg([128], use_recurrent_policy=True), act_space_name="Box", act_dim=40) == R["gru"]
    assert unsupported_reason("happo", _cfg([64], use_recurrent_policy=True, recurrent_n=2), act_space_name="Box", act_dim=40) == R["gru"]
    assert len(set(R.values())) == len(R)
    # narrower Gaussian heads and every Categorical head: what they were
    assert unsupported_reason("hatrpo", _cfg(), act_space_name="Box", act_dim=32) is None
    assert unsupported_reason("happo", _cfg(), act_space_name="Box", act_dim=20, world_size=2) is None
    assert unsupported_reason("happo", _cfg(), act_space_name="Discrete", act_dim=40, world_size=2) is None


def test_constructors_raise_the_same_texts(stub_kernels, wide):  # noqa: F811
    from harl_amd.happo import HAPPO
    from harl_amd.hatrpo import HATRPO
    R = GAUSS_WIDE_REFUSALS
    for n, hidden, over, key in ((65, [128, 128], {}, "n"), (40, [256, 256], {}, "panel"),
                                 (40, [128, 128], dict(activation_func="tanh"), "act"),
                                 (40, [128], dict(use_recurrent_policy=True), "gru"),
                                 (40, [64], dict(use_recurrent_policy=True, recurrent_n=2), "gru")):
        with pytest.raises(NotImplementedError) as e:
            _policy(n, hidden, **over)
        assert str(e.value) == R[key], (n, hidden, over)
        cfg = _cfg(hidden, **{k: v for k, v in over.items()})
        assert unsupported_reason("happo", cfg, act_space_name="Box", act_dim=n) == R[key]
    trpo = default_args([64, 64], kl_threshold=0.01, ls_step=10, accept_ratio=0.5, backtrack_coeff=0.8)
    with pytest.raises(NotImplementedError) as e:
        HATRPO(trpo, Box((19,)), Box((40,)), device=CPU)
    assert str(e.value) == R["hatrpo"]
    HATRPO(trpo, Box((19,)), Box((32,)), device=CPU)
    # data parallelism: the runner hands the communicator / column shard over after construction, and asks
    actor = HAPPO(default_args([64, 64]), Box((19,)), Box((40,)), device=CPU)
    actor._refuse_gauss_wide_dp()
    actor.shard = (8, 0, 4)
    with pytest.raises(NotImplementedError) as e:
        actor._refuse_gauss_wide_dp()
    assert str(e.value) == R["dp"]
    narrow = HAPPO(default_args([64, 64]), Box((19,)), Box((20,)), device=CPU)
    narrow.shard = (8, 0, 4)
    narrow._refuse_gauss_wide_dp()
    # accepted: the plain head's container, one table entry, the ATL(64) gradient image
    for n, hidden, over in ((33, [64, 64], {}), (64, [128, 64], {}), (40, [64], dict(use_recurrent_policy=True))):
        net = _policy(n, hidden, **over)
        assert net.gauss_wide and net.wide_head and not net.grouped and not net.discrete and net.act_w == n
        assert net._table_rows[-1][4] == n and net._table_rows[-1][10] == 64
        assert list(net.state_dict())[-3:] == ["act.action_out.log_std", "act.action_out.fc_mean.weight", "act.action_out.fc_mean.bias"]


def _sample(M, n, obs_dim, rng):
    obs = rng.standard_normal((M, obs_dim)).astype(np.float32)
    act = rng.standard_normal((M, n)).astype(np.float32)
    return obs, act, np.ones((M, 1), np.float32), np.full((M, n), -1.0, np.float32)


@pytest.mark.parametrize("recurrent", [False, True])
def test_update_and_get_actions_launch_sequence(ordered_calls, wide, recurrent):  # noqa: F811
    from harl_amd import _lib
    from harl_amd.happo import HAPPO
    n, hidden, obs_dim = 40, ([64] if recurrent else [128, 128]), 19
    L, m = (3, 8) if recurrent else (1, 24)
    M = L * m
    actor = HAPPO(default_args(hidden, use_recurrent_policy=recurrent), Box((obs_dim,)), Box((n,)), device=CPU)
    net = actor.actor
    obs, act, ones, old = _sample(M, n, obs_dim, np.random.default_rng(0))
    rnn = np.zeros((m, 1, hidden[-1]), np.float32)
    masks = np.ones((M, 1), np.float32)
    ordered_calls.clear()
    actor.update((obs, rnn, act, masks, ones, old, ones, None, ones))
    names = _names(ordered_calls)
    assert "harl_actor_head_loss" not in names and "harl_adam_fold" not in names
    assert not [c for c in names if c.startswith("harl_update_")]         # the fused routes keep their width limits
    k = names.index("harl_actor_head_loss_ls")
    # loss -> the head's weight gradient from the ATL(64) image -> ... -> combine -> log_std sums -> the optimiser's new form
    assert names[k + 1] == "harl_mlp_dw_partials"
    tail = names[names.index("harl_reduce_partials_multi"):]
    assert tail == ["harl_reduce_partials_multi", "harl_ls_reduce", "harl_adam_fold_ls"]
    loss = ordered_calls[k][1]
    assert len(loss) == 34 and loss[10] == 0 and loss[11] == n              # discrete, act_dim
    assert loss[30] is None and loss[31] == 0                                # dw_part = NULL, n_wg
    assert loss[32] == net.part_ls.data_ptr() and loss[29] == net.part_scalars.data_ptr() and loss[28] == net.dhead.data_ptr()
    Mp = L * ((m + 31) // 32 * 32) if recurrent else M
    assert net.dhead.numel() == (Mp + 31) // 32 * 32 * 64 and net.part_ls.numel() == net.n_head_blocks * 64
    head_dw = ordered_calls[k + 1][1]
    assert head_dw[0] == net.dhead.data_ptr() and head_dw[1] == 0 and head_dw[3] == 64 and head_dw[10] == hidden[-1]
    red = [a for nm, a in ordered_calls if nm == "harl_ls_reduce"][0]
    nblk = _lib.load().harl_head_blocks(Mp)
    assert red[0] == net.part_ls.data_ptr() and red[1] == nblk and red[2] == net.ls_sum.data_ptr() and red[3] == 0
    adam = [a for nm, a in ordered_calls if nm == "harl_adam_fold_ls"][0]
    assert len(adam) == 30 and adam[27] == net.ls_sum.data_ptr() and adam[11] == nblk
    assert adam[15] == net.offsets["act.action_out.log_std"][0] and adam[16] == n
    # rollout step and evaluate_actions: the plain log-prob entry point, act_w = act_dim
    ordered_calls.clear()
    acts, logp, _ = actor.get_actions(obs[:m], rnn, masks[:m], None, deterministic=True)
    assert tuple(acts.shape) == (m, n) and tuple(logp.shape) == (m, n)
    seq = [c for c in _names(ordered_calls) if c in ("harl_actor_head_logp", "harl_dist_rows", "harl_update_logp")]
    assert seq == ["harl_actor_head_logp", "harl_dist_rows"]
    acts, _ = actor.act(obs[:m], rnn, masks[:m], None, deterministic=False)
    assert tuple(acts.shape) == (m, n)
    out, ent, dist = actor.evaluate_actions(obs, rnn, act, masks, None, ones)
    assert tuple(out.shape) == (M, n) and ent.dim() == 0 and dist is not None


def test_shared_parameter_step_accumulates_the_log_std_sums(ordered_calls, wide, monkeypatch):  # noqa: F811
    """MAPPO.share_param_train: per agent segment one loss launch and one harl_ls_reduce -- the first in its set form, the
    others accumulating -- then ONE harl_adam_fold_ls; under HARL_GRAPH=1 the steps run eagerly and are counted."""
    from harl_amd.buffers import OnPolicyActorBuffer
    from harl_amd.mappo import MAPPO
    monkeypatch.setenv("HARL_GRAPH", "1")
    n, obs_dim, T, N, A = 36, 19, 4, 3, 3
    args = default_args([64, 64], ppo_epoch=2, share_param=True, episode_length=T, n_rollout_threads=N)
    actor = MAPPO(args, Box((obs_dim,)), Box((n,)), device=CPU)
    bufs = [OnPolicyActorBuffer(args, Box((obs_dim,)), Box((n,)), device=CPU) for _ in range(A)]
    ordered_calls.clear()
    actor.share_param_train(bufs, torch.zeros(T, N, 1), A, "EP")
    names = [c for c in _names(ordered_calls) if c in ("harl_actor_head_loss_ls", "harl_ls_reduce", "harl_adam_fold_ls", "harl_adam_fold",
                                                     "harl_adam_fold_dev", "harl_actor_head_loss")]
    assert names == (["harl_actor_head_loss_ls", "harl_ls_reduce"] * A + ["harl_adam_fold_ls"]) * 2
    assert [a[3] for nm, a in ordered_calls if nm == "harl_ls_reduce"] == [0, 1, 1] * 2
    adam = [a for nm, a in ordered_calls if nm == "harl_adam_fold_ls"]
    assert all(a[10] is None and a[27] == actor.actor.ls_sum.data_ptr() for a in adam)   # part_scalars NULL: sums accumulated
    st = actor.graph_stats()
    assert st["eager_steps"] == 2 and st["captures"] == 0 and st["replays"] == 0


# One HAPPO.update of a Box(32) actor, M = 77: (entry point, tag) in launch order as recorded on the commit before the switch
BOX32_SEQUENCES = {
    ((128, 128), 19): [("harl_mlp_x0n_wide", "x0n_wide"), ("harl_mlp_fwd_fused2x", "fwd_fused2"), ("harl_actor_head_loss", "actor_head_loss"),
                       ("harl_mlp_dw_partials", "dw_hidden"), ("harl_mlp_bwd_dx", "bwd_dx_dw1"),
                       ("harl_reduce_partials_multi", "reduce_partials"), ("harl_adam_fold", "adam_fold")],
    ((64, 128), 40): [("harl_mlp_x0n_wide", "x0n_wide"), ("harl_mlp_fwd_wide", "fwd_wide"), ("harl_mlp_fwd_hidden", "fwd_hidden"),
                      ("harl_actor_head_loss", "actor_head_loss"), ("harl_mlp_dw_partials", "dw_hidden"), ("harl_mlp_bwd_dx", "bwd_dx_dw1"),
                      ("harl_reduce_partials_multi", "reduce_partials"), ("harl_adam_fold", "adam_fold")],
}


@pytest.mark.parametrize("switch", [None, "1"])
@pytest.mark.parametrize("key", list(BOX32_SEQUENCES), ids=["h128_obs19", "h64_128_obs40"])
def test_box32_keeps_its_launch_sequence(stub_kernels, monkeypatch, key, switch):  # noqa: F811
    from harl_amd import _lib
    from harl_amd.happo import HAPPO
    if switch is None:
        monkeypatch.delenv("HARL_GAUSS_WIDE", raising=False)
    else:
        monkeypatch.setenv("HARL_GAUSS_WIDE", switch)
    log, inner = [], _lib.call

    def rec(name, *args, tag=None):
        log.append((name, tag, args))
        return inner(name, *args, tag=tag)

    for mod in ("nets", "happo"):
        monkeypatch.setattr(__import__(f"harl_amd.{mod}", fromlist=["x"]), "call", rec)
    hidden, obs_dim = key
    actor = HAPPO(default_args(list(hidden)), Box((obs_dim,)), Box((32,)), device=CPU)
    assert not actor.actor.gauss_wide and not hasattr(actor.actor, "part_ls")
    M = 77
    obs, act, ones, old = _sample(M, 32, obs_dim, np.random.default_rng(0))
    log.clear()
    actor.update((obs, np.zeros((M, 1, 1), np.float32), act, None, ones, old, ones, None, ones))
    assert [(nm, tag) for nm, tag, _ in log] == BOX32_SEQUENCES[key]
    loss = [a for nm, _, a in log if nm == "harl_actor_head_loss"][0]
    assert len(loss) == 33 and loss[30] is not None and loss[31] == actor.actor.n_wg   # the fused head gradient, as before
    adam = [a for nm, _, a in log if nm == "harl_adam_fold"][0]
    assert len(adam) == 29 and adam[16] == 32
