"""Categorical heads of 65..512 actions, host side (no GPU): parameter container (the reference's ONE [n, H] head matrix, seen
by the kernels as row groups of 128), layer table, refusals, and the launch sequence of update() / get_actions() with the C-ABI
calls recorded instead of executed (the arithmetic is covered by the `-m gpu` tests of tests/test_gpu_cat_wide.py)."""
import numpy as np
import pytest
import torch

from harl_amd.configs import unsupported_reason
from harl_amd.synthetic import Shapes, actor_param_shapes
from tests.gpu_checks import Box, Discrete, default_args
from tests.test_multidiscrete_cpu import stub_kernels  # noqa: F401  (fixture: the C-ABI dispatcher replaced by a recorder)

CPU = torch.device("cpu")


def _policy(n, hidden, obs_dim=19, **over):
    from harl_amd.nets import StochasticPolicy
    args = default_args(hidden, **over)
    return StochasticPolicy(args, Box((obs_dim,)), Discrete(n), CPU), args


def test_parameter_container_matches_reference_layout(stub_kernels):  # noqa: F811
    n, hidden = 200, [128, 128]
    net, args = _policy(n, hidden)
    sh = Shapes(T=4, N=2, A=1, obs_dim=19, share_obs_dim=5, act_dim=n, discrete=True, hidden_sizes=hidden)
    want = actor_param_shapes(sh, True)
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == want   # names, shapes and ORDER (act.py:24-43)
    assert want[-2:] == [("act.action_out.linear.weight", (200, 128)), ("act.action_out.linear.bias", (200,))]
    assert sum(p.numel() for p in net.parameters()) == net.n_params
    # flat_param is parameters() order: the groups are row ranges of one contiguous matrix
    assert torch.equal(net.flat_reference(), net.flat_param)
    assert net.cat_wide and not net.md and net.act_w == 1 and net.act_dim == 200


def test_group_entries_of_the_table(stub_kernels):  # noqa: F811
    net, _ = _policy(200, [128, 128])
    rows = net._table_rows
    assert len(rows) == 2 + 2 and net._md_sp == [128, 128]
    assert [r[4] for r in rows[-2:]] == [128, 72]            # rows of the two groups
    assert [r[10] for r in rows[-2:]] == [128, 128]          # partial layout of harl_mlp_dw_partials(HO = sp)
    assert [r[5] for r in rows[-2:]] == [128, 128]
    w_off, b_off = net.offsets["act.action_out.linear.weight"][0], net.offsets["act.action_out.linear.bias"][0]
    assert [r[0] for r in rows[-2:]] == [w_off, w_off + 128 * 128] and [r[1] for r in rows[-2:]] == [b_off, b_off + 128]
    # both groups fold with the last hidden LayerNorm
    assert rows[-1][2] == rows[-2][2] == net.offsets["base.mlp.fc.5.weight"][0]
    assert rows[-1][3] == rows[-2][3] == net.offsets["base.mlp.fc.5.bias"][0]
    # each group has its own full [sp][H] folded pack (zero rows past n)
    assert rows[-1][6] - rows[-2][6] == 128 * 128 + 128
    assert net.pack_arena.numel() >= rows[-1][6] + 128 * 128 + 128
    assert len(net._head_packs) == 2


def test_tail_group_of_64_rows_is_an_atl64_image(stub_kernels):  # noqa: F811
    net, _ = _policy(192, [128, 128])
    assert net._md_sp == [128, 64] and [r[4] for r in net._table_rows[-2:]] == [128, 64]
    assert [r[10] for r in net._table_rows[-2:]] == [128, 64]
    net, _ = _policy(65, [64, 64])
    assert net._md_sp == [128] and net._table_rows[-1][4] == 65
    net, _ = _policy(512, [64, 128])
    assert net._md_sp == [128] * 4 and [r[4] for r in net._table_rows[-4:]] == [128] * 4
    net, _ = _policy(129, [128, 128])
    assert net._md_sp == [128, 64] and [r[4] for r in net._table_rows[-2:]] == [128, 1]


def _sample(M, n, obs_dim, rng):
    obs = rng.standard_normal((M, obs_dim)).astype(np.float32)
    act = rng.integers(0, n, size=(M, 1)).astype(np.float32)
    ones = np.ones((M, 1), np.float32)
    avail = np.ones((M, n), np.float32)
    return obs, act, ones, avail


def _names(calls_log):
    return [c[0] for c in calls_log]


@pytest.fixture
def ordered_calls(stub_kernels, monkeypatch):  # noqa: F811
    """The recorder of stub_kernels, additionally as ONE list in launch order."""
    from harl_amd import _lib
    log = []
    inner = _lib.call

    def rec(name, *args, tag=None):
        log.append((name, args))
        return inner(name, *args, tag=tag)

    monkeypatch.setattr(_lib, "call", rec)
    for mod in ("nets", "buffers", "happo", "hatrpo", "mappo", "v_critic", "valuenorm", "runner"):
        m = __import__(f"harl_amd.{mod}", fromlist=["x"])
        if hasattr(m, "call"):
            monkeypatch.setattr(m, "call", rec)
    return log


@pytest.mark.parametrize("recurrent", [False, True])
def test_update_and_get_actions_launch_sequence(ordered_calls, recurrent):
    from harl_amd.happo import HAPPO
    n, hidden, obs_dim = 200, ([64] if recurrent else [128, 128]), 19
    L, m = (3, 8) if recurrent else (1, 24)
    M = L * m
    args = default_args(hidden, use_recurrent_policy=recurrent)
    actor = HAPPO(args, Box((obs_dim,)), Discrete(n), device=CPU)
    rng = np.random.default_rng(0)
    obs, act, ones, avail = _sample(M, n, obs_dim, rng)
    rnn = np.zeros((m, 1, hidden[-1]), np.float32)
    masks = np.ones((M, 1), np.float32)
    ordered_calls.clear()
    actor.update((obs, rnn, act, masks, ones, np.full((M, 1), -5.0, np.float32), ones, avail, ones))
    seq = [c for c in _names(ordered_calls) if c in ("harl_mlp_linear", "harl_cat_head_loss", "harl_mlp_dw_partials", "harl_mlp_bwd_dx",
                                                     "harl_actor_head_loss", "harl_md_head_loss")]
    if recurrent:  # (the composed GRU has layer GEMMs of its own; the fused 64-wide one has none)
        assert seq.count("harl_mlp_linear") == 2
    # one logits GEMM per group, then the loss, then per group the weight-gradient GEMM + the backward into the trunk
    assert seq[:7] == ["harl_mlp_linear"] * 2 + ["harl_cat_head_loss"] + ["harl_mlp_dw_partials", "harl_mlp_bwd_dx"] * 2
    assert "harl_actor_head_loss" not in seq and "harl_md_head_loss" not in seq
    loss = [a for nm, a in ordered_calls if nm == "harl_cat_head_loss"][0]
    assert loss[1] == 2 and list(loss[2]) == [128, 128] and loss[3] == n          # n_groups, sp[], n
    assert loss[7] is not None and loss[12] is not None                            # availability and active masks are passed on
    lin = [a for nm, a in ordered_calls if nm == "harl_mlp_linear"][:2]
    assert [a[3] for a in lin] == [128, 128] and all(a[2] == hidden[-1] for a in lin)
    head_dw = [a for nm, a in ordered_calls if nm == "harl_mlp_dw_partials"][:2]
    assert [a[3] for a in head_dw] == [128, 128] and all(a[1] == 0 and a[10] == hidden[-1] for a in head_dw)
    # rollout step
    ordered_calls.clear()
    acts, logp, _ = actor.get_actions(obs[:m], rnn, masks[:m], avail[:m], deterministic=True)
    assert tuple(acts.shape) == (m, 1) and tuple(logp.shape) == (m, 1)
    seq = [c for c in _names(ordered_calls) if c in ("harl_mlp_linear", "harl_cat_head_logp", "harl_dist_rows", "harl_actor_head_logp")]
    assert seq == ["harl_mlp_linear"] * 2 + ["harl_cat_head_logp", "harl_dist_rows"]
    lp = [a for nm, a in ordered_calls if nm == "harl_cat_head_logp"][0]
    assert lp[12] is not None and lp[7] is not None and lp[8] is None             # head_out requested, masked, no log-probs
    out, ent, dist = actor.evaluate_actions(obs, rnn, act, masks, avail, ones)
    assert tuple(out.shape) == (M, 1) and ent.dim() == 0 and dist is not None


def test_narrow_head_keeps_its_route(ordered_calls):
    from harl_amd.happo import HAPPO
    n, M, obs_dim = 64, 24, 19
    actor = HAPPO(default_args([128, 128]), Box((obs_dim,)), Discrete(n), device=CPU)
    assert not actor.actor.cat_wide and not actor.actor.grouped and actor.actor.wide_head
    obs, act, ones, avail = _sample(M, n, obs_dim, np.random.default_rng(1))
    ordered_calls.clear()
    actor.update((obs, np.zeros((M, 1, 1), np.float32), act, None, ones, np.full((M, 1), -4.0, np.float32), ones, avail, ones))
    actor.get_actions(obs, None, None, avail, deterministic=True)
    names = _names(ordered_calls)
    assert not [c for c in names if c.startswith("harl_cat_")] and "harl_mlp_linear" not in names
    assert "harl_actor_head_loss" in names and "harl_actor_head_logp" in names


def test_unsupported_reason_table():
    model = dict(hidden_sizes=[128, 128], activation_func="relu")
    base = dict(model=model, algo={})
    for algo in ("happo", "haa2c", "mappo"):
        for n in (65, 200, 512):
            assert unsupported_reason(algo, base, act_space_name="Discrete", act_dim=n) is None
            assert unsupported_reason(algo, base, act_dim=n) is None
        assert "512" in unsupported_reason(algo, base, act_space_name="Discrete", act_dim=513)
    assert unsupported_reason("mappo", dict(model=model, algo=dict(share_param=True)), act_space_name="Discrete", act_dim=100) is None
    rec = dict(model=dict(model, hidden_sizes=[64], use_recurrent_policy=True), algo={})
    assert unsupported_reason("happo", rec, act_space_name="Discrete", act_dim=130) is None
    assert "HATRPO" in unsupported_reason("hatrpo", base, act_space_name="Discrete", act_dim=100)
    assert unsupported_reason("hatrpo", base, act_space_name="Discrete", act_dim=64) is None
    wide = dict(model=dict(model, hidden_sizes=[256, 256]), algo={})
    assert "256" in unsupported_reason("happo", wide, act_space_name="Discrete", act_dim=100)
    assert unsupported_reason("happo", wide, act_space_name="Discrete", act_dim=64) is None
    tanh = dict(model=dict(model, activation_func="tanh"), algo={})
    assert "relu" in unsupported_reason("happo", tanh, act_space_name="Discrete", act_dim=100)
    # Gaussian heads stop where they stopped
    assert unsupported_reason("happo", base, act_space_name="Box", act_dim=40) is not None
    assert unsupported_reason("happo", base, act_space_name="Box", act_dim=100) is not None


def test_constructors_refuse_what_is_not_built(stub_kernels):  # noqa: F811
    from harl_amd.hatrpo import HATRPO
    with pytest.raises(NotImplementedError, match="512"):
        _policy(513, [128, 128])
    with pytest.raises(NotImplementedError, match="256"):
        _policy(100, [256, 256])
    with pytest.raises(NotImplementedError, match="relu"):
        _policy(100, [128, 128], activation_func="tanh")
    with pytest.raises(NotImplementedError, match="HATRPO"):
        HATRPO(default_args([64, 64], kl_threshold=0.01, ls_step=10, accept_ratio=0.5, backtrack_coeff=0.8),
               Box((19,)), Discrete(100), device=CPU)
    # the texts are the ones the up-front check returns
    model = dict(hidden_sizes=[256, 256], activation_func="relu")
    with pytest.raises(NotImplementedError) as e:
        _policy(100, [256, 256])
    assert str(e.value) == unsupported_reason("happo", dict(model=model, algo={}), act_space_name="Discrete", act_dim=100)


def test_byte_models_follow_the_header():
    from harl_amd.traffic import algorithmic_bytes
    from tests.test_traffic_cpu import _params
    names = _params("harl_cat_head_loss")
    assert [names[i] for i in (1, 2, 3, 4, 5, 7, 11, 12, 18)] == ["n_groups", "sp", "n", "M", "idx", "avail", "factor", "active", "logp_out"]
    names = _params("harl_cat_head_logp")
    assert [names[i] for i in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12)] == ["n_groups", "sp", "n", "M", "idx", "actions", "avail", "logp_out",
                                                                         "ent_out", "old_logp", "factor", "head_out"]
    B = 819200
    # n = 200: two ATL(128) images read and overwritten (2 x 1024 B), the availability row (800 B), actions / old log-probs /
    # advantages / factor / active masks (20 B)
    args = (1, 2, [128, 128], 200, B, None, 1, 1, 1, 1, None, 1, 1, 0.2, 0.01, 0, 0, 0, None, 1, 1024, 0)
    assert algorithmic_bytes("harl_cat_head_loss", args) == B * (2048.0 + 800.0 + 20.0)
    # log-prob + factor pass: the images once (1024 B), availability (800 B), actions, log-probs out, old log-probs (12 B), factor r/w (8 B)
    args = (1, 2, [128, 128], 200, B, None, 1, 1, 1, None, 1, 1, None, 0, 0, 0)
    assert algorithmic_bytes("harl_cat_head_logp", args) == B * (1024.0 + 800.0 + 12.0 + 8.0)
