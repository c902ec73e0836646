"""HATRPO on Categorical heads of 65..512 actions (HARL_TRPO_CAT_WIDE=1), host side without a GPU: what the switch accepts and
still refuses, and the launch sequence of the surrogate, the Fisher-vector product and the KL sum with the C-ABI calls recorded
instead of executed (kernels stubbed as in tests/test_cat_wide_cpu.py; the arithmetic is tests/test_gpu_trpo_cat_wide.py's)."""
import pytest
import torch

from harl_amd.configs import CAT_WIDE_REFUSALS, unsupported_reason
from tests.gpu_checks import Box, Discrete, default_args
from tests.test_cat_wide_cpu import _names, ordered_calls  # noqa: F401  (fixture: the recorder as one list in launch order)
from tests.test_multidiscrete_cpu import stub_kernels  # noqa: F401  (fixture)

CPU = torch.device("cpu")
TRPO = dict(kl_threshold=0.01, ls_step=10, accept_ratio=0.5, backtrack_coeff=0.8)
HEAD_CALLS = ("harl_mlp_linear", "harl_cat_head_loss", "harl_cat_head_fvp", "harl_mlp_dw_partials", "harl_mlp_bwd_dx",
              "harl_actor_head_loss", "harl_actor_head_fvp")


@pytest.fixture(autouse=True)
def _switch_on(monkeypatch):
    monkeypatch.setenv("HARL_TRPO_CAT_WIDE", "1")


def _hatrpo(n, hidden, obs_dim=19, **over):
    from harl_amd.hatrpo import HATRPO
    return HATRPO(default_args(hidden, **TRPO, **over), Box((obs_dim,)), Discrete(n), device=CPU)


def test_switch_accepts_wide_heads_and_keeps_the_other_refusals(stub_kernels):  # noqa: F811
    t = _hatrpo(100, [64, 64])
    assert t.actor.cat_wide and t.actor._md_sp == [128]
    model = dict(hidden_sizes=[128, 128], activation_func="relu")
    base = dict(model=model, algo={})
    for n in (65, 100, 512):
        assert unsupported_reason("hatrpo", base, None, "Discrete", n) is None
    assert unsupported_reason("hatrpo", base, None, "Discrete", 513) == CAT_WIDE_REFUSALS["n"]
    assert unsupported_reason("hatrpo", dict(model=dict(model, hidden_sizes=[256, 256]), algo={}), None, "Discrete", 100) \
        == CAT_WIDE_REFUSALS["panel"]
    assert unsupported_reason("hatrpo", dict(model=dict(model, activation_func="tanh"), algo={}), None, "Discrete", 100) \
        == CAT_WIDE_REFUSALS["act"]
    with pytest.raises(NotImplementedError, match="512") as e:
        _hatrpo(513, [128, 128])
    assert str(e.value) == CAT_WIDE_REFUSALS["n"]
    with pytest.raises(NotImplementedError, match="256") as e:
        _hatrpo(100, [256, 256])
    assert str(e.value) == CAT_WIDE_REFUSALS["panel"]
    with pytest.raises(NotImplementedError, match="relu") as e:
        _hatrpo(100, [128, 128], activation_func="tanh")
    assert str(e.value) == CAT_WIDE_REFUSALS["act"]


def test_fused_gru_is_taken_and_composed_grus_are_refused(stub_kernels):  # noqa: F811
    t = _hatrpo(130, [64], use_recurrent_policy=True)
    assert t.actor.cat_wide and t.actor.recurrent and not t.actor.gru_wide
    rec = dict(hidden_sizes=[64], activation_func="relu", use_recurrent_policy=True)
    assert unsupported_reason("hatrpo", dict(model=rec, algo={}), None, "Discrete", 130) is None
    for hidden, rn in (([128, 128], 1), ([64], 2)):
        with pytest.raises(NotImplementedError, match="GRU") as e:
            _hatrpo(130, hidden, use_recurrent_policy=True, recurrent_n=rn)
        assert str(e.value) == CAT_WIDE_REFUSALS["hatrpo_gru_wide"]
        model = dict(rec, hidden_sizes=hidden, recurrent_n=rn)
        assert unsupported_reason("hatrpo", dict(model=model, algo={}), None, "Discrete", 130) == CAT_WIDE_REFUSALS["hatrpo_gru_wide"]
        assert unsupported_reason("happo", dict(model=model, algo={}), None, "Discrete", 130) is None


def _batch(t, m, n, obs_dim):
    f = lambda *s: torch.zeros(*s, dtype=torch.float32)  # noqa: E731
    return f(m, obs_dim), f(m, 1), torch.ones(m, n), f(m, 1), f(m), f(m), torch.ones(m)


def test_surrogate_and_fvp_launch_sequence(ordered_calls):  # noqa: F811
    n, hidden, obs_dim, m = 200, [128, 128], 19, 24
    t = _hatrpo(n, hidden, obs_dim)
    net = t.actor
    obs, act, avail, old_logp, adv, factor, active = _batch(t, m, n, obs_dim)
    net.fold()
    ordered_calls.clear()
    t._surrogate(obs, m, act, avail, old_logp, adv, None, factor, active, want_grad=True)
    seq = [c for c in _names(ordered_calls) if c in HEAD_CALLS]
    # one logits GEMM per group, the loss in HATRPO's form, per group the weight-gradient GEMM + the backward into the trunk
    # (then the trunk's own layer kernels)
    assert seq.count("harl_mlp_linear") == 2 and seq.count("harl_cat_head_loss") == 1 and "harl_actor_head_loss" not in seq
    assert seq[:7] == ["harl_mlp_linear"] * 2 + ["harl_cat_head_loss"] + ["harl_mlp_dw_partials", "harl_mlp_bwd_dx"] * 2
    loss = [a for nm, a in ordered_calls if nm == "harl_cat_head_loss"][0]
    assert loss[1] == 2 and list(loss[2]) == [128, 128] and loss[3] == n and loss[4] == m
    assert loss[15] == 1 and loss[13] == 0.0 and loss[14] == 0.0           # mode 1, no clip, no entropy coefficient
    assert loss[7] is not None and loss[11] is not None and loss[12] is not None and loss[18] is None
    assert (loss[16], loss[17]) == (0, 0)

    ordered_calls.clear()
    out = t._fvp(obs, m, m, avail, torch.zeros(net.n_params))
    assert tuple(out.shape) == (net.n_params,)
    seq = [c for c in _names(ordered_calls) if c in HEAD_CALLS]
    # the logits again (2), per group W'_g x_dot and W'_g_dot x_hat + b'_g_dot (4), ONE head launch, the same backward pairs
    assert seq.count("harl_mlp_linear") == 6 and seq.count("harl_cat_head_fvp") == 1 and "harl_actor_head_fvp" not in seq
    assert seq[:11] == ["harl_mlp_linear"] * 6 + ["harl_cat_head_fvp"] + ["harl_mlp_dw_partials", "harl_mlp_bwd_dx"] * 2
    fvp = [a for nm, a in ordered_calls if nm == "harl_cat_head_fvp"][0]
    assert fvp[3] == 2 and list(fvp[4]) == [128, 128] and fvp[5] == n and fvp[6] == m
    assert fvp[7] == avail.data_ptr() and (fvp[8], fvp[9]) == (0, 0)        # availability passed on, no padding sequences
    assert list(fvp[0]) == [z.data_ptr() for z in net.md_z]                # written in place into the logits images
    lin = [a for nm, a in ordered_calls if nm == "harl_mlp_linear"]
    ws = t._tangent_ws
    assert [a[6] for a in lin[:2]] == [z.data_ptr() for z in net.md_z]
    assert [a[6] for a in lin[2::2]] == list(fvp[1]) == [z.data_ptr() for z in ws["cat_zd"][0]]
    assert [a[6] for a in lin[3::2]] == list(fvp[2]) == [z.data_ptr() for z in ws["cat_zd"][1]]
    # W'_g x_dot: the trunk tangent through the group's folded pack with a zero bias; W'_g_dot x_hat: the head input through the
    # group's block of the tangent arena, at the offsets of the folded pack
    base = net.pack_arena.data_ptr()
    for g, (a, b) in enumerate(zip(lin[2::2], lin[3::2])):
        assert a[0] == ws["xd"][-1].data_ptr() and a[4] == net._head_packs[g][0].data_ptr() and a[5] == ws["cat_zero_bias"].data_ptr()
        assert b[0] == net.xh[-1].data_ptr() and b[4] - ws["pack_d"].data_ptr() == net._head_packs[g][0].data_ptr() - base
        assert b[5] - ws["pack_d"].data_ptr() == net._head_packs[g][1].data_ptr() - base
        assert a[2:4] == b[2:4] == (128, 128)
    assert float(ws["cat_zero_bias"].abs().max()) == 0.0 and float(ws["pack_d"].abs().max()) == 0.0


def test_kl_sum_and_recurrent_head_outputs_take_the_grouped_kernels(ordered_calls):  # noqa: F811
    from harl_amd.nets import build_seq
    n, obs_dim, L, m = 130, 19, 3, 8
    t = _hatrpo(n, [64], obs_dim, use_recurrent_policy=True)
    net = t.actor
    seq = build_seq(CPU, L, m, 64, h0=torch.zeros(m, 64), masks_src=torch.ones(L * m))
    rows = L * seq["m_pad"]
    obs, act, avail, old_logp, adv, factor, active = _batch(t, L * m, n, obs_dim)
    net.fold()
    t._surrogate(obs, rows, act, avail, old_logp, adv, None, factor, active, want_grad=False, seq=seq)
    loss = [a for nm, a in ordered_calls if nm == "harl_cat_head_loss"][-1]
    assert loss[15] == 1 and (loss[16], loss[17]) == (m, seq["m_pad"])
    avail_rows = torch.ones(rows, n)
    ordered_calls.clear()
    t._fvp(obs, rows, L * m, avail_rows, torch.zeros(net.n_params), seq=seq)
    fvp = [a for nm, a in ordered_calls if nm == "harl_cat_head_fvp"]
    assert len(fvp) == 1 and fvp[0][7] == avail_rows.data_ptr() and (fvp[0][8], fvp[0][9]) == (m, seq["m_pad"])
    assert "harl_actor_head_fvp" not in _names(ordered_calls)
    ordered_calls.clear()
    ho = t._head_outputs(obs, rows, act, avail, reuse_trunk=True, seq=seq, avail_rows=avail_rows)
    assert tuple(ho.shape) == (L * m, n)                                    # padding sequences compacted away
    names = _names(ordered_calls)
    assert names.count("harl_mlp_linear") == 2 and "harl_actor_head_logp" not in names
    lp = [a for nm, a in ordered_calls if nm == "harl_cat_head_logp"][0]
    assert lp[12] is not None and lp[7] == avail_rows.data_ptr() and lp[6] is None and (lp[13], lp[14]) == (m, seq["m_pad"])
    ordered_calls.clear()
    acc = torch.zeros(1, dtype=torch.float64)
    t._kl_sum(ho, None, ho, L * m, acc=acc)
    names = _names(ordered_calls)
    assert names == ["harl_cat_kl_sum"]
    kl = ordered_calls[0][1]
    assert kl[2] == L * m and kl[3] == n and kl[4] == acc.data_ptr()


def test_byte_models_of_the_new_kernels():
    from harl_amd.traffic import algorithmic_bytes
    from tests.test_traffic_cpu import _params
    names = _params("harl_cat_head_fvp")
    assert names == ["z", "zd_a", "zd_b", "n_groups", "sp", "n", "M", "avail", "m_valid", "m_pad", "stream"]
    assert _params("harl_cat_kl_sum") == ["head_old", "head_new", "M", "n", "out_sum", "stream"]
    B = 819200
    # n = 200, two ATL(128) images: logits twice (2 048 B), each tangent set twice (2 048 B), availability twice (1 600 B), result (1 024 B)
    assert algorithmic_bytes("harl_cat_head_fvp", (1, 1, 1, 2, [128, 128], 200, B, 1, 0, 0, 0)) == B * (2048.0 + 2 * 2048.0 + 1600.0 + 1024.0)
    assert algorithmic_bytes("harl_cat_head_fvp", (1, 1, None, 2, [128, 128], 200, B, None, 0, 0, 0)) == B * (2048.0 + 2048.0 + 1024.0)
    assert algorithmic_bytes("harl_cat_kl_sum", (1, 1, B, 200, 1, 0)) == B * 1600.0
