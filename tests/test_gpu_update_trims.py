"""-m gpu: a whole HAPPO train() with the update's trimmed head and tail -- every network's input image built in ONE launch up
front (runner._prepare_inputs, harl_x0n_multi) and no post-update log-prob pass behind the last agent of the order -- against the
same train() with HARL_X0N_MULTI=0 HARL_LAST_POST_PASS=1 (one image launch per network where it is first read, one pass per
agent).  Neither changes an operand or an order of operations of anything that is kept: statistics, parameters, returns, ValueNorm
statistics and the CPU generator must come out equal bit for bit.  T = 4, N = 32 (128 rows: four slabs), MLP [128, 128],
Box(5), obs 18 / share_obs 54."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T, N = 4, 32


def _runner(A, fixed_order, seed):
    from harl_amd.runner import RUNNER_REGISTRY
    from harl_amd.synthetic import Shapes, make_buffers
    from tests.gpu_checks import DEV, Box, default_args, dev
    torch.manual_seed(seed)
    np.random.seed(seed)
    a = default_args([128, 128], ppo_epoch=2, critic_epoch=2, fixed_order=fixed_order)
    train = dict(n_rollout_threads=N, episode_length=T, use_valuenorm=True, use_linear_lr_decay=False,
                 use_proper_time_limits=True, model_dir=None, eval_interval=25, use_eval=False, log_interval=1,
                 num_env_steps=T * N * 2)
    r = RUNNER_REGISTRY["happo"](dict(algo="happo"), dict(train=train, model=dict(a), algo=dict(a)), dict(state_type="EP"),
                                 obs_spaces=[Box((18,))] * A, share_obs_space=Box((54,)), act_spaces=[Box((5,))] * A, device=DEV)
    sh = Shapes(T=T, N=N, A=A, obs_dim=18, share_obs_dim=54, act_dim=5, hidden_sizes=[128, 128])
    d = make_buffers(sh, seed + 1, inactive_p=0.1)
    for ag in range(A):
        b = r.actor_buffer[ag]
        b.obs.copy_(dev(d.obs[ag]))
        b.actions.copy_(dev(d.actions[ag]))
        b.action_log_probs.copy_(dev(d.action_log_probs[ag]))
        b.masks.copy_(dev(d.masks[ag]))
        b.active_masks.copy_(dev(d.active_masks[ag]))
    cb = r.critic_buffer
    cb.share_obs.copy_(dev(d.share_obs))
    cb.rewards.copy_(dev(d.rewards))
    cb.value_preds.copy_(dev(d.value_preds))
    cb.masks.copy_(dev(d.critic_masks))
    cb.bad_masks.copy_(dev(d.bad_masks))
    return r


def _update(A, fixed_order, seed, env, monkeypatch):
    """Two compute() + train() rounds (the second starts from caches and workspaces the first has left) -> everything they leave."""
    for k in ("HARL_X0N_MULTI", "HARL_LAST_POST_PASS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    r = _runner(A, fixed_order, seed)
    torch.manual_seed(seed + 7)
    out = {}
    for rnd in range(2):
        r.prep_rollout()
        r.compute()
        r.prep_training()
        infos, cinfo = r.train()
        torch.cuda.synchronize()
        out[f"infos{rnd}"] = torch.tensor([[float(i[k]) for k in sorted(i)] for i in infos], dtype=torch.float64)
        out[f"cinfo{rnd}"] = torch.tensor([float(cinfo[k]) for k in sorted(cinfo)], dtype=torch.float64)
    for a in range(A):
        out[f"actor{a}"] = r.actor[a].actor.flat_reference().detach().clone()
    out["critic"] = r.critic.critic.flat_reference().detach().clone()
    out["returns"] = r.critic_buffer.returns.clone()
    out["vn"] = r.value_normalizer.stats.clone()
    out["rng"] = torch.get_rng_state()
    return out


@pytest.mark.parametrize("A,fixed_order", [(2, True), (3, True), (3, False)], ids=["a2", "a3", "a3_random_order"])
def test_trimmed_update_is_bit_identical(A, fixed_order, monkeypatch):
    seed = 40 + A
    new = _update(A, fixed_order, seed, {}, monkeypatch)
    old = _update(A, fixed_order, seed, {"HARL_X0N_MULTI": "0", "HARL_LAST_POST_PASS": "1"}, monkeypatch)
    assert sorted(new) == sorted(old)
    for k in new:
        assert torch.equal(new[k], old[k]), k
    assert bool(torch.isfinite(new["infos1"]).all()) and bool(torch.isfinite(new["critic"]).all())


def test_one_image_launch_and_no_pass_behind_the_last_agent(monkeypatch):
    """The launches themselves, counted at the C-ABI boundary: per train() ONE harl_x0n_multi and no harl_mlp_x0n_wide, and
    one post-update log-prob pass fewer than agents; with both switches back, one image launch per network and a pass per agent."""
    from harl_amd import _lib, nets, runner as runner_mod

    def count(env):
        for k in ("HARL_X0N_MULTI", "HARL_LAST_POST_PASS"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        r = _runner(3, False, 50)
        r.prep_training()
        r.train()  # (workspaces allocated, LDS limits raised)
        seen = {}
        real_call, real_multi = _lib.call, _lib.x0n_multi

        def call(name, *a, **k):
            seen[name] = seen.get(name, 0) + 1
            return real_call(name, *a, **k)

        def multi(*a, **k):
            seen["harl_x0n_multi"] = seen.get("harl_x0n_multi", 0) + 1
            return real_multi(*a, **k)

        mods = [m for m in (nets, runner_mod, __import__("harl_amd.happo", fromlist=["x"]), __import__("harl_amd.v_critic", fromlist=["x"]))]
        for m in mods:
            if hasattr(m, "call"):
                monkeypatch.setattr(m, "call", call)
        monkeypatch.setattr(_lib, "x0n_multi", multi)
        r.prep_training()
        r.train()
        torch.cuda.synchronize()
        monkeypatch.undo()
        return seen

    new = count({})
    assert new.get("harl_x0n_multi", 0) == 1 and new.get("harl_mlp_x0n_wide", 0) == 0, new
    assert new["harl_update_logp"] == 2, new
    old = count({"HARL_X0N_MULTI": "0", "HARL_LAST_POST_PASS": "1"})
    assert old.get("harl_x0n_multi", 0) == 0 and old["harl_mlp_x0n_wide"] == 4 and old["harl_update_logp"] == 3, old
