"""Gaussian action heads of 33..64 dimensions (HARL_GAUSS_WIDE=1: k_gauss_head_wide in csrc/heads.hip, harl_ls_reduce and
harl_adam_fold_ls in csrc/elementwise.hip) against the oracle on the GPU: the checks, helpers and 1e-5 bar the narrower heads
are held to (tests/gpu_checks.py, tests/test_gpu_parity.py), at the smallest shapes that reach one dimension past 32, a head
without padding columns, tail slabs, several workgroups and both hidden widths.  Without the switch every test that builds such
an actor stops at the constructor's NotImplementedError."""
import numpy as np
import pytest
import torch

from tests.test_gpu_parity import TOL, _assert_all

pytestmark = pytest.mark.gpu


def _G():
    from tests import gpu_checks
    return gpu_checks


@pytest.fixture(autouse=True)
def wide(monkeypatch):
    monkeypatch.setenv("HARL_GAUSS_WIDE", "1")


SPECS = [
    dict(name="box33_h64", obs_dim=18, share_obs_dim=54, act_dim=33, discrete=False, hidden_sizes=[64, 64], M=77),
    dict(name="box40_h128", obs_dim=40, share_obs_dim=33, act_dim=40, discrete=False, hidden_sizes=[128, 128], M=513),
    dict(name="box64_128_64", obs_dim=31, share_obs_dim=65, act_dim=64, discrete=False, hidden_sizes=[128, 64], M=640),
    dict(name="box50_64_128", obs_dim=90, share_obs_dim=70, act_dim=50, discrete=False, hidden_sizes=[64, 128], M=1500),
]
BOX50 = SPECS[3]
IDS = [s["name"] for s in SPECS]


def _show(res):
    print({k: (f"{v:.2e}" if isinstance(v, float) else v) for k, v in res.items()})
    return res


@pytest.mark.parametrize("i", range(len(SPECS)), ids=IDS)
def test_forward_matches_oracle(i):
    _assert_all(_show(_G().check_forward(SPECS[i])), tol=TOL)


@pytest.mark.parametrize("i", range(len(SPECS)), ids=IDS)
def test_gradients_match_oracle(i):
    _assert_all(_show(_G().check_gradients(SPECS[i])), tol=TOL)


def test_gradients_mean_aggregation_with_inactive_agents():
    _assert_all(_show(_G().check_gradients(BOX50, agg="mean", inactive_p=0.3)), tol=TOL)


def test_gradients_without_policy_active_masks():
    """use_policy_active_masks=False: the stored active masks (30 % zeros) must be ignored."""
    _assert_all(_show(_G().check_gradients(dict(BOX50, over=dict(use_policy_active_masks=False)), inactive_p=0.3)), tol=TOL)


@pytest.mark.parametrize("i", [0, 3], ids=["box33_h64", "box50_64_128"])
def test_get_actions(i):
    """The mode is the mean, the returned log-probs are the oracle's of the returned actions, and the samples have the moments
    of N(mean, sigma) -- the bars tests/test_gpu_parity.py holds the narrower heads to."""
    res = _show(_G().check_get_actions(SPECS[i]))
    for k, v in res.items():
        if "zscore" in k:
            assert v < 0.05, (k, v)
        else:
            assert v < TOL, (k, v)


def _one_update(G, spec, M, seed=7, **over):
    """(actor, state dict, cfg, oracle sample) of one HAPPO.update at ``spec`` on synthetic rows: policy-consistent actions, stored
    log-probs 0.15 sigma around the current ones (ratios straddle the clip range), 20 % inactive rows, factors around 1."""
    from harl_amd.synthetic import Shapes, make_buffers
    sh = Shapes(T=M, N=1, A=1, obs_dim=spec["obs_dim"], share_obs_dim=spec["share_obs_dim"], act_dim=spec["act_dim"], discrete=False,
                hidden_sizes=spec["hidden_sizes"])
    d = make_buffers(sh, seed, inactive_p=0.2)
    actor, sd, args = G._mk_actor(sh, seed + 1, **over)
    cfg = G.O.PathConfig.from_reference_dicts({}, args, args)
    rng = np.random.default_rng(seed)
    obs = d.obs[0][:-1].reshape(M, -1)
    p = {k: torch.from_numpy(v) for k, v in sd.items()}
    with torch.no_grad():
        _, (mean, std) = G.O._dist_params(p, cfg, torch.from_numpy(obs), None)
        act = (mean.numpy() + std.numpy() * rng.standard_normal(mean.shape)).astype(np.float32)
        lp, _, _ = G.O.actor_evaluate_actions(p, cfg, torch.from_numpy(obs), torch.from_numpy(act), None, None)
    old_logp = (lp.numpy() + 0.15 * rng.standard_normal(lp.shape)).astype(np.float32)
    adv = rng.standard_normal((M, 1)).astype(np.float32)
    factor = (1 + 0.2 * rng.standard_normal((M, 1))).astype(np.float32)
    active = d.active_masks[0][:-1].reshape(M, 1)
    return actor, sd, cfg, (obs, act, active, old_logp, adv, None, factor)


def _hip_sample(s):
    obs, act, active, old_logp, adv, avail, factor = s
    return (obs, np.zeros((obs.shape[0], 1, 1), np.float32), act, None, active, old_logp, adv, avail, factor)


@pytest.mark.parametrize("i", [0, 1], ids=["box33", "box40"])
def test_padding_dimensions_and_tail_samples_get_zero_gradient(i):
    """After update() at M = 77 the ATL(64) dhead image holds exactly 0 in the columns past act_dim and in samples 77..95 of the
    last slab; the real entries are not all zero."""
    G = _G()
    M, n = 77, SPECS[i]["act_dim"]
    actor, _, _, s = _one_update(G, SPECS[i], M)
    actor.update(_hip_sample(s))
    torch.cuda.synchronize()
    net = actor.actor
    ns = (M + 31) // 32
    rows = G._atl_rows(net.dhead[:ns * 32 * 64], ns, 64)
    assert rows.shape == (96, 64)
    assert float(rows[:M, :n].abs().max()) > 0.0
    assert float(rows[:, n:].abs().max()) == 0.0
    assert float(rows[M:].abs().max()) == 0.0
    # ... and so do the log_std rows: nothing in the columns past act_dim
    assert float(net.part_ls.reshape(-1, 64)[:, n:].abs().max()) == 0.0 and float(net.ls_sum[n:].abs().max()) == 0.0
    assert float(net.ls_sum[:n].abs().min()) > 0.0


def _restore(actor, state):
    net, opt = actor.actor, actor.actor_optimizer
    with torch.no_grad():
        net.flat_param.copy_(state[0])
    opt.exp_avg.copy_(state[1])
    opt.exp_avg_sq.copy_(state[2])
    opt.step_count = state[3]
    net.invalidate_caches()


def test_update_is_deterministic():
    """The same update() twice from the same state: bit-identical gradient arena, loss scalars, log_std sums and parameters."""
    G = _G()
    actor, _, _, s = _one_update(G, BOX50, 1500, seed=23)
    net, opt = actor.actor, actor.actor_optimizer
    state = (net.flat_param.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.step_count)
    runs = []
    for _ in range(2):
        _restore(actor, state)
        taps = []
        actor._grad_tap = lambda gr, sc: taps.append(sc.clone())
        actor.update(_hip_sample(s))
        torch.cuda.synchronize()
        runs.append((net.flat_grad.clone(), taps[0], net.ls_sum.clone(), net.flat_param.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert float(runs[0][0].abs().max()) > 0.0 and float(runs[0][2].abs().max()) > 0.0


@pytest.mark.parametrize("i,agg", [(0, "prod"), (2, "prod"), (3, "mean")], ids=["box33_prod", "box64_prod", "box50_mean"])
def test_log_std_path(i, agg):
    """The log_std gradient's own route (wave-private LDS tiles -> part_ls -> harl_ls_reduce -> harl_adam_fold_ls): the 64 sums
    against a float64 restatement of sum_s d(loss_s)/d(log_std_d), the tapped gradient's log_std block and log_std after the
    step against the oracle's update."""
    G = _G()
    from tests.helpers import vec_rel_err
    spec = SPECS[i]
    M, n = spec["M"], spec["act_dim"]
    actor, sd, cfg, s = _one_update(G, spec, M, seed=31, action_aggregation=agg)
    obs, act, active, old_logp, adv, _, factor = s
    # float64: the unscaled sums  sum_s active (-factor min(imp adv, clip(imp) adv)) - entropy_coef sum_s active ent_s
    p64 = {k: torch.from_numpy(v).double() for k, v in sd.items()}
    ls = p64["act.action_out.log_std"].clone().requires_grad_(True)
    p64["act.action_out.log_std"] = ls
    f64 = lambda x: torch.from_numpy(x).double()  # noqa: E731
    _, (mean, std) = G.O._dist_params(p64, cfg, f64(obs), None)
    mean = mean.detach()
    lp = -((f64(act) - mean) ** 2) / (2 * std * std) - torch.log(std) - 0.5 * np.log(2 * np.pi)
    r = torch.exp(lp - f64(old_logp))
    imp = r.prod(-1, keepdim=True) if agg == "prod" else r.mean(-1, keepdim=True)
    surr = torch.min(imp * f64(adv), torch.clamp(imp, 1.0 - cfg.clip_param, 1.0 + cfg.clip_param) * f64(adv))
    ent = (0.5 + 0.5 * np.log(2 * np.pi) + torch.log(std)).sum(-1, keepdim=True)
    total = (f64(active) * (-f64(factor) * surr)).sum() - cfg.entropy_coef * (f64(active) * ent).sum()
    want = torch.autograd.grad(total, ls)[0].numpy()
    oracle = G.O.OracleHAPPO({k: torch.from_numpy(v) for k, v in sd.items()}, cfg)
    _, _, _, _, g = oracle.update(s, keep_grad=True)
    taps = []
    actor._grad_tap = lambda gr, sc: taps.append(gr.clone())
    actor.update(_hip_sample(s))
    torch.cuda.synchronize()
    net = actor.actor
    off = net.offsets["act.action_out.log_std"][0]
    got = net.ls_sum.cpu().numpy()
    assert np.all(got[n:] == 0.0)
    res = dict(ls_sum_vs_f64_vec_rel=vec_rel_err(got[:n], want),
               log_std_grad_vec_rel=vec_rel_err(taps[0][off:off + n].cpu().numpy(), g[off:off + n]),
               log_std_after_vec_rel=vec_rel_err(net.log_std().cpu().numpy(), oracle.net.flat()[off:off + n]))
    assert not np.array_equal(net.log_std().cpu().numpy(), sd["act.action_out.log_std"])
    _assert_all(_show(res), tol=TOL)


# Whole train() against the oracle, as tests/test_gpu_cat_wide.py runs it (check_baseline_shape on a case of this file's own)
TRAIN_SHAPES = {
    "box48_happo_mb2": dict(shapes=dict(T=12, N=8, A=2, obs_dim=18, share_obs_dim=54, act_dim=48, discrete=False,
                                        hidden_sizes=[128, 128]), seed=11,
                            overrides=dict(ppo_epoch=1, critic_epoch=1, actor_num_mini_batch=2)),
    "box36_mappo_shared": dict(shapes=dict(T=12, N=8, A=2, obs_dim=18, share_obs_dim=54, act_dim=36, discrete=False,
                                           hidden_sizes=[64, 64]), seed=12, algo="mappo",
                               overrides=dict(ppo_epoch=1, critic_epoch=1, share_param=True)),
    "box33_haa2c": dict(shapes=dict(T=12, N=8, A=2, obs_dim=18, share_obs_dim=54, act_dim=33, discrete=False,
                                    hidden_sizes=[128, 64]), seed=13, algo="haa2c",
                        overrides=dict(ppo_epoch=1, critic_epoch=1, a2c_epoch=1)),
}


@pytest.mark.parametrize("name", list(TRAIN_SHAPES))
def test_whole_train_matches_oracle(name, monkeypatch):
    """The first agent of an update has factor 1 and normalised advantages, so its policy loss is -mean(ratio x advantage), a
    mean that nearly cancels (box33_haa2c: 0.0127 over 96 rows of terms of order 1): the entry that shows whether the kernel's
    importance weight (formed in fp64, heads_common.h) is as good as the reference's."""
    G = _G()
    from tests import helpers as H
    spec = TRAIN_SHAPES[name]
    shared = bool(spec["overrides"].get("share_param"))

    class Case(H.SyntheticCase):
        def __init__(self, nm, shapes, seed, algo_name="happo", overrides=None, **kw):
            super().__init__(nm, shapes, seed, algo_name=algo_name, overrides=overrides, **kw)
            if algo_name == "haa2c":
                self.algo["a2c_epoch"] = (overrides or {}).get("a2c_epoch", 1)
            if shared:
                self.algo["share_param"] = self.share_param = True
                self.actor_sd = [self.actor_sd[0]] * shapes.A

    monkeypatch.setattr(H, "SyntheticCase", Case)
    monkeypatch.setitem(G.BASELINE_SHAPES, name, spec)
    if spec.get("algo") == "mappo":
        ma_train = G.O.ma_train
        monkeypatch.setattr(G.O, "ha_train", lambda *a: ma_train(*a, share_param=shared))
    _assert_all(_show(G.check_baseline_shape(name)), tol=TOL)


def test_gru_policy_update():
    spec = dict(name="rnn_box34_L5_m40", obs_dim=30, share_obs_dim=20, act_dim=34, discrete=False, hidden_sizes=[64], L=5, m=40)
    _assert_all(_show(_G().check_rnn_update(spec)), tol=TOL)


def test_box32_update_is_bit_identical_through_the_old_adam_entry_point(monkeypatch):
    """Switch off, no regression: harl_adam_fold and harl_adam_fold_dev share their kernel body with harl_adam_fold_ls.  One
    Box(32) update through the library's harl_adam_fold, and the same update from the same state with the optimiser launch
    redirected to harl_adam_fold_ls -- its log_std sums copied from the scalar row the first run published, which is where a
    32-wide head leaves them -- end in bit-identical parameter, gradient and moment arenas."""
    G = _G()
    from harl_amd import _lib, nets
    monkeypatch.delenv("HARL_GAUSS_WIDE", raising=False)
    spec = dict(obs_dim=18, share_obs_dim=54, act_dim=32, hidden_sizes=[128, 128])
    actor, _, _, s = _one_update(G, spec, 777, seed=5)
    net, opt = actor.actor, actor.actor_optimizer
    assert not net.gauss_wide and not hasattr(net, "ls_sum")
    state = (net.flat_param.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.step_count)
    real_call = nets.call
    seen = []

    def redirect(name, *args, tag=None):
        if name != "harl_adam_fold":
            return real_call(name, *args, tag=tag)
        ls = torch.zeros(64, dtype=torch.float64, device=net.scalars.device)
        ls[:32] = runs[0][4][8:40]   # (the same state and rows: the same sums, bit for bit -- test_update_is_deterministic)
        seen.append(ls)
        return real_call("harl_adam_fold_ls", *args[:27], _lib.ptr(ls), *args[27:], tag=tag)

    runs = []
    for use_new in (False, True):
        _restore(actor, state)
        monkeypatch.setattr(nets, "call", redirect if use_new else real_call)
        actor.update(_hip_sample(s))
        torch.cuda.synchronize()
        runs.append((net.flat_param.clone(), net.flat_grad.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), net.scalars.clone()))
    assert len(seen) == 1 and float(seen[0][:32].abs().min()) > 0.0
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert not torch.equal(runs[0][0], state[0])
