"""Categorical action heads of 65..512 actions (csrc/cathead.hip) against the oracle on the GPU: the same checks, helpers and
1e-5 bar the <= 64-way heads are held to (tests/gpu_checks.py, tests/test_gpu_parity.py), at the smallest shapes that reach
every group layout -- one logit beyond a group, a one-logit second group, an ATL(64) tail group, four full groups, tail slabs
and several workgroups."""
import numpy as np
import pytest
import torch

from tests.test_gpu_parity import TOL, _assert_all

pytestmark = pytest.mark.gpu


def _G():
    from tests import gpu_checks
    return gpu_checks


SPECS = [
    dict(name="cat65_h64", obs_dim=18, share_obs_dim=54, act_dim=65, discrete=True, hidden_sizes=[64, 64], M=77),
    dict(name="cat129_h128", obs_dim=40, share_obs_dim=33, act_dim=129, discrete=True, hidden_sizes=[128, 128], M=513),
    dict(name="cat192_128_64", obs_dim=31, share_obs_dim=65, act_dim=192, discrete=True, hidden_sizes=[128, 64], M=640),
    dict(name="cat200_64_128", obs_dim=90, share_obs_dim=70, act_dim=200, discrete=True, hidden_sizes=[64, 128], M=1500),
    dict(name="cat512_h128", obs_dim=18, share_obs_dim=54, act_dim=512, discrete=True, hidden_sizes=[128, 128], M=4100),
]
CAT200 = SPECS[3]


@pytest.mark.parametrize("i", range(len(SPECS)), ids=[s["name"] for s in SPECS])
def test_forward_matches_oracle(i):
    _assert_all(_G().check_forward(SPECS[i]), tol=TOL)


@pytest.mark.parametrize("i", range(len(SPECS)), ids=[s["name"] for s in SPECS])
def test_gradients_match_oracle(i):
    res = _G().check_gradients(SPECS[i])
    print({k: (f"{v:.2e}" if isinstance(v, float) else v) for k, v in res.items()})
    _assert_all(res, tol=TOL)


def test_gradients_mean_aggregation_with_inactive_agents():
    _assert_all(_G().check_gradients(CAT200, agg="mean", inactive_p=0.3), tol=TOL)


@pytest.mark.parametrize("inactive_p", [0.0, 0.3])
def test_gradients_without_policy_active_masks(inactive_p):
    """use_policy_active_masks=False: the stored active masks (30 % zeros in the second case) must be ignored."""
    _assert_all(_G().check_gradients(dict(CAT200, over=dict(use_policy_active_masks=False)), inactive_p=inactive_p), tol=TOL)


@pytest.mark.parametrize("i", [3, 4], ids=["cat200", "cat512"])
def test_get_actions(i):
    res = _G().check_get_actions(SPECS[i])
    assert res["mode_mismatch"] == 0.0 and res["unavailable_action_sampled_count"] == 0.0, res
    _assert_all(res, tol=TOL)


def _cat129_batch(M=160, n_edge=64):
    """Rows 0..n_edge-1 have exactly ONE available action: index 128 (the only logit of the second group) in the first half,
    index 0 in the second; the other rows the usual 25 % masking."""
    G = _G()
    from harl_amd.synthetic import Shapes, make_buffers
    spec = SPECS[1]
    sh = Shapes(T=M, N=1, A=1, obs_dim=spec["obs_dim"], share_obs_dim=spec["share_obs_dim"], act_dim=129, discrete=True,
                hidden_sizes=spec["hidden_sizes"])
    d = make_buffers(sh, 71, unavailable_p=0.25)
    actor, sd, args = G._mk_actor(sh, 4711)
    cfg = G.O.PathConfig.from_reference_dicts({}, args, args)
    obs = d.obs[0][:-1].reshape(M, -1)
    act = d.actions[0].reshape(M, 1).copy()
    avail = d.available_actions[0][:-1].reshape(M, -1).copy()
    only = np.where(np.arange(n_edge) < n_edge // 2, 128, 0)
    avail[:n_edge] = 0.0
    avail[np.arange(n_edge), only] = 1.0
    act[:n_edge, 0] = only
    return G, actor, sd, cfg, obs, act, avail


def test_rows_with_a_single_available_action():
    n_edge = 64
    G, actor, sd, cfg, obs, act, avail = _cat129_batch(n_edge=n_edge)
    M = obs.shape[0]
    from tests.helpers import rel_err, vec_rel_err
    # the edge rows on their own: the distribution is a point mass -> log-prob 0, entropy 0
    lp, ent, dist = actor.evaluate_actions(obs[:n_edge], None, act[:n_edge], None, avail[:n_edge], None)
    torch.cuda.synchronize()
    assert float(lp.abs().max()) <= 1e-6 and abs(float(ent)) <= 1e-6, (float(lp.abs().max()), float(ent))
    assert float(dist.entropy().abs().max()) <= 1e-6
    # the remaining rows against the oracle
    oracle = G.O.OracleHAPPO({k: torch.from_numpy(v) for k, v in sd.items()}, cfg)
    with torch.no_grad():
        ref, ent_ref, _ = oracle.evaluate_actions(obs[n_edge:], act[n_edge:], avail[n_edge:], None)
        ref_all, _, _ = oracle.evaluate_actions(obs, act, avail, None)
    got, ent, _ = actor.evaluate_actions(obs[n_edge:], None, act[n_edge:], None, avail[n_edge:], None)
    torch.cuda.synchronize()
    assert vec_rel_err(got.cpu().numpy(), ref.numpy()) < TOL and rel_err(ent.item(), float(ent_ref)) < TOL
    # one update over all rows: finite, and the oracle's gradient
    rng = np.random.default_rng(3)
    old_logp = (ref_all.numpy() + 0.15 * rng.standard_normal((M, 1))).astype(np.float32)
    adv = rng.standard_normal((M, 1)).astype(np.float32)
    factor = (1 + 0.2 * rng.standard_normal((M, 1))).astype(np.float32)
    active = np.ones((M, 1), np.float32)
    pl, ent_o, gn, imp, g = oracle.update((obs, act, active, old_logp, adv, avail, factor), keep_grad=True)
    taps = []
    actor._grad_tap = lambda gr, sc: taps.append(gr.clone())
    res = actor.update((obs, np.zeros((M, 1, 1), np.float32), act, None, active, old_logp, adv, avail, factor))
    torch.cuda.synchronize()
    gg = taps[0].cpu().numpy()
    assert np.isfinite(gg).all() and all(np.isfinite(r.item()) for r in res)
    out = dict(actor_grad_vec_rel=vec_rel_err(gg, g), actor_loss_rel=rel_err(res[0].item(), pl.item()),
               actor_entropy_rel=rel_err(res[1].item(), ent_o.item()), actor_gradnorm_rel=rel_err(res[2].item(), float(gn)),
               actor_param_after_vec_rel=vec_rel_err(actor.actor.flat_param.cpu().numpy(), oracle.net.flat()))
    print({k: f"{v:.2e}" for k, v in out.items()})
    _assert_all(out, tol=TOL)


def _one_update(G, spec, M, seed=7):
    """(actor, sample) of one HAPPO.update at ``spec`` on synthetic rows."""
    from harl_amd.synthetic import Shapes, make_buffers
    sh = Shapes(T=M, N=1, A=1, obs_dim=spec["obs_dim"], share_obs_dim=spec["share_obs_dim"], act_dim=spec["act_dim"], discrete=True,
                hidden_sizes=spec["hidden_sizes"])
    d = make_buffers(sh, seed, inactive_p=0.2, unavailable_p=0.25)
    actor, _, _ = G._mk_actor(sh, seed + 1)
    rng = np.random.default_rng(seed)
    sample = (d.obs[0][:-1].reshape(M, -1), np.zeros((M, 1, 1), np.float32), d.actions[0].reshape(M, 1), None,
              d.active_masks[0][:-1].reshape(M, 1), d.action_log_probs[0].reshape(M, 1), rng.standard_normal((M, 1)).astype(np.float32),
              d.available_actions[0][:-1].reshape(M, -1), (1 + 0.2 * rng.standard_normal((M, 1))).astype(np.float32))
    return actor, sample


@pytest.mark.parametrize("i,M", [(1, 77), (3, 100)], ids=["cat129_sp64_tail", "cat200_sp128_tail"])
def test_padding_logits_and_tail_samples_get_zero_gradient(i, M):
    """After update() the gradient images hold exactly 0 in the rows of the last group that lie past n (padding of the folded
    weight block) and in every sample past M of the last slab; the real entries are not all zero."""
    G = _G()
    spec = SPECS[i]
    n = spec["act_dim"]
    actor, sample = _one_update(G, spec, M)
    actor.update(sample)
    torch.cuda.synchronize()
    net = actor.actor
    ns = (M + 31) // 32
    for g, (img, sp) in enumerate(zip(net.md_z, net._md_sp)):
        rows = G._atl_rows(img[:ns * 32 * sp], ns, sp)
        cnt = min(128, n - 128 * g)
        assert float(rows[:M, :cnt].abs().max()) > 0.0
        if cnt < sp:
            assert float(rows[:, cnt:].abs().max()) == 0.0, (g, cnt, sp)
        assert float(rows[M:].abs().max()) == 0.0, g


def test_gru_policy_update():
    spec = dict(name="rnn_cat130_L5_m40", obs_dim=30, share_obs_dim=20, act_dim=130, discrete=True, hidden_sizes=[64], L=5, m=40)
    res = _G().check_rnn_update(spec)
    print({k: (f"{v:.2e}" if isinstance(v, float) else v) for k, v in res.items()})
    _assert_all(res, tol=TOL)


# Whole train() against the oracle.  check_baseline_shape builds its case from the HAPPO fixture's configuration and runs the
# heterogeneous-agent trainer; for HAA2C and shared-parameter MAPPO the case gets what those need (a2c_epoch; ONE parameter set
# in every agent slot) and the oracle's MAPPO trainer stands in -- same buffers, same bars.
TRAIN_SHAPES = {
    "cat150_happo_mb2": dict(shapes=dict(T=12, N=8, A=2, obs_dim=18, share_obs_dim=54, act_dim=150, discrete=True,
                                         hidden_sizes=[128, 128]), seed=11, unavailable_p=0.25,
                             overrides=dict(ppo_epoch=1, critic_epoch=1, actor_num_mini_batch=2)),
    "cat100_mappo_shared": dict(shapes=dict(T=12, N=8, A=2, obs_dim=18, share_obs_dim=54, act_dim=100, discrete=True,
                                            hidden_sizes=[64, 64]), seed=12, unavailable_p=0.25, algo="mappo",
                                overrides=dict(ppo_epoch=1, critic_epoch=1, share_param=True)),
    "cat70_haa2c": dict(shapes=dict(T=12, N=8, A=2, obs_dim=18, share_obs_dim=54, act_dim=70, discrete=True,
                                    hidden_sizes=[128, 64]), seed=13, unavailable_p=0.25, algo="haa2c",
                        overrides=dict(ppo_epoch=1, critic_epoch=1, a2c_epoch=1)),
}


@pytest.mark.parametrize("name", list(TRAIN_SHAPES))
def test_whole_train_matches_oracle(name, monkeypatch):
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
    res = G.check_baseline_shape(name)
    print({k: (f"{v:.2e}" if isinstance(v, float) else v) for k, v in res.items()})
    _assert_all(res, tol=TOL)


def test_update_is_deterministic():
    """The same update() twice from the same state: bit-identical gradient arena and loss scalars."""
    G = _G()
    actor, sample = _one_update(G, CAT200, 1500, seed=23)
    net, opt = actor.actor, actor.actor_optimizer
    state = (net.flat_param.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.step_count)
    runs = []
    for _ in range(2):
        with torch.no_grad():
            net.flat_param.copy_(state[0])
        opt.exp_avg.copy_(state[1])
        opt.exp_avg_sq.copy_(state[2])
        opt.step_count = state[3]
        net.invalidate_caches()
        taps = []
        actor._grad_tap = lambda gr, sc: taps.append(sc.clone())
        actor.update(sample)
        torch.cuda.synchronize()
        runs.append((net.flat_grad.clone(), taps[0], net.flat_param.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])
    assert float(runs[0][0].abs().max()) > 0.0


def _atl_image(rows: torch.Tensor, sp: int) -> torch.Tensor:
    """rows [ns * 32, sp] -> the ATL(sp) image (inverse of gpu_checks._atl_rows)."""
    ns = rows.shape[0] // 32
    q = torch.arange(sp // 8)
    feat = (32 * (q // 4) + 8 * (q % 4)).reshape(-1, 1, 1) + 4 * torch.arange(2).reshape(1, -1, 1) + torch.arange(4).reshape(1, 1, -1)
    r = rows.reshape(ns, 32, sp)[:, :, feat.reshape(-1)].reshape(ns, 32, sp // 8, 2, 4).permute(0, 2, 3, 1, 4)
    return r.contiguous().reshape(-1)


@pytest.mark.parametrize("n", [129, 200], ids=["n129_scalar_mask_loads", "n200_vector_mask_loads"])
def test_logp_entry_point_outputs_and_row_gather(n):
    """harl_cat_head_logp on hand-made images: log-probs, per-row entropy, normalised logits and the factor product against
    torch's float64 log_softmax, with actions / availability gathered through a row index, a tail slab, and GARBAGE (not 0)
    in the padding rows of the last image -- they must not be read into the softmax."""
    import ctypes as C
    from harl_amd import _lib
    from tests.helpers import vec_rel_err
    dev = _G().DEV
    M, rows_total = 77, 100
    g = torch.Generator().manual_seed(n)
    logits = 2.0 * torch.randn(M, n, generator=g)
    idx = torch.randperm(rows_total, generator=g)[:M]
    avail = (torch.rand(rows_total, n, generator=g) >= 0.25).float()
    actions = torch.randint(0, n, (rows_total, 1), generator=g).float()
    avail.scatter_(1, actions.long(), 1.0)
    old_logp = -5.0 + 0.1 * torch.randn(M, generator=g)
    factor0 = 1.0 + 0.2 * torch.randn(M, generator=g)
    ns = (M + 31) // 32
    sps = [128] * (n // 128) + ([64 if n % 128 <= 64 else 128] if n % 128 else [])
    imgs = []
    for gi, sp in enumerate(sps):
        blk = torch.full((ns * 32, sp), 7.0)                       # padding rows and tail samples: garbage
        cnt = min(128, n - 128 * gi)
        blk[:M, :cnt] = logits[:, 128 * gi:128 * gi + cnt]
        imgs.append(_atl_image(blk, sp).to(dev))
    zs = (C.c_void_p * len(sps))(*[t.data_ptr() for t in imgs])
    d = lambda t: t.to(dev).contiguous()  # noqa: E731
    idx_d, avail_d, act_d, old_d, fac_d = d(idx), d(avail), d(actions), d(old_logp), d(factor0)
    logp, ent, head = (torch.full((M,), 9.0, device=dev), torch.full((M,), 9.0, device=dev), torch.full((M, n), 9.0, device=dev))
    _lib.call("harl_cat_head_logp", zs, len(sps), (C.c_int * len(sps))(*sps), n, M, idx_d.data_ptr(), act_d.data_ptr(),
              avail_d.data_ptr(), logp.data_ptr(), ent.data_ptr(), old_d.data_ptr(), fac_d.data_ptr(), head.data_ptr(), 0, 0,
              _lib.stream())
    torch.cuda.synchronize()
    z = torch.where(avail[idx] == 0, torch.tensor(-1e10), logits).double()   # the fp32 value -1e10, as the reference sets it
    ref = torch.log_softmax(z, -1)
    ref_lp = ref.gather(1, actions[idx].long()).reshape(M)
    ref_ent = -(ref.clamp(min=torch.finfo(torch.float32).min) * ref.exp()).sum(-1)
    on = avail[idx] != 0
    res = dict(logp_vec_rel=vec_rel_err(logp.cpu().numpy(), ref_lp.numpy()), entropy_vec_rel=vec_rel_err(ent.cpu().numpy(), ref_ent.numpy()),
               head_out_available_vec_rel=vec_rel_err(head.cpu()[on].numpy(), ref[on].numpy()),
               head_out_masked_vec_rel=vec_rel_err(head.cpu()[~on].numpy(), ref[~on].numpy()),
               factor_vec_rel=vec_rel_err(fac_d.cpu().numpy(), (factor0.double() * torch.exp(ref_lp - old_logp.double())).numpy()))
    print({k: f"{v:.2e}" for k, v in res.items()})
    _assert_all(res, tol=TOL)
