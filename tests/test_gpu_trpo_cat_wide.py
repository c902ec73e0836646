"""HATRPO on Categorical action heads of 65..512 actions (HARL_TRPO_CAT_WIDE=1; csrc/cathead.hip: harl_cat_head_loss mode 1,
harl_cat_head_fvp, harl_cat_kl_sum) against the oracle on the GPU: the checks, helpers and bars of the <= 64-way heads
(gpu_checks.check_trpo / check_trpo_rnn: gradient and Fisher-vector product at the flat 1e-5, everything behind the conjugate-
gradient solve at max(1e-5, 2 x the oracle's own measured uncertainty)), at the smallest shapes that reach every group layout."""
import numpy as np
import pytest
import torch

from tests.test_gpu_parity import TOL, _assert_all

pytestmark = pytest.mark.gpu

TRPO = dict(kl_threshold=0.01, ls_step=10, accept_ratio=0.5, backtrack_coeff=0.8)
SPECS = [
    # one ATL(128) group with 63 padding rows, a tail slab
    dict(name="cat65_h64", obs_dim=18, share_obs_dim=54, act_dim=65, discrete=True, hidden_sizes=[64, 64], M=77),
    # a one-logit ATL(64) second group, several workgroups
    dict(name="cat129_h128", obs_dim=40, share_obs_dim=33, act_dim=129, discrete=True, hidden_sizes=[128, 128], M=513),
    # wide first layer, padding rows in an ATL(128) tail group
    dict(name="cat200_64_128", obs_dim=90, share_obs_dim=70, act_dim=200, discrete=True, hidden_sizes=[64, 128], M=300),
    # four full groups
    dict(name="cat512_h128", obs_dim=18, share_obs_dim=54, act_dim=512, discrete=True, hidden_sizes=[128, 128], M=513),
]
RNN_SPEC = dict(name="rnn_cat130_L5_m40", obs_dim=30, share_obs_dim=20, act_dim=130, discrete=True, hidden_sizes=[64], L=5, m=40)


def _G():
    from tests import gpu_checks
    return gpu_checks


@pytest.fixture(autouse=True)
def _switch_on(monkeypatch):
    monkeypatch.setenv("HARL_TRPO_CAT_WIDE", "1")


def _show(res):
    print({k: (f"{v:.2e}" if isinstance(v, float) else v) for k, v in res.items()})


@pytest.mark.parametrize("i", range(len(SPECS)), ids=[s["name"] for s in SPECS])
def test_gradient_fvp_and_update_match_oracle(i):
    res = _G().check_trpo(SPECS[i])
    _show(res)
    _assert_all(res, tol=TOL)


def test_gru_policy_gradient_fvp_and_update_match_oracle():
    """m = 40 pads to 64 sequences: m_valid / m_pad in the loss, the Fisher-vector product and the head-output pass."""
    res = _G().check_trpo_rnn(RNN_SPEC)
    _show(res)
    _assert_all(res, tol=TOL)


def _trpo_actor(spec, M, n_edge, edge_actions, seed=7):
    """HATRPO actor at ``spec`` + M synthetic rows with 25 % masking; rows 0..n_edge-1 have exactly ONE available action,
    cycling through ``edge_actions``."""
    G = _G()
    from harl_amd.hatrpo import HATRPO
    from harl_amd.synthetic import Shapes, actor_param_shapes, make_buffers, synthetic_state_dict
    n = spec["act_dim"]
    sh = Shapes(T=M, N=1, A=1, obs_dim=spec["obs_dim"], share_obs_dim=spec["share_obs_dim"], act_dim=n, discrete=True,
                hidden_sizes=spec["hidden_sizes"])
    args = G.default_args(sh.hidden_sizes, **TRPO)
    actor = HATRPO(args, G.Box((sh.obs_dim,)), G.Discrete(n), device=G.DEV)
    sd = synthetic_state_dict(actor_param_shapes(sh, args["use_feature_normalization"]), seed + 1, args["std_x_coef"])
    actor.actor.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    d = make_buffers(sh, seed, inactive_p=0.2, unavailable_p=0.25)
    obs = d.obs[0][:-1].reshape(M, -1)
    act = d.actions[0].reshape(M, 1).copy()
    avail = d.available_actions[0][:-1].reshape(M, -1).copy()
    only = np.asarray(edge_actions)[np.arange(n_edge) % len(edge_actions)]
    avail[:n_edge] = 0.0
    avail[np.arange(n_edge), only] = 1.0
    act[:n_edge, 0] = only
    rng = np.random.default_rng(seed)
    rows = dict(obs=obs, act=act, avail=avail, old_logp=d.action_log_probs[0].reshape(M, 1),
                adv=rng.standard_normal(M).astype(np.float32), factor=(1 + 0.2 * rng.standard_normal(M)).astype(np.float32),
                active=d.active_masks[0][:-1].reshape(M))
    return actor, rows, only


@pytest.mark.parametrize("i,M", [(1, 77), (2, 100)], ids=["cat129_sp64_tail", "cat200_sp128_tail"])
def test_fvp_images_zero_pattern(i, M):
    """After one _fvp the logits images (what md_backward reads) hold exactly 0 in the rows of the last group past n, in every
    sample past M of the last slab and at every unavailable action; the other entries are finite and not all zero.

    Rows with a SINGLE available action a (p a point mass): every masked entry is exactly 0, the available one is NOT -- the
    Fisher matrix of kl_approx spans all n entries (trpo_util.py:47-51), a masked entry's q = -1e10 - lse moves with lse = z_a, so
    q_dot_masked = -z_dot_a, sum_dq = -(n - 1) z_dot_a and out_a = (z_dot_a - S) - p_a sum_dq = (n - 1) z_dot_a.  That is the
    arithmetic of k_actor_head_fvp and of the oracle's double backward (the parity tests above hold it to 1e-5); the test holds
    the entry to that value at the flat 1e-5, from the tangent images the kernel read."""
    G = _G()
    spec = SPECS[i]
    n = spec["act_dim"]
    n_edge = 16
    actor, r, only = _trpo_actor(spec, M, n_edge, edge_actions=(n - 1, 0, 128, 127))
    net = actor.actor
    dv = G.dev
    d_obs, d_avail = dv(r["obs"]), dv(r["avail"])
    net.fold()
    actor._surrogate(d_obs, M, dv(r["act"]), d_avail, dv(r["old_logp"]), dv(r["adv"]), None, dv(r["factor"]), dv(r["active"]),
                     want_grad=True)
    v = torch.from_numpy(np.random.default_rng(5).standard_normal(net.n_params).astype(np.float32)).to(G.DEV)
    out = actor._fvp(d_obs, M, M, d_avail, v)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    ns = (M + 31) // 32
    avail = torch.from_numpy(r["avail"])
    zd_a, zd_b = actor._tangent_ws["cat_zd"]
    for g, (img, sp) in enumerate(zip(net.md_z, net._md_sp)):
        rows = G._atl_rows(img[:ns * 32 * sp], ns, sp).cpu()
        zdot = (G._atl_rows(zd_a[g][:ns * 32 * sp], ns, sp) + G._atl_rows(zd_b[g][:ns * 32 * sp], ns, sp)).cpu()
        cnt = min(128, n - 128 * g)
        real, av = rows[:M, :cnt], avail[:, 128 * g:128 * g + cnt]
        assert bool(torch.isfinite(rows).all())
        assert float(real[n_edge:].abs().max()) > 0.0
        if cnt < sp:
            assert float(rows[:, cnt:].abs().max()) == 0.0, (g, cnt, sp)
        assert float(rows[M:].abs().max()) == 0.0, g
        assert float(real[av == 0].abs().max()) == 0.0, g
        for row in range(n_edge):  # the single available entry of an edge row, if it lies in this group
            a = int(only[row]) - 128 * g
            if 0 <= a < cnt:
                want = (n - 1) * float(zdot[row, a])
                print(f"edge row {row} action {int(only[row])}: {float(real[row, a]):.6e} want {want:.6e}")
                assert abs(float(real[row, a]) - want) <= TOL * abs(want), (row, g, a)


_KL_CACHE = {}


def _two_heads(n, single: bool):
    """Normalised logits [300, n] of harl_cat_head_logp(head_out=...) at two nearby parameter sets: 25 % masking, or
    (``single``) exactly one available action per row."""
    key = (n, single)
    if key in _KL_CACHE:
        return _KL_CACHE[key]
    G = _G()
    from harl_amd.synthetic import Shapes, make_buffers
    M = 300
    spec = next(s for s in SPECS if s["act_dim"] == n)
    sh = Shapes(T=M, N=1, A=1, obs_dim=spec["obs_dim"], share_obs_dim=spec["share_obs_dim"], act_dim=n, discrete=True,
                hidden_sizes=spec["hidden_sizes"])
    d = make_buffers(sh, 31, unavailable_p=0.25)
    actor, _, _ = G._mk_actor(sh, 32)
    net = actor.actor
    obs, act = G.dev(d.obs[0][:-1].reshape(M, -1)), G.dev(d.actions[0].reshape(M, 1))
    avail = d.available_actions[0][:-1].reshape(M, -1).copy()
    if single:
        avail[:] = 0.0
        avail[np.arange(M), (np.arange(M) * 7) % n] = 1.0
    avail = G.dev(avail)
    heads = []
    for step in range(2):
        if step:
            with torch.no_grad():
                gen = torch.Generator().manual_seed(n)
                net.flat_param.add_((2e-3 * torch.randn(net.n_params, generator=gen)).to(G.DEV))
            net.invalidate_caches()
            net._fold_version = None
            net.fold()
        ho = torch.empty(M, n, dtype=torch.float32, device=G.DEV)
        actor._logp_pass(obs, act, avail, M, None, head_out=ho)
        heads.append(ho)
    torch.cuda.synchronize()
    _KL_CACHE[key] = heads
    return heads


def _kl_kernel(ho, hn, rows, n) -> float:
    from harl_amd import _lib
    acc = torch.zeros(1, dtype=torch.float64, device=ho.device)
    _lib.call("harl_cat_kl_sum", ho.data_ptr(), hn.data_ptr(), rows, n, acc.data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    return float(acc.item())


@pytest.mark.parametrize("n", [129, 512])
def test_kl_sum_entry_point(n):
    """harl_cat_kl_sum per quarter of 300 rows against numpy float64 of the same expression on the same fp32 inputs.  Bar, by the
    suite's noise rule with the reference arithmetic as yardstick: max(1e-5, 2 x the largest relative distance, over the four
    quarters, of torch-CPU fp32's evaluation of that expression from the float64 value)."""
    ho, hn = _two_heads(n, single=False)
    p32, q32 = ho.cpu(), hn.cpu()
    got, ref64, ref32 = [], [], []
    for k in range(4):
        lo, hi = 75 * k, 75 * (k + 1)
        got.append(_kl_kernel(ho[lo:hi], hn[lo:hi], hi - lo, n))
        p, q = p32[lo:hi].numpy().astype(np.float64), q32[lo:hi].numpy().astype(np.float64)
        ref64.append(float(((np.exp(q - p) - 1.0 - q) + p).sum()))
        ref32.append(float(((torch.exp(q32[lo:hi] - p32[lo:hi]) - 1 - q32[lo:hi]) + p32[lo:hi]).sum()))
    noise = max(abs(a - b) / abs(b) for a, b in zip(ref32, ref64))
    errs = [abs(a - b) / abs(b) for a, b in zip(got, ref64)]
    bar = max(1e-5, 2.0 * noise)
    print(dict(n=n, kl_per_row=[f"{b / 75:.3e}" for b in ref64], kernel_rel=[f"{e:.2e}" for e in errs],
               torch_fp32_rel=f"{noise:.2e}", bar=f"{bar:.2e}"))
    assert all(b > 0 for b in ref64)
    assert max(errs) <= bar, (errs, bar)
    # the whole batch in one launch accumulates INTO out_sum
    from harl_amd import _lib
    acc = torch.full((1,), 1.0, dtype=torch.float64, device=ho.device)
    _lib.call("harl_cat_kl_sum", ho.data_ptr(), hn.data_ptr(), 300, n, acc.data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    assert abs(float(acc.item()) - 1.0 - sum(ref64)) <= bar * sum(ref64)


@pytest.mark.parametrize("n", [129, 512])
def test_kl_sum_of_point_masses_is_exactly_zero(n):
    """One available action per row: its normalised logit is exactly 0 under both parameter sets, every masked one exactly
    -1e10, and in the reference's term order each entry contributes exactly 0."""
    ho, hn = _two_heads(n, single=True)
    assert _kl_kernel(ho, hn, 300, n) == 0.0
