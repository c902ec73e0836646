"""Plain action heads of 33..64 outputs on a 256-wide last layer (HARL_HEAD64_256=1: k_head256, csrc/head256.hip) against the
oracle on the GPU, with the checks and the 1e-5 bar of tests/test_gpu_parity.py: 33 = the first output in the second accumulator
tile, 64 = no padding columns; M = 77 a partial last slab inside one workgroup, 200 two workgroups with a partial last slab, 513 a
one-row tail slab.  box40_256_128 is the Gaussian head on a 128-wide last layer above a 256: the lifted "panel" refusal without
the new kernel.  check_gradients runs every Categorical spec with 25 % of the actions unavailable.  Without the switch the
Categorical all-256 specs fail at their first launch and the others at the constructor."""
import pytest
import torch

from tests import gpu_checks as G
from tests.test_gpu_gauss_wide import _hip_sample, _one_update, _restore, _show
from tests.test_gpu_parity import TOL, _assert_all

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def switches(monkeypatch):
    for v in ("HARL_HEAD64_256", "HARL_GAUSS_WIDE", "HARL_MIXED_256"):
        monkeypatch.setenv(v, "1")


SPECS = [
    dict(name="cat33_256", obs_dim=18, share_obs_dim=54, act_dim=33, discrete=True, hidden_sizes=[256, 256], M=77),
    dict(name="cat64_256", obs_dim=40, share_obs_dim=33, act_dim=64, discrete=True, hidden_sizes=[256, 256], M=200),
    dict(name="cat48_128_256", obs_dim=31, share_obs_dim=65, act_dim=48, discrete=True, hidden_sizes=[128, 256], M=513),
    dict(name="box33_256", obs_dim=18, share_obs_dim=54, act_dim=33, discrete=False, hidden_sizes=[256, 256], M=77),
    dict(name="box64_256", obs_dim=40, share_obs_dim=33, act_dim=64, discrete=False, hidden_sizes=[256, 256], M=200),
    dict(name="box40_256_128", obs_dim=31, share_obs_dim=65, act_dim=40, discrete=False, hidden_sizes=[256, 128], M=300),
]
BOX33, BOX64 = SPECS[3], SPECS[4]


@pytest.mark.parametrize("check", ["check_forward", "check_gradients"])
@pytest.mark.parametrize("spec", SPECS, ids=[s["name"] for s in SPECS])
def test_matches_oracle(spec, check):
    _assert_all(_show(getattr(G, check)(spec)), tol=TOL)


@pytest.mark.parametrize("spec", [SPECS[1], BOX64], ids=["cat64_256", "box64_256"])
def test_gradients_mean_aggregation_with_inactive_agents(spec):
    _assert_all(_show(G.check_gradients(spec, agg="mean", inactive_p=0.3)), tol=TOL)


def test_box_padding_and_tail_get_zero_gradient():
    """After update() at M = 77 the ATL(64) dhead image holds exactly 0 in the columns past act_dim and in samples 77..95 of the last
    slab, the real entries are not all zero, and part_ls / ls_sum hold exactly 0 past act_dim."""
    M, n = 77, BOX33["act_dim"]
    actor, _, _, s = _one_update(G, BOX33, M)
    actor.update(_hip_sample(s))
    torch.cuda.synchronize()
    net = actor.actor
    rows = G._atl_rows(net.dhead[:96 * 64], 3, 64)
    assert float(rows[:M, :n].abs().max()) > 0.0
    assert float(rows[:, n:].abs().max()) == 0.0 and float(rows[M:].abs().max()) == 0.0
    assert float(net.part_ls.reshape(-1, 64)[:, n:].abs().max()) == 0.0 and float(net.ls_sum[n:].abs().max()) == 0.0
    assert float(net.ls_sum[:n].abs().min()) > 0.0


def test_cat_padding_and_tail_get_zero_gradient():
    """The same image for Discrete(33) at M = 77: uniform random actions, stored log-probs around log(1 / 33)."""
    import numpy as np
    from harl_amd.synthetic import Shapes
    M, n = 77, 33
    sh = Shapes(T=M, N=1, A=1, obs_dim=18, share_obs_dim=54, act_dim=n, discrete=True, hidden_sizes=[256, 256])
    actor, _, _ = G._mk_actor(sh, 8)
    rng = np.random.default_rng(3)
    f = lambda *shape: rng.standard_normal(shape).astype(np.float32)  # noqa: E731
    act = rng.integers(0, n, (M, 1)).astype(np.float32)
    actor.update((f(M, 18), np.zeros((M, 1, 1), np.float32), act, None, np.ones((M, 1), np.float32),
                  -np.log(n) + 0.15 * f(M, 1), f(M, 1), None, 1 + 0.2 * f(M, 1)))
    torch.cuda.synchronize()
    rows = G._atl_rows(actor.actor.dhead[:96 * 64], 3, 64)
    assert float(rows[:M, :n].abs().max()) > 0.0
    assert float(rows[:, n:].abs().max()) == 0.0 and float(rows[M:].abs().max()) == 0.0


def test_update_is_deterministic():
    """The same update() twice from the same state: bit-identical gradient arena, loss scalars, log_std sums and parameters."""
    actor, _, _, s = _one_update(G, BOX64, 200, seed=23)
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


TRAIN = {
    "cat40_256_happo_mb2": dict(shapes=dict(T=12, N=8, A=2, obs_dim=18, share_obs_dim=54, act_dim=40, discrete=True,
                                            hidden_sizes=[256, 256]), seed=11, unavailable_p=0.25,
                                overrides=dict(ppo_epoch=1, critic_epoch=1, actor_num_mini_batch=2)),
    "box33_256_haa2c": dict(shapes=dict(T=12, N=8, A=2, obs_dim=18, share_obs_dim=54, act_dim=33, discrete=False,
                                        hidden_sizes=[256, 256]), seed=13, algo="haa2c",
                            overrides=dict(ppo_epoch=1, critic_epoch=1, a2c_epoch=1)),
}


@pytest.mark.parametrize("name", list(TRAIN))
def test_whole_train_matches_oracle(name, monkeypatch):
    from tests import helpers as H

    class Case(H.SyntheticCase):  # (haa2c's epoch count, as tests/test_gpu_gauss_wide.py sets it)
        def __init__(self, nm, shapes, seed, algo_name="happo", overrides=None, **kw):
            super().__init__(nm, shapes, seed, algo_name=algo_name, overrides=overrides, **kw)
            if algo_name == "haa2c":
                self.algo["a2c_epoch"] = (overrides or {}).get("a2c_epoch", 1)

    monkeypatch.setattr(H, "SyntheticCase", Case)
    monkeypatch.setitem(G.BASELINE_SHAPES, name, TRAIN[name])
    _assert_all(_show(G.check_baseline_shape(name)), tol=TOL)
