"""HATRPO on Discrete(33..64) heads on a 256-wide last layer (HARL_HEAD64_256=1 and HARL_TRPO_HEAD64_256=1) on the GPU:
harl_actor_head_fvp at H = 256 (k_head256_fvp, csrc/head256.hip) against float64 on the same fp32 inputs, then the whole path
against the oracle.  Without the feature the kernel test stops at the call's -2, the others at the constructor."""
import numpy as np
import pytest
import torch

from harl_amd._lib import call, ptr, stream
from tests import gpu_checks as G
from tests.helpers import vec_rel_err
from tests.test_gpu_head64_256 import SPECS
from tests.test_gpu_mixed_256 import _check, _f32, _image

pytestmark = pytest.mark.gpu
H = 256


@pytest.fixture(autouse=True)
def switches(monkeypatch):
    for v in ("HARL_HEAD64_256", "HARL_TRPO_HEAD64_256", "HARL_MIXED_256", "HARL_TRPO_MIXED_256"):
        monkeypatch.setenv(v, "1")


# 33: the first output in the second accumulator tile, a partial last slab in one workgroup; 64: no padding columns, two
# workgroups; 513: a one-row tail slab
@pytest.mark.parametrize("masked", [False, True], ids=["all_available", "avail25"])
@pytest.mark.parametrize("D,M", [(33, 77), (64, 200), (48, 513)])
def test_head_fvp_against_float64(D, M, masked):
    rng = np.random.default_rng(7 * D + M + masked)
    ns = (M + 31) // 32
    mp = 32 * ns
    x, xd, rstd = _f32(rng.standard_normal((mp, H))), _f32(rng.standard_normal((mp, H))), _f32(rng.random((mp, 1)) + 0.5)
    W, Wd = _f32(rng.standard_normal((D, H)) / 16.0), _f32(rng.standard_normal((D, H)) / 16.0)
    b, bd = _f32(0.1 * rng.standard_normal(D)), _f32(0.1 * rng.standard_normal(D))
    mask = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, ns * (H // 64) * 64).astype(np.int32)).to(G.DEV)
    av = np.ones((M, D))
    if masked:  # 25 % of the entries unavailable; every row keeps one available action
        av = (rng.random((M, D)) >= 0.25).astype(np.float64)
        av[np.arange(M), rng.integers(0, D, M)] = 1.0
    un = av != 0
    # the Categorical KL Hessian on the normalised logits over ALL D entries, masked ones at -1e10 (trpo_util.py:132-158)
    z = np.where(un, x[:M] @ W.T + b, -1e10)
    zd = x[:M] @ Wd.T + xd[:M] @ W.T + bd
    pr = np.exp(z - z.max(-1, keepdims=True))
    pr /= pr.sum(-1, keepdims=True)
    S = (pr * zd * un).sum(-1, keepdims=True)
    sum_dq = (zd * un).sum(-1, keepdims=True) - D * S
    dzh = np.where(un, (zd - S) - pr * sum_dq, 0.0)
    dx = dzh @ W
    want = G._relu_mask_rows(mask, ns, H).numpy()[:M] * rstd[:M] * (dx - dx.mean(-1, keepdims=True) - x[:M] * (dx * x[:M]).mean(-1, keepdims=True))

    dz, dhead = torch.full((mp * H,), float("nan"), device=G.DEV), torch.full((mp * 64,), float("nan"), device=G.DEV)
    xi, xdi = _image(x), _image(xd)
    Wv, bv, Wdv, bdv, rs = G.dev(W), G.dev(b), G.dev(Wd), G.dev(bd), G.dev(rstd.reshape(-1))
    avd = G.dev(av) if masked else None
    call("harl_actor_head_fvp", ptr(xi), ptr(xdi), ptr(mask), ptr(rs), M, H, ptr(Wv), ptr(bv), ptr(Wdv), ptr(bdv), None, 1.0, 0.5, 1, D,
         ptr(avd), 0, 0, ptr(dz), ptr(dhead), stream())
    torch.cuda.synchronize()
    dh = G._atl_rows(dhead, ns, 64).numpy()
    assert float(np.abs(dh[:, D:]).max(initial=0.0)) == 0.0 and float(np.abs(dh[M:]).max(initial=0.0)) == 0.0
    _check(dict(dzL_vec_rel=vec_rel_err(G._atl_rows(dz, ns, H)[:M].numpy(), want), dhead_vec_rel=vec_rel_err(dh[:M, :D], dzh)))


CAT = [s for s in SPECS if s["name"] in ("cat33_256", "cat64_256", "cat48_128_256")]


@pytest.mark.parametrize("spec", CAT, ids=[s["name"] for s in CAT])
def test_gradient_fvp_and_update_match_oracle(spec):
    """Surrogate gradient (mode 1 of k_head256) and Fisher-vector product at the flat 1e-5; what follows the CG solve (with the
    KL's normalised logits from head_out) at check_trpo's own bars."""
    _check(G.check_trpo(spec))


def test_whole_train_matches_oracle(monkeypatch):
    """HATRPO, two agents and the V critic: within max(1e-5, 2 x the oracle's own measured fp32 uncertainty)."""
    monkeypatch.setitem(G.BASELINE_SHAPES, "cat40_256_hatrpo", dict(
        shapes=dict(T=12, N=8, A=2, obs_dim=18, share_obs_dim=54, act_dim=40, discrete=True, hidden_sizes=[256, 256]), seed=11,
        algo="hatrpo", unavailable_p=0.25, overrides=dict(critic_epoch=1)))
    _check(G.check_baseline_shape("cat40_256_hatrpo"))
