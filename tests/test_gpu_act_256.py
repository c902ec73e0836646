"""HARL_ACT_256=1 (k_panel_rect<MT, MODE, ACT>, csrc/rect.hip): the two entry points against a float64 restatement of the layer
(Linear, activation, LayerNorm without affine, eps 1e-5; backward with the slope from the fp32 record) on the same fp32 inputs,
then the whole path against the oracle; the 1e-5 bar of tests/test_gpu_parity.py, the shapes of tests/test_gpu_mixed_256.py."""
import numpy as np
import pytest
import torch

from harl_amd._lib import call, ptr, stream
from harl_amd.nets import ACT_IDS
from tests import gpu_checks as G
from tests.helpers import vec_rel_err
from tests.test_gpu_mixed_256 import M_LARGE, M_SMALL, _check, _dw, _f32, _image

pytestmark = pytest.mark.gpu
ACTS = ["leaky_relu", "tanh", "sigmoid", "selu"]
SCALE, ALPHA = 1.0507009873554804934193349852946, 1.6732632423543772848170429916717
VALUE = {"leaky_relu": lambda z: np.where(z > 0, z, 0.01 * z), "tanh": np.tanh, "sigmoid": lambda z: 1.0 / (1.0 + np.exp(-z)),
         "selu": lambda z: SCALE * np.where(z > 0, z, ALPHA * np.expm1(np.minimum(z, 0.0)))}
SLOPE = {"leaky_relu": lambda a: np.where(a > 0, 1.0, 0.01), "tanh": lambda a: 1.0 - a * a, "sigmoid": lambda a: a * (1.0 - a),
         "selu": lambda a: np.where(a > 0, SCALE, a + SCALE * ALPHA)}
FWD = [(a, *s, M_SMALL) for s in [(256, 256, 64), (256, 256, 128), (128, 128, 256), (96, 77, 128)] for a in ACTS] + [("tanh", 256, 256, 256, M_LARGE)]
WHOLE = [(hs, disc, n, obs, M, a) for hs, disc, n, obs, M, acts in (([256, 256], False, 5, 18, 77, ACTS), ([256, 128], True, 14, 40, 513, ACTS[1::2]),
                                                                     ([128, 256], False, 5, 18, 77, ACTS[1::2])) for a in acts]  # ([1::2]: tanh, selu)


@pytest.fixture(autouse=True)
def switches(monkeypatch):
    monkeypatch.setenv("HARL_ACT_256", "1")
    monkeypatch.setenv("HARL_MIXED_256", "1")


def _layer(act, z):  # float64 (x_hat, mean, rstd) of LayerNorm(act(z)), the last two as columns
    a = VALUE[act](z)
    mean = a.mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(((a - mean) ** 2).mean(-1, keepdims=True) + 1e-5)
    return (a - mean) * rstd, mean, rstd


@pytest.mark.parametrize("act,KP,D,HO,M", FWD, ids=[f"{a}_{k}to{h}_M{m}" for a, k, _, h, m in FWD])
def test_rect_act_fwd_against_float64(act, KP, D, HO, M):
    rng, ns = np.random.default_rng(KP + HO + M), (M + 31) // 32
    mp = ns * 32
    # (columns D..KP and rows past M of the input image hold noise, as in an x0n image)
    W, b, x = _f32(rng.standard_normal((HO, D)) / np.sqrt(D)), _f32(0.1 * rng.standard_normal(HO)), _f32(rng.standard_normal((mp, KP)))
    xhat, mean, rstd = _layer(act, x[:M, :D] @ W.T + b)
    xout, mu, rs = (torch.full((n,), float("nan"), device=G.DEV) for n in (mp * HO, mp, mp))
    xi, Wd, bd = _image(x), G.dev(W), G.dev(b)
    call("harl_mlp_rect_act_fwd", ptr(xi), M, KP, ptr(Wd), D, ptr(bd), HO, ACT_IDS[act], ptr(xout), ptr(mu), ptr(rs), stream())
    torch.cuda.synchronize()
    _check(dict(xhat_vec_rel=vec_rel_err(G._atl_rows(xout, ns, HO)[:M].numpy(), xhat),
                mean_vec_rel=vec_rel_err(mu.cpu().numpy()[:M], mean[:, 0]), rstd_vec_rel=vec_rel_err(rs.cpu().numpy()[:M], rstd[:, 0])))


@pytest.mark.parametrize("HO,HI", [(64, 256), (256, 128), (256, 64), (256, 256)])
@pytest.mark.parametrize("act", ACTS)
def test_rect_act_bwd_against_float64(act, HO, HI):
    """The record below is a float64 forward rounded to fp32.  leaky_relu / selu: the slope jumps at a = 0, pre-activations whose
    value is within 1e-4 of it are moved to 0.5 (every row stays).  dz is 0 past M: dz_prev must be exactly 0 there."""
    M, rng = M_SMALL, np.random.default_rng(HO + 3 * HI + ACT_IDS[act])
    ns = (M + 31) // 32
    mp = ns * 32
    W, z, dz = _f32(rng.standard_normal((HO, HI)) / np.sqrt(HO)), rng.standard_normal((mp, HI)), np.zeros((mp, HO))
    z[np.abs(VALUE[act](z)) < 1e-4] = 0.5
    xh, mean, rstd = (_f32(t) for t in _layer(act, z))
    dz[:M] = _f32(rng.standard_normal((M, HO)))
    dzp = torch.full((mp * HI,), float("nan"), device=G.DEV)
    dzi, xhi, mud, rsd, Wd = _image(dz), _image(xh), G.dev(mean.reshape(-1)), G.dev(rstd.reshape(-1)), G.dev(W)
    call("harl_mlp_rect_act_bwd", ptr(dzi), ptr(xhi), ptr(mud), ptr(rsd), M, HO, HI, ACT_IDS[act], ptr(Wd), ptr(dzp), stream())
    torch.cuda.synchronize()
    dxh = dz @ W
    want = SLOPE[act](xh / rstd + mean) * rstd * (dxh - dxh.mean(-1, keepdims=True) - xh * (dxh * xh).mean(-1, keepdims=True))
    got, xb = G._atl_rows(dzp, ns, HI).numpy(), _f32(rng.standard_normal((mp, 64)))
    dW, db = _dw(dzp, HI, _image(xb), 64, M)
    _check(dict(dz_prev_vec_rel=vec_rel_err(got[:M], want[:M]), tail_rows_nonzero_count=float((got[M:] != 0.0).sum()),
                dw_prev_vec_rel=vec_rel_err(dW, want[:M].T @ xb[:M]), db_prev_vec_rel=vec_rel_err(db, want[:M].sum(0))))


@pytest.mark.parametrize("hs,disc,n,obs,M,act", WHOLE, ids=[f"{w[0]}_{w[5]}" for w in WHOLE])
def test_whole_path_matches_oracle(hs, disc, n, obs, M, act):
    spec = dict(name=f"{hs}_{act}", obs_dim=obs, share_obs_dim=54, act_dim=n, discrete=disc, hidden_sizes=hs, M=M, over=dict(activation_func=act))
    _check(G.check_forward(spec))
    _check(G.check_gradients(spec))


def test_whole_train_matches_oracle(monkeypatch):
    monkeypatch.setitem(G.BASELINE_SHAPES, "act_256_128_tanh", dict(
        shapes=dict(T=12, N=8, A=2, obs_dim=18, share_obs_dim=54, act_dim=5, discrete=False, hidden_sizes=[256, 128]), seed=11,
        overrides=dict(ppo_epoch=1, critic_epoch=1, actor_num_mini_batch=2, activation_func="tanh")))
    _check(G.check_baseline_shape("act_256_128_tanh"))
