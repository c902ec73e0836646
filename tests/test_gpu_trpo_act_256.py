"""HARL_TRPO_ACT_256=1 next to HARL_ACT_256=1 on the GPU: harl_mlp_rect_act_tangent (k_panel_rect<MT, 2, ACT>, csrc/rect.hip) against
float64 on the same fp32 inputs, then HATRPO's whole path against the oracle, at the bars of tests/test_gpu_trpo_mixed_256.py."""
import numpy as np
import pytest
import torch

from harl_amd._lib import call, ptr, stream
from harl_amd.nets import ACT_IDS
from tests import gpu_checks as G
from tests.helpers import vec_rel_err
from tests.test_gpu_act_256 import ACTS, SLOPE, VALUE, WHOLE, _layer
from tests.test_gpu_mixed_256 import M_LARGE, M_SMALL, _check, _f32, _image

pytestmark = pytest.mark.gpu
# (act, KP, D, HO, hidden, M).  HO = 256 runs two LDS buffers, 256 -> 64 is 2 + 2 panels, 64 -> 128 one panel per operand; the first
# layers have no second operand and end in a short panel (77 of 96 columns) or are two one-sub-panel panels (into 256)
TANGENT = ([(a, k, k, h, True, M_SMALL) for k, h in ((256, 256), (256, 64), (128, 256), (64, 128)) for a in ACTS]
           + [(a, k, d, h, False, M_SMALL) for k, d, h in ((96, 77, 128), (64, 40, 256)) for a in ACTS[1::2]]  # ([1::2]: tanh, selu)
           + [("tanh", 256, 256, 128, True, M_LARGE)])


@pytest.fixture(autouse=True)
def switches(monkeypatch):
    for v in ("HARL_ACT_256", "HARL_TRPO_ACT_256", "HARL_MIXED_256", "HARL_TRPO_MIXED_256"):
        monkeypatch.setenv(v, "1")


@pytest.mark.parametrize("act,KP,D,HO,hidden,M", TANGENT, ids=[f"{a}_{'h' if hid else 'first'}{d}to{h}_M{m}" for a, _, d, h, hid, m in TANGENT])
def test_rect_act_tangent_against_float64(act, KP, D, HO, hidden, M):
    """The record is a float64 forward rounded to fp32.  leaky_relu / selu: the slope jumps at a = 0, pre-activations whose value is
    within 1e-4 of it are moved to 0.5 (every row stays).  Columns D..KP of a first layer's image hold noise."""
    rng = np.random.default_rng(KP + 3 * HO + M + hidden + ACT_IDS[act])
    ns, mp = (M + 31) // 32, 32 * ((M + 31) // 32)
    Wd, bd, x = _f32(rng.standard_normal((HO, D)) / np.sqrt(D)), _f32(0.1 * rng.standard_normal(HO)), _f32(rng.standard_normal((mp, KP)))
    W, xd = (_f32(rng.standard_normal((HO, D)) / np.sqrt(D)), _f32(rng.standard_normal((mp, D)))) if hidden else (None, None)
    z = rng.standard_normal((mp, HO))
    z[np.abs(VALUE[act](z)) < 1e-4] = 0.5
    xh, mean, rstd = (_f32(t) for t in _layer(act, z))
    ad = SLOPE[act](xh / rstd + mean) * (x[:, :D] @ Wd.T + bd + (xd @ W.T if hidden else 0.0))
    want = rstd * (ad - ad.mean(-1, keepdims=True) - xh * (ad * xh).mean(-1, keepdims=True))
    out = torch.full((mp * HO,), float("nan"), device=G.DEV)
    xi, Wdd, bdd, xhi, mud, rsd = _image(x), G.dev(Wd), G.dev(bd), _image(xh), G.dev(mean.reshape(-1)), G.dev(rstd.reshape(-1))
    xdi, Wdev = (_image(xd), G.dev(W)) if hidden else (None, None)
    call("harl_mlp_rect_act_tangent", ptr(xdi), ptr(xi), M, KP, HO, ptr(Wdev), ptr(Wdd), D, ptr(bdd), ACT_IDS[act], ptr(xhi), ptr(mud),
         ptr(rsd), ptr(out), stream())
    torch.cuda.synchronize()
    _check(dict(xout_dot_vec_rel=vec_rel_err(G._atl_rows(out, ns, HO)[:M].numpy(), want[:M])))


@pytest.mark.parametrize("hs,disc,n,obs,M,act", WHOLE, ids=[f"{w[0]}_{w[5]}" for w in WHOLE])
def test_gradient_fvp_and_update_match_oracle(hs, disc, n, obs, M, act):
    _check(G.check_trpo(dict(name=f"{hs}_{act}", obs_dim=obs, share_obs_dim=54, act_dim=n, discrete=disc, hidden_sizes=hs, M=M,
                             over=dict(activation_func=act))))


def test_whole_train_matches_oracle(monkeypatch):
    monkeypatch.setitem(G.BASELINE_SHAPES, "act_256_128_tanh_hatrpo", dict(
        shapes=dict(T=12, N=8, A=2, obs_dim=18, share_obs_dim=54, act_dim=5, discrete=False, hidden_sizes=[256, 128]), seed=11,
        algo="hatrpo", overrides=dict(critic_epoch=1, activation_func="tanh")))
    _check(G.check_baseline_shape("act_256_128_tanh_hatrpo"))
