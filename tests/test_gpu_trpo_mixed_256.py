"""HATRPO on trunks that mix 256-wide layers with 64- / 128-wide ones (HARL_MIXED_256=1 and HARL_TRPO_MIXED_256=1) on the GPU:
harl_mlp_rect_tangent (k_panel_rect<MT, 2>, csrc/rect.hip) against float64 on the same fp32 inputs, then the whole path against the
oracle.  Without the feature the kernel test stops at the missing symbol, the others at the constructor's NotImplementedError."""
import numpy as np
import pytest
import torch

from harl_amd._lib import call, ptr, stream
from tests import gpu_checks as G
from tests.helpers import vec_rel_err
from tests.test_gpu_mixed_256 import M_LARGE, M_SMALL, SPECS, _check, _f32, _image

pytestmark = pytest.mark.gpu
# (KP, D, HO, hidden, M).  MT = HO / 32 row tiles, a panel is 8 / MT sub-panels of 32 columns: 64 -> 64 is ONE panel that holds
# both operands; 256 -> 64 2 + 2 panels; 64 -> 128 one panel per operand; HO = 256 runs two buffers; the first layers end in a
# short panel and have no second operand; 256 -> 256 is what tools/kbench.py times next to harl_mlp_panel_tangent.
TANGENT = [(64, 64, 64, True, M_SMALL), (256, 256, 64, True, M_SMALL), (256, 256, 128, True, M_SMALL),
           (64, 64, 128, True, M_SMALL), (128, 128, 256, True, M_SMALL), (64, 64, 256, True, M_SMALL), (96, 77, 128, False, M_SMALL),
           (32, 18, 64, False, M_SMALL), (256, 256, 256, True, M_SMALL), (256, 256, 128, True, M_LARGE)]


@pytest.fixture(autouse=True)
def trpo_mixed(monkeypatch):
    monkeypatch.setenv("HARL_MIXED_256", "1")
    monkeypatch.setenv("HARL_TRPO_MIXED_256", "1")


@pytest.mark.parametrize("KP,D,HO,hidden,M", TANGENT, ids=[f"{'h' if hid else 'first'}{d}to{h}_M{m}" for _, d, h, hid, m in TANGENT])
def test_rect_tangent_against_float64(KP, D, HO, hidden, M):
    """The three lines of the layer's tangent in float64; random mask words; columns D..KP of a first layer's image hold noise."""
    rng = np.random.default_rng(KP + 3 * HO + M + hidden)
    ns, mp = (M + 31) // 32, 32 * ((M + 31) // 32)
    Wd, bd = _f32(rng.standard_normal((HO, D)) / np.sqrt(D)), _f32(0.1 * rng.standard_normal(HO))
    x, xh, rstd = _f32(rng.standard_normal((mp, KP))), _f32(rng.standard_normal((mp, HO))), _f32(rng.random((mp, 1)) + 0.5)
    mask = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, ns * (HO // 64) * 64).astype(np.int32)).to(G.DEV)
    W, xd = (_f32(rng.standard_normal((HO, D)) / np.sqrt(D)), _f32(rng.standard_normal((mp, D)))) if hidden else (None, None)
    a = np.where(G._relu_mask_rows(mask, ns, HO).numpy(), x[:, :D] @ Wd.T + bd + (xd @ W.T if hidden else 0.0), 0.0)
    want = rstd * (a - a.mean(-1, keepdims=True) - xh * (a * xh).mean(-1, keepdims=True))
    out = torch.full((mp * HO,), float("nan"), device=G.DEV)
    xi, Wdd, bdd, xhi, rsd = _image(x), G.dev(Wd), G.dev(bd), _image(xh), G.dev(rstd.reshape(-1))
    xdi, Wdev = (_image(xd), G.dev(W)) if hidden else (None, None)
    call("harl_mlp_rect_tangent", ptr(xdi), ptr(xi), M, KP, HO, ptr(Wdev), ptr(Wdd), D, ptr(bdd), ptr(xhi), ptr(mask), ptr(rsd),
         ptr(out), stream())
    torch.cuda.synchronize()
    _check(dict(xout_dot_vec_rel=vec_rel_err(G._atl_rows(out, ns, HO)[:M].numpy(), want[:M])))


@pytest.mark.parametrize("spec", SPECS, ids=[s["name"] for s in SPECS])
def test_gradient_fvp_and_update_match_oracle(spec):
    """Surrogate gradient and Fisher-vector product at the flat 1e-5; what follows the CG solve at check_trpo's own bars."""
    _check(G.check_trpo(spec))


def test_whole_train_matches_oracle(monkeypatch):
    """HATRPO, two agents and the (mixed) V critic: within max(1e-5, 2 x the oracle's own measured fp32 uncertainty)."""
    monkeypatch.setitem(G.BASELINE_SHAPES, "mixed_256_128_hatrpo", dict(
        shapes=dict(T=12, N=8, A=2, obs_dim=18, share_obs_dim=54, act_dim=5, discrete=False, hidden_sizes=[256, 128]), seed=11,
        algo="hatrpo", overrides=dict(critic_epoch=1)))
    _check(G.check_baseline_shape("mixed_256_128_hatrpo"))
