"""Trunks that mix 256-wide layers with 64- / 128-wide ones (HARL_MIXED_256=1; k_panel_rect, csrc/rect.hip) on the GPU: the two
entry points against a float64 restatement of the layer (Linear, ReLU, LayerNorm without affine, eps 1e-5, and its backward) on
the same fp32 inputs, then the whole path against the oracle with the checks and the 1e-5 bar of tests/test_gpu_parity.py.
Without the feature the kernel tests stop at the missing symbol and the others at the constructor's NotImplementedError."""
import numpy as np
import pytest
import torch

from harl_amd._lib import call, ptr, stream
from tests import gpu_checks as G
from tests.helpers import vec_rel_err
from tests.test_gpu_cat_wide import _atl_image
from tests.test_gpu_parity import TOL, _assert_all

pytestmark = pytest.mark.gpu

# A workgroup iteration is 4 slabs of 32 rows; the grid cap is 512 workgroups at 2 / 4 row tiles, 256 at 8 (launch_rect,
# csrc/rect.hip).  65 569 rows = 513 iterations: a second one for workgroup 0 under either cap (32 901 rows only reach it at
# 256), and two dead waves in the last.
M_SMALL, M_LARGE = 33, 65569


@pytest.fixture(autouse=True)
def mixed(monkeypatch):
    monkeypatch.setenv("HARL_MIXED_256", "1")


def _check(res):
    print({k: (f"{v:.2e}" if isinstance(v, float) else v) for k, v in res.items()})
    _assert_all(res, tol=TOL)


def _f32(a):
    return a.astype(np.float32).astype(np.float64)


def _image(rows: np.ndarray) -> torch.Tensor:
    return _atl_image(torch.from_numpy(rows.astype(np.float32)), rows.shape[1]).to(G.DEV)


def _dw(a_img, ha, b_img, k, M):
    """harl_mlp_dw_partials of the two ATL images, its rows summed in float64: (dW [ha, k], db [ha])."""
    n_wg = max(1, min(512, ((M + 31) // 32 + 1) // 2))
    part = torch.full((n_wg * (ha * k + ha),), float("nan"), device=G.DEV)
    call("harl_mlp_dw_partials", ptr(a_img), 0, 0, ha, ptr(b_img), 0, 0, None, None, None, k, M, ptr(part), n_wg, stream())
    torch.cuda.synchronize()
    s = part.reshape(n_wg, -1).double().sum(0).cpu().numpy()
    return s[:ha * k].reshape(ha, k), s[ha * k:]


FWD = [(256, 256, 64, M_SMALL), (256, 256, 128, M_SMALL), (96, 77, 128, M_SMALL), (32, 18, 64, M_SMALL), (256, 256, 128, M_LARGE)]


@pytest.mark.parametrize("KP,D,HO,M", FWD, ids=[f"{k}to{h}_M{m}" for k, _, h, m in FWD])
def test_rect_fwd_against_float64(KP, D, HO, M):
    """Mask bits exactly (no pre-activation drawn within 1e-4 of 0).  Columns D..KP and rows past M of the input image hold noise,
    as in an x0n image.  M = 33: the next layer's weight gradient (its dz 0 past M, as the loss kernels leave it) sees 33 rows."""
    rng = np.random.default_rng(KP + HO + M)
    ns = (M + 31) // 32
    mp = ns * 32
    W, b = _f32(rng.standard_normal((HO, D)) / np.sqrt(D)), _f32(0.1 * rng.standard_normal(HO))
    x = _f32(rng.standard_normal((mp + mp // 8 + 64, KP)))
    x = x[np.abs(x[:, :D] @ W.T + b).min(-1) > 1e-4][:mp]
    assert x.shape[0] == mp
    z = x[:M, :D] @ W.T + b
    c = np.maximum(z, 0.0) - np.maximum(z, 0.0).mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt((c * c).mean(-1, keepdims=True) + 1e-5)
    xout = torch.full((mp * HO,), float("nan"), device=G.DEV)
    mask = torch.zeros(ns * (HO // 64) * 64, dtype=torch.int32, device=G.DEV)
    rs = torch.full((mp,), float("nan"), device=G.DEV)
    xi, Wd, bd = _image(x), G.dev(W), G.dev(b)
    call("harl_mlp_rect_fwd", ptr(xi), M, KP, ptr(Wd), D, ptr(bd), HO, ptr(xout), ptr(mask), ptr(rs), stream())
    torch.cuda.synchronize()
    res = dict(xhat_vec_rel=vec_rel_err(G._atl_rows(xout, ns, HO)[:M].numpy(), c * rstd),
               rstd_vec_rel=vec_rel_err(rs.cpu().numpy()[:M], rstd[:, 0]),
               mask_mismatch=float((G._relu_mask_rows(mask, ns, HO)[:M].numpy() != (z > 0)).sum()))
    if M == M_SMALL:
        dz = np.zeros((mp, 64))
        dz[:M] = _f32(rng.standard_normal((M, 64)))
        dW, db = _dw(_image(dz), 64, xout, HO, M)
        res.update(dw_next_vec_rel=vec_rel_err(dW, dz[:M].T @ (c * rstd)), db_next_vec_rel=vec_rel_err(db, dz[:M].sum(0)))
    _check(res)


BWD = [(64, 256, M_SMALL), (128, 256, M_SMALL), (256, 128, M_SMALL), (256, 64, M_SMALL), (128, 256, M_LARGE)]


@pytest.mark.parametrize("HO,HI,M", BWD, ids=[f"{o}to{i}_M{m}" for o, i, m in BWD])
def test_rect_bwd_against_float64(HO, HI, M):
    """dz is 0 past M: dz_prev must be exactly 0 there, and at M = 33 the weight gradient formed from it is the one over 33 rows."""
    rng = np.random.default_rng(HO + 3 * HI + M)
    ns = (M + 31) // 32
    mp = ns * 32
    W, xh, rstd = _f32(rng.standard_normal((HO, HI)) / np.sqrt(HO)), _f32(rng.standard_normal((mp, HI))), _f32(rng.random((mp, 1)) + 0.5)
    dz = np.zeros((mp, HO))
    dz[:M] = _f32(rng.standard_normal((M, HO)))
    mask = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, ns * (HI // 64) * 64).astype(np.int32)).to(G.DEV)
    dzp = torch.full((mp * HI,), float("nan"), device=G.DEV)
    dzi, xhi, rsd, Wd = _image(dz), _image(xh), G.dev(rstd.reshape(-1)), G.dev(W)
    call("harl_mlp_rect_bwd", ptr(dzi), ptr(xhi), ptr(mask), ptr(rsd), M, HO, HI, ptr(Wd), ptr(dzp), stream())
    torch.cuda.synchronize()
    dxh = dz @ W
    da = rstd * (dxh - dxh.mean(-1, keepdims=True) - xh * (dxh * xh).mean(-1, keepdims=True))
    want = np.where(G._relu_mask_rows(mask, ns, HI).numpy(), da, 0.0)
    got = G._atl_rows(dzp, ns, HI).numpy()
    res = dict(dz_prev_vec_rel=vec_rel_err(got[:M], want[:M]), tail_rows_nonzero_count=float((got[M:] != 0.0).sum()))
    if M == M_SMALL:
        xb = _f32(rng.standard_normal((mp, 64)))
        dW, db = _dw(dzp, HI, _image(xb), 64, M)
        res.update(dw_prev_vec_rel=vec_rel_err(dW, want[:M].T @ xb[:M]), db_prev_vec_rel=vec_rel_err(db, want[:M].sum(0)))
    _check(res)


SPECS = [
    dict(name="256_128_box5", obs_dim=18, share_obs_dim=54, act_dim=5, discrete=False, hidden_sizes=[256, 128], M=77),
    dict(name="128_256_disc14", obs_dim=40, share_obs_dim=33, act_dim=14, discrete=True, hidden_sizes=[128, 256], M=513),
    dict(name="64_256_64_box20", obs_dim=77, share_obs_dim=70, act_dim=20, discrete=False, hidden_sizes=[64, 256, 64], M=640),
    dict(name="256_64_128_disc33", obs_dim=31, share_obs_dim=65, act_dim=33, discrete=True, hidden_sizes=[256, 64, 128], M=300),
]


@pytest.mark.parametrize("spec", SPECS, ids=[s["name"] for s in SPECS])
@pytest.mark.parametrize("check", ["check_forward", "check_gradients"])
def test_whole_path_matches_oracle(check, spec):
    _check(getattr(G, check)(spec))


def test_whole_train_matches_oracle(monkeypatch):
    """HAPPO, two agents and the V critic, two minibatches: within max(1e-5, 2 x the oracle's own measured fp32 uncertainty)."""
    name = "mixed_256_128_happo_mb2"
    monkeypatch.setitem(G.BASELINE_SHAPES, name, dict(
        shapes=dict(T=12, N=8, A=2, obs_dim=18, share_obs_dim=54, act_dim=5, discrete=False, hidden_sizes=[256, 128]), seed=11,
        overrides=dict(ppo_epoch=1, critic_epoch=1, actor_num_mini_batch=2)))
    _check(G.check_baseline_shape(name))
