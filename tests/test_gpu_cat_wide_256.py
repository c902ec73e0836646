"""Categorical heads of 65..512 actions on trunks that hold a 256-wide layer (HARL_CAT_WIDE_256=1; csrc/rect.hip) on the GPU: the two
grouped entry points against float64 on the same fp32 inputs at M = 33 (a second slab with one live row) and 65 569 rows (513
workgroup iterations, dead waves), then the whole path against the oracle with the 1e-5 bar of tests/test_gpu_parity.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from harl_amd._lib import call, ptr, stream
from tests import gpu_checks as G
from tests.helpers import vec_rel_err
from tests.test_gpu_mixed_256 import _check, _f32, _image

pytestmark = pytest.mark.gpu
PAD = 5  # rows at the end of every pack that hold zero weights, as past the last action of a head


@pytest.fixture(autouse=True)
def switches(monkeypatch):
    monkeypatch.setenv("HARL_CAT_WIDE_256", "1")
    monkeypatch.setenv("HARL_MIXED_256", "1")


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _packs(rng, sps, K):
    Ws = [_f32(rng.standard_normal((sp, K)) / np.sqrt(K)) * (np.arange(sp) < sp - PAD)[:, None] for sp in sps]
    return Ws, [G.dev(W) for W in Ws]


FWD = [(256, [128], 33), (256, [128, 64], 33), (256, [128] * 4, 33), (64, [128, 64], 33), (128, [128, 128, 64], 33),
       (256, [128, 128, 64], 65569)]


@pytest.mark.parametrize("KP,sps,M", FWD, ids=[f"{k}to{'_'.join(map(str, s))}_M{m}" for k, s, m in FWD])
def test_linear_groups_against_float64(KP, sps, M):
    """Every group's image; the padding rows of a pack (zero weights) hold the bias and nothing else.  Rows past M: noise in."""
    rng = np.random.default_rng(KP + 7 * sum(sps) + M)
    ns = (M + 31) // 32
    x = _f32(rng.standard_normal((ns * 32, KP)))
    (Ws, Wd), bs = _packs(rng, sps, KP), [_f32(0.1 * rng.standard_normal(sp)) for sp in sps]
    xi, bd = _image(x), [G.dev(b) for b in bs]
    z = [torch.full((ns * 32 * sp,), float("nan"), device=G.DEV) for sp in sps]
    call("harl_mlp_rect_linear_groups", ptr(xi), M, KP, len(sps), (C.c_int * len(sps))(*sps), _ptrs(Wd), _ptrs(bd), _ptrs(z), stream())
    torch.cuda.synchronize()
    res = {}
    for g, (W, b, sp) in enumerate(zip(Ws, bs, sps)):
        got = G._atl_rows(z[g], ns, sp)[:M].numpy()
        res[f"z{g}_vec_rel"] = vec_rel_err(got, x[:M] @ W.T + b)
        res[f"z{g}_padding_not_bias_count"] = float((got[:, -PAD:] != b[-PAD:]).sum())
    _check(res)


BWD = [([128], 256, 33), ([128, 64], 256, 33), ([128] * 4, 256, 33), ([128, 64], 64, 33), ([128, 128, 64], 128, 33),
       ([128, 128], 256, 65569)]


@pytest.mark.parametrize("sps,HI,M", BWD, ids=[f"{'_'.join(map(str, s))}to{h}_M{m}" for s, h, m in BWD])
def test_bwd_groups_against_float64(sps, HI, M):
    """The sum over the groups, then the LayerNorm backward, then the mask.  dz is 0 past M: dz_prev must be exactly 0 there."""
    rng = np.random.default_rng(HI + 7 * sum(sps) + M)
    ns = (M + 31) // 32
    mp = ns * 32
    Ws, Wd = _packs(rng, sps, HI)
    xh, rstd = _f32(rng.standard_normal((mp, HI))), _f32(rng.random((mp, 1)) + 0.5)
    dzs = [np.zeros((mp, sp)) for sp in sps]
    for dz in dzs:
        dz[:M] = _f32(rng.standard_normal((M, dz.shape[1])))
    mask = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, ns * (HI // 64) * 64).astype(np.int32)).to(G.DEV)
    dzp = torch.full((mp * HI,), float("nan"), device=G.DEV)
    dzi, xhi, rsd = [_image(dz) for dz in dzs], _image(xh), G.dev(rstd.reshape(-1))
    call("harl_mlp_rect_bwd_groups", _ptrs(dzi), len(sps), (C.c_int * len(sps))(*sps), _ptrs(Wd), ptr(xhi), ptr(mask), ptr(rsd), M, HI,
         ptr(dzp), stream())
    torch.cuda.synchronize()
    dxh = sum(dz @ W for dz, W in zip(dzs, Ws))
    da = rstd * (dxh - dxh.mean(-1, keepdims=True) - xh * (dxh * xh).mean(-1, keepdims=True))
    want = np.where(G._relu_mask_rows(mask, ns, HI).numpy(), da, 0.0)
    got = G._atl_rows(dzp, ns, HI).numpy()
    _check(dict(dz_prev_vec_rel=vec_rel_err(got[:M], want[:M]), tail_rows_nonzero_count=float((got[M:] != 0.0).sum())))


SPECS = [
    dict(name="cat65_256_256", obs_dim=18, share_obs_dim=54, act_dim=65, discrete=True, hidden_sizes=[256, 256], M=77),
    dict(name="cat192_128_256", obs_dim=40, share_obs_dim=33, act_dim=192, discrete=True, hidden_sizes=[128, 256], M=513),
    dict(name="cat300_256_128", obs_dim=31, share_obs_dim=65, act_dim=300, discrete=True, hidden_sizes=[256, 128], M=300),
    dict(name="cat512_256x3", obs_dim=77, share_obs_dim=70, act_dim=512, discrete=True, hidden_sizes=[256, 256, 256], M=640),
]


@pytest.mark.parametrize("spec", SPECS, ids=[s["name"] for s in SPECS])
@pytest.mark.parametrize("check", ["check_forward", "check_gradients"])
def test_whole_path_matches_oracle(check, spec):
    _check(getattr(G, check)(spec))


def test_get_actions():
    res = G.check_get_actions(SPECS[2])
    assert res["mode_mismatch"] == 0.0 and res["unavailable_action_sampled_count"] == 0.0, res
    _check(res)


def test_whole_train_matches_oracle(monkeypatch):
    """HAPPO, two agents and the V critic, two minibatches, 25 % of the actions unavailable."""
    name = "cat150_256_256_happo_mb2"
    monkeypatch.setitem(G.BASELINE_SHAPES, name, dict(
        shapes=dict(T=12, N=8, A=2, obs_dim=18, share_obs_dim=54, act_dim=150, discrete=True, hidden_sizes=[256, 256]), seed=11,
        unavailable_p=0.25, overrides=dict(ppo_epoch=1, critic_epoch=1, actor_num_mini_batch=2)))
    _check(G.check_baseline_shape(name))
