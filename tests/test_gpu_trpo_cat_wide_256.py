"""HATRPO on Categorical heads of 65..512 actions on trunks that hold a 256-wide layer (HARL_TRPO_CAT_WIDE_256=1) on the GPU:
harl_mlp_rect_tangent_groups (csrc/rect.hip) against float64 on the same fp32 inputs, then the whole path against the oracle."""
import ctypes as C

import numpy as np
import pytest
import torch

from harl_amd._lib import call, ptr, stream
from tests import gpu_checks as G
from tests.helpers import vec_rel_err
from tests.test_gpu_cat_wide_256 import FWD, PAD, SPECS, _packs, _ptrs
from tests.test_gpu_mixed_256 import _check, _f32, _image

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def switches(monkeypatch):
    for v in ("HARL_CAT_WIDE_256", "HARL_TRPO_CAT_WIDE", "HARL_TRPO_CAT_WIDE_256", "HARL_MIXED_256", "HARL_TRPO_MIXED_256"):
        monkeypatch.setenv(v, "1")


@pytest.mark.parametrize("KP,sps,M", FWD, ids=[f"{k}to{'_'.join(map(str, s))}_M{m}" for k, s, m in FWD])
def test_tangent_groups_against_float64(KP, sps, M):
    """The forward's cases (tests/test_gpu_cat_wide_256.py).  The padding rows of a pack are zero in BOTH matrices: b'_dot."""
    rng = np.random.default_rng(KP + 7 * sum(sps) + M + 1)
    ns = (M + 31) // 32
    x, xd = _f32(rng.standard_normal((ns * 32, KP))), _f32(rng.standard_normal((ns * 32, KP)))
    (Ws, Wdev), (Wds, Wddev) = _packs(rng, sps, KP), _packs(rng, sps, KP)
    bds = [_f32(0.1 * rng.standard_normal(sp)) for sp in sps]
    xi, xdi, bdev = _image(x), _image(xd), [G.dev(b) for b in bds]
    zd = [torch.full((ns * 32 * sp,), float("nan"), device=G.DEV) for sp in sps]
    call("harl_mlp_rect_tangent_groups", ptr(xdi), ptr(xi), M, KP, len(sps), (C.c_int * len(sps))(*sps), _ptrs(Wdev), _ptrs(Wddev),
         _ptrs(bdev), _ptrs(zd), stream())
    torch.cuda.synchronize()
    res = {}
    for g, (W, Wd, bd, sp) in enumerate(zip(Ws, Wds, bds, sps)):
        got = G._atl_rows(zd[g], ns, sp)[:M].numpy()
        res[f"zd{g}_vec_rel"] = vec_rel_err(got, x[:M] @ Wd.T + bd + xd[:M] @ W.T)
        res[f"zd{g}_padding_not_bias_count"] = float((got[:, -PAD:] != bd[-PAD:]).sum())
    _check(res)


@pytest.mark.parametrize("spec", SPECS, ids=[s["name"] for s in SPECS])
def test_gradient_fvp_and_update_match_oracle(spec):
    _check(G.check_trpo(spec))  # gradient and Fisher-vector product at the flat 1e-5, behind the CG solve check_trpo's own bars


def test_whole_train_matches_oracle(monkeypatch):
    """HATRPO, two agents and the V critic, 25 % of the actions unavailable: max(1e-5, 2 x the oracle's own fp32 uncertainty)."""
    name = "cat150_256_256_hatrpo"
    monkeypatch.setitem(G.BASELINE_SHAPES, name, dict(
        shapes=dict(T=12, N=8, A=2, obs_dim=18, share_obs_dim=54, act_dim=150, discrete=True, hidden_sizes=[256, 256]), seed=11,
        algo="hatrpo", unavailable_p=0.25, overrides=dict(critic_epoch=1)))
    _check(G.check_baseline_shape(name))
