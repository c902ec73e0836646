"""-m gpu: harl_mlp_bwd_dx_dw's eight-wave kernel (k_bwd_dx_dw8, the default build) against the four-wave kernel it replaced
(k_bwd_dx_dw, a library built with -DHARL_BWD_SPLIT_WAVES=0) on the same inputs.

The two run the same slab-to-wave assignment and the same MFMA and reduction order per wave, so every output is expected to be
bit-identical: dz_prev and the per-workgroup partial rows of dW' | db' and dW_1' | db_1' (including the rows the kernel clears),
for both variants (KT = 1: fused first-layer gradient; KT = 0: dz_prev stored) and both filler settings, at ragged and small
shapes.  A second launch of the new kernel must give the same bits."""
import ctypes as C
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

H, KP = 128, 32
ROW2, ROW1 = H * H + H, H * KP + H
VARIANT = "bwd4w"

# (M, n_wg): fewer slabs than the four owner waves; a ragged last slab with a slab count that is not a multiple of 4 x grid
# and n_wg < 256; several super-rounds on the full grid with a ragged tail; n_wg > 256 (rows 256.. of the arenas cleared)
CASES = [(70, 4), (32 * 4 * 7 * 3 + 32 * 5 + 17, 7), (32 * 4 * 256 * 2 + 32 * 37 + 5, 256), (32 * 4 * 300 + 32 * 3, 300)]


@pytest.fixture(scope="module")
def libs():
    from harl_amd import _build, _lib
    extra = {k: list(v) for k, v in _build.EXTRA_FLAGS.items()}
    extra["mlp.hip"] = extra.get("mlp.hip", []) + ["-DHARL_BWD_SPLIT_WAVES=0"]
    path = _build.build(variant=VARIANT, extra=extra)
    old = C.CDLL(path)
    fn_old = old.harl_mlp_bwd_dx_dw
    fn_old.argtypes = _lib.SIGNATURES["harl_mlp_bwd_dx_dw"]
    fn_old.restype = C.c_int
    fn_new = _lib.load().harl_mlp_bwd_dx_dw
    assert os.path.realpath(path) != os.path.realpath(_lib.LIB_PATH)
    return fn_new, fn_old


def _inputs(M, seed):
    dev = torch.device("cuda:0")
    ns = (M + 31) // 32
    mp = ns * 32
    g = torch.Generator(device=dev).manual_seed(seed)
    rn = lambda *sh: torch.randn(*sh, device=dev, generator=g)  # noqa: E731
    dz, xh, x0n = rn(mp * H), rn(mp * H), rn(mp * KP)
    mask = torch.randint(-2 ** 31, 2 ** 31 - 1, (ns * 2 * 64,), device=dev, dtype=torch.int32, generator=g)
    rstd = torch.rand(mp, device=dev, generator=g) + 0.5
    W = rn(H * H) * 0.1
    return dz, xh, x0n, mask, rstd, W, mp


def _run(fn, M, n_wg, first, fill, with_dzp, ins):
    from harl_amd._lib import ptr, stream
    dz, xh, x0n, mask, rstd, W, mp = ins
    dev = dz.device
    nan = float("nan")
    dzp = torch.full((mp * H,), nan, device=dev) if with_dzp else None
    part2 = torch.full((n_wg * ROW2,), nan, device=dev)
    part1 = torch.full((n_wg * ROW1,), nan, device=dev) if first else None
    rc = fn(ptr(dz), ptr(xh), ptr(mask), ptr(rstd), M, H, H, ptr(W), ptr(dzp), ptr(x0n) if first else None, KP if first else 0,
            ptr(part1), ptr(part2), n_wg, fill, stream())
    assert rc == 0
    torch.cuda.synchronize()
    return {k: v for k, v in (("dz_prev", dzp), ("dw2_part", part2), ("dw1_part", part1)) if v is not None}


def _bits_differ(a, b):
    return int((a.view(torch.int32) != b.view(torch.int32)).sum().item())


@pytest.mark.parametrize("first", [True, False], ids=["kt1", "kt0"])
@pytest.mark.parametrize("fill", [1, 0])
@pytest.mark.parametrize("M,n_wg", CASES)
def test_split_waves_bit_identical(libs, M, n_wg, first, fill):
    fn_new, fn_old = libs
    ins = _inputs(M, seed=M + 17 * fill + (5 if first else 0))
    with_dzp = (not first) or fill == 1  # KT = 1 with and without the optional dz_prev store
    new = _run(fn_new, M, n_wg, first, fill, with_dzp, ins)
    old = _run(fn_old, M, n_wg, first, fill, with_dzp, ins)
    again = _run(fn_new, M, n_wg, first, fill, with_dzp, ins)
    assert sorted(new) == sorted(old)
    for k in new:
        assert not torch.isnan(new[k]).any(), k
        assert _bits_differ(new[k], old[k]) == 0, k
        assert _bits_differ(new[k], again[k]) == 0, k
