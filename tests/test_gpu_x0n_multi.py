"""-m gpu: harl_x0n_multi (csrc/wide.hip: the normalised-input images of several networks in ONE launch) against single
harl_mlp_x0n_wide launches, and the software-pipelined single-problem kernels against a plain torch statement of the image.

The one-launch kernel walks every problem with the walk its single launch takes, so image, mu0 and rstd0 are expected to be
bit-identical (torch.equal on the whole buffers, rows of a partly filled last slab included; the two sides start from different
fill values, so an unwritten element shows).  Shapes: D = 18 (one 32-column block, the contiguous-run walk) and D = 54 (two blocks,
the row-per-load walk); M = 1 and 31 (one partly filled slab: nothing to pipeline), 32 (one full slab), 101 (three full slabs and a
tail) and 1029 (33 slabs: with max_workgroups = 2 every wave walks at least four, so its requests run past the end of its walk
and the last one meets the partly filled slab)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
MS = (1, 31, 32, 101, 1029)


def _kp(D):
    return (D + 31) // 32 * 32


def _bufs(M, D, fill):
    ns = (M + 31) // 32
    return (torch.full((ns * 32 * _kp(D),), fill, device=DEV), torch.full((ns * 32,), fill, device=DEV),
            torch.full((ns * 32,), fill, device=DEV))


def _rows(M, D, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(M, D, device=DEV, generator=g) * 3.0 + 0.5).contiguous()


def _single(X, use_ln0):
    from harl_amd._lib import call, ptr, stream
    M, D = X.shape
    out = _bufs(M, D, 7.0)
    call("harl_mlp_x0n_wide", ptr(X), D, None, M, D, use_ln0, ptr(out[0]), ptr(out[1]), ptr(out[2]), stream())
    torch.cuda.synchronize()
    return out


def _multi(Xs, use_ln0s, max_workgroups=0):
    from harl_amd import _lib
    from harl_amd._lib import ptr
    outs = [_bufs(X.shape[0], X.shape[1], -3.0) for X in Xs]
    probs = [(ptr(X), X.shape[1], X.shape[0], X.shape[1], ln, ptr(o[0]), ptr(o[1]), ptr(o[2])) for X, ln, o in zip(Xs, use_ln0s, outs)]
    assert _lib.x0n_multi(probs, max_workgroups, tag=None)
    torch.cuda.synchronize()
    return outs


def _same(a, b, what):
    for x, y, name in zip(a, b, ("x0n", "mu0", "rstd0")):
        assert torch.equal(x, y), (what, name, int((x != y).sum().item()))


@pytest.fixture(scope="module")
def singles():
    """harl_mlp_x0n_wide of every (D, use_ln0, M), computed once."""
    out = {}
    for D in (18, 54):
        for ln in (0, 1):
            for M in MS:
                X = _rows(M, D, 1000 * D + 10 * M + ln)
                out[(D, ln, M)] = (X, _single(X, ln))
    return out


@pytest.mark.parametrize("D", [18, 54])
@pytest.mark.parametrize("use_ln0", [0, 1])
def test_one_problem_matches_the_single_launch(singles, D, use_ln0):
    for M in MS:
        X, want = singles[(D, use_ln0, M)]
        _same(_multi([X], [use_ln0])[0], want, (D, use_ln0, M))


def test_three_problems_of_different_shapes_in_one_launch(singles):
    keys = [(18, 1, 101), (54, 1, 1029), (18, 0, 31)]
    got = _multi([singles[k][0] for k in keys], [k[1] for k in keys])
    for k, g in zip(keys, got):
        _same(g, singles[k][1], k)
    # ... and with a budget below the number of problems (one workgroup each)
    got = _multi([singles[k][0] for k in keys], [k[1] for k in keys], max_workgroups=2)
    for k, g in zip(keys, got):
        _same(g, singles[k][1], k)


@pytest.mark.parametrize("D", [18, 54])
def test_two_workgroups_walk_several_slabs_per_wave(singles, D):
    X, want = singles[(D, 1, 1029)]  # 33 slabs on 8 waves: 4 or 5 each, the prefetch crosses the end of the data
    got = _multi([X], [1], max_workgroups=2)[0]
    _same(got, want, D)
    _same(_multi([X], [1], max_workgroups=2)[0], got, ("rerun", D))


def test_rerun_is_bit_identical(singles):
    keys = [(54, 1, 1029), (18, 1, 1029), (54, 0, 101)]
    a = _multi([singles[k][0] for k in keys], [k[1] for k in keys])
    b = _multi([singles[k][0] for k in keys], [k[1] for k in keys])
    for k, x, y in zip(keys, a, b):
        _same(x, y, k)


def test_full_width_rows_and_unaligned_rows(singles):
    """D = 32 and D = 64 (no pad column: no ones column either), D = 7 (one 16-byte piece per lane does not fill the wave) and a
    row tensor that starts 4 bytes into an allocation (the 16-byte requests of the pipelined walk do not apply)."""
    Xs = [_rows(70, 32, 1), _rows(65, 64, 2), _rows(133, 7, 3), _rows(97 * 18 + 1, 1, 4).reshape(-1)[1:].reshape(97, 18)]
    assert Xs[3].data_ptr() % 16 == 4
    lns = [1, 1, 1, 1]
    got = _multi(Xs, lns)
    for X, ln, g in zip(Xs, lns, got):
        _same(g, _single(X, ln), tuple(X.shape))


def test_unsupported_problems_are_refused_without_a_launch():
    from harl_amd import _lib
    from harl_amd._lib import ptr
    X = _rows(40, 70, 5)  # wider than 64
    o = _bufs(40, 70, 5.0)
    assert not _lib.x0n_multi([(ptr(X), 70, 40, 70, 1, ptr(o[0]), ptr(o[1]), ptr(o[2]))], tag=None)
    X = _rows(40, 20, 6)
    o = _bufs(40, 18, 5.0)
    assert not _lib.x0n_multi([(ptr(X), 20, 40, 18, 1, ptr(o[0]), ptr(o[1]), ptr(o[2]))], tag=None)  # strided rows (ldx != D)
    assert not _lib.x0n_multi([(ptr(X), 20, 0, 20, 1, ptr(o[0]), ptr(o[1]), ptr(o[2]))], tag=None)   # no rows
    assert not _lib.x0n_multi([], tag=None)
    torch.cuda.synchronize()
    assert all(bool((t == 5.0).all()) for t in o)


def _atl_rows(img, ns, KP):
    """ATL(KP) image -> rows [ns * 32, KP] (csrc/common.h: piece q, lane half h, sample s, element e <-> feature
    32 (q >> 2) + 8 (q & 3) + 4 h + e)."""
    t = img.reshape(ns, KP // 8, 2, 32, 4)
    q = torch.arange(KP // 8, device=img.device)
    feat = ((32 * (q // 4) + 8 * (q % 4)).reshape(-1, 1, 1) + 4 * torch.arange(2, device=img.device).reshape(1, -1, 1)
            + torch.arange(4, device=img.device).reshape(1, 1, -1))
    rows = torch.empty(ns, 32, KP, dtype=img.dtype, device=img.device)
    rows[:, :, feat.reshape(-1)] = t.permute(0, 3, 1, 2, 4).reshape(ns, 32, -1)
    return rows.reshape(ns * 32, KP)


@pytest.mark.parametrize("D", [18, 54])
@pytest.mark.parametrize("use_ln0", [0, 1])
def test_single_launch_image_against_torch(singles, D, use_ln0):
    """The pipelined single-problem kernels: pad columns exactly zero, the last pad column exactly one, use_ln0 = 0 the raw
    rows bit for bit; use_ln0 = 1 the LayerNorm of the rows (no affine) against float64.  Tolerance from the number format: the
    rows are 3 N(0, 1) + 0.5, |x| < 16; an fp32 sum of D <= 54 such terms has partial sums below 54 * 16 and at most D roundings
    of 2^-24 relative each, so the mean is off by at most 54 * 16 * 2^-24 = 5.2e-5 (bound 1e-4); the normalised value (x -
    mean) * rstd with rstd ~ 1/3 inherits a third of that plus a few roundings of a value below 6: below 3e-5 (bound 1e-4; a
    wrong column, row or statistic is off by order one)."""
    KP = _kp(D)
    for M in MS:
        X, (img, mu0, rstd0) = singles[(D, use_ln0, M)]
        ns = (M + 31) // 32
        rows = _atl_rows(img, ns, KP)[:M]
        assert bool((rows[:, D:KP - 1] == 0.0).all()), (D, M)
        assert bool((rows[:, KP - 1] == 1.0).all()), (D, M)
        if use_ln0:
            xd = X.double()
            mean = xd.mean(1, keepdim=True)
            want = (xd - mean) / torch.sqrt(((xd - mean) ** 2).mean(1, keepdim=True) + 1e-5)
            assert float((rows[:, :D].double() - want).abs().max()) < 1e-4, (D, M)
            assert float((mu0[:M].double() - mean[:, 0]).abs().max()) < 1e-4, (D, M)
        else:
            assert torch.equal(rows[:, :D], X), (D, M)
            assert bool((mu0[:M] == 0.0).all()) and bool((rstd0[:M] == 1.0).all())
