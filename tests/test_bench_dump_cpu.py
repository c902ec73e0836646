"""`bench.py --dump-outputs DIR` (host side, no GPU): what the last timed step returned or left in the runner is written as
DIR/<name>.npy in float32 / float64, and an array above its share of the size limit becomes the same seeded sample in every run."""
import os
from types import SimpleNamespace

import numpy as np
import torch


def _runner(A=3, T=4, N=8):
    g = torch.Generator().manual_seed(0)
    net = lambda n: SimpleNamespace(flat_reference=lambda t=torch.randn(n, generator=g): t)  # noqa: E731
    return SimpleNamespace(
        actor=[SimpleNamespace(actor=net(10 + a)) for a in range(A)],
        critic=SimpleNamespace(critic=net(7)),
        critic_buffer=SimpleNamespace(returns=torch.randn(T + 1, N, 1, generator=g), advantages=torch.randn(T, N, 1, generator=g)),
        value_normalizer=SimpleNamespace(stats=torch.tensor([0.5, 1.5, 0.9])))


def _infos(A=3):
    return ([{"policy_loss": torch.tensor(0.1 * a), "dist_entropy": 1.0, "actor_grad_norm": 2.0, "ratio": 1.0} for a in range(A)],
            {"value_loss": 0.25, "critic_grad_norm": 3.0})


def test_dump_writes_every_output(tmp_path):
    import bench
    r = _runner()
    names = bench.dump_outputs(r, _infos(), str(tmp_path))
    files = sorted(f[:-4] for f in os.listdir(tmp_path))
    assert files == names
    assert {"returns", "advantages", "critic_params", "value_norm_stats", "actor_params_0", "actor_params_2",
            "actor_info_policy_loss", "critic_info_value_loss"} <= set(names)
    for n in names:
        x = np.load(tmp_path / f"{n}.npy")
        assert x.dtype in (np.float32, np.float64), (n, x.dtype)
    np.testing.assert_array_equal(np.load(tmp_path / "returns.npy"), r.critic_buffer.returns.numpy())
    np.testing.assert_array_equal(np.load(tmp_path / "actor_params_1.npy"), r.actor[1].actor.flat_reference().numpy())
    np.testing.assert_allclose(np.load(tmp_path / "actor_info_policy_loss.npy"), [0.0, 0.1, 0.2], rtol=1e-6)
    assert np.load(tmp_path / "critic_info_critic_grad_norm.npy").tolist() == [3.0]


def test_dump_samples_large_arrays_the_same_way(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT", 1300)  # 13 arrays in this dump -> 100 bytes = 25 float32 each
    r = _runner(T=40, N=8)
    assert len(bench.dump_outputs(r, _infos(), str(tmp_path / "a"))) == 13
    bench.dump_outputs(r, _infos(), str(tmp_path / "b"))
    total = 0
    for f in os.listdir(tmp_path / "a"):
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        np.testing.assert_array_equal(x, y)
        total += x.nbytes
    assert total <= bench.DUMP_LIMIT
    ret = np.load(tmp_path / "a" / "returns.npy")
    assert ret.shape == (25,) and set(ret.tolist()) <= set(r.critic_buffer.returns.reshape(-1).tolist())
