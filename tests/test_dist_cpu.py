"""Data-parallel plumbing on CPU with gloo, world_size 2 (no GPU): column sharding, the packed gradient+scalar
all-reduce, and the global->local minibatch index mapping.  Per-shard gradients come from the oracle (tests may use
it): the sum over shards of *unscaled* per-shard gradient sums, divided by the global sum(active), must equal the
unsharded gradient -- the identity the sharded HAPPO update relies on."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from harl_amd.dist import Comm, local_minibatch_rows, shard_columns


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from oracle import harl_oracle as O
        from harl_amd.synthetic import Shapes, actor_param_shapes, make_buffers, synthetic_state_dict

        torch.set_num_threads(1)
        comm = Comm()
        assert comm.enabled and comm.world_size == world and comm.rank == rank
        T, N = 6, 10
        sh = Shapes(T=T, N=N, A=1, obs_dim=7, share_obs_dim=7, act_dim=3, hidden_sizes=[16, 16])
        d = make_buffers(sh, 3, inactive_p=0.2)
        cfg = O.PathConfig(hidden_sizes=[16, 16])
        sd = {k: torch.from_numpy(v) for k, v in synthetic_state_dict(actor_param_shapes(sh), 5).items()}
        rng = np.random.default_rng(0)
        adv = rng.standard_normal((T, N, 1)).astype(np.float32)
        factor = (1 + 0.1 * rng.standard_normal((T, N, 1))).astype(np.float32)

        def unscaled_grad_and_sums(cols):
            """sum over the shard's samples of d(-f*min(s1,s2)*active - coef*ent*active), plus sum(active)."""
            net = O._Net(sd, 1e-3, 1e-5, 0.0)
            f = lambda x: torch.from_numpy(np.ascontiguousarray(x[:, cols]).reshape(-1, x.shape[-1]))  # noqa: E731
            obs, act, am = f(d.obs[0][:-1]), f(d.actions[0]), f(d.active_masks[0][:-1])
            logp, _, dist_ = O.actor_evaluate_actions(net.p, cfg, obs, act, None, None)
            imp = torch.prod(torch.exp(logp - f(d.action_log_probs[0])), dim=-1, keepdim=True)
            a = f(adv)
            s = -(f(factor) * torch.min(imp * a, torch.clamp(imp, 0.8, 1.2) * a) * am).sum()
            ent = (0.5 + 0.5 * np.log(2 * np.pi) + torch.log(dist_["std"])).sum(-1, keepdim=True)
            s = s - cfg.entropy_coef * (ent * am).sum()
            s.backward()
            return net.flat_grad(), float(am.sum())

        lo, hi = shard_columns(N, rank, world)
        g_local, act_local = unscaled_grad_and_sums(slice(lo, hi))
        g_full, act_full = unscaled_grad_and_sums(slice(0, N))
        flat = torch.from_numpy(g_local.copy())
        scal = torch.zeros(48, dtype=torch.float64)
        scal[1] = act_local
        # ranks with DIFFERENT magnitudes: a per-rank (float)v + residual pair loses the cross-rank fp32 rounding of the
        # heads (1e9 + 3e7 is not an fp32 number); the fixed-grid pieces sum exactly
        scal[0] = (1e9 if rank == 0 else 3.00000017e7) + rank + 0.123456789
        scal[2] = 16777217.0 * (rank + 1)  # a count above 2^24
        from harl_amd.dist import pack_message_reference, unpack_message_reference
        msg = pack_message_reference(flat, scal)  # the [grad | hi | lo] message the device path builds in place
        comm.all_reduce_message(msg)
        flat, scal = unpack_message_reference(msg, flat.numel(), scal.numel())
        got = flat.numpy() / scal[1].item()
        want = g_full / act_full
        err = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
        want0 = sum((1e9 if r == 0 else 3.00000017e7) + r + 0.123456789 for r in range(world))
        want2 = sum(16777217.0 * (r + 1) for r in range(world))
        # minibatch index mapping: union over ranks of local rows == the global minibatch, order preserved
        torch.manual_seed(11)
        perm = torch.randperm(T * N)[: (T * N) // 2]
        loc = local_minibatch_rows(perm, N, lo, hi)
        t_, n_ = loc // (hi - lo), loc % (hi - lo) + lo
        back = (t_ * N + n_).tolist()
        keep = [int(x) for x in perm.tolist() if lo <= x % N < hi]
        # the critic's communicator (Comm.second_group): a queue of its own over the same ranks; collectives of the two
        # communicators interleaved in program order give the two independent sums
        assert comm.second_group() is comm  # opt-in: the default is ONE communicator
        os.environ["HARL_CRITIC_GROUP"] = "1"
        c2 = comm.second_group()
        assert c2 is not comm and c2.enabled and c2.world_size == world and c2.rank == rank
        ta, tb = torch.tensor([1.0 + rank], dtype=torch.float64), torch.tensor([10.0 * (1 + rank)], dtype=torch.float64)
        for _ in range(3):
            comm.all_reduce_sum(ta)
            c2.all_reduce_sum(tb)
        two_ok = float(ta.item()) == (world * (world + 1) / 2) * world ** 2 and float(tb.item()) == 10.0 * (world * (world + 1) / 2) * world ** 2
        os.environ["HARL_CRITIC_GROUP"] = "0"
        assert comm.second_group() is comm
        q.put((rank, err, abs(scal[1].item() - act_full), max(abs(scal[0].item() - want0) / want0, abs(scal[2].item() - want2)), back == keep and two_ok, (lo, hi)))
    finally:
        dist.destroy_process_group()


def test_shard_columns_partition():
    for n, w in [(4096, 8), (10, 3), (7, 8), (8192, 8)]:
        spans = [shard_columns(n, r, w) for r in range(w)]
        assert spans[0][0] == 0 and spans[-1][1] == n
        assert all(spans[i][1] == spans[i + 1][0] for i in range(w - 1))
        sizes = [b - a for a, b in spans]
        assert max(sizes) - min(sizes) <= 1


def test_world2_gloo_packed_allreduce_and_sharded_gradient_identity():
    world = 2
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    spans = sorted(r[5] for r in res)
    assert spans == [(0, 5), (5, 10)]
    for rank, err, act_err, sc_err, idx_ok, _ in res:
        assert err < 2e-6, (rank, err)          # sharded sum / global sum(active) == unsharded gradient
        assert act_err == 0.0
        assert sc_err < 1e-15, sc_err            # fp64 scalars survive the single fp32 all-reduce (fixed-grid pieces, exact sums)
        assert idx_ok


def _oneshot_cpu_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      HARL_ALLREDUCE="oneshot")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        comm = Comm()  # HARL_ALLREDUCE=oneshot without a GPU: the hipIpc exchange is not set up, the backend's all-reduce serves
        t = torch.full((5,), float(rank + 1), dtype=torch.float32)
        comm.all_reduce_sum(t)
        q.put((rank, comm.oneshot is None, comm.oneshot_status(), t.tolist()))
        comm.close()
    finally:
        dist.destroy_process_group()


def test_oneshot_request_without_gpu_falls_back_to_the_backend(monkeypatch):
    world, port = 2, _free_port()
    for var in ("HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):  # the workers see no GPU, also on a GPU box
        monkeypatch.setenv(var, "")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_oneshot_cpu_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, no_ctx, status, vals in res:
        assert no_ctx and status == 0 and vals == [3.0] * 5, (rank, no_ctx, status, vals)
