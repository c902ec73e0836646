"""HARL_GRAPH=1 on the GPU: optimiser steps replayed from a hipGraph (harl_amd/graphs.py) against the eager path of the same
build on the same inputs.  Bit-identity is the criterion everywhere: same kernels, same operands, same order."""
import numpy as np
import pytest
import torch

from tests.helpers import GoldenCase

pytestmark = pytest.mark.gpu

TOL = 1.0  # golden checks: excess <= 1 (tests/helpers.excess), as in tests/test_gpu_parity.py


def _G():
    from tests import gpu_checks
    return gpu_checks


def _assert_all(out, tol):
    bad = {k: v for k, v in out.items() if not k.startswith("_") and isinstance(v, float) and not (v <= tol)}
    assert not bad, (bad, out)


def _uniq(objs):
    out = []
    for o in objs:
        if not any(o is u for u in out):
            out.append(o)
    return out


# ---- the optimiser kernel: host scalars against the device table ---------------------------------------------------
@pytest.mark.parametrize("name", ["mpe_box_h64", "disc50_h128"])  # with / without a Gaussian log_std block
def test_adam_fold_dev_replayed_equals_adam_fold(name, monkeypatch):
    """4 eager harl_adam_fold steps with host scalars == ONE captured harl_adam_fold_dev replayed 4 times on a copy of the
    same state (gradients, partial scalars refreshed by eager copies in between; a lower lr in row 3)."""
    from harl_amd._lib import PS_STRIDE, call, ptr, stream
    monkeypatch.delenv("HARL_GRAPH", raising=False)
    G = _G()
    case = GoldenCase(name)
    torch.manual_seed(case.seed)
    actor = G.build_runner(case).actor[0]
    net, opt = actor.actor, actor.actor_optimizer
    net._ensure_ws(case.shapes.T * case.shapes.N)
    net.fold()
    dev = net.flat_param.device
    gen = torch.Generator(device="cpu").manual_seed(5)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(dev)  # noqa: E731
    n_steps, base = 4, 7  # steps 8 .. 11 of a run
    p0 = net.flat_param.clone()
    m0, v0 = 1e-3 * rnd(net.n_params), 1e-6 * rnd(net.n_params).abs()
    nblk = net.n_wg
    dwps = [1e-2 * rnd(net.total_dwp) for _ in range(n_steps)]
    grads = [rnd(net.n_params) for _ in range(n_steps)]  # (overwritten by the kernel's unfold: refreshed all the same)
    pss = [(rnd(nblk * PS_STRIDE).abs() + 0.5) for _ in range(n_steps)]  # positive sums: sum(active), ratio count > 0
    lrs = [5e-4, 5e-4, 5e-4, 3.75e-4]
    b1, b2, eps, wd = 0.9, 0.999, 1e-5, 0.0
    rows = [(lrs[k], 1.0 - b1 ** (base + 1 + k), 1.0 - b2 ** (base + 1 + k)) for k in range(n_steps)]
    ls_off = -1 if net.discrete else net.offsets["act.action_out.log_std"][0]
    assert (ls_off >= 0) == (name == "mpe_box_h64")
    info = torch.zeros(4, dtype=torch.float64, device=dev)

    def restore():
        net.flat_param.copy_(p0)
        opt.exp_avg.copy_(m0)
        opt.exp_avg_sq.copy_(v0)
        net.invalidate_caches()
        net.fold()
        info.zero_()

    def refresh(k):
        net.dwp.copy_(dwps[k])
        net.flat_grad.copy_(grads[k])
        net.part_scalars[:nblk * PS_STRIDE].copy_(pss[k])

    head = lambda: (ptr(net.flat_param), ptr(net.flat_grad), ptr(opt.exp_avg), ptr(opt.exp_avg_sq), net.n_params, ptr(net.dwp),  # noqa: E731
                    ptr(net.table), net.n_entries, ptr(net.pack_arena), ptr(net.scalars), ptr(net.part_scalars), nblk, None, 0,
                    0.0, ls_off, net.act_dim, ptr(info), 1, 10.0)
    snap = lambda: [t.clone() for t in (net.flat_param, opt.exp_avg, opt.exp_avg_sq, net.pack_arena, info, net.flat_grad)]  # noqa: E731

    restore()
    for k in range(n_steps):
        refresh(k)
        call("harl_adam_fold", *head(), rows[k][0], b1, b2, eps, wd, rows[k][1], rows[k][2], ptr(opt._ws), stream())
    torch.cuda.synchronize()
    want = snap()

    table = torch.tensor([0.0] + [x for r in rows for x in r], dtype=torch.float64).to(dev)  # [counter word | rows]
    counter = table[:1].view(torch.int32)
    dev_args = lambda s: head() + (table.data_ptr() + 8, n_steps, table.data_ptr(), b1, b2, eps, wd, ptr(opt._ws), s)  # noqa: E731
    refresh(0)
    call("harl_adam_fold_dev", *dev_args(stream()))  # the eager first run of the launch that is captured below
    torch.cuda.synchronize()
    assert int(counter[0].item()) == 1
    table[:1].zero_()
    restore()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        graph.capture_begin(capture_error_mode="thread_local")
        call("harl_adam_fold_dev", *dev_args(stream()))
        graph.capture_end()
    for k in range(n_steps):
        refresh(k)
        graph.replay()
    torch.cuda.synchronize()
    got = snap()
    for nm, a, b in zip(("param", "exp_avg", "exp_avg_sq", "pack_arena", "info", "grad"), got, want):
        assert torch.equal(a, b), (nm, float((a.double() - b.double()).abs().max()))
    assert counter.cpu().tolist()[0] == n_steps
    assert not torch.equal(want[0], p0)  # (the steps did move the parameters)


# ---- whole train(): eager against graph ------------------------------------------------------------------------------
TRAIN_CASES = ["mpe_box_h64", "mpe_box_h128", "mpe_disc_h64", "cheetah_h128x3_mb2", "fp_disc_h128_mb2", "box_mean_inactive_novn",
               "a2c_box_h64", "mappo_shared_disc_h64_mb2", "hands_h256x3", "disc50_h128"]


def _two_trains(case, graph: bool, monkeypatch):
    """compute() + train() twice on a runner built from the fixture's state, the learning rate lowered in between.
    Returns (snapshots after each call, graph_stats after each call per network, runner)."""
    G = _G()
    if graph:
        monkeypatch.setenv("HARL_GRAPH", "1")
    else:
        monkeypatch.delenv("HARL_GRAPH", raising=False)
    torch.manual_seed(case.seed)
    np.random.seed(case.seed)
    r = G.build_runner(case)
    from harl_amd.buffers import _advance_matches_randperm
    assert _advance_matches_randperm()
    torch.manual_seed(case.seed + 12345)
    r.prep_training()
    nets = _uniq(r.actor) + [r.critic]
    snaps, stats = [], []
    for it in range(2):
        if it == 1:  # what update_linear_schedule does between episodes
            for x in nets:
                x.lr_decay(2, 4)
        r.compute()
        infos, cinfo = r.train()
        torch.cuda.synchronize()
        s = dict(infos=[dict(i) for i in infos], cinfo=dict(cinfo), rng=torch.get_rng_state().clone())
        for i, a in enumerate(_uniq(r.actor)):
            o = a.actor_optimizer
            s[f"actor{i}"] = (a.actor.flat_param.clone(), o.exp_avg.clone(), o.exp_avg_sq.clone(), o.step_count)
        o = r.critic.critic_optimizer
        s["critic"] = (r.critic.critic.flat_param.clone(), o.exp_avg.clone(), o.exp_avg_sq.clone(), o.step_count)
        s["vn"] = None if r.value_normalizer is None else r.value_normalizer.stats.clone()
        snaps.append(s)
        stats.append([x.graph_stats() for x in nets])
    return snaps, stats, r


@pytest.mark.parametrize("name", TRAIN_CASES)
def test_train_graph_equals_eager(name, monkeypatch):
    case = GoldenCase(name)
    want, stats0, _ = _two_trains(case, False, monkeypatch)
    got, stats, r = _two_trains(case, True, monkeypatch)
    assert all(v == 0 for st in stats0 for s in st for v in s.values()), stats0  # nothing is counted without the switch
    for it in range(2):
        w, g = want[it], got[it]
        for k in w:
            if k in ("infos", "cinfo"):
                assert g[k] == w[k], (it, k, g[k], w[k])
            elif k == "rng":
                assert torch.equal(g[k], w[k]), (it, k)
            elif k == "vn":
                assert (w[k] is None and g[k] is None) or torch.equal(g[k], w[k]), (it, k)
            else:
                for j, nm in enumerate(("param", "exp_avg", "exp_avg_sq")):
                    assert torch.equal(g[k][j], w[k][j]), (it, k, nm, float((g[k][j].double() - w[k][j].double()).abs().max()))
                assert g[k][3] == w[k][3], (it, k, "step")
    a = case.algo
    epochs = a.get("ppo_epoch") or a.get("a2c_epoch")
    need = [(epochs - 1) * a["actor_num_mini_batch"]] * (len(stats[0]) - 1) + [(a["critic_epoch"] - 1) * a["critic_num_mini_batch"]]
    for i, (s1, s2) in enumerate(zip(stats[0], stats[1])):
        assert s1["captures"] >= 1 and s1["replays"] >= 1, (i, s1)
        assert s2["captures"] == s1["captures"], (i, s1, s2)  # the second train() reuses the graphs of the first
        assert s2["replays"] - s1["replays"] >= need[i], (i, s1, s2, need[i])
    tot = r.graph_stats()
    assert tot["replays"] == sum(s["replays"] for s in stats[1]) and tot["captures"] == sum(s["captures"] for s in stats[1])


# ---- the existing golden check under the switch ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mpe_box_h128", "cheetah_h128x3_mb2"])
def test_train_golden_under_graph_switch(name, monkeypatch):
    monkeypatch.setenv("HARL_GRAPH", "1")
    _assert_all(_G().check_train_golden(name), tol=TOL)


# ---- what stays eager -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rnn_box_h64", "md_h64_mb2", "trpo_box_h64"])
def test_ineligible_configurations_stay_eager(name, monkeypatch):
    """Recurrent, MultiDiscrete and HATRPO actors never replay; the usual golden check is green under the switch."""
    G = _G()
    monkeypatch.setenv("HARL_GRAPH", "1")
    built = []
    real = G.build_runner
    monkeypatch.setattr(G, "build_runner", lambda case: (built.append(real(case)), built[-1])[1])
    _assert_all(G.check_train_golden(name), tol=TOL)
    assert len(built) == 1
    for a in _uniq(built[0].actor):
        assert a.graph_stats()["replays"] == 0 and a.graph_stats()["captures"] == 0, a.graph_stats()
    if name != "trpo_box_h64":  # (HATRPO's critic is the plain V critic: feed-forward, untraced by that check, so it may replay)
        assert built[0].graph_stats()["replays"] == 0  # recurrent critic / the golden check traces the critic's steps


def test_traced_actor_stays_eager(monkeypatch):
    monkeypatch.setenv("HARL_GRAPH", "1")
    case = GoldenCase("mpe_box_h64")
    torch.manual_seed(case.seed)
    r = _G().build_runner(case)
    r.prep_training()
    r.actor[0]._trace = []
    r.compute()
    r.train()
    torch.cuda.synchronize()
    assert r.actor[0].graph_stats()["replays"] == 0 and r.actor[0].graph_stats()["captures"] == 0
    assert len(r.actor[0]._trace) == case.algo["ppo_epoch"]
    assert r.actor[1].graph_stats()["replays"] >= 1 and r.critic.graph_stats()["replays"] >= 1
