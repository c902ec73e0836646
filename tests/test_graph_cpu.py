"""HARL_GRAPH=1, host side without a GPU (C-ABI calls recorded instead of executed): the launch sequence is the one without the
variable, the Adam table the host writes for harl_adam_fold_dev holds exactly the doubles harl_adam_fold is handed, and the
host step counter / state_dict are untouched by the mode."""
import torch

from tests.test_hybrid_cpu import _runner
from tests.test_multidiscrete_cpu import stub_kernels  # noqa: F401  (fixture)

MODS = ("nets", "buffers", "happo", "hatrpo", "mappo", "v_critic", "valuenorm", "runner")


def _ordered_calls(monkeypatch):
    """Names of the recorded C-ABI calls in launch order (the stub keeps them per name)."""
    from harl_amd import _lib
    order, rec = [], _lib.call

    def wrapped(name, *args, tag=None):
        order.append(name)
        return rec(name, *args, tag=tag)
    monkeypatch.setattr(_lib, "call", wrapped)
    for mod in MODS:
        m = __import__(f"harl_amd.{mod}", fromlist=["x"])
        if hasattr(m, "call"):
            monkeypatch.setattr(m, "call", wrapped)
    return order


def _train(r):
    r.prep_training()
    r.train()


def test_launch_sequence_is_unchanged_without_a_gpu(stub_kernels, monkeypatch):  # noqa: F811
    order = _ordered_calls(monkeypatch)
    seqs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("HARL_GRAPH", mode)
        for hidden, kw in (([128, 128], {}), ([128, 128, 128], dict(actor_num_mini_batch=2, critic_num_mini_batch=2))):
            torch.manual_seed(3)
            r = _runner(hidden, **kw)
            del order[:]
            _train(r)
            _train(r)
            seqs[(mode, len(hidden))] = list(order)
            assert all(v == 0 for v in r.graph_stats().values())  # nothing is captured or replayed on the host
    for n in (2, 3):
        assert seqs[("1", n)] == seqs[("0", n)]
        assert "harl_adam_fold" in seqs[("1", n)] and "harl_adam_fold_dev" not in seqs[("1", n)]


def test_host_table_rows_are_the_eager_path_doubles(stub_kernels, monkeypatch):  # noqa: F811
    monkeypatch.setenv("HARL_GRAPH", "1")
    r = _runner([128, 128], actor_num_mini_batch=2)
    n_upd = 2 * 2  # ppo_epoch x minibatches (tests/test_hybrid_cpu._runner: two epochs)
    opts = [a.actor_optimizer for a in r.actor] + [r.critic.critic_optimizer]
    lr0 = [o.param_groups[0]["lr"] for o in opts]
    for it in range(2):
        if it == 1:  # the reference's update_linear_schedule between episodes
            for x in list(r.actor) + [r.critic]:
                x.lr_decay(2, 4)
        before = [o.step_count for o in opts]
        _train(r)
        for o, b, l0 in zip(opts, before, lr0):
            steps = o.step_count - b
            assert steps == (n_upd if o is not opts[-1] else 2) and b == it * steps
            tab = o.hyper_table()
            assert tab.dtype == torch.float64 and tab.shape[0] >= steps
            lr = l0 if it == 0 else l0 - l0 * (1 / 4.0)
            assert o.param_groups[0]["lr"] == lr
            for k in range(tab.shape[0]):
                t = b + 1 + k
                assert tab[k].tolist() == [lr, 1.0 - 0.9 ** t, 1.0 - 0.999 ** t], (it, k)
            assert o.hyper_rows_left() == 0  # disarmed at the end of train(): a direct update() takes the host scalars


def test_step_count_and_state_dict_do_not_depend_on_the_mode(stub_kernels, monkeypatch, tmp_path):  # noqa: F811
    got = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("HARL_GRAPH", mode)
        torch.manual_seed(3)
        r = _runner([128, 128])
        _train(r)
        _train(r)
        opts = [a.actor_optimizer for a in r.actor] + [r.critic.critic_optimizer]
        sds = [o.state_dict() for o in opts]
        got[mode] = [(o.step_count, sd["step"], sorted(sd.keys()), sd["param_groups"]) for o, sd in zip(opts, sds)]
        assert all(o.step_count == sd["step"] == 4 for o, sd in zip(opts, sds))
        # save / restore round trip: files and keys as ever, optimiser state through state_dict / load_state_dict
        r.save(str(tmp_path / mode))
        r2 = _runner([128, 128])
        r2.restore(str(tmp_path / mode))
        for a, b in zip(list(r.actor) + [r.critic], list(r2.actor) + [r2.critic]):
            na, nb = (a.actor, b.actor) if hasattr(a, "actor") else (a.critic, b.critic)
            assert torch.equal(na.flat_param, nb.flat_param)
        for o, sd, o2 in zip(opts, sds, [a.actor_optimizer for a in r2.actor] + [r2.critic.critic_optimizer]):
            o2.load_state_dict(sd)
            assert o2.step_count == o.step_count and o2.hyper_rows_left() == 0
            assert torch.equal(o2.exp_avg, o.exp_avg) and torch.equal(o2.exp_avg_sq, o.exp_avg_sq)
        got[mode + "files"] = sorted(p.name for p in (tmp_path / mode).iterdir())
    assert got["1"] == got["0"] and got["1files"] == got["0files"]
