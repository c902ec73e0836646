"""The stream schedule of a train() call (runner.OnPolicyHARunner._train_schedule), host side without a GPU: its answers against
the conditions that used to decide it between them -- _critic_first_ok, the two critic ``if``s of train() and the four expressions
behind the side stream, the post stream and the last post-update pass, quoted below as they stood before the schedule was decided
in one place -- over a sweep of switches, devices, sizes, communicators and runners.  And the staggered critic's two generator
positions (runner._StaggeredCritic), driven on the CPU with no stream and a hand-written epoch generator."""
import itertools
import os
from types import SimpleNamespace

import pytest
import torch

from tests.test_launch_trace_cpu import LT
from tests.test_multidiscrete_cpu import stub_kernels  # noqa: F401  (fixture)

SWITCHES = {"HARL_CRITIC_STREAM": (None, "auto", "0", "1"), "HARL_CRITIC_FIRST": (None, "0"), "HARL_CRITIC_EARLY": (None, "0"),
            "HARL_SIDE_STREAM": (None, "0"), "HARL_SIDE_AHEAD": (None, "0"), "HARL_POST_STREAM": (None, "0"),
            "HARL_LAST_POST_PASS": (None, "1")}
_GRU = dict(obs=128, sobs=128, use_recurrent_policy=True, data_chunk_length=4)
RUNNERS = {"ff": ([128, 128], {}), "ff_mb2": ([128, 128], dict(actor_num_mini_batch=2, critic_num_mini_batch=2)),
           "gru": ([64, 64], _GRU), "naive_rnn": ([64, 64], dict(use_naive_recurrent_policy=True)),
           "haa2c": ([128, 128], dict(algo="haa2c", a2c_epoch=2)), "hatrpo": ([128, 128], dict(algo="hatrpo", **LT._TRPO)),
           "critic_mb2": ([128, 128], dict(critic_num_mini_batch=2))}


# ---- the conditions as the parent of this schedule stated them, literally (``self`` -> ``r``)
def _parent_critic_first_ok(r, fast) -> bool:
    if not all(fast) or os.environ.get("HARL_CRITIC_FIRST", "1") == "0":
        return False
    c = r.critic
    if c.critic_num_mini_batch != 1 or c.use_recurrent_policy or c.use_naive_recurrent_policy:
        return False
    return all(hasattr(a, "fuses_old_logp") and a.fuses_old_logp() for a in r.actor)


def _parent_schedule(r, fast, B, dev):
    """train()'s own order: the critic first (on its own stream or not), else staggered, else what is left; then the four
    expressions of the log-prob passes."""
    cinfo, own = None, False
    if _parent_critic_first_ok(r, fast):
        cs_mode = os.environ.get("HARL_CRITIC_STREAM", "auto")
        if (dev.type == "cuda" and (not r.comm.enabled or r.critic.comm is not r.comm)
                and cs_mode != "0" and (cs_mode == "1" or B <= r.CRITIC_STREAM_MAX_ROWS)):
            cinfo, own = "first", True
        else:
            cinfo = "first"
    if (cinfo is None and dev.type == "cuda" and all(hasattr(a, "rng_footprint") for a in r.actor)
            and (not r.comm.enabled or r.critic.comm is not r.comm)
            and os.environ.get("HARL_CRITIC_STREAM", "1") != "0" and os.environ.get("HARL_CRITIC_EARLY", "1") != "0"):
        cinfo, own = "staggered", True
    if cinfo is None:
        cinfo = "last"
    side = os.environ.get("HARL_SIDE_STREAM", "1") != "0"
    side_lazy = os.environ.get("HARL_SIDE_AHEAD", "1") != "0"
    post_ok = dev.type == "cuda" and os.environ.get("HARL_POST_STREAM", "1") != "0"
    last_post = os.environ.get("HARL_LAST_POST_PASS", "0") == "1" or dev.type != "cuda"
    return cinfo, own, side, side_lazy, post_ok, last_post


def _communicators(r):
    """Off; on and shared with the critic; on, with a group of the critic's own."""
    for enabled, own_group in ((False, False), (True, False), (True, True)):
        r.comm = SimpleNamespace(enabled=enabled)
        r.critic.comm = SimpleNamespace(enabled=enabled) if own_group else r.comm
        yield enabled, own_group


def test_schedule_is_what_the_scattered_conditions_decided(stub_kernels, monkeypatch):  # noqa: F811
    from harl_amd.runner import OnPolicyHARunner, _TrainSchedule
    for k in LT.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    torch.manual_seed(7)
    runners = {k: LT.make_runner(hidden, **kw) for k, (hidden, kw) in RUNNERS.items()}
    seen, n = set(), 0
    for values in itertools.product(*SWITCHES.values()):
        for k, v in zip(SWITCHES, values):
            if v is None:
                monkeypatch.delenv(k, raising=False)
            else:
                monkeypatch.setenv(k, v)
        for label, r in runners.items():
            fast = [hasattr(a, "masked_moments") for a in r.actor]
            for _ in _communicators(r):
                for on_gpu, B in itertools.product((True, False), (OnPolicyHARunner.CRITIC_STREAM_MAX_ROWS, OnPolicyHARunner.CRITIC_STREAM_MAX_ROWS + 1)):
                    got = r._train_schedule(fast, B, on_gpu)
                    assert isinstance(got, _TrainSchedule), label
                    want = _parent_schedule(r, fast, B, SimpleNamespace(type="cuda" if on_gpu else "cpu"))
                    assert tuple(got) == want, (label, values, r.comm.enabled, r.critic.comm is r.comm, on_gpu, B)
                    seen.add(tuple(got))
                    n += 1
    assert n == 256 * len(RUNNERS) * 3 * 4 and OnPolicyHARunner.CRITIC_STREAM_MAX_ROWS == 150_000
    assert {s[:2] for s in seen} == {("first", True), ("first", False), ("staggered", True), ("last", False)}
    assert all({s[i] for s in seen} == {True, False} for i in (2, 3, 4, 5))
    assert not hasattr(OnPolicyHARunner, "_critic_first_ok")


# ---- the staggered critic: actors that draw 10 and 7, a critic of three epochs that draws 5 each
def _epochs(perms, fail_at=None):
    for k in range(3):
        perms.append(torch.randperm(5))
        if k == fail_at:
            raise ValueError("epoch failed")
        yield


def _in_order():
    torch.manual_seed(11)
    actors, critic = [torch.randperm(10), torch.randperm(7)], []
    for _ in _epochs(critic):
        pass
    return actors, critic, torch.get_rng_state()


def test_staggered_critic_draws_what_the_in_order_run_draws():
    from harl_amd.runner import _StaggeredCritic
    want_actors, want_critic, want_state = _in_order()
    torch.manual_seed(11)
    critic = []
    st = _StaggeredCritic(_epochs(critic), 3, [10, 7], None)
    actors = [torch.randperm(10)]
    st.epoch()
    actors.append(torch.randperm(7))
    st.epoch()
    st.finish()  # (the third epoch: fewer actors than epochs)
    assert st.left == 0 and len(critic) == 3
    torch.set_rng_state(st.state)
    assert all(torch.equal(a, b) for a, b in zip(actors + critic, want_actors + want_critic))
    assert torch.equal(torch.get_rng_state(), want_state)


def test_an_epoch_that_raises_leaves_the_generator_at_the_actors_position():
    from harl_amd.runner import _StaggeredCritic
    torch.manual_seed(11)
    st = _StaggeredCritic(_epochs([], fail_at=0), 3, [10, 7], None)
    torch.randperm(10)
    at = torch.get_rng_state()
    with pytest.raises(ValueError, match="epoch failed"):
        st.epoch()
    assert torch.equal(torch.get_rng_state(), at) and st.left == 3


def test_a_footprint_one_draw_short_is_refused_behind_the_last_actor():
    from harl_amd.runner import _StaggeredCritic
    torch.manual_seed(11)
    st = _StaggeredCritic(_epochs([]), 3, [10], None)
    torch.randperm(10)
    st.epoch()
    torch.randperm(7)
    with pytest.raises(RuntimeError, match="rng_footprint"):
        st.finish()
