"""Stream traces of whole train() calls ON THE GPU: the order in which the host enqueues every kernel launch and every stream /
event operation of two ``prep_training(); train()`` rounds, and the stream each goes to.  tools/launch_trace.py records on
device "cpu", where every stream branch of OnPolicyHARunner.train() is off; this recorder runs the real kernels and needs no seam
in the code under test: it wraps ``_lib.call`` (as launch_trace.Recorder does) and the Python-level ``torch.cuda.Stream.wait_stream``
/ ``wait_event`` and ``torch.cuda.Event.record`` / ``wait`` / ``synchronize``.  One entry per operation:

    [stream, "entry:tag"]                  a launch, on the stream that is current
    ["wait_stream", waiter, awaited]       ["wait_event", stream, event]       ["record", stream, event]       ["sync", event]
    ["train"]                              a train() call begins (written by run_config, not by the code under test)

Streams are named in order of first appearance within a configuration -- ``main`` is the stream current when the first train()
is entered, the others ``s1``, ``s2``, ... -- and events by the order of their first ``record``: no name comes from the attribute
that holds the object.  ``Stream.wait_stream`` records an event and waits for it through the same Python methods; only the
outermost call is written down.  The trace is the host's enqueue order, so it does not depend on what the GPU overlaps.

    python tools/stream_trace.py --check tests/golden/stream_traces.json   # regenerate and compare (exit status 1: differs)
    python tools/stream_trace.py --write tests/golden/stream_traces.json   # the fixture, in the form of launch_traces.json
    python tools/stream_trace.py --full a.json                             # the traces themselves

tests/test_gpu_stream_trace.py runs the comparison of --check in the suite."""
import argparse
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

_spec = importlib.util.spec_from_file_location("launch_trace", os.path.join(ROOT, "tools", "launch_trace.py"))
LT = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(LT)

# the switches OnPolicyHARunner.train() takes its stream schedule from: cleared, with LT.SWITCHES, around every run
SCHEDULE_SWITCHES = ("HARL_CRITIC_STREAM", "HARL_CRITIC_FIRST", "HARL_CRITIC_EARLY", "HARL_SIDE_STREAM", "HARL_SIDE_AHEAD",
                     "HARL_POST_STREAM", "HARL_LAST_POST_PASS")
_RNN = "rnn_disc_h64_mb2"
# name -> (golden of tests/golden, environment, agents whose active_masks are zeroed after build_runner)
CONFIGS = {
    "01_mpe": ("mpe_box_h64", {}, ()),                                                   # critic first, own stream (small B)
    "02_mpe_one_stream": ("mpe_box_h64", dict(HARL_CRITIC_STREAM="0"), ()),              # critic first, main stream
    "03_mpe_staggered": ("mpe_box_h64", dict(HARL_CRITIC_FIRST="0"), ()),                # staggered behind feed-forward agents
    "04_mpe_critic_last": ("mpe_box_h64", dict(HARL_CRITIC_FIRST="0", HARL_CRITIC_EARLY="0"), ()),
    "05_mpe_agent1_inactive": ("mpe_box_h64", dict(HARL_CRITIC_FIRST="0"), (1,)),        # count 0: side stream, not in the footprint
    "06_cheetah_mb2": ("cheetah_h128x3_mb2", {}, ()),                                    # side stream for every agent, staggered critic
    "07_rnn": (_RNN, {}, ()),                                        # staggered + side one agent ahead + post stream + _await_factor
    "08_rnn_side_up_front": (_RNN, dict(HARL_SIDE_AHEAD="0"), ()),
    "09_rnn_no_side": (_RNN, dict(HARL_SIDE_STREAM="0"), ()),
    "10_rnn_no_post_stream": (_RNN, dict(HARL_POST_STREAM="0"), ()),
    "11_rnn_last_post_pass": (_RNN, dict(HARL_LAST_POST_PASS="1"), ()),
    "12_trpo": ("trpo_disc_h64", {}, ()),                                # HATRPO: no masked_moments, all on the side stream, critic last
}


def entry_name(e):
    """The name an entry goes by in the fixture's table: its items, joined."""
    return " ".join(str(x) for x in e)


class Recorder:
    """Installs the wrappers on ``monkeypatch`` and keeps the entries in ``trace``."""

    def __init__(self, monkeypatch):
        from harl_amd import _lib
        self.trace, self._streams, self._events, self._alive, self._depth = [], {}, {}, [], 0
        self._inner = _lib.call
        monkeypatch.setattr(_lib, "call", self)
        for mod in LT.MODS:
            m = __import__(f"harl_amd.{mod}", fromlist=["x"])
            if hasattr(m, "call"):
                monkeypatch.setattr(m, "call", self)
        S, E = torch.cuda.Stream, torch.cuda.Event
        self._wrap(monkeypatch, S, "wait_stream", lambda s, other: ["wait_stream", self.stream(s), self.stream(other)])
        self._wrap(monkeypatch, S, "wait_event", lambda s, ev: ["wait_event", self.stream(s), self.event(ev)])
        self._wrap(monkeypatch, E, "record", lambda ev, stream=None: ["record", self.stream(stream), self.event(ev, True)])
        self._wrap(monkeypatch, E, "wait", lambda ev, stream=None: ["wait_event", self.stream(stream), self.event(ev)])
        self._wrap(monkeypatch, E, "synchronize", lambda ev: ["sync", self.event(ev)])

    def _wrap(self, monkeypatch, cls, method, entry):
        inner = getattr(cls, method)

        def wrapped(obj, *a, **k):
            if self._depth == 0:  # (wait_stream -> record_event + wait_event -> Event.wait: the outermost call only)
                self.trace.append(entry(obj, *a, **k))
            self._depth += 1
            try:
                return inner(obj, *a, **k)
            finally:
                self._depth -= 1
        monkeypatch.setattr(cls, method, wrapped)

    def stream(self, s=None):
        s = torch.cuda.current_stream() if s is None else s
        return self._streams.setdefault((s.device_index, s.cuda_stream), "s%d" % len(self._streams) if self._streams else "main")

    def event(self, ev, recording=False):
        """The event's number, given at its first ``record``; one that is waited for without having been recorded here
        (recorded before the recording began, or never) goes by "unrecorded"."""
        if recording and id(ev) not in self._events:
            self._alive.append(ev)  # (kept, so that no later event takes this one's id)
            self._events[id(ev)] = len(self._events)
        return self._events.get(id(ev), "unrecorded")

    def begin_train(self):
        self.stream()  # the first one names ``main``
        self.trace.append(["train"])

    def __call__(self, name, *args, tag=None):
        self.trace.append([self.stream(), f"{name}:{tag or ''}"])
        return self._inner(name, *args, tag=tag)


def run_config(name, monkeypatch, rounds=2):
    """The trace of ``rounds`` x (prep_training(); train()) of configuration ``name``: the runner built and seeded as
    tests.gpu_checks.check_train_golden does."""
    import numpy as np

    from harl_amd import nets
    from harl_amd.buffers import _advance_matches_randperm
    from tests.gpu_checks import GoldenCase, build_runner
    golden, env, inactive = CONFIGS[name]
    with monkeypatch.context() as mp:
        for k in LT.SWITCHES + SCHEDULE_SWITCHES:
            mp.delenv(k, raising=False)
        for k, v in env.items():
            mp.setenv(k, v)
        # the one piece of process-wide state with events in it, the ring of pinned upload buffers: which slot is next, and
        # whether its event has been recorded before, must not depend on what this process ran earlier
        mp.setattr(nets, "_FIRST_RING", {})
        case = GoldenCase(golden)
        torch.manual_seed(case.seed)
        np.random.seed(case.seed)
        r = build_runner(case)
        for a in inactive:
            r.actor_buffer[a].active_masks.zero_()
        assert _advance_matches_randperm()  # the one-time self-check of the generator, outside the recording
        torch.manual_seed(case.seed + 12345)
        cb = r.critic_buffer
        cb.compute_returns(cb.value_preds[-1].clone(), r.value_normalizer)
        torch.cuda.synchronize()
        rec = Recorder(mp)
        for _ in range(rounds):
            r.prep_training()
            rec.begin_train()
            r.train()
        torch.cuda.synchronize()
        return rec.trace


def all_traces():
    import pytest
    with pytest.MonkeyPatch.context() as mp:
        return {k: run_config(k, mp) for k in CONFIGS}


def summarise(traces, keep=()):
    return LT.summarise(traces, keep, name=entry_name)


def compare(want, got):
    return LT.compare(want, got, name=entry_name)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--check", metavar="FIXTURE", help="regenerate the traces and compare them with FIXTURE")
    g.add_argument("--write", metavar="FIXTURE", help="write the fixture of this tree: names and a SHA-256 per configuration")
    g.add_argument("--full", metavar="OUT", help="write the traces of this tree")
    a = ap.parse_args()
    traces, lines = LT.normalise(all_traces()), []
    if a.full:
        with open(a.full, "w") as f:
            json.dump(traces, f, separators=(",", ":"))
    elif a.write:
        keep = ()
        if os.path.exists(a.write):
            with open(a.write) as f:
                keep = json.load(f)["names"]
        LT.write_fixture(a.write, summarise(traces, keep))
    else:
        with open(a.check) as f:
            lines = compare(json.load(f), traces)
    print("\n".join(lines) if lines else "no difference")
    return 1 if lines else 0


if __name__ == "__main__":
    sys.exit(main())
